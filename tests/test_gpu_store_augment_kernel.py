"""GPU suite of hriemo_gather_rows_aug, through the C ABI, compared BIT FOR BIT (as bytes) with the host replica
tests/augment_reference.py.  The fixtures are those of test_gpu_store_gather.py: stores of 74 x fp32 (296-byte rows: the source
phase changes per segment), 300 x fp32, 768 x bf16, 5 x fp16 (rows shorter than a 16-byte chunk) and 8 x bf16; 7 utterances of 1,
2, 17, 64, 3, 1, 40 rows; the same id lists; the destination pre-filled with 0xFF with one such row on either side, inside guards
of 0xA5, once 16-byte aligned and once offset by one row; zero tails of 5 rows and of none.  Spans-only and drop-only cases run on
random store bytes (NaN / Inf patterns included: kept elements are bit copies), the noise cases on finite values.  Every (seed,
draw) is found by a search on the replica and each test asserts, on the replica, that its seed exercises the case it is about."""
import numpy as np
import pytest
import torch

import augment_reference as R

pytestmark = pytest.mark.gpu

LENS = [1, 2, 17, 64, 3, 1, 40]
OFF = [0, 1, 3, 20, 84, 87, 88, 128]
IDS = [[0], [6], [3, 3, 3], [6, 5, 4, 3, 2, 1, 0], [1, 5]]
ALL = IDS[3]
STORES = {"74 fp32": (74, torch.float32), "300 fp32": (300, torch.float32), "768 bf16": (768, torch.bfloat16),
          "5 fp16": (5, torch.float16), "8 bf16": (8, torch.bfloat16)}
CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
POISON, GUARD, G = 0xFF, 0xA5, 64
SPANS = (2, 8, 1.0)              # max_frac = 1.0: the utterances of one row can be masked (W = 1), not only the long ones
DROP = (0.4, 0.3)
DRAW = 3


def ST():
    return torch.cuda.current_stream().cuda_stream


_CACHE = {}


def _store(name, finite):
    """(rows on the device, rows on the host, offsets int64 on the device): random bytes viewed as the dtype (a NaN and an Inf
    planted), or randn cast to the dtype (finite); made once and never changed"""
    if (name, finite) not in _CACHE:
        d, dtype = STORES[name]
        es = torch.empty((), dtype=dtype).element_size()
        g = torch.Generator().manual_seed(len(name) + d)
        if finite:
            host = torch.randn(sum(LENS), d, generator=g).to(dtype)
        else:
            raw = torch.randint(0, 256, (sum(LENS), d * es), dtype=torch.uint8, generator=g)
            raw[0, :4] = torch.tensor([0, 0, 0xC0, 0x7F], dtype=torch.uint8)
            raw[-1, -4:] = torch.tensor([0, 0, 0x80, 0xFF], dtype=torch.uint8)
            host = raw.view(dtype)
        assert host.shape == (sum(LENS), d)
        _CACHE[(name, finite)] = (host.cuda(), host, torch.tensor(OFF, dtype=torch.int64).cuda())
    return _CACHE[(name, finite)]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _args(dev, off_dev, plan, n, dst_ptr, dst_rows, cfg, seed, draw, max_rows=max(LENS)):
    return [dev.data_ptr(), dev.shape[1], CODES[dev.dtype], off_dev.data_ptr(), plan.data_ptr(), n, dst_ptr, dst_rows, max_rows, seed, draw,
            cfg["modality"], cfg["thr_lo"], cfg["thr_hi"], cfg["spans"], cfg["max_width"], cfg["frac16"], cfg["noise_scale"], ST()]


def _run(name, finite, ids, tail, shift_rows, cfg, seed, draw=DRAW):
    """one launch into a guarded, poisoned buffer -> the payload's gathered rows [cu[n], d] on the host (dtype of the store), after
    the checks every case shares: equal to the replica as bytes, exact zero tail, nothing outside the destination changed"""
    from hri_emo_amd import _lib
    dev, host, off_dev = _store(name, finite)
    d, es = host.shape[1], host.element_size()
    rb, n = d * es, len(ids)
    cu = [0]
    for i in ids:
        cu.append(cu[-1] + LENS[i])
    dst_rows = cu[n] + tail
    plan = torch.tensor(ids + cu, dtype=torch.int32).cuda()
    before, size = G + shift_rows * rb, G + (shift_rows + dst_rows + 1) * rb + G
    buf = torch.full((size,), POISON, dtype=torch.uint8, device="cuda")
    buf[:G] = GUARD
    buf[size - G:] = GUARD
    was = buf.cpu()
    assert buf.data_ptr() % 16 == 0
    _lib.call("hriemo_gather_rows_aug", *_args(dev, off_dev, plan, n, buf.data_ptr() + before, dst_rows, cfg, seed, draw))
    torch.cuda.synchronize()
    got = buf.cpu()
    ref = _bytes(R.apply(host, ids, OFF, cfg["modality"], cfg, seed, draw)).view(cu[n], rb)
    payload = got[before:before + dst_rows * rb].view(dst_rows, rb)
    what = (name, ids, tail, shift_rows, cfg, seed, draw)
    bad = (payload[:cu[n]] != ref).nonzero()
    assert bad.numel() == 0, ("gathered rows differ from the replica", what, len(bad), bad[:4].tolist())
    assert not payload[cu[n]:].any(), ("zero tail", what)
    assert torch.equal(got[:before], was[:before]), ("bytes in front of the destination", what)
    assert torch.equal(got[before + dst_rows * rb:], was[before + dst_rows * rb:]), ("the row behind dst_rows and the guard", what)
    assert bool((got[before + dst_rows * rb:size - G] == POISON).all())
    return payload[:cu[n]].contiguous().view(host.dtype).view(cu[n], d)


def _seed_where(pred, what):
    """the first seed in 1 .. 4000 the predicate (on the replica) accepts: a search, so a degenerate seed cannot pass silently"""
    for seed in range(1, 4000):
        if pred(seed):
            return seed
    raise AssertionError(f"no seed in 1 .. 3999 with {what}")


def _span_facts(cfg, seed, ids=ALL, draw=DRAW):
    s, w = R.spans(seed, draw, cfg["modality"], ids, [LENS[i] for i in ids], cfg["spans"], cfg["max_width"], cfg["frac16"])
    L = np.asarray([LENS[i] for i in ids])[:, None]
    return dict(edge=bool(((w > 0) & ((s == 0) | (s + w == L))).any()), empty=bool((w == 0).any()), inner=bool(((w > 0) & (s > 0) & (s + w < L)).any()))


def _span_seed(cfg):
    ok = lambda seed: all(_span_facts(cfg, seed).values())      # noqa: E731
    seed = _seed_where(ok, "a span at an utterance's edge, an empty one and one inside")
    f = _span_facts(cfg, seed)
    assert f["edge"] and f["empty"] and f["inner"], f
    return seed


def _drop_seed(cfg):
    def ok(seed):
        f = R.drop_flags(seed, DRAW, ALL, cfg["thr_lo"], cfg["thr_hi"])
        g = R.drop_flags(seed, DRAW, [1, 5], cfg["thr_lo"], cfg["thr_hi"])
        return f.any() and not f.all() and g.any() and not g.all()
    seed = _seed_where(ok, "a dropped and a kept utterance")
    f = R.drop_flags(seed, DRAW, ALL, cfg["thr_lo"], cfg["thr_hi"])
    assert f.any() and not f.all(), f
    return seed


PARAMS = [(name, shift) for name in STORES for shift in (0, 1)]
PARAM_IDS = [f"{name}-{'offset by one row' if shift else 'aligned'}" for name, shift in PARAMS]


# ----------------------------------------------------------------------------- zeros only: random bytes, kept elements are bit copies
@pytest.mark.parametrize("name,shift_rows", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("which", [0, 1], ids=["audio", "text"])
def test_spans_only(name, shift_rows, which):
    """kept elements are the store's bytes (NaN and Inf patterns included), masked rows are zero bytes -- the replica says which"""
    cfg = R.launch_cfg(which, SPANS)
    seed = _span_seed(cfg)
    _, host, _ = _store(name, False)
    for ids in IDS:
        for tail in (5, 0):
            got = _run(name, False, ids, tail, shift_rows, cfg, seed)
            masks, _ = R.row_masks(ids, OFF, cfg, seed, DRAW)
            m = torch.from_numpy(np.concatenate(masks))
            idx = torch.tensor([r for i in ids for r in range(OFF[i], OFF[i + 1])])
            assert not _bytes(got[m]).any() and torch.equal(_bytes(got[~m]), _bytes(host[idx][~m])), (ids, tail)
    assert torch.from_numpy(np.concatenate(R.row_masks(ALL, OFF, cfg, seed, DRAW)[0])).any()


@pytest.mark.parametrize("name,shift_rows", PARAMS, ids=PARAM_IDS)
def test_drop_only_and_never_both_modalities(name, shift_rows):
    """the audio and the text launch on the same ids: a dropped utterance is all zero bytes, a kept one is the store's bytes, and no
    utterance is dropped by both launches"""
    cfg_a, cfg_t = R.launch_cfg(0, None, 0.0, DROP), R.launch_cfg(1, None, 0.0, DROP)
    seed = _seed_where(lambda s: all(f.any() and not f.all() for f in (R.drop_flags(s, DRAW, ALL, cfg_a["thr_lo"], cfg_a["thr_hi"]),
                                                                       R.drop_flags(s, DRAW, ALL, cfg_t["thr_lo"], cfg_t["thr_hi"]),
                                                                       R.drop_flags(s, DRAW, [1, 5], cfg_a["thr_lo"], cfg_a["thr_hi"]))),
                       "dropped and kept utterances in both launches")
    _, host, _ = _store(name, False)
    for ids in IDS:
        for tail in (5, 0):
            zero = []
            for cfg in (cfg_a, cfg_t):
                got = _run(name, False, ids, tail, shift_rows, cfg, seed)
                flags = R.drop_flags(seed, DRAW, ids, cfg["thr_lo"], cfg["thr_hi"])
                per, row = [], 0
                for i, u in enumerate(ids):
                    rows = got[row:row + LENS[u]]
                    row += LENS[u]
                    per.append(not _bytes(rows).any())
                    if flags[i]:
                        assert per[-1], (ids, u, "a dropped utterance is zero bytes")
                    else:
                        assert torch.equal(_bytes(rows), _bytes(host[OFF[u]:OFF[u + 1]])), (ids, u, "a kept utterance is a bit copy")
                zero.append(flags)
            assert not (zero[0] & zero[1]).any(), "never both"
    fa, ft = (R.drop_flags(seed, DRAW, ALL, c["thr_lo"], c["thr_hi"]) for c in (cfg_a, cfg_t))
    assert fa.any() and not fa.all() and ft.any() and not ft.all()


# ----------------------------------------------------------------------------- noise: finite values, every element against the replica
@pytest.mark.parametrize("name,shift_rows", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("sigma", [0.05, 1.0])
def test_noise_only(name, shift_rows, sigma):
    cfg = R.launch_cfg(0, None, sigma)
    assert cfg["noise_scale"] > 0
    _, host, _ = _store(name, True)
    for ids in IDS:
        for tail in (5, 0):
            got = _run(name, True, ids, tail, shift_rows, cfg, 1234)
    idx = torch.tensor([r for i in IDS[-1] for r in range(OFF[i], OFF[i + 1])])
    delta = (got.float() - host[idx].float())
    assert delta.abs().max() > 0 and delta.abs().max() <= 3.46 * sigma + 0.01 * host.float().abs().max(), "noise was added, bounded by 3.45 sigma"


@pytest.mark.parametrize("name,shift_rows", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("sigma", [0.05, 1.0])
def test_all_three(name, shift_rows, sigma):
    """spans, noise and drop in one launch, text modality: noise first, then exact zeros"""
    cfg = R.launch_cfg(1, SPANS, sigma, DROP)
    spans_ok = lambda s: all(_span_facts(cfg, s).values())      # noqa: E731

    def ok(s):
        f = R.drop_flags(s, DRAW, ALL, cfg["thr_lo"], cfg["thr_hi"])
        kept = [u for u, x in zip(ALL, f) if not x]
        return f.any() and len(kept) >= 3 and spans_ok(s) and any(_span_facts(cfg, s, kept).values())
    seed = _seed_where(ok, "drops, keeps and every kind of span")
    f = R.drop_flags(seed, DRAW, ALL, cfg["thr_lo"], cfg["thr_hi"])
    assert f.any() and not f.all() and all(_span_facts(cfg, seed).values())
    for ids in IDS:
        for tail in (5, 0):
            _run(name, True, ids, tail, shift_rows, cfg, seed)


# ----------------------------------------------------------------------------- keyed by the store id
def test_an_utterance_is_augmented_alike_wherever_it_stands():
    """[3, 3, 3] yields three identical copies; utterance 3 (and 6) comes out the same alone, repeated and in the full batch; another
    draw and another seed change it; the two modalities differ"""
    for name, finite, cfg in (("768 bf16", True, R.launch_cfg(0, SPANS, 0.05)), ("74 fp32", True, R.launch_cfg(0, SPANS, 1.0)),
                              ("5 fp16", False, R.launch_cfg(0, SPANS))):
        seed = _seed_where(lambda s: _span_facts(cfg, s, [3])["inner"] or _span_facts(cfg, s, [3])["edge"], "a span in utterance 3")
        three = _run(name, finite, [3, 3, 3], 5, 0, cfg, seed)
        assert torch.equal(_bytes(three[:64]), _bytes(three[64:128])) and torch.equal(_bytes(three[:64]), _bytes(three[128:]))
        full = _run(name, finite, ALL, 5, 1, cfg, seed)            # 6 5 4 3 ...: utterance 3 starts at row 40 + 1 + 3
        assert torch.equal(_bytes(full[44:108]), _bytes(three[:64]))
        six = _run(name, finite, [6], 0, 0, cfg, seed)
        assert torch.equal(_bytes(full[:40]), _bytes(six))
        other = _run(name, finite, [3, 3, 3], 5, 0, cfg, seed, draw=DRAW + 1)
        assert not torch.equal(_bytes(other), _bytes(three)), "two draws differ"
        other = _run(name, finite, [3, 3, 3], 5, 0, cfg, seed + 1)
        assert not torch.equal(_bytes(other), _bytes(three)), "two seeds differ"
        text = dict(cfg, modality=2)
        other = _run(name, finite, [3, 3, 3], 5, 0, text, seed)
        if cfg["noise_scale"]:
            assert not torch.equal(_bytes(other), _bytes(three)), "the text launch draws its own noise"


def test_many_blocks():
    """a destination of several blocks (768 bf16: 24 KiB per 16 rows) with segment boundaries inside blocks, a 100-row tail, all
    three transforms; and the 74 x fp32 store, whose chunks straddle rows, offset by one row"""
    ids = [3, 6, 3, 2, 3, 6, 0, 3]
    cfg = R.launch_cfg(0, (4, 30, 0.5), 0.05, DROP)

    def ok(s):
        f = R.drop_flags(s, DRAW, ids, cfg["thr_lo"], cfg["thr_hi"])
        kept = [u for u, x in zip(ids, f) if not x]
        return f.any() and 3 in kept and _span_facts(cfg, s, [3])["inner"]
    seed = _seed_where(ok, "a dropped utterance and a span inside utterance 3")
    f = R.drop_flags(seed, DRAW, ids, cfg["thr_lo"], cfg["thr_hi"])
    assert f.any() and not f.all()
    _run("768 bf16", True, ids, 100, 0, cfg, seed)
    _run("74 fp32", True, ids, 100, 1, cfg, seed)
    _run("768 bf16", False, ids, 100, 0, dict(cfg, noise_scale=0.0), seed)


# ----------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused():
    from hri_emo_amd import _lib
    L = _lib.lib()
    dev, host, off_dev = _store("8 bf16", False)
    plan = torch.tensor([0, 0, 1], dtype=torch.int32).cuda()
    dst = torch.full((4 * 16,), POISON, dtype=torch.uint8, device="cuda")
    cfg = R.launch_cfg(0, SPANS, 0.05, DROP)
    good = _args(dev, off_dev, plan, 1, dst.data_ptr(), 4, cfg, 1, 0)
    bad = ((0, None), (3, None), (4, None), (6, None),                      # null pointers
           (5, 0), (5, -1), (5, 513),                                       # n outside [1, 512]
           (14, 5), (14, -1),                                               # spans
           (8, 65536),                                                      # an utterance of 65536 rows
           (2, 3), (2, -1),                                                 # dtype code
           (11, 0), (11, 3),                                                # modality
           (12, cfg["thr_hi"] + 1), (13, 65537),                            # thresholds
           (4, plan.data_ptr() + 2), (3, off_dev.data_ptr() + 4),           # unaligned plan / offsets
           (1, 0), (7, 0), (16, 65537), (17, -1.0), (17, float("nan")), (6, dst.data_ptr() + 1))
    for pos, value in bad:
        args = list(good)
        args[pos] = value
        assert L.hriemo_gather_rows_aug(*args) == 1, (pos, value)
        assert b"gather_rows_aug" in L.hriemo_last_error()
        with pytest.raises(RuntimeError, match="gather_rows_aug"):
            _lib.call("hriemo_gather_rows_aug", *args)
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()), "a refusal launches nothing"
    good[17] = 0.0
    good[12] = good[13] = 0
    good[14] = 0
    assert L.hriemo_gather_rows_aug(*good) == 0                  # nothing enabled: the plain copy
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu()[:16], _bytes(host[0])) and not dst[16:].any()
