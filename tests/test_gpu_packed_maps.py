"""GPU suite of the attention-map export on packed (varlen) rows: hriemo_attn_probs_varlen (bf16 operands, v_mfma_f32_16x16x32_bf16)
and hriemo_attn_probs_f32_varlen (the fp32 mode's twin), and the models with `set_varlen(True)` + `set_varlen_maps(True)`.

Kernel level, through the C ABI.  Every case: the output is pre-filled with NaN (so a NaN-free result proves that every element
was written and that no poisoned row was read), Q and K are column slices of wider buffers, the K buffer carries NaN rows behind
cu_k[B], lse comes from the varlen forward on the same operands.  Bounds: 5e-3 absolute against the float64 softmax of the same
operands, head-averaged (the bound of hriemo_attn_probs in test_attention_fwd_bwd), rows sum to one within 1e-3 at p = 0
(test_attention_all_pad_row_is_nan); the fp32 twin 2e-6 and 1e-5 (tests/test_gpu_fp32_mode.py on the padded fp32 export).  The
operands hold bf16-representable values in both precisions, so one float64 reference serves both.

Model level: the reference's ragged goldens through the packed export, with the packed tail off and on, in both precisions; the
bounds are those of test_fusion_attention_maps_vs_golden(_fp32).  The padded path computes the PAD query rows of a map and the
packed path never does: they are exact zeros here and are compared with nothing."""
import functools
import math

import numpy as np
import pytest
import torch

import hashrng
from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu

SEED, SITE, BOFF = 1234567890123, 40, 3
SEED_DEV = 77          # the device seed word of the launches: a word of the test's own (the process-wide one moves with every captured replay)
SURPLUS = 5          # NaN rows behind cu_k[B]
NAN = float("nan")
#         H, hd, query lengths, key lengths, (out_lq, out_lk), p
CASES = {
    # length 1, the 16- and 64-row tile edges, one key past a tile, a whole query tile past a sample's end, a map wider than the
    # longest sequence
    "edges": (2, 32, [1, 17, 64], [16, 1, 65], (70, 70), 0.0),
    # three query blocks, a second key group, dropout: the keep mask of tests/hashrng.py sliced per sample
    "dropout": (8, 96, [130, 33], [40, 129], (130, 129), 0.1),
    "hd16": (4, 16, [20, 5], [9, 33], (24, 40), 0.0),
    "hd128": (2, 128, [66, 3], [70, 18], (66, 72), 0.0),
    # the decoder's form: N_e = 6 queries per sample (query_seq), a map as wide as the padded memory
    "decoder": (8, 96, [6, 6, 6], [40, 7, 23], (6, 40), 0.0),
}
BOUNDS = {False: (5e-3, 1e-3), True: (2e-6, 1e-5)}          # fp32 twin? -> (elementwise, row sum)
ENTRY = {False: ("hriemo_attn_fwd_varlen", "hriemo_attn_probs_varlen"), True: ("hriemo_attn_fwd_f32_varlen", "hriemo_attn_probs_f32_varlen")}


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    before = (_ops.varlen(), _ops.PACKED_MAPS, _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.precision())
    yield hri_emo_amd
    hri_emo_amd.set_varlen(before[0])
    _ops.PACKED_MAPS, _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32 = before[1:4]
    hri_emo_amd.set_precision(before[4])


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return torch.cuda.current_stream().cuda_stream


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(q [Nq, d], kv [Nk, 2d]) in bf16 and, per sample, the float64 head-averaged (post-dropout) probabilities [lq, lk]"""
    nh, hd, lq, lk, _, p = CASES[name]
    d = nh * hd
    g = torch.Generator().manual_seed(1000 + sum(lq) + sum(lk) + hd)
    q = (torch.randn(sum(lq), d, generator=g) * 1.5).bfloat16()
    kv = torch.randn(sum(lk), 2 * d, generator=g).bfloat16()
    keep = hashrng.attn_mask(SEED + SEED_DEV, SITE, len(lq), nh, max(lq), max(lk), p, BOFF) if p > 0 else None
    refs, rq, rk = [], 0, 0
    for b, (nq, nk) in enumerate(zip(lq, lk)):
        qb = q[rq:rq + nq].double().view(nq, nh, hd).transpose(0, 1)
        kb = kv[rk:rk + nk, :d].double().view(nk, nh, hd).transpose(0, 1)
        pr = torch.softmax(qb @ kb.transpose(-1, -2) / math.sqrt(hd), -1)
        if keep is not None:
            pr = pr * torch.from_numpy(keep[b, :, :nq, :nk]).double() * hashrng.inv_keep(p)
        refs.append(pr.mean(0))
        rq, rk = rq + nq, rk + nk
    return q, kv, refs


def _export(name, f32):
    """the packed export of a case through the C ABI -> probs [B, out_lq, out_lk] on the host"""
    from hri_emo_amd import _lib
    nh, hd, lq, lk, (olq, olk), p = CASES[name]
    q, kv, _ = _reference(name)
    d, B, nq, nk = nh * hd, len(lq), sum(lq), sum(lk)
    dt = torch.float32 if f32 else torch.bfloat16
    qw = torch.full((nq, 2 * d), NAN, dtype=dt, device="cuda")                     # Q = the right half of a [N, 2d] buffer
    qw[:, d:] = q.to(dt)
    kw = torch.full((nk + SURPLUS, 3 * d), NAN, dtype=dt, device="cuda")           # K | V = the left two thirds of a [N, 3d] buffer
    kw[:nk, :2 * d] = kv.to(dt)
    Q, K, V = qw[:, d:], kw[:, :d], kw[:, d:2 * d]
    cq, ck = _cu(lq), _cu(lk)
    o = torch.empty((nq, d), dtype=dt, device="cuda")
    lse = torch.full((B, nh, max(lq)), NAN, dtype=torch.float32, device="cuda")
    sw = torch.full((1,), SEED_DEV, dtype=torch.int64, device="cuda")          # effective seed = SEED + the device word
    fwd, exp = ENTRY[f32]
    tail = (float(p), SEED, P(sw), SITE, BOFF) + (() if f32 else (None,)) + (ST(),)
    _lib.call(fwd, P(Q), Q.stride(0), P(K), K.stride(0), P(V), V.stride(0), P(o), d, P(cq), P(ck), P(lse), B, nh, max(lq), max(lk), hd, *tail)
    probs = torch.full((B, olq, olk), NAN, dtype=torch.float32, device="cuda")
    _lib.call(exp, P(Q), Q.stride(0), P(K), K.stride(0), P(cq), P(ck), P(lse), P(probs), B, nh, max(lq), max(lk), olq, olk, hd,
              float(p), SEED, P(sw), SITE, BOFF, ST())
    torch.cuda.synchronize()
    return probs.cpu()


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(CASES))
def test_packed_export_against_float64(H, name, f32):
    nh, hd, lq, lk, (olq, olk), p = CASES[name]
    tol, tol_sum = BOUNDS[f32]
    probs = _export(name, f32)
    refs = _reference(name)[2]
    assert not torch.isnan(probs).any(), "an element was not written, or a poisoned row / column was read"
    worst = worst_sum = 0.0
    for b, (nq, nk) in enumerate(zip(lq, lk)):
        assert float(probs[b, :, nk:].abs().max()) == 0.0 if nk < olk else True, ("PAD key columns", b)
        assert float(probs[b, nq:, :].abs().max()) == 0.0 if nq < olq else True, ("PAD query rows", b)
        got = probs[b, :nq, :nk].double()
        worst = max(worst, float((got - refs[b]).abs().max()))
        if p == 0:
            worst_sum = max(worst_sum, float((got.sum(-1) - 1).abs().max()))
    print(f"{name} {'fp32' if f32 else 'bf16'}: worst |got - float64| {worst:.2e} (bound {tol:.0e}), worst |row sum - 1| {worst_sum:.2e} (bound {tol_sum:.0e})")
    assert worst <= tol, (name, worst)
    assert worst_sum <= tol_sum, (name, worst_sum)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_packed_export_refusals(H, f32):
    """one refusal per check: non-zero, hriemo_last_error set, nothing launched (the NaN-filled output stays as it is)"""
    from hri_emo_amd import _lib
    L = _lib.lib()
    fn = getattr(L, ENTRY[f32][1])
    nh, hd, B, lq, lk = 2, 32, 2, [5, 9], [7, 3]
    d = nh * hd
    dt = torch.float32 if f32 else torch.bfloat16
    q = torch.zeros((sum(lq), d + 8), dtype=dt, device="cuda")
    k = torch.zeros((sum(lk), d + 8), dtype=dt, device="cuda")
    cq, ck = _cu(lq), _cu(lk)
    lse = torch.zeros((B, nh, 9), dtype=torch.float32, device="cuda")
    probs = torch.full((B, 12, 12), NAN, dtype=torch.float32, device="cuda")
    good = dict(Q=P(q), ldq=d + 8, K=P(k), ldk=d + 8, cq=P(cq), ck=P(ck), lse=P(lse), probs=P(probs), B=B, H=nh, mq=9, mk=7, olq=12, olk=12, hd=hd)
    el = q.element_size()
    bad = {
        "empty problem": dict(B=0),
        "empty problem (no output)": dict(probs=None),
        "head width not built": dict(hd=48),
        "leading dimension": dict(ldq=d + 9),
        "unaligned operand": dict(K=P(k) + el),
        "map shorter than the longest query sequence": dict(olq=8),
        "map narrower than the longest key sequence": dict(olk=6),
        "cu_seqlens_k missing": dict(ck=None),
        "cu_seqlens_q missing": dict(cq=None),
    }
    for what, change in bad.items():
        a = dict(good, **change)
        rc = fn(a["Q"], a["ldq"], a["K"], a["ldk"], a["cq"], a["ck"], a["lse"], a["probs"], a["B"], a["H"], a["mq"], a["mk"], a["olq"],
                a["olk"], a["hd"], 0.0, 0, None, 0, 0, ST())
        assert rc != 0, what
        assert L.hriemo_last_error().decode() != "", what
    torch.cuda.synchronize()
    assert bool(torch.isnan(probs).all()), "a refused call launched"
    # and the same arguments unchanged are accepted
    a = good
    assert fn(a["Q"], a["ldq"], a["K"], a["ldk"], a["cq"], a["ck"], a["lse"], a["probs"], a["B"], a["H"], a["mq"], a["mk"], a["olq"], a["olk"],
              a["hd"], 0.0, 0, None, 0, 0, ST()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(probs).any())


# ----------------------------------------------------------------------------- model level
GOLDENS = [("cfg1_eval_ragged", 128, 4), ("hd96_eval_ragged", 768, 6)]
QK = {"audio_self": ("a", "a"), "text_self": ("t", "t"), "audio_queries_text": ("a", "t"), "text_queries_audio": ("t", "a")}


def fusion(H, d, ne, p=0.1):
    return O.closed_form_init_(H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=p)).cuda()


def close(got, ref, tol, what=""):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= tol * max(1.0, ref.abs().max().item()), (what, err, ref.abs().max().item())
    return err


def _mode(H, varlen, maps, tail):
    from hri_emo_amd import _ops
    H.set_varlen(varlen)
    H.set_varlen_maps(maps)
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = tail


def _valid(g, m):
    """valid-position masks [B, L] of audio, text and the fused memory"""
    ma, mt = g["mask_a"], g["mask_t"]
    return {"a": ~ma, "t": ~mt, "f": ~m._build_fused_mask(ma, mt, g["h_t"].shape[1])}


def _maps(pack):
    """[(name, map on the host, query side, key side)] of a return_attention pack; the decoder's queries are all valid"""
    out = []
    for li, maps in enumerate(pack["encoder"]):
        out += [(f"enc.{li}.{k}", v.float().cpu(), QK[k][0], QK[k][1]) for k, v in maps.items()]
    out += [(f"dec.{li}", v.float().cpu(), None, "f") for li, v in enumerate(pack["decoder"])]
    return out


def _spy(monkeypatch):
    from hri_emo_amd import _lib
    names, real = [], _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    return names


def _golden_through_the_packed_export(H, monkeypatch, gname, d, ne, tail, fp32):
    tol_out, tol_map, tol_sum = (1e-4, 1e-4, 1e-5) if fp32 else (5e-3, 2e-2, 5e-3)          # test_fusion_attention_maps_vs_golden(_fp32)
    packed_name, padded_name = ("hriemo_attn_probs_f32_varlen", "hriemo_attn_probs_f32") if fp32 else ("hriemo_attn_probs_varlen", "hriemo_attn_probs")
    if fp32:
        H.set_precision("fp32")
    g = load_golden(gname)
    m = fusion(H, d, ne).eval()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    with torch.no_grad():
        _mode(H, False, False, False)
        ref = m(*args, return_attention=True)
        _mode(H, True, True, tail)
        names = _spy(monkeypatch)
        logits, beta, z, pack = m(*args, return_attention=True)
        calls = list(names)
    close(logits, g["logits"], tol_out, "logits"); close(z, g["z"], tol_out, "z"); close(beta, g["beta"], tol_out, "beta")
    assert len(pack["encoder"]) == 2 and len(pack["decoder"]) == 2
    valid = _valid(g, m)
    worst = worst_pad = 0.0
    for (what, got, qs, ks), (_, pad, _, _) in zip(_maps(pack), _maps(ref[3])):
        gold = g[what]
        assert got.shape == gold.shape, (what, got.shape, gold.shape)
        vq = valid[qs] if qs is not None else torch.ones(got.shape[:2], dtype=torch.bool)
        vk = valid[ks]
        rows = vq[:, :, None].expand_as(got)
        cols = vk[:, None, :].expand_as(got)
        assert not torch.isnan(got).any(), what
        worst = max(worst, close(torch.where(rows, got, gold), gold, tol_map, what))              # valid query rows (all rows of a decoder map)
        assert float(got[~cols].abs().max()) == 0.0 if bool((~cols).any()) else True, (what, "PAD key columns")
        assert float(got[~rows].abs().max()) == 0.0 if bool((~rows).any()) else True, (what, "PAD query rows")
        sums = got.sum(-1)
        assert float((sums - 1)[vq].abs().max()) <= tol_sum, (what, "rows sum to one")
        worst_pad = max(worst_pad, float((got - pad)[rows].abs().max()))                            # packed against padded, same model
    print(f"{gname} tail={tail} {'fp32' if fp32 else 'bf16'}: worst map error vs the golden {worst:.2e}, packed vs padded {worst_pad:.2e}")
    assert worst_pad <= (1e-4 if fp32 else 5e-3), worst_pad
    # the launches: two input packs, four packed exports per encoder layer, the decoder's two with the packed tail; with the tail
    # off the decoder reads a padded memory again, so its two maps (and only those) are the padded export's
    layers, dec = len(m.cross_modal.layers), len(m.emotion_decoder.layers)
    assert calls.count("hriemo_pack_rows") == 2, calls.count("hriemo_pack_rows")
    assert calls.count(packed_name) == 4 * layers + (dec if tail else 0), calls.count(packed_name)
    assert calls.count(padded_name) == (0 if tail else dec), calls.count(padded_name)


@pytest.mark.parametrize("tail", [False, True], ids=["tail_off", "tail_on"])
@pytest.mark.parametrize("gname,d,ne", GOLDENS)
def test_goldens_through_the_packed_export(H, monkeypatch, gname, d, ne, tail):
    _golden_through_the_packed_export(H, monkeypatch, gname, d, ne, tail, fp32=False)


@pytest.mark.parametrize("tail", [False, True], ids=["tail_off", "tail_on"])
@pytest.mark.parametrize("gname,d,ne", GOLDENS)
def test_goldens_through_the_packed_export_fp32(H, monkeypatch, gname, d, ne, tail):
    _golden_through_the_packed_export(H, monkeypatch, gname, d, ne, tail, fp32=True)


def test_train_mode_maps_equal_the_padded_path_under_the_same_seed(H):
    """dropout 0.1, one seed: the packed export replays the forward's keep mask (keyed by position within the sample = the padded
    indices).  The closed-form weights make the softmaxes peaked (max p ~ 0.9999), so one wrongly keyed element moves a
    head-averaged weight by ~ 1 / (8 heads x 0.9) = 0.14 against the 5e-3 asked."""
    g = load_golden("hd96_eval_ragged")
    m = fusion(H, 768, 6, p=0.1).train()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    out = []
    with torch.no_grad():
        for varlen, maps, tail in ((False, False, False), (True, True, True)):
            _mode(H, varlen, maps, tail)
            torch.manual_seed(77)                    # the step's dropout seed comes from torch's generator
            out.append(m(*args, return_attention=True))
    valid = _valid(g, m)
    worst, dropped = 0.0, 0
    for (what, got, qs, _), (_, pad, _, _) in zip(_maps(out[1][3]), _maps(out[0][3])):
        vq = valid[qs] if qs is not None else torch.ones(got.shape[:2], dtype=torch.bool)
        rows = vq[:, :, None].expand_as(got)
        assert not torch.isnan(got).any(), what
        worst = max(worst, float((got - pad)[rows].abs().max()))
        dropped += int(((got.sum(-1) - 1).abs() > 1e-2)[vq].sum())
    print(f"train mode, dropout 0.1: packed vs padded maps {worst:.2e}; rows whose sum shows the dropout: {dropped}")
    assert worst <= 5e-3, worst
    assert dropped > 0, "the maps show no dropout: the test would not see a wrong key"
    for a, b, what in zip(out[1][:3], out[0][:3], ("logits", "beta", "z")):
        close(a, b, 5e-3, what)


def test_switch_off_keeps_the_padded_export(H, monkeypatch):
    """set_varlen(True) alone: asking for the maps sends the forward to the padded layout, as before"""
    g = load_golden("cfg1_eval_ragged")
    m = fusion(H, 128, 4).eval()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    _mode(H, True, False, True)
    names = _spy(monkeypatch)
    with torch.no_grad():
        m(*args, return_attention=True)
    assert names.count("hriemo_attn_probs_varlen") == 0 and names.count("hriemo_pack_rows") == 0
    assert names.count("hriemo_attn_probs") == 4 * len(m.cross_modal.layers) + len(m.emotion_decoder.layers)
