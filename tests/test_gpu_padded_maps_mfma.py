"""GPU suite of the attention-map export on PADDED rows from the matrix cores: hriemo_attn_probs_mfma (bf16 operands,
v_mfma_f32_16x16x32_bf16, any key-padding mask) and the models with `set_mfma_maps(True)`.

Kernel level, through the C ABI.  Every case: Q and K are column slices of wider buffers with NaN guard rows on both sides, the map
is a view into a buffer pre-filled with 0xFF bytes (an element that still holds that pattern was not written; the guard bytes on
both sides are compared afterwards), lse comes from hriemo_attn_fwd on the clean operands, the effective seed is SEED + a device
word of the test's own.  `holes` plants NaN into the PAD key rows of K for the export launches only.  Bounds, the project's own for
hriemo_attn_probs: 5e-3 absolute against the float64 softmax of the bf16 operands under the mask, head-averaged
(test_attention_fwd_bwd), rows sum to one within 1e-3 at p = 0 (test_attention_all_pad_row_is_nan), PAD key columns exactly 0.0, an
all-PAD sample NaN in every element.  There are no PAD query rows in a padded problem: every row is computed and compared.
hriemo_attn_probs (the VALU export) runs on the same buffers in every case: same NaN pattern, same PAD-column zeros; the worst
|new - old| is printed, not asserted (both kernels are held to the float64 bound).

Model level: the reference's ragged goldens with the switch on, against the goldens and against the same model with the switch
off; the bounds are those of test_fusion_attention_maps_vs_golden."""
import functools
import math

import pytest
import torch

import hashrng
from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu

SEED, SITE, BOFF = 1234567890123, 40, 3
SEED_DEV = 77          # the device seed word of the launches: a word of the test's own (the process-wide one moves with every captured replay)
GUARD = 3              # guard rows on each side of Q, K and the map
NAN = float("nan")
TOL, TOL_SUM = 5e-3, 1e-3


def _prefix(*valid):
    return lambda Lk: torch.arange(Lk)[None] >= torch.tensor(valid)[:, None]


def _holes(Lk):
    key = torch.arange(Lk)
    return torch.stack([key % 2 == 1,                      # every second key PAD
                        key < 64,                          # a dead first tile
                        (key >= 64) & (key < 128),         # a dead middle tile, live ones either side
                        key < Lk - 1])                     # only the last key valid


#         H, hd, B, Lq, Lk, mask [B, Lk] (True = PAD) or None, NaN in the PAD key rows of K
CASES = {
    "edges": (2, 32, 4, 70, 70, _prefix(1, 16, 65, 70), False),
    "holes": (2, 64, 4, 17, 130, _holes, True),
    "allpad": (2, 32, 3, 20, 70, _prefix(70, 0, 3), False),
    "dropout": (8, 96, 2, 130, 129, _prefix(129, 40), False),
    "hd16": (4, 16, 2, 24, 40, _prefix(9, 33), False),
    "hd128": (2, 128, 2, 66, 72, _prefix(70, 18), False),
    "decoder": (8, 96, 3, 6, 40, _prefix(40, 7, 23), False),
    # two key groups, the second with a partial tile
    "nomask": (2, 32, 2, 33, 193, None, False),
}
RUNS = [("edges", 0.0), ("holes", 0.0), ("allpad", 0.0), ("allpad", 0.1), ("dropout", 0.1), ("hd16", 0.0), ("hd128", 0.0), ("decoder", 0.1),
        ("nomask", 0.0)]


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    before = (_ops.varlen(), _ops.PACKED_MAPS, _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.MFMA_MAPS, _ops.precision())
    yield hri_emo_amd
    hri_emo_amd.set_varlen(before[0])
    _ops.PACKED_MAPS, _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.MFMA_MAPS = before[1:6]
    hri_emo_amd.set_precision(before[6])


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return torch.cuda.current_stream().cuda_stream


def _mask(name):
    Lk, mk = CASES[name][4], CASES[name][5]
    return None if mk is None else mk(Lk)


@functools.lru_cache(maxsize=None)
def _reference(name, p):
    """(q [B*Lq, d], kv [B*Lk, 2d]) in bf16 and the float64 head-averaged (post-dropout) probabilities [B, Lq, Lk]; an all-PAD
    sample is NaN (the softmax of a row of -inf)"""
    nh, hd, B, Lq, Lk, _, _ = CASES[name]
    d = nh * hd
    g = torch.Generator().manual_seed(2000 + Lq + Lk + hd)
    q = (torch.randn(B * Lq, d, generator=g) * 1.5).bfloat16()
    kv = torch.randn(B * Lk, 2 * d, generator=g).bfloat16()
    kpm = _mask(name)
    qh = q.double().view(B, Lq, nh, hd).transpose(1, 2)
    kh = kv[:, :d].double().view(B, Lk, nh, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(hd)
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], -math.inf)
    pr = torch.softmax(s, -1)
    if p > 0:
        keep = hashrng.attn_mask(SEED + SEED_DEV, SITE, B, nh, Lq, Lk, p, BOFF)
        pr = pr * torch.from_numpy(keep).double() * hashrng.inv_keep(p)
    return q, kv, pr.mean(1)


class GuardedMap:
    """[B, Lq, Lk] fp32 inside a buffer of 0xFF bytes, GUARD rows of Lk floats on each side"""

    def __init__(self, B, Lq, Lk):
        self.shape, self.g = (B, Lq, Lk), GUARD * Lk * 4
        self.raw = torch.full((2 * self.g + B * Lq * Lk * 4,), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.raw[self.g:self.g + B * Lq * Lk * 4].view(torch.float32).view(B, Lq, Lk)

    def host(self):
        """(the map, a mask of the elements that were never written, guard bytes intact)"""
        by = self.raw.cpu()
        m = by[self.g:len(by) - self.g].clone()
        unwritten = (m.view(torch.int32) == -1).view(self.shape)
        return m.view(torch.float32).view(self.shape), unwritten, bool((by[:self.g] == 0xFF).all() and (by[len(by) - self.g:] == 0xFF).all())


def _export(name, p):
    """both padded exports of a case through the C ABI on the same buffers -> (GuardedMap of the MFMA export, of the VALU export)"""
    from hri_emo_amd import _lib
    nh, hd, B, Lq, Lk, _, plant = CASES[name]
    q, kv, _ = _reference(name, p)
    kpm = _mask(name)
    d = nh * hd
    qw = torch.full((B * Lq + 2 * GUARD, 2 * d), NAN, dtype=torch.bfloat16, device="cuda")          # Q = the right half of a [N, 2d] buffer
    qw[GUARD:GUARD + B * Lq, d:] = q
    kw = torch.full((B * Lk + 2 * GUARD, 3 * d), NAN, dtype=torch.bfloat16, device="cuda")          # K | V = the left two thirds of a [N, 3d] buffer
    kw[GUARD:GUARD + B * Lk, :2 * d] = kv
    Q, K, V = qw[GUARD:GUARD + B * Lq, d:], kw[GUARD:GUARD + B * Lk, :d], kw[GUARD:GUARD + B * Lk, d:2 * d]
    kpm_d = None if kpm is None else kpm.cuda().view(torch.uint8).contiguous()
    o = torch.empty((B * Lq, d), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, nh, Lq), NAN, dtype=torch.float32, device="cuda")
    sw = torch.full((1,), SEED_DEV, dtype=torch.int64, device="cuda")          # effective seed = SEED + the device word
    _lib.call("hriemo_attn_fwd", P(Q), Q.stride(0), P(K), K.stride(0), P(V), V.stride(0), P(o), d, P(kpm_d), P(lse), B, nh, Lq, Lk, hd,
              float(p), SEED, P(sw), SITE, BOFF, None, ST())
    torch.cuda.synchronize()
    if kpm is not None and bool(kpm.all(1).any()):
        dead = kpm.all(1)
        assert bool((lse.cpu()[dead] == -math.inf).all()), "the lse of an all-PAD sample is -inf"
        assert not bool(torch.isinf(lse.cpu()[~dead]).any())
    if plant:
        K[kpm.reshape(-1).cuda()] = NAN          # the export launches only: a PAD key's row of K reaches no output element
    new, old = GuardedMap(B, Lq, Lk), GuardedMap(B, Lq, Lk)
    for entry, out in (("hriemo_attn_probs_mfma", new), ("hriemo_attn_probs", old)):
        _lib.call(entry, P(Q), Q.stride(0), P(K), K.stride(0), P(kpm_d), P(lse), P(out.t), B, nh, Lq, Lk, hd, float(p), SEED, P(sw), SITE,
                  BOFF, ST())
    torch.cuda.synchronize()
    return new, old


@pytest.mark.parametrize("name,p", RUNS, ids=[f"{n}-p{p}" for n, p in RUNS])
def test_padded_mfma_export_against_float64_and_the_valu_export(H, name, p):
    nh, hd, B, Lq, Lk, _, _ = CASES[name]
    ref = _reference(name, p)[2]
    kpm = _mask(name)
    if kpm is None:
        kpm = torch.zeros((B, Lk), dtype=torch.bool)
    good = ~kpm.all(1)          # samples with at least one valid key
    assert (name == "allpad") == (not bool(good.all()))
    new, old = _export(name, p)
    got, unwritten, intact = new.host()
    was, unwritten_old, intact_old = old.host()
    assert not bool(unwritten.any()), f"{int(unwritten.sum())} elements of the map were not written"
    assert intact, "the export wrote outside the map"
    assert not bool(unwritten_old.any()) and intact_old
    # NaN: every element of an all-PAD sample, and nowhere else (no guard row, pad column or poisoned PAD key row was read)
    nan = torch.isnan(got)
    assert bool(nan[~good].all()), "an all-PAD sample is NaN in every element"
    assert not bool(nan[good].any()), "NaN in a sample that has a valid key"
    g64 = got[good].double()
    worst = float((g64 - ref[good]).abs().max())
    sums = g64.sum(-1)
    worst_sum = float((sums - 1).abs().max()) if p == 0 else 0.0
    cols = kpm[good][:, None, :].expand(int(good.sum()), Lq, Lk)
    assert float(got[good][cols].abs().max()) == 0.0 if bool(cols.any()) else True, "PAD key columns are exact zeros"
    # against the parent's kernel on the same buffers
    assert torch.equal(nan, torch.isnan(was)), "NaN pattern of the VALU export"
    assert float(was[good][cols].abs().max()) == 0.0 if bool(cols.any()) else True
    diff = float((got[good] - was[good]).abs().max())
    print(f"{name} p={p}: worst |got - float64| {worst:.2e} (bound {TOL:.0e}), worst |row sum - 1| {worst_sum:.2e} (bound {TOL_SUM:.0e}), "
          f"worst |mfma - valu| {diff:.2e}")
    assert worst <= TOL, (name, worst)
    assert worst_sum <= TOL_SUM, (name, worst_sum)
    if p > 0:
        assert int(((sums - 1).abs() > 1e-2).sum()) > 0, "no row sum shows the dropout: the test would not see a wrong key"


def test_padded_mfma_export_refusals(H):
    """one refusal per check: non-zero, hriemo_last_error set, nothing launched (the NaN-filled output stays as it is)"""
    from hri_emo_amd import _lib
    L = _lib.lib()
    fn = L.hriemo_attn_probs_mfma
    nh, hd, B, Lq, Lk = 2, 32, 2, 9, 7
    d = nh * hd
    q = torch.zeros((B * Lq, d + 8), dtype=torch.bfloat16, device="cuda")
    k = torch.zeros((B * Lk, d + 8), dtype=torch.bfloat16, device="cuda")
    kpm = torch.zeros((B, Lk), dtype=torch.uint8, device="cuda")
    lse = torch.zeros((B, nh, Lq), dtype=torch.float32, device="cuda")
    probs = torch.full((B, Lq, Lk), NAN, dtype=torch.float32, device="cuda")
    good = dict(Q=P(q), ldq=d + 8, K=P(k), ldk=d + 8, kpm=P(kpm), lse=P(lse), probs=P(probs), B=B, H=nh, Lq=Lq, Lk=Lk, hd=hd, p=0.0)
    bad = {
        "empty problem": dict(B=0),
        "empty problem (no keys)": dict(Lk=0),
        "no Q": dict(Q=None),
        "no K": dict(K=None),
        "no lse": dict(lse=None),
        "no output": dict(probs=None),
        "head width not built": dict(hd=48),
        "leading dimension of Q": dict(ldq=d + 9),
        "leading dimension of K": dict(ldk=d + 12),
        "unaligned Q": dict(Q=P(q) + 2),
        "unaligned K": dict(K=P(k) + 2),
        "unaligned lse": dict(lse=P(lse) + 2),
        "unaligned output": dict(probs=P(probs) + 2),
        "dropout 1": dict(p=1.0),
        "dropout below 0": dict(p=-0.1),
        "B beyond the grid": dict(B=65536),
    }

    def call(a):
        return fn(a["Q"], a["ldq"], a["K"], a["ldk"], a["kpm"], a["lse"], a["probs"], a["B"], a["H"], a["Lq"], a["Lk"], a["hd"], a["p"], 0,
                  None, 0, 0, ST())

    for what, change in bad.items():
        assert call(dict(good, **change)) != 0, what
        assert L.hriemo_last_error().decode() != "", what
    torch.cuda.synchronize()
    assert bool(torch.isnan(probs).all()), "a refused call launched"
    # and the same arguments unchanged are accepted, with the mask and without
    assert call(good) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(probs).any())
    assert call(dict(good, kpm=None)) == 0
    torch.cuda.synchronize()


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


def _mode(H, varlen=False, maps=False, tail=False, mfma=False):
    from hri_emo_amd import _ops
    H.set_varlen(varlen)
    H.set_varlen_maps(maps)
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = tail
    H.set_mfma_maps(mfma)


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


def _same_nan_worst_diff(got, pad, what):
    """every element, PAD query rows included: the same NaN pattern asserted; the worst difference where there is a number"""
    assert torch.equal(torch.isnan(got), torch.isnan(pad)), (what, "NaN pattern")
    ok = ~torch.isnan(pad)
    return float((got - pad)[ok].abs().max()) if bool(ok.any()) else 0.0


@pytest.mark.parametrize("gname,d,ne", GOLDENS)
def test_goldens_through_the_padded_mfma_export(H, monkeypatch, gname, d, ne):
    g = load_golden(gname)
    m = fusion(H, d, ne).eval()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    with torch.no_grad():
        _mode(H)
        ref = m(*args, return_attention=True)
        _mode(H, mfma=True)
        names = _spy(monkeypatch)
        logits, beta, z, pack = m(*args, return_attention=True)
        calls = list(names)
    close(logits, g["logits"], 5e-3, "logits"); close(z, g["z"], 5e-3, "z"); close(beta, g["beta"], 5e-3, "beta")
    assert len(pack["encoder"]) == 2 and len(pack["decoder"]) == 2
    valid = _valid(g, m)
    worst = worst_off = 0.0
    for (what, got, qs, ks), (_, pad, _, _) in zip(_maps(pack), _maps(ref[3])):
        gold = g[what]
        assert got.shape == gold.shape, (what, got.shape, gold.shape)
        vq = valid[qs] if qs is not None else torch.ones(got.shape[:2], dtype=torch.bool)
        rows = vq[:, :, None].expand_as(got)
        cols = valid[ks][:, None, :].expand_as(got)
        assert not torch.isnan(got).any(), what
        worst = max(worst, close(torch.where(rows, got, gold), gold, 2e-2, what))              # valid query rows (all rows of a decoder map)
        assert float(got[~cols].abs().max()) == 0.0 if bool((~cols).any()) else True, (what, "PAD key columns")
        assert float((got.sum(-1) - 1).abs().max()) <= 5e-3, (what, "rows sum to one")          # PAD query rows are computed too
        worst_off = max(worst_off, _same_nan_worst_diff(got, pad, what))
    print(f"{gname}: worst map error vs the golden {worst:.2e}, MFMA vs VALU export {worst_off:.2e}")
    assert worst_off <= 5e-3, worst_off
    layers, dec = len(m.cross_modal.layers), len(m.emotion_decoder.layers)
    assert calls.count("hriemo_attn_probs") == 0, calls.count("hriemo_attn_probs")
    assert calls.count("hriemo_attn_probs_mfma") == 4 * layers + dec, calls.count("hriemo_attn_probs_mfma")


def test_train_mode_maps_equal_the_valu_export_under_the_same_seed(H):
    """dropout 0.1, one seed: the export replays the forward's keep mask.  The closed-form weights make the softmaxes peaked (max p
    ~ 0.9999), so one wrongly keyed element moves a head-averaged weight by ~ 1 / (8 heads x 0.9) = 0.14 against the 5e-3 asked.
    The export feeds nothing back into the forward, so logits / beta / z are bit-equal."""
    g = load_golden("hd96_eval_ragged")
    m = fusion(H, 768, 6, p=0.1).train()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    out = []
    with torch.no_grad():
        for mfma in (False, True):
            _mode(H, mfma=mfma)
            torch.manual_seed(77)                    # the step's dropout seed comes from torch's generator
            out.append(m(*args, return_attention=True))
    worst, dropped = 0.0, 0
    for (what, got, _, _), (_, pad, _, _) in zip(_maps(out[1][3]), _maps(out[0][3])):
        worst = max(worst, _same_nan_worst_diff(got, pad, what))
        dropped += int(((got.sum(-1) - 1).abs() > 1e-2).sum())
    print(f"train mode, dropout 0.1: MFMA vs VALU maps {worst:.2e}; rows whose sum shows the dropout: {dropped}")
    assert worst <= 5e-3, worst
    assert dropped > 0, "the maps show no dropout: the test would not see a wrong key"
    for a, b, what in zip(out[1][:3], out[0][:3], ("logits", "beta", "z")):
        assert torch.equal(a, b), what


def test_decoder_maps_under_varlen_with_the_tail_off(H, monkeypatch):
    """varlen + packed maps, packed tail off: the decoder reads a padded memory, so its maps (and only those) are the padded export's"""
    g = load_golden("cfg1_eval_ragged")
    m = fusion(H, 128, 4).eval()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    _mode(H, varlen=True, maps=True, tail=False, mfma=True)
    names = _spy(monkeypatch)
    with torch.no_grad():
        m(*args, return_attention=True)
    layers, dec = len(m.cross_modal.layers), len(m.emotion_decoder.layers)
    assert names.count("hriemo_attn_probs_mfma") == dec, names.count("hriemo_attn_probs_mfma")
    assert names.count("hriemo_attn_probs") == 0
    assert names.count("hriemo_attn_probs_varlen") == 4 * layers


def test_switch_off_keeps_the_valu_export(H, monkeypatch):
    """what test_switch_off_keeps_the_padded_export counts: set_varlen(True) alone, the maps come from hriemo_attn_probs"""
    g = load_golden("cfg1_eval_ragged")
    m = fusion(H, 128, 4).eval()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    _mode(H, varlen=True, maps=False, tail=True, mfma=False)
    names = _spy(monkeypatch)
    with torch.no_grad():
        m(*args, return_attention=True)
    assert names.count("hriemo_attn_probs_mfma") == 0
    assert names.count("hriemo_attn_probs_varlen") == 0 and names.count("hriemo_pack_rows") == 0
    assert names.count("hriemo_attn_probs") == 4 * len(m.cross_modal.layers) + len(m.emotion_decoder.layers)
