"""Host-side references, fp32 yardsticks, limits and edge tables for the fp32 precision mode (hri-emo_amd/csrc/fp32mode.hip): no GPU.

Everything the mode computes is fp32 in and fp32 out, so every limit here is  F * v * mag  with v = 2^-24 and `mag` the magnitude
of the float64 reference (the same expression with absolute values of its terms): never a fraction of max|ref|, so that one wrong
row of small magnitude cannot hide behind a large one.  What is reused, not re-derived:

    attn_reference   reference / magnitude / key_padding_mask / EDGE_LENGTHS / heads / rows / _run (the closed form and its hooks)
    rowops_reference ln_case / ln_fwd_ref / ln_bwd_ref / fwd32 / bwd32 / reduce32 (with their fault= arms) / colsum_ref /
                     rowdot_bwd_ref / check_elem / ratio_v / GuardedVec, LN_MARGIN
    gate_reference   PRE_MAX, sigmoid_inputs, sigmoid_ref, gin_bwd_case (a == t columns), FUSE_ROUNDINGS
    gemm_reference   Guarded, V;   hashrng: the dropout hash

New here:

attention   attn_yard32(): the closed form of attn_reference._run in fp32 on the CPU, in three orders (ATTN_ORDERS): torch's; key
            tiles of 64 with the kernel's online rescaling (running max, corr = exp(m_old - m_new), the denominator over all keys,
            dropout after the normalisation), the backward's dQ summed over key tiles and dK / dV over query tiles, every
            contraction as the MFMA chain forms it (four terms per step, the steps added in turn: _chain4); the tiles and the
            chains in reverse.  Outputs O, lse, dQ, dK, dV and the head-mean map Pmean.  Magnitudes: attn_reference.magnitude for O / dQ / dK
            / dV, |m| + 1 for lse (m the row maximum of S), mean_h P for the map.  check_attn() keeps both criteria of
            attn_reference.check with u replaced by v:
              elementwise   |got - ref| <= ATTN_FACTOR[out] v mag;  mag == 0 (dK / dV rows of PAD keys, PAD map columns): exactly 0
              per tile      every (batch, head, 64-row block): ||got - ref|| <= 3 max(max_order ||yard - ref||, r ||mag||) + v ||mag||
                            r = max_order ||yard - ref|| / ||mag|| over the WHOLE output of the case: the yardsticks' own pooled
                            error level.  A tile norm is a statistic; a ragged last tile of one row (L = 65, 129), the one
                            element of lse in it, or a dV tile whose every element carries the error of one probability (Lq = 1)
                            holds one draw, and the yardsticks' own draw there lies anywhere from 0.03 to 3 times their level:
                            such a tile is held to the pooled level instead of to a lucky draw.  The last term: the result's own
                            rounding to fp32, <= v |ref| <= v mag per element, which float64 does not have where it is exact by
                            cancellation -- one valid key: P = 1, dS = 0
            ATTN_FACTOR = TILE_FACTOR x ATTN_ENVELOPE, the MEASURED envelope of the three orders against float64 over ATTN_CASES
            (the roundings of S are not in `mag`, which counts one rounding per operand of the last product; they scale with
            |q||k| / sqrt(hd) and are what the measurement is for).
LayerNorm   the fp32 kernels take fp32 G / X / dY and recompute the row statistics in the backward, so LN_FACTOR of
            rowops_reference (bf16 inputs, statistics handed over) does not apply: LN32_ENVELOPE is measured the same way over
            LN32_FWD_CASES + LN32_BWD_CASES and every order of ROW_ORDERS ('quad' is the kernels' own lane mapping).
sums        colsum_f32, rowdot_bwd_f32, dbeta, masked_mean_f32, gate_dpre_f32: n fp32 terms, factor n (+ 1 per rounded product, + 1
            for a destination really added), the derivable rule of rowops_reference.check_sum.
splits      split_host(): hi / mid / lo from torch's bf16 rounding, split_layout(): the eight block orders of split3g_kernel.

The worst error / limit per output observed on the MI355X: profiles/2026-10-19_fp32_kernel_limits.log.
test_fp32_bound_host.py proves on the CPU that the limits pass every yardstick order and fail planted mistakes."""
import math
import re

import numpy as np
import torch

import attn_reference as A
import gate_reference as G  # (PRE_MAX, sigmoid_inputs, sigmoid_ref, gin_bwd_case: the GPU suite uses them through this module)
import hashrng
import rowops_reference as R
from gemm_reference import V, Guarded  # noqa: F401
from rowops_reference import GuardedVec, LN_MARGIN  # noqa: F401

TILE_FACTOR = A.TILE_FACTOR
HEADS = 2
ATTN_ORDERS = ("torch", "tiles", "tiles_rev")
ATTN_OUTPUTS = ("O", "lse", "dQ", "dK", "dV", "Pmean")
SEED, SITE, B_OFFSET = 0x51F0A2C3D4, 21, 3

# measured on the CPU (measure_attn over ATTN_CASES, every order of ATTN_ORDERS): the largest |yardstick - float64| / (v mag)
#   O 24.18      lse 12.51      dQ 7.34      dK 6.63      dV 32.22      Pmean 50.62
# all six at the packed hd = 128 case: O, lse, dV and the map grow with the head width (the roundings of S, about
# v sum|q||k| / sqrt(hd), move every probability; `mag` does not count them), dQ and dK hardly do.
# Rounded up here; test_fp32_bound_host.py::test_envelope_constants_cover_what_the_yardsticks_measure fails if they fall behind
ATTN_ENVELOPE = {"O": 28.0, "lse": 15.0, "dQ": 9.0, "dK": 8.0, "dV": 38.0, "Pmean": 56.0}
ATTN_FACTOR = {k: TILE_FACTOR * e for k, e in ATTN_ENVELOPE.items()}

# measured on the CPU (measure_ln32 over LN32_FWD_CASES + LN32_BWD_CASES, every order of ROW_ORDERS):
#   y 14.76 (2048 x 260)      ds (dS and dG) 3.69      xh (the xhat inside a term dy * xhat of dgamma, against xhat_mag) 3.56
# Rounded up; the same host test keeps them honest
LN32_ENVELOPE = {"y": 18.0, "ds": 5.0, "xh": 5.0}
LN32_FACTOR = {k: LN_MARGIN * e for k, e in LN32_ENVELOPE.items()}


# ================================================================================================ attention: the edges, as data
# (B, Lq, Lk, hd, mask pattern, p): padded launches.  Every Lk edge: `edges` at Lk = 130 (valid lengths 1, 15, 16, 17, 63, 64, 65,
# 127, 128, 129 and 130) with hd 16 and 64; every Lq of {1, 16, 17, 63, 64, 65, 129} with two head widths (the packed cases
# below add all of them once more as sequence lengths); every head width; both p
ATTN_PADDED = (
    (12, 17, 130, 16, "edges", 0.0), (12, 65, 130, 64, "edges", 0.1),
    (3, 129, 130, 32, "leading", 0.1), (3, 64, 130, 96, "leading", 0.0),
    (3, 1, 65, 128, "none", 0.0), (3, 63, 64, 128, "prefix", 0.1), (3, 129, 129, 16, "none", 0.1),
    (3, 16, 63, 96, "allpad", 0.0), (3, 16, 16, 64, "allpad", 0.1),
    (3, 1, 17, 32, "prefix", 0.1), (3, 17, 33, 128, "prefix", 0.0), (3, 63, 65, 32, "none", 0.0),
    (3, 64, 64, 16, "leading", 0.1), (3, 65, 15, 96, "prefix", 0.1),
)
# (hd, p): packed launches; the sequence lengths of q and of k are the `edges` lengths at 130 in two different orders, with one
# sample of length 0 in both in the middle of the batch
ATTN_PACKED = ((16, 0.1), (32, 0.0), (64, 0.0), (96, 0.1), (128, 0.1))
_EDGE130 = sorted(set(A.EDGE_LENGTHS) | {129, 130})
PACKED_LQ = tuple(_EDGE130[:6] + [0] + _EDGE130[6:])
PACKED_LK = tuple(list(reversed(_EDGE130))[:6] + [0] + list(reversed(_EDGE130))[6:])
PACKED_SURPLUS = 5           # rows behind cu[B] in every packed operand: NaN, never read, never written

ATTN_CASES = tuple(("padded",) + c for c in ATTN_PADDED) + tuple(("packed", len(PACKED_LQ), max(PACKED_LQ), max(PACKED_LK), hd, "lengths", p)
                                                                  for hd, p in ATTN_PACKED)


def attn_id(c):
    form, B, Lq, Lk, hd, mask, p = c
    return f"{form}-B{B}-{Lq}x{Lk}-hd{hd}-{mask}-p{p}"


def attn_case(c):
    """the operands of one table row.  q [B Lq, d], kv [B Lk, 2d], do [B Lq, d] fp32 in the PADDED layout (a packed launch gathers
    its rows from them: rows_q / rows_k); kpm [B, Lk] bool or None; keep [B, H, Lq, Lk] bool or None; ik the fp32 value of
    1 / (1 - p); lens_q / lens_k per sample; live: the samples with at least one valid key (the others are NaN by contract)."""
    form, B, Lq, Lk, hd, mask, p = c
    H, d = HEADS, HEADS * hd
    g = torch.Generator().manual_seed(7919 * hd + 131 * Lq + Lk + B)
    q = torch.randn(B * Lq, d, generator=g) * 1.5
    kv = torch.randn(B * Lk, 2 * d, generator=g)
    do = torch.randn(B * Lq, d, generator=g)
    if form == "packed":
        lens_q, lens_k = torch.tensor(PACKED_LQ), torch.tensor(PACKED_LK)
        kpm = torch.arange(Lk)[None] >= lens_k[:, None]
        vq = torch.arange(Lq)[None] < lens_q[:, None]
        do = do * vq.reshape(-1, 1)                       # rows that a packed launch does not have carry no gradient
    else:
        kpm = A.key_padding_mask(mask, B, Lk)
        lens_q = torch.full((B,), Lq)
        lens_k = torch.full((B,), Lk) if kpm is None else (~kpm).sum(1)
    keep = torch.from_numpy(hashrng.attn_mask(SEED, SITE, B, H, Lq, Lk, p, B_OFFSET)) if p > 0 else None
    live = torch.ones(B, dtype=torch.bool) if kpm is None else ~kpm.all(1)
    out = {"case": c, "B": B, "H": H, "Lq": Lq, "Lk": Lk, "hd": hd, "d": d, "p": p, "q": q, "kv": kv, "do": do, "kpm": kpm, "keep": keep,
           "ik": R.inv_keep32(p) if p > 0 else 1.0, "lens_q": lens_q, "lens_k": lens_k, "live": live, "packed": form == "packed"}
    if form == "packed":
        out["rows_q"] = (torch.arange(Lq)[None] < lens_q[:, None]).reshape(-1).nonzero().reshape(-1)
        out["rows_k"] = (~kpm).reshape(-1).nonzero().reshape(-1)
    return out


def _live4(c, dtype):
    """(q, k, v, dO [b, H, L, hd], kpm, keep) of the live samples in `dtype`"""
    B, H, Lq, Lk, hd, d, lv = c["B"], c["H"], c["Lq"], c["Lk"], c["hd"], c["d"], c["live"]
    q, k = A.heads(c["q"], B, Lq, H, hd)[lv].to(dtype), A.heads(c["kv"][:, :d], B, Lk, H, hd)[lv].to(dtype)
    v, do = A.heads(c["kv"][:, d:], B, Lk, H, hd)[lv].to(dtype), A.heads(c["do"], B, Lq, H, hd)[lv].to(dtype)
    return q, k, v, do, None if c["kpm"] is None else c["kpm"][lv], None if c["keep"] is None else c["keep"][lv]


def attn_ref(c):
    """(reference, magnitude) in float64 over the live samples: {O, dQ, dK, dV [b, H, L, hd], lse [b, H, Lq, 1], Pmean [b, 1, Lq, Lk]}"""
    q, k, v, do, kpm, keep = _live4(c, torch.float64)
    r = A.reference(q, k, v, do, kpm, keep, c["ik"])
    m = A.magnitude(q, k, v, do, kpm, keep, c["ik"])
    s = (q @ k.transpose(-1, -2)) / math.sqrt(c["hd"])
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float("-inf"))
    ref = {n: r[n] for n in A.OUTPUTS}
    ref["lse"], ref["Pmean"] = r["lse"][..., None], r["P"].mean(1)[:, None]
    mag = dict(m)
    mag["lse"], mag["Pmean"] = s.amax(-1).abs()[..., None] + 1.0, ref["Pmean"].clone()
    return ref, mag


def _shape6(out):
    out["lse"], out["Pmean"] = out["lse"][..., None], out["Pmean"][:, None]
    return out


def _chain4(a, b, init=None, rev=False):
    """a [.., M, K] @ b [.., K, N] the way a chain of v_mfma_f32_16x16x4_f32 forms it: four terms of the contraction per step,
    every step added to the running accumulator (`init`, or zero) in turn -- K / 4 sequential roundings where a blocked CPU GEMM
    has a handful.  rev: the steps in reverse."""
    K = a.shape[-1]
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:]) if init is None else init
    for k0 in (range(((K - 1) // 4) * 4, -1, -4) if rev else range(0, K, 4)):
        acc = acc + a[..., k0:k0 + 4] @ b[..., k0:k0 + 4, :]
    return acc


def _tiled32(q, k, v, do, kpm, keep, ik, rev, fault):
    B, H, Lq, hd = q.shape
    Lk = k.shape[2]
    scale = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt()
    ikt = torch.tensor(ik, dtype=torch.float32)
    ninf = torch.tensor(float("-inf"))
    s = _chain4(q * scale, k.transpose(-1, -2), rev=rev)
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float("-inf"))
    ktiles = list(range(0, Lk, 64))
    qtiles = list(range(0, Lq, 64))
    if rev:
        ktiles.reverse()
        qtiles.reverse()
    m, l, o = torch.full((B, H, Lq), float("-inf")), torch.zeros(B, H, Lq), torch.zeros(B, H, Lq, hd)
    m_prev = m
    for k0 in ktiles:
        st = s[..., k0:k0 + 64]
        mnew = torch.maximum(m, st.amax(-1))
        msafe = torch.where(mnew == ninf, torch.zeros(()), mnew)
        corr = torch.exp(m - msafe)
        e = torch.exp(st - msafe[..., None])
        l = l * corr + e.sum(-1)
        w = e if keep is None else torch.where(keep[..., k0:k0 + 64], e, torch.zeros(()))
        o = _chain4(w, v[:, :, k0:k0 + 64], o * corr[..., None], rev)
        m_prev, m = m, mnew
    O = o * ((ikt if keep is not None else torch.tensor(1.0)) / l)[..., None]
    lse = (m_prev if fault == "lse_stale_max" else m) + torch.log(l)
    p = torch.exp(s - lse[..., None]) if fault != "lse_stale_max" else torch.exp(s - (m + torch.log(l))[..., None])
    dp = _chain4(do, v.transpose(-1, -2), rev=rev)
    pd = p
    if keep is not None:
        dp = torch.where(keep, dp * ikt, torch.zeros(()))
        pd = torch.where(keep, p * ikt, torch.zeros(()))
    delta = (do * O).sum(-1)
    ds = p * (dp - delta[..., None])
    dq = torch.zeros_like(q)
    for k0 in ktiles:
        dq = _chain4(ds[..., k0:k0 + 64], k[:, :, k0:k0 + 64], dq, rev)
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for q0 in qtiles:
        dk = _chain4(ds[:, :, q0:q0 + 64].transpose(-1, -2), q[:, :, q0:q0 + 64], dk, rev)
        dv = _chain4(pd[:, :, q0:q0 + 64].transpose(-1, -2), do[:, :, q0:q0 + 64], dv, rev)
    return {"O": O, "lse": lse, "dQ": dq * scale, "dK": dk * scale, "dV": dv, "Pmean": pd.sum(1) * (1.0 / H)}


def attn_yard32(c, order="torch", hooks=None, fault=None):
    """the closed form in fp32 on the CPU over the live samples, same shapes as attn_ref.  order 'torch': attn_reference._run itself
    on float32 tensors (the dropout factors ride in through its Pd / dP hooks, so that nothing is promoted to float64), `hooks`
    are _run's (the mutants of test_fp32_bound_host.py).  'tiles' / 'tiles_rev': the kernels' online softmax over key tiles of 64
    and their tile-wise backward sums; fault 'lse_stale_max': lse without the running max of the last key tile."""
    q, k, v, do, kpm, keep = _live4(c, torch.float32)
    if order != "torch":
        assert hooks is None
        return _shape6(_tiled32(q, k, v, do, kpm, keep, c["ik"], order == "tiles_rev", fault))
    assert fault is None
    h = dict(hooks or {})
    if keep is not None:
        drop = keep.float() * torch.tensor(c["ik"], dtype=torch.float32)
        for n in ("Pd", "dP"):
            user = h.get(n)
            h[n] = (lambda x, user=user: x * drop) if user is None else (lambda x, user=user: user(x * drop))
    r = A._run(q, k, v, do, kpm, None, 1.0, lambda x: x, h)
    assert r["O"].dtype == torch.float32
    out = {n: r[n] for n in A.OUTPUTS}
    out["lse"], out["Pmean"] = r["lse"], r["P"].mean(1)
    return _shape6(out)


def attn_yards(c):
    return {o: attn_yard32(c, o) for o in ATTN_ORDERS}


def attn_ratios(got, ref, yards, mag, out):
    """(elementwise error / limit, per-tile error / limit) of ONE output, all [b, H or 1, L, n]; inf for a non-finite value or a
    non-zero where the magnitude is zero"""
    got = got.double()
    err = (got - ref).abs()
    if not torch.isfinite(err).all() or (err[mag == 0] > 0).any():
        return float("inf"), float("inf")
    lim = ATTN_FACTOR[out] * V * mag
    elem = float((err / lim.clamp(min=1e-300))[mag > 0].max()) if (mag > 0).any() else 0.0
    worst = torch.stack([A._tile_norms(y.double() - ref) for y in yards]).amax(0)
    pooled = max(float((y.double() - ref).norm() / mag.norm().clamp(min=1e-300)) for y in yards)
    tl = TILE_FACTOR * torch.maximum(worst, pooled * A._tile_norms(mag)) + V * A._tile_norms(mag)
    tile = float((A._tile_norms(got - ref) / tl.clamp(min=1e-300)).max())
    return elem, tile


def check_attn(got, ref, yards, mag, out, name):
    """got: ONE output [b, H or 1, L, n] of the live samples; yards: that output of every order.  Returns the two ratios (<= 1)."""
    assert got.shape == ref.shape, (name, out, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(ref).all() and torch.isfinite(mag).all() and all(torch.isfinite(y).all() for y in yards), (name, "reference is not finite")
    elem, tile = attn_ratios(got, ref, yards, mag, out)
    assert elem <= 1.0, f"{name} {out}: elementwise error is {elem:.3g} x its limit {ATTN_FACTOR[out]:g} v mag (or a zero-magnitude element is not 0)"
    assert tile <= 1.0, f"{name} {out}: per-tile error is {tile:.3g} x its limit 3 max(|yard - ref|, r |mag|) + v |mag|"
    return elem, tile


def check_attn_all(got, c, name, ref=None, mag=None, yards=None, outputs=ATTN_OUTPUTS, valid_q=None):
    """valid_q [b, Lq] bool: query rows that exist (a packed launch has no others); reference, yardsticks and magnitudes of O, lse, dQ
    and the map are zeroed elsewhere, so `got` must hold exact zeros there"""
    if ref is None:
        ref, mag = attn_ref(c)
    yards = attn_yards(c) if yards is None else yards
    out = {}
    for o in outputs:
        r, m, ys = ref[o], mag[o], [y[o] for y in yards.values()]
        if valid_q is not None and o not in ("dK", "dV"):
            w = valid_q[:, None, :, None]
            r, m, ys = r * w, m * w, [torch.where(w, y, torch.zeros(())) for y in ys]
        out[o] = check_attn(got[o], r, ys, m, o, name)
    return out


def delta_ref(c):
    """(delta = rowsum(dO * O), its magnitude E_delta = rowsum(M_O |dO|)) [b, H, Lq] in float64.  The kernel sums hd fp32 products of
    ITS O: F = hd (products and additions) + ATTN_FACTOR['O'] (O's own error, <= that many v M_O per element)"""
    q, k, v, do, kpm, keep = _live4(c, torch.float64)
    o = A.reference(q, k, v, do, kpm, keep, c["ik"])["O"]
    m_o = A.magnitude(q, k, v, do, kpm, keep, c["ik"])["O"]
    return (o * do).sum(-1), (m_o * do.abs()).sum(-1)


def delta_factor(hd):
    return hd + ATTN_FACTOR["O"]


def measure_attn(cases=ATTN_CASES, orders=ATTN_ORDERS):
    env = {o: 0.0 for o in ATTN_OUTPUTS}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for c in cases:
            case = attn_case(c)
            ref, mag = attn_ref(case)
            for o in orders:
                y = attn_yard32(case, o)
                for n in ATTN_OUTPUTS:
                    env[n] = max(env[n], R.ratio_v(y[n], ref[n], mag[n]))
    finally:
        torch.set_num_threads(threads)
    return env


# ================================================================================================ LayerNorm, fp32 in and out
LN32_WIDTHS = (4, 252, 256, 260, 1020, 1024, 1028, 2048, 4092, 4096)     # one lane; lane 63 | next chunk; NV4 4 | 16; the maximum
LN32_BWD_WIDTHS = (4, 252, 256, 260, 1020, 1024)
LN32_ROWS = (1, 3, 4, 5)
LN32_BWD_ROWS = (1, 3, 4, 5, 2047, 2048, 2049, 2053)                      # 512 blocks x 4 waves = 2048 rows per trip of the row loop
ROW_INDEX_BASE = (9, 2, 30, 2, 17)                                        # non-monotone, one row twice

# (M, d, family, p, residual, row_offset, rows entry, Y16 given)
LN32_FWD_CASES = tuple(
    [(LN32_ROWS[i % 4], d, "unit", (0.0, 0.25)[i % 2], ("x32", "none", "x32")[i % 3], (0, 1000)[i % 2], i % 3 == 1, i % 2 == 0)
     for i, d in enumerate(LN32_WIDTHS)]
    + [(M, 260, "unit", 0.25, "x32", 77, M == 5, M != 3) for M in LN32_ROWS]
    + [(5, 260, "offset", 0.25, "x32", 1 << 20, False, True), (4, 4096, "offset", 0.0, "x32", 0, True, False),
       (3, 1028, "const", 0.0, "x32", 0, False, True), (5, 4, "const", 0.0, "none", 0, True, False), (1, 1024, "offset", 0.25, "x32", 5, True, True)])
# (M, d, family, p, residual, row_offset, rows entry, dbias given, accumulate)
LN32_BWD_CASES = tuple(
    [(LN32_ROWS[i % 4], d, "unit", (0.25, 0.0)[i % 2], ("x32", "none")[i % 2], (1000, 0)[i % 2], i % 3 == 0, i % 2 == 0, i % 3 == 1)
     for i, d in enumerate(LN32_BWD_WIDTHS)]
    + [(M, 260, "unit", (0.0, 0.25)[i % 2], "x32", (0, 77)[i % 2], i % 4 == 3, i % 3 != 0, i % 2 == 1) for i, M in enumerate(LN32_BWD_ROWS)]
    + [(5, 1024, "offset", 0.25, "x32", 9, False, True, True), (4, 256, "const", 0.0, "x32", 0, True, True, False),
       (2049, 4, "unit", 0.25, "none", 3, False, False, True)])


def ln32_id(c):
    return "-".join(str(x) for x in c)


def row_index_of(M):
    return np.asarray([ROW_INDEX_BASE[i % 5] + 40 * (i // 5) for i in range(M)], dtype=np.int64)


def ln32_case(c):
    """rowops_reference.ln_case with fp32 operands: G and dY carry all 24 bits (the bf16 values times 1 + 2^-9 randn; the `const`
    family stays dyadic so that its variance is exactly 0)"""
    M, d, fam, p, resid, roff, rows = c[:7]
    case = R.ln_case(M, d, fam, p, resid, roff, row_index_of(M) if rows else None, seed=SEED, site=SITE)
    g = torch.Generator().manual_seed(13 * d + M)
    jit = lambda x: x.float() * (1 + 2.0 ** -9 * torch.randn(x.shape, generator=g))
    case["G"] = jit(case["G"]) if fam != "const" else case["G"].float()
    case["dY"] = jit(case["dY"])
    return case


def ln32_refs(case, init=None):
    """float64: (ln_fwd_ref, ln_bwd_ref) -- the backward from the EXACT row statistics, which the fp32 kernels recompute"""
    f = R.ln_fwd_ref(case)
    b = R.ln_bwd_ref(case, f["mean"], f["rstd"], init)
    b["mag_dgamma"] = (case["dY"].double().abs() * xhat_mag(f)).sum(0) + (0.0 if init is None else init["dgamma"].double().abs())
    return f, b


def xhat_mag(f):
    """what v moves xhat = (s - mean) rstd by when the statistics are computed in fp32 too: (|s| + |mean| + mean|s|) rstd -- the
    error of the row mean scales with mean|s|, not with the element's own |s|"""
    return (f["s"].abs() + (f["mean"].abs() + f["sabs"])[:, None]) * f["rstd"][:, None]


def ln32_yards(case, orders=R.ROW_ORDERS, cols=False, **kw):
    """{order: (fwd32, bwd32 from that order's own fp32 statistics)}"""
    out = {}
    for i, o in enumerate(orders):
        fw = R.fwd32(case, o)
        out[o] = (fw, R.bwd32(case, fw["mean"], fw["rstd"], o, R.COL_ORDERS[i % 3] if cols else None, **kw))
    return out


def ln32_sum_factor(name, M, accumulate=False):
    """F of dgamma / dbeta / dbias over M rows: M - 1 additions of fp32 terms; dbeta's terms are inputs; a term dy * xhat of dgamma
    carries xhat's error and the product's rounding; a term of dbias carries dS's"""
    return M + {"dbeta": 0.0, "dgamma": LN32_FACTOR["xh"] + 1, "dbias": LN32_FACTOR["ds"]}[name] + (1 if accumulate else 0)


def check_ln32_fwd(y32, y16, ref, name):
    r = {"y32": R.check_elem(y32, ref["y"], ref["mag_y"], LN32_FACTOR["y"], True, name + " y32")}
    if y16 is not None:
        assert torch.equal(y16.view(torch.int16), y32.bfloat16().view(torch.int16)), f"{name}: Y16 is not bf16(Y32) bit for bit"
    return r


def check_ln32_bwd(got, case, ref, name, accumulate=False):
    """got: {dS, dG or None, dgamma, dbeta, dbias or None} fp32; ref: ln32_refs()[1] with init folded in"""
    M = case["G"].shape[0]
    r = {"dS": R.check_elem(got["dS"], ref["dS"], ref["mag_dS"], LN32_FACTOR["ds"], True, name + " dS")}
    if got.get("dG") is not None:
        r["dG"] = R.check_elem(got["dG"], ref["dG"], ref["mag_dG"], LN32_FACTOR["ds"], True, name + " dG")
    for n in ("dgamma", "dbeta", "dbias"):
        if got.get(n) is not None:
            r[n] = R.check_elem(got[n], ref[n], ref["mag_" + n], ln32_sum_factor(n, M, accumulate), True, f"{name} {n}")
    return r


def measure_ln32(cases=None, orders=R.ROW_ORDERS):
    env = {"y": 0.0, "ds": 0.0, "xh": 0.0}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for c in (LN32_FWD_CASES + LN32_BWD_CASES if cases is None else cases):
            case = ln32_case(c)
            f, b = ln32_refs(case)
            s64 = R._resid(case, torch.float64) + case["keep"].double() * case["ik"] * case["G"].double()
            xh64 = (s64 - f["mean"][:, None]) * f["rstd"][:, None]
            xh_mag = xhat_mag(f)
            for o, (fw, bw) in ln32_yards(case, orders).items():
                xh32 = (R._s32(case) - fw["mean"][:, None]) * fw["rstd"][:, None]
                env["y"] = max(env["y"], R.ratio_v(fw["y32"], f["y"], f["mag_y"]))
                env["ds"] = max(env["ds"], R.ratio_v(bw["dS32"], b["dS"], b["mag_dS"]), R.ratio_v(bw["dG32"], b["dG"], b["mag_dG"]))
                env["xh"] = max(env["xh"], R.ratio_v(xh32, xh64, xh_mag))
    finally:
        torch.set_num_threads(threads)
    return env


# ================================================================================================ operand splits
SPLIT_K = (4, 12, 264)
SPLIT_M = (1, 5)
SPLIT_SECOND_TRIP = (2052, 4096)       # M K / 4 = 2 101 248 > 8192 * 256 = 2 097 152 vectors: the grid-stride loop's second trip
GRID_CAP_VECTORS = 8192 * 256
SPLIT_IDENTITY_MIN = 2.0 ** -100       # hi + mid + lo == x is asserted for |x| >= this (and x == 0): below, lo falls under bf16's subnormals


def split_inputs(M, K, seed=0):
    """fp32 [M, K]: +-0, subnormals (bf16-representable and not), values whose hi rounds UP (mid < 0), 1e-30 .. 1e30, and randn"""
    g = torch.Generator().manual_seed(100 * K + M + seed)
    x = torch.randn(M, K, generator=g) * torch.pow(10.0, torch.randint(-30, 31, (M, K), generator=g).float())
    special = torch.tensor([0.0, -0.0, 2.0 ** -130, -2.0 ** -140, 2.0 ** -149, 1.0 + 2.0 ** -8 + 2.0 ** -9, -(3.0 + 2.0 ** -6 + 2.0 ** -20), 1.00390625 * 1e30,
                            -1e-30, 1e30, 255.99, 2.0 ** -126, 1.0 + 2.0 ** -23, -(2.0 - 2.0 ** -23), 0.1, 65504.0])
    flat = x.reshape(-1)
    n = min(flat.numel(), special.numel())
    idx = torch.randperm(flat.numel(), generator=g)[:n]
    flat[idx] = special[:n]
    return flat.reshape(M, K)


def split_host(x, relu=False, mask=None, fault=None):
    """(t, hi, mid, lo): t = x * (mask > 0), clamped at 0 under relu; hi = bf16(t), mid = bf16(t - hi), lo = bf16(t - hi - mid), each
    by torch's round-to-nearest-even.  fault: 'mid_from_unrounded_hi' (the remainder taken against the truncated hi, not the
    stored one) | 'lo_dropped'"""
    t = x.float().clone()
    if mask is not None:
        t = torch.where(mask > 0, t, torch.zeros(()))
    if relu:
        t = torch.where(t > 0, t, torch.zeros(()))
    hi = t.bfloat16()
    r1 = t - (R.bf16_trunc(t).float() if fault == "mid_from_unrounded_hi" else hi.float())
    mid = r1.bfloat16()
    lo = (r1 - mid.float()).bfloat16()
    if fault == "lo_dropped":
        lo = torch.zeros_like(lo)
    return t, hi, mid, lo


def split_layout(form, hi, mid, lo):
    """the expected Y of split3g_kernel: forms 0 / 1 [hi | mid | hi], [hi | hi | mid] side by side, 2 / 3 the same stacked; forms
    4 / 5 [hi | mid | lo | hi | mid | hi], [hi | hi | hi | mid | mid | lo], 6 / 7 the same stacked (the kernel's comment)"""
    w = form & 1
    if form >= 4:
        blocks = [hi, hi, hi, mid, mid, lo] if w else [hi, mid, lo, hi, mid, hi]
    else:
        blocks = [hi, hi, mid] if w else [hi, mid, hi]
    return torch.cat(blocks, 1 if form in (0, 1, 4, 5) else 0)


def split_blocks(form, Y, M, K):
    """the six (three) blocks of a Y in the layout of `form`, in storage order"""
    n = 6 if form >= 4 else 3
    if form in (0, 1, 4, 5):
        return [Y[:, j * K:(j + 1) * K] for j in range(n)]
    return [Y[j * M:(j + 1) * M] for j in range(n)]


def split_sum_exact(form, Y, t):
    """forms 4 - 7: number of elements with |t| >= SPLIT_IDENTITY_MIN (or t == 0) where hi + mid + lo != t"""
    M, K = t.shape
    b = split_blocks(form, Y, M, K)
    hi, mid, lo = (b[0], b[3], b[5]) if form & 1 else (b[0], b[1], b[2])
    total = hi.double() + mid.double() + lo.double()
    held = (t.abs() >= SPLIT_IDENTITY_MIN) | (t == 0)
    return int(((total != t.double()) & held).sum())


# ================================================================================================ sums and small kernels
COLSUM_M = (1, 3, 4, 5, 63, 64, 65, 4095, 4097)
COLSUM_N = (1, 255, 256, 257)
ROWDOT_M, ROWDOT_D = (1, 7), (255, 256, 257)
DROPOUT_SECOND_TRIP = (2052, 4096)
GATE_WIDTHS = (4, 252, 256, 260)
DPRE_LENGTHS = (1, 2, 3, 70)
MEAN_LENGTHS = (1, 2, 33)
FUSE_SECOND_TRIP = (2, 1027, 4096)     # B, L, d: B L d / 4 = 2 103 296 > 8192 * 256


def far_init(n, g):
    """a non-zero destination of an accumulating call, 50 <= |x| < 100: the n v mag limit of a sum over thousands of rows is a
    few tenths, so a destination of order 1 that a kernel forgot to add could pass it"""
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0) * (50.0 + 50.0 * torch.rand(n, generator=g))


def colsum_slices(M):
    """(slices, rows_per) of hriemo_colsum_f32"""
    s = min((M + 63) // 64, 64)
    per = (M + s - 1) // s
    return (M + per - 1) // per, per


def colsum32(X, mask=None, init=None, accumulate=False, fault=None):
    """the kernel's order in fp32: per slice four accumulators over rows r, r + 1, r + 2, r + 3 and a tail into the first (one
    accumulator under a mask), the slices in turn.  fault: 'drop_tail' (the rows past the last whole group of four of a slice) |
    'ignore_accumulate'"""
    M, N = X.shape
    t = X.float() if mask is None else torch.where(mask > 0, X.float(), torch.zeros(()))
    slices, per = colsum_slices(M)
    total = torch.zeros(N)
    for sl in range(slices):
        r0, r1 = sl * per, min(M, (sl + 1) * per)
        s = [torch.zeros(N) for _ in range(4)]
        r = r0
        if mask is None:
            while r + 4 <= r1:
                for a in range(4):
                    s[a] = s[a] + t[r + a]
                r += 4
        if not (fault == "drop_tail" and mask is None):
            while r < r1:
                s[0] = s[0] + t[r]
                r += 1
        total = total + ((s[0] + s[1]) + (s[2] + s[3]))
    if accumulate and fault != "ignore_accumulate":
        total = init.float() + total
    return total


def dropout_host(X, relu, gate, p, seed, site, row_off):
    """hriemo_dropout_f32 exactly: max(x, 0) under relu, times (gate > 0), then keep ? x * fl32(1 / (1 - p)) : +0"""
    t = X.float()
    if relu:
        t = torch.where(t > 0, t, torch.zeros(()))
    if gate is not None:
        t = torch.where(gate > 0, t, torch.zeros(()))
    if p > 0:
        keep = torch.from_numpy(hashrng.rows_mask(seed, site, X.shape[0], X.shape[1], p, row_off))
        t = torch.where(keep, t * torch.tensor(R.inv_keep32(p), dtype=torch.float32), torch.zeros(()))
    return t


# ------------------------------------------------------------------------------------------------ padded fp32 gate pieces
def gate_mask(kind, B, L, seed=0):
    """[B, L] bool (True = PAD) or None: none | prefix | scattered | full (sample 0 all PAD, the others scattered)"""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(17 * L + B + seed)
    if kind == "prefix":
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[-1] = L
        return torch.arange(L)[None] >= lens[:, None]
    m = torch.rand(B, L, generator=g) < 0.4
    m[:, 0] = False
    if kind == "full":
        m[0] = True
    else:
        assert kind == "scattered"
    return m


def masked_mean32_ref(X, m):
    """(mean over valid rows or 0, magnitude, n valid) float64; X [B, L, d] fp32"""
    v = torch.ones(X.shape[:2], dtype=torch.float64) if m is None else (~m).double()
    n = v.sum(1)
    den = n.clamp(min=1)[:, None]
    return (X.double() * v[..., None]).sum(1) / den, (X.double().abs() * v[..., None]).sum(1) / den, n


def fuse32_ref(w, Aa, T, L):
    w, a, t = w.double()[:, None], Aa.double()[:, :L], T.double()[:, :L]
    return w * a + (1 - w) * t, w.abs() * a.abs() + (1 - w).abs() * t.abs()


def gate_dpre32_ref(dH, Aa, T, w, dbeta, L):
    """dpre = (sum_l dH (A - T) + dbeta / d) w (1 - w) and its magnitude; F = L terms, each a rounded difference and product (+ 2),
    dbeta / d and its addition (+ 2), 1 - w and two products (+ 3)"""
    d = w.shape[1]
    g, a, t, w = dH.double(), Aa.double()[:, :L], T.double()[:, :L], w.double()
    s, ms = (g * (a - t)).sum(1), (g.abs() * (a.abs() + t.abs())).sum(1)
    if dbeta is not None:
        s, ms = s + dbeta.double()[:, None] / d, ms + dbeta.double().abs()[:, None] / d
    return s * w * (1 - w), ms * w * (1 - w)


def dpre32_factor(L, has_dbeta):
    return L + 2 + (2 if has_dbeta else 0) + 3


def gate_in_bwd32_ref(dgin, a, t):
    d = a.shape[1]
    a, t, g = a.double(), t.double(), dgin.double()
    g0, g1, g2, g3 = (g[:, q * d:(q + 1) * d] for q in range(4))
    sg = torch.sign(a - t)
    return {"da": g0 + sg * g2 + t * g3, "mag_da": g0.abs() + sg.abs() * g2.abs() + (t * g3).abs(),
            "dt": g1 - sg * g2 + a * g3, "mag_dt": g1.abs() + sg.abs() * g2.abs() + (a * g3).abs()}


def gate_dy32_ref(dH, w, is_a, dpool, m, L, Lx):
    """dY [B, Lx, d] = (l < L ? wsel dH : 0) + (valid ? dpool / max(#valid, 1) : 0), its magnitude; 4 roundings: 1 - w, 1 / n, two
    products, one sum"""
    B, d = w.shape
    v = torch.ones(B, Lx, dtype=torch.float64) if m is None else (~m).double()
    inv = v / v.sum(1, keepdim=True).clamp(min=1)
    ws = (w if is_a else 1 - w).double()[:, None]
    y = dpool.double()[:, None] * inv[..., None]
    mag = y.abs()
    y[:, :L] += ws * dH.double()
    mag[:, :L] += ws.abs() * dH.double().abs()
    return y, mag


DY_ROUNDINGS = 5             # 1 / n, its product with dpool, 1 - w, its product with dH, the sum
# w = 1 / (1 + expf(-pre)) with the library's accurate expf: the exponential within 3 ulp = 6 v of itself (the OpenCL bound the
# device library documents), the sum and the quotient one rounding each; every factor of it scales w by at most itself
SIGMOID32_FACTOR = 8.0
FUSE_ROUNDINGS = G.FUSE_ROUNDINGS
GIN_BWD_ROUNDINGS = 4        # t g3, sg g2 (exact), two additions, one spare for a contraction's different rounding point


# ================================================================================================ which test holds which entry
_ATT, _ROW = "test_gpu_fp32_attention_kernels.py", "test_gpu_fp32_row_kernels.py"


def coverage():
    """{exported entry point: [test ids that hold it to the limits of this module (or, for entries outside fp32mode.hip and the packed
    gate twins, the existing test that does)]}"""
    att = [f"{_ATT}::test_attention_f32_padded", f"{_ATT}::test_attention_f32_refusals"]
    pk = [f"{_ATT}::test_attention_f32_packed", f"{_ATT}::test_attention_f32_refusals"]
    twin = ["test_gpu_fp32_packed_tail.py::test_packed_f32_gate_kernels_equal_padded_bit_for_bit_and_float64"]
    return {
        "hriemo_attn_fwd_f32": att + [f"{_ATT}::test_attention_f32_device_seed_word"], "hriemo_attn_bwd_f32": att, "hriemo_attn_probs_f32": att,
        "hriemo_attn_fwd_f32_varlen": pk, "hriemo_attn_bwd_f32_varlen": pk, "hriemo_attn_probs_f32_varlen": pk,
        "hriemo_split3_f32": [f"{_ROW}::test_split3_f32_forms", f"{_ROW}::test_split_second_trip", f"{_ROW}::test_row_kernel_refusals"],
        "hriemo_split_bf16x3": [f"{_ROW}::test_split_bf16x3_layouts"],
        "hriemo_dropout_f32": [f"{_ROW}::test_dropout_f32_exact", f"{_ROW}::test_dropout_f32_second_trip"],
        "hriemo_colsum_f32": [f"{_ROW}::test_colsum_f32"], "hriemo_colsum_f32_workspace_bytes": [f"{_ROW}::test_colsum_f32"],
        "hriemo_add_ln_f32": [f"{_ROW}::test_add_ln_f32_forward", f"{_ROW}::test_row_kernel_refusals"],
        "hriemo_add_ln_f32_rows": [f"{_ROW}::test_add_ln_f32_forward"],
        "hriemo_add_ln_bwd_f32": [f"{_ROW}::test_add_ln_f32_backward", f"{_ROW}::test_row_kernel_refusals"],
        "hriemo_add_ln_bwd_f32_rows": [f"{_ROW}::test_add_ln_f32_backward"],
        "hriemo_add_ln_bwd_f32_workspace_bytes": [f"{_ROW}::test_add_ln_f32_backward"],
        "hriemo_masked_mean_f32": [f"{_ROW}::test_masked_mean_f32"], "hriemo_gate_input_f32": [f"{_ROW}::test_gate_input_f32_and_backward"],
        "hriemo_gate_input_bwd_f32": [f"{_ROW}::test_gate_input_f32_and_backward"], "hriemo_sigmoid_beta_f32": [f"{_ROW}::test_sigmoid_beta_f32"],
        "hriemo_fuse_f32": [f"{_ROW}::test_fuse_f32"], "hriemo_gate_dpre_f32": [f"{_ROW}::test_gate_dpre_f32"],
        "hriemo_gate_dy_f32": [f"{_ROW}::test_gate_dy_f32"], "hriemo_rowdot_bwd_f32": [f"{_ROW}::test_rowdot_bwd_f32"],
        "hriemo_masked_mean_f32_packed": twin, "hriemo_fuse_f32_packed": twin, "hriemo_gate_dpre_f32_packed": twin, "hriemo_gate_dy_f32_packed": twin,
        # exported by other kernel files, named here because the header's fp32 pattern matches them
        "hriemo_cast_f32_to_bf16": ["test_gpu_kernels.py"], "hriemo_cast_bf16_to_f32": ["test_gpu_kernels.py"],
        "hriemo_cast_f32_to_bf16_batch": ["test_gpu_kernels.py"], "hriemo_rowsum_f32": ["test_gpu_gate_variants.py"],
        "hriemo_sumsq_f32": ["test_gpu_optimizer.py"],
    }


def header_fp32_exports(text):
    """every hriemo_*_f32* / hriemo_split* name declared in include/hriemo.h"""
    return sorted(set(re.findall(r"\b(hriemo_(?:\w*_f32\w*|split\w*))\s*\(", text)))
