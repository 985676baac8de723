"""Host-side references for the attention kernels (hri-emo_amd/csrc/attention.hip): no GPU, float64 throughout.

Three computations of the same closed-form forward + backward, all on [B, H, L, hd] float64 tensors made from the bf16
inputs (kpm [B, L_k] bool, True = PAD, or None; keep [B, H, L_q, L_k] bool dropout keep-mask or None; inv_keep = 1/(1-p)):

    S = scale * Q K^T (PAD keys -> -inf)       P = softmax(S)          Pd = P * keep * inv_keep
    O = Pd V                                   lse = logsumexp(S)
    dP = (dO V^T) * keep * inv_keep            delta = rowsum(O * dO)  dS = P * (dP - delta)
    dQ = scale * dS K                          dK = scale * dS^T Q     dV = Pd^T dO

reference()  exact float64.
yardstick()  float64 with a bf16 rounding at the kernels' rounding points and nowhere else:
               Pd -> bf16 before Pd V          attn_fwd_kernel `pf[qs][j] = (bf16_t)s[..]` (the unnormalised exp2, same relative
                                               rounding; 1/l and 1/(1-p) are applied to O afterwards)
               Pd -> bf16 before Pd^T dO       attn_bwd_dkv_hash_kernel / attn_bwd_dkv_kernel `pf[kw][..] = (bf16_t)pd`,
                                               attn_bwd_qres_kernel `pw[r] = (bf16_t)pd`
               O -> bf16                       attn_fwd_kernel `w[r] = (bf16_t)(o[qs][dt][r] * inv)`
               delta = rowsum(O_bf16 * dO)     attn_bwd_dq_kernel `part += (float)dof[..][j] * (float)ov[j]` (fp32 sum, not rounded;
                                               the single-pass kernels compute the same sum from the stored O)
               dS -> bf16 before dS K, dS^T Q  attn_bwd_dq_kernel `dsf[qs][j] = (bf16_t)s[..]`, the dK/dV kernels
                                               `dsf[kw][..] = (bf16_t)dsv`, attn_bwd_qres_kernel `dw[r] = (bf16_t)dsv`
               dQ, dK, dV -> bf16              the `w[r] = (bf16_t)v` / `wk[r]` / `wv[r]` stores
             P inside dS is NOT rounded (the backward recomputes it in fp32 from lse), nor are S, lse, dP.
magnitude()  the same products with absolute values: what one unit roundoff of an operand can move each output by.
               M_O = |Pd| |V|     M_dV = |Pd|^T |dO|     E_delta = rowsum(M_O * |dO|)
               W = P * (|dP| + |delta| + E_delta)        M_dQ = scale * W |K|     M_dK = scale * W^T |Q|

check() turns the three into two limits that come from the reference alone (see its docstring).  bf16 roundings of float64
values go through float32 first (torch has no direct conversion); the double rounding moves a result by < 2^-24 relative."""
import math

import torch

U = 2.0 ** -8           # bf16 unit roundoff (8 significant bits, round to nearest)
ELEM_FACTOR = 4.0       # elementwise: |got - ref| <= 4u * M
TILE_FACTOR = 3.0       # per 64-row tile: ||got - ref|| <= 3 * ||yard - ref|| + 2^-16 * ||M||   (GRAD_FACTOR of test_gpu_parity.py)
TILE_FP32 = 2.0 ** -16  # fp32 accumulation allowance: n * 2^-24 * sum|a||b| with n <= 256 effective terms
TILE_ROWS = 64
OUTPUTS = ("O", "dQ", "dK", "dV")


def bf16_round(x):
    return x.float().bfloat16().double()


def heads(x2d, B, L, H, hd):
    """[B*L, H*hd] (any float dtype, any row stride) -> [B, H, L, hd] float64"""
    return x2d.double().reshape(B, L, H, hd).transpose(1, 2).contiguous()


def rows(x4d):
    """[B, H, L, hd] -> [B*L, H*hd]"""
    B, H, L, hd = x4d.shape
    return x4d.transpose(1, 2).reshape(B * L, H * hd)


def _run(q, k, v, dO, kpm, keep, inv_keep, rnd, hooks=None):
    """the closed form above; rnd(x) is applied at the kernels' rounding points (identity: the exact reference).  hooks: optional
    {"scale": factor, "P" / "Pd" / "dP" / "delta" / "dS": fn(tensor) -> tensor} -- the host test plants its mutants there."""
    hooks = hooks or {}
    hook = lambda name, x: hooks[name](x) if name in hooks else x
    scale = hooks.get("scale", 1.0) / math.sqrt(q.shape[-1])
    s = (q @ k.transpose(-1, -2)) * scale
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = hook("P", torch.exp(s - lse[..., None]))                # all keys PAD: lse = -inf, -inf - -inf = NaN like softmax
    drop = None if keep is None else keep.double() * inv_keep
    pd = hook("Pd", p if drop is None else p * drop)
    pd_r = rnd(pd)
    o = rnd(pd_r @ v)
    delta = hook("delta", (o * dO).sum(-1))
    dp = dO @ v.transpose(-1, -2)
    dp = hook("dP", dp if drop is None else dp * drop)
    ds_r = rnd(hook("dS", p * (dp - delta[..., None])))
    return {"O": o, "lse": lse, "P": pd, "softmax": p, "dQ": rnd((ds_r @ k) * scale), "dK": rnd((ds_r.transpose(-1, -2) @ q) * scale),
            "dV": rnd(pd_r.transpose(-1, -2) @ dO)}


def reference(q, k, v, dO, kpm=None, keep=None, inv_keep=1.0):
    return _run(q, k, v, dO, kpm, keep, inv_keep, lambda x: x)


def yardstick(q, k, v, dO, kpm=None, keep=None, inv_keep=1.0, hooks=None):
    return _run(q, k, v, dO, kpm, keep, inv_keep, bf16_round, hooks)


def magnitude(q, k, v, dO, kpm=None, keep=None, inv_keep=1.0):
    ref = reference(q, k, v, dO, kpm, keep, inv_keep)
    scale = 1.0 / math.sqrt(q.shape[-1])
    drop = None if keep is None else keep.double() * inv_keep
    pd, p = ref["P"], ref["softmax"]                            # >= 0 already
    m_o = pd @ v.abs()
    e_delta = (m_o * dO.abs()).sum(-1)
    dp = dO @ v.transpose(-1, -2)
    dp = dp if drop is None else dp * drop
    delta = (ref["O"] * dO).sum(-1)
    w = p * (dp.abs() + (delta.abs() + e_delta)[..., None])
    return {"O": m_o, "dQ": (w @ k.abs()) * scale, "dK": (w.transpose(-1, -2) @ q.abs()) * scale,
            "dV": pd.transpose(-1, -2) @ dO.abs()}


def _tile_norms(x):
    """[B, H, L, hd] -> L2 norm of every (batch, head, 64-row block): [B, H, ceil(L/64)]"""
    B, H, L, hd = x.shape
    nt = (L + TILE_ROWS - 1) // TILE_ROWS
    pad = torch.zeros(B, H, nt * TILE_ROWS, hd, dtype=x.dtype)
    pad[:, :, :L] = x
    return pad.reshape(B, H, nt, TILE_ROWS * hd).norm(dim=-1)


def ratios(got, ref, yard, mag):
    """(worst elementwise error / its limit, worst per-tile error / its limit); a NaN or inf in `got` yields inf"""
    got = got.double()
    err = (got - ref).abs()
    if not torch.isfinite(err).all():
        return float("inf"), float("inf")
    elem = (err / (ELEM_FACTOR * U * mag + 1e-30)).max().item()
    lim = TILE_FACTOR * _tile_norms(yard - ref) + TILE_FP32 * _tile_norms(mag)
    tile = (_tile_norms(got - ref) / (lim + 1e-30)).max().item()
    return elem, tile


def check(got, ref, yard, mag, name):
    """got / ref / yard / mag: [B, H, L, hd] of ONE output.  With u = 2^-8:
      elementwise  |got - ref| <= 4u * M + 1e-30.  2u * M is the first-order bound of the rounding points listed above (one
                   rounding of an operand, one of the result; E_delta carries O's error into delta); the factor 2 on top covers
                   what the yardstick does not model (fp32 accumulation order, lazy rescaling, v_exp_f32).  M == 0 (dK / dV
                   rows of PAD keys) demands exact zeros.
      per tile     for every (batch, head, 64-row block): ||got - ref|| <= 3 * ||yard - ref|| + 2^-16 * ||M||.  The second term
                   matters only where the float64 yardstick is exact by cancellation and fp32 is not (one valid key: P = 1,
                   dP = delta, dS = 0 exactly, but the GPU sums dP and delta in different orders).
    Returns the two ratios (error / limit) after asserting both are <= 1."""
    assert torch.isfinite(ref).all() and torch.isfinite(yard).all() and torch.isfinite(mag).all(), (name, "reference is not finite")
    elem, tile = ratios(got, ref, yard, mag)
    assert elem <= 1.0, f"{name}: elementwise error is {elem:.3g} x its limit 4u*M"
    assert tile <= 1.0, f"{name}: per-tile error is {tile:.3g} x its limit 3*|yard-ref| + 2^-16*|M|"
    return elem, tile


def all_three(q, k, v, dO, kpm=None, keep=None, inv_keep=1.0, chunk_elems=6_000_000):
    """(reference, yardstick, magnitude) computed a few samples at a time, so that the [b, H, L_q, L_k] float64 temporaries stay
    small.  The dicts hold O, dQ, dK, dV [B, H, L, hd], lse [B, H, L_q] and (reference only) Pmean = head mean of Pd [B, L_q, L_k]."""
    B, H, Lq, _ = q.shape
    Lk = k.shape[2]
    step = max(1, chunk_elems // (H * Lq * Lk))
    outs = ({}, {}, {})
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        args = (q[sl], k[sl], v[sl], dO[sl], None if kpm is None else kpm[sl], None if keep is None else keep[sl], inv_keep)
        ref = reference(*args)
        ref["Pmean"] = ref["P"].mean(1)
        for out, res, names in ((outs[0], ref, OUTPUTS + ("lse", "Pmean")), (outs[1], yardstick(*args), OUTPUTS),
                                (outs[2], magnitude(*args), OUTPUTS)):
            for n in names:
                out.setdefault(n, []).append(res[n])
    return tuple({n: torch.cat(parts) for n, parts in out.items()} for out in outs)


EDGE_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)


def key_padding_mask(pattern, B, Lk):
    """[B, L_k] bool (True = PAD) or None.  Every length is assigned explicitly, sample b takes entry b % n of the pattern's list:
      none     no mask
      prefix   valid lengths L_k - L_k // 3, L_k // 2 + 1, L_k
      edges    valid lengths {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, L_k - 1, L_k} within [1, L_k]   (B >= their number)
      leading  keys 0..63 PAD (0..L_k//2-1 when L_k <= 64) / only the LAST key valid / every second key PAD   (B >= 3)
      allpad   sample 1 has every key PAD, the others are `prefix`   (B >= 2)"""
    if pattern == "none":
        return None
    kpm = torch.zeros(B, Lk, dtype=torch.bool)
    ar = torch.arange(Lk)
    if pattern in ("prefix", "allpad"):
        lens = (Lk - Lk // 3, Lk // 2 + 1, Lk)
        for b in range(B):
            kpm[b] = ar >= lens[b % 3]
        if pattern == "allpad":
            assert B >= 2
            kpm[1] = True
    elif pattern == "edges":
        lens = sorted({n for n in EDGE_LENGTHS + (Lk - 1, Lk) if 1 <= n <= Lk})
        assert B >= len(lens), f"edges at L_k = {Lk} needs B >= {len(lens)}"
        for b in range(B):
            kpm[b] = ar >= lens[b % len(lens)]
    elif pattern == "leading":
        assert B >= 3
        lead = 64 if Lk > 64 else Lk // 2
        for b in range(B):
            kpm[b] = (ar < lead, ar < Lk - 1, ar % 2 == 1)[b % 3]
    else:
        raise ValueError(pattern)
    return kpm


def make_inputs(B, H, Lq, Lk, hd, seed):
    """the recipe of test_attention_fwd_bwd: bf16 Q = 1.5 * randn [B*L_q, d], K|V = randn packed [B*L_k, 2d], dO = randn [B*L_q, d]"""
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    qb = (torch.randn(B * Lq, d, generator=g) * 1.5).bfloat16()
    kvb = torch.randn(B * Lk, 2 * d, generator=g).bfloat16()
    dob = torch.randn(B * Lq, d, generator=g).bfloat16()
    return qb, kvb, dob
