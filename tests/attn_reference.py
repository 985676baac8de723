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
values go through float32 first (torch has no direct conversion); the double rounding moves a result by < 2^-24 relative.

Packed (varlen) rows: packed_lengths() names the per-sample length patterns, make_packed() builds the packed inputs and the three
computations of every sample on its own lq[b] x lk[b] block, check_packed() applies check() sample by sample (tiles count from
the first row of each sequence).  make_packed_decidable() picks the data seed on the CPU, from the references alone."""
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
    {"scale": factor, "P" / "Pd" / "O" / "dP" / "delta" / "dS": fn(tensor) -> tensor} -- the host test plants its mutants there."""
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
    o = hook("O", rnd(pd_r @ v))
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


def yardstick_unnormalised(q, k, v, dO, keep=None, inv_keep=1.0):
    """The yardstick with the forward's P rounded where attn_fwd_kernel rounds it: the UNNORMALISED exp(S - rowmax) goes to bf16, and
    1/l and 1/(1-p) are applied to O afterwards.  The relative rounding is the same, the draw is another one: O moves by an ulp
    here and there, delta = rowsum(O * dO) with it, dQ and dK through delta.  Both realisations are the kernels' documented
    arithmetic, so inputs on which they differ by more than check() allows cannot test a kernel (a sample of a few rows and a
    few keys: a handful of roundings, nothing averages) -- the host test holds every row of the packed GPU table to that."""
    s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    pu = torch.exp(s - s.max(-1, keepdim=True).values)
    pu_r = bf16_round(pu) if keep is None else bf16_round(pu) * keep.double()
    o = bf16_round((pu_r @ v) / pu.sum(-1, keepdim=True) * inv_keep)
    return yardstick(q, k, v, dO, None, keep, inv_keep, hooks={"O": lambda _: o})


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


BUCKET_FILLER = (24, 9)      # rows of the all-zero filler sequence (queries, keys): past one 16-row sub-tile / short of one


def _edge_list(mx):
    return sorted({min(max(n, 1), mx) for n in EDGE_LENGTHS + (mx - 1, mx)})


def packed_lengths(pattern, max_lq, max_lk, B=None):
    """Per-sample lengths of a packed (varlen) launch at the maxima (max_lq, max_lk): (lq, lk, filler).  Every length is assigned
    explicitly, none is 0; B counts the real samples (None: the pattern's own minimum).
      edges    both sides draw from EDGE_LENGTHS + (max - 1, max) clipped to [1, max]; sample b takes entry b % n of the ascending
               query list and of the DESCENDING key list, so short queries meet long keys and the reverse (B >= both n)
      bucket   a captured step's launch: no sample reaches the maxima.  The longest sample has cap = max - 17 rows (max - 1 on a side
               of at most 17 rows, which is one tile anyway), so every sample leaves whole trailing 16-row sub-tiles -- and 64-row
               tiles where the side has them -- empty; the query lengths are cap, 1, (cap + 1) // 2, min(cap, 17) and the key
               lengths cap, (cap + 1) // 2, 1, min(cap, 17): long x long (self-attention, the one combination `edges` never
               makes), one query over half the keys, half the queries over one key, 17 x 17.  filler = True: ONE more sequence of all-zero rows follows as sample B
               (BUCKET_FILLER rows, at most cap), the way the loader's bucket appends its surplus rows
      ones     every length 1 except the middle sample, which sits at the maxima (B >= 3)
      single   B = 1 at the maxima"""
    if pattern == "edges":
        qs, ks = _edge_list(max_lq), _edge_list(max_lk)[::-1]
        B = max(len(qs), len(ks)) if B is None else B
        assert B >= max(len(qs), len(ks)), f"edges at ({max_lq}, {max_lk}) needs B >= {max(len(qs), len(ks))}"
        return [qs[b % len(qs)] for b in range(B)], [ks[b % len(ks)] for b in range(B)], False
    if pattern == "bucket":
        B = 4 if B is None else B
        cap = lambda mx: mx - 17 if mx > 17 else max(1, mx - 1)                                 # noqa: E731
        cq, ck = cap(max_lq), cap(max_lk)
        qs, ks = [cq, 1, (cq + 1) // 2, min(cq, 17)], [ck, (ck + 1) // 2, 1, min(ck, 17)]
        lq, lk = [qs[b % 4] for b in range(B)], [ks[b % 4] for b in range(B)]
        return lq + [min(BUCKET_FILLER[0], cap(max_lq))], lk + [min(BUCKET_FILLER[1], cap(max_lk))], True
    if pattern == "ones":
        B = 3 if B is None else B
        assert B >= 3
        lq, lk = [1] * B, [1] * B
        lq[B // 2], lk[B // 2] = max_lq, max_lk
        return lq, lk, False
    if pattern == "single":
        assert B in (None, 1)
        return [max_lq], [max_lk], False
    raise ValueError(pattern)


class Packed:
    """A packed (varlen) problem and its float64 references, sample by sample.
      qb [Nq, d], kvb [Nk, 2d] (K | V), dob [Nq, d]   bf16 rows of all samples back to back (d = H * hd); a filler's rows are zero
      cu_q, cu_k                                      row offsets, B + 1 entries each (B counts the filler)
      keep[b]                                         [1, H, lq[b], lk[b]] bool dropout keep-mask or None: the mask is keyed by the
                                                      position INSIDE the sequence, hashrng.attn_mask(...)[b, :, :lq[b], :lk[b]]
      ref[b], yard[b], mag[b]                         all_three of sample b on its own lq[b] x lk[b] block: nothing of the padded
                                                      shape or of a neighbour enters, and tiles count from the sequence's first row"""

    def sample(self, b, dq=0, dk=0, extra_k=0):
        """(q, k, v, dO) of sample b as [1, H, L, hd] float64; dq / dk shift the packed rows read (rows past the end of the buffers
        read as zero), extra_k lengthens (or, negative, shortens) the key range: the host test's mutants"""
        d = self.H * self.hd

        def take(x2d, r0, n):
            out = torch.zeros(n, x2d.shape[1], dtype=torch.float64)
            m = max(0, min(n, x2d.shape[0] - r0))
            out[:m] = x2d[r0:r0 + m].double()
            return out
        q0, k0 = self.cu_q[b] + dq, self.cu_k[b] + dk
        lq, lk = self.lq[b], self.lk[b] + extra_k
        return (heads(take(self.qb, q0, lq), 1, lq, self.H, self.hd), heads(take(self.kvb[:, :d], k0, lk), 1, lk, self.H, self.hd),
                heads(take(self.kvb[:, d:], k0, lk), 1, lk, self.H, self.hd), heads(take(self.dob, q0, lq), 1, lq, self.H, self.hd))

    def rows_q(self, b):
        return slice(self.cu_q[b], self.cu_q[b + 1])

    def rows_k(self, b):
        return slice(self.cu_k[b], self.cu_k[b + 1])

    def packed_ref(self, name):
        """the reference of one output as packed rows [N, d] float64"""
        return torch.cat([rows(self.ref[b][name]) for b in range(self.B)])


def sample_keep(seed, site, b, H, lq, lk, p, b_offset=0):
    """[1, H, lq, lk] keep-mask of sample b: hashrng.attn_mask(seed, site, B, H, max_lq, max_lk, p, b_offset)[b, :, :lq, :lk] without
    the rest of the padded mask (the hash is keyed by (b_offset + b, h) and the position inside the sequence, nothing else)"""
    import hashrng
    return torch.from_numpy(hashrng.attn_mask(seed, site, 1, H, lq, lk, p, b_offset + b))


def make_packed(lq, lk, filler, H, hd, seed, p=0.0, rng=None, with_reference=True):
    """Packed inputs from per-sample lengths (make_inputs's recipe: Q = 1.5 * randn, K | V = randn, dO = randn, bf16; the filler's
    rows are zero) and, per sample, reference / yardstick / magnitude.  rng = (seed, site, b_offset) of the dropout hash (p > 0)."""
    import hashrng
    c = Packed()
    c.B, c.H, c.hd, c.p, c.filler = len(lq), H, hd, p, filler
    c.lq, c.lk = list(lq), list(lk)
    assert len(lq) == len(lk) and min(c.lq) >= 1 and min(c.lk) >= 1
    c.cu_q, c.cu_k = [0], [0]
    for b in range(c.B):
        c.cu_q.append(c.cu_q[-1] + c.lq[b])
        c.cu_k.append(c.cu_k[-1] + c.lk[b])
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    c.qb = (torch.randn(c.cu_q[-1], d, generator=g) * 1.5).bfloat16()
    c.kvb = torch.randn(c.cu_k[-1], 2 * d, generator=g).bfloat16()
    c.dob = torch.randn(c.cu_q[-1], d, generator=g).bfloat16()
    if filler:
        c.qb[c.cu_q[-2]:] = 0
        c.kvb[c.cu_k[-2]:] = 0
        c.dob[c.cu_q[-2]:] = 0
    c.inv_keep = hashrng.inv_keep(p)
    c.keep = [sample_keep(rng[0], rng[1], b, H, c.lq[b], c.lk[b], p, rng[2]) if p > 0 else None for b in range(c.B)]
    c.ref, c.yard, c.mag = [], [], []
    if with_reference:
        for b in range(c.B):
            r, y, m = all_three(*c.sample(b), None, c.keep[b], c.inv_keep)
            c.ref.append(r), c.yard.append(y), c.mag.append(m)
    return c


DECIDABLE_TRIES = 8


def realisation_gap(c):
    """How far the two float64 realisations of the kernels' documented rounding points (yardstick, yardstick_unnormalised) stand apart
    on the packed problem c, in units of check()'s limits: the worst, over samples and outputs, of the elementwise ratio and of
    ||other - ref|| / (3 * ||yard - ref||) per 64-row tile -- WITHOUT the 2^-16 * ||M|| term, which is the allowance for fp32
    arithmetic and belongs to the GPU, not to a float64 computation.  Above 1 the per-tile rule would reject a correct kernel: the
    tile holds so few roundings (one query row over three keys, one key under dropout) that the yardstick's error is a single
    draw and not a scale."""
    worst = 0.0
    for b in range(c.B):
        other = yardstick_unnormalised(*c.sample(b), c.keep[b], c.inv_keep)
        for n in OUTPUTS:
            ref, yard = c.ref[b][n], c.yard[b][n]
            elem, _ = ratios(other[n], ref, yard, c.mag[b][n])
            tile = (_tile_norms(other[n] - ref) / (TILE_FACTOR * _tile_norms(yard - ref) + 1e-30)).max().item()
            worst = max(worst, elem, tile)
    return worst


def make_packed_decidable(lq, lk, filler, H, hd, seed, p=0.0, rng=None):
    """make_packed with the first data seed of seed, seed + 1000, seed + 2000, ... on which check() can judge a kernel
    (realisation_gap <= 1): the inputs are chosen on the CPU, from the references alone, before anything runs on a GPU.  Lengths,
    shapes and limits are untouched.  -> (Packed, index of the seed taken)"""
    for k in range(DECIDABLE_TRIES):
        c = make_packed(lq, lk, filler, H, hd, seed + 1000 * k, p, rng)
        c.gap = realisation_gap(c)
        if c.gap <= 1.0:
            return c, k
    raise AssertionError(f"no data seed in {DECIDABLE_TRIES} tries on which the two float64 realisations agree within check()'s limits")


def packed_ratios(got2d, c, name, side):
    """worst (elementwise, per tile) error / limit of packed rows got2d [N, d] over the samples; side "q" (O, dQ) or "k" (dK, dV)"""
    worst = (0.0, 0.0)
    for b in range(c.B):
        sl, L = (c.rows_q(b), c.lq[b]) if side == "q" else (c.rows_k(b), c.lk[b])
        e, t = ratios(heads(got2d[sl], 1, L, c.H, c.hd), c.ref[b][name], c.yard[b][name], c.mag[b][name])
        worst = (max(worst[0], e), max(worst[1], t))
    return worst


def check_packed(got2d, c, name, side):
    """check() of every sample of packed rows got2d [N, d] (limits unchanged: 4u * M elementwise, the per-64-row-tile rule with
    tiles counted from the first row of each sequence); returns the worst two ratios"""
    worst = (0.0, 0.0)
    for b in range(c.B):
        sl, L = (c.rows_q(b), c.lq[b]) if side == "q" else (c.rows_k(b), c.lk[b])
        e, t = check(heads(got2d[sl], 1, L, c.H, c.hd), c.ref[b][name], c.yard[b][name], c.mag[b][name],
                     f"{name} of sample {b} (lq {c.lq[b]}, lk {c.lk[b]})")
        worst = (max(worst[0], e), max(worst[1], t))
    return worst


def make_inputs(B, H, Lq, Lk, hd, seed):
    """the recipe of test_attention_fwd_bwd: bf16 Q = 1.5 * randn [B*L_q, d], K|V = randn packed [B*L_k, 2d], dO = randn [B*L_q, d]"""
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    qb = (torch.randn(B * Lq, d, generator=g) * 1.5).bfloat16()
    kvb = torch.randn(B * Lk, 2 * d, generator=g).bfloat16()
    dob = torch.randn(B * Lq, d, generator=g).bfloat16()
    return qb, kvb, dob
