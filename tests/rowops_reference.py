"""Host-side references, limits, input families and buffer helpers for the row kernels (hri-emo_amd/csrc/rowops.hip): no GPU needed.

    add_ln forward    s = x + keep * inv_keep * g      mean, rstd = (var + eps)^-1/2 (biased variance)      y = (s - mean) rstd gamma + beta
    add_ln backward   dS = rstd (dy gamma - c1 - xhat c2)    dG = keep * inv_keep * dS    dgamma = sum dy xhat    dbeta = sum dy    dbias = colsum dG
    column sum, multi-segment column reduce (optionally into a non-zero destination), rowdot forward / backward

*_ref()       float64 from the bf16 / fp32 input VALUES (inv_keep is the fp32 number the kernels multiply by), and next to every result
              its magnitude `mag`: the same expression with absolute values of the terms.  A row with a large mean loses absolute
              accuracy legitimately (s itself is rounded to fp32), so every limit scales with mag, never with |ref|.
fwd32/bwd32   the same in fp32 on the CPU: two-pass variance, bf16 round-to-nearest on store, the row statistics summed in ROW_ORDERS
              (the kernels' 64-lane butterfly over per-lane partial sums with the chunk assignment lane + 64c and with the quad
              assignment, torch's order, 64-column slabs last first) and the column sums in COL_ORDERS (per-block partial rows and
              the two-level reduce of launch_colreduce, torch's order, 64-row slabs last first).  `fault=` turns them into the faulty
              kernels of test_rowops_bound_host.py.  The ENVELOPE of a statistic is its maximum over these orders.
check_*()     the limits, all from the reference alone, with u = 2^-8 (bf16) and v = 2^-24 (fp32):
                finite       every value (an output element never stored, or a poison element read, is NaN)
                bf16         |got - ref| <= u |ref| + F v mag          fp32   |got - ref| <= F v mag          mag == 0: exactly 0
                F            plain sums of n fp32 terms (column sums, reduces, rowdot, dbeta): n, which is derivable (n - 1 additions;
                             rowdot: one more rounding per product; + 1 only where a destination or a bias is really added);
                             dgamma n + 8, dbias n + F(dS): their terms carry roundings of their own.  LayerNorm outputs
                             (y, rstd, dS / dG): LN_MARGIN x LN_ENVELOPE, the MEASURED envelope of the yardstick orders' own error
                             against float64 over LN_CASES (measure_envelope(); test_rowops_bound_host.py keeps the constants honest)
                mean         v (d + 2) mean|s|                          rstd   F v rstd (1 + (mean|s| + |mean|) rstd)
                bf16 share   elements that differ from bf16(torch-order yardstick): the rule of gemm_reference (SHARE_FACTOR x the
                             largest share on which two yardstick orders disagree + SHARE_SLACK, never more than SHARE_MAX), every
                             differing pair adjacent bf16 values unless the value cancels below the fp32 discrepancy itself

Buffers: gemm_reference.Guarded (j = 0: guard rows only, for matrices whose ABI has no leading dimension) and GuardedVec for vectors
of any length (mean, rstd, logits).  Every byte outside the logical operand is 0xFF, and so is the operand until it is written."""
import math

import numpy as np
import torch

import hashrng
from gemm_reference import (U, V, SHARE_FACTOR, SHARE_SLACK, SHARE_MAX, Guarded, bf16_ordinal, bf16_round, bf16_trunc,  # noqa: F401
                            share_cap)

EPS = 1e-5
ROW_ORDERS = ("torch", "chunk", "quad", "rev")
COL_ORDERS = ("torch", "blocks", "rev")
LN_MARGIN = 3.0          # TILE_FACTOR of gemm_reference / attn_reference
# measured on the CPU (measure_envelope over LN_CASES, every order of ROW_ORDERS; dS / dG do not depend on the column order): the
# largest |yardstick - float64| / (v mag)
#   y 18.41 (16389 x 256, where s, the row mean and beta are all small)      rstd 1.50      dS / dG 2.69 (fp32, before the bf16 rounding)
# Each of the four orders ALONE attains y 18.41 and dS 2.69 (rstd: 1.50 torch / chunk / rev, 1.40 quad): the maxima come from the
# roundings of s and of the final operations, which every order shares, not from the order of the sums -- so they do not move with
# torch's CPU summation order (build, vector ISA); the chunk and quad orders are elementwise adds and the same on every CPU, and
# measure_envelope pins torch to one thread.
# (the y statistic is a maximum of a quotient: ln_case keeps |beta| >= 0.05 so that no element has a vanishing magnitude.)
# Rounded up here; test_rowops_bound_host.py::test_envelope_constants_cover_what_the_yardsticks_measure fails if they fall behind
LN_ENVELOPE = {"y": 20.0, "rstd": 2.0, "ds": 3.0}
LN_FACTOR = {k: LN_MARGIN * e for k, e in LN_ENVELOPE.items()}
TERM_SLACK = 8           # roundings inside one term dy * xhat of dgamma (s, s - mean, xhat, the product): each <= v x the term's mag


# ------------------------------------------------------------------------------------------------ the edges, as data
WIDTHS_CHUNK = (8, 504, 512, 520, 1024, 1032, 2048, 2056, 4096)      # one active lane; NCH 1|2, 2|4, 4|8 edges; the maximum
WIDTHS_QUAD = (256, 512, 768, 1024)                                  # every width the quad mapping is built for
ROWS = (1, 3, 4, 5, 257)                                             # around one 4-row block; 65 partial rows: two-level reduce
M_STRIDE = 16389                                                     # > 4 * 4096 blocks: every grid-stride row loop takes a 2nd trip
SEED, SITE = 0x1234567811, 12

# (M, d, family, p, residual form, quad mapping, row_offset)
#   family: unit | offset (|mean| / std >= 100, fp32 twin) | const (zero variance) | zero (g = 0, no residual)
#   residual: x16 (bf16 X) | x32 (fp32 twin) | none
LN_CASES = (
    [(5, d, "unit", 0.1, ("x16", "x32", "none")[i % 3], False, 1000) for i, d in enumerate(WIDTHS_CHUNK)]      # gap 1: 2056, 4096 are NCH = 8
    + [(M, 520, "unit", 0.1, "x16", False, 77) for M in (1, 3, 4)]
    + [(257, 520, "unit", 0.1, "x32", False, 1 << 20), (257, 2056, "unit", 0.0, "x16", False, 0)]
    + [(5, 2056, "offset", 0.1, "x32", False, 1000), (257, 512, "offset", 0.0, "x32", False, 0), (4, 4096, "offset", 0.1, "x32", False, 5)]
    + [(5, 8, "const", 0.0, "x16", False, 0), (5, 2048, "const", 0.0, "x32", False, 0), (3, 4096, "const", 0.0, "x16", False, 0)]
    + [(5, 520, "zero", 0.1, "none", False, 0), (3, 2056, "zero", 0.0, "none", False, 0)]
    + [(257, 8, "unit", 0.9, "x16", False, 31)]                      # gap 4: rows that lose every element of g
    + [(5, 1032, "unit", 0.0, "x16", False, 0)]
    + [(M_STRIDE, 128, "unit", 0.1, "x16", False, 1000)]            # gap 2: the chunk-mapped row loops stride
    + [(M, d, "unit", 0.1, "x32", True, 1000) for M, d in ((5, 256), (3, 512), (4, 768), (1, 1024), (257, 768), (257, 1024))]
    + [(5, 768, "offset", 0.1, "x32", True, 9), (257, 256, "offset", 0.0, "x32", True, 0), (5, 512, "const", 0.0, "x32", True, 0),
       (5, 1024, "unit", 0.0, "x32", True, 0)]
    + [(M_STRIDE, 256, "unit", 0.1, "x32", True, 1000)]             # gap 2: the quad kernels' prefetch hand-over
)
COLSUM_M, COLSUM_N = (1, 15, 16, 17, 1000, 32785), (8, 512, 520)
ROWDOT_M, ROWDOT_D = (1, 31, 32, 33, 385), (8, 40, 768)
REDUCE_W, REDUCE_NP = (8, 40, 768, 2056), (1, 7, 8, 9, 31, 32, 33, 100)


def case_id(c):
    M, d, fam, p, res, quad, roff = c
    return f"{'quad' if quad else 'chunk'}-{M}x{d}-{fam}-p{p}-{res}"


# ------------------------------------------------------------------------------------------------ inputs
def row_keys(M, row_offset=0, row_index=None):
    """the integers that key the dropout hash of rows 0 .. M-1"""
    base = np.arange(M, dtype=np.int64) if row_index is None else np.asarray(row_index, dtype=np.int64)
    return base + int(row_offset)


def keep_mask(M, d, p, seed, site, keys):
    if p <= 0:
        return torch.ones(M, d, dtype=torch.bool)
    return torch.from_numpy(hashrng.rows_mask_at(seed, site, keys, d, p))


def inv_keep32(p):
    return float(np.float32(hashrng.inv_keep(p)))


def ln_case(M, d, family="unit", p=0.0, resid="x16", row_offset=0, row_index=None, seed=SEED, site=SITE, gen_seed=None):
    """logical operands of one add_ln call.  G, dY bf16 [M, d]; X bf16 / X32 fp32 / neither; gamma = 1 + 0.1 randn, beta = +-(0.05 + 0.1 |randn|)
    (fp32; bounded away from 0 so that mag_y is, see LN_ENVELOPE); keep [M, d] bool from the host replica of the dropout hash; ik = the fp32 value of 1 / (1 - p)."""
    g = torch.Generator().manual_seed(1000 * d + M if gen_seed is None else gen_seed)
    G = torch.randn(M, d, generator=g)
    X = torch.randn(M, d, generator=g)
    if family == "offset":             # |mean| in [112, 127], std of s about 1.04: the fp32 twin carries what bf16 could not
        assert resid == "x32"
        sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
        G, X = 0.25 * G, X + sign * (112.0 + 15.0 * torch.rand(M, 1, generator=g))
    elif family == "const":            # dyadic constants: every row sum is exact in fp32 in any order
        assert p == 0.0
        pool = torch.tensor([0.5, -1.0, 2.0, 3.0, -0.25, 1.5])
        G = pool[torch.randint(0, 6, (M, 1), generator=g)].expand(M, d).clone()
        X = pool[torch.randint(0, 6, (M, 1), generator=g)].expand(M, d).clone()
    elif family == "zero":
        assert resid == "none"
        G = torch.zeros(M, d)
    else:
        assert family == "unit"
    b = torch.randn(d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), torch.where(b < 0, -1.0, 1.0) * (0.05 + 0.1 * b.abs())
    if family == "offset":
        # one ulp of such a mean (2^-17, inherent in fp32) moves every y of the row by 7e-6: measured in the spacing of bf16 values
        # near zero that alone would pass SHARE_MAX between two correct orders, so this family keeps |y| in about [2, 6]
        gamma, beta = 0.5 * gamma, torch.where(b < 0, -1.0, 1.0) * (4.0 + 0.1 * b.abs())
    case = {"G": G.bfloat16(), "X": X.bfloat16() if resid == "x16" else None, "X32": X.float() if resid == "x32" else None,
            "gamma": gamma, "beta": beta,
            "dY": torch.randn(M, d, generator=g).bfloat16(), "eps": EPS, "p": p, "seed": seed, "site": site, "row_offset": row_offset,
            "row_index": None if row_index is None else np.asarray(row_index, dtype=np.int64), "family": family}
    case["keep"] = keep_mask(M, d, p, seed, site, row_keys(M, row_offset, row_index))
    case["ik"] = inv_keep32(p)
    return case


def with_keys(case, keys):
    """the same operands with the keep mask of other row keys (what a kernel draws that keys the hash wrongly)"""
    M, d = case["G"].shape
    out = dict(case)
    out["keep"] = keep_mask(M, d, case["p"], case["seed"], case["site"], keys)
    return out


def _resid(case, dtype):
    x = case["X32"] if case["X32"] is not None else case["X"]
    return torch.zeros(case["G"].shape, dtype=dtype) if x is None else x.to(dtype)


# ------------------------------------------------------------------------------------------------ float64 references
def ln_fwd_ref(case):
    """float64: s, mean, rstd, y, and the magnitudes mag_y = (|s| + |mean|) rstd |gamma| + |beta|, sabs = mean|s|,
    mag_rstd = rstd (1 + (mean|s| + |mean|) rstd)  (d rstd / rstd = -dvar / 2 (var + eps), |dvar| <= 2 sqrt(var) |ds|)"""
    s = _resid(case, torch.float64) + case["keep"].double() * case["ik"] * case["G"].double()
    mean = s.mean(1)
    var = (s - mean[:, None]).pow(2).mean(1)
    rstd = (var + case["eps"]).pow(-0.5)
    gam, bet = case["gamma"].double(), case["beta"].double()
    y = (s - mean[:, None]) * rstd[:, None] * gam + bet
    sabs = s.abs().mean(1)
    return {"s": s, "mean": mean, "rstd": rstd, "y": y, "sabs": sabs,
            "mag_y": (s.abs() + mean.abs()[:, None]) * rstd[:, None] * gam.abs() + bet.abs(),
            "mag_rstd": rstd * (1 + (sabs + mean.abs()) * rstd)}


def stats32(fwd):
    """the row statistics the backward is handed: the reference's, rounded to fp32 (inputs of the backward, exact from there on)"""
    return fwd["mean"].float(), fwd["rstd"].float()


def ln_bwd_ref(case, mean32, rstd32, init=None):
    """float64 from the inputs of the backward (mean32 / rstd32 are among them).  init: {name: fp32 destination} of an accumulating
    call.  Returns {name: value, 'mag_' + name: magnitude} for dS, dG, dgamma, dbeta, dbias."""
    s = _resid(case, torch.float64) + case["keep"].double() * case["ik"] * case["G"].double()
    mean, rstd = mean32.double()[:, None], rstd32.double()[:, None]
    k = case["keep"].double() * case["ik"]
    xh, xh_mag = (s - mean) * rstd, (s.abs() + mean.abs()) * rstd
    dy = case["dY"].double()
    dyg = dy * case["gamma"].double()
    c1, c2 = dyg.mean(1, keepdim=True), (dyg * xh).mean(1, keepdim=True)
    dS = rstd * (dyg - c1 - xh * c2)
    mag_dS = rstd * (dyg.abs() + dyg.abs().mean(1, keepdim=True) + xh_mag * (dyg.abs() * xh_mag).mean(1, keepdim=True))
    out = {"dS": dS, "mag_dS": mag_dS, "dG": k * dS, "mag_dG": k * mag_dS,
           "dgamma": (dy * xh).sum(0), "mag_dgamma": (dy.abs() * xh_mag).sum(0),
           "dbeta": dy.sum(0), "mag_dbeta": dy.abs().sum(0),
           "dbias": (k * dS).sum(0), "mag_dbias": (k * mag_dS).sum(0)}
    for n, v0 in (init or {}).items():
        out[n], out["mag_" + n] = out[n] + v0.double(), out["mag_" + n] + v0.double().abs()
    return out


def colsum_ref(X, init=None):
    """(sum over rows, sum of absolute values), float64; init: the fp32 destination of an accumulating call"""
    ref, mag = X.double().sum(0), X.double().abs().sum(0)
    if init is not None:
        ref, mag = ref + init.double(), mag + init.double().abs()
    return ref, mag


def reduce_ref(P, w, nseg, inits=None):
    """multi-segment column reduce of partial rows P [np, >= nseg * w]: [(ref, mag)] per segment, float64"""
    out = []
    for sg in range(nseg):
        out.append(colsum_ref(P[:, sg * w:(sg + 1) * w], None if inits is None else inits[sg]))
    return out


def rowdot_fwd_ref(Z, w, b=None):
    ref, mag = Z.double() @ w.double(), Z.double().abs() @ w.double().abs()
    if b is not None:
        ref, mag = ref + b.double(), mag + b.double().abs()
    return ref, mag


def rowdot_bwd_ref(dl, Z, w, dw0=None, db0=None):
    """dZ = bf16(fp32(dl * w)) exactly (one fp32 product, one rounding); (dw, mag), (db, mag) float64"""
    dZ = bf16_round(dl.float()[:, None] * w.float()[None, :])
    dw, mdw = dl.double() @ Z.double(), dl.double().abs() @ Z.double().abs()
    db, mdb = dl.double().sum(), dl.double().abs().sum()
    if dw0 is not None:
        dw, mdw = dw + dw0.double(), mdw + dw0.double().abs()
    if db0 is not None:
        db, mdb = db + db0.double(), mdb + db0.double().abs()
    return dZ, (dw, mdw), (db.reshape(1), mdb.reshape(1))


# ------------------------------------------------------------------------------------------------ fp32 yardsticks
_XOR = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def row_sum(t, order, skip_last_chunk=False):
    """sum over the columns of fp32 t [M, d] in one of ROW_ORDERS.  chunk / quad: lane l of 64 adds the elements of its 8-element
    chunks (4-element quads) l, l + 64, ... in turn, then the xor butterfly 32, 16, ..., 1 of wave_sum."""
    M, d = t.shape
    if skip_last_chunk:
        t = t[:, :d - 8]
        d -= 8
    if order == "torch":
        return t.sum(1)
    if order == "rev":                # 64-column slabs, last first (rev64 of gemm_reference)
        acc = torch.zeros(M)
        for lo in range(((d - 1) // 64) * 64, -1, -64):
            acc = acc + t[:, lo:lo + 64].sum(1)
        return acc
    wd = {"chunk": 8, "quad": 4}[order]
    C = (d + 64 * wd - 1) // (64 * wd)
    pad = torch.zeros(M, C * 64 * wd)
    pad[:, :d] = t
    pad = pad.view(M, C, 64, wd)
    lane = torch.zeros(M, 64)
    for c in range(C):
        for j in range(wd):
            lane = lane + pad[:, c, :, j]
    for idx in _XOR:
        lane = lane + lane[:, idx]
    return lane[:, 0].clone()


def block_partials(t, nb, twice_last=False):
    """per-block column partial sums [nb, d] of fp32 terms t [M, d] as add_ln_bwd leaves them: block b, wave w walks rows
    4b + w, + 4nb, ...; the four waves are added in turn.  twice_last: the clamped look-ahead row M - 1 consumed once more by
    the wave that prefetched it last (a fault)."""
    M, d = t.shape
    K = (M + 4 * nb - 1) // (4 * nb)
    pad = torch.zeros(K * nb * 4, d)
    pad[:M] = t
    pad = pad.view(K, nb, 4, d)
    acc = torch.zeros(nb, 4, d)
    for k in range(K):
        acc = acc + pad[k]
    if twice_last:
        r = (M - 1) % (4 * nb)
        acc[r // 4, r % 4] += t[M - 1]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def _lanes8(P, batch=False, drop=False):
    """one colreduce block over partial rows P [n, W]: 8 row-lanes g add rows g, g + 8, ... in turn (batch: four accumulators over
    rows g, g + 8, g + 16, g + 24 while q + 24 < n, the rest into the first), then the 8 lanes in turn.  drop: last row left out."""
    n = P.shape[0] - (1 if drop else 0)
    W = P.shape[1]
    lanes = []
    for g in range(8):
        s = [torch.zeros(W) for _ in range(4)]
        q = g
        if batch:
            while q + 24 < n:
                for a in range(4):
                    s[a] = s[a] + P[q + 8 * a]
                q += 32
        while q < n:
            s[0] = s[0] + P[q]
            q += 8
        lanes.append((s[0] + s[1]) + (s[2] + s[3]) if batch else s[0])
    t = torch.zeros(W)
    for g in range(8):
        t = t + lanes[g]
    return t


def reduce32(P, init=None, accumulate=False, batch=False, fault=None, stale=None):
    """fixed-order column reduce of fp32 partial rows P [np, W] -> [W].  batch=False: launch_colreduce (np <= 64 one pass, else groups
    of ceil(np / 64) rows into a scratch, then one pass over the scratch); batch=True: colreduce_batch_kernel.
    fault: 'first_pass_accumulates' (the scratch is added to, not overwritten: `stale` is what it held), 'ignore_accumulate',
    'drop_mod8' / 'drop_mod32' (last partial row lost when np is no multiple of 8 / 32)."""
    n = P.shape[0]
    drop = (fault == "drop_mod8" and n % 8 != 0) or (fault == "drop_mod32" and n % 32 != 0)
    if batch or n <= 64:
        t = _lanes8(P, batch, drop)
    else:
        per = (n + 63) // 64
        groups = [_lanes8(P[p0:min(n, p0 + per)], False, drop and p0 + per >= n) for p0 in range(0, n, per)]
        scratch = torch.stack(groups)
        if fault == "first_pass_accumulates":
            scratch = scratch + (torch.ones_like(scratch) if stale is None else stale)
        t = _lanes8(scratch)
    if accumulate and fault != "ignore_accumulate":
        t = init.float() + t
    return t


def col_sum(t, order, nb=None):
    """sum over the rows of fp32 t [M, d] in one of COL_ORDERS ('blocks': block_partials(nb) + reduce32)"""
    if order == "torch":
        return t.sum(0)
    if order == "rev":
        acc = torch.zeros(t.shape[1])
        for lo in range(((t.shape[0] - 1) // 64) * 64, -1, -64):
            acc = acc + t[lo:lo + 64].sum(0)
        return acc
    assert order == "blocks"
    return reduce32(block_partials(t, nb if nb is not None else default_blocks(t.shape[0])))


def default_blocks(M, cap=1024):
    """partial rows of the host emulation: one 4-row block each, at most `cap` (the library's cap follows the chip)"""
    return min((M + 3) // 4, cap)


def _s32(case, fault=None):
    g, x = case["G"].float(), _resid(case, torch.float32)
    ik = torch.tensor(1.0 if fault == "no_inv_keep" else case["ik"], dtype=torch.float32)
    if fault == "inv_keep_resid":
        return (x + torch.where(case["keep"], g, torch.zeros(()))) * ik
    return x + torch.where(case["keep"], g * ik, torch.zeros(()))


def fwd32(case, order="torch", fault=None):
    """the forward in fp32 as the kernels compute it -> {y (bf16), y32, mean, rstd}.  fault: one_pass | unbiased | eps_outside |
    no_eps | stats_bf16 | trunc | drop_last_chunk | no_inv_keep | inv_keep_resid"""
    s = _s32(case, fault)
    d = s.shape[1]
    invd = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(d), dtype=torch.float32)
    eps = torch.tensor(case["eps"], dtype=torch.float32)
    st = bf16_round(s).float() if fault == "stats_bf16" else s
    skip = fault == "drop_last_chunk"
    mu = row_sum(st, order, skip) * invd
    if fault == "one_pass":
        var = row_sum(st * st, order) * invd - mu * mu
    else:
        t = st - mu[:, None]
        var = row_sum(t * t, order, skip) * (1.0 / (d - 1) if fault == "unbiased" else invd)
    if fault == "eps_outside":
        rstd = 1.0 / (var.sqrt() + eps)
    elif fault == "no_eps":
        rstd = var.rsqrt()
    else:
        rstd = (var + eps).rsqrt()
    y32 = (s - mu[:, None]) * rstd[:, None] * case["gamma"].float() + case["beta"].float()
    return {"y": (bf16_trunc if fault == "trunc" else bf16_round)(y32), "y32": y32, "mean": mu, "rstd": rstd}


def bwd32(case, mean32, rstd32, order="torch", col_order="torch", fault=None, nb=None, init=None, accumulate=False):
    """the backward in fp32 as the kernels compute it -> {dX, dG (bf16), dS32, dgamma, dbeta, dbias (fp32), partials [nb, 3d]}.
    col_order None: no column sums (what a caller that only needs the dX / dG yardsticks asks for).
    fault: no_c2 | c1_lanes | dgamma_dyg | dbias_dS | lookahead_twice, or a fault of reduce32 (col_order 'blocks')."""
    s = _s32(case)
    M, d = s.shape
    invd = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(d), dtype=torch.float32)
    mu, rstd = mean32[:, None], rstd32[:, None]
    ik = torch.tensor(case["ik"], dtype=torch.float32)
    xh = (s - mu) * rstd
    dy = case["dY"].float()
    dyg = dy * case["gamma"].float()
    c1 = row_sum(dyg, order) * (1.0 / min(64, d // 8) if fault == "c1_lanes" else invd)
    c2 = row_sum(dyg * xh, order) * invd
    if fault == "no_c2":
        c2 = torch.zeros_like(c2)
    ds = rstd * (dyg - c1[:, None] - xh * c2[:, None])
    dg = torch.where(case["keep"], ds * ik, torch.zeros(()))
    terms = {"dgamma": (dyg if fault == "dgamma_dyg" else dy) * xh, "dbeta": dy, "dbias": ds if fault == "dbias_dS" else dg}
    out = {"dX": bf16_round(ds), "dG": bf16_round(dg), "dS32": ds, "dG32": dg}
    if col_order is None:
        return out
    nb = default_blocks(M) if nb is None else nb
    parts = []
    for n, t in terms.items():
        if col_order == "blocks":
            P = block_partials(t, nb, fault == "lookahead_twice")
            parts.append(P)
            out[n] = reduce32(P, None if init is None else init[n], accumulate, fault=fault)
        else:
            out[n] = col_sum(t, col_order) + (init[n].float() if accumulate else 0.0)
    if parts:
        out["partials"] = torch.cat(parts, 1)
    return out


def ln_yardsticks(case, mean32=None, rstd32=None, init=None, accumulate=False, nb=None, cols=True):
    """({order: fwd32}, {order: bwd32}) over ROW_ORDERS ('torch' first); the column order cycles through COL_ORDERS with them
    (cols=False: dX / dG only, which is all check_ln_bwd reads of a yardstick)"""
    fw = {o: fwd32(case, o) for o in ROW_ORDERS}
    bw = {}
    if mean32 is not None:
        for i, o in enumerate(ROW_ORDERS):
            bw[o] = bwd32(case, mean32, rstd32, o, COL_ORDERS[i % len(COL_ORDERS)] if cols else None, nb=nb, init=init, accumulate=accumulate)
    return fw, bw


# ------------------------------------------------------------------------------------------------ limits
def ratio_v(got, ref, mag):
    """largest |got - ref| / (v mag) (the statistic whose envelope LN_ENVELOPE records); inf where mag == 0 and got != ref"""
    err = (got.double() - ref).abs()
    if (err[mag == 0] > 0).any():
        return float("inf")
    return float((err / (V * mag).clamp(min=1e-300))[mag > 0].max()) if (mag > 0).any() else 0.0


def check_elem(got, ref, mag, factor, out_f32, name):
    """finite; |got - ref| <= (bf16: u |ref| +) factor v mag; exactly 0 where mag == 0.  Returns error / limit (<= 1)."""
    g = got.double()
    assert g.shape == ref.shape, (name, tuple(g.shape), tuple(ref.shape))
    assert torch.isfinite(ref).all() and torch.isfinite(mag).all(), (name, "reference is not finite")
    bad = int((~torch.isfinite(g)).sum())
    assert bad == 0, f"{name}: {bad} non-finite values (poison read or element not stored)"
    err = (g - ref).abs()
    lim = factor * V * mag + (0.0 if out_f32 else U * ref.abs())
    nz = int((err[lim == 0] > 0).sum())
    assert nz == 0, f"{name}: {nz} elements that must be exactly zero are not"
    r = float((err / lim.clamp(min=1e-300))[lim > 0].max()) if (lim > 0).any() else 0.0
    assert r <= 1.0, f"{name}: error is {r:.3g} x its limit ({'' if out_f32 else 'u |ref| + '}{factor:g} v mag)"
    return r


def share_ratios(got, yards, slack_lim):
    """bf16 `got` against the bf16 yardsticks (torch order first): (differing elements / cap, largest bf16 distance).  A pair more
    than one step apart counts as adjacent where |got - yard| <= slack_lim: the value cancels below the fp32 discrepancy, which
    then spans several of the tiny bf16 steps there (gemm_reference.ratios)."""
    yard = next(iter(yards.values()))
    dist = (bf16_ordinal(got.bfloat16()) - bf16_ordinal(yard)).abs()
    dist = torch.where((dist > 1) & ((got.double() - yard.double()).abs() <= slack_lim), torch.ones_like(dist), dist)
    n = got.numel()
    cap = min(SHARE_FACTOR * share_cap(yards) * n + SHARE_SLACK, SHARE_MAX * n)
    return (dist != 0).sum().item() / cap, float(dist.max().item())


def check_share(got, yards, slack_lim, name):
    share, adjacent = share_ratios(got, yards, slack_lim)
    assert adjacent <= 1.0, f"{name}: differs from the fp32 yardstick by {adjacent:.0f} bf16 steps"
    assert share <= 1.0, f"{name}: elements that differ from the fp32 yardstick are {share:.3g} x the cap"
    return share


def check_ln_fwd(got, case, ref, yards, name):
    """got: {y (bf16), y32 (fp32 or None), mean, rstd} on the CPU; ref: ln_fwd_ref; yards: {order: fwd32}.  Returns the ratios."""
    d = case["G"].shape[1]
    r = {"mean": check_elem(got["mean"], ref["mean"], ref["sabs"], d + 2, True, name + " mean"),
         "rstd": check_elem(got["rstd"], ref["rstd"], ref["mag_rstd"], LN_FACTOR["rstd"], True, name + " rstd"),
         "y": check_elem(got["y"], ref["y"], ref["mag_y"], LN_FACTOR["y"], False, name + " y")}
    if got.get("y32") is not None:
        r["y32"] = check_elem(got["y32"], ref["y"], ref["mag_y"], LN_FACTOR["y"], True, name + " y32")
    r["y share"] = check_share(got["y"], {o: f["y"] for o, f in yards.items()}, 4 * LN_FACTOR["y"] * V * ref["mag_y"], name + " y")
    return r


def bwd_sum_factor(name, M, accumulate=False):
    """F of a column sum of the backward over M rows: dbeta sums bf16 values (exact terms): M; the terms of dgamma carry
    TERM_SLACK roundings of their own; dbias sums M values of dG, each within the dS factor of its own magnitude"""
    return M + {"dbeta": 0.0, "dgamma": TERM_SLACK, "dbias": LN_FACTOR["ds"]}[name] + (1 if accumulate else 0)


def check_ln_bwd(got, case, ref, yards, name, accumulate=False):
    """got: {dX, dG (bf16 or None), dgamma, dbeta, dbias (fp32 or None)}; ref: ln_bwd_ref (with init folded in); yards: {order: bwd32}.
    dgamma / dbeta / dbias: bwd_sum_factor."""
    M = case["G"].shape[0]
    r = {}
    for n, key in (("dX", "dS"), ("dG", "dG")):
        if got.get(n) is not None:
            r[n] = check_elem(got[n], ref[key], ref["mag_" + key], LN_FACTOR["ds"], False, f"{name} {n}")
            r[n + " share"] = check_share(got[n], {o: b[n] for o, b in yards.items()}, 4 * LN_FACTOR["ds"] * V * ref["mag_" + key],
                                          f"{name} {n}")
    for n in ("dgamma", "dbeta", "dbias"):
        if got.get(n) is not None:
            r[n] = check_elem(got[n], ref[n], ref["mag_" + n], bwd_sum_factor(n, M, accumulate), True, f"{name} {n}")
    return r


def check_sum(got, ref, mag, n, name):
    """an fp32 sum whose error any order keeps within n v mag: n - 1 additions of exact terms (bf16 values, fp32 partial rows),
    + 1 for a destination or a bias that is really added, + 1 where every term is a rounded fp32 product (rowdot)"""
    return check_elem(got, ref, mag, n, True, name)


def measure_envelope(cases=LN_CASES, orders=ROW_ORDERS):
    """{y, rstd, ds}: the largest error of the fp32 yardsticks against float64 in units of v mag, over `cases`"""
    env = {"y": 0.0, "rstd": 0.0, "ds": 0.0}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _measure(env, cases, orders)
    finally:
        torch.set_num_threads(threads)
    return env


def _measure(env, cases, orders):
    for c in cases:
        M, d, fam, p, res, _, roff = c
        case = ln_case(M, d, fam, p, res, roff)
        f = ln_fwd_ref(case)
        m32, r32 = stats32(f)
        b = ln_bwd_ref(case, m32, r32)
        for o in orders:
            fw = fwd32(case, o)
            bw = bwd32(case, m32, r32, o, None)
            env["y"] = max(env["y"], ratio_v(fw["y32"], f["y"], f["mag_y"]))
            env["rstd"] = max(env["rstd"], ratio_v(fw["rstd"], f["rstd"], f["mag_rstd"]))
            env["ds"] = max(env["ds"], ratio_v(bw["dS32"], b["dS"], b["mag_dS"]), ratio_v(bw["dG32"], b["dG"], b["mag_dG"]))


# ------------------------------------------------------------------------------------------------ buffers
class GuardedVec:
    """n elements of `dtype` between `guard` elements each side, every byte 0xFF until written (Guarded, for vectors of any length)"""

    def __init__(self, n, dtype, guard=64, device="cpu"):
        self.n, self.guard = n, guard
        self.es = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * guard) * self.es,), 0xFF, dtype=torch.uint8, device=device)
        self.view = self.raw.view(dtype)[guard:guard + n]
        assert self.view.data_ptr() % 16 == 0

    @classmethod
    def of(cls, x, **kw):
        b = cls(x.numel(), x.dtype, **kw)
        b.view.copy_(x.reshape(-1))
        return b

    @property
    def ptr(self):
        return self.view.data_ptr()

    def violations(self):
        g = self.guard * self.es
        return int((self.raw[:g] != 0xFF).sum() + (self.raw[g + self.n * self.es:] != 0xFF).sum())

    def assert_intact(self, name):
        n = self.violations()
        assert n == 0, f"{name}: {n} bytes outside the logical [{self.n}] vector were written"


def first_blocks(jobs):
    """first_block of every job of a hriemo_colreduce_batch table as include/hriemo.h documents it: the running sum of
    nseg * ceil(w / 32) over the preceding jobs.  jobs: [(w, nseg)].  Returns (list, total)."""
    out, total = [], 0
    for w, nseg in jobs:
        out.append(total)
        total += nseg * math.ceil(w / 32)
    return out, total
