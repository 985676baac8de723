"""Host-side references, limits, input families and edges for the beta-gate / pool / fuse kernels (hri-emo_amd/csrc/rowops.hip) and
the legacy scalar gate: no GPU needed.  Built on rowops_reference.py (the LayerNorm rules, the summation orders, the reduce, the
buffers) the way that module is built on gemm_reference.py.

    ln_pool_fwd     Yn = LN(x) on rows l < Lkeep (bf16), mean, rstd, partials[b, c] = sum of the fp32 LN rows of chunk c (32 rows) that are valid
    gate_input      cnt = max(#valid, 1), pool = sum_c partials / cnt, gate_in = bf16 [a, t, |a - t|, a t] of the fp32 pools
    sigmoid_beta    w = 1 / (1 + exp(-pre)), beta = mean_d w
    fuse_fwd        H = bf16(w A + (1 - w) T)
    fuse_bwd_dw     partials[b, c] = sum over the 32 rows of chunk c of dH (A - T)
    gate_dpre       dpre = bf16((dbeta / d + sum_c partials, in chunk order) w (1 - w))
    gate_input_bwd  da = (g0 + sign(a - t) g2 + t g3) / cnt_a, dt = (g1 - sign(a - t) g2 + a g3) / cnt_t, sign(0) = 0
    ln_pool_bwd     dy = (l < Lf ? coef dH : 0) + (valid ? dpool : 0), coef = w | 1 - w;  dX = rstd (dy gamma - c1 - xhat c2) (bf16);
                    partials[b, c] = [sum dy xhat | sum dy] over the 16 rows of chunk c;  dgamma | dbeta = their reduce (launch_colreduce)
    legacy          masked_mean_fwd, rowsum_f32, scalar_gate_dx, gate_input_pooled

*_ref()     float64 from the bf16 / fp32 input VALUES, and next to every result its magnitude `mag_*`: the same expression with
            absolute values of the terms.  Every limit scales with mag, never with |ref| or a maximum over the tensor.
*32()       the same in fp32 on the CPU as the kernels compute it, bf16 round-to-nearest on store: row statistics in
            rowops_reference.ROW_ORDERS, column sums per chunk in CHUNK_ORDERS ('waves': wave w adds rows l = w, w + 4, ... of the chunk
            in turn, then ((w0 + w1) + w2) + w3 -- block_colsum), the reduce through reduce32.  `fault=` turns them into the faulty
            kernels of test_gate_bound_host.py.
check_*()   the limits, u = 2^-8, v = 2^-24, all from the reference alone (rowops_reference.check_elem: finite, exact zeros where mag == 0):
              plain sums   F v mag;  F = the number of additions + the roundings one term carries, stated at each factor below
              Yn, mean, rstd   the y / mean / rstd rules of rowops_reference (LN_FACTOR, d + 2)
              dX           LN_MARGIN x GATE_ENVELOPE['dx'], the MEASURED error of the yardstick orders against float64 (measure_gate_envelope)
              sigmoid      SIGMOID_FACTOR v w: 3 x the measured error of 1 / (1 + e) with e = exp2(fl(-x log2 e)) moved by one ulp either way
              bf16         u |ref| + F v mag, and the share / adjacency rule of gemm_reference against the bf16 yardsticks
"""
import math

import torch

import rowops_reference as R
from gemm_reference import U, V, Guarded, bf16_round                                         # noqa: F401
from rowops_reference import (EPS, LN_FACTOR, LN_MARGIN, ROW_ORDERS, TERM_SLACK, GuardedVec, check_elem, check_share, check_sum,  # noqa: F401
                              col_sum, ratio_v, reduce32, row_sum)

POOL_ROWS = 32           # rows of one block of ln_pool_fwd / fuse_bwd_dw
BWD_ROWS = 16            # POOL_BWD_ROWS of rowops.hip
CHUNK_ORDERS = ("waves", "torch", "rev")
GRID_CAP, BLOCK = 8192, 256          # grid cap of fuse_fwd / scalar_gate_dx

# measured on the CPU (measure_gate_envelope over BWD_CASES, every order of ROW_ORDERS, torch pinned to one thread): the largest
# |yardstick - float64| / (v mag)
#   dX 3.24 (fp32, before the bf16 rounding; the add_ln backward measures 2.69: there dy is an exact bf16 input, here it is
#   coef dH + dpool and carries up to three roundings of its own)            y 5.27, rstd 1.74: inside rowops_reference.LN_ENVELOPE
#   (20, 2), which the forward therefore REUSES (test_gate_bound_host.py asserts that it covers the gate cases)
# Rounded up; test_gate_bound_host.py::test_envelope_constants_cover_what_the_yardsticks_measure fails if it falls behind
GATE_ENVELOPE = {"dx": 4.0}
DX_FACTOR = LN_MARGIN * GATE_ENVELOPE["dx"]
# measured on the CPU (measure_sigmoid): the largest |w32 - w| / (v w) over 65536 pre-activations in [-8, 8] is 10.41 with the
# exponential moved by -1, 0, +1 ulp.  Its parts at pre = -8, where w ~ 1 / e^8 inherits the relative error of the exponential: the
# argument fl(8 log2 e) = 11.54 (half an ulp there is 5.5 v of e, the fp32 constant log2 e another 1.8 v), the exponential itself
# (1.5 ulp = 3 v), 1 + e and the reciprocal.  x 3 (LN_MARGIN), rounded up
SIGMOID_MEASURED = 10.41
SIGMOID_FACTOR = 32.0
PRE_MAX = 8.0            # |pre| of the sigmoid inputs: the error of the exponential's argument grows with it
DY_ROUNDINGS = 3         # 1 - w, coef * dH, + dpool: the roundings inside one dy of ln_pool_bwd
FUSE_ROUNDINGS = 4       # w a; 1 - w (inexact whenever w < 0.5); its product with t; the sum -- each at most v x the magnitude |w a| + |1 - w| |t|
GIN_BWD_ROUNDINGS = 5    # t g3, two additions, 1 / cnt, the product with it
DX_SCALAR_ROUNDINGS = 5  # 1 / cnt, ic dpool, 1 - beta, coef dH, the sum

# ------------------------------------------------------------------------------------------------ the edges, as data
WIDTHS = (8, 504, 512, 520, 1024, 1032, 2048, 2056, 4096)   # one lane; NCH 1|2 (the pair kernel's edge); 2|4 = CLDS / PF on|off; 4|8; the maximum
PAIR_WIDTHS = (8, 504, 512, 520, 1024)
FWD_LENGTHS = (1, 3, 4, 5, 31, 32, 33, 37, 70)              # around 4 waves and one 32-row chunk; 37, 70: a last chunk where waves own 1-2 rows
BWD_LENGTHS = (1, 3, 4, 5, 15, 16, 17, 21, 33, 70)          # the same around the 16-row chunk (17, 33: three waves of the last chunk own no row)
MASKS = ("none", "prefix", "scattered", "full", "single")
CHUNK_COUNTS = (1, 8, 9, 13)                                # gate_input / gate_dpre: a partial trip, a full trip, a second trip of the 8-wide groups
# gate_input: (audio chunks, text chunks, mask of the audio side).  Every chunk-count pair under two mask families, every family at
# least once on either side of La = 256 (27, 251 | 283, 411 rows: one and two trips of the kernel's count loop); 'full' -- the middle
# sample without a valid row, the one place where cnt = max(#valid, 1) is the clamp and not the count -- at 27, 283 and 411 rows
GATE_INPUT_CASES = ((1, 1, "full"), (1, 1, "single"), (8, 9, "none"), (8, 9, "scattered"), (9, 13, "full"), (9, 13, "scattered"),
                    (13, 8, "full"), (13, 8, "single"), (13, 8, "none"))
ROWSUM_N = (1, 255, 256, 257)
SECOND_TRIP = (2, 2053, 4096)                               # B, L, d with B L d/8 > 8192 * 256


def nch(d):
    """the DISPATCH_NCH instance that runs width d"""
    n = (d // 8 + 63) // 64
    return 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8


def chunks(L, rows):
    return (L + rows - 1) // rows


def keep_cases(L, rows):
    """Lkeep / Lf in {0, 1, mid-chunk, chunk edge, L}, as far as L has them"""
    return sorted({0, 1, min(L, rows // 2 + 3), min(L, rows), min(L, rows + rows // 2 + 1), L})


def _shapes(lengths):
    """every length at the widths of three code paths (520: NCH 2, look-ahead; 1032: NCH 4, none; 2056: NCH 8), every other width at two"""
    return [(L, d) for d in (520, 1032, 2056) for L in lengths] + [(L, d) for d in WIDTHS if d not in (520, 1032, 2056) for L in (5, 37)]


def _fwd_cases():
    """(B, L, Lkeep, d, family, twin, mask)"""
    out = []
    for i, (L, d) in enumerate(_shapes(FWD_LENGTHS)):
        ks = keep_cases(L, POOL_ROWS)
        out.append((3, L, ks[i % len(ks)], d, "unit", i % 2 == 1, MASKS[i % 5]))
    out += [(3, 70, k, d, "unit", False, "scattered") for d in (512, 2056) for k in keep_cases(70, POOL_ROWS)]
    out += [(3, 37, 33, 4096, "offset", True, "prefix"), (3, 33, 0, 520, "offset", True, "full"), (3, 37, 37, 1032, "const", True, "scattered"),
            (3, 5, 4, 8, "const", False, "none"), (3, 70, 32, 2048, "unit", True, "single")]
    return out


def _bwd_cases():
    """(B, L, Lf, d, family, twin, mask, is_a, has_dH)"""
    out = []
    for i, (L, d) in enumerate(_shapes(BWD_LENGTHS)):
        ks = keep_cases(L, BWD_ROWS)
        out.append((3, L, ks[i % len(ks)], d, "unit", i % 2 == 0, MASKS[(i + 2) % 5], (i // 2) % 2, True))
    out += [(3, 70, k, d, "unit", True, "scattered", k % 2, True) for d in (512, 2056) for k in keep_cases(70, BWD_ROWS)]
    out += [(3, 21, 17, 4096, "offset", True, "prefix", 1, True), (3, 33, 5, 520, "offset", True, "full", 0, True),
            (3, 17, 17, 1032, "const", True, "scattered", 1, True), (3, 5, 0, 8, "const", False, "none", 0, True),
            (3, 21, 0, 520, "unit", False, "single", 1, False), (3, 21, 0, 2056, "unit", True, "full", 0, False)]
    return out


FWD_CASES, BWD_CASES = _fwd_cases(), _bwd_cases()
MANY_PARTIALS = (5, 210, 8)                                 # B, L, d: 5 * 14 = 70 > 64 partial rows into launch_colreduce


def fwd_id(c):
    B, L, Lk, d, fam, twin, mask = c
    return f"{B}x{L}x{d}-keep{Lk}-{fam}-{'x32' if twin else 'x16'}-{mask}"


def bwd_id(c):
    B, L, Lf, d, fam, twin, mask, is_a, has = c
    return f"{B}x{L}x{d}-Lf{Lf}-{fam}-{'x32' if twin else 'x16'}-{mask}-{'a' if is_a else 't'}{'' if has else '-nodH'}"


# ------------------------------------------------------------------------------------------------ inputs
def make_mask(kind, B, L, g):
    """[B, L] bool, True = padding; None for 'none'.  prefix: ragged lengths >= 1; scattered: pad rows among valid ones, row 0 pad
    (a pad row below any Lkeep) and the last row valid (a valid row behind pad rows) when L > 1; full: scattered with the middle
    sample all padding; single: scattered with sample 0 keeping only its last row"""
    if kind == "none":
        return None
    if kind == "prefix":
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[0] = max(1, L // 2)
        return torch.arange(L)[None, :] >= lens[:, None]
    m = torch.rand(B, L, generator=g) < 0.4
    if L > 1:
        m[:, 0], m[:, L - 1] = True, False
    else:
        m[:] = False
    if kind == "full":
        m[B // 2] = True
    elif kind == "single":
        m[0] = True
        m[0, L - 1] = False
    else:
        assert kind == "scattered"
    return m


def gate_side(B, L, d, family="unit", twin=False, mask="none", seed=None):
    """one modality's operands.  'ln' is a rowops_reference case over the B * L rows (G = 0, no dropout: s is x itself), so that
    ln_fwd_ref / fwd32 and their rules apply as they stand; families as in rowops_reference.ln_case"""
    g = torch.Generator().manual_seed(7919 * d + 31 * L + B if seed is None else seed)
    M = B * L
    X = torch.randn(M, d, generator=g)
    if family == "offset":
        assert twin
        X = X + torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0) * (112.0 + 15.0 * torch.rand(M, 1, generator=g))
    elif family == "const":
        pool = torch.tensor([0.5, -1.0, 2.0, 3.0, -0.25, 1.5])
        X = pool[torch.randint(0, 6, (M, 1), generator=g)].expand(M, d).clone()
    else:
        assert family == "unit"
    b = torch.randn(d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), torch.where(b < 0, -1.0, 1.0) * (0.05 + 0.1 * b.abs())
    if family == "offset":             # see ln_case: keeps |y| away from the tiny bf16 steps near zero
        gamma, beta = 0.5 * gamma, torch.where(b < 0, -1.0, 1.0) * (4.0 + 0.1 * b.abs())
    ln = {"G": torch.zeros(M, d, dtype=torch.bfloat16), "X": None if twin else X.bfloat16(), "X32": X.float() if twin else None,
          "gamma": gamma, "beta": beta, "dY": None, "eps": EPS, "p": 0.0, "keep": torch.ones(M, d, dtype=torch.bool), "ik": 1.0, "family": family}
    m = make_mask(mask, B, L, g)
    return {"ln": ln, "B": B, "L": L, "d": d, "mask": m, "valid": torch.ones(B, L, dtype=torch.bool) if m is None else ~m, "gen": g}


def bwd_operands(side, Lf, has_dh=True):
    """upstream gradients of one ln_pool_bwd call: dH bf16 [B, Lf, d], w in (0, 1), dpool fp32 [B, d]"""
    g, B, d = side["gen"], side["B"], side["d"]
    return {"dH": torch.randn(B, Lf, d, generator=g).bfloat16() if has_dh else None, "w": torch.sigmoid(torch.randn(B, d, generator=g)),
            "dpool": 0.1 * torch.randn(B, d, generator=g), "Lf": Lf}


def _x(side, dtype):
    ln = side["ln"]
    return (ln["X32"] if ln["X32"] is not None else ln["X"]).to(dtype).view(side["B"], side["L"], side["d"])


def _pad_chunks(t, rows):
    """[B, L, d] -> [B, nc, rows / 4, 4, d]: chunk, trip of the wave's row loop, wave; zero rows behind L"""
    B, L, d = t.shape
    nc = chunks(L, rows)
    pad = torch.zeros(B, nc * rows, d, dtype=t.dtype)
    pad[:, :L] = t
    return pad.view(B, nc, rows // 4, 4, d)


def chunk_rows(L, rows):
    return [min(L, (c + 1) * rows) - c * rows for c in range(chunks(L, rows))]


def chunk_sums(t, rows, order="waves", fault=None):
    """column sums [B, nc, d] of the fp32 (float64: the reference) terms t [B, L, d] per chunk of `rows` rows in one of CHUNK_ORDERS.
    fault: drop_last_row (the last row of every chunk left out) | lookahead_twice (the wave that owns a chunk's last row adds it once
    more) | drop_wave3"""
    B, L, d = t.shape
    pad = _pad_chunks(t, rows).clone()
    if fault == "drop_last_row":
        for c, n in enumerate(chunk_rows(L, rows)):
            pad[:, c, (n - 1) // 4, (n - 1) % 4] = 0
    if t.dtype == torch.float64 or order == "torch":
        return pad.sum((2, 3))
    K = rows // 4
    if order == "rev":
        acc = torch.zeros(B, pad.shape[1], d)
        for k in range(K - 1, -1, -1):
            for w in range(3, -1, -1):
                acc = acc + pad[:, :, k, w]
        return acc
    assert order == "waves"
    acc = torch.zeros(B, pad.shape[1], 4, d)
    for k in range(K):
        acc = acc + pad[:, :, k]
    if fault == "lookahead_twice":
        for c, n in enumerate(chunk_rows(L, rows)):
            acc[:, c, (n - 1) % 4] += pad[:, c, (n - 1) // 4, (n - 1) % 4]
    if fault == "drop_wave3":
        acc[:, :, 3] = 0
    return ((acc[:, :, 0] + acc[:, :, 1]) + acc[:, :, 2]) + acc[:, :, 3]


def seq_sum(P, order="seq"):
    """sum over dim 1 of P [B, n, d] (fp32): in turn (the kernels' chunk order), torch's order, last first"""
    if order == "torch":
        return P.sum(1)
    acc = torch.zeros(P.shape[0], P.shape[2])
    for k in (range(P.shape[1]) if order == "seq" else range(P.shape[1] - 1, -1, -1)):
        acc = acc + P[:, k]
    return acc


SEQ_ORDERS = ("seq", "torch", "rev")


# ------------------------------------------------------------------------------------------------ ln_pool_fwd
def pool_fwd_ref(side, Lkeep):
    """float64: the rowops_reference forward of the B * L rows (mean, rstd, sabs, mag_rstd flat), yn / mag_yn [B, Lkeep, d],
    part / mag_part [B, nc, d] over the valid rows of each 32-row chunk"""
    B, L, d = side["B"], side["L"], side["d"]
    f = R.ln_fwd_ref(side["ln"])
    y, mag = f["y"].view(B, L, d), f["mag_y"].view(B, L, d)
    v = side["valid"].double()[..., None]
    out = {k: f[k] for k in ("mean", "rstd", "sabs", "mag_rstd")}
    out.update({"yn": y[:, :Lkeep], "mag_yn": mag[:, :Lkeep], "part": chunk_sums(y * v, POOL_ROWS), "mag_part": chunk_sums(mag * v, POOL_ROWS)})
    return out


def pool_fwd32(side, Lkeep, order="torch", col_order="waves", fault=None):
    """fp32 yardstick -> {y (bf16 [B, keep, d]), y32, mean, rstd, part}.  fault: pool_drop_last_row | pool_masked | pool_bf16 |
    lkeep_off_by_one (keep = Lkeep + 1 rows are stored)"""
    B, L, d = side["B"], side["L"], side["d"]
    f = R.fwd32(side["ln"], order)
    y32 = f["y32"].view(B, L, d)
    src = bf16_round(y32).float() if fault == "pool_bf16" else y32
    valid = torch.ones_like(side["valid"]) if fault == "pool_masked" else side["valid"]
    t = torch.where(valid[..., None], src, torch.zeros(()))
    keep = Lkeep + (1 if fault == "lkeep_off_by_one" and Lkeep < L else 0)
    return {"y": f["y"].view(B, L, d)[:, :keep], "y32": y32[:, :keep], "mean": f["mean"], "rstd": f["rstd"],
            "part": chunk_sums(t, POOL_ROWS, col_order, "drop_last_row" if fault == "pool_drop_last_row" else None)}


def pool_part_factor(n):
    """F of one pooled partial sum over a chunk of n rows: at most n - 1 additions that round (the first of a wave adds to zero) + 1
    for the wave hand-over, each term an fp32 LayerNorm output within LN_FACTOR['y'] v of ITS magnitude (>= |y|)"""
    return n + LN_FACTOR["y"]


def check_pool_fwd(got, side, ref, yards, Lkeep, name):
    """got: {y bf16 [B, Lkeep, d], mean, rstd [B * L], part [B, nc, d]} on the CPU; yards: {order: pool_fwd32}"""
    d, L = side["d"], side["L"]
    r = {"mean": check_elem(got["mean"], ref["mean"], ref["sabs"], d + 2, True, name + " mean"),
         "rstd": check_elem(got["rstd"], ref["rstd"], ref["mag_rstd"], LN_FACTOR["rstd"], True, name + " rstd")}
    if Lkeep > 0:
        r["y"] = check_elem(got["y"], ref["yn"], ref["mag_yn"], LN_FACTOR["y"], False, name + " Yn")
        r["y share"] = check_share(got["y"].reshape(-1, d), {o: f["y"][:, :Lkeep].reshape(-1, d) for o, f in yards.items()},
                                   (4 * LN_FACTOR["y"] * V * ref["mag_yn"]).reshape(-1, d), name + " Yn")
    assert got["part"].shape == ref["part"].shape, (name, tuple(got["part"].shape))
    r["part"] = 0.0
    for c, n in enumerate(chunk_rows(L, POOL_ROWS)):
        r["part"] = max(r["part"], check_elem(got["part"][:, c], ref["part"][:, c], ref["mag_part"][:, c], pool_part_factor(n), True,
                                              f"{name} partials of chunk {c}"))
    return r


def store_rows(view, y, Lkeep):
    """what the forward's stores leave in a [B * Lkeep + extra, d] buffer when it writes y [B, keep, d] at rows b * Lkeep + l"""
    for b in range(y.shape[0]):
        for l in range(y.shape[1]):
            view[b * Lkeep + l] = y[b, l]


def check_untouched(view, first, name):
    """every row at or past `first` of a too-large output still holds 0xFF bytes"""
    rest = view[first:].contiguous().view(torch.uint8)
    n = int((rest != 0xFF).sum())
    assert n == 0, f"{name}: {n} bytes behind row {first} were written"


# ------------------------------------------------------------------------------------------------ gate_input
def gate_input_case(B, nca, nct, d, mask="scattered", seed=None):
    """partial sums of its own (not a forward's): pa [B, nca, d], pt [B, nct, d] = randn; La, Lt with exactly that many 32-row chunks;
    the partials of column 0 are zero on both sides, so there a == t == 0 whatever the counts (the only equal pools that survive two
    different 1 / cnt exactly): mag == 0, and a, t, |a - t| and a t must be exact zeros, in fp32 and in bf16.  The mask kind shapes
    the audio side (La = 32 nca - 5 rows: above 256, the count loop's second trip, from 9 chunks on); the text side is a prefix"""
    g = torch.Generator().manual_seed(13 * d + 101 * nca + nct if seed is None else seed)
    La, Lt = 32 * nca - 5, 32 * (nct - 1) + 1
    pa, pt = torch.randn(B, nca, d, generator=g), torch.randn(B, nct, d, generator=g)
    pa[:, :, 0], pt[:, :, 0] = 0.0, 0.0
    return {"pa": pa, "pt": pt, "B": B, "d": d, "La": La, "Lt": Lt,
            "ma": make_mask(mask, B, La, g), "mt": make_mask("prefix" if mask != "none" else "none", B, Lt, g)}


def counts(m, B, L, clamp=True):
    c = torch.full((B,), float(L), dtype=torch.float64) if m is None else (~m).double().sum(1)
    return c.clamp(min=1) if clamp else c


def gate_input_ref(c):
    """float64: cnt [B, 2] (exact), a / t pools with magnitudes, gin / mag_gin [B, 4d]"""
    ca, ct = counts(c["ma"], c["B"], c["La"]), counts(c["mt"], c["B"], c["Lt"])
    a, ma = c["pa"].double().sum(1) / ca[:, None], c["pa"].double().abs().sum(1) / ca[:, None]
    t, mt = c["pt"].double().sum(1) / ct[:, None], c["pt"].double().abs().sum(1) / ct[:, None]
    return {"cnt": torch.stack([ca, ct], 1), "a": a, "mag_a": ma, "t": t, "mag_t": mt,
            "gin": torch.cat([a, t, (a - t).abs(), a * t], 1), "mag_gin": torch.cat([ma, mt, ma + mt, ma * mt], 1)}


def pool_factor(n):
    """F of a pool over n partial sums (exact fp32 inputs): n - 1 additions, 1 / cnt, the product"""
    return n + 1


def gin_factors(nca, nct):
    """F of the four quarters of gate_in: the pools' own; |a - t|: the larger + the subtraction; a t: both + the product"""
    fa, ft = pool_factor(nca), pool_factor(nct)
    return (fa, ft, max(fa, ft) + 1, fa + ft + 1)


def gate_input32(c, order="seq", fault=None):
    """fault: cnt_unclamped"""
    ca = counts(c["ma"], c["B"], c["La"], fault != "cnt_unclamped").float()
    ct = counts(c["mt"], c["B"], c["Lt"], fault != "cnt_unclamped").float()
    one = torch.tensor(1.0)
    a, t = seq_sum(c["pa"], order) * (one / ca)[:, None], seq_sum(c["pt"], order) * (one / ct)[:, None]
    return {"cnt": torch.stack([ca, ct], 1), "a": a, "t": t, "gin": bf16_round(torch.cat([a, t, (a - t).abs(), a * t], 1))}


def check_gate_input(got, c, ref, yards, name):
    """got: {cnt [B, 2], a, t [B, d] fp32, gin [B, 4d] bf16}"""
    d, nca, nct = c["d"], c["pa"].shape[1], c["pt"].shape[1]
    assert torch.isfinite(got["cnt"]).all() and torch.equal(got["cnt"].double(), ref["cnt"]), f"{name}: cnt is not max(#valid, 1)"
    r = {"a": check_sum(got["a"], ref["a"], ref["mag_a"], pool_factor(nca), name + " a_pool"),
         "t": check_sum(got["t"], ref["t"], ref["mag_t"], pool_factor(nct), name + " t_pool")}
    for q, (F, n) in enumerate(zip(gin_factors(nca, nct), ("a", "t", "|a-t|", "a*t"))):
        sl = slice(q * d, (q + 1) * d)
        r["gin " + n] = check_elem(got["gin"][:, sl], ref["gin"][:, sl], ref["mag_gin"][:, sl], F, False, f"{name} gate_in {n}")
    F = max(gin_factors(nca, nct))
    r["gin share"] = check_share(got["gin"], {o: y["gin"] for o, y in yards.items()}, 4 * F * V * ref["mag_gin"], name + " gate_in")
    return r


def gate_input_pooled_ref(a, t):
    a, t = a.double(), t.double()
    return torch.cat([a, t, (a - t).abs(), a * t], 1), torch.cat([a.abs(), t.abs(), a.abs() + t.abs(), (a * t).abs()], 1)


def check_gate_input_pooled(got, a, t, name):
    """gate_in from given fp32 pools: a, t are one rounding to bf16 (F = 0), |a - t| and a t one fp32 rounding before it.  The bf16
    rule against the yardstick is equality here: one fp32 operation per element and a round-to-nearest convert leave no summation
    order and nothing to contract, so the share of elements on which two correct kernels may differ is zero"""
    d = a.shape[1]
    ref, mag = gate_input_pooled_ref(a, t)
    assert torch.equal(got[:, :2 * d], torch.cat([a, t], 1).bfloat16()), f"{name}: the a / t quarters are not bf16(pool)"
    r = check_elem(got[:, 2 * d:], ref[:, 2 * d:], mag[:, 2 * d:], 1, False, name + " |a-t|, a*t")
    yard = gate_input_pooled32(a, t)
    n = int((R.bf16_ordinal(got.bfloat16()) != R.bf16_ordinal(yard)).sum())
    assert n == 0, f"{name}: {n} elements differ from bf16 of the one fp32 operation"
    return r


def gate_input_pooled32(a, t):
    a, t = a.float(), t.float()
    return bf16_round(torch.cat([a, t, (a - t).abs(), a * t], 1))


# ------------------------------------------------------------------------------------------------ sigmoid_beta
def exp_fast32(x, ulps=0):
    """e^x the way __expf forms it: exp2 of the fp32 product x * log2(e), within one ulp; `ulps` moves the result by that many"""
    t = x.float() * torch.tensor(math.log2(math.e), dtype=torch.float32)
    e = torch.exp2(t.double()).float()
    for _ in range(abs(ulps)):
        e = torch.nextafter(e, torch.tensor(float("inf") if ulps > 0 else 0.0))
    return e


def sigmoid32(pre, ulps=0):
    one = torch.tensor(1.0)
    return one / (one + exp_fast32(-pre, ulps))


def sigmoid_ref(pre):
    """float64: w (its own magnitude: every term is positive), beta = mean_d w"""
    w = 1.0 / (1.0 + torch.exp(-pre.double()))
    return {"w": w, "beta": w.mean(1)}


def measure_sigmoid(n=65536):
    """largest |sigmoid32 - float64| / (v w) over n points in [-PRE_MAX, PRE_MAX] with the exponential at -1, 0, +1 ulp"""
    g = torch.Generator().manual_seed(5)
    x = ((torch.rand(n, generator=g) * 2 - 1) * PRE_MAX)[None]
    ref = sigmoid_ref(x)["w"]
    return max(ratio_v(sigmoid32(x, k), ref, ref) for k in (-1, 0, 1))


def sigmoid_inputs(B, d, seed=0):
    g = torch.Generator().manual_seed(17 * d + B + seed)
    pre = (2 * torch.randn(B, d, generator=g)).clamp(-PRE_MAX, PRE_MAX)
    pre[0, 0], pre[-1, -1] = PRE_MAX, -PRE_MAX
    return pre


def beta_factor(d):
    """F of beta: d - 1 additions and the division, each term within SIGMOID_FACTOR v of itself"""
    return d + SIGMOID_FACTOR


def beta32(w32, order="torch"):
    d = w32.shape[1]
    return row_sum(w32, order) / torch.tensor(float(d))


def check_sigmoid_beta(got_w, got_beta, pre, name):
    ref = sigmoid_ref(pre)
    return {"w": check_elem(got_w, ref["w"], ref["w"], SIGMOID_FACTOR, True, name + " w"),
            "beta": check_elem(got_beta.reshape(-1), ref["beta"], ref["beta"], beta_factor(pre.shape[1]), True, name + " beta")}


# ------------------------------------------------------------------------------------------------ fuse_fwd / fuse_bwd_dw / gate_dpre
def fuse_case(B, L, d, seed=None):
    g = torch.Generator().manual_seed(3 * d + 7 * L + B if seed is None else seed)
    return {"w": torch.sigmoid(2 * torch.randn(B, d, generator=g)), "A": torch.randn(B, L, d, generator=g).bfloat16(),
            "T": torch.randn(B, L, d, generator=g).bfloat16(), "dH": torch.randn(B, L, d, generator=g).bfloat16(), "B": B, "L": L, "d": d}


def fuse_fwd_ref(c):
    w, a, t = c["w"].double()[:, None], c["A"].double(), c["T"].double()
    return w * a + (1 - w) * t, w.abs() * a.abs() + (1 - w).abs() * t.abs()


def fuse_fwd32(c, order="plain", fault=None):
    """order: plain (every operation rounded) | fma_a, fma_t (fma(w, a, fl((1 - w) t)), fma(1 - w, t, fl(w a)): the two forms a
    contracting compiler may emit) | fma (neither product rounded).  fault: coef_w (w where 1 - w belongs)"""
    w = c["w"].float()[:, None]
    omw = w if fault == "coef_w" else 1 - w
    a, t = c["A"].float(), c["T"].float()
    wa, ot = w.double() * a.double(), omw.double() * t.double()        # exact: 24 x 8 bits
    if order == "fma":
        return bf16_round((wa + ot).float())
    if order == "fma_a":
        return bf16_round((wa + ot.float().double()).float())
    if order == "fma_t":
        return bf16_round((wa.float().double() + ot).float())
    return bf16_round(w * a + omw * t)


FUSE_ORDERS = ("plain", "fma_a", "fma_t", "fma")


def check_fuse_fwd(got, c, name, ref=None):
    ref, mag = fuse_fwd_ref(c) if ref is None else ref
    d = c["d"]
    r = {"H": check_elem(got, ref, mag, FUSE_ROUNDINGS, False, name + " H")}
    yards = {o: fuse_fwd32(c, o).reshape(-1, d) for o in FUSE_ORDERS}
    r["H share"] = check_share(got.reshape(-1, d), yards, (4 * FUSE_ROUNDINGS * V * mag).reshape(-1, d), name + " H")
    return r


def fuse_bwd_dw_ref(c):
    """float64 partial sums [B, nc, d] per 32-row chunk and their magnitudes"""
    g, a, t = c["dH"].double(), c["A"].double(), c["T"].double()
    return chunk_sums(g * (a - t), POOL_ROWS), chunk_sums(g.abs() * (a.abs() + t.abs()), POOL_ROWS)


def fuse_bwd_dw32(c, col_order="waves", fault=None):
    """fault: drop_last_row | drop_wave3"""
    return chunk_sums(c["dH"].float() * (c["A"].float() - c["T"].float()), POOL_ROWS, col_order, fault)


def dw_factor(n):
    """F of a dw partial over n rows: n - 1 additions + the wave hand-over, the difference a - t and the product of every term"""
    return n + 2


def check_fuse_bwd_dw(got, c, name):
    ref, mag = fuse_bwd_dw_ref(c)
    assert got.shape == ref.shape, (name, tuple(got.shape))
    return max(check_elem(got[:, k], ref[:, k], mag[:, k], dw_factor(n), True, f"{name} dw partials of chunk {k}")
               for k, n in enumerate(chunk_rows(c["L"], POOL_ROWS)))


def dpre_case(B, nc, d, dbeta=True, seed=None):
    g = torch.Generator().manual_seed(29 * d + nc if seed is None else seed)
    return {"part": torch.randn(B, nc, d, generator=g), "dbeta": torch.randn(B, generator=g) * d ** 0.5 if dbeta else None,
            "w": torch.sigmoid(2 * torch.randn(B, d, generator=g)), "B": B, "d": d, "L": 32 * nc - 3}


def gate_dpre_ref(c):
    w = c["w"].double()
    db = 0.0 if c["dbeta"] is None else (c["dbeta"].double() / c["d"])[:, None]
    mdb = 0.0 if c["dbeta"] is None else (c["dbeta"].double().abs() / c["d"])[:, None]
    return (c["part"].double().sum(1) + db) * w * (1 - w), (c["part"].double().abs().sum(1) + mdb) * w * (1 - w)


def dpre_factor(nc, has_dbeta):
    """F of dpre: nc - 1 additions (+ dbeta / d and its addition), then 1 - w and two products"""
    return nc - 1 + (2 if has_dbeta else 0) + 3


def gate_dpre32(c, order="seq", fault=None):
    """fault: no_dbeta"""
    w = c["w"].float()
    s = seq_sum(c["part"], order)
    if c["dbeta"] is not None and fault != "no_dbeta":
        db = (c["dbeta"].float() / torch.tensor(float(c["d"])))[:, None]
        s = seq_sum(torch.cat([db.expand(-1, c["d"])[:, None], c["part"]], 1), order)
    return bf16_round(s * w * (1 - w))


def check_gate_dpre(got, c, yards, name):
    ref, mag = gate_dpre_ref(c)
    F = dpre_factor(c["part"].shape[1], c["dbeta"] is not None)
    return {"dpre": check_elem(got, ref, mag, F, False, name + " dpre"),
            "dpre share": check_share(got, yards, 4 * F * V * mag, name + " dpre")}


# ------------------------------------------------------------------------------------------------ gate_input_bwd
def gin_bwd_case(B, d, seed=None):
    """pools with a == t in every third column and a < t in the next (a > t in the rest); counts 1, 5, 33, ..."""
    g = torch.Generator().manual_seed(41 * d + B if seed is None else seed)
    t = torch.randn(B, d, generator=g)
    gap = 0.05 + torch.rand(B, d, generator=g)
    col = torch.arange(d) % 3
    a = torch.where(col == 0, t, torch.where(col == 1, t - gap, t + gap))
    cnt = torch.tensor([[1.0, 5.0], [33.0, 1.0], [7.0, 70.0]]).repeat((B + 2) // 3, 1)[:B]
    return {"a": a, "t": t, "cnt": cnt, "dgin": (0.5 * torch.randn(B, 4 * d, generator=g)).bfloat16(), "B": B, "d": d}


def gin_bwd_ref(c):
    d = c["d"]
    a, t, g = c["a"].double(), c["t"].double(), c["dgin"].double()
    g0, g1, g2, g3 = (g[:, q * d:(q + 1) * d] for q in range(4))
    sg = torch.sign(a - t)
    ca, ct = c["cnt"].double()[:, :1], c["cnt"].double()[:, 1:]
    return {"da": (g0 + sg * g2 + t * g3) / ca, "mag_da": (g0.abs() + sg.abs() * g2.abs() + (t * g3).abs()) / ca,
            "dt": (g1 - sg * g2 + a * g3) / ct, "mag_dt": (g1.abs() + sg.abs() * g2.abs() + (a * g3).abs()) / ct}


def gin_bwd32(c, fault=None):
    """fault: sign0_is_1"""
    d = c["d"]
    a, t, g = c["a"], c["t"], c["dgin"].float()
    g0, g1, g2, g3 = (g[:, q * d:(q + 1) * d] for q in range(4))
    sg = torch.where(a >= t, 1.0, -1.0) if fault == "sign0_is_1" else torch.sign(a - t)
    one = torch.tensor(1.0)
    return {"da": (g0 + sg * g2 + t * g3) * (one / c["cnt"][:, :1]), "dt": (g1 - sg * g2 + a * g3) * (one / c["cnt"][:, 1:])}


def check_gin_bwd(got, c, name):
    ref = gin_bwd_ref(c)
    return {n: check_elem(got[n], ref[n], ref["mag_" + n], GIN_BWD_ROUNDINGS, True, f"{name} {n}") for n in ("da", "dt")}


# ------------------------------------------------------------------------------------------------ ln_pool_bwd
def pool_bwd_ref(side, ops, is_a, mean32, rstd32, init=None):
    """float64 from the inputs of the backward (mean32 / rstd32 [B * L] among them).  init: {dgamma, dbeta} fp32 destinations of an
    accumulating call.  -> dX, part [B, nc, 2d] (dgamma | dbeta per 16-row chunk), dgamma, dbeta, each with its mag_*"""
    B, L, d = side["B"], side["L"], side["d"]
    x = _x(side, torch.float64)
    mean, rstd = mean32.double().view(B, L, 1), rstd32.double().view(B, L, 1)
    gam = side["ln"]["gamma"].double()
    w = ops["w"].double()
    coef = (w if is_a else 1 - w)[:, None]
    v = side["valid"].double()[..., None]
    dy, mdy = v * ops["dpool"].double()[:, None], v * ops["dpool"].double().abs()[:, None]
    Lf = ops["Lf"]
    if ops["dH"] is not None and Lf > 0:
        dy, mdy = dy.clone(), mdy.clone()
        dy[:, :Lf] += coef * ops["dH"].double()
        mdy[:, :Lf] += coef.abs() * ops["dH"].double().abs()
    xh, xh_mag = (x - mean) * rstd, (x.abs() + mean.abs()) * rstd
    dyg, mdyg = dy * gam, mdy * gam.abs()
    c1, c2 = dyg.mean(2, keepdim=True), (dyg * xh).mean(2, keepdim=True)
    out = {"dX": rstd * (dyg - c1 - xh * c2),
           "mag_dX": rstd * (mdyg + mdyg.mean(2, keepdim=True) + xh_mag * (mdyg * xh_mag).mean(2, keepdim=True)),
           "part": torch.cat([chunk_sums(dy * xh, BWD_ROWS), chunk_sums(dy, BWD_ROWS)], 2),
           "mag_part": torch.cat([chunk_sums(mdy * xh_mag, BWD_ROWS), chunk_sums(mdy, BWD_ROWS)], 2)}
    for i, n in enumerate(("dgamma", "dbeta")):
        out[n], out["mag_" + n] = out["part"][:, :, i * d:(i + 1) * d].sum((0, 1)), out["mag_part"][:, :, i * d:(i + 1) * d].sum((0, 1))
        if init is not None:
            out[n], out["mag_" + n] = out[n] + init[n].double(), out["mag_" + n] + init[n].double().abs()
    return out


def pool_bwd32(side, ops, is_a, mean32, rstd32, order="torch", col_order="waves", fault=None, init=None, accumulate=False, stale=None,
               contract=False):
    """fp32 yardstick -> {dX (bf16), dX32, part [B, nc, 2d], dgamma, dbeta}.  contract: dy = fma(coef, dH, dpool) and
    dX = rstd fma(-xhat, c2, dy gamma - c1), the roundings a contracting compiler leaves out.  fault: coef_w | stale_dh (a row at or past Lf adds the dH
    row its wave loaded last in this chunk) | dpool_dropped_past_lf | dpool_on_masked | lookahead_twice | drop_wave3 | no_gamma
    (c1 / c2 from dy, not dy gamma) | a fault of reduce32 (ignore_accumulate, first_pass_accumulates with `stale`)"""
    B, L, d = side["B"], side["L"], side["d"]
    x = _x(side, torch.float32)
    mu, rstd = mean32.view(B, L, 1), rstd32.view(B, L, 1)
    gam = side["ln"]["gamma"].float()
    w = ops["w"].float()
    coef = (w if (is_a or fault == "coef_w") else 1 - w)[:, None]
    Lf = ops["Lf"]
    valid = side["valid"]
    if fault == "dpool_on_masked":
        valid = torch.ones_like(valid)
    if fault == "dpool_dropped_past_lf":
        valid = valid & (torch.arange(L) < Lf)[None]
    dy = torch.where(valid[..., None], ops["dpool"].float()[:, None].expand(B, L, d), torch.zeros(()))
    if ops["dH"] is not None and Lf > 0:
        gh = torch.zeros(B, L, d)
        gh[:, :Lf] = ops["dH"].float()
        if fault == "stale_dh":
            for l in range(Lf, L):
                prev = l - 4
                while prev >= Lf and prev >= (l // BWD_ROWS) * BWD_ROWS:
                    prev -= 4
                if prev >= (l // BWD_ROWS) * BWD_ROWS:
                    gh[:, l] = gh[:, prev]
        dy = (dy.double() + coef.double() * gh.double()).float() if contract else dy + coef * gh
    xh = (x - mu) * rstd
    dyg = dy * gam
    s1 = dy if fault == "no_gamma" else dyg
    invd = torch.tensor(1.0) / torch.tensor(float(d))
    c1 = (row_sum(s1.reshape(-1, d), order) * invd).view(B, L, 1)
    c2 = (row_sum((s1 * xh).reshape(-1, d), order) * invd).view(B, L, 1)
    ds = rstd * ((dyg - c1).double() - xh.double() * c2.double()).float() if contract else rstd * (dyg - c1 - xh * c2)
    cf = fault if fault in ("lookahead_twice", "drop_wave3") else None
    tg, tb = dy * xh, dy
    out = {"dX": bf16_round(ds), "dX32": ds, "part": torch.cat([chunk_sums(tg, BWD_ROWS, col_order, cf), chunk_sums(tb, BWD_ROWS, col_order, cf)], 2)}
    P = out["part"].reshape(-1, 2 * d)
    for i, n in enumerate(("dgamma", "dbeta")):
        i0 = None if init is None else init[n]
        if col_order == "waves":
            out[n] = reduce32(P[:, i * d:(i + 1) * d].contiguous(), i0, accumulate, fault=fault,
                              stale=None if stale is None else stale[:, i * d:(i + 1) * d])
        else:
            out[n] = col_sum((tg, tb)[i].reshape(-1, d), col_order) + (i0.float() if accumulate else 0.0)
    return out


def bwd_part_factor(name, n):
    """F of one column partial over n rows: n - 1 additions + the wave hand-over; a term of dbeta is a dy (DY_ROUNDINGS), a term of
    dgamma dy xhat (x - mean, its product with rstd, the product with dy on top: within rowops_reference.TERM_SLACK)"""
    return n + {"dbeta": DY_ROUNDINGS, "dgamma": TERM_SLACK}[name]


def check_pool_bwd(got, side, ref, yards, name, accumulate=False):
    """got: {dX bf16 [B, L, d], part [B, nc, 2d] or None, dgamma, dbeta fp32 [d] or None}; ref: pool_bwd_ref (init folded in);
    yards: {order: pool_bwd32}"""
    B, L, d = side["B"], side["L"], side["d"]
    r = {"dX": check_elem(got["dX"], ref["dX"], ref["mag_dX"], DX_FACTOR, False, name + " dX"),
         "dX share": check_share(got["dX"].reshape(-1, d), {o: b["dX"].reshape(-1, d) for o, b in yards.items()},
                                 (4 * DX_FACTOR * V * ref["mag_dX"]).reshape(-1, d), name + " dX")}
    if got.get("part") is not None:
        assert got["part"].shape == ref["part"].shape, (name, tuple(got["part"].shape))
        for i, n in enumerate(("dgamma", "dbeta")):
            sl = slice(i * d, (i + 1) * d)
            r[n + " part"] = max(check_elem(got["part"][:, c, sl], ref["part"][:, c, sl], ref["mag_part"][:, c, sl], bwd_part_factor(n, rows),
                                            True, f"{name} {n} partials of chunk {c}") for c, rows in enumerate(chunk_rows(L, BWD_ROWS)))
    for n in ("dgamma", "dbeta"):
        if got.get(n) is not None:
            r[n] = check_elem(got[n], ref[n], ref["mag_" + n], bwd_part_factor(n, B * L) + (1 if accumulate else 0), True, f"{name} {n}")
    return r


def make_bwd(c):
    """side, operands and the float64 forward statistics rounded to fp32 (inputs of the backward, exact from there on)"""
    B, L, Lf, d, fam, twin, mask, is_a, has = c
    side = gate_side(B, L, d, fam, twin, mask)
    m32, r32 = R.stats32(R.ln_fwd_ref(side["ln"]))
    return side, bwd_operands(side, Lf, has), m32, r32


def measure_gate_envelope(cases=None, orders=ROW_ORDERS):
    """{dx, y, rstd}: the largest error of the fp32 yardsticks against float64 in units of v mag over the gate cases"""
    env = {"dx": 0.0, "y": 0.0, "rstd": 0.0}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for c in (BWD_CASES if cases is None else cases):
            side, ops, m32, r32 = make_bwd(c)
            ref = pool_bwd_ref(side, ops, c[7], m32, r32)
            f = R.ln_fwd_ref(side["ln"])
            for o in orders:
                env["dx"] = max(env["dx"], ratio_v(pool_bwd32(side, ops, c[7], m32, r32, o, "torch")["dX32"], ref["dX"], ref["mag_dX"]))
                fw = R.fwd32(side["ln"], o)
                env["y"] = max(env["y"], ratio_v(fw["y32"], f["y"], f["mag_y"]))
                env["rstd"] = max(env["rstd"], ratio_v(fw["rstd"], f["rstd"], f["mag_rstd"]))
        if cases is None:
            for c in FWD_CASES:
                side = gate_side(c[0], c[1], c[3], c[4], c[5], c[6])
                f = R.ln_fwd_ref(side["ln"])
                for o in orders:
                    fw = R.fwd32(side["ln"], o)
                    env["y"] = max(env["y"], ratio_v(fw["y32"], f["y"], f["mag_y"]))
                    env["rstd"] = max(env["rstd"], ratio_v(fw["rstd"], f["rstd"], f["mag_rstd"]))
    finally:
        torch.set_num_threads(threads)
    return env


# ------------------------------------------------------------------------------------------------ legacy scalar gate
def masked_mean_ref(X, m):
    """X bf16 [B, L, d], m [B, L] bool or None -> cnt (exact), pooled, mag"""
    B, L, d = X.shape
    v = (torch.ones(B, L, dtype=torch.bool) if m is None else ~m).double()[..., None]
    cnt = counts(m, B, L)
    return cnt, (X.double() * v).sum(1) / cnt[:, None], (X.double().abs() * v).sum(1) / cnt[:, None]


def masked_mean32(X, m, order="waves", fault=None):
    """rows l = w, w + 4, ... per wave, then ((w0 + w1) + w2) + w3, / cnt: one chunk of ceil(L / 4) * 4 rows.  fault: cnt_unclamped |
    pool_masked"""
    B, L, d = X.shape
    valid = torch.ones(B, L, dtype=torch.bool) if (m is None or fault == "pool_masked") else ~m
    t = torch.where(valid[..., None], X.float(), torch.zeros(()))
    s = chunk_sums(t, 4 * chunks(L, 4), order)[:, 0]
    return s / counts(m, B, L, fault != "cnt_unclamped").float()[:, None]


def check_masked_mean(got, got_cnt, X, m, name):
    cnt, ref, mag = masked_mean_ref(X, m)
    assert torch.isfinite(got_cnt).all() and torch.equal(got_cnt.double(), cnt), f"{name}: cnt is not max(#valid, 1)"
    return check_sum(got, ref, mag, X.shape[1], name + " pooled")       # L - 1 additions (three of them the wave hand-over) + the division


def rowsum_ref(x):
    return x.double().sum(1), x.double().abs().sum(1)


def scalar_dx_case(B, L, Lf, d, mask="scattered", seed=None):
    g = torch.Generator().manual_seed(53 * d + L if seed is None else seed)
    m = make_mask(mask, B, L, g)
    return {"dH": torch.randn(B, Lf, d, generator=g).bfloat16(), "beta": torch.sigmoid(torch.randn(B, generator=g)),
            "dpool": torch.randn(B, d, generator=g), "mask": m, "cnt": counts(m, B, L).float(), "B": B, "L": L, "Lf": Lf, "d": d}


def scalar_dx_ref(c, is_a):
    B, L, Lf, d = c["B"], c["L"], c["Lf"], c["d"]
    beta = c["beta"].double()
    coef = (beta if is_a else 1 - beta)[:, None, None]
    v = (torch.ones(B, L, dtype=torch.bool) if c["mask"] is None else ~c["mask"]).double()[..., None]
    base = c["dpool"].double()[:, None] / c["cnt"].double()[:, None, None]
    ref, mag = (v * base).clone(), (v * base.abs()).clone()
    ref[:, :Lf] += coef * c["dH"].double()
    mag[:, :Lf] += coef.abs() * c["dH"].double().abs()
    return ref, mag


def scalar_dx32(c, is_a, fault=None, contract=False):
    """contract: fma(coef, dH, fl(ic dpool)), the product a contracting compiler leaves unrounded (coef dH is exact in float64:
    24 x 8 bits).  fault: masked_div (a masked row still gets dpool / cnt) | coef_w"""
    B, L, Lf, d = c["B"], c["L"], c["Lf"], c["d"]
    beta = c["beta"].float()
    coef = (beta if (is_a or fault == "coef_w") else 1 - beta)[:, None, None]
    valid = torch.ones(B, L, dtype=torch.bool) if (c["mask"] is None or fault == "masked_div") else ~c["mask"]
    ic = torch.where(valid, (torch.tensor(1.0) / c["cnt"])[:, None].expand(B, L), torch.zeros(()))
    o = ic[..., None] * c["dpool"][:, None]
    if contract:
        o[:, :Lf] = (o[:, :Lf].double() + coef.double() * c["dH"].double()).float()
    else:
        o[:, :Lf] = o[:, :Lf] + coef * c["dH"].float()
    return bf16_round(o)


SCALAR_DX_ORDERS = ("plain", "contract")


def check_scalar_dx(got, c, is_a, name):
    ref, mag = scalar_dx_ref(c, is_a)
    d = c["d"]
    yards = {o: scalar_dx32(c, is_a, contract=o == "contract").reshape(-1, d) for o in SCALAR_DX_ORDERS}
    return {"dX": check_elem(got, ref, mag, DX_SCALAR_ROUNDINGS, False, name + " dX"),
            "dX share": check_share(got.reshape(-1, d), yards, (4 * DX_SCALAR_ROUNDINGS * V * mag).reshape(-1, d), name + " dX")}


# ------------------------------------------------------------------------------------------------ which instance runs
def second_trip(B, L, d):
    """True when the grid-stride loop of fuse_fwd / scalar_gate_dx takes a second trip: more 8-element vectors than the capped grid holds"""
    return B * L * (d // 8) > GRID_CAP * BLOCK


def coverage():
    """{kernel instance: [case ids]} from the dispatch arithmetic alone (the listing of DESIGN.md)"""
    out = {}
    for c in FWD_CASES:
        out.setdefault(f"ln_pool_fwd<{nch(c[3])}{', look-ahead' if nch(c[3]) <= 2 else ''}{', gamma/beta reloaded' if nch(c[3]) == 8 else ''}>", []).append(fwd_id(c))
    for c in BWD_CASES:
        out.setdefault(f"ln_pool_bwd<{nch(c[3])}> {'CLDS + look-ahead' if nch(c[3]) <= 2 else 'registers, no look-ahead'}", []).append(bwd_id(c))
    for d in WIDTHS:
        out.setdefault(f"fuse_bwd_dw<{nch(d)}>", []).append(f"d={d}")
    for d in PAIR_WIDTHS:
        out.setdefault(f"ln_pool_fwd_pair / ln_pool_bwd_pair <{1 if d <= 512 else 2}>", []).append(f"d={d}")
    return out
