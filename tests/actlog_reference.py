"""Float64 reference and counted error bound of an activation-log entry (csrc/actlog.hip, hri_emo_amd.train.ActivationLog).

One entry = the statistics of one activation buffer x [n_rows, d] over the rows that COUNT:
    packed rows (cu_seqlens int32 [B + 1] or longer, B real sequences): row r counts iff cu[b] <= r < cu[b + 1] for a sequence
        b < nv at a position l = r - cu[b] < L; its index in the padded numbering is b * L + l
    padded rows [B, L]: row r = b * L + l counts iff b < nv and (kpm is None or kpm[b, l] == 0); its index is r
with nv = clamp(n_valid, 1, B) (None: B).  Over the counted rows:
    n_rows        their number                                                          (exact)
    n_bad         the number of NaN / +-Inf elements                                    (exact)
    first_bad_row the smallest padded index of a counted row that holds one, -1: none   (exact)
    absmax        max |x| over the FINITE elements, 0 without one                       (exact: a maximum rounds nothing)
    sumsq         the sum of x^2 over the FINITE elements                               (fp32 arithmetic: bounded below)

The bound on sumsq, counted from the kernels' summation tree.  u = 2^-24.  All terms are >= 0, so a term that passes through k
roundings contributes at most ((1 + u)^k - 1) times itself and |got - exact| <= ((1 + u)^k - 1) * exact with k the LONGEST chain:
    probe, per thread   a block owns a chunk of R = 32 rows = R * d / V vectors of V elements (V = 8: bf16 with d % 8 == 0, V = 4:
                        fp32 with d % 4 == 0, else V = 1); a thread owns vectors tid, tid + 256, ... and adds their elements one
                        after the other with fmaf(x, x, acc) -- the square is exact inside the fma, one rounding per element:
                        T = V * ceil(min(R, n_rows) * (d / V) / 256)
    probe, wave         6 steps of the xor butterfly                                                            6 roundings
    probe, block        the four wave sums in index order                                                       3 roundings
    fold, per thread    a block owns the C = ceil(n_rows / R) chunk partials of the site; a thread adds partials tid, tid + 256,
                        ... one after the other                                                                 ceil(C / 256) roundings
    fold, wave + block  as above                                                                                9 roundings
    k = T + 9 + ceil(C / 256) + 9
For the kernel tests (d <= 776, bf16: T = 8 * ceil(32 * 97 / 256) = 104, C <= 3) k = 123: a relative bound of 7.4e-6.  The
derivation assumes no squared term underflows (assert_no_underflow: every non-zero |x| >= 2^-60).  The float64 reference rounds
with 2^-53 per operation: negligible, added as 1e-12 relative."""
import math

import numpy as np
import torch

U = 2.0 ** -24
ROWS = 32                  # rows per chunk (hriemo_act_probe_rows())
THREADS = 256
WAVE_ROUNDINGS, BLOCK_ROUNDINGS = 6, 3


def vec_of(dtype, d, ld=None):
    """elements per load of the probe for a dense, 16-byte aligned buffer of this dtype, width and leading dimension"""
    ld = d if ld is None else ld
    if dtype == torch.bfloat16:
        return 8 if (d % 8 == 0 and ld % 8 == 0) else 1
    return 4 if (d % 4 == 0 and ld % 4 == 0) else 1


def roundings(n_rows, d, vec):
    t = vec * math.ceil(min(ROWS, n_rows) * (d // vec) / THREADS)
    chunks = math.ceil(n_rows / ROWS)
    return t + WAVE_ROUNDINGS + BLOCK_ROUNDINGS + math.ceil(chunks / THREADS) + WAVE_ROUNDINGS + BLOCK_ROUNDINGS


def sumsq_bound(sumsq64, n_rows, d, vec):
    """absolute bound on |kernel sumsq - sumsq64| for a buffer of n_rows rows (counted or not) of width d"""
    return ((1.0 + U) ** roundings(n_rows, d, vec) - 1.0 + 1e-12) * float(sumsq64)


def assert_no_underflow(x):
    a = x.detach().double().abs()
    a = a[torch.isfinite(a) & (a > 0)]
    assert a.numel() == 0 or float(a.min()) >= 2.0 ** -60, "an operand whose square leaves fp32's normal range: the bound does not cover it"


def counted_rows(n_rows, B, L, cu=None, kpm=None, n_valid=None):
    """int64 [n_rows]: the padded index of every row that counts, -1 for the others"""
    nv = B if n_valid is None else min(max(int(n_valid), 1), B)
    out = np.full(n_rows, -1, dtype=np.int64)
    if cu is not None:
        cu = [int(v) for v in cu]
        for b in range(min(nv, B)):
            for r in range(max(cu[b], 0), min(cu[b + 1], n_rows)):
                if r - cu[b] < L:
                    out[r] = b * L + (r - cu[b])
        return out
    m = None if kpm is None else np.asarray(kpm).reshape(-1).astype(bool)
    for r in range(n_rows):
        if r // L < nv and (m is None or not m[r]):
            out[r] = r
    return out


def probe_ref64(x, B, L, cu=None, kpm=None, n_valid=None):
    """x: torch tensor [n_rows, d] (bf16 or fp32; a strided view is fine) -> the entry as a dict, sumsq in float64"""
    x64 = x.detach().cpu().double().numpy()
    n_rows, _ = x64.shape
    prow = counted_rows(n_rows, B, L, cu, kpm, n_valid)
    keep = prow >= 0
    rows = x64[keep]
    fin = np.isfinite(rows)
    bad_rows = prow[keep][(~fin).any(axis=1)]
    clean = np.where(fin, rows, 0.0)
    return {"n_rows": int(keep.sum()), "n_bad": int((~fin).sum()), "first_bad_row": int(bad_rows.min()) if bad_rows.size else -1,
            "absmax": float(np.abs(clean).max()) if clean.size else 0.0, "sumsq": float((clean * clean).sum())}


def check_entry(got, ref, n_rows, d, vec, what=""):
    """got: {have, n_rows, n_bad, first_bad_row, absmax, sumsq} of one (record, half, site) -> error / bound of sumsq; everything
    else is compared exactly"""
    assert int(got["have"]) == 1, (what, "have")
    for k in ("n_rows", "n_bad", "first_bad_row"):
        assert int(got[k]) == ref[k], (what, k, int(got[k]), ref[k])
    assert float(got["absmax"]) == ref["absmax"], (what, "absmax", float(got["absmax"]), ref["absmax"])
    bound = sumsq_bound(ref["sumsq"], n_rows, d, vec)
    err = abs(float(got["sumsq"]) - ref["sumsq"])
    assert err <= bound, (what, "sumsq", float(got["sumsq"]), ref["sumsq"], err, bound)
    return err / bound if bound > 0 else 0.0
