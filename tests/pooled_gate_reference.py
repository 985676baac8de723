"""Host-side references, limits and cases for the pooled gate kernels (hri-emo_amd/csrc/rowops.hip: ln_pool2_fwd, pooled_fuse_fwd /
_bwd, ln_pool_vec_bwd, ingest_padded): no GPU needed.  Built on gate_reference.py, which is imported and not edited.

    ln_pool2_fwd     mean, rstd and the masked partials of ln_pool_fwd (compared bit for bit with that kernel on the GPU);
                     keep[b, c] = sum of the fp32 LN rows l < Lkeep of 32-row chunk c, whatever the mask says
    pooled_fuse_fwd  Abar = sum_c keep_a / Lkeep, Tbar likewise, pooled = w Abar + (1 - w) Tbar
    pooled_fuse_bwd  dw = dpooled (Abar - Tbar), g_a = w dpooled / Lkeep, g_t = (1 - w) dpooled / Lkeep
    ln_pool_vec_bwd  ln_pool_bwd with dy = (l < Lkeep ? g : 0) + (valid ? dpool : 0)

Limits.  The keep partials have the summation structure of the masked partials (block_colsum over the same rows), so they take
gate_reference.pool_part_factor unchanged.  The vector backward IS gate_reference.pool_bwd_ref / pool_bwd32 with the operands
vec_ops() builds: dH = g broadcast over the Lkeep rows (fp32, exact), w = 1, is_a = 1 -- coef dH = g exactly, dy = dpool + g carries one
rounding (inside DY_ROUNDINGS = 3), so check_pool_bwd's envelope holds as it stands."""
import torch

import gate_reference as G
import rowops_reference as R
from gate_reference import U, V

B = 3
WIDTHS = (128, 136, 768, 1024)          # NCH 1 (two waves' worth of lanes idle | one lane past 128); NCH 2 inside; NCH 2 full = the pair's maximum
LENGTHS = (1, 31, 32, 33, 70)
MASKS = ("none", "prefix", "scattered")


def keeps(L):
    """Lkeep in {1, 32, 33, L - 1, L} as far as 1 <= Lkeep <= L"""
    return sorted({k for k in (1, 32, 33, L - 1, L) if 1 <= k <= L})


def cases():
    """(L, Lkeep, d, twin, mask): every (d, L, Lkeep); mask family and source form rotate so that every width and every length meets
    every mask family and both source forms"""
    out, i = [], 0
    for d in WIDTHS:
        for L in LENGTHS:
            for k in keeps(L):
                out.append((L, k, d, (i // 3) % 2 == 1, MASKS[i % 3]))
                i += 1
    return out


def pair_cases():
    """(La, Lt, Lkeep, d, twin, mask_a, mask_t): every width, every length on either side, Lkeep in {1, chunk edge, Lt}"""
    out = []
    for j, d in enumerate(WIDTHS):
        for i, (La, Lt) in enumerate(((70, 33), (33, 32), (32, 31), (31, 1), (1, 1), (70, 70))):
            k = keeps(Lt)[(i + j) % len(keeps(Lt))]
            out.append((La, Lt, k, d, (i + j) % 2 == 0, MASKS[(i + j) % 3], MASKS[(i + j + 1) % 3]))
    return out


CASES, PAIR_CASES = cases(), pair_cases()
# beyond the pair's widths: the NCH = 4 instances of the single launches (no look-ahead row), up to the kernels' maximum d = 2048
WIDE_CASES = [(33, 32, 1032, True, "scattered"), (70, 69, 1032, False, "prefix"), (31, 1, 2048, True, "none"), (70, 70, 2048, False, "scattered")]


def case_id(c):
    L, k, d, twin, mask = c
    return f"{B}x{L}x{d}-keep{k}-{'x32' if twin else 'x16'}-{mask}"


def pair_id(c):
    La, Lt, k, d, twin, ma, mt = c
    return f"{B}x{La}|{Lt}x{d}-keep{k}-{'x32' if twin else 'x16'}-{ma}|{mt}"


def make_side(L, d, twin, mask, seed=None):
    """gate_reference.gate_side; the prefix family here has the lengths {1, mid, L}"""
    side = G.gate_side(B, L, d, "unit", twin, "none" if mask == "prefix" else mask, seed)
    if mask == "prefix":
        lens = torch.tensor([1, max(1, L // 2), L])
        side["mask"] = torch.arange(L)[None, :] >= lens[:, None]
        side["valid"] = ~side["mask"]
    return side


def keep_ref(side, Lkeep):
    """float64 keep partials [B, nc, d] and their magnitudes"""
    Bs, L, d = side["B"], side["L"], side["d"]
    f = R.ln_fwd_ref(side["ln"])
    k = (torch.arange(L) < Lkeep).double()[None, :, None]
    return G.chunk_sums(f["y"].view(Bs, L, d) * k, G.POOL_ROWS), G.chunk_sums(f["mag_y"].view(Bs, L, d) * k, G.POOL_ROWS)


def keep32(side, Lkeep, order="torch", col_order="waves", fault=None):
    """fp32 yardstick of the keep partials.  fault: masked (the mask applied to the prefix sum) | off_by_one (rows l <= Lkeep)"""
    Bs, L, d = side["B"], side["L"], side["d"]
    y32 = R.fwd32(side["ln"], order)["y32"].view(Bs, L, d)
    k = torch.arange(L) < (Lkeep + (1 if fault == "off_by_one" else 0))
    sel = k[None, :].expand(Bs, L) & (side["valid"] if fault == "masked" else torch.ones(Bs, L, dtype=torch.bool))
    return G.chunk_sums(torch.where(sel[..., None], y32, torch.zeros(())), G.POOL_ROWS, col_order)


def check_keep(got, side, Lkeep, name):
    """got [B, nc, d] fp32 on the CPU: every chunk within pool_part_factor(rows of the chunk) v mag, exact zeros behind Lkeep"""
    ref, mag = keep_ref(side, Lkeep)
    assert got.shape == ref.shape, (name, tuple(got.shape))
    r = 0.0
    for c, n in enumerate(G.chunk_rows(side["L"], G.POOL_ROWS)):
        r = max(r, R.check_elem(got[:, c], ref[:, c], mag[:, c], G.pool_part_factor(n), True, f"{name} keep partials of chunk {c}"))
    return r


# ------------------------------------------------------------------------------------------------ pooled_fuse
def fuse_case(La, Lt, Lkeep, d, seed=None):
    g = torch.Generator().manual_seed(17 * d + La + 3 * Lt + Lkeep if seed is None else seed)
    nca, nct = G.chunks(La, 32), G.chunks(Lt, 32)
    ka, kt = torch.randn(B, nca, d, generator=g), torch.randn(B, nct, d, generator=g)
    nk = G.chunks(Lkeep, 32)
    ka[:, nk:], kt[:, nk:] = 0.0, 0.0                                  # what the forward leaves behind Lkeep
    return {"ka": ka, "kt": kt, "w": torch.sigmoid(torch.randn(B, d, generator=g)), "dpooled": torch.randn(B, d, generator=g),
            "La": La, "Lt": Lt, "Lkeep": Lkeep, "d": d}


def fuse_fwd_ref(c):
    """float64 -> {abar, tbar, pooled} and mag_*"""
    n = float(c["Lkeep"])
    w = c["w"].double()
    a, t = c["ka"].double().sum(1) / n, c["kt"].double().sum(1) / n
    ma, mt = c["ka"].double().abs().sum(1) / n, c["kt"].double().abs().sum(1) / n
    return {"abar": a, "tbar": t, "pooled": w * a + (1 - w) * t, "mag_abar": ma, "mag_tbar": mt, "mag_pooled": w * ma + (1 - w) * mt}


def fuse_fwd_factors(c):
    """F: a mean over n chunk sums = n - 1 additions, 1 / Lkeep and the product (gate_reference.pool_factor); pooled carries both
    means plus FUSE_ROUNDINGS"""
    nk = G.chunks(c["Lkeep"], 32)
    return G.pool_factor(nk), G.pool_factor(nk) + G.FUSE_ROUNDINGS


def check_fuse_fwd(got, c, name):
    ref = fuse_fwd_ref(c)
    Fm, Fp = fuse_fwd_factors(c)
    return {n: R.check_elem(got[n], ref[n], ref["mag_" + n], F, True, f"{name} {n}") for n, F in (("abar", Fm), ("tbar", Fm), ("pooled", Fp))}


def fuse_bwd_ref(c, abar, tbar):
    """float64 from the fp32 inputs of the backward (abar, tbar among them) -> {dw, ga, gt} and mag_*"""
    n = float(c["Lkeep"])
    g, w, a, t = c["dpooled"].double(), c["w"].double(), abar.double(), tbar.double()
    return {"dw": g * (a - t), "ga": w * g / n, "gt": (1 - w) * g / n,
            "mag_dw": g.abs() * (a.abs() + t.abs()), "mag_ga": (w * g).abs() / n, "mag_gt": ((1 - w) * g).abs() / n}


def check_fuse_bwd(got, c, abar, tbar, name):
    """F: dw = a subtraction and a product (2); g_a = product, 1 / Lkeep, product (3); g_t one more for 1 - w (4)"""
    ref = fuse_bwd_ref(c, abar, tbar)
    return {n: R.check_elem(got[n], ref[n], ref["mag_" + n], F, True, f"{name} {n}") for n, F in (("dw", 2), ("ga", 3), ("gt", 4))}


# ------------------------------------------------------------------------------------------------ ln_pool_vec_bwd
def vec_operands(side, Lkeep, has_g=True):
    """g fp32 [B, d] (the row gradient) and dpool fp32 [B, d]"""
    g = side["gen"]
    return {"g": 0.05 * torch.randn(side["B"], side["d"], generator=g) if has_g else None, "dpool": 0.1 * torch.randn(side["B"], side["d"], generator=g),
            "Lkeep": Lkeep}


def vec_ops(side, v):
    """the operands of gate_reference.pool_bwd_ref / pool_bwd32 (is_a = 1) that state the vector backward: dH = g on every row
    l < Lkeep (fp32), w = 1"""
    Bs, d, k = side["B"], side["d"], v["Lkeep"]
    dH = None if v["g"] is None else v["g"][:, None, :].expand(Bs, k, d).contiguous()
    return {"dH": dH, "w": torch.ones(Bs, d), "dpool": v["dpool"], "Lf": k}


def cross_ops(side, v, w):
    """the operands of hriemo_ln_pool_bwd (is_a = 1) for the cross-check: dH = bf16(g / w) on every row l < Lkeep"""
    Bs, d, k = side["B"], side["d"], v["Lkeep"]
    return {"dH": (v["g"] / w).bfloat16()[:, None, :].expand(Bs, k, d).contiguous(), "w": w, "dpool": v["dpool"], "Lf": k}


def cross_limit(side, v, m32, r32):
    """|dX_vec - dX_dH| allowed when dH = bf16(g / w): w dH = g (1 + e) with |e| <= U = 2^-8, the unit roundoff of bf16 (8
    significant bits, round to nearest), so dy moves by at most U |g| on rows l < Lkeep and dX, linear in dy, by U x the magnitude of
    the g-only problem; both results are rounded to bf16 (U |dX| each: 2 U |ref| and second-order terms, U^2 mag) and each carries
    DX_FACTOR v mag of fp32 arithmetic."""
    only_g = dict(vec_ops(side, v), dpool=torch.zeros_like(v["dpool"]))
    mg = G.pool_bwd_ref(side, only_g, 1, m32, r32)["mag_dX"]
    full = G.pool_bwd_ref(side, vec_ops(side, v), 1, m32, r32)
    return U * mg + 2 * U * full["dX"].abs() + 2 * G.DX_FACTOR * V * full["mag_dX"] + 2 * U * U * full["mag_dX"]


# ------------------------------------------------------------------------------------------------ ingest_padded
def ingest_case(L, d, dtype, lens, extra=3, seed=0):
    """packed rows of `dtype` for B samples of `lens`, NaN rows behind cu[B]; -> rows [sum + extra, d], cu int32 [B + 1], the padded
    fp32 VALUES [B, L, d] (zeros on PAD rows)"""
    g = torch.Generator().manual_seed(1000 * L + d + seed)
    n = sum(lens)
    rows = torch.randn(n + extra, d, generator=g).to(dtype)
    rows[n:] = float("nan")
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens), 0)
    pad = torch.zeros(len(lens), L, d)
    for b, n_b in enumerate(lens):
        pad[b, :n_b] = rows[int(cu[b]):int(cu[b]) + n_b].float()
    return rows, cu, pad
