"""Host-side references, fp32 yardsticks, limits and cases for the pooled gate of the fp32 precision mode (hri-emo_amd/csrc/fp32mode.hip:
hriemo_pool32_ln_fwd, hriemo_pool32_gate_input, hriemo_pool32_ln_bwd): no GPU needed.  Built on fp32_reference.py and
rowops_reference.py, which are imported and not edited.

    pool32_ln_fwd      y = LayerNorm(X) per row (two-pass variance, 1 / sqrt(var + eps)), never stored;
                       part_valid[b, c] = sum of y over the VALID rows of 32-row chunk c, part_keep[b, c] = over its rows l < Lkeep
    pool32_gate_input  pool = sum_c part_valid[b, c] / max(#valid_b, 1) per modality; gate_in = [a, t, |a - t|, a * t]
    pool32_ln_bwd      dYn[b, l] = (l < Lkeep ? g[b] : 0) + (valid ? dpool[b] / max(#valid_b, 1) : 0); dX = LayerNorm'(dYn) with the
                       statistics recomputed from X; dgamma = sum dYn xhat, dbeta = sum dYn over all B L rows (+ the destination)

Every reference is float64 from the fp32 input VALUES with its magnitude `mag` (the same expression over absolute values) next to
it; a limit is F v mag with v = 2^-24, and mag == 0 means exactly 0 (rowops_reference.check_elem).  Every F is COUNTED:

    chunk partial of n rows   n + LN32_FACTOR["y"]      n - 1 additions of terms that each carry the LayerNorm's own error
    pools                     nc + 1                    nc - 1 additions of the chunk sums (inputs), one division
    gate_in                   exact                     each element is ONE fp32 operation on the pools the kernel wrote
    dX                        LN32_FACTOR["ds"] + 2     dYn carries two roundings (the division, the sum); dX is linear in dYn
    dgamma / dbeta            B L + 16 / B L            fp32_reference.ln32_sum_factor; + 1 into a non-zero destination

LN32_FACTOR is fp32_reference's measured LayerNorm envelope times LN_MARGIN; nothing here needs a measurement of its own.

The fp32 yardsticks run the same arithmetic on the CPU in three orders (ORDERS): torch's sums; the kernels' (row statistics in the
quad lane mapping and the wave butterfly, chunk rows walked wave by wave -- wave w adds rows w, w + 4, ... and the four waves are
added in turn -- partial rows reduced in order); and that walk reversed.  The worst error / limit per output observed on the
MI355X: profiles/2026-10-21_pool32_kernel_limits.log.  `fault=` turns a yardstick into a faulty kernel;
test_pool32_bound_host.py proves that every order passes every case and that every fault fails at the smallest case showing it."""
import torch

import fp32_reference as F32
import rowops_reference as R
from rowops_reference import V, GuardedVec, check_elem  # noqa: F401

B = 3
EPS = R.EPS
LENGTHS = (1, 31, 32, 33, 70)
WIDTHS = (4, 252, 256, 260, 1020, 1024)          # one lane; lane 62 | 63 | the second quad of lane 0; lane 62 of the last quad | full
MASKS = ("none", "prefix", "scattered", "allpad", "single")
ORDERS = (("torch", "torch"), ("quad", "waves"), ("rev", "waves_rev"))          # (row-statistics order, row-walk order)
LN_Y, LN_DS, LN_XH = F32.LN32_FACTOR["y"], F32.LN32_FACTOR["ds"], F32.LN32_FACTOR["xh"]


def chunks(L):
    return (L + 31) // 32


def keeps(L):
    """Lkeep in {1, 32 where it fits, L - 1 where that is at least 1, L}"""
    return sorted({k for k in (1, 32, L - 1, L) if 1 <= k <= L})


def cases():
    """(L, Lkeep, d, mask, accumulate, has_g): every (d, L, Lkeep) with the mask family, accumulate and g == NULL rotating, then every
    (L, mask) at d = 260 so that every length meets every mask family"""
    out, i = [], 0
    for d in WIDTHS:
        for L in LENGTHS:
            for k in keeps(L):
                out.append((L, k, d, MASKS[i % 5], i % 2, i % 7 != 3))
                i += 1
    for L in LENGTHS:
        for j, m in enumerate(MASKS):
            out.append((L, keeps(L)[(j + 1) % len(keeps(L))], 260, m, (j + L) % 2, True))
    return list(dict.fromkeys(out))


CASES = cases()


def case_id(c):
    L, k, d, m, acc, has_g = c
    return f"{B}x{L}x{d}-keep{k}-{m}-acc{acc}-{'g' if has_g else 'nog'}"


def mask_of(kind, L, gen):
    """bool [B, L], True = PAD, or None.  prefix: lengths {1, mid, L}; scattered: every sample keeps a valid row; allpad: sample 1
    fully masked; single: sample 2 keeps exactly one row"""
    if kind == "none":
        return None
    if kind == "prefix":
        return torch.arange(L)[None, :] >= torch.tensor([1, max(1, L // 2), L])[:, None]
    m = torch.rand(B, L, generator=gen) < 0.4
    for b in range(B):
        m[b, (5 * b + 2) % L] = False
    if kind == "allpad":
        m[1] = True
    elif kind == "single":
        m[2] = True
        m[2, L // 2] = False
    else:
        assert kind == "scattered"
    return m


def make_case(c, seed=None):
    L, k, d, kind, acc, has_g = c
    gen = torch.Generator().manual_seed(1000 * d + 10 * L + k if seed is None else seed)
    X = torch.randn(B, L, d, generator=gen) + 0.5 * torch.randn(B, L, 1, generator=gen)
    b = torch.randn(d, generator=gen)
    case = {"B": B, "L": L, "Lkeep": k, "d": d, "X": X, "gamma": 1 + 0.1 * torch.randn(d, generator=gen),
            "beta": torch.where(b < 0, -1.0, 1.0) * (0.05 + 0.1 * b.abs()), "mask": mask_of(kind, L, gen),
            "g": 0.05 * torch.randn(B, d, generator=gen) if has_g else None, "dpool": 0.1 * torch.randn(B, d, generator=gen),
            "accumulate": int(acc), "init": {"dgamma": torch.randn(d, generator=gen), "dbeta": torch.randn(d, generator=gen)} if acc else None}
    case["valid"] = torch.ones(B, L, dtype=torch.bool) if case["mask"] is None else ~case["mask"]
    case["keep"] = (torch.arange(L) < k)[None, :].expand(B, L)
    return case


def chunk_rows(L):
    return [min(32, L - 32 * c) for c in range(chunks(L))]


# ------------------------------------------------------------------------------------------------ float64
def ln64(case):
    """float64 LayerNorm of every row: y, xhat, rstd and the magnitudes of rowops_reference.ln_fwd_ref / fp32_reference.xhat_mag"""
    Bs, L, d = case["B"], case["L"], case["d"]
    x = case["X"].double().view(Bs * L, d)
    mean = x.mean(1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(1, keepdim=True) + EPS).pow(-0.5)
    gam, bet = case["gamma"].double(), case["beta"].double()
    xh = (x - mean) * rstd
    sh = (Bs, L, d)
    return {"y": (xh * gam + bet).view(sh), "mag_y": ((x.abs() + mean.abs()) * rstd * gam.abs() + bet.abs()).view(sh), "xh": xh.view(sh),
            "rstd": rstd.view(Bs, L, 1), "xh_mag1": ((x.abs() + mean.abs()) * rstd).view(sh),
            "xh_mag": ((x.abs() + mean.abs() + x.abs().mean(1, keepdim=True)) * rstd).view(sh)}


def _chunk64(t, sel):
    """[B, nc, d]: per 32-row chunk the sum of the float64 rows t [B, L, d] selected by sel [B, L]"""
    Bs, L, d = t.shape
    nc = chunks(L)
    pad = torch.zeros(Bs, nc * 32, d, dtype=t.dtype)
    pad[:, :L] = t * sel[..., None].to(t.dtype)
    return pad.view(Bs, nc, 32, d).sum(2)


def fwd_ref(case):
    f = ln64(case)
    return {"valid": _chunk64(f["y"], case["valid"]), "mag_valid": _chunk64(f["mag_y"], case["valid"]),
            "keep": _chunk64(f["y"], case["keep"]), "mag_keep": _chunk64(f["mag_y"], case["keep"])}


def check_fwd(got, case, name):
    """got {valid, keep} fp32 [B, nc, d]: every chunk within (rows of the chunk + LN32_FACTOR['y']) v mag; a chunk without a selected
    row -- behind Lkeep, or all of its rows masked -- exactly 0"""
    ref = fwd_ref(case)
    r = 0.0
    for n in ("valid", "keep"):
        assert got[n].shape == ref[n].shape, (name, n, tuple(got[n].shape))
        for c, rows in enumerate(chunk_rows(case["L"])):
            r = max(r, check_elem(got[n][:, c], ref[n][:, c], ref["mag_" + n][:, c], rows + LN_Y, True, f"{name} part_{n} chunk {c}"))
    return r


def counts(case, clamp=True):
    n = case["valid"].sum(1).double()
    return n.clamp(min=1.0) if clamp else n


def pools_ref(part, case):
    """float64 from the fp32 chunk sums the kernel is handed: (pool [B, d], mag)"""
    n = counts(case)[:, None]
    return part.double().sum(1) / n, part.double().abs().sum(1) / n


def check_pools(got, part, case, name):
    ref, mag = pools_ref(part, case)
    return check_elem(got, ref, mag, chunks(case["L"]) + 1, True, name)


def gate_in32(a, t):
    """[a, t, |a - t|, a * t] from fp32 pools: each element ONE fp32 operation, so a correct kernel equals this bit for bit"""
    return torch.cat([a, t, (a - t).abs(), a * t], dim=1)


def dyn64(case):
    Bs, L, d = case["B"], case["L"], case["d"]
    n = counts(case)[:, None, None]
    g = torch.zeros(Bs, d, dtype=torch.float64) if case["g"] is None else case["g"].double()
    k, v = case["keep"][..., None].double(), case["valid"][..., None].double()
    dp = case["dpool"].double()[:, None, :] / n
    return k * g[:, None, :] + v * dp, k * g.abs()[:, None, :] + v * dp.abs()


def bwd_ref(case):
    """float64 {dX, dgamma, dbeta, mag_*}: the magnitudes of rowops_reference.ln_bwd_ref with |dy| replaced by dYn's magnitude"""
    f = ln64(case)
    dy, mdy = dyn64(case)
    gam = case["gamma"].double()
    dyg, mdyg = dy * gam, mdy * gam.abs()
    c1, c2 = dyg.mean(2, keepdim=True), (dyg * f["xh"]).mean(2, keepdim=True)
    out = {"dX": f["rstd"] * (dyg - c1 - f["xh"] * c2),
           "mag_dX": f["rstd"] * (mdyg + mdyg.mean(2, keepdim=True) + f["xh_mag1"] * (mdyg * f["xh_mag1"]).mean(2, keepdim=True)),
           "dgamma": (dy * f["xh"]).sum((0, 1)), "mag_dgamma": (mdy * f["xh_mag"]).sum((0, 1)),
           "dbeta": dy.sum((0, 1)), "mag_dbeta": mdy.sum((0, 1))}
    if case["accumulate"]:
        for n in ("dgamma", "dbeta"):
            out[n], out["mag_" + n] = out[n] + case["init"][n].double(), out["mag_" + n] + case["init"][n].double().abs()
    return out


def sum_factor(name, case):
    """B L + 16 / B L, + 1 into a non-zero destination (fp32_reference.ln32_sum_factor over all B L rows)"""
    return F32.ln32_sum_factor(name, case["B"] * case["L"], bool(case["accumulate"]))


def check_bwd(got, case, name):
    """got {dX [B, L, d], dgamma [d], dbeta [d]} fp32 on the CPU"""
    ref = bwd_ref(case)
    return {"dX": check_elem(got["dX"], ref["dX"], ref["mag_dX"], LN_DS + 2, True, name + " dX"),
            "dgamma": check_elem(got["dgamma"], ref["dgamma"], ref["mag_dgamma"], sum_factor("dgamma", case), True, name + " dgamma"),
            "dbeta": check_elem(got["dbeta"], ref["dbeta"], ref["mag_dbeta"], sum_factor("dbeta", case), True, name + " dbeta")}


# ------------------------------------------------------------------------------------------------ fp32 yardsticks
def ln32(case, row_order, fault=None):
    """fp32 on the CPU: (xhat, rstd, y) [B L, d] with the row sums in `row_order`.  fault: unbiased | eps_outside"""
    Bs, L, d = case["B"], case["L"], case["d"]
    x = case["X"].view(Bs * L, d)
    mu = (R.row_sum(x, row_order) / d)[:, None]
    t = x - mu
    var = R.row_sum(t * t, row_order) / (d - 1 if fault == "unbiased" and d > 1 else d)
    rstd = (1.0 / (torch.sqrt(var) + EPS) if fault == "eps_outside" else 1.0 / torch.sqrt(var + EPS))[:, None]
    xh = t * rstd
    return xh, rstd, xh * case["gamma"] + case["beta"]


def walk32(t, sel, order, drop_last=False):
    """[B, nc, d] fp32: per 32-row chunk the sum of the rows of t [B, L, d] selected by sel [B, L], in a row-walk order.
    waves: wave w of four adds rows w, w + 4, ... in turn, then ((w0 + w1) + w2) + w3; waves_rev: rows and waves last first"""
    Bs, L, d = t.shape
    nc = chunks(L)
    sel = sel.clone()
    if drop_last:                 # fault: the last row of every chunk never added
        for c, rows in enumerate(chunk_rows(L)):
            sel[:, 32 * c + rows - 1] = False
    pad = torch.zeros(Bs, nc * 32, d)
    pad[:, :L] = torch.where(sel[..., None], t, torch.zeros(()))
    if order == "torch":
        return pad.view(Bs, nc, 32, d).sum(2)
    pad = pad.view(Bs, nc, 8, 4, d)
    acc = torch.zeros(Bs, nc, 4, d)
    for k in (range(8) if order == "waves" else range(7, -1, -1)):
        acc = acc + pad[:, :, k]
    w = (0, 1, 2, 3) if order == "waves" else (3, 2, 1, 0)
    return ((acc[:, :, w[0]] + acc[:, :, w[1]]) + acc[:, :, w[2]]) + acc[:, :, w[3]]


def fwd32(case, order, fault=None):
    """fp32 yardstick {valid, keep}.  fault: masked_in_valid (the mask ignored on the first masked row of every sample) |
    keep_off_by_one (rows l <= Lkeep) | behind_keep (chunks behind Lkeep hold the sums of their rows) | drop_last_row |
    unbiased | eps_outside"""
    Bs, L, d, k = case["B"], case["L"], case["d"], case["Lkeep"]
    y = ln32(case, order[0], fault)[2].view(Bs, L, d)
    valid, keep = case["valid"].clone(), case["keep"].clone()
    if fault == "masked_in_valid":
        for b in range(Bs):
            bad = (~valid[b]).nonzero()
            if len(bad):
                valid[b, int(bad[0])] = True
    if fault == "keep_off_by_one":
        keep = (torch.arange(L) <= k)[None, :].expand(Bs, L)
    if fault == "behind_keep":
        keep = keep | (torch.arange(L) >= 32 * chunks(k))[None, :]
    drop = fault == "drop_last_row"
    return {"valid": walk32(y, valid, order[1], drop), "keep": walk32(y, keep, order[1], drop)}


def pools32(part, case, order, fault=None):
    """fp32 pools from the chunk sums.  fault: cnt_unclamped | keep_divisor (Lkeep in place of the number of valid rows)"""
    n = counts(case, clamp=fault != "cnt_unclamped").float()[:, None]
    if fault == "keep_divisor":
        n = torch.full_like(n, float(case["Lkeep"]))
    nc = part.shape[1]
    if order[1] == "torch":
        s = part.sum(1)
    else:
        s = torch.zeros(part.shape[0], part.shape[2])
        for c in (range(nc) if order[1] == "waves" else range(nc - 1, -1, -1)):
            s = s + part[:, c]
    return s / n


def bwd32(case, order, fault=None):
    """fp32 yardstick {dX, dgamma, dbeta}.  fault: dpool_on_masked | g_past_keep | accumulate_ignored | dbeta_from_dx |
    unbiased | eps_outside"""
    Bs, L, d = case["B"], case["L"], case["d"]
    xh, rstd, _ = ln32(case, order[0], fault)
    n = counts(case).float()[:, None, None]
    g = torch.zeros(Bs, d) if case["g"] is None else case["g"]
    keep = torch.ones(Bs, L, dtype=torch.bool) if fault == "g_past_keep" else case["keep"]
    valid = torch.ones(Bs, L, dtype=torch.bool) if fault == "dpool_on_masked" else case["valid"]
    zero = torch.zeros(())
    dy = (torch.where(keep[..., None], g[:, None, :], zero) + torch.where(valid[..., None], case["dpool"][:, None, :] / n, zero)).view(Bs * L, d)
    dyg = dy * case["gamma"]
    c1 = (R.row_sum(dyg, order[0]) / d)[:, None]
    c2 = (R.row_sum(dyg * xh, order[0]) / d)[:, None]
    dX = rstd * (dyg - c1 - xh * c2)
    every = torch.ones(Bs, L, dtype=torch.bool)
    out = {"dX": dX.view(Bs, L, d)}
    for name, terms in (("dgamma", dy * xh), ("dbeta", dX if fault == "dbeta_from_dx" else dy)):
        if order[1] == "torch":
            s = terms.sum(0)
        else:                                     # per-block partial rows (one chunk per block), then the rows in order
            part = walk32(terms.view(Bs, L, d), every, order[1]).view(-1, d)
            s = torch.zeros(d)
            for p in (range(part.shape[0]) if order[1] == "waves" else range(part.shape[0] - 1, -1, -1)):
                s = s + part[p]
        if case["accumulate"] and fault != "accumulate_ignored":
            s = case["init"][name] + s
        out[name] = s
    return out
