"""Float64 reference and counted error bounds of the unit clip modes (csrc/optim.hip: hriemo_sumsq_units,
hriemo_optim_finalize_units, hriemo_adamw_flat_units; hri_emo_amd.optim.DeviceAdamW(clip="group" | "parameter")).

The reference (clip_ref64, adamw_ref64): per clip unit u of group g
    norm_u = sqrt(sum of g_i^2 over the unit) / grad_scale
    coef_u = (max_norm_g > 0 ? min(1, max_norm_g / (norm_u + 1e-6)) : 1) / grad_scale
which is torch.nn.utils.clip_grad_norm_ applied to the unit alone, followed by torch.optim.AdamW with per-ELEMENT hyper columns
(the _ref64 idea of test_gpu_optimizer_groups.py) on the gradient coef_u * g.

The bound on a unit's sum of squares, counted from the kernels' summation tree the way health_reference.py counts its sums.
u = 2^-24.  All terms are >= 0, so a term that passes through k roundings contributes at most ((1 + u)^k - 1) times itself and
|got - exact| <= ((1 + u)^k - 1) * exact with k the LONGEST chain:
    chunk partial (hriemo_sumsq_units)
        per thread   vectors tid, tid + 256, ... of the chunk, fmaf(x, x, acc) per element:  T = 4 * ceil(ceil(len / 4) / 256)
        wave         6 steps of the xor butterfly                                                                   6
        block        the four wave sums in index order                                                              3
    unit fold (hriemo_optim_finalize_units)
        per lane     partials l, l + 64, ... of the unit's nc chunks (the first is added to 0: exact)  ceil(nc / 64) - 1
        wave         the xor butterfly                                                                              6
    k_unit = T + 9 + ceil(nc / 64) - 1 + 6
The global sum adds the U unit sums: per thread ceil(U / 256) - 1, wave 6, block 3 more.
norm = sqrtf(sum) / gs: half the relative error of the sum, plus sqrtf (1 ulp = 2 u allowed) and the quotient (u).
coef = min(1, max_norm / (norm + 1e-6)) / gs: the sum with 1e-6 (u; both addends positive), two quotients (2 u) on top of the norm's.
For full chunks (T = 128) and nc <= 128 that is k_unit = 144: 8.6e-6 on the sum, 4.5e-6 on the norm -- INSIDE the project's 1e-5
relative bound for norms and coefficients (test_gpu_optimizer.py), so the tests assert max(1e-5, counted) and print which one
applies.  The derivation assumes no square underflows (health_reference.assert_no_underflow on the operands)."""
import math

import torch

from health_reference import U as ULP, thread_roundings

PROJECT_REL = 1e-5          # norms and coefficients (test_gpu_optimizer.py)
WAVE, BLOCK = 6, 3


def elem_index(seg, per_segment):
    """per-element value of a per-segment list"""
    return torch.repeat_interleave(torch.tensor(per_segment), torch.diff(torch.tensor(seg)))


def unit_roundings(chunk_lengths):
    """k_unit of the module docstring for a unit cut into chunks of these lengths"""
    nc = len(chunk_lengths)
    return max(thread_roundings(n) for n in chunk_lengths) + WAVE + BLOCK + (math.ceil(nc / 64) - 1) + WAVE


def unit_bounds(chunks, n_units):
    """relative bounds per unit -> (sumsq, norm, coef), each a list of U floats; chunks: rows (start, length, unit, group)"""
    out = ([], [], [])
    for u in range(n_units):
        k = unit_roundings([length for _, length, unit, _ in chunks if unit == u])
        rel_sum = (1.0 + ULP) ** k - 1.0 + 1e-12
        rel_norm = rel_sum / 2.0 + 3.0 * ULP
        out[0].append(rel_sum); out[1].append(rel_norm); out[2].append(rel_norm + 3.0 * ULP)
    return out


def global_norm_bound(chunks, n_units):
    """relative bound of state.grad_norm: the worst unit's chain, then the sum of the unit sums"""
    k = max(unit_roundings([length for _, length, unit, _ in chunks if unit == u]) for u in range(n_units))
    k += (math.ceil(n_units / 256) - 1) + WAVE + BLOCK
    return ((1.0 + ULP) ** k - 1.0 + 1e-12) / 2.0 + 3.0 * ULP


def clip_ref64(g, elem_unit, unit_max_norm, grad_scale=1.0):
    """g: float64 [n]; elem_unit: int64 [n]; unit_max_norm: the max_norm of every unit's group -> (norms [U], coefs [U], global norm),
    python floats in float64"""
    U = len(unit_max_norm)
    sums = torch.zeros(U, dtype=torch.float64).index_add_(0, elem_unit, g * g)
    norms = [math.sqrt(float(s)) / grad_scale for s in sums]
    coefs = [(min(1.0, mn / (nu + 1e-6)) if mn is not None and mn > 0 else 1.0) / grad_scale for nu, mn in zip(norms, unit_max_norm)]
    return norms, coefs, math.sqrt(float(sums.sum())) / grad_scale


def adamw_ref64(p, g, m, v, cols, step, coef_elem):
    """float64 torch.optim.AdamW with per-element lr, b1, b2, eps, wd (cols: float64 [5, n]) on the gradient coef_elem * g"""
    lr, b1, b2, eps, wd = cols
    gg = g * coef_elem
    p = p * (1.0 - lr * wd)
    m = m + (gg - m) * (1.0 - b1)
    v = v * b2 + gg * gg * (1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / bc2.sqrt() + eps)
    return p, m, v


def unit_step_ref64(p, g, m, v, cols, step, elem_unit, unit_max_norm, grad_scale=1.0):
    """one step of the unit modes in float64 -> (p, m, v, norms, coefs, global norm)"""
    norms, coefs, total = clip_ref64(g, elem_unit, unit_max_norm, grad_scale)
    p, m, v = adamw_ref64(p, g, m, v, cols, step, torch.tensor(coefs, dtype=torch.float64)[elem_unit])
    return p, m, v, norms, coefs, total


def torch_units(mode, groups, flat_order):
    """the clip units of a torch twin: [(params, max_norm)] in unit order -- the groups in group mode, the parameters in
    flat-buffer order (``flat_order``: the twin's parameters in that order) in parameter mode"""
    if mode == "group":
        return [(list(g["params"]), g["max_norm"]) for g in groups]
    owner = {id(p): g["max_norm"] for g in groups for p in g["params"]}
    return [([p], owner[id(p)]) for p in flat_order]


def clip_units_torch(units):
    """per-unit torch.nn.utils.clip_grad_norm_ on the twin's gradients, in place -> the pre-clip norms"""
    norms = []
    for params, mn in units:
        if mn is not None and mn > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, mn)))
        else:
            norms.append(float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))))
    return norms
