"""Float64 reference and counted error bound of a health-log record (csrc/health.hip, hri_emo_amd.optim.HealthLog).

A record's per-parameter fields, for the slot [start, start + length) of parameter i in the flat buffers:
    grad_sq[i]   = sum of (g / grad_scale)^2 over the FINITE elements g of the gradient slot
    nonfinite[i] = number of NaN / +-Inf elements of the gradient slot (exact)
    weight_sq[i] = sum of p^2, p the parameter AFTER the update
    update_sq[i] = sum of d^2, d = step_size * m / (sqrt(v) * isb2 + eps) with the moments AFTER the update and the scalars of the
                   group that owns the parameter: step_size = lr / (1 - beta1^t), isb2 = 1 / sqrt(1 - beta2^t)
record_ref64 evaluates them in float64 from whatever p, m, v and scalars it is handed:
    * the kernel's own fp32 buffers and the fp32 words of state[] / hyper[] (scalars_from_state): then the ONLY difference to the
      kernel is the kernel's own arithmetic, which record_bound counts below -- the pairing the GPU tests assert;
    * a float64 replay of clip + torch.optim.AdamW (replay_adamw64, scalars_adamw64), or the state of a real torch.optim.AdamW
      (from_torch_adamw): an independent route to the same numbers, checked against each other on the CPU
      (test_optimizer_health_host.py).

The bound, counted from the kernel's summation tree.  u = 2^-24 (fp32 round to nearest).  Every sum is a sum of squares, so all
terms are >= 0 and a term that passes through k roundings on its way into the result contributes at most ((1 + u)^k - 1) times
itself: |got - exact| <= ((1 + u)^k - 1) * exact, k the LONGEST chain of roundings any term passes through:
    per thread    a thread owns vectors tid, tid + 256, ... of its chunk and adds their elements one after the other with
                  fmaf(x, x, acc) -- the square is exact inside the fma, one rounding per element:
                  T = 4 * ceil(ceil(len / 4) / 256) roundings for the chunk length len (T = chunk / 256 for a full chunk)
    wave          6 steps of the xor butterfly over 64 lanes                                                  6 roundings
    block         the four wave sums in index order                                                           3 roundings
    fold          the nc chunk partials of the parameter in chunk order (the first one is added to 0: exact)  nc - 1 roundings
    grad_sq only  1 / (gs * gs): one product, one quotient; times the sum                                     3 roundings
    update_sq only the term d itself, per element: sqrtf (1 ulp = 2 u allowed), * isb2 (u), + eps (u; both addends positive, so
                  their relative errors carry over at most), step_size * m (u), the quotient (1 ulp = 2 u allowed): 7 u on d,
                  (1 + u)^14 on d^2 -- counted as 14 roundings.  A compiler that contracts the product and the sum into one fma
                  only removes roundings.
    k(grad_sq) = T + 6 + 3 + (nc - 1) + 3,  k(weight_sq) = T + 6 + 3 + (nc - 1),  k(update_sq) = 14 + T + 6 + 3 + (nc - 1)
For the test layout (chunk 32768: T = 128; nc <= 4) that is k <= 154: a relative bound of 9.2e-6 on a sum whose float64 value is
known to 1e-13.  The derivation assumes no squared term underflows: the operands the tests draw keep every non-zero |x| >= 2^-60
(assert_no_underflow).  The float64 reference itself rounds with 2^-53 per operation: negligible, and added as 1e-12 relative.

Measured on MI355X (test_gpu_optimizer_health.py prints them): worst relative error 2.1e-7, worst error / bound 0.13 over all records
of the kernel tests."""
import math

import torch

U = 2.0 ** -24
THREADS = 256
TERM_ROUNDINGS = 14        # update_sq: roundings counted on d^2 (see above)
SCALE_ROUNDINGS = 3        # grad_sq: 1 / (gs * gs) and the product
WAVE_ROUNDINGS, BLOCK_ROUNDINGS = 6, 3


def pad64(n):
    return (n + 63) // 64 * 64


def slots_of(numels):
    """[(start, padded length)] of parameters laid out one behind the other the way GradBuckets does"""
    out, off = [], 0
    for n in numels:
        out.append((off, pad64(n)))
        off += pad64(n)
    return out, off


def thread_roundings(length):
    """T of the module docstring for a chunk of `length` elements"""
    return 4 * math.ceil(math.ceil(length / 4) / THREADS)


def roundings(length, chunk):
    """(k_grad, k_weight, k_update) for a slot of `length` elements cut into chunks of `chunk`"""
    nc = math.ceil(length / chunk)
    t = thread_roundings(min(length, chunk))
    tree = t + WAVE_ROUNDINGS + BLOCK_ROUNDINGS + (nc - 1)
    return tree + SCALE_ROUNDINGS, tree, tree + TERM_ROUNDINGS


def record_bound(ref, slots, chunk):
    """absolute bounds {field: float64 [P]} for the float64 record `ref` (record_ref64) of these slots"""
    ks = [roundings(length, chunk) for _, length in slots]
    out = {}
    for j, field in enumerate(("grad_sq", "weight_sq", "update_sq")):
        rel = torch.tensor([(1.0 + U) ** k[j] - 1.0 + 1e-12 for k in ks], dtype=torch.float64)
        out[field] = rel * ref[field]
    return out


def assert_no_underflow(*tensors):
    for t in tensors:
        x = t.double().abs()
        x = x[torch.isfinite(x) & (x > 0)]
        assert x.numel() == 0 or float(x.min()) >= 2.0 ** -60, "an operand whose square leaves fp32's normal range: the bound does not cover it"


def scalars_from_state(state, hyper, G):
    """the fp32 words the kernel reads, as float64: [(step_size, isb2, eps)] per group"""
    s, h = state.detach().cpu().double().reshape(-1), hyper.detach().cpu().double().reshape(-1)
    return [(float(s[8 * g + 3]), float(s[8 * g + 4]), float(h[8 * g + 3])) for g in range(G)]


def scalars_adamw64(groups, t):
    """float64 from the hyper-parameters: groups = [(lr, beta1, beta2, eps)], t the step count of the update"""
    return [(lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), eps) for lr, b1, b2, eps in groups]


def record_ref64(g, p, m, v, slots, groups_of, scalars, grad_scale=1.0, real=True):
    """g, p, m, v: flat buffers (any float dtype, any device); slots: [(start, length)] per parameter; groups_of: the group index per
    parameter; scalars: [(step_size, isb2, eps)] per group.  real=False: a skipped record (weight_sq = update_sq = 0)."""
    g, p, m, v = (None if t is None else t.detach().cpu().double() for t in (g, p, m, v))
    P = len(slots)
    out = {"grad_sq": torch.zeros(P, dtype=torch.float64), "nonfinite": torch.zeros(P, dtype=torch.int64),
           "weight_sq": torch.zeros(P, dtype=torch.float64), "update_sq": torch.zeros(P, dtype=torch.float64)}
    for i, (start, length) in enumerate(slots):
        gi = g[start:start + length]
        fin = torch.isfinite(gi)
        out["nonfinite"][i] = int((~fin).sum())
        x = torch.where(fin, gi, torch.zeros_like(gi)) / grad_scale
        out["grad_sq"][i] = (x * x).sum()
        if real:
            step_size, isb2, eps = scalars[groups_of[i]]
            pi, mi, vi = (t[start:start + length] for t in (p, m, v))
            d = step_size * mi / (vi.sqrt() * isb2 + eps)
            out["weight_sq"][i] = (pi * pi).sum()
            out["update_sq"][i] = (d * d).sum()
    return out


def replay_adamw64(p, g, m, v, slots, groups_of, groups, t, max_norm, grad_scale=1.0):
    """float64 clip_grad_norm_(max_norm) + torch.optim.AdamW (decoupled decay) of step t over the flat buffers; groups =
    [(lr, beta1, beta2, eps, weight_decay)].  -> (p, m, v, norm)"""
    p, g, m, v = (x.detach().cpu().double().clone() for x in (p, g, m, v))
    norm = math.sqrt(float((g * g).sum())) / grad_scale
    coef = (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0) / grad_scale
    for i, (start, length) in enumerate(slots):
        lr, b1, b2, eps, wd = groups[groups_of[i]]
        sl = slice(start, start + length)
        gg = g[sl] * coef
        p[sl] *= 1.0 - lr * wd
        m[sl] += (gg - m[sl]) * (1.0 - b1)
        v[sl] = v[sl] * b2 + gg * gg * (1.0 - b2)
        p[sl] -= lr / (1.0 - b1 ** t) * m[sl] / (v[sl].sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v, norm


def from_torch_adamw(opt, params, grads):
    """the record of the step a real torch.optim.AdamW has just taken, from ITS state: params in flat-buffer order, grads the
    gradients it stepped on.  -> record_ref64's dict (every parameter packed into its own 64-padded slot)"""
    slots, total = slots_of([q.numel() for q in params])
    flat = {k: torch.zeros(total, dtype=torch.float64) for k in "gpmv"}
    groups_of, groups = [], []
    for gi, group in enumerate(opt.param_groups):
        groups.append((group["lr"], group["betas"][0], group["betas"][1], group["eps"]))
    owner = {id(q): gi for gi, group in enumerate(opt.param_groups) for q in group["params"]}
    t = None
    for (start, _), q, gr in zip(slots, params, grads):
        st = opt.state[q]
        t = int(st["step"])
        n = q.numel()
        flat["g"][start:start + n] = gr.detach().double().reshape(-1)
        flat["p"][start:start + n] = q.detach().double().reshape(-1)
        flat["m"][start:start + n] = st["exp_avg"].double().reshape(-1)
        flat["v"][start:start + n] = st["exp_avg_sq"].double().reshape(-1)
        groups_of.append(owner[id(q)])
    return record_ref64(flat["g"], flat["p"], flat["m"], flat["v"], slots, groups_of, scalars_adamw64(groups, t))
