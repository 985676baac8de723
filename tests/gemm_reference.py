"""Host-side references, limits and buffer helpers for the bf16 GEMMs (hri-emo_amd/csrc/gemm.hip): no GPU needed.

A case is described in LOGICAL form, whatever the storage layout: A [M, K] and B [K, N] float64 made from bf16 values (so every
product is exact in float64), bias [N] (fp32 values) or None, aux [M, N] (bf16 values) or None, c0 [M, N] (fp32 values: the
destination of an accumulating call) or None, and the epilogue of include/hriemo.h:

    acc = A . B        y = acc (+ bias) (+ aux: epilogue 3) (+ c0)
    bf16 output:  round y to nearest, then ReLU (1) or multiply by (aux > 0) (2)          fp32 output: y

reference()   y in float64 (exact up to the float64 sum) and mag = |A| . |B| (+ |bias| + |aux| + |c0|), masked like y.
yardsticks()  the same in fp32 on the CPU, accumulated in several orders (ORDERS, plus "splitk" when the plan splits K: slabs of
              k_per_split summed in slice order, bias on slab 0, c0 last -- what splitk_reduce_kernel documents).  The ENVELOPE of
              a statistic is its maximum over these orders.
check()       the limits, all from the reference alone (docstring there).

Buffers: Guarded puts a logical [R, C] matrix into a larger allocation whose every other byte is 0xFF (bf16 / fp32 NaN):
padding columns (ld = C + 8j) and guard rows before and after.  A kernel that READS outside the logical operand turns its result
non-finite (check() refuses that), one that WRITES outside the logical result changes a guard byte (Guarded.assert_intact)."""
import torch

U = 2.0 ** -8            # bf16 unit roundoff
V = 2.0 ** -24           # fp32 unit roundoff
TILE_M, TILE_N = 256, 128
TILE_FACTOR = 3.0        # attn_reference.TILE_FACTOR
SHARE_FACTOR = 4.0       # bf16 agreement: cap = 4 x the yardstick orders' own disagreement + 8 elements
SHARE_SLACK = 8
SHARE_MAX = 0.01         # ... and never more than 1 % of the elements
ORDERS = ("torch", "seq32", "rev64")

# tile configurations of gemm.hip (kCfg): cfg -> (bm, bn, ring depth ns, bk)
TILES = {0: (128, 128, 2, 64), 1: (256, 128, 3, 64), 2: (256, 256, 2, 64), 3: (64, 128, 4, 64), 4: (256, 256, 4, 32),
         5: (320, 128, 2, 64), 6: (64, 128, 6, 64), 7: (32, 128, 7, 64), 8: (32, 64, 6, 64), 9: (256, 128, 3, 64)}
LAYOUTS = {"NT": (0, 0), "NN": (0, 1), "TN": (1, 1)}


def bf16_round(x):
    return x.float().bfloat16()


def bf16_trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (what a faulty convert does)"""
    bits = x.float().contiguous().view(torch.int32)
    return ((bits >> 16) << 16).view(torch.float32).bfloat16()


def bf16_ordinal(x):
    """bf16 -> int32 that is monotonic in the value (+0 and -0 both 0): adjacent bf16 values differ by 1"""
    b = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


# ------------------------------------------------------------------------------------------------ reference and yardsticks
def _mask(aux):
    return (aux > 0).to(aux.dtype)


def reference(A, B, bias=None, aux=None, epi=0, c0=None, out_f32=False):
    """(ref, mag), float64.  ReLU is 1-Lipschitz and the mask exact, so both leave the limit |err| <= f(mag) valid."""
    A, B = A.double(), B.double()
    y, mag = A @ B, A.abs() @ B.abs()
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    if epi == 3:
        y, mag = y + aux.double(), mag + aux.double().abs()
    if c0 is not None:
        y, mag = y + c0.double(), mag + c0.double().abs()
    if not out_f32:
        if epi == 1:
            y = y.clamp(min=0)
        if epi == 2:
            y, mag = y * _mask(aux.double()), mag * _mask(aux.double())
    return y, mag


def _kchunks(K, step, lo=0, hi=None):
    hi = K if hi is None else hi
    return [(k, min(k + step, hi)) for k in range(lo, hi, step)]


def accumulate(A32, B32, order, k_per_split=None, bias=None, step_hook=None):
    """A . B in fp32.  order: 'torch' (one matmul), 'seq32' (32-deep chunks of K in turn), 'rev64' (64-deep chunks, last first),
    'splitk' (slabs of k_per_split, each in 64-deep chunks, slab 0 carries the bias, slabs summed in slice order).
    step_hook(acc) -> acc after every chunk (the host test's faulty kernels round there).  Returns (acc, bias_applied)."""
    K = A32.shape[1]
    hook = step_hook or (lambda a: a)

    def run(chunks):
        acc = None
        for lo, hi in chunks:
            part = A32[:, lo:hi] @ B32[lo:hi]
            acc = hook(part if acc is None else acc + part)
        return acc
    if order == "torch":
        return hook(A32 @ B32), False
    if order == "seq32":
        return run(_kchunks(K, 32)), False
    if order == "rev64":
        return run(_kchunks(K, 64)[::-1]), False
    if order == "splitk":
        total = None
        for s, (lo, hi) in enumerate(_kchunks(K, k_per_split)):
            slab = run(_kchunks(K, 64, lo, hi))
            if s == 0 and bias is not None:
                slab = slab + bias
            total = slab if total is None else total + slab
        return total, bias is not None
    raise ValueError(order)


def finish(acc, bias=None, aux=None, epi=0, c0=None, out_f32=False, convert=bf16_round):
    """the epilogue on an fp32 accumulator: fp32 adds in the kernels' order, ONE rounding, then ReLU / mask on the rounded value"""
    y = acc
    if bias is not None:
        y = y + bias.float()
    if epi == 3:
        y = y + aux.float()
    if c0 is not None:
        y = y + c0.float()
    if out_f32:
        return y
    y = convert(y)
    if epi == 1:
        y = y.clamp(min=0)
    if epi == 2:
        y = y * _mask(aux.float()).bfloat16()
    return y


def yardsticks(A, B, bias=None, aux=None, epi=0, c0=None, out_f32=False, k_per_split=None):
    """{order: result in the output type}; 'torch' first.  k_per_split < K adds the split-K order."""
    A32, B32 = A.float(), B.float()
    b32 = None if bias is None else bias.float()
    orders = ORDERS + (("splitk",) if k_per_split is not None and k_per_split < A.shape[1] else ())
    out = {}
    for o in orders:
        acc, biased = accumulate(A32, B32, o, k_per_split, b32)
        out[o] = finish(acc, None if biased else b32, aux, epi, c0, out_f32)
    return out


# ------------------------------------------------------------------------------------------------ limits
def _tile_norms(x):
    M, N = x.shape
    tm, tn = (M + TILE_M - 1) // TILE_M, (N + TILE_N - 1) // TILE_N
    pad = torch.zeros(tm * TILE_M, tn * TILE_N, dtype=torch.float64)
    pad[:M, :N] = x
    return pad.reshape(tm, TILE_M, tn, TILE_N).pow(2).sum(dim=(1, 3)).sqrt()


def share_cap(yards):
    """largest share of elements on which the bf16 results of two yardstick orders differ"""
    ys = list(yards.values())
    worst = 0.0
    for i in range(len(ys)):
        for j in range(i + 1, len(ys)):
            worst = max(worst, (bf16_ordinal(ys[i]) != bf16_ordinal(ys[j])).double().mean().item())
    return worst


def ratios(got, ref, mag, yards, K, out_f32):
    """statistics of `got`, each as a fraction of its limit (<= 1 passes); a non-finite value in `got` yields inf everywhere.
    bf16: {'elem', 'share' (differing elements / cap), 'adjacent' (largest bf16 distance to the torch-order yardstick)}
    fp32: {'elem', 'tile'}"""
    g = got.double()
    if not torch.isfinite(g).all():
        return {"elem": float("inf"), "tile": float("inf"), "share": float("inf"), "adjacent": float("inf")}
    err = (g - ref).abs()
    lim = (K + 2) * V * mag + (0.0 if out_f32 else U * ref.abs())
    bad = err > lim                                        # (a zero limit demands an exact result)
    elem = (err / lim.clamp(min=1e-300))[lim > 0].max().item() if (lim > 0).any() else 0.0
    if (bad & (lim == 0)).any():
        elem = float("inf")
    if out_f32:
        env = None
        for y in yards.values():
            n = _tile_norms(y.double() - ref)
            env = n if env is None else torch.maximum(env, n)
        tl = TILE_FACTOR * env + V * _tile_norms(ref)
        tile = (_tile_norms(g - ref) / tl.clamp(min=1e-300)).max().item()
        return {"elem": elem, "tile": tile}
    yard = next(iter(yards.values()))
    dist = (bf16_ordinal(got.bfloat16()) - bf16_ordinal(yard)).abs()
    # two fp32 accumulations a, b of the same sum differ by at most D = 2 (K+2) v mag before the rounding.  Where the result
    # cancels to less than that, D spans several bf16 steps, and then |bf16(a) - bf16(b)| <= 2 |a - b| <= 2 D (s >= 2 steps of
    # width h apart means |a - b| >= (s - 1) h >= s h / 2): only such pairs may be more than one step apart.
    dist = torch.where((dist > 1) & ((g - yard.double()).abs() <= 4 * (K + 2) * V * mag), torch.ones_like(dist), dist)
    n = got.numel()
    cap = min(SHARE_FACTOR * share_cap(yards) * n + SHARE_SLACK, SHARE_MAX * n)
    return {"elem": elem, "share": (dist != 0).sum().item() / cap, "adjacent": float(dist.max().item())}


def check(got, ref, mag, yards, K, out_f32, name):
    """got: the kernel's [M, N] result (CPU).  With u = 2^-8, v = 2^-24:
      finite       every value (an element of poisoned padding that was read, or a result element never stored, is NaN)
      elementwise  bf16: |got - ref| <= u |ref| + (K+2) v mag      fp32: |got - ref| <= (K+2) v mag
                   (fp32 accumulation of K exact products in ANY order errs by at most K v mag, bias and aux / c0 add two
                   roundings, the final round-to-nearest u |y|; mag == 0 -- masked elements -- demands exact zeros)
      bf16         elements where got != bf16(torch-order yardstick): at most 4 x the largest share on which two yardstick
                   orders disagree among themselves + 8 elements, never more than 1 %; every differing pair adjacent bf16 values
                   (or, where the sum cancels below the fp32 discrepancy itself, within 4 (K+2) v mag: see ratios())
      fp32         per 256 x 128 tile ||got - ref|| <= 3 * envelope(||yard - ref||) + v ||ref||
    Returns the ratios (statistic / limit) after asserting every one is <= 1."""
    assert torch.isfinite(ref).all() and torch.isfinite(mag).all(), (name, "reference is not finite")
    assert torch.isfinite(got.double()).all(), f"{name}: {int((~torch.isfinite(got.double())).sum())} non-finite results (poison read or element not stored)"
    r = ratios(got, ref, mag, yards, K, out_f32)
    assert r["elem"] <= 1.0, f"{name}: elementwise error is {r['elem']:.3g} x its limit"
    if out_f32:
        assert r["tile"] <= 1.0, f"{name}: per-tile error is {r['tile']:.3g} x its limit 3*env|yard-ref| + v*|ref|"
    else:
        assert r["adjacent"] <= 1.0, f"{name}: differs from the fp32 yardstick by {r['adjacent']:.0f} bf16 steps"
        assert r["share"] <= 1.0, f"{name}: elements that differ from the fp32 yardstick are {r['share']:.3g} x the cap"
    return r


# ------------------------------------------------------------------------------------------------ inputs
def make_case(M, N, K, seed, bias=False, epi=0, c0=False):
    """real-valued logical operands: A = 0.5 randn, B = randn / sqrt(K), bias = 0.1 randn, aux = randn with +0.0, -0.0 and the
    smallest positive bf16 normal planted in every row (what epilogue 2's `aux > 0` has to tell apart), c0 = randn."""
    g = torch.Generator().manual_seed(seed)
    case = {"A": (0.5 * torch.randn(M, K, generator=g)).bfloat16(), "B": (torch.randn(K, N, generator=g) / K ** 0.5).bfloat16(),
            "bias": 0.1 * torch.randn(N, generator=g) if bias else None, "aux": None, "c0": None, "epi": epi}
    if epi >= 2:
        aux = torch.randn(M, N, generator=g).bfloat16()
        cols = torch.randint(0, N, (M, 3), generator=g)
        rows = torch.arange(M)
        aux[rows, cols[:, 0]] = 0.0
        aux[rows, cols[:, 1]] = -0.0
        aux[rows, cols[:, 2]] = 2.0 ** -126
        case["aux"] = aux
    if c0:
        case["c0"] = torch.randn(M, N, generator=g)
    return case


def edge_shapes(cfg, ta):
    """(Ms, Ns, Ks, K_fallback) around the tile of a configuration: M one past a tile / 7 short of two / three full tiles
    (8 past / 8 short for a transposed A, whose M must be a multiple of 8), N 8 past one tile / 8 short of two, K whose last 64-deep K-step holds 8, 56 and 32 valid
    k.  K_fallback: the longest K the configuration's ring cannot stream ((ns-2)*bk; None for 2-deep rings) -- the library must
    report configuration 0 for it."""
    bm, bn, ns, bk = TILES[cfg]
    return ([bm + 8, 2 * bm - 8, 3 * bm] if ta else [bm + 1, 2 * bm - 7, 3 * bm], [bn + 8, 2 * bn - 8], [(ns - 1) * 64 + 8, (ns - 1) * 64 + 56, 5 * 64 + 32],
            (ns - 2) * bk if ns > 2 else None)


# ------------------------------------------------------------------------------------------------ buffers
GUARD_ROWS = 320          # one tile of the tallest configuration (5: 320 x 128)


class Guarded:
    """[rows, cols] of `dtype` inside an allocation of (rows + 2 * guard) x (cols + 8 * j) elements; every byte outside the
    logical matrix -- and, until set() / a kernel writes it, inside -- is 0xFF.  .view is the logical matrix (16-byte aligned,
    row stride .ld), .ptr its address."""

    def __init__(self, rows, cols, dtype, j=1, guard=GUARD_ROWS, device="cpu"):
        assert j >= 0 and cols % 4 == 0      # (j = 0: matrices the ABI gives no leading dimension, guard rows only)
        self.rows, self.cols, self.ld, self.guard = rows, cols, cols + 8 * j, guard
        self.es = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((rows + 2 * guard) * self.ld * self.es,), 0xFF, dtype=torch.uint8, device=device)
        self.full = self.raw.view(dtype).view(rows + 2 * guard, self.ld)
        self.view = self.full[guard:guard + rows, :cols]
        assert self.view.data_ptr() % 16 == 0 and (self.ld * self.es) % 16 == 0

    @classmethod
    def of(cls, x, **kw):
        """a poisoned, guarded copy of the 2-D (or 1-D: one row) tensor x on kw['device']"""
        x2 = x if x.dim() == 2 else x[None]
        b = cls(x2.shape[0], x2.shape[1], x.dtype, **kw)
        b.view.copy_(x2)
        return b

    @property
    def ptr(self):
        return self.view.data_ptr()

    def violations(self):
        """number of bytes outside the logical matrix that are no longer 0xFF"""
        by = self.raw.view(self.rows + 2 * self.guard, self.ld * self.es)
        g, w = self.guard, self.cols * self.es
        return int((by[:g] != 0xFF).sum() + (by[g + self.rows:] != 0xFF).sum() + (by[g:g + self.rows, w:] != 0xFF).sum())

    def assert_intact(self, name):
        n = self.violations()
        assert n == 0, f"{name}: {n} bytes outside the logical [{self.rows}, {self.cols}] matrix were written"
