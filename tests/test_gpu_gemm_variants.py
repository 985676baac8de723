"""GPU suite, GEMM kernels through the C-ABI on real-valued operands (gemm_reference.py: float64 reference, limits from the
reference and the fp32 yardstick orders alone), every operand inside poisoned padding and guard rows, every result inside guards:

  1. every tile configuration forced in turn x layout x output type x epilogue at shapes that straddle the tile edges
  2. the shapes the BASELINE configurations launch, with the configuration / split-K each is expected to take (hriemo_gemm_plan)
  3. split-K against the workspace it is given; the split output; bit-identical repeats
  4. the grouped weight-gradient launch and the masked dX + column sums call
  5. NaN / Inf stay in their row
  6. hriemo_gemm_ln_fwd inside guards
  7. the work queue of configuration 9 inside a training step (eager and captured) and inside a two-stream graph

The integer tests of test_gpu_kernels.py stay the instrument for layout faults (a permuted fragment); these find what is exact
on small integers: rounding, the order of the epilogue's operations, reads past an operand's edge, stores past a result's."""
import ctypes
import json
import math
import os

import pytest
import torch

import gemm_reference as G

pytestmark = pytest.mark.gpu

WS_BYTES = 64 << 20
WORST = {}                 # (layout, output type) -> {statistic: worst ratio to its limit seen in this run}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    yield _lib.lib()
    table = {f"{k[0]} {k[1]}": v for k, v in sorted(WORST.items())}
    print("\nworst ratio to the limit, per layout and output type:\n" + json.dumps(table, indent=1))
    if os.environ.get("HRIEMO_GEMM_RATIOS"):
        with open(os.environ["HRIEMO_GEMM_RATIOS"], "w") as f:
            json.dump(table, f, indent=1)


@pytest.fixture
def forced(L):
    """force(cfg, flags): tile configuration and flag word for the test, restored afterwards"""
    prev = L.hriemo_gemm_debug_flags(9)
    L.hriemo_gemm_debug_flags(prev)

    def force(cfg, flags=None):
        L.hriemo_gemm_force_config(cfg)
        L.hriemo_gemm_debug_flags(prev if flags is None else flags)
    yield force
    L.hriemo_gemm_force_config(-1)
    L.hriemo_gemm_debug_flags(prev)


def call(name, *args):
    from hri_emo_amd import _lib
    _lib.call(name, *args)


def stream():
    return torch.cuda.current_stream().cuda_stream


def plan(ta, tb, M, N, K, f32, ws_bytes=0):
    c, s, k = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    call("hriemo_gemm_plan", ta, tb, M, N, K, int(f32), ws_bytes, ctypes.byref(c), ctypes.byref(s), ctypes.byref(k))
    return c.value, s.value, k.value


def note(layout, out_f32, r):
    w = WORST.setdefault((layout, "fp32" if out_f32 else "bf16"), {})
    for k, v in r.items():
        if k != "adjacent":
            w[k] = round(max(w.get(k, 0.0), v), 4)


def ptr(b):
    return None if b is None else b.ptr


def run_case(layout, case, out_f32=False, colsum=False, ws_bytes=WS_BYTES, rows=None, twice=False, name="", split_m=None):
    """One GEMM call on guarded, poisoned buffers, judged by gemm_reference.check.  case: logical operands (make_case).
    rows: judge these output rows only (guards and finiteness still cover the whole result).  split_m: hriemo_gemm_bf16_split.
    Returns (plan, ratios)."""
    ta, tb = G.LAYOUTS[layout]
    (M, K), N = case["A"].shape, case["B"].shape[1]
    epi, acc = case["epi"], case["c0"] is not None
    ws_bytes = ws_bytes if out_f32 else 0
    pl = plan(ta, tb, M, N, K, out_f32, ws_bytes)
    cfg, splitk, kper = pl
    dev = "cuda"
    A = G.Guarded.of(case["A"].t().contiguous() if ta else case["A"], j=1, device=dev)
    B = G.Guarded.of(case["B"] if tb else case["B"].t().contiguous(), j=2, device=dev)
    aux = None if case["aux"] is None else G.Guarded.of(case["aux"], j=3, device=dev)
    bias = None if case["bias"] is None else G.Guarded.of(case["bias"], guard=2, device=dev)
    ws = G.Guarded(1, splitk * M * N, torch.float32, guard=1, device=dev) if ws_bytes > 0 else None
    part = None
    dt = torch.float32 if out_f32 else torch.bfloat16
    bufs = {"A": A, "B": B, "aux": aux, "bias": bias, "workspace": ws}
    if split_m is None:
        Cs = [G.Guarded(M, N, dt, j=1, device=dev)]
    else:
        Cs = [G.Guarded(split_m, N, dt, j=1, device=dev), G.Guarded(M - split_m, N, dt, j=2, device=dev)]
    if colsum:
        prow = L_colsum_rows(ta, tb, M, N, K)
        part = G.Guarded(prow, N, torch.float32, j=0, device=dev)      # [rows][N]: the ABI gives the partials no leading dimension
        bufs["column-sum partials"] = part

    def launch():
        if acc:
            c0 = case["c0"].to(dev)
            Cs[0].view.copy_(c0 if split_m is None else c0[:split_m])
            if split_m is not None:
                Cs[1].view.copy_(c0[split_m:])
        else:
            for c in Cs:
                c.view.fill_(float("nan"))
        if colsum:
            call("hriemo_gemm_bf16_colsum", ta, tb, M, N, K, A.ptr, A.ld, B.ptr, B.ld, Cs[0].ptr, Cs[0].ld, aux.ptr, aux.ld, part.ptr, stream())
        elif split_m is not None:
            call("hriemo_gemm_bf16_split", ta, tb, M, N, K, A.ptr, A.ld, B.ptr, B.ld, Cs[0].ptr, Cs[0].ld, Cs[1].ptr, Cs[1].ld, split_m,
                 int(acc), ptr(ws), ws_bytes, stream())
        else:
            call("hriemo_gemm_bf16", ta, tb, M, N, K, A.ptr, A.ld, B.ptr, B.ld, Cs[0].ptr, Cs[0].ld, int(out_f32), ptr(bias), epi,
                 ptr(aux), aux.ld if aux is not None else 0, int(acc), ptr(ws), ws_bytes, stream())
        torch.cuda.synchronize()
        for n, b in list(bufs.items()) + [(f"C{i}", c) for i, c in enumerate(Cs)]:
            if b is not None:
                b.assert_intact(f"{name}: {n}")
        return torch.cat([c.view for c in Cs]).cpu()
    got = launch()
    if twice:
        assert torch.equal(launch(), got), f"{name}: not bit-identical from run to run"
    assert torch.isfinite(got.double()).all(), f"{name}: non-finite results (poison read or element not stored)"
    stored = got.double()
    sub = dict(case)
    if rows is not None:
        sub.update({k: case[k][rows] for k in ("A", "aux", "c0") if case[k] is not None})
        got = got[rows]
    ref, mag = G.reference(sub["A"], sub["B"], sub["bias"], sub["aux"], epi, sub["c0"], out_f32)
    yards = G.yardsticks(sub["A"], sub["B"], sub["bias"], sub["aux"], epi, sub["c0"], out_f32, kper if splitk > 1 else None)
    r = G.check(got, ref, mag, yards, K, out_f32, name)
    note(layout, out_f32, r)
    if colsum:
        p = part.view.double().cpu()
        assert torch.isfinite(p).all(), f"{name}: a column-sum partial was not written"
        lim = (M + 2) * G.V * stored.abs().sum(0)              # fp32 sums of M stored values in any order
        assert ((p.sum(0) - stored.sum(0)).abs() <= lim).all(), f"{name}: column sums of the stored values"
    return pl, r


def L_colsum_rows(ta, tb, M, N, K):
    from hri_emo_amd import _lib
    return _lib.lib().hriemo_gemm_colsum_rows(ta, tb, M, N, K)


def sample_rows(M, seed):
    """all rows when the result is small; else the first tile's rows, the last (ragged) tile's rows and 512 random rows"""
    if M <= 2048:
        return None
    g = torch.Generator().manual_seed(seed)
    mid = torch.randperm(M - 512, generator=g)[:512] + 256
    return torch.cat([torch.arange(256), mid.sort().values, torch.arange(M - 256, M)])


# ------------------------------------------------------------------------------------------------ 1. forced configurations
# (name, out_f32, bias, epilogue, accumulate, column sums)
COMBOS = [("bf16", False, False, 0, False, False), ("bf16+bias", False, True, 0, False, False), ("relu", False, True, 1, False, False),
          ("mask", False, False, 2, False, False), ("mask+colsum", False, False, 2, False, True), ("residual", False, True, 3, False, False),
          ("fp32", True, False, 0, False, False), ("fp32+bias", True, True, 0, False, False), ("fp32+acc", True, False, 0, True, False),
          ("fp32+bias+acc", True, True, 0, True, False)]


def built(cfg, layout, out_f32):
    """does launch_gemm build this configuration for the layout / output type (otherwise the library falls back by design)"""
    ta, tb = G.LAYOUTS[layout]
    if cfg == 5:
        return ta == 0 and not out_f32
    if cfg in (3, 6, 7, 8) and ta == 1:
        return False
    return not (cfg == 8 and tb == 1)


FORCED = [(c, 9) for c in range(10)] + [(9, 1)]


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("cfg,flags", FORCED)
def test_forced_configuration_at_tile_edges(L, forced, cfg, flags, layout):
    """Every epilogue / output type the launcher builds for this configuration and layout, at M one row past a tile, 7 short of
    two tiles and three full tiles, N 8 past and 8 short of a tile, a last K-step of 8, 56 and 32 valid k; one problem with more
    tiles than resident blocks (persistent walk; the work queue for flag word 1); one K too short for the configuration's ring,
    which the plan must report as configuration 0."""
    ta, tb = G.LAYOUTS[layout]
    forced(cfg, flags)
    Ms, Ns, Ks, kfb = G.edge_shapes(cfg, ta)
    ran = 0
    for ci, (cname, out_f32, bias, epi, acc, colsum) in enumerate(COMBOS):
        if not built(cfg, layout, out_f32):
            continue
        for i in range(3):
            M, N, K = Ms[i], Ns[(i + ci) % 2], Ks[(i + ci) % 3]
            name = f"cfg {cfg} flags {flags} {layout} {cname} {M}x{N}x{K}"
            assert plan(ta, tb, M, N, K, out_f32, WS_BYTES if out_f32 else 0)[0] == cfg, f"{name}: the forced configuration does not run"
            case = G.make_case(M, N, K, seed=1000 * cfg + 10 * ci + i, bias=bias, epi=epi, c0=acc)
            run_case(layout, case, out_f32, colsum, name=name)
            ran += 1
    if ran:
        bm, bn, ns, bk = G.TILES[cfg]
        M, N, K = (8456 if ta else 8449), 2056, Ks[0]
        assert -(-M // bm) * -(-N // bn) > 256, "more tiles than CUs"
        for cname, out_f32, bias, epi, acc, colsum in (COMBOS[5], COMBOS[4], COMBOS[9]):
            if built(cfg, layout, out_f32):
                name = f"cfg {cfg} flags {flags} {layout} {cname} {M}x{N}x{K}"
                case = G.make_case(M, N, K, seed=77 + cfg, bias=bias, epi=epi, c0=acc)
                pl, _ = run_case(layout, case, out_f32, colsum, rows=sample_rows(M, cfg), name=name)
                assert pl[0] == cfg, name
        if kfb is not None:
            assert plan(ta, tb, Ms[0], Ns[0], kfb, 0)[0] == 0 and plan(ta, tb, Ms[0], Ns[0], kfb + 8, 0)[0] == cfg
            case = G.make_case(Ms[0], Ns[0], kfb, seed=5, bias=True, epi=1)
            run_case(layout, case, name=f"cfg {cfg} {layout} K = {kfb}: fallback to configuration 0")
    else:
        # nothing of this configuration is built for the layout: the plan says so
        assert plan(ta, tb, Ms[2], Ns[0], Ks[0], 0)[0] != cfg


# ------------------------------------------------------------------------------------------------ 2. BASELINE shapes
def baseline_rows():
    """(layout, M, N, K, what) in hriemo_gemm_bf16's convention for the GEMMs of one step at BASELINE configs[1], [3], [4] (per
    GPU): encoder projections over M = B * T_a and B * T_t rows, the decoder's over B * N_e, the gate's over B."""
    out = []
    for d, rows_enc, m_dec, m_gate in ((768, (25600, 8192), 384, 64), (768, (32000, 1600), 192, 32), (1024, (12800, 4096), 224, 32)):
        for M in rows_enc:
            for N in (d, 3 * d, 2 * d, 4 * d):
                out.append(("NT", M, N, d, "projection"))
                out.append(("NN", M, d, N, "dX of it"))
                out.append(("TN", N, d, M, "dW of it"))
            out += [("NT", M, d, 4 * d, "FFN2"), ("NN", M, 4 * d, d, "dX of FFN2, masked + column sums"), ("TN", d, 4 * d, M, "dW of FFN2")]
        for N, K in ((d, d), (3 * d, d), (2048, d), (d, 2048)):
            out.append(("NT", m_dec, N, K, "decoder"))
            out.append(("NN", m_dec, K, N, "decoder dX"))
        out += [("NT", m_gate, 256, 4 * d, "gate"), ("NN", m_gate, 4 * d, 256, "gate dX")]
    seen, uniq = set(), []
    for r in out:
        if r[:4] not in seen:
            seen.add(r[:4])
            uniq.append(r)
    return uniq


# (layout, M, N, K) -> (configuration, split-K slices) on the MI355X's 256 CUs with a 64 MB workspace
BASELINE_PLAN = {}   # filled below from the table text, one row per line: keeps the table reviewable
_BASELINE_TABLE = """
NT 25600 768 768 9 1
NN 25600 768 768 9 1
TN 768 768 25600 9 14
NT 25600 2304 768 2 1
NN 25600 768 2304 9 1
TN 2304 768 25600 9 4
NT 25600 1536 768 9 1
NN 25600 768 1536 9 1
TN 1536 768 25600 9 7
NT 25600 3072 768 2 1
NN 25600 768 3072 9 1
TN 3072 768 25600 9 3
NT 25600 768 3072 9 1
NN 25600 3072 768 2 1
TN 768 3072 25600 9 3
NT 8192 768 768 9 1
NN 8192 768 768 9 1
TN 768 768 8192 9 13
NT 8192 2304 768 9 1
NN 8192 768 2304 9 1
TN 2304 768 8192 9 4
NT 8192 1536 768 9 1
NN 8192 768 1536 9 1
TN 1536 768 8192 9 7
NT 8192 3072 768 9 1
NN 8192 768 3072 9 1
TN 3072 768 8192 9 3
NT 8192 768 3072 9 1
NN 8192 3072 768 9 1
TN 768 3072 8192 9 3
NT 384 768 768 8 1
NN 384 768 768 7 1
NT 384 2304 768 7 1
NN 384 768 2304 7 1
NT 384 2048 768 7 1
NN 384 768 2048 7 1
NT 384 768 2048 8 1
NN 384 2048 768 7 1
NT 64 256 3072 8 1
NN 64 3072 256 3 1
NT 32000 768 768 9 1
NN 32000 768 768 9 1
TN 768 768 32000 9 14
NT 32000 2304 768 2 1
NN 32000 768 2304 9 1
TN 2304 768 32000 9 4
NT 32000 1536 768 9 1
NN 32000 768 1536 9 1
TN 1536 768 32000 9 7
NT 32000 3072 768 2 1
NN 32000 768 3072 9 1
TN 3072 768 32000 9 3
NT 32000 768 3072 9 1
NN 32000 3072 768 2 1
TN 768 3072 32000 9 3
NT 1600 768 768 9 1
NN 1600 768 768 9 1
TN 768 768 1600 0 5
NT 1600 2304 768 9 1
NN 1600 768 2304 9 1
TN 2304 768 1600 0 4
NT 1600 1536 768 9 1
NN 1600 768 1536 9 1
TN 1536 768 1600 0 5
NT 1600 3072 768 9 1
NN 1600 768 3072 9 1
TN 3072 768 1600 0 3
NT 1600 768 3072 9 1
NN 1600 3072 768 9 1
TN 768 3072 1600 0 3
NT 192 768 768 8 1
NN 192 768 768 7 1
NT 192 2304 768 7 1
NN 192 768 2304 7 1
NT 192 2048 768 7 1
NN 192 768 2048 7 1
NT 192 768 2048 8 1
NN 192 2048 768 7 1
NT 32 256 3072 8 1
NN 32 3072 256 3 1
NT 12800 1024 1024 9 1
NN 12800 1024 1024 9 1
TN 1024 1024 12800 9 8
NT 12800 3072 1024 9 1
NN 12800 1024 3072 9 1
TN 3072 1024 12800 9 2
NT 12800 2048 1024 9 1
NN 12800 1024 2048 9 1
TN 2048 1024 12800 9 4
NT 12800 4096 1024 9 1
NN 12800 1024 4096 9 1
TN 4096 1024 12800 9 2
NT 12800 1024 4096 9 1
NN 12800 4096 1024 9 1
TN 1024 4096 12800 9 2
NT 4096 1024 1024 9 1
NN 4096 1024 1024 9 1
TN 1024 1024 4096 9 8
NT 4096 3072 1024 9 1
NN 4096 1024 3072 9 1
TN 3072 1024 4096 9 2
NT 4096 2048 1024 9 1
NN 4096 1024 2048 9 1
TN 2048 1024 4096 9 4
NT 4096 4096 1024 9 1
NN 4096 1024 4096 9 1
TN 4096 1024 4096 9 2
NT 4096 1024 4096 9 1
NN 4096 4096 1024 9 1
TN 1024 4096 4096 9 2
NT 224 1024 1024 8 1
NN 224 1024 1024 7 1
NT 224 3072 1024 7 1
NN 224 1024 3072 7 1
NT 224 2048 1024 7 1
NN 224 1024 2048 7 1
NT 224 1024 2048 8 1
NN 224 2048 1024 7 1
NT 32 256 4096 8 1
NN 32 4096 256 3 1
"""
for _line in _BASELINE_TABLE.strip().splitlines():
    _lay, _M, _N, _K, _c, _s = _line.split()
    BASELINE_PLAN[(_lay, int(_M), int(_N), int(_K))] = (int(_c), int(_s))


def test_baseline_table_is_complete():
    assert {r[:4] for r in baseline_rows()} == set(BASELINE_PLAN), "update the table"


@pytest.mark.parametrize("row", baseline_rows(), ids=lambda r: f"{r[0]}-{r[1]}x{r[2]}x{r[3]}")
def test_baseline_shape_takes_the_expected_kernel_and_is_right(L, row):
    """The heuristics' choice for every GEMM of the BASELINE steps is pinned (a change of pick_config must update the table, so
    it cannot take a kernel out of coverage silently), every configuration of the table is one test 1 runs at its tile edges,
    and the shape is right on real-valued, poisoned, guarded operands at that choice."""
    layout, M, N, K, what = row
    ta, tb = G.LAYOUTS[layout]
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, "the table holds for 256 CUs"
    out_f32 = layout == "TN"
    got = plan(ta, tb, M, N, K, out_f32, WS_BYTES if out_f32 else 0)
    assert got[:2] == BASELINE_PLAN[row[:4]], f"{row}: plan {got[:2]}, table {BASELINE_PLAN[row[:4]]}: update the table"
    assert all(built(c, lay, lay == "TN") for (lay, *_), (c, _) in BASELINE_PLAN.items()), "a table row names a configuration test 1 cannot force"
    assert {c for c, _ in BASELINE_PLAN.values()} <= {c for c, _ in FORCED}
    colsum = "column sums" in what
    epi = 2 if colsum else (1 if (layout == "NT" and N == 4 * K) else 0)
    case = G.make_case(M, N, K, seed=M + N + K, bias=layout == "NT", epi=epi, c0=out_f32)
    run_case(layout, case, out_f32, colsum, rows=sample_rows(M, 3), name=f"{row}")


# ------------------------------------------------------------------------------------------------ 3. split-K
@pytest.mark.parametrize("layout,M,N,K,bias,acc", [("TN", 768, 768, 25600, False, True), ("NT", 800, 768, 6 * 768, True, False),
                                                   ("NN", 1024, 768, 6 * 768, False, True)])
def test_split_k_follows_the_workspace(L, layout, M, N, K, bias, acc):
    """fp32 output with no workspace, one that fits exactly two slabs, and plenty: the plan reports 1 / 2 / the full number of
    slices, the launch stays inside the splitk * M * N floats the plan names, the bias of a split launch lands once, and every
    result is bit-identical from run to run."""
    ta, tb = G.LAYOUTS[layout]
    case = G.make_case(M, N, K, seed=K + M, bias=bias, c0=acc)
    full = plan(ta, tb, M, N, K, 1, WS_BYTES)[1]
    assert full > 2
    for ws_bytes, want in ((0, 1), (2 * M * N * 4, 2), (WS_BYTES, full)):
        pl, _ = run_case(layout, case, True, ws_bytes=ws_bytes, twice=True, name=f"{layout} {M}x{N}x{K} workspace {ws_bytes}")
        assert pl[1] == want, (pl, want)


@pytest.mark.parametrize("cfg,flags", [(0, 9), (2, 9), (9, 9), (9, 1)])
@pytest.mark.parametrize("K,slices,last", [(1032, 4, 72), (1344, 5, 64)])
def test_split_k_short_last_slice(L, forced, cfg, flags, K, slices, last):
    """a last slice of 72 k (two K-steps, the second ragged: the shortest unit configuration 9 hands over) and one of 64, which
    the 3-deep ring of configuration 9 cannot stream: the library falls back to configuration 0 there"""
    forced(cfg, flags)
    M, N = 264, 136
    case = G.make_case(M, N, K, seed=K + cfg, c0=True)
    pl, _ = run_case("TN", case, True, twice=True, name=f"cfg {cfg} flags {flags} TN {M}x{N}x{K}")
    assert pl[1] == slices and K - (slices - 1) * pl[2] == last, pl
    assert pl[0] == (0 if (cfg == 9 and last == 64) else cfg), pl


@pytest.mark.parametrize("split_m", [256, 264])
@pytest.mark.parametrize("K", [4096, 200])
def test_split_output_on_and_off_a_tile_boundary(L, K, split_m):
    """hriemo_gemm_bf16_split: rows [0, split_m) to one guarded matrix, the rest to another one (split-K reduce at K = 4096, two
    launches inside the library at K = 200)"""
    M, N = 768, 264
    case = G.make_case(M, N, K, seed=K + split_m, c0=True)
    pl, _ = run_case("TN", case, True, twice=True, split_m=split_m, name=f"split output at {split_m}, K = {K}")
    assert (pl[1] > 1) == (K == 4096), pl


# ------------------------------------------------------------------------------------------------ 4. grouped dW, column sums
def test_grouped_weight_gradients_real_valued_and_guarded(L):
    """hriemo_gemm_bf16_group_tn on the 19 problems of test_gemm_group_tn_many_weight_gradients_in_one_launch: real-valued
    operands in poisoned padding, 19 guarded destinations that start finite and non-zero (accumulate), then overwritten"""
    shapes = [(384, 2304, 768), (384, 768, 768), (384, 768, 2048), (384, 2048, 768), (64, 768, 256), (64, 256, 3072), (1000, 136, 200),
              (8, 64, 64), (384, 1536, 768)] * 2 + [(72, 8, 8)]
    jobs, table = [], []
    for j, (K, M, N) in enumerate(shapes):                      # K reduction rows; result [M, N]
        case = G.make_case(M, N, K, seed=300 + j, c0=True)
        A = G.Guarded.of(case["A"].t().contiguous(), j=1 + j % 3, device="cuda")
        B = G.Guarded.of(case["B"], j=1 + (j + 1) % 3, device="cuda")
        C = G.Guarded.of(case["c0"], j=1 + (j + 2) % 3, device="cuda")
        jobs.append((case, A, B, C))
        table.append((M, N, K, A.ptr, A.ld, B.ptr, B.ld, C.ptr, C.ld))
    host = torch.tensor(table, dtype=torch.int64)
    for accumulate in (1, 0):
        call("hriemo_gemm_bf16_group_tn", host.data_ptr(), len(table), accumulate, stream())
        torch.cuda.synchronize()
        for j, (case, A, B, C) in enumerate(jobs):
            name = f"group job {j} {shapes[j]} accumulate {accumulate}"
            for n, b in (("A", A), ("B", B), ("C", C)):
                b.assert_intact(f"{name}: {n}")
            c0 = case["c0"] if accumulate else None
            K = case["A"].shape[1]
            ref, mag = G.reference(case["A"], case["B"], c0=c0, out_f32=True)
            yards = G.yardsticks(case["A"], case["B"], c0=c0, out_f32=True)
            note("TN", True, G.check(C.view.cpu(), ref, mag, yards, K, True, name))


@pytest.mark.parametrize("M,N,K", [(6000, 3072, 768), (1608, 776, 520)])
def test_masked_dx_with_column_sums_on_the_loader_consumer_kernel(L, M, N, K):
    assert plan(0, 1, M, N, K, 0)[0] == 9, "update the shapes: the heuristics no longer take configuration 9 here"
    case = G.make_case(M, N, K, seed=M, epi=2)
    run_case("NN", case, colsum=True, name=f"masked dX + column sums {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------------ 5. NaN stays in its row
@pytest.mark.parametrize("layout", ["NT", "NN"])
@pytest.mark.parametrize("cfg", [0, 2, 9])
def test_nan_and_inf_stay_in_their_rows(L, forced, cfg, layout):
    """an all-PAD sample's rows are NaN in the activations: one row of A all NaN, one element of another row +Inf; exactly those
    rows of the result are non-finite and every other row is as right as without them"""
    forced(cfg)
    ta, tb = G.LAYOUTS[layout]
    M, N, K = 520, 264, 200
    case = G.make_case(M, N, K, seed=cfg, bias=True)
    assert plan(ta, tb, M, N, K, 0)[0] == cfg
    bad = torch.zeros(M, dtype=torch.bool)
    bad[[5, 300]] = True
    A = G.Guarded.of(case["A"], j=1, device="cuda")
    A.view[5] = float("nan")
    A.view[300, 17] = float("inf")
    B = G.Guarded.of(case["B"] if tb else case["B"].t().contiguous(), j=2, device="cuda")
    bias = G.Guarded.of(case["bias"], guard=2, device="cuda")
    C = G.Guarded(M, N, torch.bfloat16, j=1, device="cuda")
    call("hriemo_gemm_bf16", ta, tb, M, N, K, A.ptr, A.ld, B.ptr, B.ld, C.ptr, C.ld, 0, bias.ptr, 0, None, 0, 0, None, 0, stream())
    torch.cuda.synchronize()
    for n, b in (("A", A), ("B", B), ("bias", bias), ("C", C)):
        b.assert_intact(n)
    got = C.view.cpu()
    assert not torch.isfinite(got[bad].float()).any(), "the NaN / Inf rows must come out non-finite"
    keep = ~bad
    ref, mag = G.reference(case["A"][keep], case["B"], case["bias"])
    yards = G.yardsticks(case["A"][keep], case["B"], case["bias"])
    note(layout, False, G.check(got[keep], ref, mag, yards, K, False, f"cfg {cfg} {layout}: rows beside a NaN row"))


# ------------------------------------------------------------------------------------------------ 6. Linear + LayerNorm
@pytest.mark.parametrize("M,d,K,p,twin,mapped", [(1100, 768, 768, 0.1, True, False), (333, 768, 768, 0.1, False, True)])
def test_gemm_ln_fwd_inside_guards(L, M, d, K, p, twin, mapped):
    """hriemo_gemm_ln_fwd (the kernel that stores through raw-buffer descriptors from an 8-wave block) at ragged M: the comparison
    of test_gemm_ln_fused_equals_gemm_then_add_ln with A and W in poisoned padding, X16 / X32 between poisoned guard rows and G, Y,
    Y32, mean, rstd between guard rows that must stay untouched (those matrices have no leading dimension: ld = d)"""
    from hri_emo_amd import _ops as ops
    g = torch.Generator().manual_seed(M + d + K)
    A = (0.5 * torch.randn(M, K, generator=g)).bfloat16().cuda()
    W = (torch.randn(d, K, generator=g) / math.sqrt(K)).bfloat16().cuda()
    b = (0.1 * torch.randn(d, generator=g)).cuda()
    X32 = torch.randn(M, d, generator=g).cuda()
    X16 = X32.bfloat16()
    gamma = (1 + 0.1 * torch.randn(d, generator=g)).cuda()
    beta = (0.1 * torch.randn(d, generator=g)).cuda()
    rows = (torch.randperm(3 * M, generator=g)[:M].sort().values.to(torch.int64).cuda()) if mapped else None
    seed, site, roff = 13572468, 5, 640
    g_ref = ops.linear_fwd(A, W, b)
    y_ref, y32_ref, mean_ref, rstd_ref = ops.add_ln_fwd(g_ref, X16, gamma, beta, p, seed, site, roff, x32=X32 if twin else None,
                                                         want32=True, rows=rows)
    kw = dict(device="cuda", guard=64)
    Ag, Wg = G.Guarded.of(A, j=1, **kw), G.Guarded.of(W, j=2, **kw)
    bg, gg, eg = (G.Guarded.of(t, guard=2, device="cuda") for t in (b, gamma, beta))
    x16g, x32g = G.Guarded.of(X16, j=0, **kw), (G.Guarded.of(X32, j=0, **kw) if twin else None)
    Gg, Yg = G.Guarded(M, d, torch.bfloat16, j=0, **kw), G.Guarded(M, d, torch.bfloat16, j=0, **kw)
    Y32g = G.Guarded(M, d, torch.float32, j=0, **kw)
    mg, rg = G.Guarded(1, (M + 3) // 4 * 4, torch.float32, j=0, guard=2, device="cuda"), G.Guarded(1, (M + 3) // 4 * 4, torch.float32, j=0, guard=2, device="cuda")
    call("hriemo_gemm_ln_fwd", M, d, K, Ag.ptr, Ag.ld, Wg.ptr, Wg.ld, bg.ptr, x16g.ptr, ptr(x32g), gg.ptr, eg.ptr, Gg.ptr, Yg.ptr, Y32g.ptr,
         mg.ptr, rg.ptr, 1e-5, float(p), seed, ops.seed_word(torch.device("cuda", 0)).data_ptr(), site, roff,
         None if rows is None else rows.data_ptr(), stream())
    torch.cuda.synchronize()
    for n, buf in (("A", Ag), ("W", Wg), ("bias", bg), ("gamma", gg), ("beta", eg), ("X16", x16g), ("X32", x32g), ("G", Gg), ("Y", Yg),
                   ("Y32", Y32g)):
        if buf is not None:
            buf.assert_intact(n)
    # mean / rstd: M floats inside a row padded to a multiple of 4; the tail and the guard rows stay 0xFF
    for n, buf in (("mean", mg), ("rstd", rg)):
        by = buf.raw.view(5, -1)
        assert (by[:2] == 0xFF).all() and (by[3:] == 0xFF).all() and (by[2, 4 * M:] == 0xFF).all(), f"{n}: stored outside its {M} floats"
    mean_f, rstd_f = mg.view[0, :M], rg.view[0, :M]
    for t in (Gg.view, Yg.view, Y32g.view, mean_f, rstd_f):
        assert torch.isfinite(t.float()).all()
    assert torch.equal(Gg.view, g_ref)
    scale = max(1.0, float(y32_ref.abs().max()))
    assert float((Y32g.view - y32_ref).abs().max()) <= 4e-6 * scale
    assert float((Yg.view.float() - y_ref.float()).abs().max()) <= 2 ** -6 * scale
    assert float((Yg.view.float() != y_ref.float()).float().mean()) <= 1e-3
    assert float((mean_f - mean_ref).abs().max()) <= 1e-6 and float((rstd_f / rstd_ref - 1).abs().max()) <= 1e-5
    # G against the float64 reference as well (it is bit-identical to hriemo_gemm_bf16's result, which tests 1-2 judge)
    case = {"A": A.cpu(), "B": W.cpu().t(), "bias": b.cpu(), "aux": None, "c0": None, "epi": 0}
    ref, mag = G.reference(case["A"], case["B"], case["bias"])
    note("NT", False, G.check(Gg.view.cpu(), ref, mag, G.yardsticks(case["A"], case["B"], case["bias"]), K, False, "gemm_ln G"))


# ------------------------------------------------------------------------------------------------ 7. the work queue in a step
def ints(shape, lo=-3, hi=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).float()


def test_training_step_is_bit_identical_on_the_work_queue_eager_and_captured(L):
    """BASELINE configs[1]'s shape at B = 8: the audio encoder's FFN GEMMs run configuration 9 with more tiles than CUs, i.e.
    the walk matters.  DataParallelStep(force_queue=...) selects it; the flag word read back after each step must say so.  A tile's
    arithmetic does not depend on who draws it and split-K slabs are summed in slice order: loss, logits and every gradient are
    bit-identical between the static walk and the queue, eagerly and over 5 replays of the captured step."""
    import hri_emo_amd as H
    from hri_emo_amd import _ops
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    B, Ta, Tt, d = 8, 400, 128, 768
    for (ta, tb, M, N, K) in ((0, 0, B * Ta, 4 * d, d), (0, 1, B * Ta, 4 * d, d)):
        assert plan(ta, tb, M, N, K, 0)[0] == 9 and -(-M // 256) * -(-N // 128) > 256, "the step no longer reaches the queue: pick another batch"
    torch.manual_seed(11)
    m = H.FusionWithEmotionDecoder(d_model=d, num_emotions=6, dropout=0.0).cuda().train()
    g = torch.Generator().manual_seed(12)
    la, lt = torch.randint(Ta // 2, Ta + 1, (B,), generator=g), torch.randint(Tt // 2, Tt + 1, (B,), generator=g)
    batch = (torch.randn(B, Ta, d, generator=g).cuda().bfloat16(), torch.randn(B, Tt, d, generator=g).cuda().bfloat16(),
             (torch.arange(Ta)[None] >= la[:, None]).cuda(), (torch.arange(Tt)[None] >= lt[:, None]).cuda(),
             (torch.rand(B, 6, generator=g) < 0.3).float().cuda())
    before = _ops.gemm_flags()
    seed_word = _ops.seed_word(torch.device("cuda", 0))
    seed_was = seed_word.clone()           # a captured step bumps it on every replay; later tests replay dropout masks from it
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    dp.set_global_batch(B)
    try:
        res = {}
        for queue in (False, True):
            dp.force_queue = queue
            loss = dp.step(*batch).clone()
            assert bool(_ops.gemm_flags() & 8) == (not queue), "the walk that was asked for is not the one in force"
            with torch.no_grad():
                logits = m(*batch[:4])[0].clone()
            res[queue] = (loss, logits, dp.buckets.flat.clone())
        assert torch.isfinite(res[True][2]).all() and float(res[True][2].abs().max()) > 0
        for a, b_, what in zip(res[False], res[True], ("loss", "logits", "gradients")):
            assert torch.equal(a, b_), f"{what} differ between the static walk and the work queue"
        dp.capture(*batch)
        for rep in range(5):
            dp.buckets.flat.fill_(float("nan"))
            loss = dp.step(*batch)
            assert not (_ops.gemm_flags() & 8)
            assert torch.equal(loss, res[True][0]) and torch.equal(dp.buckets.flat, res[True][2]), f"replay {rep}"
    finally:
        dp.release_graph()
        seed_word.copy_(seed_was)
        _ops.gemm_contended(not (before & 8), force=True)
    # a word set by the caller survives the automatic choice of a later step (world == 1 used to turn 1 into 9)
    try:
        _ops.set_gemm_flags(1)
        dp2 = DataParallelStep(H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, dropout=0.0).cuda().train(), fusion_step_loss, overlap=False)
        dp2.step(torch.randn(4, 32, 128).cuda().bfloat16(), torch.randn(4, 16, 128).cuda().bfloat16(), torch.zeros(4, 32, dtype=torch.bool).cuda(),
                 torch.zeros(4, 16, dtype=torch.bool).cuda(), torch.zeros(4, 4).cuda())
        assert _ops.gemm_flags() == 1
    finally:
        _ops.set_gemm_flags(None)
        L.hriemo_gemm_debug_flags(before)
        torch.cuda.synchronize()
        seed_word.copy_(seed_was)


def test_work_queue_in_a_graph_with_two_branches_replayed(L, forced):
    """Configuration 9, flag word 1: NT, NN + residual and the split-K weight gradient captured into one graph on two forked
    streams and replayed 5 times on integer operands, exact every time -- a queue word left non-zero by one replay would make the
    next one skip tiles."""
    from hri_emo_amd import _ops as ops
    forced(9, 1)
    M, N, K = 25600, 768, 768
    A, W, b = ints((M, K), seed=1), ints((N, K), seed=2), ints((N,), seed=3)
    dY, W2, R = ints((M, N), seed=5), ints((N, K), seed=6), ints((M, K), seed=7)
    dYs, X = ints((M, N), -2, 3, seed=8), ints((M, K), -2, 3, seed=9)
    want = ((A @ W.t() + b).bfloat16().float(), (dY @ W2 + R).bfloat16().float(), dYs.t() @ X)
    Ad, Wd, bd = A.cuda().bfloat16(), W.cuda().bfloat16(), b.cuda()
    dYd, W2d, Rd = dY.cuda().bfloat16(), W2.cuda().bfloat16(), R.cuda().bfloat16()
    dYsd, Xd = dYs.cuda().bfloat16(), X.cuda().bfloat16()
    assert plan(0, 0, M, N, K, 0)[0] == 9 and plan(0, 1, M, K, N, 0)[0] == 9 and plan(1, 1, N, K, M, 1, WS_BYTES)[0] == 9
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    dx = torch.empty((M, K), dtype=torch.bfloat16, device="cuda")
    dw = torch.empty((N, K), dtype=torch.float32, device="cuda")
    main, side = torch.cuda.Stream(), torch.cuda.Stream()

    def body():
        side.wait_stream(torch.cuda.current_stream())
        ops.gemm(0, 0, M, N, K, Ad, K, Wd, K, y, N, bias=bd)
        with torch.cuda.stream(side):
            ops.gemm(0, 1, M, K, N, dYd, N, W2d, K, dx, K, epi=3, aux=Rd, ldaux=K)
        ops.gemm(1, 1, N, K, M, dYsd, N, Xd, K, dw, K, c_f32=True)
        torch.cuda.current_stream().wait_stream(side)
    main.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(main):
        body()                                                 # eagerly first: queue words and workspace exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=main):
        body()
    for rep in range(5):
        for t in (y, dx, dw):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, ref, what in zip((y, dx, dw), want, ("NT", "NN + aux", "TN split-K")):
            assert torch.equal(got.float().cpu(), ref), f"replay {rep}: {what}"
