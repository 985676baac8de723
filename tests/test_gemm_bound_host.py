"""CPU suite: the limits of gemm_reference.check have teeth.  Emulated kernels (fp32 accumulation on the CPU in a given order,
the epilogue of gemm_common.h:store_tile) must pass when they are correct and fail at least one check for each fault a GEMM
rewrite can plausibly introduce; the guarded, poisoned buffers of the GPU suite must report a store outside the logical result and
a read outside the logical operand.  No GPU, no library call except the read-only launch-plan query."""
import ctypes

import pytest
import torch

import gemm_reference as G

M_, N_ = 520, 776          # two ragged 256 x 128 tiles each way


def emulate(case, order="seq64", out_f32=False, k_per_split=None, convert=G.bf16_round, step_hook=None, drop=None):
    """a kernel on the CPU: fp32 accumulation in `order` ('seq64': 64-deep K-steps in turn, which is NOT one of the yardstick
    orders), then the epilogue.  drop = (lo, hi): those k are left out of the contraction."""
    A32, B32 = case["A"].float(), case["B"].float()
    if drop is not None:
        keep = torch.ones(A32.shape[1], dtype=torch.bool)
        keep[drop[0]:drop[1]] = False
        A32, B32 = A32[:, keep], B32[keep]
    b32 = None if case["bias"] is None else case["bias"].float()
    if order == "seq64":
        acc = None
        for lo, hi in G._kchunks(A32.shape[1], 64):
            part = A32[:, lo:hi] @ B32[lo:hi]
            acc = part if acc is None else acc + part
            acc = step_hook(acc) if step_hook else acc
        biased = False
    else:
        acc, biased = G.accumulate(A32, B32, order, k_per_split, b32, step_hook)
    return G.finish(acc, None if biased else b32, case["aux"], case["epi"], case["c0"], out_f32, convert)


def judge(case, got, out_f32, k_per_split=None, name="emulated"):
    K = case["A"].shape[1]
    ref, mag = G.reference(case["A"], case["B"], case["bias"], case["aux"], case["epi"], case["c0"], out_f32)
    yards = G.yardsticks(case["A"], case["B"], case["bias"], case["aux"], case["epi"], case["c0"], out_f32, k_per_split)
    return G.check(got, ref, mag, yards, K, out_f32, name)


def fails(case, got, out_f32, k_per_split=None):
    with pytest.raises(AssertionError):
        judge(case, got, out_f32, k_per_split)


@pytest.mark.parametrize("K", [96, 768, 3072])
@pytest.mark.parametrize("epi,bias", [(0, False), (0, True), (1, True), (2, False), (3, True)])
def test_correct_bf16_kernels_pass_in_every_order(K, epi, bias):
    case = G.make_case(M_, N_, K, seed=K + epi, bias=bias, epi=epi)
    for order in G.ORDERS + ("seq64",):
        r = judge(case, emulate(case, order), False, name=f"{order} K={K} epi={epi}")
        assert r["elem"] <= 1.0 and r["share"] <= 1.0


@pytest.mark.parametrize("K,kper", [(96, None), (3072, None), (3072, 1024), (25600, None), (25600, 3648)])
def test_correct_fp32_kernels_pass_in_every_order(K, kper):
    case = G.make_case(264, 136, K, seed=K, bias=True, c0=True)
    orders = G.ORDERS + ("seq64",) + (("splitk",) if kper else ())
    for order in orders:
        r = judge(case, emulate(case, order, True, kper), True, kper, name=f"{order} K={K}")
        assert r["elem"] <= 0.1, "correct fp32 orders stay far below the worst-case elementwise limit"


@pytest.mark.parametrize("K", [96, 768, 3072])
def test_truncating_convert_fails(K):
    case = G.make_case(M_, N_, K, seed=1, bias=True)
    fails(case, emulate(case, convert=G.bf16_trunc), False)


@pytest.mark.parametrize("K", [96, 776, 3072])
@pytest.mark.parametrize("out_f32", [False, True])
def test_last_8_k_dropped_fails(K, out_f32):
    case = G.make_case(M_, N_, K, seed=2)
    fails(case, emulate(case, out_f32=out_f32, drop=(K - 8, K)), out_f32)


def test_one_k_step_dropped_at_25600_fails():
    case = G.make_case(264, 136, 25600, seed=3)
    fails(case, emulate(case, out_f32=True, drop=(6400, 6464)), True)
    # ... which the 2e-3 * max|want| bound of test_gemm_tn_splitk_weight_gradient_shapes lets through
    got, want = emulate(case, out_f32=True, drop=(6400, 6464)), case["A"].float() @ case["B"].float()
    assert float((got - want).abs().max()) > 0


@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("out_f32", [False, True])
def test_partial_sums_kept_in_bf16_fail(K, out_f32):
    case = G.make_case(M_, N_, K, seed=4)
    fails(case, emulate(case, out_f32=out_f32, step_hook=lambda a: a.bfloat16().float()), out_f32)


def test_bias_added_once_per_split_k_slab_fails():
    K, kper = 4608, 1152                                       # the fp32 mode's linear: K = 6 * 768, four slabs
    case = G.make_case(264, 136, K, seed=5, bias=True)
    A32, B32 = case["A"].float(), case["B"].float()
    got = None
    for lo, hi in G._kchunks(K, kper):
        slab = A32[:, lo:hi] @ B32[lo:hi] + case["bias"].float()
        got = slab if got is None else got + slab
    fails(case, got, True, kper)
    judge(case, emulate(case, "splitk", True, kper), True, kper)


@pytest.mark.parametrize("out_f32", [False, True])
def test_row_written_one_row_lower_fails(out_f32):
    case = G.make_case(M_, N_, 768, seed=6)
    good = emulate(case, out_f32=out_f32)
    got = good.clone()
    got[256] = good[255]
    fails(case, got, out_f32)


def test_residual_added_after_the_rounding_fails():
    case = G.make_case(M_, N_, 768, seed=7, epi=3)
    acc = case["A"].float() @ case["B"].float()
    got = (acc.bfloat16().float() + case["aux"].float()).bfloat16()
    fails(case, got, False)


def test_relu_mask_taken_as_aux_ge_0_fails():
    case = G.make_case(M_, N_, 768, seed=8, epi=2)
    acc = (case["A"].float() @ case["B"].float()).bfloat16()
    got = acc * (case["aux"].float() >= 0).bfloat16()
    fails(case, got, False)
    # the planted values: +0.0 and -0.0 are masked, the smallest positive normal is kept
    ref, _ = G.reference(case["A"], case["B"], None, case["aux"], 2)
    aux = case["aux"].double()
    assert (ref[aux == 0] == 0).all() and (aux == 0).sum() >= 2 * M_ - 8 and (aux == 2.0 ** -126).sum() >= M_ - 8
    assert (ref[aux == 2.0 ** -126] != 0).any()


def test_unstored_element_and_poison_read_fail():
    case = G.make_case(264, 136, 96, seed=9)
    out = G.Guarded(264, 136, torch.bfloat16)
    good = emulate(case)
    out.view.copy_(good)
    out.view[263, 128:] = out.full[0, :8]                      # a 16-byte line that was never stored: still 0xFF
    fails(case, out.view.clone(), False)
    # a kernel that reads 8 elements of the operand rows' own padding (c * 8 > krem instead of >=)
    a = G.Guarded.of(case["A"])
    b = G.Guarded.of(case["B"].t().contiguous())               # [N, K]: the padding follows k = K
    wide = a.full[a.guard:a.guard + 264, :96 + 8].float() @ b.full[b.guard:b.guard + 136, :96 + 8].float().t()
    assert not torch.isfinite(wide).any()
    fails(case, wide.bfloat16(), False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_guarded_buffer_reports_stores_outside_the_logical_matrix(dtype):
    x = torch.randn(40, 24).to(dtype)
    for j in (1, 3):
        buf = G.Guarded.of(x, j=j, guard=16)
        assert buf.ld == 24 + 8 * j and buf.view.stride(0) == buf.ld and buf.ptr % 16 == 0
        assert torch.equal(buf.view, x) and buf.violations() == 0
        assert not torch.isfinite(buf.full[:16].float()).any() and not torch.isfinite(buf.full[16:56, 24:].float()).any()
        buf.view.mul_(2)                                       # writes inside are free
        buf.assert_intact("inside")
        for r, c in ((15, 0), (56, 23), (16, 24), (55, buf.ld - 1)):      # row above, row below, first / last padding column
            b2 = G.Guarded.of(x, j=j, guard=16)
            b2.full[r, c] = 1.0
            assert b2.violations() == b2.es
            with pytest.raises(AssertionError):
                b2.assert_intact("outside")
    v = G.Guarded.of(torch.randn(24), guard=4)                 # 1-D (bias, column-sum partials, workspace): one row
    assert v.view.shape == (1, 24) and v.violations() == 0


def test_edge_shapes_straddle_every_tile_edge():
    for cfg, (bm, bn, ns, bk) in G.TILES.items():
        for ta in (0, 1):
            Ms, Ns, Ks, kfb = G.edge_shapes(cfg, ta)
            assert [(-k) % 64 for k in Ks] == [56, 8, 32] and all(k > (ns - 2) * bk and k % 8 == 0 for k in Ks)
            assert all(m % 8 == 0 for m in Ms) if ta else Ms == [bm + 1, 2 * bm - 7, 3 * bm]
            assert bm < Ms[0] < 2 * bm and bm < Ms[1] < 2 * bm and Ms[2] % bm == 0
            assert all(n % 8 == 0 and n % bn != 0 for n in Ns)
            assert (kfb is None) == (ns == 2)


def test_launch_plan_query_reports_fallbacks_and_matches_colsum_rows():
    """hriemo_gemm_plan is host code (no launch): forced configurations, every documented fallback, split-K against the workspace.
    Without a GPU the library assumes 256 CUs."""
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    L = _lib.lib()

    def plan(ta, tb, M, N, K, f32=0, ws=0):
        c, s, k = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        _lib.call("hriemo_gemm_plan", ta, tb, M, N, K, f32, ws, ctypes.byref(c), ctypes.byref(s), ctypes.byref(k))
        return c.value, s.value, k.value
    wave_rows = {0: 64, 1: 64, 2: 128, 3: 32, 4: 128, 5: 80, 6: 32, 7: 16, 8: 16, 9: 64}
    try:
        for cfg, (bm, bn, ns, bk) in G.TILES.items():
            L.hriemo_gemm_force_config(cfg)
            Ms, Ns, Ks, kfb = G.edge_shapes(cfg, 0)
            assert plan(0, 0, Ms[0], Ns[0], Ks[0]) == (cfg, 1, 64 * ns)
            assert plan(0, 1, Ms[0], Ns[0], Ks[0])[0] == (7 if cfg == 8 else cfg)
            assert plan(1, 1, Ms[2], Ns[0], Ks[0])[0] == (0 if cfg in (3, 5, 6, 7, 8) else cfg)
            assert plan(0, 0, Ms[0], Ns[0], Ks[0], 1)[0] == (0 if cfg == 5 else cfg)
            if kfb is not None:
                assert plan(0, 0, Ms[0], Ns[0], kfb)[0] == 0 and plan(0, 0, Ms[0], Ns[0], kfb + 8)[0] == cfg
            for (M, N, K) in [(Ms[1], Ns[1], Ks[2]), (1608, 776, 520)]:
                c = plan(0, 1, M, N, K)[0]
                assert L.hriemo_gemm_colsum_rows(0, 1, M, N, K) == -(-M // wave_rows[c])
        L.hriemo_gemm_force_config(0)
        M, N, K = 768, 768, 25600
        assert plan(1, 1, M, N, K, 1, 0)[1] == 1                                    # no workspace: no split
        assert plan(1, 1, M, N, K, 1, 2 * M * N * 4) == (0, 2, 12800)               # fits two slabs
        assert plan(1, 1, M, N, K, 1, 3 * M * N * 4 - 4)[1] == 2
        c, s, kper = plan(1, 1, M, N, K, 1, 64 << 20)
        assert s > 2 and kper % 64 == 0 and (s - 1) * kper < K <= s * kper
    finally:
        L.hriemo_gemm_force_config(-1)


def test_baseline_table_matches_the_plan_on_256_cus():
    """the table of test_gpu_gemm_variants.py against the library's heuristics, replayed on the host (256 CUs are assumed without
    a GPU, and are what an MI355X has): a change of pick_config shows here first.  Every configuration of the table is one the
    forced-configuration test builds for that layout."""
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    import test_gpu_gemm_variants as T
    _lib.lib().hriemo_gemm_force_config(-1)
    rows = T.baseline_rows()
    assert {r[:4] for r in rows} == set(T.BASELINE_PLAN) and len(rows) >= 100
    for (lay, M, N, K), want in T.BASELINE_PLAN.items():
        ta, tb = G.LAYOUTS[lay]
        f32 = lay == "TN"
        c, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.call("hriemo_gemm_plan", ta, tb, M, N, K, int(f32), T.WS_BYTES if f32 else 0, ctypes.byref(c), ctypes.byref(s), ctypes.byref(k))
        assert (c.value, s.value) == want, f"{lay} {M}x{N}x{K}: plan {(c.value, s.value)}, table {want}: update the table"
        assert T.built(want[0], lay, f32) and (want[0], 9) in T.FORCED
    assert {c for c, _ in T.BASELINE_PLAN.values()} == {0, 2, 3, 7, 8, 9}
