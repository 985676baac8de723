"""CPU suite: the limits of gate_reference.check_* have teeth.  The emulated gate kernels (fp32 on the CPU, bf16 round-to-nearest on
store, the row statistics, the per-chunk column sums and the reduce in a given order) must pass every check on every case the GPU
suite runs when they are correct -- which also proves that the yardstick orders themselves stay inside the bf16 share cap on these
inputs -- and fail a check for each fault a rewrite of the gate kernels in rowops.hip can plausibly introduce, at the smallest
case that shows it.  No GPU and no library call."""
import pytest
import torch

import gate_reference as G
import rowops_reference as R


def fwd_yards(side, Lkeep):
    return {o: G.pool_fwd32(side, Lkeep, o, G.CHUNK_ORDERS[i % 3]) for i, o in enumerate(R.ROW_ORDERS)}


def bwd_yards(side, ops, is_a, m32, r32, init=None, accumulate=False):
    y = {o: G.pool_bwd32(side, ops, is_a, m32, r32, o, G.CHUNK_ORDERS[i % 3], init=init, accumulate=accumulate) for i, o in enumerate(R.ROW_ORDERS)}
    y["contract"] = G.pool_bwd32(side, ops, is_a, m32, r32, "chunk", "waves", init=init, accumulate=accumulate, contract=True)
    return y


def fwd_fails(side, Lkeep, fault):
    ref, yards = G.pool_fwd_ref(side, Lkeep), fwd_yards(side, Lkeep)
    G.check_pool_fwd(G.pool_fwd32(side, Lkeep, "chunk"), side, ref, yards, Lkeep, "correct")
    with pytest.raises(AssertionError):
        G.check_pool_fwd(G.pool_fwd32(side, Lkeep, "chunk", fault=fault), side, ref, yards, Lkeep, fault)


def bwd_fails(c, fault, init=None, accumulate=False, stale=None):
    side, ops, m32, r32 = G.make_bwd(c)
    is_a = c[7]
    ref = G.pool_bwd_ref(side, ops, is_a, m32, r32, init if accumulate else None)
    yards = bwd_yards(side, ops, is_a, m32, r32, init, accumulate)
    G.check_pool_bwd(G.pool_bwd32(side, ops, is_a, m32, r32, "chunk", init=init, accumulate=accumulate), side, ref, yards, "correct", accumulate)
    with pytest.raises(AssertionError):
        G.check_pool_bwd(G.pool_bwd32(side, ops, is_a, m32, r32, "chunk", fault=fault, init=init, accumulate=accumulate, stale=stale), side, ref,
                         yards, fault, accumulate)


# ------------------------------------------------------------------------------------------------ correct kernels pass
@pytest.mark.parametrize("c", G.FWD_CASES, ids=G.fwd_id)
def test_correct_forward_passes_in_every_order(c):
    B, L, Lk, d, fam, twin, mask = c
    side = G.gate_side(B, L, d, fam, twin, mask)
    ref, yards = G.pool_fwd_ref(side, Lk), fwd_yards(side, Lk)
    for o, y in yards.items():
        G.check_pool_fwd(y, side, ref, yards, Lk, f"{o} forward")
    if mask == "full":                 # a fully masked sample pools nothing: exact zeros
        assert (ref["mag_part"][B // 2] == 0).all() and (yards["chunk"]["part"][B // 2] == 0).all()


@pytest.mark.parametrize("c", G.BWD_CASES, ids=G.bwd_id)
def test_correct_backward_passes_in_every_order(c):
    side, ops, m32, r32 = G.make_bwd(c)
    ref, yards = G.pool_bwd_ref(side, ops, c[7], m32, r32), bwd_yards(side, ops, c[7], m32, r32)
    for o, y in yards.items():
        G.check_pool_bwd(y, side, ref, yards, f"{o} backward")


@pytest.mark.parametrize("accumulate", [False, True])
def test_correct_reduce_above_64_partials_passes(accumulate):
    B, L, d = G.MANY_PARTIALS
    c = (B, L, 37, d, "unit", False, "scattered", 1, True)
    assert B * G.chunks(L, G.BWD_ROWS) > 64
    side, ops, m32, r32 = G.make_bwd(c)
    init = {n: 1 + torch.rand(d) for n in ("dgamma", "dbeta")}
    ref = G.pool_bwd_ref(side, ops, 1, m32, r32, init if accumulate else None)
    yards = bwd_yards(side, ops, 1, m32, r32, init, accumulate)
    for o, y in yards.items():
        G.check_pool_bwd(y, side, ref, yards, o, accumulate)


def test_envelope_constants_cover_what_the_yardsticks_measure():
    """GATE_ENVELOPE and SIGMOID_MEASURED are records of measurements, not padded; the forward reuses rowops_reference.LN_ENVELOPE,
    which must cover the gate cases"""
    env = G.measure_gate_envelope()
    print("measured envelope:", {k: round(v, 2) for k, v in env.items()})
    assert env["dx"] <= G.GATE_ENVELOPE["dx"] <= 2 * env["dx"], env
    assert env["y"] <= R.LN_ENVELOPE["y"] and env["rstd"] <= R.LN_ENVELOPE["rstd"], env
    s = G.measure_sigmoid()
    print("measured sigmoid:", round(s, 2))
    assert s <= G.SIGMOID_MEASURED <= 1.05 * s, s
    assert 3 * G.SIGMOID_MEASURED <= G.SIGMOID_FACTOR <= 4 * G.SIGMOID_MEASURED


def test_edges_reach_every_instance():
    """the dispatch arithmetic: every NCH instance of the forward, the backward and fuse_bwd_dw, both pair instances, both
    constant-placement paths of the backward; chunks in which waves own no row; the second trip"""
    cov = G.coverage()
    for n in (1, 2, 4, 8):
        assert any(k.startswith(f"ln_pool_fwd<{n}") for k in cov) and any(k.startswith(f"ln_pool_bwd<{n}>") for k in cov) and f"fuse_bwd_dw<{n}>" in cov
    assert sum("pair" in k for k in cov) == 2
    assert any("CLDS" in k for k in cov) and any("registers" in k for k in cov)
    assert {G.nch(d) for d in G.WIDTHS} == {1, 2, 4, 8} and [G.nch(d) for d in (512, 520, 1024, 1032, 2048, 2056)] == [1, 2, 2, 4, 4, 8]
    assert any(G.chunk_rows(L, G.BWD_ROWS)[-1] < 4 for L in G.BWD_LENGTHS) and any(G.chunk_rows(L, G.POOL_ROWS)[-1] < 4 for L in G.FWD_LENGTHS)
    assert G.second_trip(*G.SECOND_TRIP) and not G.second_trip(2, 2047, 4096)
    for L, rows in ((70, G.POOL_ROWS), (70, G.BWD_ROWS)):
        ks = G.keep_cases(L, rows)
        assert 0 in ks and 1 in ks and rows in ks and L in ks and any(k % rows not in (0, 1) and k < L for k in ks)


# ------------------------------------------------------------------------------------------------ faulty forwards fail
def test_last_row_of_a_chunk_left_out_of_the_pool_fails():
    fwd_fails(G.gate_side(1, 1, 8), 1, "pool_drop_last_row")
    fwd_fails(G.gate_side(3, 33, 8, mask="none"), 5, "pool_drop_last_row")


def test_pool_that_includes_a_masked_row_fails():
    fwd_fails(G.gate_side(3, 3, 8, mask="scattered"), 3, "pool_masked")


def test_pool_of_the_bf16_rounded_rows_fails():
    fwd_fails(G.gate_side(3, 5, 8), 5, "pool_bf16")
    fwd_fails(G.gate_side(3, 70, 520, mask="scattered"), 5, "pool_bf16")


@pytest.mark.parametrize("Lkeep", [0, 1, 4])
def test_lkeep_off_by_one_is_caught_by_the_untouched_rows(Lkeep):
    side = G.gate_side(3, 5, 8)
    B, d = 3, 8
    for fault, ok in ((None, True), ("lkeep_off_by_one", False)):
        buf = R.Guarded(B * Lkeep + 2, d, torch.bfloat16, j=0, guard=2)
        G.store_rows(buf.view, G.pool_fwd32(side, Lkeep, "chunk", fault=fault)["y"], Lkeep)
        buf.assert_intact("Yn")
        if ok:
            G.check_untouched(buf.view, B * Lkeep, "Yn")
        else:
            with pytest.raises(AssertionError):
                G.check_untouched(buf.view, B * Lkeep, "Yn")


# ------------------------------------------------------------------------------------------------ gate_input, dpre, gate_input_bwd, fuse
@pytest.mark.parametrize("nca,nct", [(1, 1), (8, 9), (9, 13), (13, 8)])
def test_gate_input_limits(nca, nct):
    c = G.gate_input_case(3, nca, nct, 40, "full")
    assert G.chunks(c["La"], 32) == nca and G.chunks(c["Lt"], 32) == nct
    ref = G.gate_input_ref(c)
    yards = {o: G.gate_input32(c, o) for o in G.SEQ_ORDERS}
    assert float(ref["cnt"][1, 0]) == 1.0      # the fully masked sample
    for o, y in yards.items():
        G.check_gate_input(y, c, ref, yards, o)
    with pytest.raises(AssertionError):        # cnt not clamped at 1
        G.check_gate_input(G.gate_input32(c, "seq", "cnt_unclamped"), c, ref, yards, "cnt_unclamped")
    short = dict(c, pa=c["pa"][:, :-1]) if nca > 1 else None
    if short is not None:                      # last chunk left out of the pool
        got = G.gate_input32(short, "seq")
        with pytest.raises(AssertionError):
            G.check_gate_input(got, c, ref, yards, "short")


@pytest.mark.parametrize("d", [8, 520, 4096])
@pytest.mark.parametrize("nca,nct,mask", G.GATE_INPUT_CASES)
def test_gate_input_cases_of_the_gpu_suite(d, nca, nct, mask):
    """every yardstick order passes on the very cases the GPU suite runs; on the 'full' ones cnt = 1 comes from the clamp, and a
    kernel without it fails; column 0 (zero partials: a == t == 0) must come out as exact zeros"""
    c = G.gate_input_case(3, nca, nct, d, mask)
    ref = G.gate_input_ref(c)
    yards = {o: G.gate_input32(c, o) for o in G.SEQ_ORDERS}
    for o, y in yards.items():
        G.check_gate_input(y, c, ref, yards, o)
    assert (ref["mag_gin"][:, ::d] == 0).all() and (yards["seq"]["gin"][:, ::d] == 0).all()
    off = {k: v.clone() for k, v in yards["seq"].items()}
    off["gin"][:, 2 * d] = 2.0 ** -100             # |a - t| of column 0 a hair off zero
    with pytest.raises(AssertionError):
        G.check_gate_input(off, c, ref, yards, "a == t column not exact")
    valid_a = G.counts(c["ma"], 3, c["La"], clamp=False)
    if mask == "full":
        assert valid_a[1] == 0 and ref["cnt"][1, 0] == 1 and (c["La"] > 256) == (nca >= 9)
        with pytest.raises(AssertionError):
            G.check_gate_input(G.gate_input32(c, "seq", "cnt_unclamped"), c, ref, yards, "cnt_unclamped")
    else:
        assert (valid_a >= 1).all()


def test_gate_input_cases_reach_every_mask_family_on_both_sides_of_256_rows():
    seen = {(m, 32 * nca - 5 > 256) for nca, _, m in G.GATE_INPUT_CASES}
    assert seen >= {(m, big) for m in ("none", "scattered", "full", "single") for big in (False, True)}
    assert {(a, t) for a, t, _ in G.GATE_INPUT_CASES} == {(1, 1), (8, 9), (9, 13), (13, 8)}


@pytest.mark.parametrize("nc", G.CHUNK_COUNTS)
@pytest.mark.parametrize("dbeta", [True, False])
def test_gate_dpre_limits(nc, dbeta):
    c = G.dpre_case(3, nc, 40, dbeta)
    yards = {o: G.gate_dpre32(c, o) for o in G.SEQ_ORDERS}
    for o, y in yards.items():
        G.check_gate_dpre(y, c, yards, o)
    if dbeta:
        with pytest.raises(AssertionError):
            G.check_gate_dpre(G.gate_dpre32(c, "seq", "no_dbeta"), c, yards, "no_dbeta")


def test_sign_of_zero_is_zero():
    c = G.gin_bwd_case(3, 9)
    a, t = c["a"], c["t"]
    assert bool((a == t).any()) and bool((a > t).any()) and bool((a < t).any())
    G.check_gin_bwd(G.gin_bwd32(c), c, "correct")
    with pytest.raises(AssertionError):
        G.check_gin_bwd(G.gin_bwd32(c, "sign0_is_1"), c, "sign0_is_1")


def test_fuse_limits_and_the_coefficient():
    c = G.fuse_case(2, 5, 40)
    for o in G.FUSE_ORDERS:
        G.check_fuse_fwd(G.fuse_fwd32(c, o), c, o)
    with pytest.raises(AssertionError):
        G.check_fuse_fwd(G.fuse_fwd32(c, "plain", "coef_w"), c, "coef_w")
    c = G.fuse_case(2, 37, 40)
    for o in G.CHUNK_ORDERS:
        G.check_fuse_bwd_dw(G.fuse_bwd_dw32(c, o), c, o)
    for fault in ("drop_last_row", "drop_wave3"):
        with pytest.raises(AssertionError):
            G.check_fuse_bwd_dw(G.fuse_bwd_dw32(c, "waves", fault), c, fault)


def test_sigmoid_limits():
    pre = G.sigmoid_inputs(3, 520)
    for k in (-1, 0, 1):
        w = G.sigmoid32(pre, k)
        for o in R.ROW_ORDERS:
            G.check_sigmoid_beta(w, G.beta32(w, o), pre, f"{k} ulp, {o}")
    w = G.sigmoid32(pre)
    with pytest.raises(AssertionError):        # beta over d - 8 columns
        G.check_sigmoid_beta(w, R.row_sum(w, "chunk", True) / 520.0, pre, "short beta")
    with pytest.raises(AssertionError):        # a half-precision exponential
        G.check_sigmoid_beta(1 / (1 + torch.exp(-pre).bfloat16().float()), G.beta32(w), pre, "bf16 exp")


# ------------------------------------------------------------------------------------------------ faulty backwards fail
def test_w_where_one_minus_w_belongs_fails():
    bwd_fails((3, 5, 5, 8, "unit", False, "none", 0, True), "coef_w")


def test_dH_applied_past_Lf_fails():
    """the stale look-ahead register: row 4 is wave 0's second row and Lf = 1 leaves wave 0 holding row 0's dH"""
    bwd_fails((3, 5, 1, 8, "unit", False, "none", 1, True), "stale_dh")
    bwd_fails((3, 21, 17, 520, "unit", True, "scattered", 0, True), "stale_dh")


def test_dpool_dropped_past_Lf_fails():
    bwd_fails((3, 5, 1, 8, "unit", False, "none", 1, True), "dpool_dropped_past_lf")
    bwd_fails((3, 5, 0, 8, "unit", False, "none", 1, True), "dpool_dropped_past_lf")


def test_dpool_applied_on_masked_rows_fails():
    bwd_fails((3, 3, 1, 8, "unit", False, "scattered", 1, True), "dpool_on_masked")
    bwd_fails((3, 5, 5, 8, "unit", False, "full", 0, True), "dpool_on_masked")


def test_look_ahead_row_consumed_twice_fails():
    bwd_fails((3, 1, 1, 8, "unit", False, "none", 1, True), "lookahead_twice")
    bwd_fails((3, 17, 5, 8, "unit", False, "none", 1, True), "lookahead_twice")


def test_wave_3_partials_dropped_fails():
    bwd_fails((3, 4, 4, 8, "unit", False, "none", 1, True), "drop_wave3")


def test_gamma_missing_from_c1_c2_fails():
    bwd_fails((3, 5, 5, 8, "unit", False, "none", 1, True), "no_gamma")


def test_accumulate_ignored_fails():
    init = {n: 1 + torch.rand(8) for n in ("dgamma", "dbeta")}
    bwd_fails((3, 5, 5, 8, "unit", False, "none", 1, True), "ignore_accumulate", init, True)


@pytest.mark.parametrize("accumulate", [False, True])
def test_accumulation_in_the_first_reduce_pass_fails_above_64_partials(accumulate):
    B, L, d = G.MANY_PARTIALS
    init = {n: 1 + torch.rand(d) for n in ("dgamma", "dbeta")}
    bwd_fails((B, L, 37, d, "unit", False, "scattered", 1, True), "first_pass_accumulates", init, accumulate)


# ------------------------------------------------------------------------------------------------ legacy scalar gate
@pytest.mark.parametrize("L", [1, 3, 4, 5])
def test_masked_mean_limits(L):
    g = torch.Generator().manual_seed(L)
    X = torch.randn(3, L, 40, generator=g).bfloat16()
    m = G.make_mask("full", 3, L, g)
    for o in G.CHUNK_ORDERS:
        got = G.masked_mean32(X, m, o)
        G.check_masked_mean(got, G.counts(m, 3, L).float(), X, m, o)
    assert (G.masked_mean32(X, m)[1] == 0).all()
    with pytest.raises(AssertionError):
        G.check_masked_mean(G.masked_mean32(X, m, fault="cnt_unclamped"), G.counts(m, 3, L, False).float(), X, m, "cnt_unclamped")
    with pytest.raises(AssertionError):
        G.check_masked_mean(G.masked_mean32(X, m, fault="pool_masked"), G.counts(m, 3, L).float(), X, m, "pool_masked")


def test_scalar_gate_dx_dividing_masked_rows_by_cnt_fails():
    c = G.scalar_dx_case(3, 5, 3, 8)
    for is_a in (1, 0):
        for o in G.SCALAR_DX_ORDERS:
            G.check_scalar_dx(G.scalar_dx32(c, is_a, contract=o == "contract"), c, is_a, o)
        with pytest.raises(AssertionError):
            G.check_scalar_dx(G.scalar_dx32(c, is_a, "masked_div"), c, is_a, "masked_div")
    with pytest.raises(AssertionError):
        G.check_scalar_dx(G.scalar_dx32(c, 0, "coef_w"), c, 0, "coef_w")


@pytest.mark.parametrize("B,Ls,d", [(3, 5, 8), (3, 21, 520), (3, 37, 4096)])
def test_scalar_gate_dx_yardsticks_stay_inside_the_share_cap_on_the_gpu_cases(B, Ls, d):
    for Lf in G.keep_cases(Ls, 4):
        c = G.scalar_dx_case(B, Ls, Lf, d, "full")
        for is_a in (1, 0):
            for o in G.SCALAR_DX_ORDERS:
                G.check_scalar_dx(G.scalar_dx32(c, is_a, contract=o == "contract"), c, is_a, f"{o} Lf={Lf}")
    # one bf16 step away from zero on every 50th element (2 %): what the elementwise limit often lets through, the share rule never
    got = G.scalar_dx32(c, 1).reshape(-1, d)
    pick = ((torch.arange(got.numel()) % 50 == 0).view(got.shape) & (got != 0)).to(torch.int16)
    off = (got.view(torch.int16) + pick).view(torch.bfloat16)
    assert int(pick.sum()) >= 3 and (R.bf16_ordinal(off) - R.bf16_ordinal(got)).abs().max() == 1
    yards = {o: G.scalar_dx32(c, 1, contract=o == "contract").reshape(-1, d) for o in G.SCALAR_DX_ORDERS}
    with pytest.raises(AssertionError, match="the cap"):
        R.check_share(off, yards, torch.zeros(got.shape, dtype=torch.float64), "one step off")


@pytest.mark.parametrize("n", G.ROWSUM_N)
def test_rowsum_and_pooled_gate_input_limits(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(3, n, generator=g)
    ref, mag = G.rowsum_ref(x)
    for o in R.ROW_ORDERS:
        pad = torch.zeros(3, (n + 7) // 8 * 8)
        pad[:, :n] = x
        G.check_sum(R.row_sum(pad, o), ref, mag, n, o)
    if n > 1:
        with pytest.raises(AssertionError):
            G.check_sum(x[:, :-1].sum(1), ref, mag, n, "short")
    a, t = torch.randn(3, 40, generator=g), torch.randn(3, 40, generator=g)
    t[:, 0] = a[:, 0]
    gin = torch.cat([a, t, (a - t).abs(), a * t], 1).bfloat16()
    G.check_gate_input_pooled(gin, a, t, "correct")
    with pytest.raises(AssertionError):
        G.check_gate_input_pooled(torch.cat([a, t, (a - t), a * t], 1).bfloat16(), a, t, "no abs")
