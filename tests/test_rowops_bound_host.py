"""CPU suite: the limits of rowops_reference.check_* have teeth.  Emulated row kernels (fp32 on the CPU, two-pass variance, bf16
round-to-nearest on store, the row statistics and column sums in a given order) must pass every check on every input family when
they are correct -- which also proves that the yardstick orders themselves stay inside the bf16 share cap on these inputs -- and
fail a check for each fault a rewrite of rowops.hip can plausibly introduce, at the smallest shape that shows it.  The guarded,
poisoned buffers of the GPU suite must report a store outside the logical result.  No GPU and no library call."""
import numpy as np
import pytest
import torch

import hashrng
import rowops_reference as R


def build(M, d, family="unit", p=0.0, resid="x16", row_offset=0, row_index=None):
    case = R.ln_case(M, d, family, p, resid, row_offset, row_index)
    fwd = R.ln_fwd_ref(case)
    m32, r32 = R.stats32(fwd)
    return case, fwd, m32, r32


def judge_fwd(case, fwd, got, name="emulated"):
    yards = {o: R.fwd32(case, o) for o in R.ROW_ORDERS}
    return R.check_ln_fwd(got, case, fwd, yards, name)


def judge_bwd(case, m32, r32, got, init=None, accumulate=False, name="emulated", nb=None):
    ref = R.ln_bwd_ref(case, m32, r32, init if accumulate else None)
    _, yards = R.ln_yardsticks(case, m32, r32, init, accumulate, nb)
    return R.check_ln_bwd(got, case, ref, yards, name, accumulate)


def fwd_fails(case, fwd, got):
    with pytest.raises(AssertionError):
        judge_fwd(case, fwd, got)


def bwd_fails(case, m32, r32, got, **kw):
    with pytest.raises(AssertionError):
        judge_bwd(case, m32, r32, got, **kw)


# ------------------------------------------------------------------------------------------------ correct kernels pass
@pytest.mark.parametrize("c", R.LN_CASES, ids=R.case_id)
def test_correct_emulations_pass_in_every_order(c):
    """every yardstick order, taken as the kernel, passes every check -- the elementwise limits, the statistics, the share cap and
    the adjacency rule -- on every case the GPU suite runs (widths up to 4096, 16389 rows, every family)"""
    M, d, fam, p, res, _, roff = c
    case, fwd, m32, r32 = build(M, d, fam, p, res, roff)
    fw, bw = R.ln_yardsticks(case, m32, r32)
    ref = R.ln_bwd_ref(case, m32, r32)
    for o in R.ROW_ORDERS:
        R.check_ln_fwd(fw[o], case, fwd, fw, f"{o} forward")
        R.check_ln_bwd(bw[o], case, ref, bw, f"{o} backward")
    if fam in ("const", "zero"):       # zero variance: y is beta to fp32 rounding, rstd is eps^-1/2
        for o in R.ROW_ORDERS:
            assert (fw[o]["y32"].double() - case["beta"].double()).abs().max() <= R.V * case["beta"].abs().max()
            assert (fw[o]["rstd"].double() * R.EPS ** 0.5 - 1).abs().max() <= 4 * R.V


def test_envelope_constants_cover_what_the_yardsticks_measure():
    """LN_ENVELOPE is a record of a measurement: the yardsticks' own error over LN_CASES stays below it, and it is not padded"""
    env = R.measure_envelope()
    print("measured envelope:", {k: round(v, 2) for k, v in env.items()})
    for k, v in env.items():
        assert v <= R.LN_ENVELOPE[k], (k, v)
        assert R.LN_ENVELOPE[k] <= 2 * v, (k, v, "the recorded envelope is more than twice what is measured")


def test_p09_at_d8_drops_whole_rows():
    case = R.ln_case(257, 8, "unit", 0.9, "x16", 31)
    assert int((~case["keep"]).all(1).sum()) >= 1


@pytest.mark.parametrize("M,nb", [(5, 2), (257, 65), (1000, 64), (1000, 100)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_correct_partials_and_two_level_reduce_pass(M, nb, accumulate):
    case, fwd, m32, r32 = build(M, 40, "unit", 0.1, "x16", 3)
    init = {n: torch.randn(40) for n in ("dgamma", "dbeta", "dbias")}
    got = R.bwd32(case, m32, r32, "chunk", "blocks", nb=nb, init=init, accumulate=accumulate)
    judge_bwd(case, m32, r32, got, init, accumulate, nb=nb)
    # the partial rows alone, summed in float64, obey the same limits (what the partial-only form of the library leaves)
    parts = got["partials"].double().sum(0)
    ref = R.ln_bwd_ref(case, m32, r32)
    for i, n in enumerate(("dgamma", "dbeta", "dbias")):
        R.check_elem(parts[i * 40:(i + 1) * 40], ref[n], ref["mag_" + n], R.bwd_sum_factor(n, M), True, n)


# ------------------------------------------------------------------------------------------------ faulty forwards fail
def test_one_pass_variance_fails_on_offset_rows():
    case, fwd, _, _ = build(5, 512, "offset", 0.0, "x32")
    assert float((fwd["mean"].abs() * fwd["rstd"]).min()) >= 100
    for o in ("chunk", "quad"):
        fwd_fails(case, fwd, R.fwd32(case, o, "one_pass"))
    judge_fwd(case, fwd, R.fwd32(case, "chunk"))


def test_unbiased_variance_fails_at_d8():
    case, fwd, _, _ = build(5, 8, "unit", 0.0, "x16")
    fwd_fails(case, fwd, R.fwd32(case, "chunk", "unbiased"))


@pytest.mark.parametrize("fault", ["eps_outside", "no_eps"])
def test_misplaced_eps_fails_on_constant_rows(fault):
    case, fwd, _, _ = build(5, 8, "const", 0.0, "x16")
    fwd_fails(case, fwd, R.fwd32(case, "chunk", fault))


def test_statistics_of_the_bf16_rounded_sum_fail():
    case, fwd, _, _ = build(5, 520, "unit", 0.1, "x32")
    fwd_fails(case, fwd, R.fwd32(case, "chunk", "stats_bf16"))


def test_truncating_convert_fails():
    case, fwd, m32, r32 = build(5, 520, "unit", 0.1, "x16")
    fwd_fails(case, fwd, R.fwd32(case, "chunk", "trunc"))
    got = R.bwd32(case, m32, r32, "chunk")
    got["dX"] = R.bf16_trunc(got["dS32"])
    bwd_fails(case, m32, r32, got)


def test_last_chunk_left_out_of_the_row_sums_fails_at_d520():
    case, fwd, _, _ = build(5, 520, "unit", 0.1, "x16")
    fwd_fails(case, fwd, R.fwd32(case, "chunk", "drop_last_chunk"))


@pytest.mark.parametrize("fault", ["no_inv_keep", "inv_keep_resid"])
def test_misapplied_inv_keep_fails(fault):
    case, fwd, _, _ = build(5, 8, "unit", 0.1, "x16", 1000)
    assert not bool(case["keep"].all())
    fwd_fails(case, fwd, R.fwd32(case, "chunk", fault))


def test_mask_keyed_by_row_instead_of_row_index_fails():
    rows = np.array([7, 2, 40, 11, 3])
    case, fwd, m32, r32 = build(5, 40, "unit", 0.3, "x16", 1000, rows)
    wrong = R.with_keys(case, R.row_keys(5, 1000))
    assert not torch.equal(wrong["keep"], case["keep"])
    fwd_fails(case, fwd, R.fwd32(wrong, "chunk"))
    bwd_fails(case, m32, r32, R.bwd32(wrong, m32, r32, "chunk"))
    assert np.array_equal(hashrng.rows_mask(R.SEED, R.SITE, 5, 40, 0.3, 1000), wrong["keep"].numpy())


def test_mask_keyed_without_row_offset_fails():
    case, fwd, m32, r32 = build(5, 40, "unit", 0.3, "x16", 1000)
    wrong = R.with_keys(case, R.row_keys(5, 0))
    fwd_fails(case, fwd, R.fwd32(wrong, "chunk"))
    bwd_fails(case, m32, r32, R.bwd32(wrong, m32, r32, "chunk"))


# ------------------------------------------------------------------------------------------------ faulty backwards fail
@pytest.mark.parametrize("fault", ["no_c2", "c1_lanes", "dgamma_dyg"])
def test_wrong_backward_formulas_fail(fault):
    case, _, m32, r32 = build(5, 520, "unit", 0.0, "x16")
    judge_bwd(case, m32, r32, R.bwd32(case, m32, r32, "chunk"))
    bwd_fails(case, m32, r32, R.bwd32(case, m32, r32, "chunk", fault=fault))


def test_dbias_from_dS_fails_under_dropout():
    case, _, m32, r32 = build(5, 8, "unit", 0.1, "x16", 1000)
    assert not bool(case["keep"].all())
    bwd_fails(case, m32, r32, R.bwd32(case, m32, r32, "chunk", fault="dbias_dS"))


def test_look_ahead_row_consumed_twice_fails():
    case, _, m32, r32 = build(5, 8, "unit", 0.0, "x16")
    judge_bwd(case, m32, r32, R.bwd32(case, m32, r32, "quad", "blocks", nb=1), nb=1)
    bwd_fails(case, m32, r32, R.bwd32(case, m32, r32, "quad", "blocks", fault="lookahead_twice", nb=1), nb=1)


def test_accumulation_in_the_first_reduce_pass_fails_above_64_partials():
    case, _, m32, r32 = build(257, 8, "unit", 0.0, "x16")           # 65 partial rows
    init = {n: torch.randn(8) for n in ("dgamma", "dbeta", "dbias")}
    for acc in (False, True):
        judge_bwd(case, m32, r32, R.bwd32(case, m32, r32, "chunk", "blocks", nb=65, init=init, accumulate=acc), init, acc, nb=65)
        bwd_fails(case, m32, r32, R.bwd32(case, m32, r32, "chunk", "blocks", "first_pass_accumulates", 65, init, acc), init=init,
                  accumulate=acc, nb=65)


@pytest.mark.parametrize("M", [5, 257])
def test_accumulate_ignored_fails(M):
    case, _, m32, r32 = build(M, 8, "unit", 0.0, "x16")
    init = {n: 1 + torch.rand(8) for n in ("dgamma", "dbeta", "dbias")}
    bwd_fails(case, m32, r32, R.bwd32(case, m32, r32, "chunk", "blocks", "ignore_accumulate", None, init, True), init=init,
              accumulate=True)


# ------------------------------------------------------------------------------------------------ the reduce alone
def partial_rows(n, W, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n, W), generator=g).float() if integer else torch.randn(n, W, generator=g)


@pytest.mark.parametrize("n", R.REDUCE_NP)
@pytest.mark.parametrize("batch", [False, True])
def test_correct_reduce_passes_and_is_exact_on_integers(n, batch):
    for w in (8, 40):
        P = partial_rows(n, w, n + w)
        ref, mag = R.colsum_ref(P)
        R.check_sum(R.reduce32(P, batch=batch), ref, mag, n, "reduce")
        Pi = partial_rows(n, w, n, integer=True)
        assert torch.equal(R.reduce32(Pi, batch=batch).double(), Pi.double().sum(0))
        init = torch.randn(w)
        ref, mag = R.colsum_ref(P, init)
        R.check_sum(R.reduce32(P, init, True, batch), ref, mag, n + 1, "accumulating reduce")
    if n == 1:                         # one partial row: the reduce is a copy
        assert torch.equal(R.reduce32(P, batch=batch), P[0])


@pytest.mark.parametrize("n,fault,batch", [(9, "drop_mod8", False), (7, "drop_mod8", False), (33, "drop_mod32", True),
                                           (31, "drop_mod32", True), (100, "drop_mod8", False), (100, "drop_mod32", True)])
def test_last_partial_row_dropped_fails(n, fault, batch):
    P = partial_rows(n, 8, n)
    ref, mag = R.colsum_ref(P)
    with pytest.raises(AssertionError):
        R.check_sum(R.reduce32(P, batch=batch, fault=fault), ref, mag, n, "reduce")
    Pi = partial_rows(n, 8, n, integer=True) + 9.0                   # (every row is non-zero in every column)
    assert not torch.equal(R.reduce32(Pi, batch=batch, fault=fault).double(), Pi.double().sum(0))


def emulated_segments(P, w, nseg, outs, faulty_pointer=False, faulty_column=False):
    """the final stores of a 3-segment reduce into guarded destinations.  faulty_pointer: segment 2 stored through segment 1's
    pointer; faulty_column: the `col < w` test left out, so the last 32-column block stores its whole width"""
    for sg in range(nseg):
        t = R.reduce32(P[:, sg * w:(sg + 1) * w].contiguous())
        dst = outs[1 if (faulty_pointer and sg == 2) else sg]
        dst.view[0].copy_(t)
        if faulty_column and w % 32:
            flat = dst.full.view(-1)
            start = dst.guard * dst.ld
            flat[start + w:start + (w + 31) // 32 * 32] = 0.0


def test_segment_written_through_the_wrong_pointer_fails():
    w, n = 40, 9
    P = partial_rows(n, 3 * w + 8, 5)                                # pstride > nseg * w
    refs = R.reduce_ref(P, w, 3)
    outs = [R.Guarded(1, w, torch.float32, j=1, guard=2) for _ in range(3)]
    emulated_segments(P, w, 3, outs)
    for o, (ref, mag) in zip(outs, refs):
        R.check_sum(o.view[0], ref, mag, n, "segment")
        o.assert_intact("segment")
    outs = [R.Guarded(1, w, torch.float32, j=1, guard=2) for _ in range(3)]
    emulated_segments(P, w, 3, outs, faulty_pointer=True)
    with pytest.raises(AssertionError):                              # segment 2 was never stored: still poison
        R.check_sum(outs[2].view[0], refs[2][0], refs[2][1], n, "segment 2")
    with pytest.raises(AssertionError):
        R.check_sum(outs[1].view[0], refs[1][0], refs[1][1], n, "segment 1")


def test_column_past_w_written_is_reported_by_the_guard():
    w, n = 40, 9
    P = partial_rows(n, w, 6)
    out = [R.Guarded(1, w, torch.float32, j=1, guard=2)]
    emulated_segments(P, w, 1, out, faulty_column=True)
    assert out[0].violations() > 0
    with pytest.raises(AssertionError):
        out[0].assert_intact("segment")


# ------------------------------------------------------------------------------------------------ guards
def test_guards_report_a_store_one_row_below_and_8_columns_to_the_right():
    case, fwd, _, _ = build(5, 40, "unit", 0.0, "x16")
    y = R.fwd32(case, "chunk")["y"]
    ok = R.Guarded(5, 40, torch.bfloat16, j=0)
    ok.view.copy_(y)
    ok.assert_intact("y")
    below = R.Guarded(5, 40, torch.bfloat16, j=0)
    below.full[below.guard + 1:below.guard + 6].copy_(y)
    assert below.violations() == 40 * 2
    assert not torch.isfinite(below.view[0].float()).any()           # ... and the row that was skipped is still poison
    right = R.Guarded(5, 40, torch.bfloat16, j=0)
    flat = right.full.view(-1)
    flat[right.guard * 40 + 8:right.guard * 40 + 8 + 200].copy_(y.reshape(-1))
    assert right.violations() == 8 * 2
    vec = R.GuardedVec(5, torch.float32)
    vec.raw.view(torch.float32)[vec.guard + 1:vec.guard + 6] = 1.0   # mean stored at row + 1
    assert vec.violations() == 4
    with pytest.raises(AssertionError):
        vec.assert_intact("mean")


def test_rows_mask_is_rows_mask_at_with_consecutive_keys():
    a = hashrng.rows_mask(99, 3, 6, 24, 0.4, 4000)
    assert np.array_equal(a, hashrng.rows_mask_at(99, 3, np.arange(6) + 4000, 24, 0.4))
    assert np.array_equal(a[[4, 1]], hashrng.rows_mask_at(99, 3, np.array([4004, 4001]), 24, 0.4))
    assert np.array_equal(hashrng.rows_mask_at(99, 3, np.array([5]), 24, 0.4),
                          hashrng.rows_mask_at(99, 3, np.array([5 + (1 << 32)]), 24, 0.4))      # keys are taken modulo 2^32


# ------------------------------------------------------------------------------------------------ column sums and rowdot
@pytest.mark.parametrize("M", [1, 17, 1000])
def test_column_sum_and_rowdot_limits(M):
    g = torch.Generator().manual_seed(M)
    X = torch.randn(M, 40, generator=g).bfloat16()
    ref, mag = R.colsum_ref(X)
    for o in R.COL_ORDERS:
        R.check_sum(R.col_sum(X.float(), o), ref, mag, M, o)
    with pytest.raises(AssertionError):                              # last row left out
        R.check_sum(R.col_sum(X.float()[:-1], "torch"), ref, mag, M, "short")
    Z, w, b, dl = X, torch.randn(40, generator=g), torch.randn(1, generator=g), torch.randn(M, generator=g)
    ref, mag = R.rowdot_fwd_ref(Z, w, b)
    prod = Z.float() * w                                             # rowdot: every term one rounded product, then the sum
    for o in R.ROW_ORDERS:
        R.check_sum(R.row_sum(prod, o) + b, ref, mag, 41, f"logits {o}")
        R.check_sum(R.row_sum(prod, o), *R.rowdot_fwd_ref(Z, w), 40, f"logits {o}, no bias")
    with pytest.raises(AssertionError):
        R.check_sum(R.row_sum(prod, "chunk"), ref, mag, 41, "logits without the bias")
    dZ, (dw, mdw), (db, mdb) = R.rowdot_bwd_ref(dl, Z, w)
    dw0, db0 = torch.randn(40, generator=g), torch.randn(1, generator=g)
    _, (dwa, mdwa), (dba, mdba) = R.rowdot_bwd_ref(dl, Z, w, dw0, db0)
    for o in R.COL_ORDERS:
        R.check_sum(R.col_sum(dl[:, None] * Z.float(), o), dw, mdw, M, f"dw {o}")
        R.check_sum(R.col_sum(dl[:, None], o), db, mdb, M, f"db {o}")
        R.check_sum(dw0 + R.col_sum(dl[:, None] * Z.float(), o), dwa, mdwa, M + 1, f"dw {o}, accumulating")
        R.check_sum(db0 + R.col_sum(dl[:, None], o), dba, mdba, M + 1, f"db {o}, accumulating")
    if M == 1:                         # one row: a column sum is a copy
        assert torch.equal(R.col_sum(X.float(), "blocks"), X.float()[0])
    assert torch.equal(dZ, (dl[:, None] * w[None, :]).bfloat16())
