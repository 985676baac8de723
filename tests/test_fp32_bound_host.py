"""CPU suite: the limits of fp32_reference.py have teeth.  Every fp32 yardstick order, taken as the kernel, passes every check at
every case the GPU suite runs (test_gpu_fp32_attention_kernels.py, test_gpu_fp32_row_kernels.py); the measured envelope constants
cover what the yardsticks measure today; and each planted mistake fails its check at every case where it changes anything at all.
No GPU and no library call."""
import functools
import os

import pytest
import torch

import attn_reference as A
import fp32_reference as F
import rowops_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def attn_bundle(c):
    case = F.attn_case(c)
    ref, mag = F.attn_ref(case)
    return case, ref, mag, F.attn_yards(case)


def judge_attn(c, got, outputs=F.ATTN_OUTPUTS):
    case, ref, mag, yards = attn_bundle(c)
    return F.check_attn_all(got, case, F.attn_id(c), ref, mag, yards, outputs)


def changed(a, b):
    """outputs on which two results differ at all (NaN counts)"""
    return [n for n in F.ATTN_OUTPUTS if n in a and not torch.equal(torch.nan_to_num(a[n].double(), nan=1e300), torch.nan_to_num(b[n].double(), nan=1e300))]


# ------------------------------------------------------------------------------------------------ the tables reach the edges
def test_attention_table_reaches_every_edge():
    pad, pk = F.ATTN_PADDED, F.ATTN_PACKED
    for hd in (16, 32, 64, 96, 128):
        assert any(c[3] == hd for c in pad) and any(c[0] == hd for c in pk)
    for lq in (1, 16, 17, 63, 64, 65, 129):
        assert len({c[3] for c in pad if c[1] == lq}) + (len(pk) if lq in F.PACKED_LQ else 0) >= 2, lq
        assert len({c[3] for c in pad if c[1] == lq}) >= 1
    edges = [c for c in pad if c[4] == "edges"]
    assert len({c[3] for c in edges}) >= 2 and all(c[0] == 12 and c[2] == 130 for c in edges)
    lens = set((~A.key_padding_mask("edges", 12, 130)).sum(1).tolist())
    assert lens == set(A.EDGE_LENGTHS) | {129, 130}
    assert {c[4] for c in pad} == {"none", "prefix", "edges", "leading", "allpad"} and {c[5] for c in pad} == {0.0, 0.1} == {p for _, p in pk}
    assert set(F.PACKED_LQ) == set(F.PACKED_LK) == lens | {0} and F.PACKED_LQ != F.PACKED_LK
    mid = F.PACKED_LQ.index(0)
    assert 0 < mid < len(F.PACKED_LQ) - 1 and F.PACKED_LK[mid] == 0


def test_row_tables_reach_every_edge():
    assert [F.colsum_slices(M) for M in (1, 64, 65, 4095, 4097)] == [(1, 1), (1, 64), (2, 33), (64, 64), (64, 65)]
    assert 4097 - 63 * 65 == 2                                     # the short last slice
    assert {F.colsum_slices(M)[1] for M in F.COLSUM_M} >= {1, 64, 65}
    M, K = F.SPLIT_SECOND_TRIP
    assert M * K // 4 > F.GRID_CAP_VECTORS >= (M - 5) * K // 4
    B, L, d = F.FUSE_SECOND_TRIP
    assert B * L * d // 4 > F.GRID_CAP_VECTORS
    assert any(c[0] > 2048 for c in F.LN32_BWD_CASES) and {c[1] for c in F.LN32_FWD_CASES} >= set(F.LN32_WIDTHS)
    assert {c[1] for c in F.LN32_BWD_CASES} >= set(F.LN32_BWD_WIDTHS) and {c[0] for c in F.LN32_BWD_CASES if c[1] == 260} >= set(F.LN32_BWD_ROWS)
    for flag in (6, 7):                                             # rows entry, Y16; and for the backward dbias, accumulate
        assert {c[flag] for c in F.LN32_FWD_CASES} == {False, True}
    for flag in (6, 7, 8):
        assert {c[flag] for c in F.LN32_BWD_CASES} == {False, True}
    assert {c[2] for c in F.LN32_FWD_CASES} == {"unit", "offset", "const"} and {c[4] for c in F.LN32_FWD_CASES} == {"x32", "none"}
    ri = F.row_index_of(7)
    assert (ri[1:] < ri[:-1]).any() and len(set(ri[:5].tolist())) < 5


def test_coverage_names_every_fp32_export_and_existing_tests():
    with open(os.path.join(HERE, "..", "include", "hriemo.h")) as f:
        names = F.header_fp32_exports(f.read())
    cov = F.coverage()
    assert len(names) >= 30 and "hriemo_attn_bwd_f32_varlen" in names and "hriemo_split_bf16x3" in names
    assert sorted(set(names) - set(cov)) == [], "exports that no test is recorded for"
    assert sorted(set(cov) - set(names)) == [], "recorded names the header does not export"
    with open(os.path.join(HERE, "..", "hri-emo_amd", "csrc", "fp32mode.hip")) as f:
        src = f.read()
    for n in names:
        if f" {n}(" in src:
            assert any(t.startswith("test_gpu_fp32_") for t in cov[n]), n
    for n, tests in cov.items():
        for t in tests:
            fn, _, test = t.partition("::")
            with open(os.path.join(HERE, fn)) as f:
                text = f.read()
            assert not test or f"def {test}(" in text, (n, t)


# ------------------------------------------------------------------------------------------------ attention: correct orders pass
@pytest.mark.parametrize("c", F.ATTN_CASES, ids=F.attn_id)
def test_every_attention_order_passes(c):
    case, ref, mag, yards = attn_bundle(c)
    for o, y in yards.items():
        r = judge_attn(c, y)
        assert all(e <= 1 and t <= 1 for e, t in r.values()), (o, r)
    # PAD keys: zero magnitude, so the limit demands exact zeros of dK / dV rows and of the map's columns
    if case["kpm"] is not None:
        pad = case["kpm"][case["live"]]
        assert float(mag["dK"].transpose(1, 2)[pad].abs().max() if pad.any() else 0.0) == 0.0
        assert float(mag["Pmean"][:, 0].transpose(1, 2)[pad].abs().max() if pad.any() else 0.0) == 0.0


def test_envelope_constants_cover_what_the_yardsticks_measure():
    """ATTN_ENVELOPE and LN32_ENVELOPE are records of a measurement: the yardsticks stay below them, and they are not padded"""
    for env, const in ((F.measure_attn(), F.ATTN_ENVELOPE), (F.measure_ln32(), F.LN32_ENVELOPE)):
        print("measured envelope:", {k: round(v, 2) for k, v in env.items()})
        for k, v in env.items():
            assert v <= const[k], (k, v)
            assert const[k] <= 2 * v, (k, v, "the recorded envelope is more than twice what is measured")


# ------------------------------------------------------------------------------------------------ attention: planted mistakes fail
def _set(x, idx, val):
    y = x.clone()
    y[idx] = val
    return y


def _hooks(kind, case):
    ik = torch.tensor(case["ik"], dtype=torch.float32)
    Lq, Lk = case["Lq"], case["Lk"]
    if kind == "key63_dropped":
        return {"P": lambda x: _set(x, (..., 63), 0.0)} if Lk > 63 else None
    if kind == "keys64_127_not_rescaled":
        return {"Pd": lambda x: _set(x, (..., slice(64, 128)), x[..., 64:128] / ik)} if Lk > 64 and case["p"] > 0 else None
    if kind == "dP_not_rescaled":
        return {"dP": lambda x: x / ik} if case["p"] > 0 else None
    if kind == "delta_from_row_before":
        return {"delta": lambda x: _set(x, (..., -1), x[..., -2])} if Lq > 1 else None
    if kind == "dS_last_three_keys":
        return {"dS": lambda x: _set(x, (..., -1, slice(Lk - 3, Lk)), 0.0)}
    raise ValueError(kind)


HOOK_MUTANTS = ("key63_dropped", "keys64_127_not_rescaled", "dP_not_rescaled", "delta_from_row_before", "dS_last_three_keys")


@pytest.mark.parametrize("kind", HOOK_MUTANTS)
def test_attention_mutants_fail_wherever_they_change_anything(kind):
    hit = 0
    for c in F.ATTN_CASES:
        case, ref, mag, yards = attn_bundle(c)
        hooks = _hooks(kind, case)
        if hooks is None:
            continue
        got = F.attn_yard32(case, "torch", hooks)
        diff = changed(got, yards["torch"])
        if not diff:
            continue
        hit += 1
        bad = [o for o in F.ATTN_OUTPUTS if max(F.attn_ratios(got[o], ref[o], [y[o] for y in yards.values()], mag[o], o)) > 1.0]
        assert bad, (kind, F.attn_id(c), "changes", diff, "and passes every check")
        with pytest.raises(AssertionError):
            judge_attn(c, got)
    assert hit >= 4, (kind, hit)


@pytest.mark.parametrize("c", F.ATTN_CASES, ids=F.attn_id)
def test_a_kernel_that_rounds_to_bf16_anywhere_fails_the_fp32_limits(c):
    """attn_reference.yardstick: float64 with bf16 roundings of P, O, dS and of the stored gradients -- far outside every fp32 limit"""
    case, ref, mag, yards = attn_bundle(c)
    q, k, v, do, kpm, keep = F._live4(case, torch.float64)
    y = A.yardstick(q, k, v, do, kpm, keep, case["ik"])
    for o in A.OUTPUTS:
        e, t = F.attn_ratios(y[o], ref[o], [yy[o] for yy in yards.values()], mag[o], o)
        assert e > 1.0 and t > 1.0, (o, e, t)


def test_lse_without_the_last_tiles_running_max_fails():
    hit = 0
    for c in F.ATTN_CASES:
        case, ref, mag, yards = attn_bundle(c)
        for o in ("tiles", "tiles_rev"):
            got = F.attn_yard32(case, o, fault="lse_stale_max")
            if not changed(got, yards[o]):
                continue
            hit += 1
            assert changed(got, yards[o]) == ["lse"]
            with pytest.raises(AssertionError):
                judge_attn(c, got, ("lse",))
    assert hit >= len(F.ATTN_CASES)          # (single-tile cases change as well: their lse becomes -inf)


def test_delta_bound_is_the_n_term_rule():
    case, ref, mag, yards = attn_bundle(F.ATTN_CASES[1])
    dref, dmag = F.delta_ref(case)
    q, k, v, do, kpm, keep = F._live4(case, torch.float32)
    got = (do * yards["tiles"]["O"]).sum(-1)
    R.check_elem(got, dref, dmag, F.delta_factor(case["hd"]), True, "delta")
    with pytest.raises(AssertionError):
        R.check_elem(torch.roll(got, 1, -1), dref, dmag, F.delta_factor(case["hd"]), True, "delta of the row before")


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_got(case, order, **kw):
    fw = R.fwd32(case, order)
    bw = R.bwd32(case, fw["mean"], fw["rstd"], order, "blocks", **kw)
    return fw, {"dS": bw["dS32"], "dG": bw["dG32"], "dgamma": bw["dgamma"], "dbeta": bw["dbeta"], "dbias": bw["dbias"]}


@pytest.mark.parametrize("c", F.LN32_FWD_CASES, ids=F.ln32_id)
def test_every_layernorm_forward_order_passes(c):
    case = F.ln32_case(c)
    f, _ = F.ln32_refs(case)
    for o in R.ROW_ORDERS:
        fw = R.fwd32(case, o)
        F.check_ln32_fwd(fw["y32"], fw["y32"].bfloat16(), f, f"{o} forward")
    d = c[1]
    if d >= 16:
        bad = R.fwd32(case, "quad", "drop_last_chunk")
        if not torch.equal(bad["y32"], R.fwd32(case, "quad")["y32"]):
            with pytest.raises(AssertionError):
                F.check_ln32_fwd(bad["y32"], None, f, "last chunk skipped")
    y32 = R.fwd32(case, "torch")["y32"]
    if not torch.equal(R.bf16_trunc(y32), y32.bfloat16()):
        with pytest.raises(AssertionError):
            F.check_ln32_fwd(y32, R.bf16_trunc(y32), f, "Y16 truncated")


@pytest.mark.parametrize("c", F.LN32_BWD_CASES, ids=F.ln32_id)
def test_every_layernorm_backward_order_passes_and_faults_fail(c):
    M, d, fam, p, resid, roff, rows, dbias, acc = c
    case = F.ln32_case(c)
    g = torch.Generator().manual_seed(M + d)
    init = {n: F.far_init(d, g) for n in ("dgamma", "dbeta", "dbias")} if acc else None
    _, b = F.ln32_refs(case, init)
    nb = min((M + 3) // 4, 512)
    for o in R.ROW_ORDERS:
        _, got = _ln_got(case, o, nb=nb, init=init, accumulate=acc)
        F.check_ln32_bwd(got, case, b, f"{o} backward", acc)
    # last block's look-ahead row counted twice: dgamma / dbeta / dbias
    _, got = _ln_got(case, "quad", fault="lookahead_twice", nb=nb, init=init, accumulate=acc)
    with pytest.raises(AssertionError):
        F.check_ln32_bwd(got, case, b, "row counted twice", acc)
    if acc:                                   # stale destination: the reduce overwrites where it must add
        _, got = _ln_got(case, "quad", fault="ignore_accumulate", nb=nb, init=init, accumulate=True)
        with pytest.raises(AssertionError):
            F.check_ln32_bwd(got, case, b, "accumulate ignored", True)
    _, good = _ln_got(case, "quad", nb=nb, init=init, accumulate=acc)
    _, got = _ln_got(case, "quad", fault="no_c2", nb=nb, init=init, accumulate=acc)
    if not torch.equal(got["dS"], good["dS"]):          # (zero-variance rows: xhat = 0, the term is not there)
        with pytest.raises(AssertionError):
            F.check_ln32_bwd(got, case, b, "no c2", acc)


# ------------------------------------------------------------------------------------------------ column sums, rowdot
@pytest.mark.parametrize("M", F.COLSUM_M)
def test_colsum_emulation_passes_and_faults_fail(M):
    g = torch.Generator().manual_seed(M)
    for N in (1, 257):
        X = torch.randn(M, N, generator=g)
        mask = torch.randn(M, N, generator=g)
        init = F.far_init(N, g)                  # a destination no limit mistakes for rounding: |init| >= 50
        for mk, acc in ((None, False), (mask, True), (None, True)):
            t = X if mk is None else X * (mk > 0)
            ref, mag = R.colsum_ref(t, init if acc else None)
            n = M + (1 if acc else 0)
            R.check_sum(F.colsum32(X, mk, init, acc), ref, mag, n, "colsum32")
            R.check_sum(R.reduce32(t.float(), init, acc), ref, mag, n, "reduce32")
            if acc:
                for got in (F.colsum32(X, mk, init, acc, "ignore_accumulate"), R.reduce32(t.float(), init, acc, fault="ignore_accumulate")):
                    with pytest.raises(AssertionError):
                        R.check_sum(got, ref, mag, n, "stale destination")
            _, per = F.colsum_slices(M)
            # (n v mag is a few tenths at 4095 rows: of the 257 columns some always show three dropped rows, a single column need not)
            if mk is None and N > 1 and (min(per, M) % 4 or M % per % 4):
                with pytest.raises(AssertionError):
                    R.check_sum(F.colsum32(X, None, init, acc, "drop_tail"), ref, mag, n, "tail rows dropped")


@pytest.mark.parametrize("M", F.ROWDOT_M)
@pytest.mark.parametrize("d", F.ROWDOT_D)
def test_rowdot_bwd_bounds(M, d):
    g = torch.Generator().manual_seed(M * d)
    dl, Z, w = torch.randn(M, generator=g), torch.randn(M, d, generator=g), torch.randn(d, generator=g)
    dw0, db0 = torch.randn(d, generator=g), torch.randn(1, generator=g)
    _, (dw, mdw), (db, mdb) = R.rowdot_bwd_ref(dl, Z, w, dw0, db0)
    got = dw0.clone()
    for r in range(M):
        got = got + dl[r] * Z[r]
    R.check_sum(got, dw, mdw, M + 2, "dw")
    with pytest.raises(AssertionError):
        R.check_sum(got - dw0, dw, mdw, M + 2, "dw: stale destination")
    with pytest.raises(AssertionError):
        R.check_sum(got - dl[M - 1] * Z[M - 1], dw, mdw, M + 2, "dw: last row dropped")
    R.check_sum(db0 + dl.sum(), db, mdb, M + 1, "db")


# ------------------------------------------------------------------------------------------------ operand splits
@pytest.mark.parametrize("form", range(8))
def test_split_layouts_and_the_exact_sum_identity(form):
    M, K = 5, 12
    x = F.split_inputs(M, K)
    t, hi, mid, lo = F.split_host(x)
    Y = F.split_layout(form, hi, mid, lo)
    assert tuple(Y.shape) == ((M, (6 if form >= 4 else 3) * K) if form in (0, 1, 4, 5) else ((6 if form >= 4 else 3) * M, K))
    blocks = F.split_blocks(form, Y, M, K)
    names = {0: "hmh", 1: "hhm", 2: "hmh", 3: "hhm", 4: "hmlhmh", 5: "hhhmml", 6: "hmlhmh", 7: "hhhmml"}[form]
    for blk, n in zip(blocks, names):
        assert torch.equal(blk.view(torch.int16), {"h": hi, "m": mid, "l": lo}[n].view(torch.int16))
    assert bool((mid.float()[(hi.float().abs() > t.abs())] != 0).any())           # some hi rounded away from zero: mid has the other sign
    assert bool(((mid.float() * t) < 0).any())
    if form >= 4:
        assert F.split_sum_exact(form, Y, t) == 0
        for fault in ("mid_from_unrounded_hi", "lo_dropped"):
            _, h2, m2, l2 = F.split_host(x, fault=fault)
            assert F.split_sum_exact(form, F.split_layout(form, h2, m2, l2), t) > 0, fault


def test_split_relu_and_mask_on_the_host():
    x = F.split_inputs(5, 264)
    mask = torch.randn(5, 264)
    t, hi, mid, lo = F.split_host(x, relu=True, mask=mask)
    assert bool((t >= 0).all()) and bool((t[mask <= 0] == 0).all()) and bool((t[(mask > 0) & (x > 0)] == x[(mask > 0) & (x > 0)]).all())
    assert F.split_sum_exact(4, F.split_layout(4, hi, mid, lo), t) == 0


def test_dropout_host_matches_the_hash():
    import hashrng
    X = torch.randn(7, 12)
    y = F.dropout_host(X, False, None, 0.25, F.SEED, F.SITE, 11)
    keep = torch.from_numpy(hashrng.rows_mask(F.SEED, F.SITE, 7, 12, 0.25, 11))
    assert bool((y[~keep] == 0).all()) and torch.equal(y[keep], X[keep] * torch.tensor(R.inv_keep32(0.25)))
    assert 0 < int((~keep).sum()) < keep.numel()
