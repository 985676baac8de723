"""GPU suite, beta-gate / pool / fuse kernels (hri-emo_amd/csrc/rowops.hip) and the legacy scalar gate through the C-ABI against
gate_reference.py: float64 references, limits from the reference and the fp32 yardstick orders alone.  Every input sits in a poisoned
buffer between guards, every output is pre-filled with 0xFF between guards and compared with them afterwards; each kernel runs on
inputs of its own, so no limit inherits another kernel's error:

  1. hriemo_ln_pool_fwd at every width where the per-lane chunk count changes, around 4 waves and one 32-row chunk, every mask
     family (a fully masked sample in the middle), both source forms, Lkeep in {0, 1, mid-chunk, chunk edge, L}
  2. gate_input, sigmoid_beta, fuse_fwd (and the second trip of its grid-stride loop), fuse_bwd_dw, gate_dpre, gate_input_bwd
  3. hriemo_ln_pool_bwd: the same edges around the 16-row chunk, both coefficients, Lf cases, accumulation into non-zero destinations,
     the partial-only form, more than 64 partial rows into the reduce, the workspace at exactly its documented size
  4. the pair launches against the same references (and bit for bit against the single launches)
  5. the legacy scalar gate; the error returns

test_gate_bound_host.py proves on the CPU that these limits pass correct kernels in every summation order and fail faulty ones."""
import pytest
import torch

import gate_reference as G
import rowops_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib.lib()


def call(name, *args):
    from hri_emo_amd import _lib
    _lib.call(name, *args)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(b):
    return None if b is None else b.ptr


def mat(x):
    """a [.., d] tensor as a guarded [rows, d] matrix"""
    return None if x is None else R.Guarded.of(x.reshape(-1, x.shape[-1]), j=0, guard=GUARD, device=DEV)


def vec(x):
    return None if x is None else R.GuardedVec.of(x, device=DEV)


def mask8(m):
    return None if m is None else vec(m.to(torch.uint8))


def omat(rows, d, dtype):
    return R.Guarded(rows, d, dtype, j=0, guard=GUARD, device=DEV)


def ovec(n, dtype=torch.float32):
    return R.GuardedVec(n, dtype, device=DEV)


def intact(bufs, name):
    torch.cuda.synchronize()
    for n, b in bufs.items():
        if b is not None:
            b.assert_intact(f"{name}: {n}")


def untouched(b):
    return bool((b.view.contiguous().view(torch.uint8) == 0xFF).all())


def show(name, r):
    print(name, {k: round(v, 3) for k, v in r.items()} if isinstance(r, dict) else round(r, 3))


# ------------------------------------------------------------------------------------------------ launches
def fwd_bufs(side, Lkeep):
    B, Ls, d, ln = side["B"], side["L"], side["d"], side["ln"]
    return {"X": mat(ln["X"]), "X32": mat(ln["X32"]), "mask": mask8(side["mask"]), "gamma": vec(ln["gamma"]), "beta": vec(ln["beta"]),
            "Yn": omat(B * Lkeep + 2, d, torch.bfloat16),             # too large by two rows, which must stay 0xFF
            "mean": ovec(B * Ls), "rstd": ovec(B * Ls), "part": omat(B * G.chunks(Ls, G.POOL_ROWS), d, torch.float32)}


def fwd_args(b, side, Lkeep):
    return (ptr(b["X"]), ptr(b["X32"]), ptr(b["mask"]), b["gamma"].ptr, b["beta"].ptr, b["Yn"].ptr, b["mean"].ptr, b["rstd"].ptr, b["part"].ptr)


def fwd_out(b, side, Lkeep, name):
    B, Ls, d = side["B"], side["L"], side["d"]
    intact(b, name)
    yn = b["Yn"].view.cpu()
    G.check_untouched(yn, B * Lkeep, name + " Yn")
    return {"y": yn[:B * Lkeep].view(B, Lkeep, d), "mean": b["mean"].view.cpu(), "rstd": b["rstd"].view.cpu(),
            "part": b["part"].view.cpu().view(B, -1, d)}


def run_fwd(side, Lkeep, name):
    b = fwd_bufs(side, Lkeep)
    call("hriemo_ln_pool_fwd", *fwd_args(b, side, Lkeep), side["B"], side["L"], Lkeep, side["d"], R.EPS, stream())
    return fwd_out(b, side, Lkeep, name)


def judge_fwd(got, side, Lkeep, name):
    yards = {o: G.pool_fwd32(side, Lkeep, o, "waves") for o in R.ROW_ORDERS}
    r = G.check_pool_fwd(got, side, G.pool_fwd_ref(side, Lkeep), yards, Lkeep, name)
    show(name, r)
    return r


def bwd_bufs(L, side, ops, m32, r32, reduce=True, accumulate=False, init=None):
    B, Ls, d, ln = side["B"], side["L"], side["d"], side["ln"]
    wsn = L.hriemo_ln_pool_bwd_workspace_bytes(B, Ls, d) // 4
    nc = L.hriemo_ln_pool_bwd_chunks(Ls)
    assert nc == G.chunks(Ls, G.BWD_ROWS) and wsn == (B * nc + 64) * 2 * d
    dH = ops["dH"]
    if dH is not None and ops["Lf"] == 0:
        dH_b = omat(1, d, torch.bfloat16)                             # no row may be read: the buffer is poison throughout
    else:
        dH_b = mat(dH)
    b = {"dH": dH_b, "w": vec(ops["w"]) if dH is not None else None, "dpool": mat(ops["dpool"]), "mask": mask8(side["mask"]),
         "X": mat(ln["X"]), "X32": mat(ln["X32"]), "gamma": vec(ln["gamma"]), "mean": vec(m32), "rstd": vec(r32),
         "dX": omat(B * Ls, d, torch.bfloat16), "workspace": R.GuardedVec(wsn, torch.float32, guard=1024, device=DEV)}
    for n in ("dgamma", "dbeta"):
        b[n] = None if not reduce else vec(init[n]) if accumulate else ovec(d)
    return b


def bwd_side_args(b):
    return (b["dpool"].ptr, ptr(b["mask"]), ptr(b["X"]), ptr(b["X32"]), b["gamma"].ptr, b["mean"].ptr, b["rstd"].ptr, b["dX"].ptr,
            ptr(b["dgamma"]), ptr(b["dbeta"]))


def bwd_out(L, b, side, name, reduce):
    B, Ls, d = side["B"], side["L"], side["d"]
    intact(b, name)
    nc = L.hriemo_ln_pool_bwd_chunks(Ls)
    ws = b["workspace"].view.cpu()
    if not reduce or B * nc <= 64:                                    # the scratch of the two-level reduce: not needed, not touched
        G.check_untouched(ws, B * nc * 2 * d, name + " workspace")
    return {"dX": b["dX"].view.cpu().view(B, Ls, d), "part": ws[:B * nc * 2 * d].view(B, nc, 2 * d),
            "dgamma": b["dgamma"].view.cpu() if reduce else None, "dbeta": b["dbeta"].view.cpu() if reduce else None}


def run_bwd(L, side, ops, is_a, m32, r32, name, reduce=True, accumulate=False, init=None):
    b = bwd_bufs(L, side, ops, m32, r32, reduce, accumulate, init)
    call("hriemo_ln_pool_bwd", ptr(b["dH"]), ops["Lf"], ptr(b["w"]), is_a, *bwd_side_args(b), int(accumulate), side["B"], side["L"], side["d"],
         b["workspace"].ptr, stream())
    return bwd_out(L, b, side, name, reduce)


def judge_bwd(got, side, ops, is_a, m32, r32, name, accumulate=False, init=None):
    yards = {o: G.pool_bwd32(side, ops, is_a, m32, r32, o, "torch") for o in R.ROW_ORDERS}
    yards["contract"] = G.pool_bwd32(side, ops, is_a, m32, r32, "chunk", "torch", contract=True)
    ref = G.pool_bwd_ref(side, ops, is_a, m32, r32, init if accumulate else None)
    r = G.check_pool_bwd(got, side, ref, yards, name, accumulate)
    show(name, r)
    return r


# ------------------------------------------------------------------------------------------------ 1. ln_pool_fwd
@pytest.mark.parametrize("c", G.FWD_CASES, ids=G.fwd_id)
def test_ln_pool_fwd(L, c):
    B, Ls, Lk, d, fam, twin, mask = c
    side = G.gate_side(B, Ls, d, fam, twin, mask)
    name = G.fwd_id(c)
    got = run_fwd(side, Lk, name)
    judge_fwd(got, side, Lk, name)
    if mask == "full":
        assert (got["part"][B // 2] == 0).all(), "a fully masked sample pools exact zeros"


# ------------------------------------------------------------------------------------------------ 2. the small gate kernels
@pytest.mark.parametrize("d", [8, 520, 4096])
@pytest.mark.parametrize("nca,nct,mask", G.GATE_INPUT_CASES)
def test_gate_input(L, d, nca, nct, mask):
    B = 3
    c = G.gate_input_case(B, nca, nct, d, mask)
    assert L.hriemo_pool_chunks(c["La"]) == nca and L.hriemo_pool_chunks(c["Lt"]) == nct
    valid_a = G.counts(c["ma"], B, c["La"], clamp=False)
    if mask == "full":                 # the middle sample has no valid audio row: its reference cnt is 1 by the clamp, not by a count
        assert valid_a[B // 2] == 0 and G.gate_input_ref(c)["cnt"][B // 2, 0] == 1 and (valid_a[[0, 2]] > 1).all()
    elif mask == "single":
        assert valid_a[0] == 1
    else:
        assert (valid_a > 1).all()
    b = {"pa": mat(c["pa"]), "pt": mat(c["pt"]), "ma": mask8(c["ma"]), "mt": mask8(c["mt"]), "gin": omat(B, 4 * d, torch.bfloat16),
         "a": omat(B, d, torch.float32), "t": omat(B, d, torch.float32), "cnt": ovec(2 * B)}
    call("hriemo_gate_input", b["pa"].ptr, b["pt"].ptr, ptr(b["ma"]), ptr(b["mt"]), B, c["La"], c["Lt"], d, b["gin"].ptr, b["a"].ptr, b["t"].ptr,
         b["cnt"].ptr, stream())
    name = f"gate_input d={d} chunks {nca}|{nct} {mask}"
    intact(b, name)
    got = {"cnt": b["cnt"].view.cpu().view(B, 2), "a": b["a"].view.cpu(), "t": b["t"].view.cpu(), "gin": b["gin"].view.cpu()}
    show(name, G.check_gate_input(got, c, G.gate_input_ref(c), {o: G.gate_input32(c, o) for o in G.SEQ_ORDERS}, name))
    # the legacy entry point on the pools this one produced (inputs from here on)
    a_b, t_b, gin2 = mat(got["a"]), mat(got["t"]), omat(B, 4 * d, torch.bfloat16)
    call("hriemo_gate_input_pooled", a_b.ptr, t_b.ptr, gin2.ptr, B, d, stream())
    intact({"a": a_b, "t": t_b, "gin": gin2}, name + " pooled")
    G.check_gate_input_pooled(gin2.view.cpu(), got["a"], got["t"], name + " pooled")


@pytest.mark.parametrize("d", G.WIDTHS)
def test_sigmoid_beta(L, d):
    B = 3
    pre = G.sigmoid_inputs(B, d)
    b = {"pre": mat(pre), "w": omat(B, d, torch.float32), "beta": ovec(B)}
    call("hriemo_sigmoid_beta", b["pre"].ptr, b["w"].ptr, b["beta"].ptr, B, d, stream())
    intact(b, f"sigmoid_beta d={d}")
    show(f"sigmoid_beta d={d}", G.check_sigmoid_beta(b["w"].view.cpu(), b["beta"].view.cpu(), pre, f"sigmoid_beta d={d}"))


def run_fuse_fwd(c, name):
    B, Ls, d = c["B"], c["L"], c["d"]
    b = {"w": mat(c["w"]), "A": mat(c["A"]), "T": mat(c["T"]), "H": omat(B * Ls, d, torch.bfloat16)}
    call("hriemo_fuse_fwd", b["w"].ptr, b["A"].ptr, b["T"].ptr, b["H"].ptr, B, Ls, d, stream())
    intact(b, name)
    return b["H"].view.cpu().view(B, Ls, d)


@pytest.mark.parametrize("B,Ls,d", [(3, 5, 8), (3, 37, 520), (1, 1, 4096), (2, 33, 2056)])
def test_fuse_fwd(L, B, Ls, d):
    c = G.fuse_case(B, Ls, d)
    name = f"fuse_fwd {B}x{Ls}x{d}"
    show(name, G.check_fuse_fwd(run_fuse_fwd(c, name), c, name))


def test_fuse_fwd_second_trip_of_the_grid_stride_loop(L):
    B, Ls, d = G.SECOND_TRIP
    assert B * Ls * (d // 8) > G.GRID_CAP * G.BLOCK and G.second_trip(B, Ls, d), "the capped grid covers every vector in one trip"
    c = G.fuse_case(B, Ls, d)
    name = f"fuse_fwd {B}x{Ls}x{d}"
    show(name, G.check_fuse_fwd(run_fuse_fwd(c, name), c, name))


@pytest.mark.parametrize("d", G.WIDTHS)
def test_fuse_bwd_dw(L, d):
    """every DISPATCH_NCH instance; 70 rows: two full chunks and one in which the waves own 1-2 rows; 33: three waves without a row"""
    for B, Ls in ((2, 70), (3, 33)) if d in (520, 1032, 2056) else ((2, 37),):
        c = G.fuse_case(B, Ls, d)
        b = {"dH": mat(c["dH"]), "A": mat(c["A"]), "T": mat(c["T"]), "part": omat(B * G.chunks(Ls, G.POOL_ROWS), d, torch.float32)}
        call("hriemo_fuse_bwd_dw", b["dH"].ptr, b["A"].ptr, b["T"].ptr, b["part"].ptr, B, Ls, d, stream())
        name = f"fuse_bwd_dw<{G.nch(d)}> {B}x{Ls}x{d}"
        intact(b, name)
        show(name, G.check_fuse_bwd_dw(b["part"].view.cpu().view(B, -1, d), c, name))


@pytest.mark.parametrize("d", [8, 520, 4096])
@pytest.mark.parametrize("nc", G.CHUNK_COUNTS)
@pytest.mark.parametrize("dbeta", [True, False])
def test_gate_dpre(L, d, nc, dbeta):
    B = 3
    c = G.dpre_case(B, nc, d, dbeta)
    assert L.hriemo_pool_chunks(c["L"]) == nc
    b = {"part": mat(c["part"]), "dbeta": vec(c["dbeta"]), "w": mat(c["w"]), "dpre": omat(B, d, torch.bfloat16)}
    call("hriemo_gate_dpre", b["part"].ptr, c["L"], ptr(b["dbeta"]), b["w"].ptr, b["dpre"].ptr, B, d, stream())
    name = f"gate_dpre d={d} chunks={nc} dbeta={dbeta}"
    intact(b, name)
    show(name, G.check_gate_dpre(b["dpre"].view.cpu(), c, {o: G.gate_dpre32(c, o) for o in G.SEQ_ORDERS}, name))


@pytest.mark.parametrize("d", [8, 520, 4096])
def test_gate_input_bwd(L, d):
    B = 3
    c = G.gin_bwd_case(B, d)
    b = {"dgin": mat(c["dgin"]), "a": mat(c["a"]), "t": mat(c["t"]), "cnt": vec(c["cnt"]), "da": omat(B, d, torch.float32), "dt": omat(B, d, torch.float32)}
    call("hriemo_gate_input_bwd", b["dgin"].ptr, b["a"].ptr, b["t"].ptr, b["cnt"].ptr, b["da"].ptr, b["dt"].ptr, B, d, stream())
    intact(b, f"gate_input_bwd d={d}")
    show(f"gate_input_bwd d={d}", G.check_gin_bwd({"da": b["da"].view.cpu(), "dt": b["dt"].view.cpu()}, c, f"gate_input_bwd d={d}"))


# ------------------------------------------------------------------------------------------------ 3. ln_pool_bwd
@pytest.mark.parametrize("c", G.BWD_CASES, ids=G.bwd_id)
def test_ln_pool_bwd(L, c):
    side, ops, m32, r32 = G.make_bwd(c)
    name = G.bwd_id(c)
    got = run_bwd(L, side, ops, c[7], m32, r32, name)
    judge_bwd(got, side, ops, c[7], m32, r32, name)


@pytest.mark.parametrize("d", [520, 1032])
@pytest.mark.parametrize("B,Ls", [(3, 21), G.MANY_PARTIALS[:2]])
def test_ln_pool_bwd_operand_forms(L, d, B, Ls):
    """accumulate = 0 | 1 into non-zero destinations and the partial-only form, on both sides of the 64-partial threshold of
    launch_colreduce and on both constant-placement paths"""
    c = (B, Ls, min(Ls, 37), d, "unit", True, "scattered", 1, True)
    side, ops, m32, r32 = G.make_bwd(c)
    name = "forms " + G.bwd_id(c)
    nc = L.hriemo_ln_pool_bwd_chunks(Ls)
    assert (B * nc > 64) == (Ls == G.MANY_PARTIALS[1])
    g = torch.Generator().manual_seed(B + d)
    init = {n: 1.0 + torch.rand(d, generator=g) for n in ("dgamma", "dbeta")}
    plain = run_bwd(L, side, ops, 1, m32, r32, name)
    judge_bwd(plain, side, ops, 1, m32, r32, name)
    acc = run_bwd(L, side, ops, 1, m32, r32, name + " accumulate", accumulate=True, init=init)
    judge_bwd(acc, side, ops, 1, m32, r32, name + " accumulate", True, init)
    part = run_bwd(L, side, ops, 1, m32, r32, name + " partial-only", reduce=False)
    judge_bwd(part, side, ops, 1, m32, r32, name + " partial-only")
    assert torch.equal(part["part"], plain["part"]) and torch.equal(part["dX"], plain["dX"])


# ------------------------------------------------------------------------------------------------ 4. the pair launches
@pytest.mark.parametrize("d", G.PAIR_WIDTHS)
@pytest.mark.parametrize("La,Lt,Lk", [(70, 33, 33), (33, 5, 4), (37, 32, 0)])
def test_ln_pool_fwd_pair(L, d, La, Lt, Lk):
    B = 3
    assert L.hriemo_ln_pool_pair_supported(d) == 1
    sa, st = G.gate_side(B, La, d, "unit", True, "scattered", seed=d + La), G.gate_side(B, Lt, d, "unit", False, "full", seed=d + Lt + 1)
    name = f"pair<{1 if d <= 512 else 2}> d={d} {La}|{Lt} keep {Lk}"
    single = [run_fwd(s, Lk, name + " single") for s in (sa, st)]
    ba, bt = fwd_bufs(sa, Lk), fwd_bufs(st, Lk)
    call("hriemo_ln_pool_fwd_pair", *fwd_args(ba, sa, Lk), La, *fwd_args(bt, st, Lk), Lt, B, Lk, d, R.EPS, stream())
    for s, b, one, tag in ((sa, ba, single[0], " audio"), (st, bt, single[1], " text")):
        got = fwd_out(b, s, Lk, name + tag)
        judge_fwd(got, s, Lk, name + tag)
        for k in got:
            assert torch.equal(got[k], one[k]), (name + tag, k, "the pair launch and the single launch differ")


@pytest.mark.parametrize("d", G.PAIR_WIDTHS)
@pytest.mark.parametrize("La,Lt,Lf", [(33, 17, 16), (21, 5, 5), (70, 16, 3)])
def test_ln_pool_bwd_pair(L, d, La, Lt, Lf):
    B = 3
    ca = (B, La, Lf, d, "unit", True, "scattered", 1, True)
    ct = (B, Lt, Lf, d, "unit", False, "full", 0, True)
    (sa, oa, ma, ra), (st, ot, mt, rt) = G.make_bwd(ca), G.make_bwd(ct)
    ot = dict(ot, dH=oa["dH"], w=oa["w"])                              # one dH and one w feed both sides
    name = f"pair<{1 if d <= 512 else 2}> d={d} {La}|{Lt} Lf {Lf}"
    g = torch.Generator().manual_seed(d)
    init = {n: 1.0 + torch.rand(d, generator=g) for n in ("dgamma", "dbeta")}
    for reduce, acc in ((True, False), (True, True), (False, False)):
        tag = f"{name} reduce={reduce} acc={acc}"
        single = [run_bwd(L, sa, oa, 1, ma, ra, tag + " single a", reduce, acc, init), run_bwd(L, st, ot, 0, mt, rt, tag + " single t", reduce, acc, init)]
        ba, bt = bwd_bufs(L, sa, oa, ma, ra, reduce, acc, init), bwd_bufs(L, st, ot, mt, rt, reduce, acc, init)
        call("hriemo_ln_pool_bwd_pair", ba["dH"].ptr, Lf, ba["w"].ptr, *bwd_side_args(ba), La, ba["workspace"].ptr,
             *bwd_side_args(bt), Lt, bt["workspace"].ptr, int(acc), B, d, stream())
        intact({"dH (text copy, unused)": bt["dH"]}, tag)
        for s, o, b, is_a, m32, r32, one, side_tag in ((sa, oa, ba, 1, ma, ra, single[0], " audio"), (st, ot, bt, 0, mt, rt, single[1], " text")):
            got = bwd_out(L, b, s, tag + side_tag, reduce)
            judge_bwd(got, s, o, is_a, m32, r32, tag + side_tag, acc, init)
            for k in got:
                assert (got[k] is None and one[k] is None) or torch.equal(got[k], one[k]), (tag + side_tag, k, "pair and single launch differ")


def test_pair_launches_refuse_wide_rows(L):
    B, d, Ls = 3, 1032, 5
    assert L.hriemo_ln_pool_pair_supported(d) == 0
    c = (B, Ls, Ls, d, "unit", False, "none", 1, True)
    side, ops, m32, r32 = G.make_bwd(c)
    ba, bt = fwd_bufs(side, Ls), fwd_bufs(side, Ls)
    with pytest.raises(RuntimeError, match=r"hriemo_ln_pool_fwd_pair failed \(\d+\): .*d=1032"):
        call("hriemo_ln_pool_fwd_pair", *fwd_args(ba, side, Ls), Ls, *fwd_args(bt, side, Ls), Ls, B, Ls, d, R.EPS, stream())
    intact(ba, "fwd pair refused")
    assert all(untouched(b[k]) for b in (ba, bt) for k in ("Yn", "mean", "rstd", "part"))
    ba, bt = bwd_bufs(L, side, ops, m32, r32), bwd_bufs(L, side, ops, m32, r32)
    with pytest.raises(RuntimeError, match=r"hriemo_ln_pool_bwd_pair failed \(\d+\): .*d=1032"):
        call("hriemo_ln_pool_bwd_pair", ba["dH"].ptr, Ls, ba["w"].ptr, *bwd_side_args(ba), Ls, ba["workspace"].ptr,
             *bwd_side_args(bt), Ls, bt["workspace"].ptr, 0, B, d, stream())
    intact(ba, "bwd pair refused")
    assert all(untouched(b[k]) for b in (ba, bt) for k in ("dX", "workspace", "dgamma", "dbeta"))


# ------------------------------------------------------------------------------------------------ 5. legacy scalar gate, error returns
@pytest.mark.parametrize("d", [8, 512, 520, 4096])
@pytest.mark.parametrize("Ls", [1, 3, 4, 5])
def test_masked_mean_fwd(L, d, Ls):
    B = 3
    g = torch.Generator().manual_seed(1000 * Ls + d)
    X = torch.randn(B, Ls, d, generator=g).bfloat16()
    for kind in ("full", "none"):
        m = G.make_mask(kind, B, Ls, g)
        b = {"X": mat(X), "mask": mask8(m), "pooled": omat(B, d, torch.float32), "cnt": ovec(B)}
        call("hriemo_masked_mean_fwd", b["X"].ptr, ptr(b["mask"]), b["pooled"].ptr, b["cnt"].ptr, B, Ls, d, stream())
        name = f"masked_mean {B}x{Ls}x{d} {kind}"
        intact(b, name)
        show(name, G.check_masked_mean(b["pooled"].view.cpu(), b["cnt"].view.cpu(), X, m, name))
        if kind == "full":
            assert (b["pooled"].view.cpu()[B // 2] == 0).all()


@pytest.mark.parametrize("n", G.ROWSUM_N)
def test_rowsum_f32(L, n):
    B = 3
    x = torch.randn(B, n, generator=torch.Generator().manual_seed(n))
    b = {"x": vec(x), "out": ovec(B)}
    call("hriemo_rowsum_f32", b["x"].ptr, b["out"].ptr, B, n, stream())
    intact(b, f"rowsum n={n}")
    ref, mag = G.rowsum_ref(x)
    got = b["out"].view.cpu()
    show(f"rowsum n={n}", G.check_sum(got, ref, mag, n, f"rowsum n={n}"))
    if n == 1:
        assert torch.equal(got, x[:, 0])


@pytest.mark.parametrize("B,Ls,d", [(3, 5, 8), (3, 21, 520), (3, 37, 4096), G.SECOND_TRIP])
def test_scalar_gate_dx(L, B, Ls, d):
    second = (B, Ls, d) == G.SECOND_TRIP
    assert G.second_trip(B, Ls, d) == second
    for Lf in ((1000,) if second else G.keep_cases(Ls, 4)):
        c = G.scalar_dx_case(B, Ls, Lf, d, "full" if B > 2 else "scattered")
        dH_b = omat(1, d, torch.bfloat16) if Lf == 0 else mat(c["dH"])
        for is_a in (1, 0):
            b = {"dH": dH_b, "beta": vec(c["beta"]), "dpool": mat(c["dpool"]), "cnt": vec(c["cnt"]), "mask": mask8(c["mask"]),
                 "dX": omat(B * Ls, d, torch.bfloat16)}
            call("hriemo_scalar_gate_dx", b["dH"].ptr, Lf, b["beta"].ptr, is_a, b["dpool"].ptr, b["cnt"].ptr, ptr(b["mask"]), b["dX"].ptr, B, Ls, d, stream())
            name = f"scalar_gate_dx {B}x{Ls}x{d} Lf={Lf} is_a={is_a}"
            intact(b, name)
            show(name, G.check_scalar_dx(b["dX"].view.cpu().view(B, Ls, d), c, is_a, name))
            if second:
                break


def test_error_returns_launch_nothing(L):
    B, Ls, d = 3, 5, 520
    c = (B, Ls, Ls, d, "unit", False, "none", 1, True)
    side, ops, m32, r32 = G.make_bwd(c)
    fc = G.fuse_case(B, Ls, d)
    # (Lkeep | Lf, d as passed, workspace NULL, dgamma without dbeta)
    for Lk, db, ws_null, lone_dgamma in ((Ls + 1, d, False, False), (Ls, 516, False, False), (Ls, 4104, False, False), (Ls, d, True, False),
                                         (Ls, d, False, True)):
        fb, bb = fwd_bufs(side, Ls), bwd_bufs(L, side, ops, m32, r32)
        if not (ws_null or lone_dgamma):
            with pytest.raises(RuntimeError, match=r"hriemo_ln_pool_fwd failed \(\d+\): \S+"):
                call("hriemo_ln_pool_fwd", *fwd_args(fb, side, Ls), B, Ls, Lk, db, R.EPS, stream())
        args = list(bwd_side_args(bb))
        if lone_dgamma:
            args[9] = None
        with pytest.raises(RuntimeError, match=r"hriemo_ln_pool_bwd failed \(\d+\): \S+"):
            call("hriemo_ln_pool_bwd", bb["dH"].ptr, Lk, bb["w"].ptr, 1, *args, 0, B, Ls, db, None if ws_null else bb["workspace"].ptr, stream())
        intact(fb, "error return")
        intact(bb, "error return")
        assert all(untouched(fb[k]) for k in ("Yn", "mean", "rstd", "part")) and all(untouched(bb[k]) for k in ("dX", "workspace", "dgamma", "dbeta")), \
            (Lk, db, ws_null, lone_dgamma)
    for db in (516, 4104):
        outs = {"H": omat(B * Ls, d, torch.bfloat16), "part": omat(B, d, torch.float32), "pooled": omat(B, d, torch.float32), "cnt": ovec(B),
                "dX": omat(B * Ls, d, torch.bfloat16)}
        ins = {"w": mat(fc["w"]), "A": mat(fc["A"]), "T": mat(fc["T"]), "dH": mat(fc["dH"]), "beta": vec(torch.rand(B)), "cnt1": vec(torch.ones(B))}
        with pytest.raises(RuntimeError, match=r"hriemo_fuse_fwd failed \(\d+\): \S+"):
            call("hriemo_fuse_fwd", ins["w"].ptr, ins["A"].ptr, ins["T"].ptr, outs["H"].ptr, B, Ls, db, stream())
        with pytest.raises(RuntimeError, match=r"hriemo_fuse_bwd_dw failed \(\d+\): \S+"):
            call("hriemo_fuse_bwd_dw", ins["dH"].ptr, ins["A"].ptr, ins["T"].ptr, outs["part"].ptr, B, Ls, db, stream())
        with pytest.raises(RuntimeError, match=r"hriemo_masked_mean_fwd failed \(\d+\): \S+"):
            call("hriemo_masked_mean_fwd", ins["A"].ptr, None, outs["pooled"].ptr, outs["cnt"].ptr, B, Ls, db, stream())
        with pytest.raises(RuntimeError, match=r"hriemo_scalar_gate_dx failed \(\d+\): \S+"):
            call("hriemo_scalar_gate_dx", ins["dH"].ptr, Ls, ins["beta"].ptr, 1, ins["w"].ptr, ins["cnt1"].ptr, None, outs["dX"].ptr, B, Ls, db, stream())
        intact(outs, "error return")
        assert all(untouched(o) for o in outs.values()), db
    dX = omat(B * Ls, d, torch.bfloat16)
    ins = {"dH": mat(fc["dH"]), "beta": vec(torch.rand(B)), "dpool": mat(fc["w"]), "cnt": vec(torch.ones(B))}
    with pytest.raises(RuntimeError, match=r"hriemo_scalar_gate_dx failed \(\d+\): .*Lf"):
        call("hriemo_scalar_gate_dx", ins["dH"].ptr, Ls + 1, ins["beta"].ptr, 1, ins["dpool"].ptr, ins["cnt"].ptr, None, dX.ptr, B, Ls, d, stream())
    intact({"dX": dX}, "error return")
    assert untouched(dX)
