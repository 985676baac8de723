"""GPU suite, the pooled gate kernels of the fp32 precision mode (hri-emo_amd/csrc/fp32mode.hip: hriemo_pool32_ln_fwd,
hriemo_pool32_gate_input, hriemo_pool32_ln_bwd) through the C-ABI against pool32_reference.py: float64 references, limits F v mag
with every F counted.  Every input sits in a buffer between guards of 0xFF, every output is pre-filled with 0xFF (NaN) between
guards, and every guard byte is compared afterwards.  Every launch runs twice on fresh buffers and must agree bit for bit.

Shapes: B = 3, L in {1, 31, 32, 33, 70}, Lkeep in {1, 32, L - 1, L} where they fit, d in {4, 252, 256, 260, 1020, 1024}; masks none /
prefix / scattered / one fully masked sample / one sample with a single valid row; accumulate 0 and 1; g == NULL
(pool32_reference.CASES; test_pool32_bound_host.py checks the coverage and proves the limits on the CPU)."""
import pytest
import torch

import pool32_reference as P
from rowops_reference import GuardedVec

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


def vec(x):
    return None if x is None else GuardedVec.of(x.contiguous(), device=DEV)


def out(n):
    return GuardedVec(n, torch.float32, device=DEV)


def ptr(b):
    return None if b is None else b.ptr


def intact(bufs, name):
    torch.cuda.synchronize()
    for n, b in bufs.items():
        if b is not None:
            b.assert_intact(f"{name}: {n}")


def run_fwd(case, name):
    Bs, Ls, d = case["B"], case["L"], case["d"]
    nc = P.chunks(Ls)
    b = {"X": vec(case["X"]), "mask": vec(None if case["mask"] is None else case["mask"].to(torch.uint8)), "gamma": vec(case["gamma"]),
         "beta": vec(case["beta"]), "valid": out(Bs * nc * d), "keep": out(Bs * nc * d)}
    call("hriemo_pool32_ln_fwd", b["X"].ptr, ptr(b["mask"]), b["gamma"].ptr, b["beta"].ptr, b["valid"].ptr, b["keep"].ptr, Bs, Ls, case["Lkeep"], d,
         P.EPS, stream())
    intact(b, name)
    return {n: b[n].view.cpu().view(Bs, nc, d) for n in ("valid", "keep")}


def run_bwd(L, case, name):
    Bs, Ls, d = case["B"], case["L"], case["d"]
    wsn = L.hriemo_pool32_ln_bwd_workspace_bytes(Bs, Ls, d) // 4
    assert wsn > 0
    acc = case["accumulate"]
    b = {"g": vec(case["g"]), "dpool": vec(case["dpool"]), "mask": vec(None if case["mask"] is None else case["mask"].to(torch.uint8)),
         "X": vec(case["X"]), "gamma": vec(case["gamma"]), "dX": out(Bs * Ls * d),
         "dgamma": vec(case["init"]["dgamma"]) if acc else out(d), "dbeta": vec(case["init"]["dbeta"]) if acc else out(d),
         "ws": out(wsn)}                                 # the workspace at exactly its documented size
    call("hriemo_pool32_ln_bwd", ptr(b["g"]), case["Lkeep"], b["dpool"].ptr, ptr(b["mask"]), b["X"].ptr, b["gamma"].ptr, b["dX"].ptr,
         b["dgamma"].ptr, b["dbeta"].ptr, acc, Bs, Ls, d, P.EPS, b["ws"].ptr, stream())
    intact(b, name)
    return {"dX": b["dX"].view.cpu().view(Bs, Ls, d), "dgamma": b["dgamma"].view.cpu(), "dbeta": b["dbeta"].view.cpu()}


def same(a, b, name):
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), f"{name}: {n} differs between two launches on the same inputs"


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_pool32_ln_fwd(L, c):
    case, name = P.make_case(c), P.case_id(c)
    got = run_fwd(case, name)
    same(got, run_fwd(case, name), name)
    print(name, "partials", round(P.check_fwd(got, case, name), 3))


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_pool32_gate_input(L, c):
    """audio side: the case; text side: the case's shorter sibling (Lt = Lkeep rows, its own mask family) -- pools against float64
    from the partials the forward kernel wrote, gate_in bit for bit against hriemo_gate_input_f32 on the pools this kernel wrote"""
    La, k, d, kind = c[:4]
    name = P.case_id(c)
    ca = P.make_case(c)
    ct = P.make_case((k, k, d, P.MASKS[(P.MASKS.index(kind) + 2) % 5], 0, True), seed=77 + d + k)
    pa, pt = run_fwd(ca, name)["valid"], run_fwd(ct, name + " text")["valid"]

    def launch():
        b = {"pa": vec(pa), "ma": vec(None if ca["mask"] is None else ca["mask"].to(torch.uint8)), "pt": vec(pt),
             "mt": vec(None if ct["mask"] is None else ct["mask"].to(torch.uint8)), "a": out(P.B * d), "t": out(P.B * d), "gin": out(P.B * 4 * d)}
        call("hriemo_pool32_gate_input", b["pa"].ptr, ptr(b["ma"]), La, b["pt"].ptr, ptr(b["mt"]), k, b["a"].ptr, b["t"].ptr, b["gin"].ptr, P.B, d,
             stream())
        intact(b, name)
        return {"a": b["a"].view.cpu().view(P.B, d), "t": b["t"].view.cpu().view(P.B, d), "gin": b["gin"].view.cpu().view(P.B, 4 * d)}, b

    got, b = launch()
    same(got, launch()[0], name)
    ra = P.check_pools(got["a"], pa, ca, name + " a_pool")
    rt = P.check_pools(got["t"], pt, ct, name + " t_pool")
    old = out(P.B * 4 * d)
    call("hriemo_gate_input_f32", b["a"].ptr, b["t"].ptr, old.ptr, P.B, d, stream())
    torch.cuda.synchronize()
    old.assert_intact(name + " gate_input_f32")
    assert torch.equal(got["gin"].view(torch.int32), old.view.cpu().view(P.B, 4 * d).view(torch.int32)), f"{name}: gate_in is not hriemo_gate_input_f32's bit for bit"
    assert torch.equal(got["gin"].view(torch.int32), P.gate_in32(got["a"], got["t"]).view(torch.int32)), f"{name}: gate_in is not [a, t, |a - t|, a * t] of the pools"
    print(name, "pools", round(ra, 3), round(rt, 3))


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_pool32_ln_bwd(L, c):
    case, name = P.make_case(c), P.case_id(c)
    got = run_bwd(L, case, name)
    same(got, run_bwd(L, case, name), name)
    print(name, {k: round(v, 3) for k, v in P.check_bwd(got, case, name).items()})


def test_pool32_ln_bwd_without_affine_gradients(L):
    """dgamma == dbeta == NULL: dX alone, the workspace not needed"""
    case = P.make_case((33, 32, 260, "scattered", 0, True))
    full = run_bwd(L, case, "with affine")
    Bs, Ls, d = case["B"], case["L"], case["d"]
    b = {"g": vec(case["g"]), "dpool": vec(case["dpool"]), "mask": vec(case["mask"].to(torch.uint8)), "X": vec(case["X"]), "gamma": vec(case["gamma"]),
         "dX": out(Bs * Ls * d)}
    call("hriemo_pool32_ln_bwd", b["g"].ptr, case["Lkeep"], b["dpool"].ptr, b["mask"].ptr, b["X"].ptr, b["gamma"].ptr, b["dX"].ptr, None, None, 0,
         Bs, Ls, d, P.EPS, None, stream())
    intact(b, "no affine")
    assert torch.equal(b["dX"].view.cpu().view(Bs, Ls, d), full["dX"])


def test_refusals(L):
    """d = 1028, d = 6, Lkeep = 0, Lkeep > L, one of dgamma / dbeta NULL: an error with a message, nothing launched"""
    Bs, Ls = 3, 4
    x, o = torch.zeros(Bs * Ls * 1028, device=DEV), torch.zeros(Bs * Ls * 1028, device=DEV)
    v, w = torch.zeros(Bs * 1028, device=DEV), torch.zeros(Bs * 1028, device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    for d, k, word in ((1028, 1, "1024"), (6, 1, "multiple of 4"), (8, 0, "Lkeep"), (8, Ls + 1, "Lkeep")):
        with pytest.raises(RuntimeError, match=word):
            call("hriemo_pool32_ln_fwd", p(x), None, p(v), p(v), p(o), p(ws), Bs, Ls, k, d, P.EPS, stream())
        with pytest.raises(RuntimeError, match=word):
            call("hriemo_pool32_ln_bwd", p(v), k, p(w), None, p(x), p(v), p(o), p(ws), p(ws[4096:]), 0, Bs, Ls, d, P.EPS, p(ws[8192:]), stream())
    for dg, db in ((None, p(ws)), (p(ws), None)):
        with pytest.raises(RuntimeError, match="both NULL"):
            call("hriemo_pool32_ln_bwd", p(v), 1, p(w), None, p(x), p(v), p(o), dg, db, 0, Bs, Ls, 8, P.EPS, p(ws[8192:]), stream())
    assert L.hriemo_pool32_ln_bwd_workspace_bytes(0, 4, 8) == 0
    torch.cuda.synchronize()
    assert float(o.abs().sum()) == 0.0 and float(ws.abs().sum()) == 0.0
