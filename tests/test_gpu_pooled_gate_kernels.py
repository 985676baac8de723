"""GPU suite, the pooled gate kernels (hri-emo_amd/csrc/rowops.hip) through the C-ABI against pooled_gate_reference.py and
gate_reference.py.  Every input sits in a poisoned buffer between guards, every output is pre-filled with 0xFF between guards.

  1. hriemo_ln_pool2_fwd: mean, rstd and the masked partials torch.equal to hriemo_ln_pool_fwd's on the same inputs; the keep
     partials against float64 under gate_reference.pool_part_factor; single and _pair (the pair bit for bit against the singles)
  2. hriemo_pooled_fuse_fwd / _bwd against float64
  3. hriemo_ln_pool_vec_bwd against float64 under the envelope of the ln_pool_bwd test (check_pool_bwd), and against
     hriemo_ln_pool_bwd fed dH = bf16(g / w) within that rounding; single and _pair
  4. hriemo_ingest_padded: PAD rows exact zeros, valid rows bit-equal to hriemo_ingest_rows + hriemo_unpack_rows, NaN behind cu[B]
  5. the error returns

Shapes: B = 3, d in {128, 136, 768, 1024}, L in {1, 31, 32, 33, 70}, Lkeep in {1, 32, 33, L - 1, L} where <= L; masks none / prefix
with lengths {1, mid, L} / scattered; with and without the fp32 twin (test_classifier_packed_host.py checks the coverage); the
single launches also at d = 1032 and 2048 (PG.WIDE_CASES: the instances behind the pair's widths)."""
import pytest
import torch

import gate_reference as G
import pooled_gate_reference as PG
import rowops_reference as R
import test_gpu_gate_variants as TV
from test_gpu_gate_variants import call, intact, mask8, mat, omat, ovec, ptr, stream, vec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ 1. forward
def fwd2_bufs(side):
    Bs, Ls, d, ln = side["B"], side["L"], side["d"], side["ln"]
    nc = G.chunks(Ls, G.POOL_ROWS)
    return {"X": mat(ln["X"]), "X32": mat(ln["X32"]), "mask": mask8(side["mask"]), "gamma": vec(ln["gamma"]), "beta": vec(ln["beta"]),
            "mean": ovec(Bs * Ls), "rstd": ovec(Bs * Ls), "part": omat(Bs * nc, d, torch.float32), "keep": omat(Bs * nc, d, torch.float32)}


def fwd2_args(b):
    return (ptr(b["X"]), ptr(b["X32"]), ptr(b["mask"]), b["gamma"].ptr, b["beta"].ptr, b["mean"].ptr, b["rstd"].ptr, b["part"].ptr, b["keep"].ptr)


def fwd2_out(b, side, name):
    intact(b, name)
    Bs, d = side["B"], side["d"]
    return {"mean": b["mean"].view.cpu(), "rstd": b["rstd"].view.cpu(), "part": b["part"].view.cpu().view(Bs, -1, d),
            "keep": b["keep"].view.cpu().view(Bs, -1, d)}


def judge_fwd2(got, side, k, name):
    old = TV.run_fwd(side, 0, name + " (ln_pool_fwd)")            # Lkeep = 0: no Yn row, the statistics and the masked partials
    for n in ("mean", "rstd", "part"):
        assert torch.equal(got[n], old[n]), f"{name}: {n} differs from hriemo_ln_pool_fwd's"
    r = PG.check_keep(got["keep"], side, k, name)
    print(name, "keep partials", round(r, 3))


@pytest.mark.parametrize("c", PG.CASES + PG.WIDE_CASES, ids=PG.case_id)
def test_ln_pool2_fwd(L, c):
    Ls, k, d, twin, mask = c
    side = PG.make_side(Ls, d, twin, mask)
    b = fwd2_bufs(side)
    call("hriemo_ln_pool2_fwd", *fwd2_args(b), PG.B, Ls, k, d, R.EPS, stream())
    judge_fwd2(fwd2_out(b, side, PG.case_id(c)), side, k, PG.case_id(c))


@pytest.mark.parametrize("c", PG.PAIR_CASES, ids=PG.pair_id)
def test_ln_pool2_fwd_pair(L, c):
    La, Lt, k, d, twin, ma, mt = c
    sa, st = PG.make_side(La, d, twin, ma), PG.make_side(Lt, d, twin, mt, seed=4242 + d + Lt)
    ba, bt = fwd2_bufs(sa), fwd2_bufs(st)
    call("hriemo_ln_pool2_fwd_pair", *fwd2_args(ba), La, *fwd2_args(bt), Lt, PG.B, k, d, R.EPS, stream())
    name = PG.pair_id(c)
    for side, b, tag in ((sa, ba, " audio"), (st, bt, " text")):
        got = fwd2_out(b, side, name + tag)
        judge_fwd2(got, side, k, name + tag)
        one = fwd2_bufs(side)
        call("hriemo_ln_pool2_fwd", *fwd2_args(one), PG.B, side["L"], k, d, R.EPS, stream())
        single = fwd2_out(one, side, name + tag + " single")
        for n in got:
            assert torch.equal(got[n], single[n]), f"{name}{tag}: {n} of the pair differs from the single launch"


# ------------------------------------------------------------------------------------------------ 2. the [B, d] kernels
@pytest.mark.parametrize("d", PG.WIDTHS)
@pytest.mark.parametrize("La,Lt,k", [(70, 33, 33), (33, 32, 1), (70, 70, 69), (1, 1, 1), (70, 70, 32)])
def test_pooled_fuse_fwd_and_bwd(L, d, La, Lt, k):
    c = PG.fuse_case(La, Lt, k, d)
    name = f"pooled_fuse {La}|{Lt} keep{k} d={d}"
    b = {"ka": mat(c["ka"]), "kt": mat(c["kt"]), "w": mat(c["w"]), "abar": omat(PG.B, d, torch.float32), "tbar": omat(PG.B, d, torch.float32),
         "pooled": omat(PG.B, d, torch.float32)}
    call("hriemo_pooled_fuse_fwd", b["ka"].ptr, La, b["kt"].ptr, Lt, b["w"].ptr, k, b["abar"].ptr, b["tbar"].ptr, b["pooled"].ptr, PG.B, d, stream())
    intact(b, name)
    got = {n: b[n].view.cpu() for n in ("abar", "tbar", "pooled")}
    TV.show(name, PG.check_fuse_fwd(got, c, name))
    for has_g in (True, False):
        bb = {"g": mat(c["dpooled"]) if has_g else None, "abar": mat(got["abar"]), "tbar": mat(got["tbar"]), "w": mat(c["w"]),
              "dw": omat(PG.B, d, torch.float32), "ga": omat(PG.B, d, torch.float32), "gt": omat(PG.B, d, torch.float32)}
        call("hriemo_pooled_fuse_bwd", ptr(bb["g"]), bb["abar"].ptr, bb["tbar"].ptr, bb["w"].ptr, k, bb["dw"].ptr, bb["ga"].ptr, bb["gt"].ptr, PG.B, d, stream())
        intact(bb, name + " bwd")
        out = {n: bb[n].view.cpu() for n in ("dw", "ga", "gt")}
        if has_g:
            TV.show(name + " bwd", PG.check_fuse_bwd(out, c, got["abar"], got["tbar"], name + " bwd"))
        else:
            assert all((v == 0).all() for v in out.values()), "no upstream gradient: exact zeros"


# ------------------------------------------------------------------------------------------------ 3. backward
def vbwd_bufs(L, side, v, m32, r32, reduce=True):
    Bs, Ls, d, ln = side["B"], side["L"], side["d"], side["ln"]
    wsn = L.hriemo_ln_pool_bwd_workspace_bytes(Bs, Ls, d) // 4
    b = {"g": mat(v["g"]), "dpool": mat(v["dpool"]), "mask": mask8(side["mask"]), "X": mat(ln["X"]), "X32": mat(ln["X32"]),
         "gamma": vec(ln["gamma"]), "mean": vec(m32), "rstd": vec(r32), "dX": omat(Bs * Ls, d, torch.bfloat16),
         "workspace": R.GuardedVec(wsn, torch.float32, guard=1024, device=TV.DEV)}
    for n in ("dgamma", "dbeta"):
        b[n] = ovec(d) if reduce else None
    return b


def vbwd_side_args(b):
    return (ptr(b["g"]), b["dpool"].ptr, ptr(b["mask"]), ptr(b["X"]), ptr(b["X32"]), b["gamma"].ptr, b["mean"].ptr, b["rstd"].ptr, b["dX"].ptr,
            ptr(b["dgamma"]), ptr(b["dbeta"]))


def make_vbwd(c, has_g=True):
    Ls, k, d, twin, mask = c
    side = PG.make_side(Ls, d, twin, mask)
    m32, r32 = R.stats32(R.ln_fwd_ref(side["ln"]))
    return side, PG.vec_operands(side, k, has_g), m32, r32


def run_vbwd(L, side, v, m32, r32, name, reduce=True):
    b = vbwd_bufs(L, side, v, m32, r32, reduce)
    a = vbwd_side_args(b)
    call("hriemo_ln_pool_vec_bwd", a[0], v["Lkeep"], *a[1:], 0, side["B"], side["L"], side["d"], b["workspace"].ptr, stream())
    return TV.bwd_out(L, b, side, name, reduce)


@pytest.mark.parametrize("c", PG.CASES + PG.WIDE_CASES, ids=PG.case_id)
def test_ln_pool_vec_bwd(L, c):
    side, v, m32, r32 = make_vbwd(c)
    name = PG.case_id(c)
    got = run_vbwd(L, side, v, m32, r32, name, reduce=c[1] % 2 == 1)
    TV.judge_bwd(got, side, PG.vec_ops(side, v), 1, m32, r32, name)
    # rows at or past Lkeep of a masked-out position get an exact zero gradient
    dead = (~side["valid"]) & (torch.arange(c[0]) >= c[1])[None, :]
    assert (got["dX"][dead] == 0).all()
    # cross-check: hriemo_ln_pool_bwd with dH = bf16(g / w) on rows l < Lkeep
    w = torch.sigmoid(torch.randn(PG.B, c[2], generator=side["gen"]))
    old = TV.run_bwd(L, side, PG.cross_ops(side, v, w), 1, m32, r32, name + " (ln_pool_bwd)")
    err, lim = (got["dX"].double() - old["dX"].double()).abs(), PG.cross_limit(side, v, m32, r32)
    print(name, "cross-check: largest error / limit", float((err / lim.clamp(min=1e-300)).max()))
    assert (err <= lim).all(), f"{name}: {int((err > lim).sum())} elements differ from hriemo_ln_pool_bwd by more than the rounding of dH"


def test_ln_pool_vec_bwd_without_a_row_gradient(L):
    side, v, m32, r32 = make_vbwd((33, 32, 136, True, "scattered"), has_g=False)
    got = run_vbwd(L, side, v, m32, r32, "no g")
    TV.judge_bwd(got, side, PG.vec_ops(side, v), 1, m32, r32, "no g")


@pytest.mark.parametrize("c", PG.PAIR_CASES, ids=PG.pair_id)
@pytest.mark.parametrize("reduce", [True, False])
def test_ln_pool_vec_bwd_pair(L, c, reduce):
    La, Lt, k, d, twin, ma, mt = c
    name = PG.pair_id(c)
    sides = [make_vbwd((La, k, d, twin, ma)), make_vbwd((Lt, k, d, twin, mt))]
    bufs = [vbwd_bufs(L, s, v, m, r, reduce) for s, v, m, r in sides]
    call("hriemo_ln_pool_vec_bwd_pair", k, *vbwd_side_args(bufs[0]), La, bufs[0]["workspace"].ptr, *vbwd_side_args(bufs[1]), Lt, bufs[1]["workspace"].ptr,
         0, PG.B, d, stream())
    for (side, v, m32, r32), b, tag in zip(sides, bufs, (" audio", " text")):
        got = TV.bwd_out(L, b, side, name + tag, reduce)
        TV.judge_bwd(got, side, PG.vec_ops(side, v), 1, m32, r32, name + tag)
        single = run_vbwd(L, side, v, m32, r32, name + tag + " single", reduce)
        for n in ("dX", "part") + (("dgamma", "dbeta") if reduce else ()):
            assert torch.equal(got[n], single[n]), f"{name}{tag}: {n} of the pair differs from the single launch"


# ------------------------------------------------------------------------------------------------ 4. ingest
@pytest.mark.parametrize("dtype,xt", [(torch.float32, 0), (torch.bfloat16, 1), (torch.float16, 2)])
@pytest.mark.parametrize("Ls,d,lens", [(33, 128, [33, 1, 20]), (1, 136, [1, 1, 1]), (70, 768, [32, 70, 33]), (5, 1024, [1, 5, 4])])
@pytest.mark.parametrize("twin", [True, False])
def test_ingest_padded(L, dtype, xt, Ls, d, lens, twin):
    rows, cu, pad = PG.ingest_case(Ls, d, dtype, lens)
    Bs, n = len(lens), sum(lens)
    name = f"ingest_padded {dtype} {Bs}x{Ls}x{d}"
    b = {"X": mat(rows), "cu": vec(cu), "Y16": omat(Bs * Ls, d, torch.bfloat16), "Y32": omat(Bs * Ls, d, torch.float32) if twin else None}
    call("hriemo_ingest_padded", b["X"].ptr, xt, d, b["cu"].ptr, n + 3, Bs, Ls, d, b["Y16"].ptr, ptr(b["Y32"]), stream())
    intact(b, name)
    y16 = b["Y16"].view.cpu().view(Bs, Ls, d)
    padmask = torch.arange(Ls)[None, :] >= torch.tensor(lens)[:, None]
    assert (y16.view(torch.int16)[padmask] == 0).all(), "PAD rows of the bf16 output are not exact zeros"
    # the two launches it replaces, on the same (poisoned) source: packed pair, then scattered
    p16, p32 = omat(n, d, torch.bfloat16), omat(n, d, torch.float32)
    call("hriemo_ingest_rows", b["X"].ptr, xt, d, b["cu"].ptr, 1, Bs, Ls, d, n, p16.ptr, p32.ptr, None, None, 0, None, stream())
    u16, u32 = omat(Bs * Ls, d, torch.bfloat16), omat(Bs * Ls, d, torch.float32)
    call("hriemo_unpack_rows", p16.ptr, p32.ptr, b["cu"].ptr, Bs, Ls, d, u16.ptr, u32.ptr, stream())
    intact({"p16": p16, "p32": p32, "u16": u16, "u32": u32}, name + " reference launches")
    assert torch.equal(y16.view(torch.int16), u16.view.cpu().view(Bs, Ls, d).view(torch.int16)), "bf16 rows differ from ingest_rows + unpack_rows"
    assert torch.equal(y16.float(), pad.bfloat16().float()), "bf16 rows are not the rounded source values"
    if twin:
        y32 = b["Y32"].view.cpu().view(Bs, Ls, d)
        assert (y32.view(torch.int32)[padmask] == 0).all(), "PAD rows of the fp32 twin are not exact zeros"
        assert torch.equal(y32.view(torch.int32), u32.view.cpu().view(Bs, Ls, d).view(torch.int32)), "fp32 twin differs from ingest_rows + unpack_rows"
        assert torch.equal(y32, pad)


# ------------------------------------------------------------------------------------------------ 5. error returns
def test_error_returns(L):
    def refused(name, *args):
        from hri_emo_amd import _lib
        with pytest.raises(RuntimeError, match=name):
            _lib.call(name, *args)

    side = PG.make_side(5, 128, False, "none")
    b = fwd2_bufs(side)
    a = fwd2_args(b)
    refused("hriemo_ln_pool2_fwd", *a, PG.B, 5, 0, 128, R.EPS, stream())                 # Lkeep < 1
    refused("hriemo_ln_pool2_fwd", *a, PG.B, 5, 6, 128, R.EPS, stream())                 # Lkeep > L
    refused("hriemo_ln_pool2_fwd", *a, PG.B, 5, 5, 124, R.EPS, stream())                 # d % 8
    refused("hriemo_ln_pool2_fwd", *a, PG.B, 5, 5, 2056, R.EPS, stream())                # d > 2048
    refused("hriemo_ln_pool2_fwd", *a[:7], a[7], a[7], PG.B, 5, 5, 128, R.EPS, stream())  # one buffer for both partial sets
    refused("hriemo_ln_pool2_fwd_pair", *a, 5, *a, 5, PG.B, 5, 1032, R.EPS, stream())    # pairs: d <= 1024
    refused("hriemo_pooled_fuse_fwd", a[7], 5, a[8], 5, a[3], 6, a[7], a[7], a[7], PG.B, 128, stream())
    refused("hriemo_ingest_padded", a[0], 3, 128, a[3], 15, PG.B, 5, 128, a[7], None, stream())      # unknown dtype
    refused("hriemo_ingest_padded", a[0], 1, 128, a[3], 15, PG.B, 5, 128, None, None, stream())      # no output
    intact(b, "refused calls")
    for n in ("mean", "rstd", "part", "keep"):
        assert TV.untouched(b[n]), f"a refused call wrote {n}"
