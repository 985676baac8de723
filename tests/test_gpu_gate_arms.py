"""GPU suite, the gate Functions (hri_emo_amd._ops.BetaGateFn, PooledGateFn) on every arm of their "both modalities" step:

  pair          one launch for both modalities (d <= 1024, what hriemo_ln_pool_pair_supported accepts)
  two streams   the text side on the side stream beside the audio side (BetaGateFn only)
  serial        two single launches on one stream

The kernel-level suites (test_gpu_gate_variants.py, test_gpu_pooled_gate_kernels.py) hold every launch against float64 and the pair
launches bit for bit against the single ones through the C-ABI; here the Functions run forward and backward at d = 136 (the pair arm
at a width that is no multiple of 64 lanes x 8) and d = 1032 (the smallest width the pair launches refuse: the library picks the arm),
and whatever arm runs must return the same bits.  Arm (a) is also held against the float64 references of gate_reference.py /
pooled_gate_reference.py with their limits, stage by stage from the VALUES each stage read (the tensors the Function saved for its
backward), so that the code is not compared with itself alone:

  LayerNorm outputs and row statistics   the y / mean / rstd rules of check_pool_fwd
  H                                      check_fuse_fwd from (w, An, Tn)
  beta                                   check_sigmoid_beta from the pre-activation (the second Linear run again on the saved hidden layer)
  dX, dgamma, dbeta                      check_pool_bwd from (dH, w, dpool) with dpool = the masked means' gradients (_gate_weights_bwd run
                                         again on the saved tensors)
  MLP gradients (PooledGateFn, and the   the fp32 rule of gemm_reference.check, |got - ref| <= (K + 2) v mag with K = B rows of reduction,
  accumulating case)                     from the bf16 dpre / dhid the backward forms

Accumulating case: the parameters opted into fused weight-gradient accumulation, .grad pre-filled -- the deferred launch-boundary
reduce and the accumulate = 1 reduce; LayerNorm gradients within check_pool_bwd's accumulate limit (one more rounding for the non-zero
destination) of float64(pre-fill + sum); MLP gradients against pre-fill + the non-accumulating run's: both are within (B + 2) v mag of
the exact sum, the accumulating one adds one rounding into the destination, the host's fp32 addition another:
(2 (B + 2) + 2) v (mag + |pre-fill|)."""
import contextlib

import pytest
import torch

import gate_reference as G
import pooled_gate_reference as PG
import rowops_reference as R
import test_gpu_gate_variants as TV

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, LA, LT, HID = 3, 37, 21, 32
WIDTHS = (136, 1032)
LENS_A, LENS_T = (20, 37, 5), (1, 21, 9)          # prefix masks: sample 0 keeps ONE text row, sample 1 is fully valid on both sides
NAMES = ("ga", "ba", "gt", "bt", "w1", "b1", "w2", "b2")
V = G.V


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hri_emo_amd import _ops
    return _ops


@contextlib.contextmanager
def flags(ops, **kw):
    old = {k: getattr(ops, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


_cases = {}


def case(d):
    """{sides (audio, text), params (CPU, NAMES order), dH, dbeta, dpooled}: built once per width, never written"""
    if d not in _cases:
        sides = []
        for Ls, lens, seed in ((LA, LENS_A, 1), (LT, LENS_T, 2)):
            s = G.gate_side(B, Ls, d, "unit", True, "none", seed=1000 * d + seed)
            s["mask"] = torch.arange(Ls)[None, :] >= torch.tensor(lens)[:, None]
            s["valid"] = ~s["mask"]
            sides.append(s)
        g = torch.Generator().manual_seed(77 * d)
        mlp = (torch.randn(HID, 4 * d, generator=g) / (4 * d) ** 0.5, 0.1 * torch.randn(HID, generator=g),
               torch.randn(d, HID, generator=g) / HID ** 0.5, 0.1 * torch.randn(d, generator=g))
        params = (sides[0]["ln"]["gamma"], sides[0]["ln"]["beta"], sides[1]["ln"]["gamma"], sides[1]["ln"]["beta"]) + mlp
        _cases[d] = {"sides": sides, "params": params, "dH": torch.randn(B, LT, d, generator=g).bfloat16(),
                     "dbeta": torch.randn(B, 1, generator=g), "dpooled": torch.randn(B, d, generator=g),
                     "prefill": tuple(0.25 + 0.5 * torch.rand(p.shape, generator=g) for p in params)}
    return _cases[d]


def run(ops, d, pooled=False, fused=False):
    """one forward + backward of the Function with upstream gradients for both outputs -> {out, beta, dxa, dxt, NAMES..., saved, params}"""
    c = case(d)
    sa_, st_ = c["sides"]
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in c["params"]]
    if fused:
        ops.enable_fused_wgrad(params)
        for p, g in zip(params, c["prefill"]):
            p.grad = g.clone().to(DEV)
    xa32, xt32 = sa_["ln"]["X32"].view(B, LA, d).to(DEV), st_["ln"]["X32"].view(B, LT, d).to(DEV)
    xa, xt = xa32.bfloat16().requires_grad_(), xt32.bfloat16().requires_grad_()
    sa, st = ops.Seq.padded(B, LA, sa_["mask"].to(DEV)), ops.Seq.padded(B, LT, st_["mask"].to(DEV))
    if pooled:
        out, beta = ops.PooledGateFn.apply(xa, xa32, xt, xt32, *params, ops.Shadows(), sa, st)
        dout = c["dpooled"].to(DEV)
    else:
        out, beta = ops.BetaGateFn.apply(xa, xa32, xt, xt32, *params, ops.Shadows(), sa, st, ops.Seq.padded(B, LT))
        dout = c["dH"].to(DEV)
    saved = out.grad_fn.saved_tensors
    torch.autograd.backward([out, beta], [dout, c["dbeta"].to(DEV)])
    torch.cuda.synchronize()
    r = {"out": out.detach(), "beta": beta.detach(), "dxa": xa.grad, "dxt": xt.grad, "saved": saved, "params": params}
    r.update({n: p.grad for n, p in zip(NAMES, params)})
    return r


def assert_same(a, b, what):
    for k in ("out", "beta", "dxa", "dxt") + NAMES:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs between the arms"


def judge_ln(y, mean, rstd, side, name):
    """the LayerNorm outputs of the LT fused rows and the statistics of every row: the rules of gate_reference.check_pool_fwd"""
    ref = G.pool_fwd_ref(side, LT)
    d = side["d"]
    R.check_elem(mean.cpu(), ref["mean"], ref["sabs"], d + 2, True, name + " mean")
    R.check_elem(rstd.cpu(), ref["rstd"], ref["mag_rstd"], G.LN_FACTOR["rstd"], True, name + " rstd")
    if y is not None:
        R.check_elem(y.cpu(), ref["yn"], ref["mag_yn"], G.LN_FACTOR["y"], False, name + " Yn")


def judge_beta(ops, beta, w, hid, w2_16, b2, name):
    pre = ops.linear_fwd(hid, w2_16, b2, out_f32=True).cpu()
    assert float(pre.abs().max()) <= G.PRE_MAX, "the case left the range SIGMOID_FACTOR was measured on"
    TV.show(name, G.check_sigmoid_beta(w.cpu(), beta.cpu(), pre, name))


def mlp_backward(ops, part, Lp, dbeta, w, hid, gin, a_pool, t_pool, cnt, w1_16, w2_16, params, d):
    """the backward of _gate_weights run again on the saved tensors -> (da, dt) on the GPU and {name: (ref, mag)} in float64 of the
    four MLP gradients from the bf16 dpre / dhid it forms"""
    from hri_emo_amd import _lib
    sink = ops.GradSink(params[4:])
    da, dt = ops._gate_weights_bwd(part, Lp, dbeta, w, hid, gin, a_pool, t_pool, cnt, w1_16, w2_16, sink, tuple(params[4:]), B, d)[:2]
    dpre = torch.empty((B, d), dtype=torch.bfloat16, device=DEV)
    _lib.call("hriemo_gate_dpre", part.data_ptr(), Lp, dbeta.data_ptr(), w.data_ptr(), dpre.data_ptr(), B, d, TV.stream())
    dhid = ops.linear_dx(dpre, w2_16, epi=2, aux=hid)
    p64, h64, g64, i64 = dpre.double().cpu(), dhid.double().cpu(), hid.double().cpu(), gin.double().cpu()
    ref = {"w2": (p64.T @ g64, p64.abs().T @ g64.abs()), "b2": (p64.sum(0), p64.abs().sum(0)),
           "w1": (h64.T @ i64, h64.abs().T @ i64.abs()), "b1": (h64.sum(0), h64.abs().sum(0))}
    return da, dt, ref


def judge_mlp(got, ref, name):
    for n, (r64, mag) in ref.items():
        R.check_elem(got[n].cpu(), r64, mag, B + 2, True, f"{name} d{n}")


def judge_accumulated(acc, plain, prefill, ref, name):
    for n, (r64, mag) in ref.items():
        p = prefill[NAMES.index(n)]
        lim = (2 * (B + 2) + 2) * V * (mag + p.double().abs())
        err = (acc[n].cpu().double() - (p + plain[n].cpu()).double()).abs()
        assert bool((err <= lim).all()), f"{name} d{n}: {float((err / lim.clamp(min=1e-300)).max()):.2f} x the limit"


def judge_beta_gate(ops, r, d, name, plain=None):
    """arm (a) of BetaGateFn against float64; plain: the non-accumulating run when r accumulated into pre-filled .grad"""
    from hri_emo_amd import _lib
    c = case(d)
    (xa, xt, An, Tn, mean_a, rstd_a, mean_t, rstd_t, gin, a_pool, t_pool, cnt, hid, w, w1_16, w2_16) = r["saved"][:16]
    judge_ln(An, mean_a, rstd_a, c["sides"][0], name + " audio")
    judge_ln(Tn, mean_t, rstd_t, c["sides"][1], name + " text")
    TV.show(name, G.check_fuse_fwd(r["out"].cpu(), {"w": w.cpu(), "A": An.cpu(), "T": Tn.cpu(), "d": d}, name))
    judge_beta(ops, r["beta"], w, hid, w2_16, r["params"][7], name)
    dH, dbeta = c["dH"].to(DEV), c["dbeta"].to(DEV)
    part = torch.empty((B, _lib.lib().hriemo_pool_chunks(LT), d), dtype=torch.float32, device=DEV)
    ops.fuse_bwd_dw(dH, An, Tn, part, ops.Seq.padded(B, LT), d)
    acc = plain is not None
    # (parameters that are NOT opted in: this second backward must not add to the .grad under test)
    da, dt, ref = mlp_backward(ops, part, LT, dbeta, w, hid, gin, a_pool, t_pool, cnt, w1_16, w2_16, (plain if acc else r)["params"], d)
    for side, is_a, dpool, m32, r32, dx, gn, bn in ((c["sides"][0], 1, da, mean_a, rstd_a, r["dxa"], "ga", "ba"),
                                                    (c["sides"][1], 0, dt, mean_t, rstd_t, r["dxt"], "gt", "bt")):
        o = {"dH": c["dH"], "w": w.cpu(), "dpool": dpool.cpu(), "Lf": LT}
        got = {"dX": dx.cpu(), "dgamma": r[gn].cpu(), "dbeta": r[bn].cpu()}
        init = {"dgamma": c["prefill"][NAMES.index(gn)], "dbeta": c["prefill"][NAMES.index(bn)]} if acc else None
        TV.judge_bwd(got, side, o, is_a, m32.cpu(), r32.cpu(), f"{name} {'audio' if is_a else 'text'}", acc, init)
    if acc:
        judge_accumulated(r, plain, c["prefill"], ref, name)
    else:
        judge_mlp(r, ref, name)


# ------------------------------------------------------------------------------------------------ 1. BetaGateFn, padded
@pytest.mark.parametrize("d", WIDTHS)
def test_beta_gate_arms_return_the_same_bits(ops, d):
    from hri_emo_amd import _lib
    assert _lib.lib().hriemo_ln_pool_pair_supported(d) == (1 if d == 136 else 0)
    a = run(ops, d)
    if ops.side_stream(torch.device(DEV, torch.cuda.current_device())) is not None:
        with flags(ops, GATE_PAIR=False):
            assert_same(a, run(ops, d), f"d={d}, defaults | text on the side stream")
    with flags(ops, GATE_PAIR=False, GATE_TWO_STREAMS=False):
        assert_same(a, run(ops, d), f"d={d}, defaults | serial")
    judge_beta_gate(ops, a, d, f"BetaGateFn d={d}")


# ------------------------------------------------------------------------------------------------ 2. accumulation into .grad
def test_beta_gate_arms_accumulate_into_grad(ops):
    d = 136
    plain = run(ops, d)
    a = run(ops, d, fused=True)
    with flags(ops, GATE_PAIR=False, GATE_TWO_STREAMS=False):
        assert_same(a, run(ops, d, fused=True), "accumulating, defaults | serial")
    judge_beta_gate(ops, a, d, "BetaGateFn accumulating", plain)


# ------------------------------------------------------------------------------------------------ 3. PooledGateFn
@pytest.mark.parametrize("d", WIDTHS)
def test_pooled_gate_arms(ops, d, monkeypatch):
    from hri_emo_amd import _lib
    name = f"PooledGateFn d={d}"
    c = case(d)
    a = run(ops, d, pooled=True)
    if d == 136:
        monkeypatch.setattr(_lib.lib(), "hriemo_ln_pool_pair_supported", lambda d_: 0)
        assert_same(a, run(ops, d, pooled=True), name + ", pair | two single launches")
        monkeypatch.undo()
    (xa, xt, mean_a, rstd_a, mean_t, rstd_t, gin, a_pool, t_pool, cnt, hid, w, w1_16, w2_16, ga, gt, h_a32, h_t32, abar, tbar) = a["saved"]
    nk = G.chunks(LT, G.POOL_ROWS)
    for side, mean, rstd, bar, tag in ((c["sides"][0], mean_a, rstd_a, abar, " audio"), (c["sides"][1], mean_t, rstd_t, tbar, " text")):
        judge_ln(None, mean, rstd, side, name + tag)
        # the unmasked mean over l < LT from the inputs: every keep partial within pool_part_factor(rows) v mag (check_keep), their
        # mean pool_factor(nk) more roundings (check_fuse_fwd's abar / tbar)
        kr, km = PG.keep_ref(side, LT)
        R.check_elem(bar.cpu(), kr.sum(1) / LT, km.sum(1) / LT, G.pool_part_factor(G.POOL_ROWS) + G.pool_factor(nk), True, name + tag + " mean")
    w64, a64, t64 = w.double().cpu(), abar.double().cpu(), tbar.double().cpu()
    R.check_elem(a["out"].cpu(), w64 * a64 + (1 - w64) * t64, w64 * a64.abs() + (1 - w64) * t64.abs(), G.FUSE_ROUNDINGS, True, name + " pooled")
    judge_beta(ops, a["beta"], w, hid, w2_16, a["params"][7], name)
    f32 = dict(dtype=torch.float32, device=DEV)
    dwf, g_a, g_t = torch.empty((B, d), **f32), torch.empty((B, d), **f32), torch.empty((B, d), **f32)
    dpooled, dbeta = c["dpooled"].to(DEV), c["dbeta"].to(DEV)
    _lib.call("hriemo_pooled_fuse_bwd", dpooled.data_ptr(), abar.data_ptr(), tbar.data_ptr(), w.data_ptr(), LT, dwf.data_ptr(), g_a.data_ptr(),
              g_t.data_ptr(), B, d, TV.stream())
    TV.show(name, PG.check_fuse_bwd({"dw": dwf.cpu(), "ga": g_a.cpu(), "gt": g_t.cpu()}, {"Lkeep": LT, "dpooled": c["dpooled"], "w": w.cpu()},
                                    abar.cpu(), tbar.cpu(), name))
    da, dt, ref = mlp_backward(ops, dwf, 1, dbeta, w, hid, gin, a_pool, t_pool, cnt, w1_16, w2_16, a["params"], d)
    for side, g, dpool, m32, r32, dx, gn, bn, tag in ((c["sides"][0], g_a, da, mean_a, rstd_a, a["dxa"], "ga", "ba", " audio"),
                                                     (c["sides"][1], g_t, dt, mean_t, rstd_t, a["dxt"], "gt", "bt", " text")):
        o = PG.vec_ops(side, {"g": g.cpu(), "dpool": dpool.cpu(), "Lkeep": LT})
        TV.judge_bwd({"dX": dx.cpu(), "dgamma": a[gn].cpu(), "dbeta": a[bn].cpu()}, side, o, 1, m32.cpu(), r32.cpu(), name + tag)
    judge_mlp(a, ref, name)
