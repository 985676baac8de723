"""GPU suite of DeviceAdamW(clip="group" | "parameter") on the d = 128 model (cfg1_train_p0): against a torch twin that is given
COPIES OF THE SAME GRADIENTS and runs per-unit torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with the same groups -- under
LambdaLR with one lambda per group and under GradScaler with a forced inf step --, with averaging and a health log attached, through
state dicts in both directions, and recorded inside captured packed steps.

Bounds are those of test_gpu_optimizer.py: |x - ref| <= 2e-6 * max(1, |ref|) per parameter tensor against the twin, 1e-5 relative
for norms and coefficients.  The groups are optim.decay_groups' (matrices / vectors) with max_norm 0.05 / 5.0: the matrix group's
norm is about 5.7 and the vector group's about 0.75 on this batch, and 14 of the 40 matrices exceed 0.05 on their own, so both modes
have clipped AND unclipped units -- asserted from the twin's norms in every step.

Bit-identity claims and why they hold: an optimizer recorded in a captured step launches the kernels its eager step() launches, so
"captured step with the update inside" equals "the same captured forward / backward followed by the eager opt.step()"; the health
kernels only read the gradient buffer on a skipped step, so its record equals that of a clip="global" optimizer on the same
gradients (grad_norm excepted on a finite skip: the unit modes add the same squares in another order -- the test skips on a NaN,
where both hold NaN)."""
import copy

import numpy as np
import pytest
import torch

from clip_reference import clip_units_torch, torch_units
from test_gpu_optimizer_groups import Spy, copy_grads, golden_batch, inverse_decay, make_twin, small_model, step_loss, warmup_cosine

pytestmark = pytest.mark.gpu

MODES = ["group", "parameter"]
MN = (0.05, 5.0)


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)


def bits(t):
    return t.view(torch.int32)


def clip_groups(named):
    """decay_groups' split with max_norm 0.05 for the matrices and 5.0 for the vectors"""
    from hri_emo_amd.optim import decay_groups
    groups = decay_groups(named, 1e-2)
    assert len(groups) == 2
    for g, mn in zip(groups, MN):
        g["max_norm"] = mn
    return groups


def plain_groups(named):
    """the same split without the max_norm keys (what clip="global" takes)"""
    return [{k: v for k, v in g.items() if k != "max_norm"} for g in clip_groups(named)]


def build(m, **kw):
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    buckets = GradBuckets(m.parameters(), overlap=False)
    return buckets, DeviceAdamW(buckets, **kw)


def twin_units(mode, m, twin, buckets, ref_opt):
    """the twin's clip units in the optimizer's unit order"""
    name_of = {id(p): n for n, p in m.named_parameters()}
    flat = [twin[name_of[id(p)]] for p in sorted(buckets.params, key=lambda q: buckets._offsets[id(q)])]
    return torch_units(mode, ref_opt.param_groups, flat)


def assert_close_to_twin(m, twin, what):
    for n, p in m.named_parameters():
        err = (p.detach() - twin[n].detach()).abs().max().item()
        assert err <= 2e-6 * max(1.0, twin[n].abs().max().item()), (what, n, err)


def ref_adamw(twin):
    groups = clip_groups(twin.items())
    opt = torch.optim.AdamW([{k: v for k, v in g.items() if k != "max_norm"} for g in groups], lr=1e-3, weight_decay=1e-2)
    for g, mn in zip(opt.param_groups, MN):
        g["max_norm"] = mn
    return opt


# ------------------------------------------------------------------------------------------------- 1. against the torch twin
@pytest.mark.parametrize("mode", MODES)
def test_unit_clip_follows_the_torch_twin_under_two_lambdas(H, mode):
    """three steps, LambdaLR(opt, [f0, f1]); per unit the norm and coefficient clip_arrays() reports against the twin's
    clip_grad_norm_, the parameters against the twin's"""
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = ref_adamw(twin)
    buckets, opt = build(m, param_groups=clip_groups(m.named_parameters()), lr=1e-3, weight_decay=1e-2, max_norm=1.0, clip=mode)
    assert [g["max_norm"] for g in opt.param_groups] == list(MN)
    units = twin_units(mode, m, twin, buckets, ref_opt)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [warmup_cosine(), inverse_decay])
    ref_sched = torch.optim.lr_scheduler.LambdaLR(ref_opt, [warmup_cosine(), inverse_decay])
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        step_loss(m, batch).backward()
        copy_grads(m, twin)
        total = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in twin.values()])))
        norms = clip_units_torch(units)
        clipped = [mn is not None and mn > 0 and nu > mn for nu, (_, mn) in zip(norms, units)]
        assert any(clipped) and not all(clipped), ("the twin must have clipped and unclipped units", step, norms)
        assert tuple(g["lr"] for g in opt.param_groups) == tuple(g["lr"] for g in ref_opt.param_groups)
        ref_opt.step(); ref_sched.step()
        opt.step(); sched.step()
        a = opt.clip_arrays()
        assert a["mode"] == mode and len(a["norm"]) == len(units) and a["max_norm"] == [mn for _, mn in units]
        coefs = [min(1.0, mn / (nu + 1e-6)) for nu, (_, mn) in zip(norms, units)]
        for u, (nu, cu) in enumerate(zip(norms, coefs)):
            assert abs(float(a["norm"][u]) - nu) <= 1e-5 * nu + 1e-30 and abs(float(a["coef"][u]) - cu) <= 1e-5 * cu, (step, u, a["norm"][u], nu)
        assert abs(float(opt.grad_norm) - total) <= 1e-5 * total, "grad_norm stays the norm over everything"
        assert float(opt._state[2]) == float(a["coef"].min()), "state.coef holds the smallest unit coefficient"
        assert_close_to_twin(m, twin, (mode, step))
    assert float(opt.device_step) == 3.0 and float(opt.skipped) == 0.0
    with torch.no_grad():
        m.eval()(*batch[:4])


def test_unit_modes_without_param_groups(H):
    """G = 1: clip="parameter" clips every tensor against the constructor's max_norm; clip="group" with one group IS the global
    clip, to the project's bounds (the sums are formed in another order)"""
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(list(twin.values()), lr=1e-3, weight_decay=1e-2)
    ref_opt.param_groups[0]["max_norm"] = 0.05
    buckets, opt = build(m, lr=1e-3, weight_decay=1e-2, max_norm=0.05, clip="parameter")
    assert len(opt.param_groups) == 1 and opt._unit_group.numel() == len(buckets.params)
    units = twin_units("parameter", m, twin, buckets, ref_opt)
    for step in range(2):
        opt.zero_grad()
        step_loss(m, batch).backward()
        copy_grads(m, twin)
        norms = clip_units_torch(units)
        assert any(nu > 0.05 for nu in norms) and any(nu <= 0.05 for nu in norms)
        ref_opt.step(); opt.step()
        assert_close_to_twin(m, twin, step)
    m2 = small_model(H)
    twin2 = make_twin(m2)
    ref2 = torch.optim.AdamW(list(twin2.values()), lr=1e-3, weight_decay=1e-2)
    _, opt2 = build(m2, lr=1e-3, weight_decay=1e-2, max_norm=0.05, clip="group")
    opt2.zero_grad()
    step_loss(m2, batch).backward()
    copy_grads(m2, twin2)
    tn = float(torch.nn.utils.clip_grad_norm_(list(twin2.values()), 0.05))
    ref2.step(); opt2.step()
    a = opt2.clip_arrays()
    assert a["unit"] == [0] and abs(float(a["norm"][0]) - tn) <= 1e-5 * tn and float(a["norm"][0]) == float(opt2.grad_norm)
    assert_close_to_twin(m2, twin2, "one group")


# --------------------------------------------------------------------------------------------------------------- 2. GradScaler
@pytest.mark.parametrize("mode", MODES)
def test_grad_scaler_with_a_forced_inf_step(H, mode):
    """GradScaler.step(opt) without unscale_: the unscale is fused into every unit's coefficient.  Step 1 carries an inf in one
    gradient: both sides skip, both scalers back off, and the norms of that step are in clip_state while its coefficients are not"""
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = ref_adamw(twin)
    buckets, opt = build(m, param_groups=clip_groups(m.named_parameters()), lr=1e-3, weight_decay=1e-2, clip=mode)
    units = twin_units(mode, m, twin, buckets, ref_opt)
    scaler, ref_scaler = torch.amp.GradScaler("cuda"), torch.amp.GradScaler("cuda")
    ref_scaler.scale(torch.zeros((), device="cuda"))
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        scaler.scale(step_loss(m, batch)).backward()
        if step == 1:
            buckets.flat[5] = float("inf")
            coef_before = opt.clip_arrays()["coef"]
        copy_grads(m, twin)
        ref_scaler.unscale_(ref_opt)
        if step != 1:
            clip_units_torch(units)
        ref_scaler.step(ref_opt); ref_scaler.update()
        scaler.step(opt); scaler.update()
        assert float(opt.skipped) == (1.0 if step >= 1 else 0.0)
        if step == 1:
            a = opt.clip_arrays()
            assert not np.isfinite(a["norm"]).all() and np.isfinite(a["norm"]).any(), "the unit that holds the inf shows in the norms"
            assert np.array_equal(a["coef"], coef_before), "a skipped step writes no coefficient"
        assert_close_to_twin(m, twin, (mode, step))
    assert float(opt.device_step) == 2.0 and scaler.get_scale() == ref_scaler.get_scale()


# ---------------------------------------------------------------------------------------------------- 3. averaging and the log
@pytest.mark.parametrize("mode", MODES)
def test_ema_average_moves_on_real_updates_and_stays_on_a_skipped_one(H, mode):
    batch = golden_batch()
    m = small_model(H)
    _, opt = build(m, param_groups=clip_groups(m.named_parameters()), lr=1e-3, weight_decay=1e-2, clip=mode, averaging="ema", avg_decay=0.5)
    for step in range(2):
        opt.zero_grad()
        step_loss(m, batch).backward()
        before = opt.avg.clone()
        opt.step()
        if step == 0:
            assert torch.equal(bits(opt.avg), bits(opt.flat_p)), "the first averaging update copies the parameters"
        else:
            want = before + 0.5 * (opt.flat_p - before)
            assert float((opt.avg - want).abs().max()) <= 2e-6 * max(1.0, float(want.abs().max()))
    assert float(opt.n_averaged) == 2.0
    opt.zero_grad()
    step_loss(m, batch).backward()
    opt.buckets.flat[-1] = float("nan")
    before = [t.clone() for t in (opt.avg, opt.flat_p, opt.m, opt.v, opt._avg_state)]
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.skipped) == 1.0 and float(opt.device_step) == 2.0
    for old, new, what in zip(before, (opt.avg, opt.flat_p, opt.m, opt.v, opt._avg_state), ("avg", "p", "m", "v", "avg_state")):
        assert torch.equal(bits(old), bits(new)), ("a skipped step moves nothing", what)
    with opt.averaged_weights():
        assert torch.equal(bits(opt.flat_p), bits(before[0]))
    assert "averaging" in opt.state_dict() and opt.state_dict()["clip"] == {"mode": mode}


@pytest.mark.parametrize("mode", MODES)
def test_health_record_of_a_skipped_step_equals_the_global_optimizers(H, mode):
    """the same gradients, one NaN among them, through a clip="global" and a unit-mode optimizer with health=True: the records are
    equal bit for bit (both grad_norm words hold NaN) and blame() names the same parameter; clip_state shows the unit too"""
    batch = golden_batch()
    ma = small_model(H)
    mb = copy.deepcopy(ma)
    ba, glob = build(ma, param_groups=plain_groups(ma.named_parameters()), lr=1e-3, weight_decay=1e-2, max_norm=5.0, health=True)
    bb, unit = build(mb, param_groups=clip_groups(mb.named_parameters()), lr=1e-3, weight_decay=1e-2, max_norm=5.0, clip=mode, health=True)
    for m_, opt in ((ma, glob), (mb, unit)):
        opt.health.name_parameters(m_.named_parameters())
    unit.name_parameters(mb.named_parameters())
    glob.zero_grad()
    step_loss(ma, batch).backward()
    order = sorted(ba.params, key=lambda q: ba._offsets[id(q)])
    victim = 3
    ba.flat[ba._offsets[id(order[victim])] + 1] = float("nan")
    bb.flat.copy_(ba.flat)
    glob.step(); unit.step()
    ra, rb = glob.health.arrays(), unit.health.arrays()
    assert ra["n_recorded"] == rb["n_recorded"] == 1 and ra["kind"].tolist() == rb["kind"].tolist() == [1]
    for key in ("step", "grad_sq", "nonfinite", "weight_sq", "update_sq"):
        assert np.array_equal(ra[key].view(np.int32), rb[key].view(np.int32)), key
    assert np.isnan(ra["grad_norm"]).all() and np.isnan(rb["grad_norm"]).all()
    assert glob.health.blame() == unit.health.blame() and [n for n, _ in unit.health.blame()] == [ra["names"][victim]]
    a = unit.clip_arrays()
    bad = [u for u, x in zip(a["unit"], a["norm"]) if np.isnan(x)]
    if mode == "parameter":
        assert bad == [ra["names"][victim]]
    else:
        owner = {id(p): gi for gi, g in enumerate(unit.param_groups) for p in g["params"]}
        order_b = sorted(bb.params, key=lambda q: bb._offsets[id(q)])
        assert bad == [owner[id(order_b[victim])]]


# --------------------------------------------------------------------------------------------------------------- 4. state dict
@pytest.mark.parametrize("mode", MODES)
def test_state_dict_round_trips_in_both_directions(H, mode):
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = ref_adamw(twin)
    buckets, opt = build(m, param_groups=clip_groups(m.named_parameters()), lr=1e-3, weight_decay=1e-2, clip=mode)
    units = twin_units(mode, m, twin, buckets, ref_opt)

    def one_step(tag):
        opt.zero_grad()
        step_loss(m, batch).backward()
        copy_grads(m, twin)
        clip_units_torch(units)
        ref_opt.step(); opt.step()
        assert_close_to_twin(m, twin, tag)

    one_step("before")
    sd, ref_sd = copy.deepcopy(opt.state_dict()), copy.deepcopy(ref_opt.state_dict())
    assert sd["clip"] == {"mode": mode} and [g["max_norm"] for g in sd["param_groups"]] == list(MN)
    assert list(sd["state"].keys()) == list(ref_sd["state"].keys())
    for d in (sd, ref_sd):
        d["param_groups"][0]["lr"], d["param_groups"][1]["lr"] = 5e-4, 7e-5
    ref_sd["param_groups"][0]["max_norm"] = 0.07              # the twin's dict carries the key too (ref_adamw put it there)
    opt.m.zero_(); opt.v.zero_()
    opt.load_state_dict(ref_sd)                                # a torch.optim.AdamW dict: no "clip" key
    ref_opt.load_state_dict(sd)                                # torch ignores the "clip" key
    ref_opt.param_groups[0]["max_norm"] = 0.07
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 7e-5] and [g["max_norm"] for g in opt.param_groups] == [0.07, 5.0]
    assert float(opt.device_step) == 1.0
    units = twin_units(mode, m, twin, buckets, ref_opt)
    one_step("after")
    assert 0.07 in opt.clip_arrays()["max_norm"] and 0.05 not in opt.clip_arrays()["max_norm"]
    other = "group" if mode == "parameter" else "parameter"
    with pytest.raises(ValueError, match=f"written with clip='{other}', this optimizer was built with clip='{mode}'"):
        opt.load_state_dict({**opt.state_dict(), "clip": {"mode": other}})
    opt.load_state_dict(opt.state_dict())


def test_clip_arrays_names(H):
    m = small_model(H)
    buckets, opt = build(m, param_groups=clip_groups(m.named_parameters()), clip="parameter")
    P = len(buckets.params)
    assert opt.clip_arrays()["unit"] == list(range(P)), "indices until names are attached"
    opt.name_parameters(m.named_parameters())
    name_of = {id(p): n for n, p in m.named_parameters()}
    a = opt.clip_arrays()
    assert a["unit"] == [name_of[id(p)] for p in sorted(buckets.params, key=lambda q: buckets._offsets[id(q)])]
    assert set(a) == {"mode", "unit", "norm", "coef", "max_norm"} and a["norm"].shape == a["coef"].shape == (P,)
    assert a["max_norm"] == [MN[0] if p.dim() >= 2 else MN[1] for p in sorted(buckets.params, key=lambda q: buckets._offsets[id(q)])]
    m2 = small_model(H)
    _, opt2 = build(m2, param_groups=clip_groups(m2.named_parameters()), clip="group")
    opt2.name_parameters(m2.named_parameters())
    a2 = opt2.clip_arrays()
    assert a2["unit"] == [0, 1] and a2["max_norm"] == list(MN) and a2["mode"] == "group"


# ------------------------------------------------------------------------------------------------------------ 5. in-graph steps
D, NE, NB, TA, TT = 128, 4, 5, 70, 40


def _batches():
    gen = torch.Generator().manual_seed(11)
    out = []
    for la, lt in (([70, 33, 32, 1, 17], [40, 1, 32, 31, 16]), ([12, 70, 5], [8, 40, 3])):
        out.append((torch.randn(sum(la), D, generator=gen).cuda(), torch.randn(sum(lt), D, generator=gen).cuda(), la, lt,
                    (torch.rand(len(la), NE, generator=gen) < 0.3).float().cuda()))
    return out


def _loss(accum):
    from hri_emo_amd.train import mosei_step_loss

    def loss(logits, beta, y, n_valid=None):
        return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=accum, n_valid=n_valid)
    return loss


def test_parameter_clip_inside_the_captured_packed_step(H):
    """capture_packed(optimizer=opt), clip="parameter": three replays equal the same captured forward / backward followed by the
    eager opt.step(), bit for bit -- losses, p, m, v, state and clip_state"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    b0 = _batches()[0]
    torch.manual_seed(3)
    m0 = H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=0.0).cuda().train()
    runs = {}
    for arm in ("in_graph", "graph_plus_eager"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, _loss(1), overlap=False)
        dp.set_global_batch(NB)
        opt = DeviceAdamW(dp.buckets, param_groups=clip_groups(m.named_parameters()), lr=1e-3, weight_decay=1e-2, clip="parameter")
        before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt._state, opt._clip_state)]
        dp.capture_packed(*b0, pad_to=(TA, TT), optimizer=opt if arm == "in_graph" else None)
        torch.cuda.synchronize()
        for old, new in zip(before, (opt.flat_p, opt.m, opt.v, opt._state, opt._clip_state)):
            assert torch.equal(old, new), "capture_packed() must not move parameters, moments, the state block or clip_state"
        losses = []
        for _ in range(3):
            losses.append(float(dp.step_packed(*b0)))
            if arm != "in_graph":
                opt.step()
        torch.cuda.synchronize()
        assert float(opt.device_step) == 3.0 and float(opt.skipped) == 0.0
        a = opt.clip_arrays()
        assert (a["coef"] < 1.0).any() and (a["coef"] == 1.0).any(), "clipped and unclipped units in the captured step"
        runs[arm] = (losses, opt.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt._state.clone(), opt._clip_state.clone())
        dp.release_graph()
    a, b = runs["in_graph"], runs["graph_plus_eager"]
    assert a[0] == b[0], (a[0], b[0])
    for x, y, what in zip(a[1:], b[1:], ("p", "m", "v", "state", "clip_state")):
        assert torch.equal(bits(x), bits(y)), what
    assert abs(a[0][2] - a[0][0]) > 1e-4, ("the updates must be visible in the loss", a[0])


def test_group_clip_with_accumulation_a_short_batch_and_an_average(H):
    """capture_packed(grad_accum=2, partial_batches=True, optimizer=opt), clip="group", averaging="ema": micro-step 0 is held --
    nothing of p, m, v, avg, clip_state moves --, micro-step 1 (a SHORT batch) carries one update.  Against the same captured
    micro-steps followed by the eager opt.step(): everything torch.equal over two groups of micro-steps."""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    batches = _batches()
    torch.manual_seed(3)
    m0 = H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=0.0).cuda().train()
    runs = {}
    for arm in ("in_graph", "graph_plus_eager"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, _loss(2), overlap=False)
        dp.set_global_batch(NB)
        opt = DeviceAdamW(dp.buckets, param_groups=clip_groups(m.named_parameters()), lr=1e-3, weight_decay=1e-2, clip="group",
                          averaging="ema", avg_decay=0.5)
        dp.capture_packed(*batches[0], pad_to=(TA, TT), optimizer=opt if arm == "in_graph" else None, grad_accum=2, partial_batches=True)
        torch.cuda.synchronize()
        losses = []
        for group in range(2):
            held = (opt.flat_p, opt.m, opt.v, opt.avg, opt._clip_state, opt._avg_state)
            before = [t.clone() for t in held] + [opt._state.clone()]
            losses.append(float(dp.step_packed(*batches[0])))
            torch.cuda.synchronize()
            st = opt._state.clone()
            st[1] = before[-1][1]
            assert all(torch.equal(bits(x), bits(y)) for x, y in zip(held + (st,), before)), "micro-step 0 is held"
            losses.append(float(dp.step_packed(*batches[1])))
            if arm != "in_graph":
                opt.step()
            torch.cuda.synchronize()
            assert float(opt.device_step) == group + 1.0 and float(opt.skipped) == 0.0 and float(opt.n_averaged) == group + 1.0
            assert not torch.equal(opt.flat_p, before[0]) and not torch.equal(opt._clip_state, before[4])
        runs[arm] = (losses,) + tuple(t.clone() for t in (opt.flat_p, opt.m, opt.v, opt.avg, opt._state, opt._clip_state))
        dp.release_graph()
    a, b = runs["in_graph"], runs["graph_plus_eager"]
    assert a[0] == b[0], (a[0], b[0])
    for x, y, what in zip(a[1:], b[1:], ("p", "m", "v", "avg", "state", "clip_state")):
        assert torch.equal(bits(x), bits(y)), what


# ------------------------------------------------------------------------------------------------------------ 6. launch lists
def test_launch_lists(H, monkeypatch):
    """clip="global" issues the _lib.call names it always did, in all four forms; a unit mode issues its three entries, the same
    three under a step-control block and -- with the _avg update -- under averaging; the health launches follow unchanged"""
    ctl = torch.tensor([5, 1, 1, 0], dtype=torch.int32, device="cuda")
    spy = Spy(monkeypatch)

    def lists(**kw):
        m = small_model(H)
        _, opt = build(m, **kw)
        spy.take()
        opt.step()
        eager = spy.take()
        opt._enqueue(ctl=ctl)
        return eager, spy.take()

    plain = ["hriemo_sumsq_f32", "hriemo_optim_finalize", "hriemo_adamw_flat_dev"]
    assert lists(clip="global") == (plain, ["hriemo_sumsq_f32", "hriemo_optim_finalize_ctl", "hriemo_adamw_flat_dev"])
    grouped = ["hriemo_sumsq_f32", "hriemo_optim_finalize_groups", "hriemo_adamw_flat_groups"]
    m = small_model(H)
    _, opt = build(m, param_groups=plain_groups(m.named_parameters()), clip="global")
    spy.take()
    opt.step(); opt._enqueue(ctl=ctl)
    assert spy.take() == grouped * 2
    avg = ["hriemo_sumsq_f32", "hriemo_optim_finalize_avg", "hriemo_adamw_flat_dev_avg"]
    assert lists(clip="global", averaging="swa") == (avg, avg)
    units = ["hriemo_sumsq_units", "hriemo_optim_finalize_units", "hriemo_adamw_flat_units"]
    for mode in MODES:
        assert lists(clip=mode) == (units, units)
        assert lists(clip=mode, averaging="ema") == (units[:2] + ["hriemo_adamw_flat_units_avg"],) * 2
        assert lists(clip=mode, health=True) == (units + ["hriemo_health_sweep", "hriemo_health_fold"],) * 2
    torch.cuda.synchronize()
