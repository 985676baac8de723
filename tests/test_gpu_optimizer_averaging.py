"""GPU suite of DeviceAdamW's in-graph weight averaging (hri_emo_amd.optim, csrc/optim.hip): hriemo_optim_finalize_avg,
hriemo_adamw_flat_dev_avg, hriemo_adamw_flat_groups_avg and hriemo_swap_fp32 through the C ABI on guarded buffers, and the optimizer
built with averaging= on the d = 128 model -- against torch.optim.AdamW + torch.optim.swa_utils.AveragedModel, recorded inside
captured steps, evaluated through averaged_weights(), through state dicts in both directions, and its launch lists.

Bounds.  p, m, v and state[]: BIT-identical to the existing entries run on clones (the averaging forms call the same per-vector
function).  avg after an averaging update: per element against float64 from the kernel's own fp32 inputs, within
avg_reference.avg_update_ref64's bound (derived there, every factor counted).  The weight w: bit for bit avg_reference.weight32.
Against the torch twin, per parameter: the average is a convex combination of parameter values, each within test_gpu_optimizer.py's
2e-6 * max(1, |ref|), so the exact combination is within the same; every averaging update after the first (which copies) then
rounds on either side -- ours: the fp32 weight (relative 2^-24 of w, times |p - avg| <= 2 R), the difference and the fma; torch's
lerp likewise -- at most 4 roundings of 2^-24 R each per side, R = max(1, max |ref|): (2e-6 + 8 k 2^-24) R after k such updates.

The kernel sequences.  The issue words its sequence as five events with start = 1, every = 2 whose SECOND update is the first
averaging update; under the rule it fixes (t > start and (t - start) % every == 0) the second update (t = 2) does not average with
every = 2.  Both readings run: "start 1 every 2" keeps those parameters and carries every kind of event the issue names -- a
non-averaging update, the first averaging update (avg = p bit for bit), a found_inf skip, a hold, a later averaging update --
in seven events; "start 1 every 1" is the five-event order as worded."""
import copy

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from avg_reference import avg_update_ref64, walk, weight32
from rowops_reference import GuardedVec
from test_gpu_eval_step import NB, PAD, _batches, _close, _eager, _keep, _loss, _model
from test_gpu_optimizer_groups import (CASES, GV, HYPER, N_SWEEP, SENTINEL, ST, VEC, Spy, build, golden_batch, small_model, step_loss,
                                       two_groups)

pytestmark = pytest.mark.gpu

MODE_WORD = {"ema": 1.0, "swa": 2.0}
SCHEDULES = {
    "start 1 every 2": (1, 2, ["update", "update", "update", "skip", "hold", "update", "update"],
                        ["none", "none", "first", "untouched", "untouched", "none", "update"]),
    "start 1 every 1": (1, 1, ["update", "update", "skip", "hold", "update"], ["none", "first", "untouched", "untouched", "update"]),
}


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    yield hri_emo_amd
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_ingest(False)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- 1. kernels
def _run_form(form, n, seg_h, sg_h, mode, decay, start, every, events, records):
    from hri_emo_amd import _lib
    G, S, nblocks = (3, len(sg_h), 1024) if form == "groups" else (1, 1, 1024)
    gen = torch.Generator(device="cuda").manual_seed(n + G)
    pad = n >= 8                                                # the last vector plays a parameter's padding: zeros in p and g
    p0 = torch.randn(n, generator=gen, device="cuda")
    if pad:
        p0[-4:] = 0.0
    p, m, v, g = GV(p0), GV(torch.zeros(n)), GV(torch.zeros(n)), GuardedVec(n, torch.float32, device="cuda")
    avg = GV(p0)                                                # the bit copy the optimizer starts from
    partial, hyper = GuardedVec(nblocks, torch.float32, device="cuda"), GV(HYPER[:G].reshape(-1))
    state0 = torch.full((G * 8,), SENTINEL)
    state0[:8] = 0.0
    state = GV(state0)
    avg_hyper = GV(torch.tensor([MODE_WORD[mode], decay, float(start), float(every)], dtype=torch.float32))
    avg_state = GV(torch.zeros(4))
    seg, seg_group = GV(torch.tensor(seg_h, dtype=torch.int64)), GV(torch.tensor(sg_h, dtype=torch.int32))
    ctl = GV(torch.tensor([5, 0, 0, 0], dtype=torch.int32))
    scale_t, inf_t = torch.tensor([8.0], device="cuda"), torch.zeros(1, device="cuda")
    bufs = [p, m, v, g, avg, partial, hyper, state, avg_hyper, avg_state, seg, seg_group, ctl]
    P = lambda t: None if t is None else t.data_ptr()
    C = lambda c: None if c is None else c.ptr

    def update_avg():
        if form == "dev":
            _lib.call("hriemo_adamw_flat_dev_avg", p.ptr, g.ptr, m.ptr, v.ptr, n, hyper.ptr, state.ptr, avg.ptr, avg_state.ptr, ST())
        else:
            _lib.call("hriemo_adamw_flat_groups_avg", p.ptr, g.ptr, m.ptr, v.ptr, n, seg.ptr, seg_group.ptr, S, hyper.ptr, state.ptr, G,
                      avg.ptr, avg_state.ptr, ST())

    def new(gs, fi, c):
        _lib.call("hriemo_sumsq_f32", g.ptr, n, partial.ptr, nblocks, ST())
        _lib.call("hriemo_optim_finalize_avg", partial.ptr, nblocks, hyper.ptr, G, P(gs), P(fi), state.ptr, C(c), avg_hyper.ptr,
                  avg_state.ptr, ST())
        update_avg()
        torch.cuda.synchronize()

    def old(pre, gs, fi, c):
        """the EXISTING entries on clones of p, m, v, state -> their views"""
        pc, mc, vc, sc = (GV(t) for t in pre)
        _lib.call("hriemo_sumsq_f32", g.ptr, n, partial.ptr, nblocks, ST())
        if form == "groups":
            _lib.call("hriemo_optim_finalize_groups", partial.ptr, nblocks, hyper.ptr, G, P(gs), P(fi), sc.ptr, C(c), ST())
            _lib.call("hriemo_adamw_flat_groups", pc.ptr, g.ptr, mc.ptr, vc.ptr, n, seg.ptr, seg_group.ptr, S, hyper.ptr, sc.ptr, G, ST())
        else:
            if c is None:
                _lib.call("hriemo_optim_finalize", partial.ptr, nblocks, hyper.ptr, P(gs), P(fi), sc.ptr, ST())
            else:
                _lib.call("hriemo_optim_finalize_ctl", partial.ptr, nblocks, hyper.ptr, P(gs), P(fi), sc.ptr, c.ptr, ST())
            _lib.call("hriemo_adamw_flat_dev", pc.ptr, g.ptr, mc.ptr, vc.ptr, n, hyper.ptr, sc.ptr, ST())
        torch.cuda.synchronize()
        for b in (pc, mc, vc, sc):
            b.assert_intact("clone")
        return pc.view, mc.view, vc.view, sc.view

    def intact():
        for i, b in enumerate(bufs):
            b.assert_intact(f"{form} buffer {i}")

    n_updates = sum(ev == "update" for ev in events)
    seen = 0
    for i, (ev, (t, kind, n_avg, w_ref)) in enumerate(zip(events, records)):
        gs = fi = c = None
        scale = 1.5
        if ev == "update":
            seen += 1
            if seen == 2:                                      # scaled gradients, the unscale fused into the clip coefficient
                gs, fi, scale = scale_t, inf_t, 8.0 * 3.0
            if seen == n_updates:                              # the last one through the step-control block, last = 1
                ctl.view[2] = 1
                c = ctl
        elif ev == "skip":
            inf_t.fill_(1.0)
            gs, fi = scale_t, inf_t
        else:
            ctl.view[2] = 0
            c = ctl
        gh = torch.randn(n, generator=gen, device="cuda") * scale
        if pad:
            gh[-4:] = 0.0
        g.view.copy_(gh)
        pre = [b.view.clone() for b in (p, m, v, state)]
        pre_avg, pre_as = avg.view.clone(), avg_state.view.clone()
        new(gs, fi, c)
        what = f"{form} event {i} ({ev}, t = {t}, {kind})"
        for got, ref, name in zip((p.view, m.view, v.view, state.view), old(pre, gs, fi, c), ("p", "m", "v", "state")):
            assert same_bits(got, ref), (what, name, "differs from the existing entries")
        assert float(state.view[0]) == t, what
        a_s = avg_state.view.cpu()
        if kind == "untouched":
            assert same_bits(avg.view, pre_avg) and same_bits(avg_state.view, pre_as), (what, "a skipped / held step moved the average")
            assert float(state.view[1]) == 1.0
        else:
            assert float(state.view[1]) == 0.0 and not same_bits(p.view, pre[0]), what
            assert float(a_s[3]) == t, (what, "stamp")
            if kind == "none":
                assert same_bits(avg.view, pre_avg) and same_bits(avg_state.view[:2], pre_as[:2]) and float(a_s[2]) == 0.0, what
            else:
                assert float(a_s[0]) == n_avg == float(pre_as[0]) + 1 and float(a_s[2]) == (2.0 if kind == "first" else 1.0), (what, a_s)
                assert same_bits(a_s[1], w_ref), (what, "w", float(a_s[1]), float(w_ref))
                if kind == "first":
                    assert same_bits(avg.view, p.view), (what, "the first averaging update copies the bits of p")
                else:
                    ref, bound = avg_update_ref64(pre_avg, p.view, a_s[1])
                    err = (avg.view.double() - ref).abs()
                    print(f"{what}: w {float(a_s[1]):.6e}  max |err| {float(err.max()):.3e}  max err / bound {float((err / bound).max()):.3f}")
                    assert bool((err <= bound).all()), (what, float(err.max()), float((err / bound).max()))
                    assert not same_bits(avg.view, pre_avg) and not same_bits(avg.view, p.view), (what, "the average did not move")
        if pad:
            assert int(bits(avg.view[-4:]).abs().sum()) == 0 and int(bits(p.view[-4:]).abs().sum()) == 0, (what, "padding stays +0")
        intact()
        inf_t.fill_(0.0)
    assert [r[1] for r in records].count("update") >= 1 and float(avg_state.view[0]) == records[-1][2]
    # a stale flag is no update: the flag word set, the stamp that of another step -- and a word that is no flag under the right stamp
    g.view.copy_(torch.randn(n, generator=gen, device="cuda"))
    for flag, stamp in ((1.0, float(state.view[0]) - 1.0), (2.0, 0.0), (7.0, float(state.view[0]))):
        avg_state.view[2], avg_state.view[3] = flag, stamp
        state.view[1] = 0.0
        pre_p, pre_avg = p.view.clone(), avg.view.clone()
        update_avg()
        torch.cuda.synchronize()
        assert same_bits(avg.view, pre_avg) and (n < 8 or not same_bits(p.view, pre_p)), (form, "stale flag", flag, stamp)
    intact()


@pytest.mark.parametrize("schedule", list(SCHEDULES), ids=list(SCHEDULES))
@pytest.mark.parametrize("mode", ["ema", "swa"])
@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_averaging_kernels_through_the_c_abi(H, case, mode, schedule):
    """hriemo_sumsq_f32 -> hriemo_optim_finalize_avg -> hriemo_adamw_flat_dev_avg (G = 1) and -> hriemo_adamw_flat_groups_avg
    (G = 3, the groups test's segment tables) over a sequence of real updates, a found_inf skip and a hold: p, m, v and state[]
    bit-identical to the existing entries on clones after EVERY event; avg, avg_state and the guards as the module docstring says"""
    n, seg_h, sg_h = CASES[case]
    start, every, events, kinds = SCHEDULES[schedule]
    decay = 0.9
    records = walk(mode, decay, start, every, events)
    assert [r[1] for r in records] == kinds, "the sequence must hold the events its name promises"
    for form in ("dev", "groups"):
        _run_form(form, n, seg_h, sg_h, mode, decay, start, every, events, records)


@pytest.mark.parametrize("n", [4, 3072, N_SWEEP + 8])
def test_swap_exchanges_every_bit(H, n):
    """NaN payloads (quiet, signalling, negative), -0, denormals and infinities cross unchanged, the guards stay, a second swap
    restores both buffers; n % 4 != 0, overlapping and identical buffers are refused in front of the launch"""
    from hri_emo_amd import _lib
    special = torch.tensor([0x7FC12345, -0x3FFFFF, 0x7F800001, -0x80000000, 0x00000001, -0x7F800001, 0x7F800000, 0x007FFFFF], dtype=torch.int64)
    special = special.to(torch.int32)                           # 0xFFC00001, 0x80000000, 0x807FFFFF as two's complement
    gen = torch.Generator().manual_seed(n)
    a0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    b0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    a0[:4], b0[:4] = special[:4], special[4:]
    if n >= 16:
        a0[-8:], b0[-8:] = special.flip(0), special
    a, b = GV(a0.view(torch.float32)), GV(b0.view(torch.float32))
    _lib.call("hriemo_swap_fp32", a.ptr, b.ptr, n, ST())
    torch.cuda.synchronize()
    assert torch.equal(bits(a.view).cpu(), b0) and torch.equal(bits(b.view).cpu(), a0)
    a.assert_intact("a"); b.assert_intact("b")
    for args, msg in (((a.ptr, b.ptr, n + 2), "multiple of 4"), ((a.ptr, a.ptr, n), "overlap"), ((a.ptr, a.ptr + 16, n), "overlap")):
        if msg == "overlap" and n == 4 and args[1] != args[0]:
            continue                                            # 16 bytes apart at n = 4: two neighbouring vectors, no overlap
        with pytest.raises(RuntimeError, match="swap_fp32.*" + msg):
            _lib.call("hriemo_swap_fp32", *args, ST())
    torch.cuda.synchronize()
    assert torch.equal(bits(a.view).cpu(), b0) and torch.equal(bits(b.view).cpu(), a0), "a refused call launches nothing"
    _lib.call("hriemo_swap_fp32", a.ptr, b.ptr, n, ST())
    torch.cuda.synchronize()
    assert torch.equal(bits(a.view).cpu(), a0) and torch.equal(bits(b.view).cpu(), b0), "a second swap restores both buffers"
    a.assert_intact("a"); b.assert_intact("b")


# ------------------------------------------------------------------------------------------------- 2. against torch's AveragedModel
class Holder(torch.nn.Module):
    """the CPU twin's parameters as a module (AveragedModel wants one), in the model's named_parameters order"""

    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)


@pytest.mark.parametrize("mode,grouped", [("ema", False), ("swa", False), ("ema", True), ("swa", True)],
                         ids=["ema", "swa", "ema two groups", "swa two groups"])
def test_average_follows_adamw_plus_averaged_model(H, mode, grouped):
    """six steps, avg_start = 2, avg_every = 2 (averaging updates at t = 4, the copy, and t = 6), step 3 clipped: the twin is a CPU
    clip_grad_norm_ + torch.optim.AdamW + AveragedModel fed copies of the same gradients, update_parameters called on exactly the
    averaging steps"""
    from hri_emo_amd.optim import is_averaging_step
    decay, start, every = 0.9, 2, 2
    batch = golden_batch()
    m = small_model(H)
    names = [n for n, _ in m.named_parameters()]
    holder = Holder([torch.nn.Parameter(p.detach().cpu().clone()) for _, p in m.named_parameters()])
    twin = dict(zip(names, holder.ps))
    ref_opt = torch.optim.AdamW(two_groups(twin.items(), **VEC) if grouped else list(holder.parameters()), lr=1e-3, weight_decay=1e-2)
    am = AveragedModel(holder, multi_avg_fn=get_ema_multi_avg_fn(decay)) if mode == "ema" else AveragedModel(holder)
    kw = dict(param_groups=two_groups(m.named_parameters(), **VEC)) if grouped else {}
    buckets, opt = build(H, m, lr=1e-3, weight_decay=1e-2, max_norm=5.0, averaging=mode, avg_decay=decay, avg_start=start,
                         avg_every=every, **kw)
    start_bits = opt.flat_p.clone()
    assert same_bits(opt.avg, start_bits) and float(opt.n_averaged) == 0.0
    later = 0
    for step in range(6):
        opt.zero_grad(set_to_none=True)
        step_loss(m, batch, 40.0 if step == 3 else 1.0).backward()
        for n, p in m.named_parameters():
            twin[n].grad = p.grad.detach().cpu().clone()
        torch.nn.utils.clip_grad_norm_(list(holder.parameters()), 5.0)
        ref_opt.step()
        opt.step()
        t = step + 1
        if is_averaging_step(t, start, every):
            later += int(am.n_averaged) > 0
            am.update_parameters(holder)
        assert float(opt.device_step) == t and float(opt.n_averaged) == int(am.n_averaged), (t, float(opt.n_averaged), int(am.n_averaged))
        if int(am.n_averaged) == 0:
            assert same_bits(opt.avg, start_bits), "before the first averaging update the average keeps every bit"
        for i, (n, p) in enumerate(m.named_parameters()):
            ref = twin[n].detach()
            err = float((p.detach().cpu() - ref).abs().max())
            assert err <= 2e-6 * max(1.0, float(ref.abs().max())), (t, n, "p", err)
            if int(am.n_averaged) > 0:
                aref = am.module.ps[i].detach()
                aerr = float((opt._avg_view(p).cpu() - aref).abs().max())
                tol = (2e-6 + 8 * later * 2.0 ** -24) * max(1.0, float(aref.abs().max()))
                assert aerr <= tol, (t, n, "avg", aerr, tol)
    assert float(opt.n_averaged) == 2.0 and later == 1 and float(opt.skipped) == 0.0
    assert not same_bits(opt.avg, opt.flat_p), "after the second averaging update the average is not the parameters"


# ------------------------------------------------------------------------------------------------------------ 3. in-graph steps
def test_averaging_inside_the_captured_step(H):
    """capture(optimizer=opt) with averaging="ema", start 1, every 1: the replay that holds the update against the same captured
    forward / backward followed by the eager opt.step() -- loss, p, m, v, avg and n_averaged bit for bit over four steps; a replay
    inside averaged_weights() raises before anything is enqueued"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import fusion_step_loss
    batch = golden_batch()
    m0 = small_model(H, closed_form=False, seed=11)
    runs = {}
    for mode in ("in_graph", "graph_plus_eager"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0, averaging="ema", avg_decay=0.5, avg_start=1, avg_every=1)
        before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt._state, opt.avg, opt._avg_state)]
        dp.capture(*batch, optimizer=opt if mode == "in_graph" else None)
        torch.cuda.synchronize()
        for old, new in zip(before, (opt.flat_p, opt.m, opt.v, opt._state, opt.avg, opt._avg_state)):
            assert same_bits(old, new), "capture() must not move parameters, moments, the average or the state blocks"
        losses = []
        for step in range(4):
            losses.append(float(dp.step(*batch)))
            if mode != "in_graph":
                opt.step()
            assert float(opt.n_averaged) == max(0, step), (mode, step)
            if step == 1:
                assert same_bits(opt.avg, opt.flat_p), "the first averaging update copies"
        if mode == "in_graph":
            kept = [t.clone() for t in (opt.flat_p, opt.avg, opt.buckets.flat, opt._state)]
            with opt.averaged_weights():
                with pytest.raises(RuntimeError, match="inside `with opt.averaged_weights"):
                    dp.step(*batch)
            torch.cuda.synchronize()
            for old, new in zip(kept, (opt.flat_p, opt.avg, opt.buckets.flat, opt._state)):
                assert same_bits(old, new), "the refused replay enqueued nothing, the way out restored the parameters"
        assert float(opt.device_step) == 4.0 and float(opt.skipped) == 0.0
        runs[mode] = (losses, opt.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.avg.clone(), opt._avg_state.clone())
        dp.release_graph()
    a, b = runs["in_graph"], runs["graph_plus_eager"]
    assert a[0] == b[0], (a[0], b[0])
    for x, y, what in zip(a[1:], b[1:], ("p", "m", "v", "avg", "avg_state")):
        assert same_bits(x, y), what
    assert not same_bits(a[4], a[1])


def test_averaging_inside_the_packed_step_with_accumulation_a_short_batch_and_a_skip(H):
    """capture_packed(grad_accum=2, partial_batches=True, optimizer=opt) with two groups and averaging="swa": three groups of two
    micro-steps, the second micro-step a SHORT batch.  Micro-step 0 is held: nothing of the average moves.  The middle group's
    gradient buffer is poisoned with an inf between its micro-steps, so its update is SKIPPED on the device: n_averaged advances
    once per group of micro-steps and not on the skipped one.  Against the same captured micro-steps followed by the eager
    opt.step(): p, m, v, avg, n_averaged bit for bit."""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import mosei_step_loss
    D, NE, NB_, TA, TT = 128, 4, 5, 70, 40
    gen = torch.Generator().manual_seed(11)
    batches = []
    for la, lt in (([70, 33, 32, 1, 17], [40, 1, 32, 31, 16]), ([12, 70, 5], [8, 40, 3])):
        batches.append((torch.randn(sum(la), D, generator=gen).cuda(), torch.randn(sum(lt), D, generator=gen).cuda(), la, lt,
                        (torch.rand(len(la), NE, generator=gen) < 0.3).float().cuda()))

    def loss_half(logits, beta, y, n_valid=None):
        return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=2, n_valid=n_valid)

    torch.manual_seed(3)
    m0 = H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=0.0).cuda().train()
    runs = {}
    for mode in ("in_graph", "graph_plus_eager"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, loss_half, overlap=False)
        dp.set_global_batch(NB_)
        opt = DeviceAdamW(dp.buckets, param_groups=two_groups(m.named_parameters(), **VEC), lr=1e-3, weight_decay=1e-2, max_norm=5.0,
                          averaging="swa")
        dp.capture_packed(*batches[0], pad_to=(TA, TT), optimizer=opt if mode == "in_graph" else None, grad_accum=2, partial_batches=True)
        torch.cuda.synchronize()
        want_n, want_t = [1.0, 1.0, 2.0], [1.0, 1.0, 2.0]
        for group in range(3):
            before = [t.clone() for t in (opt.flat_p, opt.avg, opt._avg_state)]
            dp.step_packed(*batches[0])
            torch.cuda.synchronize()
            assert all(same_bits(a, b) for a, b in zip((opt.flat_p, opt.avg, opt._avg_state), before)), "micro-step 0 is held"
            if group == 1:
                dp.buckets.flat[0] = float("inf")              # the running sum of this group: its norm is not finite
            dp.step_packed(*batches[1])
            if mode != "in_graph":
                opt.step()
            torch.cuda.synchronize()
            assert float(opt.n_averaged) == want_n[group] and float(opt.device_step) == want_t[group] and dp.micro_step == 0, (mode, group)
            assert float(opt.skipped) == (0.0 if group == 0 else 1.0)
            if group == 1:
                assert all(same_bits(a, b) for a, b in zip((opt.flat_p, opt.avg, opt._avg_state), before)), "a skipped update"
            else:
                assert not same_bits(opt.flat_p, before[0]) and not same_bits(opt.avg, before[1])
        runs[mode] = (opt.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.avg.clone(), opt._avg_state.clone())
        dp.release_graph()
    for x, y, what in zip(runs["in_graph"], runs["graph_plus_eager"], ("p", "m", "v", "avg", "avg_state")):
        assert same_bits(x, y), what


# ------------------------------------------------------------------------------------------------- 4. evaluation on the average
def _same(got, ref, what):
    for name, a, b in zip(("logits", "beta", "z", "loss"), got, ref):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and torch.equal(a, b), (what, name, float((a.double() - b.double()).abs().max()))


def _train_and_evaluate(H, enter):
    """three captured training steps with averaging, an evaluation on the average (enter=True) or none, a fourth step ->
    (loss of step 4, p, m, v, avg, avg_state)"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    m = _model(H)
    b0 = _batches()[0]
    dp = DataParallelStep(m, _loss(), overlap=False)
    dp.set_global_batch(NB)
    opt = DeviceAdamW(dp.buckets, lr=1e-2, weight_decay=1e-2, max_norm=5.0, averaging="ema", avg_decay=0.5)
    dp.capture_packed(*b0, pad_to=PAD, optimizer=opt)
    for _ in range(3):
        dp.step_packed(*b0)
    torch.cuda.synchronize()
    assert float(opt.n_averaged) == 3.0 and not same_bits(opt.avg, opt.flat_p)
    if enter:
        plain, stat = H.EvalStep(m, _loss()), H.EvalStep(m, _loss(), stationary=True)
        plain.capture_packed(*b0, pad_to=PAD)
        stat.capture_packed(*b0, pad_to=PAD)
        on_params = _keep(plain.eval_packed(*b0))
        _same(_keep(stat.eval_packed(*b0)), on_params, "on the parameters")
        p_bits, avg_bits = opt.flat_p.clone(), opt.avg.clone()
        # the reference: a fresh model loaded from averaged_state_dict(model), its own captured evaluation
        fresh = _model(H)
        fresh.load_state_dict(opt.averaged_state_dict(m))
        ref_step = H.EvalStep(fresh, _loss())
        ref_step.capture_packed(*b0, pad_to=PAD)
        ref = _keep(ref_step.eval_packed(*b0))
        assert not torch.equal(ref[0], on_params[0]), "the average evaluates differently from the parameters"
        with opt.averaged_weights() as inside:
            assert inside is opt and same_bits(opt.flat_p, avg_bits) and same_bits(opt.avg, p_bits)
            _same(_keep(plain.eval_packed(*b0)), ref, "EvalStep inside averaged_weights()")
            _same(_keep(stat.eval_packed(*b0)), ref, "EvalStep(stationary=True) inside averaged_weights()")
            _close(_keep(_eager(m, b0)), ref, "the eager forward inside averaged_weights()")
            for what, call in (("step", opt.step), ("replay", lambda: dp.step_packed(*b0)), ("state_dict", opt.state_dict),
                               ("load_state_dict", lambda: opt.load_state_dict({"state": {}, "param_groups": []})),
                               ("averaged_state_dict", lambda: opt.averaged_state_dict(m)),
                               ("nested", lambda: opt.averaged_weights().__enter__())):
                with pytest.raises(RuntimeError, match="inside `with opt.averaged_weights"):
                    call()
            assert dp.micro_step == 0
        assert same_bits(opt.flat_p, p_bits) and same_bits(opt.avg, avg_bits) and not opt._swapped
        _same(_keep(plain.eval_packed(*b0)), on_params, "EvalStep after the block")
        _same(_keep(stat.eval_packed(*b0)), on_params, "EvalStep(stationary=True) after the block")
        # an exception inside the block still swaps back
        with pytest.raises(KeyError, match="boom"):
            with opt.averaged_weights():
                assert same_bits(opt.flat_p, avg_bits)
                raise KeyError("boom")
        assert same_bits(opt.flat_p, p_bits) and same_bits(opt.avg, avg_bits) and not opt._swapped
        for es in (plain, stat, ref_step):
            es.release_graph()
    loss = float(dp.step_packed(*b0))
    torch.cuda.synchronize()
    out = (loss, opt.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.avg.clone(), opt._avg_state.clone())
    dp.release_graph()
    return out


def test_evaluation_on_the_average_and_training_continues_bit_identically(H):
    """inside averaged_weights() EvalStep -- default and stationary=True -- gives the bits of a fresh model loaded from
    averaged_state_dict(model), the eager forward agrees to its usual 1e-5; step(), a replay, state_dict() and a nested block
    raise; an exception swaps back; and the training step after the block equals, bit for bit, the same step of a run that never
    entered it"""
    a = _train_and_evaluate(H, enter=True)
    b = _train_and_evaluate(H, enter=False)
    assert a[0] == b[0], (a[0], b[0])
    for x, y, what in zip(a[1:], b[1:], ("p", "m", "v", "avg", "avg_state")):
        assert same_bits(x, y), what


# --------------------------------------------------------------------------------------------------------------- 5. state dicts
def test_state_dict_round_trips_and_torch_both_ways(H):
    batch = golden_batch()
    m = small_model(H)
    kw = dict(lr=1e-3, weight_decay=1e-2, max_norm=5.0, averaging="ema", avg_decay=0.75, avg_start=1, avg_every=1)
    buckets, opt = build(H, m, **kw)
    for step in range(3):
        opt.zero_grad()
        step_loss(m, batch).backward()
        opt.step()
    assert float(opt.n_averaged) == 2.0
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd) == {"state", "param_groups", "averaging"} and float(sd["averaging"]["n_averaged"]) == 2.0
    # round trip through DeviceAdamW: exact
    m2 = small_model(H)
    buckets2, opt2 = build(H, m2, **{**kw, "avg_decay": 0.5, "avg_start": 9})
    m2.load_state_dict(m.state_dict())                         # the model first, then the optimizer
    opt2.load_state_dict(sd)
    assert (opt2.avg_decay, opt2.avg_start, opt2.avg_every) == (0.75, 1, 1) and float(opt2.n_averaged) == 2.0
    for x, y, what in ((opt.flat_p, opt2.flat_p, "p"), (opt.m, opt2.m, "m"), (opt.v, opt2.v, "v"), (opt.avg, opt2.avg, "avg")):
        assert same_bits(x, y), what
    assert float(opt2.device_step) == 3.0
    opt.zero_grad()
    step_loss(m, batch).backward()
    buckets2.flat.copy_(buckets.flat)                          # the same gradients
    opt.step(); opt2.step()
    for x, y, what in ((opt.flat_p, opt2.flat_p, "p"), (opt.avg, opt2.avg, "avg"), (opt._avg_state, opt2._avg_state, "avg_state")):
        assert same_bits(x, y), (what, "after a step from the loaded state")
    assert float(opt2.n_averaged) == 3.0
    # into torch.optim.AdamW (the unknown top-level key is ignored) and back: the average restarts from the current parameters
    twin = [p.detach().clone().requires_grad_(True) for p in m.parameters()]
    ref_opt = torch.optim.AdamW(twin, lr=1e-3, weight_decay=1e-2)
    ref_opt.load_state_dict(sd)
    ref_sd = ref_opt.state_dict()
    assert "averaging" not in ref_sd and float(ref_sd["state"][0]["step"]) == 3.0
    opt.load_state_dict(ref_sd)
    assert float(opt.n_averaged) == 0.0 and same_bits(opt.avg, opt.flat_p) and float(opt.device_step) == 3.0
    assert same_bits(opt._avg_state, torch.zeros(4, device="cuda"))
    # another mode, other shapes: refused, nothing written
    before = [t.clone() for t in (opt2.avg, opt2.m, opt2._avg_state)]
    other = copy.deepcopy(sd)
    other["averaging"]["mode"] = "swa"
    with pytest.raises(ValueError, match="average is 'swa'"):
        opt2.load_state_dict(other)
    other = copy.deepcopy(sd)
    other["averaging"]["avg"][0] = other["averaging"]["avg"][0].reshape(-1)[:-1].clone()
    with pytest.raises(ValueError, match="averages' shapes do not match"):
        opt2.load_state_dict(other)
    for old, new in zip(before, (opt2.avg, opt2.m, opt2._avg_state)):
        assert same_bits(old, new)
    # without averaging= the dict is the dict of before
    m3 = small_model(H)
    _, opt3 = build(H, m3, lr=1e-3)
    assert set(opt3.state_dict()) == {"state", "param_groups"}


# ------------------------------------------------------------------------------------------------------------ 6. launch lists
def test_launch_lists_with_and_without_averaging(H, monkeypatch):
    """without averaging= the lists are those of before; with it three launches per step -- sumsq, the averaging finalize (one
    entry for plain, ctl and groups), the averaging update; averaged_weights() is one swap in and one out.  The host attributes are
    uploaded with hyper: a changed avg_start takes effect on the next step, an invalid one raises before anything is enqueued."""
    ctl = torch.tensor([5, 1, 1, 0], dtype=torch.int32, device="cuda")
    m0 = small_model(H)
    _, opt0 = build(H, m0)
    m1 = small_model(H)
    _, opt1 = build(H, m1, averaging="ema", avg_decay=0.9)
    m2 = small_model(H)
    _, opt2 = build(H, m2, param_groups=two_groups(m2.named_parameters()), averaging="swa")
    spy = Spy(monkeypatch)
    opt0.step()
    assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize", "hriemo_adamw_flat_dev"]
    opt0._enqueue(ctl=ctl)
    assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize_ctl", "hriemo_adamw_flat_dev"]
    for opt, update in ((opt1, "hriemo_adamw_flat_dev_avg"), (opt2, "hriemo_adamw_flat_groups_avg")):
        opt.step()
        assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize_avg", update]
        opt._enqueue(ctl=ctl)
        assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize_avg", update]
        with opt.averaged_weights():
            assert spy.take() == ["hriemo_swap_fp32"]
        assert spy.take() == ["hriemo_swap_fp32"]
        torch.cuda.synchronize()
        assert float(opt.device_step) == 2.0 and float(opt.n_averaged) == 2.0
    opt1.avg_start = 5
    opt1.step()
    assert float(opt1.device_step) == 3.0 and float(opt1.n_averaged) == 2.0, "avg_start = 5 travels with the hyper block"
    opt1.avg_start, opt1.avg_every = 0, 3
    opt1.step()
    opt1.step()
    opt1.step()
    assert float(opt1.device_step) == 6.0 and float(opt1.n_averaged) == 3.0, "t = 6 is the only multiple of 3 among 4, 5, 6"
    spy.take()
    opt1.avg_every = 0
    with pytest.raises(ValueError, match="avg_every=0"):
        opt1.step()
    assert spy.take() == [] and float(opt1.device_step) == 6.0
