"""GPU suite of the device-state optimizer (hri_emo_amd.optim.DeviceAdamW, csrc/optim.hip): the kernels through the C ABI, the
torch Optimizer surface the reference's MOSEI trainer uses (LambdaLR, GradScaler, NaN / Inf skipping, state dicts;
scripts/fusion/train_mosei_fusion_seq_level_decoder.py:367-402, 564-584) and the optimizer recorded inside the captured step.

Where a torch twin is used it receives COPIES OF THE SAME GRADIENTS, so only the optimizer arithmetic is compared.  Parameter
bound: |p - p_twin| <= 2e-6 * max(1, max|p_twin|) per parameter -- per step at most half an ulp of p (6e-8 |p|) plus lr times a
few ulp, over the at most 6 steps used here <= 4e-7 |p|.  Gradient norm: 1e-5 relative (fp32 sums of ~1e5 squares in two
different orders)."""
import copy
import math

import pytest
import torch

from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu
GUARD = 64                                      # guard words on both sides of a buffer (256 B: the interior stays 16-B aligned)


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)


def cu(t):
    return None if t is None else t.cuda()


def small_model(H, closed_form=True, seed=7):
    torch.manual_seed(seed)
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.0)
    if closed_form:
        O.closed_form_init_(m)
    return m.cuda().train()


def golden_batch():
    g = load_golden("cfg1_train_p0")
    return tuple(cu(g[k]) for k in ("h_a", "h_t", "mask_a", "mask_t", "y"))


def make_twin(m):
    return {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}


def copy_grads(m, twin):
    for n, p in m.named_parameters():
        twin[n].grad = p.grad.detach().clone()


def assert_params_close(m, twin, what):
    for n, p in m.named_parameters():
        ref = twin[n].detach()
        err = (p.detach() - ref).abs().max().item()
        assert err <= 2e-6 * max(1.0, ref.abs().max().item()), (what, n, err)


def step_loss(m, batch, scale=1.0):
    logits, beta, _ = m(*batch[:4])
    loss = O.train_step_loss(logits, beta, batch[4])
    return loss * scale if scale != 1.0 else loss


def warmup_cosine(warm=2, total=6):
    """linear warm-up, then a cosine to zero (the MOSEI trainer's LambdaLR, :367-380)"""
    def f(step):
        if step < warm:
            return (step + 1) / (warm + 1)
        return 0.5 * (1.0 + math.cos(math.pi * (step - warm) / max(1, total - warm)))
    return f


# ---------------------------------------------------------------------------------------------------------------- 1. kernels
class Guarded:
    """n fp32 words between two runs of GUARD words of 0xFF bytes"""

    def __init__(self, n, fill=None):
        self.raw = torch.full(((n + 2 * GUARD) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.raw.view(torch.float32)[GUARD:GUARD + n]
        if fill is not None:
            self.t.copy_(fill)

    def guards_intact(self):
        g = GUARD * 4
        return bool((self.raw[:g] == 0xFF).all()) and bool((self.raw[-g:] == 0xFF).all())


def _adamw_ref64(p, g, m, v, hyper, step, grad_scale):
    """float64 evaluation of clip_grad_norm_ + torch.optim.AdamW on the fp32 hyper-parameters the kernels read"""
    lr, b1, b2, eps, wd, max_norm = (float(x) for x in hyper[:6])
    norm = math.sqrt(float((g * g).sum())) / grad_scale
    coef = (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0) / grad_scale
    gg = g * coef
    p = p * (1.0 - lr * wd)
    m = m + (gg - m) * (1.0 - b1)
    v = v * b2 + gg * gg * (1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v, norm, coef


@pytest.mark.parametrize("n", [4, 4 * 255, 4 * 256 * 4096 + 4])
def test_kernels_through_the_c_abi(H, n):
    """hriemo_sumsq_f32 -> hriemo_optim_finalize -> hriemo_adamw_flat_dev on guarded buffers: one vector, just under one block,
    one vector past a full sweep of the capped grid.  Two updates (the second with a GradScaler-style scale and bias correction
    of step 2) against float64, then a step with found_inf = 1 that must leave everything but `skipped` bit-identical."""
    from hri_emo_amd import _lib
    P = lambda t: None if t is None else t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(n)
    nblocks = 1024
    p0, m0, v0 = torch.randn(n, generator=gen), torch.zeros(n), torch.zeros(n)
    hyper_host = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 5.0, 0.0, 0.0], dtype=torch.float32)
    p, m, v, g = Guarded(n, p0), Guarded(n, m0), Guarded(n, v0), Guarded(n)
    partial, hyper, state = Guarded(nblocks), Guarded(8, hyper_host), Guarded(8, torch.zeros(8))
    scale_t, inf_t = torch.tensor([8.0], device="cuda"), torch.zeros(1, device="cuda")
    bufs = (p, m, v, g, partial, hyper, state)
    rp, rm, rv = p0.double(), m0.double(), v0.double()

    def launch(gs, fi):
        _lib.call("hriemo_sumsq_f32", P(g.t), n, P(partial.t), nblocks, st)
        _lib.call("hriemo_optim_finalize", P(partial.t), nblocks, P(hyper.t), P(gs), P(fi), P(state.t), st)
        _lib.call("hriemo_adamw_flat_dev", P(p.t), P(g.t), P(m.t), P(v.t), n, P(hyper.t), P(state.t), st)
        torch.cuda.synchronize()

    for step, gs in ((1, None), (2, scale_t)):
        # step 1: a norm under max_norm for n = 4 and far above it for the large sizes; step 2: scaled gradients
        gh = torch.randn(n, generator=gen) * (1.5 if step == 1 else 8.0 * 3.0)
        g.t.copy_(gh)
        launch(gs, None if gs is None else inf_t)
        rp, rm, rv, norm, coef = _adamw_ref64(rp, gh.double(), rm, rv, hyper_host.double(), step, 1.0 if gs is None else 8.0)
        s = state.t.cpu()
        assert s[0].item() == step and s[1].item() == 0.0 and s[7].item() == 0.0, s
        assert abs(s[6].item() - norm) <= 1e-5 * norm and abs(s[2].item() - coef) <= 1e-5 * coef, (s, norm, coef)
        for got, ref, what in ((p.t, rp, "p"), (m.t, rm, "m"), (v.t, rv, "v")):
            err = (got.cpu().double() - ref).abs()
            assert bool((err <= 2e-6 * ref.abs().clamp_min(1.0)).all()), (what, step, err.max().item())
        assert all(b.guards_intact() for b in bufs), step
    # a skipped step: found_inf = 1
    before = [b.t.clone() for b in (p, m, v)]
    inf_t.fill_(1.0)
    launch(scale_t, inf_t)
    s = state.t.cpu()
    assert s[0].item() == 2.0 and s[1].item() == 1.0 and s[7].item() == 1.0, s
    for b, old in zip((p, m, v), before):
        assert torch.equal(b.t, old)
    assert all(b.guards_intact() for b in bufs)


# ------------------------------------------------------------------------------------------------------ 2. scheduler and clip
def test_lambda_lr_schedule_and_clip_follow_torch(H):
    """torch.optim.lr_scheduler.LambdaLR drives DeviceAdamW like any torch optimizer (warm-up + cosine); 6 steps, one of them
    with a x40 loss so that it clips, against clip_grad_norm_(5.0) + torch.optim.AdamW + the same scheduler."""
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(list(twin.values()), lr=1e-4, weight_decay=1e-2)
    buckets = GradBuckets(m.parameters(), overlap=False)
    opt = DeviceAdamW(buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)
    assert isinstance(opt, torch.optim.Optimizer)
    assert len(opt.param_groups) == 1 and all(a is b for a, b in zip(opt.param_groups[0]["params"], buckets.params))
    with pytest.raises(RuntimeError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(4, device="cuda"))]})
    sched = torch.optim.lr_scheduler.LambdaLR(opt, warmup_cosine())
    ref_sched = torch.optim.lr_scheduler.LambdaLR(ref_opt, warmup_cosine())
    lrs = []
    for step in range(6):
        opt.zero_grad(set_to_none=True)                      # the trainer's call: the flat views must survive it
        assert all(p.grad is not None and p.grad.data_ptr() == buckets.flat.data_ptr() + buckets._offsets[id(p)] * 4
                   for p in buckets.params)
        step_loss(m, batch, 40.0 if step == 3 else 1.0).backward()
        copy_grads(m, twin)
        tn_ref = torch.nn.utils.clip_grad_norm_(list(twin.values()), 5.0)
        ref_opt.step(); ref_sched.step()
        lrs.append(opt.param_groups[0]["lr"])
        assert opt.step() is None
        sched.step()
        assert abs(float(opt.grad_norm) - float(tn_ref)) <= 1e-5 * float(tn_ref), (step, float(opt.grad_norm), float(tn_ref))
        if step == 3:
            assert float(tn_ref) > 5.0, "the scaled step is meant to exercise clipping"
        assert_params_close(m, twin, step)
    assert len(set(lrs)) == 6 and lrs[2] == pytest.approx(1e-4), lrs      # the schedule really moved lr between the steps
    assert float(opt.device_step) == 6.0 and float(opt.skipped) == 0.0
    with torch.no_grad():                                    # the model still runs on the re-homed parameter storage
        m.eval()(*batch[:4])


# --------------------------------------------------------------------------------------------------------------- 3. GradScaler
@pytest.mark.parametrize("stage", ["unscaled_torch_clip", "fused_unscale_and_clip"])
def test_grad_scaler_both_stages(H, stage):
    """(a) scale -> backward -> unscale_ -> torch clip -> scaler.step -> update with max_norm=None (grad_scale is None after
    unscale_); (b) no unscale_: scaler.step hands grad_scale over and the unscale is fused into the clip coefficient (the scale is
    a power of two: exact).  Twin: the reference loop (:387-402) on torch.optim.AdamW with its own GradScaler."""
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(list(twin.values()), lr=1e-4, weight_decay=1e-2)
    buckets = GradBuckets(m.parameters(), overlap=False)
    fused = stage == "fused_unscale_and_clip"
    opt = DeviceAdamW(buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0 if fused else None)
    scaler, ref_scaler = torch.amp.GradScaler("cuda"), torch.amp.GradScaler("cuda")
    ref_scaler.scale(torch.zeros((), device="cuda"))          # the twin's scaler never scales a loss itself: create its scale
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        scaler.scale(step_loss(m, batch, 40.0 if step == 1 else 1.0)).backward()
        copy_grads(m, twin)
        ref_scaler.unscale_(ref_opt)
        tn_ref = torch.nn.utils.clip_grad_norm_(list(twin.values()), 5.0)
        ref_scaler.step(ref_opt); ref_scaler.update()
        if not fused:
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        scaler.step(opt); scaler.update()
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
        if step == 1:
            assert float(tn_ref) > 5.0, "the scaled step is meant to exercise clipping"
        if fused:                                             # the norm the optimizer reports is the unscaled, pre-clip one
            assert abs(float(opt.grad_norm) - float(tn_ref)) <= 1e-5 * float(tn_ref), (step, float(opt.grad_norm), float(tn_ref))
        assert_params_close(m, twin, (stage, step))
    assert float(opt.device_step) == 3.0 and float(opt.skipped) == 0.0 and scaler.get_scale() == ref_scaler.get_scale()


# --------------------------------------------------------------------------------------------------------------------- 4. skip
def test_inf_under_grad_scaler_skips_the_step_and_halves_the_scale(H):
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    batch = golden_batch()
    m = small_model(H)
    buckets = GradBuckets(m.parameters(), overlap=False)
    opt = DeviceAdamW(buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    scaler = torch.amp.GradScaler("cuda")
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        scaler.scale(step_loss(m, batch)).backward()
        if step == 1:
            buckets.params[3].grad.view(-1)[1] = float("inf")
            before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt.device_step)]
            scale_before = scaler.get_scale()
        scaler.step(opt); scaler.update()
    assert float(before[3]) == 1.0 and bool(before[1].abs().max() > 0)           # the first step was a real one
    for old, new in zip(before, (opt.flat_p, opt.m, opt.v, opt.device_step)):
        assert torch.equal(old, new)
    assert float(opt.skipped) == 1.0
    assert scaler.get_scale() == 0.5 * scale_before


def test_nan_without_scaler_is_skipped_and_costs_no_step(H):
    """the reference loop's NaN guard (:564-584) without the host read: a NaN gradient skips the update on the device; the next
    finite step equals a twin that never saw the bad one (bias correction of step 1, not 2)"""
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(list(twin.values()), lr=1e-3, weight_decay=1e-2)
    buckets = GradBuckets(m.parameters(), overlap=False)
    opt = DeviceAdamW(buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    opt.zero_grad()
    step_loss(m, batch).backward()
    buckets.params[0].grad.view(-1)[5] = float("nan")
    before = [t.clone() for t in (opt.flat_p, opt.m, opt.v)]
    opt.step()
    assert float(opt.skipped) == 1.0 and float(opt.device_step) == 0.0 and math.isnan(float(opt.grad_norm))
    for old, new in zip(before, (opt.flat_p, opt.m, opt.v)):
        assert torch.equal(old, new)
    opt.zero_grad()
    step_loss(m, batch).backward()
    copy_grads(m, twin)
    torch.nn.utils.clip_grad_norm_(list(twin.values()), 5.0)
    ref_opt.step()
    opt.step()
    assert float(opt.skipped) == 1.0 and float(opt.device_step) == 1.0
    assert_params_close(m, twin, "first finite step after a skipped one")


# --------------------------------------------------------------------------------------------------------------- 5. state dict
def test_state_dict_round_trips_with_torch_adamw(H):
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(list(twin.values()), lr=1e-3, weight_decay=1e-2)
    buckets = GradBuckets(m.parameters(), overlap=False)
    opt = DeviceAdamW(buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)

    def two_steps(tag):
        for step in range(2):
            opt.zero_grad()
            step_loss(m, batch).backward()
            copy_grads(m, twin)
            torch.nn.utils.clip_grad_norm_(list(twin.values()), 5.0)
            ref_opt.step(); opt.step()
            assert_params_close(m, twin, (tag, step))

    two_steps("before")
    sd, ref_sd = copy.deepcopy(opt.state_dict()), copy.deepcopy(ref_opt.state_dict())
    # keys and shapes of torch.optim.AdamW(model.parameters())'s state dict
    assert list(sd["state"].keys()) == list(ref_sd["state"].keys()) and len(sd["param_groups"]) == 1
    assert sd["param_groups"][0]["params"] == ref_sd["param_groups"][0]["params"]
    assert set(ref_sd["param_groups"][0]) <= set(sd["param_groups"][0])
    for k, ent in ref_sd["state"].items():
        assert set(sd["state"][k]) == set(ent) == {"step", "exp_avg", "exp_avg_sq"}
        assert all(sd["state"][k][f].shape == ent[f].shape for f in ent) and float(sd["state"][k]["step"]) == 2.0
    # both ways, each with an lr only the loaded group carries
    sd["param_groups"][0]["lr"] = ref_sd["param_groups"][0]["lr"] = 5e-4
    views = [opt.state[p]["exp_avg"].data_ptr() for p in buckets.params]
    opt.m.zero_(); opt.v.zero_()                               # whatever comes back comes from the loaded dict
    opt.load_state_dict(ref_sd)
    ref_opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 5e-4 and ref_opt.param_groups[0]["lr"] == 5e-4
    assert views == [opt.state[p]["exp_avg"].data_ptr() for p in buckets.params], "the moments must stay views into the flat buffers"
    assert float(opt.device_step) == 2.0
    for k, p in enumerate(buckets.params):
        assert torch.equal(opt.state[p]["exp_avg"], ref_sd["state"][k]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], ref_sd["state"][k]["exp_avg_sq"])
    two_steps("after")
    assert float(opt.device_step) == 4.0
    # one flat update has one step count
    bad = copy.deepcopy(ref_opt.state_dict())
    bad["state"][1]["step"] = bad["state"][1]["step"] + 3
    with pytest.raises(ValueError, match="step"):
        opt.load_state_dict(bad)


# ------------------------------------------------------------------------------------------------------------ 6. in-graph step
def test_optimizer_inside_the_captured_step(H):
    """capture(optimizer=opt): dp.step() alone is the trainer step -- forward, loss, backward and the update in one replay, lr
    moved by a scheduler between replays.  Against a copy that replays forward / backward and steps the same optimizer eagerly
    (the same kernels: bit-identical), and against the fully eager loop (bf16 trajectories, 2e-3 as the packed loop's test)."""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import fusion_step_loss
    batch = golden_batch()
    m0 = small_model(H, closed_form=False, seed=11)
    runs = {}
    for mode in ("in_graph", "graph_plus_eager", "eager"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, warmup_cosine(warm=2, total=4))
        if mode != "eager":
            before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt.device_step)]
            dp.capture(*batch, optimizer=opt if mode == "in_graph" else None)
            torch.cuda.synchronize()
            for old, new in zip(before, (opt.flat_p, opt.m, opt.v, opt.device_step)):
                assert torch.equal(old, new), "capture() must not move parameters, moments or the step count"
        losses = []
        for step in range(4):
            losses.append(float(dp.step(*batch)))
            if mode != "in_graph":
                opt.step()
            sched.step()
        assert float(opt.device_step) == 4.0 and float(opt.skipped) == 0.0, mode
        with torch.no_grad():
            logits = m.eval()(*batch[:4])[0].clone()
        runs[mode] = (losses, opt.flat_p.clone(), logits)
        dp.release_graph()
    a, b, c = runs["in_graph"], runs["graph_plus_eager"], runs["eager"]
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (a[0], b[0])
    assert abs(a[0][3] - a[0][0]) > 1e-4, ("the updates must be visible in the loss", a[0])
    for x, y in zip(a[0], c[0]):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), (a[0], c[0])


# ------------------------------------------------------------------------------------------------------------------- 7. packed
def test_packed_training_loop_with_the_optimizer_in_every_bucket_graph(H):
    """the loop of test_gpu_varlen.py::test_packed_training_loop_end_to_end with capture(optimizer=opt): every bucket graph --
    those captured on first sight inside step() too -- applies exactly one update per step"""
    from hri_emo_amd import data
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import fusion_step_loss
    g = torch.Generator().manual_seed(21)
    d, ne, B, Ta, Tt = 128, 4, 4, 48, 24
    samples = []
    for _ in range(6 * B):
        la, lt = int(torch.randint(5, Ta + 1, (1,), generator=g)), int(torch.randint(3, Tt + 1, (1,), generator=g))
        samples.append((torch.randn(la, d, generator=g), torch.zeros(la, dtype=torch.bool), torch.randn(lt, d, generator=g),
                        torch.zeros(lt, dtype=torch.bool), (torch.rand(ne, generator=g) < 0.3).float()))
    loader = [data.collate_seq_batch(samples[i:i + B], pad_to=(Ta, Tt)) for i in range(0, len(samples), B)]
    torch.manual_seed(3)
    m0 = H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=0.0).cuda().train()
    traj = []
    for packed in (False, True):
        H.set_varlen(packed)
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
        batches = data.DevicePrefetcher(loader, "cuda", convert=lambda t: (t[0], t[2], t[1], t[3], t[4]), mask_slots=(2, 3))
        losses = []
        for i, (h_a, h_t, m_a, m_t, y, lens) in enumerate(batches):
            if packed and i == 0:
                dp.capture(h_a, h_t, m_a, m_t, y, lengths=lens, optimizer=opt)
                assert float(opt.device_step) == 0.0
            if packed:
                losses.append(float(dp.step(h_a, h_t, m_a, m_t, y, lengths=lens)))
            else:
                losses.append(float(dp.step(h_a, h_t, m_a, m_t, y)))
                opt.step()
            assert float(opt.device_step) == i + 1.0, (packed, i)
        if packed:
            assert len(dp._pb.graphs) >= 2          # the six batches do not all fall into one bucket
            dp.release_graph()
        assert float(opt.device_step) == len(loader) and float(opt.skipped) == 0.0
        traj.append(losses)
    for a, b in zip(*traj):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), traj      # bf16 path, weights diverge slowly over the six updates
    assert traj[0][-1] != traj[0][0]


# ---------------------------------------------------------------------------------------------------- 8. exchange after update
def test_capture_with_optimizer_needs_captured_collectives_at_world_2(H):
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW, FusedClipAdamW
    from hri_emo_amd.train import fusion_step_loss
    batch = golden_batch()
    m = small_model(H)
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    opt = DeviceAdamW(dp.buckets)
    dp.world = 2
    with pytest.raises(RuntimeError, match="collectives=True"):
        dp.capture(*batch, optimizer=opt)
    dp.world = 1
    with pytest.raises(TypeError):                      # an optimizer whose scalars are host values cannot be recorded
        dp.capture(*batch, optimizer=FusedClipAdamW(dp.buckets))
    assert not dp.captured
