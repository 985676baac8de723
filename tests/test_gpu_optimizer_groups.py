"""GPU suite of DeviceAdamW's parameter groups (hri_emo_amd.optim, csrc/optim.hip): hriemo_optim_finalize_groups and
hriemo_adamw_flat_groups through the C ABI on guarded buffers, and the optimizer built with param_groups= on the d = 128 model
(cfg1_train_p0) -- against torch.optim.AdamW with the same groups, under LambdaLR with one lambda per group, under GradScaler,
through state dicts in both directions, and recorded inside captured steps.

Bounds are those test_gpu_optimizer.py derives in its header: |x - ref| <= 2e-6 * max(1, |ref|) for p, m and v (per element against
float64 in the kernel tests, per parameter against the torch twin in the optimizer tests), 1e-5 relative for the gradient norm and
the clip coefficient.  Where a torch twin is used it receives COPIES OF THE SAME GRADIENTS.

Bit-identity claims and why they hold: the grouped update kernel and the single-group one call ONE inline function per 16-byte
vector, so a group's elements must equal, bit for bit, what hriemo_optim_finalize + hriemo_adamw_flat_dev give under that group's
hyper row; and an optimizer recorded in a captured step launches the kernels its eager step() launches, so "captured step with the
update inside" equals "the same captured forward / backward followed by the eager opt.step()" bit for bit (the pairing
test_gpu_optimizer.py::test_optimizer_inside_the_captured_step asserts for one group; a fully eager forward / backward is a
different launch list and agrees to 1e-5 .. 2e-3 only, as the step tests record)."""
import copy
import math

import pytest
import torch

from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)
from rowops_reference import GuardedVec

pytestmark = pytest.mark.gpu


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)


def ST():
    return torch.cuda.current_stream().cuda_stream


def GV(x):
    return GuardedVec.of(x.contiguous(), device="cuda")


# ---------------------------------------------------------------------------------------------------------------- 1. kernels
# G = 3 with distinct lr, betas, eps and weight decay; max_norm is global (row 0 is the one the kernels read)
HYPER = torch.tensor([[1e-3, 0.90, 0.999, 1e-8, 1e-2, 5.0, 0.0, 0.0],
                      [3e-4, 0.80, 0.990, 1e-6, 0.0, 5.0, 0.0, 0.0],
                      [2e-3, 0.95, 0.980, 1e-7, 5e-2, 5.0, 0.0, 0.0]], dtype=torch.float32)
N_SWEEP = 4 * 256 * 4096                        # elements one sweep of the capped grid covers
CASES = {
    "one vector": (4, [0, 4], [2]),
    "a group owning non-adjacent segments": (28, [0, 4, 12, 28], [1, 0, 1]),
    "one block's edge": (3072, [0, 1020, 1024, 1028, 3072], [0, 1, 2, 0]),
    "a thread's second sweep lands in another group": (N_SWEEP + 8, [0, N_SWEEP, N_SWEEP + 4, N_SWEEP + 8], [0, 1, 2]),
}
SENTINEL = -7.0                                 # words of state rows g >= 1 that no kernel may write


def _ref64(p, g, m, v, cols, step, grad_scale, max_norm):
    """float64 clip_grad_norm_ + torch.optim.AdamW with per-ELEMENT lr, b1, b2, eps, wd (cols: float64 [5, n]); ONE norm over all of g"""
    lr, b1, b2, eps, wd = cols
    norm = math.sqrt(float((g * g).sum())) / grad_scale
    coef = (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0) / grad_scale
    gg = g * coef
    p = p * (1.0 - lr * wd)
    m = m + (gg - m) * (1.0 - b1)
    v = v * b2 + gg * gg * (1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / bc2.sqrt() + eps)
    return p, m, v, norm, coef


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_grouped_kernels_through_the_c_abi(H, case):
    """hriemo_sumsq_f32 -> hriemo_optim_finalize_groups -> hriemo_adamw_flat_groups.  Three updates (the second with a grad scale of
    8, the third through the step-control block with last = 1), each against float64 AND, per group, bit for bit against the
    single-group entries run with that group's hyper row on a clone of the whole buffers; a HOLD (ctl.last = 0) that touches
    nothing but state.skip; a found_inf step that leaves p, m, v bit-identical; the launcher's limits; every guard intact."""
    from hri_emo_amd import _lib
    n, seg_h, sg_h = CASES[case]
    S, G, nblocks = len(sg_h), 3, 1024
    gen = torch.Generator().manual_seed(n)
    elem_group = torch.repeat_interleave(torch.tensor(sg_h), torch.diff(torch.tensor(seg_h)))
    assert elem_group.numel() == n
    cols = HYPER.double()[elem_group][:, :5].t().contiguous()
    masks = [(elem_group == k).cuda() for k in range(G)]
    p0 = torch.randn(n, generator=gen)
    p, m, v, g = GV(p0), GV(torch.zeros(n)), GV(torch.zeros(n)), GuardedVec(n, torch.float32, device="cuda")
    partial, hyper = GuardedVec(nblocks, torch.float32, device="cuda"), GV(HYPER.reshape(-1))
    state0 = torch.full((G * 8,), SENTINEL)
    state0[:8] = 0.0
    state = GV(state0)
    seg, seg_group = GV(torch.tensor(seg_h, dtype=torch.int64)), GV(torch.tensor(sg_h, dtype=torch.int32))
    ctl = GV(torch.tensor([5, 0, 0, 0], dtype=torch.int32))
    hyper_rows = [GV(HYPER[k]) for k in range(G)]
    scale_t, inf_t = torch.tensor([8.0], device="cuda"), torch.zeros(1, device="cuda")
    bufs = [p, m, v, g, partial, hyper, state, seg, seg_group, ctl] + hyper_rows
    P = lambda t: None if t is None else t.data_ptr()

    def grouped(gs, fi, c=None, S_=S, G_=G):
        _lib.call("hriemo_sumsq_f32", g.ptr, n, partial.ptr, nblocks, ST())
        _lib.call("hriemo_optim_finalize_groups", partial.ptr, nblocks, hyper.ptr, G_, P(gs), P(fi), state.ptr, None if c is None else c.ptr, ST())
        _lib.call("hriemo_adamw_flat_groups", p.ptr, g.ptr, m.ptr, v.ptr, n, seg.ptr, seg_group.ptr, S_, hyper.ptr, state.ptr, G_, ST())
        torch.cuda.synchronize()

    def single(k, pre, gs, fi, c=None):
        """the EXISTING entries with hyper row k on clones of the whole buffers -> (p, m, v, state[8])"""
        pc, mc, vc, sc = (GV(t) for t in pre)
        _lib.call("hriemo_sumsq_f32", g.ptr, n, partial.ptr, nblocks, ST())
        if c is None:
            _lib.call("hriemo_optim_finalize", partial.ptr, nblocks, hyper_rows[k].ptr, P(gs), P(fi), sc.ptr, ST())
        else:
            _lib.call("hriemo_optim_finalize_ctl", partial.ptr, nblocks, hyper_rows[k].ptr, P(gs), P(fi), sc.ptr, c.ptr, ST())
        _lib.call("hriemo_adamw_flat_dev", pc.ptr, g.ptr, mc.ptr, vc.ptr, n, hyper_rows[k].ptr, sc.ptr, ST())
        torch.cuda.synchronize()
        for b in (pc, mc, vc, sc):
            b.assert_intact("clone")
        return pc.view, mc.view, vc.view, sc.view

    def intact():
        for i, b in enumerate(bufs):
            b.assert_intact(f"buffer {i}")

    rp, rm, rv = p0.double(), torch.zeros(n).double(), torch.zeros(n).double()
    for step, gs, c in ((1, None, None), (2, scale_t, None), (3, None, ctl)):
        # step 1: a norm under max_norm for n = 4 and far above it for the large sizes; step 2: scaled gradients
        gh = torch.randn(n, generator=gen) * (1.5 if step != 2 else 8.0 * 3.0)
        g.view.copy_(gh)
        if c is not None:
            # HOLD first: last = 0 touches nothing but state.skip
            before = [b.view.clone() for b in (p, m, v, state)]
            grouped(gs, None, c)
            for b, old, what in zip((p, m, v), before, "pmv"):
                assert torch.equal(b.view, old), f"the held launch moved {what}"
            st = state.view.clone()
            assert float(st[1]) == 1.0 and float(before[3][1]) == 0.0, "the hold sets state.skip"
            st[1] = before[3][1]
            assert torch.equal(st.view(torch.int32), before[3].view(torch.int32)), "every other word of every row stays"
            intact()
            ctl.view[2] = 1
            state.view[1] = 0.0                                # the singles below start from the state in front of the hold
        pre = [b.view.clone() for b in (p, m, v)] + [state.view[:8].clone()]
        grouped(gs, None if gs is None else inf_t, c)
        rp, rm, rv, norm, coef = _ref64(rp, gh.double(), rm, rv, cols, step, 1.0 if gs is None else 8.0, 5.0)
        s = state.view.cpu()
        print(f"{case} step {step}: norm {s[6].item():.6e} ref {norm:.6e}  coef {s[2].item():.6e} ref {coef:.6e}")
        assert s[0].item() == step and s[1].item() == 0.0 and s[7].item() == 0.0, s
        assert abs(s[6].item() - norm) <= 1e-5 * norm and abs(s[2].item() - coef) <= 1e-5 * coef, (s, norm, coef)
        for got, ref, what in ((p.view, rp, "p"), (m.view, rm, "m"), (v.view, rv, "v")):
            err = (got.cpu().double() - ref).abs()
            print(f"   {what}: max |err| {err.max().item():.3e}")
            assert bool((err <= 2e-6 * ref.abs().clamp_min(1.0)).all()), (what, step, err.max().item())
        for k in range(1, G):
            row = s[8 * k:8 * k + 8]
            assert all(row[w].item() == SENTINEL for w in (0, 1, 2, 6, 7)), ("rows g >= 1: words 3, 4, 5 and nothing else", k, row)
        # the same inputs through the single-group kernels, one run per group
        for k in range(G):
            sp, sm, sv, ss = single(k, pre, gs, None if gs is None else inf_t, c)
            for got, one, what in ((p.view, sp, "p"), (m.view, sm, "m"), (v.view, sv, "v")):
                assert torch.equal(got[masks[k]], one[masks[k]]), (what, "group", k, "step", step)
            if k == 0:
                assert torch.equal(state.view[:8].view(torch.int32), ss.view(torch.int32)), "row 0 is the single-group state word for word"
            else:
                assert torch.equal(state.view[8 * k + 3:8 * k + 6], ss[3:6]), ("step_size, 1/sqrt(bc2), decay of group", k)
        intact()
    # a skipped step: found_inf = 1
    before = [b.view.clone() for b in (p, m, v, state)]
    inf_t.fill_(1.0)
    grouped(scale_t, inf_t)
    s = state.view.cpu()
    assert s[0].item() == 3.0 and s[1].item() == 1.0 and s[7].item() == 1.0, s
    for b, old in zip((p, m, v), before):
        assert torch.equal(b.view, old)
    assert torch.equal(state.view[8:], before[3][8:]), "a skipped step writes no word of the rows g >= 1"
    intact()
    # the limits: refused in front of the launch
    inf_t.fill_(0.0)
    state.view[1] = 0.0                                        # not skipped: a launch that did run would move p
    before = [b.view.clone() for b in (p, m, v, state)]
    with pytest.raises(RuntimeError, match=r"S=2049 segments"):
        _lib.call("hriemo_adamw_flat_groups", p.ptr, g.ptr, m.ptr, v.ptr, n, seg.ptr, seg_group.ptr, 2049, hyper.ptr, state.ptr, G, ST())
    with pytest.raises(RuntimeError, match=r"G=17 groups"):
        _lib.call("hriemo_adamw_flat_groups", p.ptr, g.ptr, m.ptr, v.ptr, n, seg.ptr, seg_group.ptr, S, hyper.ptr, state.ptr, 17, ST())
    with pytest.raises(RuntimeError, match=r"G=17 groups"):
        _lib.call("hriemo_optim_finalize_groups", partial.ptr, nblocks, hyper.ptr, 17, None, None, state.ptr, None, ST())
    torch.cuda.synchronize()
    for b, old in zip((p, m, v, state), before):
        assert torch.equal(b.view, old), "a refused call launches nothing"
    intact()


# ------------------------------------------------------------------------------------------------------- the d = 128 model
def cu(t):
    return None if t is None else t.cuda()


def small_model(H, closed_form=True, seed=7):
    torch.manual_seed(seed)
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.0)
    if closed_form:
        O.closed_form_init_(m)
    return m.cuda().train()


_GOLDEN = {}


def golden_batch():
    if "b" not in _GOLDEN:
        g = load_golden("cfg1_train_p0")
        _GOLDEN["b"] = tuple(cu(g[k]) for k in ("h_a", "h_t", "mask_a", "mask_t", "y"))
    return _GOLDEN["b"]


def step_loss(m, batch, scale=1.0):
    logits, beta, _ = m(*batch[:4])
    loss = O.train_step_loss(logits, beta, batch[4])
    return loss * scale if scale != 1.0 else loss


def warmup_cosine(warm=2, total=6):
    def f(step):
        if step < warm:
            return (step + 1) / (warm + 1)
        return 0.5 * (1.0 + math.cos(math.pi * (step - warm) / max(1, total - warm)))
    return f


def inverse_decay(step):
    return 1.0 / (1.0 + 0.5 * step)


VEC = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6)        # what the no-decay group sets besides weight_decay = 0


def two_groups(named, **vec):
    """decay_groups' split (matrices decay, vectors do not) with the second group's own settings"""
    from hri_emo_amd.optim import decay_groups
    groups = decay_groups(named, 1e-2)
    assert len(groups) == 2
    groups[1].update(vec)
    return groups


def make_twin(m):
    return {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}


def copy_grads(m, twin):
    for n, p in m.named_parameters():
        twin[n].grad = p.grad.detach().clone()


def assert_close_to_twin(m, twin, opt, ref_opt, what, moments=True):
    for n, p in m.named_parameters():
        pairs = [("p", p.detach(), twin[n].detach())]
        if moments:
            pairs += [(k, opt.state[p][k], ref_opt.state[twin[n]][k]) for k in ("exp_avg", "exp_avg_sq")]
        for kind, got, ref in pairs:
            err = (got - ref).abs().max().item()
            assert err <= 2e-6 * max(1.0, ref.abs().max().item()), (what, n, kind, err)


def build(H, m, **kw):
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    buckets = GradBuckets(m.parameters(), overlap=False)
    return buckets, DeviceAdamW(buckets, **kw)


# ------------------------------------------------------------------------------------------------- 2. against torch.optim.AdamW
def test_two_groups_under_two_lambdas_follow_torch(H):
    """six steps against clip_grad_norm_(5.0) + torch.optim.AdamW with the same two groups and LambdaLR(opt, [f0, f1]); step 3
    carries a x40 loss so that it clips (one norm over both groups)"""
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(two_groups(twin.items(), **VEC), lr=1e-4, weight_decay=1e-2)
    buckets, opt = build(H, m, param_groups=two_groups(m.named_parameters(), **VEC), lr=1e-4, weight_decay=1e-2, max_norm=5.0)
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["weight_decay"] == 0.0 and opt.param_groups[1]["betas"] == (0.8, 0.99)
    assert opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["eps"] == 1e-8, "missing keys take the constructor's values"
    assert sorted(id(p) for g in opt.param_groups for p in g["params"]) == sorted(id(p) for p in buckets.params)
    with pytest.raises(RuntimeError, match="fixed at construction"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(4, device="cuda"))]})
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [warmup_cosine(), inverse_decay])
    ref_sched = torch.optim.lr_scheduler.LambdaLR(ref_opt, [warmup_cosine(), inverse_decay])
    lrs = []
    for step in range(6):
        opt.zero_grad(set_to_none=True)
        step_loss(m, batch, 40.0 if step == 3 else 1.0).backward()
        copy_grads(m, twin)
        tn_ref = torch.nn.utils.clip_grad_norm_(list(twin.values()), 5.0)
        lrs.append(tuple(g["lr"] for g in opt.param_groups))
        assert lrs[-1] == tuple(g["lr"] for g in ref_opt.param_groups)
        ref_opt.step(); ref_sched.step()
        assert opt.step() is None
        sched.step()
        assert abs(float(opt.grad_norm) - float(tn_ref)) <= 1e-5 * float(tn_ref), (step, float(opt.grad_norm), float(tn_ref))
        if step == 3:
            assert float(tn_ref) > 5.0, "the scaled step is meant to exercise clipping"
        assert_close_to_twin(m, twin, opt, ref_opt, step)
    assert len(set(lrs)) == 6 and all(a != b for a, b in lrs), lrs            # both schedules moved, and differently
    assert float(opt.device_step) == 6.0 and float(opt.skipped) == 0.0
    with torch.no_grad():                                    # the model still runs on the re-homed parameter storage
        m.eval()(*batch[:4])


def test_a_group_with_lr_zero_keeps_its_parameters_while_its_moments_move(H):
    """lr = 0, eps > 0, weight decay set: decay = 1 - 0 * wd = 1 and step_size = 0, so p * 1 - 0 * m / (...) is p bit for bit, while
    m and v follow the gradients; the other group trains"""
    batch = golden_batch()
    m = small_model(H)
    named = list(m.named_parameters())
    frozen = [p for n, p in named if n.startswith("emotion_decoder")]
    rest = [p for n, p in named if not n.startswith("emotion_decoder")]
    assert frozen and rest
    before = [p.detach().clone() for p in frozen]
    moving = [p.detach().clone() for p in rest]
    buckets, opt = build(H, m, param_groups=[{"params": rest}, {"params": frozen, "lr": 0.0, "eps": 1e-8, "weight_decay": 0.1}],
                         lr=1e-3, max_norm=5.0)
    for step in range(2):
        opt.zero_grad()
        step_loss(m, batch).backward()
        opt.step()
    assert float(opt.device_step) == 2.0
    for p, old in zip(frozen, before):
        assert torch.equal(p.detach(), old)
        assert float(opt.state[p]["exp_avg_sq"].abs().max()) > 0 or float(p.grad.abs().max()) == 0
    assert any(float(opt.state[p]["exp_avg"].abs().max()) > 0 for p in frozen), "the frozen group's moments move"
    assert any(not torch.equal(p.detach(), old) for p, old in zip(rest, moving)), "the other group trains"


def test_groups_built_from_generators_train_the_model(H):
    """{"params": <generator>}: the groups keep their parameters (read once), every p.data is re-homed and one step moves the
    MODEL's parameters, exactly as the same groups given as lists do"""
    batch = golden_batch()
    runs = []
    for as_generators in (False, True):
        m = small_model(H)
        named = list(m.named_parameters())
        dec = [p for n, p in named if n.startswith("emotion_decoder")]
        rest = [p for n, p in named if not n.startswith("emotion_decoder")]
        wrap = (lambda ps: (p for p in ps)) if as_generators else list
        buckets, opt = build(H, m, param_groups=[{"params": wrap(rest)}, {"params": wrap(dec), "lr": 3e-5}], lr=1e-3, max_norm=5.0)
        assert [len(g["params"]) for g in opt.param_groups] == [len(rest), len(dec)] and len(opt.state) == len(named)
        start = [p.detach().clone() for _, p in named]
        opt.zero_grad()
        step_loss(m, batch).backward()
        opt.step()
        assert all(not torch.equal(p.detach(), old) for (_, p), old in zip(named, start) if float(p.grad.abs().max()) > 0)
        runs.append(torch.cat([p.detach().reshape(-1) for _, p in named]))
    assert torch.equal(*runs)


def test_one_explicit_group_equals_the_default_optimizer_bit_for_bit(H):
    """param_groups=[all parameters] runs the grouped launches with G = 1, S = 1: p, m, v and all 8 words of state equal those of
    the default-constructed optimizer (the single-group launches) after three steps, one of them clipped"""
    batch = golden_batch()
    runs = []
    for grouped in (False, True):
        m = small_model(H)
        kw = dict(param_groups=[{"params": list(m.parameters())}]) if grouped else {}
        buckets, opt = build(H, m, lr=1e-3, weight_decay=1e-2, max_norm=5.0, **kw)
        assert opt._state.shape == (8,) and opt._hyper.shape == (8,)
        for step in range(3):
            opt.zero_grad()
            step_loss(m, batch, 40.0 if step == 1 else 1.0).backward()
            opt.step()
        runs.append([t.clone() for t in (opt.flat_p, opt.m, opt.v, opt._state)])
    for a, b, what in zip(*runs, ("p", "m", "v", "state")):
        assert torch.equal(a, b), what


# --------------------------------------------------------------------------------------------------------------- 3. GradScaler
@pytest.mark.parametrize("stage", ["unscaled_torch_clip", "fused_unscale_and_clip"])
def test_grad_scaler_both_stages_with_two_groups(H, stage):
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(two_groups(twin.items(), **VEC), lr=1e-4, weight_decay=1e-2)
    fused = stage == "fused_unscale_and_clip"
    buckets, opt = build(H, m, param_groups=two_groups(m.named_parameters(), **VEC), lr=1e-4, weight_decay=1e-2,
                         max_norm=5.0 if fused else None)
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
        assert_close_to_twin(m, twin, opt, ref_opt, (stage, step))
    assert float(opt.device_step) == 3.0 and float(opt.skipped) == 0.0 and scaler.get_scale() == ref_scaler.get_scale()


# --------------------------------------------------------------------------------------------------------------- 4. state dict
def test_state_dict_round_trips_with_a_two_group_torch_adamw(H):
    batch = golden_batch()
    m = small_model(H)
    twin = make_twin(m)
    ref_opt = torch.optim.AdamW(two_groups(twin.items(), **VEC), lr=1e-3, weight_decay=1e-2)
    buckets, opt = build(H, m, param_groups=two_groups(m.named_parameters(), **VEC), lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    order = [p for g in opt.param_groups for p in g["params"]]           # parameter ids follow group order

    def two_steps(tag):
        for step in range(2):
            opt.zero_grad()
            step_loss(m, batch).backward()
            copy_grads(m, twin)
            torch.nn.utils.clip_grad_norm_(list(twin.values()), 5.0)
            ref_opt.step(); opt.step()
            assert_close_to_twin(m, twin, opt, ref_opt, (tag, step))

    two_steps("before")
    sd, ref_sd = copy.deepcopy(opt.state_dict()), copy.deepcopy(ref_opt.state_dict())
    assert list(sd["state"].keys()) == list(ref_sd["state"].keys()) and len(sd["param_groups"]) == 2
    for a, b in zip(sd["param_groups"], ref_sd["param_groups"]):
        assert a["params"] == b["params"] and set(b) <= set(a)
        assert all(a[k] == b[k] for k in ("lr", "betas", "eps", "weight_decay")), "per-group settings come from the groups"
    for k, ent in ref_sd["state"].items():
        assert set(sd["state"][k]) == set(ent) == {"step", "exp_avg", "exp_avg_sq"}
        assert all(sd["state"][k][f].shape == ent[f].shape for f in ent) and float(sd["state"][k]["step"]) == 2.0
    # both ways, each group with an lr only the loaded dict carries
    for d in (sd, ref_sd):
        d["param_groups"][0]["lr"], d["param_groups"][1]["lr"] = 5e-4, 7e-5
    views = [opt.state[p]["exp_avg"].data_ptr() for p in order]
    opt.m.zero_(); opt.v.zero_()                               # whatever comes back comes from the loaded dict
    opt.load_state_dict(ref_sd)
    ref_opt.load_state_dict(sd)
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 7e-5] == [g["lr"] for g in ref_opt.param_groups]
    assert opt.param_groups[1]["betas"] == (0.8, 0.99) and all(g["max_norm"] == 5.0 for g in opt.param_groups)
    assert views == [opt.state[p]["exp_avg"].data_ptr() for p in order], "the moments must stay views into the flat buffers"
    assert float(opt.device_step) == 2.0
    for k, p in enumerate(order):
        assert torch.equal(opt.state[p]["exp_avg"], ref_sd["state"][k]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], ref_sd["state"][k]["exp_avg_sq"])
    two_steps("after")
    assert float(opt.device_step) == 4.0
    # another grouping is refused: one group over everything, and the two groups cut elsewhere
    flat_twin = torch.optim.AdamW(list(twin.values()), lr=1e-3)
    with pytest.raises(ValueError, match="different grouping"):
        opt.load_state_dict(flat_twin.state_dict())
    params = list(twin.values())
    other = torch.optim.AdamW([{"params": params[:3]}, {"params": params[3:]}], lr=1e-3)
    with pytest.raises(ValueError, match="different grouping"):
        opt.load_state_dict(other.state_dict())
    # and a single-group optimizer refuses the two-group dict
    m1 = small_model(H)
    _, opt1 = build(H, m1)
    with pytest.raises(ValueError, match="different grouping"):
        opt1.load_state_dict(ref_opt.state_dict())


# ------------------------------------------------------------------------------------------------------------ 5. in-graph steps
def test_two_groups_inside_the_captured_step(H):
    """capture(optimizer=opt) with two groups and two lambdas: the replay that holds the update against the same captured forward /
    backward followed by the eager opt.step() -- loss, parameters and both moments torch.equal over four steps -- and, against an
    error both graph arms could share, against the fully eager loop (bf16 trajectories: 2e-3 on the losses, the bound of
    test_gpu_optimizer.py::test_optimizer_inside_the_captured_step)"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import fusion_step_loss
    batch = golden_batch()
    m0 = small_model(H, closed_form=False, seed=11)
    runs = {}
    for mode in ("in_graph", "graph_plus_eager", "eager"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        opt = DeviceAdamW(dp.buckets, param_groups=two_groups(m.named_parameters(), **VEC), lr=1e-3, weight_decay=1e-2, max_norm=5.0)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, [warmup_cosine(warm=2, total=4), inverse_decay])
        if mode != "eager":
            before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt._state)]
            dp.capture(*batch, optimizer=opt if mode == "in_graph" else None)
            torch.cuda.synchronize()
            for old, new in zip(before, (opt.flat_p, opt.m, opt.v, opt._state)):
                assert torch.equal(old, new), "capture() must not move parameters, moments or the state block"
        losses = []
        for step in range(4):
            losses.append(float(dp.step(*batch)))
            if mode != "in_graph":
                opt.step()
            sched.step()
        assert float(opt.device_step) == 4.0 and float(opt.skipped) == 0.0, mode
        runs[mode] = (losses, opt.flat_p.clone(), opt.m.clone(), opt.v.clone())
        dp.release_graph()
    a, b, c = runs["in_graph"], runs["graph_plus_eager"], runs["eager"]
    assert a[0] == b[0], (a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert abs(a[0][3] - a[0][0]) > 1e-4, ("the updates must be visible in the loss", a[0])
    for x, y in zip(a[0], c[0]):
        assert abs(x - y) <= 2e-3 * max(1.0, abs(y)), (a[0], c[0])


def test_two_groups_inside_the_packed_step_with_accumulation_and_a_short_batch(H):
    """capture_packed(grad_accum=2, partial_batches=True, optimizer=opt) with two groups: micro-step 0 is held (nothing of the
    optimizer moves), micro-step 1 -- a SHORT batch -- carries one update.  Against the same captured micro-steps without an
    optimizer in the graph, followed by the eager opt.step(): losses, parameters and both moments torch.equal over two groups of
    micro-steps."""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import mosei_step_loss
    D, NE, NB, TA, TT = 128, 4, 5, 70, 40
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
        dp.set_global_batch(NB)
        opt = DeviceAdamW(dp.buckets, param_groups=two_groups(m.named_parameters(), **VEC), lr=1e-3, weight_decay=1e-2, max_norm=5.0)
        dp.capture_packed(*batches[0], pad_to=(TA, TT), optimizer=opt if mode == "in_graph" else None, grad_accum=2, partial_batches=True)
        torch.cuda.synchronize()
        losses = []
        for group in range(2):
            before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt._state)]
            losses.append(float(dp.step_packed(*batches[0])))
            torch.cuda.synchronize()
            st = opt._state.clone()
            st[1] = before[3][1]
            assert all(torch.equal(a, b) for a, b in zip((opt.flat_p, opt.m, opt.v, st), before)), "micro-step 0 is held"
            losses.append(float(dp.step_packed(*batches[1])))
            if mode != "in_graph":
                opt.step()
            torch.cuda.synchronize()
            assert float(opt.device_step) == group + 1.0 and float(opt.skipped) == 0.0 and dp.micro_step == 0
            assert not torch.equal(opt.flat_p, before[0])
        runs[mode] = (losses, opt.flat_p.clone(), opt.m.clone(), opt.v.clone())
        dp.release_graph()
    a, b = runs["in_graph"], runs["graph_plus_eager"]
    assert a[0] == b[0], (a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------------------ 6. launch lists
class Spy:
    """records the name of every _lib.call"""

    def __init__(self, monkeypatch):
        from hri_emo_amd import _lib
        self.names, real = [], _lib.call

        def spy(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", spy)

    def take(self):
        out, self.names = self.names, []
        return out


def test_launch_lists_of_the_default_and_the_grouped_optimizer(H, monkeypatch):
    """built without param_groups the optimizer records exactly the three existing entries (the _ctl finalize under a step-control
    block); built with them, three launches as well: the sum of squares and the two grouped entries"""
    m = small_model(H)
    buckets, opt = build(H, m)
    ctl = torch.tensor([5, 1, 1, 0], dtype=torch.int32, device="cuda")
    spy = Spy(monkeypatch)
    opt.step()
    assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize", "hriemo_adamw_flat_dev"]
    opt._enqueue(ctl=ctl)
    assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize_ctl", "hriemo_adamw_flat_dev"]
    m2 = small_model(H)
    buckets2, opt2 = build(H, m2, param_groups=two_groups(m2.named_parameters()))
    spy.take()
    opt2.step()
    assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize_groups", "hriemo_adamw_flat_groups"]
    opt2._enqueue(ctl=ctl)
    assert spy.take() == ["hriemo_sumsq_f32", "hriemo_optim_finalize_groups", "hriemo_adamw_flat_groups"]
    torch.cuda.synchronize()
    assert float(opt.device_step) == 2.0 and float(opt2.device_step) == 2.0
