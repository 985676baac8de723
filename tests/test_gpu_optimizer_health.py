"""GPU suite of DeviceAdamW's health log (hri_emo_amd.optim.HealthLog, csrc/health.hip): hriemo_health_sweep and hriemo_health_fold
through the C ABI behind the real sumsq / finalize / update launches on guarded synthetic flat buffers, and the log attached to
DeviceAdamW -- on five synthetic vectors, on the d = 128 model, and recorded inside captured steps.

Layout (the smallest on which the kernels can still go wrong): P = 5 parameters whose slots are 64 elements (a 6-element bias),
chunk, chunk + 64, 3 chunk + 128 and 64 again -- one block with a single vector, a full chunk, a chunk and a 64-element tail, four
chunks, and a last slot -- in two groups with their own lr, betas and eps, the group changing in the middle and back; and P = 1 with
one 64-element slot.  Operands are real-valued with magnitudes spread over five decades.

Bounds.  grad_sq, weight_sq, update_sq: health_reference.record_bound, counted from the kernel's summation tree, against float64
from the kernel's own fp32 buffers and state words; the worst error / bound ratio is printed.  nonfinite, the header, the ring
order: exact.  sqrt(sum grad_sq) against grad_norm: 1e-5 relative, test_gpu_optimizer.py's bound for the norm (two fixed-order
fp32 sums of the same terms).  Everything the log only READS -- p, m, v, state, the gradients, the losses -- bit for bit.

The eager twin of a captured step is the SAME captured forward / backward followed by the eager opt.step() (the pairing
test_gpu_optimizer_groups.py explains: a fully eager forward / backward is another launch list)."""
import copy

import numpy as np
import pytest
import torch

import health_reference as R
from rowops_reference import GuardedVec
from test_gpu_eval_step import NB, PAD, _batches, _loss, _model
from test_gpu_optimizer_groups import GV, ST, build, golden_batch, small_model, step_loss, two_groups, VEC

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
HYPER = torch.tensor([[1e-3, 0.90, 0.999, 1e-8, 1e-2, 5.0, 0.0, 0.0],
                      [3e-4, 0.80, 0.990, 1e-6, 0.0, 5.0, 0.0, 0.0]], dtype=torch.float32)


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


def chunk():
    from hri_emo_amd.optim import HEALTH_CHUNK
    return HEALTH_CHUNK


def layout(name):
    c = chunk()
    if name == "one slot":
        return [6], [0], 1
    numels = [6, c, c + 64, 3 * c + 128, 64]
    return (numels, [0, 0, 0, 0, 0], 1) if name == "one group" else (numels, [0, 0, 1, 1, 0], 2)


def spread(n, gen, lo, hi):
    """real values whose magnitudes cover the decades 10^lo .. 10^hi"""
    return torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * (hi - lo) + lo)


def bits(t):
    return t.contiguous().view(torch.int32)


class World:
    """the flat buffers of a step between guards, the tables, and the launches of one step through the C ABI"""

    def __init__(self, name, capacity=4, every=1, seed=0):
        from hri_emo_amd.optim import health_chunks
        self.numels, self.groups_of, self.G = layout(name)
        self.P, self.capacity, self.every = len(self.numels), capacity, every
        self.slots, self.n = R.slots_of(self.numels)
        self.gen = torch.Generator().manual_seed(1000 + seed + self.n)
        self.live = torch.zeros(self.n, dtype=torch.bool)
        for (s, _), k in zip(self.slots, self.numels):
            self.live[s:s + k] = True
        self.rows = health_chunks([(s, length, g) for (s, length), g in zip(self.slots, self.groups_of)], chunk())
        self.C = len(self.rows)
        p0 = spread(self.n, self.gen, -3, 1) * self.live
        self.p, self.m, self.v = GV(p0), GV(torch.zeros(self.n)), GV(torch.zeros(self.n))
        self.g = GuardedVec(self.n, torch.float32, device="cuda")
        self.sumsq = GuardedVec(1024, torch.float32, device="cuda")
        self.hyper, self.state = GV(HYPER[:self.G].reshape(-1)), GV(torch.zeros(self.G * 8))
        seg, seg_group = [0], []
        for (s, _), g in zip(self.slots, self.groups_of):
            if seg_group and seg_group[-1] == g:
                continue
            if seg_group:
                seg.append(s)
            seg_group.append(g)
        seg.append(self.n)
        self.seg, self.seg_group = GV(torch.tensor(seg, dtype=torch.int64)), GV(torch.tensor(seg_group, dtype=torch.int32))
        self.chunks = GV(torch.tensor(self.rows, dtype=torch.int64).reshape(-1))
        self.hpart = GV(torch.full((self.C * 4,), -3.0))
        img = torch.full((4 + capacity * (4 + 4 * self.P),), FILL, dtype=torch.int32)
        img[:4] = 0
        self.log = GV(img)
        self.ctl = GV(torch.tensor([5, 0, 0, 0], dtype=torch.int32))
        self.bufs = [self.p, self.m, self.v, self.g, self.sumsq, self.hyper, self.state, self.seg, self.seg_group, self.chunks, self.hpart,
                     self.log, self.ctl]
        self.new_grad()

    def new_grad(self, scale=1.0):
        self.g.view.copy_(spread(self.n, self.gen, -4, 0) * self.live * scale)

    def update(self, gs=None, fi=None, ctl=None):
        from hri_emo_amd import _lib
        P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        c = None if ctl is None else ctl.ptr
        _lib.call("hriemo_sumsq_f32", self.g.ptr, self.n, self.sumsq.ptr, 1024, ST())
        _lib.call("hriemo_optim_finalize_groups", self.sumsq.ptr, 1024, self.hyper.ptr, self.G, P(gs), P(fi), self.state.ptr, c, ST())
        _lib.call("hriemo_adamw_flat_groups", self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.n, self.seg.ptr, self.seg_group.ptr,
                  self.seg_group.n, self.hyper.ptr, self.state.ptr, self.G, ST())

    def health(self, gs=None, ctl=None, chunks=None, **kw):
        from hri_emo_amd import _lib
        P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        c = None if ctl is None else ctl.ptr
        a = dict(chunks=(chunks or self.chunks).ptr, C=self.C, every=self.every, capacity=self.capacity, log=self.log.ptr, partial=self.hpart.ptr)
        a.update(kw)
        _lib.call("hriemo_health_sweep", self.g.ptr, self.p.ptr, self.m.ptr, self.v.ptr, self.n, a["chunks"], a["C"], self.hyper.ptr,
                  self.state.ptr, self.G, c, a["every"], a["partial"], ST())
        _lib.call("hriemo_health_fold", a["partial"], a["chunks"], a["C"], self.P, self.state.ptr, c, P(gs), a["every"], a["capacity"],
                  a["log"], ST())

    def step(self, gs=None, fi=None, ctl=None):
        self.update(gs, fi, ctl)
        self.health(gs, ctl)
        torch.cuda.synchronize()
        self.intact()

    def intact(self, extra=()):
        for i, b in enumerate(list(self.bufs) + list(extra)):
            b.assert_intact(f"buffer {i}")

    def arrays(self):
        from hri_emo_amd.optim import decode_health
        return decode_health(self.log.view.cpu().numpy(), self.P, self.capacity)

    def snapshot(self):
        return [b.view.clone() for b in (self.p, self.m, self.v, self.state, self.log, self.hpart)]

    def restore(self, snap):
        for b, t in zip((self.p, self.m, self.v, self.state, self.log, self.hpart), snap):
            b.view.copy_(t)

    def check(self, a, idx, kind, gs=1.0, what=""):
        """record idx of the decoded arrays against float64 from the buffers as they are now, within the counted bound"""
        st = self.state.view.cpu()
        assert int(a["kind"][idx]) == kind and float(a["step"][idx]) == float(st[0]), (what, a["kind"], a["step"], st)
        assert np.float32(a["grad_norm"][idx]).view(np.int32) == int(bits(st[6:7])[0]), (what, "grad_norm is the word the finalize wrote")
        R.assert_no_underflow(self.g.view, self.p.view)
        ref = R.record_ref64(self.g.view, self.p.view, self.m.view, self.v.view, self.slots, self.groups_of,
                             R.scalars_from_state(self.state.view, self.hyper.view, self.G), grad_scale=gs, real=kind == 0)
        bound = R.record_bound(ref, self.slots, chunk())
        assert a["nonfinite"][idx].tolist() == ref["nonfinite"].tolist(), (what, a["nonfinite"][idx], ref["nonfinite"])
        for key in ("grad_sq", "weight_sq", "update_sq"):
            got = torch.from_numpy(a[key][idx].astype(np.float64))
            assert bool(torch.isfinite(got).all()), (what, key, got)
            err = (got - ref[key]).abs()
            ratio = float((err / bound[key].clamp_min(1e-300)).max())
            rel = float((err / ref[key].clamp_min(1e-300)).max())
            print(f"{what} {key}: max rel err {rel:.3e}, max err / bound {ratio:.3f}")
            assert bool((err <= bound[key]).all()), (what, key, err, bound[key])
            if kind == 0 or key == "grad_sq":
                assert bool((ref[key] > 0).all()), (what, key, "every parameter carries a figure")
        return ref


# ---------------------------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("name", ["one group", "two groups", "one slot"])
def test_real_update_records_are_within_the_counted_bound(H, name):
    """two real updates: each record within the bound of float64, nonfinite all zeros, the header the words of state[], the norm
    of the per-parameter sums the grad_norm; slots of the ring not reached yet keep every bit"""
    w = World(name, capacity=4, every=1)
    Rw = 4 + 4 * w.P
    for t in (1, 2):
        w.new_grad(3.0 if t == 2 else 1.0)
        w.step()
        a = w.arrays()
        assert a["n_recorded"] == t and a["step"].tolist() == [float(s) for s in range(1, t + 1)]
        ref = w.check(a, t - 1, 0, what=f"{name} t = {t}")
        assert int(ref["nonfinite"].sum()) == 0 and not a["nonfinite"].any()
        norm = float(np.sqrt(a["grad_sq"][t - 1].astype(np.float64).sum()))
        assert abs(norm - float(a["grad_norm"][t - 1])) <= 1e-5 * norm, (norm, a["grad_norm"])
        rest = w.log.view[4 + t * Rw:].cpu()
        assert bool((rest == FILL).all()), "slots the ring has not reached are untouched"
    assert float(w.state.view[7]) == 0.0


def test_a_skipped_step_names_the_parameters_with_non_finite_gradients(H):
    """NaN at the first and the last element of one parameter, +Inf in the middle of the four-chunk parameter, -Inf at the last
    element of another one's first chunk: the step is skipped, the record has kind 1, exact counts, finite sums within bound for
    EVERY parameter (a non-finite element is left out of grad_sq), p, m and v keep every bit"""
    w = World("two groups", capacity=4)
    w.step()
    c = chunk()
    s = [start for start, _ in w.slots]
    w.new_grad()
    w.g.view[s[1]] = float("nan")
    w.g.view[s[1] + c - 1] = float("nan")
    w.g.view[s[3] + c + c // 2] = float("inf")
    w.g.view[s[2] + c - 1] = float("-inf")
    before = w.snapshot()
    w.step()
    st = w.state.view.cpu()
    assert float(st[0]) == 1.0 and float(st[1]) == 1.0 and float(st[7]) == 1.0 and not np.isfinite(float(st[6]))
    for b, old, what in zip((w.p, w.m, w.v), before, "pmv"):
        assert torch.equal(bits(b.view), bits(old)), f"the skipped step moved {what}"
    a = w.arrays()
    assert a["n_recorded"] == 2 and a["kind"].tolist() == [0, 1] and a["step"].tolist() == [1.0, 1.0]
    assert a["nonfinite"][1].tolist() == [0, 2, 1, 1, 0]
    w.check(a, 1, 1, what="skip on a non-finite norm")
    assert not a["weight_sq"][1].any() and not a["update_sq"][1].any()


def test_found_inf_alone_and_a_grad_scale(H):
    """found_inf = 1 over finite gradients scaled by 1024: kind 2, no non-finite element, the UNSCALED grad_sq; then a real update
    with the same scale: kind 0, the unscaled grad_sq again"""
    w = World("two groups", capacity=4)
    scale_t, inf_t = torch.tensor([1024.0], device="cuda"), torch.ones(1, device="cuda")
    w.new_grad(1024.0)
    w.step(scale_t, inf_t)
    a = w.arrays()
    assert a["kind"].tolist() == [2] and a["step"].tolist() == [0.0] and not a["nonfinite"].any() and np.isfinite(a["grad_norm"][0])
    assert float(w.state.view[7]) == 1.0
    ref = w.check(a, 0, 2, gs=1024.0, what="found_inf alone")
    unscaled = R.record_ref64(w.g.view / 1024.0, None, None, None, w.slots, w.groups_of, None, real=False)
    assert bool(((ref["grad_sq"] - unscaled["grad_sq"]).abs() <= 1e-12 * unscaled["grad_sq"]).all())
    inf_t.zero_()
    w.step(scale_t, inf_t)
    a = w.arrays()
    assert a["kind"].tolist() == [2, 0] and a["step"].tolist() == [0.0, 1.0]
    w.check(a, 1, 0, gs=1024.0, what="real update under a grad scale")
    norm = float(np.sqrt(a["grad_sq"][1].astype(np.float64).sum()))
    assert abs(norm - float(a["grad_norm"][1])) <= 1e-5 * norm


def test_sampling_and_the_ring(H):
    """every = 2, capacity = 3: six real updates with a skipped step behind the third.  Records: t = 2, the skip (always recorded),
    t = 4, t = 6 -- the ring ends holding the last three in order; a step that does not record moves no bit of log or partials"""
    w = World("two groups", capacity=3, every=2)
    Rw = 4 + 4 * w.P
    scale_t, inf_t = torch.tensor([1.0], device="cuda"), torch.zeros(1, device="cuda")
    want = []                                                  # (step, kind) of the records so far
    events = ["u", "u", "u", "skip", "u", "u", "u"]
    t = 0
    for ev in events:
        w.new_grad()
        inf_t.fill_(1.0 if ev == "skip" else 0.0)
        before = (w.log.raw.clone(), w.hpart.raw.clone())
        w.step(scale_t, inf_t)
        t += ev == "u"
        records = ev == "skip" or t % 2 == 0
        if records:
            want.append((float(t), 2 if ev == "skip" else 0))
        else:
            assert torch.equal(w.log.raw, before[0]) and torch.equal(w.hpart.raw, before[1]), (ev, t, "a non-recording step wrote")
        a = w.arrays()
        assert a["n_recorded"] == len(want) and list(zip(a["step"].tolist(), a["kind"].tolist())) == want[-3:], (ev, t, a["step"], a["kind"])
        if len(want) < 3:
            assert bool((w.log.view[4 + len(want) * Rw:].cpu() == FILL).all()), "slots the ring has not reached are untouched"
        if records:
            w.check(a, len(a["kind"]) - 1, want[-1][1], what=f"event {ev} t = {t}")
    assert want == [(2.0, 0), (3.0, 2), (4.0, 0), (6.0, 0)] and float(w.state.view[0]) == 6.0 and float(w.state.view[7]) == 1.0
    assert int(w.log.view[0]) == 4 and bits(w.log.view[4:5]).item() == np.float32(6.0).view(np.int32), "record 3 wrapped into slot 0"


def test_held_micro_steps_record_nothing_and_the_same_step_gives_the_same_bits(H):
    """ctl.last = 0: not a word of the log or the partials moves (compared byte for byte, guards included); ctl.last = 1: the
    record is written.  The same step run twice from the same state: torch.equal records and partials."""
    w = World("two groups", capacity=2)
    w.step()
    w.new_grad()
    before = (w.log.raw.clone(), w.hpart.raw.clone(), w.snapshot())
    w.ctl.view[2] = 0
    w.step(ctl=w.ctl)
    assert torch.equal(w.log.raw, before[0]) and torch.equal(w.hpart.raw, before[1]), "a held micro-step moved the log"
    assert float(w.state.view[1]) == 1.0 and float(w.state.view[0]) == 1.0
    for b, old in zip((w.p, w.m, w.v), before[2]):
        assert torch.equal(bits(b.view), bits(old))
    w.ctl.view[2] = 1
    snap = w.snapshot()
    w.step(ctl=w.ctl)
    a = w.arrays()
    assert a["n_recorded"] == 2 and a["step"].tolist() == [1.0, 2.0] and a["kind"].tolist() == [0, 0]
    w.check(a, 1, 0, what="last = 1")
    first = (w.log.view.clone(), w.hpart.view.clone(), w.p.view.clone())
    w.restore(snap)
    w.hpart.view.fill_(-3.0)
    w.step(ctl=w.ctl)
    assert torch.equal(w.log.view, first[0]) and torch.equal(bits(w.hpart.view), bits(first[1])) and torch.equal(bits(w.p.view), bits(first[2]))


def test_refusals_and_a_table_that_breaks_its_contract(H):
    """overlapping buffers, capacity = 0 and every = 0 raise through hriemo_last_error and launch nothing; a chunk table with
    parameter indices, starts, lengths and groups out of range is clamped: the record is written, every guard stays intact"""
    w = World("two groups", capacity=2)
    w.step()
    before = (w.log.raw.clone(), w.hpart.raw.clone())
    for kw, msg in ((dict(log=w.hpart.ptr), "health_fold.*log overlaps"), (dict(partial=w.g.ptr + 64), "health_sweep.*partial overlaps"),
                    (dict(capacity=0), "health_fold.*capacity=0"), (dict(every=0), "health_sweep.*every=0"), (dict(C=0), "health_sweep.*C=0")):
        with pytest.raises(RuntimeError, match=msg):
            w.health(**kw)
    with pytest.raises(RuntimeError, match="health_fold.*every=0"):
        from hri_emo_amd import _lib
        _lib.call("hriemo_health_fold", w.hpart.ptr, w.chunks.ptr, w.C, w.P, w.state.ptr, None, None, 0, w.capacity, w.log.ptr, ST())
    torch.cuda.synchronize()
    assert torch.equal(w.log.raw, before[0]), "a refused fold launches nothing"
    rows = torch.tensor(w.rows, dtype=torch.int64)
    rows[0, 2], rows[1, 2], rows[-1, 2] = 99, -5, 1 << 40       # parameter indices outside [0, P)
    rows[2, 0], rows[2, 1], rows[2, 3] = w.n + 4096, 1 << 40, 99   # a start behind the buffer, a length beyond it, a group outside [0, G)
    rows[3, 0], rows[3, 1], rows[3, 3] = -4096, 6, -2           # a negative start, a length that is no multiple of 4
    broken = GV(rows.reshape(-1))
    w.health(chunks=broken)
    torch.cuda.synchronize()
    w.intact(extra=[broken])
    a = w.arrays()
    assert a["n_recorded"] == 2 and a["kind"].tolist() == [0, 0], "the record is written, into the ring"
    assert bool(np.isfinite(a["grad_sq"][1]).all())


# ------------------------------------------------------------------------------------------------- 2. attached to DeviceAdamW
def test_blame_and_ratios_through_the_optimizer(H):
    """five vectors of the kernel layout in two groups behind a real GradBuckets + DeviceAdamW(health=...): a real update (ratios
    against float64), the poisoned step (blame names exactly the three parameters with their counts, p / m / v keep every bit), a
    found_inf-only skip (blame == [])"""
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW, HealthLog
    numels, _, _ = layout("two groups")
    gen = torch.Generator().manual_seed(77)
    params = [torch.nn.Parameter(spread(k, gen, -3, 1).cuda()) for k in numels]
    buckets = GradBuckets(params, overlap=False)
    order = sorted(range(5), key=lambda j: buckets._offsets[id(params[j])])
    groups = [{"params": [params[j] for j in order[:2]]}, {"params": [params[j] for j in order[2:]], **VEC}]
    opt = DeviceAdamW(buckets, param_groups=groups, lr=1e-3, weight_decay=1e-2, max_norm=5.0, health=HealthLog(capacity=4))
    log = opt.health
    assert log.n_params == 5 and log.names == [f"param{i}" for i in range(5)]
    log.name_parameters((f"layer{j}.weight", q) for j, q in enumerate(params))
    names = [f"layer{j}.weight" for j in order]
    assert log.names == names
    live = torch.zeros_like(buckets.flat, dtype=torch.bool)
    for q in params:
        live[buckets._offsets[id(q)]:buckets._offsets[id(q)] + q.numel()] = True
    buckets.flat.copy_(spread(buckets.flat.numel(), gen, -4, 0).cuda() * live)
    opt.step()
    torch.cuda.synchronize()
    assert log.blame() is None
    slots = [(buckets._offsets[id(params[j])], R.pad64(params[j].numel())) for j in order]
    ref = R.record_ref64(buckets.flat, opt.flat_p, opt.m, opt.v, slots, [0, 0, 1, 1, 1], R.scalars_from_state(opt._state, opt._hyper, 2))
    bound = R.record_bound(ref, slots, chunk())
    ratios = log.ratios()
    assert list(ratios) == names
    for i, name in enumerate(names):
        exact = float((ref["update_sq"][i] / ref["weight_sq"][i]).sqrt())
        rel = 0.5 * float(bound["update_sq"][i] / ref["update_sq"][i] + bound["weight_sq"][i] / ref["weight_sq"][i]) * 1.001 + 2.0 ** -23
        assert abs(ratios[name] - exact) <= rel * exact, (name, ratios[name], exact)
    # the poisoned step
    sizes = sorted(range(5), key=lambda i: slots[i][1])          # by slot length: 64, 64, chunk, chunk + 64, 3 chunk + 128
    one, edge, multi = sizes[2], sizes[3], sizes[4]
    c = chunk()
    buckets.flat.copy_(spread(buckets.flat.numel(), gen, -4, 0).cuda() * live)
    buckets.flat[slots[one][0]] = float("nan")
    buckets.flat[slots[one][0] + c - 1] = float("nan")
    buckets.flat[slots[multi][0] + c + c // 2] = float("inf")
    buckets.flat[slots[edge][0] + c - 1] = float("-inf")
    before = [t.clone() for t in (opt.flat_p, opt.m, opt.v)]
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.skipped) == 1.0 and float(opt.device_step) == 1.0
    want = {one: 2, multi: 1, edge: 1}
    assert log.blame() == [(names[i], want[i]) for i in sorted(want)]
    for old, new, what in zip(before, (opt.flat_p, opt.m, opt.v), "pmv"):
        assert torch.equal(bits(old), bits(new)), what
    a = log.arrays()
    assert a["kind"].tolist() == [0, 1] and a["n_recorded"] == 2 and bool(np.isfinite(a["grad_sq"]).all())
    with pytest.raises(ValueError, match="skipped step"):
        log.ratios()
    # found_inf alone, through GradScaler's hand-over
    buckets.flat.copy_(spread(buckets.flat.numel(), gen, -4, 0).cuda() * live * 1024.0)
    opt.grad_scale, opt.found_inf = torch.tensor(1024.0, device="cuda"), torch.tensor(1.0, device="cuda")
    opt.step()
    torch.cuda.synchronize()
    a = log.arrays()
    assert a["kind"].tolist() == [0, 1, 2] and float(opt.skipped) == 2.0 and log.blame() == []
    unscaled = R.record_ref64(buckets.flat / 1024.0, None, None, None, slots, [0] * 5, None, real=False)
    b = R.record_bound(unscaled, slots, chunk())
    assert bool(((torch.from_numpy(a["grad_sq"][2].astype(np.float64)) - unscaled["grad_sq"]).abs() <= b["grad_sq"]).all())
    log.reset()
    assert log.arrays()["n_recorded"] == 0 and log.blame() is None
    assert set(opt.state_dict()) == {"state", "param_groups"}


def test_a_log_attached_changes_no_bit_of_the_training(H):
    """two DeviceAdamW on identical copies of the d = 128 model, five steps, one with health=HealthLog(every=1): parameters,
    moments and state[] torch.equal after every step; the log holds five real-update records named after the model"""
    from hri_emo_amd.optim import HealthLog
    batch = golden_batch()
    m0 = small_model(H)
    ma, mb = copy.deepcopy(m0), copy.deepcopy(m0)
    _, plain = build(H, ma, param_groups=two_groups(ma.named_parameters(), **VEC), lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    _, logged = build(H, mb, param_groups=two_groups(mb.named_parameters(), **VEC), lr=1e-3, weight_decay=1e-2, max_norm=5.0,
                      health=HealthLog(every=1))
    logged.health.name_parameters(mb.named_parameters())
    for step in range(5):
        for m, opt in ((ma, plain), (mb, logged)):
            opt.zero_grad()
            step_loss(m, batch, 40.0 if step == 3 else 1.0).backward()
            opt.step()
        torch.cuda.synchronize()
        assert torch.equal(bits(plain.buckets.flat), bits(logged.buckets.flat)), (step, "gradients")
        for x, y, what in ((plain.flat_p, logged.flat_p, "p"), (plain.m, logged.m, "m"), (plain.v, logged.v, "v"), (plain._state, logged._state, "state")):
            assert torch.equal(bits(x), bits(y)), (step, what)
    a = logged.health.arrays()
    assert a["n_recorded"] == 5 and a["step"].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0] and not a["kind"].any() and not a["nonfinite"].any()
    assert sorted(a["names"]) == sorted(n for n, _ in mb.named_parameters())
    norms = np.sqrt(a["grad_sq"].astype(np.float64).sum(axis=1))
    assert bool((np.abs(norms - a["grad_norm"]) <= 1e-5 * norms).all()), (norms, a["grad_norm"])
    assert float(a["grad_norm"][4]) == float(logged.grad_norm)
    r = logged.health.ratios()
    assert list(r) == a["names"]
    for j, name in enumerate(a["names"]):
        if a["weight_sq"][4][j] > 0:
            assert r[name] == float(np.sqrt(np.float64(a["update_sq"][4][j]) / np.float64(a["weight_sq"][4][j]))), name


def _loss_half(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import mosei_step_loss
    return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=2, n_valid=n_valid)


@pytest.mark.parametrize("variant", ["plain", "grad_accum 2", "ema"])
def test_the_log_inside_the_captured_packed_step(H, variant):
    """capture_packed(..., optimizer=opt) with a log attached, four step_packed replays.  The records equal, bit for bit, those of
    the eager twin (the same captured forward / backward, then the eager opt.step()); losses and parameters equal a captured run
    WITHOUT the log.  grad_accum = 2: two records for four replays, none from the held micro-steps.  averaging="ema": the average
    is untouched by the log too."""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW, HealthLog
    accum = 2 if variant == "grad_accum 2" else 1
    kw = dict(averaging="ema", avg_decay=0.5) if variant == "ema" else {}
    cap = dict(grad_accum=2, partial_batches=True) if accum == 2 else {}
    b0 = _batches()[0]
    m0 = _model(H)
    runs = {}
    for arm in ("in graph", "eager twin", "no log"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, _loss_half if accum == 2 else _loss(), overlap=False)
        dp.set_global_batch(NB)
        health = None if arm == "no log" else HealthLog(capacity=8, every=1)
        opt = DeviceAdamW(dp.buckets, param_groups=two_groups(m.named_parameters(), **VEC), lr=1e-3, weight_decay=1e-2, max_norm=5.0,
                          health=health, **kw)
        dp.capture_packed(*b0, pad_to=PAD, optimizer=None if arm == "eager twin" else opt, **cap)
        torch.cuda.synchronize()
        if health is not None:
            assert int(health._buf.abs().sum()) == 0, "capture() records nothing"
        losses = []
        for i in range(4):
            losses.append(float(dp.step_packed(*b0)))
            if arm == "eager twin" and (i + 1) % accum == 0:
                opt.step()
            torch.cuda.synchronize()
            if health is not None:
                assert int(health._buf[0]) == (i + 1) // accum, (arm, i, "held micro-steps record nothing")
        assert float(opt.device_step) == 4 // accum and float(opt.skipped) == 0.0
        runs[arm] = (losses, opt.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt._state.clone(),
                     opt.avg.clone() if variant == "ema" else None, None if health is None else health._buf.clone(),
                     None if health is None else health.arrays())
        dp.release_graph()
    a, e, n = runs["in graph"], runs["eager twin"], runs["no log"]
    assert torch.equal(a[6], e[6]), "the records of the captured step are those of the eager twin, bit for bit"
    arr = a[7]
    assert arr["n_recorded"] == 4 // accum and arr["step"].tolist() == [float(t) for t in range(1, 4 // accum + 1)] and not arr["kind"].any()
    norms = np.sqrt(arr["grad_sq"].astype(np.float64).sum(axis=1))
    assert bool((np.abs(norms - arr["grad_norm"]) <= 1e-5 * norms).all()) and bool((arr["weight_sq"].sum(axis=1) > 0).all())
    assert a[0] == n[0], (a[0], n[0])
    for x, y, what in zip(a[1:6], n[1:6], ("p", "m", "v", "state", "avg")):
        assert (x is None and y is None) or torch.equal(bits(x), bits(y)), what
