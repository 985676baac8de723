"""GPU suite of the two opt-in arguments of DataParallelStep.capture_packed: partial_batches (a short last batch served by the captured
graphs: ghost utterances on the host, n_valid as device data) and grad_accum (micro-steps inside the graph: hriemo_grad_begin in
place of the memset, the optimizer held by hriemo_optim_finalize_ctl).  Shapes: those of test_gpu_step_packed.py (d128: B = 5,
T_a = 70, T_t = 40).  A captured step is compared with an eager one at the tolerance test_step_packed_against_the_eager_padded_step
applies between the two: loss 1e-5 * max(1, |ref|), flat gradients (every parameter gradient is a view of that buffer) 1e-5
relative L2; parameters after an update likewise 1e-5 relative L2."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

D, NE, NB, TA, TT = 128, 4, 5, 70, 40
LENGTHS = [([70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),
           ([12, 70, 5, 40, 9], [8, 40, 3, 20, 7])]


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    keep = (_ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.gemm_mode(), _ops.precision())
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    yield hri_emo_amd
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_ingest(False)
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = keep[:3]
    hri_emo_amd.set_gemm_mode(keep[3])
    hri_emo_amd.set_precision(keep[4])


_CACHE = {}


def _batches():
    """[(rows_a, rows_t, la, lt, y)] for LENGTHS: computed once, never changed"""
    if "b" not in _CACHE:
        g = torch.Generator().manual_seed(11)
        out = []
        for la, lt in LENGTHS:
            ra, rt = torch.randn(sum(la), D, generator=g).cuda(), torch.randn(sum(lt), D, generator=g).cuda()
            y = (torch.rand(NB, NE, generator=g) < 0.3).float().cuda()
            out.append((ra, rt, list(la), list(lt), y))
        _CACHE["b"] = out
    return _CACHE["b"]


def _head(batch, n):
    """the first n utterances of a ragged batch"""
    ra, rt, la, lt, y = batch
    return ra[:sum(la[:n])], rt[:sum(lt[:n])], la[:n], lt[:n], y[:n]


def _model(H, p=0.0):
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=p).cuda().train()


def _dp(m, loss_fn=None):
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    dp = DataParallelStep(m, loss_fn or fusion_step_loss, overlap=False)
    dp.set_global_batch(NB)
    return dp


def _close(loss, flat, ref_loss, ref_flat, what):
    rel = float((flat - ref_flat).norm() / ref_flat.norm())
    print(f"{what}: loss {float(loss):.7f} vs {float(ref_loss):.7f}, relative L2 {rel:.2e}")
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss))), (what, float(loss), float(ref_loss))
    assert rel <= 1e-5, (what, rel)


class Spy:
    def __init__(self, monkeypatch):
        from hri_emo_amd import _lib
        self.names, real = [], _lib.call

        def spy(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", spy)


# ----------------------------------------------------------------------------- 4. a short batch, end to end
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_short_batch_against_the_eager_step_on_its_own_utterances(H, precision):
    """(a) the first 3 utterances through the graph captured for 5 (two ghosts) against the eager forward_packed step on those 3
    (use_graph(False) of a step captured without the option: code that exists without this feature); (d) n = 1 runs, finite"""
    H.set_precision(precision)
    m0 = _model(H)
    full, short = _batches()[0], _head(_batches()[0], 3)
    ref = _dp(copy.deepcopy(m0))
    ref.capture_packed(*full, pad_to=(TA, TT))
    ref.use_graph(False)
    ref_loss = ref.step_packed(*short).clone()
    ref_flat = ref.buckets.flat.clone()
    dp = _dp(copy.deepcopy(m0))
    dp.capture_packed(*full, pad_to=(TA, TT), partial_batches=True)
    loss = dp.step_packed(*short)
    torch.cuda.synchronize()
    front = dp._pb.front
    assert front.ctl.dev.tolist() == [3, 1, 1, 0] and front.lens.dev.tolist() == [[70, 33, 32, 1, 1], [40, 1, 32, 1, 1]]
    _close(loss, dp.buckets.flat, ref_loss, ref_flat, f"{precision} n = 3")
    worst = max(float((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30)) for p, q in zip(dp.model.parameters(), ref.model.parameters()))
    print(f"{precision}: worst relative L2 of a single parameter's gradient {worst:.2e}")
    assert worst <= 1e-5, "every parameter gradient on its own, not only the flat buffer as a whole"
    one = _head(full, 1)
    ref_loss = ref.step_packed(*one).clone()
    ref_flat = ref.buckets.flat.clone()
    loss = dp.step_packed(*one)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dp.buckets.flat).all()) and bool(torch.isfinite(loss)), "n = 1"
    _close(loss, dp.buckets.flat, ref_loss, ref_flat, f"{precision} n = 1")
    ref.release_graph()
    dp.release_graph()


def test_short_batch_sees_no_stale_static_state(H):
    """(b) the short step gives the same bits after a full batch, after another short batch, and with NaN planted in the static target
    rows behind it"""
    m0 = _model(H)
    full0, full1 = _batches()
    short = _head(full0, 3)
    dp = _dp(copy.deepcopy(m0))
    dp.capture_packed(*full0, pad_to=(TA, TT), partial_batches=True)
    runs = []
    for prelude, poison in ((full1, False), (_head(full1, 2), False), (_head(full1, 4), True)):
        dp.step_packed(*prelude)
        if poison:
            dp._static[4][3:] = float("nan")
        loss = dp.step_packed(*short)
        torch.cuda.synchronize()
        runs.append((loss.clone(), dp.buckets.flat.clone()))
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dp.buckets.flat).all())
    for i in (1, 2):
        assert torch.equal(runs[0][0], runs[i][0]) and torch.equal(runs[0][1], runs[i][1]), i
    dp.release_graph()


def test_full_batch_equals_the_step_captured_without_the_option(H):
    """(c) dropout 0.1, the generator and the seed word alike: loss and flat gradients torch.equal, batch after batch"""
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    m0 = _model(H, 0.1)
    out = []
    for kw in ({}, {"partial_batches": True}, {"partial_batches": False, "grad_accum": 1}):
        dp = _dp(copy.deepcopy(m0))
        torch.manual_seed(5)
        dp.capture_packed(*_batches()[0], pad_to=(TA, TT), **kw)
        _ops.seed_word(torch.device("cuda", 0)).copy_(word)
        res = []
        for b in (_batches()[0], _batches()[1], _batches()[0]):
            loss = dp.step_packed(*b)
            torch.cuda.synchronize()
            res.append((loss.clone(), dp.buckets.flat.clone()))
        out.append(res)
        dp.release_graph()
    for other in out[1:]:
        for i, ((la, ga), (lb, gb)) in enumerate(zip(out[0], other)):
            assert torch.equal(la, lb) and torch.equal(ga, gb), (i, float(la), float(lb), int((ga != gb).sum()))
    assert not torch.equal(out[0][0][1], out[0][2][1]), "dropout is fresh per replay"


def test_short_batch_refusals_leave_the_static_state_untouched(H):
    """(e) n = 0 and n = 6 raise ValueError and write nothing; (f) without the option n = 4 is refused as before; a loss_fn without
    an n_valid keyword is a TypeError at capture"""
    full = _batches()[0]
    ra, rt, la, lt, y = full
    dp = _dp(_model(H))
    with pytest.raises(TypeError, match="n_valid"):
        _dp(_model(H), loss_fn=lambda logits, beta, y: logits.sum()).capture_packed(*full, pad_to=(TA, TT), partial_batches=True)
    dp.capture_packed(*full, pad_to=(TA, TT), partial_batches=True)
    dp.step_packed(*full)
    torch.cuda.synchronize()
    front = dp._pb.front
    state = lambda: [t.clone() for t in (dp._static[0], dp._static[1], dp._static[4], front.lens.dev, front.lens.host, front.ctl.dev,      # noqa: E731
                                         front.ctl.host, dp._pb.cu_a, dp._pb.cu_t, dp._pb.cu_f, dp.buckets.flat) + front.masks]
    before = state()
    bad = {
        "n = 0": (ra[:0], rt[:0], [], [], y[:0]),
        "n = 6": (torch.cat([ra, ra[:la[0]]]), torch.cat([rt, rt[:lt[0]]]), la + la[:1], lt + lt[:1], torch.cat([y, y[:1]])),
        "targets of the full batch with a short one": _head(full, 3)[:4] + (y,),
    }
    for what, args in bad.items():
        with pytest.raises(ValueError):
            dp.step_packed(*args)
        torch.cuda.synchronize()
        for a, b in zip(before, state()):
            assert torch.equal(a, b), what
    dp.release_graph()
    dp = _dp(_model(H))
    dp.capture_packed(*full, pad_to=(TA, TT))
    assert dp._pb.front.ctl is None
    with pytest.raises(ValueError, match="B = 5"):
        dp.step_packed(*_head(full, 4))
    dp.release_graph()


# ----------------------------------------------------------------------------- 5. accumulation, end to end
def _loss_half(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import mosei_step_loss
    return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=2, n_valid=n_valid)


def _loss_whole(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import mosei_step_loss
    return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=1, n_valid=n_valid)


@pytest.mark.parametrize("second_short", [False, True], ids=["two full micro-batches", "the second one short"])
def test_accumulation_in_the_graph_against_step_accumulated(H, monkeypatch, second_short):
    """grad_accum = 2 (the 1/2 scale is exact), optimizer in the graph.  Micro-step 0 moves neither parameters nor moments nor the
    step count nor `skipped`; micro-step 1 is one update.  Parameters against an identical second model run eagerly:
    step_accumulated on the same two ragged batches, then opt.step().  A second group follows and is compared as well."""
    from hri_emo_amd.optim import DeviceAdamW
    m0 = _model(H)
    b0, b1 = _batches()
    micro = [b0, _head(b1, 3) if second_short else b1]
    ref = _dp(copy.deepcopy(m0), _loss_whole)                  # step_accumulated scales by 1 / k itself
    ropt = DeviceAdamW(ref.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    dp = _dp(copy.deepcopy(m0), _loss_half)
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    spy = Spy(monkeypatch)
    dp.capture_packed(*b0, pad_to=(TA, TT), optimizer=opt, grad_accum=2, partial_batches=second_short)
    names = spy.names[:]
    assert names.count("hriemo_grad_begin") == 3 and names.count("hriemo_optim_finalize_ctl") == 1 and "hriemo_optim_finalize" not in names
    assert ("hriemo_fusion_loss_n" in names) == second_short and ("hriemo_fusion_loss" in names) != second_short
    torch.cuda.synchronize()
    for group in range(2):
        before = [t.clone() for t in (opt.flat_p, opt.m, opt.v, opt._state)]
        assert dp.micro_step == 0
        l0 = dp.step_packed(*micro[0]).clone()
        torch.cuda.synchronize()
        assert dp.micro_step == 1
        for a, b, name in zip((opt.flat_p, opt.m, opt.v), before, "pmv"):
            assert torch.equal(a, b), f"micro-step 0 moved {name}"
        assert torch.equal(opt.device_step, before[3][0]) and torch.equal(opt.skipped, before[3][7]) and torch.equal(opt.grad_norm, before[3][6])
        g0 = dp.buckets.flat.clone()
        l1 = dp.step_packed(*micro[1]).clone()
        torch.cuda.synchronize()
        assert dp.micro_step == 0
        assert float(opt.device_step) == float(before[3][0]) + 1.0 and torch.equal(opt.skipped, before[3][7])
        assert not torch.equal(dp.buckets.flat, g0), "micro-step 1 added to the gradients of micro-step 0"
        total = ref.step_accumulated(micro, pad_to=(TA, TT))
        ref_flat = ref.buckets.flat.clone()
        ropt.step()
        torch.cuda.synchronize()
        _close(l0 + l1, dp.buckets.flat, total, ref_flat, f"group {group}: summed loss, accumulated gradients")
        rel = float((opt.flat_p - ropt.flat_p).norm() / ropt.flat_p.norm())
        print(f"group {group}: parameters relative L2 {rel:.2e}")
        assert rel <= 1e-5, (group, rel)
        assert float(opt.device_step) == float(ropt.device_step)
    dp.release_graph()


def test_flush_accumulated_updates_on_what_is_there(H):
    """a group of 2 cut short after one micro-step: flush_accumulated() is one update on the gradients of that micro-step (no rerun:
    the flat buffer keeps its bits), equal to a plain DeviceAdamW.step() of a twin from the same gradients; the next call opens a
    new group (first = 1)"""
    from hri_emo_amd.optim import DeviceAdamW
    m0 = _model(H)
    b0, b1 = _batches()
    dp = _dp(copy.deepcopy(m0), _loss_half)
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    twin = _dp(copy.deepcopy(m0), _loss_half)
    topt = DeviceAdamW(twin.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    dp.capture_packed(*b0, pad_to=(TA, TT), optimizer=opt, grad_accum=2)
    assert dp.flush_accumulated() == 0 and float(opt.device_step) == 0.0
    dp.step_packed(*b1)
    torch.cuda.synchronize()
    g = dp.buckets.flat.clone()
    assert dp.flush_accumulated() == 1 and dp.micro_step == 0
    twin.buckets.flat.copy_(g)
    topt.step()
    torch.cuda.synchronize()
    assert torch.equal(dp.buckets.flat, g) and float(opt.device_step) == 1.0
    assert torch.equal(opt.flat_p, topt.flat_p) and torch.equal(opt.m, topt.m) and torch.equal(opt.v, topt.v)
    dp.step_packed(*b0)
    torch.cuda.synchronize()
    assert dp._pb.front.ctl.dev.tolist() == [NB, 1, 0, 0] and dp.micro_step == 1 and float(opt.device_step) == 1.0
    dp.release_graph()


# ----------------------------------------------------------------------------- the prefetcher stages a short batch
def test_prefetcher_stages_a_short_batch_in_the_buffers_of_the_full_ones(H):
    """full, full, short, full, short at ring depth 2: the short batches meet ring set 0 after a full one and are staged in ITS buffers
    (same base addresses, y and the rows handed out as [:n] views with the loader's values); step_packed fed from the prefetcher
    equals step_packed fed directly"""
    from hri_emo_amd.data import DevicePrefetcher
    b0, b1 = _batches()
    host = [tuple(t.cpu() if isinstance(t, torch.Tensor) else t for t in b) for b in (b0, b1, _head(b0, 3), b1, _head(b1, 2))]
    loader = [(ra, torch.tensor(la), rt, torch.tensor(lt), y) for ra, rt, la, lt, y in host]
    pf = DevicePrefetcher(loader, "cuda", depth=2, convert=lambda b: (b[0], b[1].tolist(), b[2], b[3].tolist(), b[4]),
                          ragged={0: NB * TA, 2: NB * TT})
    dp = _dp(_model(H))
    dp.capture_packed(*b0, pad_to=(TA, TT), partial_batches=True)
    direct = []
    for ra, rt, la, lt, y in host:
        loss = dp.step_packed(ra.cuda(), rt.cuda(), la, lt, y.cuda())
        torch.cuda.synchronize()
        direct.append((loss.clone(), dp.buckets.flat.clone()))
    bases = {}
    for i, (ra, la, rt, lt, y) in enumerate(pf):
        ent = pf._ring[i % 2]
        sig = tuple(t.data_ptr() for t in (ent["host"][0], ent["dev"][0], ent["host"][4], ent["dev"][4]))
        assert bases.setdefault(i % 2, sig) == sig, f"batch {i}: ring set {i % 2} was re-allocated"
        assert ent["dev"][4].shape[0] == NB and y.data_ptr() == ent["dev"][4].data_ptr()
        assert y.shape == loader[i][4].shape and torch.equal(y.cpu(), loader[i][4]) and torch.equal(ra.cpu(), loader[i][0])
        assert la == loader[i][1].tolist() and lt == loader[i][3].tolist()
        loss = dp.step_packed(ra, rt, la, lt, y)
        torch.cuda.synchronize()
        assert torch.equal(loss, direct[i][0]) and torch.equal(dp.buckets.flat, direct[i][1]), i
    dp.release_graph()
