"""GPU suite: FusionClassifier through the captured steps -- DataParallelStep.capture_packed / step_packed (partial batches, gradient
accumulation in the graph), capture_store / step_store, EvalStep with EpochStats(kind="single_label") and PredictionLog, fresh dropout
masks per replay.  B = 4, d = 128, pad_to = (40, 35), the single-label loss (train.fusion_step_loss_single_label).  The recipes are
those of test_gpu_step_packed.py, test_gpu_step_packed_partial.py, test_gpu_store_step.py and test_gpu_eval_step.py.  On the code
before FusionClassifier had a forward_packed entry every test here ends in `TypeError: the model has no forward_packed entry`."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, NC, NB, PAD = 128, 4, 4, (40, 35)
LENGTHS = [([40, 5, 1, 33], [35, 20, 1, 32]),           # sample 1: audio shorter than text -- audio PAD rows are pooled
           ([12, 40, 7, 20], [8, 35, 3, 19]),
           ([40] * NB, [35] * NB)]


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    keep = _ops.POOLED_GATE
    yield hri_emo_amd
    _ops.POOLED_GATE = keep
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)


_CACHE = {}


def _batches():
    """[(padded batch (h_a, h_t, m_a, m_t, y), ragged batch (rows_a, rows_t, la, lt, y))] for LENGTHS: computed once, never changed"""
    if "b" not in _CACHE:
        g = torch.Generator().manual_seed(11)
        out = []
        for la, lt in LENGTHS:
            h_a, h_t = torch.randn(NB, PAD[0], D, generator=g).cuda(), torch.randn(NB, PAD[1], D, generator=g).cuda()
            m_a = (torch.arange(PAD[0])[None] >= torch.tensor(la)[:, None]).cuda()
            m_t = (torch.arange(PAD[1])[None] >= torch.tensor(lt)[:, None]).cuda()
            h_a[m_a], h_t[m_t] = 0.0, 0.0                                     # zero padding, as the collate pads
            y = torch.randint(0, NC, (NB,), generator=g).cuda()
            out.append(((h_a, h_t, m_a, m_t, y), (h_a[~m_a].contiguous(), h_t[~m_t].contiguous(), list(la), list(lt), y)))
        _CACHE["b"] = out
    return _CACHE["b"]


def _head(batch, n):
    ra, rt, la, lt, y = batch
    return ra[:sum(la[:n])], rt[:sum(lt[:n])], la[:n], lt[:n], y[:n]


def _model(H, p=0.0):
    torch.manual_seed(3)
    return H.FusionClassifier(D, NC, 8, 2, 32, dropout=p).cuda().train()


def _loss(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import fusion_step_loss_single_label
    return fusion_step_loss_single_label(logits, beta, y, n_valid=n_valid)


def _loss_half(logits, beta, y, n_valid=None):
    """the single-label loss divided by grad_accum = 2 (the scale argument of the fused loss: exact)"""
    from hri_emo_amd._ops import FusionLossCEFn
    return FusionLossCEFn.apply(logits, beta, y, 1, 0.01, 0.5, *(() if n_valid is None else (n_valid,)))


def _dp(m, loss=_loss):
    from hri_emo_amd.dp import DataParallelStep
    dp = DataParallelStep(m, loss, overlap=False)
    dp.set_global_batch(NB)
    return dp


def _close(loss, flat, ref_loss, ref_flat, what):
    rel = float((flat - ref_flat).norm() / ref_flat.norm())
    print(f"{what}: loss {float(loss):.7f} vs {float(ref_loss):.7f}, relative L2 {rel:.2e}")
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss))), (what, float(loss), float(ref_loss))
    assert rel <= 1e-5, (what, rel)


# ----------------------------------------------------------------------------- against the mask-fed captured step
def _captured_run(m0, packed, word, p):
    """on a copy of m0: capture on batch 0 with DeviceAdamW in the graph, every batch once, batch 0 again -> [(loss, flat gradients,
    parameters)]"""
    from hri_emo_amd import _ops
    from hri_emo_amd.optim import DeviceAdamW
    dp = _dp(copy.deepcopy(m0))
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    torch.manual_seed(5)                             # the warm-up and capture passes draw their dropout seeds from torch's generator
    pad0, rag0 = _batches()[0]
    _ops.POOLED_GATE = not packed                    # the mask-fed arm is forward() through the pooled path
    if packed:
        dp.capture_packed(*rag0, pad_to=PAD, optimizer=opt)
    else:
        dp.capture(*pad0, lengths=(rag0[2], rag0[3]), optimizer=opt)
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)              # both arms replay from the same seed word
    out = []
    for i in (0, 1, 2, 0):
        pad, rag = _batches()[i]
        loss = dp.step_packed(*rag) if packed else dp.step(*pad, lengths=(rag[2], rag[3]))
        torch.cuda.synchronize()
        out.append((loss.clone(), dp.buckets.flat.clone(), opt.flat_p.clone()))
    dp.release_graph()
    _ops.POOLED_GATE = False
    return out


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_step_packed_equals_the_mask_fed_captured_step(H, p):
    """three different ragged batches (and the first again) through capture_packed(optimizer=DeviceAdamW): loss, flat gradients and
    parameters torch.equal to capture() / step() of the zero-padded batches with POOLED_GATE = True.  set_varlen(True) puts the mask-fed
    arm on the same row-count buckets (a bucket met for the first time is captured on the spot in both arms, so both draw the same
    dropout seeds from torch's generator); the classifier's encoder runs padded in both arms whatever set_varlen says"""
    from hri_emo_amd import _ops
    H.set_varlen(True)
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    m0 = _model(H, p)
    a, b = _captured_run(m0, True, word, p), _captured_run(m0, False, word, p)
    for i, (x, y) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(x[0])) and torch.equal(x[0], y[0]), (i, "loss", float(x[0]), float(y[0]))
        assert torch.equal(x[1], y[1]), (i, "flat gradients", int((x[1] != y[1]).sum()))
        assert torch.equal(x[2], y[2]), (i, "parameters")
    assert float(a[0][0]) != float(a[1][0]) and not torch.equal(a[0][2], a[3][2])


def test_two_replays_with_dropout_draw_fresh_masks(H):
    m = _model(H, 0.2)
    dp = _dp(m)
    rag = _batches()[0][1]
    torch.manual_seed(5)
    dp.capture_packed(*rag, pad_to=PAD)
    l0 = float(dp.step_packed(*rag))
    g0 = dp.buckets.flat.clone()
    l1 = float(dp.step_packed(*rag))
    torch.cuda.synchronize()
    assert l0 != l1 and not torch.equal(g0, dp.buckets.flat), "two replays of one batch at p = 0.2 drew the same masks"
    dp.release_graph()


# ----------------------------------------------------------------------------- short batches, accumulation
def test_short_batch_against_the_eager_step_on_its_own_utterances(H):
    """the first 3 utterances through the graph captured for 4 (one ghost) against the eager forward_packed step on those 3"""
    m0 = _model(H)
    full = _batches()[0][1]
    short = _head(full, 3)
    ref = _dp(copy.deepcopy(m0))
    ref.capture_packed(*full, pad_to=PAD)
    ref.use_graph(False)
    ref_loss = ref.step_packed(*short).clone()
    ref_flat = ref.buckets.flat.clone()
    dp = _dp(copy.deepcopy(m0))
    dp.capture_packed(*full, pad_to=PAD, partial_batches=True)
    loss = dp.step_packed(*short)
    torch.cuda.synchronize()
    assert dp._pb.front.ctl.dev.tolist() == [3, 1, 1, 0] and dp._pb.front.lens.dev.tolist() == [[40, 5, 1, 1], [35, 20, 1, 1]]
    _close(loss, dp.buckets.flat, ref_loss, ref_flat, "n = 3")
    ref.release_graph()
    dp.release_graph()


def test_accumulation_in_the_graph_against_step_accumulated(H):
    """grad_accum = 2, optimizer in the graph: micro-step 0 moves no parameter, micro-step 1 is one update; gradients and parameters
    against step_accumulated + opt.step() of an identical model run eagerly"""
    from hri_emo_amd.optim import DeviceAdamW
    m0 = _model(H)
    micro = [_batches()[0][1], _batches()[1][1]]
    ref = _dp(copy.deepcopy(m0), _loss)                        # step_accumulated scales by 1 / k itself
    ropt = DeviceAdamW(ref.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    dp = _dp(copy.deepcopy(m0), _loss_half)
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    dp.capture_packed(*micro[0], pad_to=PAD, optimizer=opt, grad_accum=2)
    torch.cuda.synchronize()
    before = opt.flat_p.clone()
    l0 = dp.step_packed(*micro[0]).clone()
    torch.cuda.synchronize()
    assert dp.micro_step == 1 and torch.equal(opt.flat_p, before), "micro-step 0 moved the parameters"
    l1 = dp.step_packed(*micro[1]).clone()
    torch.cuda.synchronize()
    assert dp.micro_step == 0 and float(opt.device_step) == 1.0
    total = ref.step_accumulated(micro, pad_to=PAD)
    ref_flat = ref.buckets.flat.clone()
    ropt.step()
    torch.cuda.synchronize()
    _close(l0 + l1, dp.buckets.flat, total, ref_flat, "summed loss, accumulated gradients")
    rel = float((opt.flat_p - ropt.flat_p).norm() / ropt.flat_p.norm())
    assert rel <= 1e-5, rel
    dp.release_graph()


# ----------------------------------------------------------------------------- the store
def _store():
    from hri_emo_amd.data import DeviceFeatureStore
    if "store" not in _CACHE:
        g = torch.Generator().manual_seed(23)
        la = [40, 5, 1, 33, 12, 40, 7, 20, 40, 3]
        lt = [35, 20, 1, 32, 8, 35, 3, 19, 35, 2]
        samples = [(torch.randn(a, D, generator=g), torch.zeros(a, dtype=torch.bool), torch.randn(t, D, generator=g),
                    torch.zeros(t, dtype=torch.bool), int(torch.randint(0, NC, (1,), generator=g))) for a, t in zip(la, lt)]
        _CACHE["store"] = DeviceFeatureStore.from_samples(samples, "cuda", loss_type="single_label", chunk_bytes=64 << 10)
    return _CACHE["store"]


def _packed(store, ids):
    ra, la, rt, lt, y = store.fetch(ids)
    return ra, rt, la, lt, y


IDS = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 0, 9, 5], [7, 6, 5, 4]]


def _store_arm(m0, store, by_id, word):
    from hri_emo_amd import _ops
    from hri_emo_amd.optim import DeviceAdamW
    dp = _dp(copy.deepcopy(m0))
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    torch.manual_seed(5)
    if by_id:
        dp.capture_store(store, IDS[0], optimizer=opt)
    else:
        dp.capture_packed(*_packed(store, IDS[0]), pad_to=store.pad_to, optimizer=opt)
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    out = []
    for ids in IDS:
        loss = dp.step_store(ids) if by_id else dp.step_packed(*_packed(store, ids))
        torch.cuda.synchronize()
        out.append((loss.clone(), dp.buckets.flat.clone(), opt.flat_p.clone()))
    dp.release_graph()
    return out


def test_step_store_equals_step_packed_on_the_fetched_batch(H):
    from hri_emo_amd import _ops
    store = _store()
    assert tuple(store.pad_to) == PAD
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    m0 = _model(H, 0.2)
    a, b = _store_arm(m0, store, True, word), _store_arm(m0, store, False, word)
    for i, (x, y) in enumerate(zip(a, b)):
        for j, name in enumerate(("loss", "flat gradients", "parameters")):
            assert torch.equal(x[j], y[j]), (i, name)


# ----------------------------------------------------------------------------- evaluation
def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y, equal_nan=True), (what, k)
        else:
            assert x == y or (x != x and y != y), (what, k, x, y)


def test_eval_step_with_stats_and_log_equals_the_eager_evaluation(H):
    """EvalStep(stats=EpochStats("single_label"), log=PredictionLog) over three batches (the last one short), by capture_packed and by
    capture_store: outputs, loss, EpochStats.result() and PredictionLog.arrays() bit-identical to the eager evaluation (model.eval(),
    forward_packed, the loss, the two updates) and to train.evaluate_packed / evaluate_store"""
    from hri_emo_amd.train import EpochStats, PredictionLog, evaluate_packed, evaluate_store
    store = _store()
    m = _model(H, 0.2)                                           # evaluation runs in eval mode: dropout is off
    batches = [IDS[0], IDS[1], [8, 9]]
    fetched = [store.fetch(ids) for ids in batches]
    new = lambda: (EpochStats(NC, 32, kind="single_label"), PredictionLog(NC, 32, kind="single_label"))          # noqa: E731
    (sa, la_), (sb, lb), (sc, lc) = new(), new(), new()
    ea, eb = H.EvalStep(m, _loss, stats=sa, log=la_), H.EvalStep(m, _loss, stats=sb, log=lb)
    ea.capture_store(store, batches[0])
    eb.capture_packed(*_packed(store, batches[0]), pad_to=store.pad_to)
    assert m.training
    for ids, (ra, la, rt, lt, y) in zip(batches, fetched):
        got, mid = ea.eval_store(ids), eb.eval_packed(ra, rt, la, lt, y)
        m.eval()
        with torch.no_grad():
            logits, beta, z = m.forward_packed(ra, rt, la, lt, pad_to=store.pad_to)
            loss = _loss(logits, beta, y)
            sc.update(logits, beta, y, loss)
            lc.update(logits, beta)
        m.train()
        torch.cuda.synchronize()
        for x, w, r, name in zip(got, mid, (logits, beta, z, loss), ("logits", "beta", "pooled", "loss")):
            assert x.shape == r.shape and torch.equal(x, r) and torch.equal(w, r), (ids, name)
        assert got[0].shape == (len(ids), NC)
    for s, l, what in ((sa, la_, "capture_store"), (sb, lb, "capture_packed")):
        _same(s.result(), sc.result(), what + " EpochStats")
        _same(l.arrays(), lc.arrays(), what + " PredictionLog")
    assert sa.result()["n_samples"] == 10
    ea.release_graph()
    eb.release_graph()
    s1, s2, s3, s4 = (EpochStats(NC, 32, kind="single_label") for _ in range(4))
    e1, e2 = H.EvalStep(m, _loss, stats=s1), H.EvalStep(m, _loss, stats=s2)
    evaluate_store(m, store, batches, _loss, s1, step=e1)
    evaluate_packed(m, fetched, _loss, s2, pad_to=store.pad_to, step=e2)
    evaluate_store(m, store, batches, _loss, s3)
    evaluate_packed(m, fetched, _loss, s4, pad_to=store.pad_to)
    for s, what in ((s1, "evaluate_store(step)"), (s2, "evaluate_packed(step)"), (s3, "evaluate_store"), (s4, "evaluate_packed")):
        _same(s.result(), sc.result(), what)
    e1.release_graph()
    e2.release_graph()
    assert all(p.grad is None for p in m.parameters()), "an evaluation creates no gradients"
