"""GPU suite of dp.EvalStep: the captured evaluation of ragged batches (capture_packed / eval_packed) against the eager
model.eval() + forward_packed + loss under no_grad, at the bound test_step_packed_against_the_eager_padded_step applies between a
captured and an eager form: 1e-5 relative L2 per output, loss 1e-5 * max(1, |ref|).  Shapes: those of test_gpu_step_packed*.py
(d128: B = 5, T_a = 70, T_t = 40, a length-1 sequence in each modality)."""
import copy
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, NE, NB, TA, TT = 128, 4, 5, 70, 40
LENGTHS = [([70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),          # 153 / 120 rows -> buckets 160 / 128
           ([12, 70, 5, 40, 9], [8, 40, 3, 20, 7])]             # 136 / 78        -> 144 / 80
KEYS = [(160, 128), (144, 80)]
PAD = (TA, TT)


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


def _tail(on):
    from hri_emo_amd import _ops
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = _ops.PACKED_TAIL_MX8 = bool(on)


_CACHE = {}


def _make(da, dt, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for la, lt in LENGTHS:
        ra, rt = torch.randn(sum(la), da, generator=g).cuda(), torch.randn(sum(lt), dt, generator=g).cuda()
        y = (torch.rand(NB, NE, generator=g) < 0.3).float().cuda()
        out.append((ra, rt, list(la), list(lt), y))
    return out


def _batches():
    """[(rows_a, rows_t, la, lt, y)] for LENGTHS: computed once, never changed"""
    if "b" not in _CACHE:
        _CACHE["b"] = _make(D, D, 11)
    return _CACHE["b"]


def _head(batch, n):
    """the first n utterances of a ragged batch"""
    ra, rt, la, lt, y = batch
    return ra[:sum(la[:n])], rt[:sum(lt[:n])], la[:n], lt[:n], y[:n]


def _model(H, p=0.0):
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=p).cuda().train()


def _loss():
    from hri_emo_amd.train import fusion_step_loss
    return fusion_step_loss


def _eager(m, batch, loss_fn=None):
    """the reference of every comparison: model.eval() + forward_packed + loss under no_grad -> (logits, beta, z, loss)"""
    ra, rt, la, lt, y = batch
    was = m.training
    m.eval()
    try:
        with torch.no_grad():
            logits, beta, z = m.forward_packed(ra, rt, la, lt, pad_to=PAD)
            loss = (loss_fn or _loss())(logits, beta, y)
    finally:
        m.train(was)
    torch.cuda.synchronize()
    return logits, beta, z, loss


def _close(got, ref, what):
    for name, a, b in zip(("logits", "beta", "z"), got[:3], ref[:3]):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"{what}: {name} relative L2 {rel:.2e}")
        assert rel <= 1e-5, (what, name, rel)
    if ref[3] is not None:
        a, b = float(got[3]), float(ref[3])
        print(f"{what}: loss {a:.7f} vs {b:.7f}")
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (what, a, b)


def _keep(out):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.clone() for t in out)


class Spy:
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


# ----------------------------------------------------------------------------- 1. captured against eager
@pytest.mark.parametrize("precision,tail", [("bf16", False), ("bf16", True), ("fp32", True)],
                         ids=["bf16 tail off", "bf16 tail on", "fp32 tail on"])
def test_eval_packed_against_the_eager_evaluation(H, precision, tail):
    """two batches in two buckets, each again after the other: every output and the loss; two graphs alive; the returned tensors
    are cut to the batch; use_graph(False) gives the eager outputs"""
    H.set_precision(precision)
    _tail(tail)
    m = _model(H)
    es = H.EvalStep(m, _loss())
    assert not es.captured
    es.capture_packed(*_batches()[0], pad_to=PAD)
    assert es.captured and list(es._pb.graphs) == [KEYS[0]] and m.training
    for i in (0, 1, 0, 1):
        got = _keep(es.eval_packed(*_batches()[i]))
        assert got[0].shape == (NB, NE) and got[3].dim() == 0
        _close(got, _eager(m, _batches()[i]), f"{precision} tail {tail} batch {i}")
    assert list(es._pb.graphs) == KEYS and len(es._pb.graphs) == 2
    es.use_graph(False)
    _close(_keep(es.eval_packed(*_batches()[1])), _eager(m, _batches()[1]), "use_graph(False)")
    assert all(p.grad is None for p in m.parameters()), "an evaluation creates no gradients"
    es.release_graph()
    assert not es.captured


# ----------------------------------------------------------------------------- 2. short batches
def test_short_batches_through_the_graphs_captured_for_five(H):
    """n = 3 and n = 1 against the eager evaluation of those utterances alone: the loss is the mean over n; the control block reads
    [n, 1, 1, 0], the lengths block shows the length-1 ghosts; NaN planted in the static target rows behind n changes nothing"""
    m = _model(H)
    es = H.EvalStep(m, _loss())
    full = _batches()[0]
    es.capture_packed(*full, pad_to=PAD)
    for n, lens in ((3, [[70, 33, 32, 1, 1], [40, 1, 32, 1, 1]]), (1, [[70, 1, 1, 1, 1], [40, 1, 1, 1, 1]])):
        short = _head(full, n)
        es._static[4][n:] = float("nan")
        got = _keep(es.eval_packed(*short))
        front = es._pb.front
        assert front.ctl.dev.tolist() == [n, 1, 1, 0] and front.lens.dev.tolist() == lens
        assert got[0].shape == (n, NE) and got[1].shape[0] == n and got[2].shape[0] == n
        assert all(bool(torch.isfinite(t).all()) for t in got)
        _close(got, _eager(m, short), f"n = {n}")
    es.release_graph()


# ----------------------------------------------------------------------------- 3. weights move
def test_an_evaluation_behind_an_optimizer_replay_sees_the_new_weights(H):
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    m = _model(H)
    b0 = _batches()[0]
    dp = DataParallelStep(m, _loss(), overlap=False)
    dp.set_global_batch(NB)
    opt = DeviceAdamW(dp.buckets, lr=1e-2, weight_decay=1e-2, max_norm=5.0)
    dp.capture_packed(*b0, pad_to=PAD, optimizer=opt)
    es = H.EvalStep(m, _loss())
    es.capture_packed(*b0, pad_to=PAD)
    first = _keep(es.eval_packed(*b0))
    _close(first, _eager(m, b0), "before the update")
    dp.step_packed(*b0)
    second = _keep(es.eval_packed(*b0))
    _close(second, _eager(m, b0), "after the update")
    assert not torch.equal(first[0], second[0]) and float(first[3]) != float(second[3]), "the replay still ran on the old weights"
    es.release_graph()
    dp.release_graph()


# ----------------------------------------------------------------------------- 4. training is untouched
def test_training_is_untouched_by_evaluations_between_its_steps(H):
    """three step_packed at dropout 0.1 (optimizer in the graph), with and without eval_packed calls between them -- one of which
    meets a new bucket: losses and final parameters torch.equal; across every eval_packed the device seed word, torch's CPU
    generator and the flat gradient buffer keep their bits"""
    from hri_emo_amd import _ops
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    word = _ops.seed_word(torch.device("cuda", 0))
    word0 = word.clone()
    m0 = _model(H, 0.1)
    b0, b1 = _batches()
    runs = []
    for with_eval in (False, True):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, _loss(), overlap=False)
        dp.set_global_batch(NB)
        opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
        torch.manual_seed(5)
        dp.capture_packed(*b0, pad_to=PAD, optimizer=opt)
        es = None
        if with_eval:
            es = H.EvalStep(m, _loss())
            rng, w = torch.get_rng_state(), word.clone()
            es.capture_packed(*b0, pad_to=PAD)
            torch.cuda.synchronize()
            assert torch.equal(torch.get_rng_state(), rng) and torch.equal(word, w) and m.training
        word.copy_(word0)
        losses = []
        for i, b in enumerate((b0, b1, b0)):
            losses.append(dp.step_packed(*b).clone())
            if es is not None:
                torch.cuda.synchronize()
                rng, w, flat = torch.get_rng_state(), word.clone(), dp.buckets.flat.clone()
                n_graphs = len(es._pb.graphs)
                out = _keep(es.eval_packed(*(b1 if i == 0 else _head(b0, 3))))
                assert len(es._pb.graphs) == n_graphs + (1 if i == 0 else 0), "the first evaluation meets a new bucket"
                assert torch.equal(torch.get_rng_state(), rng) and torch.equal(word, w) and torch.equal(dp.buckets.flat, flat), i
                assert m.training and bool(torch.isfinite(out[0]).all())
        torch.cuda.synchronize()
        runs.append((losses, opt.flat_p.clone()))
        if es is not None:
            es.release_graph()
        dp.release_graph()
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), (float(a), float(b))
    assert torch.equal(runs[0][1], runs[1][1]), int((runs[0][1] != runs[1][1]).sum())
    assert not torch.equal(runs[0][0][0], runs[0][0][2]), "dropout is fresh per replay"


def test_no_gradients_on_a_fresh_model_and_the_training_flag_comes_back(H):
    for training in (True, False):
        m = _model(H, 0.1).train(training)
        es = H.EvalStep(m, _loss())
        es.capture_packed(*_batches()[0], pad_to=PAD)
        es.eval_packed(*_batches()[1])                       # a new bucket: a capture inside eval_packed
        assert m.training == training
        ra, rt, la, lt, y = _batches()[0]
        with pytest.raises(ValueError):
            es.eval_packed(torch.cat([ra, ra[:la[0]]]), torch.cat([rt, rt[:lt[0]]]), la + la[:1], lt + lt[:1], torch.cat([y, y[:1]]))
        assert m.training == training
        es.use_graph(False)
        es.eval_packed(*_batches()[1])
        assert m.training == training
        assert all(p.grad is None for p in m.parameters())
        es.release_graph()


# ----------------------------------------------------------------------------- 5. what a replay launches
def test_what_the_capture_records_and_a_replay_launches(H, monkeypatch):
    from hri_emo_amd.train import EpochStats, PredictionLog
    m = _model(H, 0.1)
    stats, log = EpochStats(NE, 32), PredictionLog(NE, 32)
    es = H.EvalStep(m, _loss(), stats=stats, log=log)
    spy = Spy(monkeypatch)
    es.capture_packed(*_batches()[0], pad_to=PAD)
    names = spy.take()
    assert names[0] == "hriemo_seq_tables" and names.count("hriemo_seq_tables") == 3, "two warm-up passes and the capture pass"
    recorded = names[len(names) - 1 - names[::-1].index("hriemo_seq_tables"):]
    assert recorded.count("hriemo_seq_tables") == 1 and recorded.count("hriemo_stats_update") == 1 and recorded.count("hriemo_predict_log") == 1
    assert names.count("hriemo_stats_update") == 1 and names.count("hriemo_predict_log") == 1, "no warm-up pass feeds stats or log"
    assert recorded.index("hriemo_stats_update") < recorded.index("hriemo_predict_log") == len(recorded) - 1
    assert sum(n.startswith("hriemo_fusion_loss") for n in recorded) == 1 and "hriemo_fusion_loss_n" in recorded
    assert recorded.count("hriemo_ingest_rows") == 2
    for n in names:
        assert n != "hriemo_seed_bump" and not any(s in n for s in ("_bwd", "adamw", "sumsq", "optim_", "grad_begin")), n
    es.eval_packed(*_batches()[0])
    torch.cuda.synchronize()
    assert spy.take() == [], "a replay of a known bucket launches nothing from the host"
    es.eval_packed(*_head(_batches()[0], 3))                 # with its two ghosts: the bucket of batch 1, not seen yet
    names = spy.take()
    assert names.count("hriemo_seq_tables") == 3 and names.count("hriemo_stats_update") == 1 and names.count("hriemo_predict_log") == 1
    es.eval_packed(*_batches()[1])
    torch.cuda.synchronize()
    assert spy.take() == [] and list(es._pb.graphs) == KEYS, "a short batch and a full one share a bucket's graph"
    es.release_graph()
    # without stats and log: neither launch
    es = H.EvalStep(m, _loss())
    es.capture_packed(*_batches()[0], pad_to=PAD)
    names = spy.take()
    assert "hriemo_stats_update" not in names and "hriemo_predict_log" not in names and names.count("hriemo_seq_tables") == 3
    es.release_graph()


# ----------------------------------------------------------------------------- 6. statistics and log
def test_statistics_and_log_fed_inside_the_graph(H):
    """three batches, the last short, against twins fed eagerly from the tensors eval_packed returned: counters equal, logs
    torch.equal, float64 sums within 1e-12; the integers of result() (tp / fp / fn at every threshold, 2U) equal; the warm-up passes
    of a capture leave both untouched"""
    from hri_emo_amd.train import EpochStats, PredictionLog
    m = _model(H)
    stats, log = EpochStats(NE, 32), PredictionLog(NE, 32)
    twin_s, twin_l = EpochStats(NE, 32), PredictionLog(NE, 32)
    es = H.EvalStep(m, _loss(), stats=stats, log=log)
    b0, b1 = _batches()
    es.capture_packed(*b0, pad_to=PAD)
    torch.cuda.synchronize()
    assert stats.counters.tolist() == [0] * 8 and stats.sums.tolist() == [0.0] * 4 and log.counters.tolist() == [0] * 4
    for i, b in enumerate((b0, b1, _head(b0, 3))):
        logits, beta, z, loss = es.eval_packed(*b)            # b1: a capture in the middle of the epoch
        twin_s.update(logits, beta, b[4], loss)
        twin_l.update(logits, beta)
        torch.cuda.synchronize()
    assert stats.counters.tolist() == twin_s.counters.tolist() and stats.counters.tolist()[:3] == [13, 13, 3]
    assert log.counters.tolist() == twin_l.counters.tolist() == [13, 13, 0, 0]
    assert torch.equal(stats.probs, twin_s.probs) and torch.equal(stats.truth, twin_s.truth)
    assert torch.equal(log.probs, twin_l.probs) and torch.equal(log.beta_mean, twin_l.beta_mean)
    assert torch.equal(log.probs[:, :13], stats.probs[:, :13]), "both logs hold the same bits"
    for a, b in zip(stats.sums.tolist(), twin_s.sums.tolist()):
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)
    r, t = stats.result(), twin_s.result()
    for name in ("tp", "fp", "fn", "sweep_counts", "auc_2u", "n_pos", "n_neg"):
        assert np.array_equal(r[name], t[name]), name
    assert r["n_samples"] == 13 and r["n_batches"] == 3
    out = log.arrays()
    assert out["y_prob"].shape == (13, NE) and out["beta_mean"].shape == (13,) and out["n_nonfinite"] == 0
    assert np.array_equal(out["y_prob"], stats.probs[:, :13].t().cpu().numpy())
    es.release_graph()


# ----------------------------------------------------------------------------- 7. prediction-only graphs
def test_prediction_only_graphs(H):
    from hri_emo_amd.train import EpochStats, PredictionLog
    m = _model(H)
    b0, b1 = _batches()
    log = PredictionLog(NE, 16)
    es = H.EvalStep(m, _loss(), log=log)                      # a loss_fn without targets: prediction-only all the same
    es.capture_packed(*b0[:4], pad_to=PAD)
    assert es._static[4] is None
    got = _keep(es.eval_packed(*b1[:4]))
    assert got[3] is None
    _close(got, _eager(m, b1)[:3] + (None,), "prediction-only")
    short = _keep(es.eval_packed(*_head(b0, 3)[:4]))
    _close(short, _eager(m, _head(b0, 3))[:3] + (None,), "prediction-only, n = 3")
    torch.cuda.synchronize()
    assert log.counters.tolist() == [8, 8, 0, 0]
    with pytest.raises(ValueError, match="prediction-only"):
        es.eval_packed(*b0)
    es.release_graph()
    with pytest.raises(ValueError, match="statistics"):
        H.EvalStep(m, _loss(), stats=EpochStats(NE, 16)).capture_packed(*b0[:4], pad_to=PAD)
    es = H.EvalStep(m, _loss())
    es.capture_packed(*b0, pad_to=PAD)
    with pytest.raises(ValueError, match="captured with targets"):
        es.eval_packed(*b0[:4])
    es.release_graph()


# ----------------------------------------------------------------------------- 8. accounting
def test_graph_accounting(H):
    from hri_emo_amd import _ops
    from hri_emo_amd.dp import DataParallelStep
    _tail(True)
    m = _model(H)
    b0, b1 = _batches()
    alive0 = _ops.GRAPHS_ALIVE
    es = H.EvalStep(m, _loss())
    es.capture_packed(*b0, pad_to=PAD)
    assert _ops.GRAPHS_ALIVE == alive0 + 1
    es.eval_packed(*b1)
    assert _ops.GRAPHS_ALIVE == alive0 + 2 == alive0 + len(es._pb.graphs)
    dp = DataParallelStep(copy.deepcopy(m), _loss(), overlap=False)
    dp.set_global_batch(NB)
    dp.capture_packed(*b0, pad_to=PAD)
    assert _ops.GRAPHS_ALIVE == alive0 + 3 and es.ctx is not dp.ctx
    before = _keep(es.eval_packed(*b0))
    loss = dp.step_packed(*b0).clone()
    dp.release_graph()
    assert _ops.GRAPHS_ALIVE == alive0 + 2 and es.captured
    after = _keep(es.eval_packed(*b0))
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    dp.capture_packed(*b0, pad_to=PAD)
    es.release_graph()
    assert _ops.GRAPHS_ALIVE == alive0 + 1 and not es.captured and dp.captured
    assert torch.equal(dp.step_packed(*b0), loss)
    dp.release_graph()
    assert _ops.GRAPHS_ALIVE == alive0
    # max_graphs = 1: the evicted bucket's graph dies with its record
    es = H.EvalStep(m, _loss(), max_graphs=1)
    es.capture_packed(*b0, pad_to=PAD)
    first = _keep(es.eval_packed(*b0))
    graph0 = weakref.ref(es._pb.graphs[KEYS[0]].graph)
    es.eval_packed(*b1)
    assert list(es._pb.graphs) == [KEYS[1]] and _ops.GRAPHS_ALIVE == alive0 + 1
    gc.collect()
    assert graph0() is None, "the evicted bucket's graph is still alive"
    again = _keep(es.eval_packed(*b0))
    assert list(es._pb.graphs) == [KEYS[0]] and all(torch.equal(a, b) for a, b in zip(first, again))
    es.release_graph()
    assert _ops.GRAPHS_ALIVE == alive0


# ----------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_static_state_untouched(H):
    m = _model(H)
    ra, rt, la, lt, y = _batches()[0]
    with pytest.raises(TypeError, match="forward_packed"):
        H.EvalStep(torch.nn.Linear(4, 4).cuda(), _loss()).capture_packed(ra, rt, la, lt, y, pad_to=PAD)
    with pytest.raises(TypeError, match="n_valid"):
        H.EvalStep(m, lambda logits, beta, y: logits.sum()).capture_packed(ra, rt, la, lt, y, pad_to=PAD)
    es = H.EvalStep(m, _loss())
    with pytest.raises(RuntimeError, match="capture_packed"):
        es.eval_packed(ra, rt, la, lt, y)
    with pytest.raises(ValueError, match="pad_to"):
        es.capture_packed(ra, rt, la, lt, y, pad_to=None)
    es.capture_packed(ra, rt, la, lt, y, pad_to=PAD)
    es.eval_packed(ra, rt, la, lt, y)
    torch.cuda.synchronize()
    front = es._pb.front
    state = lambda: [t.clone() for t in (es._static[0], es._static[1], es._static[4], front.lens.dev, front.lens.host, front.ctl.dev,      # noqa: E731
                                         front.ctl.host, es._pb.cu_a, es._pb.cu_t, es._pb.cu_f) + front.masks]
    before = state()
    bad = {
        "n = 6": (torch.cat([ra, ra[:la[0]]]), torch.cat([rt, rt[:lt[0]]]), la + la[:1], lt + lt[:1], torch.cat([y, y[:1]])),
        "n = 0": (ra[:0], rt[:0], [], [], y[:0]),
        "another width": (ra[:, :64].contiguous(), rt[:, :64].contiguous(), la, lt, y),
        "another dtype": (ra.bfloat16(), rt.bfloat16(), la, lt, y),
        "a length of 0": (ra, rt, [la[0] - 1, 0] + la[2:], lt, y),
        "a length past L": (ra, rt, la, [TT + 1] + lt[1:], y),
        "rows that do not add up": (ra[:-1], rt, la, lt, y),
        "a CUDA lengths tensor": (ra, rt, torch.tensor(la).cuda(), lt, y),
        "targets of another shape": (ra, rt, la, lt, y[:, :3].contiguous()),
        "targets of the full batch with a short one": _head(_batches()[0], 3)[:4] + (y,),
        "no targets": (ra, rt, la, lt, None),
    }
    for what, args in bad.items():
        with pytest.raises(ValueError):
            es.eval_packed(*args)
        torch.cuda.synchronize()
        for a, b in zip(before, state()):
            assert torch.equal(a, b), what
    H.set_precision("fp32")
    with pytest.raises(RuntimeError, match="precision"):
        es.eval_packed(ra, rt, la, lt, y)
    H.set_precision("bf16")
    _tail(True)
    with pytest.raises(RuntimeError, match="PACKED_TAIL"):
        es.eval_packed(ra, rt, la, lt, y)
    _tail(False)
    H.set_ingest(True)
    with pytest.raises(RuntimeError, match="ingest"):
        es.eval_packed(ra, rt, la, lt, y)
    H.set_ingest(False)
    torch.cuda.synchronize()
    for a, b in zip(before, state()):
        assert torch.equal(a, b), "a mode switch"
    assert len(es._pb.graphs) == 1, "nothing was captured under another setting"
    es.eval_packed(ra, rt, la, lt, y)
    es.release_graph()


# ----------------------------------------------------------------------------- 10. MOSEI wrapper
def test_mosei_eval_packed(H):
    """d_audio 74, d_text 300, d = 128 (the shapes of test_mosei_step_packed), mosei_step_loss with the beta entropy term"""
    import functools
    from hri_emo_amd.train import mosei_step_loss
    loss_fn = functools.partial(mosei_step_loss, beta_entropy=0.01)
    batches = _make(74, 300, 5)
    torch.manual_seed(3)
    m = H.MoseiFusionWithEmotionDecoder(d_audio=74, d_text=300, d_model=D, num_emotions=NE, n_heads=8, dropout=0.2).cuda().train()
    _tail(True)
    es = H.EvalStep(m, loss_fn)
    es.capture_packed(*batches[0], pad_to=PAD)
    assert es._static[0].shape[1] == 74 and es._static[1].shape[1] == 300
    for i, b in enumerate((batches[0], batches[1], _head(batches[0], 2))):
        _close(_keep(es.eval_packed(*b)), _eager(m, b, loss_fn), f"mosei batch {i}")
    es.release_graph()


# ----------------------------------------------------------------------------- 11. evaluate_packed(step=...)
def test_evaluate_packed_with_a_step(H):
    """a three-batch epoch with a short last batch, captured on the spot from the first batch, against step=None"""
    from hri_emo_amd.train import EpochStats, evaluate_packed
    m = _model(H)
    b0, b1 = _batches()
    epoch = [(ra, la, rt, lt, y) for ra, rt, la, lt, y in (b0, b1, _head(b0, 3))]
    ref = evaluate_packed(m, epoch, _loss(), EpochStats(NE, 32), pad_to=PAD).result()
    stats = EpochStats(NE, 32)
    es = H.EvalStep(m, _loss(), stats=stats)
    with pytest.raises(ValueError, match="pad_to"):
        evaluate_packed(m, epoch, _loss(), stats, step=es)
    with pytest.raises(ValueError, match="another"):
        evaluate_packed(m, epoch, _loss(), EpochStats(NE, 32), pad_to=PAD, step=es)
    assert evaluate_packed(m, epoch, _loss(), stats, pad_to=PAD, step=es) is stats and es.captured and m.training
    got = stats.result()
    assert got["n_samples"] == ref["n_samples"] == 13 and got["n_batches"] == ref["n_batches"] == 3
    for name in ("avg_loss", "mean_beta"):
        print(f"{name}: {got[name]:.9f} vs {ref[name]:.9f}")
        assert abs(got[name] - ref[name]) <= 1e-5 * abs(ref[name]), name
    stats.reset()
    evaluate_packed(m, epoch, _loss(), stats, step=es)       # a captured step needs no pad_to
    again = stats.result()
    assert again["n_samples"] == 13 and again["avg_loss"] == got["avg_loss"]
    es.release_graph()
