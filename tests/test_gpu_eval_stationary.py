"""GPU suite of dp.EvalStep(stationary=True): bucket graphs that hold only what depends on the batch, the weight forms and the
decoder's query prologue in the step's weights pass, replayed only when the weights moved.

The reference of every comparison is the default captured step on the same model (torch.equal: the weights pass runs the same
kernels on the same shapes in the same order) and, through _close, the eager evaluation at test_gpu_eval_step.py's 1e-5 bound.
Helpers and shapes are that module's: d = 128, N_e = 4, B = 5, pad (70, 40), its two length sets with a length-1 sequence in
each modality."""
import collections
import copy
import gc
import weakref

import numpy as np
import pytest
import torch

from test_gpu_eval_step import D, KEYS, NB, NE, PAD, Spy, _batches, _close, _eager, _head, _keep, _loss, _make, _model, _tail

pytestmark = pytest.mark.gpu

CASTS = ("hriemo_cast_f32_to_bf16", "hriemo_cast_f32_to_bf16_batch", "hriemo_cast_copy_batch")


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    keep = (_ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.gemm_mode(), _ops.precision(), _ops.varlen_maps(),
            _ops.mfma_maps())
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    yield hri_emo_amd
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_ingest(False)
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = keep[:3]
    hri_emo_amd.set_gemm_mode(keep[3])
    hri_emo_amd.set_precision(keep[4])
    hri_emo_amd.set_varlen_maps(keep[5])
    hri_emo_amd.set_mfma_maps(keep[6])


def _same(got, ref, what):
    """logits, beta, z and the loss of two evaluations: the same bits"""
    for name, a, b in zip(("logits", "beta", "z", "loss"), got, ref):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and torch.equal(a, b), (what, name, float((a.double() - b.double()).abs().max()))


def _pair(H, m, loss_fn, batch, **kw):
    """a default and a stationary step on one model, both captured on `batch`"""
    plain, stat = H.EvalStep(m, loss_fn, **kw.get("plain", {})), H.EvalStep(m, loss_fn, stationary=True, **kw.get("stat", {}))
    plain.capture_packed(*batch, pad_to=PAD)
    stat.capture_packed(*batch, pad_to=PAD)
    return plain, stat


def _passes(es, spy):
    """wrap es._pass: -> the list [(record, launch names)] that fills as passes run"""
    seen, real = [], es._pass

    def wrapped(record):
        spy.take()
        out = real(record)
        seen.append((record, spy.take()))
        return out

    es._pass = wrapped
    return seen


# ----------------------------------------------------------------------------- 1. same bits
@pytest.mark.parametrize("precision,tail", [("bf16", False), ("bf16", True), ("fp32", True)],
                         ids=["bf16 tail off", "bf16 tail on", "fp32 tail on"])
def test_same_bits_as_the_default_step(H, precision, tail):
    """both batches and the 3-utterance head of the first, each twice (the static prologue is read again and again): logits, beta,
    z and the loss torch.equal to the default step's, and within 1e-5 of the eager evaluation"""
    H.set_precision(precision)
    _tail(tail)
    m = _model(H)
    b0, b1 = _batches()
    plain, stat = _pair(H, m, _loss(), b0)
    assert stat.stationary and not plain.stationary and plain._weights is None and len(stat._weights.records) == 1
    for i, batch in enumerate((b0, b1, _head(b0, 3)) * 2):
        ref = _keep(plain.eval_packed(*batch))
        got = _keep(stat.eval_packed(*batch))
        what = f"{precision} tail {tail} input {i}"
        _same(got, ref, what)
        _close(got, _eager(m, batch), what)
    assert list(stat._pb.graphs) == KEYS and m.training
    stat.release_graph()
    plain.release_graph()


# ----------------------------------------------------------------------------- 2. MX-fp8
def test_same_bits_in_mx_fp8_mode(H, monkeypatch):
    """16 utterances of 70 audio rows: 1120 packed rows >= MX_MIN_ROWS, so the audio stream's GEMMs run on MX-fp8 operands whose
    weight forms (mx8_shadow, get_cat_mx8) the bucket graph of the stationary step no longer derives"""
    from hri_emo_amd import _ops
    H.set_gemm_mode("mx_fp8")
    _tail(True)
    n = 16
    assert n * PAD[0] >= _ops.MX_MIN_ROWS
    g = torch.Generator().manual_seed(17)
    la, lt = [PAD[0]] * n, [PAD[1], 1, 32, 31] * 4
    batch = (torch.randn(sum(la), D, generator=g).cuda(), torch.randn(sum(lt), D, generator=g).cuda(), la, lt,
             (torch.rand(n, NE, generator=g) < 0.3).float().cuda())
    m = _model(H)
    spy = Spy(monkeypatch)
    plain, stat = H.EvalStep(m, _loss()), H.EvalStep(m, _loss(), stationary=True)
    seen_p, seen_s = _passes(plain, spy), _passes(stat, spy)
    plain.capture_packed(*batch, pad_to=PAD)
    stat.capture_packed(*batch, pad_to=PAD)
    rec_p, rec_s = seen_p[-1], seen_s[-1]
    assert rec_p[0] and rec_s[0]
    assert "hriemo_gemm_mx8" in rec_p[1], "the default step's recorded pass runs no MX-fp8 GEMM: this case would test nothing"
    assert "hriemo_gemm_mx8" in rec_s[1]
    assert rec_s[1].count("hriemo_quant_mx8") < rec_p[1].count("hriemo_quant_mx8"), "the weight quantisers are still in the bucket graph"
    assert not any(name in CASTS for name in rec_s[1])
    short = _head(batch, 9)
    for i, b in enumerate((batch, short, batch)):
        ref = _keep(plain.eval_packed(*b))
        got = _keep(stat.eval_packed(*b))
        _same(got, ref, f"mx_fp8 input {i}")
        _close(got, _eager(m, b), f"mx_fp8 input {i}")
    # the weights move: the MX-fp8 forms are refreshed in the buffers the bucket graph points at
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.03)
    ref = _keep(plain.eval_packed(*batch))
    moved = _keep(stat.eval_packed(*batch))
    _same(moved, ref, "mx_fp8 after an in-place edit")
    assert not torch.equal(moved[0], got[0])
    stat.release_graph()
    plain.release_graph()


# ----------------------------------------------------------------------------- 3. what is launched
def test_what_the_weights_pass_and_a_bucket_graph_hold(H, monkeypatch):
    from hri_emo_amd import _ops
    m = _model(H, 0.1)
    b0, b1 = _batches()
    spy = Spy(monkeypatch)
    plain, stat = H.EvalStep(m, _loss()), H.EvalStep(m, _loss(), stationary=True)
    seen_p, seen_s = _passes(plain, spy), _passes(stat, spy)
    plain.capture_packed(*b0, pad_to=PAD)
    stat.capture_packed(*b0, pad_to=PAD)
    assert [r for r, _ in seen_p] == [False, False, True]
    assert [r for r, _ in seen_s] == [False, False, False, True], "the pass that finds the forms, two warm-up passes, the recording"
    rec_p, rec_s = seen_p[-1][1], seen_s[-1][1]
    spy.take()
    # a call with unmoved weights on a known bucket
    stat.eval_packed(*b0)
    torch.cuda.synchronize()
    assert spy.take() == [], "a replay of a known bucket with unmoved weights launches nothing from the host"
    # the weights pass, launch by launch: every form is stale after the bump
    _ops.bump_weights_epoch()
    stat._weights.eager()
    weights = spy.take()
    assert collections.Counter(weights) + collections.Counter(rec_s) == collections.Counter(rec_p), \
        (collections.Counter(rec_p) - collections.Counter(weights) - collections.Counter(rec_s),
         collections.Counter(weights) + collections.Counter(rec_s) - collections.Counter(rec_p))
    assert any(n in CASTS for n in weights) and any(n in CASTS for n in rec_p)
    assert not any(n.startswith("hriemo_cast_f32_to_bf16") or n == "hriemo_cast_copy_batch" for n in rec_s), rec_s
    assert rec_s.count("hriemo_expand_rows") == rec_p.count("hriemo_expand_rows") - 1 and weights.count("hriemo_expand_rows") == 1
    assert rec_s[0] == "hriemo_seq_tables" and "hriemo_seq_tables" not in weights
    # after the move: the pass is a graph, so the next call launches nothing from the host either, and runs it
    assert stat._weights.moved()
    stat.eval_packed(*b0)
    torch.cuda.synchronize()
    assert spy.take() == [] and not stat._weights.moved()
    stat.eval_packed(*b0)
    torch.cuda.synchronize()
    assert spy.take() == []
    # a new bucket: its capture records no weight derivation (and, the forms being fresh, its other passes launch none)
    n_seen = len(seen_s)
    stat.eval_packed(*b1)
    torch.cuda.synchronize()
    new = seen_s[n_seen:]
    assert [r for r, _ in new] == [False, False, False, True] and list(stat._pb.graphs) == KEYS
    assert len(stat._weights.records) == 1, "the second bucket asks for no form the first did not"
    for _, names in new:
        assert not any(n.startswith("hriemo_cast_f32_to_bf16") or n == "hriemo_cast_copy_batch" for n in names), names
    assert new[-1][1].count("hriemo_expand_rows") == rec_s.count("hriemo_expand_rows")
    spy.take()
    stat.eval_packed(*b1)
    torch.cuda.synchronize()
    assert spy.take() == []
    stat.release_graph()
    plain.release_graph()


# ----------------------------------------------------------------------------- 4. weights move
def test_every_way_the_weights_move(H):
    """a captured optimizer replay (WEIGHTS_EPOCH), an eager torch.optim step and load_state_dict (parameter versions), an in-place
    edit of emotion_queries alone (the prologue's own freshness): each time equal to the default step, close to the eager
    evaluation, and another result than before"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    m = _model(H)
    b0 = _batches()[0]
    dp = DataParallelStep(m, _loss(), overlap=False)
    dp.set_global_batch(NB)
    opt = DeviceAdamW(dp.buckets, lr=1e-2, weight_decay=1e-2, max_norm=5.0)
    dp.capture_packed(*b0, pad_to=PAD, optimizer=opt)
    plain, stat = _pair(H, m, _loss(), b0)
    last = _keep(stat.eval_packed(*b0))
    _same(last, _keep(plain.eval_packed(*b0)), "before any move")
    torch_opt = torch.optim.AdamW(m.parameters(), lr=1e-2)

    def load_perturbed():
        g = torch.Generator().manual_seed(23)
        m.load_state_dict({k: v + 0.02 * torch.randn(v.shape, generator=g).to(v.device) for k, v in m.state_dict().items()})

    def scale_queries():
        with torch.no_grad():
            m.emotion_decoder.emotion_queries.mul_(1.5)

    moves = (("DeviceAdamW in the graph", lambda: dp.step_packed(*b0)), ("torch.optim.AdamW.step", torch_opt.step),
             ("load_state_dict", load_perturbed), ("emotion_queries.mul_", scale_queries))
    for what, move in moves:
        move()
        assert stat._weights.moved(), what
        got = _keep(stat.eval_packed(*b0))
        assert not stat._weights.moved()
        _same(got, _keep(plain.eval_packed(*b0)), what)
        _close(got, _eager(m, b0), what)
        assert not torch.equal(got[0], last[0]) and float(got[3]) != float(last[3]), f"{what}: the replay still ran on the old weights"
        _same(_keep(stat.eval_packed(*b0)), got, f"{what}, again")
        last = got
    stat.release_graph()
    plain.release_graph()
    dp.release_graph()


# ----------------------------------------------------------------------------- 5. training is untouched
def test_training_is_untouched_by_stationary_evaluations_between_its_steps(H):
    """test_gpu_eval_step.py's three step_packed at dropout 0.1 (optimizer in the graph), with and without stationary eval_packed
    calls between them -- one of which meets a new bucket: losses and final parameters torch.equal; across every evaluation the
    device seed word, torch's CPU generator and the flat gradient buffer keep their bits"""
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
            es = H.EvalStep(m, _loss(), stationary=True)
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
                batch = b1 if i == 0 else _head(b0, 3)
                out = _keep(es.eval_packed(*batch))
                assert len(es._pb.graphs) == n_graphs + (1 if i == 0 else 0), "the first evaluation meets a new bucket"
                assert torch.equal(torch.get_rng_state(), rng) and torch.equal(word, w) and torch.equal(dp.buckets.flat, flat), i
                assert m.training and bool(torch.isfinite(out[0]).all())
                _close(out, _eager(m, batch), f"behind step {i}")
                assert torch.equal(torch.get_rng_state(), rng) and torch.equal(word, w)
        torch.cuda.synchronize()
        runs.append((losses, opt.flat_p.clone()))
        if es is not None:
            es.release_graph()
        dp.release_graph()
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), (float(a), float(b))
    assert torch.equal(runs[0][1], runs[1][1]), int((runs[0][1] != runs[1][1]).sum())
    assert not torch.equal(runs[0][0][0], runs[0][0][2]), "dropout is fresh per replay"


# ----------------------------------------------------------------------------- 6. everything attached
def _equal_values(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _equal_values(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _equal_values(x, y, f"{what}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b), what
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b, equal_nan=True), what
    else:
        assert a == b or (a != a and b != b), (what, a, b)


@pytest.mark.parametrize("tail", [False, True], ids=["tail off", "tail on"])
def test_statistics_prediction_log_and_attention_log_attached(H, tail):
    """EpochStats, PredictionLog and AttentionLog on a stationary step, two batches and a short one: result(), arrays() and the
    logged maps equal the default step's bit for bit (tail off: the decoder's padded map goes through the append)"""
    from hri_emo_amd.train import AttentionLog, EpochStats, PredictionLog
    _tail(tail)
    H.set_varlen_maps(True)
    m = _model(H)
    b0, b1 = _batches()
    steps = []
    for stationary in (False, True):
        es = H.EvalStep(m, _loss(), stats=EpochStats(NE, 32), log=PredictionLog(NE, 32), attn_log=AttentionLog.for_model(m, 12, PAD),
                        stationary=stationary)
        es.capture_packed(*b0, pad_to=PAD)
        steps.append(es)
    plain, stat = steps
    for i, batch in enumerate((b0, b1, _head(b0, 3))):
        _same(_keep(stat.eval_packed(*batch)), _keep(plain.eval_packed(*batch)), f"batch {i}")
    torch.cuda.synchronize()
    assert stat.stats.counters.tolist()[:3] == [13, 13, 3] and stat.attn_log.counters.tolist()[0] == 12
    _equal_values(stat.stats.result(), plain.stats.result(), "EpochStats.result()")
    _equal_values(stat.log.arrays(), plain.log.arrays(), "PredictionLog.arrays()")
    _equal_values(stat.attn_log.arrays(), plain.attn_log.arrays(), "AttentionLog.arrays()")
    assert torch.equal(stat.stats._small, plain.stats._small) and torch.equal(stat.log._buf, plain.log._buf)
    assert torch.equal(stat.attn_log._small, plain.attn_log._small)
    for a, b in zip(stat.attn_log._tensors(), plain.attn_log._tensors()):
        assert torch.equal(a, b)
    assert any(bool(t.any()) for t in stat.attn_log.decoder_maps), "no decoder map was logged"
    stat.release_graph()
    plain.release_graph()


def test_capture_store_and_evaluate_store(H):
    from test_gpu_store_step import FULL, _store
    from test_gpu_store_step import _loss as store_loss
    from hri_emo_amd.train import EpochStats, evaluate_store
    store = _store()
    m = _model(H)
    plain, stat = H.EvalStep(m, store_loss), H.EvalStep(m, store_loss, stationary=True)
    plain.capture_store(store, FULL[0])
    stat.capture_store(store, FULL[0])
    for ids in (FULL[0], FULL[1], [3, 11], FULL[2]):
        _same(_keep(stat.eval_store(ids)), _keep(plain.eval_store(ids)), f"ids {ids}")
    with torch.no_grad():
        m.emotion_decoder.emotion_queries.add_(0.25)
    _same(_keep(stat.eval_store(FULL[1])), _keep(plain.eval_store(FULL[1])), "after an in-place edit")
    stat.release_graph()
    plain.release_graph()
    # a whole split through train.evaluate_store with a stationary step
    results = []
    for stationary in (False, True):
        stats = EpochStats(NE, 32)
        es = H.EvalStep(m, store_loss, stats=stats, stationary=stationary)
        evaluate_store(m, store, [FULL[0], FULL[1], [3, 11]], store_loss, stats, step=es)
        results.append(stats.result())
        es.release_graph()
    _equal_values(results[1], results[0], "evaluate_store")


def test_the_mosei_wrapper_and_the_classifier(H):
    """audio_proj / text_proj (widths 74 / 300, K-padded shadows) and a model without a decoder: no prologue"""
    import functools
    import test_gpu_classifier_steps as C
    from hri_emo_amd.train import mosei_step_loss
    _tail(True)
    loss_fn = functools.partial(mosei_step_loss, beta_entropy=0.01)
    batches = _make(74, 300, 5)
    torch.manual_seed(3)
    m = H.MoseiFusionWithEmotionDecoder(d_audio=74, d_text=300, d_model=D, num_emotions=NE, n_heads=8, dropout=0.2).cuda().train()
    plain, stat = _pair(H, m, loss_fn, batches[0])
    assert stat._weights.decoder is m.backbone.emotion_decoder and stat._weights.records[0].out is not None
    for i, b in enumerate((batches[0], batches[1], _head(batches[0], 2))):
        got = _keep(stat.eval_packed(*b))
        _same(got, _keep(plain.eval_packed(*b)), f"mosei batch {i}")
        _close(got, _eager(m, b, loss_fn), f"mosei batch {i}")
    with torch.no_grad():
        m.audio_proj.weight.mul_(0.9)
    _same(_keep(stat.eval_packed(*batches[0])), _keep(plain.eval_packed(*batches[0])), "mosei after audio_proj moved")
    stat.release_graph()
    plain.release_graph()
    clf = C._model(H)
    rag = [r for _, r in C._batches()]
    plain, stat = H.EvalStep(clf, C._loss), H.EvalStep(clf, C._loss, stationary=True)
    plain.capture_packed(*rag[0], pad_to=C.PAD)
    stat.capture_packed(*rag[0], pad_to=C.PAD)
    assert stat._weights.decoder is None and stat._weights.records[0].out is None
    for i, b in enumerate((rag[0], rag[1], C._head(rag[0], 3))):
        _same(_keep(stat.eval_packed(*b)), _keep(plain.eval_packed(*b)), f"classifier batch {i}")
    with torch.no_grad():
        clf.classifier[1].weight.mul_(1.1)
    _same(_keep(stat.eval_packed(*rag[0])), _keep(plain.eval_packed(*rag[0])), "classifier after its head moved")
    stat.release_graph()
    plain.release_graph()


# ----------------------------------------------------------------------------- 7. guards and ownership
def test_a_parameter_that_moved_to_other_memory_is_refused(H):
    """DeviceAdamW built after the capture re-homes every p.data: RuntimeError naming the re-capture, nothing enqueued, the static
    state unchanged; a new capture serves again"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    m = _model(H)
    b0, b1 = _batches()
    stat = H.EvalStep(m, _loss(), stationary=True)
    stat.capture_packed(*b0, pad_to=PAD)
    before_out = _keep(stat.eval_packed(*b0))
    front = stat._pb.front
    state = lambda: [t.clone() for t in (stat._static[0], stat._static[1], stat._static[4], front.lens.dev, front.lens.host, front.ctl.dev,    # noqa: E731
                                         front.ctl.host, stat._pb.cu_a, stat._pb.cu_t, stat._pb.cu_f) + front.masks]
    torch.cuda.synchronize()
    before = state()
    ptr = m.emotion_decoder.emotion_queries.data_ptr()
    dp = DataParallelStep(m, _loss(), overlap=False)
    DeviceAdamW(dp.buckets, lr=1e-3)
    assert m.emotion_decoder.emotion_queries.data_ptr() != ptr, "the optimizer did not re-home the parameters: this case tests nothing"
    for args in (b1, b0):
        with pytest.raises(RuntimeError, match="capture again"):
            stat.eval_packed(*args)
    torch.cuda.synchronize()
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    assert len(stat._pb.graphs) == 1, "nothing was captured on the old pointers"
    stat.capture_packed(*b0, pad_to=PAD)
    got = _keep(stat.eval_packed(*b0))
    _same(got, before_out, "captured again on the re-homed parameters")
    stat.release_graph()


def test_the_weights_pass_is_owned_released_and_counted(H):
    from hri_emo_amd import _ops
    m = _model(H)
    b0, b1 = _batches()
    alive0 = _ops.GRAPHS_ALIVE
    stat = H.EvalStep(m, _loss(), stationary=True)
    stat.capture_packed(*b0, pad_to=PAD)
    assert _ops.GRAPHS_ALIVE == alive0 + 2 == alive0 + len(stat._pb.graphs) + len(stat._weights.records)
    stat.eval_packed(*b1)
    assert _ops.GRAPHS_ALIVE == alive0 + 3
    graph = weakref.ref(stat._weights.records[0].graph)
    handed = weakref.ref(stat._weights.records[0].out[0])
    graphed = _keep(stat.eval_packed(*b1))
    stat.use_graph(False)
    _close(_keep(stat.eval_packed(*b1)), _eager(m, b1), "use_graph(False)")
    _close(graphed, _eager(m, b1), "the replay")
    assert stat.ctx.prologue is None and not stat.ctx.stationary
    stat.use_graph(True)
    stat.capture_packed(*b0, pad_to=PAD)          # a re-capture replaces the weights pass with the bucket graphs
    assert _ops.GRAPHS_ALIVE == alive0 + 2
    gc.collect()
    assert graph() is None and handed() is None, "the replaced weights pass is still alive"
    graph = weakref.ref(stat._weights.records[0].graph)
    stat.release_graph()
    assert _ops.GRAPHS_ALIVE == alive0 and not stat.captured and stat._weights is None
    gc.collect()
    assert graph() is None, "release_graph() left the weights pass alive"
    with pytest.raises(RuntimeError, match="capture_packed"):
        stat.eval_packed(*b0)
