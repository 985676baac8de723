"""GPU suite of the store front door of the captured steps: DataParallelStep.capture_store / step_store and EvalStep.capture_store /
eval_store (a batch is a list of utterance ids of a data.DeviceFeatureStore, gathered by hriemo_gather_rows in front of the replay)
against capture_packed / step_packed / eval_packed fed with ``store.fetch(ids)`` -- the same graphs on the same static bytes, so
everything is torch.equal.  Shapes: those of test_gpu_step_packed.py (d128: B = 5, pad_to = (70, 40), bucket granule 8 rows), plus
the MOSEI wrapper at widths 74 / 300."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, NE, NB, TA, TT = 128, 4, 5, 70, 40
LA = [70, 33, 32, 1, 17, 12, 70, 5, 40, 9, 70, 3]
LT = [40, 1, 32, 31, 16, 8, 40, 3, 20, 7, 40, 2]
# row counts 153 / 120 -> bucket (160, 128); 136 / 78 -> (144, 80); 188 / 91 -> (192, 96); 136 / 78 again, in another order
FULL = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [0, 5, 1, 6, 11], [9, 8, 7, 6, 5]]
KEYS = [(160, 128), (144, 80), (192, 96), (144, 80)]


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


def _store(da=D, dt=D):
    """the split of 12 utterances on the GPU (fp32 rows, multi-label targets): built once per width pair, never changed"""
    from hri_emo_amd.data import DeviceFeatureStore
    if (da, dt) not in _CACHE:
        g = torch.Generator().manual_seed(11 + da)
        samples = [(torch.randn(la, da, generator=g), torch.zeros(la, dtype=torch.bool), torch.randn(lt, dt, generator=g),
                    torch.zeros(lt, dtype=torch.bool), (torch.rand(NE, generator=g) < 0.3).float()) for la, lt in zip(LA, LT)]
        _CACHE[(da, dt)] = DeviceFeatureStore.from_samples(samples, "cuda", chunk_bytes=64 << 10)
        _CACHE[("samples", da, dt)] = samples
    return _CACHE[(da, dt)]


def _packed(store, ids):
    """store.fetch(ids) in step_packed's argument order"""
    ra, la, rt, lt, y = store.fetch(ids)
    return ra, rt, la, lt, y


def _model(H, p=0.0, mosei=False):
    torch.manual_seed(3)
    if mosei:
        return H.MoseiFusionWithEmotionDecoder(d_audio=74, d_text=300, d_model=D, num_emotions=NE, n_heads=8, dropout=p).cuda().train()
    return H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=p).cuda().train()


def _loss(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import fusion_step_loss
    return fusion_step_loss(logits, beta, y, n_valid=n_valid)


def _loss2(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import mosei_step_loss
    return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=2, n_valid=n_valid)


def _dp(m, loss=_loss):
    from hri_emo_amd.dp import DataParallelStep
    dp = DataParallelStep(m, loss, overlap=False)
    dp.set_global_batch(NB)
    return dp


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


def _arm(m0, store, batches, by_id, word, loss=_loss, flush=False, **kw):
    """on a copy of m0: capture on batches[0] with DeviceAdamW in the graph, every batch once -> the state after every step
    (loss, flat gradients, parameters, device_step, micro_step), the bucket keys in capture order, what flush_accumulated returned"""
    from hri_emo_amd import _ops
    from hri_emo_amd.optim import DeviceAdamW
    dp = _dp(copy.deepcopy(m0), loss)
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    torch.manual_seed(5)                             # the warm-up and capture passes draw their dropout seeds from torch's generator
    if by_id:
        dp.capture_store(store, batches[0], optimizer=opt, **kw)
    else:
        dp.capture_packed(*_packed(store, batches[0]), pad_to=store.pad_to, optimizer=opt, **kw)
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)              # both arms replay from the same seed word
    out = []
    for ids in batches:
        loss_t = dp.step_store(ids) if by_id else dp.step_packed(*_packed(store, ids))
        torch.cuda.synchronize()
        out.append((loss_t.clone(), dp.buckets.flat.clone(), opt.flat_p.clone(), float(opt.device_step), dp.micro_step))
    flushed = None
    if flush:
        flushed = dp.flush_accumulated()
        torch.cuda.synchronize()
        out.append((torch.zeros(()), dp.buckets.flat.clone(), opt.flat_p.clone(), float(opt.device_step), dp.micro_step))
    keys = list(dp._pb.graphs)
    dp.release_graph()
    return out, keys, flushed


def _assert_equal_arms(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[0].cpu(), y[0].cpu()), (i, "loss", float(x[0]), float(y[0]))
        assert torch.equal(x[1], y[1]), (i, "flat gradients", int((x[1] != y[1]).sum()))
        assert torch.equal(x[2], y[2]), (i, "parameters", int((x[2] != y[2]).sum()))
        assert x[3] == y[3] and x[4] == y[4], (i, "device_step / micro_step", x[3:], y[3:])


# ----------------------------------------------------------------------------- the reference of this suite, checked on its own
@pytest.mark.parametrize("widths", [(D, D), (74, 300)], ids=["d128", "mosei 74/300"])
def test_fetch_on_the_device_equals_the_collate(widths):
    """every other test here compares against store.fetch(ids), which on the GPU runs through the same plan words, pointer
    arithmetic and kernel as step_store.  So fetch itself is held against ground truth that shares none of it: collate_seq_packed of
    the host samples, moved to the device -- audio rows, text rows and targets, n > 1, repeats and a short batch included"""
    from hri_emo_amd.data import collate_seq_packed
    store = _store(*widths)
    samples = _CACHE[("samples",) + widths]
    for ids in FULL + [[5, 6, 7], [11, 11, 0], [8]]:
        got = store.fetch(ids)
        ref = collate_seq_packed([samples[i] for i in ids])
        torch.cuda.synchronize()
        for name, x, y in zip(("rows_a", "lengths_a", "rows_t", "lengths_t", "y"), got, ref):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y), (ids, name)
        assert got[0].is_cuda and got[2].is_cuda and got[4].is_cuda and not got[1].is_cuda and not got[3].is_cuda


# ----------------------------------------------------------------------------- equal steps
@pytest.mark.parametrize("mosei", [False, True], ids=["d128", "mosei 74/300"])
def test_step_store_equals_step_packed_on_the_fetched_batch(H, mosei):
    """two models with equal weights, DeviceAdamW in the graph, dropout 0.1: four batches over three buckets; after every step the
    loss, the flat gradient buffer, the parameters and device_step are torch.equal"""
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    store = _store(74, 300) if mosei else _store()
    assert store.pad_to == (TA, TT) and len(store) == 12
    m0 = _model(H, 0.1, mosei)
    by_id, keys_id, _ = _arm(m0, store, FULL, True, word)
    packed, keys_packed, _ = _arm(m0, store, FULL, False, word)
    assert keys_id == keys_packed == [KEYS[0], KEYS[2], KEYS[1]], keys_id          # LRU order: the bucket of batch 1 came back last
    _assert_equal_arms(by_id, packed)
    assert [s[3] for s in by_id] == [1.0, 2.0, 3.0, 4.0]
    assert bool(torch.isfinite(by_id[-1][2]).all()) and not torch.equal(by_id[0][2], by_id[-1][2])


def test_short_batches_and_accumulation(H):
    """partial_batches=True and grad_accum=2: a full batch, a batch of 1 < n < B, a batch of one, a full batch, and a fifth micro-step
    that flush_accumulated() closes -- alike on both arms after every call"""
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    store = _store()
    batches = [FULL[0], [5, 6, 7], [8], FULL[2], [10, 11]]
    m0 = _model(H, 0.1)
    by_id, keys_id, f_id = _arm(m0, store, batches, True, word, _loss2, flush=True, partial_batches=True, grad_accum=2)
    packed, keys_packed, f_packed = _arm(m0, store, batches, False, word, _loss2, flush=True, partial_batches=True, grad_accum=2)
    assert f_id == f_packed == 1 and keys_id == keys_packed
    _assert_equal_arms(by_id, packed)
    assert [s[3] for s in by_id] == [0.0, 1.0, 1.0, 2.0, 2.0, 3.0] and [s[4] for s in by_id] == [1, 0, 1, 0, 1, 0]


# ----------------------------------------------------------------------------- the graphs are capture_packed's
def test_the_captured_graphs_and_their_launch_lists_are_unchanged(H, monkeypatch):
    """the launches recorded during capture_store are those of capture_packed plus the three gathers of the one load in front;
    a replayed step_store issues hriemo_gather_rows three times and nothing else, and the static state then holds the batch"""
    store = _store()
    m0 = _model(H)
    spy = Spy(monkeypatch)
    a, b = _dp(copy.deepcopy(m0)), _dp(copy.deepcopy(m0))
    a.capture_store(store, FULL[0])
    names_store = spy.take()
    b.capture_packed(*_packed(store, FULL[0]), pad_to=store.pad_to)
    names_packed = [n for n in spy.take() if n != "hriemo_gather_rows"]          # fetch() gathers too
    assert names_store[:3] == ["hriemo_gather_rows"] * 3 and names_store.count("hriemo_gather_rows") == 3
    assert names_store[3:] == names_packed
    a.step_store(FULL[0])
    torch.cuda.synchronize()
    assert spy.take() == ["hriemo_gather_rows"] * 3
    ra, rt, la, lt, y = _packed(store, FULL[3])
    spy.take()
    a.step_store(FULL[1])                            # a new bucket: captured on the spot, one load in front
    first = spy.take()
    assert first[:3] == ["hriemo_gather_rows"] * 3 and first.count("hriemo_gather_rows") == 3
    loss = a.step_store(FULL[3])                     # the same bucket, other ids
    torch.cuda.synchronize()
    assert spy.take() == ["hriemo_gather_rows"] * 3
    key = KEYS[3]
    assert torch.equal(a._static[0][:ra.shape[0]], ra) and not a._static[0][ra.shape[0]:key[0]].any()
    assert torch.equal(a._static[1][:rt.shape[0]], rt) and not a._static[1][rt.shape[0]:key[1]].any()
    assert torch.equal(a._static[4], y) and a._pb.front.lens.dev.tolist() == [la.tolist(), lt.tolist()]
    b.step_packed(ra, rt, la, lt, y)
    torch.cuda.synchronize()
    assert torch.equal(loss, b._pb.graphs[key].loss) and torch.equal(a.buckets.flat, b.buckets.flat)
    a.release_graph()
    b.release_graph()


# ----------------------------------------------------------------------------- refusals
def test_refusals_leave_the_static_state_untouched(H, monkeypatch):
    from hri_emo_amd.data import DeviceFeatureStore
    store = _store()
    dp = _dp(_model(H))
    with pytest.raises(RuntimeError, match="capture_store"):
        dp.step_store(FULL[0])
    with pytest.raises(ValueError, match="outside"):
        dp.capture_store(store, FULL[0], pad_to=(TA, TT - 1))
    with pytest.raises(ValueError):
        dp.capture_store(store, [0, 1, 12])
    assert not dp.captured
    dp.capture_store(store, FULL[0])
    dp.step_store(FULL[0])
    torch.cuda.synchronize()
    front = dp._pb.front
    state = lambda: [t.clone() for t in (dp._static[0], dp._static[1], dp._static[4], front.lens.dev, front.lens.host,      # noqa: E731
                                         dp._feed.block.dev, dp._feed.block.host)]
    before = state()
    spy = Spy(monkeypatch)
    for bad in ([0, 1, 2, 3, 12], [0, 1, 2, 3, -1], [0, 1, 2, 3, 4, 5], [0, 1, 2], []):
        with pytest.raises(ValueError):
            dp.step_store(bad)
    with pytest.raises(RuntimeError, match="captured step"):
        store.append([])
    torch.cuda.synchronize()
    assert spy.take() == []
    for x, y in zip(before, state()):
        assert torch.equal(x, y)
    # a store that was replaced by a longer version of itself after the capture is refused
    g = torch.Generator().manual_seed(2)
    sample = lambda: (torch.randn(4, D, generator=g), torch.zeros(4, dtype=torch.bool), torch.randn(3, D, generator=g),      # noqa: E731
                      torch.zeros(3, dtype=torch.bool), torch.zeros(NE))
    own = DeviceFeatureStore.from_samples([sample() for _ in range(NB)], "cuda")
    dp.capture_store(own, list(range(NB)))
    store.append([])                                  # the shared store is free again (and an empty append changes nothing)
    assert len(store) == 12 and store.version == 1
    dp.release_graph()
    own.append([sample()])
    assert len(own) == NB + 1 and torch.equal(own.fetch([NB])[0].cpu(), own.rows_a[-4:].cpu())
    dp.capture_store(own, list(range(NB)))
    own._holders.clear()                              # what release_graph() does, behind the step's back
    own.append([sample()])
    with pytest.raises(RuntimeError, match="changed"):
        dp.step_store(list(range(NB)))
    dp.release_graph()
    # a capture that fails half way gives the store back: no feed stays behind that would refuse append
    def boom(key):
        raise RuntimeError("capture failed")
    monkeypatch.setattr(dp, "_packed_graph", boom)
    with pytest.raises(RuntimeError, match="capture failed"):
        dp.capture_store(own, list(range(NB)))
    assert dp.store is None and len(own._holders) == 0
    own.append([sample()])
    assert len(own) == NB + 3


# ----------------------------------------------------------------------------- evaluation
def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y, equal_nan=True), (what, k)
        else:
            assert x == y or (x != x and y != y), (what, k, x, y)


def test_eval_store_equals_eval_packed_on_the_fetched_batch(H):
    """three batches, the last one short: outputs, loss, EpochStats.result() and PredictionLog.arrays() equal; evaluate_store gives
    what evaluate_packed gives; use_graph(False) is the eager evaluation of the fetched batch"""
    from hri_emo_amd.train import EpochStats, PredictionLog, evaluate_packed, evaluate_store
    store = _store()
    m = _model(H)
    batches = [FULL[0], FULL[1], [10, 11]]
    sa, la_, sb, lb = EpochStats(NE, 32), PredictionLog(NE, 32), EpochStats(NE, 32), PredictionLog(NE, 32)
    ea, eb = H.EvalStep(m, _loss, stats=sa, log=la_), H.EvalStep(m, _loss, stats=sb, log=lb)
    ea.capture_store(store, batches[0])
    eb.capture_packed(*_packed(store, batches[0]), pad_to=store.pad_to)
    for ids in batches:
        got = ea.eval_store(ids)
        ref = eb.eval_packed(*_packed(store, ids))
        torch.cuda.synchronize()
        for x, y, name in zip(got, ref, ("logits", "beta", "z", "loss")):
            assert x.shape == y.shape and torch.equal(x, y), (ids, name)
        assert got[0].shape[0] == len(ids)
    _same(sa.result(), sb.result(), "EpochStats")
    _same(la_.arrays(), lb.arrays(), "PredictionLog")
    assert sa.result()["n_samples"] == 12 and list(ea._pb.graphs) == list(eb._pb.graphs)
    ea.use_graph(False)
    eb.use_graph(False)
    got, ref = ea.eval_store(batches[2]), eb.eval_packed(*_packed(store, batches[2]))
    torch.cuda.synchronize()
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    ea.release_graph()
    eb.release_graph()
    # the epoch loops: captured on the spot from the first batch
    s1, s2, s3, s4 = (EpochStats(NE, 32) for _ in range(4))
    e1, e2 = H.EvalStep(m, _loss, stats=s1), H.EvalStep(m, _loss, stats=s2)
    fetched = [store.fetch(ids) for ids in batches]
    evaluate_store(m, store, batches, _loss, s1, step=e1)
    evaluate_packed(m, fetched, _loss, s2, pad_to=store.pad_to, step=e2)
    _same(s1.result(), s2.result(), "evaluate_store(step) against evaluate_packed(step)")
    evaluate_store(m, store, batches, _loss, s3)
    evaluate_packed(m, fetched, _loss, s4, pad_to=store.pad_to)
    _same(s3.result(), s4.result(), "evaluate_store against evaluate_packed, eager")
    # a step reads the store it was captured on: handed in with another store it is refused, not run on the wrong split
    other = _store(74, 300)
    assert e1.store is store
    with pytest.raises(ValueError, match="another store"):
        evaluate_store(m, other, batches, _loss, s1, step=e1)
    e1.release_graph()
    e2.release_graph()
    assert e1.store is None


def test_prediction_only_eval_store(H):
    from hri_emo_amd.train import PredictionLog
    store = _store()
    m = _model(H)
    ea, eb = H.EvalStep(m, log=PredictionLog(NE, 16)), H.EvalStep(m, log=PredictionLog(NE, 16))
    ea.capture_store(store, FULL[1])
    assert ea._static[4] is None
    ra, rt, la, lt, _ = _packed(store, FULL[1])
    eb.capture_packed(ra, rt, la, lt, pad_to=store.pad_to)
    ra, rt, la, lt, _ = _packed(store, [3, 4])
    got, ref = ea.eval_store([3, 4]), eb.eval_packed(ra, rt, la, lt)
    torch.cuda.synchronize()
    assert got[3] is None and all(torch.equal(x, y) for x, y in zip(got[:3], ref[:3]))
    _same(ea.log.arrays(), eb.log.arrays(), "PredictionLog")
    ea.release_graph()
    eb.release_graph()


# ----------------------------------------------------------------------------- the eager arm
def test_use_graph_false_is_the_eager_step_packed(H):
    store = _store()
    m0 = _model(H)
    a, b = _dp(copy.deepcopy(m0)), _dp(copy.deepcopy(m0))
    a.capture_store(store, FULL[0])
    b.capture_packed(*_packed(store, FULL[0]), pad_to=store.pad_to)
    a.use_graph(False)
    b.use_graph(False)
    for ids in (FULL[1], [2, 3]):                     # the eager arm takes any n <= B
        torch.manual_seed(9)
        la = a.step_store(ids)
        torch.manual_seed(9)
        lb = b.step_packed(*_packed(store, ids))
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.buckets.flat, b.buckets.flat)
    a.release_graph()
    b.release_graph()
