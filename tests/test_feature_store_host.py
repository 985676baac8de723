"""Host suite of data.DeviceFeatureStore on a CPU device (torch indexing in place of the gather kernel): parity with
collate_seq_packed, masks, crop, sanitise, batches, the plan arithmetic against ghost_plan / packed_tables, and the refusals of the
store front door of the captured steps -- each of them before anything is enqueued (counted on _lib.call)."""
import itertools

import pytest
import torch

LA = [1, 2, 17, 64, 3, 1, 40, 9, 33]
LT = [1, 1, 9, 40, 2, 1, 16, 9, 20]
NE = 4


def _samples(dtype=torch.float32, da=12, dt=8, single=False, seed=0, pad_inside=False):
    """reference-dataset items; pad_inside: stored longer than valid, with PAD rows in the MIDDLE and at the end of the stored length"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (la, lt) in enumerate(zip(LA, LT)):
        extra = 3 if pad_inside else 0
        xa, xt = torch.randn(la + extra, da, generator=g).to(dtype), torch.randn(lt + extra, dt, generator=g).to(dtype)
        ka, kt = torch.zeros(la + extra, dtype=torch.bool), torch.zeros(lt + extra, dtype=torch.bool)
        if pad_inside:
            ka[torch.randperm(la + extra, generator=g)[:extra]] = True         # PAD rows anywhere inside the stored length
            kt[-extra:] = True
        y = int(torch.randint(0, NE, (1,), generator=g)) if single else (torch.rand(NE, generator=g) < 0.3).float()
        out.append((xa, ka, xt, kt, y))
    return out


def _store(samples, **kw):
    from hri_emo_amd.data import DeviceFeatureStore
    return DeviceFeatureStore.from_samples(samples, "cpu", **kw)


IDS = [[0], [8], [3, 3, 3], [8, 7, 6, 5, 4, 3, 2, 1, 0], [1, 5], [2, 6, 4]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("single", [False, True], ids=["multi_label", "single_label"])
@pytest.mark.parametrize("pad_inside", [False, True], ids=["all valid", "PAD rows inside"])
def test_fetch_equals_the_collate(dtype, single, pad_inside):
    """from_samples + fetch(ids) == collate_seq_packed on the same samples, bit for bit; with PAD rows inside the stored length the
    mask decides, not the stored length; tiny upload chunks (several per store) change nothing"""
    from hri_emo_amd.data import collate_seq_packed
    samples = _samples(dtype, single=single, pad_inside=pad_inside)
    loss_type = "single_label" if single else "multi_label"
    for chunk in (64 << 20, 256):
        store = _store(samples, loss_type=loss_type, chunk_bytes=chunk)
        assert len(store) == len(samples) and store.dtype == dtype
        assert store.lengths_a == LA and store.lengths_t == LT, "the valid rows, whatever the stored length"
        assert store.offsets_a == list(itertools.accumulate(LA, initial=0)) and store.off_t.tolist() == store.offsets_t
        assert store.pad_to == (max(LA), max(LT))
        assert store.rows_a.shape == (sum(LA), 12) and store.rows_a.dtype == dtype and store.off_a.dtype == torch.int64
        assert store.y.dtype == (torch.int64 if single else torch.float32) and store.y.shape == ((len(LA),) if single else (len(LA), NE))
        assert store.nbytes == sum(t.numel() * t.element_size() for t in (store.rows_a, store.rows_t, store.off_a, store.off_t, store.off_y, store.y))
        for ids in IDS:
            got = store.fetch(ids)
            ref = collate_seq_packed([samples[i] for i in ids], loss_type)
            for a, b, name in zip(got, ref, ("rows_a", "lengths_a", "rows_t", "lengths_t", "y")):
                assert a.dtype == b.dtype and torch.equal(a, b), (ids, name)
            assert got[0].data_ptr() != store.rows_a.data_ptr(), "fresh tensors"


def test_store_dtype_casts_the_rows():
    from hri_emo_amd.data import collate_seq_packed
    samples = _samples(torch.float32)
    store = _store(samples, dtype=torch.bfloat16)
    ref = collate_seq_packed([samples[i] for i in (2, 3)])
    got = store.fetch([2, 3])
    assert got[0].dtype == torch.bfloat16 and torch.equal(got[0], ref[0].bfloat16()) and torch.equal(got[2], ref[2].bfloat16())
    with pytest.raises(ValueError):
        _store(samples, dtype=torch.float64)


def test_crop_is_the_trainers_crop_center():
    """max_len: rows (L - max) // 2 .. + max of the valid rows, for an odd and an even surplus; an utterance exactly at the limit and
    shorter ones are not cropped"""
    samples = _samples()
    ma, mt = 17, 9                                     # audio: 64 (surplus 47, odd), 40 (23, odd), 33 (16, even), 17 (at the limit)
    store = _store(samples, max_len=(ma, mt))          # text: 40 (31, odd), 16 (7, odd), 20 (11, odd), 9 (at the limit)
    assert store.lengths_a == [min(v, ma) for v in LA] and store.lengths_t == [min(v, mt) for v in LT]
    assert store.pad_to == (ma, mt)
    surplus = set()
    for i, (xa, _, xt, _, _) in enumerate(samples):
        ra, _, rt, _, _ = store.fetch([i])
        for x, r, m in ((xa, ra, ma), (xt, rt, mt)):
            if x.shape[0] > m:
                s = (x.shape[0] - m) // 2
                surplus.add((x.shape[0] - m) % 2)
                assert torch.equal(r, x[s:s + m]), i
            else:
                assert torch.equal(r, x), i
    assert surplus == {0, 1}
    assert torch.equal(store.fetch([2])[0], samples[2][0]) and LA[2] == ma, "exactly at the limit: untouched"
    with pytest.raises(ValueError):
        _store(samples, max_len=(0, 4))


def test_sanitise():
    samples = _samples()
    xa = samples[2][0].clone()
    xa[0, 0], xa[3, 1], xa[5, 2] = float("nan"), float("inf"), float("-inf")
    samples[2] = (xa,) + samples[2][1:]
    got = _store(samples).fetch([2])[0]
    ref = xa.clone()
    ref[0, 0] = ref[3, 1] = ref[5, 2] = 0.0
    assert torch.equal(got, ref) and bool(torch.isfinite(got).all())
    raw = _store(samples, sanitize=False).fetch([2])[0]
    assert torch.isnan(raw[0, 0]) and raw[3, 1] == float("inf") and raw[5, 2] == float("-inf")


@pytest.mark.parametrize("bucket_mult", [50, 1, 0])
@pytest.mark.parametrize("shuffle", [True, False])
def test_batches_cover_every_id_once(bucket_mult, shuffle):
    store = _store(_samples())
    g = torch.Generator().manual_seed(1)
    batches = store.batches(4, shuffle=shuffle, generator=g, bucket_mult=bucket_mult)
    assert sorted(i for b in batches for i in b) == list(range(len(store)))
    assert sorted(len(b) for b in batches) == [1, 4, 4], "the short last batch is kept"
    if not shuffle and bucket_mult == 0:
        assert batches == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]
    if bucket_mult == 50:
        from hri_emo_amd.data import length_bucketed_batches
        assert batches == length_bucketed_batches(LA, 4, shuffle, torch.Generator().manual_seed(1), 50)


@pytest.mark.parametrize("ids", [[3, 0, 6, 2, 8], [5, 1], [4], [7, 7, 7]], ids=["full", "two", "one", "repeats"])
def test_plan_arithmetic_equals_ghost_plan_and_packed_tables(ids):
    """the plan block the host writes for a batch of n <= B ids: per operand {ids, dst_cu}, dst_cu = the first n + 1 entries of
    packed_tables' cu_seqlens for the batch completed with ghosts; the bucket key the step picks is ghost_plan's"""
    from hri_emo_amd import dp
    store = _store(_samples())
    B, (La, Lt) = 5, store.pad_to
    feed = dp._StoreFeed(store, B, (La, Lt), "cpu")
    got_ids, la, lt = feed.batch(ids, True, "test")
    n = len(ids)
    assert got_ids == ids and la == [LA[i] for i in ids] and lt == [LT[i] for i in ids]
    gla, glt, key, own = dp.ghost_plan(la, lt, B, La, Lt)
    assert gla[n:] == [1] * (B - n) and own == (sum(la), sum(lt))
    tkey, cu_a, cu_t, _ = dp.packed_tables(gla, glt, B, La, Lt)
    assert tkey == key
    words = store.plan_words(ids, feed.stride)
    assert len(words) == 3 * feed.stride == feed.block.host.numel()
    for p, cu in enumerate((cu_a[:n + 1], cu_t[:n + 1], list(range(n + 1)))):
        plan = words[p * feed.stride:(p + 1) * feed.stride]
        assert plan[:n] == ids and plan[n:2 * n + 1] == cu and not any(plan[2 * n + 1:]), p
    assert cu_a[n] == own[0] <= key[0] and cu_t[n] == own[1] <= key[1], "the zero tail runs from the own rows to the bucket's end"
    # what _load_ragged hands the fill: the same key and own rows
    seen = []
    pb = dp._PackedState(B, La, Lt, "cpu", dp._RaggedFront(_Block(), (), True, partial=True, accum=1, ctl=_Block()))
    assert dp._load_ragged(pb, [None] * 5, lambda static, n_utt, own_, key_: seen.append((n_utt, own_, key_)), la, lt) == key
    assert seen == [(n, own, key)]
    assert pb.front.lens.up == [[gla, glt]] and pb.front.ctl.up == [dp.ctl_words(n, 1, 1)]
    with pytest.raises(ValueError):
        store.plan_words(ids, 2 * n)


class _Block:
    def __init__(self):
        self.up = []

    def upload(self, values):
        self.up.append(values)


class _Calls:
    def __init__(self, monkeypatch):
        from hri_emo_amd import _lib
        self.n = 0

        def spy(name, *args):
            self.n += 1
            raise AssertionError(f"{name} enqueued")

        monkeypatch.setattr(_lib, "call", spy)


def _fake_graph(step, store, B, partial):
    """make `step` (built by its own constructor, on the CPU) count as captured on `store`: a packed state with one bucket graph that
    replays nothing, blocks that record their uploads, and the store's feed -- its device work would be _lib.calls: none may happen"""
    import types
    from hri_emo_amd import dp
    La, Lt = store.pad_to
    step._static = [torch.zeros(8, 12), torch.zeros(8, 8), None, None, torch.zeros(B, NE)]
    step._pb = dp._PackedState(B, La, Lt, "cpu", dp._RaggedFront(_Block(), (), False, partial=partial, accum=1, ctl=_Block()))
    step._pb.graphs[(8, 8)] = dp._GraphRecord(types.SimpleNamespace(replay=lambda: None), torch.zeros(()), [])
    step._feed = dp._StoreFeed(store, B, (La, Lt), "cpu")
    return step


def _cpu_step(store, B, partial):
    from hri_emo_amd import dp
    return _fake_graph(dp.DataParallelStep(torch.nn.Linear(2, 2), lambda logits, beta, y, n_valid=None: 0, overlap=False), store, B, partial)


def test_a_step_reads_the_store_it_was_captured_on(monkeypatch):
    """step_store / eval_store take ids only: they refer to the captured store (step.store).  evaluate_store refuses a step that was
    captured on another store -- or by capture_packed -- before anything runs, instead of evaluating the wrong split"""
    from hri_emo_amd import dp, train
    val, test = _store(_samples()), _store(_samples(seed=3))
    calls = _Calls(monkeypatch)
    model, loss = torch.nn.Linear(2, 2), (lambda logits, beta, y, n_valid=None: 0)
    es = dp.EvalStep(model, loss)
    assert es.store is None and _cpu_step(val, 4, True).store is val
    _fake_graph(es, val, 4, True)
    assert es.captured and es.store is val
    with pytest.raises(ValueError, match="another store"):
        train.evaluate_store(model, test, [[0, 1]], loss, None, step=es)
    es._feed.close()
    es._feed = None                                            # the same graphs after capture_packed: no store at all
    with pytest.raises(ValueError, match="capture_packed"):
        train.evaluate_store(model, val, [[0, 1]], loss, None, step=es)
    assert calls.n == 0 and es._pb.front.lens.up == []


def test_refusals_come_before_anything_is_enqueued(monkeypatch):
    from hri_emo_amd import dp
    store = _store(_samples())
    calls = _Calls(monkeypatch)
    N = len(store)
    for bad in ([N], [-1], [0, N, 1], []):
        with pytest.raises(ValueError):
            store.fetch(bad)
        with pytest.raises(ValueError):
            store.check_ids(bad)
    s = _cpu_step(store, 4, partial=True)
    for bad in ([N], [-1], [0, 1, 2, 3, 4]):                  # an id at len(store), a negative id, n > B
        with pytest.raises(ValueError):
            s.step_store(bad)
    strict = _cpu_step(store, 4, partial=False)
    with pytest.raises(ValueError, match="B = 4"):
        strict.step_store([0, 1])
    short = dp._StoreFeed(store, 4, (16, 9), "cpu")           # pad_to shorter than utterance 3
    with pytest.raises(ValueError, match="outside"):
        short.batch([3], True, "test")
    short.close()
    # the store is held by the captured steps: no append
    with pytest.raises(RuntimeError, match="captured step"):
        store.append(_samples(seed=1)[:2])
    assert len(store) == N and store.version == 1
    # released: it grows, ids continue, and a step captured on the old version refuses it
    strict._feed.close()
    s._feed.close()
    store.append(_samples(seed=1)[:2])
    assert len(store) == N + 2 and store.version == 2 and store.lengths_a == LA + LA[:2] and store.off_y.tolist() == list(range(N + 3))
    assert torch.equal(store.fetch([N + 1])[0], _samples(seed=1)[1][0])
    with pytest.raises(RuntimeError, match="changed"):
        s.step_store([0, 1])
    # no capture_store: step_store / eval_store have nothing to read
    fresh = dp.DataParallelStep(torch.nn.Linear(2, 2), lambda logits, beta, y, n_valid=None: 0, overlap=False)
    with pytest.raises(RuntimeError, match="capture_store"):
        fresh.step_store([0])
    ev = dp.EvalStep(torch.nn.Linear(2, 2))
    with pytest.raises(RuntimeError, match="capture_store"):
        ev.eval_store([0])
    with pytest.raises(TypeError):
        ev.capture_store(store, [0])                           # no forward_packed entry
    assert calls.n == 0, "a refusal enqueues nothing"
    assert s._pb.front.lens.up == [] and strict._pb.front.lens.up == [], "and uploads nothing"


def test_gather_entry_in_header_and_binding():
    import os
    from hri_emo_amd import _lib
    assert _lib._SIGS["hriemo_gather_rows"] == ("plppiplp", "i")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "hriemo.h")).read()
    assert "int hriemo_gather_rows(const void* store, long row_bytes, const long long* offsets, const int* plan, int n, void* dst, long dst_rows," in header
