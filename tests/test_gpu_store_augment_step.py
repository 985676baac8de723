"""GPU suite of the augmented store front door of the captured trainer step: DataParallelStep.capture_store(..., augment=aug) /
step_store against capture_packed / step_packed fed with ``store.fetch(ids, augment=aug, draw=d)`` -- the same graphs on the same
static bytes, so everything is torch.equal -- plus the draw counter, reproducibility, short batches and accumulation, shard
independence, the classifier, and evaluation, which is never augmented.  Model, store and recipes are those of
test_gpu_store_step.py (d128: B = 5, pad_to = (70, 40), 12 utterances in fp32)."""
import copy

import pytest
import torch

import augment_reference as R
import test_gpu_store_step as S

pytestmark = pytest.mark.gpu

H = S.H                           # the fixture that restores the package's switches
FULL = S.FULL
TM = dict(spans=2, max_width=8, max_frac=0.5)


def _aug(seed=1234):
    from hri_emo_amd.data import StoreAugment
    return StoreAugment(seed, time_mask=TM, noise_std=(0.05, 0.1), modality_drop=(0.2, 0.2))


def _packed(store, ids, aug, draw):
    ra, la, rt, lt, y = store.fetch(ids, augment=aug, draw=draw)
    return ra, rt, la, lt, y


def _arm(m0, store, batches, by_id, word, aug, loss=S._loss, graph=True, **kw):
    """test_gpu_store_step._arm with an augment: by_id -- capture_store(augment=aug) and step_store; otherwise capture_packed and
    step_packed on the batch fetched with the same augment at the draw the other arm uses (aug.draw, advanced by hand here)"""
    from hri_emo_amd import _ops
    from hri_emo_amd.optim import DeviceAdamW
    dp = S._dp(copy.deepcopy(m0), loss)
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    torch.manual_seed(5)
    start = aug.draw
    if by_id:
        dp.capture_store(store, batches[0], optimizer=opt, augment=aug, **kw)
        assert aug.draw == start, "capture_store leaves the draw as it found it"
    else:
        dp.capture_packed(*_packed(store, batches[0], aug, None), pad_to=store.pad_to, optimizer=opt, **kw)
    if not graph:
        dp.use_graph(False)
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    out = []
    for k, ids in enumerate(batches):
        if not graph:
            torch.manual_seed(9 + k)
        if by_id:
            loss_t = dp.step_store(ids)
            assert aug.draw == start + k + 1, "one draw per accepted call"
        else:
            loss_t = dp.step_packed(*_packed(store, ids, aug, start + k))
        torch.cuda.synchronize()
        out.append((loss_t.clone(), dp.buckets.flat.clone(), opt.flat_p.clone(), float(opt.device_step), dp.micro_step))
    dp.release_graph()
    return out


# ----------------------------------------------------------------------------- the reference of this suite, checked on its own
def test_fetch_with_an_augment_equals_the_replica():
    """every other test compares against store.fetch(ids, augment=aug, draw=d); here that is held against the host replica, both
    modalities, and fetch neither advances the draw nor touches the targets"""
    store = S._store()
    aug = _aug()
    aug.draw = 5
    host_a, host_t = store.rows_a.cpu(), store.rows_t.cpu()
    changed = 0
    for ids in FULL + [[5, 6, 7], [11, 11, 0], [8]]:
        for draw in (None, 2):
            ra, la, rt, lt, y = store.fetch(ids, augment=aug, draw=draw)
            pa, _, pt, _, py = store.fetch(ids)
            torch.cuda.synchronize()
            d = 5 if draw is None else draw
            for which, got, host, off, sigma in ((0, ra, host_a, store.offsets_a, 0.05), (1, rt, host_t, store.offsets_t, 0.1)):
                cfg = R.launch_cfg(which, (2, 8, 0.5), sigma, (0.2, 0.2))
                ref = R.apply(host, ids, off, which + 1, cfg, 1234, d)
                assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32)), (ids, draw, which)
            assert torch.equal(y, py) and la.tolist() == [store.lengths_a[i] for i in ids]
            changed += int(not torch.equal(ra, pa)) + int(not torch.equal(rt, pt))
    assert aug.draw == 5 and changed == 28


# ----------------------------------------------------------------------------- equal steps
@pytest.mark.parametrize("graph", [True, False], ids=["captured", "use_graph(False)"])
def test_step_store_with_an_augment_equals_step_packed_on_the_augmented_fetch(H, graph):
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    store = S._store()
    m0 = S._model(H, 0.1)
    a, b = _aug(), _aug()
    a.draw = b.draw = 7
    by_id = _arm(m0, store, FULL, True, word, a, graph=graph)
    packed = _arm(m0, store, FULL, False, word, b, graph=graph)
    S._assert_equal_arms(by_id, packed)
    assert a.draw == 7 + len(FULL) and b.draw == 7
    # and the augment matters: the plain step on the same ids gives another loss
    plain, _, _ = S._arm(m0, store, FULL[:1], True, word)
    assert not torch.equal(plain[0][0].cpu(), by_id[0][0].cpu())


def test_draw_counter_and_refusals(H):
    store = S._store()
    aug = _aug()
    dp = S._dp(S._model(H))
    dp.capture_store(store, FULL[0], augment=aug)
    assert aug.draw == 0 and dp._feed.augment is aug
    dp.step_store(FULL[0])
    dp.step_store(FULL[1])
    assert aug.draw == 2
    for bad in ([0, 1, 2, 3, 12], [0, 1, 2, 3, 4, 5], [0, 1, 2], []):
        with pytest.raises(ValueError):
            dp.step_store(bad)
    assert aug.draw == 2, "a refused call leaves the draw alone"
    dp.use_graph(False)
    with pytest.raises(ValueError):
        dp.step_store([0, 12])
    assert aug.draw == 2
    dp.step_store([2, 3])
    assert aug.draw == 3
    with pytest.raises(TypeError, match="StoreAugment"):
        dp.capture_store(store, FULL[0], augment=dict(seed=1))
    assert dp.captured, "refused before the old step is given up"
    dp.release_graph()


def test_resetting_the_draw_reproduces_a_step(H):
    store = S._store()
    aug = _aug()
    dp = S._dp(S._model(H))
    dp.capture_store(store, FULL[0], augment=aug)
    aug.draw = 40
    rows = []
    for _ in range(2):
        dp.step_store(FULL[0])
        torch.cuda.synchronize()
        rows.append((dp._static[0].clone(), dp._static[1].clone(), dp._pb.graphs[S.KEYS[0]].loss.clone()))
    assert not torch.equal(rows[0][0], rows[1][0]) and not torch.equal(rows[0][1], rows[1][1]), "consecutive steps on the same ids differ"
    aug.draw = 40
    dp.step_store(FULL[0])
    torch.cuda.synchronize()
    assert torch.equal(dp._static[0], rows[0][0]) and torch.equal(dp._static[1], rows[0][1])
    ra, _, rt, _, y = store.fetch(FULL[0], augment=aug, draw=40)
    assert torch.equal(dp._static[0][:ra.shape[0]], ra) and torch.equal(dp._static[1][:rt.shape[0]], rt) and torch.equal(dp._static[4], y)
    assert not dp._static[0][ra.shape[0]:S.KEYS[0][0]].any() and not dp._static[1][rt.shape[0]:S.KEYS[0][1]].any()
    dp.release_graph()


def test_short_batches_and_accumulation(H):
    """partial_batches=True, grad_accum=2: full, short, one utterance, full -- every micro-step a draw of its own, alike on both arms;
    the ghost utterances' rows (behind the batch's own) stay zero"""
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    store = S._store()
    batches = [FULL[0], [5, 6, 7], [8], FULL[2]]
    m0 = S._model(H, 0.1)
    a, b = _aug(), _aug()
    by_id = _arm(m0, store, batches, True, word, a, S._loss2, partial_batches=True, grad_accum=2)
    packed = _arm(m0, store, batches, False, word, b, S._loss2, partial_batches=True, grad_accum=2)
    S._assert_equal_arms(by_id, packed)
    assert a.draw == 4 and [s[3] for s in by_id] == [0.0, 1.0, 1.0, 2.0]
    dp = S._dp(copy.deepcopy(m0), S._loss2)
    dp.capture_store(store, FULL[0], augment=a, partial_batches=True, grad_accum=2)
    dp.step_store([5, 6, 7])
    torch.cuda.synchronize()
    ra, _, rt, _, _ = store.fetch([5, 6, 7], augment=a, draw=4)
    key = max(dp._pb.graphs, key=lambda k: 0 if k == S.KEYS[0] else 1)          # the short batch's bucket
    assert torch.equal(dp._static[0][:ra.shape[0]], ra) and not dp._static[0][ra.shape[0]:key[0]].any()
    assert torch.equal(dp._static[1][:rt.shape[0]], rt) and not dp._static[1][rt.shape[0]:key[1]].any()
    assert a.draw == 5
    dp.release_graph()


def test_shard_independence():
    """the two halves of a batch fetched apart equal the parts of the batch fetched whole: the key is the store id"""
    store = S._store()
    aug = _aug(99)
    ids = [0, 5, 1, 6, 11, 9, 3]
    for k in (1, 3, 6):
        ra, la, rt, lt, _ = store.fetch(ids, augment=aug, draw=6)
        a0, _, t0, _, _ = store.fetch(ids[:k], augment=aug, draw=6)
        a1, _, t1, _, _ = store.fetch(ids[k:], augment=aug, draw=6)
        assert torch.equal(torch.cat([a0, a1]), ra) and torch.equal(torch.cat([t0, t1]), rt)
    other = store.fetch(ids, augment=aug, draw=7)
    assert not torch.equal(other[0], ra) and not torch.equal(other[2], rt)


def test_classifier(H):
    """FusionClassifier goes through the same feed: one captured-vs-eager equality"""
    from hri_emo_amd.data import DeviceFeatureStore
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss_single_label
    g = torch.Generator().manual_seed(23)
    la, lt = [40, 5, 1, 33, 12, 40, 7, 20], [35, 20, 1, 32, 8, 35, 3, 19]
    samples = [(torch.randn(x, S.D, generator=g), torch.zeros(x, dtype=torch.bool), torch.randn(t, S.D, generator=g),
                torch.zeros(t, dtype=torch.bool), int(torch.randint(0, 4, (1,), generator=g))) for x, t in zip(la, lt)]
    store = DeviceFeatureStore.from_samples(samples, "cuda", loss_type="single_label")
    loss = lambda logits, beta, y, n_valid=None: fusion_step_loss_single_label(logits, beta, y, n_valid=n_valid)      # noqa: E731
    torch.manual_seed(3)
    m0 = H.FusionClassifier(S.D, 4, 8, 2, 32, dropout=0.0).cuda().train()
    aug = _aug()
    steps = []
    for _ in range(2):
        dp = DataParallelStep(copy.deepcopy(m0), loss, overlap=False)
        dp.set_global_batch(4)
        steps.append(dp)
    a, b = steps
    a.capture_store(store, [0, 1, 2, 3], augment=aug)
    b.capture_packed(*_packed(store, [0, 1, 2, 3], aug, 0), pad_to=store.pad_to)
    for k, ids in enumerate(([4, 5, 6, 7], [7, 0, 3, 2])):
        la_ = a.step_store(ids)
        lb_ = b.step_packed(*_packed(store, ids, aug, k))
        torch.cuda.synchronize()
        assert torch.equal(la_, lb_) and torch.equal(a.buckets.flat, b.buckets.flat), ids
    assert aug.draw == 2
    a.release_graph()
    b.release_graph()


# ----------------------------------------------------------------------------- evaluation is never augmented
def test_evaluation_is_not_augmented(H):
    store = S._store()
    m = S._model(H)
    aug = _aug()
    ev = H.EvalStep(m, S._loss)
    with pytest.raises(TypeError, match="augment"):
        ev.capture_store(store, FULL[0], augment=aug)
    ev.capture_store(store, FULL[0])
    before = [t.clone() for t in ev.eval_store(FULL[1])]
    dp = S._dp(copy.deepcopy(m))
    dp.capture_store(store, FULL[0], augment=aug)
    dp.step_store(FULL[1])
    after = [t.clone() for t in ev.eval_store(FULL[1])]
    torch.cuda.synchronize()
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert ev._feed.augment is None
    ev.release_graph()
    dp.release_graph()


# ----------------------------------------------------------------------------- no augment: the parent's calls
def test_without_an_augment_the_calls_are_the_plain_gathers(H, monkeypatch):
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    store = S._store()
    m0 = S._model(H, 0.1)
    one, _, _ = S._arm(m0, store, FULL, True, word, augment=None)
    two, _, _ = S._arm(m0, store, FULL, True, word)
    S._assert_equal_arms(one, two)
    spy = S.Spy(monkeypatch)
    dp = S._dp(copy.deepcopy(m0))
    dp.capture_store(store, FULL[0], augment=None)
    names = spy.take()
    assert names.count("hriemo_gather_rows") == 3 and "hriemo_gather_rows_aug" not in names
    dp.step_store(FULL[0])
    store.fetch(FULL[1], augment=None)
    assert spy.take() == ["hriemo_gather_rows"] * 6
    dp.release_graph()
    aug = _aug()
    dp.capture_store(store, FULL[0], augment=aug)
    spy.take()
    dp.step_store(FULL[0])
    assert spy.take() == ["hriemo_gather_rows_aug", "hriemo_gather_rows_aug", "hriemo_gather_rows"]
    dp.release_graph()
