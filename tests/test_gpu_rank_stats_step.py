"""GPU suite of the ranking metrics and the confusion matrix at the class level: train.EpochStats on the device fed with the `grid`
case of tests/golden/epoch_stats.npz (ranking / pr_curve / roc_curve / per_class_table against sklearn's recorded results), and
EpochStats(kind="single_label", confusion=True) attached to a captured FusionClassifier step_packed and to an EvalStep, at the shapes
of test_gpu_classifier_steps.py (B = 4, d = 128, pad_to = (40, 35)).

Bounds.  The grid case's logits are multiples of 1/8: distinct logits differ in probability by >= 3e-4 and equal ones tie under any
monotonic fp32 sigmoid, so every integer -- and every float64 ratio formed from them -- is the fixture's: 1e-12, the bound of
test_rank_stats_host.py.  The thresholds of the curves are the logged probabilities themselves, 1 / (1 + expf(-x)) on the device
against the fixture's correctly rounded sigmoid: expf within 1 ulp, the addition and the division half an ulp each, the relative
error of e / (1 + e) in e below 1 -- 2 ulp of relative error, up to 4 fp32 steps across a binade edge; the bound
test_gpu_epoch_stats_kernels.py applies to the same expression.  The confusion matrix is compared exactly: the step's own logits
(EvalStep: bit-identical to the eager evaluation; the captured train step: within 1e-5 of the eager pass, and the test asserts that
no eager row has its two largest logits closer than 1e-4, ten times that bound)."""
import copy

import numpy as np
import pytest
import torch

import rank_reference as R
from test_gpu_classifier_steps import H, NB, NC, PAD, _batches, _dp, _head, _loss, _model  # noqa: F401  (H is the fixture)
from test_gpu_step_packed import Spy
from test_rank_stats_host import TOL, check_ranking, check_single_label, close, golden

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- ranking on the device
def _fed_on_the_device(case="grid", n=1000):
    """batches of 64; the last one is short by n_valid (a device word), NaN rows behind its samples"""
    from hri_emo_amd.train import EpochStats
    g, _ = golden()
    st = EpochStats(6, 1000)
    x, y = g[f"{case}_logits"], g[f"{case}_targets"]
    for lo in range(0, n, 64):
        nv = min(64, n - lo)
        xb, yb = torch.full((64, 6), float("nan")), torch.full((64, 6), float("nan"))
        xb[:nv], yb[:nv] = x[lo:lo + nv], y[lo:lo + nv]
        st.update(xb.cuda(), None, yb.cuda(), torch.tensor(0.5, device="cuda"), n_valid=torch.tensor([nv], dtype=torch.int32, device="cuda"))
    return st


def _same_result(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k


def test_ranking_on_the_device_reproduces_sklearn(H, monkeypatch):
    from hri_emo_amd.train import EpochStats
    _, f = golden()
    st = _fed_on_the_device()
    before = st.result()
    spy = Spy(monkeypatch)
    rk = check_ranking(st, "grid", 1000, thr_ulp=4)
    assert spy.take() == ["hriemo_stats_rank", "hriemo_stats_auc"], "ranking(): one launch plus the AUC launch; the curves are host arithmetic"
    _same_result(before, st.result())
    assert rk["macro_auc"] == before["macro_auc"]
    cpu = EpochStats(6, 1000, device="cpu")
    g, _ = golden()
    cpu.update(g["grid_logits"], None, g["grid_targets"], torch.tensor(0.5))
    host = cpu.ranking()
    for k in ("ge_pos", "ge_neg", "truth", "n_pos", "n_neg"):
        assert np.array_equal(rk[k], host[k]), k
    rows = st.per_class_table(["happy", "sad", "anger", "fear", "disgust", "surprise"])
    ap, auc = f["grid_1000_ap"].numpy(), f["grid_1000_auc"].numpy()
    for c, r in enumerate(rows):
        assert list(r) == ["class_", "prevalence", "auc", "auprc", "f1_raw", "f1_cal", "thr"]
        close(r["auprc"], 0.0 if np.isnan(ap[c]) else ap[c], "auprc")
        close(r["auc"], auc[c], "auc")
        assert r["prevalence"] == rk["n_pos"][c] / 1000.0 and r["f1_raw"] == before["per_class_f1"][c] and r["thr"] == float(before["calibrated_thresholds"][c])
    assert abs(np.mean([r["f1_cal"] for r in rows]) - before["macro_f1_calibrated"]) <= TOL
    st.reset()                                               # a shorter epoch in the same buffers: stale ranks must not show
    st.update(g["grid_logits"][:37].cuda(), None, g["grid_targets"][:37].cuda(), torch.tensor(0.5, device="cuda"))
    check_ranking(st, "grid", 37, thr_ulp=4)
    torch.cuda.synchronize()
    assert int(st._rank[:, :, 37:].abs().sum()) == 0


def test_single_label_epoch_on_the_device_reproduces_sklearn(H):
    """the fixture's four-class epoch through update() on the device, the last batch short by n_valid"""
    from hri_emo_amd.train import EpochStats
    _, f = golden()
    x, y = f["sl_logits"], f["sl_labels"]
    st = EpochStats(4, 1, kind="single_label", confusion=True)
    for lo in range(0, 1000, 64):
        nv = min(64, 1000 - lo)
        xb, yb = torch.full((64, 4), float("nan")), torch.full((64,), 9, dtype=torch.int64)
        xb[:nv], yb[:nv] = x[lo:lo + nv], y[lo:lo + nv]
        st.update(xb.cuda(), None, yb.cuda(), torch.tensor(0.5, device="cuda"), n_valid=torch.tensor([nv], dtype=torch.int32, device="cuda"))
    check_single_label(st.result())
    st.update(torch.zeros(2, 4, device="cuda"), None, torch.tensor([1, 4], device="cuda"), torch.tensor(0.5, device="cuda"))
    with pytest.raises(ValueError, match="outside"):
        st.result()
    st.reset()
    assert st.result()["confusion"].sum() == 0 and int(st.cm.abs().sum()) == 0


# ----------------------------------------------------------------------------- the captured steps
def _labelled(rag, ignore=None):
    """the batch with a label replaced by the criterion's ignore_index (a new tuple: the cached batches stay as they are)"""
    if ignore is None:
        return rag
    y = rag[4].clone()
    y[ignore] = -100
    return rag[:4] + (y,)


def _host_matrix(m0, order, eval_mode=False):
    """cm from eager forward_packed passes on a copy of m0; asserts that no row's argmax hangs on less than 1e-4"""
    m = copy.deepcopy(m0)
    m.eval() if eval_mode else m.train()
    cm = np.zeros(NC * NC + 2, dtype=np.int64)
    with torch.no_grad():
        for ra, rt, la, lt, y in order:
            logits = m.forward_packed(ra, rt, la, lt, pad_to=PAD)[0].float().cpu()
            top = logits.topk(2, dim=1).values
            gap = float((top[:, 0] - top[:, 1]).min())
            print(f"smallest gap between the two largest eager logits of a row: {gap:.3e}")
            assert gap > 1e-4, "input condition: the eager argmax is the captured step's"
            cm += R.confusion(logits.numpy(), y.cpu().numpy(), NC)
    return cm


def test_captured_train_step_feeds_the_confusion_matrix(H, monkeypatch):
    """three arms on copies of one model, DeviceAdamW in the graph, partial_batches: no statistics / EpochStats("single_label") /
    the same with confusion=True.  The option adds exactly one launch right behind hriemo_stats_update; warm-up passes leave cm zero;
    losses, flat gradients and parameters are torch.equal in all arms; without the option the launch list is the plain one"""
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import EpochStats
    m0 = _model(H)
    rags = [rag for _, rag in _batches()]
    order = [rags[0], _labelled(rags[1], 2), rags[2], rags[0], _head(rags[1], 3)]
    arms, opts, stats = [], [], [None, EpochStats(NC, 1, kind="single_label"), EpochStats(NC, 1, kind="single_label", confusion=True)]
    spy, names = Spy(monkeypatch), []
    for st in stats:
        dp = _dp(copy.deepcopy(m0))
        opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
        if st is not None:
            dp.attach_stats(st)
        spy.take()
        dp.capture_packed(*rags[0], pad_to=PAD, optimizer=opt, partial_batches=True)
        names.append(spy.take())
        arms.append(dp)
        opts.append(opt)
    base, plain, full = names
    assert plain.count("hriemo_stats_update") == 1 and "hriemo_stats_confusion" not in plain + base
    assert [n for n in plain if n != "hriemo_stats_update"] == base, "without the option: the launch list of the statistics as they were"
    at = full.index("hriemo_stats_update")
    assert full[at + 1] == "hriemo_stats_confusion" and full[:at + 1] + full[at + 2:] == plain, "one more launch, right behind the update"
    torch.cuda.synchronize()
    assert int(stats[2].cm.abs().sum()) == 0 and stats[2].counters.tolist()[:3] == [0, 0, 0], "warm-up and capture passes leave no trace"
    params = [opt.flat_p.clone() for opt in opts]
    assert torch.equal(params[0], params[2])
    for i, rag in enumerate(order):
        out = []
        for dp, opt in zip(arms, opts):
            loss = dp.step_packed(*rag)
            torch.cuda.synchronize()
            out.append((loss.clone(), dp.buckets.flat.clone(), opt.flat_p.clone()))
        for other in out[1:]:
            for a, b, what in zip(out[0], other, ("loss", "flat gradients", "parameters")):
                assert torch.equal(a, b), (i, what)
    assert not torch.equal(params[0], opts[2].flat_p), "the optimizer moved the parameters"
    a, b = stats[1].result(), stats[2].result()
    n = sum(len(r[2]) for r in order)
    assert all(a[k] == b[k] for k in a) and b["n_samples"] == n and b["n_batches"] == len(order)
    assert b["confusion"].sum() == n - 1 and b["n_ignored"] == 1 and b["n_correct"] == int(np.trace(b["confusion"]))
    for dp in arms:
        dp.release_graph()


def test_captured_train_step_confusion_equals_the_eager_logits(H):
    """no optimizer (the weights stay m0's): the matrix of five replays -- three buckets, one short batch, one ignored label -- equals
    the matrix formed on the host from eager forward_packed logits of the same batches; the eager step (use_graph(False)) feeds it too"""
    from hri_emo_amd.train import EpochStats
    m0 = _model(H)
    rags = [rag for _, rag in _batches()]
    order = [rags[0], _labelled(rags[1], 2), rags[2], rags[0], _head(rags[1], 3)]
    want = _host_matrix(m0, order)
    st = EpochStats(NC, 1, kind="single_label", confusion=True)
    dp = _dp(copy.deepcopy(m0))
    dp.attach_stats(st)
    dp.capture_packed(*rags[0], pad_to=PAD, partial_batches=True)
    for rag in order:
        dp.step_packed(*rag)
    res = st.result()
    assert np.array_equal(res["confusion"].reshape(-1), want[:NC * NC]) and res["n_ignored"] == want[NC * NC] == 1
    scores = R.confusion_scores(res["confusion"])
    for k in ("macro_f1", "weighted_f1", "uar"):
        assert abs(res[k] - scores[k]) <= TOL, k
    st.reset()
    dp.use_graph(False)
    for rag in order:
        dp.step_packed(*rag)
    assert np.array_equal(st.result()["confusion"], res["confusion"])
    dp.release_graph()


def test_eval_step_feeds_the_confusion_matrix(H, monkeypatch):
    """EvalStep(stats=EpochStats(confusion=True)): the capture records the confusion launch once, right behind the update, and no
    warm-up pass runs it; three batches (the last one short) give the matrix of the eager evaluation's logits; every other key of
    result() equals the run without the option, whose launch list lacks only that launch"""
    from hri_emo_amd.train import EpochStats, evaluate_packed
    m = _model(H, 0.2)                                           # evaluation runs in eval mode: dropout is off
    rags = [rag for _, rag in _batches()]
    order = [rags[0], _labelled(rags[1], 0), _head(rags[2], 2)]
    want = _host_matrix(m, order, eval_mode=True)
    plain, full = EpochStats(NC, 1, kind="single_label"), EpochStats(NC, 1, kind="single_label", confusion=True)
    first = H.EvalStep(m, _loss)                                 # a model's first capture also creates its bf16 weight forms: not part
    first.capture_packed(*rags[0], pad_to=PAD)                   # of either launch list below
    first.release_graph()
    spy, names, outs = Spy(monkeypatch), [], []
    for st in (plain, full):
        es = H.EvalStep(m, _loss, stats=st)
        spy.take()
        es.capture_packed(*rags[0], pad_to=PAD)
        names.append(spy.take())
        torch.cuda.synchronize()
        assert st.counters.tolist()[:3] == [0, 0, 0] and (st.cm is None or int(st.cm.abs().sum()) == 0), "warm-up passes leave no trace"
        outs.append([[t.clone() for t in es.eval_packed(*rag)] for rag in order])
        es.release_graph()
    assert "hriemo_stats_confusion" not in names[0] and names[1].count("hriemo_stats_confusion") == 1
    at = names[1].index("hriemo_stats_confusion")
    assert names[1][at - 1] == "hriemo_stats_update" and names[1][:at] + names[1][at + 1:] == names[0]
    for a, b in zip(*outs):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "outputs and loss do not depend on the option"
    a, b = plain.result(), full.result()
    assert all(a[k] == b[k] for k in a)
    assert np.array_equal(b["confusion"].reshape(-1), want[:NC * NC]) and b["n_ignored"] == 1 and b["n_samples"] == 2 * NB + 2
    third = EpochStats(NC, 1, kind="single_label", confusion=True)
    evaluate_packed(m, [(ra, la, rt, lt, y) for ra, rt, la, lt, y in order], _loss, third, pad_to=PAD)
    assert np.array_equal(third.result()["confusion"], b["confusion"])
    assert m.training
