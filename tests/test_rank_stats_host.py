"""CPU suite of the ranking metrics and the single-label confusion statistics of train.EpochStats (the CPU path: the kernels'
definitions in numpy) against sklearn's results recorded in tests/golden/rank_stats.npz and against tests/rank_reference.py, for every
case, prefix and class of tests/golden/epoch_stats.npz.  Integers are compared exactly; floats at 1e-12, the project's bound for
float64 ratios of exact integers formed on the host (measured here: 2.2e-16)."""
import math

import numpy as np
import pytest
import torch

import rank_reference as R
from conftest import load_golden

TOL = 1e-12
NS = (1, 37, 64, 255, 256, 257, 301, 1000)
CURVE_NS = (301, 1000)
_G = {}


def golden():
    if not _G:
        _G["in"], _G["out"] = load_golden("epoch_stats"), load_golden("rank_stats")
        assert tuple(_G["in"]["ns"].tolist()) == NS == tuple(_G["out"]["ns"].tolist()) and tuple(_G["out"]["curve_ns"].tolist()) == CURVE_NS
        assert bytes(_G["out"]["sklearn_version"].numpy()).decode().count(".") >= 1
    return _G["in"], _G["out"]


def fed(case, n, device="cpu", batch=64):
    """an EpochStats holding the first n samples of a case, fed in batches of 64 whose last one is short by n_valid"""
    from hri_emo_amd.train import EpochStats
    g, _ = golden()
    st = EpochStats(6, 1000, device=device)
    x, y = g[f"{case}_logits"], g[f"{case}_targets"]
    for lo in range(0, n, batch):
        nv = min(batch, n - lo)
        st.update(x[lo:lo + batch], None, y[lo:lo + batch], torch.tensor(0.5), n_valid=None if nv == x[lo:lo + batch].shape[0] else nv)
    return st


def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "nan pattern")
    ok = ~np.isnan(a)
    worst = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
    assert worst <= TOL, (what, worst)
    return worst


def same_thresholds(got, want, ulp, what):
    """thresholds against the fixture's: equal, or -- where the log holds another fp32 sigmoid's bits -- within `ulp` fp32 steps"""
    want = np.asarray(want, dtype=got.dtype)
    assert got.shape == want.shape and np.array_equal(np.isinf(got), np.isinf(want)), what
    a, b = got[~np.isinf(got)].astype(np.float32), want[~np.isinf(want)].astype(np.float32)
    worst = int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0
    assert worst <= ulp, (what, worst, f"THRESHOLDS only: fp32 probabilities, {ulp} ulp; every integer stays exact and every ratio at {TOL}")


def check_ranking(st, case, n, thr_ulp=0):
    """every check of one (case, prefix): shared with the GPU suite, which feeds the same logits on the device (thr_ulp: how far the
    logged probabilities, and with them the curves' thresholds, may lie from the fixture's correctly rounded sigmoid)"""
    _, f = golden()
    rk = st.ranking()
    C = 6
    assert rk["n_logged"] == n and rk["ge_pos"].shape == rk["ge_neg"].shape == rk["probs"].shape == rk["truth"].shape == (C, n)
    assert rk["ge_pos"].dtype == rk["ge_neg"].dtype == np.int64 and rk["probs"].dtype == np.float32 and rk["truth"].dtype == bool
    ap_want, auc_want = f[f"{case}_{n}_ap"].numpy(), f[f"{case}_{n}_auc"].numpy()
    worst = 0.0
    for c in range(C):
        p, t = rk["probs"][c], rk["truth"][c]
        gp, gn = R.ge_counts(p, t)
        assert np.array_equal(rk["ge_pos"][c], gp) and np.array_equal(rk["ge_neg"][c], gn), (case, n, c)
        assert (rk["n_pos"][c], rk["n_neg"][c]) == (int(t.sum()), int((~t).sum()))
        want = 0.0 if math.isnan(ap_want[c]) else float(ap_want[c])           # sklearn has no value without a positive: 0.0 as stated
        worst = max(worst, close(rk["average_precision"][c], want, (case, n, c, "ap")), close(rk["average_precision"][c], R.average_precision(p, t), "ap ref"))
        worst = max(worst, close(rk["per_class_auc"][c], auc_want[c], (case, n, c, "auc")), close(rk["per_class_auc"][c], R.auc(p, t), "auc ref"))
        if rk["n_pos"][c] == 0:
            with pytest.raises(ValueError, match="no positive"):
                st.pr_curve(c, rk)
        if rk["n_pos"][c] == 0 or rk["n_neg"][c] == 0:
            with pytest.raises(ValueError, match="both kinds"):
                st.roc_curve(c, rk)
        if rk["n_pos"][c] > 0:
            got, ref = st.pr_curve(c, rk), R.pr_curve(p, t)
            assert got[2].dtype == np.float32 and np.array_equal(got[2], ref[2])
            worst = max(worst, close(got[0], ref[0], "precision ref"), close(got[1], ref[1], "recall ref"))
            k = f"{case}_{n}_c{c}_pr_"
            if n in CURVE_NS:
                same_thresholds(got[2], f[k + "thresholds"].numpy(), thr_ulp, k)
                worst = max(worst, close(got[0], f[k + "precision"].numpy(), k), close(got[1], f[k + "recall"].numpy(), k))
        if rk["n_pos"][c] > 0 and rk["n_neg"][c] > 0:
            got, ref = st.roc_curve(c, rk), R.roc_curve(p, t)
            assert np.isinf(got[2][0]) and got[0][0] == got[1][0] == 0.0 and np.array_equal(got[2], ref[2])
            worst = max(worst, close(got[0], ref[0], "fpr ref"), close(got[1], ref[1], "tpr ref"))
            k = f"{case}_{n}_c{c}_roc_"
            if n in CURVE_NS:
                same_thresholds(got[2], f[k + "thresholds"].numpy(), thr_ulp, k)
                worst = max(worst, close(got[0], f[k + "fpr"].numpy(), k), close(got[1], f[k + "tpr"].numpy(), k))
    has = rk["n_pos"] > 0
    assert abs(rk["macro_ap"] - (float(rk["average_precision"][has].mean()) if has.any() else 0.0)) <= TOL
    print(f"{case} n = {n}: largest float difference {worst:.3g}")
    return rk


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("case", ["cont", "grid"])
def test_ranking_and_curves_reproduce_sklearn(case, n):
    st = fed(case, n)
    before = st.result()
    rk = check_ranking(st, case, n)
    after = st.result()
    assert rk["macro_auc"] == before["macro_auc"] == after["macro_auc"]
    assert np.array_equal(rk["n_pos"], before["n_pos"]) and np.array_equal(rk["n_neg"], before["n_neg"])
    if rk["n_pos"][0] > 0:
        assert np.array_equal(st.pr_curve(0)[0], st.pr_curve(0, rk)[0]), "without a ranking handed in, one is taken"


def test_classes_without_a_kind_and_all_tied():
    """grid: class 3 has no positive (AP 0.0, AUC nan, both curves refused), class 4 no negative (AP 1.0, precision 1 everywhere, ROC
    refused), every probability of class 5 ties (one distinct threshold: AP = precision = prevalence, AUC 0.5)"""
    st = fed("grid", 1000)
    rk = st.ranking()
    assert rk["n_pos"][3] == 0 and rk["average_precision"][3] == 0.0 and math.isnan(rk["per_class_auc"][3])
    assert (rk["ge_pos"][3] == 0).all() and rk["ge_neg"][3].min() >= 1
    for fn in (st.pr_curve, st.roc_curve):
        with pytest.raises(ValueError):
            fn(3, rk)
    assert rk["n_neg"][4] == 0 and rk["average_precision"][4] == 1.0 and math.isnan(rk["per_class_auc"][4])
    precision, recall, thr = st.pr_curve(4, rk)
    assert (precision == 1.0).all() and recall[0] == 1.0 and recall[-1] == 0.0 and (rk["ge_neg"][4] == 0).all()
    with pytest.raises(ValueError, match="both kinds"):
        st.roc_curve(4, rk)
    prevalence = rk["n_pos"][5] / 1000.0
    precision, recall, thr = st.pr_curve(5, rk)
    assert thr.shape == (1,) and precision.tolist() == [prevalence, 1.0] and recall.tolist() == [1.0, 0.0]
    assert abs(rk["average_precision"][5] - prevalence) <= TOL and rk["per_class_auc"][5] == 0.5
    assert (rk["ge_pos"][5] == rk["n_pos"][5]).all() and (rk["ge_neg"][5] == rk["n_neg"][5]).all()
    fpr, tpr, thr = st.roc_curve(5, rk)
    assert fpr.tolist() == [0.0, 1.0] and tpr.tolist() == [0.0, 1.0] and np.isinf(thr[0])
    both = ~np.isnan(rk["per_class_auc"])
    assert abs(rk["macro_auc"] - rk["per_class_auc"][both].mean()) <= TOL and abs(rk["macro_ap"] - rk["average_precision"][[0, 1, 2, 4, 5]].mean()) <= TOL


def test_per_class_table_has_the_reference_columns():
    _, f = golden()
    st = fed("cont", 1000)
    names = ["happy", "sad", "anger", "fear", "disgust", "surprise"]
    rows = st.per_class_table(names)
    res, rk = st.result(), st.ranking()
    assert [r["class_"] for r in rows] == names and len(rows) == 6
    f1_cal = []
    for c, r in enumerate(rows):
        assert list(r) == ["class_", "prevalence", "auc", "auprc", "f1_raw", "f1_cal", "thr"]
        assert r["prevalence"] == rk["n_pos"][c] / 1000.0 and r["f1_raw"] == res["per_class_f1"][c] and r["thr"] == float(res["calibrated_thresholds"][c])
        want_ap, want_auc = f["cont_1000_ap"].numpy()[c], f["cont_1000_auc"].numpy()[c]
        close(r["auprc"], 0.0 if math.isnan(want_ap) else want_ap, "auprc")
        close(r["auc"], want_auc, "auc")
        sw = res["sweep_counts"][c]
        at = int(np.flatnonzero(np.linspace(0.05, 0.95, 19).astype(np.float32) == res["calibrated_thresholds"][c])[0])
        den = 2 * sw[at, 0] + sw[at, 1] + sw[at, 2]
        assert r["f1_cal"] == (2.0 * sw[at, 0] / den if den else 0.0), "the sweep's F1 at the chosen grid point"
        f1_cal.append(r["f1_cal"])
    assert abs(np.mean(f1_cal) - res["macro_f1_calibrated"]) <= TOL
    assert [r["class_"] for r in st.per_class_table()] == [str(c) for c in range(6)]
    with pytest.raises(ValueError, match="names"):
        st.per_class_table(names[:5])


def test_ranking_takes_the_refusals_of_result():
    from hri_emo_amd.train import EpochStats
    st = EpochStats(2, 4, device="cpu")
    st.update(torch.zeros(3, 2), None, torch.ones(3, 2), torch.tensor(1.0))
    st.update(torch.zeros(3, 2), None, torch.ones(3, 2), torch.tensor(1.0))
    with pytest.raises(RuntimeError, match="overflowed"):
        st.ranking()
    st = EpochStats(2, 4, device="cpu")
    st.update(torch.tensor([[0.0, float("nan")]]), None, torch.ones(1, 2), torch.tensor(1.0))
    with pytest.raises(ValueError, match="non-finite"):
        st.ranking()
    with pytest.raises(ValueError, match="multi_label"):
        EpochStats(4, 4, kind="single_label", device="cpu").ranking()
    empty = EpochStats(2, 4, device="cpu").ranking()
    assert empty["ge_pos"].shape == (2, 0) and empty["macro_ap"] == 0.0 and empty["macro_auc"] == 0.0


# ----------------------------------------------------------------------------- single-label: the confusion matrix
def test_confusion_is_refused_for_the_multi_label_kind():
    from hri_emo_amd.train import EpochStats
    with pytest.raises(ValueError, match="single_label"):
        EpochStats(6, 8, kind="multi_label", confusion=True, device="cpu")
    with pytest.raises(ValueError, match="at most 64"):
        EpochStats(65, 8, kind="single_label", confusion=True, device="cpu")
    plain = EpochStats(4, 8, kind="single_label", device="cpu")
    plain.update(torch.zeros(2, 4), None, torch.tensor([0, 1]), torch.tensor(1.0))
    assert plain.cm is None and set(plain.result()) == {"n_samples", "n_batches", "n_skipped", "n_correct", "avg_loss", "accuracy", "mean_beta"}


def check_single_label(res):
    """result() of the fixture's single-label epoch against sklearn's recorded values and the reference; shared with the GPU suite"""
    _, f = golden()
    m = res["confusion"]
    assert m.dtype == np.int64 and np.array_equal(m, f["sl_confusion"].numpy()) and res["n_ignored"] == int(f["sl_n_ignored"]) == 11
    assert (m[:, 2] == 0).all() and m[2].sum() > 0, "class 2 is never predicted"
    ref = R.confusion_scores(m)
    for k in ("macro_f1", "weighted_f1", "uar"):
        assert abs(res[k] - float(f["sl_" + k])) <= TOL and abs(res[k] - ref[k]) <= TOL, k
    for k in ("per_class_f1", "per_class_recall"):
        close(res[k], f["sl_" + k].numpy(), k)
        close(res[k], ref[k], k)
    assert abs(np.trace(m) / m.sum() - float(f["sl_accuracy"])) <= TOL
    assert res["n_correct"] == int(np.trace(m)) and res["n_samples"] == 1000 and abs(res["accuracy"] - np.trace(m) / 1000.0) <= TOL


def test_single_label_confusion_reproduces_sklearn():
    from hri_emo_amd.train import EpochStats
    _, f = golden()
    x, y = f["sl_logits"], f["sl_labels"]
    st = EpochStats(4, 1, kind="single_label", confusion=True, device="cpu")
    for lo in range(0, 1000, 64):
        xb, yb = x[lo:lo + 64], y[lo:lo + 64]
        st.update(xb, None, yb, torch.tensor(0.5))
    res = st.result()
    check_single_label(res)
    assert np.array_equal(np.concatenate([res["confusion"].reshape(-1), [res["n_ignored"], 0]]), R.confusion(x.numpy(), y.numpy(), 4))
    st.reset()
    again = st.result()
    assert again["confusion"].sum() == 0 and again["n_ignored"] == 0 and again["macro_f1"] == 0.0 and again["uar"] == 0.0 and again["weighted_f1"] == 0.0


def test_single_label_confusion_edge_rules():
    """n_valid cuts the batch (NaN rows behind it), a NaN logit counts as maximal, ties take the first index, a skipped batch leaves no
    trace, a label outside [0, C) that is not -100 makes result() raise"""
    from hri_emo_amd.train import EpochStats
    nan = float("nan")
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, nan, 5.0, nan], [7.0, 1.0, 0.0, 7.0], [nan, nan, nan, nan]])
    y = torch.tensor([1, 0, 1, 3, 7])
    st = EpochStats(4, 1, kind="single_label", skip_nonfinite=True, confusion=True, device="cpu")
    st.update(x, None, y, torch.tensor(1.0), n_valid=4)
    st.update(x, None, y, torch.tensor(nan), n_valid=4)
    res = st.result()
    want = np.zeros((4, 4), dtype=np.int64)
    want[1, 1], want[0, 0], want[3, 0] = 2, 1, 1
    assert np.array_equal(res["confusion"], want) and res["n_skipped"] == 1 and res["n_ignored"] == 0
    assert np.array_equal(R.confusion(x[:4].numpy(), y[:4].numpy(), 4)[:16].reshape(4, 4), want)
    assert res["per_class_recall"].tolist() == [1.0, 1.0, 0.0, 0.0] and res["uar"] == 2.0 / 3.0, "class 2 has no support: not in the UAR"
    assert abs(res["macro_f1"] - (2.0 / 3.0 + 1.0 + 0.0) / 3.0) <= TOL, "class 2 occurs neither as a label nor as a prediction"
    st.update(x, None, y, torch.tensor(1.0))
    with pytest.raises(ValueError, match="outside"):
        st.result()
