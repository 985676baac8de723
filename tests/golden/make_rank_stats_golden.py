"""Writes tests/golden/rank_stats.npz: sklearn's ranking metrics and single-label F1s as recorded data, for
hri_emo_amd.train.EpochStats.ranking / pr_curve / roc_curve / per_class_table, EpochStats(confusion=True) and the hriemo_stats_rank /
hriemo_stats_confusion kernels.  Run once on a CPU that has sklearn:

    python tests/golden/make_rank_stats_golden.py

Multi-label inputs: the logits / targets of tests/golden/epoch_stats.npz (read here, not duplicated); probabilities are
torch.sigmoid in float64 rounded to fp32, as that fixture's maker defines them; a label is positive when its target is > 0.
Recorded per case (cont, grid) and prefix n in that fixture's `ns`, per class: average_precision_score and roc_auc_score (nan where
sklearn has no value: a class without positives, or without one of the two kinds).  For n = 301 and n = 1000 also
precision_recall_curve (classes with a positive) and roc_curve(drop_intermediate=False) (classes with both kinds).

The layout every consumer of the fixture relies on is ASSERTED here by brute force (counts from an O(n^2) comparison), so the
fixture cannot silently encode another one.  With ge_pos[i] / ge_neg[i] = the number of positives / negatives j with p_j >= p_i:
  precision_recall_curve   one point per distinct probability in ascending order, precision = ge_pos / (ge_pos + ge_neg),
                           recall = ge_pos / n_pos, then the point (1, 0); thresholds = the distinct probabilities
  roc_curve                the point (0, 0) with threshold inf, then the same points in descending order, fpr = ge_neg / n_neg,
                           tpr = ge_pos / n_pos
  average_precision_score  the mean over the positives of ge_pos / (ge_pos + ge_neg)
Both curves must match exactly (difference 0), average precision within 1e-14.

Single-label case (C = 4, N = 1000): logits on a grid of 1/4 (so rows tie), class 2 never predicted, the label -100 (the criterion's
ignore_index) in every 97th sample.  Recorded over the labelled samples, prediction = the first maximal logit: confusion_matrix,
f1_score(average="macro" | "weighted" | None), accuracy_score, recall_score(average="macro" | None).

sklearn.__version__ is recorded."""
import os
import warnings

import numpy as np
import sklearn
import torch
from sklearn.metrics import (accuracy_score, average_precision_score, confusion_matrix, f1_score, precision_recall_curve, recall_score,
                             roc_auc_score, roc_curve)

HERE = os.path.dirname(os.path.abspath(__file__))
CURVE_NS = (301, 1000)


def brute(p, t):
    ge = p[None, :] >= p[:, None]                       # [i, j]: p_j >= p_i
    return (ge & t[None, :]).sum(1).astype(np.float64), (ge & ~t[None, :]).sum(1).astype(np.float64)


def distinct(p, gp, gn):
    thr, first = np.unique(p, return_index=True)
    return thr, gp[first], gn[first]


def multi_label(out):
    src = np.load(os.path.join(HERE, "epoch_stats.npz"))
    ns = [int(n) for n in src["ns"]]
    out["ns"], out["curve_ns"] = np.asarray(ns), np.asarray(CURVE_NS)
    assert set(CURVE_NS) <= set(ns)
    for case in ("cont", "grid"):
        logits, targets = torch.from_numpy(src[f"{case}_logits"]), src[f"{case}_targets"]
        probs = torch.sigmoid(logits.double()).float().numpy()
        truth = targets > 0
        C = probs.shape[1]
        for n in ns:
            ap, auc = np.full(C, np.nan), np.full(C, np.nan)
            for c in range(C):
                p, t = probs[:n, c], truth[:n, c]
                n_pos, n_neg = int(t.sum()), int((~t).sum())
                gp, gn = brute(p, t)
                if n_pos:
                    ap[c] = average_precision_score(t, p)
                    mine = float((gp[t] / (gp[t] + gn[t])).sum() / n_pos)
                    assert abs(mine - ap[c]) <= 1e-14, (case, n, c, mine, ap[c])
                if n_pos and n_neg:
                    auc[c] = roc_auc_score(t, p)
                if n not in CURVE_NS:
                    continue
                thr, dp, dn = distinct(p, gp, gn)
                k = f"{case}_{n}_c{c}_"
                if n_pos:
                    precision, recall, th = precision_recall_curve(t, p)
                    assert np.array_equal(th, thr) and np.array_equal(precision, np.append(dp / (dp + dn), 1.0)), (case, n, c)
                    assert np.array_equal(recall, np.append(dp / n_pos, 0.0)), (case, n, c)
                    out.update({k + "pr_precision": precision, k + "pr_recall": recall, k + "pr_thresholds": th})
                if n_pos and n_neg:
                    fpr, tpr, th = roc_curve(t, p, drop_intermediate=False)
                    assert np.isinf(th[0]) and np.array_equal(th[1:], thr[::-1]), (case, n, c)
                    assert np.array_equal(fpr, np.append(0.0, dn[::-1] / n_neg)) and np.array_equal(tpr, np.append(0.0, dp[::-1] / n_pos)), (case, n, c)
                    out.update({k + "roc_fpr": fpr, k + "roc_tpr": tpr, k + "roc_thresholds": th})
            out[f"{case}_{n}_ap"], out[f"{case}_{n}_auc"] = ap, auc


def single_label(out):
    N, C = 1000, 4
    g = np.random.default_rng(20261021)
    labels = g.integers(0, C, N)
    logits = np.round(2.0 * g.standard_normal((N, C)) * 4.0) / 4.0
    logits[np.arange(N), labels] += 1.5 * (labels != 2)
    logits[:, 2] = -12.0 + np.round(g.standard_normal(N) * 4.0) / 4.0          # never maximal
    logits = logits.astype(np.float32)
    labels[::97] = -100
    pred = logits.argmax(1)                                                    # the first maximal logit
    assert (pred != 2).all() and ((np.sort(logits, 1)[:, -1] == np.sort(logits, 1)[:, -2]).sum() > 10), "class 2 never predicted; tied rows"
    keep = labels != -100
    y, yp = labels[keep], pred[keep]
    assert set(y.tolist()) == set(range(C)) and int((~keep).sum()) == 11
    out.update({"sl_logits": logits, "sl_labels": labels.astype(np.int64), "sl_confusion": confusion_matrix(y, yp, labels=list(range(C))).astype(np.int64),
                "sl_n_ignored": np.asarray(int((~keep).sum())),
                "sl_macro_f1": np.asarray(f1_score(y, yp, average="macro")), "sl_weighted_f1": np.asarray(f1_score(y, yp, average="weighted")),
                "sl_per_class_f1": f1_score(y, yp, average=None, labels=list(range(C))), "sl_accuracy": np.asarray(accuracy_score(y, yp)),
                "sl_uar": np.asarray(recall_score(y, yp, average="macro")), "sl_per_class_recall": recall_score(y, yp, average=None, labels=list(range(C)))})


def main():
    out = {"sklearn_version": np.frombuffer(sklearn.__version__.encode(), dtype=np.uint8)}        # ASCII bytes: conftest.load_golden reads numbers
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # a class 2 that is never predicted: sklearn sets its precision to 0 and says so
        multi_label(out)
        single_label(out)
    path = os.path.join(HERE, "rank_stats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays, sklearn", sklearn.__version__)
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
