"""Independent numpy reference of the ranking metrics and the single-label confusion statistics (hriemo_stats_rank,
hriemo_stats_confusion, train.EpochStats.ranking / pr_curve / roc_curve / result() with confusion=True).  Nothing here imports the
package: the integers come from a sort of the NEGATED probabilities plus searchsorted, the ratios from the integers in float64.

Conventions: probs fp32 [n], truth bool [n] of ONE class; ge_pos[i] / ge_neg[i] = the number of positives / negatives j with
p_j >= p_i (sample i counts itself in the plane of its own kind)."""
import numpy as np


def ge_counts(probs, truth):
    """(ge_pos, ge_neg) int64 [n]: q >= p  <=>  -q <= -p, the number of which is searchsorted(sort(-q), -p, 'right')"""
    probs, truth = np.asarray(probs, dtype=np.float32), np.asarray(truth, dtype=bool)
    neg_p = -probs.astype(np.float64)                       # exact: fp32 negated in float64
    out = []
    for kind in (truth, ~truth):
        out.append(np.searchsorted(np.sort(neg_p[kind]), neg_p, side="right").astype(np.int64))
    return out[0], out[1]


def rank_block(probs, truth, n, capacity):
    """what hriemo_stats_rank stores for a class-major log probs / truth [C, >= n]: int32-valued [C, 2, capacity], zeros at i >= n"""
    C = probs.shape[0]
    out = np.zeros((C, 2, capacity), dtype=np.int64)
    for c in range(C):
        out[c, 0, :n], out[c, 1, :n] = ge_counts(probs[c, :n], truth[c, :n])
    return out


def average_precision(probs, truth):
    """mean over the positives of ge_pos / (ge_pos + ge_neg); 0.0 without a positive"""
    truth = np.asarray(truth, dtype=bool)
    if not truth.any():
        return 0.0
    gp, gn = ge_counts(probs, truth)
    gp, gn = gp[truth].astype(np.float64), gn[truth].astype(np.float64)
    return float(np.sum(gp / (gp + gn)) / truth.sum())


def auc(probs, truth):
    """Mann-Whitney with ties as halves; nan where a kind is missing"""
    probs, truth = np.asarray(probs, dtype=np.float32), np.asarray(truth, dtype=bool)
    pos, neg = probs[truth], np.sort(probs[~truth])
    if pos.size == 0 or neg.size == 0:
        return float("nan")
    below, upto = np.searchsorted(neg, pos, "left"), np.searchsorted(neg, pos, "right")
    return float((2 * below + (upto - below)).sum()) / (2.0 * pos.size * neg.size)


def _distinct(probs, truth):
    gp, gn = ge_counts(probs, truth)
    order = np.argsort(probs, kind="stable")
    sp = np.asarray(probs, dtype=np.float32)[order]
    first = order[np.concatenate([[True], sp[1:] != sp[:-1]])]
    return np.asarray(probs, dtype=np.float32)[first], gp[first].astype(np.float64), gn[first].astype(np.float64)


def pr_curve(probs, truth):
    """sklearn.metrics.precision_recall_curve's layout: distinct probabilities ascending, then (1, 0)"""
    thr, gp, gn = _distinct(probs, truth)
    n_pos = float(np.asarray(truth, dtype=bool).sum())
    return np.append(gp / (gp + gn), 1.0), np.append(gp / n_pos, 0.0), thr


def roc_curve(probs, truth):
    """sklearn.metrics.roc_curve(drop_intermediate=False)'s layout: (0, 0) at inf, then distinct probabilities descending"""
    thr, gp, gn = _distinct(probs, truth)
    truth = np.asarray(truth, dtype=bool)
    return (np.append(0.0, gn[::-1] / float((~truth).sum())), np.append(0.0, gp[::-1] / float(truth.sum())),
            np.append(np.inf, thr[::-1].astype(np.float64)))


IGNORE = -100


def first_argmax(logits):
    """the first maximal logit's index, a NaN counting as maximal (torch.argmax's rule), in a plain loop over the classes"""
    x = np.asarray(logits, dtype=np.float32)
    best, bv = np.zeros(x.shape[0], dtype=np.int64), x[:, 0].copy()
    for c in range(1, x.shape[1]):
        v = x[:, c]
        take = (v > bv) | (np.isnan(v) & ~np.isnan(bv))
        best[take], bv[take] = c, v[take]
    return best


def confusion(logits, labels, C):
    """cm int64 [C * C + 2]: matrix (row = label, column = first argmax), n_ignored (label -100), n_bad (any other label outside [0, C))"""
    labels = np.asarray(labels, dtype=np.int64)
    pred = first_argmax(logits)
    cm = np.zeros(C * C + 2, dtype=np.int64)
    ok = (labels >= 0) & (labels < C)
    np.add.at(cm, labels[ok] * C + pred[ok], 1)
    cm[C * C] = int((labels == IGNORE).sum())
    cm[C * C + 1] = int((~ok & (labels != IGNORE)).sum())
    return cm


def confusion_scores(m):
    """macro / weighted F1, per-class F1 and recall, UAR from a confusion matrix [C, C] (zero_division = 0; macro over the classes that
    occur as a label or a prediction, UAR over the classes with support)"""
    m = np.asarray(m, dtype=np.float64)
    tp, support, predicted = np.diag(m), m.sum(1), m.sum(0)
    den = support + predicted
    f1 = np.divide(2.0 * tp, den, out=np.zeros_like(tp), where=den > 0)
    recall = np.divide(tp, support, out=np.zeros_like(tp), where=support > 0)
    return {"per_class_f1": f1, "per_class_recall": recall, "macro_f1": float(f1[den > 0].mean()) if (den > 0).any() else 0.0,
            "weighted_f1": float((f1 * support).sum() / support.sum()) if support.sum() > 0 else 0.0,
            "uar": float(recall[support > 0].mean()) if (support > 0).any() else 0.0}
