"""Losses of the reference's trainers as ONE kernel each (value + gradients, hriemo_fusion_loss):
  fusion_step_loss        scripts/fusion/train_fusion_seq_level_decoder.py:312-326 (multi-label branch):
                          BCEWithLogits(logits, y) - 0.01*mean(beta*(1-beta))
  fusion_step_loss_single_label   the same trainer's single_label branch (:312-314, criterion nn.CrossEntropyLoss() :413-414):
                          CrossEntropy(logits, class index) - 0.01*mean(beta*(1-beta))   (hriemo_fusion_loss_ce)
  mosei_step_loss         scripts/fusion/train_mosei_fusion_seq_level_decoder.py:340-347,383-387,569:
                          BCEWithLogits(logits, y; pos_weight) + beta_entropy*H(beta), divided by grad_accum
CPU tensors (the gloo tests drive the CPU oracle through dp.py) take the same formulas in plain torch."""
import numpy as np
import torch
import torch.nn.functional as F


# n_valid (all three losses): None, or a 0-dim / 1-element int32 tensor n with 1 <= n <= B.  Only the first n samples count: both
# means run over them, the samples behind them ("ghosts": the padding of a short last batch inside a captured step,
# dp.capture_packed(partial_batches=True)) add no loss term and get exactly zero gradients, whatever their rows hold.  On the GPU
# the count is read by the kernel (hriemo_fusion_loss_n / _ce_n), so a captured step follows it from replay to replay; on the CPU
# the formulas slice [:n].


def _head(n_valid, *tensors):
    """the CPU formulas' view of n_valid: every tensor cut to its first n samples"""
    if n_valid is None:
        return tensors
    n = int(n_valid)
    if not 1 <= n <= tensors[0].shape[0]:
        raise ValueError(f"n_valid = {n} outside [1, {tensors[0].shape[0]}]")
    return tuple(None if t is None else t[:n] for t in tensors)


def fusion_step_loss(logits, beta, targets, n_valid=None):
    if logits.is_cuda:
        from ._ops import FusionLossFn
        return FusionLossFn.apply(logits, beta, targets, None, 1, 0.01, 1.0, *(() if n_valid is None else (n_valid,)))
    logits, beta, targets = _head(n_valid, logits, beta, targets)
    return F.binary_cross_entropy_with_logits(logits, targets) - 0.01 * (beta * (1.0 - beta)).mean()


def fusion_step_loss_single_label(logits, beta, labels, n_valid=None):
    if logits.is_cuda:
        from ._ops import FusionLossCEFn
        return FusionLossCEFn.apply(logits, beta, labels, 1, 0.01, 1.0, *(() if n_valid is None else (n_valid,)))
    logits, beta, labels = _head(n_valid, logits, beta, labels)
    return F.cross_entropy(logits, labels) - 0.01 * (beta * (1.0 - beta)).mean()


def beta_entropy_loss(beta, eps=1e-8):
    b = torch.clamp(beta, eps, 1.0 - eps)
    return (-(b * torch.log(b) + (1 - b) * torch.log(1 - b))).mean()


def mosei_step_loss(logits, beta, targets, pos_weight=None, beta_entropy=0.0, grad_accum=1, n_valid=None):
    if logits.is_cuda:
        from ._ops import FusionLossFn
        return FusionLossFn.apply(logits, beta if beta_entropy > 0 else None, targets, pos_weight, 2, float(beta_entropy), 1.0 / grad_accum,
                                  *(() if n_valid is None else (n_valid,)))
    logits, beta, targets = _head(n_valid, logits, beta, targets)
    loss = F.binary_cross_entropy_with_logits(logits, targets, pos_weight=pos_weight)
    if beta is not None and beta_entropy > 0:
        loss = loss + beta_entropy * beta_entropy_loss(beta)
    return loss / grad_accum


# ---------------------------------------------------------------------------------------------------------------- epoch statistics
# What the reference's trainers report per epoch, without a read-back per step (hriemo_stats_update / _counts / _auc, csrc/metrics.hip):
#   train_fusion_seq_level_decoder.py:300-372          sample-weighted mean loss, accuracy, mean beta
#   train_mosei_fusion_seq_level_decoder.py:119-171,367-495   mean loss (non-finite batches skipped), mean beta, micro / macro F1,
#                                                      macro AUC, calibrate_thresholds' sweep and the macro F1 at its thresholds
# The device (and the CPU twin below) produce INTEGERS only: tp / fp / fn per class and threshold, 2U per class (the Mann-Whitney
# count with ties as halves, doubled), n_pos, n_neg, the counters.  Every ratio is formed here in float64.

SWEEP = tuple(float(t) for t in np.linspace(0.05, 0.95, 19))        # calibrate_thresholds' grid (:165)
_MAX_THRESHOLDS = 64          # STATS_MAX_THRESHOLDS of csrc/metrics.hip
_CTR = ("cursor", "n_samples", "n_batches", "n_skipped", "n_correct", "n_nonfinite", "overflow")
_MAX_CONFUSION_CLASSES = 64   # CONFUSION_MAX_CLASSES of csrc/metrics.hip
_IGNORE_INDEX = -100          # nn.CrossEntropyLoss's ignore_index: such a sample has no label


def thresholds_up(thresholds):
    """float64 thresholds -> float32, each the SMALLEST fp32 value >= its threshold.  The reference compares fp32 probabilities with
    float64 thresholds (numpy promotes p); p >= t64 holds exactly when p >= that fp32 value, so an fp32 comparison against the
    rounded-up threshold takes the reference's decision for the same p."""
    t = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    r = t.astype(np.float32)
    low = r.astype(np.float64) < t
    r[low] = np.nextafter(r[low], np.float32(np.inf))
    return r


def _f1(tp, fp, fn):
    """2 tp / (2 tp + fp + fn) in float64, 0 where the denominator is 0 (f1_score(..., zero_division=0))"""
    tp, den = np.asarray(tp, dtype=np.float64), 2.0 * np.asarray(tp, dtype=np.float64) + np.asarray(fp, dtype=np.float64) + np.asarray(fn, dtype=np.float64)
    return np.where(den > 0, 2.0 * tp / np.where(den > 0, den, 1.0), 0.0)


def _calibrate(sweep_counts, sweep, per_class):
    """calibrate_thresholds' choice from the sweep's integers [C, S, 3]: per class the FIRST grid point of strictly greater F1 (start
    0.5 / -1) and the F1 there -> (thresholds float32 [C], F1 float64 [C]); without a sweep: 0.5 and the F1 at 0.5.  The one place
    the selection rule lives: result() and per_class_table() both read it."""
    C, S = sweep_counts.shape[0], sweep_counts.shape[1]
    f1_sweep = _f1(sweep_counts[:, :, 0], sweep_counts[:, :, 1], sweep_counts[:, :, 2])          # [C, S]
    chosen, f1_cal = np.full(C, 0.5, dtype=np.float32), np.zeros(C)
    for c in range(C):
        best, best_t = -1.0, 0.5
        for s in range(S):
            if f1_sweep[c, s] > best:
                best, best_t = float(f1_sweep[c, s]), sweep[s]
        chosen[c] = best_t
        f1_cal[c] = best if S > 0 else per_class[c]
    return chosen, f1_cal


class EpochStats:
    """The statistics of one training or validation epoch, accumulated where the step runs.

    EpochStats(num_outputs, capacity, kind="multi_label" | "single_label", skip_nonfinite=False, device=...): `capacity` is the
    number of samples the epoch's log holds (multi-label: sigmoid(logits) as fp32 [C, capacity] and [target > 0] as uint8);
    skip_nonfinite is the MOSEI trainer's `continue` on a NaN / Inf loss (:390-393, :452-454): such a batch only counts in n_skipped.

    update(logits, beta, targets, loss, n_valid=None, loss_scale=1.0) enqueues ONE launch (hriemo_stats_update) on the current stream
    and reads nothing back; it can be recorded into a captured step (dp.DataParallelStep.attach_stats).  targets: float [B, C]
    (multi-label; a label counts as positive when > 0, so the MOSEI trainer's raw and normalised targets give the same bits) or
    int64 [B] (single-label).  loss: the scalar the loss wrote; loss_scale undoes a 1/grad_accum inside it (the reference logs the raw
    loss).  n_valid: None or a 1-element int32 tensor on the device (a Python int on the CPU path too): only the first
    clamp(n_valid, 1, B) samples count, whatever the rows behind them hold.

    result(thresholds=None): two launches over the log (hriemo_stats_counts, hriemo_stats_auc), ONE read-back, and the ratios in
    float64: avg_loss = |sum_loss / max(1, n_samples)|, accuracy (multi-label: every label of the sample has [p > 0.5] == [target >
    0]; single-label: first argmax == label), mean_beta, n_samples, n_batches, n_skipped; multi-label also micro_f1, macro_f1,
    per_class_f1 (prediction p >= 0.5), macro_auc (mean over the classes that have both kinds, 0.0 without one),
    calibrated_thresholds (float32 [C]; per class the first threshold of the sweep -- default SWEEP, np.linspace(0.05, 0.95, 19) --
    with strictly greater F1, start 0.5 / -1 as calibrate_thresholds), macro_f1_calibrated, and the integers themselves: tp, fp, fn
    [C] at 0.5, sweep_counts [C, S, 3], auc_2u, n_pos, n_neg [C].  RuntimeError if the log overflowed, ValueError if non-finite
    logits were logged.

    Thresholds: the kernels compare fp32 p with thresholds_up(t), which is the reference's `p >= t` for float64 t.  The calibrated
    thresholds are returned as the reference returns them, rounded to NEAREST fp32; macro_f1_calibrated is read from the sweep's own
    counts at the chosen grid points, while the reference compares a second time against those rounded values.  The two differ
    only where a probability lies within one fp32 ulp of a grid threshold.

    confusion=True (single_label only): update() enqueues hriemo_stats_confusion right behind hriemo_stats_update -- same n_valid,
    loss and skip_nonfinite -- and result() gains confusion (int64 [C, C], rows = label, columns = first argmax), n_ignored (labels
    equal to the criterion's ignore_index -100), per_class_f1, per_class_recall, macro_f1 (over the classes that occur as a label or
    a prediction: f1_score(average="macro")), weighted_f1 and uar (mean recall over the classes with support), all float64 from the
    integers with zero_division = 0; the matrix lives in the buffer result() reads back, so it stays ONE read-back.  ValueError if a
    label was neither in [0, C) nor -100.  What the four-class trainers report (train_text_baseline.py:59-61,
    linear_probe_baseline.py:132-133).

    ranking() / pr_curve(c) / roc_curve(c) / per_class_table() (multi_label): average precision and the precision-recall and ROC
    curves of the reporting layer (tools/mosei_export_per_class_metrics.py, scripts/infer/mosei_plot_metrics.py) from two integers
    per logged sample (hriemo_stats_rank), ratios in float64 on the host; see ranking().

    CPU tensors take the same definitions in plain torch / numpy (the log lives in host memory).  Statistics are per rank."""

    def __init__(self, num_outputs, capacity, kind="multi_label", skip_nonfinite=False, device="cuda", confusion=False):
        if kind not in ("multi_label", "single_label"):
            raise ValueError("EpochStats: kind is 'multi_label' or 'single_label'")
        if int(num_outputs) < 1 or int(capacity) < 1:
            raise ValueError("EpochStats: num_outputs and capacity are positive")
        if confusion and kind != "single_label":
            raise ValueError("EpochStats: confusion=True needs kind='single_label': a confusion matrix is defined for one label per sample "
                             "(the multi-label kind reports tp / fp / fn per class)")
        if confusion and int(num_outputs) > _MAX_CONFUSION_CLASSES:
            raise ValueError(f"EpochStats: confusion=True takes at most {_MAX_CONFUSION_CLASSES} classes")
        self.confusion = bool(confusion)
        self.C, self.capacity, self.kind, self.skip_nonfinite = int(num_outputs), int(capacity), kind, bool(skip_nonfinite)
        self.device = torch.device(device)
        self.multi = kind == "multi_label"
        C, dev = self.C, self.device
        self.tiles = (self.capacity + 255) // 256            # hriemo_stats_auc_tiles
        # everything result() reads back is ONE buffer: counters int32[8] | sums float64[4] | npn int32[C, 2] | counts
        # int32[C, 64, 3] | auc partials uint64[C, tiles] | cm int32[C * C + 2] (confusion=True); every part starts 8-byte aligned
        o_npn = 64
        o_cnt = o_npn + 8 * C
        o_auc = o_cnt + 4 * C * _MAX_THRESHOLDS * 3
        o_cm = o_auc + 8 * C * self.tiles
        self._small = torch.zeros(o_cm + (4 * (C * C + 2) if self.confusion else 0), dtype=torch.uint8, device=dev)
        self._parts = (o_npn, o_cnt, o_auc, o_cm)
        self.counters, self.sums, self._npn, self._counts, self._partial = self._views(self._small)
        self.cm = self._cm_view(self._small)         # {confusion matrix [C, C] (row = label), n_ignored, n_bad}, or None
        self._rank = None                            # int32 [C, 2, capacity], allocated by the first ranking()
        if self.multi:
            self.probs = torch.zeros(C, self.capacity, dtype=torch.float32, device=dev)
            self.truth = torch.zeros(C, self.capacity, dtype=torch.uint8, device=dev)
        else:
            self.probs = self.truth = None
        self._thr = torch.zeros(_MAX_THRESHOLDS, dtype=torch.float32, device=dev)

    def _views(self, buf):
        o_npn, o_cnt, o_auc, o_cm = self._parts
        return (buf[:32].view(torch.int32), buf[32:64].view(torch.float64), buf[o_npn:o_cnt].view(torch.int32).view(self.C, 2),
                buf[o_cnt:o_auc].view(torch.int32), buf[o_auc:o_cm].view(torch.int64).view(self.C, self.tiles))

    def _cm_view(self, buf):
        return buf[self._parts[3]:].view(torch.int32) if self.confusion else None

    def reset(self):
        """a new epoch: counters, sums and the confusion matrix to zero (the log needs no clearing: only entries in front of the
        cursor are ever read)"""
        self._small[:64].zero_()
        if self.confusion:
            self.cm.zero_()

    # ---- update
    def _check(self, logits, beta, targets, loss):
        if logits.dim() != 2 or logits.shape[1] != self.C:
            raise ValueError(f"EpochStats.update: logits of shape {tuple(logits.shape)}; expected [B, {self.C}]")
        B = logits.shape[0]
        want = (B, self.C) if self.multi else (B,)
        if tuple(targets.shape) != want:
            raise ValueError(f"EpochStats.update: targets of shape {tuple(targets.shape)}; the {self.kind} kind takes {want}")
        if beta is not None and (beta.numel() == 0 or beta.numel() % B != 0):
            raise ValueError(f"EpochStats.update: beta of {beta.numel()} values for {B} samples")
        if loss.numel() != 1:
            raise ValueError("EpochStats.update: loss is one scalar")
        return B

    def update(self, logits, beta, targets, loss, n_valid=None, loss_scale=1.0):
        B = self._check(logits, beta, targets, loss)
        if not logits.is_cuda:
            return self._update_cpu(logits, beta, targets, loss, n_valid, float(loss_scale), B)
        from . import _lib, _ops
        p = _ops._p
        nv = _ops._n_valid_word((n_valid,), logits)
        x = logits.detach().contiguous().float()
        y = targets.detach().contiguous()
        y = y.float() if self.multi else y.to(torch.int64)
        bt = beta.detach().contiguous().float() if beta is not None else None
        lv = loss.detach().reshape(1).float()
        _lib.call("hriemo_stats_update", p(x), p(y) if self.multi else None, None if self.multi else p(y), p(lv), float(loss_scale),
                  p(bt), bt.numel() // B if bt is not None else 0, p(nv), B, self.C, int(self.skip_nonfinite), p(self.probs), p(self.truth),
                  self.capacity, p(self.counters), p(self.sums), _ops._stream())
        if self.confusion:
            _lib.call("hriemo_stats_confusion", p(x), p(y), p(lv), int(self.skip_nonfinite), p(nv), B, self.C, p(self.cm), _ops._stream())

    def _update_cpu(self, logits, beta, targets, loss, n_valid, loss_scale, B):
        import math
        nv = B if n_valid is None else min(max(int(n_valid), 1), B)
        ctr, lv = self.counters, float(loss)
        if self.skip_nonfinite and not math.isfinite(lv):
            ctr[3] += 1
            return
        x = logits.detach()[:nv].float()
        if self.multi:
            # float64, rounded to fp32: torch's fp32 CPU sigmoid sends the last numel % 16 elements of a tensor down a scalar path
            # that can differ by an ulp, and two equal logits in two batches must tie in the AUC
            pr, t = torch.sigmoid(x.double()).float(), targets.detach()[:nv] > 0
            ctr[4] += int(((pr > 0.5) == t).all(dim=1).sum())
            cur = int(ctr[0])
            if cur + nv <= self.capacity:
                self.probs[:, cur:cur + nv] = pr.t()
                self.truth[:, cur:cur + nv] = t.t().to(torch.uint8)
                ctr[5] += int((~torch.isfinite(x)).sum())
                ctr[0] = cur + nv
            else:
                ctr[6] = 1
        else:
            pred, lab = x.argmax(dim=1).numpy(), targets.detach()[:nv].to(torch.int64).numpy()
            ctr[4] += int((pred == lab).sum())
            if self.confusion:
                cm, C = self.cm.numpy(), self.C
                ok = (lab >= 0) & (lab < C)
                np.add.at(cm, lab[ok] * C + pred[ok], 1)
                cm[C * C] += int((lab == _IGNORE_INDEX).sum())
                cm[C * C + 1] += int((~ok & (lab != _IGNORE_INDEX)).sum())
        ctr[1] += nv
        ctr[2] += 1
        self.sums[0] += lv * loss_scale * nv
        if beta is not None:
            b = beta.detach().reshape(B, -1)[:nv].double()
            self.sums[1] += float(b.sum())
            self.sums[2] += b.numel()

    # ---- result
    def _integers_cpu(self, thr, n):
        """tp / fp / fn [C, S, 3], 2U [C], n_pos / n_neg [C, 2] of the first n log entries, the kernels' definitions in numpy"""
        pr, t = self.probs[:, :n].numpy(), self.truth[:, :n].numpy() != 0
        pred = pr[:, None, :] >= thr[None, :, None]                                  # fp32 against fp32
        tt = t[:, None, :]
        counts = np.stack([(pred & tt).sum(2), (pred & ~tt).sum(2), (~pred & tt).sum(2)], axis=2).astype(np.int64)
        two_u, npn = np.zeros(self.C, dtype=np.int64), np.zeros((self.C, 2), dtype=np.int64)
        for c in range(self.C):
            pos, neg = pr[c][t[c]], np.sort(pr[c][~t[c]])
            below, upto = np.searchsorted(neg, pos, "left"), np.searchsorted(neg, pos, "right")
            two_u[c] = int((2 * below + (upto - below)).sum())
            npn[c] = (pos.size, neg.size)
        return counts, two_u, npn

    def result(self, thresholds=None):
        sweep = np.asarray(SWEEP if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        if sweep.size + 1 > _MAX_THRESHOLDS:
            raise ValueError(f"EpochStats.result: at most {_MAX_THRESHOLDS - 1} thresholds")
        grid = np.concatenate([[0.5], sweep])                # entry 0: the reported F1s; the rest: the calibration sweep
        thr = thresholds_up(grid)
        S = thr.size
        on_gpu = self.device.type == "cuda"
        if on_gpu:
            if self.multi:
                from . import _lib, _ops
                p = _ops._p
                with torch.cuda.device(self.device):
                    self._thr[:S].copy_(torch.from_numpy(thr), non_blocking=True)
                    _lib.call("hriemo_stats_counts", p(self.probs), p(self.truth), self.capacity, self.C, p(self.counters), p(self._thr), S,
                              p(self._counts), _ops._stream())
                    _lib.call("hriemo_stats_auc", p(self.probs), p(self.truth), self.capacity, self.C, p(self.counters), p(self._partial),
                              p(self._npn), _ops._stream())
            host = self._small.cpu()                                                  # the epoch's one read-back
            ctr, sums, npn, counts, partial = self._views(host)
            cm = self._cm_view(host)
        else:
            ctr, sums, cm = self.counters, self.sums, self.cm
        ctr, sums = [int(v) for v in ctr.tolist()], [float(v) for v in sums.tolist()]
        out = dict(zip(_CTR[1:5], ctr[1:5]))
        n = out["n_samples"]
        out["avg_loss"] = abs(sums[0] / max(1, n))
        out["accuracy"] = out["n_correct"] / n if n > 0 else 0.0
        out["mean_beta"] = sums[1] / sums[2] if sums[2] > 0 else 0.0
        if not self.multi:
            if self.confusion:
                out.update(self._confusion_metrics(cm.numpy().astype(np.int64)))
            return out
        if ctr[6]:
            raise RuntimeError(f"EpochStats: the log of {self.capacity} samples overflowed ({n} samples were offered); size capacity for the epoch")
        if ctr[5]:
            raise ValueError(f"EpochStats: {ctr[5]} non-finite logits were logged; F1 / AUC of this epoch are undefined")
        n_log = ctr[0]
        if on_gpu:
            counts = counts[:self.C * S * 3].view(self.C, S, 3).numpy().astype(np.int64)
            two_u, npn = partial.numpy().sum(axis=1), npn.numpy().astype(np.int64)
        else:
            counts, two_u, npn = self._integers_cpu(thr, n_log)
        tp, fp, fn = counts[:, 0, 0], counts[:, 0, 1], counts[:, 0, 2]
        per_class = _f1(tp, fp, fn)
        both = (npn[:, 0] > 0) & (npn[:, 1] > 0)
        auc = two_u[both].astype(np.float64) / (2.0 * npn[both, 0].astype(np.float64) * npn[both, 1].astype(np.float64))
        chosen, f1_cal = _calibrate(counts[:, 1:], sweep, per_class)
        out.update(n_logged=n_log, micro_f1=float(_f1(tp.sum(), fp.sum(), fn.sum())), macro_f1=float(per_class.mean()),
                   per_class_f1=per_class, macro_auc=float(auc.mean()) if auc.size else 0.0, calibrated_thresholds=chosen,
                   macro_f1_calibrated=float(f1_cal.mean()), tp=tp, fp=fp, fn=fn, sweep_counts=counts[:, 1:], auc_2u=two_u,
                   n_pos=npn[:, 0], n_neg=npn[:, 1])
        return out

    # ---- single-label: the confusion matrix
    def _confusion_metrics(self, cm):
        """the keys result() gains with confusion=True, in float64 from the integers cm [C * C + 2] (zero_division = 0 throughout)"""
        C = self.C
        n_ignored, n_bad = int(cm[C * C]), int(cm[C * C + 1])
        if n_bad:
            raise ValueError(f"EpochStats: {n_bad} labels outside [0, {C}) that are not the ignore_index {_IGNORE_INDEX}")
        m = cm[:C * C].reshape(C, C).copy()
        tp, support, predicted = np.diag(m), m.sum(axis=1), m.sum(axis=0)
        f1 = _f1(tp, predicted - tp, support - tp)
        recall = np.where(support > 0, tp / np.where(support > 0, support, 1).astype(np.float64), 0.0)
        present = (support + predicted) > 0              # f1_score(labels=None): the classes that occur as a label or a prediction
        n = float(support.sum())
        return {"confusion": m, "n_ignored": n_ignored, "per_class_f1": f1, "per_class_recall": recall,
                "macro_f1": float(f1[present].mean()) if present.any() else 0.0,
                "weighted_f1": float((f1 * support).sum() / n) if n > 0 else 0.0,
                "uar": float(recall[support > 0].mean()) if (support > 0).any() else 0.0}

    # ---- multi-label: ranking metrics
    def _ranks_cpu(self, n):
        """ge_pos / ge_neg [C, n] of the first n log entries by sorting: the kernel's definition (hriemo_stats_rank) in numpy"""
        pr, t = self.probs[:, :n].numpy(), self.truth[:, :n].numpy() != 0
        ge = np.zeros((2, self.C, n), dtype=np.int64)
        for c in range(self.C):
            for plane, kind in enumerate((t[c], ~t[c])):
                q = np.sort(pr[c][kind])
                ge[plane, c] = q.size - np.searchsorted(q, pr[c], "left")
        return ge[0], ge[1]

    def ranking(self):
        """The ranking metrics of the reference's reporting layer (tools/mosei_export_per_class_metrics.py,
        scripts/infer/mosei_plot_metrics.py) from integers: one launch (hriemo_stats_rank) plus hriemo_stats_auc over the log, then
        the read-back of the small block, the ranks and the first n_logged columns of the log.  multi_label only.  Returns
        ge_pos, ge_neg (int64 [C, n]: per logged sample the number of positives / negatives of its class with p_j >= p_i, itself
        included), probs (fp32 [C, n]), truth (bool [C, n]), n_pos, n_neg, per_class_auc (float64 [C], nan where a class lacks one
        kind), macro_auc (result()'s), average_precision (float64 [C]: the mean over the positives of ge_pos / (ge_pos + ge_neg) --
        sklearn's average_precision_score, ties included; 0.0 for a class without positives, as mosei_plot_metrics.py:47,135) and
        macro_ap (mean over the classes with a positive, 0.0 without one).  RuntimeError / ValueError as result()."""
        if not self.multi:
            raise ValueError("EpochStats.ranking: ranking metrics belong to the multi_label kind (single_label keeps no log)")
        C = self.C
        if self.device.type == "cuda":
            from . import _lib, _ops
            p = _ops._p
            with torch.cuda.device(self.device):
                if self._rank is None:
                    self._rank = torch.zeros(C, 2, self.capacity, dtype=torch.int32, device=self.device)
                _lib.call("hriemo_stats_rank", p(self.probs), p(self.truth), self.capacity, C, p(self.counters), p(self._rank), _ops._stream())
                _lib.call("hriemo_stats_auc", p(self.probs), p(self.truth), self.capacity, C, p(self.counters), p(self._partial),
                          p(self._npn), _ops._stream())
            ctr, _, npn, _, partial = self._views(self._small.cpu())
        else:
            ctr = self.counters
        ctr = [int(v) for v in ctr.tolist()]
        if ctr[6]:
            raise RuntimeError(f"EpochStats: the log of {self.capacity} samples overflowed ({ctr[1]} samples were offered); size capacity for the epoch")
        if ctr[5]:
            raise ValueError(f"EpochStats: {ctr[5]} non-finite logits were logged; ranking metrics of this epoch are undefined")
        n = min(max(ctr[0], 0), self.capacity)
        if self.device.type == "cuda":
            rank = self._rank[:, :, :n].cpu().numpy().astype(np.int64)
            ge_pos, ge_neg = rank[:, 0], rank[:, 1]
            two_u, npn = partial.numpy().sum(axis=1), npn.numpy().astype(np.int64)
            probs, truth = self.probs[:, :n].cpu().numpy(), self.truth[:, :n].cpu().numpy() != 0
        else:
            ge_pos, ge_neg = self._ranks_cpu(n)
            _, two_u, npn = self._integers_cpu(np.zeros(1, dtype=np.float32), n)
            probs, truth = self.probs[:, :n].numpy().copy(), self.truth[:, :n].numpy() != 0
        n_pos, n_neg = npn[:, 0], npn[:, 1]
        both = (n_pos > 0) & (n_neg > 0)
        auc = np.full(C, np.nan)
        auc[both] = two_u[both].astype(np.float64) / (2.0 * n_pos[both].astype(np.float64) * n_neg[both].astype(np.float64))
        ap = np.zeros(C)
        for c in range(C):
            if n_pos[c] > 0:
                gp, gn = ge_pos[c][truth[c]].astype(np.float64), ge_neg[c][truth[c]].astype(np.float64)
                ap[c] = float((gp / (gp + gn)).sum() / float(n_pos[c]))
        return {"ge_pos": ge_pos, "ge_neg": ge_neg, "probs": probs, "truth": truth, "n_pos": n_pos, "n_neg": n_neg, "n_logged": n,
                "per_class_auc": auc, "macro_auc": float(auc[both].mean()) if both.any() else 0.0, "average_precision": ap,
                "macro_ap": float(ap[n_pos > 0].mean()) if (n_pos > 0).any() else 0.0}

    @staticmethod
    def _distinct(rk, c):
        """per distinct probability of class c, ascending: (probability, ge_pos, ge_neg) -- tied samples share their two counts"""
        thr, first = np.unique(rk["probs"][c], return_index=True)
        return thr, rk["ge_pos"][c][first].astype(np.float64), rk["ge_neg"][c][first].astype(np.float64)

    def pr_curve(self, c, ranking=None):
        """(precision, recall, thresholds) of class c in sklearn.metrics.precision_recall_curve's layout: one point per distinct
        probability in ascending order, precision = ge_pos / (ge_pos + ge_neg), recall = ge_pos / n_pos, then the point (1, 0).
        Pure host arithmetic on a ranking() result (taken now when none is passed).  ValueError for a class without positives."""
        rk = self.ranking() if ranking is None else ranking
        if int(rk["n_pos"][c]) == 0:
            raise ValueError(f"EpochStats.pr_curve: class {c} has no positive sample; its recall is undefined")
        thr, gp, gn = self._distinct(rk, c)
        return np.append(gp / (gp + gn), 1.0), np.append(gp / float(rk["n_pos"][c]), 0.0), thr

    def roc_curve(self, c, ranking=None):
        """(fpr, tpr, thresholds) of class c in sklearn.metrics.roc_curve(..., drop_intermediate=False)'s layout: the point (0, 0)
        with threshold inf, then one point per distinct probability in descending order, fpr = ge_neg / n_neg, tpr = ge_pos / n_pos.
        Pure host arithmetic on a ranking() result.  ValueError for a class that lacks positives or negatives."""
        rk = self.ranking() if ranking is None else ranking
        if int(rk["n_pos"][c]) == 0 or int(rk["n_neg"][c]) == 0:
            raise ValueError(f"EpochStats.roc_curve: class {c} has {int(rk['n_pos'][c])} positives and {int(rk['n_neg'][c])} negatives; "
                             "the curve needs both kinds")
        thr, gp, gn = self._distinct(rk, c)
        return (np.append(0.0, gn[::-1] / float(rk["n_neg"][c])), np.append(0.0, gp[::-1] / float(rk["n_pos"][c])),
                np.append(np.inf, thr[::-1].astype(np.float64)))

    def per_class_table(self, names=None, thresholds=None):
        """The reference's per-class table (tools/mosei_export_per_class_metrics.py:10-17) from one result(thresholds) and one
        ranking(): a list of dicts class_, prevalence (n_pos / n), auc (nan where a class lacks one kind), auprc (average
        precision), f1_raw (p >= 0.5), f1_cal (the sweep's F1 at the chosen grid point, as macro_f1_calibrated), thr."""
        names = [str(c) for c in range(self.C)] if names is None else list(names)
        if len(names) != self.C:
            raise ValueError(f"EpochStats.per_class_table: {len(names)} names for {self.C} classes")
        res, rk = self.result(thresholds), self.ranking()
        sweep = np.asarray(SWEEP if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        _, f1_cals = _calibrate(res["sweep_counts"], sweep, res["per_class_f1"])           # result()'s own rule on result()'s integers
        n = max(1, res["n_logged"])
        rows = []
        for c in range(self.C):
            f1_cal = float(f1_cals[c])
            rows.append({"class_": names[c], "prevalence": float(res["n_pos"][c]) / n, "auc": float(rk["per_class_auc"][c]),
                         "auprc": float(rk["average_precision"][c]), "f1_raw": float(res["per_class_f1"][c]), "f1_cal": f1_cal,
                         "thr": float(res["calibrated_thresholds"][c])})
        return rows


# ------------------------------------------------------------------------------------------------------------------ prediction log
_PL = ("cursor", "n_samples", "overflow", "n_nonfinite")        # counters[4] of hriemo_predict_log


class PredictionLog:
    """The products of the reference's inference driver (scripts/infer/mosei_eval_infer.py: {split}_y_prob.npy, {split}_beta_mean.npy),
    accumulated where the forward runs: probabilities, per-sample mean beta and -- single-label -- the argmax of every sample, without
    targets and without a read-back per batch.

    PredictionLog(num_outputs, capacity, kind="multi_label" | "single_label", device=...): `capacity` is the number of samples the
    log holds.  multi_label logs p = sigmoid(logits) (the bits EpochStats logs for the same logits), single_label the fp32 softmax
    over the classes (row maximum subtracted) and the first maximal logit's index (torch.argmax's rule).

    update(logits, beta=None, n_valid=None) enqueues ONE launch (hriemo_predict_log) on the current stream and reads nothing back; it
    can be recorded into a captured step (dp.EvalStep(log=...)).  beta: None or B * k values, k per sample; the log keeps each
    sample's mean (float64 sum in index order, stored as fp32).  n_valid: None or a 1-element int32 tensor on the device (a Python
    int on the CPU path too): only the first clamp(n_valid, 1, B) samples are logged, whatever the rows behind them hold.

    reset() starts over (the log needs no clearing: only entries in front of the cursor are ever read).

    arrays(): ONE read-back -> dict(y_prob float32 [n, C], sample-major as the reference saves it; beta_mean float32 [n], or None
    when no update carried beta; pred int32 [n], single_label only; n_nonfinite, the number of NaN / Inf logits logged; n_samples).
    RuntimeError if the log overflowed.

    CPU tensors take the same definitions in plain torch / numpy (sigmoid and softmax in float64, rounded to fp32)."""

    def __init__(self, num_outputs, capacity, kind="multi_label", device="cuda"):
        if kind not in ("multi_label", "single_label"):
            raise ValueError("PredictionLog: kind is 'multi_label' or 'single_label'")
        if int(num_outputs) < 1 or int(capacity) < 1:
            raise ValueError("PredictionLog: num_outputs and capacity are positive")
        self.C, self.capacity, self.kind = int(num_outputs), int(capacity), kind
        self.device = torch.device(device)
        self.multi = kind == "multi_label"
        # everything arrays() reads back is ONE buffer: counters int32[4] | probs fp32 [C, capacity] | beta_mean fp32 [capacity] |
        # pred int32 [capacity]
        C, cap = self.C, self.capacity
        self._parts = (16, 16 + 4 * C * cap, 16 + 4 * (C + 1) * cap)
        self._buf = torch.zeros(16 + 4 * (C + 2) * cap, dtype=torch.uint8, device=self.device)
        self.counters, self.probs, self.beta_mean, self.pred = self._views(self._buf)
        self._has_beta = False

    def _views(self, buf):
        a, b, c = self._parts
        return (buf[:a].view(torch.int32), buf[a:b].view(torch.float32).view(self.C, self.capacity), buf[b:c].view(torch.float32),
                buf[c:].view(torch.int32))

    def reset(self):
        self.counters.zero_()

    def update(self, logits, beta=None, n_valid=None):
        if logits.dim() != 2 or logits.shape[1] != self.C:
            raise ValueError(f"PredictionLog.update: logits of shape {tuple(logits.shape)}; expected [B, {self.C}]")
        B = logits.shape[0]
        if B < 1:
            raise ValueError("PredictionLog.update: an empty batch")
        if beta is not None and (beta.numel() == 0 or beta.numel() % B != 0):
            raise ValueError(f"PredictionLog.update: beta of {beta.numel()} values for {B} samples")
        if logits.device.type != self.device.type:
            raise ValueError(f"PredictionLog.update: logits on {logits.device}; the log lives on {self.device}")
        self._has_beta = self._has_beta or beta is not None
        if not logits.is_cuda:
            return self._update_cpu(logits, beta, n_valid, B)
        from . import _lib, _ops
        p = _ops._p
        nv = _ops._n_valid_word((n_valid,), logits)
        x = logits.detach().contiguous().float()
        bt = beta.detach().contiguous().float() if beta is not None else None
        _lib.call("hriemo_predict_log", p(x), p(bt), bt.numel() // B if bt is not None else 0, p(nv), B, self.C, 0 if self.multi else 1,
                  p(self.probs), p(self.beta_mean), None if self.multi else p(self.pred), self.capacity, p(self.counters), _ops._stream())

    def _update_cpu(self, logits, beta, n_valid, B):
        nv = B if n_valid is None else min(max(int(n_valid), 1), B)
        ctr = self.counters
        ctr[1] += nv
        cur = int(ctr[0])
        if cur < 0 or cur + nv > self.capacity:
            ctr[2] = 1
            return
        x = logits.detach()[:nv].float()
        if self.multi:
            pr = torch.sigmoid(x.double()).float()
        else:
            pr = torch.softmax(x.double(), dim=1).float()
            self.pred[cur:cur + nv] = x.argmax(dim=1).to(torch.int32)
        self.probs[:, cur:cur + nv] = pr.t()
        if beta is not None:
            self.beta_mean[cur:cur + nv] = beta.detach().reshape(B, -1)[:nv].double().mean(dim=1).float()
        ctr[3] += int((~torch.isfinite(x)).sum())
        ctr[0] = cur + nv

    def arrays(self):
        ctr, probs, beta_mean, pred = self._views(self._buf.cpu())                    # the one read-back
        ctr = dict(zip(_PL, (int(v) for v in ctr.tolist())))
        if ctr["overflow"]:
            raise RuntimeError(f"PredictionLog: the log of {self.capacity} samples overflowed ({ctr['n_samples']} samples were offered); "
                               "size capacity for the split")
        n = ctr["cursor"]
        out = {"y_prob": np.ascontiguousarray(probs[:, :n].numpy().T), "beta_mean": beta_mean[:n].numpy().copy() if self._has_beta else None,
               "n_nonfinite": ctr["n_nonfinite"], "n_samples": ctr["n_samples"]}
        if not self.multi:
            out["pred"] = pred[:n].numpy().copy()
        return out


# ------------------------------------------------------------------------------------------------------------------- attention log
_AL = ("cursor", "n_offered", "n_batches", "spare")             # counters[4] of hriemo_attn_log_plan
ENCODER_SITES = ("audio_self", "text_self", "audio_queries_text", "text_queries_audio")      # the keys of a layer's map dict


class AttentionLog:
    """The third product of the reference's inference driver (scripts/infer/mosei_eval_infer.py --dump_attn --attn_max_samples K:
    {split}_attentions.pt), accumulated where the forward runs: the head-averaged attention maps of the FIRST `capacity` samples of
    a split, without an intermediate [B, Lq, Lk] tensor and without a read-back per batch.

    AttentionLog(capacity, pad_to=(L_a, L_t), num_layers_fusion=2, num_layers_decoder=2, num_emotions=4, encoder=True,
    decoder=True, device=...).  State: one fp32 [capacity, Lq, Lk] tensor per attention site -- ``encoder_maps``: per fusion layer
    {audio_self [L_a, L_a], text_self [L_t, L_t], audio_queries_text [L_a, L_t], text_queries_audio [L_t, L_a]}; ``decoder_maps``:
    per decoder layer [N_e, L_t] -- and ``counters`` int32 [4] {cursor, n_offered, n_batches, spare}, ``window`` int32 [4]
    {slot0, n_take, 0, 0}, ``lengths`` int32 [2, capacity] (audio row, text row); ``nbytes`` is all of it.  encoder=False /
    decoder=False: that half has no tensors and its exports are not launched at all.

    The rule (hriemo_attn_log_plan; `plan` below is the same rule in plain torch for CPU tensors): a pass that offers nv samples
    takes n_take = clamp(capacity - cursor, 0, nv) of them, samples 0 .. n_take-1 into slots cursor .. cursor+n_take-1, their
    lengths beside them; cursor += n_take, n_offered += nv, n_batches += 1.  A full log takes nothing and is the normal end state.
    A cursor outside [0, capacity] counts as full.

    Fed by ``forward_packed(..., attn_log=log)`` (needs set_varlen_maps(True)) and, inside the graph, by
    ``dp.EvalStep(..., attn_log=log)``: one plan launch at the top of the pass, then every attention site exports straight into
    its slots.  ``append(maps, lengths, n_valid=None)`` feeds maps that exist already (the structure forward(return_attention=True)
    returns, padded to pad_to) through the same rule.

    reset(): counters to zero (the maps need no clearing: only slots in front of the cursor are ever read).
    arrays(): reads back the first `cursor` slots only -> dict(encoder: per layer {name: float32 [n, Lq, Lk]}, decoder: per layer
    float32 [n, N_e, L_t], lengths int32 [2, n], n_logged, n_offered).
    as_reference(batch_size): the reference's ``collected_attns`` -- {"encoder": [per batch [per layer {name: array}]], "decoder":
    [per batch [per layer array]]}, every batch of `batch_size` logged samples cropped to its own longest audio and text length (the
    reference's pad-to-batch-max collate; the decoder's keys are the text length).  Two differences from the reference: the log
    holds exactly the first `capacity` samples (the reference admits whole batches while seen < max, so it can run over), and PAD
    query rows are zeros, as in the packed export everywhere else."""

    def __init__(self, capacity, pad_to, num_layers_fusion=2, num_layers_decoder=2, num_emotions=4, encoder=True, decoder=True,
                 device="cuda"):
        if int(capacity) < 1:
            raise ValueError("AttentionLog: capacity is positive")
        try:
            La, Lt = (int(v) for v in pad_to)
        except (TypeError, ValueError):
            raise ValueError("AttentionLog: pad_to = (L_a, L_t)") from None
        if Lt < 1 or La < Lt:
            raise ValueError(f"AttentionLog: pad_to = ({La}, {Lt}); 1 <= L_t <= L_a (the gate fuses over the text length)")
        if not (encoder or decoder):
            raise ValueError("AttentionLog: neither the encoder's nor the decoder's maps were asked for")
        if int(num_layers_fusion) < 1 or int(num_layers_decoder) < 1 or int(num_emotions) < 1:
            raise ValueError("AttentionLog: num_layers_fusion, num_layers_decoder and num_emotions are positive")
        self.capacity, self.pad_to = int(capacity), (La, Lt)
        self.num_layers_fusion, self.num_layers_decoder, self.num_emotions = int(num_layers_fusion), int(num_layers_decoder), int(num_emotions)
        self.encoder, self.decoder = bool(encoder), bool(decoder)
        self.device = torch.device(device)
        cap, dev = self.capacity, self.device
        # counters int32[4] | window int32[4] | lengths int32 [2, capacity]: ONE buffer, one read-back
        self._small = torch.zeros(8 + 2 * cap, dtype=torch.int32, device=dev)
        self.counters, self.window, self.lengths = self._views(self._small)
        shapes = dict(zip(ENCODER_SITES, ((La, La), (Lt, Lt), (La, Lt), (Lt, La))))
        self.encoder_maps = [{k: torch.zeros((cap,) + s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
                             for _ in range(self.num_layers_fusion)] if self.encoder else []
        self.decoder_maps = [torch.zeros(cap, self.num_emotions, Lt, dtype=torch.float32, device=dev)
                             for _ in range(self.num_layers_decoder)] if self.decoder else []

    @classmethod
    def for_model(cls, model, capacity, pad_to, encoder=True, decoder=True, device=None):
        """the log of `model` (a FusionWithEmotionDecoder, or the MOSEI wrapper around one): layer counts, num_emotions and the
        device are the model's"""
        core = getattr(model, "backbone", model)
        if not (hasattr(core, "cross_modal") and hasattr(core, "emotion_decoder")):
            raise TypeError("AttentionLog.for_model: the model has no fusion encoder / emotion decoder (FusionWithEmotionDecoder or its MOSEI wrapper)")
        if device is None:
            device = next(core.parameters()).device
        return cls(capacity, pad_to, len(core.cross_modal.layers), len(core.emotion_decoder.layers), core.emotion_decoder.num_emotions,
                   encoder=encoder, decoder=decoder, device=device)

    def _views(self, buf):
        return buf[:4], buf[4:8], buf[8:].view(2, self.capacity)

    def _tensors(self):
        return [t for layer in self.encoder_maps for t in layer.values()] + list(self.decoder_maps)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._tensors()) + self._small.numel() * 4

    def reset(self):
        self._small[:8].zero_()

    def mismatch(self, model, pad=None):
        """None, or what keeps this log from taking `model`'s maps at the padded lengths `pad` -- as one sentence"""
        core = getattr(model, "backbone", model)
        if pad is not None and (int(pad[0]), int(pad[1])) != self.pad_to:
            return f"the log's pad_to is {self.pad_to}, the forward's padded lengths are {(int(pad[0]), int(pad[1]))}"
        have = (len(core.cross_modal.layers), len(core.emotion_decoder.layers), core.emotion_decoder.num_emotions)
        for name, mine, its, on in (("num_layers_fusion", self.num_layers_fusion, have[0], self.encoder),
                                    ("num_layers_decoder", self.num_layers_decoder, have[1], self.decoder),
                                    ("num_emotions", self.num_emotions, have[2], self.decoder)):
            if on and mine != its:
                return f"the log's {name} is {mine}, the model's is {its}"
        if self._small.device != next(core.parameters()).device:
            return f"the log lives on {self._small.device}, the model on {next(core.parameters()).device}"
        return None

    # ---- the window rule
    def plan(self, lens=None, n_valid=None, B=None, record=True):
        """The top of one pass: lens int32 [2, B] on the log's device (None: no lengths are logged), n_valid None or a 1-element
        int32 tensor on the device (a Python int on the CPU path too).  ONE launch (hriemo_attn_log_plan), nothing read back.
        record=False: the closed window {0, 0} and nothing else (hriemo_attn_log_close) -- a warm-up pass."""
        if lens is not None:
            if lens.dim() != 2 or lens.shape[0] != 2 or lens.dtype != torch.int32 or not lens.is_contiguous():
                raise ValueError(f"AttentionLog.plan: lengths of shape {tuple(lens.shape)} / {lens.dtype} (expected contiguous int32 [2, B])")
            if lens.device.type != self.device.type:
                raise ValueError(f"AttentionLog.plan: lengths on {lens.device}; the log lives on {self.device}")
            B = lens.shape[1] if B is None else B
            if lens.shape[1] != B:
                raise ValueError(f"AttentionLog.plan: lengths of {lens.shape[1]} samples for B = {B}")
        if B is None or int(B) < 1:
            raise ValueError("AttentionLog.plan: B (or the lengths block) is required, B >= 1")
        B = int(B)
        if self.device.type != "cuda":
            return self._plan_cpu(lens, n_valid, B, record)
        from . import _lib, _ops
        p = _ops._p
        if not record:
            _lib.call("hriemo_attn_log_close", p(self.window), _ops._stream())
            return
        nv = _ops._n_valid_word((n_valid,), self.counters)
        _lib.call("hriemo_attn_log_plan", p(lens), p(nv), B, self.capacity, p(self.counters), p(self.window),
                  p(self.lengths) if lens is not None else None, _ops._stream())

    def _plan_cpu(self, lens, n_valid, B, record):
        ctr, win = self.counters, self.window
        win.zero_()
        if not record:
            return
        nv = B if n_valid is None else min(max(int(n_valid), 1), B)
        cur = int(ctr[0])
        take = min(self.capacity - cur, nv) if 0 <= cur <= self.capacity else 0
        if lens is not None and take > 0:
            self.lengths[:, cur:cur + take] = lens[:, :take]
        win[0], win[1] = cur, take
        ctr[0] = cur + take if take > 0 else cur
        ctr[1] += nv
        ctr[2] += 1

    def sites(self, B):
        """(per fusion layer {name: _ops.LogSite} | None, per decoder layer _ops.LogSite | None) for a pass of B samples: what the
        model's attention sites take in the place of their need flag"""
        from ._ops import LogSite
        enc = [{k: LogSite(t, self.window, self.capacity, B) for k, t in layer.items()} for layer in self.encoder_maps]
        dec = [LogSite(t, self.window, self.capacity, B) for t in self.decoder_maps]
        return enc or None, dec or None

    def append(self, maps, lengths, n_valid=None):
        """Maps that exist already through the window rule: maps = {"encoder": [per layer {name: [B, Lq, Lk]}], "decoder": [per
        layer [B, N_e, L_t]]} at the log's padded lengths (the half the log does not keep is ignored), lengths int32 [2, B]."""
        lengths = torch.as_tensor(lengths, dtype=torch.int32).to(self.device).contiguous()
        B = lengths.shape[1] if lengths.dim() == 2 else -1
        pairs = []
        if self.encoder:
            if len(maps["encoder"]) != self.num_layers_fusion:
                raise ValueError(f"AttentionLog.append: {len(maps['encoder'])} encoder layers; the log keeps {self.num_layers_fusion}")
            pairs += [(layer[k], mine[k]) for layer, mine in zip(maps["encoder"], self.encoder_maps) for k in ENCODER_SITES]
        if self.decoder:
            if len(maps["decoder"]) != self.num_layers_decoder:
                raise ValueError(f"AttentionLog.append: {len(maps['decoder'])} decoder layers; the log keeps {self.num_layers_decoder}")
            pairs += list(zip(maps["decoder"], self.decoder_maps))
        for src, dst in pairs:
            if tuple(src.shape) != (B,) + tuple(dst.shape[1:]) or src.device.type != self.device.type:
                raise ValueError(f"AttentionLog.append: a map of shape {tuple(src.shape)} on {src.device}; expected {(B,) + tuple(dst.shape[1:])} on {self.device}")
        self.plan(lengths, n_valid, B)
        for src, dst in pairs:
            self._append_one(src, dst)

    def _append_one(self, src, dst):
        """one site's [B, Lq, Lk] maps into its log under the current window"""
        src = src.detach().contiguous().float()
        if self.device.type != "cuda":
            slot0, take = int(self.window[0]), int(self.window[1])
            take = min(take, src.shape[0], self.capacity - slot0) if slot0 >= 0 else 0
            if take > 0:
                dst[slot0:slot0 + take] = src[:take]
            return
        from . import _lib, _ops
        p = _ops._p
        _lib.call("hriemo_attn_log_append", p(src), src.shape[0], src[0].numel(), p(self.window), p(dst), self.capacity, _ops._stream())

    # ---- read-back
    def arrays(self):
        ctr, _, lengths = self._views(self._small.cpu())
        ctr = dict(zip(_AL, (int(v) for v in ctr.tolist())))
        n = min(max(ctr["cursor"], 0), self.capacity)
        host = lambda t: t[:n].cpu().numpy().copy()          # noqa: E731
        return {"encoder": [{k: host(t) for k, t in layer.items()} for layer in self.encoder_maps],
                "decoder": [host(t) for t in self.decoder_maps], "lengths": lengths[:, :n].numpy().copy(), "n_logged": n,
                "n_offered": ctr["n_offered"]}

    def as_reference(self, batch_size):
        if int(batch_size) < 1:
            raise ValueError("AttentionLog.as_reference: batch_size is positive")
        arr = self.arrays()
        out = {"encoder": [], "decoder": []}
        for i in range(0, arr["n_logged"], int(batch_size)):
            j = min(i + int(batch_size), arr["n_logged"])
            ma, mt = int(arr["lengths"][0, i:j].max()), int(arr["lengths"][1, i:j].max())
            crop = dict(zip(ENCODER_SITES, ((ma, ma), (mt, mt), (ma, mt), (mt, ma))))
            if self.encoder:
                out["encoder"].append([{k: np.ascontiguousarray(layer[k][i:j, :crop[k][0], :crop[k][1]]) for k in ENCODER_SITES}
                                       for layer in arr["encoder"]])
            if self.decoder:
                out["decoder"].append([np.ascontiguousarray(t[i:j, :, :mt]) for t in arr["decoder"]])
        return out


ACT_HALVES = ("forward", "gradient")
ACT_PROBE_ROWS = 32            # rows per chunk of hriemo_act_probe (hriemo_act_probe_rows())
_ACT_ENC = ("audio_self", "text_self", "audio_cross", "audio_ffn", "text_cross", "text_ffn")      # CrossModalBlock._site order
_ACT_DEC = ("self", "cross", "ffn")                                                               # ExplainableDecoderLayer._site order
_ACT_FIELDS = ("have", "n_rows", "n_bad", "first_bad_row", "absmax", "sumsq")


def activation_site_names(num_layers_fusion, num_layers_decoder):
    """the sites of an ActivationLog in forward order (23 for two encoder and two decoder layers)"""
    names = ["input.audio", "input.text"]
    names += [f"enc{i}.{s}" for i in range(int(num_layers_fusion)) for s in _ACT_ENC]
    names += ["gate.w", "gate.fused"]
    names += [f"dec{j}.{s}" for j in range(int(num_layers_decoder)) for s in _ACT_DEC]
    return names + ["logits"]


class ActivationLog:
    """Activation-side blame for a step that runs inside a graph: per sub-layer, the statistics of its output (forward half) and of
    the summed gradient that arrives at its backward for that output (gradient half) -- n_rows, n_bad (non-finite elements),
    first_bad_row, absmax and sumsq over the finite elements of the rows that count -- written by the pass itself into a ring of
    `capacity` records in device memory (csrc/actlog.hip), read back once when asked.  Where ``optim.HealthLog.blame()`` names the
    parameters whose gradient was not finite, ``blame()`` here names the sub-layer, sample and position where a non-finite value
    first appeared.

    ``ActivationLog.for_model(model, capacity=16, every=1, sites=None, device=None, max_rows=65536)`` builds the site table of a
    FusionWithEmotionDecoder or its MOSEI wrapper (``activation_site_names``): input.audio, input.text (the rows the encoder starts
    from); per encoder layer enc{i}.audio_self, .text_self, .audio_cross, .audio_ffn, .text_cross, .text_ffn and per decoder layer
    dec{j}.self, .cross, .ffn (each sub-layer's LayerNorm output); gate.w (the gate vector [B, d]), gate.fused (the decoder's
    memory); logits.  sites: names or fnmatch patterns -- only those launch a probe; the record keeps every site's words, the
    others with have = 0.  every: pass p of the run records iff p % every == 0.  max_rows sizes the per-site partial sums: the
    largest row count of one activation buffer a pass may probe.

    Rows that count: those of the real sequences of the batch inside their lengths -- PAD rows, the filler sequence and surplus rows
    of a bucket plan and the ghost utterances of a short batch (n_valid) never do, whatever they hold.  The gradient half of a site
    no backward node receives a gradient for keeps have = 0: gate.w, the input.* sites when the inputs need no gradient, every site of an
    evaluation pass.  Under a
    ``GradScaler`` the gradient half holds the statistics of the SCALED gradients (the log sits in front of the unscale).

    Use: eagerly ``with log.watch(): out = model(...); loss.backward(); log.close_backward()``; in a captured trainer step
    ``dp.DataParallelStep.attach_activations(log)`` before capture; in a captured evaluation ``dp.EvalStep(..., act_log=log)``
    (forward half only).  Warm-up passes of a capture never record.  bf16 precision only (both GEMM modes): under
    ``set_precision("fp32")`` a pass with a log installed raises NotImplementedError.

    arrays(): one read-back -> {"sites", "n_passes", "n_recorded", "pass" [n], "halves" [n], "forward": {field: [n, S]},
    "gradient": {field: [n, S]}}, records oldest first, fields have, n_rows, n_bad, first_bad_row, absmax, sumsq and rms =
    sqrt(sumsq / (n_rows * d)) formed here in float64.  blame(record=-1): None if the record holds no non-finite element, else
    {"half", "site", "sample", "position", "n_bad"}: the first site in forward order whose forward half has n_bad > 0; if the
    forward is clean, the first site in backward (reverse) order whose gradient half has.  reset() clears the ring.
    ``decode`` and ``blame_of`` are the same rules on a host image of the state: the CPU mirror."""

    HEADER = 8                 # counters int32 [4] | window int32 [4]
    REC_HEADER, ENTRY = 4, 8

    def __init__(self, names, widths, keys=None, capacity=16, every=1, sites=None, device="cuda", max_rows=65536):
        import fnmatch
        if int(capacity) < 1 or int(every) < 1 or int(max_rows) < 1:
            raise ValueError("ActivationLog: capacity, every and max_rows are positive")
        self.names, self.widths = list(names), [int(w) for w in widths]
        if len(self.names) != len(self.widths) or not self.names:
            raise ValueError("ActivationLog: one width per site, at least one site")
        self.capacity, self.every, self.max_rows = int(capacity), int(every), int(max_rows)
        self.device = torch.device(device)
        S = self.S = len(self.names)
        if sites is None:
            chosen = set(self.names)
        else:
            chosen = set()
            for pat in ([sites] if isinstance(sites, str) else list(sites)):
                hit = fnmatch.filter(self.names, pat)
                if not hit:
                    raise ValueError(f"ActivationLog: no site matches {pat!r}; the sites are {', '.join(self.names)}")
                chosen.update(hit)
        self.selected = [n for n in self.names if n in chosen]
        # key -> site index, selected sites only: what _ops.probe looks up (a sub-layer's dropout site id, or the site's name)
        by_name = {n: i for i, n in enumerate(self.names)}
        self.index = {k: by_name[n] for k, n in (keys or {}).items() if n in chosen}
        self.index.update({n: by_name[n] for n in self.selected})
        self.row_len = [None] * S          # rows per sample of the site's buffer, noted by its first probe: first_bad_row -> (sample, position)
        self.recording = True              # False: the passes are warm-up passes (paused())
        self.open = [False, False]         # a pass's forward / gradient half is open: begin_pass .. end_forward / close_backward
        self.n_valid = None                # the step's device word: the ghosts behind it never count
        self.chunk_cap = (self.max_rows + ACT_PROBE_ROWS - 1) // ACT_PROBE_ROWS
        self._counts_at = self.HEADER
        self._ring_at = self.HEADER + (2 * S + 3) // 4 * 4
        self.rec_words = self.REC_HEADER + 2 * S * self.ENTRY
        # counters | window | counts | ring: ONE buffer, one read-back
        self._small = torch.zeros(self._ring_at + self.capacity * self.rec_words, dtype=torch.int32, device=self.device)
        self.counters, self.window = self._small[:4], self._small[4:8]
        self.counts, self.ring = self._small[self._counts_at:self._counts_at + 2 * S], self._small[self._ring_at:]
        self.partial = None
        if self.device.type == "cuda":
            from . import _lib
            if _lib.lib().hriemo_act_probe_rows() != ACT_PROBE_ROWS:
                raise RuntimeError("ActivationLog: the library's chunk of rows is not this module's")
            self.partial = torch.zeros(2 * S * self.chunk_cap * 8, dtype=torch.float32, device=self.device)

    @classmethod
    def for_model(cls, model, capacity=16, every=1, sites=None, device=None, max_rows=65536):
        core = getattr(model, "backbone", model)
        if not (hasattr(core, "cross_modal") and hasattr(core, "beta_gate") and hasattr(core, "emotion_decoder")
                and hasattr(core, "_run")):
            raise NotImplementedError(f"ActivationLog.for_model: {type(model).__name__} is not served (FusionWithEmotionDecoder and "
                                      "MoseiFusionWithEmotionDecoder are; FusionClassifier and the legacy block and gate are open)")
        enc, dec = core.cross_modal.layers, core.emotion_decoder.layers
        names = activation_site_names(len(enc), len(dec))
        d, ne = core.emotion_decoder.d_model, core.emotion_decoder.num_emotions
        widths = [ne if n == "logits" else d for n in names]
        keys = {}
        for i, layer in enumerate(enc):
            keys.update({layer._site[j]: f"enc{i}.{s}" for j, s in enumerate(_ACT_ENC)})
        # the gradient of the encoder's input rows is what layer 0's self-attentions return for them
        keys.update({("input", enc[0]._site[0]): "input.audio", ("input", enc[0]._site[1]): "input.text"})
        for j, layer in enumerate(dec):
            keys.update({layer._site[k]: f"dec{j}.{s}" for k, s in enumerate(_ACT_DEC)})
        if device is None:
            device = next(core.parameters()).device
        return cls(names, widths, keys, capacity, every, sites, device, max_rows)

    @property
    def nbytes(self):
        return self._small.numel() * 4 + (self.partial.numel() * 4 if self.partial is not None else 0)

    def reset(self):
        self._small.zero_()

    # ---- the pass
    def _guard(self):
        from . import _ops
        if _ops.precision() == "fp32":
            raise NotImplementedError('ActivationLog: set_precision("fp32") is not served (the fp32 sub-layers have no probes); '
                                      'detach the log or switch to set_precision("bf16")')

    def watch(self):
        """``with log.watch():`` -- the log is installed on the step context in force: every pass of a served model inside the block
        plans, probes and folds its forward half; ``close_backward()`` behind ``loss.backward()`` folds the gradient half.  Only a
        pass of the whole model is a pass of the log: a sub-module called on its own inside the block (``model.cross_modal(...)``,
        ``model.beta_gate(...)``) has no plan launch in front and launches no probe; a backward that runs behind
        ``close_backward()`` launches none either.  Entering the block forgets the n_valid word of a step the log served before."""
        return _ActWatch(self)

    def paused(self):
        """``with log.paused():`` -- the passes inside are warm-up passes: they run under the closed window and leave no trace"""
        return _ActPaused(self)

    def begin_pass(self):
        """the top of a pass, in front of every fork: ONE launch (hriemo_act_log_plan)"""
        self._guard()
        from . import _lib, _ops
        p = _ops._p
        _lib.call("hriemo_act_log_plan", 1 if self.recording else 0, self.every, self.capacity, self.S, p(self.counters), p(self.window),
                  p(self.counts), p(self.ring), _ops._stream())
        self.open = [True, True]

    def _fold(self, half):
        from . import _lib, _ops
        p = _ops._p
        _lib.call("hriemo_act_log_fold", p(self.partial), p(self.counts), p(self.window), half, self.S, self.chunk_cap, self.capacity,
                  p(self.ring), _ops._stream())

    def end_forward(self):
        """the end of the forward, behind every join: the forward half's fold"""
        self._fold(0)
        self.open[0] = False

    def close_backward(self):
        """behind ``loss.backward()``: the gradient half's fold"""
        self._fold(1)
        self.open[1] = False

    def probe(self, site, half, x, seq):
        """hriemo_act_probe of x (rows laid out as the _ops.Seq `seq`) for site index `site` on the current stream"""
        from . import _lib, _ops
        p = _ops._p
        if x.dtype not in (torch.bfloat16, torch.float32) or x.device != self._small.device:
            raise TypeError(f"ActivationLog: a {x.dtype} activation on {x.device} at site {self.names[site]}")
        d = x.shape[-1]
        x2 = x.reshape(-1, d)
        if x2.stride(1) != 1 or x2.data_ptr() != x.data_ptr():
            raise ValueError(f"ActivationLog: site {self.names[site]} handed rows that are not dense")
        n_rows = x2.shape[0]
        if n_rows != seq.N:
            raise ValueError(f"ActivationLog: site {self.names[site]}: {n_rows} rows, the layout has {seq.N}")
        if n_rows > self.max_rows:
            raise ValueError(f"ActivationLog: site {self.names[site]} has {n_rows} rows; the log was sized for max_rows={self.max_rows}")
        self.row_len[site] = seq.L
        kpm = None
        if not seq.packed and seq.kpm is not None:
            kpm = seq.kpm if seq.kpm.is_contiguous() else seq.kpm.contiguous()
        _lib.call("hriemo_act_probe", p(x2), 0 if x.dtype == torch.bfloat16 else 1, n_rows, d, x2.stride(0), p(seq.cu) if seq.packed else None,
                  p(kpm), seq.Breal, seq.L, p(self.n_valid), p(self.window), site, half, self.S, self.chunk_cap, p(self.partial),
                  p(self.counts), _ops._stream())

    # ---- read-back
    @classmethod
    def decode(cls, image, names, widths, capacity):
        """The records of a host image of the state (counters | window | counts | ring, int32), oldest first.  Closed passes leave
        no record; a ring that wrapped holds the latest `capacity` records."""
        img = np.ascontiguousarray(np.asarray(image, dtype=np.int32))
        S, cap = len(names), int(capacity)
        ring_at = cls.HEADER + (2 * S + 3) // 4 * 4
        rw = cls.REC_HEADER + 2 * S * cls.ENTRY
        if img.size != ring_at + cap * rw:
            raise ValueError(f"ActivationLog.decode: an image of {img.size} words; {S} sites and capacity {cap} make {ring_at + cap * rw}")
        n_passes, n_rec = int(img[0]), int(img[1])
        n = min(max(n_rec, 0), cap)
        order = [(n_rec - n + i) % cap for i in range(n)]
        recs = img[ring_at:].reshape(cap, rw)[order] if n else np.zeros((0, rw), np.int32)
        ent = recs[:, cls.REC_HEADER:].reshape(n, 2, S, cls.ENTRY)
        out = {"sites": list(names), "n_passes": n_passes, "n_recorded": n_rec, "pass": recs[:, 0].copy(), "halves": recs[:, 1].copy()}
        w = np.asarray(widths, dtype=np.float64)[None, :]
        for h, half in enumerate(ACT_HALVES):
            e = ent[:, h]
            f = {k: e[:, :, i].copy() for i, k in enumerate(_ACT_FIELDS[:4])}
            f["absmax"] = e[:, :, 4].copy().view(np.float32)
            f["sumsq"] = e[:, :, 5].copy().view(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                rms = np.sqrt(f["sumsq"].astype(np.float64) / (f["n_rows"].astype(np.float64) * w))
            f["rms"] = np.where((f["have"] == 1) & (f["n_rows"] > 0), rms, np.nan)
            out[half] = f
        return out

    @staticmethod
    def blame_of(arr, row_len, record=-1):
        """the blame rule on decoded records: forward before gradient, forward order, reverse order for the gradients"""
        n = len(arr["pass"])
        if n == 0:
            return None
        r = range(n)[record]
        S = len(arr["sites"])
        for half, order in (("forward", range(S)), ("gradient", range(S - 1, -1, -1))):
            f = arr[half]
            for s in order:
                if f["have"][r, s] == 1 and f["n_bad"][r, s] > 0:
                    row, L = int(f["first_bad_row"][r, s]), row_len[s]
                    if L is None or L < 1 or row < 0:
                        sample = position = None
                    else:
                        sample, position = row // L, row % L
                    return {"half": half, "site": arr["sites"][s], "sample": sample, "position": position, "n_bad": int(f["n_bad"][r, s])}
        return None

    def arrays(self):
        return self.decode(self._small.cpu().numpy(), self.names, self.widths, self.capacity)

    def blame(self, record=-1):
        return self.blame_of(self.arrays(), self.row_len, record)

    @property
    def n_recorded(self):
        return int(self._small[1].item())


class _ActWatch:
    def __init__(self, log):
        self.log, self.prev = log, None

    def __enter__(self):
        from . import _ops
        self.log._guard()
        self.ctx = _ops.CTX
        self.log.n_valid, self.log.open = None, [False, False]
        self.prev, self.ctx.act_log = self.ctx.act_log, self.log
        return self.log

    def __exit__(self, *exc):
        self.ctx.act_log, self.log.open = self.prev, [False, False]
        return False


class _ActPaused:
    def __init__(self, log):
        self.log, self.prev = log, True

    def __enter__(self):
        self.prev, self.log.recording = self.log.recording, False
        return self.log

    def __exit__(self, *exc):
        self.log.recording = self.prev
        return False


def evaluate_packed(model, batches, loss_fn, stats, pad_to=None, step=None):
    """The reference's evaluate() bodies (train_fusion_seq_level_decoder.py:342-372, train_mosei_fusion_seq_level_decoder.py:432-495)
    on ragged batches: model.eval() under torch.no_grad(); for every data.collate_seq_packed batch (rows_a, lengths_a, rows_t,
    lengths_t, labels): forward_packed -> loss_fn(logits, beta, labels) -> stats.update.  Nothing is read back per batch --
    ``stats.result()`` afterwards is the epoch's one read-back.  Without `step` these are eager launches; the module's training
    mode is restored.  step: a ``dp.EvalStep`` built on this model with this loss_fn and these stats -- every batch is then ONE
    ``eval_packed`` (a graph replay that holds the forward, the loss and the statistics' update; short batches included).  A step
    that holds no graph yet is captured on the spot from the first batch, which needs pad_to=(L_a, L_t).  Returns `stats`."""
    if step is not None:
        if step.model is not model or step.stats is not stats or step.loss_fn is not loss_fn:
            raise ValueError("evaluate_packed(step=...): the EvalStep was built on another model, loss_fn or stats")
        for rows_a, len_a, rows_t, len_t, y in batches:
            if not step.captured:
                if pad_to is None:
                    raise ValueError("evaluate_packed(step=...): pad_to=(L_a, L_t) is required to capture the step from the first batch")
                step.capture_packed(rows_a, rows_t, len_a, len_t, y, pad_to=pad_to)
            step.eval_packed(rows_a, rows_t, len_a, len_t, y)
        return stats
    was = model.training
    dev = next(model.parameters()).device
    model.eval()
    try:
        with torch.no_grad():
            for rows_a, len_a, rows_t, len_t, y in batches:
                y = y.to(dev, non_blocking=True)
                logits, beta, _ = model.forward_packed(rows_a.to(dev, non_blocking=True), rows_t.to(dev, non_blocking=True), len_a, len_t,
                                                       pad_to=pad_to)
                stats.update(logits, beta, y, loss_fn(logits, beta, y))
    finally:
        model.train(was)
    return stats


def evaluate_store(model, store, batches, loss_fn, stats, step=None):
    """evaluate_packed() on a ``data.DeviceFeatureStore``: `batches` are lists of utterance ids (``store.batches(B, shuffle=False)``),
    nothing but those ids and their lengths crosses to the device per batch.  Without `step`: model.eval() under torch.no_grad(),
    ``store.fetch(ids)`` -> forward_packed (pad_to = store.pad_to) -> loss_fn -> stats.update, eager launches.  step: a
    ``dp.EvalStep`` built on this model with this loss_fn and these stats -- every batch is then ONE ``eval_store`` (plan upload,
    one gather launch per operand, one graph replay).  A step that holds no graph yet is captured on the spot from the first batch,
    which therefore must be a full one (no later batch may be larger).  A step that IS captured must have been captured on this very
    store (``step.store is store``): eval_store's ids refer to the captured store, so a step of the validation store handed in with
    the test store would evaluate the wrong split without a sign -- ValueError before anything runs (one EvalStep per store, or
    ``step.release_graph()`` first).  Returns `stats`."""
    if step is not None:
        if step.model is not model or step.stats is not stats or step.loss_fn is not loss_fn:
            raise ValueError("evaluate_store(step=...): the EvalStep was built on another model, loss_fn or stats")
        if step.captured and step.store is not store:
            raise ValueError("evaluate_store(step=...): the EvalStep was captured " + ("by capture_packed" if step.store is None else
                             "on another store") + "; its ids would not refer to this store (one step per store, or release_graph() first)")
        for ids in batches:
            if not step.captured:
                step.capture_store(store, ids)
            step.eval_store(ids)
        return stats
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            for ids in batches:
                rows_a, len_a, rows_t, len_t, y = store.fetch(ids)
                logits, beta, _ = model.forward_packed(rows_a, rows_t, len_a, len_t, pad_to=store.pad_to)
                stats.update(logits, beta, y, loss_fn(logits, beta, y))
    finally:
        model.train(was)
    return stats
