"""Losses of the reference's trainers as ONE kernel each (value + gradients, hriemo_fusion_loss):
  fusion_step_loss        scripts/fusion/train_fusion_seq_level_decoder.py:312-326 (multi-label branch):
                          BCEWithLogits(logits, y) - 0.01*mean(beta*(1-beta))
  fusion_step_loss_single_label   the same trainer's single_label branch (:312-314, criterion nn.CrossEntropyLoss() :413-414):
                          CrossEntropy(logits, class index) - 0.01*mean(beta*(1-beta))   (hriemo_fusion_loss_ce)
  mosei_step_loss         scripts/fusion/train_mosei_fusion_seq_level_decoder.py:340-347,383-387,569:
                          BCEWithLogits(logits, y; pos_weight) + beta_entropy*H(beta), divided by grad_accum
CPU tensors (the gloo tests drive the CPU oracle through dp.py) take the same formulas in plain torch."""
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
