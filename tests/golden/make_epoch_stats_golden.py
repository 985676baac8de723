"""Writes tests/golden/epoch_stats.npz: inputs and expected epoch statistics for hri_emo_amd.train.EpochStats and the
hriemo_stats_* kernels.  Run once on a CPU, with the reference checkout's root on PYTHONPATH (it needs sklearn / pandas / tqdm):

    PYTHONPATH=<reference root> python tests/golden/make_epoch_stats_golden.py

The reference's MOSEI trainer module is imported at run time; its own multilabel_metrics_from_logits and calibrate_thresholds
produce the recorded floating-point results.  The integers (tp / fp / fn per class and threshold, 2U, n_pos, n_neg) are derived
here from torch.sigmoid on the CPU by brute force.  Tests read the fixture only.

torch's fp32 CPU sigmoid is not a function of the value alone: the last numel % 16 elements of a tensor take a scalar path whose
result can differ by an ulp from the vector path's, so two equal logits need not tie.  The integers are therefore derived from
probs(): torch.sigmoid in float64, rounded to fp32 (the correctly rounded fp32 sigmoid, the same for equal logits; asserted).  The
reference's functions apply their own fp32 sigmoid to the first n samples; their results are recorded only for the prefixes n at
which those probabilities give the same integers as probs() (`<case>_ref_ns`; asserted to include 64, 256, 301 and 1000).

Two cases, C = 6 outputs, N = 1000 samples, statistics recorded for every prefix n in NS:
  cont   logits ~ 2 randn (+ 1.5 where the target is positive).  Input condition (asserted, not a tolerance): every float64
         probability is at least MARGIN = 1e-6 away from all 20 thresholds (0.5 and the 19-point sweep), or its logit is exactly 0;
         offending logits are redrawn.  fp32 sigmoid implementations differ by a few ulp (~2e-7), so every implementation takes
         the same threshold decisions.  Class 3 has no positive.
  grid   logits are multiples of 1/8 in [-6, 6], positives shifted up by 1; 0 included: p = 0.5 exactly, which tells `>= 0.5` of
         the F1s from `> 0.5` of the accuracy.  Distinct logits differ in probability by >= 3e-4, equal ones tie exactly, so 2U is
         the same integer for every monotonic fp32 sigmoid.  Class 3 has no positive, class 4 no negative, every logit of class 5
         is 0.25 (all tie).  The MARGIN condition is asserted here too.
Both cases carry beta [N], per-batch losses for batches of BATCH samples, and the avg_loss / mean_beta the reference's
train_one_epoch arithmetic (:404-420) makes of them."""
import importlib
import os

import numpy as np
import torch

N, C, BATCH, MARGIN = 1000, 6, 64, 1e-6
NS = (1, 37, 64, 255, 256, 257, 301, 1000)
SWEEP = np.linspace(0.05, 0.95, 19)
GRID = np.concatenate([[0.5], SWEEP])


def margin_ok(logits):
    p = torch.sigmoid(logits.double()).numpy()
    return (np.abs(p[..., None] - GRID).min(-1) >= MARGIN) | (logits.numpy() == 0.0)


def targets_for(g, special):
    """MOSEI-style annotations in [0, 3] (a third of them positive), negatives as noise; `special` = {class: 'nopos' | 'noneg'}"""
    y = torch.where(torch.rand(N, C, generator=g) < 0.35, torch.randint(1, 10, (N, C), generator=g).float() / 3.0, torch.zeros(N, C))
    y = torch.where(torch.rand(N, C, generator=g) < 0.05, -torch.ones(N, C) / 3.0, y)
    for c, what in special.items():
        y[:, c] = 0.0 if what == "nopos" else 1.0
    return y


def probs(logits):
    return torch.sigmoid(logits.double()).float()


def integers(logits, y, n, p=None):
    p = (probs(logits[:n]) if p is None else p).numpy()        # fp32
    t = y[:n].numpy() > 0
    pred = p.astype(np.float64)[:, :, None] >= GRID[None, None, :]          # the reference's comparison: fp32 p against float64 t
    tt = t[:, :, None]
    counts = np.stack([(pred & tt).sum(0), (pred & ~tt).sum(0), (~pred & tt).sum(0)], axis=2).astype(np.int64)      # [C, 20, 3]
    two_u = np.zeros(C, dtype=np.int64)
    for c in range(C):
        pos, neg = p[t[:, c], c], p[~t[:, c], c]
        two_u[c] = int((2 * (pos[:, None] > neg[None, :]) + (pos[:, None] == neg[None, :])).sum())
    correct = int(((p > 0.5) == t).all(1).sum())
    return counts, two_u, t.sum(0).astype(np.int64), (~t).sum(0).astype(np.int64), correct


def main():
    ref = importlib.import_module("scripts.fusion.train_mosei_fusion_seq_level_decoder")
    from sklearn.metrics import f1_score
    g = torch.Generator().manual_seed(20261019)
    out = {"ns": np.asarray(NS), "batch": np.asarray(BATCH), "sweep": SWEEP}
    # the logits carry some signal (positives shifted up), so that F1 varies over the sweep and the calibration has something to find
    y_cont, y_grid = targets_for(g, {3: "nopos"}), targets_for(g, {3: "nopos", 4: "noneg"})
    shift = 1.5 * (y_cont > 0).float()
    cont = 2.0 * torch.randn(N, C, generator=g) + shift
    while True:
        bad = ~torch.from_numpy(margin_ok(cont))
        if not bad.any():
            break
        cont[bad] = 2.0 * torch.randn(int(bad.sum()), generator=g) + shift[bad]
    grid = (torch.randint(-40, 33, (N, C), generator=g).float() / 8.0 + (y_grid > 0).float()).clamp(-6.0, 6.0)
    grid[:, 5] = 0.25
    grid[::97, 0] = 0.0
    assert margin_ok(cont).all() and margin_ok(grid).all() and (grid == 0).any()
    assert bool((grid * 8 == (grid * 8).round()).all()) and float(grid.abs().max()) <= 6.0
    for x in (cont, grid):                                    # equal logits tie exactly, distinct ones do not
        assert len(torch.unique(torch.stack([x.reshape(-1), probs(x).reshape(-1)]), dim=1)[0]) == len(x.unique()) == len(probs(x).unique())
    pg = torch.sigmoid(grid.double()).unique()
    assert float((pg[1:] - pg[:-1]).min()) >= 3e-4
    cases = {"cont": (cont, y_cont), "grid": (grid, y_grid)}
    for name, (logits, y) in cases.items():
        beta = torch.rand(N, generator=g)
        nb = (N + BATCH - 1) // BATCH
        losses = (0.3 + torch.rand(nb, generator=g)).float()
        out.update({f"{name}_logits": logits.numpy(), f"{name}_targets": y.numpy(), f"{name}_beta": beta.numpy(),
                    f"{name}_losses": losses.numpy()})
        total, seen, betas = 0.0, 0, []                       # the reference's logging arithmetic, train_one_epoch :404-420
        for b in range(nb):
            bs = min(BATCH, N - b * BATCH)
            total += losses[b].item() * bs
            seen += bs
            betas.extend(beta[b * BATCH:b * BATCH + bs].float().view(-1).tolist())
        out[f"{name}_avg_loss"] = np.asarray(abs(total / max(1, seen)))
        out[f"{name}_mean_beta"] = np.asarray(float(np.mean(betas)))
        ref_ns = []
        for n in NS:
            counts, two_u, n_pos, n_neg, correct = integers(logits, y, n)
            k = f"{name}_{n}_"
            out.update({k + "counts": counts, k + "two_u": two_u, k + "n_pos": n_pos, k + "n_neg": n_neg, k + "correct": np.asarray(correct)})
            p32 = torch.sigmoid(logits[:n])                     # what the reference's functions see
            seen = integers(logits, y, n, p32)
            if not all(np.array_equal(a, b) for a, b in zip(seen, (counts, two_u, n_pos, n_neg, correct))):
                continue                                        # a tie broken by the scalar tail of the fp32 sigmoid
            ref_ns.append(n)
            micro, macro, auc = ref.multilabel_metrics_from_logits(logits[:n], y[:n])
            ths = ref.calibrate_thresholds(p32.numpy(), y[:n].numpy(), steps=19)
            cal = f1_score((y[:n].numpy() > 0).astype(int), (p32.numpy() >= ths[None, :]).astype(int), average="macro", zero_division=0)
            out.update({k + "micro_f1": np.asarray(float(micro)), k + "macro_f1": np.asarray(float(macro)), k + "macro_auc": np.asarray(float(auc)),
                        k + "thresholds": np.asarray(ths), k + "macro_f1_cal": np.asarray(float(cal))})
        assert {64, 256, 301, 1000} <= set(ref_ns), ref_ns
        out[f"{name}_ref_ns"] = np.asarray(ref_ns)
        print(name, "reference results recorded for n =", ref_ns)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "epoch_stats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
