"""GPU suite of the epoch statistics inside the trainer step: DataParallelStep.attach_stats (the update recorded in the captured
step; warm-up passes never count; losses and gradients untouched), accumulation with loss_scale, the mask-fed capture() / step()
path, and train.evaluate_packed.  Model and batches: those of test_gpu_step_packed.py (d128, B = 5, T_a = 70, T_t = 40, dropout 0).

A captured step and an eager forward_packed pass on the same weights agree to the bound test_gpu_step_packed.py applies between
them (loss within 1e-5 * max(1, |ref|)), not bit for bit; so statistics fed from the two sides are compared as: integer counts
equal (the logits are not within 1e-5 of a threshold's logit), avg_loss / mean_beta within 1e-5 * max(1, |ref|).  Where both sides
hold the same bits (the loss tensors step_packed returns against the sums the update kernel formed from them) the bound is 1e-12."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_step_packed import H, NB, NE, TA, TT, Spy, _batches, _dp, _model, _tail  # noqa: F401  (H is the fixture)

pytestmark = pytest.mark.gpu

INTS = ("tp", "fp", "fn", "sweep_counts", "auc_2u", "n_pos", "n_neg")


def _head(rag, n):
    ra, rt, la, lt, y = rag
    lt = [int(v) for v in lt]
    return ra[:sum(la[:n])], rt[:sum(lt[:n])], la[:n], lt[:n], y[:n]


def _eager_stats(m0, rags, loss_fn, n_out=NE):
    """an EpochStats fed with forward_packed on every batch: weights of m0, no graph, nothing captured"""
    from hri_emo_amd.train import EpochStats
    m, st = copy.deepcopy(m0), EpochStats(n_out, 64)
    with torch.no_grad():
        for ra, rt, la, lt, y in rags:
            logits, beta, _ = m.forward_packed(ra, rt, la, lt, pad_to=(TA, TT))
            st.update(logits, beta, y, loss_fn(logits, beta, y))
    return st.result()


def _assert_same_statistics(got, ref):
    for k in INTS:
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in ("n_samples", "n_batches", "n_skipped", "n_correct", "n_logged"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert np.array_equal(got["calibrated_thresholds"], ref["calibrated_thresholds"])
    for k in ("micro_f1", "macro_f1", "macro_auc", "macro_f1_calibrated", "accuracy"):
        assert got[k] == ref[k], k                             # float64 from equal integers
    for k in ("avg_loss", "mean_beta"):
        print(f"{k}: {got[k]:.9f} vs {ref[k]:.9f}")
        assert abs(got[k] - ref[k]) <= 1e-5 * max(1.0, abs(ref[k])), (k, got[k], ref[k])


@pytest.mark.parametrize("partial", [False, True], ids=["full batches", "partial_batches"])
def test_captured_step_with_statistics_attached(H, monkeypatch, partial):
    """batch 0 (captured), 1 and 2 (new buckets, captured mid-epoch: two warm-ups + the capture pass each), 0 again, and with
    partial_batches a short last batch of 3: n_batches / n_samples count the calls and their utterances, every loss and flat gradient
    is torch.equal to the run without statistics, the statistics equal those of eager forward_packed passes"""
    from hri_emo_amd.train import EpochStats, fusion_step_loss
    _tail(True)
    m0 = _model(H)
    rags = [rag for _, rag in _batches()]
    order = [rags[0], rags[1], rags[2], rags[0]] + ([_head(rags[1], 3)] if partial else [])
    off, on = _dp(copy.deepcopy(m0)), _dp(copy.deepcopy(m0))
    stats = EpochStats(NE, 64)
    on.attach_stats(stats)
    spy = Spy(monkeypatch)
    off.capture_packed(*rags[0], pad_to=(TA, TT), partial_batches=partial)
    base = spy.take()
    on.capture_packed(*rags[0], pad_to=(TA, TT), partial_batches=partial)
    names = spy.take()
    assert names.count("hriemo_stats_update") == 1, "the capture pass records it, the two warm-up passes do not run it"
    assert [n for n in names if n != "hriemo_stats_update"] == base, "every other launch of the capture is unchanged"
    with pytest.raises(RuntimeError, match="before capture"):
        on.attach_stats(None)
    torch.cuda.synchronize()
    assert stats.counters.tolist()[:3] == [0, 0, 0], "capture itself counts nothing"
    for i, rag in enumerate(order):
        a = off.step_packed(*rag).clone()
        ga = off.buckets.flat.clone()
        b = on.step_packed(*rag)
        torch.cuda.synchronize()
        assert torch.equal(a, b), (i, float(a), float(b))
        assert torch.equal(ga, on.buckets.flat), (i, int((ga != on.buckets.flat).sum()))
    # a bucket met mid-epoch: its capture pass records the update once more, nothing else launches it (replays launch nothing)
    assert len(on._pb.graphs) == (4 if partial else 3) and spy.take().count("hriemo_stats_update") == len(on._pb.graphs) - 1
    got = stats.result()
    assert got["n_batches"] == len(order) and got["n_samples"] == sum(len(r[2]) for r in order)
    _assert_same_statistics(got, _eager_stats(m0, order, fusion_step_loss))
    # the same statistics from eager steps (use_graph(False)): attach_stats is honoured there too, once per step
    stats.reset()
    on.use_graph(False)
    for rag in order:
        on.step_packed(*rag)
    _assert_same_statistics(stats.result(), got)
    off.release_graph()
    on.release_graph()


def _loss_half(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import mosei_step_loss
    return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=2, n_valid=n_valid)


def test_accumulation_logs_the_undivided_loss(H, monkeypatch):
    """grad_accum = 2, optimizer in the graph, loss_scale = 2: the update is recorded behind backward and in front of the optimizer's
    launches; micro-step 1 meets a new bucket (captured inside the open group: its warm-ups do not count); avg_loss is the
    sample-weighted mean of twice the halved losses step_packed returned (same bits in, float64 arithmetic: 1e-12)"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import EpochStats
    _tail(True)
    rags = [rag for _, rag in _batches()]
    dp = DataParallelStep(_model(H), _loss_half, overlap=False)
    dp.set_global_batch(NB)
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    stats = EpochStats(NE, 64, skip_nonfinite=True)
    dp.attach_stats(stats, loss_scale=2.0)
    spy = Spy(monkeypatch)
    dp.capture_packed(*rags[0], pad_to=(TA, TT), optimizer=opt, grad_accum=2)
    names = spy.take()
    assert names.count("hriemo_stats_update") == 1
    at = names.index("hriemo_stats_update")
    assert names[at + 1:] == ["hriemo_sumsq_f32", "hriemo_optim_finalize_ctl", "hriemo_adamw_flat_dev"], names[at:]
    assert max(i for i, n in enumerate(names) if n.startswith("hriemo_fusion_loss")) < at
    losses = []
    for rag in (rags[0], rags[1], rags[2], rags[0]):
        losses.append(dp.step_packed(*rag).clone())
    torch.cuda.synchronize()
    assert float(opt.device_step) == 2.0
    r = stats.result()
    assert (r["n_batches"], r["n_samples"], r["n_skipped"], r["n_logged"]) == (4, 4 * NB, 0, 4 * NB)
    want = abs(sum(float(l) * 2.0 * NB for l in losses) / (4 * NB))
    print(f"avg_loss {r['avg_loss']:.9f}, from the returned losses {want:.9f}")
    assert abs(r["avg_loss"] - want) <= 1e-12 * want
    assert 0.0 < r["mean_beta"] < 1.0
    dp.release_graph()


def test_mask_fed_captured_step(H):
    """capture() / step() on padded batches (varlen off: one plain graph): two replays count twice, the loss equals the run without
    statistics, the statistics equal those of the eager padded forward"""
    from hri_emo_amd.train import EpochStats, fusion_step_loss
    H.set_varlen(False)
    m0 = _model(H)
    pads = [pad for pad, _ in _batches()[:2]]
    off, on = _dp(copy.deepcopy(m0)), _dp(copy.deepcopy(m0))
    stats, ref = EpochStats(NE, 16), EpochStats(NE, 16)
    on.attach_stats(stats)
    off.capture(*pads[0])
    on.capture(*pads[0])
    m = copy.deepcopy(m0)
    for pad in pads:
        a = off.step(*pad).clone()
        b = on.step(*pad)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(off.buckets.flat, on.buckets.flat)
        with torch.no_grad():
            logits, beta, _ = m(*pad[:4])
            ref.update(logits, beta, pad[4], fusion_step_loss(logits, beta, pad[4]))
    got = stats.result()
    assert got["n_batches"] == 2 and got["n_samples"] == 2 * NB
    _assert_same_statistics(got, ref.result())
    off.release_graph()
    on.release_graph()


def _definitions(logits, y):
    """the epoch's integers and ratios from the definitions, in numpy float64, on the model's own logits (torch.sigmoid in fp32)"""
    p, t = torch.sigmoid(logits).cpu().numpy(), y.cpu().numpy() > 0
    grid = np.concatenate([[0.5], np.linspace(0.05, 0.95, 19)])
    pred = p.astype(np.float64)[:, :, None] >= grid
    tp, fp, fn = (pred & t[:, :, None]).sum(0), (pred & ~t[:, :, None]).sum(0), (~pred & t[:, :, None]).sum(0)
    den = 2 * tp + fp + fn
    f1 = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)                    # [C, 20]
    aucs = []
    for c in range(p.shape[1]):
        pos, neg = p[t[:, c], c], p[~t[:, c], c]
        if pos.size and neg.size:
            aucs.append(((2 * (pos[:, None] > neg[None, :]) + (pos[:, None] == neg[None, :])).sum()) / (2.0 * pos.size * neg.size))
    den0 = 2 * tp[:, 0].sum() + fp[:, 0].sum() + fn[:, 0].sum()
    return {"tp": tp[:, 0], "fp": fp[:, 0], "fn": fn[:, 0], "micro_f1": 2.0 * tp[:, 0].sum() / den0 if den0 else 0.0, "macro_f1": f1[:, 0].mean(),
            "macro_auc": float(np.mean(aucs)) if aucs else 0.0, "macro_f1_calibrated": f1[:, 1:].max(1).mean(),
            "n_correct": int(((p > 0.5) == t).all(1).sum())}


def test_evaluate_packed(H, monkeypatch):
    """three ragged batches in data.collate_seq_packed's form (host tensors): the statistics against the float64 definitions on the
    model's own eval-mode logits; besides the model's launches only one loss and one update launch per batch; the module's mode is
    restored"""
    from hri_emo_amd.train import EpochStats, evaluate_packed, fusion_step_loss
    _tail(True)
    m = _model(H)
    batches = [(ra.cpu(), torch.tensor(la), rt.cpu(), torch.as_tensor(lt), y.cpu()) for _, (ra, rt, la, lt, y) in _batches()]
    spy = Spy(monkeypatch)
    m.eval()
    logits, losses = [], []
    with torch.no_grad():
        m.forward_packed(batches[0][0].cuda(), batches[0][2].cuda(), batches[0][1], batches[0][3], pad_to=(TA, TT))
        spy.take()                                           # the first pass also casts the bf16 weight shadows: not part of the baseline
        for ra, la, rt, lt, y in batches:
            out = m.forward_packed(ra.cuda(), rt.cuda(), la, lt, pad_to=(TA, TT))
            logits.append(out[0])
            losses.append(float(fusion_step_loss(out[0], out[1], y.cuda())))
    plain = [n for n in spy.take() if not n.startswith("hriemo_fusion_loss")]
    m.train()
    stats = EpochStats(NE, 3 * NB)
    assert evaluate_packed(m, batches, fusion_step_loss, stats, pad_to=(TA, TT)) is stats and m.training
    names = spy.take()
    rest = [n for n in names if n != "hriemo_stats_update" and not n.startswith("hriemo_fusion_loss")]
    assert rest == plain, "no launch besides the model's, the loss's and the update's"
    assert names.count("hriemo_stats_update") == 3 and sum(n.startswith("hriemo_fusion_loss") for n in names) == 3
    m.eval()
    evaluate_packed(m, batches[:1], fusion_step_loss, EpochStats(NE, NB), pad_to=(TA, TT))
    assert not m.training
    r = stats.result()
    want = _definitions(torch.cat(logits), torch.cat([b[4] for b in batches]))
    for k in ("tp", "fp", "fn"):
        assert np.array_equal(r[k], want[k]), (k, r[k], want[k])
    assert r["n_correct"] == want["n_correct"] and r["n_samples"] == 3 * NB and r["n_batches"] == 3
    for k in ("micro_f1", "macro_f1", "macro_auc", "macro_f1_calibrated"):
        assert abs(r[k] - want[k]) <= 1e-12, (k, r[k], want[k])
    mean = sum(l * NB for l in losses) / (3 * NB)
    assert abs(r["avg_loss"] - abs(mean)) <= 1e-12 * abs(mean)
