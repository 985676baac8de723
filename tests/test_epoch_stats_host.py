"""CPU suite of hri_emo_amd.train.EpochStats: the plain torch / numpy path against tests/golden/epoch_stats.npz (recorded from the
reference's own multilabel_metrics_from_logits / calibrate_thresholds by tests/golden/make_epoch_stats_golden.py; integers by brute
force from torch.sigmoid), ghosts, skipped batches, overflow, single-label argmax ties, the threshold round-up helper."""
import numpy as np
import pytest
import torch

from conftest import load_golden

C = 6
_G = {}


def G():
    if not _G:
        _G.update(load_golden("epoch_stats"))
    return _G


def feed(stats, g, case, n, batch=None):
    """the first n samples of a fixture case in batches of the fixture's batch size, the short last batch as it comes"""
    batch = int(g["batch"]) if batch is None else batch
    logits, y, beta, losses = (g[f"{case}_{k}"] for k in ("logits", "targets", "beta", "losses"))
    for i, lo in enumerate(range(0, n, batch)):
        hi = min(n, lo + batch)
        stats.update(logits[lo:hi], beta[lo:hi], y[lo:hi], losses[i])
    return stats


def assert_matches_fixture(r, g, case, n, whole_epoch):
    k = f"{case}_{n}_"
    counts = g[k + "counts"].numpy()
    assert np.array_equal(np.stack([r["tp"], r["fp"], r["fn"]], 1), counts[:, 0]) and np.array_equal(r["sweep_counts"], counts[:, 1:])
    assert np.array_equal(r["auc_2u"], g[k + "two_u"].numpy()) and np.array_equal(r["n_pos"], g[k + "n_pos"].numpy())
    assert np.array_equal(r["n_neg"], g[k + "n_neg"].numpy())
    assert r["n_correct"] == int(g[k + "correct"]) and r["n_samples"] == r["n_logged"] == n
    if n in g[f"{case}_ref_ns"].tolist():                      # the prefixes for which the reference's own results are recorded
        for name, key in (("micro_f1", "micro_f1"), ("macro_f1", "macro_f1"), ("macro_auc", "macro_auc"), ("macro_f1_calibrated", "macro_f1_cal")):
            assert abs(r[name] - float(g[k + key])) <= 1e-12, (case, n, name, r[name], float(g[k + key]))
        assert r["calibrated_thresholds"].dtype == np.float32 and np.array_equal(r["calibrated_thresholds"], g[k + "thresholds"].numpy())
    assert abs(r["accuracy"] - int(g[k + "correct"]) / n) <= 1e-12
    if whole_epoch:
        assert abs(r["avg_loss"] - float(g[f"{case}_avg_loss"])) <= 1e-12 and abs(r["mean_beta"] - float(g[f"{case}_mean_beta"])) <= 1e-12


@pytest.mark.parametrize("case", ["cont", "grid"])
def test_cpu_path_reproduces_the_reference(case):
    from hri_emo_amd.train import EpochStats
    g = G()
    for n in [int(x) for x in g["ns"]]:
        stats = feed(EpochStats(C, 1024, device="cpu"), g, case, n)
        r = stats.result()
        assert_matches_fixture(r, g, case, n, whole_epoch=(n == 1000))
        assert r["n_batches"] == -(-n // int(g["batch"])) and r["n_skipped"] == 0
    assert {64, 256, 301, 1000} <= set(g[f"{case}_ref_ns"].tolist())
    stats.reset()
    assert stats.result()["n_samples"] == 0 and stats.result()["macro_auc"] == 0.0 and stats.result()["avg_loss"] == 0.0


def test_grid_case_tells_the_two_comparisons_apart():
    """a logit of exactly 0 is predicted positive by the F1s (p >= 0.5) and negative by the accuracy (p > 0.5)"""
    from hri_emo_amd.train import EpochStats
    st = EpochStats(1, 4, device="cpu")
    st.update(torch.zeros(2, 1), None, torch.tensor([[1.0], [0.0]]), torch.tensor(1.0))
    r = st.result()
    assert (int(r["tp"][0]), int(r["fp"][0]), int(r["fn"][0])) == (1, 1, 0) and r["n_correct"] == 1 and r["mean_beta"] == 0.0


def test_ghosts_skips_overflow_and_loss_scale():
    from hri_emo_amd.train import EpochStats
    g = G()
    logits, y, beta = g["cont_logits"][:10].clone(), g["cont_targets"][:10].clone(), g["cont_beta"][:10].clone()
    ref = EpochStats(C, 32, device="cpu")
    ref.update(logits[:7], beta[:7], y[:7], torch.tensor(0.5), loss_scale=2.0)
    want = ref.result()
    logits[7:], y[7:], beta[7:] = float("nan"), float("nan"), float("nan")          # ghosts: whatever their rows hold
    st = EpochStats(C, 32, skip_nonfinite=True, device="cpu")
    st.update(logits, beta, y, torch.tensor(0.5), n_valid=torch.tensor([7], dtype=torch.int32), loss_scale=2.0)
    got = st.result()
    assert got["avg_loss"] == want["avg_loss"] == 1.0 and got["n_samples"] == 7
    for k in ("tp", "fp", "fn", "auc_2u", "n_pos", "n_neg", "sweep_counts", "calibrated_thresholds"):
        assert np.array_equal(got[k], want[k]), k
    assert got["mean_beta"] == want["mean_beta"] and got["n_correct"] == want["n_correct"]
    # a skipped non-finite batch changes only n_skipped
    before = (st.counters.clone(), st.sums.clone(), st.probs.clone(), st.truth.clone())
    st.update(logits[:7], beta[:7], y[:7], torch.tensor(float("nan")))
    st.update(logits[:7], beta[:7], y[:7], torch.tensor(float("inf")))
    assert st.counters[3] == 2
    st.counters[3] = 0
    for a, b in zip(before, (st.counters, st.sums, st.probs, st.truth)):
        assert torch.equal(a, b)
    # without the flag a NaN loss is summed like the IEMOCAP trainer sums it
    plain = EpochStats(C, 32, device="cpu")
    plain.update(logits[:7], beta[:7], y[:7], torch.tensor(float("nan")))
    assert plain.result()["avg_loss"] != plain.result()["avg_loss"] and plain.result()["n_skipped"] == 0
    # overflow: 25 + 7 fit exactly, one more sample does not; sums and counters still move, result() refuses
    fit = feed(EpochStats(C, 32, device="cpu"), g, "cont", 25, batch=25)
    fit.update(logits[:7], beta[:7], y[:7], torch.tensor(0.5))
    assert fit.result()["n_logged"] == 32
    over = feed(EpochStats(C, 32, device="cpu"), g, "cont", 26, batch=26)
    log = (over.probs.clone(), over.truth.clone())
    over.update(logits[:7], beta[:7], y[:7], torch.tensor(0.5))
    assert over.counters.tolist()[:3] == [26, 33, 2] and over.counters[6] == 1
    assert torch.equal(log[0], over.probs) and torch.equal(log[1], over.truth)
    with pytest.raises(RuntimeError, match="overflow"):
        over.result()
    bad = EpochStats(C, 32, device="cpu")
    bad.update(logits, beta[:7].repeat(2)[:10], y.nan_to_num(0.0), torch.tensor(0.5))
    with pytest.raises(ValueError, match="non-finite"):
        bad.result()


def test_single_label_argmax_ties_and_keys():
    from hri_emo_amd.train import EpochStats
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0], [7.0, 1.0, 0.0, 7.0], [0.0, 1.0, 2.0, 3.0]])
    labels = torch.tensor([1, 0, 3, 0, 3])                   # first maximal index: 1, 0, 2, 0, 3 -> 4 correct
    st = EpochStats(4, 1, kind="single_label", device="cpu")
    st.update(x, torch.full((5, 3), 0.25), labels, torch.tensor(2.0))
    st.update(x, torch.full((5, 3), 0.75), labels, torch.tensor(4.0), n_valid=2)
    r = st.result()
    assert r["n_correct"] == 6 and r["n_samples"] == 7 and r["n_batches"] == 2 and abs(r["accuracy"] - 6 / 7) <= 1e-12
    assert abs(r["avg_loss"] - (2.0 * 5 + 4.0 * 2) / 7) <= 1e-12 and abs(r["mean_beta"] - (15 * 0.25 + 6 * 0.75) / 21) <= 1e-12
    assert "micro_f1" not in r and "calibrated_thresholds" not in r
    with pytest.raises(ValueError, match="kind"):
        EpochStats(4, 8, kind="multiclass", device="cpu")
    with pytest.raises(ValueError, match="targets of shape"):
        st.update(x, None, torch.zeros(5, 4), torch.tensor(1.0))


def test_thresholds_round_up_to_fp32():
    """r = thresholds_up(t): float64(r) >= t and the next fp32 below r is < t, so `p >= r` in fp32 is `p >= t` in float64"""
    from hri_emo_amd.train import SWEEP, thresholds_up
    t = np.asarray(SWEEP, dtype=np.float64)
    assert np.array_equal(t, np.linspace(0.05, 0.95, 19))
    r = thresholds_up(t)
    assert r.dtype == np.float32 and r.shape == (19,)
    assert (r.astype(np.float64) >= t).all()
    assert (np.nextafter(r, np.float32(-np.inf)).astype(np.float64) < t).all()
    assert thresholds_up(0.5)[0] == np.float32(0.5) and (r != t.astype(np.float32)).any(), "some grid point rounds down to nearest"
    for p in (np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))):
        assert np.array_equal(p >= r, p.astype(np.float64) >= t)


def test_custom_sweep_and_limits():
    from hri_emo_amd.train import EpochStats
    g = G()
    st = feed(EpochStats(C, 1024, device="cpu"), g, "cont", 301)
    r = st.result(thresholds=[0.5])
    assert np.array_equal(r["calibrated_thresholds"], np.full(C, 0.5, dtype=np.float32))
    assert abs(r["macro_f1_calibrated"] - r["macro_f1"]) <= 1e-15 and np.array_equal(r["sweep_counts"][:, 0], np.stack([r["tp"], r["fp"], r["fn"]], 1))
    with pytest.raises(ValueError, match="thresholds"):
        st.result(thresholds=np.linspace(0.01, 0.99, 64))


def test_attach_stats_counts_every_eager_step_once():
    """DataParallelStep on the CPU oracle (no graph, no GPU): step() and every micro-batch of step_accumulated() update the attached
    statistics exactly once, with the loss as the loss function returned it (step_accumulated's own 1/k is not logged)"""
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import EpochStats, fusion_step_loss
    from oracle import hri_emo_oracle as O
    torch.manual_seed(0)
    model = O.FusionWithEmotionDecoder(d_model=64, num_emotions=3, n_heads=4, dropout=0.0).train()
    B, Ta, Tt = 4, 12, 6
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(3):
        m_a = torch.arange(Ta)[None] >= torch.randint(Ta // 2, Ta + 1, (B, 1), generator=g)
        m_t = torch.arange(Tt)[None] >= torch.randint(Tt // 2, Tt + 1, (B, 1), generator=g)
        batches.append((torch.randn(B, Ta, 64, generator=g), torch.randn(B, Tt, 64, generator=g), m_a, m_t,
                        (torch.rand(B, 3, generator=g) < 0.4).float()))
    ref = EpochStats(3, 16, device="cpu")
    with torch.no_grad():
        for h_a, h_t, m_a, m_t, y in batches:
            logits, beta, _ = model(h_a, h_t, m_a, m_t)
            ref.update(logits, beta, y, fusion_step_loss(logits, beta, y))
    want = ref.result()
    dp = DataParallelStep(model, fusion_step_loss, overlap=False)
    plain = [float(dp.step(*b)) for b in batches[:1]]
    stats = EpochStats(3, 16, device="cpu")
    dp.attach_stats(stats)
    assert float(dp.step(*batches[0])) == plain[0], "the step itself is unchanged"
    dp.step_accumulated(batches[1:])
    got = stats.result()
    assert got["n_batches"] == 3 and got["n_samples"] == 3 * B
    for k in ("tp", "fp", "fn", "auc_2u", "n_pos", "n_neg", "sweep_counts"):
        assert np.array_equal(got[k], want[k]), k
    assert abs(got["avg_loss"] - want["avg_loss"]) <= 1e-12 and abs(got["mean_beta"] - want["mean_beta"]) <= 1e-12
    dp.attach_stats(None)
    dp.step(*batches[0])
    assert stats.result()["n_batches"] == 3
