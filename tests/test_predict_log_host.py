"""CPU suite of train.PredictionLog: the CPU path against the numpy definitions the kernel suite (test_gpu_predict_log_kernel.py)
holds hriemo_predict_log to -- float64 sigmoid / softmax rounded to fp32, first argmax, float64 mean of a sample's beta values --
the layout arrays() hands back, the overflow error, and the binding's signature."""
import numpy as np
import pytest
import torch

NAN = float("nan")


def _batch(B, C, bps, seed):
    g = torch.Generator().manual_seed(seed)
    return 2.0 * torch.randn(B, C, generator=g), (torch.rand(B, bps, generator=g) if bps else None)


def _softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def test_binding_and_export():
    import hri_emo_amd
    from hri_emo_amd import _lib, dp, train
    assert _lib._SIGS["hriemo_predict_log"] == ("ppipiiipppipp", "i") and hasattr(_lib.lib(), "hriemo_predict_log")
    assert hri_emo_amd.EvalStep is dp.EvalStep and "EvalStep" in hri_emo_amd.__all__
    assert train.PredictionLog(4, 8, device="cpu").arrays()["y_prob"].shape == (0, 4)


@pytest.mark.parametrize("kind", ["multi_label", "single_label"])
def test_cpu_path_against_the_numpy_definitions(kind):
    """three batches, the second short with NaN behind n_valid, the third with beta of 3 values per sample given as [B * 3]"""
    from hri_emo_amd.train import PredictionLog
    C = 6
    log = PredictionLog(C, 32, kind=kind, device="cpu")
    xs, bs = [], []
    for i, (B, nv) in enumerate(((5, None), (5, 3), (7, 9))):
        x, beta = _batch(B, C, 3, i)
        if kind == "single_label" and i == 0:
            x[0, 1] = x[0, 4] = 9.0                                        # a tie: index 1
            x[1] = torch.tensor([1e4, -1e4, 80.0, -80.0, 0.0, 0.0])
        n = B if nv is None else min(max(nv, 1), B)
        x[n:], beta[n:] = NAN, NAN
        log.update(x, beta.reshape(-1) if i == 2 else beta, n_valid=nv)
        xs.append(x[:n].numpy())
        bs.append(beta[:n].numpy())
    out = log.arrays()
    x, beta = np.concatenate(xs), np.concatenate(bs)
    assert out["n_samples"] == 15 and out["n_nonfinite"] == 0 and log.counters.tolist() == [15, 15, 0, 0]
    assert out["y_prob"].dtype == np.float32 and out["y_prob"].shape == (15, C) and out["y_prob"].flags["C_CONTIGUOUS"]
    if kind == "multi_label":
        ref = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
        assert "pred" not in out
    else:
        ref = _softmax64(x).astype(np.float32)
        assert out["pred"].dtype == np.int32 and np.array_equal(out["pred"], x.argmax(axis=1)) and out["pred"][0] == 1 and out["pred"][1] == 0
        assert np.isfinite(out["y_prob"]).all() and out["y_prob"][1, 0] == 1.0
    assert np.array_equal(out["y_prob"], ref)
    assert out["beta_mean"].dtype == np.float32 and np.array_equal(out["beta_mean"], beta.astype(np.float64).mean(axis=1).astype(np.float32))
    log.reset()
    again = log.arrays()
    assert again["y_prob"].shape == (0, C) and again["n_samples"] == 0


def test_without_beta_the_mean_is_none_and_non_finite_logits_are_counted():
    from hri_emo_amd.train import PredictionLog
    log = PredictionLog(4, 8, device="cpu")
    x, _ = _batch(5, 4, 0, 3)
    x[1, 2], x[2, 0], x[4, 1] = NAN, float("inf"), NAN
    log.update(x, n_valid=4)                                               # row 4 lies behind n_valid
    out = log.arrays()
    assert out["beta_mean"] is None and out["n_nonfinite"] == 2 and out["y_prob"].shape == (4, 4)


def test_overflow_and_refusals():
    from hri_emo_amd.train import PredictionLog
    log = PredictionLog(4, 8, device="cpu")
    x, beta = _batch(5, 4, 1, 4)
    log.update(x, beta, n_valid=3)
    log.update(x, beta)                                                    # 3 + 5 == 8: fits exactly
    assert log.counters.tolist() == [8, 8, 0, 0] and log.arrays()["y_prob"].shape == (8, 4)
    before = log.probs.clone()
    log.update(x, beta, n_valid=1)
    assert log.counters.tolist() == [8, 9, 1, 0] and torch.equal(log.probs, before)
    with pytest.raises(RuntimeError, match="overflowed"):
        log.arrays()
    with pytest.raises(ValueError):
        PredictionLog(4, 8, kind="ranking", device="cpu")
    with pytest.raises(ValueError):
        PredictionLog(0, 8, device="cpu")
    with pytest.raises(ValueError):
        log.update(torch.zeros(5, 3))
    with pytest.raises(ValueError):
        log.update(x, torch.zeros(7))
