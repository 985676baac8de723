"""Host suite of data.StoreAugment and of the replica the GPU suites compare against (tests/augment_reference.py): every refusal of
the constructor, the state_dict round trip, the refusal of an augment on a CPU store, and the statistics of the hash-driven
transforms -- noise moments and neighbour correlations, span widths and bounds, the drop rate."""
import numpy as np
import pytest
import torch

import augment_reference as R
import hashrng

TM = dict(spans=2, max_width=40, max_frac=0.5)


def _aug(*a, **kw):
    from hri_emo_amd.data import StoreAugment
    return StoreAugment(*a, **kw)


@pytest.mark.parametrize("kw", [
    dict(time_mask=dict(spans=0, max_width=4, max_frac=0.5)),
    dict(time_mask=dict(spans=5, max_width=4, max_frac=0.5)),
    dict(time_mask=dict(spans=1.5, max_width=4, max_frac=0.5)),
    dict(time_mask=dict(spans=1, max_width=0, max_frac=0.5)),
    dict(time_mask=dict(spans=1, max_width=4, max_frac=0.0)),
    dict(time_mask=dict(spans=1, max_width=4, max_frac=1.5)),
    dict(time_mask=dict(spans=1, max_width=4)),
    dict(time_mask=dict(spans=1, max_width=4, max_frac=0.5, width=3)),
    dict(time_mask=(TM, TM, TM)),
    dict(time_mask=(TM, "text")),
    dict(noise_std=(-0.1, 0.0)),
    dict(noise_std=(0.1, float("inf"))),
    dict(noise_std=(0.1, float("nan"))),
    dict(noise_std=(0.1,)),
    dict(modality_drop=(-0.1, 0.2)),
    dict(modality_drop=(0.5, 0.5)),
    dict(modality_drop=(0.2, 0.9)),
    dict(modality_drop=(0.1, 0.1, 0.1)),
], ids=lambda kw: repr(kw)[:60])
def test_constructor_refusals(kw):
    with pytest.raises(ValueError, match="StoreAugment"):
        _aug(1, **kw)


def test_an_augment_that_does_nothing_is_refused_by_name():
    for kw in ({}, dict(noise_std=(0.0, 0.0)), dict(modality_drop=(0.0, 0.0)), dict(time_mask=(None, None), noise_std=(0, 0))):
        with pytest.raises(ValueError, match="no transform is enabled"):
            _aug(1, **kw)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            _aug(seed, time_mask=TM)
    _aug((1 << 64) - 1, time_mask=TM)
    _aug(1, time_mask=(None, TM))                     # one modality is enough
    _aug(1, noise_std=(0.0, 0.01))
    _aug(1, modality_drop=(0.0, 0.25))


def test_launch_arguments_are_the_replicas():
    """the scalars data.StoreAugment hands to the kernel are those the replica derives from the same configuration"""
    a = _aug(77, time_mask=(TM, dict(spans=4, max_width=7, max_frac=1.0)), noise_std=(0.05, 1.0), modality_drop=(0.1, 0.25))
    assert a.draw == 0
    a.draw = 9
    for which, tm, sigma in ((0, (2, 40, 0.5), 0.05), (1, (4, 7, 1.0), 1.0)):
        cfg = R.launch_cfg(which, tm, sigma, (0.1, 0.25))
        seed, draw, modality, lo, hi, spans, width, frac16, scale = a.launch_args(which)
        assert (seed, draw) == (77, 9) and a.launch_args(which, 3)[1] == 3
        assert dict(modality=modality, thr_lo=lo, thr_hi=hi, spans=spans, max_width=width, frac16=frac16, noise_scale=scale) == cfg
    assert a.launch_args(0)[3:5] == (0, hashrng.thr16(0.1)) and a.launch_args(1)[3:5] == (hashrng.thr16(0.1), hashrng.thr16(0.1) + hashrng.thr16(0.25))
    assert a.launch_args(1)[7] == 65536 and a.launch_args(0)[7] == 32768
    assert a.launch_args(0)[8] == float(np.float32(0.05 / np.sqrt(21845.0)))
    assert a.launch_args(0, (1 << 32) + 5)[1] == 5
    assert a.draw == 9, "launch_args never advances the counter"
    with pytest.raises(ValueError, match="draw"):
        a.launch_args(0, -1)


def test_state_dict_round_trip_and_another_configuration():
    a = _aug(1234, time_mask=TM, noise_std=(0.05, 0.0), modality_drop=(0.1, 0.0))
    a.draw = 41
    state = a.state_dict()
    assert state["seed"] == 1234 and state["draw"] == 41
    import json
    state = json.loads(json.dumps(state))              # plain values: survives a checkpoint's serialisation
    b = _aug(5, time_mask=TM, noise_std=(0.05, 0.0), modality_drop=(0.1, 0.0))
    b.load_state_dict(state)
    assert (b.seed, b.draw) == (1234, 41) and b.state_dict() == a.state_dict()
    assert b.launch_args(0) == a.launch_args(0) and b.launch_args(1) == a.launch_args(1)
    for other in (_aug(5, time_mask=TM, noise_std=(0.06, 0.0), modality_drop=(0.1, 0.0)), _aug(5, time_mask=TM, modality_drop=(0.1, 0.0)),
                  _aug(5, time_mask=dict(spans=3, max_width=40, max_frac=0.5), noise_std=(0.05, 0.0), modality_drop=(0.1, 0.0))):
        with pytest.raises(ValueError, match="another configuration"):
            other.load_state_dict(state)
        assert (other.seed, other.draw) == (5, 0), "a refused load changes nothing"


def test_an_augment_on_a_cpu_store_is_refused_by_name():
    from hri_emo_amd.data import DeviceFeatureStore
    g = torch.Generator().manual_seed(0)
    samples = [(torch.randn(n, 6, generator=g), torch.zeros(n, dtype=torch.bool), torch.randn(n, 4, generator=g), torch.zeros(n, dtype=torch.bool),
                torch.zeros(3)) for n in (3, 5)]
    store = DeviceFeatureStore.from_samples(samples, "cpu")
    a = _aug(1, time_mask=TM)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        store.fetch([0, 1], augment=a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        store.gather_into(None, 5, 2, None, 0, None, 0, None, augment=a)
    with pytest.raises(TypeError, match="StoreAugment"):
        store.fetch([0, 1], augment=dict(seed=1))
    assert a.draw == 0
    ref = store.fetch([1, 0])
    for x, y in zip(store.fetch([1, 0], augment=None, draw=None), ref):
        assert torch.equal(x, y)


def test_evaluation_takes_no_augment():
    """EvalStep.capture_store / eval_store and train.evaluate_store have no augment parameter: passing one is a TypeError from the
    signature, before anything else is looked at"""
    import inspect
    from hri_emo_amd import dp, train
    a = _aug(1, time_mask=TM)
    ev = dp.EvalStep(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError, match="augment"):
        ev.capture_store(None, [0], augment=a)
    with pytest.raises(TypeError, match="augment"):
        ev.eval_store([0], augment=a)
    with pytest.raises(TypeError, match="augment"):
        train.evaluate_store(None, None, [], None, None, augment=a)
    assert "augment" in inspect.signature(dp.DataParallelStep.capture_store).parameters


def test_entry_in_header_and_binding():
    import os
    import re
    from hri_emo_amd import _lib
    assert _lib._SIGS["hriemo_gather_rows_aug"] == ("piippipllQIiIIiIIfp", "i")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "hriemo.h")).read()
    proto = re.search(r"int hriemo_gather_rows_aug\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(_lib._SIGS["hriemo_gather_rows_aug"][0])
    assert "hriemo_gather_rows_aug" in open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "store.hip")).read()


# ----------------------------------------------------------------------------- statistics of the replica
@pytest.mark.parametrize("seed", [1, 1234, 2 ** 40 + 7])
def test_noise_statistics(seed):
    """1365 x 768 = 2^20 elements of one utterance, scaled to unit variance: mean, variance and the correlation of neighbours along
    both axes within about five standard errors; bounded by 510 / sqrt(21845) = 3.45 sigma"""
    ku = R.utterance_keys(seed, 3, 1, [5])[0]
    z = R.noise_k(R.noise_key(ku), 1365, 768) / np.sqrt(R.NOISE_VAR)
    mean, var = z.mean(), z.var()
    corr_c, corr_r = np.mean(z[:, 1:] * z[:, :-1]), np.mean(z[1:] * z[:-1])
    print(f"seed {seed}: mean {mean:.5f} var {var:.5f} corr col {corr_c:.5f} row {corr_r:.5f} max {np.abs(z).max():.3f}")
    assert abs(mean) <= 5e-3 and abs(var - 1.0) <= 1e-2
    assert abs(corr_c) <= 5e-3 and abs(corr_r) <= 5e-3
    assert np.abs(z).max() <= 510 / np.sqrt(R.NOISE_VAR) + 1e-12


def test_span_properties():
    """200 000 ids at L = 400, max_width = 40 (max_frac 0.5: the width cap decides): 0 <= w <= 40, every span ends inside the
    utterance, the mean width is 20; a short utterance is capped by max_frac instead"""
    ids = np.arange(200000)
    s, w = R.spans(1234, 0, 1, ids, [400] * len(ids), 1, 40, 32768)
    print(f"mean width {w.mean():.3f}, widths {w.min()} .. {w.max()}, last masked row {int((s + w).max()) - 1}")
    assert w.min() == 0 and w.max() == 40 and s.min() >= 0 and (s + w).max() <= 400
    assert abs(w.mean() - 20.0) <= 0.1
    s, w = R.spans(1234, 0, 1, ids[:5000], [9] * 5000, 4, 40, 32768)            # W = (9 * 0.5) = 4
    assert w.max() == 4 and (s + w).max() <= 9 and s.shape == (5000, 4)
    s, w = R.spans(1234, 0, 1, ids[:5000], [1] * 5000, 2, 40, 65536)            # L = 1, max_frac = 1: w in {0, 1}; an empty span may sit at row 1
    assert set(w.ravel().tolist()) == {0, 1} and (s + w).max() <= 1 and not s[w == 1].any()


def test_drop_rate_and_exclusion():
    ids = np.arange(200000)
    t = hashrng.thr16(0.1)
    a = R.drop_flags(1234, 0, ids, 0, t)
    b = R.drop_flags(1234, 0, ids, t, 2 * t)
    print(f"drop rate audio {a.mean():.4f} text {b.mean():.4f}")
    assert abs(a.mean() - 0.1) <= 0.003 and abs(b.mean() - 0.1) <= 0.003
    assert not (a & b).any(), "one draw decides: never both modalities"
    assert not R.drop_flags(1234, 0, ids, 0, 0).any()
