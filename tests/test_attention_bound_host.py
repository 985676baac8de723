"""Host proof of the acceptance criteria the GPU attention tests use (tests/attn_reference.py): the bf16 yardstick passes
check(), and small, realistic kernel mistakes planted into the yardstick fail it.  No GPU; float64 on the CPU."""
import pytest
import torch

import attn_reference as R
import hashrng

SHAPES = [  # B, H, Lq, Lk, hd, mask pattern, p
    (2, 2, 400, 400, 96, "prefix", 0.1),
    (2, 2, 128, 400, 96, "prefix", 0.1),
    (2, 2, 400, 128, 96, "prefix", 0.1),
    (1, 4, 50, 1000, 32, "prefix", 0.0),
    (1, 2, 200, 200, 128, "none", 0.0),
    (3, 2, 32, 16, 16, "prefix", 0.1),
    (12, 1, 70, 400, 64, "edges", 0.1),       # the mask patterns of the GPU variant table: every reference finite, exact zeros
    (3, 2, 100, 200, 32, "leading", 0.1),     # where the magnitude is zero
]
SEED, SITE, BOFF = 1234567890123, 40, 5


def _keys_from(lo, hi, fn):
    def hook(x):
        x = x.clone()
        x[..., lo:hi] = fn(x[..., lo:hi])
        return x
    return hook


def _delta_of_row_before(delta):
    delta = delta.clone()
    delta[..., -1] = delta[..., -2]
    return delta


def _ds_tail_missing(ds):
    ds = ds.clone()
    ds[..., -1, -3:] = 0.0
    return ds


def mutants(Lq, Lk, kpm, p):
    """name -> hooks for yardstick(); only the mutants that change something at this shape"""
    inv = hashrng.inv_keep(p)
    out = {"scale_times_1p2e-7": {"scale": 1.0 + 2.0 ** -7}}
    if Lk >= 64 and (kpm is None or not bool(kpm[:, 63].all())):
        out["key63_dropped_from_P"] = {"P": _keys_from(63, 64, lambda x: x * 0.0)}
    if p > 0 and Lk > 64 and (kpm is None or not bool(kpm[:, 64].all())):
        out["keep_without_rescale_keys_64_127"] = {"Pd": _keys_from(64, 128, lambda x: x / inv)}
    if p > 0:
        out["dP_masked_not_rescaled"] = {"dP": lambda x: x / inv}
    if Lq >= 2:
        out["delta_of_last_row_from_row_before"] = {"delta": _delta_of_row_before}
    if kpm is None and Lk >= 3:
        out["last_three_keys_missing_from_dS_of_last_row"] = {"dS": _ds_tail_missing}
    return out


def _case(B, H, Lq, Lk, hd, pattern, p):
    qb, kvb, dob = R.make_inputs(B, H, Lq, Lk, hd, 100 + Lq + Lk)
    d = H * hd
    q, dO = R.heads(qb, B, Lq, H, hd), R.heads(dob, B, Lq, H, hd)
    k, v = R.heads(kvb[:, :d], B, Lk, H, hd), R.heads(kvb[:, d:], B, Lk, H, hd)
    kpm = R.key_padding_mask(pattern, B, Lk)
    keep = torch.from_numpy(hashrng.attn_mask(SEED, SITE, B, H, Lq, Lk, p, BOFF)) if p > 0 else None
    return (q, k, v, dO, kpm, keep, hashrng.inv_keep(p))


@pytest.mark.parametrize("B,H,Lq,Lk,hd,pattern,p", SHAPES)
def test_yardstick_passes_and_every_mutant_fails(B, H, Lq, Lk, hd, pattern, p):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    args = _case(B, H, Lq, Lk, hd, pattern, p)
    kpm = args[4]
    ref, yard, mag = R.reference(*args), R.yardstick(*args), R.magnitude(*args)
    for n in R.OUTPUTS:
        assert torch.isfinite(ref[n]).all() and torch.isfinite(mag[n]).all()
        elem, tile = R.check(yard[n], ref[n], yard[n], mag[n], n)
        print(f"  yardstick {n}: elementwise {elem:.3f}, per tile {tile:.3f} of the limit")
        assert elem <= 0.5                                       # (measured <= 0.40) the kernels get the other half
        assert bool((yard[n][mag[n] == 0] == 0).all())           # zero magnitude: exact zeros
    if kpm is not None:                                          # dK / dV rows of PAD keys have zero magnitude
        pad = kpm[:, None, :, None].expand_as(mag["dK"])
        assert bool((mag["dK"][pad] == 0).all()) and bool((mag["dV"][pad] == 0).all())
    for name, hooks in mutants(Lq, Lk, kpm, p).items():
        mut = R.yardstick(*args, hooks=hooks)
        worst = {n: R.ratios(mut[n], ref[n], yard[n], mag[n]) for n in R.OUTPUTS}
        top = max(max(r) for r in worst.values())
        print(f"  mutant {name}: " + ", ".join(f"{n} {e:.2f}/{t:.2f}" for n, (e, t) in worst.items()))
        assert top > 1.0, f"mutant {name} passes check() on every tensor: {worst}"
        caught = 0
        for n in R.OUTPUTS:
            try:
                R.check(mut[n], ref[n], yard[n], mag[n], n)
            except AssertionError:
                caught += 1
        assert caught >= 1, name


def test_every_mutant_is_exercised():
    seen = set()
    for B, H, Lq, Lk, hd, pattern, p in SHAPES:
        seen |= set(mutants(Lq, Lk, R.key_padding_mask(pattern, B, Lk), p))
    assert len(seen) == 6, seen


def test_check_rejects_non_finite_and_nonzero_where_magnitude_is_zero():
    ref = torch.zeros(1, 1, 64, 16, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    R.check(ref.clone(), ref, ref, mag, "zeros")
    bad = ref.clone()
    bad[0, 0, 3, 5] = 1e-20
    with pytest.raises(AssertionError):
        R.check(bad, ref, ref, mag, "tiny")
    bad[0, 0, 3, 5] = float("nan")
    with pytest.raises(AssertionError):
        R.check(bad, ref, ref, mag + 1.0, "nan")
