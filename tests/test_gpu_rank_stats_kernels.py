"""GPU suite of hriemo_stats_rank and hriemo_stats_confusion through the C ABI (csrc/metrics.hip), the log written by the test: the
fixture's probabilities (float64 sigmoid rounded to fp32, tests/golden/epoch_stats.npz) go straight into probs / truth, so no sigmoid
implementation takes part in the comparison.  Everything the kernels deliver is an integer and is compared exactly with
tests/rank_reference.py.  Every buffer is a GuardedVec: 0xFF outside the operand and inside it until written, so the log behind the
cursor is poison (NaN probabilities, truth bytes 0xFF) and an element of `rank` the kernel skipped would read -1."""
import numpy as np
import pytest
import torch

import rank_reference as R
from conftest import load_golden
from rowops_reference import GuardedVec

pytestmark = pytest.mark.gpu

NAN = float("nan")
_G = {}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def fixture_log(case):
    """(probs fp32 [6, 1000], truth bool [6, 1000]) of a case, class-major: computed once, never changed"""
    if case not in _G:
        g = load_golden("epoch_stats")
        _G[case] = (torch.sigmoid(g[f"{case}_logits"].double()).float().t().contiguous().numpy(), (g[f"{case}_targets"] > 0).t().contiguous().numpy())
    return _G[case]


def run_rank(L, probs, truth, n, capacity, cursor=None):
    """the first n columns of probs / truth [C, >= n] as a log of `capacity` entries, NaN / 0xFF behind them -> rank int64 [C, 2, capacity]"""
    C = probs.shape[0]
    gp = GuardedVec(C * capacity, torch.float32, device="cuda")
    gt = GuardedVec(C * capacity, torch.uint8, device="cuda")
    log_p, log_t = np.full((C, capacity), np.nan, dtype=np.float32), np.full((C, capacity), 0xFF, dtype=np.uint8)
    log_p[:, :n], log_t[:, :n] = probs[:, :n], truth[:, :n]
    gp.view.copy_(torch.from_numpy(log_p).reshape(-1))
    gt.view.copy_(torch.from_numpy(log_t).reshape(-1))
    ctr = GuardedVec.of(torch.tensor([n if cursor is None else cursor, 1, 2, 3, 4, 5, 6, 7], dtype=torch.int32), device="cuda")
    rank = GuardedVec(C * 2 * capacity, torch.int32, device="cuda")
    L.call("hriemo_stats_rank", gp.ptr, gt.ptr, capacity, C, ctr.ptr, rank.ptr, stream())
    torch.cuda.synchronize()
    for name, b in (("probs", gp), ("truth", gt), ("counters", ctr), ("rank", rank)):
        b.assert_intact(name)
    assert torch.equal(gp.view.view(torch.int32).cpu(), torch.from_numpy(log_p).reshape(-1).view(torch.int32)), "the log is read only"
    assert ctr.view.cpu().tolist()[1:] == [1, 2, 3, 4, 5, 6, 7]
    return rank.view.cpu().numpy().reshape(C, 2, capacity).astype(np.int64)


@pytest.mark.parametrize("C", [1, 6])
@pytest.mark.parametrize("cap", ["n", 1000, 1031])
@pytest.mark.parametrize("n", [1, 37, 255, 256, 257, 513, 1000])
def test_rank_equals_the_reference_counts(L, n, cap, C):
    """both cases (cont: distinct probabilities; grid: ties, a class without positives, one without negatives, one all tied); C = 1
    takes class 0 of cont and the all-tied class 5 of grid.  capacity = n: the last block is the log's last; 1031: no multiple of 256"""
    capacity = n if cap == "n" else cap
    for case in ("cont", "grid"):
        probs, truth = fixture_log(case)
        if C == 1:
            k = 0 if case == "cont" else 5
            probs, truth = probs[k:k + 1], truth[k:k + 1]
        got = run_rank(L, probs, truth, n, capacity)
        assert (got[:, :, n:] == 0).all(), "elements at or past the cursor read 0"
        want = R.rank_block(probs, truth, n, capacity)
        assert np.array_equal(got, want), (case, int((got != want).sum()))
        for c in range(C):
            t = truth[c, :n]
            assert (got[c, 0, :n][t] >= 1).all() and (got[c, 1, :n][~t] >= 1).all(), "an entry counts itself"
            assert got[c, 0, :n].max(initial=0) <= t.sum() and got[c, 1, :n].max(initial=0) <= (~t).sum()


@pytest.mark.parametrize("cursor,n", [(0, 0), (-3, 0), (5000, 300), (301, 300)])
def test_rank_cursor_at_zero_and_clamped(L, cursor, n):
    """a cursor of 0 (or below): every element is stored as 0; a cursor above the capacity counts as the capacity"""
    probs, truth = fixture_log("grid")
    got = run_rank(L, probs, truth, n, 300, cursor=cursor)
    assert np.array_equal(got, R.rank_block(probs, truth, n, 300))
    if n == 0:
        assert not got.any()


def test_rank_nan_probability_gets_zero(L):
    """a NaN inside the log (the host refuses such an epoch anyway): it compares false with everything -- 0 / 0 for itself, and it
    counts for nobody"""
    probs, truth = (a[:, :300].copy() for a in fixture_log("cont"))
    probs[2, 100] = NAN
    got = run_rank(L, probs, truth, 300, 300)
    keep = np.arange(300) != 100
    want = R.rank_block(probs[:, keep], truth[:, keep], 299, 299)
    assert got[2, 0, 100] == 0 and got[2, 1, 100] == 0 and np.array_equal(got[:, :, keep][2], want[2])


def test_rank_refusals_launch_nothing(L):
    lib = L.lib()
    gp, gt = GuardedVec(8, torch.float32, device="cuda"), GuardedVec(8, torch.uint8, device="cuda")
    ctr, rank = GuardedVec(8, torch.int32, device="cuda"), GuardedVec(16, torch.int32, device="cuda")
    ok = [gp.ptr, gt.ptr, 8, 1, ctr.ptr, rank.ptr, stream()]
    for at, bad in ((2, 0), (2, -1), (3, 0), (0, None), (1, None), (4, None), (5, None), (4, ctr.ptr + 2), (5, rank.ptr + 1)):
        args = list(ok)
        args[at] = bad
        assert lib.hriemo_stats_rank(*args) != 0, (at, bad)
        assert L.lib().hriemo_last_error().decode().startswith("stats_rank")
    torch.cuda.synchronize()
    assert (rank.raw == 0xFF).all() and (ctr.raw == 0xFF).all(), "nothing was launched"


# ----------------------------------------------------------------------------- confusion
def sl_batch(B, C, seed):
    """logits on a grid of 1/4 (rows tie), a NaN logit in every 11th row, labels in [0, C) with -100 / out-of-range ones mixed in"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(-8, 9, (B, C), generator=g).float() / 4.0)
    y = torch.randint(0, C, (B,), generator=g)
    x[torch.arange(B), y] += 0.5
    for b in range(0, B, 11):
        x[b, (b // 11) % C] = NAN
    if C > 2 and B > 3:
        x[3] = 1.0                                       # a full tie: the first index
    y[5::13] = -100
    y[7::29] = C                                         # one past the last class
    y[8::31] = -1
    if B > 40:
        y[40] = 1 << 40                                  # does not fit an int32: nothing may be indexed with it
    return x, y


class Cm:
    """cm of one epoch in a guarded buffer + the reference's counts of what was offered"""

    def __init__(self, C):
        self.C = C
        self.cm = GuardedVec(C * C + 2, torch.int32, device="cuda")
        self.cm.view.zero_()
        self.want = np.zeros(C * C + 2, dtype=np.int64)
        self.bufs = []

    def update(self, L, x, y, loss=0.5, n_valid=None, skip=0, counted=True):
        B, C = x.shape
        nv = B if n_valid is None else min(max(n_valid, 1), B)
        gx, gy = GuardedVec.of(x, device="cuda"), GuardedVec.of(y, device="cuda")
        gl = GuardedVec.of(torch.tensor([loss], dtype=torch.float32), device="cuda")
        gn = GuardedVec.of(torch.tensor([n_valid], dtype=torch.int32), device="cuda") if n_valid is not None else None
        L.call("hriemo_stats_confusion", gx.ptr, gy.ptr, gl.ptr, skip, gn.ptr if gn else None, B, C, self.cm.ptr, stream())
        self.bufs += [b for b in (gx, gy, gl, gn) if b is not None]
        if counted:
            self.want += R.confusion(x[:nv].numpy(), y[:nv].numpy(), C)

    def check(self):
        torch.cuda.synchronize()
        self.cm.assert_intact("cm")
        for b in self.bufs:
            b.assert_intact("an input")
        got = self.cm.view.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, self.want), (got, self.want)
        return got


@pytest.mark.parametrize("n_valid", [None, 1, "B-1"])
@pytest.mark.parametrize("B", [1, 64, 257, 300])
def test_confusion_counts_only_the_valid_samples(L, B, n_valid):
    """C = 4.  The rows behind n_valid hold NaN logits and labels that would count as bad; B - 1 = 0 for B = 1 clamps to 1; B = 257
    and 300: a second trip of the block"""
    nv = B - 1 if n_valid == "B-1" else n_valid
    x, y = sl_batch(B, 4, 10 + B)
    if nv is not None:
        x[max(nv, 1):], y[max(nv, 1):] = NAN, 12345
    st = Cm(4)
    st.update(L, x, y, n_valid=nv)
    got = st.check()
    assert got.sum() == (B if nv is None else max(nv, 1)), "every valid sample lands in exactly one cell"
    if B >= 64 and nv is None:
        assert got[16] > 0 and got[17] > 0, "the batch holds ignored and bad labels"


def test_confusion_ties_and_nan_take_the_stated_index(L):
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, NAN, 5.0, NAN], [7.0, 1.0, 0.0, 7.0], [0.0, 1.0, 2.0, 3.0], [NAN, NAN, NAN, NAN]])
    y = torch.tensor([1, 0, 1, 3, 3, 2])
    st = Cm(4)
    st.update(L, x, y)
    got = st.check()[:16].reshape(4, 4)
    want = np.zeros((4, 4), dtype=np.int64)
    want[1, 1], want[0, 0], want[3, 0], want[3, 3], want[2, 0] = 2, 1, 1, 1, 1
    assert np.array_equal(got, want)


@pytest.mark.parametrize("C", [1, 64])
def test_confusion_smallest_and_largest_class_count(L, C):
    x, y = sl_batch(300, C, 3)
    st = Cm(C)
    st.update(L, x, y)
    st.update(L, x, y, n_valid=77)
    st.check()


@pytest.mark.parametrize("skip", [0, 1])
def test_confusion_non_finite_loss(L, skip):
    """skip_nonfinite and a NaN / Inf loss: cm untouched -- the batch hriemo_stats_update only counts in n_skipped; without it the batch counts"""
    x, y = sl_batch(64, 4, 4)
    st = Cm(4)
    st.update(L, x, y, skip=skip)
    st.update(L, x, y, loss=NAN, skip=skip, counted=not skip)
    st.update(L, x, y, loss=float("inf"), skip=skip, counted=not skip)
    st.update(L, x, y, loss=float("-inf"), skip=skip, counted=not skip)
    assert st.check().sum() == (64 if skip else 256)


def test_confusion_three_launches_equal_one_concatenated_batch(L):
    x, y = sl_batch(300, 4, 5)
    one, three = Cm(4), Cm(4)
    one.update(L, x, y)
    for lo, hi in ((0, 7), (7, 8), (8, 300)):
        three.update(L, x[lo:hi], y[lo:hi])
    assert np.array_equal(one.check(), three.check())


def test_confusion_refusals_launch_nothing(L):
    lib = L.lib()
    gx, gy = GuardedVec(16, torch.float32, device="cuda"), GuardedVec(4, torch.int64, device="cuda")
    gl, gn, cm = GuardedVec(1, torch.float32, device="cuda"), GuardedVec(1, torch.int32, device="cuda"), GuardedVec(18, torch.int32, device="cuda")
    ok = [gx.ptr, gy.ptr, gl.ptr, 0, gn.ptr, 4, 4, cm.ptr, stream()]
    for at, bad in ((5, 0), (6, 0), (6, 65), (0, None), (1, None), (2, None), (7, None), (4, gn.ptr + 2), (7, cm.ptr + 1)):
        args = list(ok)
        args[at] = bad
        assert lib.hriemo_stats_confusion(*args) != 0, (at, bad)
        assert L.lib().hriemo_last_error().decode().startswith("stats_confusion")
    torch.cuda.synchronize()
    assert (cm.raw == 0xFF).all(), "nothing was launched"
