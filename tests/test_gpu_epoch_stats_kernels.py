"""GPU suite of the epoch-statistics kernels through the C ABI (csrc/metrics.hip): hriemo_stats_update against a host model of its
contract (logged probabilities within 4 ulp of torch.sigmoid, truth bits and counters exact, float64 sums within 1e-12 relative of a
float64 host sum), hriemo_stats_counts / hriemo_stats_auc on logs the update kernel wrote from the logits of
tests/golden/epoch_stats.npz against the fixture's integers, exactly.  Every buffer is a GuardedVec: 0xFF outside the operand --
and inside it until written, so the log past the cursor is poison (NaN probabilities, truth bytes 0xFF)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from rowops_reference import GuardedVec

pytestmark = pytest.mark.gpu

CTR = {"cursor": 0, "n_samples": 1, "n_batches": 2, "n_skipped": 3, "n_correct": 4, "n_nonfinite": 5, "overflow": 6}
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


class State:
    """the device state of one epoch in guarded buffers + the host model of what hriemo_stats_update does to it"""

    def __init__(self, C, capacity, single=False, cursor=0):
        self.C, self.cap, self.single = C, capacity, single
        self.probs = GuardedVec(C * capacity, torch.float32, device="cuda")
        self.truth = GuardedVec(C * capacity, torch.uint8, device="cuda")
        self.counters = GuardedVec(8, torch.int32, device="cuda")
        self.sums = GuardedVec(4, torch.float64, device="cuda")
        self.counters.view.zero_()
        self.sums.view.zero_()
        self.counters.view[0] = cursor
        self.m_ctr, self.m_sums = [cursor, 0, 0, 0, 0, 0, 0, 0], [0.0, 0.0, 0.0]
        self.m_probs = np.full((C, capacity), np.nan, dtype=np.float32)      # NaN: never written
        self.m_truth = np.full((C, capacity), 0xFF, dtype=np.uint8)
        self.bufs = []

    def update(self, L, x, tgt, loss, beta=None, n_valid=None, loss_scale=1.0, skip=0):
        """one launch (operands in guarded buffers of their own) and the same step on the host model"""
        B, C = x.shape
        gx = GuardedVec.of(x, device="cuda")
        gt = GuardedVec.of(tgt if self.single else tgt.float(), device="cuda")
        gl = GuardedVec.of(torch.tensor([loss], dtype=torch.float32), device="cuda")
        gb = GuardedVec.of(beta, device="cuda") if beta is not None else None
        gn = GuardedVec.of(torch.tensor([n_valid], dtype=torch.int32), device="cuda") if n_valid is not None else None
        bps = beta.numel() // B if beta is not None else 0
        L.call("hriemo_stats_update", gx.ptr, None if self.single else gt.ptr, gt.ptr if self.single else None, gl.ptr, float(loss_scale),
               gb.ptr if gb else None, bps, gn.ptr if gn else None, B, C, skip, None if self.single else self.probs.ptr,
               None if self.single else self.truth.ptr, self.cap, self.counters.ptr, self.sums.ptr, stream())
        self.bufs += [g for g in (gx, gt, gl, gb, gn) if g is not None]
        # ---- host model
        nv = B if n_valid is None else min(max(n_valid, 1), B)
        c = self.m_ctr
        if skip and not math.isfinite(loss):
            c[3] += 1
            return
        xs = x[:nv]
        if self.single:
            c[4] += int((xs.argmax(1) == tgt[:nv]).sum())
        else:
            p, t = torch.sigmoid(xs), tgt[:nv] > 0
            c[4] += int(((p > 0.5) == t).all(1).sum())
            if c[0] + nv <= self.cap:
                self.m_probs[:, c[0]:c[0] + nv] = p.t().numpy()
                self.m_truth[:, c[0]:c[0] + nv] = t.t().numpy()
                c[5] += int((~torch.isfinite(xs)).sum())
                c[0] += nv
            else:
                c[6] = 1
        c[1] += nv
        c[2] += 1
        self.m_sums[0] += float(np.float32(loss)) * loss_scale * nv
        if beta is not None:
            self.m_sums[1] += float(beta.reshape(B, -1)[:nv].double().sum())
            self.m_sums[2] += nv * bps

    def check(self):
        torch.cuda.synchronize()
        for name, g in (("probs", self.probs), ("truth", self.truth), ("counters", self.counters), ("sums", self.sums)):
            g.assert_intact(name)
        for g in self.bufs:
            g.assert_intact("an input")
        ctr = self.counters.view.cpu().tolist()
        assert ctr[:7] == self.m_ctr[:7], (ctr, self.m_ctr)
        sums = self.sums.view.cpu().tolist()
        for i, (a, b) in enumerate(zip(sums[:3], self.m_sums)):
            if b != b:
                assert a != a, (i, a)
            else:
                assert abs(a - b) <= 1e-12 * abs(b), (i, a, b)
        if self.single:
            return
        got_p = self.probs.view.cpu().numpy().reshape(self.C, self.cap)
        got_t = self.truth.view.cpu().numpy().reshape(self.C, self.cap)
        assert np.array_equal(got_t, self.m_truth), "truth bits (0xFF: never written)"
        written = ~np.isnan(self.m_probs)
        assert np.array_equal(np.isnan(got_p), ~written), "entries written / left alone"
        ulp = np.abs(got_p[written].view(np.int32).astype(np.int64) - self.m_probs[written].view(np.int32).astype(np.int64))
        worst = int(ulp.max()) if ulp.size else 0
        print(f"logged probabilities: {int(written.sum())} values, largest distance to torch.sigmoid {worst} ulp")
        assert worst <= 4, worst


def batch(B, C, seed, bps=1):
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(B, C, generator=g)
    y = torch.where(torch.rand(B, C, generator=g) < 0.4, torch.rand(B, C, generator=g) * 3.0, torch.zeros(B, C))
    y = torch.where(torch.rand(B, C, generator=g) < 0.1, -torch.ones(B, C), y)
    beta = torch.rand(B * bps, generator=g) if bps else None
    return x, y, beta


# ----------------------------------------------------------------------------- update
@pytest.mark.parametrize("n_valid", [None, 1, 3, 5])
def test_update_counts_only_the_valid_samples(L, n_valid):
    """B = 5, C = 6: the rows behind n_valid hold NaN (logits, targets, beta) and leave no trace; a logit of exactly 0 in a valid row"""
    x, y, beta = batch(5, 6, 1)
    x[0, 2] = 0.0
    if n_valid is not None:
        x[n_valid:], y[n_valid:], beta[n_valid:] = NAN, NAN, NAN
    st = State(6, 16)
    st.update(L, x, y, 0.75, beta, n_valid)
    st.check()
    assert st.m_ctr[0] == (5 if n_valid is None else n_valid) and st.m_ctr[5] == 0


def test_update_second_trip_of_the_block_and_three_betas_per_sample(L):
    x, y, beta = batch(300, 6, 2, bps=3)
    x[257:], y[257:] = NAN, NAN
    beta[257 * 3:] = NAN
    st = State(6, 320)
    st.update(L, x, y, 1.25, beta, 257, loss_scale=2.0)
    st.check()
    assert st.m_ctr[:3] == [257, 257, 1]


def test_update_one_class_no_beta_and_clamped_n_valid(L):
    x, y, _ = batch(5, 1, 3, bps=0)
    st = State(1, 16)
    st.update(L, x, y, 0.5)
    st.update(L, x, y, 0.5, n_valid=0)              # clamp(0, 1, B) = 1, as hriemo_fusion_loss_n
    st.update(L, x, y, 0.5, n_valid=9)              # clamp(9, 1, B) = 5
    st.check()
    assert st.m_ctr[:3] == [11, 11, 3] and st.m_sums[2] == 0.0


def test_update_single_label_ties_take_the_first_maximum(L):
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0], [7.0, 1.0, 0.0, 7.0], [0.0, 1.0, 2.0, 3.0]])
    labels = torch.tensor([1, 0, 3, 0, 3])
    st = State(4, 1, single=True)
    st.update(L, x, labels, 2.0, torch.full((15,), 0.25))
    assert st.m_ctr[4] == 4
    st.update(L, x, labels, 4.0, torch.full((5,), 0.75), n_valid=2)
    st.check()
    assert st.m_ctr[:5] == [0, 7, 2, 0, 6]


@pytest.mark.parametrize("skip", [0, 1])
def test_update_non_finite_loss(L, skip):
    """skip_nonfinite: a NaN / Inf loss bumps n_skipped and nothing else; without it the batch is logged and the sum goes NaN"""
    x, y, beta = batch(5, 6, 4)
    st = State(6, 16)
    st.update(L, x, y, 0.5, beta, skip=skip)
    st.update(L, x, y, NAN, beta, skip=skip)
    if skip:
        st.update(L, x, y, float("inf"), beta, skip=skip)
    st.check()
    assert st.m_ctr[:4] == ([5, 5, 1, 2] if skip else [10, 10, 2, 0])


@pytest.mark.parametrize("room", [0, -1])
def test_update_at_the_end_of_the_log(L, room):
    """cursor at capacity - nv: the batch fits exactly; one further: the overflow word is set, the log stays untouched, sums and counters move"""
    x, y, beta = batch(5, 6, 5)
    x[3:] = NAN
    st = State(6, 32, cursor=32 - 3 - room)
    st.update(L, x, y, 0.5, beta, 3)
    st.check()
    assert st.m_ctr[6] == (0 if room == 0 else 1) and st.m_ctr[1] == 3 and st.m_ctr[0] == (32 if room == 0 else 30)


def test_three_launches_equal_one_concatenated_batch(L):
    x, y, beta = batch(21, 6, 6)
    one, three = State(6, 32), State(6, 32)
    one.update(L, x, y, 0.5, beta)
    for lo, hi in ((0, 7), (7, 8), (8, 21)):
        three.update(L, x[lo:hi], y[lo:hi], 0.5, beta[lo:hi])
    one.check()
    three.check()
    assert torch.equal(one.probs.view.view(torch.int32), three.probs.view.view(torch.int32)), "bit for bit, the poison behind the cursor included"
    assert torch.equal(one.truth.view, three.truth.view)
    a, b = one.counters.view.cpu().tolist(), three.counters.view.cpu().tolist()
    assert a[0] == b[0] == 21 and a[1] == b[1] and a[4] == b[4] and (a[2], b[2]) == (1, 3)
    sa, sb = one.sums.view.cpu().tolist(), three.sums.view.cpu().tolist()
    assert abs(sa[0] - sb[0]) <= 1e-12 * abs(sa[0]) and abs(sa[1] - sb[1]) <= 1e-12 * abs(sa[1]) and sa[2] == sb[2] == 21.0


# ----------------------------------------------------------------------------- counts / auc
CAP = 1024
_LOGS = {}


def fixture_log(L, case):
    """the fixture's 1000 samples written by the update kernel in ONE launch; the cursor is then set per test"""
    if case not in _LOGS:
        g = load_golden("epoch_stats")
        st = State(6, CAP)
        st.update(L, g[f"{case}_logits"], g[f"{case}_targets"], 0.5)
        st.check()
        _LOGS[case] = (g, st)
    return _LOGS[case]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 301, 1000])
@pytest.mark.parametrize("case", ["cont", "grid"])
def test_counts_and_auc_equal_the_fixture_integers(L, case, n):
    """the first n log entries (cursor = n; what lies behind the cursor -- later fixture samples up to 1000, 0xFF poison behind them --
    must not count): tp / fp / fn at 0.5 and the 19 sweep thresholds, 2U, n_pos, n_neg, all exactly the fixture's"""
    from hri_emo_amd.train import thresholds_up
    g, st = fixture_log(L, case)
    C, S = 6, 20
    st.counters.view[0] = n
    thr = GuardedVec.of(torch.from_numpy(thresholds_up(np.concatenate([[0.5], g["sweep"].numpy()]))), device="cuda")
    tiles = L.lib().hriemo_stats_auc_tiles(CAP)
    assert tiles == 4 and L.lib().hriemo_stats_auc_tiles(1025) == 5 and L.lib().hriemo_stats_auc_tiles(1) == 1
    out = GuardedVec(C * S * 3, torch.int32, device="cuda")
    partial = GuardedVec(C * tiles, torch.int64, device="cuda")
    npn = GuardedVec(C * 2, torch.int32, device="cuda")
    L.call("hriemo_stats_counts", st.probs.ptr, st.truth.ptr, CAP, C, st.counters.ptr, thr.ptr, S, out.ptr, stream())
    L.call("hriemo_stats_auc", st.probs.ptr, st.truth.ptr, CAP, C, st.counters.ptr, partial.ptr, npn.ptr, stream())
    torch.cuda.synchronize()
    for name, b in (("thresholds", thr), ("counts", out), ("partial", partial), ("npn", npn), ("probs", st.probs), ("truth", st.truth),
                    ("counters", st.counters)):
        b.assert_intact(name)
    k = f"{case}_{n}_"
    assert np.array_equal(out.view.cpu().numpy().reshape(C, S, 3), g[k + "counts"].numpy())
    part = partial.view.cpu().numpy().reshape(C, tiles)
    assert (part >= 0).all(), "every tile is stored"
    assert (part[:, -(-n // 256):] == 0).all(), "tiles past the cursor hold 0"
    assert np.array_equal(part.sum(1), g[k + "two_u"].numpy()), (part.sum(1), g[k + "two_u"])
    got = npn.view.cpu().numpy().reshape(C, 2)
    assert np.array_equal(got[:, 0], g[k + "n_pos"].numpy()) and np.array_equal(got[:, 1], g[k + "n_neg"].numpy())


def test_epoch_stats_on_the_device_reproduces_the_reference(L):
    """train.EpochStats on CUDA tensors, fed in the fixture's batches: every float of result() within 1e-12 of the reference's, the
    thresholds equal, and equal to the CPU path's integers"""
    from hri_emo_amd.train import EpochStats
    g = load_golden("epoch_stats")
    bs = int(g["batch"])
    for case in ("cont", "grid"):
        dev, cpu = EpochStats(6, 1000, device="cuda"), EpochStats(6, 1000, device="cpu")
        for i, lo in enumerate(range(0, 1000, bs)):
            args = [g[f"{case}_{k}"][lo:lo + bs] for k in ("logits", "beta", "targets")] + [g[f"{case}_losses"][i]]
            cpu.update(*args)
            dev.update(*[a.cuda() for a in args])
        r, h = dev.result(), cpu.result()
        k = f"{case}_1000_"
        for name, key in (("micro_f1", "micro_f1"), ("macro_f1", "macro_f1"), ("macro_auc", "macro_auc"), ("macro_f1_calibrated", "macro_f1_cal")):
            assert abs(r[name] - float(g[k + key])) <= 1e-12, (case, name)
        assert np.array_equal(r["calibrated_thresholds"], g[k + "thresholds"].numpy())
        assert abs(r["avg_loss"] - float(g[f"{case}_avg_loss"])) <= 1e-12 and abs(r["mean_beta"] - float(g[f"{case}_mean_beta"])) <= 1e-12
        for name in ("tp", "fp", "fn", "sweep_counts", "auc_2u", "n_pos", "n_neg"):
            assert np.array_equal(r[name], h[name]), name
        assert (r["n_samples"], r["n_batches"], r["n_correct"], r["n_logged"]) == (1000, 16, int(g[k + "correct"]), 1000)
        dev.reset()
        assert dev.result()["n_samples"] == 0
