"""GPU suite of hriemo_predict_log through the C ABI (csrc/metrics.hip) against float64 numpy references.  Every output (probs,
beta_mean, pred) is a GuardedVec: 0xFF outside the operand -- and inside it until written, so an entry the kernel should have
left alone still reads as poison.  Rows behind nv = clamp(n_valid, 1, B) hold NaN in logits and beta.

Bounds.  kind 0: torch.equal with the log hriemo_stats_update writes for the same logits, and within 4 ulp of torch.sigmoid (the
bound of test_gpu_epoch_stats_kernels.py).  kind 1 against the float64 softmax rounded to fp32: SOFTMAX_ULP = twice the worst
distance measured on the first MI355X run over these inputs (worst 3 ulp over 39 744 values; profiles/2026-10-20_eval_step.log),
under the cap of 16 ulp above which the arithmetic would be wrong (no max subtraction, a 16-bit format somewhere), not noisy.
Rows sum to 1 within C ulp of 1.  beta_mean within 1 ulp of the float64 mean rounded to fp32."""
import numpy as np
import pytest
import torch

from rowops_reference import GuardedVec

pytestmark = pytest.mark.gpu

NAN = float("nan")
SOFTMAX_ULP = 6
assert SOFTMAX_ULP <= 16
BS, CS, BPS, NVS = (1, 5, 43, 64, 65), (1, 4, 6, 7), (None, 1, 128, 130), (None, 0, 3, "B", "B+3")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def ulps(a, b):
    """distance in fp32 representation steps between two float32 arrays of finite values of equal sign (or zero)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


class Log:
    """the device state of one prediction log in guarded buffers"""

    def __init__(self, C, cap, cursor=0, counters=None):
        self.C, self.cap = C, cap
        self.probs = GuardedVec(C * cap, torch.float32, device="cuda")
        self.beta_mean = GuardedVec(cap, torch.float32, device="cuda")
        self.pred = GuardedVec(cap, torch.int32, device="cuda")
        self.counters = GuardedVec.of(torch.tensor(counters or [cursor, 0, 0, 0], dtype=torch.int32), device="cuda")
        self.inputs = []

    def launch(self, L, kind, x, beta=None, bps=0, n_valid=None, pred=True, beta_mean=True):
        B, C = x.shape
        gx = GuardedVec.of(x, device="cuda")
        gb = GuardedVec.of(beta, device="cuda") if beta is not None else None
        gn = GuardedVec.of(torch.tensor([n_valid], dtype=torch.int32), device="cuda") if n_valid is not None else None
        self.inputs += [g for g in (gx, gb, gn) if g is not None]
        L.call("hriemo_predict_log", gx.ptr, gb.ptr if gb else None, bps, gn.ptr if gn else None, B, C, kind, self.probs.ptr,
               self.beta_mean.ptr if beta_mean else None, self.pred.ptr if pred else None, self.cap, self.counters.ptr, stream())

    def read(self):
        torch.cuda.synchronize()
        for name, g in (("probs", self.probs), ("beta_mean", self.beta_mean), ("pred", self.pred), ("counters", self.counters)):
            g.assert_intact(name)
        for g in self.inputs:
            g.assert_intact("an input")
        return (self.probs.view.cpu().numpy().reshape(self.C, self.cap), self.beta_mean.view.cpu().numpy(), self.pred.view.cpu().numpy(),
                self.counters.view.cpu().tolist())


def untouched(a):
    """entries that still hold the 0xFF poison"""
    return a.view(np.int32) == -1


def make(B, C, bps, n_valid, seed, special=False):
    """logits [B, C], beta [B * bps] | None and nv; the rows behind nv are NaN"""
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(B, C, generator=g)
    if special and C >= 2:
        # rows that overflow an unshifted softmax, and ties
        for b, row in enumerate(([80.0, -80.0], [-80.0, 80.0], [1e4, -1e4], [-1e4, 1e4], [3.0, 3.0], [-80.0, -80.0], [1e4, 1e4])):
            if b < B:
                x[b, :2] = torch.tensor(row)
                x[b, 2:] = x[b, 2:].clamp(-3.0, 3.0)
        if B > 7 and C >= 3:
            x[7] = 0.5
            x[7, C - 1] = 2.0
            x[7, 1] = 2.0                       # the maximum twice: index 1 wins
    beta = torch.rand(B * bps, generator=g) if bps else None
    nv = B if n_valid is None else min(max(n_valid, 1), B)
    x[nv:] = NAN
    if beta is not None:
        beta[nv * bps:] = NAN
    return x, beta, nv


def softmax64(x):
    x = x.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


_WORST = {"softmax": 0, "values": 0}


@pytest.mark.parametrize("kind", [0, 1], ids=["multi_label", "single_label"])
@pytest.mark.parametrize("B", BS)
def test_log_against_the_float64_references(L, B, kind):
    """every C, beta_per_sample and n_valid of the issue at this B, appended at cursor 3 of a log of B + 9 samples"""
    cap, cursor = B + 9, 3
    worst_sig = worst_soft = worst_beta = 0
    for C in CS:
        for bps in BPS:
            for nvs in NVS:
                n_valid = {"B": B, "B+3": B + 3}.get(nvs, nvs)
                x, beta, nv = make(B, C, bps, n_valid, seed=B * 100 + C, special=(kind == 1))
                log = Log(C, cap, cursor)
                log.launch(L, kind, x, beta, bps or 0, n_valid, pred=(kind == 1))
                what = (B, C, bps, nvs)
                if kind == 0:
                    # the statistics' log of the same logits
                    st_p, st_t = GuardedVec(C * cap, torch.float32, device="cuda"), GuardedVec(C * cap, torch.uint8, device="cuda")
                    st_c = GuardedVec.of(torch.tensor([cursor] + [0] * 7, dtype=torch.int32), device="cuda")
                    st_s = GuardedVec.of(torch.zeros(4, dtype=torch.float64), device="cuda")
                    gx, gy = GuardedVec.of(x, device="cuda"), GuardedVec.of(torch.zeros(B, C), device="cuda")
                    gl = GuardedVec.of(torch.tensor([0.5]), device="cuda")
                    gn = GuardedVec.of(torch.tensor([n_valid if n_valid is not None else B], dtype=torch.int32), device="cuda")
                    L.call("hriemo_stats_update", gx.ptr, gy.ptr, None, gl.ptr, 1.0, None, 0, gn.ptr, B, C, 0, st_p.ptr, st_t.ptr, cap, st_c.ptr,
                           st_s.ptr, stream())
                probs, bmean, pred, ctr = log.read()
                assert ctr == [cursor + nv, nv, 0, 0], (what, ctr)
                sl = slice(cursor, cursor + nv)
                assert untouched(probs[:, :cursor]).all() and untouched(probs[:, cursor + nv:]).all(), what
                assert not untouched(probs[:, sl]).any() and np.isfinite(probs[:, sl]).all(), what
                xs = x[:nv]
                if kind == 0:
                    assert torch.equal(log.probs.view.view(torch.int32), st_p.view.view(torch.int32)), (what, "not the bits of hriemo_stats_update")
                    d = ulps(probs[:, sl], torch.sigmoid(xs).t().numpy())
                    worst_sig = max(worst_sig, int(d.max()))
                    assert untouched(pred).all(), what
                else:
                    ref = softmax64(xs.numpy()).astype(np.float32).T
                    d = ulps(probs[:, sl], ref)
                    worst_soft = max(worst_soft, int(d.max()))
                    _WORST["values"] += d.size
                    total = probs[:, sl].astype(np.float64).sum(axis=0)
                    assert (np.abs(total - 1.0) <= C * 2.0 ** -23).all(), (what, total)
                    assert np.array_equal(pred[sl], xs.numpy().argmax(axis=1)), what
                    assert np.array_equal(pred[sl], xs.argmax(dim=1).numpy()), (what, "torch.argmax")
                    assert untouched(pred[:cursor]).all() and untouched(pred[cursor + nv:]).all(), what
                if bps:
                    refb = beta.reshape(B, bps)[:nv].double().numpy().mean(axis=1).astype(np.float32)
                    worst_beta = max(worst_beta, int(ulps(bmean[sl], refb).max()))
                    assert untouched(bmean[:cursor]).all() and untouched(bmean[cursor + nv:]).all(), what
                else:
                    assert untouched(bmean).all(), what
    _WORST["softmax"] = max(_WORST["softmax"], worst_soft)
    print(f"B = {B} kind {kind}: worst distance to torch.sigmoid {worst_sig} ulp, to the float64 softmax {worst_soft} ulp "
          f"(so far {_WORST['softmax']} ulp over {_WORST['values']} values), beta_mean {worst_beta} ulp")
    assert worst_sig <= 4 and worst_soft <= SOFTMAX_ULP and worst_beta <= 1


def test_single_label_extreme_rows_and_ties(L):
    """logits of +-80 and +-1e4 stay finite (the row maximum is subtracted), ties pick the first index, pred = NULL is accepted"""
    x, _, _ = make(8, 4, None, None, seed=5, special=True)
    log = Log(4, 8)
    log.launch(L, 1, x)
    probs, _, pred, ctr = log.read()
    assert ctr == [8, 8, 0, 0] and np.isfinite(probs).all()
    assert pred.tolist() == [0, 1, 0, 1, 0, int(x[5].argmax()), 0, 1], pred.tolist()
    assert probs[0, 0] == 1.0 and probs[1, 0] == 0.0 and probs[0, 2] == 1.0 and probs[1, 3] == 1.0
    assert probs[0, 4] == probs[1, 4] and probs[0, 6] == probs[1, 6]
    assert int(ulps(probs, softmax64(x.numpy()).astype(np.float32).T).max()) <= SOFTMAX_ULP
    log = Log(4, 8)
    log.launch(L, 1, x, pred=False)
    probs2, _, pred2, _ = log.read()
    assert np.array_equal(probs, probs2) and untouched(pred2).all()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("room", [0, -1])
def test_the_end_of_the_log(L, kind, room):
    """cursor + nv == capacity fits; one sample more sets overflow, appends nothing, leaves every canary and still counts n_samples"""
    x, beta, nv = make(5, 6, 2, 3, seed=7)
    cap = 32
    log = Log(6, cap, counters=[cap - 3 - room, 10, 0, 0])
    log.launch(L, kind, x, beta, 2, 3)
    probs, bmean, pred, ctr = log.read()
    if room == 0:
        assert ctr == [cap, 13, 0, 0]
        assert not untouched(probs[:, cap - 3:]).any() and untouched(probs[:, :cap - 3]).all() and not untouched(bmean[cap - 3:]).any()
    else:
        assert ctr == [cap - 2, 13, 1, 0]
        assert untouched(probs).all() and untouched(bmean).all() and untouched(pred).all()


@pytest.mark.parametrize("kind", [0, 1])
def test_non_finite_logits_are_counted_among_the_logged_rows_only(L, kind):
    x, _, _ = make(6, 4, None, None, seed=9)
    x[0, 1], x[2, 0], x[2, 3], x[3, 2] = NAN, float("inf"), float("-inf"), NAN
    x[4:] = NAN                                                  # behind n_valid = 4: never read, never counted
    log = Log(4, 16, counters=[0, 0, 0, 2])
    log.launch(L, kind, x, n_valid=4)
    probs, _, pred, ctr = log.read()
    assert ctr == [4, 4, 0, 2 + 4], ctr
    assert np.isfinite(probs[:, 1]).all() and untouched(probs[:, 4:]).all()
    if kind == 1:
        assert pred[:4].tolist() == [1, int(x[1].argmax()), 0, 2], "a NaN counts as maximal (torch.argmax), else the first maximum"
    # an overflowing batch counts no non-finite logits: none was logged
    log = Log(4, 3, counters=[0, 0, 0, 0])
    log.launch(L, kind, x, n_valid=4)
    assert log.read()[3] == [0, 4, 1, 0]


def test_refusals_leave_the_log_untouched(L):
    x, beta, _ = make(5, 4, 2, None, seed=11)
    gx, gb = GuardedVec.of(x, device="cuda"), GuardedVec.of(beta, device="cuda")
    gn = GuardedVec.of(torch.tensor([3, 3], dtype=torch.int32), device="cuda")
    log = Log(4, 16)
    ok = dict(logits=gx.ptr, beta=gb.ptr, bps=2, n_valid=gn.ptr, B=5, C=4, kind=0, probs=log.probs.ptr, beta_mean=log.beta_mean.ptr,
              pred=log.pred.ptr, capacity=16, counters=log.counters.ptr)
    bad = [("B", 0), ("C", 0), ("capacity", 0), ("B", -1), ("kind", 2), ("kind", -1), ("logits", None), ("probs", None), ("counters", None),
           ("bps", 0), ("n_valid", gn.ptr + 2), ("counters", log.counters.ptr + 1), ("pred", log.pred.ptr + 2)]
    for name, value in bad:
        args = dict(ok)
        args[name] = value
        rc = L.lib().hriemo_predict_log(*args.values(), stream())
        assert rc != 0 and b"predict_log" in L.lib().hriemo_last_error(), (name, value, rc)
    probs, bmean, pred, ctr = log.read()
    assert ctr == [0, 0, 0, 0] and untouched(probs).all() and untouched(bmean).all() and untouched(pred).all()
    assert L.lib().hriemo_predict_log(*ok.values(), stream()) == 0
    assert log.read()[3] == [3, 3, 0, 0]
