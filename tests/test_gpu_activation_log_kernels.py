"""GPU suite of the activation log's kernels, through the C ABI: hriemo_act_log_plan, hriemo_act_probe, hriemo_act_log_fold
(csrc/actlog.hip) against the float64 reference of actlog_reference.py.

n_rows, n_bad, first_bad_row, absmax and have are compared exactly, sumsq within the bound counted from the kernels' summation
tree.  Shapes: with R = 32 rows per chunk, n_rows in {1, R - 1, R, R + 1, 2R + 1}, d in {8, 64, 776}, bf16 and fp32 sources whose
leading dimension is larger than d with NaN-poisoned columns between the rows; every row layout the probe serves, with whatever
must not count (PAD rows, the filler sequence, surplus rows, ghosts) poisoned with NaN and Inf.  The state lives between guard
words that must keep their bits."""
import numpy as np
import pytest
import torch

import actlog_reference as R

pytestmark = pytest.mark.gpu

RR = R.ROWS
GUARD, G = 0x7FC0BEEF, 64
NAN, INF = float("nan"), float("inf")
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratio():
    yield
    print(f"\nactivation log kernels: worst sumsq error / bound {WORST['ratio']:.3f}")


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return torch.cuda.current_stream().cuda_stream


class State:
    """the log's device state in the layout of train.ActivationLog (counters | window | counts | ring, and partial), each between
    guards"""

    def __init__(self, S=2, capacity=4, chunk_cap=4, every=1):
        from hri_emo_amd.train import ActivationLog as L
        self.S, self.cap, self.chunk_cap, self.every = S, capacity, chunk_cap, every
        self.ring_at = L.HEADER + (2 * S + 3) // 4 * 4
        self.rw = L.REC_HEADER + 2 * S * L.ENTRY
        n = self.ring_at + capacity * self.rw
        self.buf = torch.full((G + n + G,), GUARD, dtype=torch.int32, device="cuda")
        self.small = self.buf[G:G + n]
        self.small.zero_()
        self.counters, self.window = self.small[:4], self.small[4:8]
        self.counts, self.ring = self.small[8:8 + 2 * S], self.small[self.ring_at:]
        pn = 2 * S * chunk_cap * 8
        self.pbuf = torch.full((G + pn + G,), GUARD, dtype=torch.int32, device="cuda")
        self.partial = self.pbuf[G:G + pn].view(torch.float32)
        self.pbuf[G:G + pn] = 0

    def plan(self, record=1):
        from hri_emo_amd import _lib
        _lib.call("hriemo_act_log_plan", record, self.every, self.cap, self.S, P(self.counters), P(self.window), P(self.counts),
                  P(self.ring), ST())

    def probe(self, x, n_rows, d, ld, B, L, cu=None, kpm=None, n_valid=None, site=0, half=0):
        from hri_emo_amd import _lib
        _lib.call("hriemo_act_probe", P(x), 0 if x.dtype == torch.bfloat16 else 1, n_rows, d, ld, P(cu), P(kpm), B, L, P(n_valid),
                  P(self.window), site, half, self.S, self.chunk_cap, P(self.partial), P(self.counts), ST())

    def fold(self, half=0):
        from hri_emo_amd import _lib
        _lib.call("hriemo_act_log_fold", P(self.partial), P(self.counts), P(self.window), half, self.S, self.chunk_cap, self.cap,
                  P(self.ring), ST())

    def arrays(self):
        from hri_emo_amd.train import ActivationLog as L
        return L.decode(self.small.cpu().numpy(), [f"s{i}" for i in range(self.S)], [1] * self.S, self.cap)

    def entry(self, half=0, site=0, record=-1):
        f = self.arrays()[("forward", "gradient")[half]]
        return {k: f[k][record, site] for k in ("have", "n_rows", "n_bad", "first_bad_row", "absmax", "sumsq")}

    def guards_intact(self):
        n, pn = self.small.numel(), self.partial.numel()
        for b, m in ((self.buf, n), (self.pbuf, pn)):
            assert bool((b[:G] == GUARD).all()) and bool((b[G + m:] == GUARD).all()), "a guard word was written"


def strided(n_rows, d, dtype, seed, scale=1.0):
    """randn rows [n_rows, d] inside a buffer of leading dimension d + 8 whose columns between the rows hold NaN -> (buffer, view)"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((n_rows, d + 8), NAN, dtype=dtype)
    buf[:, :d] = (torch.randn(n_rows, d, generator=g) * scale).to(dtype)
    buf = buf.cuda()
    return buf, buf[:, :d]


def run_and_check(st, buf, x, B, L, what, cu=None, kpm=None, n_valid=None, site=0, half=0):
    """plan + probe + fold of one buffer; the entry against the reference"""
    n_rows, d = x.shape
    ld = buf.shape[1]
    R.assert_no_underflow(x)
    cu_d = None if cu is None else torch.tensor(cu, dtype=torch.int32, device="cuda")
    kpm_d = None if kpm is None else torch.as_tensor(np.asarray(kpm), dtype=torch.uint8).cuda().contiguous()
    nv_d = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device="cuda")
    st.plan()
    st.probe(buf, n_rows, d, ld, B, L, cu_d, kpm_d, nv_d, site, half)
    st.fold(half)
    torch.cuda.synchronize()
    ref = R.probe_ref64(x, B, L, cu, kpm, n_valid)
    ratio = R.check_entry(st.entry(half, site), ref, n_rows, d, R.vec_of(x.dtype, d, ld), what)
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: n_rows {ref['n_rows']} n_bad {ref['n_bad']} first {ref['first_bad_row']} sumsq err/bound {ratio:.3f}")
    st.guards_intact()
    return ref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [8, 64, 776])
def test_every_row_counts_at_the_chunk_edges(dtype, d):
    st = State()
    for n_rows in (1, RR - 1, RR, RR + 1, 2 * RR + 1):
        for variant in ("clean", "nan first row", "nan last row + inf last column", "zeros"):
            buf, x = strided(n_rows, d, dtype, seed=n_rows * 7 + d)
            if variant == "nan first row":
                x[0, d // 2] = NAN
            elif variant == "nan last row + inf last column":
                x[n_rows - 1, 0] = NAN
                x[n_rows // 2, d - 1] = -INF
            elif variant == "zeros":
                x.zero_()
            ref = run_and_check(st, buf, x, n_rows, 1, f"{variant} n_rows={n_rows} d={d}")
            assert ref["n_rows"] == n_rows
            if variant == "zeros":
                assert ref["sumsq"] == 0.0 and ref["absmax"] == 0.0 and ref["n_bad"] == 0
            if variant == "nan last row + inf last column":
                assert ref["n_bad"] == 2 and ref["first_bad_row"] == n_rows // 2


@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 4), (torch.bfloat16, 12), (torch.float32, 4), (torch.float32, 6)],
                         ids=["bf16-4", "bf16-12", "fp32-4", "fp32-6"])
def test_widths_that_are_no_vector_multiple(dtype, d):
    """the logits [B, N_e] are the narrow case of the model (fp32, d = 4: one vector); anything else goes element by element"""
    st = State()
    for n_rows in (1, RR + 1):
        buf, x = strided(n_rows, d, dtype, seed=d)
        x[n_rows - 1, d - 1] = INF
        run_and_check(st, buf, x, n_rows, 1, f"narrow n_rows={n_rows} d={d}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_padded_rows_with_masks(dtype):
    B, L, d = 3, 23, 64                      # 69 rows: three chunks, samples that straddle them
    st = State()
    prefix = np.arange(L)[None, :] >= np.array([23, 5, 1])[:, None]
    rng = np.random.RandomState(3)
    holes = rng.rand(B, L) < 0.5             # not a prefix
    holes[:, 0], holes[2, :] = True, True
    holes[2, L - 1] = False                  # sample 2: its only row is the last one
    for name, kpm in (("prefix", prefix), ("no prefix", holes)):
        buf, x = strided(B * L, d, dtype, seed=11)
        pad = torch.from_numpy(kpm.reshape(-1)).cuda()
        x[pad] = NAN                         # PAD rows may hold anything
        x[pad, 1] = INF
        ref = run_and_check(st, buf, x, B, L, f"padded {name} clean", kpm=kpm)
        assert ref["n_bad"] == 0 and ref["n_rows"] == int((~kpm).sum())
        keep = np.flatnonzero(~kpm.reshape(-1))
        x[keep[0], 0] = NAN                  # the first and the last row that count, and one in between in another chunk
        x[keep[-1], d - 1] = INF
        x[keep[len(keep) // 2], 3] = -INF
        ref = run_and_check(st, buf, x, B, L, f"padded {name} bad", kpm=kpm)
        assert ref["n_bad"] == 3 and ref["first_bad_row"] == keep[0]
        x[keep[0], 0] = 1.0                  # the minimum now comes from a later chunk
        ref = run_and_check(st, buf, x, B, L, f"padded {name} bad later", kpm=kpm)
        assert ref["first_bad_row"] == keep[len(keep) // 2]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_packed_rows_with_filler_surplus_and_ghosts(dtype):
    L, d = RR, 64
    lens, filler, surplus = (1, RR, 3), 7, 5
    cu = [0, 1, 1 + RR, 4 + RR, 4 + RR + filler]                 # B = 3 real sequences, then the filler sequence of a bucket plan
    n_rows = cu[-1] + surplus
    st = State()
    buf, x = strided(n_rows, d, dtype, seed=5)
    x[cu[3]:] = NAN                                              # filler and surplus rows may hold anything
    x[cu[3]:, d - 1] = INF
    ref = run_and_check(st, buf, x, 3, L, "packed clean", cu=cu)
    assert ref["n_rows"] == sum(lens) and ref["n_bad"] == 0
    # bad rows in two chunks: sequence 1 spans rows 1 .. 32, so its last row lies in the second chunk
    x[cu[2] - 1, 5] = NAN
    x[cu[3] - 1, d - 1] = INF                                    # the last row that counts, last column
    ref = run_and_check(st, buf, x, 3, L, "packed bad in chunk 1", cu=cu)
    assert ref["n_bad"] == 2 and ref["first_bad_row"] == 1 * L + (RR - 1)
    x[0, 0] = NAN                                                # the first row that counts
    x[3, 2] = INF
    ref = run_and_check(st, buf, x, 3, L, "packed bad in both chunks", cu=cu)
    assert ref["n_bad"] == 4 and ref["first_bad_row"] == 0
    # n_valid below B: the ghosts are poisoned and must not count; 0 and 9 clamp into [1, B]
    buf, x = strided(n_rows, d, dtype, seed=6)
    x[cu[2]:] = NAN
    ref = run_and_check(st, buf, x, 3, L, "packed n_valid=2", cu=cu, n_valid=2)
    assert ref["n_rows"] == 1 + RR and ref["n_bad"] == 0
    x[cu[1]:] = INF
    ref = run_and_check(st, buf, x, 3, L, "packed n_valid=0", cu=cu, n_valid=0)
    assert ref["n_rows"] == 1 and ref["n_bad"] == 0
    ref = run_and_check(st, buf, x, 3, L, "packed n_valid=9", cu=cu, n_valid=9)
    assert ref["n_rows"] == sum(lens) and ref["n_bad"] == (RR + 3) * d
    # padded with ghosts
    buf, x = strided(3 * 5, d, dtype, seed=7)
    x[5:] = NAN
    ref = run_and_check(st, buf, x, 3, 5, "padded n_valid=1", n_valid=1)
    assert ref["n_rows"] == 5 and ref["n_bad"] == 0


def test_sites_and_halves_keep_apart_and_absent_sites_stay_absent():
    st = State(S=3, capacity=2, chunk_cap=3)
    buf0, x0 = strided(RR + 1, 64, torch.bfloat16, seed=1)
    buf2, x2 = strided(5, 8, torch.float32, seed=2)
    x2[4, 7] = NAN
    st.plan()
    st.probe(buf0, RR + 1, 64, 72, RR + 1, 1, site=0, half=0)
    st.probe(buf2, 5, 8, 16, 5, 1, site=2, half=0)
    st.probe(buf2, 5, 8, 16, 5, 1, site=0, half=1)
    st.fold(0)
    arr = st.arrays()
    assert arr["halves"].tolist() == [1] and arr["gradient"]["have"][0].tolist() == [0, 0, 0]      # the gradient half is not folded yet
    st.fold(1)
    torch.cuda.synchronize()
    arr = st.arrays()
    assert arr["pass"].tolist() == [0] and arr["halves"].tolist() == [3]
    assert arr["forward"]["have"][0].tolist() == [1, 0, 1] and arr["gradient"]["have"][0].tolist() == [1, 0, 0]
    R.check_entry(st.entry(0, 0), R.probe_ref64(x0, RR + 1, 1), RR + 1, 64, 8, "site 0 forward")
    R.check_entry(st.entry(0, 2), R.probe_ref64(x2, 5, 1), 5, 8, 4, "site 2 forward")
    R.check_entry(st.entry(1, 0), R.probe_ref64(x2, 5, 1), 5, 8, 4, "site 0 gradient")
    assert st.entry(1, 0)["first_bad_row"] == 4
    st.guards_intact()


def test_closed_window_leaves_every_byte_and_a_rerun_gives_the_same_bits():
    st = State()
    buf, x = strided(2 * RR + 1, 776, torch.bfloat16, seed=9)
    x[40, 3] = NAN
    run_and_check(st, buf, x, 2 * RR + 1, 1, "first run")
    first_small, first_part = st.buf.clone(), st.pbuf.clone()
    # a warm-up pass: the closed window and nothing else; probe and fold exit
    st.pbuf[G:-G] = GUARD                                         # anything a stray store would change
    st.plan(record=0)
    st.probe(buf, 2 * RR + 1, 776, 784, 2 * RR + 1, 1)
    st.fold(0)
    torch.cuda.synchronize()
    want = first_small.clone()
    want[G + 4:G + 8] = 0
    assert torch.equal(st.buf, want), "a pass under the closed window changed counters, counts or the ring"
    assert bool((st.pbuf == GUARD).all()), "a probe under the closed window stored a partial"
    # the same pass again, into the next slot: the same bits
    st.pbuf[G:-G] = 0
    run_and_check(st, buf, x, 2 * RR + 1, 1, "second run")
    assert torch.equal(st.pbuf, first_part)
    ring = st.ring.view(st.cap, st.rw)
    assert torch.equal(ring[0, 1:], ring[1, 1:]) and ring[0, 0].item() == 0 and ring[1, 0].item() == 1
    assert st.counters.tolist() == [2, 2, 0, 0]


def test_ring_wraps_at_capacity_and_every_third_pass_records():
    st = State(capacity=3)
    buf, x = strided(3, 8, torch.float32, seed=4)
    for p in range(5):
        x[:, 0] = float(p + 1)
        st.plan()
        st.probe(buf, 3, 8, 16, 3, 1)
        st.fold(0)
    torch.cuda.synchronize()
    arr = st.arrays()
    assert arr["n_passes"] == 5 and arr["n_recorded"] == 5 and arr["pass"].tolist() == [2, 3, 4]
    assert arr["forward"]["absmax"][:, 0].tolist() == [max(3.0, float(x[:, 1:].abs().max())), max(4.0, float(x[:, 1:].abs().max())),
                                                       max(5.0, float(x[:, 1:].abs().max()))]
    st.guards_intact()
    st = State(capacity=4, every=3)
    for p in range(8):
        x[:, 0] = 100.0 + p
        st.plan()
        st.probe(buf, 3, 8, 16, 3, 1)
        st.fold(0)
    st.plan(record=0)                                            # a warm-up pass in between counts nothing
    torch.cuda.synchronize()
    arr = st.arrays()
    assert arr["n_passes"] == 8 and arr["n_recorded"] == 3 and arr["pass"].tolist() == [0, 3, 6]
    assert arr["forward"]["absmax"][:, 0].tolist() == [100.0, 103.0, 106.0]
    st.guards_intact()


