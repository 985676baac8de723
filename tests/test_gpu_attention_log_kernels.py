"""GPU suite of the attention log's kernels, through the C ABI: hriemo_attn_log_plan / _close, hriemo_attn_probs_varlen_log and its
fp32 twin hriemo_attn_probs_varlen_log_fp32, hriemo_attn_log_append.

The two export entries run the kernels of hriemo_attn_probs_varlen / _f32_varlen with one more pointer, so the check is exact: for
every window, slot slot0 + b of the log is torch.equal to probs[b] of the non-log entry on the same operands, and every other
byte of the log and of the poisoned guard rows around it keeps its bits (the log is pre-filled with one NaN pattern, the guards
with another, and all comparisons are made on the int32 view).  Operands: B = 5, H = 2, head widths 16 and 96, query lengths
(70, 1, 64, 65, 33), key lengths (40, 130, 1, 64, 128) -- the keys cross the 128-key block edge of the MFMA kernel -- maps
[72, 136], capacity 8.  The plan entry runs the batch sequences of tests/test_attention_log_host.py against that file's Python
model of the rule."""
import functools

import numpy as np
import pytest
import torch

from test_attention_log_host import SEQUENCES, fresh, lens_of, model_plan

pytestmark = pytest.mark.gpu

B, NH, LQ, LK, OUT, CAP = 5, 2, (70, 1, 64, 65, 33), (40, 130, 1, 64, 128), (72, 136), 8
LOG_NAN, GUARD_NAN = 0x7FC0DEAD, 0x7FC0BEEF          # two quiet-NaN payloads
#          {slot0, n_take}: the slots written
WINDOWS = {"{0, 5}": (0, 5), "{3, 5} exact fit": (3, 5), "{6, 2}": (6, 2), "{8, 0} full": (8, 0), "{0, 1}": (0, 1),
           "stale {6, 5}": (6, 5), "{-1, 3}": (-1, 3)}
ENTRY = {False: ("hriemo_attn_fwd_varlen", "hriemo_attn_probs_varlen"), True: ("hriemo_attn_fwd_f32_varlen", "hriemo_attn_probs_f32_varlen")}
LOG_ENTRY = {False: "hriemo_attn_probs_varlen_log", True: "hriemo_attn_probs_varlen_log_fp32"}


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return torch.cuda.current_stream().cuda_stream


def written(slot0, n_take, n=B):
    """the (sample, slot) pairs a window lets through"""
    return [(b, slot0 + b) for b in range(min(n_take, n)) if slot0 >= 0 and slot0 + b < CAP]


def test_the_windows_mean_what_the_issue_says():
    assert [s for _, s in written(6, 5)] == [6, 7] and written(-1, 3) == [] and written(8, 0) == []
    assert [s for _, s in written(3, 5)] == [3, 4, 5, 6, 7]


def guarded(elems):
    """(whole buffer as int32, the log [CAP, elems] as fp32 between two guard rows)"""
    buf = torch.full((CAP + 2, elems), GUARD_NAN, dtype=torch.int32, device="cuda")
    buf[1:CAP + 1] = LOG_NAN
    return buf, buf[1:CAP + 1].view(torch.float32)


def check(buf, ref, slot0, n_take, what):
    """slots of the window == ref[b] bit for bit, every other word of log and guards untouched"""
    want = torch.full_like(buf, GUARD_NAN)
    want[1:CAP + 1] = LOG_NAN
    pairs = written(slot0, n_take)
    for b, s in pairs:
        want[1 + s] = ref[b].reshape(-1).view(torch.int32)
    assert torch.equal(buf, want), (what, "slots written", [s for _, s in pairs],
                                    "words off", int((buf != want).sum()), "rows off", (buf != want).any(dim=1).nonzero().flatten().tolist())
    for b, s in pairs:
        assert torch.equal(buf[1 + s].view(torch.float32).view(ref[b].shape), ref[b]), (what, b, s)


@functools.lru_cache(maxsize=None)
def operands(f32, hd):
    """(Q, K, cu_q, cu_k, lse, probs of the non-log entry [B, 72, 136]): computed once per precision and head width"""
    from hri_emo_amd import _lib
    d = NH * hd
    dt = torch.float32 if f32 else torch.bfloat16
    g = torch.Generator().manual_seed(40 + hd)
    q = (torch.randn(sum(LQ), d, generator=g) * 1.5).to(dt).cuda()
    kv = torch.randn(sum(LK), 2 * d, generator=g).to(dt).cuda()
    K, V = kv[:, :d], kv[:, d:]
    cq = torch.tensor([0] + list(np.cumsum(LQ)), dtype=torch.int32, device="cuda")
    ck = torch.tensor([0] + list(np.cumsum(LK)), dtype=torch.int32, device="cuda")
    o = torch.empty((sum(LQ), d), dtype=dt, device="cuda")
    lse = torch.zeros((B, NH, max(LQ)), dtype=torch.float32, device="cuda")
    fwd, exp = ENTRY[f32]
    tail = (0.0, 0, None, 0, 0) + (() if f32 else (None,)) + (ST(),)
    _lib.call(fwd, P(q), q.stride(0), P(K), K.stride(0), P(V), V.stride(0), P(o), d, P(cq), P(ck), P(lse), B, NH, max(LQ), max(LK), hd, *tail)
    probs = torch.full((B,) + OUT, float("nan"), dtype=torch.float32, device="cuda")
    _lib.call(exp, P(q), q.stride(0), P(K), K.stride(0), P(cq), P(ck), P(lse), P(probs), B, NH, max(LQ), max(LK), OUT[0], OUT[1], hd,
              0.0, 0, None, 0, 0, ST())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(probs).any())
    return q, K, cq, ck, lse, probs


def export_log(f32, hd, log, window, capacity=CAP, n=B):
    from hri_emo_amd import _lib
    q, K, cq, ck, lse, _ = operands(f32, hd)
    fn = getattr(_lib.lib(), LOG_ENTRY[f32])
    return fn(P(q), q.stride(0), P(K), K.stride(0), P(cq), P(ck), P(lse), P(log), n, NH, max(LQ), max(LK), OUT[0], OUT[1], hd,
              0.0, 0, None, 0, 0, P(window), capacity, ST())


@pytest.mark.parametrize("hd", [16, 96])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_export_into_the_log_under_every_window(f32, hd):
    ref = operands(f32, hd)[5]
    for what, (slot0, n_take) in WINDOWS.items():
        buf, log = guarded(OUT[0] * OUT[1])
        window = torch.tensor([slot0, n_take, 0, 0], dtype=torch.int32, device="cuda")
        assert export_log(f32, hd, log, window) == 0, what
        torch.cuda.synchronize()
        check(buf, ref, slot0, n_take, (what, f32, hd))


@pytest.mark.parametrize("elems", [160, 259], ids=["N_e x L_t = 160", "259: past one chunk"])
def test_append_under_every_window(elems):
    from hri_emo_amd import _lib
    maps = torch.randn(B, elems, generator=torch.Generator().manual_seed(elems)).cuda()
    for what, (slot0, n_take) in WINDOWS.items():
        buf, log = guarded(elems)
        window = torch.tensor([slot0, n_take, 0, 0], dtype=torch.int32, device="cuda")
        _lib.call("hriemo_attn_log_append", P(maps), B, elems, P(window), P(log), CAP, ST())
        torch.cuda.synchronize()
        check(buf, maps, slot0, n_take, (what, elems))


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_plan_against_the_python_model(name):
    """the batch sequences of the host test: counters, window and logged lengths after every launch; the lengths sit between
    guard words; the close entry leaves everything but the window untouched"""
    from hri_emo_amd import _lib
    capacity, seq = SEQUENCES[name]
    state = fresh(capacity)
    small = torch.full((2 + 8 + 2 * capacity + 2,), GUARD_NAN, dtype=torch.int32, device="cuda")
    counters, window, lengths = small[2:6], small[6:10], small[10:10 + 2 * capacity].view(2, capacity)
    counters.zero_(); window.fill_(-7); lengths.zero_()
    for i, (nB, nv) in enumerate(seq):
        lens = lens_of(nB, 100 + i)
        dev = lens.cuda()
        word = None if nv is None else torch.tensor([nv], dtype=torch.int32, device="cuda")
        _lib.call("hriemo_attn_log_plan", P(dev), P(word), nB, capacity, P(counters), P(window), P(lengths), ST())
        win = model_plan(state, capacity, nB, nv, lens.numpy())
        assert window.tolist() == [win[0], win[1], 0, 0], (name, i, window.tolist(), win)
        assert counters.tolist() == [state["cursor"], state["n_offered"], state["n_batches"], 0], (name, i, counters.tolist())
        assert np.array_equal(lengths.cpu().numpy(), state["lengths"]), (name, i)
    before = small.clone()
    _lib.call("hriemo_attn_log_close", P(window), ST())
    assert window.tolist() == [0, 0, 0, 0]
    after = small.clone()
    after[6:10] = before[6:10]
    assert torch.equal(after, before), "the closed window touched something else"
    assert small[:2].tolist() == [GUARD_NAN] * 2 and small[-2:].tolist() == [GUARD_NAN] * 2


@pytest.mark.parametrize("cursor", [-1, CAP + 1], ids=["-1", "capacity + 1"])
def test_plan_with_a_corrupt_cursor_takes_nothing(cursor):
    from hri_emo_amd import _lib
    counters = torch.tensor([cursor, 4, 2, 0], dtype=torch.int32, device="cuda")
    window = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    lengths = torch.full((2, CAP), 99, dtype=torch.int32, device="cuda")
    lens = lens_of(5, 3).cuda()
    _lib.call("hriemo_attn_log_plan", P(lens), None, 5, CAP, P(counters), P(window), P(lengths), ST())
    assert window.tolist() == [cursor, 0, 0, 0] and counters.tolist() == [cursor, 9, 3, 0]
    assert bool((lengths == 99).all())
    # and no export or append under that window writes anything
    buf, log = guarded(160)
    maps = torch.ones(B, 160, device="cuda")
    _lib.call("hriemo_attn_log_append", P(maps), B, 160, P(window), P(log), CAP, ST())
    torch.cuda.synchronize()
    check(buf, maps, cursor, 0, "corrupt cursor")


def test_plan_without_a_lengths_block():
    from hri_emo_amd import _lib
    counters = torch.zeros(4, dtype=torch.int32, device="cuda")
    window = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.call("hriemo_attn_log_plan", None, None, 5, CAP, P(counters), P(window), None, ST())
    _lib.call("hriemo_attn_log_plan", None, None, 5, CAP, P(counters), P(window), None, ST())
    assert window.tolist() == [5, 3, 0, 0] and counters.tolist() == [8, 10, 2, 0]


def test_refusals_launch_nothing():
    from hri_emo_amd import _lib
    L = _lib.lib()
    counters = torch.tensor([2, 2, 1, 0], dtype=torch.int32, device="cuda")
    window = torch.tensor([0, 5, 0, 0], dtype=torch.int32, device="cuda")
    lengths = torch.full((2, CAP), 99, dtype=torch.int32, device="cuda")
    lens = lens_of(5, 3).cuda()
    buf, log = guarded(OUT[0] * OUT[1])
    maps = torch.ones(B, OUT[0] * OUT[1], device="cuda")
    st = ST()
    plan = dict(lens=P(lens), nv=None, B=5, cap=CAP, ctr=P(counters), win=P(window), lengths=P(lengths))
    for what, change in {"B 0": dict(B=0), "capacity 0": dict(cap=0), "no counters": dict(ctr=None), "no window": dict(win=None),
                         "lens without lengths": dict(lengths=None), "lengths without lens": dict(lens=None),
                         "misaligned counters": dict(ctr=P(counters) + 2), "misaligned window": dict(win=P(window) + 1),
                         "misaligned n_valid": dict(nv=P(counters) + 1)}.items():
        a = dict(plan, **change)
        assert L.hriemo_attn_log_plan(a["lens"], a["nv"], a["B"], a["cap"], a["ctr"], a["win"], a["lengths"], st) != 0, what
        assert L.hriemo_last_error().decode() != "", what
    assert L.hriemo_attn_log_close(None, st) != 0 and L.hriemo_attn_log_close(P(window) + 2, st) != 0
    app = dict(maps=P(maps), B=B, elems=OUT[0] * OUT[1], win=P(window), log=P(log), cap=CAP)
    for what, change in {"B 0": dict(B=0), "B past the grid": dict(B=65536), "no elements": dict(elems=0), "capacity 0": dict(cap=0),
                         "no maps": dict(maps=None), "no window": dict(win=None), "no log": dict(log=None),
                         "misaligned log": dict(log=P(log) + 2), "misaligned window": dict(win=P(window) + 2)}.items():
        a = dict(app, **change)
        assert L.hriemo_attn_log_append(a["maps"], a["B"], a["elems"], a["win"], a["log"], a["cap"], st) != 0, what
        assert L.hriemo_last_error().decode() != "", what
    for f32 in (False, True):
        q, K, cq, ck, lse, _ = operands(f32, 16)
        fn = getattr(L, LOG_ENTRY[f32])
        good = dict(Q=P(q), K=P(K), cq=P(cq), lse=P(lse), log=P(log), B=B, olk=OUT[1], hd=16, win=P(window), cap=CAP)
        for what, change in {"no window": dict(win=None), "misaligned window": dict(win=P(window) + 2), "capacity 0": dict(cap=0),
                             "capacity -1": dict(cap=-1), "no log": dict(log=None), "B 0": dict(B=0), "head width not built": dict(hd=48),
                             "map narrower than the longest key sequence": dict(olk=100), "cu_seqlens_q missing": dict(cq=None),
                             "no lse": dict(lse=None)}.items():
            a = dict(good, **change)
            rc = fn(a["Q"], q.stride(0), a["K"], K.stride(0), a["cq"], P(ck), a["lse"], a["log"], a["B"], NH, max(LQ), max(LK), OUT[0],
                    a["olk"], a["hd"], 0.0, 0, None, 0, 0, a["win"], a["cap"], st)
            assert rc != 0, (f32, what)
            assert L.hriemo_last_error().decode() != "", (f32, what)
    torch.cuda.synchronize()
    assert counters.tolist() == [2, 2, 1, 0] and window.tolist() == [0, 5, 0, 0] and bool((lengths == 99).all())
    check(buf, maps, 0, 0, "a refused call launched")
