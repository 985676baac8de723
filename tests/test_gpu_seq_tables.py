"""GPU suite of hriemo_seq_tables, through the C ABI: the lengths of a ragged batch (int32, device) -> the three cu_seqlens arrays
and the three dense key-padding masks of a packed step, from ONE launch.  Everything is an integer, so every comparison with the
numpy reference is array_equal.  Every output is a dense payload inside a 0xFF-filled allocation with guard regions on both sides
(the mask row stride is the payload exactly: the masks are dense); the guards are compared afterwards, and the mask payloads start
at every byte alignment in turn."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                      # bytes on either side of every payload
OUTS = ("cu_a", "cu_t", "cu_f", "mask_a", "mask_t", "mask_f")


def ST():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """`n` elements of int32 / uint8 at byte offset GUARD + shift of a 0xFF-filled allocation, GUARD bytes and more behind them"""

    def __init__(self, n, item, shift=0):
        self.n, self.item, self.lo = n, item, GUARD + shift
        self.raw = torch.full((self.lo + n * item + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.ptr = self.raw.data_ptr() + self.lo

    def payload(self):
        by = self.raw.cpu().numpy()[self.lo:self.lo + self.n * self.item]
        return by.view(np.int32) if self.item == 4 else by

    def intact(self):
        by = self.raw.cpu().numpy()
        return bool((by[:self.lo] == 0xFF).all() and (by[self.lo + self.n * self.item:] == 0xFF).all())

    def untouched(self):
        return bool((self.raw == 0xFF).all())


def _reference(la, lt, B, La, Lt, rows_a, rows_t):
    la, lt = np.clip(np.asarray(la, np.int64), 1, La), np.clip(np.asarray(lt, np.int64), 1, Lt)
    lf = np.minimum(la, lt)
    cu = lambda ls, n: np.concatenate([[0], np.cumsum(ls), [n]]).astype(np.int32)       # noqa: E731
    mask = lambda ls, L: (np.arange(L)[None, :] >= ls[:, None]).astype(np.uint8).reshape(-1)       # noqa: E731
    return {"cu_a": cu(la, rows_a), "cu_t": cu(lt, rows_t), "cu_f": cu(lf, rows_t),
            "mask_a": mask(la, La), "mask_t": mask(lt, Lt), "mask_f": mask(lf, Lt)}


def _launch(la, lt, B, La, Lt, rows_a, rows_t, want=OUTS, shift=0, raw=False, null_lengths=None):
    """-> (return code | None, {name: Guarded})"""
    from hri_emo_amd import _lib
    lens = torch.tensor([list(la), list(lt)], dtype=torch.int32).cuda()
    sizes = {"cu_a": (B + 2, 4), "cu_t": (B + 2, 4), "cu_f": (B + 2, 4), "mask_a": (B * La, 1), "mask_t": (B * Lt, 1), "mask_f": (B * Lt, 1)}
    out = {k: Guarded(max(sizes[k][0], 1), sizes[k][1], shift if sizes[k][1] == 1 else 0) for k in want}
    ptr = lambda k: out[k].ptr if k in out else None       # noqa: E731
    pa = None if null_lengths == "a" else lens[0].data_ptr()
    pt = None if null_lengths == "t" else lens[1].data_ptr()
    args = (pa, pt, B, La, Lt, rows_a, rows_t) + tuple(ptr(k) for k in OUTS) + (ST(),)
    if raw:
        rc = _lib.lib().hriemo_seq_tables(*args)
    else:
        rc = _lib.call("hriemo_seq_tables", *args)
    torch.cuda.synchronize()
    return rc, out


def _lengths(B, La, Lt, seed):
    g = np.random.default_rng(seed)
    la, lt = g.integers(1, La + 1, B), g.integers(1, Lt + 1, B)
    la[0], lt[0] = La, 1                         # the extremes are always in: a full and a one-row sequence per modality
    la[-1], lt[-1] = 1, Lt
    return la.tolist(), lt.tolist()


def _check(la, lt, B, La, Lt, rows_a, rows_t, want=OUTS, shift=0):
    _, out = _launch(la, lt, B, La, Lt, rows_a, rows_t, want, shift)
    ref = _reference(la, lt, B, La, Lt, rows_a, rows_t)
    for k in want:
        got = out[k].payload()
        assert np.array_equal(got, ref[k]), (k, B, La, Lt, shift, np.flatnonzero(got != ref[k])[:8])
        assert out[k].intact(), f"{k}: a guard byte was written (B={B} La={La} Lt={Lt} shift={shift})"
    for k, n in (("cu_a", rows_a), ("cu_t", rows_t), ("cu_f", rows_t)):
        if k in want:
            assert int(out[k].payload()[B + 1]) == n and int(out[k].payload()[0]) == 0
    return out


SHAPES = [
    pytest.param(1, 7, 3, id="B1"),
    pytest.param(64, 9, 5, id="B64: one full wave"),
    pytest.param(65, 9, 5, id="B65: carry across a wave"),
    pytest.param(70, 9, 5, id="B70"),
    pytest.param(300, 9, 5, id="B300: a second trip of the scan loop"),
    pytest.param(1100, 3, 2, id="B1100: five trips"),
]


@pytest.mark.parametrize("B,La,Lt", SHAPES)
def test_tables_equal_the_numpy_reference(B, La, Lt):
    """all six outputs from one launch, two launches bit-identical"""
    la, lt = _lengths(B, La, Lt, B)
    rows_a, rows_t = sum(la) + 3, sum(lt) + 1
    a = _check(la, lt, B, La, Lt, rows_a, rows_t)
    b = _check(la, lt, B, La, Lt, rows_a, rows_t)
    for k in OUTS:
        assert np.array_equal(a[k].payload(), b[k].payload())


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_odd_widths_and_both_minima(shift):
    """B = 5, La = 37, Lt = 23: rows that start at every byte alignment (the 32-bit stores' head and tail), lengths 1 and L, and
    la < lt / la > lt pairs for the fused minimum; the mask payloads themselves start `shift` bytes off a 16-byte boundary"""
    B, La, Lt = 5, 37, 23
    la, lt = [37, 1, 5, 23, 12], [23, 23, 1, 9, 20]
    assert any(x < y for x, y in zip(la, lt)) and any(x > y for x, y in zip(la, lt))
    _check(la, lt, B, La, Lt, 80, 88, shift=shift)


def test_each_output_alone_and_in_pairs():
    """every NULL combination that leaves at least one output: alone, in pairs, the three cu only, the three masks only"""
    B, La, Lt = 70, 9, 5
    la, lt = _lengths(B, La, Lt, 3)
    combos = [(k,) for k in OUTS] + list(itertools.combinations(OUTS, 2)) + [OUTS[:3], OUTS[3:]]
    for want in combos:
        _check(la, lt, B, La, Lt, sum(la) + 8, sum(lt) + 8, want=want, shift=1)


def test_lengths_are_clamped_for_memory_safety():
    """0, -3 and L + 3 behave as 1, 1 and L"""
    B, La, Lt = 4, 11, 6
    got = _check([0, -3, La + 3, 4], [Lt + 3, 0, -3, 2], B, La, Lt, 40, 24)
    same = _check([1, 1, La, 4], [Lt, 1, 1, 2], B, La, Lt, 40, 24)
    for k in OUTS:
        assert np.array_equal(got[k].payload(), same[k].payload())
    assert got["cu_a"].payload().tolist() == [0, 1, 2, 2 + La, 6 + La, 40]


@pytest.mark.parametrize("case", ["B=0", "La=0", "Lt=0", "Lt>La", "no lengths_a", "no lengths_t", "no output", "cu_a without rows",
                                  "cu_t without rows", "cu_f without rows", "negative rows"])
def test_refusals_launch_nothing(case):
    """every refusal of the header: non-zero, hriemo_last_error set, the poisoned outputs untouched"""
    from hri_emo_amd import _lib
    B, La, Lt, ra, rt, want, null = 5, 9, 5, 50, 30, OUTS, None
    if case == "B=0":
        B = 0
    elif case == "La=0":
        La = 0
    elif case == "Lt=0":
        Lt = 0
    elif case == "Lt>La":
        Lt = La + 1
    elif case.startswith("no lengths"):
        null = case[-1]
    elif case == "no output":
        want = ()
    elif case == "cu_a without rows":
        ra, want = 0, ("cu_a", "mask_t")
    elif case == "cu_t without rows":
        rt, want = 0, ("cu_t",)
    elif case == "cu_f without rows":
        rt, want = 0, ("cu_f", "mask_a")
    elif case == "negative rows":
        ra, want = -8, OUTS
    rc, out = _launch([3] * 5, [2] * 5, B, La, Lt, ra, rt, want, raw=True, null_lengths=null)
    assert rc != 0, case
    msg = _lib.lib().hriemo_last_error().decode()
    expect = ("bad shape" if case in ("B=0", "La=0", "Lt=0", "Lt>La") else "both length arrays" if null else "no output" if not want
              else "cu_a needs" if ra <= 0 else "cu_t / cu_f need")
    assert "seq_tables" in msg and expect in msg, (case, msg)
    for k in out:
        assert out[k].untouched(), f"{case}: {k} was written"
    # (row counts are not needed for outputs that do not carry them)
    if case == "cu_a without rows":
        _check([3] * 5, [2] * 5, 5, 9, 5, 0, 30, want=("cu_t", "mask_a"))


def test_wrapper_writes_the_trainer_buffers():
    """_ops.seq_tables on tensors: the [2, B] lengths block in, int32 / uint8 tensors out; a tensor of the wrong size is refused on
    the host"""
    from hri_emo_amd import _ops
    B, La, Lt = 5, 70, 40
    la, lt = [70, 33, 32, 1, 17], [40, 1, 32, 31, 16]
    lens = torch.tensor([la, lt], dtype=torch.int32).cuda()
    cu = tuple(torch.full((B + 2,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    masks = tuple(torch.full((B, L), 0xFF, dtype=torch.uint8, device="cuda") for L in (La, Lt, Lt))
    _ops.seq_tables(lens, La, Lt, rows=(160, 128), cu=cu, masks=masks)
    ref = _reference(la, lt, B, La, Lt, 160, 128)
    for t, k in zip(cu + masks, OUTS):
        assert np.array_equal(t.cpu().numpy().reshape(-1), ref[k]), k
    plans, (m_a, m_t) = _ops.plans_from_lengths(la, lt, La, Lt, lens.device)
    assert torch.equal(masks[0].view(torch.bool), m_a) and torch.equal(masks[1].view(torch.bool), m_t)
    assert torch.equal(masks[2].view(torch.bool), m_a[:, :Lt] | m_t)
    for c, p in zip(cu, plans):
        assert torch.equal(c[:B + 1], p.cu)
    with pytest.raises(ValueError, match="seq_tables"):
        _ops.seq_tables(lens, La, Lt, rows=(160, 128), cu=(cu[0][:B + 1], None, None))
    with pytest.raises(ValueError, match="seq_tables"):
        _ops.seq_tables(lens.long(), La, Lt, rows=(160, 128), cu=cu)
