"""CPU suite of the ragged front door of the captured step: the shared bucket-row helper against the formula of capture()'s
docstring and against packed_tables, the new C-ABI entry in the header, the library and the binding, and the ragged mode of
data.DevicePrefetcher on a CPU device."""
import ctypes
import os
import random
import re

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _formula(n, B, L, buckets):
    """capture()'s docstring, worked out independently: the packed row count is rounded up to a multiple of 1/`buckets` of the padded
    rows (a multiple of 8 rows, at least 8, at most one sequence), and the surplus rows form one extra sequence that is never
    empty: the smallest multiple of the granule that is GREATER than n"""
    g = (B * L) // buckets
    g -= g % 8
    g = min(max(g, 8), L)
    rows = n + 1
    while rows % g:
        rows += 1
    return rows


def test_bucket_rows_is_the_arithmetic_of_packed_key():
    from hri_emo_amd import dp
    rnd = random.Random(7)
    for trial in range(300):
        B = rnd.choice([1, 2, 5, 8, 64])
        La = rnd.choice([3, 8, 37, 70, 400, 1000])
        Lt = rnd.randint(1, La)
        la = [rnd.randint(1, La) for _ in range(B)]
        lt = [rnd.randint(1, Lt) for _ in range(B)]
        if trial % 10 == 0:
            la, lt = [La] * B, [Lt] * B                          # all full: the surplus sequence lies past B * L
        if trial % 10 == 1:
            la, lt = [1] * B, [1] * B
        want = (_formula(sum(la), B, La, dp._VARLEN_BUCKETS), _formula(sum(lt), B, Lt, dp._VARLEN_BUCKETS))
        assert (dp.bucket_rows(sum(la), B, La), dp.bucket_rows(sum(lt), B, Lt)) == want, (B, La, Lt, la, lt)
        key, cu_a, cu_t, cu_f = dp.packed_tables(*dp.mask_lengths(None, None, (la, lt), B, La, Lt), B, La, Lt)
        assert key == want
        assert cu_a[-1] == want[0] and cu_t[-1] == want[1] and cu_f[-1] == want[1]
        for n, rows, L in ((sum(la), want[0], La), (sum(lt), want[1], Lt)):
            assert n < rows and rows - n <= L
        # the static row sources of capture_packed are as long as the largest bucket: every batch's bucket fits
        assert dp.bucket_rows(B * La, B, La) >= want[0] and dp.bucket_rows(B * Lt, B, Lt) >= want[1]


def test_packed_tables_against_brute_force_prefix_sums():
    from hri_emo_amd import dp
    cases = [([5], [3], 1, 9, 4),                                    # B = 1
             ([1, 1, 1, 1], [1, 1, 1, 1], 4, 96, 40),                # every length 1
             ([96] * 4, [40] * 4, 4, 96, 40),                        # every length L: the full batch still gets its surplus sequence
             ([7, 96, 1, 33], [40, 2, 1, 17], 4, 96, 40),
             ([3, 400, 250, 1, 399, 17, 64, 128], [128, 1, 77, 5, 9, 100, 64, 2], 8, 400, 128)]
    for la, lt, B, La, Lt in cases:
        key, cu_a, cu_t, cu_f = dp.packed_tables(la, lt, B, La, Lt)
        assert key == (_formula(sum(la), B, La, dp._VARLEN_BUCKETS), _formula(sum(lt), B, Lt, dp._VARLEN_BUCKETS))
        for cu, lens, rows in ((cu_a, la, key[0]), (cu_t, lt, key[1]), (cu_f, [min(a, t) for a, t in zip(la, lt)], key[1])):
            assert type(cu) is list and len(cu) == B + 2
            assert cu[:B + 1] == [sum(lens[:i]) for i in range(B + 1)] and cu[B + 1] == rows
            assert cu[B] < cu[B + 1], "the surplus sequence is never empty"
        assert key[0] - cu_a[B] <= La and key[1] - cu_t[B] <= Lt, "and never longer than one padded sequence"
        assert dp.ghost_plan(la, lt, B, La, Lt)[2] == key, "a full batch: ghost_plan's key is this key"
    assert dp.packed_tables([96] * 4, [40] * 4, 4, 96, 40)[0] == (dp.bucket_rows(4 * 96, 4, 96), dp.bucket_rows(4 * 40, 4, 40))


def test_state_classes_need_no_gpu():
    from hri_emo_amd import dp
    lens = dp._HostBlock([[1] * 3] * 2, "cpu")
    assert lens.dev.tolist() == lens.host.tolist() == [[1, 1, 1], [1, 1, 1]] and lens.dev.dtype == lens.host.dtype == torch.int32
    masks = tuple(torch.ones(3, L, dtype=torch.uint8) for L in (9, 4, 4))
    front = dp._RaggedFront(lens, masks, same_width=True, partial=True, accum=2, ctl=dp._HostBlock(dp.ctl_words(3, 1, 1), "cpu"))
    assert front.ctl.dev.tolist() == [3, 1, 1, 0] and (front.partial, front.accum) == (True, 2)
    assert all(b.dtype == torch.bool and b.data_ptr() == m.data_ptr() for b, m in zip(front.bool, masks))
    pb = dp._PackedState(3, 9, 4, "cpu", front)
    assert pb["graphs"] is pb.graphs and len(pb["graphs"]) == 0 and pb.pool is None and pb.front is front
    assert [t.tolist() for t in (pb.cu_a, pb.cu_t, pb.cu_f)] == [[0] * 5] * 3 and pb.cu_a.data_ptr() != pb.cu_t.data_ptr()
    assert dp._PackedState(3, 9, 4, "cpu").front is None
    rec = dp._GraphRecord(object(), torch.zeros(()), [])
    pb.graphs[(16, 8)] = rec
    assert pb["graphs"][(16, 8)] is rec and rec.seqs is None
    s = object.__new__(dp.DataParallelStep)
    s._record, s._pb, s._replay = None, None, True
    assert not s.captured and not s._replaying
    s._pb = pb
    assert s.captured and s._replaying
    s._record, s._pb = rec, None
    assert s.captured


def test_seq_tables_in_header_library_and_binding():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hriemo.h")).read(), flags=re.S)
    m = re.search(r"int\s+hriemo_seq_tables\s*\(([^)]*)\)\s*;", hdr)
    assert m, "hriemo_seq_tables is not declared in include/hriemo.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 14 and args[-1].startswith("hriemo_stream_t")
    codes = "".join("p" if ("*" in a or "hriemo_stream_t" in a) else "i" for a in args)
    assert all(("*" in a) or a.startswith("int ") or "hriemo_stream_t" in a for a in args)
    assert _lib._SIGS["hriemo_seq_tables"] == (codes, "i") and codes == "ppiiiiippppppp"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hriemo_seq_tables"), "declared but not exported"
    from hri_emo_amd import _ops, dp
    assert callable(_ops.seq_tables) and hasattr(dp.DataParallelStep, "capture_packed") and hasattr(dp.DataParallelStep, "step_packed")


def test_prefetcher_ragged_mode_passes_through_on_cpu():
    """on a CPU device the batches pass through unchanged, ragged entries and host-side lengths included"""
    from hri_emo_amd.data import DevicePrefetcher, collate_seq_packed
    g = torch.Generator().manual_seed(2)
    samples = []
    for n_a, n_t in ((5, 3), (9, 9), (2, 1), (7, 4), (3, 1), (8, 2)):
        samples.append((torch.randn(n_a, 16, generator=g), torch.zeros(n_a, dtype=torch.bool), torch.randn(n_t, 16, generator=g),
                        torch.zeros(n_t, dtype=torch.bool), (torch.rand(4, generator=g) < 0.3).float()))
    loader = [collate_seq_packed(samples[i:i + 2]) for i in range(0, 6, 2)]
    assert len({b[0].shape[0] for b in loader}) == 3
    convert = lambda b: (b[0], b[1].tolist(), b[2], b[3].tolist(), b[4])       # noqa: E731
    out = list(DevicePrefetcher(loader, "cpu", convert=convert, ragged={0: 18, 2: 18}))
    assert len(out) == 3
    for got, ref in zip(out, loader):
        assert got[0] is ref[0] and got[2] is ref[2] and got[4] is ref[4]
        assert got[1] == ref[1].tolist() and got[3] == ref[3].tolist()
