"""GPU suite of hriemo_gather_rows, through the C ABI: rows of a device-resident store gathered by utterance id, compared BIT FOR
BIT (as bytes) with torch indexing.  Stores: the MOSEI widths in fp32 (74: 296-byte rows, utterance starts on 8-byte boundaries
only, and source and destination phases that differ from segment to segment; 300), 768 x bf16, 5 x fp16 (10-byte rows, shorter
than one 16-byte chunk), 8 x bf16 (a row is exactly one chunk) and a targets store with one 6 x fp32 row per utterance.  7
utterances of 1, 2, 17, 64, 3, 1, 40 rows; the store's bytes are random, NaN and Inf patterns included.  The destination is
pre-filled with 0xFF (NaN in every format) with one more such row on either side, inside guards of 0xA5: gathered rows equal the
reference, the rows from dst_cu[n] to dst_rows are exact zeros, an empty tail leaves the next row's poison, nothing outside the
destination changes -- with the destination 16-byte aligned and offset by one row.  No test passes an out-of-range id."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [1, 2, 17, 64, 3, 1, 40]
IDS = [[0], [6], [3, 3, 3], [6, 5, 4, 3, 2, 1, 0], [1, 5]]
STORES = {"74 fp32": (74, torch.float32, False), "300 fp32": (300, torch.float32, False), "768 bf16": (768, torch.bfloat16, False),
          "5 fp16": (5, torch.float16, False), "8 bf16": (8, torch.bfloat16, False), "targets 6 fp32": (6, torch.float32, True)}
POISON, GUARD, G = 0xFF, 0xA5, 64


def ST():
    return torch.cuda.current_stream().cuda_stream


_CACHE = {}


def _store(name):
    """(store bytes [N_rows, row_bytes] uint8 on the device -- viewed by the kernel as `dtype` rows --, its CPU copy, offsets int64 on
    the device, host offsets); made once per store and never changed"""
    if name not in _CACHE:
        d, dtype, targets = STORES[name]
        lens = [1] * len(LENS) if targets else LENS
        rb = d * torch.empty((), dtype=dtype).element_size()
        g = torch.Generator().manual_seed(len(name) + d)
        host = torch.randint(0, 256, (sum(lens), rb), dtype=torch.uint8, generator=g)
        host[0, :4] = torch.tensor([0, 0, 0xC0, 0x7F], dtype=torch.uint8)          # a NaN and an Inf, whatever the generator drew
        host[-1, -4:] = torch.tensor([0, 0, 0x80, 0xFF], dtype=torch.uint8)
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        _CACHE[name] = (host.cuda(), host, torch.tensor(off, dtype=torch.int64).cuda(), off, rb)
    return _CACHE[name]


def _run(name, ids, tail, shift_rows):
    from hri_emo_amd import _lib
    dev, host, off_dev, off, rb = _store(name)
    n = len(ids)
    cu = [0]
    for i in ids:
        cu.append(cu[-1] + off[i + 1] - off[i])
    dst_rows = cu[n] + tail
    plan = torch.tensor(ids + cu, dtype=torch.int32).cuda()
    # [guard | shift_rows poison rows | dst_rows rows | one poison row | guard]
    before, size = G + shift_rows * rb, G + (shift_rows + dst_rows + 1) * rb + G
    buf = torch.full((size,), POISON, dtype=torch.uint8, device="cuda")
    buf[:G] = GUARD
    buf[size - G:] = GUARD
    was = buf.cpu()
    assert buf.data_ptr() % 16 == 0
    _lib.call("hriemo_gather_rows", dev.data_ptr(), rb, off_dev.data_ptr(), plan.data_ptr(), n, buf.data_ptr() + before, dst_rows, ST())
    torch.cuda.synchronize()
    got = buf.cpu()
    idx = [r for i in ids for r in range(off[i], off[i + 1])]
    ref = torch.cat([host[torch.tensor(idx)], torch.zeros(tail, rb, dtype=torch.uint8)])
    payload = got[before:before + dst_rows * rb].view(dst_rows, rb)
    what = (name, ids, tail, shift_rows)
    assert torch.equal(payload[:cu[n]], ref[:cu[n]]), ("gathered rows", what)
    assert not payload[cu[n]:].any(), ("zero tail", what)
    assert torch.equal(got[:before], was[:before]), ("bytes in front of the destination", what)
    assert torch.equal(got[before + dst_rows * rb:], was[before + dst_rows * rb:]), ("the row behind dst_rows and the guard", what)
    assert bool((got[before + dst_rows * rb:size - G] == POISON).all())


@pytest.mark.parametrize("shift_rows", [0, 1], ids=["aligned", "offset by one row"])
@pytest.mark.parametrize("name", list(STORES))
def test_gather_equals_torch_indexing(name, shift_rows):
    """every id list with a zero tail of 5 rows and with an empty one (dst_rows == dst_cu[n]: the next row keeps its poison).  For 74
    fp32 the one-row offset shifts the destination by 8 bytes modulo 16 against the source; for 5 fp16 it leaves it 2-byte aligned."""
    for ids in IDS:
        for tail in (5, 0):
            _run(name, ids, tail, shift_rows)


def test_gather_many_blocks():
    """a destination of several blocks (768 bf16: 24 KiB per 16 rows; 64-row utterances repeated) with segment boundaries inside
    blocks and a long zero tail"""
    _run("768 bf16", [3, 6, 3, 2, 3, 6, 0, 3], 100, 0)
    _run("74 fp32", [3, 6, 3, 2, 3, 6, 0, 3], 100, 1)


def test_bad_arguments_are_refused():
    from hri_emo_amd import _lib
    L = _lib.lib()
    dev, _, off_dev, off, rb = _store("8 bf16")
    plan = torch.tensor([0, 0, 1], dtype=torch.int32).cuda()
    dst = torch.full((4 * rb,), POISON, dtype=torch.uint8, device="cuda")
    good = [dev.data_ptr(), rb, off_dev.data_ptr(), plan.data_ptr(), 1, dst.data_ptr(), 4, ST()]
    for pos, value in ((4, 0), (4, -1), (4, 1 << 20), (1, 0), (6, 0), (0, None), (2, None), (3, None), (5, None), (3, plan.data_ptr() + 2)):
        args = list(good)
        args[pos] = value
        assert L.hriemo_gather_rows(*args) == 1, (pos, value)
        assert b"gather_rows" in L.hriemo_last_error()
        with pytest.raises(RuntimeError, match="gather_rows"):
            _lib.call("hriemo_gather_rows", *args)
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()), "a refusal launches nothing"
    assert L.hriemo_gather_rows(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu()[:rb], _store("8 bf16")[1][0]) and not dst[rb:].any()
