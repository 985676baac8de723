"""What the GPU attention variant tests share (test_gpu_attention_variants.py: padded entries, test_gpu_attention_variants_packed.py:
packed entries): the launch plan read through the ABI and the guarded device buffers."""
import ctypes

import torch

W = "W"                 # batch size found at run time: the first one that takes the wide (128-row) backward tile
GUARD_ROWS = 128        # one wide tile before and after every row buffer
GUARD_FLOATS = 64       # lse / delta
SENTINEL = 0xFF         # guard byte: 0xFFFF is a bf16 NaN and 0xFFFFFFFF an fp32 NaN, so a guard that is READ poisons a result too

FWD_FORM = {128: "fwd<4,2>", 64: "fwd<4,1>", 16: "fwd<1,1>"}       # rows per block -> <waves, 16-row sub-tiles per wave>
BWD_SIDE = {128: "w128", 64: "n64", 16: "1w"}


def plan(L_, B, H, Lq, Lk, hd, cus=0):
    """hriemo_attn_plan (host code, no launch; cus = 0: this device): (fwd_rows, bwd_form, dq_rows, dkv_rows, dq_colsum_rows,
    kv_colsum_rows), or None where the library refuses the shape"""
    out = [ctypes.c_int() for _ in range(6)]
    if L_.hriemo_attn_plan(B, H, Lq, Lk, hd, cus, *(ctypes.byref(o) for o in out)) != 0:
        return None
    return tuple(o.value for o in out)


def forward_form(L_, B, H, Lq, Lk, hd, cus=0):
    return FWD_FORM[plan(L_, B, H, Lq, Lk, hd, cus)[0]]


def backward_form(L_, B, H, Lq, Lk, hd, cus=0):
    """the form hriemo_attn_bwd takes for this shape, from the plan it launches"""
    _, form, dq_rows, dkv_rows, _, _ = plan(L_, B, H, Lq, Lk, hd, cus)
    if form == 1:
        return "fused-KW1" if dkv_rows == 64 else "fused-KW2"
    if form == 2:
        return "qres"
    return f"two-kernel(dq={BWD_SIDE[dq_rows]},dkv={BWD_SIDE[dkv_rows]})"


def wide_batch(L_, H, Lq, Lk, hd, want, lo=1, cus=0):
    """the first batch size >= lo whose backward takes the form `want`"""
    for B in range(lo, 129):
        if backward_form(L_, B, H, Lq, Lk, hd, cus) == want:
            return B
    raise AssertionError(f"no batch size in {lo}..128 takes {want} at H={H}, Lq={Lq}, Lk={Lk}, hd={hd} on this device: "
                         "update the variant table so that the 128-row backward tiles stay covered")


class Guarded:
    """rows x cols payload of `dtype` inside a byte buffer pre-filled with SENTINEL: guard rows before and after, and a leading
    dimension wider than the payload.  .t is the payload view handed to the kernels, .intact() compares every guard byte."""

    def __init__(self, rows, cols, dtype, ld=None, guard_rows=GUARD_ROWS, fill=None):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.ld, self.g = rows, cols, ld, guard_rows
        self.item = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((rows + 2 * guard_rows) * ld * self.item,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.raw.view(dtype).view(rows + 2 * guard_rows, ld)[guard_rows:guard_rows + rows, :cols]
        assert self.t.data_ptr() % 16 == 0
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        by = self.raw.cpu().numpy().reshape(self.rows + 2 * self.g, self.ld * self.item)
        return bool((by[:self.g] == SENTINEL).all() and (by[self.g + self.rows:] == SENTINEL).all() and
                    (by[self.g:self.g + self.rows, self.cols * self.item:] == SENTINEL).all())


class GuardedFlat:
    """n contiguous elements with `guard` sentinel elements each side"""

    def __init__(self, n, dtype, guard):
        self.n, self.guard = n, guard
        self.item = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * guard) * self.item,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.raw.view(dtype)[guard:guard + n]
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        by = self.raw.cpu().numpy()
        g = self.guard * self.item
        return bool((by[:g] == SENTINEL).all() and (by[g + self.n * self.item:] == SENTINEL).all())
