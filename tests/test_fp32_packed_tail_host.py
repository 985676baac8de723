"""Host side of the fp32 packed tail (no GPU): the switch.  `_ops.PACKED_TAIL_FP32` keeps the packed rows going through the gate
and the decoder's memory in the fp32 precision mode; `_ops.PACKED_TAIL` keeps meaning the bf16 tail alone
(tests/test_packed_tail_host.py pins that half), and the MX-fp8 mode unpacks whatever is set."""
import pytest


@pytest.fixture()
def ops():
    from hri_emo_amd import _ops
    saved = (_ops.precision(), _ops.gemm_mode(), _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32)
    yield _ops
    _ops.set_precision(saved[0])
    _ops.set_gemm_mode(saved[1])
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32 = saved[2], saved[3]


def test_both_switches_ship_off():
    """read from the module's text: another test of this process may have set them"""
    import inspect
    import re
    from hri_emo_amd import _ops
    src = inspect.getsource(_ops)
    assert re.findall(r"^PACKED_TAIL = (\w+)$", src, re.M) == ["False"]
    assert re.findall(r"^PACKED_TAIL_FP32 = (\w+)$", src, re.M) == ["False"]


def test_fp32_packs_the_tail_only_with_its_own_switch(ops):
    ops.set_gemm_mode("bf16")
    ops.set_precision("fp32")
    ops.PACKED_TAIL, ops.PACKED_TAIL_FP32 = False, False
    assert ops.packed_tail() is False
    ops.PACKED_TAIL = True                           # the bf16 switch alone leaves the fp32 tail unpacked
    assert ops.packed_tail() is False
    ops.PACKED_TAIL, ops.PACKED_TAIL_FP32 = False, True
    assert ops.packed_tail() is True
    ops.PACKED_TAIL = True
    assert ops.packed_tail() is True


def test_the_fp32_switch_does_not_pack_the_bf16_tail(ops):
    ops.set_gemm_mode("bf16")
    ops.set_precision("bf16")
    ops.PACKED_TAIL, ops.PACKED_TAIL_FP32 = False, True
    assert ops.packed_tail() is False
    ops.PACKED_TAIL = True
    assert ops.packed_tail() is True


def test_mx_fp8_unpacks_whatever_is_set(ops):
    ops.PACKED_TAIL, ops.PACKED_TAIL_FP32 = True, True
    ops.set_precision("bf16")
    ops.set_gemm_mode("mx_fp8")
    assert ops.packed_tail() is False
    ops.set_gemm_mode("bf16")
    assert ops.packed_tail() is True


def test_the_four_packed_entries_are_bound():
    """header, library and binding table agree (tests/test_abi_and_host.py compares the three sets); here: the names the issue fixes"""
    from hri_emo_amd import _lib
    for name in ("hriemo_masked_mean_f32_packed", "hriemo_fuse_f32_packed", "hriemo_gate_dpre_f32_packed", "hriemo_gate_dy_f32_packed"):
        assert name in _lib._SIGS, name
        assert hasattr(_lib.lib(), name), name
