"""Host side of the MX-fp8 mode on packed rows (no GPU): which switch answers packed_tail() in which mode, and the two new entries
in the three places that name the C ABI (header, bindings, library)."""
import itertools
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hriemo_attn_fwd_q_varlen", "hriemo_fuse_fwd_packed_q")


def test_packed_tail_truth_table():
    """bf16 operands / bf16 precision: PACKED_TAIL; fp32 precision (bf16 operands): PACKED_TAIL_FP32; MX-fp8 operands / bf16
    precision: PACKED_TAIL_MX8; MX-fp8 with fp32 precision: never.  No switch answers for another mode."""
    from hri_emo_amd import _ops
    saved = (_ops.GEMM_MODE, _ops.PRECISION, _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8)
    try:
        assert saved[2:] == (False, False, False), "the tail switches ship off"
        for gemm, prec in itertools.product(("bf16", "mx_fp8"), ("bf16", "fp32")):
            _ops.set_gemm_mode(gemm)
            _ops.set_precision(prec)
            for t16, t32, t8 in itertools.product((False, True), repeat=3):
                _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = t16, t32, t8
                want = {("bf16", "bf16"): t16, ("bf16", "fp32"): t32, ("mx_fp8", "bf16"): t8, ("mx_fp8", "fp32"): False}[(gemm, prec)]
                assert _ops.packed_tail() is want, (gemm, prec, t16, t32, t8)
        _ops.set_gemm_mode("mx_fp8")
        _ops.set_precision("bf16")
        _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = True, True, False
        assert _ops.packed_tail() is False          # the two older switches alone leave the fp8 mode on its previous launches
    finally:
        _ops.GEMM_MODE, _ops.PRECISION, _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = saved


def test_attention_copy_switch_ships_on():
    from hri_emo_amd import _ops
    assert _ops.ATTN_Q_VARLEN is True


def test_new_entries_are_declared_bound_and_exported():
    from hri_emo_amd import _lib
    hdr = open(os.path.join(REPO, "include", "hriemo.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert name in _lib._SIGS, name
        assert hasattr(L, name), name
    # the packed launch takes the arguments of hriemo_attn_fwd_varlen, then Oq, ldoq, So, ldso, n_rows in front of the stream
    assert _lib._SIGS["hriemo_attn_fwd_q_varlen"][0] == _lib._SIGS["hriemo_attn_fwd_varlen"][0][:-1] + "plpll" + "p"
    assert _lib._SIGS["hriemo_fuse_fwd_packed_q"][0] == _lib._SIGS["hriemo_fuse_fwd_packed"][0][:-1] + "ppl" + "p"
