"""The limits of tests/pool32_reference.py, proved on the CPU: every fp32 yardstick order passes every case, every planted fault
fails at the smallest case that shows it, and the switch, its exports and the header's declarations are in place (no GPU)."""
import os
import re

import pytest
import torch

import pool32_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _run(case, order, fault=None):
    """forward, pools and backward of one yardstick order (the fault planted wherever it applies), checked as the GPU suite checks"""
    name = f"{order[1]}{'/' + fault if fault else ''}"
    fw = P.fwd32(case, order, fault)
    P.check_fwd(fw, case, name)
    pool = P.pools32(fw["valid"], case, order, fault)
    P.check_pools(pool, fw["valid"], case, name + " pool")
    P.check_bwd(P.bwd32(case, order, fault), case, name)


def test_the_case_table_covers_the_edges():
    for d in P.WIDTHS:
        for L in P.LENGTHS:
            for k in P.keeps(L):
                assert any(c[:3] == (L, k, d) for c in P.CASES), (L, k, d)
    for L in P.LENGTHS:
        assert {c[3] for c in P.CASES if c[0] == L} == set(P.MASKS), L
    for d in P.WIDTHS:
        assert {c[4] for c in P.CASES if c[2] == d} == {0, 1} and {c[5] for c in P.CASES if c[2] == d} == {True, False}, d
    assert P.keeps(70) == [1, 32, 69, 70] and P.keeps(1) == [1] and P.keeps(32) == [1, 31, 32]
    assert len({P.case_id(c) for c in P.CASES}) == len(P.CASES)
    # the mask families are what they say
    g = torch.Generator().manual_seed(0)
    for L in P.LENGTHS:
        assert P.mask_of("none", L, g) is None
        assert (~P.mask_of("prefix", L, g)).sum(1).tolist() == [1, max(1, L // 2), L]
        assert (~P.mask_of("scattered", L, g)).sum(1).min() >= 1
        assert (~P.mask_of("allpad", L, g)).sum(1)[1] == 0
        assert (~P.mask_of("single", L, g)).sum(1)[2] == 1


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_every_yardstick_order_passes(c):
    case = P.make_case(c)
    for order in P.ORDERS:
        _run(case, order)


def test_gate_in_is_one_operation_per_element():
    g = torch.Generator().manual_seed(3)
    a, t = torch.randn(3, 8, generator=g), torch.randn(3, 8, generator=g)
    gin = P.gate_in32(a, t)
    assert gin.shape == (3, 32) and torch.equal(gin[:, :8], a) and torch.equal(gin[:, 8:16], t)
    assert torch.equal(gin[:, 16:24].double(), (a.double() - t.double()).float().abs().double())
    assert torch.equal(gin[:, 24:].double(), (a.double() * t.double()).float().double())


# fault -> the smallest case of the table's families that shows it: (L, Lkeep, d, mask, accumulate, has_g)
FAULTS = {
    "masked_in_valid": (1, 1, 4, "allpad", 0, True),          # one row, masked: part_valid must be exactly 0
    "keep_off_by_one": (31, 1, 4, "none", 0, True),           # the first length with a row behind Lkeep
    "behind_keep": (33, 32, 4, "none", 0, True),              # the first length with a chunk behind Lkeep
    "drop_last_row": (1, 1, 4, "none", 0, True),              # row 0 is the last row of its chunk
    "cnt_unclamped": (1, 1, 4, "allpad", 0, True),            # 0 / 0
    "keep_divisor": (31, 31, 4, "prefix", 0, True),           # 1, 15 and 31 valid rows against Lkeep = 31
    "dpool_on_masked": (1, 1, 4, "allpad", 0, False),         # g == NULL: dYn of the masked row must be exactly 0
    "g_past_keep": (31, 1, 4, "none", 0, True),
    "unbiased": (1, 1, 4, "none", 0, True),                   # d / (d - 1) = 4 / 3
    "eps_outside": (1, 1, 4, "none", 0, True),
    "accumulate_ignored": (1, 1, 4, "none", 1, True),
    "dbeta_from_dx": (1, 1, 4, "none", 0, True),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_every_fault_fails_at_its_smallest_case(fault):
    case = P.make_case(FAULTS[fault])
    for order in P.ORDERS:
        _run(case, order)                              # the case itself passes in every order
        with pytest.raises(AssertionError):
            _run(case, order, fault)


def test_faults_in_the_test_table_are_the_issue_list():
    assert len(FAULTS) == 12


def test_counted_factors():
    case = P.make_case((70, 32, 260, "scattered", 1, True))
    assert P.sum_factor("dgamma", case) == 3 * 70 + 16 + 1 and P.sum_factor("dbeta", case) == 3 * 70 + 1
    case = P.make_case((70, 32, 260, "scattered", 0, True))
    assert P.sum_factor("dgamma", case) == 3 * 70 + 16 and P.sum_factor("dbeta", case) == 3 * 70
    assert P.LN_Y == 54.0 and P.LN_DS == 15.0 and P.chunk_rows(70) == [32, 32, 6] and P.chunks(32) == 1 and P.chunks(33) == 2


def test_switch_exports_and_refusal_message():
    import hri_emo_amd as H
    from hri_emo_amd import _ops, dp
    assert _ops.POOLED_GATE_FP32 is False and H.pooled_gate_fp32() is False
    assert "set_pooled_gate_fp32" in H.__all__ and "pooled_gate_fp32" in H.__all__
    keep = (_ops.precision(), _ops.gemm_mode())
    try:
        H.set_pooled_gate_fp32(1)
        assert _ops.POOLED_GATE_FP32 is True and H.pooled_gate_fp32() is True
        _ops._require_pooled_path("x")                                       # bf16 / bf16: served whatever the switch says
        H.set_precision("fp32")
        _ops._require_pooled_path("x")
        assert dp._mode_switches()[-1] == ("POOLED_GATE_FP32", True)
        H.set_gemm_mode("mx_fp8")
        with pytest.raises(NotImplementedError, match="GEMM mode"):
            _ops._require_pooled_path("x")
        H.set_gemm_mode("bf16")
        H.set_pooled_gate_fp32(False)
        assert dp._mode_switches()[-1] == ("POOLED_GATE_FP32", False)
        with pytest.raises(NotImplementedError, match="POOLED_GATE_FP32"):
            _ops._require_pooled_path("x")
        H.set_precision("bf16")
        _ops._require_pooled_path("x")
        # in bf16 precision the switch is not read and not recorded
        assert [n for n, _ in dp._mode_switches()] == ["precision", "gemm_mode", "PACKED_TAIL", "PACKED_TAIL_FP32", "PACKED_TAIL_MX8", "ingest"]
    finally:
        H.set_pooled_gate_fp32(False)
        H.set_precision(keep[0])
        H.set_gemm_mode(keep[1])


def test_header_declares_the_pool32_exports_and_the_binding_knows_them():
    from hri_emo_amd import _lib
    text = open(os.path.join(ROOT, "include", "hriemo.h")).read()
    names = sorted(set(re.findall(r"\b(hriemo_pool32_\w+)\s*\(", text)))
    assert names == ["hriemo_pool32_gate_input", "hriemo_pool32_ln_bwd", "hriemo_pool32_ln_bwd_workspace_bytes", "hriemo_pool32_ln_fwd"]
    for n in names:
        assert n in _lib._SIGS, n
        # (the fp32 coverage table of fp32_reference.py lists names of two other shapes; these must not fall under them)
        assert not re.fullmatch(r"hriemo_\w*_f32\w*", n) and not n.startswith("hriemo_split")
