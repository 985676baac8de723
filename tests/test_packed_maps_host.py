"""Host side of the attention-map export on packed (varlen) rows (no GPU): the opt-in switch, what _ops.attn_rows hands a sub-layer
that is asked for its map, and the two C-ABI entry points (hriemo_attn_probs_varlen, hriemo_attn_probs_f32_varlen)."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS_A = [70, 33, 32, 1, 17]
LENS_T = [40, 1, 32, 31, 16]
B, LA, LT = 5, 70, 40
REFUSAL = "attention maps are exported by the padded path only"


def _masks():
    return (torch.arange(LA)[None] >= torch.tensor(LENS_A)[:, None]), (torch.arange(LT)[None] >= torch.tensor(LENS_T)[:, None])


@pytest.fixture
def maps_switch():
    from hri_emo_amd import _ops
    before = _ops.PACKED_MAPS
    yield _ops
    _ops.PACKED_MAPS = before


def test_the_switch_is_off_by_default_and_exported(maps_switch):
    import hri_emo_amd as H
    _ops = maps_switch
    assert _ops.PACKED_MAPS is False and H.varlen_maps() is False
    assert "set_varlen_maps" in H.__all__ and "varlen_maps" in H.__all__
    H.set_varlen_maps(True)
    assert H.varlen_maps() is True and _ops.PACKED_MAPS is True
    H.set_varlen_maps(0)
    assert H.varlen_maps() is False
    # a module constant and a setter, not an environment switch
    src = open(os.path.join(REPO, "hri-emo_amd", "_ops.py")).read()
    assert not re.search(r"environ[^\n]*MAPS", src)


def test_attn_rows_hands_out_the_packed_rows_with_the_switch_on(maps_switch):
    _ops = maps_switch
    m_a, m_t = _masks()
    sa, st, sf = _ops.seq_plans(m_a, m_t, B, LA, LT)
    sq = _ops.query_seq(B, 6, torch.device("cpu"))
    _ops.set_varlen_maps(True)
    assert _ops.attn_rows(sa, sa, True) == (5, 70, 70, None, (sa.cu, sa.cu), 70, sa.idx, False) == _ops.attn_rows(sa, sa, False)
    assert _ops.attn_rows(sa, st, True) == (5, 70, 40, None, (sa.cu, st.cu), 70, sa.idx, False) == _ops.attn_rows(sa, st, False)
    assert _ops.attn_rows(sq, sf, True) == (5, 6, 40, None, (sq.cu, sf.cu), 6, None, False) == _ops.attn_rows(sq, sf, False)
    # the padded layouts are what they were
    pt = _ops.Seq.padded(B, LT, m_t)
    assert _ops.attn_rows(pt, pt, True) == (5, 40, 40, pt.kpm, None, 40, None, False)


def test_attn_rows_still_refuses_bucket_plans_and_mixed_layouts(maps_switch):
    _ops = maps_switch
    m_a, m_t = _masks()
    sa, st, _ = _ops.seq_plans(m_a, m_t, B, LA, LT)
    pa, pt = _ops.Seq.padded(B, LA, m_a), _ops.Seq.padded(B, LT, m_t)
    rows = 128
    cu = torch.tensor([0, 40, 41, 73, 104, 120, rows], dtype=torch.int32)
    sb = _ops.seq_bucket(cu, B, LT, rows)
    _ops.set_varlen_maps(True)
    # a bucket plan's filler sequence has no sample to export: on either side of the sub-layer
    for q, k in ((sb, sb), (sa, sb), (sb, sa)):
        with pytest.raises(ValueError, match=REFUSAL):
            _ops.attn_rows(q, k, True)
    assert _ops.attn_rows(sb, sb, False).B == B + 1          # (without the map the bucket plan runs as before)
    for q, k in ((sa, pt), (pa, st), (sa.with_kpm(m_a), st), (sa, st.with_kpm(m_t))):
        with pytest.raises(ValueError, match="packed sequences carry their lengths; no key_padding_mask"):
            _ops.attn_rows(q, k, True)


def test_attn_rows_refuses_as_before_with_the_switch_off(maps_switch):
    _ops = maps_switch
    m_a, m_t = _masks()
    sa, st, sf = _ops.seq_plans(m_a, m_t, B, LA, LT)
    sq = _ops.query_seq(B, 6, torch.device("cpu"))
    _ops.set_varlen_maps(False)
    for q, k in ((sa, sa), (sa, st), (sq, sf)):
        with pytest.raises(ValueError, match=REFUSAL):
            _ops.attn_rows(q, k, True)


def test_the_two_entry_points_are_declared_exported_and_bound():
    from hri_emo_amd import _lib
    hdr = open(os.path.join(REPO, "include", "hriemo.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    args = "plplppppiiiiiiifQpIip"      # Q ldq K ldk cu_q cu_k lse probs | B H max_q max_k out_lq out_lk hd | p seed seed_dev site b_off stream
    for name in ("hriemo_attn_probs_varlen", "hriemo_attn_probs_f32_varlen"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert _lib._SIGS[name] == (args, "i")
    # the padded entry points are what they were
    assert _lib._SIGS["hriemo_attn_probs"] == _lib._SIGS["hriemo_attn_probs_f32"] == ("plplpppiiiiifQpIip", "i")
