"""Host side of the packed tail (no GPU): the fused sequence plan -- sample b of the fused memory has min(la[b], lt[b]) rows,
because the reference ORs the two prefix masks cut to the text length (models/fusion_with_emotion_decoder.py:62-79)."""

import torch

LENS_A = [70, 33, 32, 1, 17]
LENS_T = [40, 1, 32, 31, 16]
LENS_F = [40, 1, 32, 1, 16]
B, LA, LT = 5, 70, 40


def _masks():
    return (torch.arange(LA)[None] >= torch.tensor(LENS_A)[:, None]), (torch.arange(LT)[None] >= torch.tensor(LENS_T)[:, None])


def _cum(lens):
    out = [0]
    for x in lens:
        out.append(out[-1] + x)
    return out


def test_fused_plan_comes_from_the_masks():
    from hri_emo_amd import _ops
    m_a, m_t = _masks()
    plans = _ops.seq_plans(m_a, m_t, B, LA, LT)
    assert plans is not None and len(plans) == 3
    sa, st, sf = plans
    assert sa.cu.tolist() == _cum(LENS_A) and st.cu.tolist() == _cum(LENS_T)
    assert sf.cu.tolist() == _cum(LENS_F) and sf.cu.dtype == torch.int32
    assert (sf.B, sf.Breal, sf.L, sf.Lmax, sf.N, sf.surplus, sf.idx) == (B, B, LT, 40, sum(LENS_F), False, None)
    # what the reference's fused mask leaves valid
    fused = m_a[:, :LT] | m_t
    assert (~fused).sum(1).tolist() == LENS_F
    assert _ops.seq_plans(m_a, m_t, B, LA, LT)[2] is sf          # cached: no second read of the lengths


def test_masks_that_are_not_prefixes_give_no_plan():
    from hri_emo_amd import _ops
    m_a, m_t = _masks()
    hole = m_t.clone(); hole[0, 3] = True
    assert _ops.seq_plans(m_a, hole, B, LA, LT) is None
    empty = m_a.clone(); empty[2, :] = True
    assert _ops.seq_plans(empty, m_t, B, LA, LT) is None
    assert _ops.seq_plans(None, m_t, B, LA, LT) is None


def test_bucket_fused_plan_rides_in_the_text_bucket():
    from hri_emo_amd import _ops, dp
    m_a, m_t = _masks()
    for lengths in (None, (LENS_A, LENS_T)):
        (ra, rt), _, cu_t, cu_f = dp.packed_tables(*dp.mask_lengths(m_a, m_t, lengths, B, LA, LT), B, LA, LT)
        assert cu_f[:B + 1] == _cum(LENS_F)
        assert cu_f[B + 1] == rt == cu_t[B + 1] and cu_f[B] < rt          # ends at the text bucket's row count
    sf = _ops.seq_bucket_fused(torch.tensor(cu_f, dtype=torch.int32), B, LT, rt)
    # the surplus rows form no sequence on the attention side: B sequences, not B + 1, and the plan says that rows are left over
    assert (sf.B, sf.Breal, sf.N, sf.L, sf.Lmax, sf.surplus) == (B, B, rt, LT, LT, True)
    st = _ops.seq_bucket(torch.tensor(cu_t, dtype=torch.int32), B, LT, rt)
    assert st.B == B + 1 and st.N == sf.N


def test_decoder_query_plan_is_trivial():
    from hri_emo_amd import _ops
    sq = _ops.query_seq(B, 6, torch.device("cpu"))
    assert sq.cu.tolist() == [6 * b for b in range(B + 1)] and sq.idx is None and (sq.B, sq.L, sq.Lmax, sq.N) == (B, 6, 6, 6 * B)
    assert _ops.query_seq(B, 6, torch.device("cpu")) is sq


def test_the_tail_unpacks_outside_the_bf16_path():
    from hri_emo_amd import _ops
    prec, mode, tail = _ops.precision(), _ops.gemm_mode(), _ops.PACKED_TAIL
    try:
        _ops.PACKED_TAIL = False
        assert not _ops.packed_tail()
        _ops.PACKED_TAIL = True
        assert _ops.packed_tail()
        _ops.set_precision("fp32")
        assert not _ops.packed_tail()
        _ops.set_precision("bf16")
        _ops.set_gemm_mode("mx_fp8")
        assert not _ops.packed_tail()
    finally:
        _ops.set_precision(prec)
        _ops.set_gemm_mode(mode)
        _ops.PACKED_TAIL = tail


# ----------------------------------------------------------------------------- the layout value (Seq) and attn_rows
def test_padded_layout():
    import pytest
    from hri_emo_amd import _ops
    _, m_t = _masks()
    s = _ops.Seq.padded(B, LT, m_t)
    assert (s.cu, s.idx, s.B, s.Breal, s.L, s.Lmax, s.N, s.surplus) == (None, None, 5, 5, 40, 40, 200, False)
    assert s.kpm.dtype == torch.uint8 and tuple(s.kpm.shape) == (5, 40) and torch.equal(s.kpm.bool(), m_t)
    assert s.kpm.data_ptr() == m_t.data_ptr()                    # a bool mask is viewed, not copied
    assert not s.packed and s.shape(16) == (5, 40, 16)
    assert _ops.Seq.padded(B, LT).kpm is None
    with pytest.raises(ValueError, match="key_padding_mask shape"):
        _ops.Seq.padded(B, LA, m_t)
    with pytest.raises(ValueError, match="rows of its layout"):
        s.holds(torch.zeros(B, LA, 16))
    s.holds(torch.zeros(B, LT, 16))


def test_attn_rows_of_the_five_layouts():
    import pytest
    from hri_emo_amd import _ops
    m_a, m_t = _masks()
    # padded self-attention (text) and padded cross-attention (audio queries, text keys: the keys' mask)
    pa, pt = _ops.Seq.padded(B, LA, m_a), _ops.Seq.padded(B, LT, m_t)
    assert _ops.attn_rows(pt, pt, False) == (5, 40, 40, pt.kpm, None, 40, None, False)
    assert _ops.attn_rows(pt, pt, True) == (5, 40, 40, pt.kpm, None, 40, None, False)          # maps: the padded path exports them
    assert _ops.attn_rows(pa, pt, False) == (5, 70, 40, pt.kpm, None, 70, None, False)
    # packed self-attention from seq_plan
    sa, st, sf = _ops.seq_plans(m_a, m_t, B, LA, LT)
    assert sa.packed and sa.kpm is None and sa.shape(16) == (1, sum(LENS_A), 16)
    assert _ops.attn_rows(sa, sa, False) == (5, 70, 70, None, (sa.cu, sa.cu), 70, sa.idx, False)
    assert _ops.attn_rows(st, st, False) == (5, 40, 40, None, (st.cu, st.cu), 40, st.idx, False)
    # packed cross-attention, both directions
    assert _ops.attn_rows(sa, st, False) == (5, 70, 40, None, (sa.cu, st.cu), 70, sa.idx, False)
    assert _ops.attn_rows(st, sa, False) == (5, 40, 70, None, (st.cu, sa.cu), 40, st.idx, False)
    # bucket plan: the filler rows are one more sequence
    rows = 128
    cu = torch.tensor(_cum(LENS_T) + [rows], dtype=torch.int32)
    sb = _ops.seq_bucket(cu, B, LT, rows)
    assert _ops.attn_rows(sb, sb, False) == (6, 40, 40, None, (cu, cu), 40, sb.idx, False)
    # the decoder: N_e = 6 query rows per sample on the fused memory of a bucket, whose surplus rows are no sequence
    cu_f = torch.tensor(_cum(LENS_F) + [rows], dtype=torch.int32)
    sq, sbf = _ops.query_seq(B, 6, torch.device("cpu")), _ops.seq_bucket_fused(cu_f, B, LT, rows)
    assert _ops.attn_rows(sq, sbf, False) == (5, 6, 40, None, (sq.cu, cu_f), 6, None, True)
    assert _ops.attn_rows(sq, sf, False) == (5, 6, 40, None, (sq.cu, sf.cu), 6, None, False)
    # the two refusals live here and nowhere else
    for q, k in ((sa, sa), (sa, st), (sq, sbf)):
        with pytest.raises(ValueError, match="attention maps are exported by the padded path only"):
            _ops.attn_rows(q, k, True)
    for q, k in ((sa, pt), (pa, st), (sa.with_kpm(m_a), st), (sa, st.with_kpm(m_t))):
        with pytest.raises(ValueError, match="packed sequences carry their lengths; no key_padding_mask"):
            _ops.attn_rows(q, k, False)


def test_a_plan_with_the_masks_riding_along():
    """the gate's copies (Seq.with_kpm): every field of the plan, plus the padded mask its valid counts are read from"""
    from hri_emo_amd import _ops
    m_a, m_t = _masks()
    sa = _ops.seq_plan(m_a, B, LA)
    g = sa.with_kpm(m_a)
    assert (g.cu, g.idx, g.B, g.Breal, g.L, g.Lmax, g.N, g.surplus) == (sa.cu, sa.idx, sa.B, sa.Breal, sa.L, sa.Lmax, sa.N, sa.surplus)
    assert g.kpm.dtype == torch.uint8 and torch.equal(g.kpm.bool(), m_a) and sa.kpm is None
    p = _ops.Seq.padded(B, LT).with_kpm(m_t)
    assert not p.packed and torch.equal(p.kpm.bool(), m_t)


def test_cross_attention_refuses_half_given_shared_projections(monkeypatch):
    """CrossAttnLN owns its Q projection unless q_pre is given and its K | V projection unless kv_pre is; q_pre comes from a
    SharedProjFn node together with the gradient slots and the K | V half, so q_pre without slots, slots without q_pre and q_pre
    without kv_pre are refused in forward, before anything touches the device (CPU tensors here, and no library call)."""
    import pytest
    from hri_emo_amd import _lib, _ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(_lib, "lib", no_call)
    d, nh = 32, 2
    xq, xkv = torch.randn(2, 3, d), torch.randn(2, 5, d)
    w_in, b_in, w_out, b_out = torch.randn(3 * d, d), torch.zeros(3 * d), torch.randn(d, d), torch.zeros(d)
    gamma, beta = torch.ones(d), torch.zeros(d)
    sq, sk = _ops.Seq.padded(2, 3), _ops.Seq.padded(2, 5)
    q_pre, kv_pre = torch.randn(6, d), torch.randn(10, 2 * d)
    slots = (object(), object())          # (never looked into: the refusal comes first)

    def apply(**kw):
        opt = dict(kv_pre=None, join_q=None, q_pre=None, slots=None)
        opt.update(kw)
        return _ops.CrossAttnLN.apply(xq, None, xkv, w_in, b_in, w_out, b_out, gamma, beta, _ops.Shadows(), nh, sq, sk, 0.0, 0, 4, 0, False,
                                      opt["kv_pre"], opt["join_q"], opt["q_pre"], opt["slots"])

    with torch.no_grad():
        for kw in (dict(q_pre=q_pre, kv_pre=kv_pre), dict(slots=slots, kv_pre=kv_pre), dict(q_pre=q_pre, slots=slots)):
            with pytest.raises(ValueError, match="q_pre and slots"):
                apply(**kw)
