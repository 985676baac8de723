"""GPU suite of the MX-fp8 GEMM mode on packed (varlen) rows.

Kernel level (through the C ABI): hriemo_attn_fwd_q_varlen and hriemo_fuse_fwd_packed_q leave the MX-fp8 copy of what they store --
bit-identical to hriemo_quant_mx8 of it and to the host emulation (tests/mx8_emul.py), the scale byte of packed row r in column r --
without changing the bf16 results of the launches without the copy; every output lives in a 0xFF-filled buffer with guard rows.
Then the wrapper (`_ops.ATTN_Q_VARLEN`), the model with `_ops.PACKED_TAIL_MX8` against the oracles and against the tail-off arm in
one process, the launches of a step, and the captured bucket graphs."""
import pytest
import torch

from mx8_emul import mx8_quantize, mx8_roundtrip
from oracle import hri_emo_oracle as O          # the checker (tests only)
from test_gpu_packed_tail import Guarded, P, ST, _cu

pytestmark = pytest.mark.gpu


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    saved = (_ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.ATTN_Q_VARLEN)
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_gemm_mode("bf16")
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.ATTN_Q_VARLEN = saved


def _mode(H, gemm, varlen, tail, attn_q=True):
    from hri_emo_amd import _ops
    H.set_gemm_mode(gemm)
    H.set_varlen(varlen)
    _ops.PACKED_TAIL_MX8 = tail
    _ops.ATTN_Q_VARLEN = attn_q


def _scale_cols_intact(g, n):
    """the scale columns at and past `n` of a Guarded [K/32, ld] buffer still hold the fill pattern"""
    return bool((g.t[:, n:] == 0xFF).all())


# ----------------------------------------------------------------------------- 1. attention epilogue on packed rows
def _lens(B, L, gen):
    pool = sorted({min(max(x, 1), L) for x in (1, 15, 16, 17, 63, 64, 65, L - 1, L)})
    lens = [pool[int(i)] for i in torch.randint(0, len(pool), (B,), generator=gen)]
    lens[int(torch.randint(0, B, (1,), generator=gen))] = L          # at least one sample at full length
    return lens


@pytest.mark.parametrize("filler", [0, 8])
@pytest.mark.parametrize("B,NH,Lq,Lk,hd,p", [(5, 4, 70, 33, 32, 0.1), (4, 8, 130, 70, 64, 0.1), (6, 8, 16, 40, 96, 0.0), (3, 8, 129, 130, 128, 0.1)])
def test_attention_packed_forward_leaves_the_quantised_output(H, B, NH, Lq, Lk, hd, p, filler):
    """hriemo_attn_fwd_q_varlen on all three forward tiles (L_q <= 16, <= 64, > 64) and both key-tile counts, lengths on the tile
    edges, with and without the trailing all-zero filler sequence of a bucket: O / lse bit for bit those of hriemo_attn_fwd_varlen,
    Oq / So those of the separate quantiser, of the padded hriemo_attn_fwd_q launch under the prefix masks (valid rows) and of the
    host emulation; guard bytes and the scale columns >= n_rows untouched."""
    from hri_emo_amd import _lib, _ops as ops
    L_ = _lib.lib()
    d = NH * hd
    g = torch.Generator().manual_seed(B * 1000 + Lq + filler)
    lq, lk = _lens(B, Lq, g), _lens(B, Lk, g)
    vq = torch.arange(Lq)[None] < torch.tensor(lq)[:, None]
    vk = torch.arange(Lk)[None] < torch.tensor(lk)[:, None]
    q3 = (torch.randn(B, Lq, d, generator=g) * 1.5).bfloat16()
    for b in range(B):
        # PAD query rows of the padded layout: what the packed launch's lanes past the end read (the sample's last row, clamped).
        # The forward moves its softmax reference exponent by a wave-uniform vote, so a row's rounding depends on the rows that
        # share its wave; with these rows the padded and the packed launch hold the same vote by construction.
        q3[b, lq[b]:] = q3[b, lq[b] - 1]
    q2 = q3.view(B * Lq, d).cuda()
    kv2 = torch.randn(B * Lk, 2 * d, generator=g)
    kv2[:, d:] *= torch.exp(torch.randn(B * Lk, 1, generator=g))          # values of very different magnitude: so are the blocks of O
    kv2 = kv2.bfloat16().cuda()
    iq, ik = vq.reshape(-1).nonzero().reshape(-1).cuda(), vk.reshape(-1).nonzero().reshape(-1).cuda()
    qp, kvp = q2.index_select(0, iq), kv2.index_select(0, ik)
    nq_real, nseq = int(iq.numel()), B + (1 if filler else 0)
    if filler:
        qp = torch.cat([qp, torch.zeros(filler, d, dtype=qp.dtype, device="cuda")])
        kvp = torch.cat([kvp, torch.zeros(filler, 2 * d, dtype=kvp.dtype, device="cuda")])
    qp, kvp = qp.contiguous(), kvp.contiguous()
    n_rows = qp.shape[0]
    cq = _cu(lq, n_rows if filler else None)
    ck = _cu(lk, kvp.shape[0] if filler else None)
    seed, site, boff = 24680, 5, 3
    sw = P(ops.seed_word(q2.device))
    ldoq, ldso = d + 32, L_.hriemo_mx8_scale_ld(n_rows)

    def outputs():
        return Guarded(n_rows, d, torch.bfloat16), Guarded(nseq * NH, Lq, torch.float32)

    O0, lse0 = outputs()
    _lib.call("hriemo_attn_fwd_varlen", P(qp), d, P(kvp), 2 * d, P(kvp[:, d:]), 2 * d, P(O0.t), d, P(cq), P(ck), P(lse0.t), nseq, NH, Lq, Lk, hd,
              float(p), seed, sw, site, boff, None, ST())
    O1, lse1 = outputs()
    Oq, So = Guarded(n_rows, ldoq, torch.uint8), Guarded(d // 32, ldso, torch.uint8)
    _lib.call("hriemo_attn_fwd_q_varlen", P(qp), d, P(kvp), 2 * d, P(kvp[:, d:]), 2 * d, P(O1.t), d, P(cq), P(ck), P(lse1.t), nseq, NH, Lq, Lk, hd,
              float(p), seed, sw, site, boff, None, P(Oq.t), ldoq, P(So.t), ldso, n_rows, ST())
    torch.cuda.synchronize()
    assert torch.equal(O1.full.view(torch.uint8), O0.full.view(torch.uint8)), "O (and its guard rows)"
    assert torch.equal(lse1.full.view(torch.uint8), lse0.full.view(torch.uint8)), "lse (and its guard rows)"
    assert O1.intact() and O1.written() and lse1.intact()
    assert Oq.intact() and So.intact(), "guard rows of Oq / So"
    assert bool((Oq.t[:, d:] == 0xFF).all()), "bytes between the payload and ldoq"
    assert _scale_cols_intact(So, n_rows), "scale columns >= n_rows"
    # the separate quantiser
    q_sep, s_sep = ops.quant_mx8(O1.t)
    assert torch.equal(Oq.t[:, :d], q_sep), float((Oq.t[:, :d] != q_sep).float().mean())
    assert torch.equal(So.t[:, :n_rows], s_sep[:, :n_rows])
    # the host emulation
    q_emu, s_emu = mx8_quantize(O1.t.float().cpu())
    assert torch.equal(Oq.t[:, :d].cpu(), q_emu) and torch.equal(So.t[:, :n_rows].t().cpu(), s_emu)
    # the padded launch on the same data under the prefix mask: its valid rows
    kpm = (~vk).cuda().view(torch.uint8)
    Mp = B * Lq
    op, lsep = torch.empty(Mp, d, dtype=torch.bfloat16, device="cuda"), torch.empty(B, NH, Lq, dtype=torch.float32, device="cuda")
    oqp = torch.empty(Mp, d, dtype=torch.uint8, device="cuda")
    ldp = L_.hriemo_mx8_scale_ld(Mp)
    sop = torch.empty(d // 32, ldp, dtype=torch.uint8, device="cuda")
    _lib.call("hriemo_attn_fwd_q", P(q2), d, P(kv2), 2 * d, P(kv2[:, d:]), 2 * d, P(op), d, P(kpm), P(lsep), B, NH, Lq, Lk, hd, float(p), seed, sw,
              site, boff, None, P(oqp), d, P(sop), ldp, ST())
    assert torch.equal(O1.t[:nq_real], op.index_select(0, iq)), "O vs the padded launch"
    assert torch.equal(Oq.t[:nq_real, :d], oqp.index_select(0, iq)), "Oq vs the padded launch"
    assert torch.equal(So.t[:, :nq_real], sop.index_select(1, iq)), "So vs the padded launch"
    if filler:          # zero queries on zero keys / values: O = 0, whose quantised form is zero bytes with scale byte 0
        assert float(O1.t[nq_real:].float().abs().sum()) == 0.0
        assert int(Oq.t[nq_real:, :d].max()) == 0 and int(So.t[:, nq_real:n_rows].max()) == 0


def test_attention_packed_copy_is_refused_without_room(H):
    """the host check of the packed launch: ldso is held against n_rows (the packed row count the caller states)"""
    from hri_emo_amd import _lib, _ops as ops
    B, NH, L, hd = 2, 4, 16, 32
    d = NH * hd
    q = torch.zeros(20, 3 * d, dtype=torch.bfloat16, device="cuda")
    o, lse = torch.empty(20, d, dtype=torch.bfloat16, device="cuda"), torch.empty(B, NH, L, dtype=torch.float32, device="cuda")
    oq, so = torch.empty(20, d, dtype=torch.uint8, device="cuda"), torch.empty(d // 32, 256, dtype=torch.uint8, device="cuda")
    cu = _cu([16, 4])
    args = (P(q), 3 * d, P(q[:, d:]), 3 * d, P(q[:, 2 * d:]), 3 * d, P(o), d, P(cu), P(cu), P(lse), B, NH, L, L, hd, 0.0, 1, P(ops.seed_word(q.device)),
            0, 0, None, P(oq), d, P(so))
    with pytest.raises(RuntimeError):
        _lib.call("hriemo_attn_fwd_q_varlen", *args, 16, 20, ST())          # 16 scale columns for 20 packed rows
    _lib.call("hriemo_attn_fwd_q_varlen", *args, 256, 20, ST())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 2. wrapper
def _self_attn_site(ops, d, NH, lens, L, seed=5):
    g = torch.Generator().manual_seed(seed)
    Bn = len(lens)
    mask = (torch.arange(L)[None] >= torch.tensor(lens)[:, None]).cuda()
    seq = ops.seq_plan(mask, Bn, L)
    x = torch.randn(1, seq.N, d, generator=g).bfloat16().cuda()
    par = [t.cuda() for t in (torch.randn(3 * d, d, generator=g) / d ** 0.5, 0.1 * torch.randn(3 * d, generator=g),
                              torch.randn(d, d, generator=g) / d ** 0.5, 0.1 * torch.randn(d, generator=g),
                              1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g))]
    sh = ops.Shadows()

    def run():
        with torch.no_grad():
            return ops.SelfAttnLN.apply(x, None, *par, sh, NH, seq, 0.0, 11, 40, 0, False)
    return run, seq, mask


def _spy(monkeypatch, _lib):
    calls = []
    real = _lib.call

    def spy(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    return calls


def _between_attention_and_out_proj(names, attn):
    i = names.index(attn)
    j = next(k for k in range(i + 1, len(names)) if names[k].startswith("hriemo_gemm"))
    return names[i + 1:j], names[j]


def test_wrapper_takes_the_packed_entry_and_tags_o(H, monkeypatch):
    from hri_emo_amd import _lib, _ops as ops
    monkeypatch.setattr(ops, "MX_MIN_ROWS", 1)
    _mode(H, "mx_fp8", True, False)
    # ops.attn_fwd itself: a tagged o whose copy is the quantiser's
    NH, hd, L, lens = 8, 32, 40, [40, 7, 33]
    d = NH * hd
    cu = _cu(lens)
    n = sum(lens)
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(n, 3 * d, generator=g).bfloat16().cuda()
    o, lse = ops.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], 3, NH, L, L, hd, None, 0.0, 1, 2, 0, cu=(cu, cu))
    oq, so = ops.mx_of(o)
    q2, s2 = ops.quant_mx8(o)
    assert torch.equal(oq, q2) and torch.equal(so[:, :n], s2[:, :n])
    ops.ATTN_Q_VARLEN = False
    o0, lse0 = ops.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], 3, NH, L, L, hd, None, 0.0, 1, 2, 0, cu=(cu, cu))
    vq = (torch.arange(L)[None] < torch.tensor(lens)[:, None]).cuda()[:, None, :].expand(3, NH, L)          # lse keeps the padded indexing
    assert ops.mx_of(o0) is None and torch.equal(o0, o) and torch.equal(lse0[vq], lse[vq])
    ops.ATTN_Q_VARLEN = True

    # one packed SelfAttnLN forward: the launches between the attention and the out-projection GEMM
    run, seq, _ = _self_attn_site(ops, d, NH, lens, L)
    run()                                                  # warm-up: weight shadows
    calls = _spy(monkeypatch, _lib)
    y1 = run()[0]
    on = [c[0] for c in calls]
    del calls[:]
    ops.ATTN_Q_VARLEN = False
    y0 = run()[0]
    off = [c[0] for c in calls]
    assert "hriemo_attn_fwd_varlen" not in on
    gap, gemm = _between_attention_and_out_proj(on, "hriemo_attn_fwd_q_varlen")
    assert "hriemo_quant_mx8" not in gap and gemm == "hriemo_gemm_mx8", (gap, gemm)
    assert "hriemo_attn_fwd_q_varlen" not in off
    gap, gemm = _between_attention_and_out_proj(off, "hriemo_attn_fwd_varlen")
    assert gap == ["hriemo_quant_mx8"] and gemm == "hriemo_gemm_mx8", (gap, gemm)
    assert len(off) == len(on) + 1          # the parent's sequence is this one plus the quantiser launch
    assert torch.equal(y0, y1), "the two arms are bit-equal"

    # head dim 16: the plain packed launch
    ops.ATTN_Q_VARLEN = True
    run16, _, _ = _self_attn_site(ops, 128, 8, lens, L)
    run16()
    del calls[:]
    run16()
    n16 = [c[0] for c in calls]
    assert "hriemo_attn_fwd_varlen" in n16 and "hriemo_attn_fwd_q_varlen" not in n16


# ----------------------------------------------------------------------------- 3. fuse kernel
FB, FL = 5, 40
FLENS = [40, 1, 32, 1, 16]          # fused lengths: L, one-row samples, the 32-row chunk edge


@pytest.mark.parametrize("surplus", [0, 8])
@pytest.mark.parametrize("d", [128, 768, 1024])          # the NCH 1 and 2 arms; 768 = 96 chunks: lanes 32..63 of the second pass idle
def test_fuse_packed_leaves_the_quantised_memory(H, d, surplus):
    from hri_emo_amd import _lib, _ops as ops
    L_ = _lib.lib()
    g = torch.Generator().manual_seed(d + surplus)
    nf_real = sum(FLENS)
    Nf = nf_real + surplus
    cu_f = _cu(FLENS)

    def rows():
        x = torch.randn(Nf, d, generator=g) * torch.exp(2 * torch.randn(Nf, 1, generator=g))
        x[3, 32:64] = 0.0          # an all-zero block (in both operands)
        return x.bfloat16().cuda()

    A, T = rows(), rows()
    w = torch.sigmoid(torch.randn(FB, d, generator=g)).cuda()
    H0 = Guarded(Nf, d, torch.bfloat16)
    _lib.call("hriemo_fuse_fwd_packed", P(w), P(A), P(T), P(H0.t), P(cu_f), Nf, FB, FL, d, ST())
    lds = L_.hriemo_mx8_scale_ld(Nf)
    H1, Hq, Hs = Guarded(Nf, d, torch.bfloat16), Guarded(Nf, d, torch.uint8), Guarded(d // 32, lds, torch.uint8)
    _lib.call("hriemo_fuse_fwd_packed_q", P(w), P(A), P(T), P(H1.t), P(cu_f), Nf, FB, FL, d, P(Hq.t), P(Hs.t), lds, ST())
    torch.cuda.synchronize()
    assert torch.equal(H1.full.view(torch.uint8), H0.full.view(torch.uint8)), "H (and its guard rows)"
    assert H1.intact() and H1.written() and Hq.intact() and Hs.intact()
    assert _scale_cols_intact(Hs, Nf), "scale columns >= n_fused"
    q2, s2 = ops.quant_mx8(H1.t)
    assert torch.equal(Hq.t, q2), float((Hq.t != q2).float().mean())
    assert torch.equal(Hs.t[:, :Nf], s2[:, :Nf])
    q_emu, s_emu = mx8_quantize(H1.t.float().cpu())
    assert torch.equal(Hq.t.cpu(), q_emu) and torch.equal(Hs.t[:, :Nf].t().cpu(), s_emu)
    assert int(Hs.t[1, 3]) == 0 and int(Hq.t[3, 32:64].max()) == 0, "the all-zero block"
    if surplus:
        assert float(H1.t[nf_real:].float().abs().sum()) == 0.0
        assert int(Hq.t[nf_real:].max()) == 0 and int(Hs.t[:, nf_real:Nf].max()) == 0, "surplus rows: zero bytes, zero scale bytes"


# ----------------------------------------------------------------------------- 4. model against the oracle
def _ragged(B, Ta, Tt, d, seed):
    g = torch.Generator().manual_seed(seed)
    h_a, h_t = torch.randn(B, Ta, d, generator=g), torch.randn(B, Tt, d, generator=g)
    la = torch.randint(max(1, Ta // 2), Ta + 1, (B,), generator=g)
    lt = torch.randint(max(1, Tt // 2), Tt + 1, (B,), generator=g)
    la[0], lt[0] = Ta, Tt
    return h_a, h_t, torch.arange(Ta)[None] >= la[:, None], torch.arange(Tt)[None] >= lt[:, None]


def _err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


@pytest.mark.parametrize("B,Ta,Tt,d,ne", [(3, 100, 40, 768, 6), (4, 32, 16, 128, 4)])
def test_fusion_mx_fp8_packed_tail_vs_oracle_and_emulated_yardstick(H, monkeypatch, B, Ta, Tt, d, ne):
    """the three assertions of test_gpu_mx8.test_fusion_mx_fp8_vs_oracle_and_emulated_yardstick, on ragged prefix masks with the
    packed encoder and the packed fp8 tail"""
    from hri_emo_amd import _ops as ops
    monkeypatch.setattr(ops, "MX_MIN_ROWS", 1)
    torch.manual_seed(1234)
    kw = dict(d_model=d, num_emotions=ne, n_heads=8, dropout=0.1, num_layers_fusion=2, num_layers_decoder=2)
    ref = O.FusionWithEmotionDecoder(**kw).eval()
    m = H.FusionWithEmotionDecoder(**kw)
    m.load_state_dict(ref.state_dict())
    m.cuda().eval()
    h_a, h_t, m_a, m_t = _ragged(B, Ta, Tt, d, 5)
    with torch.no_grad():
        out32 = ref(h_a, h_t, m_a, m_t)
        O.LINEAR_OPERAND_HOOK = mx8_roundtrip
        try:
            out8 = ref(h_a, h_t, m_a, m_t)
        finally:
            O.LINEAR_OPERAND_HOOK = None
        _mode(H, "mx_fp8", True, True)
        assert ops.packed_tail()
        got = m(h_a.cuda(), h_t.cuda(), m_a.cuda(), m_t.cuda())
    for name, g8, r32, r8 in zip(("logits", "beta", "z"), got, out32, out8):
        yard = _err(r8, r32)
        e32, e8 = _err(g8, r32), _err(g8, r8)
        print(f"d={d} {name}: vs fp32 oracle {e32:.3e}, vs emulated-fp8 oracle {e8:.3e}, yardstick {yard:.3e}")
        assert e32 <= 6e-2, (name, "vs fp32 oracle", e32, "yardstick", yard)
        assert e32 <= max(1e-2, 2.5 * yard), (name, e32, yard)
        assert e8 <= max(1.5e-2, 1.5 * yard), (name, "vs emulated-fp8 oracle", e8, "yardstick", yard)


# ----------------------------------------------------------------------------- 5. tail on against tail off
SHAPES = {                      # d, N_e, B, T_a, T_t, audio lengths, text lengths
    "d128": (128, 4, 5, 70, 40, [70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),
    "d768": (768, 6, 3, 48, 20, [48, 10, 33], [20, 17, 5]),
    "d256": (256, 4, 5, 70, 40, [70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),          # head dim 32 (the launch test)
}


def _batch(name, seed=11):
    d, ne, nb, Ta, Tt, la, lt = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    h_a, h_t = torch.randn(nb, Ta, d, generator=g).cuda(), torch.randn(nb, Tt, d, generator=g).cuda()
    m_a = (torch.arange(Ta)[None] >= torch.tensor(la)[:, None]).cuda()
    m_t = (torch.arange(Tt)[None] >= torch.tensor(lt)[:, None]).cuda()
    y = (torch.rand(nb, ne, generator=g) < 0.3).float().cuda()
    return h_a, h_t, m_a, m_t, y


def _model(H, name, p):
    d, ne = SHAPES[name][:2]
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=p).cuda()


def _train_step(H, m, batch, tail, seed=None):
    from hri_emo_amd.train import fusion_step_loss
    _mode(H, "mx_fp8", True, tail)
    m.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)                    # the step's dropout seed comes from torch's generator
    logits, beta, z = m(*batch[:4])
    loss = fusion_step_loss(logits, beta, batch[4])
    loss.backward()
    return float(loss), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("name", ["d128", "d768"])
def test_packed_fp8_tail_equals_the_unpacked_tail(H, monkeypatch, name):
    """mx_fp8 + varlen, PACKED_TAIL_MX8 True against False (the parent's launches, the yardstick).  The forward operands of every
    GEMM row are bit-identical in both arms, so the bounds are the bf16 tail's (tests/test_gpu_packed_tail.py): 1e-5 of
    max(1, max|ref|) on the eval outputs, relative L2 1e-5 (dropout 0) / 1e-4 (dropout 0.1, one seed) on every parameter gradient.
    Measured on MI355X: the eval outputs are bit-equal (0.0) at both shapes; worst gradient 5.5e-8 (d128) / 1.5e-8 (d768) at
    dropout 0 and 5.1e-8 / 1.6e-8 at dropout 0.1, each time the second decoder layer's cross-attention in-projection weight -- the
    fp32 summation order of the K | V weight-gradient GEMM over N_f instead of B * L_t rows, as on the bf16 tail."""
    from hri_emo_amd import _ops as ops
    monkeypatch.setattr(ops, "MX_MIN_ROWS", 1)
    batch = _batch(name)
    m = _model(H, name, 0.1).eval()
    out = {}
    with torch.no_grad():
        for tail in (False, True):
            _mode(H, "mx_fp8", True, tail)
            assert ops.packed_tail() == tail
            out[tail] = [x.float().clone() for x in m(*batch[:4])]
    for a, b, what in zip(out[True], out[False], ("logits", "beta", "z")):
        err, bound = float((a - b).abs().max()), 1e-5 * max(1.0, float(b.abs().max()))
        print(f"{name} eval {what}: tail on vs off {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (what, err)
    for p, seed, bound in ((0.0, None, 1e-5), (0.1, 77, 1e-4)):
        m = _model(H, name, p).train()
        l0, g0 = _train_step(H, m, batch, False, seed)
        l1, g1 = _train_step(H, m, batch, True, seed)
        rels = {n: float((g1[n] - g0[n]).norm() / g0[n].norm().clamp_min(1e-20)) for n in g0}
        worst = max(rels, key=rels.get)
        print(f"{name} p={p}: loss {l0:.6f} / {l1:.6f}, worst relative L2 gradient difference {rels[worst]:.2e} ({worst})")
        assert abs(l0 - l1) <= 1e-5 * max(1.0, abs(l0)), (p, l0, l1)
        for n, rel in rels.items():
            assert rel <= bound, (p, n, rel)


# ----------------------------------------------------------------------------- 6. launches
def test_packed_fp8_tail_launches(H, monkeypatch):
    """one forward + backward under mx_fp8 + varlen (head dim 32: every attention site takes the fused quantiser).  Tail on: nothing
    is scattered back or gathered behind the encoder, the fuse kernel leaves the quantised memory (once), no quantiser launch reads
    that memory, and the decoder's memory K | V GEMMs run in fp8 over the N_f packed rows.  Tail off: the parent's launches."""
    from hri_emo_amd import _lib, _ops as ops
    monkeypatch.setattr(ops, "MX_MIN_ROWS", 1)
    name = "d256"
    d, _, nb, _, Tt, la, lt = SHAPES[name]
    n_f = sum(min(a, t) for a, t in zip(la, lt))
    assert n_f not in (sum(la), sum(lt), nb * Tt)
    batch = _batch(name)
    m = _model(H, name, 0.0).train()
    layers = len(m.emotion_decoder.layers)
    _train_step(H, m, batch, True)                   # warm-up: shadows, plans
    _train_step(H, m, batch, False)
    calls = _spy(monkeypatch, _lib)
    _train_step(H, m, batch, True)
    on = list(calls)
    del calls[:]
    _train_step(H, m, batch, False)
    off = list(calls)
    names, names_off = [c[0] for c in on], [c[0] for c in off]
    assert names.count("hriemo_unpack_rows") == 0 and names.count("hriemo_pack_rows") == 2
    assert names.count("hriemo_fuse_fwd_packed_q") == 1 and "hriemo_fuse_fwd_packed" not in names and "hriemo_fuse_fwd" not in names
    # hriemo_fuse_fwd_packed_q(w, A, T, H, cu_f, n_f, B, L, d, Hq, Hs, lds, stream)
    fuse = next(a for n, a in on if n == "hriemo_fuse_fwd_packed_q")
    assert fuse[5] == n_f
    # hriemo_quant_mx8(X, ldx, src_is_f32, M, K, ...): none reads H
    assert not any(n == "hriemo_quant_mx8" and (a[0] == fuse[3] or a[3] == n_f) for n, a in on), "a quantiser launch on the memory"
    # hriemo_gemm_mx8(M, N, K, Aq, ...): the K | V projections of the memory read the fuse kernel's bytes, N_f rows of them
    kv = [a for n, a in on if n.startswith("hriemo_gemm_mx8") and a[3] == fuse[9]]
    assert len(kv) == layers and all(a[:3] == (n_f, 2 * d, d) for a in kv), [a[:3] for a in kv]
    assert "hriemo_attn_fwd_varlen" not in names
    assert names.count("hriemo_attn_fwd_q_varlen") == names_off.count("hriemo_attn_fwd_q_varlen") + layers      # the decoder's cross-attentions

    assert names_off.count("hriemo_unpack_rows") == 2 and names_off.count("hriemo_pack_rows") == 4
    assert "hriemo_fuse_fwd" in names_off and not any("_packed" in n for n in names_off)
    assert len([a for n, a in off if n == "hriemo_quant_mx8" and a[3] == nb * Tt]) == 1, "the parent quantises the padded memory"
    kv_off = [a for n, a in off if n.startswith("hriemo_gemm_mx8") and a[:3] == (nb * Tt, 2 * d, d)]
    assert len(kv_off) == layers
    assert names_off.count("hriemo_quant_mx8") == names.count("hriemo_quant_mx8") + 1


# ----------------------------------------------------------------------------- 7. captured
def test_captured_bucket_graphs_run_the_packed_fp8_tail(H, monkeypatch):
    """DataParallelStep with bucket graphs under mx_fp8 and the packed tail: three batches in two buckets (two ragged batches with
    the same lengths, one all-full) against the eager tail-off step on the same batch (the bounds of the tail-on / tail-off test at
    dropout 0); a second replay of the first batch is bit-identical; as many graphs as the bf16 tail captures for these batches."""
    from test_gpu_varlen import _ragged_batch
    from hri_emo_amd import _ops as ops
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    monkeypatch.setattr(ops, "MX_MIN_ROWS", 1)
    nb, Ta, Tt, d = 4, 96, 40, 128

    def stepper():          # one model + DataParallelStep per capture (a capture bakes the mode in)
        torch.manual_seed(3)
        m = H.FusionWithEmotionDecoder(d_model=d, num_emotions=4, n_heads=8, dropout=0.0).cuda().train()
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(nb)
        return dp

    b0 = _ragged_batch(nb, Ta, Tt, d, 4, 4, 20, 5)[0]
    h_a, h_t, _, _, y = _ragged_batch(nb, Ta, Tt, d, 4, 9, 20, 5)[0]
    batches = [b0, _ragged_batch(nb, Ta, Tt, d, 4, 5, Ta, Tt)[0], (h_a, h_t, b0[2].clone(), b0[3].clone(), y)]

    def graphs_of(dp, gemm, bf16_tail, mx8_tail):
        H.set_gemm_mode(gemm)
        H.set_varlen(True)
        ops.PACKED_TAIL, ops.PACKED_TAIL_MX8 = bf16_tail, mx8_tail
        assert ops.packed_tail()
        dp.capture(*batches[0])
        res, keys = [], set()
        for batch in batches + [batches[0]]:
            loss = float(dp.step(*batch))
            torch.cuda.synchronize()
            keys.add(tuple(int(x) for x in (dp._pb.cu_a[-1], dp._pb.cu_t[-1])))
            res.append((loss, dp.buckets.flat.clone()))
        n = len(dp._pb.graphs)
        dp.release_graph()
        return res, keys, n

    _, keys16, n16 = graphs_of(stepper(), "bf16", True, False)
    ops.PACKED_TAIL = False
    dp = stepper()
    _mode(H, "mx_fp8", True, False)
    ref = []
    for batch in batches:                      # the eager tail-off step (the parent's path) is the yardstick
        ref.append((float(dp.step(*batch)), dp.buckets.flat.clone()))
    res, keys, n = graphs_of(dp, "mx_fp8", False, True)
    for i in range(3):
        loss, flat = res[i]
        rel = float((flat - ref[i][1]).norm() / ref[i][1].norm())
        print(f"batch {i}: loss {loss:.6f} vs {ref[i][0]:.6f}, flat gradients relative L2 {rel:.2e}")
        assert abs(loss - ref[i][0]) <= 1e-5 * max(1.0, abs(ref[i][0])), (i, loss, ref[i][0])
        assert rel <= 1e-5, (i, rel)
    assert res[3][0] == res[0][0] and torch.equal(res[3][1], res[0][1]), "a second replay of the first batch"
    assert n == len(keys) == 2 and (n, keys) == (n16, keys16)
