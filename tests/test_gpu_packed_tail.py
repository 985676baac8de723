"""GPU suite of the packed (varlen) tail: the gate and the decoder's memory on packed rows, with no unpack behind the encoder.

Kernel level (through the C ABI): the packed gate kernels must reproduce the padded kernels BIT FOR BIT on the valid rows -- a
block walks the positions the padded block walks, in the same order, and the only difference is that the padded launch also adds
the exact zeros of the PAD positions.  Every output lives in a 0xFF-filled buffer with guard rows around it.  Then the modules
(`_ops.PACKED_TAIL` True against False in one process, and against the reference's ragged goldens), the launches of a step, and
the captured bucket graphs."""
import pytest
import torch

from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu

B, LA, LT = 5, 70, 40
LENS_A = [70, 33, 32, 1, 17]
LENS_T = [40, 1, 32, 31, 16]
LENS_F = [40, 1, 32, 1, 16]          # min(la, lt): chunk edges 31 / 32 / 33 and 16 / 17, a one-row sample, la < lt, la > lt, la == lt
GUARD = 4


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    tail = _ops.PACKED_TAIL
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)
    _ops.PACKED_TAIL = tail


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """[rows, cols] output inside a 0xFF-filled allocation with GUARD rows in front and behind"""

    def __init__(self, rows, cols, dtype):
        self.full = torch.empty((rows + 2 * GUARD, cols), dtype=dtype, device="cuda")
        self.full.view(torch.uint8).fill_(0xFF)
        self.t = self.full[GUARD:GUARD + rows]

    def intact(self):
        g = torch.cat([self.full[:GUARD].reshape(-1).view(torch.uint8), self.full[-GUARD:].reshape(-1).view(torch.uint8)])
        return bool((g == 0xFF).all())

    def written(self):
        """no row of the body still holds the fill pattern"""
        return not bool((self.t.reshape(self.t.shape[0], -1).view(torch.uint8) == 0xFF).all(1).any())


def _cu(lens, tail=None):
    c = [0]
    for x in lens:
        c.append(c[-1] + x)
    if tail is not None:
        c.append(tail)
    return torch.tensor(c, dtype=torch.int32, device="cuda")


def _rows(lens, L):
    """padded row of every packed row"""
    return torch.cat([b * L + torch.arange(n) for b, n in enumerate(lens)]).cuda()


def _pack(x, lens, surplus, fill=0.0):
    """[B, L, ...] -> packed [sum(lens) + surplus, ...]; the surplus rows hold `fill`"""
    L = x.shape[1]
    flat = x.reshape((x.shape[0] * L,) + tuple(x.shape[2:]))
    p = flat.index_select(0, _rows(lens, L))
    if surplus:
        p = torch.cat([p, torch.full((surplus,) + tuple(p.shape[1:]), fill, dtype=p.dtype, device=p.device)])
    return p.contiguous()


@pytest.mark.parametrize("surplus", [0, 8])
@pytest.mark.parametrize("d", [128, 768])          # the NCH 1 and 2 arms
def test_packed_gate_kernels_equal_padded_bit_for_bit(H, d, surplus):
    """hriemo_ln_pool_fwd_packed(_pair) / hriemo_fuse_fwd_packed / hriemo_fuse_bwd_dw_packed / hriemo_ln_pool_bwd_packed(_pair)
    against hriemo_ln_pool_fwd / hriemo_fuse_fwd / hriemo_fuse_bwd_dw / hriemo_ln_pool_bwd on the padded layout whose PAD
    positions hold the zeros hriemo_unpack_rows writes.  torch.equal throughout (it compares values, so a signed zero in a sum of
    exact zeros would not matter)."""
    from hri_emo_amd import _lib
    L_ = _lib.lib()
    g = torch.Generator().manual_seed(100 + d + surplus)
    va = (torch.arange(LA)[None] < torch.tensor(LENS_A)[:, None])
    vt = (torch.arange(LT)[None] < torch.tensor(LENS_T)[:, None])
    vf = (torch.arange(LT)[None] < torch.tensor(LENS_F)[:, None])
    xa32 = ((torch.randn(B, LA, d, generator=g) * 1.3 + 0.2) * va[..., None]).cuda()
    xt32 = (torch.randn(B, LT, d, generator=g) * vt[..., None]).cuda()
    xa16, xt16 = xa32.bfloat16(), xt32.bfloat16()
    ga, ba = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.1 * torch.randn(d, generator=g)).cuda()
    gt, bt = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.1 * torch.randn(d, generator=g)).cuda()
    w = torch.sigmoid(torch.randn(B, d, generator=g)).cuda()
    dH = (torch.randn(B, LT, d, generator=g) * vf[..., None]).bfloat16().cuda()          # dH = 0 for l >= lf[b]
    da, dt = torch.randn(B, d, generator=g).cuda(), torch.randn(B, d, generator=g).cuda()
    ma, mt = (~va).cuda().view(torch.uint8), (~vt).cuda().view(torch.uint8)
    nca, nct, ncf = (L_.hriemo_pool_chunks(x) for x in (LA, LT, LT))
    f32 = dict(dtype=torch.float32, device="cuda")
    bf = dict(dtype=torch.bfloat16, device="cuda")

    # ---------------- the padded kernels (the reference of this test)
    An, Tn, Hp = torch.empty(B, LT, d, **bf), torch.empty(B, LT, d, **bf), torch.empty(B, LT, d, **bf)
    mean_a, rstd_a, mean_t, rstd_t = torch.empty(B * LA, **f32), torch.empty(B * LA, **f32), torch.empty(B * LT, **f32), torch.empty(B * LT, **f32)
    pa, pt = torch.empty(B, nca, d, **f32), torch.empty(B, nct, d, **f32)
    _lib.call("hriemo_ln_pool_fwd", P(xa16), P(xa32), P(ma), P(ga), P(ba), P(An), P(mean_a), P(rstd_a), P(pa), B, LA, LT, d, 1e-5, ST())
    _lib.call("hriemo_ln_pool_fwd", P(xt16), P(xt32), P(mt), P(gt), P(bt), P(Tn), P(mean_t), P(rstd_t), P(pt), B, LT, LT, d, 1e-5, ST())
    _lib.call("hriemo_fuse_fwd", P(w), P(An), P(Tn), P(Hp), B, LT, d, ST())
    part = torch.empty(B, ncf, d, **f32)
    _lib.call("hriemo_fuse_bwd_dw", P(dH), P(An), P(Tn), P(part), B, LT, d, ST())
    dxa, dxt = torch.empty(B, LA, d, **bf), torch.empty(B, LT, d, **bf)
    dga, dba, dgt, dbt = (torch.empty(d, **f32) for _ in range(4))
    wsa = torch.empty(L_.hriemo_ln_pool_bwd_workspace_bytes(B, LA, d) // 4, **f32)
    wst = torch.empty(L_.hriemo_ln_pool_bwd_workspace_bytes(B, LT, d) // 4, **f32)
    _lib.call("hriemo_ln_pool_bwd", P(dH), LT, P(w), 1, P(da), P(ma), P(xa16), P(xa32), P(ga), P(mean_a), P(rstd_a), P(dxa), P(dga), P(dba),
              0, B, LA, d, P(wsa), ST())
    _lib.call("hriemo_ln_pool_bwd", P(dH), LT, P(w), 0, P(dt), P(mt), P(xt16), P(xt32), P(gt), P(mean_t), P(rstd_t), P(dxt), P(dgt), P(dbt),
              0, B, LT, d, P(wst), ST())

    # ---------------- the packed operands: exact fit, or 8 surplus rows in every packed buffer
    Na, Nt, Nf = sum(LENS_A) + surplus, sum(LENS_T) + surplus, sum(LENS_F) + surplus
    nseq = B + 1 if surplus else B
    cu_a, cu_t, cu_f = _cu(LENS_A, Na if surplus else None), _cu(LENS_T, Nt if surplus else None), _cu(LENS_F)
    ia, it, i_f = _rows(LENS_A, LA), _rows(LENS_T, LT), _rows(LENS_F, LT)
    xa16p, xa32p, xt16p, xt32p = _pack(xa16, LENS_A, surplus), _pack(xa32, LENS_A, surplus), _pack(xt16, LENS_T, surplus), _pack(xt32, LENS_T, surplus)
    dHp = _pack(dH, LENS_F, surplus, fill=float("nan"))          # nothing may read the surplus rows of dH
    na_real, nt_real, nf_real = sum(LENS_A), sum(LENS_T), sum(LENS_F)

    def forward(pair):
        o = dict(An=Guarded(Nf, d, torch.bfloat16), Tn=Guarded(Nf, d, torch.bfloat16), mean_a=Guarded(Na, 1, torch.float32),
                 rstd_a=Guarded(Na, 1, torch.float32), mean_t=Guarded(Nt, 1, torch.float32), rstd_t=Guarded(Nt, 1, torch.float32),
                 pa=Guarded(B * nca, d, torch.float32), pt=Guarded(B * nct, d, torch.float32))
        if pair:
            _lib.call("hriemo_ln_pool_fwd_packed_pair",
                      P(xa16p), P(xa32p), P(cu_a), nseq, Na, P(ga), P(ba), P(o["An"].t), P(o["mean_a"].t), P(o["rstd_a"].t), P(o["pa"].t), LA,
                      P(xt16p), P(xt32p), P(cu_t), nseq, Nt, P(gt), P(bt), P(o["Tn"].t), P(o["mean_t"].t), P(o["rstd_t"].t), P(o["pt"].t), LT,
                      P(cu_f), Nf, B, d, 1e-5, ST())
        else:
            _lib.call("hriemo_ln_pool_fwd_packed", P(xa16p), P(xa32p), P(cu_a), nseq, Na, P(ga), P(ba), P(o["An"].t), P(o["mean_a"].t),
                      P(o["rstd_a"].t), P(o["pa"].t), LA, P(cu_f), Nf, B, d, 1e-5, ST())
            _lib.call("hriemo_ln_pool_fwd_packed", P(xt16p), P(xt32p), P(cu_t), nseq, Nt, P(gt), P(bt), P(o["Tn"].t), P(o["mean_t"].t),
                      P(o["rstd_t"].t), P(o["pt"].t), LT, P(cu_f), Nf, B, d, 1e-5, ST())
        return o

    fw = forward(False)
    for k, v in fw.items():
        assert v.intact(), ("guard rows", k)
        assert v.written(), ("every row is written", k)
    assert torch.equal(fw["An"].t[:nf_real], An.view(B * LT, d)[i_f]), "Yn audio"
    assert torch.equal(fw["Tn"].t[:nf_real], Tn.view(B * LT, d)[i_f]), "Yn text"
    assert torch.equal(fw["mean_a"].t[:na_real, 0], mean_a[ia]) and torch.equal(fw["rstd_a"].t[:na_real, 0], rstd_a[ia])
    assert torch.equal(fw["mean_t"].t[:nt_real, 0], mean_t[it]) and torch.equal(fw["rstd_t"].t[:nt_real, 0], rstd_t[it])
    assert torch.equal(fw["pa"].t, pa.view(B * nca, d)), "pooled partials audio"
    assert torch.equal(fw["pt"].t, pt.view(B * nct, d)), "pooled partials text"
    assert float(fw["An"].t[nf_real:].float().abs().sum()) == 0.0 and float(fw["Tn"].t[nf_real:].float().abs().sum()) == 0.0, "surplus rows of Yn"
    fwp = forward(True)
    for k in fw:
        assert torch.equal(fwp[k].full.view(torch.uint8), fw[k].full.view(torch.uint8)), ("pair launch == single launches", k)

    Hk = Guarded(Nf, d, torch.bfloat16)
    _lib.call("hriemo_fuse_fwd_packed", P(w), P(fw["An"].t), P(fw["Tn"].t), P(Hk.t), P(cu_f), Nf, B, LT, d, ST())
    assert Hk.intact() and Hk.written()
    assert torch.equal(Hk.t[:nf_real], Hp.view(B * LT, d)[i_f]), "H"
    assert float(Hk.t[nf_real:].float().abs().sum()) == 0.0, "surplus rows of H"

    partk = Guarded(B * ncf, d, torch.float32)
    _lib.call("hriemo_fuse_bwd_dw_packed", P(dHp), P(fw["An"].t), P(fw["Tn"].t), P(partk.t), P(cu_f), Nf, B, LT, d, ST())
    assert partk.intact() and partk.written()
    assert torch.equal(partk.t, part.view(B * ncf, d)), "dw partials"

    def backward(pair):
        o = dict(dxa=Guarded(Na, d, torch.bfloat16), dxt=Guarded(Nt, d, torch.bfloat16), dga=Guarded(1, d, torch.float32),
                 dba=Guarded(1, d, torch.float32), dgt=Guarded(1, d, torch.float32), dbt=Guarded(1, d, torch.float32))
        wa, wt = torch.empty_like(wsa), torch.empty_like(wst)
        if pair:
            _lib.call("hriemo_ln_pool_bwd_packed_pair", P(dHp), P(cu_f), Nf, P(w),
                      P(da), P(xa16p), P(xa32p), P(cu_a), nseq, Na, P(ga), P(fw["mean_a"].t), P(fw["rstd_a"].t), P(o["dxa"].t), P(o["dga"].t),
                      P(o["dba"].t), LA, P(wa),
                      P(dt), P(xt16p), P(xt32p), P(cu_t), nseq, Nt, P(gt), P(fw["mean_t"].t), P(fw["rstd_t"].t), P(o["dxt"].t), P(o["dgt"].t),
                      P(o["dbt"].t), LT, P(wt), 0, B, d, ST())
        else:
            _lib.call("hriemo_ln_pool_bwd_packed", P(dHp), P(cu_f), Nf, P(w), 1, P(da), P(xa16p), P(xa32p), P(cu_a), nseq, Na, P(ga),
                      P(fw["mean_a"].t), P(fw["rstd_a"].t), P(o["dxa"].t), P(o["dga"].t), P(o["dba"].t), 0, B, LA, d, P(wa), ST())
            _lib.call("hriemo_ln_pool_bwd_packed", P(dHp), P(cu_f), Nf, P(w), 0, P(dt), P(xt16p), P(xt32p), P(cu_t), nseq, Nt, P(gt),
                      P(fw["mean_t"].t), P(fw["rstd_t"].t), P(o["dxt"].t), P(o["dgt"].t), P(o["dbt"].t), 0, B, LT, d, P(wt), ST())
        return o

    bw = backward(False)
    for k, v in bw.items():
        assert v.intact(), ("guard rows", k)
        assert v.written(), ("every row is written", k)
    assert torch.equal(bw["dxa"].t[:na_real], dxa.view(B * LA, d)[ia]), "dX audio"
    assert torch.equal(bw["dxt"].t[:nt_real], dxt.view(B * LT, d)[it]), "dX text"
    assert float(bw["dxa"].t[na_real:].float().abs().sum()) == 0.0 and float(bw["dxt"].t[nt_real:].float().abs().sum()) == 0.0, "surplus rows of dX"
    for k, ref in (("dga", dga), ("dba", dba), ("dgt", dgt), ("dbt", dbt)):
        assert torch.equal(bw[k].t[0], ref), k          # the packed partial sums leave out exact zeros only
    bwp = backward(True)
    for k in bw:
        assert torch.equal(bwp[k].full.view(torch.uint8), bw[k].full.view(torch.uint8)), ("pair launch == single launches", k)
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("hd", [16, 96])
def test_attention_varlen_at_the_decoder_shape(H, hd, p):
    """hriemo_attn_{fwd,bwd}_varlen with cu_seqlens_q != cu_seqlens_k: N_e = 6 queries for every sample, the fused memory's
    lf[b] keys -- against the padded call with the fused key padding mask (what the decoder ran before)."""
    from hri_emo_amd import _ops as ops
    NH, Lq, Lk = 8, 6, LT
    d = NH * hd
    g = torch.Generator().manual_seed(31 + hd)
    lk = torch.tensor(LENS_F)
    q2 = (torch.randn(B * Lq, d, generator=g) * 1.5).bfloat16().cuda()
    kv2 = torch.randn(B * Lk, 2 * d, generator=g).bfloat16().cuda()
    do2 = torch.randn(B * Lq, d, generator=g).bfloat16().cuda()
    vk = (torch.arange(Lk)[None] < lk[:, None]).cuda()
    kpm = (~vk).view(torch.uint8)
    seed, site, boff = 13579, 7, 2
    o, lse, mb = ops.attn_fwd(q2, kv2[:, :d], kv2[:, d:], B, NH, Lq, Lk, hd, kpm, p, seed, site, boff, want_bits=True)
    dq, dkv = torch.empty_like(q2), torch.empty_like(kv2)
    ops.attn_bwd(q2, kv2[:, :d], kv2[:, d:], o, do2, dq, dkv[:, :d], dkv[:, d:], lse, B, NH, Lq, Lk, hd, kpm, p, seed, site, boff, mask_bits=mb)
    ik = vk.reshape(-1).nonzero().reshape(-1)
    cq = torch.arange(B + 1, dtype=torch.int32, device="cuda") * Lq
    ck = _cu(LENS_F)
    kvp = kv2.index_select(0, ik).contiguous()
    for use_bits in (True, False):
        Og, dQg, dKVg = Guarded(B * Lq, d, torch.bfloat16), Guarded(B * Lq, d, torch.bfloat16), Guarded(int(lk.sum()), 2 * d, torch.bfloat16)
        lsep = torch.empty((B, NH, Lq), dtype=torch.float32, device="cuda")
        mbp = None
        if mb is not None:
            mbp = torch.empty_like(mb)
        from hri_emo_amd import _lib
        _lib.call("hriemo_attn_fwd_varlen", P(q2), d, P(kvp), 2 * d, P(kvp[:, d:]), 2 * d, P(Og.t), d, P(cq), P(ck), P(lsep), B, NH, Lq, Lk, hd,
                  float(p), seed, P(ops.seed_word(q2.device)), site, boff, P(mbp), ST())
        ops.attn_bwd(q2, kvp[:, :d], kvp[:, d:], Og.t, do2, dQg.t, dKVg.t[:, :d], dKVg.t[:, d:], lsep, B, NH, Lq, Lk, hd, None, p, seed, site, boff,
                     mask_bits=mbp if use_bits else None, cu=(cq, ck))
        assert Og.intact() and dQg.intact() and dKVg.intact()
        assert torch.equal(Og.t, o), "O"
        assert torch.equal(lsep, lse), "lse"
        assert torch.equal(dQg.t, dq), ("dQ", use_bits)
        assert torch.equal(dKVg.t, dkv.index_select(0, ik)), ("dK|dV", use_bits)
    assert float(dkv.float()[(~vk).reshape(-1)].abs().max()) == 0.0          # masked keys of the padded side: exact zeros


# ----------------------------------------------------------------------------- model level
SHAPES = {                      # d, N_e, B, T_a, T_t, audio lengths, text lengths
    "d128": (128, 4, B, LA, LT, LENS_A, LENS_T),
    "d768": (768, 6, 3, 48, 20, [48, 10, 33], [20, 17, 5]),          # the hd96 fixture's shape; sample 1 has la < lt
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


def _mode(H, varlen, tail):
    from hri_emo_amd import _ops
    H.set_varlen(varlen)
    _ops.PACKED_TAIL = tail


MODES = (("padded", False, False), ("unpacked tail", True, False), ("packed tail", True, True))


@pytest.mark.parametrize("name", list(SHAPES))
def test_eval_packed_tail_equals_padded(H, name):
    """logits, beta, z of the packed tail against the padded path and against the packed encoder with the tail unpacked"""
    m = _model(H, name, 0.1).eval()
    h_a, h_t, m_a, m_t, _ = _batch(name)
    out = {}
    with torch.no_grad():
        for what, varlen, tail in MODES:
            _mode(H, varlen, tail)
            out[what] = [x.float().clone() for x in m(h_a, h_t, m_a, m_t)]
    for other in ("padded", "unpacked tail"):
        for a, b, what in zip(out["packed tail"], out[other], ("logits", "beta", "z")):
            err, bound = float((a - b).abs().max()), 1e-5 * max(1.0, float(b.abs().max()))
            print(f"{name} {what} packed tail vs {other}: {err:.3e} (bound {bound:.1e})")
            assert err <= bound, (what, other, err)


@pytest.mark.parametrize("gname,d,ne", [("cfg1_eval_ragged", 128, 4), ("hd96_eval_ragged", 768, 6)])
def test_eval_packed_tail_holds_the_goldens(H, gname, d, ne):
    """the reference's ragged fixtures through the packed tail: the bound of test_fusion_eval_varlen_equals_padded_and_golden"""
    from hri_emo_amd import _ops
    g = load_golden(gname)
    m = O.closed_form_init_(H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=0.1)).cuda().eval()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    with torch.no_grad():
        _mode(H, False, False)
        ref = m(*args)
        _mode(H, True, True)
        got = m(*args)
    assert _ops.seq_plans(args[2], args[3], args[0].shape[0], args[0].shape[1], args[1].shape[1]) is not None
    for a, b, what in zip(got, ref, ("logits", "beta", "z")):
        assert float((a.float() - b.float()).abs().max()) <= 1e-5 * max(1.0, float(b.float().abs().max())), what
        r = g[what]
        assert float((a.float().cpu() - r).abs().max()) <= 5e-3 * max(1.0, float(r.abs().max())), what


def _train_step(H, m, batch, varlen, tail, seed=None):
    from hri_emo_amd.train import fusion_step_loss
    _mode(H, varlen, tail)
    m.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)                    # the step's dropout seed comes from torch's generator
    logits, beta, z = m(*batch[:4])
    loss = fusion_step_loss(logits, beta, batch[4])
    loss.backward()
    return float(loss), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_train_step_packed_tail_equals_padded(H, name):
    """loss and every parameter gradient: relative L2 1e-5 at dropout 0, 1e-4 at dropout 0.1 with one seed (the bounds of
    tests/test_gpu_varlen.py; measured there 1.2e-7, the fp32 summation order of the weight-gradient GEMMs)"""
    batch = _batch(name)
    for p, seed, bound in ((0.0, None, 1e-5), (0.1, 77, 1e-4)):
        m = _model(H, name, p).train()
        l0, g0 = _train_step(H, m, batch, False, False, seed)
        l1, g1 = _train_step(H, m, batch, True, True, seed)
        worst = max(float((g1[n] - g0[n]).norm() / g0[n].norm().clamp_min(1e-20)) for n in g0)
        print(f"{name} p={p}: loss {l0:.6f} / {l1:.6f}, worst relative L2 gradient difference {worst:.2e}")
        assert abs(l0 - l1) <= 1e-5 * max(1.0, abs(l0)), (p, l0, l1)
        for n in g0:
            rel = float((g1[n] - g0[n]).norm() / g0[n].norm().clamp_min(1e-20))
            assert rel <= bound, (p, n, rel)


def test_packed_tail_launches(H, monkeypatch):
    """a spy on _lib.call: with the packed tail one forward + backward scatters nothing back (no hriemo_unpack_rows), gathers only
    the two inputs, and runs the packed gate entries; with it off the tail's two unpack launches (forward) and the two pack
    launches of their backward are there again, beside the two input packs."""
    from hri_emo_amd import _lib
    batch = _batch("d128")
    m = _model(H, "d128", 0.0).train()
    _train_step(H, m, batch, True, True)             # warm-up: shadows, plans
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    _train_step(H, m, batch, True, True)
    on = list(names)
    del names[:]
    _train_step(H, m, batch, True, False)
    off = list(names)
    assert on.count("hriemo_unpack_rows") == 0 and on.count("hriemo_pack_rows") == 2, (on.count("hriemo_unpack_rows"), on.count("hriemo_pack_rows"))
    assert any(n in on for n in ("hriemo_ln_pool_fwd_packed_pair", "hriemo_ln_pool_fwd_packed"))
    assert any(n in on for n in ("hriemo_ln_pool_bwd_packed_pair", "hriemo_ln_pool_bwd_packed"))
    assert "hriemo_fuse_fwd_packed" in on and "hriemo_fuse_bwd_dw_packed" in on
    assert not any(n in on for n in ("hriemo_ln_pool_fwd", "hriemo_ln_pool_fwd_pair", "hriemo_fuse_fwd", "hriemo_ln_pool_bwd", "hriemo_ln_pool_bwd_pair"))
    assert off.count("hriemo_unpack_rows") == 2 and off.count("hriemo_pack_rows") == 4, (off.count("hriemo_unpack_rows"), off.count("hriemo_pack_rows"))
    assert not any(n.endswith("_packed") or n.endswith("_packed_pair") for n in off)
    assert on.count("hriemo_attn_fwd_varlen") == off.count("hriemo_attn_fwd_varlen") + len(m.emotion_decoder.layers)      # the decoder's cross-attentions


# ----------------------------------------------------------------------------- captured
def test_captured_bucket_graphs_run_the_packed_tail(H):
    """DataParallelStep with bucket graphs: a ragged, an all-full and an all-one batch (three buckets) against the eager padded
    step; a second replay of the first batch is bit-identical to its first; the fused plan rides in the text bucket, so there
    is one graph per distinct (audio rows, text rows) key."""
    from test_gpu_varlen import _ragged_batch
    from hri_emo_amd import _ops
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    torch.manual_seed(3)
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.0).cuda().train()
    nb, Ta, Tt, d = 4, 96, 40, 128
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    dp.set_global_batch(nb)
    batches = [_ragged_batch(nb, Ta, Tt, d, 4, 4, 20, 5)[0], _ragged_batch(nb, Ta, Tt, d, 4, 5, Ta, Tt)[0]]
    h_a, h_t, _, _, y = _ragged_batch(nb, Ta, Tt, d, 4, 6, 1, 1)[0]
    one = torch.arange(Ta, device="cuda")[None].expand(nb, Ta) >= 1
    batches.append((h_a, h_t, one.contiguous(), one[:, :Tt].contiguous(), y))
    assert bool((~batches[1][2]).all()) and bool((~batches[1][3]).all())          # all-full
    _mode(H, False, False)
    ref = []
    for batch in batches:                      # the padded eager step is the yardstick
        ref.append((float(dp.step(*batch)), dp.buckets.flat.clone()))
    _mode(H, True, True)
    dp.capture(*batches[0])
    keys, first = set(), None
    for i, batch in enumerate(batches):
        loss = float(dp.step(*batch))
        torch.cuda.synchronize()
        keys.add(tuple(int(x) for x in (dp._pb.cu_a[-1], dp._pb.cu_t[-1])))
        assert int(dp._pb.cu_f[-1]) == int(dp._pb.cu_t[-1])
        rel = float((dp.buckets.flat - ref[i][1]).norm() / ref[i][1].norm())
        print(f"batch {i}: loss {loss:.6f} vs {ref[i][0]:.6f}, flat gradients relative L2 {rel:.2e}")
        assert abs(loss - ref[i][0]) <= 1e-5 * max(1.0, abs(ref[i][0])), (i, loss, ref[i][0])
        assert rel <= 1e-5, (i, rel)
        if i == 0:
            first = (loss, dp.buckets.flat.clone())
    loss = float(dp.step(*batches[0]))
    torch.cuda.synchronize()
    assert loss == first[0] and torch.equal(dp.buckets.flat, first[1]), "a second replay of the first batch"
    assert len(dp._pb.graphs) == len(keys) == 3
    dp.release_graph()
