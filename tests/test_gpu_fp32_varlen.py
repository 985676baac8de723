"""GPU suite of the fp32 precision mode on packed (varlen) sequences: with set_precision("fp32") and set_varlen(True) the TACFN
encoder runs on the valid rows only (hriemo_attn_*_f32_varlen with cu_seqlens, hriemo_add_ln_*_f32_rows, the six-product Linear on
[N_valid, d]).  Kernels first (against the padded fp32 kernels and float64), then the switch itself, the modules on the ragged
golden fixtures, a training step's gradients and the captured DataParallelStep."""
import math

import pytest
import torch

from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu
TOL = 1e-4               # outputs against the goldens: the bound of tests/test_gpu_fp32_mode.py
GRAD_TOL = 1e-3          # gradients against the fp32 oracle, relative L2 per parameter (tests/test_gpu_fp32_mode.py)


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    # captured replays bump the device seed word and the dropout tests set it: later test files replay the hash from its value
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    hri_emo_amd.set_precision("fp32")
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_precision("bf16")
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    torch.cuda.synchronize()


def cu(t):
    return None if t is None else t.cuda()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def _word():
    from hri_emo_amd import _ops
    return int(_ops.seed_word(torch.device("cuda", 0)).item()) & ((1 << 64) - 1)


def _cu_of(lens, extra=None):
    c = [0]
    for x in lens:
        c.append(c[-1] + int(x))
    if extra is not None:
        c.append(c[-1] + extra)
    return torch.tensor(c, dtype=torch.int32).cuda()


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,H_,Lq,Lk,hd,p,bucket", [(5, 8, 100, 40, 96, 0.1, False), (4, 4, 128, 128, 64, 0.0, False),
                                                    (3, 8, 50, 200, 128, 0.1, False), (6, 2, 70, 70, 32, 0.1, True),
                                                    (4, 8, 6, 77, 96, 0.0, True), (3, 2, 130, 65, 32, 0.0, False)])
def test_attention_f32_varlen_equals_padded_and_float64(H, B, H_, Lq, Lk, hd, p, bucket):
    """packed fp32 attention forward and backward (O, LSE, dQ, dK, dV) on ragged lengths -- a one-row sample, a full-length one,
    Lq != Lk, and the bucketed form dp.py captures (B + 1 sequences, the last one made of surplus rows) -- equals the padded fp32
    kernels on every valid row, and both equal float64 under the dropout keep-mask the hash defines for the PADDED indices"""
    import hashrng
    from hri_emo_amd import _fp32
    g = torch.Generator().manual_seed(Lq * 5 + Lk + hd)
    d = H_ * hd
    lq = torch.randint(1, Lq + 1, (B,), generator=g); lk = torch.randint(1, Lk + 1, (B,), generator=g)
    lq[0], lk[0] = Lq, Lk
    lq[1], lk[1] = 1, 1
    q = torch.randn(B, Lq, d, generator=g) * 1.5
    kv = torch.randn(B, Lk, 2 * d, generator=g)
    do = torch.randn(B, Lq, d, generator=g)
    vq = torch.arange(Lq)[None] < lq[:, None]; vk = torch.arange(Lk)[None] < lk[:, None]
    do = do * vq[:, :, None]                        # PAD query rows carry no gradient in the model
    kpm = (~vk).cuda().view(torch.uint8)
    seed, site, boff = 424242, 16, 2
    drop = (p, seed, site, boff) if p > 0 else None
    q2, kv2, do2 = q.view(B * Lq, d).cuda(), kv.view(B * Lk, 2 * d).cuda(), do.view(B * Lq, d).cuda()
    o, lse = _fp32.attn(q2, kv2[:, :d], kv2[:, d:], B, H_, Lq, Lk, hd, kpm, want_lse=True, drop=drop)
    dq = torch.empty_like(q2); dkv = torch.empty_like(kv2)
    _fp32.attn_bwd(q2, kv2[:, :d], kv2[:, d:], o, do2, lse, dq, dkv[:, :d], dkv[:, d:], B, H_, Lq, Lk, hd, kpm, drop=drop)
    # packed operands (with the bucket's surplus sequence: random rows, its own sequence, never read by a real one)
    iq, ik = vq.reshape(-1).nonzero().reshape(-1).cuda(), vk.reshape(-1).nonzero().reshape(-1).cuda()
    qp, kvp, dop = q2.index_select(0, iq), kv2.index_select(0, ik), do2.index_select(0, iq)
    AB, ALq, ALk = B, int(lq.max()), int(lk.max())
    sq = sk = None
    if bucket:
        sq, sk = min(Lq, 9), min(Lk, 13)
        qp = torch.cat([qp, torch.randn(sq, d, generator=g).cuda()])
        kvp = torch.cat([kvp, torch.randn(sk, 2 * d, generator=g).cuda()])
        dop = torch.cat([dop, torch.zeros(sq, d).cuda()])
        AB, ALq, ALk = B + 1, Lq, Lk                # the bucketed Seq: Lmax = the padded length
    qp, kvp, dop = qp.contiguous(), kvp.contiguous(), dop.contiguous()
    cuq, cuk = _cu_of(lq.tolist(), sq), _cu_of(lk.tolist(), sk)
    op, lsep = _fp32.attn(qp, kvp[:, :d], kvp[:, d:], AB, H_, ALq, ALk, hd, None, want_lse=True, drop=drop, cu=(cuq, cuk))
    dqp = torch.empty_like(qp); dkvp = torch.empty_like(kvp)
    _fp32.attn_bwd(qp, kvp[:, :d], kvp[:, d:], op, dop, lsep, dqp, dkvp[:, :d], dkvp[:, d:], AB, H_, ALq, ALk, hd, None, drop=drop,
                   cu=(cuq, cuk))
    nq, nk = int(lq.sum()), int(lk.sum())
    assert bool(torch.isfinite(op).all()) and bool(torch.isfinite(dqp).all()) and bool(torch.isfinite(dkvp).all())
    # == the padded kernels on every valid row (same tiles, same order: PAD keys only add exact zeros there)
    for got, ref, what in ((op[:nq], o.index_select(0, iq), "O"), (dqp[:nq], dq.index_select(0, iq), "dQ"),
                           (dkvp[:nk], dkv.index_select(0, ik), "dK|dV")):
        assert _maxrel(got, ref) <= 1e-6, (what, _maxrel(got, ref))
    for b in range(B):
        n = int(lq[b])
        assert _maxrel(lsep[b, :, :n], lse[b, :, :n]) <= 1e-6, ("lse", b)
    # float64 under the hash's keep-mask of the padded (batch, query, key) indices
    q4 = q.double().view(B, Lq, H_, hd).transpose(1, 2).detach().requires_grad_(True)
    k4 = kv[:, :, :d].double().reshape(B, Lk, H_, hd).transpose(1, 2).detach().requires_grad_(True)
    v4 = kv[:, :, d:].double().reshape(B, Lk, H_, hd).transpose(1, 2).detach().requires_grad_(True)
    s = (q4 @ k4.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~vk[:, None, None, :], float("-inf"))
    pr = torch.softmax(s, -1)
    if p > 0:
        keep = hashrng.attn_mask((seed + _word()) & ((1 << 64) - 1), site, B, H_, Lq, Lk, p, boff)
        pr = pr * torch.from_numpy(keep).double() * hashrng.inv_keep(p)
    ref = (pr @ v4).transpose(1, 2).reshape(B, Lq, d)
    ref.backward(do.double())
    ref_o = ref.detach().reshape(B * Lq, d)[vq.reshape(-1)]
    assert _maxrel(op[:nq], ref_o) <= 2e-5, ("O vs float64", _maxrel(op[:nq], ref_o))

    def back(t, L):
        return t.transpose(1, 2).reshape(B * L, d)

    vqf, vkf = vq.reshape(-1), vk.reshape(-1)
    for got, r, what in ((dqp[:nq], back(q4.grad, Lq)[vqf], "dQ"), (dkvp[:nk, :d], back(k4.grad, Lk)[vkf], "dK"),
                         (dkvp[:nk, d:], back(v4.grad, Lk)[vkf], "dV")):
        err = float((got.double().cpu() - r).abs().max() / r.abs().max())
        assert err <= 2e-5, (what, err)


@pytest.mark.parametrize("B,L,d,p,row_off", [(6, 50, 768, 0.1, 0), (4, 33, 128, 0.5, 700), (3, 20, 1024, 0.25, 7)])
def test_add_ln_f32_rows_equals_add_ln_f32_at_the_same_rows(H, B, L, d, p, row_off):
    """hriemo_add_ln_f32_rows / hriemo_add_ln_bwd_f32_rows on gathered rows equal hriemo_add_ln_f32 / _bwd_f32 at the same padded
    rows, residual dropout included (keyed by row_index[row] + row_offset)"""
    from hri_emo_amd import _fp32
    g = torch.Generator().manual_seed(B * L + d)
    M = B * L
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    valid = (torch.arange(L)[None] < lens[:, None]).reshape(-1)
    idx = valid.nonzero().reshape(-1).cuda()
    G, X, dY = (torch.randn(M, d, generator=g).cuda() for _ in range(3))
    dY = dY * valid[:, None].cuda()                 # nothing reads PAD rows: their gradient is zero
    gamma = (1.0 + 0.1 * torch.randn(d, generator=g)).cuda()
    beta = (0.1 * torch.randn(d, generator=g)).cuda()
    drop = (p, 5150, 40, row_off)
    y16, y32 = _fp32.add_ln(G, X, gamma, beta, drop=drop)
    Gp, Xp, dYp = G.index_select(0, idx).contiguous(), X.index_select(0, idx).contiguous(), dY.index_select(0, idx).contiguous()
    y16p, y32p = _fp32.add_ln(Gp, Xp, gamma, beta, drop=drop, rows=idx)
    assert torch.equal(y32p, y32.index_select(0, idx)) and torch.equal(y16p, y16.index_select(0, idx))
    ds, dg, dgam, dbet, dbias = _fp32.add_ln_bwd(dY, G, X, gamma, drop=drop)
    dsp, dgp, dgamp, dbetp, dbiasp = _fp32.add_ln_bwd(dYp, Gp, Xp, gamma, drop=drop, rows=idx)
    assert torch.equal(dsp, ds.index_select(0, idx)) and torch.equal(dgp, dg.index_select(0, idx))
    assert not torch.equal(dgp, dsp)                # the dropout is really on
    for a, b, what in ((dgamp, dgam, "dgamma"), (dbetp, dbet, "dbeta"), (dbiasp, dbias, "dbias")):
        assert _maxrel(a, b) <= 1e-5, (what, _maxrel(a, b))      # column sums over N_valid rows: summation order only


# ----------------------------------------------------------------------------- the switch and the modules
def _fusion(H, d, ne, p=0.1):
    return O.closed_form_init_(H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=p)).cuda()


def _spy(monkeypatch):
    from hri_emo_amd import _lib, _ops
    seen = {"pack": 0, "attn_f32_varlen": 0}
    pack, call = _ops.pack_pair, _lib.call

    def pack_spy(*a, **k):
        seen["pack"] += 1
        return pack(*a, **k)

    def call_spy(name, *a):
        if name in ("hriemo_attn_fwd_f32_varlen", "hriemo_attn_bwd_f32_varlen"):
            seen["attn_f32_varlen"] += 1
        return call(name, *a)

    monkeypatch.setattr(_ops, "pack_pair", pack_spy)
    monkeypatch.setattr(_lib, "call", call_spy)
    return seen


def test_fp32_varlen_takes_the_packed_path_and_falls_back_on_non_prefix_masks(H, monkeypatch):
    g = load_golden("cfg1_eval_ragged")
    m = _fusion(H, 128, 4).eval()
    seen = _spy(monkeypatch)
    H.set_varlen(True)
    with torch.no_grad():
        m(cu(g["h_a"]), cu(g["h_t"]), cu(g["mask_a"]), cu(g["mask_t"]))
    assert seen["pack"] == 2 and seen["attn_f32_varlen"] == 2 * 4, seen       # 2 modalities packed; 2 blocks x 4 attention cores
    ma = g["mask_a"].clone()
    ma[0, 3] = True                                   # a hole inside the valid prefix: the padded path runs
    seen["pack"] = seen["attn_f32_varlen"] = 0
    with torch.no_grad():
        got = m(cu(g["h_a"]), cu(g["h_t"]), cu(ma), cu(g["mask_t"]))
        assert seen == {"pack": 0, "attn_f32_varlen": 0}, seen
        H.set_varlen(False)
        ref = m(cu(g["h_a"]), cu(g["h_t"]), cu(ma), cu(g["mask_t"]))
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    H.set_varlen(True)                                # return_attention: padded as well
    seen["pack"] = 0
    with torch.no_grad():
        m(cu(g["h_a"]), cu(g["h_t"]), cu(g["mask_a"]), cu(g["mask_t"]), return_attention=True)
    assert seen["pack"] == 0


@pytest.mark.parametrize("name,d,ne", [("cfg1_eval_ragged", 128, 4), ("hd96_eval_ragged", 768, 6)])
def test_fusion_eval_fp32_varlen_equals_padded_and_golden(H, name, d, ne):
    g = load_golden(name)
    m = _fusion(H, d, ne).eval()
    args = (cu(g["h_a"]), cu(g["h_t"]), cu(g["mask_a"]), cu(g["mask_t"]))
    with torch.no_grad():
        H.set_varlen(False)
        ref = m(*args)
        H.set_varlen(True)
        got = m(*args)
    for a, b, what in zip(got, ref, ("logits", "beta", "z")):
        assert _maxrel(a, b) <= 1e-5, (what, _maxrel(a, b))
    for out in (got, ref):
        for a, what in zip(out, ("logits", "beta", "z")):
            assert _maxrel(a, g[what]) <= TOL, (what, _maxrel(a, g[what]))


# ----------------------------------------------------------------------------- training step
def _ragged(B, Ta, Tt, d, ne, seed, lo_a, lo_t):
    g = torch.Generator().manual_seed(seed)
    h_a, h_t = torch.randn(B, Ta, d, generator=g), torch.randn(B, Tt, d, generator=g)
    la = torch.randint(lo_a, Ta + 1, (B,), generator=g); lt = torch.randint(lo_t, Tt + 1, (B,), generator=g)
    la[0], lt[0] = Ta, Tt
    m_a, m_t = torch.arange(Ta)[None] >= la[:, None], torch.arange(Tt)[None] >= lt[:, None]
    y = (torch.rand(B, ne, generator=g) < 0.3).float()
    return (h_a, h_t, m_a, m_t, y), (la.tolist(), lt.tolist())


def _step(model, h_a, h_t, m_a, m_t, y, seed=77):
    h_a = h_a.clone().requires_grad_(True)
    h_t = h_t.clone().requires_grad_(True)
    torch.manual_seed(seed)                          # the step's dropout seed comes from torch's generator
    logits, beta, z = model(h_a, h_t, m_a, m_t)
    loss = O.train_step_loss(logits, beta, y)
    model.zero_grad()
    loss.backward()
    return loss.detach(), logits.detach(), z.detach(), h_a.grad, h_t.grad, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fp32_varlen_train_step_equals_padded_and_the_oracle(H, monkeypatch, p):
    """every parameter gradient of the packed fp32 step equals the padded fp32 step's (relative L2 <= 1e-5), and -- the padded
    step's dropout masks replayed into the fp32 oracle -- stays within 1e-3 of the reference's arithmetic"""
    import hashrng
    from hri_emo_amd import _ops
    B, Ta, Tt, d, ne = 3, 100, 40, 256, 5
    torch.manual_seed(1234)
    kw = dict(d_model=d, num_emotions=ne, n_heads=8, dropout=p)
    ref = O.FusionWithEmotionDecoder(**kw).train()
    m = H.FusionWithEmotionDecoder(**kw)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    (h_a, h_t, m_a, m_t, y), _ = _ragged(B, Ta, Tt, d, ne, 11, 30, 10)
    args = (cu(h_a), cu(h_t), cu(m_a), cu(m_t), cu(y))
    log = []
    monkeypatch.setattr(_ops, "DROP_LOG", log)
    H.set_varlen(False)
    pad = _step(m, *args)
    monkeypatch.setattr(_ops, "DROP_LOG", None)
    H.set_varlen(True)
    seen = _spy(monkeypatch)
    pk = _step(m, *args)
    assert seen["pack"] == 2 and seen["attn_f32_varlen"] == 2 * 2 * 4, seen          # forward and backward of 8 cores
    assert _maxrel(pk[0].reshape(1), pad[0].reshape(1)) <= 1e-5
    worst = max((_rel(pk[5][n], pad[5][n]), n) for n in pad[5])
    assert worst[0] <= 1e-5, worst
    assert _rel(pk[3], pad[3]) <= 1e-5 and _rel(pk[4], pad[4]) <= 1e-5
    monkeypatch.undo()
    word = _word()
    cursor = [0]

    def replay_dropout(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        e = log[cursor[0]]
        cursor[0] += 1
        seed = (e[1] + word) & ((1 << 64) - 1)
        if e[0] == "attn":
            _, _, site, B_, H_, Lq, Lk, pp, b_off = e
            k = hashrng.attn_mask(seed, site, B_, H_, Lq, Lk, pp, b_off)
        else:
            _, _, site, M, N, pp, row_off = e
            k = hashrng.rows_mask(seed, site, M, N, pp, row_off)
        keep = torch.from_numpy(k.reshape(tuple(x.shape)))
        return x * (keep.to(x.dtype) * hashrng.inv_keep(pp))

    monkeypatch.setattr(torch.nn.functional, "dropout", replay_dropout)
    r = _step(ref, h_a, h_t, m_a, m_t, y)
    monkeypatch.undo()
    assert cursor[0] == len(log) and (len(log) > 0) == (p > 0)
    assert _maxrel(pk[1], r[1]) <= TOL and _maxrel(pk[2], r[2]) <= TOL
    rows = sorted(((_rel(pk[5][n], r[5][n]), n) for n in r[5]), reverse=True)
    assert rows[0][0] <= GRAD_TOL, ("worst five:", rows[:5])
    assert _rel(pk[3], r[3]) <= GRAD_TOL and _rel(pk[4], r[4]) <= GRAD_TOL
    print(f"fp32 packed step p={p}: vs padded worst {worst[0]:.2e} ({worst[1]}); vs oracle worst {rows[0][0]:.2e} ({rows[0][1]})")


# ----------------------------------------------------------------------------- captured step
def _dp(H, d, ne, p, B):
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    torch.manual_seed(3)
    m = H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=p).cuda().train()
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    dp.set_global_batch(B)
    return m, dp


def test_captured_fp32_padded_step_equals_eager_and_follows_weight_updates(H):
    """the padded fp32 step captured into a graph: a replay equals the eager step, also after the weights were changed in place
    between replays (the split copies of the fp32 masters are refreshed inside the graph, as the bf16 shadows are)"""
    B, Ta, Tt, d, ne = 4, 96, 40, 128, 4
    m, dp = _dp(H, d, ne, 0.0, B)
    (batch, _) = _ragged(B, Ta, Tt, d, ne, 5, 30, 10)
    batch = tuple(cu(t) for t in batch)
    first = [prm.detach().clone() for prm in m.parameters()]

    def update():                                     # an optimizer step's worth of in-place change to every matrix
        with torch.no_grad():
            for prm in m.parameters():
                if prm.dim() == 2:
                    prm.mul_(0.97)

    eager = []
    for _ in range(2):
        eager.append((float(dp.step(*batch)), dp.buckets.flat.clone()))
        update()
    with torch.no_grad():                             # back to the first weights
        for prm, w in zip(m.parameters(), first):
            prm.copy_(w)
    dp.capture(*batch)
    for i in range(2):
        loss = float(dp.step(*batch))
        torch.cuda.synchronize()
        assert abs(loss - eager[i][0]) <= 1e-6 * max(1.0, abs(eager[i][0])), (i, loss, eager[i][0])
        assert _rel(dp.buckets.flat, eager[i][1]) <= 1e-6, (i, _rel(dp.buckets.flat, eager[i][1]))
        update()
    dp.release_graph()


def test_captured_fp32_packed_step_serves_every_batch(H):
    """fp32 + varlen, captured: one capture, then batches with other lengths -- the captured bucket, new buckets captured on the
    spot -- each equal to the padded eager fp32 step on the same batch (dropout 0), a replay bit-identical to the eager packed step
    on the same bucket plan; with dropout, replays from the same seed word are bit-identical, another seed is another draw"""
    from hri_emo_amd import _ops
    B, Ta, Tt, d, ne = 6, 150, 60, 128, 5
    m, dp = _dp(H, d, ne, 0.0, B)
    batches = [_ragged(B, Ta, Tt, d, ne, s, lo_a, lo_t) for s, lo_a, lo_t in ((4, 40, 10), (5, 40, 10), (6, 120, 50), (7, 1, 1))]
    batches = [(tuple(cu(t) for t in b), lens) for b, lens in batches]
    ref = []
    H.set_varlen(False)
    for batch, _ in batches:
        ref.append((float(dp.step(*batch)), dp.buckets.flat.clone()))
    H.set_varlen(True)
    eager = float(dp.step(*batches[0][0]))           # eager packed step (its own, unbucketed plan)
    assert abs(eager - ref[0][0]) <= 1e-5 * max(1.0, abs(ref[0][0]))
    assert _rel(dp.buckets.flat, ref[0][1]) <= 1e-5
    dp.capture(*batches[0][0])
    seen = set()
    for i, (batch, lens) in enumerate(batches):
        loss = float(dp.step(*batch, lengths=lens if i % 2 else None))
        torch.cuda.synchronize()
        seen.add(tuple(int(x) for x in (dp._pb.cu_a[-1], dp._pb.cu_t[-1])))
        assert abs(loss - ref[i][0]) <= 1e-5 * max(1.0, abs(ref[i][0])), (i, loss, ref[i][0])
        assert _rel(dp.buckets.flat, ref[i][1]) <= 1e-5, (i, _rel(dp.buckets.flat, ref[i][1]))
        if i == 0:                                    # the replay against the eager packed step on the same bucket plan
            replay_flat = dp.buckets.flat.clone()
            rec = dp._pb.graphs[dp._mask_seen.key]
            with _ops.use_context(dp.ctx):
                dp.ctx.seq_override = rec.seqs
                try:
                    eager_b = float(dp._fwd_bwd(*dp._static))
                finally:
                    dp.ctx.seq_override = None
            dp.buckets.finish()
            torch.cuda.synchronize()
            assert eager_b == loss and torch.equal(dp.buckets.flat, replay_flat), (eager_b, loss, _rel(dp.buckets.flat, replay_flat))
    assert len(dp._pb.graphs) == len(seen) >= 3
    dp.release_graph()
    # dropout on: replays of a bucket graph from the same seed word are bit-identical, another seed is another draw
    m, dp = _dp(H, d, ne, 0.1, B)
    batch = batches[1][0]
    dp.step(*batch)
    dp.capture(*batch)
    sw = _ops.seed_word(batch[0].device)
    outs = []
    for seed in (123, 123, 124):
        sw.fill_(seed)
        loss = dp.step(*batch)
        torch.cuda.synchronize()
        outs.append((float(loss), dp.buckets.flat.clone()))
    assert math.isfinite(outs[0][0]) and bool(torch.isfinite(outs[0][1]).all())
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])
    assert outs[2][0] != outs[0][0]
    dp.release_graph()
