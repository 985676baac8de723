"""GPU suite of the fp32 packed tail (`set_precision("fp32")` + `set_varlen(True)` + `_ops.PACKED_TAIL_FP32`): the gate and the
decoder's memory on the encoder's packed rows, with no unpack behind the encoder.

Kernel level (through the C ABI): the packed arm of the four gate kernels that index by sequence position must reproduce the
padded arm BIT FOR BIT on the valid rows -- it is the same kernel body, walking the same positions in the same order, and the
padded launch only adds the exact zeros of the PAD positions -- and the chain (LayerNorm -> pool -> fuse, dpre / dY -> LayerNorm
backward) is also held against float64.  Every output lives in a 0xFF-filled buffer with guard rows around it.  Then the modules
(switch on against off and against the padded path, and against the reference's ragged goldens), a training step against the
padded step and the fp32 oracle, the launches of a step, and the captured bucket graphs."""
import pytest
import torch

from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu

B, LA, LT = 5, 70, 40
LENS_A = [70, 33, 32, 1, 17]
LENS_T = [40, 1, 32, 31, 16]
LENS_F = [40, 1, 32, 1, 16]          # min(la, lt): a one-row sample, la < lt, la > lt, la == lt, odd and even lengths (two accumulators)
GUARD = 4
TOL = 1e-4               # outputs against the goldens: the fp32 mode's bound (tests/test_gpu_fp32_mode.py)
GRAD_TOL = 1e-3          # gradients against the fp32 oracle, relative L2 per parameter (tests/test_gpu_fp32_mode.py)
PACKED_TOL = 1e-5        # packed against padded


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    # captured replays bump the device seed word and the dropout tests set it: later test files replay the hash from its value
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    tail, tail32 = _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32
    hri_emo_amd.set_precision("fp32")
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_precision("bf16")
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32 = tail, tail32
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    torch.cuda.synchronize()


def _mode(H, varlen, tail):
    from hri_emo_amd import _ops
    H.set_varlen(varlen)
    _ops.PACKED_TAIL_FP32 = tail


MODES = (("padded", False, False), ("unpacked tail", True, False), ("packed tail", True, True))


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return torch.cuda.current_stream().cuda_stream


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


def _cu(lens):
    c = [0]
    for x in lens:
        c.append(c[-1] + x)
    return torch.tensor(c, dtype=torch.int32, device="cuda")


def _rows(lens, L):
    """padded row of every packed row"""
    return torch.cat([b * L + torch.arange(n) for b, n in enumerate(lens)]).cuda()


def _pack(x, lens, surplus):
    """[B, L, d] -> packed [sum(lens) + surplus, d]; the rows behind the last sample hold NaN (nothing may read them)"""
    L = x.shape[1]
    p = x.reshape(x.shape[0] * L, x.shape[2]).index_select(0, _rows(lens, L))
    if surplus:
        p = torch.cat([p, torch.full((surplus, p.shape[1]), float("nan"), dtype=p.dtype, device=p.device)])
    return p.contiguous()


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("surplus", [0, 8])
@pytest.mark.parametrize("d", [128, 768])          # one and three column blocks of 256
def test_packed_f32_gate_kernels_equal_padded_bit_for_bit_and_float64(H, d, surplus):
    """hriemo_masked_mean_f32_packed / hriemo_fuse_f32_packed / hriemo_gate_dpre_f32_packed / hriemo_gate_dy_f32_packed against
    hriemo_masked_mean_f32 / hriemo_fuse_f32 / hriemo_gate_dpre_f32 / hriemo_gate_dy_f32 on the padded layout whose PAD positions
    hold the zeros hriemo_unpack_rows writes (dH: the zeros the masked decoder produces at fused-PAD positions).  torch.equal
    throughout (it compares values, so the sign of a zero in a sum of exact zeros would not matter).
    Float64, with the yardsticks of tests/test_gpu_fp32_mode.py: pooled within 1e-5 (its gate test); H within the LayerNorm's
    5e-6 * max(1, max|ref|) -- a convex combination does not amplify the error of its inputs -- plus the fuse kernel's own 1e-6;
    dpre, dY and the LayerNorm backward's dX / dgamma / dbeta within 2e-5 of max|ref| (its backward row-kernel test)."""
    from hri_emo_amd import _fp32, _lib
    g = torch.Generator().manual_seed(200 + d + surplus)
    va = (torch.arange(LA)[None] < torch.tensor(LENS_A)[:, None])
    vt = (torch.arange(LT)[None] < torch.tensor(LENS_T)[:, None])
    vf = (torch.arange(LT)[None] < torch.tensor(LENS_F)[:, None])
    xa = ((torch.randn(B, LA, d, generator=g) * 1.3 + 0.2) * va[..., None])
    xt = (torch.randn(B, LT, d, generator=g) * vt[..., None])
    ga, ba = (1 + 0.1 * torch.randn(d, generator=g)), (0.1 * torch.randn(d, generator=g))
    gt, bt = (1 + 0.1 * torch.randn(d, generator=g)), (0.1 * torch.randn(d, generator=g))
    w = torch.sigmoid(torch.randn(B, d, generator=g))
    dH = (torch.randn(B, LT, d, generator=g) * vf[..., None])          # dH = 0 for l >= lf[b]
    da, dt = torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)
    dbeta = torch.randn(B, generator=g)
    xa_d, xt_d, ga_d, ba_d, gt_d, bt_d, w_d, dH_d, da_d, dt_d, dbeta_d = (x.cuda() for x in (xa, xt, ga, ba, gt, bt, w, dH, da, dt, dbeta))
    ma, mt = (~va).cuda().view(torch.uint8), (~vt).cuda().view(torch.uint8)
    f32 = dict(dtype=torch.float32, device="cuda")

    # ---------------- the padded kernels (the reference of the bit-for-bit half)
    _, An = _fp32.add_ln(xa_d.view(B * LA, d), None, ga_d, ba_d, want16=False)
    _, Tn = _fp32.add_ln(xt_d.view(B * LT, d), None, gt_d, bt_d, want16=False)
    pool_a, pool_t = torch.empty(B, d, **f32), torch.empty(B, d, **f32)
    _lib.call("hriemo_masked_mean_f32", P(An), P(ma), P(pool_a), B, LA, d, ST())
    _lib.call("hriemo_masked_mean_f32", P(Tn), P(mt), P(pool_t), B, LT, d, ST())
    H32 = torch.empty(B * LT, d, **f32)
    H16 = torch.empty(B * LT, d, dtype=torch.bfloat16, device="cuda")
    _lib.call("hriemo_fuse_f32", P(w_d), P(An), LA, P(Tn), LT, P(H32), P(H16), B, LT, d, ST())
    dpre = torch.empty(B, d, **f32)
    _lib.call("hriemo_gate_dpre_f32", P(dH_d), P(An), LA, P(Tn), LT, P(w_d), P(dbeta_d), P(dpre), B, LT, d, ST())
    dYa, dYt = torch.empty(B * LA, d, **f32), torch.empty(B * LT, d, **f32)
    _lib.call("hriemo_gate_dy_f32", P(dH_d), P(w_d), 1, P(da_d), P(ma), P(dYa), B, LT, LA, d, ST())
    _lib.call("hriemo_gate_dy_f32", P(dH_d), P(w_d), 0, P(dt_d), P(mt), P(dYt), B, LT, LT, d, ST())

    # ---------------- the packed operands: exact fit, or 8 NaN rows behind the last sample of every packed buffer
    na, nt, nf = sum(LENS_A), sum(LENS_T), sum(LENS_F)
    Na, Nt, Nf = na + surplus, nt + surplus, nf + surplus
    cu_a, cu_t, cu_f = _cu(LENS_A), _cu(LENS_T), _cu(LENS_F)
    ia, it, i_f = _rows(LENS_A, LA), _rows(LENS_T, LT), _rows(LENS_F, LT)
    xa_p, xt_p, dH_p = _pack(xa_d, LENS_A, surplus), _pack(xt_d, LENS_T, surplus), _pack(dH_d, LENS_F, surplus)
    _, An_p = _fp32.add_ln(xa_p, None, ga_d, ba_d, want16=False)          # row-wise: the packed rows as they are
    _, Tn_p = _fp32.add_ln(xt_p, None, gt_d, bt_d, want16=False)
    assert torch.equal(An_p[:na], An[ia]) and torch.equal(Tn_p[:nt], Tn[it])
    if surplus:
        assert bool(torch.isnan(An_p[na:]).all()) and bool(torch.isnan(Tn_p[nt:]).all()) and bool(torch.isnan(dH_p[nf:]).all())

    out = dict(pool_a=Guarded(B, d, torch.float32), pool_t=Guarded(B, d, torch.float32), H32=Guarded(Nf, d, torch.float32),
               H16=Guarded(Nf, d, torch.bfloat16), dpre=Guarded(B, d, torch.float32), dYa=Guarded(Na, d, torch.float32),
               dYt=Guarded(Nt, d, torch.float32))
    _lib.call("hriemo_masked_mean_f32_packed", P(An_p), P(cu_a), Na, P(out["pool_a"].t), B, LA, d, ST())
    _lib.call("hriemo_masked_mean_f32_packed", P(Tn_p), P(cu_t), Nt, P(out["pool_t"].t), B, LT, d, ST())
    _lib.call("hriemo_fuse_f32_packed", P(w_d), P(An_p), P(cu_a), Na, LA, P(Tn_p), P(cu_t), Nt, LT, P(out["H32"].t), P(out["H16"].t),
              P(cu_f), Nf, B, LT, d, ST())
    _lib.call("hriemo_gate_dpre_f32_packed", P(dH_p), P(cu_f), Nf, P(An_p), P(cu_a), Na, LA, P(Tn_p), P(cu_t), Nt, LT, P(w_d), P(dbeta_d),
              P(out["dpre"].t), B, LT, d, ST())
    _lib.call("hriemo_gate_dy_f32_packed", P(dH_p), P(cu_f), Nf, P(w_d), 1, P(da_d), P(cu_a), Na, P(out["dYa"].t), B, LT, LA, d, ST())
    _lib.call("hriemo_gate_dy_f32_packed", P(dH_p), P(cu_f), Nf, P(w_d), 0, P(dt_d), P(cu_t), Nt, P(out["dYt"].t), B, LT, LT, d, ST())
    torch.cuda.synchronize()
    for k, v in out.items():
        assert v.intact(), ("guard rows", k)
        assert v.written(), ("every row is written", k)
        assert bool(torch.isfinite(v.t.float()).all()), ("finite", k)
    assert torch.equal(out["pool_a"].t, pool_a) and torch.equal(out["pool_t"].t, pool_t), "pooled"
    assert torch.equal(out["H32"].t[:nf], H32[i_f]), "H32"
    assert torch.equal(out["H16"].t[:nf], H16[i_f]), "H16"
    assert torch.equal(out["dpre"].t, dpre), "dpre"
    assert torch.equal(out["dYa"].t[:na], dYa[ia]), "dY audio"
    assert torch.equal(out["dYt"].t[:nt], dYt[it]), "dY text"
    assert float(out["H32"].t[nf:].abs().sum()) == 0.0 and float(out["H16"].t[nf:].float().abs().sum()) == 0.0, "surplus rows of H"
    assert float(out["dYa"].t[na:].abs().sum()) == 0.0 and float(out["dYt"].t[nt:].abs().sum()) == 0.0, "filler rows of dY"
    # the padded launch's PAD rows of dY are exact zeros too: the LayerNorm backward sums them into dgamma / dbeta
    assert float(dYa[(~va).reshape(-1).cuda()].abs().sum()) == 0.0 and float(dYt[(~vt).reshape(-1).cuda()].abs().sum()) == 0.0

    # ---------------- the chain against float64 torch math
    def leaf(t):
        return t.double().requires_grad_(True)

    xa64, xt64, ga64, ba64, gt64, bt64, w64 = (leaf(t) for t in (xa, xt, ga, ba, gt, bt, w))
    A64 = torch.nn.functional.layer_norm(xa64, (d,), ga64, ba64, 1e-5)
    T64 = torch.nn.functional.layer_norm(xt64, (d,), gt64, bt64, 1e-5)
    A64.retain_grad(); T64.retain_grad()
    ka, kt = va.double()[..., None], vt.double()[..., None]
    pa64 = (A64 * ka).sum(1) / ka.sum(1).clamp(min=1.0)
    pt64 = (T64 * kt).sum(1) / kt.sum(1).clamp(min=1.0)
    H64 = w64[:, None, :] * A64[:, :LT] + (1 - w64[:, None, :]) * T64
    ((H64 * dH.double()).sum() + (pa64 * da.double()).sum() + (pt64 * dt.double()).sum()).backward()
    w64d = w64.detach()
    dpre64 = (w64.grad + dbeta.double()[:, None] / d) * w64d * (1 - w64d)

    def err(got, ref):
        return float((got.double().cpu() - ref).abs().max())

    assert err(out["pool_a"].t, pa64.detach()) <= 1e-5 and err(out["pool_t"].t, pt64.detach()) <= 1e-5
    Href = H64.detach().reshape(B * LT, d)[i_f.cpu()]
    assert err(out["H32"].t[:nf], Href) <= 5e-6 * max(1.0, float(Href.abs().max())) + 1e-6
    assert torch.equal(out["H16"].t.float(), out["H32"].t.bfloat16().float())
    assert err(out["dpre"].t, dpre64) <= 2e-5 * float(dpre64.abs().max())
    for key, grad, x_p, x64, gam_d, gam64, bet64, idx, n, lens, L in (
            ("dYa", A64.grad, xa_p, xa64, ga_d, ga64, ba64, ia, na, LENS_A, LA), ("dYt", T64.grad, xt_p, xt64, gt_d, gt64, bt64, it, nt, LENS_T, LT)):
        ref = grad.reshape(B * L, d)[idx.cpu()]
        assert err(out[key].t[:n], ref) <= 2e-5 * float(ref.abs().max()), key
        # the LayerNorm backward on the packed rows as they are (the valid rows: this test's filler rows of X hold NaN)
        dx, _, dgam, dbet, _ = _fp32.add_ln_bwd(out[key].t[:n].contiguous(), x_p[:n].contiguous(), None, gam_d, want_dbias=False)
        for got, r, what in ((dx, x64.grad.reshape(B * L, d)[idx.cpu()], "dX"), (dgam, gam64.grad, "dgamma"), (dbet, bet64.grad, "dbeta")):
            assert err(got, r) <= 2e-5 * float(r.abs().max()), (key, what, err(got, r))


# ----------------------------------------------------------------------------- eval
SHAPES = {                      # the two of tests/test_gpu_packed_tail.py: d, N_e, B, T_a, T_t, audio lengths, text lengths
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


def _eval_three_ways(H, m, args):
    out = {}
    with torch.no_grad():
        for what, varlen, tail in MODES:
            _mode(H, varlen, tail)
            out[what] = [x.float().clone() for x in m(*args)]
    for other in ("padded", "unpacked tail"):
        for a, b, what in zip(out["packed tail"], out[other], ("logits", "beta", "z")):
            e = _maxrel(a, b)
            print(f"{what} packed tail vs {other}: {e:.3e}")
            assert e <= PACKED_TOL, (what, other, e)
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_eval_fp32_packed_tail_equals_padded(H, name):
    """logits, beta, z of the packed tail against the padded fp32 path and against the packed encoder with the tail unpacked"""
    m = _model(H, name, 0.1).eval()
    _eval_three_ways(H, m, _batch(name)[:4])


@pytest.mark.parametrize("gname,d,ne", [("cfg1_eval_ragged", 128, 4), ("hd96_eval_ragged", 768, 6)])
def test_eval_fp32_packed_tail_holds_the_goldens(H, gname, d, ne):
    """the reference's ragged fixtures through the packed tail: 1e-5 against the other two paths, 1e-4 against the goldens"""
    from hri_emo_amd import _ops
    g = load_golden(gname)
    m = O.closed_form_init_(H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=0.1)).cuda().eval()
    args = tuple(g[k].cuda() for k in ("h_a", "h_t", "mask_a", "mask_t"))
    assert _ops.seq_plans(args[2], args[3], args[0].shape[0], args[0].shape[1], args[1].shape[1]) is not None
    out = _eval_three_ways(H, m, args)
    for a, what in zip(out["packed tail"], ("logits", "beta", "z")):
        assert _maxrel(a, g[what]) <= TOL, (what, _maxrel(a, g[what]))


# ----------------------------------------------------------------------------- training step
def _ragged(nb, Ta, Tt, d, ne, seed, lo_a, lo_t):
    """the batch of tests/test_gpu_fp32_varlen.py's training-step test"""
    g = torch.Generator().manual_seed(seed)
    h_a, h_t = torch.randn(nb, Ta, d, generator=g), torch.randn(nb, Tt, d, generator=g)
    la = torch.randint(lo_a, Ta + 1, (nb,), generator=g); lt = torch.randint(lo_t, Tt + 1, (nb,), generator=g)
    la[0], lt[0] = Ta, Tt
    m_a, m_t = torch.arange(Ta)[None] >= la[:, None], torch.arange(Tt)[None] >= lt[:, None]
    y = (torch.rand(nb, ne, generator=g) < 0.3).float()
    return h_a, h_t, m_a, m_t, y


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
def test_fp32_packed_tail_train_step_equals_padded_and_the_oracle(H, monkeypatch, p):
    """loss, dX of both inputs and every parameter gradient of the step with the packed tail: relative L2 <= 1e-5 against the
    padded fp32 step (same dropout masks: the keys are those of the padded rows), and -- the padded step's masks replayed into the
    fp32 oracle -- within 1e-3 of the reference's arithmetic"""
    import hashrng
    from hri_emo_amd import _ops
    nb, Ta, Tt, d, ne = 3, 100, 40, 256, 5
    torch.manual_seed(1234)
    kw = dict(d_model=d, num_emotions=ne, n_heads=8, dropout=p)
    ref = O.FusionWithEmotionDecoder(**kw).train()
    m = H.FusionWithEmotionDecoder(**kw)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    h_a, h_t, m_a, m_t, y = _ragged(nb, Ta, Tt, d, ne, 11, 30, 10)
    args = (cu(h_a), cu(h_t), cu(m_a), cu(m_t), cu(y))
    log = []
    monkeypatch.setattr(_ops, "DROP_LOG", log)
    _mode(H, False, False)
    pad = _step(m, *args)
    monkeypatch.setattr(_ops, "DROP_LOG", None)
    _mode(H, True, True)
    pk = _step(m, *args)
    assert _maxrel(pk[0].reshape(1), pad[0].reshape(1)) <= PACKED_TOL
    worst = max((_rel(pk[5][n], pad[5][n]), n) for n in pad[5])
    print(f"fp32 packed tail p={p}: loss {float(pad[0]):.6f} / {float(pk[0]):.6f}, dX {_rel(pk[3], pad[3]):.2e} / {_rel(pk[4], pad[4]):.2e}, "
          f"worst parameter {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= PACKED_TOL, worst
    assert _rel(pk[3], pad[3]) <= PACKED_TOL and _rel(pk[4], pad[4]) <= PACKED_TOL
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
    print(f"fp32 packed tail p={p}: vs oracle worst {rows[0][0]:.2e} ({rows[0][1]})")
    assert rows[0][0] <= GRAD_TOL, ("worst five:", rows[:5])
    assert _rel(pk[3], r[3]) <= GRAD_TOL and _rel(pk[4], r[4]) <= GRAD_TOL


# ----------------------------------------------------------------------------- launches
def _train_step(H, m, batch, varlen, tail):
    from hri_emo_amd.train import fusion_step_loss
    _mode(H, varlen, tail)
    m.zero_grad(set_to_none=True)
    logits, beta, z = m(*batch[:4])
    loss = fusion_step_loss(logits, beta, batch[4])
    loss.backward()
    return float(loss)


def test_fp32_packed_tail_launches(H, monkeypatch):
    """a spy on _lib.call in the fp32 mode: with the switch on one forward + backward scatters nothing back (no
    hriemo_unpack_rows), gathers only the two inputs, and runs the four packed gate entries in place of their padded forms; with
    it off the tail's two unpack launches (forward) and the two pack launches of their backward are there again, beside the two
    input packs, and no packed gate entry runs."""
    from hri_emo_amd import _lib
    batch = _batch("d128")
    m = _model(H, "d128", 0.0).train()
    _train_step(H, m, batch, True, True)             # warm-up: split weights, plans
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
    packed = ("hriemo_masked_mean_f32_packed", "hriemo_fuse_f32_packed", "hriemo_gate_dpre_f32_packed", "hriemo_gate_dy_f32_packed")
    assert on.count("hriemo_unpack_rows") == 0 and on.count("hriemo_pack_rows") == 2, (on.count("hriemo_unpack_rows"), on.count("hriemo_pack_rows"))
    assert [on.count(n) for n in packed] == [2, 1, 1, 2], [on.count(n) for n in packed]
    assert not any(n[:-len("_packed")] in on for n in packed)
    assert off.count("hriemo_unpack_rows") == 2 and off.count("hriemo_pack_rows") == 4, (off.count("hriemo_unpack_rows"), off.count("hriemo_pack_rows"))
    assert not any(n.endswith("_f32_packed") for n in off)
    assert [off.count(n[:-len("_packed")]) for n in packed] == [2, 1, 1, 2]
    layers = len(m.emotion_decoder.layers)           # the decoder's cross-attentions
    assert on.count("hriemo_attn_fwd_f32_varlen") == off.count("hriemo_attn_fwd_f32_varlen") + layers
    assert on.count("hriemo_attn_bwd_f32_varlen") == off.count("hriemo_attn_bwd_f32_varlen") + layers


# ----------------------------------------------------------------------------- captured
def test_captured_bucket_graphs_run_the_fp32_packed_tail(H):
    """DataParallelStep with bucket graphs in the fp32 mode: a ragged, an all-full and an all-one batch (three buckets) against the
    eager padded fp32 step; a second replay of the first batch is bit-identical to its first; the fused plan rides in the text
    bucket, so there is one graph per distinct (audio rows, text rows) key.  Before the packed steps a 0xFF-filled tensor larger
    than the step's activations is allocated and freed: recycled blocks then read as NaN, and a missed zero-fill of the surplus
    dK | dV rows (or of the fused memory's surplus rows) shows as a non-finite gradient."""
    from test_gpu_varlen import _ragged_batch
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
    for batch in batches:                      # the padded eager fp32 step is the yardstick
        ref.append((float(dp.step(*batch)), dp.buckets.flat.clone()))
    torch.cuda.synchronize()
    poison = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")          # > the step's activations (a few tens of MB)
    poison.fill_(0xFF)
    del poison
    _mode(H, True, True)
    dp.capture(*batches[0])
    keys, first = set(), None
    for i, batch in enumerate(batches):
        loss = float(dp.step(*batch))
        torch.cuda.synchronize()
        keys.add(tuple(int(x) for x in (dp._pb.cu_a[-1], dp._pb.cu_t[-1])))
        assert int(dp._pb.cu_f[-1]) == int(dp._pb.cu_t[-1])
        assert bool(torch.isfinite(dp.buckets.flat).all()), i
        rel = float((dp.buckets.flat - ref[i][1]).norm() / ref[i][1].norm())
        print(f"batch {i}: loss {loss:.6f} vs {ref[i][0]:.6f}, flat gradients relative L2 {rel:.2e}")
        assert abs(loss - ref[i][0]) <= PACKED_TOL * max(1.0, abs(ref[i][0])), (i, loss, ref[i][0])
        assert rel <= PACKED_TOL, (i, rel)
        if i == 0:
            first = (loss, dp.buckets.flat.clone())
    loss = float(dp.step(*batches[0]))
    torch.cuda.synchronize()
    assert loss == first[0] and torch.equal(dp.buckets.flat, first[1]), "a second replay of the first batch"
    assert len(dp._pb.graphs) == len(keys) == 3
    dp.release_graph()
