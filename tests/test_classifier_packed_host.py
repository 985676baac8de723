"""CPU suite for the FusionClassifier's ragged front door: the golden fixture against the oracle, the argument checks of
forward_packed (all raised before anything touches a device), and the float64 restatements the GPU kernel tests of the pooled gate
stand on (pooled_gate_reference.py), each held against plain torch / autograd here."""
import pytest
import torch
import torch.nn.functional as F

import gate_reference as G
import pooled_gate_reference as PG
import rowops_reference as R
from conftest import load_golden
from oracle import hri_emo_oracle as O

TOL = 1e-5          # the oracle's tolerance against the reference (test_oracle_golden.py)
CFG = (128, 4, 8, 2, 32)


def close(a, b, tol=TOL, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= tol * max(1.0, b.abs().max().item()), (what, err)


def strided(flat):
    return flat[torch.linspace(0, flat.numel() - 1, 64).long()]


def masks_of(g, case):
    La, Lt = (int(v) for v in g[case + ".pad"])
    ma = torch.arange(La)[None, :] >= g[case + ".len_a"][:, None]
    mt = torch.arange(Lt)[None, :] >= g[case + ".len_t"][:, None]
    return (ma, mt) if bool(ma.any() or mt.any()) else (None, None)


@pytest.mark.parametrize("case", ["seq", "eq"])
def test_oracle_classifier_reproduces_the_golden_train_step(case):
    g = load_golden("classifier_train_p0")
    m = O.closed_form_init_(O.FusionClassifier(*CFG, dropout=0.0)).train()
    ma, mt = masks_of(g, case)
    if case == "seq":          # the fixture's shape: audio shorter than text in sample 1, PAD input rows zero
        assert int(g["seq.len_a"][1]) < int(g["seq.len_t"][1]) and (g["seq.h_a"][ma] == 0).all() and (g["seq.h_t"][mt] == 0).all()
    logits, beta, pooled = m(g[case + ".h_a"], g[case + ".h_t"], ma, mt)
    loss = F.cross_entropy(logits, g[case + ".y"])
    loss.backward()
    close(logits, g[case + ".logits"], what="logits"); close(beta, g[case + ".beta"], what="beta")
    close(pooled, g[case + ".pooled"], what="pooled"); close(loss.reshape(1), g[case + ".loss"], what="loss")
    for n, p in m.named_parameters():
        close(p.grad.norm().reshape(1), g[f"{case}.g.norm.{n}"], what=n)
        close(strided(p.grad.reshape(-1)), g[f"{case}.g.samp.{n}"], what=n)


def test_oracle_classifier_reproduces_the_golden_utterance_level_eval():
    g = load_golden("classifier_train_p0")
    m = O.closed_form_init_(O.FusionClassifier(*CFG, dropout=0.0)).eval()
    with torch.no_grad():
        logits, beta, pooled = m(g["utt.h_a"], g["utt.h_t"])
    close(logits, g["utt.logits"]); close(beta, g["utt.beta"]); close(pooled, g["utt.pooled"])


# ------------------------------------------------------------------------------------------------ argument checks
def _clf():
    import hri_emo_amd as H
    return H.FusionClassifier(*CFG)


def test_forward_packed_argument_checks_are_those_of_the_fusion_model():
    m = _clf()
    d = CFG[0]
    ra, rt = torch.zeros(7, d), torch.zeros(5, d)
    with pytest.raises(RuntimeError, match="L_t=4 > L_a=3"):
        m.forward_packed(torch.zeros(6, d), rt, [3, 3], [4, 1], pad_to=(3, 4))
    with pytest.raises(ValueError, match="audio length 0 outside"):
        m.forward_packed(ra, rt, [7, 0], [4, 1])
    with pytest.raises(ValueError, match="text length 5 outside"):
        m.forward_packed(torch.zeros(8, d), torch.zeros(6, d), [4, 4], [5, 1], pad_to=(4, 4))
    with pytest.raises(ValueError, match="is not \\[sum\\(lengths\\)"):
        m.forward_packed(ra, rt, [4, 4], [4, 1])
    with pytest.raises(ValueError, match="audio and"):
        m.forward_packed(ra, rt, [4, 3], [5])
    with pytest.raises(ValueError, match="dtype"):
        m.forward_packed(ra.double(), rt.double(), [4, 3], [4, 1])
    with pytest.raises(ValueError, match="differ in width"):
        m.forward_packed(ra, torch.zeros(5, d + 8), [4, 3], [4, 1])
    for kw in ({"return_attention": True}, {"attn_log": object()}):
        with pytest.raises(ValueError, match="not exported by the classifier"):
            m.forward_packed(ra, rt, [4, 3], [4, 1], **kw)
    with pytest.raises(RuntimeError, match="MI355X only"):          # a well-formed batch gets as far as the device check
        m.forward_packed(ra, rt, [4, 3], [4, 1])
    with pytest.raises(RuntimeError, match="MI355X only"):          # utterance level: lengths of all 1, pad_to = (1, 1)
        m.forward_packed(torch.zeros(3, d), torch.zeros(3, d), [1, 1, 1], [1, 1, 1], pad_to=(1, 1))


def test_pooled_gate_switch_is_off_by_default_and_the_model_has_the_packed_entries():
    from hri_emo_amd import _ops
    import hri_emo_amd as H
    import inspect
    assert _ops.POOLED_GATE is False and _ops.pooled_gate() is False
    m = _clf()
    ref = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8)
    for name in ("forward_packed", "_forward_rows"):
        assert list(inspect.signature(getattr(m, name)).parameters) == list(inspect.signature(getattr(ref, name)).parameters), name


# ------------------------------------------------------------------------------------------------ the float64 restatements
def test_pooled_identity_is_the_unmasked_mean_of_the_fused_sequence():
    """pooled = w Abar + (1 - w) Tbar over l < L_t  ==  oracle BetaGate's h_fusion.mean(1), PAD rows included (float64)"""
    torch.manual_seed(3)
    Bs, La, Lt, d = 3, 9, 6, 16
    gate = O.BetaGate(d, 8).double()
    h_a, h_t = torch.randn(Bs, La, d).double(), torch.randn(Bs, Lt, d).double()
    ma = torch.arange(La)[None, :] >= torch.tensor([9, 2, 5])[:, None]          # sample 1: audio shorter than the text length
    mt = torch.arange(Lt)[None, :] >= torch.tensor([6, 4, 1])[:, None]
    hf, _ = gate(h_a, h_t, ma, mt)
    An, Tn = gate.norm_a(h_a), gate.norm_t(h_t)
    mm = lambda x, m: (x * (~m)[..., None]).sum(1) / (~m).sum(1, keepdim=True).clamp(min=1)          # noqa: E731
    a, t = mm(An, ma), mm(Tn, mt)
    w = torch.sigmoid(gate.mlp(torch.cat([a, t, (a - t).abs(), a * t], -1)))
    pooled = w * An[:, :Lt].mean(1) + (1 - w) * Tn.mean(1)
    assert (pooled - hf.mean(1)).abs().max() <= 1e-12


@pytest.mark.parametrize("c", [c for c in PG.CASES if c[2] in (128, 136)][::3], ids=PG.case_id)
def test_keep_partials_reference_and_its_limit(c):
    """keep_ref is the prefix sum of float64 LayerNorm rows; the fp32 yardstick in every order passes check_keep, the two faults
    (mask applied, Lkeep off by one) fail it wherever they change a sum"""
    L, k, d, twin, mask = c
    side = PG.make_side(L, d, twin, mask)
    ln = side["ln"]
    x = (ln["X32"] if twin else ln["X"]).double().view(PG.B, L, d)
    y = F.layer_norm(x, (d,), ln["gamma"].double(), ln["beta"].double(), R.EPS)
    ref, _ = PG.keep_ref(side, k)
    assert (ref.sum(1) - y[:, :k].sum(1)).abs().max() <= 1e-9
    nk = G.chunks(k, 32)
    assert (ref[:, nk:] == 0).all()
    for order in R.ROW_ORDERS:
        for col in G.CHUNK_ORDERS:
            PG.check_keep(PG.keep32(side, k, order, col), side, k, PG.case_id(c))
    if k < L:
        with pytest.raises(AssertionError):
            PG.check_keep(PG.keep32(side, k, fault="off_by_one"), side, k, "off by one")
    if mask != "none" and bool(side["mask"][:, :k].any()):
        with pytest.raises(AssertionError):
            PG.check_keep(PG.keep32(side, k, fault="masked"), side, k, "masked")


@pytest.mark.parametrize("c", [c for c in PG.CASES if c[2] == 136][::2], ids=PG.case_id)
def test_vector_backward_restatement_is_autograd_and_passes_the_existing_envelope(c):
    """pool_bwd_ref on vec_ops (dH = g on rows l < Lkeep, w = 1) is the float64 autograd gradient of
    sum_b g[b] . sum_{l < Lkeep} LN(x)[b, l] + dpool[b] . sum_{valid l} LN(x)[b, l]; the fp32 yardsticks pass check_pool_bwd"""
    L, k, d, twin, mask = c
    side = PG.make_side(L, d, twin, mask)
    v = PG.vec_operands(side, k)
    fw = R.ln_fwd_ref(side["ln"])
    m32, r32 = R.stats32(fw)
    ops = PG.vec_ops(side, v)
    ref = G.pool_bwd_ref(side, ops, 1, m32, r32)
    ln = side["ln"]
    x = (ln["X32"] if twin else ln["X"]).double().view(PG.B, L, d).clone().requires_grad_(True)
    gam, bet = ln["gamma"].double().requires_grad_(True), ln["beta"].double().requires_grad_(True)
    y = F.layer_norm(x, (d,), gam, bet, R.EPS)
    obj = (y[:, :k].sum(1) * v["g"].double()).sum() + ((y * side["valid"].double()[..., None]).sum(1) * v["dpool"].double()).sum()
    obj.backward()
    # (the reference takes the fp32-rounded statistics as inputs: agreement to their rounding)
    assert (ref["dX"] - x.grad).abs().max() <= 1e-5 * max(1.0, x.grad.abs().max().item())
    assert (ref["dgamma"] - gam.grad).abs().max() <= 1e-5 * max(1.0, gam.grad.abs().max().item())
    assert (ref["dbeta"] - bet.grad).abs().max() <= 1e-9 * max(1.0, bet.grad.abs().max().item())
    yards = {o: G.pool_bwd32(side, ops, 1, m32, r32, o, "torch") for o in R.ROW_ORDERS}
    for o in R.ROW_ORDERS:
        b = G.pool_bwd32(side, ops, 1, m32, r32, o, "waves")
        G.check_pool_bwd({"dX": b["dX"], "part": b["part"], "dgamma": b["dgamma"], "dbeta": b["dbeta"]}, side, ref, yards, PG.case_id(c))
    # the cross-check's limit: the dH form of the same gradient (dH = bf16(g / w)) lies inside cross_limit of the vector form
    w = torch.sigmoid(torch.randn(PG.B, d, generator=side["gen"]))
    a = G.pool_bwd32(side, PG.cross_ops(side, v, w), 1, m32, r32, "torch", "waves")["dX"].double()
    b = G.pool_bwd32(side, ops, 1, m32, r32, "torch", "waves")["dX"].double()
    assert ((a - b).abs() <= PG.cross_limit(side, v, m32, r32)).all()


@pytest.mark.parametrize("La,Lt,k", [(70, 33, 33), (33, 32, 1), (70, 70, 69)])
def test_pooled_fuse_limits(La, Lt, k):
    c = PG.fuse_case(La, Lt, k, 136)
    one = torch.tensor(1.0)
    inv = one / torch.tensor(float(k))
    a32, t32 = G.seq_sum(c["ka"]) * inv, G.seq_sum(c["kt"]) * inv
    got = {"abar": a32, "tbar": t32, "pooled": c["w"] * a32 + (one - c["w"]) * t32}
    PG.check_fuse_fwd(got, c, "pooled_fuse_fwd")
    g = c["dpooled"]
    PG.check_fuse_bwd({"dw": g * (a32 - t32), "ga": c["w"] * g * inv, "gt": (one - c["w"]) * g * inv}, c, a32, t32, "pooled_fuse_bwd")
    with pytest.raises(AssertionError):          # the masked-mean divisor in place of Lkeep
        PG.check_fuse_fwd(dict(got, abar=G.seq_sum(c["ka"]) / float(k + 1)), c, "wrong divisor")


def test_ingest_case_layout():
    rows, cu, pad = PG.ingest_case(33, 16, torch.float32, [33, 1, 20])
    assert cu.tolist() == [0, 33, 34, 54] and torch.isnan(rows[54:]).all() and not torch.isnan(rows[:54]).any()
    assert torch.equal(pad[1, 0], rows[33]) and (pad[1, 1:] == 0).all() and (pad[2, 20:] == 0).all()


def test_cases_cover_the_issue_axes():
    assert {c[2] for c in PG.CASES} == set(PG.WIDTHS) and {c[0] for c in PG.CASES} == set(PG.LENGTHS)
    for d in PG.WIDTHS:
        sub = [c for c in PG.CASES if c[2] == d]
        assert {c[4] for c in sub} == set(PG.MASKS) and {c[3] for c in sub} == {True, False}
        assert {(c[0], c[1]) for c in sub} == {(L, k) for L in PG.LENGTHS for k in PG.keeps(L)}
    for L in PG.LENGTHS:
        assert {c[4] for c in PG.CASES if c[0] == L} == set(PG.MASKS) or L == 1
    assert {c[3] for c in PG.PAIR_CASES} == set(PG.WIDTHS)
