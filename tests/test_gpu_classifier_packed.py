"""GPU suite, model level: FusionClassifier on ragged batches (forward_packed / _forward_rows, the pooled gate) against the golden
fixture tests/golden/classifier_train_p0.npz (the reference on the CPU, tests/golden/make_classifier_golden.py), against forward()
with _ops.POOLED_GATE = True on the zero-padded batch (torch.equal), the head's Dropout as a counter-hash site, and the unchanged
default of forward()."""
import pytest
import torch
import torch.nn.functional as F

import hashrng
from conftest import load_golden
from oracle import hri_emo_oracle as O

pytestmark = pytest.mark.gpu

CFG = (128, 4, 8, 2, 32)
TOL = 1e-2                 # the bound of test_legacy_block_and_fusion_classifier_vs_golden: 1e-2 * max(1, |ref|_inf)
GRAD_FLOOR = 4e-2          # the rule of test_fusion_train_step_grads (test_gpu_parity.py), restated: every parameter's relative L2
GRAD_FACTOR = 3.0          # error <= max(GRAD_FLOOR, GRAD_FACTOR x the error of the oracle under CPU autocast(bf16) on that parameter)


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    keep = (_ops.POOLED_GATE, _ops.DROP_LOG)
    yield hri_emo_amd
    _ops.POOLED_GATE, _ops.DROP_LOG = keep
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)


def err_of(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())


def close(got, ref, tol, what):
    e, scale = err_of(got, ref)
    print(f"{what}: max error {e:.3e} (bound {tol * scale:.3e})")
    assert e <= tol * scale, (what, e, scale)


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def model(H, p=0.0):
    ref = O.closed_form_init_(O.FusionClassifier(*CFG, dropout=p))
    m = H.FusionClassifier(*CFG, dropout=p)
    m.load_state_dict(ref.state_dict(), strict=True)
    return m.cuda(), ref


def ragged(g, case):
    """the fixture's padded batch and its packed rows on the device"""
    h_a, h_t = g[case + ".h_a"], g[case + ".h_t"]
    la, lt = g[case + ".len_a"].tolist(), g[case + ".len_t"].tolist()
    pad = tuple(int(v) for v in g[case + ".pad"])
    ma = torch.arange(pad[0])[None, :] >= torch.tensor(la)[:, None]
    mt = torch.arange(pad[1])[None, :] >= torch.tensor(lt)[:, None]
    return {"h_a": h_a.cuda(), "h_t": h_t.cuda(), "ma": ma.cuda(), "mt": mt.cuda(), "ra": h_a[~ma].contiguous().cuda(),
            "rt": h_t[~mt].contiguous().cuda(), "la": la, "lt": lt, "pad": pad, "y": g[case + ".y"].cuda()}


# ------------------------------------------------------------------------------------------------ against the golden
@pytest.mark.parametrize("case", ["seq", "eq"])
def test_forward_packed_eval_against_the_golden(H, case):
    g = load_golden("classifier_train_p0")
    m, _ = model(H)
    m.eval()
    b = ragged(g, case)
    with torch.no_grad():
        logits, beta, pooled = m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
        old = m(b["h_a"], b["h_t"], b["ma"], b["mt"])                    # the path of record, for the figures of DESIGN 1
    assert pooled.dtype == torch.float32 and logits.shape == (4, CFG[1]) and beta.shape == (4, 1)
    for name, got, prev in zip(("logits", "beta", "pooled"), (logits, beta, pooled), old):
        print(f"{case} {name}: h_fusion path error {err_of(prev, g[f'{case}.{name}'])[0]:.3e}")
        close(got, g[f"{case}.{name}"], TOL, f"{case} {name}")


def test_forward_packed_utterance_level_against_the_golden(H):
    """[B, d] inputs are lengths of all 1 with pad_to = (1, 1)"""
    g = load_golden("classifier_train_p0")
    m, _ = model(H)
    m.eval()
    n = g["utt.h_a"].shape[0]
    with torch.no_grad():
        logits, beta, pooled = m.forward_packed(g["utt.h_a"].cuda(), g["utt.h_t"].cuda(), [1] * n, [1] * n, pad_to=(1, 1))
    for name, got in zip(("logits", "beta", "pooled"), (logits, beta, pooled)):
        close(got, g["utt." + name], TOL, "utt " + name)


def _oracle_grads(ref, g, case, autocast):
    ma = torch.arange(g[case + ".h_a"].shape[1])[None, :] >= g[case + ".len_a"][:, None]
    mt = torch.arange(g[case + ".h_t"].shape[1])[None, :] >= g[case + ".len_t"][:, None]
    masked = bool(ma.any() or mt.any())
    ref.zero_grad()
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            logits, _, _ = ref(g[case + ".h_a"], g[case + ".h_t"], ma if masked else None, mt if masked else None)
        logits = logits.float()
    else:
        logits, _, _ = ref(g[case + ".h_a"], g[case + ".h_t"], ma if masked else None, mt if masked else None)
    F.cross_entropy(logits, g[case + ".y"]).backward()
    return {n: p.grad.detach().clone() for n, p in ref.named_parameters()}


@pytest.mark.parametrize("case", ["seq", "eq"])
def test_forward_packed_train_step_grads_against_the_golden(H, case):
    """dropout 0, the trainer's CrossEntropyLoss: loss, logits and EVERY parameter's gradient.  The fp32 oracle is pinned to the
    golden (norm and strided sample of every gradient); the bound per parameter is max(4e-2, 3 x the error of the oracle under CPU
    autocast(bfloat16) on that parameter) in relative L2, in_proj_bias over its q and v thirds (the K third's gradient is exactly 0)."""
    g = load_golden("classifier_train_p0")
    m, ref = model(H)
    m.train()
    ref.train()
    b = ragged(g, case)
    gr = _oracle_grads(ref, g, case, False)
    for n in gr:          # the live fp32 oracle IS the golden
        assert abs(gr[n].norm().item() - g[f"{case}.g.norm.{n}"].item()) <= 1e-4 * max(1.0, g[f"{case}.g.norm.{n}"].item()), n
    gy = _oracle_grads(ref, g, case, True)
    logits, beta, pooled = m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
    loss = F.cross_entropy(logits, b["y"])
    loss.backward()
    close(logits, g[case + ".logits"], TOL, case + " logits")
    close(loss.reshape(1), g[case + ".loss"], TOL, case + " loss")

    def rel(a, r, n):
        if n.endswith("in_proj_bias"):
            d3 = a.numel() // 3
            return _rel(torch.cat([a[:d3], a[2 * d3:]]), torch.cat([r[:d3], r[2 * d3:]]))
        return _rel(a, r)

    bad, rows = [], []
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape, n
        em, ey = rel(p.grad, gr[n], n), rel(gy[n], gr[n], n)
        rows.append((round(em, 4), round(ey, 4), n))
        if not em <= max(GRAD_FLOOR, GRAD_FACTOR * ey):
            bad.append((n, round(em, 4), round(ey, 4)))
    rows.sort(reverse=True)
    print(case, "worst five (mine, yardstick, name):", rows[:5])
    assert not bad, ("parameters over max(4e-2, 3 x yardstick) (name, mine, yardstick):", bad)


# ------------------------------------------------------------------------------------------------ bit-equality with forward()
@pytest.mark.parametrize("mode", ["eval", "train p 0", "train p 0.2"])
@pytest.mark.parametrize("varlen", [False, True], ids=["varlen off", "varlen on"])
def test_pooled_forward_of_the_padded_batch_equals_forward_packed(H, mode, varlen):
    """POOLED_GATE = True: forward(zero-padded batch, masks) and forward_packed(ragged batch) are the same launches on the same bits --
    outputs and (in train mode) every parameter gradient torch.equal, whatever set_varlen says; p = 0.2 under the same manual_seed"""
    from hri_emo_amd import _ops
    g = load_golden("classifier_train_p0")
    p = 0.2 if mode.endswith("0.2") else 0.0
    m, _ = model(H, p)
    m.train(mode != "eval")
    H.set_varlen(varlen)
    b = ragged(g, "seq")
    outs = []
    for packed in (False, True):
        m.zero_grad(set_to_none=True)
        _ops.POOLED_GATE = not packed
        torch.manual_seed(77)
        with torch.set_grad_enabled(mode != "eval"):
            if packed:
                out = m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
            else:
                out = m(b["h_a"], b["h_t"], b["ma"], b["mt"])
            if mode != "eval":
                F.cross_entropy(out[0], b["y"]).backward()
        torch.cuda.synchronize()
        outs.append(([t.detach().clone() for t in out], [q.grad.clone() for q in m.parameters()] if mode != "eval" else []))
    for name, x, y in zip(("logits", "beta", "pooled"), outs[0][0], outs[1][0]):
        assert torch.isfinite(x).all() and torch.equal(x, y), (mode, name)
    for (n, _), x, y in zip(m.named_parameters(), outs[0][1], outs[1][1]):
        assert torch.equal(x, y), (mode, n)
    if p > 0:
        _ops.POOLED_GATE = False
        torch.manual_seed(78)
        again = m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
        assert not torch.equal(again[0], outs[1][0][0]), "another seed draws other masks"


def test_input_gradients_of_forward_packed(H):
    """rows that require grad get the packed gradient: equal to the valid rows of the padded input's gradient"""
    from hri_emo_amd import _ops
    g = load_golden("classifier_train_p0")
    m, _ = model(H)
    m.train()
    b = ragged(g, "seq")
    ra, rt = b["ra"].clone().requires_grad_(True), b["rt"].clone().requires_grad_(True)
    F.cross_entropy(m.forward_packed(ra, rt, b["la"], b["lt"], pad_to=b["pad"])[0], b["y"]).backward()
    _ops.POOLED_GATE = True
    h_a, h_t = b["h_a"].clone().requires_grad_(True), b["h_t"].clone().requires_grad_(True)
    F.cross_entropy(m(h_a, h_t, b["ma"], b["mt"])[0], b["y"]).backward()
    assert torch.equal(ra.grad, h_a.grad[~b["ma"]]) and torch.equal(rt.grad, h_t.grad[~b["mt"]])


# ------------------------------------------------------------------------------------------------ the head's dropout
def test_head_dropout_is_a_hash_site(H):
    """the head's Dropout is the LAST entry of DROP_LOG: ("rows", seed, site, B, d, p, batch offset); hashrng rebuilds its keep-mask and
    the logits are the head's second Linear applied to relu(...) * keep / (1 - p)"""
    from hri_emo_amd import _ops
    g = load_golden("classifier_train_p0")
    m, _ = model(H, 0.2)
    m.train()
    b = ragged(g, "seq")
    log = []
    _ops.DROP_LOG = log
    torch.manual_seed(5)
    logits, beta, pooled = m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
    _ops.DROP_LOG = None
    kind, seed, site, M, N, p, roff = log[-1]
    assert (kind, site, M, N, p, roff) == ("rows", m._site, 4, CFG[0], 0.2, 0) and site not in [e[2] for e in log[:-1]]
    word = int(_ops.seed_word(torch.device("cuda", 0)).item())
    keep = torch.from_numpy(hashrng.rows_mask((seed + word) & ((1 << 64) - 1), site, M, N, p, roff)).cuda()
    assert 0.6 < keep.float().mean().item() < 0.95
    head = m.classifier
    with torch.no_grad():
        h = F.relu(head[1](head[0](pooled)))
        inv = torch.tensor(hashrng.inv_keep(p), dtype=torch.float32, device="cuda")
        want = head[4](torch.where(keep, h * inv, torch.zeros((), device="cuda")))
    assert (logits - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    # backward: the gradient of the dropped activations carries the same mask
    h2 = h.clone().requires_grad_(True)
    y = _ops.DropoutF32Fn.apply(h2, p, seed, site, roff)
    y.backward(torch.ones_like(y))
    assert torch.equal(h2.grad != 0, keep) and torch.equal(y != 0, keep & (h != 0))


# ------------------------------------------------------------------------------------------------ the default is unchanged
def test_forward_default_is_unchanged_and_reads_the_switch(H, monkeypatch):
    """switch off: forward() returns, bit for bit, what the code path of record returns -- the encoder's _fwd_pair, the vector gate's
    _fwd_pair, torch's mean over the fused sequence, the torch head -- and it asks pooled_gate() exactly once"""
    from hri_emo_amd import _ops
    g = load_golden("classifier_train_p0")
    m, _ = model(H)
    m.eval()
    b = ragged(g, "seq")
    asked = []
    real = _ops.pooled_gate
    monkeypatch.setattr(_ops, "pooled_gate", lambda: asked.append(1) or real())
    names, call = [], _ops._lib.call
    monkeypatch.setattr(_ops._lib, "call", lambda name, *a: names.append(name) or call(name, *a))
    with torch.no_grad():
        got = m(b["h_a"], b["h_t"], b["ma"], b["mt"])
        assert asked == [1] and "hriemo_ln_pool2_fwd_pair" not in names and "hriemo_fuse_fwd" in names
        a, a32 = _ops.as_pair(b["h_a"])
        t, t32 = _ops.as_pair(b["h_t"])
        a, a32, t, t32, _, seqs = m.cross_modal._fwd_pair(a, a32, t, t32, b["ma"], b["mt"], False)
        hf, beta = m.beta_gate._fwd_pair(a, a32, t, t32, b["ma"], b["mt"], seqs)
        pooled = hf.float().mean(dim=1)
        want = (m.classifier(pooled), beta, pooled)
        names.clear()
        _ops.POOLED_GATE = True
        other = m(b["h_a"], b["h_t"], b["ma"], b["mt"])
        assert "hriemo_ln_pool2_fwd_pair" in names and "hriemo_fuse_fwd" not in names
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert not torch.equal(other[2], got[2]), "the pooled path does not round the LayerNorm outputs to bf16"


def test_refusals(H):
    m, _ = model(H)
    g = load_golden("classifier_train_p0")
    b = ragged(g, "seq")
    H.set_precision("fp32")
    try:
        with pytest.raises(NotImplementedError):
            m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
    finally:
        H.set_precision("bf16")
    plan, masks = __import__("hri_emo_amd")._ops.plans_from_lengths(b["la"], b["lt"], *b["pad"], b["ra"].device)
    with pytest.raises(ValueError, match="not exported by the classifier"):
        m._forward_rows(b["ra"], b["rt"], plan, masks, b["pad"], return_attention=True)
    with pytest.raises(ValueError, match="pads to"):
        m._forward_rows(b["ra"], b["rt"], plan, masks, (b["pad"][0] + 1, b["pad"][1]))
