"""GPU suite, model level: FusionClassifier's ragged path in the fp32 precision mode (set_precision("fp32") +
set_pooled_gate_fp32(True): _fp32.pooled_gate on hriemo_pool32_*) -- forward_packed against the golden fixture
tests/golden/classifier_train_p0.npz and the live fp32 oracle (outputs 1e-4, every gradient 1e-3 in relative L2, with and without
dropout), forward() under POOLED_GATE on the zero-padded batch (torch.equal), the refusals, and the captured steps at B = 4
(capture_packed / step_packed with DeviceAdamW in the graph, short batches, capture_store / step_store, EvalStep default and
stationary).  Without the fp32 pooled gate every test here but the switch-off refusal ends in NotImplementedError."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hashrng
from conftest import load_golden
from oracle import hri_emo_oracle as O

pytestmark = pytest.mark.gpu

CFG = (128, 4, 8, 2, 32)
TOL = 1e-4                 # the fp32 mode's tested output bound (test_gpu_fp32_mode.py): 1e-4 * max(1, |ref|_inf)
GRAD_TOL = 1e-3            # per parameter, relative L2 against the fp32 oracle (test_gpu_fp32_mode.py)
NB, PAD = 4, (40, 35)


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    keep = (_ops.POOLED_GATE, _ops.DROP_LOG, _ops.POOLED_GATE_FP32, _ops.precision(), _ops.gemm_mode())
    hri_emo_amd.set_precision("fp32")
    hri_emo_amd.set_pooled_gate_fp32(True)
    yield hri_emo_amd
    _ops.POOLED_GATE, _ops.DROP_LOG = keep[:2]
    hri_emo_amd.set_pooled_gate_fp32(keep[2])
    hri_emo_amd.set_precision(keep[3])
    hri_emo_amd.set_gemm_mode(keep[4])
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)


def close(got, ref, tol, what, show=True):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e, scale = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    if show:
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


_G = {}


def golden():
    if "g" not in _G:
        _G["g"] = load_golden("classifier_train_p0")
    return _G["g"]


def ragged(case):
    """the fixture's padded batch (CPU, with its masks) and its packed rows on the device"""
    g = golden()
    h_a, h_t = g[case + ".h_a"], g[case + ".h_t"]
    la, lt = g[case + ".len_a"].tolist(), g[case + ".len_t"].tolist()
    pad = tuple(int(v) for v in g[case + ".pad"])
    ma = torch.arange(pad[0])[None, :] >= torch.tensor(la)[:, None]
    mt = torch.arange(pad[1])[None, :] >= torch.tensor(lt)[:, None]
    return {"h_a": h_a, "h_t": h_t, "ma": ma, "mt": mt, "ra": h_a[~ma].contiguous().cuda(), "rt": h_t[~mt].contiguous().cuda(), "la": la,
            "lt": lt, "pad": pad, "y": g[case + ".y"], "masked": bool(ma.any() or mt.any())}


# ------------------------------------------------------------------------------------------------ eval outputs
@pytest.mark.parametrize("case", ["seq", "eq"])
def test_forward_packed_eval_against_the_golden_fp32(H, case):
    m, _ = model(H)
    m.eval()
    b = ragged(case)
    with torch.no_grad():
        logits, beta, pooled = m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
    assert pooled.dtype == torch.float32 and logits.shape == (4, CFG[1]) and beta.shape == (4, 1)
    for name, got in zip(("logits", "beta", "pooled"), (logits, beta, pooled)):
        close(got, golden()[f"{case}.{name}"], TOL, f"{case} {name}")


def test_forward_packed_utterance_level_against_the_golden_fp32(H):
    g = golden()
    m, _ = model(H)
    m.eval()
    n = g["utt.h_a"].shape[0]
    with torch.no_grad():
        out = m.forward_packed(g["utt.h_a"].cuda(), g["utt.h_t"].cuda(), [1] * n, [1] * n, pad_to=(1, 1))
    for name, got in zip(("logits", "beta", "pooled"), out):
        close(got, g["utt." + name], TOL, "utt " + name)


def test_bf16_and_fp16_rows_are_widened(H):
    """bf16 rows have no fp32 twin and are widened, fp16 rows travel in the twin: both equal the fp32 rows of the same values"""
    m, _ = model(H)
    m.eval()
    b = ragged("seq")
    with torch.no_grad():
        for dt in (torch.bfloat16, torch.float16):
            ra, rt = b["ra"].to(dt), b["rt"].to(dt)
            low = m.forward_packed(ra, rt, b["la"], b["lt"], pad_to=b["pad"])
            wide = m.forward_packed(ra.float(), rt.float(), b["la"], b["lt"], pad_to=b["pad"])
            assert low[0].dtype == torch.float32 and low[2].dtype == (torch.float32 if dt == torch.bfloat16 else dt)
            assert torch.isfinite(low[0]).all() and torch.equal(low[0], wide[0]) and torch.equal(low[1], wide[1]), dt


# ------------------------------------------------------------------------------------------------ train steps
def _oracle_step(ref, b, rows_grad=False):
    ref.zero_grad()
    h_a, h_t = b["h_a"].clone().requires_grad_(rows_grad), b["h_t"].clone().requires_grad_(rows_grad)
    logits, beta, pooled = ref(h_a, h_t, b["ma"] if b["masked"] else None, b["mt"] if b["masked"] else None)
    loss = F.cross_entropy(logits, b["y"])
    loss.backward()
    return loss.detach(), logits.detach(), {n: p.grad.detach().clone() for n, p in ref.named_parameters()}, h_a.grad, h_t.grad


def _grad_rows(m, gr, what):
    rows = []
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape, n
        rows.append((_rel(p.grad, gr[n]), n))
    rows.sort(reverse=True)
    print(what, "worst five (relative L2, name):", [(round(e, 6), n) for e, n in rows[:5]])
    assert rows[0][0] <= GRAD_TOL, (what, "worst five:", rows[:5])


@pytest.mark.parametrize("case", ["seq", "eq"])
def test_train_step_p0_against_the_fp32_oracle(H, case):
    """dropout 0, nn.CrossEntropyLoss: loss within 1e-5, every parameter's gradient within 1e-3 (relative L2) of the live fp32 oracle,
    which is pinned to the golden's gradient record"""
    g = golden()
    m, ref = model(H)
    m.train()
    ref.train()
    b = ragged(case)
    loss_r, logits_r, gr, _, _ = _oracle_step(ref, b)
    for n in gr:
        assert abs(gr[n].norm().item() - g[f"{case}.g.norm.{n}"].item()) <= 1e-4 * max(1.0, g[f"{case}.g.norm.{n}"].item()), n
        flat = gr[n].reshape(-1)
        if f"{case}.g.samp.{n}" in g:                # 64 strided samples of a matrix (tests/golden/make_golden.py: grad_record)
            close(flat[torch.linspace(0, flat.numel() - 1, 64).long()], g[f"{case}.g.samp.{n}"], 1e-4, f"oracle {n} samples", show=False)
    logits, beta, pooled = m.forward_packed(b["ra"], b["rt"], b["la"], b["lt"], pad_to=b["pad"])
    loss = F.cross_entropy(logits, b["y"].cuda())
    loss.backward()
    close(loss.reshape(1), loss_r.reshape(1), 1e-5, case + " loss")
    close(loss.reshape(1), g[case + ".loss"].reshape(1), 1e-5, case + " loss against the golden")
    close(logits, logits_r, TOL, case + " logits")
    _grad_rows(m, gr, case)


def test_train_step_with_dropout_equals_the_oracle_under_the_same_masks(H, monkeypatch):
    """p = 0.2, the trainers' configuration: the forward logs every dropout site (_ops.DROP_LOG, the head's last), hashrng rebuilds
    the keep-masks, the fp32 oracle runs the step with them in place of torch's draws"""
    from hri_emo_amd import _ops
    m, ref = model(H, 0.2)
    m.train()
    ref.train()
    b = ragged("seq")
    word = int(_ops.seed_word(torch.device("cuda", 0)).item())
    log = []
    monkeypatch.setattr(_ops, "DROP_LOG", log)
    torch.manual_seed(5)
    ra, rt = b["ra"].clone().requires_grad_(True), b["rt"].clone().requires_grad_(True)
    logits, beta, pooled = m.forward_packed(ra, rt, b["la"], b["lt"], pad_to=b["pad"])
    loss = F.cross_entropy(logits, b["y"].cuda())
    loss.backward()
    monkeypatch.setattr(_ops, "DROP_LOG", None)
    assert log and log[-1][0] == "rows" and log[-1][2] == m._site and log[-1][3:6] == (4, CFG[0], 0.2)

    def keep_of(e, shape):
        seed = (e[1] + word) & ((1 << 64) - 1)
        if e[0] == "attn":
            _, _, site, B_, H_, Lq, Lk, p, b_off = e
            k = hashrng.attn_mask(seed, site, B_, H_, Lq, Lk, p, b_off)
        else:
            _, _, site, M, N, p, row_off = e
            k = hashrng.rows_mask(seed, site, M, N, p, row_off)
        assert int(np.prod(k.shape)) == int(np.prod(shape)), (e, tuple(shape))
        return torch.from_numpy(k.reshape(tuple(shape))), hashrng.inv_keep(e[-2] if e[0] == "attn" else e[5])

    cursor = [0]

    def replay_dropout(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        e = log[cursor[0]]
        cursor[0] += 1
        keep, scale = keep_of(e, x.shape)
        return x * (keep.to(x.dtype) * scale)

    monkeypatch.setattr(torch.nn.functional, "dropout", replay_dropout)
    loss_r, logits_r, gr, ga_r, gt_r = _oracle_step(ref, b, rows_grad=True)
    assert cursor[0] == len(log)                       # the oracle visited exactly the logged sites, in order, the head's last
    monkeypatch.undo()
    close(loss.reshape(1), loss_r.reshape(1), 1e-5, "loss")
    close(logits, logits_r, TOL, "logits")
    _grad_rows(m, gr, "p = 0.2")
    ea, et = _rel(ra.grad, ga_r[~b["ma"]]), _rel(rt.grad, gt_r[~b["mt"]])
    print(f"input gradients: d loss / d rows_a {ea:.2e}, d loss / d rows_t {et:.2e}")
    assert ea <= GRAD_TOL and et <= GRAD_TOL, ("input gradients", ea, et)
    torch.manual_seed(78)                              # and the masks matter: torch's own draws give another loss
    assert abs(float(_oracle_step(ref, b)[0]) - float(loss_r)) > 1e-5


# ------------------------------------------------------------------------------------------------ equivalence and refusals
def test_pooled_forward_of_the_padded_batch_equals_forward_packed_fp32(H):
    from hri_emo_amd import _ops
    m, _ = model(H)
    m.train()
    b = ragged("seq")
    y = b["y"].cuda()
    ra, rt = b["ra"].clone().requires_grad_(True), b["rt"].clone().requires_grad_(True)
    out_p = m.forward_packed(ra, rt, b["la"], b["lt"], pad_to=b["pad"])
    F.cross_entropy(out_p[0], y).backward()
    grads_p = [q.grad.clone() for q in m.parameters()]
    m.zero_grad(set_to_none=True)
    _ops.POOLED_GATE = True
    h_a, h_t = b["h_a"].cuda().requires_grad_(True), b["h_t"].cuda().requires_grad_(True)
    out_f = m(h_a, h_t, b["ma"].cuda(), b["mt"].cuda())
    F.cross_entropy(out_f[0], y).backward()
    for name, x, w in zip(("logits", "beta", "pooled"), out_f, out_p):
        assert torch.isfinite(x).all() and torch.equal(x, w), name
    for (n, q), w in zip(m.named_parameters(), grads_p):
        assert torch.equal(q.grad, w), n
    assert torch.equal(ra.grad, h_a.grad[~b["ma"].cuda()]) and torch.equal(rt.grad, h_t.grad[~b["mt"].cuda()])


def test_refusals_fp32(H):
    m, _ = model(H)
    m.eval()
    b = ragged("seq")
    args = (b["ra"], b["rt"], b["la"], b["lt"])
    H.set_pooled_gate_fp32(False)
    with pytest.raises(NotImplementedError, match="POOLED_GATE_FP32"), torch.no_grad():
        m.forward_packed(*args, pad_to=b["pad"])
    H.set_pooled_gate_fp32(True)
    H.set_gemm_mode("mx_fp8")
    with pytest.raises(NotImplementedError, match="GEMM mode"), torch.no_grad():
        m.forward_packed(*args, pad_to=b["pad"])
    H.set_gemm_mode("bf16")
    with pytest.raises(ValueError, match="not exported by the classifier"), torch.no_grad():
        m.forward_packed(*args, pad_to=b["pad"], return_attention=True)


# ------------------------------------------------------------------------------------------------ captured steps, B = 4
LENGTHS = [([40, 5, 1, 33], [35, 20, 1, 32]), ([12, 40, 7, 20], [8, 35, 3, 19])]


def _batches():
    if "b" not in _G:
        g = torch.Generator().manual_seed(11)
        out = []
        for la, lt in LENGTHS:
            out.append((torch.randn(sum(la), CFG[0], generator=g).cuda(), torch.randn(sum(lt), CFG[0], generator=g).cuda(), list(la), list(lt),
                        torch.randint(0, CFG[1], (NB,), generator=g).cuda()))
        _G["b"] = out
    return _G["b"]


def _loss(logits, beta, y, n_valid=None):
    from hri_emo_amd.train import fusion_step_loss_single_label
    return fusion_step_loss_single_label(logits, beta, y, n_valid=n_valid)


def _cmodel(H, p=0.0):
    torch.manual_seed(3)
    return H.FusionClassifier(*CFG, dropout=p).cuda().train()


def _dp(m):
    from hri_emo_amd.dp import DataParallelStep
    dp = DataParallelStep(m, _loss, overlap=False)
    dp.set_global_batch(NB)
    return dp


def _two_steps(m0, graph, batches, **kw):
    from hri_emo_amd.optim import DeviceAdamW
    dp = _dp(copy.deepcopy(m0))
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
    dp.capture_packed(*_batches()[0], pad_to=PAD, optimizer=opt, **kw)
    dp.use_graph(graph)
    out = []
    for b in batches:
        loss = dp.step_packed(*b)
        torch.cuda.synchronize()
        out.append((loss.clone(), opt.flat_p.clone()))
    dp.release_graph()
    return out


def _head(batch, n):
    ra, rt, la, lt, y = batch
    return ra[:sum(la[:n])], rt[:sum(lt[:n])], la[:n], lt[:n], y[:n]


def test_two_replays_of_step_packed_equal_two_eager_steps(H):
    """DeviceAdamW in the graph: loss and every parameter after each of two replays torch.equal to the eager forward_packed step
    (use_graph(False)) on an identical model"""
    m0 = _cmodel(H)
    a, b = _two_steps(m0, True, _batches()), _two_steps(m0, False, _batches())
    for i, (x, w) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(x[0])) and torch.equal(x[0], w[0]), (i, "loss", float(x[0]), float(w[0]))
        assert torch.equal(x[1], w[1]), (i, "parameters", int((x[1] != w[1]).sum()))
    assert not torch.equal(a[0][1], a[1][1])


def test_short_batch_of_3_under_partial_batches(H):
    m0 = _cmodel(H)
    short = [_head(_batches()[0], 3)]
    a, b = _two_steps(m0, True, short, partial_batches=True), _two_steps(m0, False, short, partial_batches=True)
    rel = float((a[0][1] - b[0][1]).norm() / b[0][1].norm())
    print(f"n = 3: loss {float(a[0][0]):.7f} vs {float(b[0][0]):.7f}, parameters relative L2 {rel:.2e}")
    assert abs(float(a[0][0]) - float(b[0][0])) <= 1e-5 * max(1.0, abs(float(b[0][0]))) and rel <= 1e-5


def test_accumulation_in_the_graph_against_the_eager_micro_steps(H):
    """grad_accum = 2, DeviceAdamW in the graph: micro-step 0 moves no parameter, micro-step 1 is one update; the parameters against
    the same two micro-steps run eagerly (use_graph(False)) on an identical model"""
    m0 = _cmodel(H)
    a = _two_steps(m0, True, _batches(), grad_accum=2)
    b = _two_steps(m0, False, _batches(), grad_accum=2)
    assert torch.equal(a[0][1], b[0][1]), "micro-step 0 holds the update in both arms: the parameters are the initial ones"
    assert not torch.equal(a[1][1], a[0][1]), "micro-step 1 carries the update"
    rel = float((a[1][1] - b[1][1]).norm() / b[1][1].norm())
    print(f"grad_accum = 2: losses {float(a[0][0]):.7f} {float(a[1][0]):.7f} vs {float(b[0][0]):.7f} {float(b[1][0]):.7f}, parameters relative L2 {rel:.2e}")
    for x, w in zip(a, b):
        assert abs(float(x[0]) - float(w[0])) <= 1e-5 * max(1.0, abs(float(w[0])))
    assert rel <= 1e-5


def _store():
    from hri_emo_amd.data import DeviceFeatureStore
    if "store" not in _G:
        g = torch.Generator().manual_seed(23)
        la = [40, 5, 1, 33, 12, 40, 7, 20]
        lt = [35, 20, 1, 32, 8, 35, 3, 19]
        samples = [(torch.randn(a, CFG[0], generator=g), torch.zeros(a, dtype=torch.bool), torch.randn(t, CFG[0], generator=g),
                    torch.zeros(t, dtype=torch.bool), int(torch.randint(0, CFG[1], (1,), generator=g))) for a, t in zip(la, lt)]
        _G["store"] = DeviceFeatureStore.from_samples(samples, "cuda", loss_type="single_label", chunk_bytes=64 << 10)
    return _G["store"]


IDS = [[0, 1, 2, 3], [4, 5, 6, 7]]


def _packed(store, ids):
    ra, la, rt, lt, y = store.fetch(ids)
    return ra, rt, la, lt, y


def test_step_store_equals_step_packed_on_the_fetched_batch_fp32(H):
    from hri_emo_amd import _ops
    from hri_emo_amd.optim import DeviceAdamW
    store = _store()
    assert tuple(store.pad_to) == PAD
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    m0 = _cmodel(H, 0.2)
    arms = []
    for by_id in (True, False):
        dp = _dp(copy.deepcopy(m0))
        opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0)
        torch.manual_seed(5)
        if by_id:
            dp.capture_store(store, IDS[0], optimizer=opt)
        else:
            dp.capture_packed(*_packed(store, IDS[0]), pad_to=store.pad_to, optimizer=opt)
        _ops.seed_word(torch.device("cuda", 0)).copy_(word)
        out = []
        for ids in IDS:
            loss = dp.step_store(ids) if by_id else dp.step_packed(*_packed(store, ids))
            torch.cuda.synchronize()
            out.append((loss.clone(), dp.buckets.flat.clone(), opt.flat_p.clone()))
        dp.release_graph()
        arms.append(out)
    for i, (x, w) in enumerate(zip(*arms)):
        for j, name in enumerate(("loss", "flat gradients", "parameters")):
            assert torch.isfinite(x[j]).all() and torch.equal(x[j], w[j]), (i, name)


@pytest.mark.parametrize("stationary", [False, True], ids=["default", "stationary"])
def test_eval_step_equals_the_eager_evaluation_fp32(H, stationary):
    m = _cmodel(H, 0.2)
    es = H.EvalStep(m, _loss, stationary=True) if stationary else H.EvalStep(m, _loss)
    es.capture_packed(*_batches()[0], pad_to=PAD)
    for b in (_batches()[0], _batches()[1], _head(_batches()[1], 2)):
        got = es.eval_packed(*b)
        m.eval()
        with torch.no_grad():
            logits, beta, z = m.forward_packed(*b[:4], pad_to=PAD)
            loss = _loss(logits, beta, b[4])
        m.train()
        torch.cuda.synchronize()
        for x, r, name in zip(got, (logits, beta, z, loss), ("logits", "beta", "pooled", "loss")):
            assert x.shape == r.shape and torch.isfinite(x).all() and torch.equal(x, r), (name, len(b[2]))
    if not stationary:
        # the switch moved since the capture: the replay is refused, and served again once it is back
        H.set_pooled_gate_fp32(False)
        with pytest.raises(RuntimeError, match="captured with POOLED_GATE_FP32"):
            es.eval_packed(*_batches()[0])
        H.set_pooled_gate_fp32(True)
        es.eval_packed(*_batches()[0])
    es.release_graph()
