"""GPU suite of train.ActivationLog on the model: a log attached changes no bit of any result and adds only its own three launches;
every site records what actlog_reference.py computes from the tensors the model hands out; blame() names the site, sample and
position of a non-finite value that data alone produced; warm-up passes leave no trace.  Tiny model: d = 64, 2 heads, one and two
layers, B = 3, lengths (20, 9, 14) / (12, 7, 3) padded to (24, 16), N_e = 4.

Ghost utterances at the model level: a training step multiplies the (zero) output gradients of its ghosts with their input rows, so
those rows must stay finite whatever a log does; the ghosts' TARGETS are poisoned there.  The evaluation step has no backward:
there the ghosts' input rows themselves are poisoned, their activations are NaN, and the log must still blame nothing."""
import copy

import numpy as np
import pytest
import torch

import actlog_reference as R

pytestmark = pytest.mark.gpu

D, NE, NB, PAD = 64, 4, 3, (24, 16)
LA, LT = [20, 9, 14], [12, 7, 3]
NEW = {"hriemo_act_log_plan", "hriemo_act_probe", "hriemo_act_log_fold"}
NAN, INF = float("nan"), float("inf")


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    keep = (_ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.gemm_mode(), _ops.precision(), _ops.varlen())
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    yield hri_emo_amd
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(keep[5])
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = keep[:3]
    hri_emo_amd.set_gemm_mode(keep[3])
    hri_emo_amd.set_precision(keep[4])
    assert _ops.CTX.act_log is None


def _tail(on):
    from hri_emo_amd import _ops
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = _ops.PACKED_TAIL_MX8 = bool(on)


_CACHE = {}


def _batch():
    """(ragged (rows_a, rows_t, la, lt, y), padded (h_a, h_t, m_a, m_t, y)): computed once, never changed"""
    if "b" not in _CACHE:
        g = torch.Generator().manual_seed(5)
        h_a, h_t = torch.randn(NB, PAD[0], D, generator=g).cuda(), torch.randn(NB, PAD[1], D, generator=g).cuda()
        m_a = (torch.arange(PAD[0])[None] >= torch.tensor(LA)[:, None]).cuda()
        m_t = (torch.arange(PAD[1])[None] >= torch.tensor(LT)[:, None]).cuda()
        h_a[m_a], h_t[m_t] = 0.0, 0.0
        y = (torch.rand(NB, NE, generator=g) < 0.4).float().cuda()
        _CACHE["b"] = ((h_a[~m_a].contiguous(), h_t[~m_t].contiguous(), list(LA), list(LT), y), (h_a, h_t, m_a, m_t, y))
    return _CACHE["b"]


def _head(batch, n):
    ra, rt, la, lt, y = batch
    return ra[:sum(la[:n])], rt[:sum(lt[:n])], la[:n], lt[:n], y[:n]


def _model(H, layers=1, p=0.1):
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=2, num_layers_fusion=layers, num_layers_decoder=layers,
                                      beta_hidden=32, dropout=p).cuda().train()


def _log(m, **kw):
    from hri_emo_amd.train import ActivationLog
    return ActivationLog.for_model(m, **{"capacity": 4, "max_rows": 256, **kw})


def _eager(m, packed, log=None, y=None):
    """one eager forward + backward (dropout seeds drawn from a fixed generator state) -> [logits, beta, z, loss, every gradient]"""
    from hri_emo_amd.train import fusion_step_loss
    rag, pad = _batch()
    m.zero_grad(set_to_none=True)
    torch.manual_seed(17)

    def run():
        logits, beta, z = m.forward_packed(*rag[:4], pad_to=PAD) if packed else m(*pad[:4])
        loss = fusion_step_loss(logits, beta, rag[4] if y is None else y)
        loss.backward()
        return logits, beta, z, loss

    if log is None:
        out = run()
    else:
        with log.watch():
            out = run()
            log.close_backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out] + [p.grad.clone() for p in m.parameters()]


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y) or (bool(torch.isnan(x).any()) and torch.equal(torch.isnan(x), torch.isnan(y))
                                     and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))), (what, i)


class Spy:
    def __init__(self, monkeypatch):
        from hri_emo_amd import _lib
        self.names, real = [], _lib.call

        def spy(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", spy)

    def take(self):
        out, self.names = self.names, []
        return out


def _missing(arr, half, record=-1):
    return [n for n, h in zip(arr["sites"], arr[half]["have"][record]) if h == 0]


# ----------------------------------------------------------------------------- eager: same bits, only the three new launches
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "forward_packed"])
def test_eager_pass_keeps_every_bit_and_adds_only_its_own_launches(H, monkeypatch, layers, packed):
    H.set_varlen(False)
    m0 = _model(H, layers)
    spy = Spy(monkeypatch)
    ref = _eager(copy.deepcopy(m0), packed)
    plain = spy.take()
    m = copy.deepcopy(m0)
    log = _log(m)
    got = _eager(m, packed, log)
    logged = spy.take()
    _same(got, ref, "with a log attached")
    assert not NEW & set(plain)
    assert [n for n in logged if n not in NEW] == plain, "a log changed the launches of the pass itself"
    S = len(log.names)
    assert logged.count("hriemo_act_log_plan") == 1 and logged.count("hriemo_act_log_fold") == 2
    assert logged.count("hriemo_act_probe") == S + (S - 3)                      # gate.w and the input.* sites get no gradient
    assert logged[0] == "hriemo_act_log_plan" or packed                         # (forward_packed: behind the two ingest launches)
    arr = log.arrays()
    assert arr["n_passes"] == 1 and arr["n_recorded"] == 1 and arr["halves"].tolist() == [3]
    assert _missing(arr, "forward") == []
    assert _missing(arr, "gradient") == ["input.audio", "input.text", "gate.w"]
    assert int(arr["forward"]["n_bad"].sum()) == 0 and int(arr["gradient"]["n_bad"].sum()) == 0 and log.blame() is None
    # sites= : only the selected ones launch, the pass keeps its bits
    m = copy.deepcopy(m0)
    some = _log(m, sites=["enc*.audio_ffn", "gate.fused", "logits"])
    _same(_eager(m, packed, some), ref, "with a partial log attached")
    logged = spy.take()
    assert logged.count("hriemo_act_probe") == 2 * (layers + 2)
    # a sub-module called on its own inside watch() has no plan in front: it launches no probe and leaves the log as it was
    rag, pad = _batch()
    before = some._small.clone()
    with some.watch():
        with torch.no_grad():
            ea, et = m.cross_modal(*pad[:4])
            m.beta_gate(ea, et, pad[2], pad[3])
    torch.cuda.synchronize()
    assert not NEW & set(spy.take()) and torch.equal(some._small, before)
    arr = some.arrays()
    assert [n for n in arr["sites"] if n not in _missing(arr, "forward")] == some.selected == [n for n in arr["sites"] if n not in _missing(arr, "gradient")]


@pytest.mark.parametrize("mode,tail", [("bf16", True), ("mx_fp8", False), ("mx_fp8", True)])
def test_both_gemm_modes_and_the_packed_tail(H, mode, tail):
    H.set_gemm_mode(mode)
    _tail(tail)
    m0 = _model(H, 2)
    ref = _eager(copy.deepcopy(m0), True)
    m = copy.deepcopy(m0)
    log = _log(m)
    _same(_eager(m, True, log), ref, f"{mode}, packed tail {tail}")
    arr = log.arrays()
    assert _missing(arr, "forward") == [] and _missing(arr, "gradient") == ["input.audio", "input.text", "gate.w"]
    assert log.blame() is None


def test_inputs_that_need_a_gradient_record_it_and_the_mosei_wrapper_is_served(H):
    from hri_emo_amd.train import mosei_step_loss
    torch.manual_seed(3)
    m = H.MoseiFusionWithEmotionDecoder(d_audio=10, d_text=12, d_model=D, num_emotions=NE, n_heads=2, num_layers_fusion=1,
                                        num_layers_decoder=1, beta_hidden=32, dropout=0.0).cuda().train()
    g = torch.Generator().manual_seed(1)
    ra, rt = torch.randn(sum(LA), 10, generator=g).cuda(), torch.randn(sum(LT), 12, generator=g).cuda()
    log = _log(m)
    with log.watch():
        logits, beta, _ = m.forward_packed(ra, rt, LA, LT, pad_to=PAD)
        mosei_step_loss(logits, beta, _batch()[0][4]).backward()
        log.close_backward()
    arr = log.arrays()
    assert _missing(arr, "forward") == [] and _missing(arr, "gradient") == ["gate.w"]      # the projected rows need a gradient
    assert arr["gradient"]["n_rows"][-1, 0] == sum(LA) and arr["gradient"]["n_rows"][-1, 1] == sum(LT)


# ----------------------------------------------------------------------------- recorded values
def test_recorded_values_match_the_reference(H):
    H.set_varlen(False)
    rag, pad = _batch()
    m = _model(H, 2, p=0.0)
    log = _log(m)
    got = _eager(m, True, log)
    logits, z = got[0], got[2]
    arr = log.arrays()
    f = arr["forward"]
    site = {n: i for i, n in enumerate(arr["sites"])}
    entry = lambda n: {k: f[k][-1, site[n]] for k in ("have", "n_rows", "n_bad", "first_bad_row", "absmax", "sumsq")}      # noqa: E731
    cu_a, cu_t = np.concatenate([[0], np.cumsum(LA)]), np.concatenate([[0], np.cumsum(LT)])
    worst = 0.0
    # the rows the encoder starts from: the bf16 copies of the caller's rows, packed
    for name, rows, cu, L in (("input.audio", rag[0], cu_a, PAD[0]), ("input.text", rag[1], cu_t, PAD[1])):
        x = rows.bfloat16()
        worst = max(worst, R.check_entry(entry(name), R.probe_ref64(x, NB, L, cu=cu), x.shape[0], D, 8, name))
    # the decoder's output: the bf16 member of the pair whose fp32 twin is z
    zb = z.bfloat16().reshape(NB * NE, D)
    worst = max(worst, R.check_entry(entry("dec1.ffn"), R.probe_ref64(zb, NB, NE), NB * NE, D, 8, "dec1.ffn"))
    worst = max(worst, R.check_entry(entry("logits"), R.probe_ref64(logits.reshape(NB, NE), NB, 1), NB, NE, 4, "logits"))
    print(f"activation log on the model: worst sumsq error / bound {worst:.3f}")
    rms = f["rms"][-1]
    assert np.isfinite(rms).all() and rms[site["dec1.ffn"]] == np.sqrt(float(f["sumsq"][-1, site["dec1.ffn"]]) / (NB * NE * D))
    # the counts of every site: audio / text / fused / query rows of the real sequences
    na, nt, nf, nq = sum(LA), sum(LT), sum(min(a, t) for a, t in zip(LA, LT)), NB * NE
    want = {"input.audio": na, "input.text": nt, "gate.w": NB, "gate.fused": nf, "logits": NB}
    for n in arr["sites"]:
        rows = want.get(n, na if ".audio_" in n else (nt if ".text_" in n else nq))
        assert f["n_rows"][-1, site[n]] == rows, (n, f["n_rows"][-1, site[n]], rows)
    # the padded run of the same batch agrees on n_rows and n_bad, forward and gradient
    m2 = _model(H, 2, p=0.0)
    log2 = _log(m2)
    log2.n_valid = torch.tensor([1], dtype=torch.int32, device="cuda")      # what a partial-batch step left behind: watch() forgets it
    _eager(m2, False, log2)
    arr2 = log2.arrays()
    assert arr2["n_recorded"] == 1
    # the sites reachable through the public modules, on the padded run (dropout 0: the sub-modules give the model's own bits):
    # the encoder's last outputs under the two padding masks, the gate's fused memory under their OR cut to the text length
    h_a, h_t, m_a, m_t = pad[:4]
    with torch.no_grad():
        ea, et = m2.cross_modal(h_a, h_t, m_a, m_t)
        hf, _ = m2.beta_gate(ea, et, m_a, m_t)
    assert log2.arrays()["n_passes"] == 1, "a sub-module called on its own is no pass of the log"
    f2 = arr2["forward"]
    entry2 = lambda n: {k: f2[k][-1, site[n]] for k in ("have", "n_rows", "n_bad", "first_bad_row", "absmax", "sumsq")}      # noqa: E731
    fused = (m_a[:, :PAD[1]] | m_t).cpu().numpy()
    for name, x, L, kpm in (("enc1.audio_ffn", ea, PAD[0], m_a.cpu().numpy()), ("enc1.text_ffn", et, PAD[1], m_t.cpu().numpy()),
                            ("gate.fused", hf, PAD[1], fused)):
        xb = x.bfloat16().reshape(NB * L, D)
        ref = R.probe_ref64(xb, NB, L, kpm=kpm)
        assert ref["n_rows"] == int((~kpm).sum()) and ref["sumsq"] > 0
        ratio = R.check_entry(entry2(name), ref, NB * L, D, 8, f"padded {name}")
        print(f"padded {name}: n_rows {ref['n_rows']} absmax {ref['absmax']} sumsq error / bound {ratio:.3f}")
        # the same site of the packed run saw the same rows: same counts, and values that differ by the packed kernels' rounding only
        assert entry(name)["n_rows"] == ref["n_rows"]
        assert abs(float(entry(name)["sumsq"]) - ref["sumsq"]) <= 1e-2 * ref["sumsq"], name
    for half in ("forward", "gradient"):
        for k in ("have", "n_rows", "n_bad"):
            assert arr[half][k][-1].tolist() == arr2[half][k][-1].tolist(), (half, k)
    assert log.row_len == log2.row_len
    # reset() clears the ring
    log.reset()
    assert log.arrays()["n_recorded"] == 0 and log.blame() is None


# ----------------------------------------------------------------------------- blame, from data alone
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "forward_packed"])
def test_blame_names_site_sample_and_position(H, packed):
    H.set_varlen(False)
    rag, pad = _batch()
    m0 = _model(H, 2, p=0.0)
    # (a) one NaN in one audio input row of sample 2
    l = 5
    bad_rag = (rag[0].clone(),) + rag[1:]
    bad_rag[0][LA[0] + LA[1] + l, 7] = NAN
    bad_pad = (pad[0].clone(),) + pad[1:]
    bad_pad[0][2, l, 7] = NAN
    _CACHE_was = _CACHE["b"]
    try:
        _CACHE["b"] = (bad_rag, bad_pad)
        m = copy.deepcopy(m0)
        log = _log(m)
        _eager(m, packed, log)
    finally:
        _CACHE["b"] = _CACHE_was
    b = log.blame()
    assert b == {"half": "forward", "site": "input.audio", "sample": 2, "position": l, "n_bad": 1}, b
    arr = log.arrays()
    s = {n: i for i, n in enumerate(arr["sites"])}
    assert arr["forward"]["n_bad"][-1, s["input.text"]] == 0 and arr["forward"]["n_bad"][-1, s["enc0.text_self"]] == 0
    assert arr["forward"]["n_bad"][-1, s["enc0.audio_self"]] > 0 and arr["forward"]["first_bad_row"][-1, s["enc0.audio_self"]] // PAD[0] == 2
    # (b) an Inf in the second weight of enc0's text FFN
    m = copy.deepcopy(m0)
    with torch.no_grad():
        m.cross_modal.layers[0].ffn_t[2].weight[3, 11] = INF
    log = _log(m)
    _eager(m, packed, log)
    b = log.blame()
    assert b["half"] == "forward" and b["site"] == "enc0.text_ffn" and b["sample"] == 0 and b["position"] == 0, b
    # (c) finite inputs, a NaN target: a clean forward, the gradient blame starts at the logits
    m = copy.deepcopy(m0)
    y = rag[4].clone()
    y[1, 2] = NAN
    log = _log(m)
    _eager(m, packed, log, y=y)
    arr = log.arrays()
    assert int(arr["forward"]["n_bad"].sum()) == 0
    b = log.blame()
    assert b["half"] == "gradient" and b["site"] == "logits", b


# ----------------------------------------------------------------------------- the captured trainer step
def _dp(m, log=None, stats=None, **opt_kw):
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.optim import DeviceAdamW
    from hri_emo_amd.train import fusion_step_loss
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    dp.set_global_batch(NB)
    if stats is not None:
        dp.attach_stats(stats)
    if log is not None:
        dp.attach_activations(log)
    return dp, DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0, **opt_kw)


def _stats_integers(stats):
    r = stats.result()
    return [int(r[k]) for k in ("n_samples", "n_batches", "n_skipped")] + [np.asarray(r[k]).tolist() for k in ("tp", "fp", "fn")]


@pytest.mark.parametrize("kw", [{}, {"partial_batches": True}, {"grad_accum": 2}], ids=["plain", "partial", "accum2"])
def test_captured_step_keeps_every_bit_and_warm_ups_leave_no_trace(H, kw):
    from hri_emo_amd import _ops
    from hri_emo_amd.train import EpochStats
    rag, _ = _batch()
    other = (rag[0][:sum(LA) - 9], rag[1], [20, 9, 5], LT, rag[4])            # fewer audio rows: another bucket, met mid-run
    short = _head(rag, 2)
    steps = [rag, other, rag, short if "partial_batches" in kw else rag]
    m0 = _model(H, 1)
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    runs = []
    for with_log in (False, True):
        _ops.seed_word(torch.device("cuda", 0)).copy_(word)
        m = copy.deepcopy(m0)
        log = _log(m, capacity=8) if with_log else None
        stats = EpochStats(NE, 64)
        dp, opt = _dp(m, log, stats)
        torch.manual_seed(23)
        dp.capture_packed(*rag, pad_to=PAD, optimizer=opt, **kw)
        if with_log:
            assert log.n_recorded == 0, "the warm-up passes of the capture recorded"
        losses = []
        for i, b in enumerate(steps):
            if "partial_batches" in kw and b is short:
                dp._static[4][2:] = NAN                                        # the ghost's targets may hold anything
            losses.append(dp.step_packed(*b).clone())
            if with_log:
                assert log.n_recorded == i + 1, f"step {i}: a new bucket's warm-up passes recorded"
        torch.cuda.synchronize()
        runs.append(losses + [p.detach().clone() for p in m.parameters()] + [dp.buckets.flat.clone(), opt.skipped.clone()])
        ints = _stats_integers(stats)
        runs[-1].append(torch.tensor(ints[:3]))
        runs[-1].append(torch.tensor(ints[3:]))
        if with_log:
            arr = log.arrays()
            assert arr["pass"].tolist() == [0, 1, 2, 3] and arr["halves"].tolist() == [3] * 4
            assert _missing(arr, "forward") == [] and _missing(arr, "gradient") == ["input.audio", "input.text", "gate.w"]
            assert log.blame() is None and int(arr["forward"]["n_bad"].sum()) == 0 and int(arr["gradient"]["n_bad"].sum()) == 0
            s = {n: i for i, n in enumerate(arr["sites"])}
            assert arr["forward"]["n_rows"][:, s["input.audio"]].tolist() == [sum(b[2]) for b in steps]      # fillers and ghosts never count
            assert arr["forward"]["n_rows"][:, s["logits"]].tolist() == [len(b[2]) for b in steps]
            assert arr["gradient"]["n_rows"][:, s["dec0.ffn"]].tolist() == [len(b[2]) * NE for b in steps]
        dp.release_graph()
    _same(runs[1], runs[0], f"captured step {kw}")


def test_captured_step_blames_the_input_row_that_made_the_optimizer_skip(H):
    from hri_emo_amd.optim import HealthLog
    rag, _ = _batch()
    m = _model(H, 1)
    log = _log(m)
    dp, opt = _dp(m, log, health=HealthLog(capacity=4))
    dp.capture_packed(*rag, pad_to=PAD, optimizer=opt)
    dp.step_packed(*rag)
    torch.cuda.synchronize()
    assert float(opt.skipped) == 0.0 and log.blame() is None
    bad = (rag[0].clone(),) + rag[1:]
    l = 3
    bad[0][LA[0] + LA[1] + l, 0] = NAN
    dp.step_packed(*bad)
    torch.cuda.synchronize()
    assert float(opt.skipped) == 1.0
    b = log.blame()
    assert b == {"half": "forward", "site": "input.audio", "sample": 2, "position": l, "n_bad": 1}, b
    assert opt.health.blame(), "the parameter-side log names the parameters, the activation log where it started"
    dp.step_packed(*rag)
    torch.cuda.synchronize()
    assert log.blame() is None and log.blame(record=-2) == b
    dp.release_graph()


def test_attach_comes_before_capture_and_every_skips_passes(H):
    rag, _ = _batch()
    m = _model(H, 1)
    dp, opt = _dp(m)
    dp.capture_packed(*rag, pad_to=PAD, optimizer=opt)
    with pytest.raises(RuntimeError, match="attach_activations"):
        dp.attach_activations(_log(m))
    dp.release_graph()
    m = _model(H, 1)
    log = _log(m, every=3, capacity=2)
    dp, opt = _dp(m, log)
    dp.capture_packed(*rag, pad_to=PAD, optimizer=opt)
    for _ in range(7):
        dp.step_packed(*rag)
    torch.cuda.synchronize()
    arr = log.arrays()
    assert arr["n_passes"] == 7 and arr["n_recorded"] == 3 and arr["pass"].tolist() == [3, 6]      # capacity 2: the ring wrapped
    dp.release_graph()


# ----------------------------------------------------------------------------- the captured evaluation
@pytest.mark.parametrize("stationary", [False, True], ids=["default", "stationary"])
def test_eval_step_records_the_forward_half_and_ghosts_blame_nothing(H, stationary):
    from hri_emo_amd.train import fusion_step_loss
    rag, _ = _batch()
    short = _head(rag, 2)
    m = _model(H, 2).eval()
    outs = []
    for with_log in (False, True):
        log = _log(m) if with_log else None
        es = H.EvalStep(m, fusion_step_loss, stationary=stationary, **({"act_log": log} if with_log else {}))
        es.capture_packed(*rag, pad_to=PAD)
        if with_log:
            assert log.n_recorded == 0
        res = [t.clone() for t in es.eval_packed(*rag)]
        # a short batch: the ghost's input rows (behind the batch's rows in the static sources) hold NaN
        es._static[0][sum(short[2]):] = NAN
        es._static[1][sum(short[3]):] = NAN
        res += [t.clone() for t in es.eval_packed(*short)]
        torch.cuda.synchronize()
        outs.append(res)
        if with_log:
            arr = log.arrays()
            assert arr["n_recorded"] == 2 and arr["halves"].tolist() == [1, 1]
            assert _missing(arr, "forward") == (["dec0.self"] if stationary else [])
            assert _missing(arr, "gradient") == arr["sites"]
            assert log.blame() is None and log.blame(record=0) is None and int(arr["forward"]["n_bad"].sum()) == 0
            s = {n: i for i, n in enumerate(arr["sites"])}
            assert arr["forward"]["n_rows"][:, s["input.text"]].tolist() == [sum(LT), sum(LT[:2])]
            assert arr["forward"]["n_rows"][:, s["logits"]].tolist() == [3, 2]
        es.release_graph()
    _same(outs[1], outs[0], "EvalStep with a log")
