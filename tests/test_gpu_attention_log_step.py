"""GPU suite of the attention log inside the captured evaluation: dp.EvalStep(attn_log=...), forward_packed(attn_log=...).

The logged maps come from the kernels of forward_packed(return_attention=True) with another store address, so they are compared
with torch.equal against that eager forward's maps for the same sample; logits, beta, z, the loss, EpochStats and PredictionLog
against an EvalStep without a log, also with torch.equal.  Shapes: those of test_gpu_eval_step.py (d = 128, B = 5, T_a = 70,
T_t = 40, a length-1 sequence in each modality), its parametrisation over precision and tail.  The golden case applies the
bounds of test_gpu_packed_maps.py: 2e-2 (bf16) and 1e-4 (fp32) of the largest reference value."""
import pytest
import torch

from conftest import load_golden
from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu

D, NE, NB, TA, TT = 128, 4, 5, 70, 40
PAD = (TA, TT)
#          audio lengths, text lengths                      bucket
EPOCH = [([70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),        # (160, 128)
         ([12, 70, 5, 40, 9], [8, 40, 3, 20, 7]),           # (144, 80): met mid-epoch, captured on the spot
         ([70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),
         ([20, 1, 44], [9, 40, 1])]                         # the short last batch: two ghost utterances
CAP = 12                                                    # takes 5, 5, 2, 0
MODES = [("bf16", False), ("bf16", True), ("fp32", True)]
MODE_IDS = ["bf16 tail off", "bf16 tail on", "fp32 tail on"]
SITES = ("audio_self", "text_self", "audio_queries_text", "text_queries_audio")


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    keep = (_ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.gemm_mode(), _ops.precision(), _ops.varlen_maps(),
            _ops.mfma_maps(), _ops.varlen(), _ops.ingest())
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    yield hri_emo_amd
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = keep[:3]
    hri_emo_amd.set_gemm_mode(keep[3])
    hri_emo_amd.set_precision(keep[4])
    hri_emo_amd.set_varlen_maps(keep[5])
    hri_emo_amd.set_mfma_maps(keep[6])
    hri_emo_amd.set_varlen(keep[7])
    hri_emo_amd.set_ingest(keep[8])


def _mode(H, precision, tail):
    from hri_emo_amd import _ops
    H.set_precision(precision)
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = _ops.PACKED_TAIL_MX8 = bool(tail)
    H.set_varlen_maps(True)


_CACHE = {}


def _epoch(da=D, dt=D, seed=11):
    """[(rows_a, rows_t, la, lt, y)] for EPOCH: made once per width, never changed"""
    if (da, dt) not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        out = []
        for la, lt in EPOCH:
            ra, rt = torch.randn(sum(la), da, generator=g).cuda(), torch.randn(sum(lt), dt, generator=g).cuda()
            out.append((ra, rt, list(la), list(lt), (torch.rand(len(la), NE, generator=g) < 0.3).float().cuda()))
        _CACHE[(da, dt)] = out
    return _CACHE[(da, dt)]


def _model(H):
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=0.0).cuda().train()


def _loss():
    from hri_emo_amd.train import fusion_step_loss
    return fusion_step_loss


def _eager_maps(m, batch):
    """the maps of the eager forward_packed(return_attention=True), eval mode, no_grad"""
    ra, rt, la, lt, _ = batch
    was = m.training
    m.eval()
    try:
        with torch.no_grad():
            pack = m.forward_packed(ra, rt, la, lt, pad_to=PAD, return_attention=True)[3]
    finally:
        m.train(was)
    torch.cuda.synchronize()
    return pack


def _keep(out):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.clone() for t in out)


def _log_state(log):
    torch.cuda.synchronize()
    return [log._small.clone()] + [t.clone() for t in log._tensors()]


def _same_state(log, state):
    torch.cuda.synchronize()
    return all(torch.equal(a, b) for a, b in zip([log._small] + log._tensors(), state))


def _against_eager(log, m, epoch, what, encoder=True, decoder=True):
    """every logged slot == the eager map of that sample; the lengths; returns the number of slots compared"""
    slot, cap = 0, log.capacity
    lens = log.lengths.cpu()
    for batch in epoch:
        if slot >= cap:
            break
        pack = _eager_maps(m, batch)
        n = min(len(batch[2]), cap - slot)
        pairs = []
        if encoder:
            pairs += [(f"enc.{li}.{k}", layer[k], log.encoder_maps[li][k]) for li, layer in enumerate(pack["encoder"]) for k in SITES]
        if decoder:
            pairs += [(f"dec.{li}", t, log.decoder_maps[li]) for li, t in enumerate(pack["decoder"])]
        for name, ref, mine in pairs:
            diff = float((mine[slot:slot + n] - ref[:n]).abs().max())
            if diff != 0.0:
                print(f"{what}: {name} slots {slot}..{slot + n - 1}: max |logged - eager| {diff:.3e}")
            assert torch.equal(mine[slot:slot + n], ref[:n]), (what, name, slot, diff)
        assert lens[:, slot:slot + n].tolist() == [batch[2][:n], batch[3][:n]], (what, "lengths", slot)
        slot += n
    return slot


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


def _passes(es, spy):
    """wrap es._pass: -> the list [(record, launch names)] that fills as passes run"""
    seen, real = [], es._pass

    def wrapped(record):
        spy.take()
        out = real(record)
        seen.append((record, spy.take()))
        return out

    es._pass = wrapped
    return seen


# ----------------------------------------------------------------------------- 1. the epoch
@pytest.mark.parametrize("precision,tail", MODES, ids=MODE_IDS)
def test_an_epoch_of_5_5_5_3_into_a_log_of_12(H, precision, tail):
    from hri_emo_amd.train import AttentionLog, EpochStats, PredictionLog
    _mode(H, precision, tail)
    m, epoch = _model(H), _epoch()
    plain = H.EvalStep(m, _loss(), stats=EpochStats(NE, 32), log=PredictionLog(NE, 32))
    alog = AttentionLog.for_model(m, CAP, PAD)
    es = H.EvalStep(m, _loss(), EpochStats(NE, 32), PredictionLog(NE, 32), None, attn_log=alog)          # max_graphs stays positional
    plain.capture_packed(*epoch[0], pad_to=PAD)
    fresh = _log_state(alog)
    es.capture_packed(*epoch[0], pad_to=PAD)
    assert _same_state_but_window(alog, fresh), "capture_packed (warm-up passes and the recording) touched the log"
    for i, batch in enumerate(epoch):
        ref = _keep(plain.eval_packed(*batch))
        got = _keep(es.eval_packed(*batch))
        for name, a, b in zip(("logits", "beta", "z", "loss"), got, ref):
            assert torch.equal(a, b), (precision, tail, i, name, float((a - b).abs().max()))
    assert len(es._pb.graphs) == 3          # the short batch's rows fit a smaller bucket: captured with the log already full
    assert alog.counters.tolist() == [CAP, 18, 4, 0] and alog.window.tolist() == [CAP, 0, 0, 0]
    assert torch.equal(es.stats._small, plain.stats._small) and torch.equal(es.log._buf, plain.log._buf)
    assert _against_eager(alog, m, epoch, f"{precision} tail {tail}") == CAP
    arr = alog.arrays()
    assert arr["n_logged"] == CAP and arr["n_offered"] == 18 and arr["encoder"][1]["text_queries_audio"].shape == (CAP, TT, TA)
    ref = alog.as_reference(NB)
    assert [len(b[0]["audio_self"]) for b in ref["encoder"]] == [5, 5, 2] and ref["decoder"][1][0].shape == (5, NE, 40)
    es.release_graph()
    plain.release_graph()


def _same_state_but_window(log, state):
    """bit-unchanged but for the window words (a closed window is written by every warm-up pass)"""
    torch.cuda.synchronize()
    now = [log._small.clone()] + log._tensors()
    now[0][4:8] = state[0][4:8]
    return all(torch.equal(a, b) for a, b in zip(now, state))


# ----------------------------------------------------------------------------- 2. ghosts, mid-epoch bucket
def test_ghost_utterances_are_never_logged(H):
    """the short batch first, into a log with room: 3 slots, not 5; then a full batch behind it"""
    from hri_emo_amd.train import AttentionLog
    _mode(H, "bf16", False)
    m, epoch = _model(H), _epoch()
    alog = AttentionLog.for_model(m, 16, PAD)
    es = H.EvalStep(m, _loss(), attn_log=alog)
    es.capture_packed(*epoch[0], pad_to=PAD)
    order = [epoch[3], epoch[0]]
    for batch in order:
        es.eval_packed(*batch)
    assert alog.counters.tolist() == [8, 8, 2, 0] and alog.window.tolist() == [3, 5, 0, 0]
    assert _against_eager(alog, m, order, "short batch first") == 8
    assert all(not bool(t[8:].any()) for t in alog._tensors()), "a slot behind the cursor was written"
    es.release_graph()


@pytest.mark.parametrize("precision,tail", MODES[1:], ids=MODE_IDS[1:])
def test_a_bucket_met_mid_epoch_leaves_the_log_alone_while_it_warms_up(H, monkeypatch, precision, tail):
    from hri_emo_amd.train import AttentionLog
    _mode(H, precision, tail)
    m, epoch = _model(H), _epoch()
    alog = AttentionLog.for_model(m, CAP, PAD)
    es = H.EvalStep(m, _loss(), attn_log=alog)
    es.capture_packed(*epoch[0], pad_to=PAD)
    es.eval_packed(*epoch[0])
    before = _log_state(alog)
    assert before[0][:4].tolist() == [5, 5, 1, 0]
    spy = Spy(monkeypatch)
    seen, real, checks = [], es._pass, []

    def wrapped(record):
        spy.take()
        out = real(record)
        names = spy.take()
        seen.append((record, names))
        if not record:
            checks.append(_same_state_but_window(alog, before) and alog.window.tolist() == [0, 0, 0, 0])
        return out

    es._pass = wrapped
    es.eval_packed(*epoch[1])                         # a new bucket: warm-up passes, the capture, then the replay
    assert len(es._pb.graphs) == 2 and [r for r, _ in seen][-1] is True and len(seen) >= 2
    assert checks and all(checks), "a warm-up pass moved the log"
    for record, names in seen:
        assert names.count("hriemo_attn_log_plan") == (1 if record else 0) and names.count("hriemo_attn_log_close") == (0 if record else 1)
    assert alog.counters.tolist() == [10, 10, 2, 0]
    assert all(torch.equal(a[:5], b[:5]) for a, b in zip(alog._tensors(), before[1:])), "the first batch's slots moved"
    assert _against_eager(alog, m, epoch[:2], "mid-epoch bucket") == 10
    es.release_graph()


# ----------------------------------------------------------------------------- 3. launches
@pytest.mark.parametrize("encoder", [True, False], ids=["both halves", "decoder only"])
@pytest.mark.parametrize("precision,tail", MODES, ids=MODE_IDS)
def test_launches_of_the_recorded_pass(H, monkeypatch, precision, tail, encoder):
    from hri_emo_amd.train import AttentionLog
    _mode(H, precision, tail)
    m, epoch = _model(H), _epoch()
    alog = AttentionLog.for_model(m, CAP, PAD, encoder=encoder)
    es = H.EvalStep(m, _loss(), attn_log=alog)
    spy = Spy(monkeypatch)
    seen = _passes(es, spy)
    es.capture_packed(*epoch[0], pad_to=PAD)
    recorded = [names for record, names in seen if record]
    assert len(recorded) == 1 and seen[-1][0] is True
    names = recorded[0]
    f32 = precision == "fp32"
    logged, plain = ("hriemo_attn_probs_varlen_log_fp32", "hriemo_attn_probs_f32_varlen") if f32 else ("hriemo_attn_probs_varlen_log", "hriemo_attn_probs_varlen")
    padded = ("hriemo_attn_probs_f32",) if f32 else ("hriemo_attn_probs", "hriemo_attn_probs_mfma")
    layers, dec = len(m.cross_modal.layers), len(m.emotion_decoder.layers)
    assert names.count("hriemo_attn_log_plan") == 1 and names.count("hriemo_attn_log_close") == 0
    assert names.index("hriemo_attn_log_plan") == names.index("hriemo_seq_tables") + 1, "the plan sits directly behind the tables"
    assert names.count(logged) == (4 * layers if encoder else 0) + (dec if tail else 0), names.count(logged)
    assert names.count(plain) == 0, "a varlen site exported into a tensor of its own"
    assert sum(names.count(p) for p in padded) == (0 if tail else dec)
    assert names.count("hriemo_attn_log_append") == (0 if tail else dec)
    for record, warm in seen[:-1]:
        assert not record and warm.count("hriemo_attn_log_plan") == 0 and warm.count("hriemo_attn_log_close") == 1
        assert warm.count(logged) == names.count(logged)          # the same launch list, under the closed window
    # the decoder-only log still holds the decoder's maps of the eager forward
    for batch in epoch[:2]:
        es.eval_packed(*batch)
    assert _against_eager(alog, m, epoch[:2], f"{precision} tail {tail} encoder {encoder}", encoder=encoder) == 10
    assert alog.encoder_maps == [] or encoder
    es.release_graph()


# ----------------------------------------------------------------------------- 4. the golden
def _close(got, ref, tol, what):
    err = float((got - ref).abs().max())
    assert err <= tol * max(1.0, float(ref.abs().max())), (what, err)
    return err


@pytest.mark.parametrize("precision,tail", MODES, ids=MODE_IDS)
def test_the_ragged_golden_as_batches_of_5_and_3(H, precision, tail):
    """cfg1_eval_ragged, B = 8, through graphs captured for 5: the logged maps against the golden maps on the valid query rows"""
    from hri_emo_amd.train import AttentionLog
    tol = 1e-4 if precision == "fp32" else 2e-2          # test_gpu_packed_maps.py's map bounds
    _mode(H, precision, tail)
    g = load_golden("cfg1_eval_ragged")
    m = O.closed_form_init_(H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.1)).cuda().eval()
    ma, mt = g["mask_a"], g["mask_t"]
    la, lt = (~ma).sum(1).tolist(), (~mt).sum(1).tolist()
    pad = (g["h_a"].shape[1], g["h_t"].shape[1])
    assert len(la) == 8

    def rows(lo, hi):
        ra = torch.cat([g["h_a"][b, :la[b]] for b in range(lo, hi)]).cuda()
        rt = torch.cat([g["h_t"][b, :lt[b]] for b in range(lo, hi)]).cuda()
        return ra, rt, la[lo:hi], lt[lo:hi]

    alog = AttentionLog.for_model(m, 8, pad)
    es = H.EvalStep(m, attn_log=alog)
    es.capture_packed(*rows(0, 5), pad_to=pad)
    out = [_keep(es.eval_packed(*rows(lo, hi))) for lo, hi in ((0, 5), (5, 8))]
    logits = torch.cat([o[0] for o in out]).float().cpu()
    _close(logits, g["logits"].float(), 1e-4 if precision == "fp32" else 5e-3, "logits")
    arr = alog.arrays()
    assert arr["n_logged"] == 8 and arr["lengths"].tolist() == [la, lt]
    valid = {"a": ~ma, "t": ~mt}
    qk = {"audio_self": "aa", "text_self": "tt", "audio_queries_text": "at", "text_queries_audio": "ta"}
    worst = 0.0
    for li in range(2):
        for k in SITES:
            got, gold = torch.from_numpy(arr["encoder"][li][k]), g[f"enc.{li}.{k}"].float()
            assert got.shape == gold.shape, (k, got.shape, gold.shape)
            rws = valid[qk[k][0]][:, :, None].expand_as(got)
            worst = max(worst, _close(torch.where(rws, got, gold), gold, tol, f"enc.{li}.{k}"))
            assert not bool(got[~rws].any()), (k, "PAD query rows are zeros")
        got, gold = torch.from_numpy(arr["decoder"][li]), g[f"dec.{li}"].float()
        assert got.shape == gold.shape
        worst = max(worst, _close(got, gold, tol, f"dec.{li}"))
    print(f"cfg1_eval_ragged {precision} tail {tail}: worst logged map error vs the golden {worst:.2e} (bound {tol:.0e})")
    es.release_graph()


# ----------------------------------------------------------------------------- 5. wrapper, eager, refusals
def test_the_mosei_wrapper(H):
    from hri_emo_amd.train import AttentionLog
    _mode(H, "bf16", True)
    epoch = _epoch(74, 300, 5)
    torch.manual_seed(3)
    m = H.MoseiFusionWithEmotionDecoder(d_audio=74, d_text=300, d_model=D, num_emotions=NE, n_heads=8, dropout=0.2).cuda().train()
    alog = AttentionLog.for_model(m, CAP, PAD)
    assert alog.num_emotions == NE and alog.mismatch(m, PAD) is None
    es = H.EvalStep(m, attn_log=alog)
    es.capture_packed(*epoch[0][:4], pad_to=PAD)
    for batch in epoch:
        es.eval_packed(*batch[:4])
    assert alog.counters.tolist() == [CAP, 18, 4, 0]
    assert _against_eager(alog, m, epoch, "MOSEI wrapper") == CAP
    es.release_graph()


@pytest.mark.parametrize("precision,tail", MODES, ids=MODE_IDS)
def test_eager_equals_captured_bit_for_bit(H, precision, tail):
    """use_graph(False) is forward_packed(attn_log=...): the same log, the same outputs; and forward_packed(attn_log=...) on its own"""
    from hri_emo_amd.train import AttentionLog
    _mode(H, precision, tail)
    m, epoch = _model(H), _epoch()
    alog = AttentionLog.for_model(m, CAP, PAD)
    es = H.EvalStep(m, _loss(), attn_log=alog)
    es.capture_packed(*epoch[0], pad_to=PAD)
    outs = [_keep(es.eval_packed(*batch)) for batch in epoch]
    captured = _log_state(alog)
    alog.reset()
    for t in alog._tensors():
        t.zero_()
    es.use_graph(False)
    for batch, ref in zip(epoch, outs):
        got = _keep(es.eval_packed(*batch))
        for name, a, b in zip(("logits", "beta", "z", "loss"), got, ref):
            diff = float((a - b).abs().max())
            if diff != 0.0:
                print(f"{precision} tail {tail}: eager {name} differs from captured by {diff:.3e}")
            assert torch.equal(a, b), (name, diff)
    assert _same_state(alog, captured), "the eager evaluation left another log than the replays"
    es.release_graph()
    # the model's own entry: the 3-tuple, the log fed
    alog.reset()
    m.eval()
    with torch.no_grad():
        out = m.forward_packed(*epoch[3][:4], pad_to=PAD, attn_log=alog)
    m.train()
    assert len(out) == 3 and alog.counters.tolist() == [3, 3, 1, 0]
    assert _against_eager(alog, m, [epoch[3]], "forward_packed(attn_log=)") == 3


def test_append_on_the_device_equals_the_cpu_twin(H):
    """AttentionLog.append (hriemo_attn_log_plan + one hriemo_attn_log_append per site) against the same maps through the CPU twin:
    5, 5, 3-of-5 into a log of 12"""
    from hri_emo_amd.train import AttentionLog
    kw = dict(capacity=CAP, pad_to=(9, 5), num_layers_fusion=1, num_layers_decoder=2, num_emotions=3)
    dev, cpu = AttentionLog(device="cuda", **kw), AttentionLog(device="cpu", **kw)
    g = torch.Generator().manual_seed(2)
    dims = dict(zip(SITES, ((9, 9), (5, 5), (9, 5), (5, 9))))
    for n_valid in (None, None, 3):
        maps = {"encoder": [{k: torch.rand(NB, *dims[k], generator=g) for k in SITES}], "decoder": [torch.rand(NB, 3, 5, generator=g) for _ in range(2)]}
        lens = torch.stack([torch.randint(1, 10, (NB,), generator=g), torch.randint(1, 6, (NB,), generator=g)]).to(torch.int32)
        cpu.append(maps, lens, n_valid)
        on_dev = {"encoder": [{k: v.cuda() for k, v in maps["encoder"][0].items()}], "decoder": [t.cuda() for t in maps["decoder"]]}
        dev.append(on_dev, lens, None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert dev.counters.tolist() == cpu.counters.tolist() == [CAP, 13, 3, 0] and dev.window.tolist() == cpu.window.tolist() == [10, 2, 0, 0]
    assert torch.equal(dev._small.cpu(), cpu._small)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(dev._tensors(), cpu._tensors()))
    a, b = dev.as_reference(NB), cpu.as_reference(NB)
    assert [x.shape for x in a["decoder"][2]] == [x.shape for x in b["decoder"][2]] and len(a["encoder"]) == 3


def test_refusals_leave_the_step_and_the_log_untouched(H):
    from hri_emo_amd.train import AttentionLog
    _mode(H, "bf16", True)
    m, epoch = _model(H), _epoch()
    alog = AttentionLog.for_model(m, CAP, PAD)
    es = H.EvalStep(m, _loss(), attn_log=alog)
    es.capture_packed(*epoch[0], pad_to=PAD)
    es.eval_packed(*epoch[0])
    state = _log_state(alog)
    graphs, static = dict(es._pb.graphs), [None if t is None else t.clone() for t in es._static]

    def untouched():
        return (_same_state(alog, state) and dict(es._pb.graphs) == graphs
                and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(es._static, static)))

    # capture without the packed export: ValueError, the old graphs stay
    H.set_varlen_maps(False)
    with pytest.raises(ValueError, match="set_varlen_maps"):
        es.capture_packed(*epoch[1], pad_to=PAD)
    with pytest.raises(RuntimeError, match="varlen_maps"):
        es.eval_packed(*epoch[0])
    m.eval()
    with pytest.raises(ValueError, match="set_varlen_maps"), torch.no_grad():
        m.forward_packed(*epoch[0][:4], pad_to=PAD, attn_log=alog)
    H.set_varlen_maps(True)
    assert untouched()
    with pytest.raises(ValueError, match="exclude"), torch.no_grad():
        m.forward_packed(*epoch[0][:4], pad_to=PAD, attn_log=alog, return_attention=True)
    with pytest.raises(ValueError, match="pad_to"), torch.no_grad():
        m.forward_packed(*epoch[0][:4], pad_to=(TA + 2, TT), attn_log=alog)
    with pytest.raises(ValueError, match="pad_to"), torch.no_grad():
        m._forward_rows(epoch[0][0], epoch[0][1], None, None, (TA + 2, TT), attn_log=alog)
    m.train()
    assert untouched()
    # a log that does not fit: the mismatch is named, nothing is released
    for kw, word in ((dict(pad_to=(TA + 2, TT)), "pad_to"), (dict(num_layers_fusion=3), "num_layers_fusion"),
                     (dict(num_layers_decoder=1), "num_layers_decoder"), (dict(num_emotions=6), "num_emotions")):
        args = dict(capacity=4, pad_to=PAD, num_layers_fusion=2, num_layers_decoder=2, num_emotions=NE)
        args.update(kw)
        es.attn_log = AttentionLog(**args)
        with pytest.raises(ValueError, match=word):
            es.capture_packed(*epoch[0], pad_to=PAD)
    es.attn_log = alog
    assert untouched()
    # a switch that picks the export kernel moved since the capture
    H.set_mfma_maps(not H.mfma_maps())
    with pytest.raises(RuntimeError, match="mfma_maps"):
        es.eval_packed(*epoch[0])
    H.set_mfma_maps(not H.mfma_maps())
    assert untouched()
    es.eval_packed(*epoch[1])
    assert alog.counters.tolist() == [10, 10, 2, 0]
    # without a log the recorded switches are exactly the six of before
    plain = H.EvalStep(m, _loss())
    plain.capture_packed(*epoch[0], pad_to=PAD)
    assert [n for n, _ in plain._modes] == ["precision", "gemm_mode", "PACKED_TAIL", "PACKED_TAIL_FP32", "PACKED_TAIL_MX8", "ingest"]
    assert [n for n, _ in es._modes][6:] == ["varlen_maps", "mfma_maps"]
    plain.release_graph()
    es.release_graph()
