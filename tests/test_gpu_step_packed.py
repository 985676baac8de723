"""GPU suite of the ragged front door of the captured trainer step: DataParallelStep.capture_packed / step_packed (packed rows and
host lengths in; hriemo_seq_tables as the first launch of every bucket graph) against the eager padded step (the 1e-5 packed-
against-padded bound of DESIGN 1), against the mask-fed captured step (torch.equal: the ingest launch writes the same bits from
either source layout, the bucket plans and every table are the same), with the optimizer in the graph, through the MOSEI wrapper,
its refusals, and data.DevicePrefetcher(ragged=...).  Shapes: those of test_gpu_forward_packed.py (d128: B = 5, T_a = 70, T_t = 40,
bucket granule 8 rows); three batches that land in three row-count buckets."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

D, NE, NB, TA, TT = 128, 4, 5, 70, 40
LENGTHS = [([70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),          # 153 / 120 rows -> buckets 160 / 128
           ([12, 70, 5, 40, 9], [8, 40, 3, 20, 7]),             # 136 / 78        -> 144 / 80
           ([TA] * NB, [TT] * NB)]                              # all full: 350 / 200 -> 352 / 208 (the surplus sequence lies past B*L)
KEYS = [(160, 128), (144, 80), (352, 208)]


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    keep = (_ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.gemm_mode(), _ops.precision())
    word = _ops.seed_word(torch.device("cuda", 0)).clone()           # a captured step bumps it on every replay; later tests
    yield hri_emo_amd                                                # replay dropout masks from it
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_ingest(False)
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8 = keep[:3]
    hri_emo_amd.set_gemm_mode(keep[3])
    hri_emo_amd.set_precision(keep[4])


def _tail(on):
    from hri_emo_amd import _ops
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = _ops.PACKED_TAIL_MX8 = bool(on)


def _make(da, dt, seed):
    """[(padded batch (h_a, h_t, m_a, m_t, y), ragged batch (rows_a, rows_t, la, lt, y))] for LENGTHS, widths da / dt"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for la, lt in LENGTHS:
        h_a, h_t = torch.randn(NB, TA, da, generator=g).cuda(), torch.randn(NB, TT, dt, generator=g).cuda()
        m_a = (torch.arange(TA)[None] >= torch.tensor(la)[:, None]).cuda()
        m_t = (torch.arange(TT)[None] >= torch.tensor(lt)[:, None]).cuda()
        h_a[m_a], h_t[m_t] = 0.0, 0.0                                     # zero padding, as the collate pads
        y = (torch.rand(NB, NE, generator=g) < 0.3).float().cuda()
        out.append(((h_a, h_t, m_a, m_t, y), (h_a[~m_a].contiguous(), h_t[~m_t].contiguous(), la, torch.tensor(lt), y)))
    return out


_CACHE = {}


def _batches():
    if "b" not in _CACHE:
        _CACHE["b"] = _make(D, D, 11)
    return _CACHE["b"]


def _model(H, p=0.0):
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=8, dropout=p).cuda().train()


def _dp(m):
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    dp.set_global_batch(NB)
    return dp


def _padded_reference(H, precision):
    """the eager padded step (varlen off, tails off, dropout 0) on every batch: computed once per precision, never changed"""
    if precision not in _CACHE:
        H.set_precision(precision)
        H.set_varlen(False)
        H.set_ingest(False)
        _tail(False)
        dp = _dp(_model(H))
        _CACHE[precision] = [(float(dp.step(*pad)), dp.buckets.flat.clone()) for pad, _ in _batches()]
    return _CACHE[precision]


class Spy:
    """records the name of every _lib.call"""

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


def _host_tables(la, lt):
    """what the host path makes of the lengths: packed_tables' cu_seqlens (the lists _packed_key uploads) and plans_from_lengths' masks"""
    from hri_emo_amd import _ops, dp as dpm
    lt = [int(x) for x in lt]
    key, *cus = dpm.packed_tables(*dpm.mask_lengths(None, None, (la, lt), NB, TA, TT), NB, TA, TT)
    host = {name: torch.tensor(cu, dtype=torch.int32) for name, cu in zip(("cu_a", "cu_t", "cu_f"), cus)}
    plans, (m_a, m_t) = _ops.plans_from_lengths(la, lt, TA, TT, torch.device("cuda", 0))
    return key, host, plans, (m_a, m_t, m_a[:, :TT] | m_t)


def _assert_tables(dp, la, lt):
    key, host, plans, masks = _host_tables(la, lt)
    pb = dp._pb
    for name, plan in zip(("cu_a", "cu_t", "cu_f"), plans):
        dev = getattr(pb, name)
        assert torch.equal(dev.cpu(), host[name]), (name, dev.tolist(), host[name].tolist())
        assert torch.equal(dev[:NB + 1], plan.cu), name
    for got, ref, name in zip(pb.front.masks, masks, ("mask_a", "mask_t", "mask_f")):
        assert got.dtype == torch.uint8 and torch.equal(got.view(torch.bool), ref), name
    assert pb.front.lens.dev.tolist() == [list(la), [int(x) for x in lt]]
    return key


def _assert_launches(names, passes, tail):
    """`passes` passes of the step: hriemo_seq_tables once per pass and first in it, hriemo_ingest_rows once per modality, and no
    hriemo_pack_rows takes a module input in: with the tail packed there is none at all; with the tail unpacked the only ones are
    the two gradient gathers of the encoder outputs' scatter (UnpackFn.backward), behind the loss launch of their pass"""
    assert names.count("hriemo_seq_tables") == passes and names.count("hriemo_ingest_rows") == 2 * passes, names
    assert names.count("hriemo_pack_rows") == (0 if tail else 2 * passes), names.count("hriemo_pack_rows")
    backward = False
    for n in names:
        if n == "hriemo_seq_tables":
            backward = False
        elif n.startswith("hriemo_fusion_loss"):
            backward = True
        elif n == "hriemo_pack_rows":
            assert backward, "a hriemo_pack_rows launch in a forward pass"
    if passes:
        assert any(n.startswith("hriemo_fusion_loss") for n in names)


# ----------------------------------------------------------------------------- against the eager padded step
@pytest.mark.parametrize("precision,tail", [("bf16", False), ("bf16", True), ("fp32", True)],
                         ids=["bf16 tail off", "bf16 tail on", "fp32 tail on"])
def test_step_packed_against_the_eager_padded_step(H, monkeypatch, precision, tail):
    """three batches over three buckets: loss within 1e-5 * max(1, |ref|) and flat gradients within 1e-5 relative L2 of the eager
    padded step; a second replay of the first batch bit-identical; one graph per distinct bucket key; every pass of a bucket's
    capture (two warm-ups + the capture) launches hriemo_seq_tables once and hriemo_ingest_rows once per modality, a replay
    launches nothing from the host, nothing packs; after every step the device tables equal the host's"""
    ref = _padded_reference(H, precision)
    H.set_precision(precision)
    H.set_varlen(False)                              # the ragged front door runs the packed encoder whatever set_varlen says
    _tail(tail)
    dp = _dp(_model(H))
    spy = Spy(monkeypatch)
    first = _batches()[0][1]
    dp.capture_packed(*first, pad_to=(TA, TT))
    names = spy.take()
    assert names[0] == "hriemo_seq_tables", names[:3]
    _assert_launches(names, 3, tail)
    keys, once = [], None
    for i, (_, rag) in enumerate(_batches()):
        loss = float(dp.step_packed(*rag))
        torch.cuda.synchronize()
        names = spy.take()
        keys.append(_assert_tables(dp, rag[2], rag[3]))
        assert keys[-1] == KEYS[i]
        passes = 0 if i == 0 else 3                  # a bucket met for the first time is captured on the spot
        _assert_launches(names, passes, tail)
        rel = float((dp.buckets.flat - ref[i][1]).norm() / ref[i][1].norm())
        print(f"{precision} tail {tail} batch {i}: loss {loss:.7f} vs {ref[i][0]:.7f}, flat gradients relative L2 {rel:.2e}")
        assert abs(loss - ref[i][0]) <= 1e-5 * max(1.0, abs(ref[i][0])), (i, loss, ref[i][0])
        assert rel <= 1e-5, (i, rel)
        if i == 0:
            once = (loss, dp.buckets.flat.clone())
    loss = float(dp.step_packed(*first))
    torch.cuda.synchronize()
    assert loss == once[0] and torch.equal(dp.buckets.flat, once[1]), "a second replay of the first batch"
    assert spy.take() == [], "a replay of a known bucket launches nothing from the host"
    assert len(dp._pb.graphs) == len(set(keys)) == 3
    # use_graph(False): the eager forward_packed step on the same batch
    dp.use_graph(False)
    eager = float(dp.step_packed(*first))
    rel = float((dp.buckets.flat - once[1]).norm() / once[1].norm())
    assert abs(eager - once[0]) <= 1e-5 * max(1.0, abs(once[0])) and rel <= 1e-5, (eager, once[0], rel)
    dp.release_graph()


# ----------------------------------------------------------------------------- against the mask-fed captured step
def _captured_run(m0, packed, word, opt_steps=0):
    """on a copy of m0 (a copy keeps the dropout sites of its modules, a second model from the same seed would not): capture on
    batch 0, every batch once, batch 0 again -> [(loss, flat gradients)] (and the parameters after `opt_steps` optimizer-in-graph
    steps instead when asked)"""
    from hri_emo_amd import _ops
    from hri_emo_amd.optim import DeviceAdamW
    dp = _dp(copy.deepcopy(m0))
    opt = DeviceAdamW(dp.buckets, lr=1e-3, weight_decay=1e-2, max_norm=5.0) if opt_steps else None
    before = opt.flat_p.clone() if opt_steps else None
    torch.manual_seed(5)                             # the warm-up and capture passes draw their dropout seeds from torch's generator
    pad0, rag0 = _batches()[0]
    if packed:
        dp.capture_packed(*rag0, pad_to=(TA, TT), optimizer=opt)
    else:
        dp.capture(*pad0, lengths=(rag0[2], rag0[3].tolist()), optimizer=opt)
    if opt_steps:
        torch.cuda.synchronize()
        assert torch.equal(opt.flat_p, before) and float(opt.device_step) == 0.0, "capture itself moves nothing"
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)              # both arms replay from the same seed word
    out = []
    order = [0, 1, 2, 0] if not opt_steps else list(range(opt_steps))
    for i in order:
        pad, rag = _batches()[i]
        loss = dp.step_packed(*rag) if packed else dp.step(*pad, lengths=(rag[2], rag[3].tolist()))
        torch.cuda.synchronize()
        out.append((loss.clone(), dp.buckets.flat.clone()))
    n_graphs = len(dp._pb.graphs)
    params = (before, opt.flat_p.clone(), float(opt.device_step)) if opt_steps else None
    dp.release_graph()
    return out, n_graphs, params


@pytest.mark.parametrize("p,tail", [(0.0, False), (0.1, False), (0.1, True)], ids=["p 0 tail off", "p 0.1 tail off", "p 0.1 tail on"])
def test_step_packed_equals_the_mask_fed_captured_step(H, p, tail):
    """capture / step(..., lengths=) with set_varlen(True) and set_ingest(True) against capture_packed / step_packed on the same
    batches and buckets: every loss and every flat gradient torch.equal, dropout included"""
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    H.set_varlen(True)
    H.set_ingest(True)
    _tail(tail)
    m0 = _model(H, p)
    fed, n_fed, _ = _captured_run(m0, False, word)
    rag, n_rag, _ = _captured_run(m0, True, word)
    assert n_fed == n_rag == 3
    for i, ((la, ga), (lb, gb)) in enumerate(zip(fed, rag)):
        assert torch.equal(la, lb), (i, float(la), float(lb))
        assert torch.equal(ga, gb), (i, int((ga != gb).sum()))
    if p > 0:
        assert not torch.equal(rag[0][1], rag[3][1]), "dropout is fresh per replay: the seed word moved between the two replays of batch 0"


def test_optimizer_in_the_graph_equals_the_mask_fed_step(H):
    """capture_packed(optimizer=DeviceAdamW): after two step_packed calls the parameters equal those of two mask-fed captured steps
    on the same batches, bit for bit; capture itself moved nothing"""
    from hri_emo_amd import _ops
    word = _ops.seed_word(torch.device("cuda", 0)).clone()
    H.set_varlen(True)
    H.set_ingest(True)
    _tail(True)
    m0 = _model(H)
    _, _, fed = _captured_run(m0, False, word, opt_steps=2)
    _, _, rag = _captured_run(m0, True, word, opt_steps=2)
    assert torch.equal(fed[0], rag[0]) and fed[2] == rag[2] == 2.0
    assert torch.equal(fed[1], rag[1]), int((fed[1] != rag[1]).sum())
    assert bool(torch.isfinite(rag[1]).all()) and not torch.equal(rag[1], rag[0]), "two updates moved the parameters"


# ----------------------------------------------------------------------------- MOSEI wrapper
def test_mosei_step_packed(H):
    """d_audio 74, d_text 300, d = 128: the projections run over the bucket's rows of the static sources, so the rows behind the
    batch must be finite -- NaN planted there BEFORE the step is zeroed by the trainer.  Results finite and within 1e-5 of the
    eager padded step."""
    batches = _make(74, 300, 5)
    torch.manual_seed(3)
    m0 = H.MoseiFusionWithEmotionDecoder(d_audio=74, d_text=300, d_model=D, num_emotions=NE, n_heads=8, dropout=0.0).cuda().train()
    H.set_varlen(False)
    _tail(False)
    dp = _dp(copy.deepcopy(m0))
    ref = [(float(dp.step(*pad)), dp.buckets.flat.clone()) for pad, _ in batches]
    _tail(True)
    dp = _dp(copy.deepcopy(m0))
    dp.capture_packed(*batches[0][1], pad_to=(TA, TT))
    assert dp._static[0].shape == (KEYS[2][0], 74) and dp._static[1].shape == (KEYS[2][1], 300)       # the largest bucket
    for i, (_, rag) in enumerate(batches):
        for src, n in ((dp._static[0], rag[0].shape[0]), (dp._static[1], rag[1].shape[0])):
            src[n:] = float("nan")
        loss = float(dp.step_packed(*rag))
        torch.cuda.synchronize()
        flat = dp.buckets.flat
        assert bool(torch.isfinite(flat).all()) and loss == loss, (i, loss)
        rel = float((flat - ref[i][1]).norm() / ref[i][1].norm())
        print(f"mosei batch {i}: loss {loss:.7f} vs {ref[i][0]:.7f}, flat gradients relative L2 {rel:.2e}")
        assert abs(loss - ref[i][0]) <= 1e-5 * max(1.0, abs(ref[i][0])), (i, loss, ref[i][0])
        assert rel <= 1e-5, (i, rel)
    dp.release_graph()


# ----------------------------------------------------------------------------- refusals
def test_refusals_leave_the_static_state_untouched(H):
    dp = _dp(_model(H))
    ra, rt, la, lt, y = _batches()[0][1]
    with pytest.raises(RuntimeError, match="capture_packed"):
        dp.step_packed(ra, rt, la, lt, y)
    with pytest.raises(ValueError, match="pad_to"):
        dp.capture_packed(ra, rt, la, lt, y, pad_to=None)
    dp.capture_packed(ra, rt, la, lt, y, pad_to=(TA, TT))
    dp.step_packed(ra, rt, la, lt, y)
    torch.cuda.synchronize()
    front = dp._pb.front
    state = lambda: [t.clone() for t in (dp._static[0], dp._static[1], dp._static[4], front.lens.dev, front.lens.host, dp._pb.cu_a,      # noqa: E731
                                         dp._pb.cu_t, dp._pb.cu_f) + front.masks]
    before = state()
    lt = lt.tolist()
    bad = {
        "another B": (ra[:sum(la[:4])], rt[:sum(lt[:4])], la[:4], lt[:4], y[:4]),
        "a length of 0": (ra, rt, [la[0] - 1, 0] + la[2:], lt, y),
        "a length past L": (ra, rt, la, [TT + 1] + lt[1:], y),
        "rows that do not add up": (ra[:-1], rt, la, lt, y),
        "a CUDA lengths tensor": (ra, rt, torch.tensor(la).cuda(), lt, y),
        "another width": (ra[:, :64].contiguous(), rt[:, :64].contiguous(), la, lt, y),
    }
    for what, args in bad.items():
        with pytest.raises(ValueError) as e:
            dp.step_packed(*args)
        if what == "another B":
            assert "B = 5" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        for a, b in zip(before, state()):
            assert torch.equal(a, b), what
    with pytest.raises(RuntimeError, match="step_packed"):
        dp.step(*_batches()[0][0])
    dp.release_graph()


# ----------------------------------------------------------------------------- who owns a captured graph
def test_bucket_graph_accounting_after_capture_packed(H, monkeypatch):
    """cap 2, the three batches of three buckets: _ops.GRAPHS_ALIVE counts exactly the entries of the graphs mapping after every
    step_packed, the evicted (first-captured) bucket's graph object dies with its record, the bucket that comes back reproduces
    loss and gradients bit for bit, and release_graph() returns the count to where it started"""
    import gc
    import weakref
    from hri_emo_amd import _ops, dp as dpmod
    monkeypatch.setattr(dpmod, "_VARLEN_MAX_GRAPHS", 2)
    _tail(True)
    dp = _dp(_model(H))
    rags = [rag for _, rag in _batches()]
    alive0 = _ops.GRAPHS_ALIVE
    dp.capture_packed(*rags[0], pad_to=(TA, TT))
    assert _ops.GRAPHS_ALIVE == alive0 + 1 and dp.captured and list(dp._pb.graphs) == [KEYS[0]]
    graph0 = weakref.ref(dp._pb.graphs[KEYS[0]].graph)
    first = float(dp.step_packed(*rags[0]))
    g0 = dp.buckets.flat.clone()
    for i in (1, 2):
        dp.step_packed(*rags[i])
        assert _ops.GRAPHS_ALIVE == alive0 + len(dp._pb.graphs) == alive0 + min(i + 1, 2)
    assert list(dp._pb.graphs) == [KEYS[1], KEYS[2]], "the first-captured bucket is the one evicted"
    gc.collect()
    assert graph0() is None, "the evicted bucket's graph is still alive: something besides the graphs mapping held it"
    again = float(dp.step_packed(*rags[0]))                # captured afresh, bucket 1 goes
    torch.cuda.synchronize()
    assert list(dp._pb.graphs) == [KEYS[2], KEYS[0]] and _ops.GRAPHS_ALIVE == alive0 + 2
    assert again == first and torch.equal(dp.buckets.flat, g0)
    dp.release_graph()
    assert _ops.GRAPHS_ALIVE == alive0 and not dp.captured
    if alive0 == 0:
        assert _ops._ws_retired == []


def test_two_captured_steps_in_one_process_count_and_release_independently(H):
    """one DataParallelStep captured plain (padded), one by capture_packed with two bucket graphs: the counter is the sum of their
    records; releasing either leaves the other's replay bit-identical to its replay before"""
    from hri_emo_amd import _ops
    H.set_varlen(False)
    _tail(True)
    m0 = _model(H)
    plain, packed = _dp(copy.deepcopy(m0)), _dp(copy.deepcopy(m0))
    (pad0, rag0), (_, rag1) = _batches()[:2]
    alive0 = _ops.GRAPHS_ALIVE

    def replay_plain():
        loss = plain.step(*pad0)
        torch.cuda.synchronize()
        return loss.clone(), plain.buckets.flat.clone()

    def replay_packed():
        out = []
        for rag in (rag0, rag1):
            loss = packed.step_packed(*rag)
            torch.cuda.synchronize()
            out += [loss.clone(), packed.buckets.flat.clone()]
        return out

    plain.capture(*pad0)
    assert plain._record is not None and plain._pb is None and _ops.GRAPHS_ALIVE == alive0 + 1
    packed.capture_packed(*rag0, pad_to=(TA, TT))
    was_packed = replay_packed()
    assert packed._record is None and len(packed._pb.graphs) == 2 and _ops.GRAPHS_ALIVE == alive0 + 1 + 2
    replay_plain()
    plain.release_graph()
    assert not plain.captured and _ops.GRAPHS_ALIVE == alive0 + len(packed._pb.graphs) == alive0 + 2
    assert all(torch.equal(a, b) for a, b in zip(replay_packed(), was_packed))
    plain.capture(*pad0)
    assert _ops.GRAPHS_ALIVE == alive0 + 3
    was_plain = replay_plain()
    packed.release_graph()
    assert not packed.captured and _ops.GRAPHS_ALIVE == alive0 + 1
    assert all(torch.equal(a, b) for a, b in zip(replay_plain(), was_plain))
    plain.release_graph()
    assert _ops.GRAPHS_ALIVE == alive0


# ----------------------------------------------------------------------------- the prefetcher's ragged mode
def test_prefetcher_ragged_mode_feeds_step_packed(H):
    """four batches, three different row counts, ring depth 2: the pinned staging and the device buffers of the ragged entries are
    allocated once per ring set (base addresses identical for every batch the set serves), only the batch's rows are handed out,
    the values are the loader's; step_packed fed from the prefetcher equals step_packed fed directly"""
    from hri_emo_amd.data import DevicePrefetcher
    host = [tuple(t.cpu() if isinstance(t, torch.Tensor) else t for t in rag) for _, rag in _batches()]
    host.append(host[1])
    loader = [(ra, torch.tensor(la), rt, lt, y) for ra, rt, la, lt, y in host]          # collate_seq_packed's order
    pf = DevicePrefetcher(loader, "cuda", depth=2, convert=lambda b: (b[0], b[1].tolist(), b[2], b[3].tolist(), b[4]),
                          ragged={0: NB * TA, 2: NB * TT})
    dp = _dp(_model(H))
    dp.capture_packed(*_batches()[0][1], pad_to=(TA, TT))
    direct = []
    for ra, rt, la, lt, y in host:
        loss = dp.step_packed(ra.cuda(), rt.cuda(), la, lt, y.cuda())
        torch.cuda.synchronize()
        direct.append((loss.clone(), dp.buckets.flat.clone()))
    bases, n = {}, 0
    for i, (ra, la, rt, lt, y) in enumerate(pf):
        ent = pf._ring[i % 2]
        sig = tuple(t.data_ptr() for t in (ent["host"][0], ent["dev"][0], ent["host"][2], ent["dev"][2]))
        assert bases.setdefault(i % 2, sig) == sig, f"batch {i}: a ragged buffer of ring set {i % 2} was re-allocated"
        assert ent["host"][0].shape[0] == NB * TA and ent["dev"][2].shape[0] == NB * TT and ent["host"][0].is_pinned()
        assert ra.data_ptr() == ent["dev"][0].data_ptr() and rt.data_ptr() == ent["dev"][2].data_ptr()
        assert isinstance(la, list) and la == [int(x) for x in loader[i][1]] and lt == [int(x) for x in loader[i][3]]
        assert ra.shape == loader[i][0].shape and torch.equal(ra.cpu(), loader[i][0]) and torch.equal(rt.cpu(), loader[i][2])
        assert torch.equal(y.cpu(), loader[i][4])
        loss = dp.step_packed(ra, rt, la, lt, y)
        torch.cuda.synchronize()
        assert torch.equal(loss, direct[i][0]) and torch.equal(dp.buckets.flat, direct[i][1]), i
        n += 1
    assert n == 4 and len({h[0].shape[0] for h in host}) == 3
    with pytest.raises(ValueError, match="capacity"):
        list(DevicePrefetcher(loader, "cuda", ragged={0: 100}))
    dp.release_graph()
