"""GPU suite of the packed front door at model level: `forward_packed` (ragged rows in, no padded batch anywhere) against `forward`
on the padded batch, against the oracle, with attention maps, through the MOSEI wrapper; the `set_ingest` switch against the
launches it replaces (outputs, gradients, and a spy on `_lib.call`); and captured bucket graphs with the switch on.
The ingest launch writes the bits as_pair + hriemo_pack_rows write, so everything behind it is compared with torch.equal."""
import ctypes

import pytest
import torch

from oracle import hri_emo_oracle as O          # the checker (tests only)

pytestmark = pytest.mark.gpu

SHAPES = {                      # d, N_e, B, T_a, T_t, audio lengths, text lengths
    "d128": (128, 4, 5, 70, 40, [70, 33, 32, 1, 17], [40, 1, 32, 31, 16]),
    "d768": (768, 6, 3, 48, 20, [48, 10, 33], [20, 17, 5]),
}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    keep = (_ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.PACKED_MAPS, _ops.gemm_mode(), _ops.precision())
    word = _ops.seed_word(torch.device("cuda", 0)).clone()           # a captured step bumps it on every replay; later tests
    yield hri_emo_amd                                                # replay dropout masks from it
    _ops.seed_word(torch.device("cuda", 0)).copy_(word)
    hri_emo_amd.set_varlen(False)
    hri_emo_amd.set_ingest(False)
    _ops.PACKED_TAIL, _ops.PACKED_TAIL_FP32, _ops.PACKED_TAIL_MX8, _ops.PACKED_MAPS = keep[:4]
    hri_emo_amd.set_gemm_mode(keep[4])
    hri_emo_amd.set_precision(keep[5])


def _tail(on):
    from hri_emo_amd import _ops
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = _ops.PACKED_TAIL_MX8 = bool(on)


def _batch(name, dtype=torch.float32, seed=11):
    """padded batch + masks + targets, and the same samples as packed rows + lengths"""
    d, ne, nb, Ta, Tt, la, lt = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    h_a, h_t = torch.randn(nb, Ta, d, generator=g).to(dtype).cuda(), torch.randn(nb, Tt, d, generator=g).to(dtype).cuda()
    m_a = (torch.arange(Ta)[None] >= torch.tensor(la)[:, None]).cuda()
    m_t = (torch.arange(Tt)[None] >= torch.tensor(lt)[:, None]).cuda()
    y = (torch.rand(nb, ne, generator=g) < 0.3).float().cuda()
    return (h_a, h_t, m_a, m_t, y), (h_a[~m_a].contiguous(), h_t[~m_t].contiguous(), la, torch.tensor(lt), (Ta, Tt))


def _model(H, name, p):
    d, ne = SHAPES[name][:2]
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=p).cuda()


def _step(m, fwd, y, inputs, seed=77):
    """one training step from the fixed seed -> (loss, parameter gradients, input gradients)"""
    from hri_emo_amd.train import fusion_step_loss
    m.zero_grad(set_to_none=True)
    for x in inputs:
        x.grad = None
    torch.manual_seed(seed)                        # the step's dropout seed comes from torch's generator
    logits, beta, _ = fwd()
    loss = fusion_step_loss(logits, beta, y)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}, [x.grad for x in inputs]


def _same_step(a, b):
    assert torch.equal(a[0], b[0]), (float(a[0]), float(b[0]))
    assert a[1].keys() == b[1].keys()
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), f"{n}: {int((a[1][n] != b[1][n]).sum())} elements differ"


# ----------------------------------------------------------------------------- forward_packed against forward
@pytest.mark.parametrize("tail", [False, True], ids=["tail off", "tail on"])
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_packed_equals_forward(H, name, kind, tail):
    """eval: logits, beta, z torch.equal; train at p = 0.1 from one seed: loss and every parameter gradient torch.equal, and the
    input gradients equal on the valid rows (the packed rows are the same bits, so everything behind them is)"""
    (h_a, h_t, m_a, m_t, y), (ra, rt, la, lt, pad) = _batch(name, DTYPES[kind])
    H.set_varlen(True)
    _tail(tail)
    m = _model(H, name, 0.1).eval()
    with torch.no_grad():
        ref = m(h_a, h_t, m_a, m_t)
        H.set_varlen(False)                        # forward_packed runs the packed encoder whatever set_varlen says
        got = m.forward_packed(ra, rt, la, lt)
        got_pad = m.forward_packed(ra, rt, la, lt, pad_to=pad)
        H.set_varlen(True)
    for a, b, c, what in zip(got, ref, got_pad, ("logits", "beta", "z")):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a, b) and torch.equal(c, b), (what, float((a.float() - b.float()).abs().max()))
    m.train()
    h_a.requires_grad_(True), h_t.requires_grad_(True), ra.requires_grad_(True), rt.requires_grad_(True)
    padded = _step(m, lambda: m(h_a, h_t, m_a, m_t), y, (h_a, h_t))
    packed = _step(m, lambda: m.forward_packed(ra, rt, la, lt, pad_to=pad), y, (ra, rt))
    _same_step(padded, packed)
    for gp, gr, mask in ((padded[2][0], packed[2][0], m_a), (padded[2][1], packed[2][1], m_t)):
        assert gr is not None and gr.dtype == DTYPES[kind] and float(gr.float().abs().max()) > 0
        assert torch.equal(gp[~mask], gr)
        assert float(gp[mask].float().abs().max()) == 0.0


@pytest.mark.parametrize("precision,bound", [("bf16", 5e-3), ("fp32", 1e-4)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_packed_against_the_oracle(H, name, precision, bound):
    """eval outputs against the oracle on the padded batch: the bf16 bound of DESIGN 1 (5e-3 of max(1, max|ref|)), 1e-4 in
    fp32 precision"""
    d, ne = SHAPES[name][:2]
    (h_a, h_t, m_a, m_t, _), (ra, rt, la, lt, _) = _batch(name)
    ref_m = O.closed_form_init_(O.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=0.1)).eval()
    m = H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=0.1)
    m.load_state_dict(ref_m.state_dict())
    m = m.cuda().eval()
    with torch.no_grad():
        ref = ref_m(h_a.cpu(), h_t.cpu(), m_a.cpu(), m_t.cpu())
        H.set_precision(precision)
        got = m.forward_packed(ra, rt, la, lt)
    for a, r, what in zip(got, ref, ("logits", "beta", "z")):
        err, lim = float((a.float().cpu() - r).abs().max()), bound * max(1.0, float(r.abs().max()))
        print(f"{name} {precision} {what}: {err:.3e} (bound {lim:.1e})")
        assert err <= lim, (what, err, lim)


def _same_tree(a, b, path="maps"):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _same_tree(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, f"{path}[{i}]")
    elif a is None:
        assert b is None, path
    else:
        assert a.shape == b.shape and a.dtype == b.dtype, (path, a.shape, b.shape)
        assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0)), path
    return True


@pytest.mark.parametrize("tail", [False, True], ids=["tail off", "tail on"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_packed_attention_maps(H, name, tail):
    """return_attention with the packed export on: every map is forward's, bit for bit, in the pad_to shapes"""
    (h_a, h_t, m_a, m_t, _), (ra, rt, la, lt, pad) = _batch(name)
    nb = SHAPES[name][2]
    H.set_varlen(True)
    H.set_varlen_maps(True)
    _tail(tail)
    m = _model(H, name, 0.1).eval()
    with torch.no_grad():
        ref = m(h_a, h_t, m_a, m_t, return_attention=True)
        got = m.forward_packed(ra, rt, la, lt, pad_to=pad, return_attention=True)
    for a, b in zip(got[:3], ref[:3]):
        assert torch.equal(a, b)
    assert _same_tree(got[3], ref[3])
    enc = got[3]["encoder"][0]
    assert enc["audio_self"].shape == (nb, pad[0], pad[0]) and enc["audio_queries_text"].shape == (nb, pad[0], pad[1])
    assert enc["text_queries_audio"].shape == (nb, pad[1], pad[0])


def test_mosei_forward_packed(H):
    """MOSEI wrapper (d_audio 74, d_text 300, d = 128): forward_packed against forward under varlen, outputs and every parameter
    gradient within 1e-5 relative L2 -- the packed-against-padded bound of DESIGN 1 (the projections run with another M)"""
    from hri_emo_amd.train import fusion_step_loss
    _, ne, nb, Ta, Tt, la, lt = SHAPES["d128"]
    g = torch.Generator().manual_seed(5)
    x_a, x_t = torch.randn(nb, Ta, 74, generator=g).cuda(), torch.randn(nb, Tt, 300, generator=g).cuda()
    m_a = (torch.arange(Ta)[None] >= torch.tensor(la)[:, None]).cuda()
    m_t = (torch.arange(Tt)[None] >= torch.tensor(lt)[:, None]).cuda()
    y = (torch.rand(nb, ne, generator=g) < 0.3).float().cuda()
    torch.manual_seed(3)
    m = H.MoseiFusionWithEmotionDecoder(d_audio=74, d_text=300, d_model=128, num_emotions=ne, n_heads=8, dropout=0.0).cuda().train()
    H.set_varlen(True)
    res = []
    for fwd in (lambda: m(x_a, x_t, m_a, m_t), lambda: m.forward_packed(x_a[~m_a], x_t[~m_t], la, lt)):
        m.zero_grad(set_to_none=True)
        out = fwd()
        fusion_step_loss(out[0], out[1], y).backward()
        res.append(([o.detach().float() for o in out], {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-20))       # noqa: E731
    for a, b, what in zip(res[1][0], res[0][0], ("logits", "beta", "z")):
        print(f"mosei {what}: relative L2 {rel(a, b):.2e}")
        assert rel(a, b) <= 1e-5, (what, rel(a, b))
    worst = max(rel(res[1][1][n], res[0][1][n]) for n in res[0][1])
    print(f"mosei worst parameter gradient: relative L2 {worst:.2e}")
    for n in res[0][1]:
        assert rel(res[1][1][n], res[0][1][n]) <= 1e-5, (n, rel(res[1][1][n], res[0][1][n]))


# ----------------------------------------------------------------------------- the switch against the launches it replaces
class Spy:
    """records (name, args) of every _lib.call, split at mark()"""

    def __init__(self, monkeypatch):
        from hri_emo_amd import _lib
        self.calls, real = [], _lib.call

        def spy(name, *args):
            self.calls.append((name, args))
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", spy)

    def take(self):
        out, self.calls = self.calls, []
        return out


def _mx_batch():
    """d = 128, B = 8: the smallest batch whose packed audio rows reach _ops.MX_MIN_ROWS (8 x 128 = 1024 rows of 136 padded)"""
    from hri_emo_amd import _ops
    la, lt, Ta, Tt = [136, 128, 128, 128, 128, 128, 128, 120], [40, 1, 32, 31, 16, 40, 8, 24], 136, 40
    assert sum(la) == _ops.MX_MIN_ROWS and sum(la) - 1 < _ops.MX_MIN_ROWS
    g = torch.Generator().manual_seed(12)
    h_a, h_t = torch.randn(8, Ta, 128, generator=g).cuda(), torch.randn(8, Tt, 128, generator=g).cuda()
    m_a = (torch.arange(Ta)[None] >= torch.tensor(la)[:, None]).cuda()
    m_t = (torch.arange(Tt)[None] >= torch.tensor(lt)[:, None]).cuda()
    return h_a, h_t, m_a, m_t, (torch.rand(8, 4, generator=g) < 0.3).float().cuda()


@pytest.mark.parametrize("setting,kind", [("padded", "fp32"), ("varlen", "fp32"), ("fp32 precision", "fp32"), ("mx_fp8", "fp32"),
                                          ("varlen", "fp16"), ("varlen", "bf16"), ("padded", "fp16"), ("padded", "bf16"),
                                          ("mx_fp8 padded", "bf16")])
def test_ingest_switch_equals_the_launches_it_replaces(H, monkeypatch, setting, kind):
    """set_ingest(True) against off through plain forward: loss, parameter and input gradients torch.equal; the spy shows two
    hriemo_ingest_rows and no hriemo_pack_rows in the forward with the switch on (in fp8 mode no hriemo_quant_mx8 of a module
    input either), none at all with it off.  ("mx_fp8 padded": a bf16 batch that keeps its layout, 8 x 136 = 1088 audio rows.)"""
    h_a, h_t, m_a, m_t, y = _mx_batch() if setting.startswith("mx_fp8") else _batch("d128", DTYPES[kind])[0]
    h_a, h_t = h_a.to(DTYPES[kind]), h_t.to(DTYPES[kind])
    H.set_varlen(not setting.endswith("padded"))
    _tail(True)
    if setting == "fp32 precision":
        H.set_precision("fp32")
    if setting.startswith("mx_fp8"):
        H.set_gemm_mode("mx_fp8")
    m = _model(H, "d128", 0.1).train()
    h_a, h_t = h_a.clone().requires_grad_(True), h_t.clone().requires_grad_(True)
    fwd = lambda: m(h_a, h_t, m_a, m_t)                                         # noqa: E731
    _step(m, fwd, y, (h_a, h_t))                                                # warm-up: shadows, plans
    spy = Spy(monkeypatch)
    seen, steps = {}, {}
    for on in (False, True):
        H.set_ingest(on)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(77)
        with torch.no_grad():
            m.eval()
            out = [o.clone() for o in m(h_a, h_t, m_a, m_t)]
            m.train()
        seen[on] = spy.take()
        steps[on] = _step(m, fwd, y, (h_a, h_t)) + (out,)
        spy.take()
    H.set_ingest(False)
    _same_step(steps[False], steps[True])
    for a, b in zip(steps[False][2] + steps[False][3], steps[True][2] + steps[True][3]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    names = {on: [n for n, _ in seen[on]] for on in seen}
    assert names[False].count("hriemo_ingest_rows") == 0
    if kind == "bf16" and setting == "padded":
        assert names[True].count("hriemo_ingest_rows") == 0          # a bf16 tensor that keeps its layout is its own pair
        return
    if setting == "mx_fp8 padded":                                   # ... and in fp8 mode gets its quantised copy from one launch
        launches = [a for n, a in seen[True] if n == "hriemo_ingest_rows"]
        assert len(launches) == 1 and launches[0][8] == 8 * 136 and launches[0][9] is None and launches[0][11] is not None
        assert names[True].count("hriemo_quant_mx8") == names[False].count("hriemo_quant_mx8") - 1
        return
    assert names[True].count("hriemo_ingest_rows") == 2 and names[True].count("hriemo_pack_rows") == 0
    assert names[False].count("hriemo_pack_rows") == (0 if setting == "padded" else 2)
    if setting == "mx_fp8":
        # the first layer's in-projection precedes the first attention launch: what is quantised before that is a module input
        head = {on: seen[on][:next(i for i, (n, _) in enumerate(seen[on]) if n.startswith("hriemo_attn_fwd"))] for on in seen}
        q_off = [a for n, a in head[False] if n == "hriemo_quant_mx8"]
        packed_off = [a[7] for n, a in head[False] if n == "hriemo_pack_rows"]
        assert len(q_off) == 1 and q_off[0][0] in packed_off and q_off[0][3] == 1024, "the spy must see the parent's quantiser on the packed audio input"
        assert [n for n, _ in head[True]].count("hriemo_quant_mx8") == 0, "a module input was quantised by a launch of its own"
        assert names[True].count("hriemo_quant_mx8") == names[False].count("hriemo_quant_mx8") - 1
        mx = [a for n, a in seen[True] if n == "hriemo_ingest_rows" and a[11] is not None]
        assert len(mx) == 1 and mx[0][8] == 1024                     # the audio rows carry the copy; the text rows are too few


def test_inputs_without_grad_cost_no_backward_launch(H, monkeypatch):
    """inputs that need no gradient: no hriemo_unpack_rows in the backward for them, and as many NN GEMM launches as with the
    switch off (the first layer's input-gradient skip keeps firing); inputs that do need one get exactly the two scatters"""
    from hri_emo_amd import _lib, _ops
    L = _lib.lib()
    nn = [L.hriemo_prof_name(c).decode() for c in range(L.hriemo_prof_nclass())].index("gemm_bf16_nn")
    h_a, h_t, m_a, m_t, y = _batch("d128")[0]
    H.set_varlen(True)
    _tail(True)
    m = _model(H, "d128", 0.1).train()
    fwd = lambda: m(h_a, h_t, m_a, m_t)                                         # noqa: E731
    _step(m, fwd, y, ())
    _ops.side_stream(torch.device("cuda", torch.cuda.current_device()))         # settles TWO_STREAMS from the environment
    two, _ops.TWO_STREAMS = _ops.TWO_STREAMS, False
    spy = Spy(monkeypatch)
    counts, unpacks = {}, {}
    try:
        for on in (False, True):
            H.set_ingest(on)
            L.hriemo_prof_enable(1)
            _step(m, fwd, y, ())
            ms, n, work = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
            L.hriemo_prof_collect(nn, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(work))
            counts[on] = n.value
            unpacks[on] = [name for name, _ in spy.take()].count("hriemo_unpack_rows")
    finally:
        L.hriemo_prof_enable(0)
        _ops.TWO_STREAMS = two
    print(f"\n  gemm_bf16_nn launches per step: switch off {counts[False]}, on {counts[True]}")
    assert counts[True] == counts[False] and unpacks == {False: 0, True: 0}
    h_a, h_t = h_a.clone().requires_grad_(True), h_t.clone().requires_grad_(True)
    H.set_ingest(True)
    _step(m, lambda: m(h_a, h_t, m_a, m_t), y, (h_a, h_t))
    assert [name for name, _ in spy.take()].count("hriemo_unpack_rows") == 2


# ----------------------------------------------------------------------------- captured
def test_captured_bucket_graphs_with_the_switch_on(H, monkeypatch):
    """DataParallelStep in varlen mode with INGEST_ROWS on: three batches over two row-count buckets (two ragged batches with the
    same lengths share one, an all-full batch opens the other; every bucket has its filler sequence of surplus rows); replays
    within 1e-5 of the eager padded step with the switch off, a second replay bit-identical, the captured steps ingest and do
    not pack"""
    from test_gpu_varlen import _ragged_batch
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    from hri_emo_amd import _ops
    torch.manual_seed(3)
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.0).cuda().train()
    nb, Ta, Tt, d = 4, 96, 40, 128
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    dp.set_global_batch(nb)
    first = _ragged_batch(nb, Ta, Tt, d, 4, 4, 20, 5)[0]
    other = _ragged_batch(nb, Ta, Tt, d, 4, 14, 20, 5)[0]
    batches = [first, (other[0], other[1], first[2], first[3], other[4]), _ragged_batch(nb, Ta, Tt, d, 4, 5, Ta, Tt)[0]]
    assert not bool(first[2].logical_not().all()) and bool((~batches[2][2]).all())
    H.set_varlen(False)
    _tail(False)
    ref = [(float(dp.step(*batch)), dp.buckets.flat.clone()) for batch in batches]      # the padded eager step is the yardstick
    H.set_varlen(True)
    _tail(True)
    H.set_ingest(True)
    spy = Spy(monkeypatch)
    dp.capture(*batches[0])
    keys, once = set(), None
    for i, batch in enumerate(batches):
        loss = float(dp.step(*batch))
        torch.cuda.synchronize()
        keys.add(tuple(int(x) for x in (dp._pb.cu_a[-1], dp._pb.cu_t[-1])))
        assert int(dp._pb.cu_a[-1]) > int(dp._pb.cu_a[nb]), "the bucket has surplus rows behind the last sample"
        rel = float((dp.buckets.flat - ref[i][1]).norm() / ref[i][1].norm())
        print(f"batch {i}: loss {loss:.6f} vs {ref[i][0]:.6f}, flat gradients relative L2 {rel:.2e}")
        assert abs(loss - ref[i][0]) <= 1e-5 * max(1.0, abs(ref[i][0])), (i, loss, ref[i][0])
        assert rel <= 1e-5, (i, rel)
        if i == 0:
            once = (loss, dp.buckets.flat.clone())
    loss = float(dp.step(*batches[0]))
    torch.cuda.synchronize()
    assert loss == once[0] and torch.equal(dp.buckets.flat, once[1]), "a second replay of the first batch"
    assert len(dp._pb.graphs) == len(keys) == 2
    names = [n for n, _ in spy.take()]
    assert names.count("hriemo_ingest_rows") >= 2 * len(keys) and "hriemo_pack_rows" not in names
    dp.release_graph()
    assert _ops.CTX.seq_override is None
