"""GPU suite: input gradients only where autograd asks for them.  The first encoder layer's x is the model's input; when it needs
no gradient, SelfAttnLN.backward neither has add_ln_bwd store the residual gradient dS (NULL dX) nor runs the dX GEMM that is
its only reader.  Nothing else may change: loss and every parameter gradient are compared BIT FOR BIT between a step whose
inputs require grad and one whose inputs do not, on padded and on packed (varlen) rows, the NN GEMM launch count must drop by
exactly the two skipped GEMMs (audio and text self-attention of layer 0), and a stand-alone CrossModalBlock with inputs that
require grad must return the input gradients of the unconditional path (_ops.FORCE_INPUT_GRAD)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

D, HEADS, NE, B, TA, TT, P = 256, 8, 4, 2, 40, 24, 0.1
SEED = 77                   # the step's dropout seed word comes from torch's generator


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    from hri_emo_amd import _ops
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)
    _ops.FORCE_INPUT_GRAD = False


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(11)
    h_a, h_t = torch.randn(B, TA, D, generator=g).cuda(), torch.randn(B, TT, D, generator=g).cuda()
    y = (torch.rand(B, NE, generator=g) < 0.3).float().cuda()
    return h_a, h_t, y


def masks(ragged):
    """prefix padding masks (True = PAD): full rows, or ragged lengths with sample 0 at full length"""
    la, lt = ([TA, 23], [TT, 9]) if ragged else ([TA, TA], [TT, TT])
    return ((torch.arange(TA)[None] >= torch.tensor(la)[:, None]).cuda(), (torch.arange(TT)[None] >= torch.tensor(lt)[:, None]).cuda())


def model(H):
    torch.manual_seed(3)
    return H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=HEADS, num_layers_fusion=1, num_layers_decoder=1,
                                      dropout=P).cuda().train()


def step(m, batch, m_a, m_t, inputs_need_grad):
    """one training step from the fixed seed -> (loss, parameter gradients, input gradients)"""
    from hri_emo_amd.train import fusion_step_loss
    h_a, h_t, y = batch
    h_a, h_t = h_a.clone().requires_grad_(inputs_need_grad), h_t.clone().requires_grad_(inputs_need_grad)
    m.zero_grad(set_to_none=True)
    torch.manual_seed(SEED)
    logits, beta, _ = m(h_a, h_t, m_a, m_t)
    loss = fusion_step_loss(logits, beta, y)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}, (h_a.grad, h_t.grad)


def assert_same_step(a, b):
    (la, ga, _), (lb, gb, _) = a, b
    assert torch.equal(la, lb), (float(la), float(lb))
    assert ga.keys() == gb.keys()
    for n in ga:
        assert torch.equal(ga[n], gb[n]), f"{n}: {int((ga[n] != gb[n]).sum())} elements differ"


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_step_without_input_grads_is_bit_equal(H, batch, packed):
    from hri_emo_amd import _ops
    H.set_varlen(packed)
    m_a, m_t = masks(ragged=packed)
    if packed:
        assert _ops.seq_plan(m_a, B, TA) is not None, "prefix masks: the packed path must run"
    m = model(H)
    with_grad = step(m, batch, m_a, m_t, True)
    without = step(m, batch, m_a, m_t, False)
    assert_same_step(with_grad, without)
    for g in with_grad[2]:
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
    assert without[2] == (None, None)


def test_two_nn_gemms_fewer(H, batch):
    """kernels in a row on one stream, counted by the library's own launch counters"""
    from hri_emo_amd import _lib, _ops
    L = _lib.lib()
    names = [L.hriemo_prof_name(c).decode() for c in range(L.hriemo_prof_nclass())]
    nn = names.index("gemm_bf16_nn")
    m_a, m_t = masks(ragged=False)
    m = model(H)
    _ops.side_stream(torch.device("cuda", torch.cuda.current_device()))      # settles TWO_STREAMS from the environment
    two = _ops.TWO_STREAMS
    _ops.TWO_STREAMS = False
    counts = []
    try:
        for need in (True, False):
            L.hriemo_prof_enable(1)
            step(m, batch, m_a, m_t, need)
            ms, n, work = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
            L.hriemo_prof_collect(nn, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(work))
            counts.append(n.value)
    finally:
        L.hriemo_prof_enable(0)
        _ops.TWO_STREAMS = two
    print(f"\n  gemm_bf16_nn launches per step: inputs need grad {counts[0]}, inputs need none {counts[1]}")
    assert counts[1] == counts[0] - 2, counts


def test_block_input_gradients_unchanged(H):
    """CrossModalBlock on its own: inputs that require grad get the gradients of the unconditional path, and with inputs that need
    none the parameter gradients are those of the unconditional path as well"""
    from hri_emo_amd import _ops
    torch.manual_seed(5)
    blk = H.CrossModalBlock(D, HEADS, P).cuda().train()
    g = torch.Generator().manual_seed(12)
    a0, t0 = torch.randn(B, TA, D, generator=g).cuda(), torch.randn(B, TT, D, generator=g).cuda()
    wa, wt = torch.randn(B, TA, D, generator=g).cuda(), torch.randn(B, TT, D, generator=g).cuda()
    m_a, m_t = masks(ragged=True)

    def run(need, force):
        _ops.FORCE_INPUT_GRAD = force
        a, t = a0.clone().requires_grad_(need), t0.clone().requires_grad_(need)
        blk.zero_grad(set_to_none=True)
        torch.manual_seed(SEED)
        ya, yt = blk(a, t, m_a, m_t)
        ((ya.float() * wa).sum() + (yt.float() * wt).sum()).backward()
        torch.cuda.synchronize()
        _ops.FORCE_INPUT_GRAD = False
        return (a.grad, t.grad), {n: p.grad.detach().clone() for n, p in blk.named_parameters()}

    (ga, gt), pg = run(True, False)
    (ga_f, gt_f), pg_f = run(True, True)
    assert ga is not None and gt is not None and float(ga.abs().max()) > 0.0 and float(gt.abs().max()) > 0.0
    assert torch.equal(ga, ga_f) and torch.equal(gt, gt_f)
    (na, nt), pg_n = run(False, False)
    (fa, ft), pg_nf = run(False, True)          # forced: dS and the dX GEMM run although nobody reads the result
    assert na is None and nt is None and fa is None and ft is None
    for n in pg:
        assert torch.equal(pg[n], pg_f[n]) and torch.equal(pg[n], pg_n[n]) and torch.equal(pg[n], pg_nf[n]), n
