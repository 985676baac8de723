"""GPU suite of the kernels behind the step-control block of a captured ragged step, through the C ABI on guarded buffers:

  hriemo_fusion_loss_n / hriemo_fusion_loss_ce_n   the trainer losses with the number of samples that count in device memory
  hriemo_grad_begin                                the conditional start of the flat gradient buffer (ctl.first)
  hriemo_optim_finalize_ctl                        the optimizer hold (ctl.last)

References are float64, computed here from the first n samples alone.  Limits are those of the existing loss tests
(test_gpu_gate_kernels.py): loss and dlogits 2e-6 * max(1, |ref|), dbeta 1e-5 * max(1e-3, max |ref|).  Everything a ghost sample
could be read from is NaN (labels: an index far outside [0, C), which poisons the loss when read); every output starts as 0xFF
bytes (NaN), so a ghost gradient that is not stored, or stored as 0 * NaN, shows."""
import pytest
import torch
import torch.nn.functional as F

from rowops_reference import GuardedVec

pytestmark = pytest.mark.gpu
BAD_LABEL = 10 ** 12


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib


def ST():
    return torch.cuda.current_stream().cuda_stream


def G(x):
    return GuardedVec.of(x.contiguous(), device="cuda")


def _reg64(beta, mode, coef):
    if mode == 1:
        return -coef * (beta * (1 - beta)).mean()
    if mode == 2:
        b = torch.clamp(beta, 1e-8, 1 - 1e-8)
        return coef * (-(b * torch.log(b) + (1 - b) * torch.log(1 - b))).mean()
    return beta.sum() * 0.0


def _bce_case(B, Ne, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ne, generator=g) * 3
    y = (torch.rand(B, Ne, generator=g) < 0.3).float()
    beta = 0.05 + 0.9 * torch.rand(B, generator=g)
    pw = 0.5 + 3 * torch.rand(Ne, generator=g)
    return x, y, beta, pw


def _run_bce(lib, x, y, beta, pw, mode, coef, scale, n=None):
    """-> loss [1], dlogits [B, Ne], dbeta [B] on the CPU; n None: the existing entry"""
    B, Ne = x.shape
    bx, by, bb = G(x), G(y), G(beta)
    bp = G(pw) if pw is not None else None
    loss, dx, db = GuardedVec(1, torch.float32, device="cuda"), GuardedVec(B * Ne, torch.float32, device="cuda"), GuardedVec(B, torch.float32, device="cuda")
    bufs = [bx, by, bb, loss, dx, db] + ([bp] if bp is not None else [])
    common = (bx.ptr, by.ptr, bp.ptr if bp is not None else None, bb.ptr if mode else None, B, Ne, mode, coef, scale, loss.ptr, dx.ptr,
              db.ptr if mode else None)
    if n is None:
        lib.call("hriemo_fusion_loss", *common, ST())
    else:
        nv = GuardedVec.of(torch.tensor([n, -7, -7, -7], dtype=torch.int32), device="cuda")
        bufs.append(nv)
        lib.call("hriemo_fusion_loss_n", *common, nv.ptr, ST())
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        b.assert_intact(f"buffer {i}")
    return loss.view.cpu(), dx.view.cpu().view(B, Ne), (db.view.cpu() if mode else None)


def _check_bce(lib, B, Ne, n, mode, with_pw, coef=0.05, scale=0.5):
    x, y, beta, pw = _bce_case(B, Ne, 100 * B + n)
    pw = pw if with_pw else None
    xg, yg, bg = x.clone(), y.clone(), beta.clone()
    xg[n:], yg[n:], bg[n:] = float("nan"), float("nan"), float("nan")
    loss, dx, db = _run_bce(lib, xg, yg, bg, pw, mode, coef, scale, n=n)
    x64, b64 = x[:n].double().requires_grad_(True), beta[:n].double().requires_grad_(True)
    ref = (F.binary_cross_entropy_with_logits(x64, y[:n].double(), pos_weight=None if pw is None else pw.double()) + _reg64(b64, mode, coef)) * scale
    ref.backward()
    print(f"BCE B {B} n {n} mode {mode} pw {with_pw}: loss {float(loss):.8f} ref {float(ref):.8f}, max |dx err| "
          f"{float((dx[:n].double() - x64.grad).abs().max()):.2e}")
    assert not bool(torch.isnan(dx[n:]).any()) and bool((dx[n:] == 0).all()), "ghost rows of dlogits are exactly zero"
    assert abs(float(loss) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
    assert float((dx[:n].double() - x64.grad).abs().max()) <= 2e-6 * max(1.0, float(x64.grad.abs().max()))
    if mode:
        assert not bool(torch.isnan(db[n:]).any()) and bool((db[n:] == 0).all()), "ghost entries of dbeta are exactly zero"
        assert float((db[:n].double() - b64.grad).abs().max()) <= 1e-5 * max(1e-3, float(b64.grad.abs().max()))


@pytest.mark.parametrize("with_pw", [False, True], ids=["no pw", "pw"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_masked_bce_loss_against_float64_over_the_first_n(lib, n, mode, with_pw):
    _check_bce(lib, 5, 6, n, mode, with_pw)


def test_masked_bce_loss_past_one_trip_of_the_block(lib):
    """B = 300, n_valid = 257: 1542 valid elements (seven trips of the 256-thread loop), ghosts in the second trip of the sample loop"""
    _check_bce(lib, 300, 6, 257, 2, True)


def _ce_case(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * 4
    lab = torch.randint(0, C, (B,), generator=g)
    beta = 0.05 + 0.9 * torch.rand(B, generator=g)
    return x, lab, beta


def _run_ce(lib, x, lab, beta, mode, coef, scale, n=None):
    B, C = x.shape
    bx, bl, bb = G(x), G(lab), G(beta)
    loss, dx, db = GuardedVec(1, torch.float32, device="cuda"), GuardedVec(B * C, torch.float32, device="cuda"), GuardedVec(B, torch.float32, device="cuda")
    bufs = [bx, bl, bb, loss, dx, db]
    common = (bx.ptr, bl.ptr, bb.ptr if mode else None, B, C, mode, coef, scale, loss.ptr, dx.ptr, db.ptr if mode else None)
    if n is None:
        lib.call("hriemo_fusion_loss_ce", *common, ST())
    else:
        nv = GuardedVec.of(torch.tensor([n, -7, -7, -7], dtype=torch.int32), device="cuda")
        bufs.append(nv)
        lib.call("hriemo_fusion_loss_ce_n", *common, nv.ptr, ST())
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        b.assert_intact(f"buffer {i}")
    return loss.view.cpu(), dx.view.cpu().view(B, C), (db.view.cpu() if mode else None)


def _check_ce(lib, B, C, n, mode, ignore, coef=0.05, scale=0.5):
    """ignore: one -100 label among the valid rows (row min(1, n - 1); with n = 1 that leaves no labelled sample: NaN loss, as torch)"""
    x, lab, beta = _ce_case(B, C, 100 * B + n)
    if ignore:
        lab[min(1, n - 1)] = -100
    xg, lg, bg = x.clone(), lab.clone(), beta.clone()
    xg[n:], lg[n:], bg[n:] = float("nan"), BAD_LABEL, float("nan")
    loss, dx, db = _run_ce(lib, xg, lg, bg, mode, coef, scale, n=n)
    x64, b64 = x[:n].double().requires_grad_(True), beta[:n].double().requires_grad_(True)
    ref = (F.cross_entropy(x64, lab[:n]) + _reg64(b64, mode, coef)) * scale
    ref.backward()
    print(f"CE B {B} n {n} mode {mode} ignore {ignore}: loss {float(loss):.8f} ref {float(ref):.8f}")
    assert not bool(torch.isnan(dx[n:]).any()) and bool((dx[n:] == 0).all()), "ghost rows of dlogits are exactly zero"
    if bool((lab[:n] == -100).all()):
        assert torch.isnan(ref).item() and torch.isnan(loss).item(), "no labelled sample among the valid ones: NaN, as torch"
        assert bool((dx[:n] == 0).all())
    else:
        assert abs(float(loss) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
        assert float((dx[:n].double() - x64.grad).abs().max()) <= 2e-6 * max(1.0, float(x64.grad.abs().max()))
        assert bool((dx[:n][lab[:n] == -100] == 0).all())
    if mode:
        assert not bool(torch.isnan(db[n:]).any()) and bool((db[n:] == 0).all()), "ghost entries of dbeta are exactly zero"
        assert float((db[:n].double() - b64.grad).abs().max()) <= 1e-5 * max(1e-3, float(b64.grad.abs().max()))


@pytest.mark.parametrize("ignore", [False, True], ids=["all labelled", "one -100"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_masked_ce_loss_against_float64_over_the_first_n(lib, n, mode, ignore):
    _check_ce(lib, 5, 4, n, mode, ignore)


def test_masked_ce_loss_past_one_trip_of_the_block(lib):
    _check_ce(lib, 300, 4, 257, 1, True)


@pytest.mark.parametrize("B", [5, 300])
def test_all_valid_is_bit_identical_to_the_unmasked_entries(lib, B):
    """n_valid == B: loss, dlogits and dbeta torch.equal to hriemo_fusion_loss / hriemo_fusion_loss_ce; n_valid is clamped to [1, B]
    on the device (B + 3 behaves as B, 0 and -4 as 1)"""
    for mode in (0, 1, 2):
        for with_pw in (False, True):
            x, y, beta, pw = _bce_case(B, 6, 7 * B + mode)
            old = _run_bce(lib, x, y, beta, pw if with_pw else None, mode, 0.05, 0.5)
            for n in (B, B + 3):
                new = _run_bce(lib, x, y, beta, pw if with_pw else None, mode, 0.05, 0.5, n=n)
                for a, b in zip(old, new):
                    assert (a is None and b is None) or torch.equal(a, b), ("bce", mode, with_pw, n)
        x, lab, beta = _ce_case(B, 4, 9 * B + mode)
        lab[1] = -100
        old = _run_ce(lib, x, lab, beta, mode, 0.05, 0.5)
        for n in (B, B + 3):
            new = _run_ce(lib, x, lab, beta, mode, 0.05, 0.5, n=n)
            for a, b in zip(old, new):
                assert (a is None and b is None) or torch.equal(a, b), ("ce", mode, n)
    x, y, beta, pw = _bce_case(B, 6, 3)
    one = _run_bce(lib, x, y, beta, pw, 1, 0.05, 0.5, n=1)
    for n in (0, -4):
        for a, b in zip(one, _run_bce(lib, x, y, beta, pw, 1, 0.05, 0.5, n=n)):
            assert torch.equal(a, b), n


# ----------------------------------------------------------------------------------------------------- hriemo_grad_begin
@pytest.mark.parametrize("n", [4, 1020, 4 * 256 * 4096 + 4])
def test_grad_begin_zeroes_or_keeps_every_bit(lib, n):
    """one vector; just under one block; one vector past a full sweep of the capped grid (the grid-stride loop takes a second trip).
    The pattern holds a NaN with a payload, -0, a denormal and an infinity.  first = 1: every word is +0 (compared as int32);
    first = 0: every bit stays; the guards stay in both cases."""
    g = torch.Generator().manual_seed(n)
    pat = torch.randn(n, generator=g)
    bits = pat.view(torch.int32)
    specials = torch.tensor([0x7FC12345, -0x80000000, 0x00000123, 0x7F800000], dtype=torch.int64).to(torch.int32)
    for j in range(4):                                         # `bits` is a view of `pat`: the specials land in the pattern
        bits[j::max(4, n // 61)] = specials[j]
    bits[n - 4:] = specials                                    # the last vector, too
    for first in (0, 1):
        buf = GuardedVec.of(pat, device="cuda")
        ctl = GuardedVec.of(torch.tensor([5, first, 1, 0], dtype=torch.int32), device="cuda")
        lib.call("hriemo_grad_begin", buf.ptr, n, ctl.ptr, ST())
        torch.cuda.synchronize()
        got = buf.view.view(torch.int32).cpu()
        if first:
            assert int((got != 0).sum()) == 0, "first = 1: every word is +0"
        else:
            assert torch.equal(got, bits), "first = 0: bit-identical"
        buf.assert_intact("flat")
        ctl.assert_intact("ctl")
    bad = GuardedVec.of(pat[:8], device="cuda")
    with pytest.raises(RuntimeError, match="grad_begin"):
        lib.call("hriemo_grad_begin", bad.ptr, 6, ctl.ptr, ST())
    with pytest.raises(RuntimeError, match="grad_begin"):
        lib.call("hriemo_grad_begin", bad.ptr + 4, 4, ctl.ptr, ST())


# ----------------------------------------------------------------------------------------------------- the optimizer hold
def test_optimizer_hold_then_release_equals_one_plain_step(lib):
    """DeviceAdamW._enqueue(ctl=): a held finalize + update (last = 0) leaves flat_p, m, v and all 8 words of state bit-identical
    except state.skip; the following last = 1 finalize + update gives what ONE plain DeviceAdamW.step() gives from the same start"""
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW

    def make():
        torch.manual_seed(5)
        net = torch.nn.Sequential(torch.nn.Linear(48, 40), torch.nn.Linear(40, 7)).cuda()
        buckets = GradBuckets(net.parameters(), overlap=False)
        opt = DeviceAdamW(buckets, lr=1e-3, weight_decay=1e-2, max_norm=1.0)
        return net, buckets, opt

    g = torch.Generator().manual_seed(1)
    (_, b1, o1), (_, b2, o2) = make(), make()
    grads = [torch.randn(b1.flat.numel(), generator=g).cuda() * s for s in (1.0, 3.0)]
    for b, o in ((b1, o1), (b2, o2)):                      # one plain step first: step = 1, moments and every state word non-trivial
        b.flat.copy_(grads[0])
        o.step()
        b.flat.copy_(grads[1])
    ctl = torch.tensor([5, 0, 0, 0], dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (o1.flat_p, o1.m, o1.v, o1._state)]
    o1._upload_hyper()
    o1._enqueue(ctl=ctl)                                       # held
    torch.cuda.synchronize()
    assert torch.equal(o1.flat_p, before[0]) and torch.equal(o1.m, before[1]) and torch.equal(o1.v, before[2])
    st = o1._state.clone()
    assert float(st[1]) == 1.0 and float(before[3][1]) == 0.0, "the hold sets state.skip"
    st[1] = before[3][1]
    assert torch.equal(st.view(torch.int32), before[3].view(torch.int32)), "step, skipped, grad_norm and the rest of state stay"
    ctl[2] = 1
    o1._enqueue(ctl=ctl)                                       # released
    o2.step()
    torch.cuda.synchronize()
    assert float(o1.device_step) == 2.0 and float(o1.skipped) == 0.0
    for name, a, b in (("p", o1.flat_p, o2.flat_p), ("m", o1.m, o2.m), ("v", o1.v, o2.v), ("state", o1._state, o2._state)):
        assert torch.equal(a, b), name
    assert not torch.equal(o1.flat_p, before[0])


# ----------------------------------------------------------------------------------------------------- through hri_emo_amd.train
def test_the_three_losses_with_n_valid_against_their_cpu_formulas(lib):
    """train.fusion_step_loss / fusion_step_loss_single_label / mosei_step_loss with n_valid= on the GPU (the autograd Functions on the
    _n entries, an outer factor flowing through backward) against the CPU formulas on the first n samples; a host integer or a
    tensor of another dtype is refused"""
    from hri_emo_amd import train
    g = torch.Generator().manual_seed(8)
    B, Ne, n = 5, 6, 3
    x, beta = torch.randn(B, Ne, generator=g) * 3, 0.05 + 0.9 * torch.rand(B, 1, generator=g)
    y, lab = (torch.rand(B, Ne, generator=g) < 0.3).float(), torch.randint(0, Ne, (B,), generator=g)
    pw = 0.5 + 3 * torch.rand(Ne, generator=g)
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    cases = ((train.fusion_step_loss, y, {}), (train.fusion_step_loss_single_label, lab, {}),
             (train.mosei_step_loss, y, dict(pos_weight=pw, beta_entropy=0.05, grad_accum=2)))
    for fn, tgt, kw in cases:
        xc, bc = x[:n].clone().requires_grad_(True), beta[:n].clone().requires_grad_(True)
        ref = fn(xc, bc, tgt[:n], **kw)
        (ref * 3.0).backward()
        xg, bg = x.clone(), beta.clone()
        xg[n:], bg[n:] = float("nan"), float("nan")
        xd, bd = xg.cuda().requires_grad_(True), bg.cuda().requires_grad_(True)
        kwd = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        loss = fn(xd, bd, tgt.cuda(), n_valid=nv, **kwd)
        (loss * 3.0).backward()
        assert abs(float(loss) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref))), fn.__name__
        assert float((xd.grad[:n].cpu() - xc.grad).abs().max()) <= 3 * 2e-6 * max(1.0, float(xc.grad.abs().max()) / 3), fn.__name__
        assert float((bd.grad[:n].cpu() - bc.grad).abs().max()) <= 1e-5 * max(1e-3, float(bc.grad.abs().max())), fn.__name__
        assert bool((xd.grad[n:] == 0).all()) and bool((bd.grad[n:] == 0).all()), fn.__name__
    for bad in (3, torch.tensor([3], device="cuda"), torch.tensor([3], dtype=torch.int32)):
        with pytest.raises(TypeError, match="n_valid"):
            train.fusion_step_loss(x.cuda(), beta.cuda(), y.cuda(), n_valid=bad)
