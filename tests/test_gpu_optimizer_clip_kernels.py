"""GPU suite of the unit clip kernels (csrc/optim.hip): hriemo_sumsq_units -> hriemo_optim_finalize_units ->
hriemo_adamw_flat_units through the C ABI on guarded buffers, every guard intact after every launch, with sentinel words in
clip_state and in the state rows no kernel may touch.

Bounds: norm_u, coef_u and the global norm against float64 (clip_reference.py) within max(1e-5 relative -- the project's bound for
norms and coefficients --, the bound counted from the summation tree); for every shape here the counted bound is the NARROWER one
(<= 4.5e-6), so 1e-5 applies, and the test prints both.  p, m, v against float64 within 2e-6 * max(1, |ref|), the bound
test_gpu_optimizer.py derives.  Bit-identity claims and why they hold: the unit update kernel and the single-group one call ONE
inline function per 16-byte vector, so a unit's elements equal what hriemo_adamw_flat_dev writes on a clone under the group's hyper
row and a state block whose coef is the coef_u read from clip_state; with every unit unclipped both paths use coef = 1 / gs exactly,
so the whole step equals the existing sumsq_f32 + finalize_groups + adamw_flat_groups path.

Measured on MI355X over all six shapes (the test prints every figure): worst relative error of a unit norm 5.3e-8, of a unit
coefficient 7.0e-8; worst |err| of p 7.2e-7 against the 2e-6 bound."""
import math

import pytest
import torch

from clip_reference import PROJECT_REL, elem_index, global_norm_bound, unit_bounds, unit_step_ref64
from health_reference import assert_no_underflow
from rowops_reference import GuardedVec

pytestmark = pytest.mark.gpu


@pytest.fixture()
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd
    yield hri_emo_amd
    hri_emo_amd.set_varlen(False)


def ST():
    return torch.cuda.current_stream().cuda_stream


def GV(x):
    return GuardedVec.of(x.contiguous(), device="cuda")


# three groups with distinct lr, betas, eps, weight decay AND max_norm (word 5 of every row is read in the unit modes)
HYPER = torch.tensor([[1e-3, 0.90, 0.999, 1e-8, 1e-2, 5.0, 0.0, 0.0],
                      [3e-4, 0.80, 0.990, 1e-6, 0.0, 0.5, 0.0, 0.0],
                      [2e-3, 0.95, 0.980, 1e-7, 5e-2, -1.0, 0.0, 0.0]], dtype=torch.float32)
MAX_NORM = [5.0, 0.5, -1.0]
N_SWEEP = 4 * 256 * 4096                        # elements one sweep of the capped grid covers
CHUNK = 32768
# name -> (seg, seg_group, seg_unit, unit_group, the unscaled gradient norm every unit is given)
CASES = {
    "a: one unit of 64 elements": ([0, 64], [0], [0], [0], [12.0]),
    "b: units of one chunk and of a chunk plus 64": ([0, CHUNK, 2 * CHUNK + 64], [0, 1], [0, 1], [0, 1], [4.0, 7.0]),
    "c: a unit owning two non-adjacent slots": ([0, 64, 192, 256], [1, 0, 1], [1, 0, 1], [0, 1], [20.0, 0.3]),
    "d: clipped x100, just under, unclipped": ([0, 1024, 3072, 3136], [0, 1, 2], [0, 1, 2], [0, 1, 2], [500.0, 0.49, 3.0]),
    "e: a unit boundary at N_SWEEP": ([0, N_SWEEP, N_SWEEP + 64, N_SWEEP + 128], [0, 1, 2], [0, 1, 2], [0, 1, 2], [50.0, 0.2, 9.0]),
    "f: an all-zero unit": ([0, 64, 128], [0, 1], [0, 1], [0, 1], [2.0, 0.0]),
}
SENTINEL = -7.0


def _gradient(gen, n, elem_unit, targets, scale):
    """fp32 gradient whose unit u has (float64) norm targets[u], times the power-of-two grad scale (exact)"""
    g = torch.randn(n, generator=gen).double()
    for u, t in enumerate(targets):
        mask = elem_unit == u
        g[mask] *= t / float(g[mask].norm())
    return g.float() * scale


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_unit_kernels_through_the_c_abi(H, case):
    from hri_emo_amd import _lib
    from hri_emo_amd.optim import unit_chunk_table
    seg_h, sg_h, su_h, ug_h, targets = CASES[case]
    n, S, U, G, nblocks = seg_h[-1], len(sg_h), len(ug_h), 3, 1024
    chunks_h, uc_h = unit_chunk_table(seg_h, su_h, ug_h)
    C = len(chunks_h)
    gen = torch.Generator().manual_seed(n + S)
    elem_group, elem_unit = elem_index(seg_h, sg_h), elem_index(seg_h, su_h)
    assert elem_unit.numel() == n
    unit_mn = [MAX_NORM[g] for g in ug_h]
    cols = HYPER.double()[elem_group][:, :5].t().contiguous()
    masks = [(elem_unit == u).cuda() for u in range(U)]
    rel_sum, rel_norm, rel_coef = unit_bounds(chunks_h, U)
    rel_total = global_norm_bound(chunks_h, U)
    print(f"{case}: C = {C}; counted relative bounds: norm {max(rel_norm):.2e}, coef {max(rel_coef):.2e}, global {rel_total:.2e}; "
          f"the project's {PROJECT_REL:.0e} is {'wider: it applies' if PROJECT_REL >= max(rel_coef + [rel_total]) else 'narrower: the counted bound applies'}")
    tol_norm = [max(PROJECT_REL, r) for r in rel_norm]
    tol_coef = [max(PROJECT_REL, r) for r in rel_coef]
    tol_total = max(PROJECT_REL, rel_total)

    p0 = torch.randn(n, generator=gen)
    p, m, v, g = GV(p0), GV(torch.zeros(n)), GV(torch.zeros(n)), GuardedVec(n, torch.float32, device="cuda")
    partial, partial_old = GuardedVec(C, torch.float32, device="cuda"), GuardedVec(nblocks, torch.float32, device="cuda")
    hyper = GV(HYPER.reshape(-1))
    state0 = torch.full((G * 8,), SENTINEL)
    state0[:8] = 0.0
    state = GV(state0)
    clip = GV(torch.full((2 * U,), SENTINEL))
    seg, seg_group, seg_unit = (GV(torch.tensor(t, dtype=dt)) for t, dt in ((seg_h, torch.int64), (sg_h, torch.int32), (su_h, torch.int32)))
    chunks = GV(torch.tensor(chunks_h, dtype=torch.int64).reshape(-1))
    unit_chunks, unit_group = GV(torch.tensor(uc_h, dtype=torch.int32)), GV(torch.tensor(ug_h, dtype=torch.int32))
    ctl = GV(torch.tensor([5, 0, 0, 0], dtype=torch.int32))
    hyper_rows = [GV(HYPER[k]) for k in range(G)]
    scale_t, inf_t = torch.tensor([8.0], device="cuda"), torch.zeros(1, device="cuda")
    bufs = [p, m, v, g, partial, partial_old, hyper, state, clip, seg, seg_group, seg_unit, chunks, unit_chunks, unit_group, ctl] + hyper_rows
    P = lambda t: None if t is None else t.data_ptr()

    def units(gs, fi, c=None, hy=hyper, S_=S, U_=U, G_=G, seg_ptr=None):
        _lib.call("hriemo_sumsq_units", g.ptr, n, chunks.ptr, C, partial.ptr, ST())
        _lib.call("hriemo_optim_finalize_units", partial.ptr, C, unit_chunks.ptr, unit_group.ptr, U_, hy.ptr, G_, P(gs), P(fi), state.ptr,
                  None if c is None else c.ptr, clip.ptr, None, None, ST())
        _lib.call("hriemo_adamw_flat_units", p.ptr, g.ptr, m.ptr, v.ptr, n, seg.ptr if seg_ptr is None else seg_ptr, seg_group.ptr,
                  seg_unit.ptr, S_, hy.ptr, state.ptr, G_, clip.ptr, U_, ST())
        torch.cuda.synchronize()

    def single(u, pre, st_row0, coef_u):
        """the EXISTING hriemo_adamw_flat_dev with the hyper row of unit u's group on clones of the whole buffers, under a state
        block that holds coef_u and the group's step_size, 1 / sqrt(bc2) and decay as the unit finalize left them"""
        k = ug_h[u]
        pc, mc, vc = (GV(t) for t in pre)
        blk = st_row0.clone()
        blk[2] = coef_u
        blk[3:6] = state.view[8 * k + 3:8 * k + 6]
        sc = GV(blk)
        _lib.call("hriemo_adamw_flat_dev", pc.ptr, g.ptr, mc.ptr, vc.ptr, n, hyper_rows[k].ptr, sc.ptr, ST())
        torch.cuda.synchronize()
        for b in (pc, mc, vc, sc):
            b.assert_intact("clone")
        return pc.view, mc.view, vc.view

    def groups_finalize(pre_state, gs, fi, c):
        """the EXISTING sumsq_f32 + finalize_groups on a clone of the state block -> state [G * 8]"""
        sc = GV(pre_state)
        _lib.call("hriemo_sumsq_f32", g.ptr, n, partial_old.ptr, nblocks, ST())
        _lib.call("hriemo_optim_finalize_groups", partial_old.ptr, nblocks, hyper.ptr, G, P(gs), P(fi), sc.ptr, None if c is None else c.ptr, ST())
        torch.cuda.synchronize()
        sc.assert_intact("state clone")
        return sc.view

    def intact():
        for i, b in enumerate(bufs):
            b.assert_intact(f"buffer {i}")

    rp, rm, rv = p0.double(), torch.zeros(n).double(), torch.zeros(n).double()
    for step, gs, c in ((1, None, None), (2, scale_t, None), (3, None, ctl)):
        scale = 1.0 if gs is None else 8.0
        gh = _gradient(gen, n, elem_unit, targets, scale)
        assert_no_underflow(gh)
        g.view.copy_(gh)
        ref = unit_step_ref64(rp, gh.double(), rm, rv, cols, step, elem_unit, unit_mn, scale)
        rp, rm, rv, norms, coefs, total = ref
        if case.startswith("d"):
            # the float64 reference itself: unit 0 clipped about 100-fold, unit 1 not clipped (just under), unit 2 has no max_norm
            assert coefs[0] * scale < 0.011 and norms[1] < 0.5 and coefs[1] * scale == 1.0 and coefs[2] * scale == 1.0 and norms[2] > 0.5
        if c is not None:
            # HOLD first: last = 0 touches nothing but state.skip
            before = [b.view.clone() for b in (p, m, v, state, clip)]
            units(gs, None, c)
            for b, old, what in zip((p, m, v, clip), before[:3] + before[4:], ("p", "m", "v", "clip_state")):
                assert torch.equal(b.view.view(torch.int32), old.view(torch.int32)), f"the held launch moved {what}"
            st = state.view.clone()
            assert float(st[1]) == 1.0 and float(before[3][1]) == 0.0, "the hold sets state.skip"
            st[1] = before[3][1]
            assert torch.equal(st.view(torch.int32), before[3].view(torch.int32)), "every other word of every row stays"
            intact()
            ctl.view[2] = 1
            state.view[1] = 0.0
        pre = [b.view.clone() for b in (p, m, v)]
        pre_state = state.view.clone()
        units(gs, None if gs is None else inf_t, c)
        s, cs = state.view.cpu(), clip.view.cpu().reshape(U, 2)
        assert s[0].item() == step and s[1].item() == 0.0 and s[7].item() == 0.0, s
        for u in range(U):
            en = abs(cs[u, 0].item() - norms[u]) / max(norms[u], 1e-30) if norms[u] else abs(cs[u, 0].item())
            ec = abs(cs[u, 1].item() - coefs[u]) / coefs[u]
            print(f"   step {step} unit {u}: norm {cs[u, 0].item():.6e} ref {norms[u]:.6e} rel {en:.2e} (bound {tol_norm[u]:.1e}, counted "
                  f"{rel_norm[u]:.1e})  coef {cs[u, 1].item():.6e} ref {coefs[u]:.6e} rel {ec:.2e} (bound {tol_coef[u]:.1e})")
            assert en <= tol_norm[u] and ec <= tol_coef[u], (step, u, cs[u], norms[u], coefs[u])
        assert abs(s[6].item() - total) <= tol_total * total, (s[6].item(), total)
        assert s[2].item() == cs[:, 1].min().item(), "state.coef holds the smallest unit coefficient"
        if case.startswith("d"):
            assert cs[1, 1].item() == 1.0 / scale and cs[2, 1].item() == 1.0 / scale, "unclipped units: coef is exactly 1 / gs"
        if case.startswith("f"):
            assert cs[1, 0].item() == 0.0 and cs[1, 1].item() == 1.0 / scale, "an all-zero unit: norm 0, coef 1"
        for got, want, what in ((p.view, rp, "p"), (m.view, rm, "m"), (v.view, rv, "v")):
            err = (got.cpu().double() - want).abs()
            print(f"   step {step} {what}: max |err| {err.max().item():.3e}")
            assert bool((err <= 2e-6 * want.abs().clamp_min(1.0)).all()), (what, step, err.max().item())
        for k in range(1, G):
            row = s[8 * k:8 * k + 8]
            assert all(row[w].item() == SENTINEL for w in (0, 1, 2, 6, 7)), ("rows g >= 1: words 3, 4, 5 and nothing else", k, row)
        # every word of state but the two the unit modes define anew (coef, grad_norm) is finalize_groups' bit for bit
        old = groups_finalize(pre_state, gs, None if gs is None else inf_t, c).cpu()
        same = [w for w in range(G * 8) if w not in (2, 6)]
        assert torch.equal(s[same].view(torch.int32), old[same].view(torch.int32)), (s, old)
        assert abs(s[6].item() - old[6].item()) <= 2 * tol_total * total
        # per unit, bit for bit: the single-group update under coef_u
        for u in range(U):
            sp, sm, sv = single(u, pre, state.view[:8], clip.view[2 * u + 1])
            for got, one, what in ((p.view, sp, "p"), (m.view, sm, "m"), (v.view, sv, "v")):
                assert torch.equal(got[masks[u]].view(torch.int32), one[masks[u]].view(torch.int32)), (what, "unit", u, "step", step)
        intact()

    # a skipped step: found_inf = 1 -- p, m, v stay, the norms are written, the coef column is not
    clip_norms_before = clip.view.clone()
    clip.view[1::2] = SENTINEL
    before = [b.view.clone() for b in (p, m, v, state)]
    inf_t.fill_(1.0)
    units(scale_t, inf_t)
    s, cs = state.view.cpu(), clip.view.cpu().reshape(U, 2)
    assert s[0].item() == 3.0 and s[1].item() == 1.0 and s[7].item() == 1.0, s
    for b, old in zip((p, m, v), before):
        assert torch.equal(b.view.view(torch.int32), old.view(torch.int32))
    assert torch.equal(state.view[8:], before[3][8:]), "a skipped step writes no word of the rows g >= 1"
    assert all(cs[u, 1].item() == SENTINEL for u in range(U)), "a skipped step leaves the coef column alone"
    # the gradient buffer still holds step 3's (unscaled) values, read under a grad scale of 8
    assert all(abs(cs[u, 0].item() * 8.0 - clip_norms_before[2 * u].item()) <= 1e-6 * clip_norms_before[2 * u].item() for u in range(U))
    intact()

    # one NaN in unit 1 (the only unit where there is one): skipped on the norm, that unit's norm is NaN, the others finite
    bad = min(1, U - 1)
    where = int(torch.nonzero(elem_unit == bad)[-1])
    inf_t.fill_(0.0)
    state.view[1] = 0.0
    old_val = g.view[where].clone()
    g.view[where] = float("nan")
    before = [b.view.clone() for b in (p, m, v, state)]
    units(None, None)
    s, cs = state.view.cpu(), clip.view.cpu().reshape(U, 2)
    assert s[0].item() == 3.0 and s[1].item() == 1.0 and s[7].item() == 2.0 and math.isnan(s[6].item()), s
    for b, old in zip((p, m, v), before):
        assert torch.equal(b.view.view(torch.int32), old.view(torch.int32))
    assert math.isnan(cs[bad, 0].item()) and all(math.isfinite(cs[u, 0].item()) for u in range(U) if u != bad), cs
    assert all(cs[u, 1].item() == SENTINEL for u in range(U)), "the coef column is untouched"
    g.view[where] = old_val
    intact()

    # every unit unclipped (max_norm <= 0 in every row): bit for bit the existing grouped path, coef = 1 / gs exactly in both
    hy_off = HYPER.clone()
    hy_off[:, 5] = torch.tensor([0.0, -1.0, -3.0])
    hyper_off = GV(hy_off.reshape(-1))
    start = [b.view.clone() for b in (p, m, v, state)]
    state.view[1] = 0.0
    start[3][1] = 0.0
    units(scale_t, inf_t, hy=hyper_off)
    got = [b.view.clone() for b in (p, m, v)]
    assert not torch.equal(got[0], start[0]) and float(state.view[0]) == 4.0
    for b, old in zip((p, m, v, state), start):
        b.view.copy_(old)
    _lib.call("hriemo_sumsq_f32", g.ptr, n, partial_old.ptr, nblocks, ST())
    _lib.call("hriemo_optim_finalize_groups", partial_old.ptr, nblocks, hyper_off.ptr, G, scale_t.data_ptr(), inf_t.data_ptr(), state.ptr, None, ST())
    _lib.call("hriemo_adamw_flat_groups", p.ptr, g.ptr, m.ptr, v.ptr, n, seg.ptr, seg_group.ptr, S, hyper_off.ptr, state.ptr, G, ST())
    torch.cuda.synchronize()
    assert float(state.view[0]) == 4.0 and float(state.view[2]) == 0.125
    for b, mine, what in zip((p, m, v), got, "pmv"):
        assert torch.equal(b.view.view(torch.int32), mine.view(torch.int32)), ("unclipped units against the grouped path", what)
    hyper_off.assert_intact("hyper_off")
    intact()

    # the limits: refused in front of the launch
    state.view[1] = 0.0                                        # not skipped: a launch that did run would move p
    before = [b.view.clone() for b in (p, m, v, state, clip)]
    upd = lambda **kw: _lib.call("hriemo_adamw_flat_units", p.ptr, g.ptr, m.ptr, v.ptr, n, kw.get("seg", seg.ptr), seg_group.ptr, seg_unit.ptr,
                                 kw.get("S", S), hyper.ptr, state.ptr, kw.get("G", G), clip.ptr, kw.get("U", U), ST())
    fin = lambda **kw: _lib.call("hriemo_optim_finalize_units", partial.ptr, kw.get("C", C), unit_chunks.ptr, unit_group.ptr, kw.get("U", U),
                                 hyper.ptr, kw.get("G", G), None, None, state.ptr, None, clip.ptr, None, None, ST())
    with pytest.raises(RuntimeError, match=r"adamw_flat_units: U=2049 units"):
        upd(U=2049)
    with pytest.raises(RuntimeError, match=r"adamw_flat_units: S=2049 segments"):
        upd(S=2049)
    with pytest.raises(RuntimeError, match=r"adamw_flat_units: G=17 groups"):
        upd(G=17)
    with pytest.raises(RuntimeError, match=r"adamw_flat_units: seg .* is not 8-byte aligned"):
        upd(seg=seg.ptr + 4)
    with pytest.raises(RuntimeError, match=r"optim_finalize_units: U=2049 units"):
        fin(U=2049, C=4096)
    with pytest.raises(RuntimeError, match=r"optim_finalize_units: G=17 groups"):
        fin(G=17)
    with pytest.raises(RuntimeError, match=r"sumsq_units: C=0 chunks"):
        _lib.call("hriemo_sumsq_units", g.ptr, n, chunks.ptr, 0, partial.ptr, ST())
    with pytest.raises(RuntimeError, match=r"sumsq_units: chunks .* 8-byte aligned"):
        _lib.call("hriemo_sumsq_units", g.ptr, n, chunks.ptr + 4, C, partial.ptr, ST())
    with pytest.raises(RuntimeError, match=r"sumsq_units: C=\d+ chunks"):            # more chunks than 16-byte vectors (or than 2^20)
        _lib.call("hriemo_sumsq_units", g.ptr, n, chunks.ptr, n // 4 + 1, partial.ptr, ST())
    torch.cuda.synchronize()
    for b, old in zip((p, m, v, state, clip), before):
        assert torch.equal(b.view.view(torch.int32), old.view(torch.int32)), "a refused call launches nothing"
    intact()
