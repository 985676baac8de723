"""GPU suite, attention: every kernel variant hri-emo_amd/csrc/attention.hip can launch on the padded path, against the float64
reference of tests/attn_reference.py with limits that come from that reference alone (attn_reference.check), at mask patterns
that sit on the tile edges, and with every output inside a guarded buffer so that a store outside it is seen.

The variant table names, per row, the form each launch must take.  Both forms are asserted THROUGH THE ABI (hriemo_attn_plan:
the plan the launches themselves follow), so a change of the heuristics that takes a kernel out of the table fails here with
"update the table" instead of thinning the coverage silently.  Rows with B = W use the first batch size for which
the ABI reports the 128-row tile on this device (it depends on the CU count); finding none is a failure.  Nothing skips."""
import numpy as np
import pytest
import torch

import attn_reference as R
import hashrng
from attn_gpu import (BWD_SIDE, FWD_FORM, GUARD_FLOATS, GUARD_ROWS, SENTINEL, W, Guarded, GuardedFlat,  # noqa: F401  (other test
                      backward_form, forward_form, plan, wide_batch)                                # files read them from here)

pytestmark = pytest.mark.gpu

SEED, SITE, BOFF = 1234567890123, 40, 5

VARIANTS = [  # B, H, Lq, Lk, hd, mask pattern, p, forward form, backward form
    # two-kernel backward, 128-row tiles (self-audio at 16 utterances per rank; B from the scan)
    (W, 8, 400, 400, 96, "edges", 0.1, "fwd<4,2>", "two-kernel(dq=w128,dkv=w128)"),
    (W, 8, 256, 256, 96, "leading", 0.1, "fwd<4,2>", "two-kernel(dq=w128,dkv=w128)"),
    (W, 8, 256, 192, 96, "allpad", 0.1, "fwd<4,2>", "two-kernel(dq=w128,dkv=n64)"),
    (W, 8, 192, 256, 96, "none", 0.1, "fwd<4,2>", "two-kernel(dq=n64,dkv=w128)"),
    (W, 8, 200, 200, 16, "prefix", 0.1, "fwd<4,2>", "two-kernel(dq=w128,dkv=w128)"),
    (W, 8, 200, 200, 32, "none", 0.1, "fwd<4,2>", "two-kernel(dq=w128,dkv=w128)"),
    (W, 8, 200, 200, 64, "prefix", 0.1, "fwd<4,2>", "two-kernel(dq=w128,dkv=w128)"),
    (W, 8, 200, 200, 96, "prefix", 0.0, "fwd<4,2>", "two-kernel(dq=w128,dkv=w128)"),
    # two-kernel backward, 64-row tiles
    (2, 8, 400, 400, 96, "prefix", 0.1, "fwd<4,2>", "two-kernel(dq=n64,dkv=n64)"),      # self-audio at the headline shape
    (2, 8, 400, 400, 96, "prefix", 0.0, "fwd<4,2>", "two-kernel(dq=n64,dkv=n64)"),
    (4, 4, 400, 400, 128, "prefix", 0.1, "fwd<4,2>", "two-kernel(dq=n64,dkv=n64)"),     # head_dim 128 is never wide
    (2, 8, 200, 300, 16, "prefix", 0.1, "fwd<4,2>", "two-kernel(dq=n64,dkv=n64)"),
    (12, 2, 130, 400, 64, "edges", 0.1, "fwd<4,2>", "two-kernel(dq=n64,dkv=n64)"),
    (3, 4, 150, 200, 32, "leading", 0.1, "fwd<4,2>", "two-kernel(dq=n64,dkv=n64)"),
    (3, 2, 129, 129, 96, "allpad", 0.0, "fwd<4,2>", "two-kernel(dq=n64,dkv=n64)"),
    # key-resident single pass, 64 < L_k <= 128
    (2, 8, 128, 128, 96, "prefix", 0.1, "fwd<4,2>", "fused-KW2"),                       # self-text
    (2, 8, 400, 128, 96, "prefix", 0.1, "fwd<4,1>", "fused-KW2"),                       # a2t
    (9, 2, 100, 128, 128, "edges", 0.1, "fwd<4,2>", "fused-KW2"),
    (3, 4, 70, 100, 64, "leading", 0.1, "fwd<4,2>", "fused-KW2"),
    (3, 4, 128, 128, 32, "allpad", 0.1, "fwd<4,2>", "fused-KW2"),
    (2, 4, 200, 70, 64, "none", 0.2, "fwd<4,2>", "fused-KW2"),
    # key-resident single pass, 16 < L_k <= 64
    (6, 4, 100, 64, 96, "edges", 0.1, "fwd<4,2>", "fused-KW1"),
    (4, 8, 48, 17, 32, "edges", 0.1, "fwd<4,1>", "fused-KW1"),
    (3, 4, 70, 40, 64, "leading", 0.1, "fwd<4,2>", "fused-KW1"),
    (3, 2, 33, 64, 128, "allpad", 0.1, "fwd<4,1>", "fused-KW1"),
    (2, 2, 33, 17, 32, "none", 0.2, "fwd<4,1>", "fused-KW1"),
    # query-resident single pass, 16 < L_q <= 128 < L_k
    (2, 8, 128, 400, 96, "prefix", 0.1, "fwd<4,2>", "qres"),                            # t2a
    (2, 8, 17, 129, 96, "none", 0.2, "fwd<4,1>", "qres"),                               # the smallest shape that takes it
    (2, 4, 128, 1000, 64, "prefix", 0.1, "fwd<4,2>", "qres"),
    (12, 2, 100, 300, 128, "edges", 0.1, "fwd<4,2>", "qres"),
    (3, 4, 64, 200, 32, "leading", 0.1, "fwd<4,1>", "qres"),
    (3, 2, 50, 200, 64, "allpad", 0.0, "fwd<4,1>", "qres"),
    # one-wave forms (L <= 16 on a side)
    (2, 8, 6, 6, 96, "none", 0.1, "fwd<1,1>", "two-kernel(dq=1w,dkv=1w)"),
    (2, 8, 6, 400, 96, "prefix", 0.1, "fwd<1,1>", "two-kernel(dq=1w,dkv=n64)"),         # decoder queries over a long memory
    (2, 8, 400, 16, 32, "prefix", 0.1, "fwd<4,1>", "two-kernel(dq=n64,dkv=1w)"),
    (3, 8, 32, 16, 16, "prefix", 0.1, "fwd<4,1>", "two-kernel(dq=n64,dkv=1w)"),
    (4, 2, 10, 16, 16, "edges", 0.1, "fwd<1,1>", "two-kernel(dq=1w,dkv=1w)"),
    (3, 2, 12, 16, 64, "leading", 0.1, "fwd<1,1>", "two-kernel(dq=1w,dkv=1w)"),
    (3, 2, 16, 12, 128, "allpad", 0.1, "fwd<1,1>", "two-kernel(dq=1w,dkv=1w)"),
    (2, 4, 16, 16, 32, "none", 0.1, "fwd<1,1>", "two-kernel(dq=1w,dkv=1w)"),
    (2, 2, 6, 6, 16, "none", 0.0, "fwd<1,1>", "two-kernel(dq=1w,dkv=1w)"),
]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _ops
    return _ops


def _ids():
    return [f"{B}x{H}x{Lq}x{Lk}-hd{hd}-{pat}-p{p}-{bwd}" for B, H, Lq, Lk, hd, pat, p, _, bwd in VARIANTS]


@pytest.mark.parametrize("B,H,Lq,Lk,hd,pattern,p,fwd,bwd", VARIANTS, ids=_ids())
def test_attention_variant(ops, B, H, Lq, Lk, hd, pattern, p, fwd, bwd):
    from hri_emo_amd import _lib
    L_ = _lib.lib()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if B == W:
        B = wide_batch(L_, H, Lq, Lk, hd, bwd)
    got_form = backward_form(L_, B, H, Lq, Lk, hd)
    assert got_form == bwd, (f"the backward of (B={B}, H={H}, Lq={Lq}, Lk={Lk}, hd={hd}) is now {got_form}, the variant table "
                             f"says {bwd}: update the table so that every kernel form stays covered")
    assert forward_form(L_, B, H, Lq, Lk, hd) == fwd, (forward_form(L_, B, H, Lq, Lk, hd), fwd)
    d = H * hd
    qb, kvb, dob = R.make_inputs(B, H, Lq, Lk, hd, 100 + Lq + Lk)
    kpm = R.key_padding_mask(pattern, B, Lk)
    keep = torch.from_numpy(hashrng.attn_mask(SEED, SITE, B, H, Lq, Lk, p, BOFF)) if p > 0 else None
    ref, yard, mag = R.all_three(R.heads(qb, B, Lq, H, hd), R.heads(kvb[:, :d], B, Lk, H, hd), R.heads(kvb[:, d:], B, Lk, H, hd),
                                 R.heads(dob, B, Lq, H, hd), kpm, keep, hashrng.inv_keep(p))
    good = torch.ones(B, dtype=torch.bool)          # samples with at least one valid key
    if kpm is not None:
        good = ~kpm.all(1)
    assert (pattern == "allpad") == (not bool(good.all()))

    # inputs: guard rows (and pad columns) that read as NaN; outputs: guard bytes compared after the launches
    ld1, ld2 = d + 8, 2 * d + 16
    q_g = Guarded(B * Lq, d, torch.bfloat16, ld1, fill=qb.cuda())
    kv_g = Guarded(B * Lk, 2 * d, torch.bfloat16, ld2, fill=kvb.cuda())
    do_g = Guarded(B * Lq, d, torch.bfloat16, ld1, fill=dob.cuda())
    o_g = Guarded(B * Lq, d, torch.bfloat16, ld1)
    lse_g = GuardedFlat(B * H * Lq, torch.float32, GUARD_FLOATS)
    nkt = (Lk + 63) // 64
    mb_g = None
    if p > 0:
        assert L_.hriemo_attn_mask_bytes(B, H, Lq, Lk) == B * H * Lq * nkt * 8
        mb_g = Guarded(B * H * Lq, nkt, torch.int64)
    kpm_d = kpm.cuda().view(torch.uint8) if kpm is not None else None
    qd, kd, vd, dod, o = q_g.t, kv_g.t[:, :d], kv_g.t[:, d:], do_g.t, o_g.t
    seed_word = ops.seed_word(qd.device)
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    guarded = {"Q": q_g, "K|V": kv_g, "dO": do_g, "O": o_g, "lse": lse_g}
    if mb_g is not None:
        guarded["mask bits"] = mb_g

    _lib.call("hriemo_attn_fwd", qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(), vd.stride(0),
              o.data_ptr(), o.stride(0), ptr(kpm_d), lse_g.t.data_ptr(), B, H, Lq, Lk, hd, float(p), SEED, seed_word.data_ptr(),
              SITE, BOFF, ptr(None if mb_g is None else mb_g.t), stream)
    torch.cuda.synchronize()
    lse = lse_g.t.view(B, H, Lq)
    worst = {}

    def checked(name, got2d, L):
        got = R.heads(got2d.float().cpu(), B, L, H, hd)
        worst[name] = R.check(got[good], ref[name][good], yard[name][good], mag[name][good], name)
        return got

    o4 = checked("O", o, Lq)
    if not good.all():
        assert torch.isnan(o4[~good]).all(), "O of a sample whose keys are all PAD is NaN, like the reference"
    lse_ref = ref["lse"][good]
    assert (lse.cpu().double()[good] - lse_ref).abs().max() <= 2e-3 * max(1.0, lse_ref.abs().max().item())
    if p > 0:
        # bit 16*g + 4*n + r of word (b, h, q, tile) <-> key 64*tile + 16*n + 4*g + r, equal to the host replica of the hash
        w = mb_g.t.view(B, H, Lq, nkt).cpu().numpy().astype(np.uint64)
        key = np.arange(Lk)
        bitpos = ((key % 16) // 4) * 16 + ((key % 64) // 16) * 4 + key % 4
        got_keep = ((w[..., key // 64] >> bitpos.astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert np.array_equal(got_keep, keep.numpy())

    pr_g = Guarded(B * Lq, Lk, torch.float32)
    guarded["probs"] = pr_g
    _lib.call("hriemo_attn_probs", qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), ptr(kpm_d), lse_g.t.data_ptr(),
              pr_g.t.data_ptr(), B, H, Lq, Lk, hd, float(p), SEED, seed_word.data_ptr(), SITE, BOFF, stream)
    probs = pr_g.t.view(B, Lq, Lk).cpu()
    assert (probs[good].double() - ref["Pmean"][good]).abs().max() <= 5e-3
    if kpm is not None:
        gk = kpm[good]
        assert float(probs[good][gk[:, None, :].expand(gk.shape[0], Lq, Lk)].abs().max()) == 0.0
    if not good.all():
        assert torch.isnan(probs[~good]).all()

    def backward(name, bits, partials):
        dq_g = Guarded(B * Lq, d, torch.bfloat16, ld1)
        dkv_g = Guarded(B * Lk, 2 * d, torch.bfloat16, ld2)
        delta_g = GuardedFlat(B * H * Lq, torch.float32, GUARD_FLOATS)
        guarded.update({f"dQ ({name})": dq_g, f"dK|dV ({name})": dkv_g, f"delta ({name})": delta_g})
        pq_g = pkv_g = None
        if partials:
            rq, rk = L_.hriemo_attn_bwd_dq_colsum_rows(B, H, Lq, Lk, hd), L_.hriemo_attn_bwd_kv_colsum_rows(B, H, Lq, Lk, hd)
            pq_g, pkv_g = Guarded(rq, d, torch.float32, guard_rows=8), Guarded(rk, 2 * d, torch.float32, guard_rows=8)
            guarded.update({"dQ partials": pq_g, "dK|dV partials": pkv_g})
        dq, dk, dv = dq_g.t, dkv_g.t[:, :d], dkv_g.t[:, d:]
        _lib.call("hriemo_attn_bwd", qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(), vd.stride(0),
                  o.data_ptr(), o.stride(0), dod.data_ptr(), dod.stride(0), dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0),
                  dv.data_ptr(), dv.stride(0), ptr(kpm_d), lse_g.t.data_ptr(), delta_g.t.data_ptr(), B, H, Lq, Lk, hd, float(p), SEED,
                  seed_word.data_ptr(), SITE, BOFF, ptr(None if pq_g is None else pq_g.t), ptr(None if pkv_g is None else pkv_g.t),
                  ptr(mb_g.t if bits else None), stream)
        torch.cuda.synchronize()
        return dq, dkv_g.t, pq_g, pkv_g

    dq, dkv, _, _ = backward("bit words" if p > 0 else "no dropout", p > 0, False)
    dq4 = checked("dQ", dq, Lq)
    checked("dK", dkv[:, :d], Lk)
    checked("dV", dkv[:, d:], Lk)
    if not good.all():
        assert torch.isnan(dq4[~good]).all(), "dQ of a sample whose keys are all PAD is NaN, like the reference"
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))     # bits: NaN == NaN
    if p > 0:       # mask from the bit words == mask replayed from the hash: bit-identical gradients
        dq_h, dkv_h, _, _ = backward("hash", False, False)
        assert same(dq_h, dq) and same(dkv_h, dkv)
    dq2, dkv2, pq_g, pkv_g = backward("partials", p > 0, True)
    assert same(dq2, dq) and same(dkv2, dkv)
    if good.all():
        # column-sum partials (in-projection bias gradient): sums of the fp32 values BEFORE their bf16 rounding, compared with
        # the column sums of the reference gradients; at least as close to them as the column sums of the stored tiles are
        dq_ref = R.rows(ref["dQ"]).float()
        dkv_ref = torch.cat([R.rows(ref["dK"]), R.rows(ref["dV"])], 1).float()
        for name, part, full, r in (("dq", pq_g.t, dq, dq_ref.sum(0)), ("dkv", pkv_g.t, dkv, dkv_ref.sum(0))):
            got = part.sum(0).cpu()
            stored = full.float().sum(0).cpu()
            assert not torch.isnan(part).any(), name       # every partial row is written
            scale = max(1.0, r.abs().max().item())
            assert (got - r).abs().max() <= 2e-2 * scale, (name, (got - r).abs().max(), scale)
            assert (got - stored).abs().max() <= 1e-2 * scale, (name, "vs stored tiles", (got - stored).abs().max())
            assert (got - r).norm() <= 1.05 * (stored - r).norm() + 1e-6 * scale, (name, (got - r).norm(), (stored - r).norm())

    broken = [name for name, g in guarded.items() if not g.intact()]
    assert not broken, f"bytes outside the payload were written: {broken}"
    print(f"\n  [attn-variant] B={B} H={H} Lq={Lq} Lk={Lk} hd={hd} mask={pattern} p={p}: {fwd}, {got_form} (asserted through the ABI); "
          + "error / limit (elementwise, per tile): " + ", ".join(f"{n} {e:.3f} {t:.3f}" for n, (e, t) in worst.items()))
