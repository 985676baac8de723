"""GPU suite, attention backward: a dropout hash word belongs to a key PAIR (low half: the even key, high half: the odd one), and
in the dK/dV kernels that replay the hash a lane owns ONE key, so lanes i and i ^ 1 evaluate the same word and each keeps its
half.  Masks are defined by the hash: the replay (mask_bits = NULL) must give the bits of the backward that reads the forward's
mask words -- dQ, dK, dV, delta and both column-sum partial buffers are compared bit for bit -- and the forward's words must be
the host replica of the hash (tests/hashrng.py).  This pins the keep decisions at the places where a key pair is split, for any
later change of how the lanes of a pair come by their word.

Shapes: the smallest that reach each dK/dV arm with a hash replay -- asserted through hriemo_attn_plan first, as
test_gpu_attention_variants.py does -- each with an odd L_k (the last key pair is half outside), a prefix key mask of odd length,
b_offset 3 and an L_q that is no multiple of the 32-query tile.  Everything sits in guarded buffers."""
import numpy as np
import pytest
import torch

import attn_reference as R
import hashrng
from test_gpu_attention_variants import GUARD_FLOATS, Guarded, GuardedFlat, backward_form

pytestmark = pytest.mark.gpu

SEED, SITE, BOFF = 987654321987, 12, 3
W = "W"                 # batch size found at run time: the first one whose dK/dV tile is the 128-row one

CASES = [  # B, H, Lq, Lk, hd, dK/dV arm
    (2, 2, 193, 193, 96, "two-kernel dkv=n64"),
    (2, 2, 193, 193, 32, "two-kernel dkv=n64"),
    (2, 2, 150, 13, 32, "two-kernel dkv=1w"),
    (W, 8, 193, 193, 32, "two-kernel dkv=w128"),
    # the key-resident single pass replays the hash in the BITS == false arm of attn_bwd_dkv_kernel
    (2, 2, 150, 101, 96, "fused-KW2"),
    (2, 2, 150, 101, 32, "fused-KW2"),
    (2, 2, 150, 41, 32, "fused-KW1"),
]


def arm(L_, B, H, Lq, Lk, hd):
    form = backward_form(L_, B, H, Lq, Lk, hd)
    if form.startswith("two-kernel"):
        return "two-kernel " + form[form.index("dkv="):-1]
    return form


def wide_batch(L_, H, Lq, Lk, hd):
    for B in range(1, 129):
        if arm(L_, B, H, Lq, Lk, hd) == "two-kernel dkv=w128":
            return B
    raise AssertionError(f"no batch size in 1..128 takes the 128-row dK/dV tile at H={H}, Lq={Lq}, Lk={Lk}, hd={hd} on this device")


def odd_prefix_mask(B, Lk):
    """[B, L_k] bool, True = PAD: valid prefixes of odd length L_k - 2 - 4 * (b % 3) (L_k is odd), so a mask edge splits a key pair"""
    assert Lk % 2 == 1
    valid = torch.tensor([Lk - 2 - 4 * (b % 3) for b in range(B)])
    assert bool((valid % 2 == 1).all()) and bool((valid >= 1).all())
    return torch.arange(Lk)[None, :] >= valid[:, None]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,Lq,Lk,hd,want", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-hd{c[4]}-{c[5].replace(' ', '-')}" for c in CASES])
def test_hash_replay_equals_bit_words(B, H, Lq, Lk, hd, want, p):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib, _ops
    L_ = _lib.lib()
    if B == W:
        B = wide_batch(L_, H, Lq, Lk, hd)
    got = arm(L_, B, H, Lq, Lk, hd)
    assert got == want, f"the backward of (B={B}, H={H}, Lq={Lq}, Lk={Lk}, hd={hd}) is now {got}, not {want}: pick a shape that reaches it"
    assert Lq % 32 != 0 and Lk % 2 == 1
    d = H * hd
    qb, kvb, dob = R.make_inputs(B, H, Lq, Lk, hd, 7 + Lq + Lk + hd)
    kpm = odd_prefix_mask(B, Lk)
    ld1, ld2 = d + 8, 2 * d + 16
    q_g = Guarded(B * Lq, d, torch.bfloat16, ld1, fill=qb.cuda())
    kv_g = Guarded(B * Lk, 2 * d, torch.bfloat16, ld2, fill=kvb.cuda())
    do_g = Guarded(B * Lq, d, torch.bfloat16, ld1, fill=dob.cuda())
    o_g = Guarded(B * Lq, d, torch.bfloat16, ld1)
    lse_g = GuardedFlat(B * H * Lq, torch.float32, GUARD_FLOATS)
    nkt = (Lk + 63) // 64
    assert L_.hriemo_attn_mask_bytes(B, H, Lq, Lk) == B * H * Lq * nkt * 8
    mb_g = Guarded(B * H * Lq, nkt, torch.int64)
    kpm_d = kpm.cuda().view(torch.uint8)
    qd, kd, vd, dod, o = q_g.t, kv_g.t[:, :d], kv_g.t[:, d:], do_g.t, o_g.t
    seed_word = _ops.seed_word(qd.device)
    stream = torch.cuda.current_stream().cuda_stream
    guarded = {"Q": q_g, "K|V": kv_g, "dO": do_g, "O": o_g, "lse": lse_g, "mask bits": mb_g}

    _lib.call("hriemo_attn_fwd", qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(), vd.stride(0),
              o.data_ptr(), o.stride(0), kpm_d.data_ptr(), lse_g.t.data_ptr(), B, H, Lq, Lk, hd, float(p), SEED, seed_word.data_ptr(),
              SITE, BOFF, mb_g.t.data_ptr(), stream)
    torch.cuda.synchronize()
    # bit 16*g + 4*n + r of word (b, h, q, tile) <-> key 64*tile + 16*n + 4*g + r: the forward's words are the host replica's mask
    keep = hashrng.attn_mask(SEED, SITE, B, H, Lq, Lk, p, BOFF)
    w = mb_g.t.view(B, H, Lq, nkt).cpu().numpy().astype(np.uint64)
    key = np.arange(Lk)
    bitpos = ((key % 16) // 4) * 16 + ((key % 64) // 16) * 4 + key % 4
    assert np.array_equal(((w[..., key // 64] >> bitpos.astype(np.uint64)) & np.uint64(1)).astype(bool), keep)

    rq, rk = L_.hriemo_attn_bwd_dq_colsum_rows(B, H, Lq, Lk, hd), L_.hriemo_attn_bwd_kv_colsum_rows(B, H, Lq, Lk, hd)

    def backward(name, bits):
        dq_g = Guarded(B * Lq, d, torch.bfloat16, ld1)
        dkv_g = Guarded(B * Lk, 2 * d, torch.bfloat16, ld2)
        delta_g = GuardedFlat(B * H * Lq, torch.float32, GUARD_FLOATS)
        pq_g, pkv_g = Guarded(rq, d, torch.float32, guard_rows=8), Guarded(rk, 2 * d, torch.float32, guard_rows=8)
        guarded.update({f"dQ ({name})": dq_g, f"dK|dV ({name})": dkv_g, f"delta ({name})": delta_g, f"dQ partials ({name})": pq_g,
                        f"dK|dV partials ({name})": pkv_g})
        dq, dk, dv = dq_g.t, dkv_g.t[:, :d], dkv_g.t[:, d:]
        _lib.call("hriemo_attn_bwd", qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(), vd.stride(0),
                  o.data_ptr(), o.stride(0), dod.data_ptr(), dod.stride(0), dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0),
                  dv.data_ptr(), dv.stride(0), kpm_d.data_ptr(), lse_g.t.data_ptr(), delta_g.t.data_ptr(), B, H, Lq, Lk, hd, float(p), SEED,
                  seed_word.data_ptr(), SITE, BOFF, pq_g.t.data_ptr(), pkv_g.t.data_ptr(), mb_g.t.data_ptr() if bits else None, stream)
        torch.cuda.synchronize()
        return {"dQ": dq, "dK": dk, "dV": dv, "delta": delta_g.t, "dQ partials": pq_g.t, "dK|dV partials": pkv_g.t}

    from_bits, from_hash = backward("bit words", True), backward("hash", False)
    as_bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)      # bits: NaN == NaN
    for name in from_bits:
        if not (name == "delta" and want.startswith("fused")):              # the single pass keeps delta inside the block
            assert not torch.isnan(from_bits[name].float()).any(), name     # every sample has a valid key: all of it is written
        differ = int((as_bits(from_hash[name]) != as_bits(from_bits[name])).sum())
        assert differ == 0, f"{name}: {differ} elements of the hash replay differ from the bit-word backward"
    # the masked keys of every sample, and with them the pad half of the split pair, get exact zeros
    dkv = torch.cat([from_hash["dK"], from_hash["dV"]], 1).view(B, Lk, 2 * d)
    assert float(dkv[kpm.cuda()].abs().max()) == 0.0
    broken = [name for name, g in guarded.items() if not g.intact()]
    assert not broken, f"bytes outside the payload were written: {broken}"
