"""GPU suite, attention on packed (varlen) rows: every kernel form hriemo_attn_fwd_varlen / hriemo_attn_bwd_varlen can launch, against
the float64 reference of every sample on its own lq[b] x lk[b] block (attn_reference.make_packed / check_packed: limits from the
reference alone), at per-sample lengths that sit on the tile edges, inside guarded buffers -- the standard
test_gpu_attention_variants.py sets for the padded entries.

On packed rows the row after a sequence's last row is the NEXT SAMPLE'S data, the key-padding mask is gone (bounds are the only
protection) and the kernel form follows the launch maxima while every block sees its own sample's lengths.  So, per row of the table:
  * both forms are asserted THROUGH THE ABI at the maxima (hriemo_attn_plan; "update the table" on a change of the heuristics; rows
    with B = W take the first batch size with the 128-row tile on this device, finding none is a failure; nothing skips);
  * O, dQ, dK, dV of every sample meet attn_reference.check, lse its 2e-3 bound, the mask words the host replica of the hash;
  * bit words == hash replay and the run with column-sum partials == the run without, bit for bit; every partial row is written, rows of
    tiles that hold no row of their sample are +0, the sums meet the reference under the padded test's three bounds;
  * the same data through the PADDED entries (prefix key_padding_mask, dO zero on PAD query rows) gives the same bits on the valid rows;
  * isolation: with the rows of every OTHER sample overwritten by NaN, the middle sample's results (and partial rows) keep their bits;
  * the all-zero filler sequence of a `bucket` row comes out exactly zero; every guard byte and the 8 surplus rows behind
    cu_seqlens[B] of every packed buffer keep their sentinel.

Layout of the side buffers (localize() in attention.hip), with bh = b * H + h and nkt(L) = ceil(L / 64):
  lse, delta     padded slots: element (b, h, q) at bh * max_lq + q
  mask words     a padded slot of max_lq * nkt(max_lk) words per (b, h), COMPACT inside it with the sample's own key-tile count:
                 word (b, h, q, kt) at bh * max_lq * nkt(max_lk) + q * nkt(lk[b]) + kt; bit 16*g + 4*n + r <-> key 64*kt + 16*n + 4*g + r
  partials       two-kernel form: row b * tiles(max) + tile on either side; single-pass forms: row b"""
import numpy as np
import pytest
import torch

import attn_reference as R
from attn_gpu import GUARD_FLOATS, W, Guarded, GuardedFlat, backward_form, forward_form, plan, wide_batch

pytestmark = pytest.mark.gpu

SEED, SITE, BOFF = 1234567890123, 40, 5
SEED0 = 100             # data seed of a row: SEED0 + max_lq + max_lk, stepped by R.make_packed_decidable where the references demand it
SURPLUS = 8             # rows of every packed buffer past cu_seqlens[B]: no sequence owns them, nothing may touch them
N64, N1, W128 = "n64", "1w", "w128"
two = lambda dq, dkv: f"two-kernel(dq={dq},dkv={dkv})"      # noqa: E731

# B: real samples (None: the pattern's minimum; W: from the scan, a `bucket` row's filler included in the scanned size)
VARIANTS = [  # B, H, max_lq, max_lk, hd, length pattern, p, forward form, backward form
    # key-resident single pass, 16 < max_lk <= 64 (blocks also meet samples of <= 16 keys)
    (None, 2, 70, 64, 32, "edges", 0.1, "fwd<4,2>", "fused-KW1"),
    (4, 2, 33, 17, 64, "bucket", 0.1, "fwd<4,1>", "fused-KW1"),            # the smallest shape that takes it
    (None, 2, 70, 64, 96, "edges", 0.0, "fwd<4,2>", "fused-KW1"),
    (4, 2, 40, 33, 128, "bucket", 0.1, "fwd<4,1>", "fused-KW1"),
    # key-resident single pass, 64 < max_lk <= 128 (two sub-tiles per wave; samples of <= 16 and <= 64 keys in it)
    (None, 2, 130, 128, 64, "edges", 0.1, "fwd<4,1>", "fused-KW2"),
    (4, 2, 100, 65, 96, "bucket", 0.1, "fwd<4,2>", "fused-KW2"),
    (None, 2, 200, 128, 128, "edges", 0.0, "fwd<4,2>", "fused-KW2"),
    (4, 4, 70, 100, 32, "bucket", 0.1, "fwd<4,2>", "fused-KW2"),
    (3, 2, 100, 65, 32, "ones", 0.1, "fwd<4,2>", "fused-KW2"),
    (2, 4, 400, 128, 96, "bucket", 0.1, "fwd<4,1>", "fused-KW2"),          # a2t at the headline lengths, two utterances + filler
    # query-resident single pass: 16 < max_lq <= 128 < max_lk (samples of <= 16 queries or <= 128 keys in it) ...
    (None, 2, 128, 129, 64, "edges", 0.1, "fwd<4,2>", "qres"),
    (4, 2, 17, 200, 32, "bucket", 0.1, "fwd<4,1>", "qres"),
    (None, 2, 100, 300, 128, "edges", 0.0, "fwd<4,2>", "qres"),
    (1, 2, 64, 200, 96, "single", 0.1, "fwd<4,1>", "qres"),
    # ... and its branch 16 < max_lq <= 128, max_lk <= 16
    (None, 2, 100, 16, 32, "edges", 0.1, "fwd<4,2>", "qres"),
    (4, 2, 100, 16, 96, "bucket", 0.1, "fwd<4,2>", "qres"),
    # two-kernel backward, 64-row tiles: blocks whose whole tile lies past their sample's end on either side
    (None, 2, 130, 130, 32, "edges", 0.1, "fwd<4,2>", two(N64, N64)),
    (4, 4, 70, 70, 16, "bucket", 0.1, "fwd<4,2>", two(N64, N64)),
    (None, 2, 33, 100, 16, "edges", 0.0, "fwd<4,1>", two(N64, N64)),
    (4, 2, 129, 129, 128, "bucket", 0.1, "fwd<4,2>", two(N64, N64)),
    (4, 2, 130, 150, 64, "bucket", 0.0, "fwd<4,2>", two(N64, N64)),
    (2, 4, 400, 400, 96, "bucket", 0.1, "fwd<4,2>", two(N64, N64)),        # self-audio at the headline lengths
    # two-kernel backward, one-wave forms (max <= 16 on a side)
    (None, 2, 200, 16, 32, "edges", 0.1, "fwd<4,2>", two(N64, N1)),
    (4, 2, 200, 16, 64, "bucket", 0.0, "fwd<4,2>", two(N64, N1)),
    (None, 2, 33, 16, 16, "edges", 0.1, "fwd<4,1>", two(N64, N1)),
    (None, 2, 6, 200, 96, "edges", 0.1, "fwd<1,1>", two(N1, N64)),         # decoder queries over a long memory
    (4, 2, 6, 200, 16, "bucket", 0.0, "fwd<1,1>", two(N1, N64)),
    (None, 2, 16, 16, 32, "edges", 0.1, "fwd<1,1>", two(N1, N1)),
    (4, 2, 6, 6, 16, "bucket", 0.1, "fwd<1,1>", two(N1, N1)),
    (None, 2, 12, 16, 128, "edges", 0.0, "fwd<1,1>", two(N1, N1)),
    (4, 4, 16, 12, 64, "bucket", 0.1, "fwd<1,1>", two(N1, N1)),
    # two-kernel backward, 128-row tiles (B from the scan)
    (W, 8, 200, 200, 16, "edges", 0.1, "fwd<4,2>", two(W128, W128)),
    (W, 8, 200, 200, 64, "bucket", 0.1, "fwd<4,2>", two(W128, W128)),
    (W, 8, 200, 200, 96, "edges", 0.0, "fwd<4,2>", two(W128, W128)),
    (W, 8, 256, 192, 32, "edges", 0.1, "fwd<4,2>", two(W128, N64)),
    (W, 8, 192, 256, 32, "bucket", 0.0, "fwd<4,2>", two(N64, W128)),
]


def data_seed(Lq, Lk):
    return SEED0 + Lq + Lk


def resolve(L_, B, H, Lq, Lk, hd, pattern, bwd, cus=0):
    """-> (lq, lk, filler) of a table row (cus = 0: the batch size of a B = W row is scanned on this device)"""
    if B == W:
        total = wide_batch(L_, H, Lq, Lk, hd, bwd, lo=len(R.packed_lengths(pattern, Lq, Lk)[0]), cus=cus)
        B = total - (1 if pattern == "bucket" else 0)
    return R.packed_lengths(pattern, Lq, Lk, B)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _ops
    return _ops


def _ids():
    return [f"{B}x{H}x{Lq}x{Lk}-hd{hd}-{pat}-p{p}-{bwd}" for B, H, Lq, Lk, hd, pat, p, _, bwd in VARIANTS]


def _bits(t):
    """a tensor's bytes, so that NaN == NaN and -0 != +0"""
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("B,H,Lq,Lk,hd,pattern,p,fwd,bwd", VARIANTS, ids=_ids())
def test_attention_variant_packed(ops, B, H, Lq, Lk, hd, pattern, p, fwd, bwd):
    from hri_emo_amd import _lib
    L_ = _lib.lib()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lq, lk, filler = resolve(L_, B, H, Lq, Lk, hd, pattern, bwd)
    B = len(lq)                                                        # the launch's batch size: the filler is its last sample
    got_form = backward_form(L_, B, H, Lq, Lk, hd)
    assert got_form == bwd, (f"the backward of (B={B}, H={H}, Lq={Lq}, Lk={Lk}, hd={hd}) is now {got_form}, the variant table "
                             f"says {bwd}: update the table so that every kernel form stays covered")
    assert forward_form(L_, B, H, Lq, Lk, hd) == fwd, (forward_form(L_, B, H, Lq, Lk, hd), fwd)
    assert max(lq) <= Lq and max(lk) <= Lk and min(lq) >= 1 and min(lk) >= 1
    assert pattern != "bucket" or (max(lq) < Lq and max(lk) < Lk)      # no sequence reaches the launch maxima
    _, form, dq_rows, dkv_rows, rq, rk = plan(L_, B, H, Lq, Lk, hd)
    d = H * hd
    c, seed_index = R.make_packed_decidable(lq, lk, filler, H, hd, data_seed(Lq, Lk), p, (SEED, SITE, BOFF))
    nq, nk = c.cu_q[-1], c.cu_k[-1]
    nkt = (Lk + 63) // 64
    ld1, ld2 = d + 8, 2 * d + 16
    seed_word = torch.zeros(1, dtype=torch.int64, device="cuda")          # the device word added to SEED: zero, the host replica hashes SEED
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()            # noqa: E731
    cu_q = torch.tensor(c.cu_q, dtype=torch.int32).cuda()
    cu_k = torch.tensor(c.cu_k, dtype=torch.int32).cuda()
    assert cu_q.data_ptr() != cu_k.data_ptr()
    guarded, surplus = {}, {}

    def row_buffer(name, n, cols, ld, fill=None):
        """n packed rows + SURPLUS rows that stay sentinel (NaN when read), inside guard rows, ld > cols"""
        g = Guarded(n + SURPLUS, cols, torch.bfloat16, ld)
        if fill is not None:
            g.t[:n].copy_(fill.cuda())
        guarded[name], surplus[name] = g, (g, n)
        return g

    class Run:
        """the buffers of one forward + backward over packed inputs (q, kv, do: bf16 on the host)"""

        def __init__(self, tag, q, kv, do):
            self.tag = tag
            self.q_g, self.kv_g, self.do_g = (row_buffer(f"Q ({tag})", nq, d, ld1, q), row_buffer(f"K|V ({tag})", nk, 2 * d, ld2, kv),
                                              row_buffer(f"dO ({tag})", nq, d, ld1, do))
            self.o_g = row_buffer(f"O ({tag})", nq, d, ld1)
            self.lse_g = guarded[f"lse ({tag})"] = GuardedFlat(B * H * Lq, torch.float32, GUARD_FLOATS)
            self.mb_g = None
            if p > 0:
                assert L_.hriemo_attn_mask_bytes(B, H, Lq, Lk) == B * H * Lq * nkt * 8
                self.mb_g = guarded[f"mask bits ({tag})"] = Guarded(B * H * Lq, nkt, torch.int64)

        def forward(self):
            qd, kd, vd, o = self.q_g.t, self.kv_g.t[:, :d], self.kv_g.t[:, d:], self.o_g.t
            _lib.call("hriemo_attn_fwd_varlen", qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(), vd.stride(0),
                      o.data_ptr(), o.stride(0), cu_q.data_ptr(), cu_k.data_ptr(), self.lse_g.t.data_ptr(), B, H, Lq, Lk, hd, float(p),
                      SEED, seed_word.data_ptr(), SITE, BOFF, ptr(None if self.mb_g is None else self.mb_g.t), stream)
            torch.cuda.synchronize()
            return o[:nq], self.lse_g.t.view(B, H, Lq)

        def backward(self, name, bits, partials):
            """-> dQ [nq, d], dK|dV [nk, 2d], dQ partials, dK|dV partials (Guarded or None)"""
            tag = f"{self.tag}, {name}"
            dq_g, dkv_g = row_buffer(f"dQ ({tag})", nq, d, ld1), row_buffer(f"dK|dV ({tag})", nk, 2 * d, ld2)
            delta_g = guarded[f"delta ({tag})"] = GuardedFlat(B * H * Lq, torch.float32, GUARD_FLOATS)
            pq_g = pkv_g = None
            if partials:
                assert (rq, rk) == (L_.hriemo_attn_bwd_dq_colsum_rows(B, H, Lq, Lk, hd), L_.hriemo_attn_bwd_kv_colsum_rows(B, H, Lq, Lk, hd))
                pq_g, pkv_g = Guarded(rq, d, torch.float32, guard_rows=8), Guarded(rk, 2 * d, torch.float32, guard_rows=8)
                guarded.update({f"dQ partials ({tag})": pq_g, f"dK|dV partials ({tag})": pkv_g})
            qd, kd, vd, o, dod = self.q_g.t, self.kv_g.t[:, :d], self.kv_g.t[:, d:], self.o_g.t, self.do_g.t
            dq, dk, dv = dq_g.t, dkv_g.t[:, :d], dkv_g.t[:, d:]
            _lib.call("hriemo_attn_bwd_varlen", qd.data_ptr(), qd.stride(0), kd.data_ptr(), kd.stride(0), vd.data_ptr(), vd.stride(0),
                      o.data_ptr(), o.stride(0), dod.data_ptr(), dod.stride(0), dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0),
                      dv.data_ptr(), dv.stride(0), cu_q.data_ptr(), cu_k.data_ptr(), self.lse_g.t.data_ptr(), delta_g.t.data_ptr(), B, H,
                      Lq, Lk, hd, float(p), SEED, seed_word.data_ptr(), SITE, BOFF, ptr(None if pq_g is None else pq_g.t),
                      ptr(None if pkv_g is None else pkv_g.t), ptr(self.mb_g.t if bits else None), stream)
            torch.cuda.synchronize()
            return dq[:nq], dkv_g.t[:nk], pq_g, pkv_g

    # ---- forward: O and lse of every sample, the mask words
    run = Run("packed", c.qb, c.kvb, c.dob)
    o, lse = run.forward()
    worst = {"O": R.check_packed(o.float().cpu(), c, "O", "q")}
    lse_h = lse.cpu().double()
    for b in range(B):
        ref_lse = c.ref[b]["lse"][0]
        assert (lse_h[b, :, :lq[b]] - ref_lse).abs().max() <= 2e-3 * max(1.0, ref_lse.abs().max().item()), ("lse", b)
    if p > 0:
        words = run.mb_g.t.reshape(B * H, Lq * nkt).cpu().numpy().astype(np.uint64)
        for b in range(B):
            nkt_b = (lk[b] + 63) // 64
            w = words[b * H:(b + 1) * H, :lq[b] * nkt_b].reshape(H, lq[b], nkt_b)     # compact inside the padded slot
            key = np.arange(lk[b])
            bitpos = ((key % 16) // 4) * 16 + ((key % 64) // 16) * 4 + key % 4
            got_keep = ((w[..., key // 64] >> bitpos.astype(np.uint64)) & np.uint64(1)).astype(bool)
            assert np.array_equal(got_keep, c.keep[b][0].numpy()), ("mask words", b)

    # ---- backward: bit words (or no dropout), the hash replay, the column-sum partials
    dq, dkv, _, _ = run.backward("bit words" if p > 0 else "no dropout", p > 0, False)
    dq_h, dkv_h = dq.float().cpu(), dkv.float().cpu()
    worst["dQ"] = R.check_packed(dq_h, c, "dQ", "q")
    worst["dK"] = R.check_packed(dkv_h[:, :d], c, "dK", "k")
    worst["dV"] = R.check_packed(dkv_h[:, d:], c, "dV", "k")
    if p > 0:
        dq_r, dkv_r, _, _ = run.backward("hash", False, False)
        assert _same(dq_r, dq) and _same(dkv_r, dkv), "the hash replay and the bit words give other gradients"
    dq2, dkv2, pq_g, pkv_g = run.backward("partials", p > 0, True)
    assert _same(dq2, dq) and _same(dkv2, dkv), "the column-sum partials change the gradients"
    tq, tk = (-(-Lq // dq_rows), -(-Lk // dkv_rows)) if form == 0 else (1, 1)
    assert (rq, rk) == (B * tq, B * tk)
    part_rows = lambda b: (slice(b * tq, (b + 1) * tq), slice(b * tk, (b + 1) * tk))       # noqa: E731
    dq_ref = c.packed_ref("dQ").float().sum(0)
    dkv_ref = torch.cat([c.packed_ref("dK"), c.packed_ref("dV")], 1).float().sum(0)
    for name, part, full, r in (("dq", pq_g.t, dq, dq_ref), ("dkv", pkv_g.t, dkv, dkv_ref)):
        assert not torch.isnan(part).any(), (name, "a partial row was not written")
        got = part.sum(0).cpu()
        stored = full.float().sum(0).cpu()
        scale = max(1.0, r.abs().max().item())
        assert (got - r).abs().max() <= 2e-2 * scale, (name, (got - r).abs().max(), scale)
        assert (got - stored).abs().max() <= 1e-2 * scale, (name, "vs stored tiles", (got - stored).abs().max())
        assert (got - r).norm() <= 1.05 * (stored - r).norm() + 1e-6 * scale, (name, (got - r).norm(), (stored - r).norm())
    if form == 0:       # tiles that hold no row of their sample: exactly +0
        for b in range(B):
            for t in range(tq):
                if t * dq_rows >= lq[b]:
                    assert not _bits(pq_g.t[b * tq + t]).any(), ("dQ partials of an empty tile", b, t)
            for t in range(tk):
                if t * dkv_rows >= lk[b]:
                    assert not _bits(pkv_g.t[b * tk + t]).any(), ("dK|dV partials of an empty tile", b, t)
    if filler:
        fq, fk = c.rows_q(B - 1), c.rows_k(B - 1)
        for name, t in (("O", o[fq]), ("dQ", dq[fq]), ("dK|dV", dkv[fk])):
            assert float(t.float().abs().max()) == 0.0, (name, "of the all-zero filler sequence")

    # ---- equals padded: the same data through hriemo_attn_fwd / hriemo_attn_bwd with a prefix key_padding_mask
    g = torch.Generator().manual_seed(7)
    q_p, kv_p = (torch.randn(B * Lq, d, generator=g) * 1.5).bfloat16(), torch.randn(B * Lk, 2 * d, generator=g).bfloat16()
    do_p = torch.zeros(B * Lq, d, dtype=torch.bfloat16)                                  # PAD query rows carry no gradient
    iq = torch.cat([b * Lq + torch.arange(lq[b]) for b in range(B)])
    ik = torch.cat([b * Lk + torch.arange(lk[b]) for b in range(B)])
    q_p[iq], kv_p[ik], do_p[iq] = c.qb, c.kvb, c.dob
    q_p, kv_p, do_p, iq, ik = q_p.cuda(), kv_p.cuda(), do_p.cuda(), iq.cuda(), ik.cuda()
    kpm = (torch.arange(Lk)[None] >= torch.tensor(lk)[:, None]).cuda().view(torch.uint8)
    o_p, dq_p, dkv_p = torch.empty_like(q_p), torch.empty_like(q_p), torch.empty_like(kv_p)
    lse_p, delta_p = torch.empty(B, H, Lq, device="cuda"), torch.empty(B, H, Lq, device="cuda")
    mb_p = torch.empty(B * H * Lq * nkt, dtype=torch.int64, device="cuda") if p > 0 else None
    kp, vp, dkp, dvp = kv_p[:, :d], kv_p[:, d:], dkv_p[:, :d], dkv_p[:, d:]
    _lib.call("hriemo_attn_fwd", q_p.data_ptr(), q_p.stride(0), kp.data_ptr(), kp.stride(0), vp.data_ptr(), vp.stride(0), o_p.data_ptr(),
              o_p.stride(0), kpm.data_ptr(), lse_p.data_ptr(), B, H, Lq, Lk, hd, float(p), SEED, seed_word.data_ptr(), SITE, BOFF, ptr(mb_p),
              stream)
    _lib.call("hriemo_attn_bwd", q_p.data_ptr(), q_p.stride(0), kp.data_ptr(), kp.stride(0), vp.data_ptr(), vp.stride(0), o_p.data_ptr(),
              o_p.stride(0), do_p.data_ptr(), do_p.stride(0), dq_p.data_ptr(), dq_p.stride(0), dkp.data_ptr(), dkp.stride(0), dvp.data_ptr(),
              dvp.stride(0), kpm.data_ptr(), lse_p.data_ptr(), delta_p.data_ptr(), B, H, Lq, Lk, hd, float(p), SEED, seed_word.data_ptr(),
              SITE, BOFF, None, None, ptr(mb_p), stream)
    torch.cuda.synchronize()
    assert _same(o_p[iq], o), "O: packed != padded"
    vq = (torch.arange(Lq)[None] < torch.tensor(lq)[:, None])[:, None, :].expand(B, H, Lq).cuda()
    assert _same(lse_p[vq], lse[vq]), "lse: packed != padded"
    assert _same(dq_p[iq], dq), "dQ: packed != padded"
    assert _same(dkv_p[ik], dkv), "dK|dV: packed != padded"

    # ---- isolation: every other sample's rows are NaN, the middle sample keeps its bits
    real = B - 1 if filler else B
    if real > 1:
        bs = real // 2
        sq, sk = c.rows_q(bs), c.rows_k(bs)
        nan = lambda x, sl: torch.full_like(x, float("nan")).index_copy_(0, torch.arange(sl.start, sl.stop), x[sl])   # noqa: E731
        lone = Run("isolated", nan(c.qb, sq), nan(c.kvb, sk), nan(c.dob, sq))
        o_i, lse_i = lone.forward()
        dq_i, dkv_i, pq_i, pkv_i = lone.backward("partials", p > 0, True)
        pq_s, pk_s = part_rows(bs)
        for name, a, b_ in (("O", o_i[sq], o[sq]), ("lse", lse_i[bs, :, :lq[bs]], lse[bs, :, :lq[bs]]), ("dQ", dq_i[sq], dq[sq]),
                            ("dK|dV", dkv_i[sk], dkv[sk]), ("dQ partials", pq_i.t[pq_s], pq_g.t[pq_s]),
                            ("dK|dV partials", pkv_i.t[pk_s], pkv_g.t[pk_s])):
            assert _same(a, b_), f"{name} of sample {bs} (lq {lq[bs]}, lk {lk[bs]}) depends on another sample's rows"

    broken = [name for name, g_ in guarded.items() if not g_.intact()]
    assert not broken, f"bytes outside the payload were written: {broken}"
    touched = [name for name, (g_, n) in surplus.items() if not bool((_bits(g_.t[n:]) == 0xFF).all())]
    assert not touched, f"surplus rows behind cu_seqlens[B] were written: {touched}"
    print(f"\n  [attn-variant-packed] B={B}{' (filler included)' if filler else ''} H={H} max_lq={Lq} max_lk={Lk} hd={hd} lengths={pattern} "
          f"p={p} data seed #{seed_index}: {fwd}, {got_form} (asserted through the ABI); error / limit (elementwise, per tile): "
          + ", ".join(f"{n} {e:.3f} {t:.3f}" for n, (e, t) in worst.items()))
