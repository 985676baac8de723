"""Attention-map export: the padded hriemo_attn_probs (VALU dot products) against the packed hriemo_attn_probs_varlen (MFMA, on
cu_seqlens) and the padded hriemo_attn_probs_mfma (MFMA under the key-padding mask, on the padded operands) on the same data, at the four encoder sites and the decoder site of cfg 2 (d = 768, 8 heads of 96, T_a = 400, T_t = 128,
N_e = 6, B = 64), at valid fraction 0.72 and 1.0; then the eval forward of FusionWithEmotionDecoder at B = 64 with
return_attention=True, padded against packed and against padded with the MFMA maps (set_mfma_maps), and with return_attention=False
as the floor.

Method: HIP events around REPS back-to-back launches (the launches of one arm queue behind each other, so the window is device
time), the three arms alternated inside every round, median over ROUNDS rounds after a warm-up of both; the model forwards one event
pair per forward, arms alternated, median.  The packed map is compared with the padded one on the valid region first, the padded MFMA map on every element.
(profiles/attn_probs_packed.log: the two-arm run; profiles/attn_probs_padded.log: this one.)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H                                   # noqa: E402
from hri_emo_amd import _lib, _ops                        # noqa: E402

B, TA, TT, NE, D, NH = 64, 400, 128, 6, 768, 8
HD = D // NH
REPS, ROUNDS = 20, 7


def lengths(L, frac, gen):
    """B lengths with mean ~ frac * L, the longest = L (so the padded and the packed launch see the same maxima)"""
    if frac >= 1.0:
        return torch.full((B,), L, dtype=torch.long)
    lo = max(1, int(round((2 * frac - 1) * L)))
    n = torch.randint(lo, L + 1, (B,), generator=gen)
    n[0] = L
    return n


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS          # us per launch


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def site(name, Lq, Lk, lq, lk, gen):
    p = lambda t: t.data_ptr()          # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    qw = (torch.randn(B * Lq, 3 * D, generator=gen) * 1.5).bfloat16().cuda()      # Q = a column slice of the [N, 3d] projection
    kw = torch.randn(B * Lk, 2 * D, generator=gen).bfloat16().cuda()              # K | V = the [N, 2d] projection
    q, k, v = qw[:, :D], kw[:, :D], kw[:, D:]
    vq = torch.arange(Lq)[None] < lq[:, None]
    vk = torch.arange(Lk)[None] < lk[:, None]
    kpm = (~vk).cuda().view(torch.uint8)
    _, lse = _ops.attn_fwd(q, k, v, B, NH, Lq, Lk, HD, kpm, 0.0, 0, 0, 0)
    out_pad = torch.empty((B, Lq, Lk), dtype=torch.float32, device="cuda")
    out_mf = torch.empty((B, Lq, Lk), dtype=torch.float32, device="cuda")
    # the packed operands: the valid rows, back to back
    qp = qw.index_select(0, vq.reshape(-1).nonzero().reshape(-1).cuda()).contiguous()
    kp = kw.index_select(0, vk.reshape(-1).nonzero().reshape(-1).cuda()).contiguous()
    cq = torch.zeros(B + 1, dtype=torch.int32)
    ck = torch.zeros(B + 1, dtype=torch.int32)
    cq[1:], ck[1:] = torch.cumsum(lq, 0), torch.cumsum(lk, 0)
    cq, ck = cq.cuda(), ck.cuda()
    mq, mk = int(lq.max()), int(lk.max())
    _, lse_p = _ops.attn_fwd(qp[:, :D], kp[:, :D], kp[:, D:], B, NH, mq, mk, HD, None, 0.0, 0, 0, 0, cu=(cq, ck))
    out_pk = torch.empty((B, Lq, Lk), dtype=torch.float32, device="cuda")
    sw = _ops.seed_word(qw.device)

    def padded():
        _lib.call("hriemo_attn_probs", p(q), 3 * D, p(k), 2 * D, p(kpm), p(lse), p(out_pad), B, NH, Lq, Lk, HD, 0.0, 0, p(sw), 0, 0, st)

    def padded_mfma():
        _lib.call("hriemo_attn_probs_mfma", p(q), 3 * D, p(k), 2 * D, p(kpm), p(lse), p(out_mf), B, NH, Lq, Lk, HD, 0.0, 0, p(sw), 0, 0, st)

    def packed():
        _lib.call("hriemo_attn_probs_varlen", p(qp), 3 * D, p(kp), 2 * D, p(cq), p(ck), p(lse_p), p(out_pk), B, NH, mq, mk, Lq, Lk, HD,
                  0.0, 0, p(sw), 0, 0, st)

    padded(); packed(); padded_mfma()
    torch.cuda.synchronize()
    both = (vq[:, :, None] & vk[:, None, :]).cuda()
    diff = float(((out_pad - out_pk).abs() * both).max())
    diff_mf = float((out_pad - out_mf).abs().max())          # every element: the two padded exports have one contract
    for _ in range(2):
        timed(padded); timed(packed); timed(padded_mfma)
    tp, tk, tm = [], [], []
    for _ in range(ROUNDS):
        tp.append(timed(padded)); tk.append(timed(packed)); tm.append(timed(padded_mfma))
    a, b, c = median(tp), median(tk), median(tm)
    flop = 2.0 * NH * HD * float((lq * lk).sum())          # QK^T on the valid (query, key) pairs
    byts = 4.0 * B * Lq * Lk                               # the map, the only large stream
    print(f"{name:10s} {Lq:4d} x {Lk:4d}  padded VALU {a:9.1f} us [{min(tp):.1f} .. {max(tp):.1f}]   packed MFMA {b:8.1f} us [{min(tk):.1f} .. {max(tk):.1f}]"
          f"   {a / b:6.2f} x   packed: {flop / b / 1e6:7.1f} TFLOP/s on valid pairs, map {byts / b / 1e3:7.1f} GB/s   max |padded - packed| on valid {diff:.1e}",
          flush=True)
    spread = max((max(t) - min(t)) / median(t) for t in (tp, tm))
    print(f"{'':10s} {'':11s}  padded MFMA {c:9.1f} us [{min(tm):.1f} .. {max(tm):.1f}]   {a / c:6.2f} x the padded VALU export, map {byts / c / 1e3:7.1f} GB/s"
          f"   round-to-round spread (max - min) / median {100 * spread:.1f} %   max |VALU - MFMA| on every element {diff_mf:.1e}", flush=True)
    return a, b, c


def forwards(frac, gen):
    m = H.FusionWithEmotionDecoder(d_model=D, num_emotions=NE, n_heads=NH, dropout=0.1).cuda().eval()
    la, lt = lengths(TA, frac, gen), lengths(TT, frac, gen)
    h_a, h_t = torch.randn(B, TA, D, generator=gen).cuda(), torch.randn(B, TT, D, generator=gen).cuda()
    m_a, m_t = (torch.arange(TA)[None] >= la[:, None]).cuda(), (torch.arange(TT)[None] >= lt[:, None]).cuda()
    arms = {"padded, maps": (False, False, True, False), "padded, MFMA maps": (False, False, True, True), "packed, maps": (True, True, True, False),
            "padded, no maps": (False, False, False, False), "packed, no maps": (True, True, False, False)}

    def run(arm):
        varlen, tail, need, mfma = arms[arm]
        H.set_varlen(varlen)
        H.set_varlen_maps(varlen)
        H.set_mfma_maps(mfma)
        _ops.PACKED_TAIL = tail
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            e0.record()
            m(h_a, h_t, m_a, m_t, return_attention=need)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):
        for arm in arms:
            run(arm)
    ts = {arm: [] for arm in arms}
    for _ in range(11):
        for arm in arms:
            ts[arm].append(run(arm))
    for arm in arms:
        print(f"eval forward B={B}, valid fraction {frac:.2f}, {arm:17s}: {median(ts[arm]):7.3f} ms [{min(ts[arm]):.3f} .. {max(ts[arm]):.3f}]", flush=True)
    H.set_varlen(False); H.set_varlen_maps(False); H.set_mfma_maps(False); _ops.PACKED_TAIL = False


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    print(f"# {torch.cuda.get_device_name(0)}; us per launch, median of {ROUNDS} rounds of {REPS} launches [min .. max]", flush=True)
    slower, slower_mf = [], []
    for frac in (0.72, 1.0):
        gen = torch.Generator().manual_seed(7)
        la, lt = lengths(TA, frac, gen), lengths(TT, frac, gen)
        lf = torch.minimum(la, lt)
        ne = torch.full((B,), NE, dtype=torch.long)
        print(f"## valid fraction {frac:.2f}: audio {float(la.float().mean()) / TA:.3f}, text {float(lt.float().mean()) / TT:.3f}")
        for name, Lq, Lk, lq, lk in (("audio_self", TA, TA, la, la), ("text_self", TT, TT, lt, lt), ("a2t", TA, TT, la, lt),
                                     ("t2a", TT, TA, lt, la), ("decoder", NE, TT, ne, lf)):
            a, b, c = site(name, Lq, Lk, lq, lk, gen)
            if not b < a:
                slower.append((frac, name))
            if not c < a:
                slower_mf.append((frac, name, round(c, 1), round(a, 1)))
    print("packed MFMA export faster than the padded export at every site" if not slower else f"packed export NOT faster at: {slower}")
    print("padded MFMA export faster than the padded VALU export at every site" if not slower_mf
          else f"padded MFMA export NOT faster at (valid fraction, site, us, VALU us): {slower_mf}")
    for frac in (0.72, 1.0):
        forwards(frac, torch.Generator().manual_seed(11))


if __name__ == "__main__":
    main()
