"""A/B of the two front doors of the captured packed step, in ONE process, rounds interleaved: cfg 2 (B = 64, T_a = 400, T_t = 128,
d = 768), bf16 inputs, dropout 0.1, varlen + packed tail, valid fraction ~0.72 and 1.0.

Both arms include the host -> device hand-over through data.DevicePrefetcher from pinned host batches:
  A  the mask-fed path: collate_seq_batch(pad_to=...) batches, DataParallelStep.step(..., lengths=), INGEST_ROWS on
  B  the ragged path:   collate_seq_packed batches, DevicePrefetcher(ragged=...), DataParallelStep.step_packed
Wall clock over `steps` steps per round behind a synchronize, median of `rounds` rounds per arm, arm A's round-to-round spread
(max - min) / median.  A third figure with the inputs resident (the static buffers fed to themselves: no row copies): replays
only, timed by device events -- the table kernel + one [2, B] copy against three host-built cu_seqlens uploads.  Bytes per batch
are the algorithm's, from the shapes.  Every bucket graph the loader needs is captured before the first timed round.

usage: python scripts_dev/bench_step_packed.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _ops, data  # noqa: E402
from hri_emo_amd.dp import DataParallelStep  # noqa: E402
from hri_emo_amd.train import fusion_step_loss  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, TA, TT, D, NE, NBATCH = 64, 400, 128, 768, 6, 4
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)


def samples(valid, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        la = TA if valid == 1.0 else int(torch.randint(int(0.44 * TA), TA + 1, (1,), generator=g))
        lt = TT if valid == 1.0 else int(torch.randint(int(0.44 * TT), TT + 1, (1,), generator=g))
        out.append((torch.randn(la, D, generator=g), torch.zeros(la, dtype=torch.bool), torch.randn(lt, D, generator=g),
                    torch.zeros(lt, dtype=torch.bool), (torch.rand(NE, generator=g) < 0.3).float()))
    return out


def pin(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).contiguous().pin_memory()


def loaders(valid):
    """NBATCH distinct batches in both forms, bf16 features, pinned (what a DataLoader with pin_memory=True hands over)"""
    pad, rag = [], []
    for i in range(NBATCH):
        s = samples(valid, 100 + i)
        h_a, m_a, h_t, m_t, y = data.collate_seq_batch(s, pad_to=(TA, TT))
        pad.append((pin(h_a, torch.bfloat16), pin(m_a), pin(h_t, torch.bfloat16), pin(m_t), pin(y)))
        r_a, l_a, r_t, l_t, y = data.collate_seq_packed(s)
        rag.append((pin(r_a, torch.bfloat16), l_a, pin(r_t, torch.bfloat16), l_t, pin(y)))
    return pad, rag


def model_and_step():
    torch.manual_seed(1234)
    dp = DataParallelStep(H.FusionWithEmotionDecoder(**CFG).to(dev).train(), fusion_step_loss, overlap=False)
    dp.set_global_batch(B)
    return dp


def run(valid):
    pad, rag = loaders(valid)
    n_a, n_t = [int(b[1].sum()) for b in rag], [int(b[3].sum()) for b in rag]
    frac = (sum(n_a) / TA + sum(n_t) / TT) / (2 * B * NBATCH)
    bytes_a = B * (TA + TT) * D * 2 + B * (TA + TT) + B * NE * 4
    bytes_b = (sum(n_a) + sum(n_t)) / NBATCH * D * 2 + 2 * B * 4 + B * NE * 4
    feed_a = lambda items: data.DevicePrefetcher(items, dev, convert=lambda t: (t[0], t[2], t[1], t[3], t[4]), mask_slots=(2, 3))   # noqa: E731
    feed_b = lambda items: data.DevicePrefetcher(items, dev, convert=lambda t: (t[0], t[1].tolist(), t[2], t[3].tolist(), t[4]),   # noqa: E731
                                                 ragged={0: B * TA, 2: B * TT})
    dp_a, dp_b = model_and_step(), model_and_step()
    # capture + every bucket graph the loader needs, outside the timed rounds
    for i, (h_a, h_t, m_a, m_t, y, lens) in enumerate(feed_a(pad)):
        if i == 0:
            dp_a.capture(h_a, h_t, m_a, m_t, y, lengths=lens)
        dp_a.step(h_a, h_t, m_a, m_t, y, lengths=lens)
    for i, (r_a, l_a, r_t, l_t, y) in enumerate(feed_b(rag)):
        if i == 0:
            dp_b.capture_packed(r_a, r_t, l_a, l_t, y, pad_to=(TA, TT))
        dp_b.step_packed(r_a, r_t, l_a, l_t, y)
    torch.cuda.synchronize()
    graphs = (len(dp_a._pb.graphs), len(dp_b._pb.graphs))
    items_a, items_b = [pad[i % NBATCH] for i in range(STEPS)], [rag[i % NBATCH] for i in range(STEPS)]

    def wall_a():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for h_a, h_t, m_a, m_t, y, lens in feed_a(items_a):
            dp_a.step(h_a, h_t, m_a, m_t, y, lengths=lens)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3

    def wall_b():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r_a, l_a, r_t, l_t, y in feed_b(items_b):
            dp_b.step_packed(r_a, r_t, l_a, l_t, y)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    # inputs resident: the static buffers fed to themselves (the last loader batch is in them): no row copies
    la_list, lt_list = rag[-1][1].tolist(), rag[-1][3].tolist()
    sa, sb = dp_a._static, dp_b._static
    res_a = lambda: dp_a.step(*sa, lengths=(la_list, lt_list))                                               # noqa: E731
    res_b = lambda: dp_b.step_packed(sb[0][:sum(la_list)], sb[1][:sum(lt_list)], la_list, lt_list, sb[4])     # noqa: E731
    wall_a(), wall_b(), events(res_a), events(res_b)                                                          # warm-up
    t = {"A": [], "B": [], "A resident": [], "B resident": []}
    for r in range(ROUNDS):
        t["A"].append(wall_a())
        t["B"].append(wall_b())
        t["A resident"].append(events(res_a))
        t["B resident"].append(events(res_b))
        print(f"valid {valid}: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + " ms/step", flush=True)
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    print(f"cfg2 B={B} bf16 inputs, dropout 0.1, valid fraction {frac:.3f}, {NBATCH} distinct batches, bucket graphs A {graphs[0]} / B {graphs[1]}; "
          f"host -> device bytes per batch A {bytes_a / 1e6:.1f} MB, B {bytes_b / 1e6:.1f} MB (B / A = {bytes_b / bytes_a:.3f})")
    print(f"  with hand-over (wall clock, {STEPS} steps per round, median of {ROUNDS}): A {med['A']:.3f} ms (spread {spread['A']:.4f}), "
          f"B {med['B']:.3f} ms (spread {spread['B']:.4f}); B - A = {med['B'] - med['A']:+.3f} ms, A's spread = {spread['A'] * med['A']:.3f} ms")
    print(f"  inputs resident (device events): A {med['A resident']:.3f} ms (spread {spread['A resident']:.4f}), "
          f"B {med['B resident']:.3f} ms (spread {spread['B resident']:.4f}); B - A = {med['B resident'] - med['A resident']:+.3f} ms", flush=True)
    dp_a.release_graph()
    dp_b.release_graph()


H.set_varlen(True)
H.set_ingest(True)
_ops.PACKED_TAIL = True
print(f"bench_step_packed: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, steps per round {STEPS}")
for v in (0.72, 1.0):
    run(v)
