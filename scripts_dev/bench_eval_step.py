"""A/B of the two forms of train.evaluate_packed, in ONE process, rounds interleaved: cfg 2 (T_a = 400, T_t = 128, d = 768) at
B = 64 and at B = 8 (the default batch of the reference's scripts/infer/mosei_eval_infer.py), bf16 inputs, valid fraction ~0.72.

  E  eager:    evaluate_packed(model, batches, loss_fn, stats)              -- ~150 launches per batch issued from Python
  C  captured: evaluate_packed(model, batches, loss_fn, stats, step=es)     -- dp.EvalStep: copies into the static buffers + one replay

Both arms include the host -> device hand-over through data.DevicePrefetcher(ragged=...) from pinned host batches and feed an
EpochStats (reset per round; result(), the epoch's one read-back, is the same in both arms and stays outside).  An "epoch" is
`steps` batches; it is timed by a pair of device events around it AND by the wall clock behind a synchronize; medians of `rounds`
rounds per arm, every arm's round-to-round spread (max - min) / median.  Every bucket graph the loader needs is captured before the
first timed round.

Separately: the device time of the weight re-cast inside one eval replay.  The cast launches of the capture pass (fp32 masters ->
bf16 shadows: hriemo_cast_f32_to_bf16, _batch, hriemo_cast_copy_batch) are recorded with their arguments, captured into a graph of
their own and replayed alone, timed by device events -- back to back on one stream, so an upper bound of what they cost inside
the step, where some of them run on the side stream beside the first fusion layer.  Beside it: one eval replay with the inputs
resident.

usage: python scripts_dev/bench_eval_step.py [rounds] [steps]"""
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops, data  # noqa: E402
from hri_emo_amd.train import EpochStats, evaluate_packed, fusion_step_loss  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 64
TA, TT, D, NE, NBATCH = 400, 128, 768, 6, 4
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)
CASTS = {"hriemo_cast_f32_to_bf16": 0, "hriemo_cast_f32_to_bf16_batch": 3, "hriemo_cast_copy_batch": 4}     # name -> int64 words per job of its host table


def samples(B, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        la = int(torch.randint(int(0.44 * TA), TA + 1, (1,), generator=g))
        lt = int(torch.randint(int(0.44 * TT), TT + 1, (1,), generator=g))
        out.append((torch.randn(la, D, generator=g), torch.zeros(la, dtype=torch.bool), torch.randn(lt, D, generator=g),
                    torch.zeros(lt, dtype=torch.bool), (torch.rand(NE, generator=g) < 0.3).float()))
    return out


def pin(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).contiguous().pin_memory()


def loader(B):
    """NBATCH distinct ragged batches, bf16 features, pinned (what a DataLoader with pin_memory=True hands over)"""
    out = []
    for i in range(NBATCH):
        r_a, l_a, r_t, l_t, y = data.collate_seq_packed(samples(B, 100 + i))
        out.append((pin(r_a, torch.bfloat16), l_a, pin(r_t, torch.bfloat16), l_t, pin(y)))
    return out


class CastSpy:
    """records the weight-cast launches of what runs inside `with`: (name, arguments, the copied host table or None); `passes`
    holds the index of the first cast of every pass (a pass starts with hriemo_seq_tables)"""

    def __enter__(self):
        self.calls, self.passes, self.real = [], [], _lib.call

        def spy(name, *args):
            words = CASTS.get(name)
            if name == "hriemo_seq_tables":
                self.passes.append(len(self.calls))
            elif words is not None:
                table = None
                if words:
                    table = torch.tensor(list((ctypes.c_int64 * (words * args[1])).from_address(args[0])), dtype=torch.int64)
                self.calls.append((name, args, table))
            return self.real(name, *args)

        _lib.call = spy
        return self

    def __exit__(self, *exc):
        _lib.call = self.real
        return False


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def recast_graph(calls):
    """the recorded cast launches of ONE pass as a graph of their own"""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()

    def issue():
        for name, args, table in calls:
            _lib.call(name, *((table.data_ptr(),) + tuple(args[1:-1]) if table is not None else args[:-1]), _ops._stream())

    with torch.cuda.stream(side):
        issue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        issue()
    return g


def run(B):
    rag = loader(B)
    n_a, n_t = [int(b[1].sum()) for b in rag], [int(b[3].sum()) for b in rag]
    frac = (sum(n_a) / TA + sum(n_t) / TT) / (2 * B * NBATCH)
    feed = lambda items: data.DevicePrefetcher(items, dev, convert=lambda t: (t[0], t[1].tolist(), t[2], t[3].tolist(), t[4]),   # noqa: E731
                                               ragged={0: B * TA, 2: B * TT})
    torch.manual_seed(1234)
    model = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
    cap = STEPS * B * (ROUNDS + 2)
    stats_e, stats_c = EpochStats(NE, cap), EpochStats(NE, cap)
    es = H.EvalStep(model, fusion_step_loss, stats=stats_c)
    # capture + every bucket graph the loader needs, outside the timed rounds.  The capture pass (the last of the three) re-casts
    # EVERY shadow (CTX.capturing); the warm-up passes in front of it only the stale ones
    with CastSpy() as spy:
        first = next(iter(feed(rag[:1])))
        es.capture_packed(first[0], first[2], first[1], first[3], first[4], pad_to=(TA, TT))
    casts = spy.calls[spy.passes[-1]:]
    elements = sum(int(t.view(-1, CASTS[n])[:, 2].sum()) if t is not None else int(a[2]) for n, a, t in casts)
    evaluate_packed(model, feed(rag), fusion_step_loss, stats_c, step=es)
    torch.cuda.synchronize()
    graphs = len(es._pb.graphs)
    items = [rag[i % NBATCH] for i in range(STEPS)]

    def epoch(step):
        stats = stats_c if step is not None else stats_e
        stats.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        evaluate_packed(model, feed(items), fusion_step_loss, stats, pad_to=(TA, TT), step=step)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS, (time.perf_counter() - t0) / STEPS * 1e3

    epoch(None), epoch(es)                                                             # warm-up
    t = {"E events": [], "E wall": [], "C events": [], "C wall": []}
    for r in range(ROUNDS):
        for arm, step in (("E", None), ("C", es)):
            ev, wall = epoch(step)
            t[arm + " events"].append(ev)
            t[arm + " wall"].append(wall)
        print(f"B {B}: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + " ms/batch", flush=True)
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    a, b = stats_e.result(), stats_c.result()
    print(f"cfg2 B={B} bf16 inputs, valid fraction {frac:.3f}, {NBATCH} distinct batches, {graphs} bucket graphs; both arms: n_samples "
          f"{a['n_samples']} / {b['n_samples']}, avg_loss {a['avg_loss']:.6f} / {b['avg_loss']:.6f}")
    for kind in ("events", "wall"):
        e, c = med[f"E {kind}"], med[f"C {kind}"]
        print(f"  with hand-over ({kind}, {STEPS} batches per round, median of {ROUNDS}): eager {e:.3f} ms/batch (spread {spread[f'E {kind}']:.4f} = "
              f"{spread[f'E {kind}'] * e:.3f} ms), captured {c:.3f} ms/batch (spread {spread[f'C {kind}']:.4f}); eager - captured = {e - c:+.3f} ms, "
              f"eager / captured = {e / c:.2f}")
    # inputs resident: the static buffers fed to themselves (the last loader batch is in them)
    la, lt = rag[(NBATCH - 1)][1].tolist(), rag[(NBATCH - 1)][3].tolist()
    s = es._static
    resident = lambda: es.eval_packed(s[0][:sum(la)], s[1][:sum(lt)], la, lt, s[4])                       # noqa: E731
    stats_c.reset()
    events(resident, 3)
    stats_c.reset()
    t_replay = statistics.median(events(resident, STEPS) for _ in range(ROUNDS))
    g = recast_graph(casts)
    events(g.replay, 3)
    t_cast = statistics.median(events(g.replay, STEPS) for _ in range(ROUNDS))
    print(f"  one eval replay, inputs resident (device events): {t_replay:.3f} ms; the weight re-cast inside it: {len(casts)} launches over "
          f"{elements / 1e6:.1f} M elements, replayed alone as a graph of their own {t_cast:.3f} ms = {t_cast / t_replay:.1%} of the replay "
          f"(the three passes of the capture issued {len(spy.calls)})", flush=True)
    del g
    es.release_graph()


H.set_varlen(True)
H.set_ingest(True)
_ops.PACKED_TAIL = True
print(f"bench_eval_step: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, batches per round {STEPS}")
for b in (64, 8):
    run(b)
