"""Optimizer step at cfg 2 (d=768, N_e=6: 54.6 M parameters), one GPU, one process.

  (a) FusedClipAdamW.step() against DeviceAdamW.step() on the same flat gradients: HIP events around every step, the two
      alternated repetition by repetition (box-to-box spread is ~4 %), lr changed before every step as a scheduler
      does (DeviceAdamW then uploads its 32-byte hyper block every time).  The device-state step moves the same bytes plus one
      one-block launch: it may take at most 5 % longer (exit status 1 otherwise).
  (b) the trainer step at B = 64 (T_a=400, T_t=128, dropout 0.1): captured forward / backward + eager DeviceAdamW.step() against
      capture(optimizer=opt), everything in one replay.  Wall clock per trainer step (host clock around K steps that end in a
      device synchronise), interleaved rounds.  No threshold: the expected gain is the removed host launches and gaps.

  python scripts_dev/bench_optim.py [--reps R] [--rounds N] [--steps K] [--skip-step]"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H                                   # noqa: E402
from hri_emo_amd.dp import DataParallelStep, GradBuckets   # noqa: E402
from hri_emo_amd.optim import DeviceAdamW, FusedClipAdamW  # noqa: E402
from hri_emo_amd.train import fusion_step_loss            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60, help="(a): alternating repetitions per optimizer")
ap.add_argument("--rounds", type=int, default=6, help="(b): interleaved rounds")
ap.add_argument("--steps", type=int, default=20, help="(b): trainer steps per round")
ap.add_argument("--skip-step", action="store_true", help="(a) only")
a = ap.parse_args()
if a.reps < 50:
    sys.exit("bench_optim: --reps >= 50")

B, Ta, Tt, d, ne = 64, 400, 128, 768, 6
dev = torch.device("cuda", 0)
torch.manual_seed(1234)
m0 = H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=0.1).to(dev).train()
nparam = sum(p.numel() for p in m0.parameters())
print(f"cfg 2 model: {nparam / 1e6:.1f} M parameters", flush=True)


def lr_at(i):
    return 1e-4 * (0.5 + 0.5 * ((i * 37) % 101) / 101.0)          # another value every step, as under a scheduler


# ---------------------------------------------------------------- (a) the optimizer step alone
opts = {}
g = torch.Generator().manual_seed(99)
for name, cls in (("FusedClipAdamW", FusedClipAdamW), ("DeviceAdamW", DeviceAdamW)):
    m = copy.deepcopy(m0)
    buckets = GradBuckets(m.parameters(), overlap=False)
    if not opts:
        grads = (torch.randn(buckets.flat.numel(), generator=g) * 1e-2).to(dev)
    buckets.flat.copy_(grads)
    opts[name] = (cls(buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0), m)


def set_lr(opt, lr):
    if isinstance(opt, DeviceAdamW):
        opt.param_groups[0]["lr"] = lr
    else:
        opt.lr = lr


for i in range(5):
    for opt, _ in opts.values():
        set_lr(opt, lr_at(i))
        opt.step()
torch.cuda.synchronize()
ev = {k: [] for k in opts}
wall = {k: [] for k in opts}
for i in range(a.reps):
    for name, (opt, _) in opts.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        set_lr(opt, lr_at(5 + i))
        t0 = time.perf_counter()
        e0.record()
        opt.step()
        e1.record()
        torch.cuda.synchronize()
        wall[name].append((time.perf_counter() - t0) * 1e3)
        ev[name].append(e0.elapsed_time(e1))
for name in opts:
    ts = sorted(ev[name])
    print(f"(a) {name}.step(): median {statistics.median(ts):.4f} ms, min {ts[0]:.4f}, p90 {ts[int(0.9 * len(ts))]:.4f} (HIP events, "
          f"{a.reps} alternating repetitions); host clock incl. synchronise: median {statistics.median(wall[name]):.4f} ms", flush=True)
ratio = statistics.median(ev["DeviceAdamW"]) / statistics.median(ev["FusedClipAdamW"])
ok = ratio <= 1.05
print(f"(a) DeviceAdamW / FusedClipAdamW = {ratio:.3f} (bound 1.05): {'ok' if ok else 'EXCEEDED'}", flush=True)
del opts, grads
torch.cuda.empty_cache()

# ---------------------------------------------------------------- (b) the trainer step
if not a.skip_step:
    g = torch.Generator().manual_seed(4321)
    batch = (torch.randn(B, Ta, d, generator=g).to(dev), torch.randn(B, Tt, d, generator=g).to(dev), None, None,
             (torch.rand(B, ne, generator=g) < 0.3).float().to(dev))
    runs = {}
    for mode in ("replay + eager opt.step()", "one replay"):
        m = copy.deepcopy(m0)
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        opt = DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)
        dp.capture(*batch, optimizer=opt if mode == "one replay" else None)
        runs[mode] = (dp, opt)

    def trainer_step(mode, i):
        dp, opt = runs[mode]
        opt.param_groups[0]["lr"] = lr_at(i)
        dp.step(*batch)
        if mode != "one replay":
            opt.step()

    for mode in runs:
        for i in range(5):
            trainer_step(mode, i)
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for r in range(a.rounds):
        for mode in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                trainer_step(mode, r * a.steps + i)
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
    for mode, ts in times.items():
        dp, opt = runs[mode]
        print(f"(b) {mode}: {statistics.median(ts):.3f} ms per trainer step (median of {a.rounds} rounds of {a.steps} steps; rounds "
              f"{', '.join(f'{t:.3f}' for t in ts)}); device_step {int(opt.device_step)}, skipped {int(opt.skipped)}", flush=True)
    e, o = statistics.median(times["replay + eager opt.step()"]), statistics.median(times["one replay"])
    print(f"(b) one replay / (replay + eager opt.step()) = {o / e:.3f} ({(e - o) * 1e3:.0f} us per trainer step)", flush=True)
    for dp, _ in runs.values():
        dp.release_graph()
sys.exit(0 if ok else 1)
