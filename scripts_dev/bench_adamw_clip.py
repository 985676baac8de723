"""What per-group and per-parameter clipping cost the in-graph AdamW step at cfg 2 (d = 768, N_e = 6: 54.6 M parameters), one GPU,
one process.  HIP events, medians of `rounds` interleaved rounds with each arm's spread (max - min) / median.

  (a) the norm kernel alone on cfg 2's flat gradient buffer (4 B per element in every arm):
        f32        hriemo_sumsq_f32, 1024 blocks grid-striding over the buffer
        group      hriemo_sumsq_units with the chunk table of clip="group" over the matrix / vector split (2 units)
        parameter  hriemo_sumsq_units with the chunk table of clip="parameter" (one unit per parameter tensor)
  (b) the three launches of a step (norm, finalize, update: 4 + 28 B per element in every arm):
        global     hriemo_sumsq_f32 -> hriemo_optim_finalize_groups -> hriemo_adamw_flat_groups (the matrix / vector split)
        group      hriemo_sumsq_units -> hriemo_optim_finalize_units -> hriemo_adamw_flat_units, the same split as 2 units
        parameter  the same three with one unit and one segment per parameter tensor
  (c) one captured step_packed (B = 64, T_a = 400, T_t = 128, bf16 inputs resident in the static buffers, dropout 0.1, varlen +
      packed tail) with the optimizer in the graph: clip="global" against clip="parameter", both over the decay_groups split.

No threshold: the expectation is "level with the global arm"; the verdict lines say whether a unit arm is slower than it by more
than both spreads.

usage: python scripts_dev/bench_adamw_clip.py [rounds] [launches] [steps] [--skip-step]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops  # noqa: E402
from hri_emo_amd.dp import DataParallelStep, GradBuckets  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW, clip_units, decay_groups, group_segments  # noqa: E402
from hri_emo_amd.train import fusion_step_loss  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROUNDS = int(args[0]) if len(args) > 0 else 7
LAUNCHES = int(args[1]) if len(args) > 1 else 20
STEPS = int(args[2]) if len(args) > 2 else 10
SKIP_STEP = "--skip-step" in sys.argv
B, TA, TT, D, NE = 64, 400, 128, 768, 6
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)
dev = torch.device("cuda", 0)
P = lambda t: t.data_ptr()  # noqa: E731


def stats(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def verdict(name, base_name, base, arm):
    (mb, sb), (ma, sa) = base, arm
    slower = ma - mb > sb * mb and ma - mb > sa * ma
    print(f"    {name}: {ma / mb:.4f} x {base_name} ({(ma - mb) * 1e3:+.1f} us); spreads {sb * mb * 1e3:.1f} us / {sa * ma * 1e3:.1f} us: "
          f"{'SLOWER by more than both spreads' if slower else 'inside the spread'}", flush=True)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds_of(arms, reps, unit):
    for fn in arms.values():
        timed(fn, reps)                                        # warm-up: code objects loaded, every arm has run
    ts = {k: [] for k in arms}
    for r in range(ROUNDS):
        for k, fn in arms.items():
            ts[k].append(timed(fn, reps))
        print(f"    round {r}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in ts.items()) + f" ms per {unit}", flush=True)
    return {k: stats(v) for k, v in ts.items()}


# ---------------------------------------------------------------- (a), (b) the kernels on cfg 2's flat buffer
def kernel_arms():
    torch.manual_seed(1234)
    m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
    buckets = GradBuckets(m.parameters(), overlap=False)
    n = buckets.flat.numel()
    groups = decay_groups(m.named_parameters(), 1e-2)
    g = torch.Generator().manual_seed(99)
    buckets.flat.copy_((torch.randn(n, generator=g) * 1e-2).to(dev))
    grad = buckets.flat
    p, mm, vv = (torch.randn(n, generator=g) * 0.05).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    hyper = torch.tensor([[1e-4, 0.9, 0.999, 1e-8, 1e-2, 5.0, 0, 0], [1e-4, 0.9, 0.999, 1e-8, 0.0, 5.0, 0, 0]], device=dev).reshape(-1)
    st = torch.cuda.current_stream().cuda_stream
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    seg, seg_group = group_segments(buckets, groups)
    glob = dict(seg=i64(seg), seg_group=i32(seg_group), partial=torch.zeros(1024, device=dev), state=torch.zeros(16, device=dev))
    unit = {}
    for mode in ("group", "parameter"):
        t = clip_units(buckets, groups, mode)
        unit[mode] = dict(seg=i64(t["seg"]), seg_group=i32(t["seg_group"]), seg_unit=i32(t["seg_unit"]), chunks=i64(t["chunks"]),
                          unit_chunks=i32(t["unit_chunks"]), unit_group=i32(t["unit_group"]), partial=torch.zeros(len(t["chunks"]), device=dev),
                          state=torch.zeros(16, device=dev), clip=torch.zeros(2 * len(t["unit_group"]), device=dev))
        short = sum(1 for r in t["chunks"] if r[1] < 32768)
        print(f"    clip={mode!r}: {len(t['unit_group'])} units, {len(t['seg_group'])} segments, {len(t['chunks'])} chunks ({short} shorter than 32768)", flush=True)

    def sumsq_f32():
        _lib.call("hriemo_sumsq_f32", P(grad), n, P(glob["partial"]), 1024, st)

    def sumsq_units(mode):
        u = unit[mode]
        _lib.call("hriemo_sumsq_units", P(grad), n, P(u["chunks"]), u["partial"].numel(), P(u["partial"]), st)

    def step_global():
        sumsq_f32()
        _lib.call("hriemo_optim_finalize_groups", P(glob["partial"]), 1024, P(hyper), 2, None, None, P(glob["state"]), None, st)
        _lib.call("hriemo_adamw_flat_groups", P(p), P(grad), P(mm), P(vv), n, P(glob["seg"]), P(glob["seg_group"]), glob["seg_group"].numel(),
                  P(hyper), P(glob["state"]), 2, st)

    def step_units(mode):
        u = unit[mode]
        U, S = u["unit_group"].numel(), u["seg_group"].numel()
        sumsq_units(mode)
        _lib.call("hriemo_optim_finalize_units", P(u["partial"]), u["partial"].numel(), P(u["unit_chunks"]), P(u["unit_group"]), U, P(hyper), 2,
                  None, None, P(u["state"]), None, P(u["clip"]), None, None, st)
        _lib.call("hriemo_adamw_flat_units", P(p), P(grad), P(mm), P(vv), n, P(u["seg"]), P(u["seg_group"]), P(u["seg_unit"]), S, P(hyper),
                  P(u["state"]), 2, P(u["clip"]), U, st)

    # Timing only: every arm updates the same p / m / v again and again from one fixed gradient.  The values are not meant to be a
    # sensible trajectory; the bytes moved are what the arms share.
    print(f"(a) cfg 2 flat gradient buffer: {n} elements ({n * 4 / 1e9:.3f} GB per norm), {len(buckets.params)} parameters", flush=True)
    res = rounds_of({"f32": sumsq_f32, "group": lambda: sumsq_units("group"), "parameter": lambda: sumsq_units("parameter")}, LAUNCHES, "launch")
    for k, (med, spread) in res.items():
        print(f"(a) {k:>9}: median {med:.4f} ms per launch (spread {spread:.4f}; {ROUNDS} interleaved rounds of {LAUNCHES} launches, HIP "
              f"events): {n * 4 / med / 1e9:.2f} TB/s", flush=True)
    for k in ("group", "parameter"):
        verdict(k, "f32", res["f32"], res[k])
    print(f"(b) the three launches of a step ({n * 32 / 1e9:.3f} GB per step)", flush=True)
    res = rounds_of({"global": step_global, "group": lambda: step_units("group"), "parameter": lambda: step_units("parameter")}, LAUNCHES, "step")
    for k, (med, spread) in res.items():
        print(f"(b) {k:>9}: median {med:.4f} ms per step (spread {spread:.4f}; {ROUNDS} interleaved rounds of {LAUNCHES} steps, HIP events): "
              f"{n * 32 / med / 1e9:.2f} TB/s", flush=True)
    for k in ("group", "parameter"):
        verdict(k, "global", res["global"], res[k])


# ---------------------------------------------------------------- (c) one captured step_packed
def step_arms():
    H.set_varlen(True)
    H.set_ingest(True)
    _ops.PACKED_TAIL = True
    g = torch.Generator().manual_seed(4321)
    la, lt = [TA] * B, [TT] * B
    rows_a = torch.randn(sum(la), D, generator=g).to(dev, torch.bfloat16)
    rows_t = torch.randn(sum(lt), D, generator=g).to(dev, torch.bfloat16)
    y = (torch.rand(B, NE, generator=g) < 0.3).float().to(dev)
    runs = {}
    for name in ("global", "parameter"):
        torch.manual_seed(1234)
        m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        opt = DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0, param_groups=decay_groups(m.named_parameters(), 1e-2), clip=name)
        dp.capture_packed(rows_a, rows_t, la, lt, y, pad_to=(TA, TT), optimizer=opt)
        runs[name] = (dp, opt)

    def replay(dp):
        sb = dp._static
        return lambda: dp.step_packed(sb[0][:sum(la)], sb[1][:sum(lt)], la, lt, sb[4])     # inputs resident: the static buffers fed to themselves

    res = rounds_of({k: replay(dp) for k, (dp, _) in runs.items()}, STEPS, "step")
    for k, (med, spread) in res.items():
        dp, opt = runs[k]
        print(f"(c) captured step_packed, clip={k!r}: median {med:.3f} ms (spread {spread:.4f}; {ROUNDS} interleaved rounds of {STEPS} replays, "
              f"HIP events); device_step {int(opt.device_step)}, skipped {int(opt.skipped)}", flush=True)
    verdict("parameter", "global", res["global"], res["parameter"])
    for dp, _ in runs.values():
        dp.release_graph()


print(f"bench_adamw_clip: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, launches per round {LAUNCHES}, steps per round {STEPS}", flush=True)
kernel_arms()
torch.cuda.empty_cache()
if not SKIP_STEP:
    step_arms()
