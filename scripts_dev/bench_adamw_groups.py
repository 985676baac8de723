"""What parameter groups cost the in-graph AdamW update at cfg 2 (d = 768, N_e = 6: 54.6 M parameters), one GPU, one process.

  (a) the update kernel alone on cfg 2's flat buffer, HIP events around `launches` back-to-back launches, medians of `rounds`
      interleaved rounds with each arm's spread (max - min) / median:
        single     hriemo_adamw_flat_dev, the single-group kernel (its device code is unchanged by the grouped kernel's arrival)
        split      hriemo_adamw_flat_groups with the matrix / vector split of optim.decay_groups (2 groups, 2 segments)
        every      hriemo_adamw_flat_groups with a group change at every parameter (2 groups alternating in flat-buffer order:
                   one segment per parameter)
      Every arm moves the same 28 B per element (p, m, v read and written, g read); bytes / time is printed for each.
  (b) one captured step_packed (B = 64, T_a = 400, T_t = 128, bf16 inputs resident in the static buffers, dropout 0.1, varlen +
      packed tail) with the optimizer in the graph: DeviceAdamW built without param_groups against the decay_groups split.  Device
      events around `steps` replays, medians of `rounds` interleaved rounds, spreads.

No threshold: the expectation is "inside the spread"; the last lines say whether a grouped arm is slower than the single-group
one by more than both spreads.

usage: python scripts_dev/bench_adamw_groups.py [rounds] [launches] [steps] [--skip-step]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops  # noqa: E402
from hri_emo_amd.dp import DataParallelStep, GradBuckets  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW, decay_groups, group_segments  # noqa: E402
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


def verdict(name, base, arm):
    (mb, sb), (ma, sa) = base, arm
    slower = ma - mb > sb * mb and ma - mb > sa * ma
    print(f"    {name}: {ma / mb:.4f} x single ({(ma - mb) * 1e3:+.1f} us); spreads {sb * mb * 1e3:.1f} us / {sa * ma * 1e3:.1f} us: "
          f"{'SLOWER by more than both spreads' if slower else 'inside the spread'}", flush=True)


# ---------------------------------------------------------------- (a) the update kernel alone
def kernel_arms():
    torch.manual_seed(1234)
    m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
    buckets = GradBuckets(m.parameters(), overlap=False)
    n = buckets.flat.numel()
    order = sorted(buckets.params, key=lambda p: buckets._offsets[id(p)])
    tables = {"split": group_segments(buckets, decay_groups(m.named_parameters(), 1e-2)),
              "every": group_segments(buckets, [{"params": order[0::2]}, {"params": order[1::2]}])}
    g = torch.Generator().manual_seed(99)
    buckets.flat.copy_((torch.randn(n, generator=g) * 1e-2).to(dev))
    p, mm, vv = (torch.randn(n, generator=g) * 0.05).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    partial = torch.zeros(1024, device=dev)
    hyper = torch.tensor([[1e-4, 0.9, 0.999, 1e-8, 1e-2, 5.0, 0, 0], [1e-4, 0.9, 0.999, 1e-8, 0.0, 5.0, 0, 0]], device=dev).reshape(-1)
    state = torch.zeros(16, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("hriemo_sumsq_f32", P(buckets.flat), n, P(partial), 1024, st)
    _lib.call("hriemo_optim_finalize_groups", P(partial), 1024, P(hyper), 2, None, None, P(state), None, st)
    # Timing only: every arm updates the same p / m / v again and again from one fixed gradient, and the single arm reads row 0 of
    # a two-group finalize.  The values are not meant to be a sensible trajectory; the bytes moved are what the arms share.
    dev_tables = {k: (torch.tensor(s, dtype=torch.int64, device=dev), torch.tensor(q, dtype=torch.int32, device=dev)) for k, (s, q) in tables.items()}
    arms = {"single": lambda: _lib.call("hriemo_adamw_flat_dev", P(p), P(buckets.flat), P(mm), P(vv), n, P(hyper), P(state), st)}
    for k, (s, q) in dev_tables.items():
        arms[k] = (lambda s=s, q=q: _lib.call("hriemo_adamw_flat_groups", P(p), P(buckets.flat), P(mm), P(vv), n, P(s), P(q), q.numel(),
                                              P(hyper), P(state), 2, st))
    print(f"(a) cfg 2 flat buffer: {n} elements ({n * 28 / 1e9:.3f} GB per update), {len(order)} parameters; segments: "
          + ", ".join(f"{k} {len(q)}" for k, (s, q) in tables.items()), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / LAUNCHES

    for fn in arms.values():
        timed(fn)                                              # warm-up: code objects loaded, every arm has run
    ts = {k: [] for k in arms}
    for r in range(ROUNDS):
        for k, fn in arms.items():
            ts[k].append(timed(fn))
        print(f"    round {r}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in ts.items()) + " ms per launch", flush=True)
    res = {k: stats(v) for k, v in ts.items()}
    for k, (med, spread) in res.items():
        print(f"(a) {k:>6}: median {med:.4f} ms per launch (spread {spread:.4f}; {ROUNDS} interleaved rounds of {LAUNCHES} launches, HIP "
              f"events): {n * 28 / med / 1e9:.2f} TB/s", flush=True)
    for k in ("split", "every"):
        verdict(k, res["single"], res[k])


# ---------------------------------------------------------------- (b) one captured step_packed
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
    for name in ("one group", "two groups"):
        torch.manual_seed(1234)
        m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        kw = dict(param_groups=decay_groups(m.named_parameters(), 1e-2)) if name == "two groups" else {}
        opt = DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0, **kw)
        dp.capture_packed(rows_a, rows_t, la, lt, y, pad_to=(TA, TT), optimizer=opt)
        runs[name] = (dp, opt)

    def timed(dp):
        sb = dp._static
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            dp.step_packed(sb[0][:sum(la)], sb[1][:sum(lt)], la, lt, sb[4])     # inputs resident: the static buffers fed to themselves
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    for dp, _ in runs.values():
        timed(dp)
    ts = {k: [] for k in runs}
    for r in range(ROUNDS):
        for k, (dp, _) in runs.items():
            ts[k].append(timed(dp))
        print(f"    round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in ts.items()) + " ms per step", flush=True)
    res = {k: stats(v) for k, v in ts.items()}
    for k, (med, spread) in res.items():
        dp, opt = runs[k]
        print(f"(b) captured step_packed, {k}: median {med:.3f} ms (spread {spread:.4f}; {ROUNDS} interleaved rounds of {STEPS} replays, HIP "
              f"events); device_step {int(opt.device_step)}, skipped {int(opt.skipped)}", flush=True)
    verdict("two groups", res["one group"], res["two groups"])
    for dp, _ in runs.values():
        dp.release_graph()


print(f"bench_adamw_groups: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, launches per round {LAUNCHES}, steps per round {STEPS}", flush=True)
kernel_arms()
torch.cuda.empty_cache()
if not SKIP_STEP:
    step_arms()
