"""What in-graph weight averaging costs the AdamW update at cfg 2 (d = 768, N_e = 6: 54.6 M parameters), one GPU, one process.

  (a) kernels alone on cfg 2's flat buffer, HIP events around `launches` back-to-back launches, medians of `rounds` interleaved
      rounds with each arm's spread (max - min) / median:
        parent     hriemo_adamw_flat_dev, the update kernel of before (its device code is unchanged)          28 B / element
        avg on     hriemo_adamw_flat_dev_avg on an AVERAGING update (flag 1: avg read and written too)        36 B / element
        avg off    hriemo_adamw_flat_dev_avg on a real update that does not average (avg untouched)           28 B / element
        unfused    what a user writes today: hriemo_adamw_flat_dev, then avg.lerp_(p, w) over the flat buffer 28 + 12 B / element
        swap       hriemo_swap_fp32 of the parameter buffer and the average (one way of averaged_weights())    16 B / element
  (b) one captured step_packed (B = 64, T_a = 400, T_t = 128, bf16 inputs resident in the static buffers, dropout 0.1, varlen +
      packed tail) with the optimizer in the graph: DeviceAdamW without averaging against averaging="ema" on every step.

No threshold.  The last lines say whether "avg off" is slower than the parent, and whether the fused "avg on" beats the unfused arm,
by more than both arms' spreads.

usage: python scripts_dev/bench_adamw_avg.py [rounds] [launches] [steps] [--skip-step]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops  # noqa: E402
from hri_emo_amd.dp import DataParallelStep, GradBuckets  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW  # noqa: E402
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
    """is `arm` slower than `base` by more than both spreads / faster by more than both spreads / inside the spread"""
    (mb, sb), (ma, sa) = base, arm
    gap = max(sb * mb, sa * ma)
    word = "SLOWER by more than both spreads" if ma - mb > gap else "FASTER by more than both spreads" if mb - ma > gap else "inside the spread"
    print(f"    {name}: {ma / mb:.4f} x {base_name} ({(ma - mb) * 1e3:+.1f} us); spreads {sb * mb * 1e3:.1f} us / {sa * ma * 1e3:.1f} us: {word}",
          flush=True)


# ---------------------------------------------------------------- (a) the kernels alone
def kernel_arms():
    torch.manual_seed(1234)
    m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
    buckets = GradBuckets(m.parameters(), overlap=False)
    n = buckets.flat.numel()
    g = torch.Generator().manual_seed(99)
    buckets.flat.copy_((torch.randn(n, generator=g) * 1e-2).to(dev))
    p, mm, vv = (torch.randn(n, generator=g) * 0.05).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    avg = p.clone()
    partial = torch.zeros(1024, device=dev)
    hyper = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 1e-2, 5.0, 0, 0], device=dev)
    state = torch.zeros(8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("hriemo_sumsq_f32", P(buckets.flat), n, P(partial), 1024, st)
    _lib.call("hriemo_optim_finalize", P(partial), 1024, P(hyper), None, None, P(state), st)
    torch.cuda.synchronize()
    stamp = float(state[0])
    w = 1e-3
    as_on = torch.tensor([5.0, w, 1.0, stamp], device=dev)     # n_averaged, w, flag = averaging update, stamp = this step
    as_off = torch.tensor([5.0, w, 0.0, stamp], device=dev)    # a real update that does not average
    # Timing only: every arm updates the same p / m / v / avg again and again from one fixed gradient and one fixed state block.
    # The values are not meant to be a sensible trajectory; the bytes moved per launch are what is compared.

    def parent():
        _lib.call("hriemo_adamw_flat_dev", P(p), P(buckets.flat), P(mm), P(vv), n, P(hyper), P(state), st)

    def fused(a_s):
        return lambda: _lib.call("hriemo_adamw_flat_dev_avg", P(p), P(buckets.flat), P(mm), P(vv), n, P(hyper), P(state), P(avg), P(a_s), st)

    def unfused():
        parent()
        avg.lerp_(p, w)

    arms = {"parent": (parent, 28), "avg on": (fused(as_on), 36), "avg off": (fused(as_off), 28), "unfused": (unfused, 40),
            "swap": (lambda: _lib.call("hriemo_swap_fp32", P(p), P(avg), n, st), 16)}
    print(f"(a) cfg 2 flat buffer: {n} elements ({n * 28 / 1e9:.3f} GB per update, {n * 36 / 1e9:.3f} GB per averaging update)", flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / LAUNCHES

    for fn, _ in arms.values():
        timed(fn)                                              # warm-up: code objects loaded, every arm has run
    ts = {k: [] for k in arms}
    for r in range(ROUNDS):
        for k, (fn, _) in arms.items():
            ts[k].append(timed(fn))
        print(f"    round {r}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in ts.items()) + " ms per launch", flush=True)
    res = {k: stats(v) for k, v in ts.items()}
    for k, (med, spread) in res.items():
        print(f"(a) {k:>8}: median {med:.4f} ms per launch (spread {spread:.4f}; {ROUNDS} interleaved rounds of {LAUNCHES} launches, HIP "
              f"events): {arms[k][1]} B / element, {n * arms[k][1] / med / 1e9:.2f} TB/s", flush=True)
    verdict("avg off", "parent", res["parent"], res["avg off"])
    verdict("avg on", "parent", res["parent"], res["avg on"])
    verdict("avg on", "unfused", res["unfused"], res["avg on"])


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
    for name in ("no averaging", "ema every step"):
        torch.manual_seed(1234)
        m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        kw = dict(averaging="ema", avg_decay=0.999) if name == "ema every step" else {}
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
        n_avg = f", n_averaged {int(opt.n_averaged)}" if opt.averaging else ""
        print(f"(b) captured step_packed, {k}: median {med:.3f} ms (spread {spread:.4f}; {ROUNDS} interleaved rounds of {STEPS} replays, HIP "
              f"events); device_step {int(opt.device_step)}, skipped {int(opt.skipped)}{n_avg}", flush=True)
    verdict("ema every step", "no averaging", res["no averaging"], res["ema every step"])
    for dp, _ in runs.values():
        dp.release_graph()


print(f"bench_adamw_avg: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, launches per round {LAUNCHES}, steps per round {STEPS}", flush=True)
kernel_arms()
torch.cuda.empty_cache()
if not SKIP_STEP:
    step_arms()
