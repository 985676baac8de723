"""What the health log costs the device-state AdamW step at cfg 2 (d = 768, N_e = 6: 54.6 M parameters), one GPU, one process.

  (a) the optimizer's launches alone on cfg 2's flat buffers (DeviceAdamW._enqueue: what a captured step records), HIP events
      around `launches` back-to-back steps, medians of `rounds` interleaved rounds with each arm's spread (max - min) / median:
        parent          sumsq + finalize + update, no log: the three launches of before                       32 B / element
        idle            the same + the two health launches on steps that do NOT record (every = 2^24 - 1)      32 B / element
        record          the same on steps that all record a real update (every = 1)                      32 + 16 B / element
        parent skipped  the three launches with found_inf = 1 (the update kernel returns at once)               4 B / element
        record skipped  the same with the log: every skipped step records, sweeping the gradients only      4 + 4 B / element
        sweep, fold     hriemo_health_sweep / hriemo_health_fold alone on a recording real update               16 B / element
  (b) one captured step_packed (B = 64, T_a = 400, T_t = 128, bf16 inputs resident in the static buffers, dropout 0.1, varlen +
      packed tail) with the optimizer in the graph: no log, HealthLog(every=1), HealthLog(every=50).

No threshold.  The last lines of each part report the differences against both arms' spreads.

usage: python scripts_dev/bench_adamw_health.py [rounds] [launches] [steps] [--skip-step]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops  # noqa: E402
from hri_emo_amd.dp import DataParallelStep, GradBuckets  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW, HealthLog  # noqa: E402
from hri_emo_amd.train import fusion_step_loss  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROUNDS = int(args[0]) if len(args) > 0 else 7
LAUNCHES = int(args[1]) if len(args) > 1 else 20
STEPS = int(args[2]) if len(args) > 2 else 10
SKIP_STEP = "--skip-step" in sys.argv
B, TA, TT, D, NE = 64, 400, 128, 768, 6
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)
dev = torch.device("cuda", 0)
P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
NEVER = 2 ** 24 - 1


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


def rounds_of(arms, timed, unit):
    for fn in arms.values():
        timed(fn)                                              # warm-up: code objects loaded, every arm has run
    ts = {k: [] for k in arms}
    for r in range(ROUNDS):
        for k, fn in arms.items():
            ts[k].append(timed(fn))
        print(f"    round {r}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in ts.items()) + f" ms per {unit}", flush=True)
    return {k: stats(v) for k, v in ts.items()}


# ---------------------------------------------------------------- (a) the optimizer's launches alone
def kernel_arms():
    gen = torch.Generator().manual_seed(99)
    opts = {}
    for name, health in (("parent", None), ("idle", HealthLog(capacity=8, every=NEVER)), ("record", HealthLog(capacity=8, every=1))):
        torch.manual_seed(1234)
        m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
        buckets = GradBuckets(m.parameters(), overlap=False)
        opt = DeviceAdamW(buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0, health=health)
        n = buckets.flat.numel()
        if not opts:
            grad = (torch.randn(n, generator=gen) * 1e-2).to(dev) * (opt.flat_p != 0)   # zeros in the padding, as backward leaves it
        buckets.flat.copy_(grad)
        opt._upload_hyper()
        opts[name] = (opt, m)
    torch.cuda.synchronize()
    n = opts["parent"][0].buckets.flat.numel()
    log = opts["record"][0].health
    print(f"(a) cfg 2 flat buffer: {n} elements, {log.n_params} parameter tensors, {log.n_chunks} chunks", flush=True)
    found = torch.ones(1, device=dev)
    one = torch.ones(1, device=dev)
    # Timing only: every arm steps again and again on one fixed gradient.  The values are no sensible trajectory; the bytes moved
    # per step are what is compared.
    rec = opts["record"][0]
    st = torch.cuda.current_stream().cuda_stream

    def sweep():
        _lib.call("hriemo_health_sweep", P(rec.buckets.flat), P(rec.flat_p), P(rec.m), P(rec.v), n, P(log._chunks), log.n_chunks, P(rec._hyper),
                  P(rec._state), 1, None, 1, P(log._partial), st)

    def fold():
        _lib.call("hriemo_health_fold", P(log._partial), P(log._chunks), log.n_chunks, log.n_params, P(rec._state), None, None, 1, log.capacity,
                  P(log._buf), st)

    # the order matters to the last two arms: they run behind "record", on the state of a real update (state.skip = 0)
    arms = {"parent": lambda: opts["parent"][0]._enqueue(), "idle": lambda: opts["idle"][0]._enqueue(),
            "parent skipped": lambda: opts["parent"][0]._enqueue(one, found), "record skipped": lambda: rec._enqueue(one, found),
            "record": lambda: rec._enqueue(), "sweep": sweep, "fold": fold}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / LAUNCHES

    res = rounds_of(arms, timed, "step")
    bytes_per = {"parent": 32, "idle": 32, "record": 48, "parent skipped": 4, "record skipped": 8, "sweep": 16, "fold": 0}
    for k, (med, spread) in res.items():
        rate = f", {bytes_per[k]} B / element, {n * bytes_per[k] / med / 1e9:.2f} TB/s" if bytes_per[k] else ""
        print(f"(a) {k:>15}: median {med:.4f} ms (spread {spread:.4f}; {ROUNDS} interleaved rounds of {LAUNCHES}, HIP events){rate}", flush=True)
    a = rec.health.arrays()
    print(f"(a) the log after the run: n_recorded {a['n_recorded']}, kinds in the ring {sorted(set(a['kind'].tolist()))}; idle log n_recorded "
          f"{opts['idle'][0].health.arrays()['n_recorded']}", flush=True)
    verdict("idle", "parent", res["parent"], res["idle"])
    verdict("record", "parent", res["parent"], res["record"])
    verdict("record skipped", "parent skipped", res["parent skipped"], res["record skipped"])
    upd = res["record"][0] - res["parent"][0]
    print(f"    a real-update record adds {upd * 1e3:.1f} us; sweep alone {res['sweep'][0] * 1e3:.1f} us + fold alone {res['fold'][0] * 1e3:.1f} us",
          flush=True)


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
    for name, health in (("no log", None), ("every 1", HealthLog(every=1)), ("every 50", HealthLog(every=50))):
        torch.manual_seed(1234)
        m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        opt = DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0, health=health)
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

    res = rounds_of({k: dp for k, (dp, _) in runs.items()}, timed, "step")
    for k, (med, spread) in res.items():
        dp, opt = runs[k]
        rec = f", n_recorded {opt.health.arrays()['n_recorded']}" if opt.health else ""
        print(f"(b) captured step_packed, {k}: median {med:.3f} ms (spread {spread:.4f}; {ROUNDS} interleaved rounds of {STEPS} replays, HIP "
              f"events); device_step {int(opt.device_step)}, skipped {int(opt.skipped)}{rec}", flush=True)
    verdict("every 1", "no log", res["no log"], res["every 1"])
    verdict("every 50", "no log", res["no log"], res["every 50"])
    for dp, _ in runs.values():
        dp.release_graph()


print(f"bench_adamw_health: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, launches per round {LAUNCHES}, steps per round {STEPS}", flush=True)
kernel_arms()
torch.cuda.empty_cache()
if not SKIP_STEP:
    step_arms()
