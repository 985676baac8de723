"""What the activation log (train.ActivationLog) costs the captured step at cfg 2 (d = 768, T_a = 400, T_t = 128, N_e = 6, bf16
inputs resident in the static buffers, dropout 0.1, varlen + packed tail, DeviceAdamW in the graph), one GPU, one process.

  (1) one captured step_packed at B = 64 and at B = 8, five arms, HIP events around `steps` back-to-back replays, medians of
      `rounds` interleaved rounds with each arm's spread (max - min) / median:
        no log      the step of before: the yardstick
        idle        a log attached with every = 2^30: no timed pass records, every probe and fold launch exits at its first word
        every 1     every pass records all 23 sites, forward and gradient
        tail sites  every = 1 with sites = enc*.audio_ffn, enc*.text_ffn, gate.fused, dec*.ffn, logits
        one site    every = 1 with sites = logits: the plan, two probes of [B, N_e] and the two folds -- what a pass costs before
                    any tensor is read
  (2) one captured EvalStep evaluation at B = 8, without and with a log (every = 1, forward half only).

What traffic predicts, printed beside the measurement: a recording pass reads every probed tensor once -- the bytes are summed
from the log's own n_rows -- and this project measured roughly 3 us for a launch of exiting blocks.

No threshold.  The last lines of each part report the differences against both arms' spreads.

usage: python scripts_dev/bench_activation_log.py [rounds] [steps]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _ops  # noqa: E402
from hri_emo_amd.dp import DataParallelStep  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW  # noqa: E402
from hri_emo_amd.train import ActivationLog, fusion_step_loss  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROUNDS = int(args[0]) if len(args) > 0 else 7
STEPS = int(args[1]) if len(args) > 1 else 10
TA, TT, D, NE = 400, 128, 768, 6
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)
TAIL_SITES = ["enc*.audio_ffn", "enc*.text_ffn", "gate.fused", "dec*.ffn", "logits"]
NEVER = 2 ** 30
LAUNCH_US, HBM_TBS = 3.0, 4.0          # an exiting launch as measured in this project; a streaming read as the health sweep reaches it
dev = torch.device("cuda", 0)


def stats(ts):
    med = statistics.median(ts)
    return med, (max(ts) - min(ts)) / med


def verdict(name, base_name, base, arm):
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


def predicted(log):
    """(launches of a pass, bytes a recording pass reads) from the newest record"""
    a = log.arrays()
    if len(a["pass"]) == 0:
        return None
    nbytes = launches = 0
    for half in ("forward", "gradient"):
        f = a[half]
        for s, name in enumerate(a["sites"]):
            if f["have"][-1, s]:
                launches += 1
                nbytes += int(f["n_rows"][-1, s]) * log.widths[s] * (4 if name in ("gate.w", "logits") else 2)
    return launches + 1 + bin(int(a["halves"][-1])).count("1"), nbytes          # + the plan and one fold per half


def batch(B):
    g = torch.Generator().manual_seed(4321)
    la, lt = [TA] * B, [TT] * B
    rows_a = torch.randn(sum(la), D, generator=g).to(dev, torch.bfloat16)
    rows_t = torch.randn(sum(lt), D, generator=g).to(dev, torch.bfloat16)
    y = (torch.rand(B, NE, generator=g) < 0.3).float().to(dev)
    return rows_a, rows_t, la, lt, y


def step_arms(B):
    rows_a, rows_t, la, lt, y = batch(B)
    runs = {}
    for name, kw in (("no log", None), ("idle", dict(every=NEVER)), ("every 1", dict(every=1)), ("tail sites", dict(every=1, sites=TAIL_SITES)),
                     ("one site", dict(every=1, sites=["logits"]))):
        torch.manual_seed(1234)
        m = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
        dp = DataParallelStep(m, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        log = None
        if kw is not None:
            log = ActivationLog.for_model(m, capacity=4, **kw)
            dp.attach_activations(log)
        opt = DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)
        dp.capture_packed(rows_a, rows_t, la, lt, y, pad_to=(TA, TT), optimizer=opt)
        if name == "idle":
            dp.step_packed(rows_a, rows_t, la, lt, y)          # pass 0 records under any `every`: it is taken here, outside the timing
        runs[name] = (dp, opt, log)

    def timed(dp):
        sb = dp._static
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            dp.step_packed(sb[0][:sum(la)], sb[1][:sum(lt)], la, lt, sb[4])     # inputs resident: the static buffers fed to themselves
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    print(f"(1) captured step_packed, B = {B}", flush=True)
    res = rounds_of({k: r[0] for k, r in runs.items()}, timed, "step")
    for k, (med, spread) in res.items():
        dp, opt, log = runs[k]
        note = ""
        if log is not None:
            a = log.arrays()
            launches, nbytes = predicted(log)
            note = (f"; n_passes {a['n_passes']}, n_recorded {a['n_recorded']}, blame {log.blame()}; a recording pass: {launches} launches, "
                    f"{nbytes / 1e6:.1f} MB read = {nbytes / HBM_TBS / 1e6:.1f} us at {HBM_TBS:.0f} TB/s; exiting launches: "
                    f"{launches * LAUNCH_US:.0f} us at {LAUNCH_US:.0f} us each if none overlapped")
        print(f"(1) B = {B}, {k}: median {med:.3f} ms (spread {spread:.4f}; {ROUNDS} interleaved rounds of {STEPS} replays, HIP events); "
              f"device_step {int(opt.device_step)}, skipped {int(opt.skipped)}{note}", flush=True)
    for k in ("idle", "every 1", "tail sites", "one site"):
        verdict(k, "no log", res["no log"], res[k])
    for dp, _, _ in runs.values():
        dp.release_graph()
    del runs
    torch.cuda.empty_cache()


def eval_arms(B):
    rows_a, rows_t, la, lt, y = batch(B)
    torch.manual_seed(1234)
    m = H.FusionWithEmotionDecoder(**CFG).to(dev).eval()
    runs = {}
    for name, on in (("no log", False), ("every 1", True)):
        log = ActivationLog.for_model(m, capacity=4) if on else None
        es = H.EvalStep(m, fusion_step_loss, **({"act_log": log} if on else {}))
        es.capture_packed(rows_a, rows_t, la, lt, y, pad_to=(TA, TT))
        runs[name] = (es, log)

    def timed(es):
        sb = es._static
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            es.eval_packed(sb[0][:sum(la)], sb[1][:sum(lt)], la, lt, sb[4])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    print(f"(2) captured EvalStep, B = {B}", flush=True)
    res = rounds_of({k: r[0] for k, r in runs.items()}, timed, "evaluation")
    for k, (med, spread) in res.items():
        es, log = runs[k]
        note = ""
        if log is not None:
            launches, nbytes = predicted(log)
            note = (f"; n_recorded {log.arrays()['n_recorded']}; a recording pass: {launches} launches, {nbytes / 1e6:.1f} MB read = "
                    f"{nbytes / HBM_TBS / 1e6:.1f} us at {HBM_TBS:.0f} TB/s")
        print(f"(2) B = {B}, {k}: median {med:.3f} ms (spread {spread:.4f}; {ROUNDS} interleaved rounds of {STEPS} replays, HIP events){note}",
              flush=True)
    verdict("every 1", "no log", res["no log"], res["every 1"])
    for es, _ in runs.values():
        es.release_graph()


print(f"bench_activation_log: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, steps per round {STEPS}", flush=True)
H.set_varlen(True)
H.set_ingest(True)
_ops.PACKED_TAIL = True
step_arms(64)
step_arms(8)
eval_arms(8)
