"""A/B of the packed tail on the bench's ragged headline step (cfg 2, valid fraction ~0.72), captured, in ONE process:
`_ops.PACKED_TAIL` False (the encoder's output unpacked in front of the gate: the launches from before the packed tail) against
True.  Two models from one seed, one DataParallelStep each (a capture bakes the switch in), replays interleaved round by round
and timed with device events.  `profile off|on [replays]` runs one arm alone for rocprofv3 --kernel-trace --stats.
A leading `fp32` runs the same A/B in the fp32 precision mode: the switch is `_ops.PACKED_TAIL_FP32`, the batch and the model are
those of scripts_dev/bench_fp32_varlen.py (cfg 2 shape, dropout 0.1), and the yardstick is the False arm of the same run.
A leading `mx8` runs the MX-fp8 GEMM mode at the cfg-5 shape (d = 1024, 4 + 2 layers, N_e = 7, B = 32) with THREE arms: (a)
`_ops.ATTN_Q_VARLEN` False, tail off (the launches from before the fused quantiser on packed rows), (b) `ATTN_Q_VARLEN` True, tail
off, (c) (b) plus `_ops.PACKED_TAIL_MX8`; `profile a|b|c` runs one of them alone.
usage: python scripts_dev/ab_packed_tail.py [bf16|fp32|mx8] [rounds] [replays per round]  |  [bf16|fp32|mx8] profile off|on|a|b|c [replays]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _ops  # noqa: E402
from hri_emo_amd.dp import DataParallelStep  # noqa: E402
from hri_emo_amd.train import fusion_step_loss  # noqa: E402

argv = sys.argv[1:]
PREC = argv.pop(0) if argv and argv[0] in ("bf16", "fp32", "mx8") else "bf16"
SWITCH = {"fp32": "PACKED_TAIL_FP32", "mx8": "PACKED_TAIL_MX8"}.get(PREC, "PACKED_TAIL")
dev = torch.device("cuda", 0)
B, T_A, T_T = (32 if PREC == "mx8" else 64), bench.T_A, bench.T_T
g = torch.Generator().manual_seed(4321)
la = torch.randint(T_A // 2, T_A + 1, (B,), generator=g)
lt = torch.randint(T_T // 2, T_T + 1, (B,), generator=g)
if PREC == "fp32":           # the batch of scripts_dev/bench_fp32_varlen.py, draw for draw
    assert (T_A, T_T) == (400, 128), (T_A, T_T)
    H.set_precision("fp32")
    CFG = dict(d_model=768, num_emotions=6, n_heads=8, dropout=0.1)
    h_a, h_t = torch.randn(B, T_A, 768, generator=g).to(dev), torch.randn(B, T_T, 768, generator=g).to(dev)
    m_a, m_t = (torch.arange(T_A)[None] >= la[:, None]).to(dev), (torch.arange(T_T)[None] >= lt[:, None]).to(dev)
    rb = (h_a, h_t, m_a, m_t, (torch.rand(B, 6, generator=g) < 0.3).float().to(dev))
else:
    if PREC == "mx8":        # cfg 5 in its fp8 form (bench.py --workload cfg5_fp8), ragged
        wl = bench.WORKLOADS["cfg5_fp8"]
        assert (wl["T_a"], wl["T_t"], wl["batch"]) == (T_A, T_T, B)
        bench.CFG = dict(wl["model"], beta_hidden=256, dropout=0.1)
        H.set_gemm_mode(wl["gemm"])
    CFG = bench.CFG
    batch = bench.synth(B, 0, dev)
    rb = (batch[0], batch[1], (torch.arange(T_A)[None] >= la[:, None]).to(dev), (torch.arange(T_T)[None] >= lt[:, None]).to(dev), batch[4])
valid = float((la.sum() / T_A + lt.sum() / T_T) / (2 * B))
H.set_varlen(True)


def arm(tail, attn_q=True):
    setattr(_ops, SWITCH, tail)
    _ops.ATTN_Q_VARLEN = attn_q
    torch.manual_seed(1234)
    model = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
    dp = DataParallelStep(model, fusion_step_loss, overlap=False)
    dp.set_global_batch(B)
    dp.step(*rb)
    dp.capture(*rb)
    for _ in range(5):
        dp.step(*rb)
    torch.cuda.synchronize()
    return dp


def timed(dp, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        dp.step(*rb)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


MX8_ARMS = {"a": (False, False), "b": (False, True), "c": (True, True)}          # (PACKED_TAIL_MX8, ATTN_Q_VARLEN)

if argv and argv[0] == "profile":
    dp = arm(*MX8_ARMS[argv[1]]) if PREC == "mx8" else arm(argv[1] == "on")
    n = int(argv[2]) if len(argv) > 2 else 20
    print(f"{SWITCH} {argv[1]}: {timed(dp, n):.3f} ms/step over {n} replays (under the profiler), valid fraction {valid:.3f}")
    sys.exit(0)

rounds = int(argv[0]) if argv else 7
n = int(argv[1]) if len(argv) > 1 else 30
NOTE = (" (dropout on: each capture draws its own seed, so the arms differ by their masks; equality is the tests' business)"
        if CFG.get("dropout", 0.0) > 0 else "")
if PREC == "mx8":
    arms = {k: arm(*v) for k, v in MX8_ARMS.items()}
    res = {k: (float(dp.step(*rb)), dp.buckets.flat.clone()) for k, dp in arms.items()}
    print(f"mx_fp8 cfg 5 ragged step, B={B}, valid fraction {valid:.3f}; loss " + ", ".join(f"({k}) {v[0]:.6f}" for k, v in res.items())
          + "; flat gradients relative L2 vs (a): " + ", ".join(f"({k}) {float((res[k][1] - res['a'][1]).norm() / res['a'][1].norm()):.2e}" for k in "bc") + NOTE)
    print("arms: (a) ATTN_Q_VARLEN False, tail off; (b) ATTN_Q_VARLEN True, tail off; (c) ATTN_Q_VARLEN True, PACKED_TAIL_MX8 True")
    t = {k: [] for k in arms}
    for r in range(rounds):
        for k, dp in arms.items():
            t[k].append(timed(dp, n))
        print(f"round {r}: " + ", ".join(f"({k}) {t[k][-1]:.3f} ms/step" for k in arms))
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"median of {rounds} rounds x {n} replays: "
          + "; ".join(f"({k}) {med[k]:.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f}, spread {max(t[k]) - min(t[k]):.3f})" for k in arms))
    print(f"(b) - (a) = {med['b'] - med['a']:+.3f} ms, (c) - (b) = {med['c'] - med['b']:+.3f} ms, (c) / (a) = {med['c'] / med['a']:.4f}")
    sys.exit(0)
off, on = arm(False), arm(True)
loss_off, loss_on = float(off.step(*rb)), float(on.step(*rb))
rel = float((on.buckets.flat - off.buckets.flat).norm() / off.buckets.flat.norm())
print(f"{PREC} cfg 2 ragged step, B={B}, valid fraction {valid:.3f}; loss off {loss_off:.6f} on {loss_on:.6f}, flat gradients relative L2 {rel:.2e}" + NOTE)
t_off, t_on = [], []
for r in range(rounds):
    t_off.append(timed(off, n))
    t_on.append(timed(on, n))
    print(f"round {r}: {SWITCH} off {t_off[-1]:.3f} ms/step, on {t_on[-1]:.3f} ms/step")
m_off, m_on = statistics.median(t_off), statistics.median(t_on)
print(f"median of {rounds} rounds x {n} replays: off {m_off:.3f} ms (min {min(t_off):.3f}, max {max(t_off):.3f}), "
      f"on {m_on:.3f} ms (min {min(t_on):.3f}, max {max(t_on):.3f}); on / off = {m_on / m_off:.4f}, "
      f"difference {m_off - m_on:+.3f} ms; round-to-round spread off {max(t_off) - min(t_off):.3f} ms, on {max(t_on) - min(t_on):.3f} ms")
