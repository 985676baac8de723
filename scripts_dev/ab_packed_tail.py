"""A/B of the packed tail on the bench's ragged headline step (cfg 2, valid fraction ~0.72), captured, in ONE process:
`_ops.PACKED_TAIL` False (the encoder's output unpacked in front of the gate: the launches from before the packed tail) against
True.  Two models from one seed, one DataParallelStep each (a capture bakes the switch in), replays interleaved round by round
and timed with device events.  `profile off|on [replays]` runs one arm alone for rocprofv3 --kernel-trace --stats.
usage: python scripts_dev/ab_packed_tail.py [rounds] [replays per round]  |  profile off|on [replays]"""
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

dev = torch.device("cuda", 0)
B, T_A, T_T = 64, bench.T_A, bench.T_T
batch = bench.synth(B, 0, dev)
g = torch.Generator().manual_seed(4321)
la = torch.randint(T_A // 2, T_A + 1, (B,), generator=g)
lt = torch.randint(T_T // 2, T_T + 1, (B,), generator=g)
rb = (batch[0], batch[1], (torch.arange(T_A)[None] >= la[:, None]).to(dev), (torch.arange(T_T)[None] >= lt[:, None]).to(dev), batch[4])
valid = float((la.sum() / T_A + lt.sum() / T_T) / (2 * B))
H.set_varlen(True)


def arm(tail):
    _ops.PACKED_TAIL = tail
    torch.manual_seed(1234)
    model = H.FusionWithEmotionDecoder(**bench.CFG).to(dev).train()
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


if len(sys.argv) > 1 and sys.argv[1] == "profile":
    dp = arm(sys.argv[2] == "on")
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    print(f"PACKED_TAIL {sys.argv[2]}: {timed(dp, n):.3f} ms/step over {n} replays (under the profiler), valid fraction {valid:.3f}")
    sys.exit(0)

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
n = int(sys.argv[2]) if len(sys.argv) > 2 else 30
off, on = arm(False), arm(True)
loss_off, loss_on = float(off.step(*rb)), float(on.step(*rb))
rel = float((on.buckets.flat - off.buckets.flat).norm() / off.buckets.flat.norm())
print(f"cfg 2 ragged step, B={B}, valid fraction {valid:.3f}; loss off {loss_off:.6f} on {loss_on:.6f}, flat gradients relative L2 {rel:.2e}")
t_off, t_on = [], []
for r in range(rounds):
    t_off.append(timed(off, n))
    t_on.append(timed(on, n))
    print(f"round {r}: PACKED_TAIL off {t_off[-1]:.3f} ms/step, on {t_on[-1]:.3f} ms/step")
m_off, m_on = statistics.median(t_off), statistics.median(t_on)
print(f"median of {rounds} rounds x {n} replays: off {m_off:.3f} ms (min {min(t_off):.3f}, max {max(t_off):.3f}), "
      f"on {m_on:.3f} ms (min {min(t_on):.3f}, max {max(t_on):.3f}); on / off = {m_on / m_off:.4f}, "
      f"difference {m_off - m_on:+.3f} ms")
