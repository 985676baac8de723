"""fp32 precision mode, training step at cfg 2 (B=64, T_a=400, T_t=128, d=768, N_e=6, dropout 0.1), captured (DataParallelStep,
one GPU): the padded encoder against the packed (varlen) one on the same ragged batch -- valid length ~U[L/2, L] per sample and
modality, the pattern of bench.py --full's packed leg (valid fraction ~0.75).  Both steps are captured in one process and timed in
interleaved rounds (median of the rounds).

  python scripts_dev/bench_fp32_varlen.py [--mode both|padded|packed] [--rounds R] [--steps K]
--mode padded / packed: that step alone (warm-up, capture, K replays), e.g. under rocprofv3 --kernel-trace --stats for a per-kernel
table of one of the two."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H                                   # noqa: E402
from hri_emo_amd.dp import DataParallelStep                # noqa: E402
from hri_emo_amd.train import fusion_step_loss            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("both", "padded", "packed"), default="both")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
a = ap.parse_args()

B, Ta, Tt, d, ne = 64, 400, 128, 768, 6
dev = torch.device("cuda", 0)
H.set_precision("fp32")
torch.manual_seed(1234)
m = H.FusionWithEmotionDecoder(d_model=d, num_emotions=ne, n_heads=8, dropout=0.1).to(dev).train()
g = torch.Generator().manual_seed(4321)
la = torch.randint(Ta // 2, Ta + 1, (B,), generator=g)
lt = torch.randint(Tt // 2, Tt + 1, (B,), generator=g)
h_a, h_t = torch.randn(B, Ta, d, generator=g).to(dev), torch.randn(B, Tt, d, generator=g).to(dev)
m_a, m_t = (torch.arange(Ta)[None] >= la[:, None]).to(dev), (torch.arange(Tt)[None] >= lt[:, None]).to(dev)
y = (torch.rand(B, ne, generator=g) < 0.3).float().to(dev)
batch = (h_a, h_t, m_a, m_t, y)
valid = float((la.sum() / Ta + lt.sum() / Tt) / (2 * B))
print(f"fp32 training step, cfg 2 shape, ragged batch: valid fraction audio {float(la.sum()) / (B * Ta):.3f} text "
      f"{float(lt.sum()) / (B * Tt):.3f} mean {valid:.3f}", flush=True)

steps = {}
for mode in (("padded", "packed") if a.mode == "both" else (a.mode,)):
    H.set_varlen(mode == "packed")
    dp = DataParallelStep(m, fusion_step_loss, overlap=False)
    dp.set_global_batch(B)
    dp.step(*batch)
    dp.capture(*batch)
    for _ in range(3):
        dp.step(*batch)
    torch.cuda.synchronize()
    steps[mode] = dp
    print(f"{mode}: captured, loss {float(dp.step(*batch)):.6f}", flush=True)
H.set_varlen(False)

times = {k: [] for k in steps}
for r in range(a.rounds):
    for mode, dp in steps.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            dp.step(*batch)
        torch.cuda.synchronize()
        times[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
for mode, ts in times.items():
    print(f"{mode}: {statistics.median(ts):.3f} ms/step (median of {a.rounds} rounds of {a.steps} replays; rounds "
          f"{', '.join(f'{t:.3f}' for t in ts)})", flush=True)
if len(times) == 2:
    pad, pk = statistics.median(times["padded"]), statistics.median(times["packed"])
    print(f"packed / padded = {pk / pad:.3f} at valid fraction {valid:.3f}", flush=True)
for dp in steps.values():
    dp.release_graph()
