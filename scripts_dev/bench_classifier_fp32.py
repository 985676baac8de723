"""FusionClassifier in the fp32 precision mode, sequence level (d = 768, pad_to = (400, 128), dropout 0.2, valid fraction ~0.72,
single-label loss), in ONE process, arms interleaved, by the method of bench_classifier_step.py: wall clock over `steps` calls per round
behind a synchronize, median of `rounds` rounds per arm, spread = (max - min) / median.  set_precision("fp32"),
set_pooled_gate_fp32(True).

  1. the trainer step at B = 8 and B = 64
       A   eager padded: forward(padded batch, masks) as the path of record runs it (_fp32.beta_gate, h_fusion [B, L, d], torch's mean),
           the loss, backward, DeviceAdamW.step()
       B   step_store: the captured ragged step (_fp32.pooled_gate on hriemo_pool32_*, DeviceAdamW in the graph) on a DeviceFeatureStore
  2. the gate-plus-pool segment alone, eager launches, forward + backward on fp32 encoder outputs, device events, at B = 64 and B = 8
       A   BetaGateFn (h_fusion [B, L, d]) + h_fusion.mean(1)
       B   PooledGateFn
  3. one batch in eval mode: max |pooled_A - pooled_B| and max |beta_A - beta_B|

usage: python scripts_dev/bench_classifier_fp32.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _ops, data  # noqa: E402
from hri_emo_amd.dp import DataParallelStep  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW  # noqa: E402
from hri_emo_amd.train import fusion_step_loss_single_label  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
TA, TT, D, NC, NBATCH = 400, 128, 768, 4, 6


def loss(logits, beta, y, n_valid=None):
    return fusion_step_loss_single_label(logits, beta, y, n_valid=n_valid)


def corpus(n, seed=100):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        la = TA if i == 0 else int(torch.randint(int(0.44 * TA), TA + 1, (1,), generator=g))
        lt = TT if i == 0 else int(torch.randint(int(0.44 * TT), TT + 1, (1,), generator=g))
        out.append((torch.randn(la, D, generator=g), torch.zeros(la, dtype=torch.bool), torch.randn(lt, D, generator=g),
                    torch.zeros(lt, dtype=torch.bool), int(torch.randint(0, NC, (1,), generator=g))))
    return out


def trainer():
    torch.manual_seed(1234)
    dp = DataParallelStep(H.FusionClassifier(D, NC, 8, 2, 256, dropout=0.2).to(dev).train(), loss, overlap=False)
    return dp, DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)


def timed(run, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def ab(title, unit, arm_a, arm_b, calls):
    t = {"A": [], "B": []}
    for r in range(ROUNDS):
        for k in (("A", "B") if r % 2 == 0 else ("B", "A")):
            t[k].append(timed(arm_a if k == "A" else arm_b, calls))
    print(title)
    med = {}
    for k, ms in t.items():
        med[k] = statistics.median(ms)
        print(f"  {k}  {med[k]:.3f} ms per {unit} (spread {(max(ms) - min(ms)) / med[k]:.4f} = {max(ms) - min(ms):.3f} ms)", flush=True)
    print(f"  B - A = {med['B'] - med['A']:+.3f} ms per {unit}; A / B = {med['A'] / med['B']:.2f}x", flush=True)


def step_arms(B):
    samples = corpus(B * NBATCH)
    store = data.DeviceFeatureStore.from_samples(samples, dev, loss_type="single_label")
    batches = store.batches(B, shuffle=False, bucket_mult=0)
    padded = []
    for ids in batches:
        h_a, m_a, h_t, m_t, y = data.collate_seq_batch([samples[i] for i in ids], loss_type="single_label", pad_to=(TA, TT))
        padded.append(tuple(t.to(dev) for t in (h_a, h_t, m_a, m_t, y)))
    valid = sum(s[0].shape[0] + s[2].shape[0] for s in samples) / (len(samples) * (TA + TT))
    (dp_a, opt_a), (dp_b, opt_b) = trainer(), trainer()
    dp_a.set_global_batch(B)
    dp_b.set_global_batch(B)
    epochs = max(1, STEPS // NBATCH)

    def train_a():
        for _ in range(epochs):
            for b in padded:
                dp_a.step(*b)
                opt_a.step()

    def train_b():
        for _ in range(epochs):
            for ids in batches:
                dp_b.step_store(ids)

    dp_b.capture_store(store, batches[0], pad_to=(TA, TT), optimizer=opt_b)
    train_a()
    train_b()
    torch.cuda.synchronize()
    print(f"\nB = {B}: {len(store)} utterances, valid fraction {valid:.3f}, {NBATCH} batches per epoch, {len(dp_b._pb.graphs)} bucket graphs")
    ab(f"1. the fp32 trainer step at B = {B}: A eager padded forward() + opt.step(), B step_store (fp32 pooled gate, optimizer in the graph)",
       "step", train_a, train_b, epochs * NBATCH)
    dp_b.release_graph()
    if B == 8:                                   # 3. both tails on one batch, eval mode
        m = dp_a.module if hasattr(dp_a, "module") else dp_a.model
        m.eval()
        ra, la, rt, lt, _ = store.fetch(batches[0])
        with torch.no_grad():
            out_a = m(*padded[0][:4])
            out_b = m.forward_packed(ra, rt, la, lt, pad_to=(TA, TT))
        m.train()
        print(f"3. eval, one batch of {B}: max |pooled_A - pooled_B| = {float((out_a[2] - out_b[2]).abs().max()):.3e} (max |pooled| "
              f"{float(out_b[2].abs().max()):.3f}), max |beta_A - beta_B| = {float((out_a[1] - out_b[1]).abs().max()):.3e}", flush=True)


def gate_arms(B):
    torch.manual_seed(7)
    m = H.FusionClassifier(D, NC, 8, 2, 256, dropout=0.0).to(dev).train()
    g = m.beta_gate
    a32 = torch.randn(B, TA, D, device=dev)
    t32 = torch.randn(B, TT, D, device=dev)
    la = torch.randint(int(0.44 * TA), TA + 1, (B,))
    lt = torch.randint(int(0.44 * TT), TT + 1, (B,))
    ma = (torch.arange(TA)[None] >= la[:, None]).to(dev)
    mt = (torch.arange(TT)[None] >= lt[:, None]).to(dev)
    gp = torch.randn(B, D, device=dev)
    seqs = (_ops.Seq.padded(B, TA), _ops.Seq.padded(B, TT), _ops.Seq.padded(B, TT))
    xs = (a32.bfloat16(), a32.clone().requires_grad_(True), t32.bfloat16(), t32.clone().requires_grad_(True))
    n = 20

    def old():
        for _ in range(n):
            hf, beta = g._fwd_pair(*xs, ma, mt, seqs)
            pooled = hf.float().mean(dim=1)
            torch.autograd.backward([pooled, beta], [gp, torch.ones_like(beta)])

    def new():
        for _ in range(n):
            pooled, beta = _ops.PooledGateFn.apply(*xs, g.norm_a.weight, g.norm_a.bias, g.norm_t.weight, g.norm_t.bias, g.mlp[0].weight, g.mlp[0].bias,
                                                   g.mlp[2].weight, g.mlp[2].bias, g._sh, _ops.Seq.padded(B, TA, ma), _ops.Seq.padded(B, TT, mt))
            torch.autograd.backward([pooled, beta], [gp, torch.ones_like(beta)])

    def events(run):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    old()
    new()
    t = {"A": [], "B": []}
    for r in range(ROUNDS):
        for k in (("A", "B") if r % 2 == 0 else ("B", "A")):
            t[k].append(events(old if k == "A" else new))
    print(f"2. fp32 gate + pool, forward + backward, eager launches, B = {B}: device time between events, us per call")
    for k, us in t.items():
        med = statistics.median(us)
        print(f"  {k}  {med:.1f} us (spread {(max(us) - min(us)) / med:.3f})", flush=True)
    print(f"  B - A = {statistics.median(t['B']) - statistics.median(t['A']):+.1f} us", flush=True)


def main():
    H.set_precision("fp32")
    H.set_pooled_gate_fp32(True)
    print(f"bench_classifier_fp32: precision {H.precision()}, rounds {ROUNDS}, steps per round {STEPS}, {torch.cuda.get_device_name(0)}", flush=True)
    for B in (8, 64):
        step_arms(B)
    for B in (64, 8):
        gate_arms(B)


if __name__ == "__main__":
    main()
