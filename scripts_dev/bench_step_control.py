"""What the step-control block of the captured ragged step costs and buys, in ONE process, rounds interleaved, by the method of
bench_step_packed.py: cfg 2 (B = 64, T_a = 400, T_t = 128, d = 768), bf16 inputs, dropout 0.1, valid fraction ~0.73, the host ->
device hand-over through data.DevicePrefetcher(ragged=...) from pinned host batches included, wall clock over `steps` calls per
round behind a synchronize, median of `rounds` rounds per arm, spread = (max - min) / median.  Every arm has DeviceAdamW as its
optimizer, and every bucket graph an arm needs is captured before the first timed round.

  1. the full-batch step
       P   capture_packed(optimizer=opt): the launches of the step as it was before the two options existed (memset,
           hriemo_fusion_loss, hriemo_optim_finalize)
       Q   capture_packed(optimizer=opt, partial_batches=True, grad_accum=2) and its group length then set to 1, so that EVERY call
           has first = last = 1: the work of P with hriemo_grad_begin in place of the memset, hriemo_fusion_loss_n and
           hriemo_optim_finalize_ctl, and the control block's upload
       Q2  the same capture left at grad_accum = 2 (an update every second call), per call
  2. an epoch's tail, a batch of B / 2 utterances
       T   the graph with ghosts (the step of Q)
       E   what there was before: use_graph(False), the eager forward_packed step + opt.step()
  3. grad_accum = 4, per group of four full micro-batches
       G   four step_packed calls of capture_packed(optimizer=opt, grad_accum=4)
       S   eager step_accumulated(pad_to=...) + opt.step()

usage: python scripts_dev/bench_step_control.py [rounds] [steps]"""
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
from hri_emo_amd.train import mosei_step_loss  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, TA, TT, D, NE, NBATCH = 64, 400, 128, 768, 6, 4
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)


def loss_k(k):
    def loss(logits, beta, y, n_valid=None):
        return mosei_step_loss(logits, beta, y, beta_entropy=0.01, grad_accum=k, n_valid=n_valid)
    return loss


def samples(seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(B):
        la = int(torch.randint(int(0.44 * TA), TA + 1, (1,), generator=g))
        lt = int(torch.randint(int(0.44 * TT), TT + 1, (1,), generator=g))
        out.append((torch.randn(la, D, generator=g), torch.zeros(la, dtype=torch.bool), torch.randn(lt, D, generator=g),
                    torch.zeros(lt, dtype=torch.bool), (torch.rand(NE, generator=g) < 0.3).float()))
    return out


def pin(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).contiguous().pin_memory()


def loader(n_utt):
    """NBATCH distinct ragged batches of the first n_utt utterances, bf16 features, pinned"""
    out = []
    for i in range(NBATCH):
        r_a, l_a, r_t, l_t, y = data.collate_seq_packed(samples(100 + i)[:n_utt])
        out.append((pin(r_a, torch.bfloat16), l_a, pin(r_t, torch.bfloat16), l_t, pin(y)))
    return out


def feed(items):
    return data.DevicePrefetcher(items, dev, convert=lambda t: (t[0], t[1].tolist(), t[2], t[3].tolist(), t[4]), ragged={0: B * TA, 2: B * TT})


def make(k, **kw):
    torch.manual_seed(1234)
    dp = DataParallelStep(H.FusionWithEmotionDecoder(**CFG).to(dev).train(), loss_k(k), overlap=False)
    dp.set_global_batch(B)
    opt = DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)
    return dp, opt, kw


def prepare(arm, items):
    dp, opt, kw = arm
    for i, (r_a, l_a, r_t, l_t, y) in enumerate(feed(items)):
        if i == 0 and not dp.captured:
            dp.capture_packed(r_a, r_t, l_a, l_t, y, pad_to=(TA, TT), optimizer=opt, **kw)
        dp.step_packed(r_a, r_t, l_a, l_t, y)
    dp.flush_accumulated()
    torch.cuda.synchronize()


def wall(fn, items, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(items)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / per * 1e3


def report(title, t, base, unit):
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    print(title)
    for k in t:
        d = "" if k == base else f"; {k} - {base} = {med[k] - med[base]:+.3f} ms"
        print(f"  {k:3s} {med[k]:.3f} ms per {unit} (spread {spread[k]:.4f} = {spread[k] * med[k]:.3f} ms){d}", flush=True)


H.set_varlen(True)
H.set_ingest(True)
_ops.PACKED_TAIL = True
print(f"bench_step_control: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, steps per round {STEPS}; cfg2 B={B} bf16 inputs, dropout 0.1, "
      f"hand-over included (wall clock), median of {ROUNDS}")
full, half = loader(B), loader(B // 2)
n_a, n_t = [int(b[1].sum()) for b in full], [int(b[3].sum()) for b in full]
print(f"valid fraction {(sum(n_a) / TA + sum(n_t) / TT) / (2 * B * NBATCH):.3f}, {NBATCH} distinct batches")
steps_full = [full[i % NBATCH] for i in range(STEPS)]
steps_half = [half[i % NBATCH] for i in range(STEPS)]


def stepper(arm):
    def run(items):
        for r_a, l_a, r_t, l_t, y in feed(items):
            arm[0].step_packed(r_a, r_t, l_a, l_t, y)
    return run


# ---- 1. the full-batch step
P, Q, Q2 = make(1), make(1, partial_batches=True, grad_accum=2), make(2, partial_batches=True, grad_accum=2)
for arm in (P, Q, Q2):
    prepare(arm, full)
Q[0]._pb.front.accum = 1            # groups of one on the graph captured for accumulation: first = last = 1 on every call
prepare(Q, half)                          # the tail's bucket graphs (arm T)
arms = {"P": stepper(P), "Q": stepper(Q), "Q2": stepper(Q2)}
for fn in arms.values():
    wall(fn, steps_full, STEPS)
t = {k: [] for k in arms}
for r in range(ROUNDS):
    for k, fn in arms.items():
        t[k].append(wall(fn, steps_full, STEPS))
    print(f"full batch: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + " ms/call", flush=True)
report(f"1. full batch, optimizer in the graph (bucket graphs P {len(P[0]._pb.graphs)} / Q {len(Q[0]._pb.graphs)})", t, "P", "call")

# ---- 2. an epoch's tail: B / 2 utterances
E = P
E[0].use_graph(False)
arms = {"E": stepper(E), "T": stepper(Q)}
for fn in arms.values():
    wall(fn, steps_half, STEPS)
t = {k: [] for k in arms}
for r in range(ROUNDS):
    for k, fn in arms.items():
        t[k].append(wall(fn, steps_half, STEPS))
    print(f"tail: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + " ms/call", flush=True)
report(f"2. a batch of {B // 2} utterances: eager forward_packed step + opt.step() (E) against the graph with ghosts (T)", t, "E", "call")
for arm in (P, Q, Q2):
    arm[0].release_graph()

# ---- 3. grad_accum = 4
G, S = make(4, grad_accum=4), make(1)
prepare(G, full)
groups = [[full[(4 * j + i) % NBATCH] for i in range(4)] for j in range(max(1, STEPS // 4))]


def run_g(items):
    for r_a, l_a, r_t, l_t, y in feed([b for grp in items for b in grp]):
        G[0].step_packed(r_a, r_t, l_a, l_t, y)


class Group:
    """k micro-batches drawn from the prefetcher one at a time (it lends out one batch: the ring reuses a set two batches later)"""

    def __init__(self, it, k):
        self.it, self.k = it, k

    def __len__(self):
        return self.k

    def __iter__(self):
        for _ in range(self.k):
            r_a, l_a, r_t, l_t, y = next(self.it)
            yield r_a, r_t, l_a, l_t, y


def run_s(items):
    it = iter(feed([b for grp in items for b in grp]))
    for grp in items:
        S[0].step_accumulated(Group(it, len(grp)), pad_to=(TA, TT))
        S[1].step()


arms = {"S": run_s, "G": run_g}
for fn in arms.values():
    wall(fn, groups, len(groups))
t = {k: [] for k in arms}
for r in range(ROUNDS):
    for k, fn in arms.items():
        t[k].append(wall(fn, groups, len(groups)))
    print(f"grad_accum 4: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + " ms/group", flush=True)
report("3. grad_accum = 4: eager step_accumulated + opt.step() (S) against four captured micro-steps (G)", t, "S", "group of 4")
G[0].release_graph()
