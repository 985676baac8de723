"""What the epoch statistics cost inside the captured ragged step and what they save against reading back, in ONE process, rounds
interleaved, by the method of bench_step_control.py: cfg 2 (B = 64, T_a = 400, T_t = 128, d = 768), bf16 inputs, dropout 0.1, valid
fraction ~0.73, hand-over through data.DevicePrefetcher(ragged=...) from pinned host batches included, wall clock over `steps`
calls per round behind a synchronize, median of `rounds` rounds per arm, spread = (max - min) / median.  Every arm has DeviceAdamW
in the graph, and every bucket graph an arm needs is captured before the first timed round.

  1. the train step
       P   capture_packed(optimizer=opt), no statistics: the step as it is without attach_stats
       A   the same with attach_stats(EpochStats): one more one-block launch per replay; result() once per round, outside the window
           The bar: |A - P| within P's own round-to-round spread of this run.
  2. the reference's habit on the same epoch
       R   the step of P, and after every replay loss.item(), logits.cpu(), beta.cpu() (the logits / beta buffers of the replayed
           bucket graph, kept from its capture pass by a wrapper around the loss function).  No bar.
  3. the epoch kernels: hriemo_stats_counts + hriemo_stats_auc over a log of N = 2 000 and N = 16 000 entries (C = 6, 20
     thresholds), HIP events around the two launches, median of 10; and result() as a whole (launches, the read-back, the float64
     ratios), wall clock.  No bar.
  4. validation: train.evaluate_packed over `steps` batches + result() against an eager loop that reads loss.item(), logits.cpu(),
     beta.cpu() per batch (the reference's evaluate(); its sklearn metrics on the host afterwards are NOT included).  No bar.

usage: python scripts_dev/bench_epoch_stats.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops, data  # noqa: E402
from hri_emo_amd.dp import DataParallelStep  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW  # noqa: E402
from hri_emo_amd.train import EpochStats, evaluate_packed, mosei_step_loss, thresholds_up, SWEEP  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, TA, TT, D, NE, NBATCH = 64, 400, 128, 768, 6, 4
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)


def loss(logits, beta, y, n_valid=None):
    return mosei_step_loss(logits, beta, y, beta_entropy=0.01, n_valid=n_valid)


class KeepOutputs:
    """the loss function of arm R: remembers the logits / beta tensors of the latest pass (of a capture pass: the graph's own buffers)"""

    def __init__(self):
        self.last = None

    def __call__(self, logits, beta, y, n_valid=None):
        self.last = (logits.detach(), beta.detach())
        return loss(logits, beta, y, n_valid=n_valid)


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


def loader():
    out = []
    for i in range(NBATCH):
        r_a, l_a, r_t, l_t, y = data.collate_seq_packed(samples(100 + i))
        out.append((pin(r_a, torch.bfloat16), l_a, pin(r_t, torch.bfloat16), l_t, pin(y)))
    return out


def feed(items):
    return data.DevicePrefetcher(items, dev, convert=lambda t: (t[0], t[1].tolist(), t[2], t[3].tolist(), t[4]), ragged={0: B * TA, 2: B * TT})


def make(loss_fn, stats=None):
    torch.manual_seed(1234)
    dp = DataParallelStep(H.FusionWithEmotionDecoder(**CFG).to(dev).train(), loss_fn, overlap=False)
    dp.set_global_batch(B)
    if stats is not None:
        dp.attach_stats(stats)
    return dp, DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)


def prepare(arm, items, keep=None, by_graph=None):
    dp, opt = arm
    for i, (r_a, l_a, r_t, l_t, y) in enumerate(feed(items)):
        if i == 0:
            dp.capture_packed(r_a, r_t, l_a, l_t, y, pad_to=(TA, TT), optimizer=opt)
        dp.step_packed(r_a, r_t, l_a, l_t, y)
        if keep is not None:
            by_graph.setdefault(next(reversed(dp._pb.graphs)), keep.last)      # a bucket met first: keep.last is its capture pass
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
    return med, spread


H.set_varlen(True)
H.set_ingest(True)
_ops.PACKED_TAIL = True
print(f"bench_epoch_stats: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, steps per round {STEPS}; cfg2 B={B} bf16 inputs, dropout 0.1, "
      f"hand-over included (wall clock), median of {ROUNDS}")
full = loader()
steps_full = [full[i % NBATCH] for i in range(STEPS)]

# ---- 1. + 2. the train step
stats = EpochStats(NE, STEPS * B, skip_nonfinite=True)
keep, by_graph = KeepOutputs(), {}
P, A, R = make(loss), make(loss, stats), make(keep)
prepare(P, full)
prepare(A, full)
prepare(R, full, keep, by_graph)


def stepper(arm):
    def run(items):
        for r_a, l_a, r_t, l_t, y in feed(items):
            arm[0].step_packed(r_a, r_t, l_a, l_t, y)
    return run


def run_r(items):
    dp = R[0]
    total, betas, logs = 0.0, [], []
    for r_a, l_a, r_t, l_t, y in feed(items):
        l = dp.step_packed(r_a, r_t, l_a, l_t, y)
        logits, beta = by_graph[next(reversed(dp._pb.graphs))]
        total += l.item() * B
        betas.extend(beta.float().cpu().view(-1).tolist())
        logs.append(logits.cpu())


arms = {"P": stepper(P), "A": stepper(A), "R": run_r}
for fn in arms.values():
    wall(fn, steps_full, STEPS)
t = {k: [] for k in arms}
t_result = []
for r in range(ROUNDS):
    stats.reset()
    for k, fn in arms.items():
        t[k].append(wall(fn, steps_full, STEPS))
    t0 = time.perf_counter()
    res = stats.result()
    t_result.append((time.perf_counter() - t0) * 1e3)
    assert res["n_batches"] == STEPS and res["n_samples"] == STEPS * B, res
    print(f"train step: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + f" ms/call; result() {t_result[-1]:.3f} ms", flush=True)
med, spread = report(f"1. / 2. cfg 2 ragged captured step, optimizer in the graph ({len(P[0]._pb.graphs)} bucket graphs): no statistics (P), "
                     "attach_stats (A), read-back of loss / logits / beta per replay (R)", t, "P", "call")
inside = abs(med["A"] - med["P"]) <= spread["P"] * med["P"]
print(f"  |A - P| = {abs(med['A'] - med['P']):.3f} ms, P's spread {spread['P'] * med['P']:.3f} ms: {'within' if inside else 'OUTSIDE'} the spread")
print(f"  result() of a {STEPS * B}-sample epoch: median {statistics.median(t_result):.3f} ms (once per epoch)")
for arm in (P, A, R):
    arm[0].release_graph()

# ---- 3. the epoch kernels
thr = torch.from_numpy(thresholds_up([0.5] + list(SWEEP))).to(dev)
for N in (2000, 16000):
    st = EpochStats(NE, N)
    g = torch.Generator().manual_seed(N)
    for lo in range(0, N, 1000):
        x = (2.0 * torch.randn(1000, NE, generator=g)).to(dev)
        st.update(x, None, ((torch.rand(1000, NE, generator=g) < 0.3).float()).to(dev), torch.ones((), device=dev))
    ev = []
    p = _ops._p
    for _ in range(11):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call("hriemo_stats_counts", p(st.probs), p(st.truth), N, NE, p(st.counters), p(thr), 20, p(st._counts), _ops._stream())
        _lib.call("hriemo_stats_auc", p(st.probs), p(st.truth), N, NE, p(st.counters), p(st._partial), p(st._npn), _ops._stream())
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    w = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = st.result()
        w.append((time.perf_counter() - t0) * 1e3)
    print(f"3. N = {N}: counts + auc kernels {statistics.median(ev[1:]):.3f} ms (HIP events, median of 10, min {min(ev[1:]):.3f}); "
          f"result() {statistics.median(w):.3f} ms wall; macro_auc {res['macro_auc']:.4f}, n_logged {res['n_logged']}", flush=True)

# ---- 4. validation
torch.manual_seed(1234)
model = H.FusionWithEmotionDecoder(**CFG).to(dev)
vstats = EpochStats(NE, STEPS * B)


def run_v(items):
    vstats.reset()
    evaluate_packed(model, items, loss, vstats, pad_to=(TA, TT)).result()


def run_e(items):
    model.eval()
    total, betas, logs = 0.0, [], []
    with torch.no_grad():
        for r_a, l_a, r_t, l_t, y in items:
            y = y.to(dev, non_blocking=True)
            logits, beta, _ = model.forward_packed(r_a.to(dev, non_blocking=True), r_t.to(dev, non_blocking=True), l_a, l_t, pad_to=(TA, TT))
            total += loss(logits, beta, y).item() * B
            betas.extend(beta.float().cpu().view(-1).tolist())
            logs.append(logits.cpu())


arms = {"E": run_e, "V": run_v}
for fn in arms.values():
    wall(fn, steps_full, STEPS)
t = {k: [] for k in arms}
for r in range(ROUNDS):
    for k, fn in arms.items():
        t[k].append(wall(fn, steps_full, STEPS))
    print(f"validation: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + " ms/batch", flush=True)
report("4. validation, eager forward_packed per batch: loss.item() / logits.cpu() / beta.cpu() per batch (E) against evaluate_packed + "
       "result() (V)", t, "E", "batch")
