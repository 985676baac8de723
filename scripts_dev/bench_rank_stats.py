"""What the ranking metrics cost on the device and what they save against the reference's habit, and what confusion=True costs inside
the captured single-label step; ONE process, arms interleaved, median of `rounds` rounds, spread = (max - min) / median.

  1. ranking metrics over a log of n samples, C = 6, n = 1871 / 4662 / 16326 (MOSEI val / test / train) and 65536.  The log is
     written directly (sigmoid of 2 randn + 1.5 on the positives, 30 % positives, cursor = n): the kernels read nothing else.
       K   hriemo_stats_rank alone, and hriemo_stats_rank + hriemo_stats_auc, HIP events around the launches
       R   EpochStats.ranking() as a whole: the two launches, the read-backs, average precision per class in float64
       D   ranking() plus pr_curve() of every class on that result (host arithmetic): what the host arm below produces
       H   what the reference does today (scripts/infer/mosei_plot_metrics.py): probs.cpu() / truth.cpu() of the log, then
           sklearn's average_precision_score and precision_recall_curve per class.  Without sklearn on the machine: a numpy sort +
           cumulative-sum form of the same two results; the script says which one ran.
     No bar.
  2. the captured single-label step (FusionClassifier, d = 768, pad_to = (400, 128), dropout 0.2, DeviceAdamW in the graph) through
     step_packed at B = 8 and B = 64:
       P   attach_stats(EpochStats(kind="single_label"))
       A   the same with confusion=True: one more one-block launch per replay
     Reported, not judged: A - P beside P's own round-to-round spread of this run (the script prints whether it lies within).

usage: python scripts_dev/bench_rank_stats.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops, data  # noqa: E402
from hri_emo_amd.dp import DataParallelStep  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW  # noqa: E402
from hri_emo_amd.train import EpochStats, fusion_step_loss_single_label  # noqa: E402

try:
    from sklearn.metrics import average_precision_score, precision_recall_curve
    HOST = "sklearn"
except ImportError:
    HOST = "numpy (sort + cumulative sums; sklearn is not installed here)"

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 24
NE = 6


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m if m else 0.0


# ---------------------------------------------------------------------------------------------------------------- 1. ranking
def filled(n):
    st = EpochStats(NE, n)
    g = torch.Generator().manual_seed(n)
    t = torch.rand(NE, n, generator=g) < 0.3
    x = 2.0 * torch.randn(NE, n, generator=g) + 1.5 * t.float()
    st.probs.copy_(torch.sigmoid(x))
    st.truth.copy_(t.to(torch.uint8))
    st.counters[0], st.counters[1] = n, n
    return st


def numpy_host(p, t):
    """average precision and the PR curve of one class by a descending sort and cumulative sums (the stand-in for sklearn)"""
    order = np.argsort(-p, kind="stable")
    ps, ts = p[order], t[order]
    last = np.r_[np.flatnonzero(np.diff(ps)), ps.size - 1]
    tp = np.cumsum(ts)[last].astype(np.float64)
    fp = (1 + last) - tp
    precision, recall = tp / (tp + fp), tp / max(1.0, tp[-1])
    ap = float(np.sum(np.diff(np.r_[0.0, recall]) * precision))
    return ap, (np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0], ps[last][::-1])


def host_arm(st, n):
    p, t = st.probs[:, :n].cpu().numpy(), st.truth[:, :n].cpu().numpy() != 0
    out = []
    for c in range(NE):
        if HOST == "sklearn":
            out.append((average_precision_score(t[c], p[c]), precision_recall_curve(t[c], p[c])))
        else:
            out.append(numpy_host(p[c], t[c]))
    return out


def device_arm(st):
    rk = st.ranking()
    return rk, [st.pr_curve(c, rk) for c in range(NE)]


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def ranking_arms(n):
    st = filled(n)
    p = _ops._p
    st.ranking()                                             # allocates the rank block; warm-up of both launches

    def k_rank():
        _lib.call("hriemo_stats_rank", p(st.probs), p(st.truth), n, NE, p(st.counters), p(st._rank), _ops._stream())

    def k_both():
        k_rank()
        _lib.call("hriemo_stats_auc", p(st.probs), p(st.truth), n, NE, p(st.counters), p(st._partial), p(st._npn), _ops._stream())

    host_arm(st, n)
    t = {"K rank": [], "K rank+auc": [], "R ranking()": [], "D ranking()+curves": [], "H host": []}
    for r in range(ROUNDS):
        t["K rank"].append(events(k_rank))
        t["K rank+auc"].append(events(k_both))
        t["R ranking()"].append(wall(st.ranking)[0])
        d, (rk, curves) = wall(lambda: device_arm(st))
        h, ref = wall(lambda: host_arm(st, n))
        t["D ranking()+curves"].append(d)
        t["H host"].append(h)
    worst = max(abs(float(rk["average_precision"][c]) - float(ref[c][0])) for c in range(NE))
    same = all(len(curves[c][0]) == len(ref[c][1][0]) and float(np.abs(curves[c][0] - ref[c][1][0]).max()) <= 1e-12 for c in range(NE))
    print(f"1. n = {n}, C = {NE}: host arm = {HOST}")
    for k, v in t.items():
        m, s = med_spread(v)
        print(f"  {k:20s} {m:9.3f} ms (spread {s:.3f}, min {min(v):.3f})", flush=True)
    pairs = 2.0 * NE * n * n
    m = statistics.median(t["K rank"])
    print(f"  rank kernel: {pairs / (m * 1e-3) / 1e12:.2f} T comparisons/s; AP device vs host: largest difference {worst:.2e}; PR curves equal: {same}", flush=True)


# ---------------------------------------------------------------------------------------------------------------- 2. the step
TA, TT, D, NC, NBATCH = 400, 128, 768, 4, 6


def loss(logits, beta, y, n_valid=None):
    return fusion_step_loss_single_label(logits, beta, y, n_valid=n_valid)


def corpus(n, seed=100):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        la = TA if i == 0 else int(torch.randint(int(0.44 * TA), TA + 1, (1,), generator=g))
        lt = TT if i == 0 else int(torch.randint(int(0.44 * TT), TT + 1, (1,), generator=g))
        out.append((torch.randn(la, D, generator=g).bfloat16(), torch.zeros(la, dtype=torch.bool), torch.randn(lt, D, generator=g).bfloat16(),
                    torch.zeros(lt, dtype=torch.bool), int(torch.randint(0, NC, (1,), generator=g))))
    return out


def step_arms(B):
    store = data.DeviceFeatureStore.from_samples(corpus(B * NBATCH), dev, loss_type="single_label")
    fetched = []
    for ids in store.batches(B, shuffle=False, bucket_mult=0):
        ra, la, rt, lt, y = store.fetch(ids)
        fetched.append((ra, rt, la, lt, y))
    epochs = max(1, STEPS // NBATCH)
    arms = {}
    for k, confusion in (("P", False), ("A", True)):
        torch.manual_seed(1234)
        dp = DataParallelStep(H.FusionClassifier(D, NC, 8, 2, 256, dropout=0.2).to(dev).train(), loss, overlap=False)
        dp.set_global_batch(B)
        opt = DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)
        st = EpochStats(NC, 1, kind="single_label", confusion=confusion)
        dp.attach_stats(st)
        dp.capture_packed(*fetched[0], pad_to=(TA, TT), optimizer=opt)
        arms[k] = (dp, st)

    def run(k):
        dp = arms[k][0]
        for _ in range(epochs):
            for b in fetched:
                dp.step_packed(*b)

    for k in arms:
        run(k)                                               # every bucket graph is captured before the first timed round
    t = {k: [] for k in arms}
    for r in range(ROUNDS):
        for k in (("P", "A") if r % 2 == 0 else ("A", "P")):
            arms[k][1].reset()
            t[k].append(wall(lambda: run(k))[0] / (epochs * NBATCH))
    res = arms["A"][1].result()
    assert res["n_samples"] == epochs * NBATCH * B and int(res["confusion"].sum()) == res["n_samples"], res
    mp, sp = med_spread(t["P"])
    ma, sa = med_spread(t["A"])
    inside = abs(ma - mp) <= sp * mp
    print(f"2. captured single-label step_packed, B = {B}, {len(arms['P'][0]._pb.graphs)} bucket graphs, {epochs * NBATCH} calls per round")
    print(f"  P  {mp:.3f} ms per call (spread {sp:.4f} = {sp * mp:.3f} ms)")
    print(f"  A  {ma:.3f} ms per call (spread {sa:.4f} = {sa * ma:.3f} ms); A - P = {ma - mp:+.3f} ms: {'within' if inside else 'OUTSIDE'} P's spread", flush=True)
    for dp, _ in arms.values():
        dp.release_graph()


def main():
    print(f"bench_rank_stats: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, steps per round {STEPS}")
    for n in (1871, 4662, 16326, 65536):
        ranking_arms(n)
    for B in (8, 64):
        step_arms(B)


if __name__ == "__main__":
    main()
