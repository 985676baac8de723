"""hriemo_gather_rows_aug against the plain hriemo_gather_rows, in ONE process on ONE plan, arms interleaved, by the method of
ab_store_step.py: cfg 2's batch (B = 64, T_a = 400, T_t = 128, d = 768, bf16 rows, valid fraction ~0.72).

1. the gathers of one batch alone -- HIP events around `REPS` back-to-back gathers of the batch (audio, text, targets) into the
   static sources of a captured step, per round; median of `rounds` rounds per arm, spread = (max - min) / median:
     plain   three hriemo_gather_rows launches
     a       spans + modality drop, no per-element hash
     b       noise only (one mix24 per element)
     c       all three transforms
2. the captured train step (DeviceAdamW in the graph) on store.batches: step_store without an augment against step_store with (c),
   wall clock per step behind a synchronize, the same interleaving.

usage: python scripts_dev/bench_store_augment.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ab_store_step import CFG, D, NBATCH, NE, TA, TT, corpus, dev, loss  # noqa: E402
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import data  # noqa: E402
from hri_emo_amd.dp import DataParallelStep, bucket_rows  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 24
REPS = 20
B = 64
TM = dict(spans=2, max_width=40, max_frac=0.2)
ARMS = {"plain": None,
        "a": dict(time_mask=TM, modality_drop=(0.1, 0.1)),
        "b": dict(noise_std=(0.05, 0.05)),
        "c": dict(time_mask=TM, noise_std=(0.05, 0.05), modality_drop=(0.1, 0.1))}


def trainer():
    torch.manual_seed(1234)
    dp = DataParallelStep(H.FusionWithEmotionDecoder(**CFG).to(dev).train(), loss, overlap=False)
    dp.set_global_batch(B)
    return dp, DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)


def summary(title, t, unit, base):
    print(title)
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        print(f"  {k:6s} {med[k]:9.3f} {unit} (spread {(max(v) - min(v)) / med[k]:.4f} = {max(v) - min(v):.3f} {unit}); x {med[k] / med[base]:.3f} of {base}",
              flush=True)
    return med


def main():
    print(f"bench_store_augment: rounds {ROUNDS}, steps per round {STEPS}, {torch.cuda.get_device_name(0)}")
    samples = corpus(B * NBATCH)
    store = data.DeviceFeatureStore.from_samples(samples, dev)
    batches = store.batches(B, shuffle=False, bucket_mult=0)
    augs = {k: None if kw is None else data.StoreAugment(1234, **kw) for k, kw in ARMS.items()}
    (dp_p, opt_p), (dp_c, opt_c) = trainer(), trainer()
    dp_p.capture_store(store, batches[0], pad_to=(TA, TT), optimizer=opt_p)
    dp_c.capture_store(store, batches[0], pad_to=(TA, TT), optimizer=opt_c, augment=augs["c"])
    for dp in (dp_p, dp_c):
        for ids in batches:
            dp.step_store(ids)
    torch.cuda.synchronize()
    print(f"store of {len(store)} utterances, {store.nbytes / 1e6:.1f} MB, {store.dtype}; {len(dp_p._pb.graphs)} / {len(dp_c._pb.graphs)} bucket graphs")

    # 1. the gathers alone, on the plan of batch 0
    ids = batches[0]
    la, lt = [store.lengths_a[i] for i in ids], [store.lengths_t[i] for i in ids]
    key = (bucket_rows(sum(la), B, TA), bucket_rows(sum(lt), B, TT))
    feed, static = dp_p._feed, dp_p._static
    feed.block.upload(store.plan_words(ids, feed.stride))
    moved = 2 * 2 * D * (sum(la) + sum(lt)) + 2 * D * (key[0] - sum(la) + key[1] - sum(lt)) + 2 * 4 * NE * B

    def gathers(aug):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r in range(REPS):
            store.gather_into(feed.block.dev, feed.stride, len(ids), static[0], key[0], static[1], key[1], static[4], aug, r)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / REPS

    for aug in augs.values():
        gathers(aug)
    t = {k: [] for k in ARMS}
    order = list(ARMS)
    for r in range(ROUNDS):
        for k in (order if r % 2 == 0 else order[::-1]):
            t[k].append(gathers(augs[k]))
    med = summary(f"1. the gathers of one batch ({sum(la)} + {sum(lt)} rows, buckets {key}, {moved / 1e6:.1f} MB read + written by the plain copy), "
                  f"us per batch over {REPS} back-to-back batches", t, "us", "plain")
    print("  plain: %.2f TB/s" % (moved / med["plain"] / 1e6))

    # 2. the captured step
    epochs = max(1, STEPS // NBATCH)
    t = {"plain": [], "c": []}
    for r in range(ROUNDS):
        for k in (("plain", "c") if r % 2 == 0 else ("c", "plain")):
            dp = dp_p if k == "plain" else dp_c
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(epochs):
                for ids in batches:
                    dp.step_store(ids)
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / (epochs * NBATCH) * 1e3)
    ms = summary("2. the captured train step, step_store (DeviceAdamW in the graph), ms per step", t, "ms", "plain")
    print(f"  share of the step: plain gathers {med['plain'] / ms['plain'] / 10:.2f} %, gathers of (c) {med['c'] / ms['c'] / 10:.2f} %; "
          f"c - plain = {(ms['c'] - ms['plain']) * 1e3:+.1f} us per step against {(med['c'] - med['plain']):+.1f} us of gather time")
    dp_p.release_graph()
    dp_c.release_graph()


if __name__ == "__main__":
    main()
