"""Epochs fed from a data.DeviceFeatureStore against epochs fed from the host, in ONE process, arms interleaved, by the method of
bench_epoch_stats.py: cfg 2 (B = 64, T_a = 400, T_t = 128, d = 768), bf16 rows, dropout 0.1, valid fraction ~0.72, DeviceAdamW in
the graph, every bucket graph captured before the first timed round; wall clock over `steps` calls per round behind a synchronize,
hand-over included, median of `rounds` rounds per arm, spread = (max - min) / median.

  A   the host-fed step: torch DataLoader over the in-memory samples (bf16, one process, no workers) with collate_seq_packed,
      data.DevicePrefetcher(ragged=...) and step_packed.  ONE loader and ONE prefetcher per arm, built and run through an epoch
      before the first timed round and iterated once per epoch, as a trainer does: the pinned ring and the device buffers are
      allocated once, outside every window
  B   store.batches(...) and step_store: the same utterances in the same batches, resident on the device

Per arm: ms per step; host CPU seconds per batch by time.process_time, taken from the first call of the round to the return of the
last one (the synchronize that closes the window is outside: a waiting host may spin).  Then the gather alone: HIP events around
the three hriemo_gather_rows launches of one batch, median of 20, against the bytes they read and write.  Then the same two arms for
the evaluation (EvalStep: eval_packed against eval_store) at B = 64 and B = 8.

usage: python scripts_dev/ab_store_step.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import data  # noqa: E402
from hri_emo_amd.dp import DataParallelStep, bucket_rows  # noqa: E402
from hri_emo_amd.optim import DeviceAdamW  # noqa: E402
from hri_emo_amd.train import mosei_step_loss  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 24
TA, TT, D, NE, NBATCH = 400, 128, 768, 6, 6
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)


def loss(logits, beta, y, n_valid=None):
    return mosei_step_loss(logits, beta, y, beta_entropy=0.01, n_valid=n_valid)


def corpus(n, seed=100):
    """n utterances in memory, bf16, every stored row valid; lengths uniform in [0.44 L, L]: valid fraction ~0.72"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        la = int(torch.randint(int(0.44 * TA), TA + 1, (1,), generator=g))
        lt = int(torch.randint(int(0.44 * TT), TT + 1, (1,), generator=g))
        out.append((torch.randn(la, D, generator=g).bfloat16(), torch.zeros(la, dtype=torch.bool), torch.randn(lt, D, generator=g).bfloat16(),
                    torch.zeros(lt, dtype=torch.bool), (torch.rand(NE, generator=g) < 0.3).float()))
    return out


def host_feed(samples, batches, B):
    loader = torch.utils.data.DataLoader(samples, batch_sampler=batches, collate_fn=data.collate_seq_packed, num_workers=0)
    return data.DevicePrefetcher(loader, dev, convert=lambda t: (t[0], t[1].tolist(), t[2], t[3].tolist(), t[4]), ragged={0: B * TA, 2: B * TT})


def trainer():
    torch.manual_seed(1234)
    dp = DataParallelStep(H.FusionWithEmotionDecoder(**CFG).to(dev).train(), loss, overlap=False)
    return dp, DeviceAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)


def timed(run, calls):
    """-> (ms per call, host CPU seconds per call)"""
    torch.cuda.synchronize()
    t0, c0 = time.perf_counter(), time.process_time()
    run()
    c1 = time.process_time()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3, (c1 - c0) / calls


def report(title, t, unit):
    print(title)
    out = {}
    for k, rounds in t.items():
        ms, cpu = [r[0] for r in rounds], [r[1] for r in rounds]
        med, cmed = statistics.median(ms), statistics.median(cpu)
        out[k] = (med, (max(ms) - min(ms)) / med, cmed)
        print(f"  {k}  {med:.3f} ms per {unit} (spread {(max(ms) - min(ms)) / med:.4f} = {max(ms) - min(ms):.3f} ms); host CPU {cmed * 1e3:.3f} ms per "
              f"batch (spread {(max(cpu) - min(cpu)) / max(cmed, 1e-12):.3f})", flush=True)
    d = out["B"][0] - out["A"][0]
    print(f"  B - A = {d:+.3f} ms per {unit}; A's own round-to-round spread {out['A'][1] * out['A'][0]:.3f} ms -> "
          + ("B is WORSE than A by more than A's spread" if d > out["A"][1] * out["A"][0] else "B is not worse than A beyond A's spread"), flush=True)
    return out


def ab(title, unit, arm_a, arm_b, epochs):
    t = {"A": [], "B": []}
    for r in range(ROUNDS):
        for k in (("A", "B") if r % 2 == 0 else ("B", "A")):
            t[k].append(timed(lambda: [(arm_a if k == "A" else arm_b)() for _ in range(epochs)], epochs * NBATCH))
    return report(title, t, unit)


def main():
    print(f"ab_store_step: rounds {ROUNDS}, steps per round {STEPS}, {torch.cuda.get_device_name(0)}")
    for B in (64, 8):
        samples = corpus(B * NBATCH)
        store = data.DeviceFeatureStore.from_samples(samples, dev)
        batches = store.batches(B, shuffle=False, bucket_mult=0)
        rows = (sum(store.lengths_a), sum(store.lengths_t))
        print(f"\nB = {B}: store of {len(store)} utterances, {store.nbytes / 1e6:.1f} MB, {store.dtype}, pad_to {store.pad_to}, valid fraction "
              f"{rows[0] / (len(store) * TA):.3f} / {rows[1] / (len(store) * TT):.3f}; {NBATCH} batches per epoch")
        epochs = max(1, STEPS // NBATCH)
        if B == 64:
            (dp_a, opt_a), (dp_b, opt_b) = trainer(), trainer()
            dp_a.set_global_batch(B)
            dp_b.set_global_batch(B)

            feed_a = host_feed(samples, batches, B)

            def train_a():
                for r_a, l_a, r_t, l_t, y in feed_a:
                    dp_a.step_packed(r_a, r_t, l_a, l_t, y)

            def train_b():
                for ids in batches:
                    dp_b.step_store(ids)

            r_a, l_a, r_t, l_t, y = next(iter(feed_a))
            dp_a.capture_packed(r_a, r_t, l_a, l_t, y, pad_to=(TA, TT), optimizer=opt_a)
            dp_b.capture_store(store, batches[0], pad_to=(TA, TT), optimizer=opt_b)
            train_a()
            train_b()
            torch.cuda.synchronize()
            assert list(dp_a._pb.graphs) == list(dp_b._pb.graphs)
            print(f"  {len(dp_a._pb.graphs)} bucket graphs per arm")
            ab("1. the train step (DeviceAdamW in the graph)", "step", train_a, train_b, epochs)
            # the gather alone
            ids = batches[0]
            la, lt = [store.lengths_a[i] for i in ids], [store.lengths_t[i] for i in ids]
            key = (bucket_rows(sum(la), B, TA), bucket_rows(sum(lt), B, TT))
            feed = dp_b._feed
            feed.block.upload(store.plan_words(ids, feed.stride))
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
            for a, b in ev:
                a.record()
                store.gather_into(feed.block.dev, feed.stride, len(ids), dp_b._static[0], key[0], dp_b._static[1], key[1], dp_b._static[4])
                b.record()
            torch.cuda.synchronize()
            us = statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3
            moved = 2 * 2 * D * (sum(la) + sum(lt)) + 2 * D * (key[0] - sum(la) + key[1] - sum(lt)) + 2 * 4 * NE * B
            print(f"2. the gather of one batch (three launches, {sum(la)} + {sum(lt)} rows, buckets {key}): {us:.1f} us for {moved / 1e6:.1f} MB read + "
                  f"written = {moved / us / 1e6:.2f} TB/s; the plan block is {feed.block.host.numel() * 4} bytes, the lengths block {2 * B * 4}")
            dp_a.release_graph()
            dp_b.release_graph()
        torch.manual_seed(1234)
        model = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
        ev_a, ev_b = H.EvalStep(model, loss), H.EvalStep(model, loss)

        feed_e = host_feed(samples, batches, B)

        def eval_a():
            for r_a, l_a, r_t, l_t, y in feed_e:
                ev_a.eval_packed(r_a, r_t, l_a, l_t, y)

        def eval_b():
            for ids in batches:
                ev_b.eval_store(ids)

        r_a, l_a, r_t, l_t, y = next(iter(feed_e))
        ev_a.capture_packed(r_a, r_t, l_a, l_t, y, pad_to=(TA, TT))
        ev_b.capture_store(store, batches[0], pad_to=(TA, TT))
        eval_a()
        eval_b()
        torch.cuda.synchronize()
        ab(f"3. the evaluation at B = {B} (forward + loss in the graph)", "batch", eval_a, eval_b, epochs)
        ev_a.release_graph()
        ev_b.release_graph()


if __name__ == "__main__":
    main()
