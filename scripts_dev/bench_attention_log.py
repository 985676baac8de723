"""What the attention log costs inside the captured evaluation, in ONE process, rounds interleaved: cfg 2 (T_a = 400, T_t = 128,
d = 768) at B = 64 and at B = 8 (the default batch of the reference's scripts/infer/mosei_eval_infer.py), bf16 inputs, valid
fraction ~0.72, the host -> device hand-over through data.DevicePrefetcher(ragged=...) from pinned host batches included.

  a  dp.EvalStep without a log                                  -- the path from before the log: the baseline
  b  dp.EvalStep(attn_log=...), the log takes EVERY batch       -- capacity B, the cursor reset in front of each replay
  c  dp.EvalStep(attn_log=...), the log is FULL                 -- every export block reads the window and exits
  d  what the reference's driver does with --dump_attn          -- eager forward_packed(return_attention=True) and a per-batch
                                                                   .cpu() of every map

Every arm computes the loss and feeds an EpochStats (reset per round).  An "epoch" is `steps` batches, timed by a pair of device
events around it AND by the wall clock behind a synchronize; medians of `rounds` rounds per arm and every arm's own round-to-round
spread (max - min) / median.  Every bucket graph the loader needs is captured before the first timed round.  Reported: c - a
against a's own spread (the claim: inside it), b - a (the price of the maps themselves, roughly their HBM write), b against d.

usage: python scripts_dev/bench_attention_log.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _ops, data  # noqa: E402
from hri_emo_amd.train import AttentionLog, EpochStats, fusion_step_loss  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 24
TA, TT, D, NE, NBATCH = 400, 128, 768, 6, 4
PAD = (TA, TT)
CFG = dict(d_model=D, num_emotions=NE, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256, dropout=0.1)


def samples(B, seed):
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


def loader(B):
    """NBATCH distinct ragged batches, bf16 features, pinned (what a DataLoader with pin_memory=True hands over)"""
    out = []
    for i in range(NBATCH):
        r_a, l_a, r_t, l_t, y = data.collate_seq_packed(samples(B, 100 + i))
        out.append((pin(r_a, torch.bfloat16), l_a, pin(r_t, torch.bfloat16), l_t, pin(y)))
    return out


def run(B):
    rag = loader(B)
    frac = (sum(int(b[1].sum()) for b in rag) / TA + sum(int(b[3].sum()) for b in rag) / TT) / (2 * B * NBATCH)
    feed = lambda items: data.DevicePrefetcher(items, dev, convert=lambda t: (t[0], t[1].tolist(), t[2], t[3].tolist(), t[4]),   # noqa: E731
                                               ragged={0: B * TA, 2: B * TT})
    torch.manual_seed(1234)
    model = H.FusionWithEmotionDecoder(**CFG).to(dev).train()
    cap = STEPS * B * 2
    stats = {k: EpochStats(NE, cap) for k in "abcd"}
    logs = {"b": AttentionLog.for_model(model, B, PAD), "c": AttentionLog.for_model(model, B, PAD)}
    steps = {"a": H.EvalStep(model, fusion_step_loss, stats=stats["a"]),
             "b": H.EvalStep(model, fusion_step_loss, stats=stats["b"], attn_log=logs["b"]),
             "c": H.EvalStep(model, fusion_step_loss, stats=stats["c"], attn_log=logs["c"])}
    # capture + every bucket graph the loader needs, outside the timed rounds; c's log fills here and stays full
    for k, es in steps.items():
        for i, (ra, la, rt, lt, y) in enumerate(feed(rag)):
            if i == 0:
                es.capture_packed(ra, rt, la, lt, y, pad_to=PAD)
            es.eval_packed(ra, rt, la, lt, y)
    torch.cuda.synchronize()
    assert logs["c"].counters.tolist()[0] == B, "the log of arm c is not full"
    graphs = [len(es._pb.graphs) for es in steps.values()]
    items = [rag[i % NBATCH] for i in range(STEPS)]
    host_bytes = [0]

    def epoch(arm):
        stats[arm].reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        if arm == "d":
            model.eval()
            with torch.no_grad():
                for ra, la, rt, lt, y in feed(items):
                    logits, beta, _, pack = model.forward_packed(ra, rt, la, lt, pad_to=PAD, return_attention=True)
                    stats[arm].update(logits, beta, y, fusion_step_loss(logits, beta, y))
                    enc = [{k: v.detach().float().cpu().numpy() for k, v in layer.items()} for layer in pack["encoder"]]
                    dec = [t.detach().float().cpu().numpy() for t in pack["decoder"]]
                    host_bytes[0] = sum(v.nbytes for layer in enc for v in layer.values()) + sum(t.nbytes for t in dec)
            model.train()
        else:
            es = steps[arm]
            for ra, la, rt, lt, y in feed(items):
                if arm == "b":
                    logs["b"].reset()
                es.eval_packed(ra, rt, la, lt, y)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS, (time.perf_counter() - t0) / STEPS * 1e3

    for arm in "abcd":
        epoch(arm)                                                                         # warm-up
    t = {f"{arm} {kind}": [] for arm in "abcd" for kind in ("events", "wall")}
    for r in range(ROUNDS):
        for arm in "abcd":
            ev, wall = epoch(arm)
            t[f"{arm} events"].append(ev)
            t[f"{arm} wall"].append(wall)
        print(f"B {B}: round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in t.items()) + " ms/batch", flush=True)
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    assert logs["b"].counters.tolist()[0] == B and logs["c"].counters.tolist()[0] == B
    n = [s.result()["n_samples"] for s in stats.values()]
    print(f"cfg2 B={B} bf16 inputs, valid fraction {frac:.3f}, {NBATCH} distinct batches, bucket graphs {graphs}; n_samples per arm {n}; "
          f"the log of B samples: {logs['b'].nbytes / 1e6:.1f} MB; arm d moves {host_bytes[0] / 1e6:.1f} MB to the host per batch")
    for kind in ("events", "wall"):
        a, b, c, d = (med[f"{arm} {kind}"] for arm in "abcd")
        sa = spread[f"a {kind}"] * a
        print(f"  {kind}, {STEPS} batches per round, median of {ROUNDS} (own spread): "
              + ", ".join(f"{arm} {med[f'{arm} {kind}']:.3f} ms/batch ({spread[f'{arm} {kind}'] * med[f'{arm} {kind}']:.3f})" for arm in "abcd"))
        print(f"    c - a = {c - a:+.3f} ms against a's spread of {sa:.3f} ms: {'inside' if abs(c - a) <= sa else 'OUTSIDE'}; "
              f"b - a = {b - a:+.3f} ms (the maps: {logs['b'].nbytes / 1e6:.1f} MB written -> {logs['b'].nbytes / 1e6 / max(b - a, 1e-9):.0f} GB/s "
              f"if all of it were the write); d / b = {d / b:.2f}, d - b = {d - b:+.3f} ms", flush=True)
    for es in steps.values():
        es.release_graph()


H.set_varlen(True)
H.set_varlen_maps(True)
H.set_ingest(True)
_ops.PACKED_TAIL = True
print(f"bench_attention_log: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, batches per round {STEPS}")
for b in (64, 8):
    run(b)
