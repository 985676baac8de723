"""A/B of the two forms of the captured evaluation, in ONE process, rounds interleaved:

  D  default:    dp.EvalStep(model, loss_fn)                    -- every bucket graph re-derives every weight form and runs the
                                                                   decoder's query prologue
  S  stationary: dp.EvalStep(model, loss_fn, stationary=True)   -- both live in the step's weights pass, replayed only when the
                                                                   weights moved; here they never move inside a timed round

Configurations: cfg 2 (T_a = 400, T_t = 128, d = 768, N_e = 6), bf16 inputs, valid fraction ~0.72, at B = 64 and B = 8 (the default
batch of the reference's scripts/infer/mosei_eval_infer.py); fp32 precision at B = 8; mx_fp8 at cfg 5's shape (d = 1024, 4 + 2
layers, N_e = 7) at B = 32.  Each twice: "hand-over" (pinned host batches through data.DevicePrefetcher(ragged=...), then
eval_packed) and "resident" (the static buffers fed to themselves: the replay alone).  An epoch is `steps` batches, timed by a pair
of device events around it and by the wall clock behind a synchronize; medians of `rounds` rounds per arm, every arm's own
round-to-round spread (max - min).  Every bucket graph the loader needs is captured before the first timed round.  The verdict per
line: is D - S larger than the larger of the two spreads?

Separately, per configuration: the weights pass replayed alone (device events) -- what an evaluation that follows an update pays
in front of its bucket graph -- and the same pass issued eagerly (wall clock), for the launch count.

usage: python scripts_dev/bench_eval_stationary.py [rounds] [steps]"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _lib, _ops, data  # noqa: E402
from hri_emo_amd.train import fusion_step_loss  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 64
NBATCH = 4
CFG2 = dict(T=(400, 128), model=dict(d_model=768, num_emotions=6, n_heads=8, num_layers_fusion=2, num_layers_decoder=2, beta_hidden=256,
                                    dropout=0.1))
CFG5 = dict(T=(400, 128), model=dict(d_model=1024, num_emotions=7, n_heads=8, num_layers_fusion=4, num_layers_decoder=2, dropout=0.1))


def samples(B, seed, TA, TT, D, NE):
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


def loader(B, TA, TT, D, NE):
    """NBATCH distinct ragged batches, bf16 features, pinned (what a DataLoader with pin_memory=True hands over)"""
    out = []
    for i in range(NBATCH):
        r_a, l_a, r_t, l_t, y = data.collate_seq_packed(samples(B, 100 + i, TA, TT, D, NE))
        out.append((pin(r_a, torch.bfloat16), l_a, pin(r_t, torch.bfloat16), l_t, pin(y)))
    return out


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def count_launches(fn):
    real, names = _lib.call, []

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    _lib.call = spy
    try:
        fn()
    finally:
        _lib.call = real
    return names


def ab(what, arms, epoch):
    """ROUNDS interleaved rounds of epoch(step) -> (events ms/batch, wall ms/batch) per arm; prints medians, spreads, the verdict"""
    for es in arms.values():
        epoch(es)                                                                      # warm-up
    t = {f"{a} {k}": [] for a in arms for k in ("events", "wall")}
    for _ in range(ROUNDS):
        for a, es in arms.items():
            ev, wall = epoch(es)
            t[f"{a} events"].append(ev)
            t[f"{a} wall"].append(wall)
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: max(v) - min(v) for k, v in t.items()}
    for kind in ("events", "wall"):
        d, s = med[f"D {kind}"], med[f"S {kind}"]
        sd, ss = spread[f"D {kind}"], spread[f"S {kind}"]
        verdict = "OUTSIDE" if abs(d - s) > max(sd, ss) else "inside"
        print(f"  {what} ({kind}, {STEPS} batches per round, median of {ROUNDS}): default {d:.3f} ms/batch (spread {sd:.3f} ms), stationary "
              f"{s:.3f} ms/batch (spread {ss:.3f} ms); default - stationary = {d - s:+.3f} ms = {(d - s) / d:+.1%}: {verdict} the arms' spread",
              flush=True)


def run(name, cfg, B, precision="bf16", gemm="bf16"):
    TA, TT = cfg["T"]
    D, NE = cfg["model"]["d_model"], cfg["model"]["num_emotions"]
    H.set_precision(precision)
    H.set_gemm_mode(gemm)
    rag = loader(B, TA, TT, D, NE)
    frac = (sum(int(b[1].sum()) for b in rag) / TA + sum(int(b[3].sum()) for b in rag) / TT) / (2 * B * NBATCH)
    feed = lambda items: data.DevicePrefetcher(items, dev, convert=lambda t: (t[0], t[1].tolist(), t[2], t[3].tolist(), t[4]),   # noqa: E731
                                               ragged={0: B * TA, 2: B * TT})
    torch.manual_seed(1234)
    model = H.FusionWithEmotionDecoder(**cfg["model"]).to(dev).train()
    arms = {"D": H.EvalStep(model, fusion_step_loss), "S": H.EvalStep(model, fusion_step_loss, stationary=True)}
    first = next(iter(feed(rag[:1])))
    for es in arms.values():
        es.capture_packed(first[0], first[2], first[1], first[3], first[4], pad_to=(TA, TT))
        for ra, la, rt, lt, y in feed(rag):                                            # every bucket graph, outside the timed rounds
            es.eval_packed(ra, rt, la, lt, y)
        torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(arms["D"]._replay_bucket(next(reversed(arms["D"]._pb.graphs)), B),
                                                 arms["S"]._replay_bucket(next(reversed(arms["S"]._pb.graphs)), B)))
    wp = arms["S"]._weights
    print(f"{name}: B = {B}, precision {precision}, gemm {gemm}, bf16 inputs, valid fraction {frac:.3f}, {NBATCH} distinct batches, "
          f"{len(arms['S']._pb.graphs)} bucket graphs per arm, weights pass of {len(wp.records)} graph(s) over {len(wp.entries)} form requests; "
          f"outputs of the two arms bit-equal: {same}", flush=True)
    items = [rag[i % NBATCH] for i in range(STEPS)]

    def handover(es):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for ra, la, rt, lt, y in feed(items):
            es.eval_packed(ra, rt, la, lt, y)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS, (time.perf_counter() - t0) / STEPS * 1e3

    la, lt = rag[NBATCH - 1][1].tolist(), rag[NBATCH - 1][3].tolist()

    def resident(es):
        s = es._static
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = events(lambda: es.eval_packed(s[0][:sum(la)], s[1][:sum(lt)], la, lt, s[4]), STEPS)
        return ev, (time.perf_counter() - t0) / STEPS * 1e3

    ab("with hand-over", arms, handover)
    ab("inputs resident", arms, resident)
    # the weights pass alone: what an evaluation behind an update pays in front of its bucket graph
    events(wp.replay, 3)
    t_graph = [events(wp.replay, STEPS) for _ in range(ROUNDS)]
    _ops.bump_weights_epoch()
    names = count_launches(wp.eager)
    torch.cuda.synchronize()
    walls = []
    for _ in range(ROUNDS):
        _ops.bump_weights_epoch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wp.eager()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    print(f"  the weights pass alone: replayed as its graph {statistics.median(t_graph):.3f} ms (device events, spread "
          f"{max(t_graph) - min(t_graph):.3f} ms); issued eagerly {len(names)} launches, {statistics.median(walls):.3f} ms wall", flush=True)
    for es in arms.values():
        es.release_graph()


H.set_varlen(True)
H.set_ingest(True)
_ops.PACKED_TAIL = _ops.PACKED_TAIL_FP32 = _ops.PACKED_TAIL_MX8 = True
print(f"bench_eval_stationary: {torch.cuda.get_device_name(0)}, rounds {ROUNDS}, batches per round {STEPS}")
run("cfg2", CFG2, 64)
run("cfg2", CFG2, 8)
run("cfg2 fp32", CFG2, 8, precision="fp32")
run("cfg5 mx_fp8", CFG5, 32, gemm="mx_fp8")
