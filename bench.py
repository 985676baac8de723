#!/usr/bin/env python3
"""bench.py -- utterances/sec, fwd+bwd, of FusionWithEmotionDecoder on MI355X (BASELINE.json metric).

A step = one pass of the hot path over one batch of synthetic utterances already resident in HBM:
forward (train mode, dropout 0.1) -> BCEWithLogits - 0.01*beta-reg -> backward -> (N>1) gradient all-reduce
over RCCL.  N=1 workload = BASELINE.json configs[1]: d=768, T_a=400, T_t=128, N_e=6, batch 64, bf16.
For N>1 launch with torch.distributed.run (one rank per GPU); per-GPU batch stays 64 (weak scaling).

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps and reports them (`value`,
`ms_per_step`); the secondary measurements need runs of their own and come with --full only: ragged / packed masks,
optimizer, host -> device hand-over, cross-attention cores, `roofline` (dominant kernel, HIP-event timed on the launch
stream inside libhriemo.so) and, at N=1, `cpu_baseline` (the CPU oracle timed on this box's host cores, bounded sample).

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step handed its caller as .npy files
(float32): `loss.npy` (shape (1,)) and `grads.npy`, a fixed seeded sample of every parameter's gradient (the gradients
concatenated in `named_parameters()` order, GRAD_SAMPLE positions drawn uniformly with generator seed 0, sorted).
The inputs, weights and dropout seeds are fixed, so two builds run with the same arguments can be compared file by file.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# BASELINE.json configs; "cfg2" (configs[1]) is the headline the metric is quoted on and the default.  The others are the
# single-GPU forms of configs[3] (MOSEI shape) and configs[4] (d=1024, 4+2 layers, N_e=7; "cfg5_fp8": forward projection / FFN
# GEMMs on MX-fp8 operands) so that the driver can run them too: --workload.  FLOPs per utterance: SURVEY.md 8(d).
WORKLOADS = {
    "cfg2": dict(model=dict(d_model=768, num_emotions=6, n_heads=8, num_layers_fusion=2, num_layers_decoder=2), T_a=400, T_t=128, batch=64,
                 flop=65.378e9, gemm="bf16"),
    "cfg4": dict(model=dict(d_model=768, num_emotions=6, n_heads=8, num_layers_fusion=2, num_layers_decoder=2), T_a=1000, T_t=50, batch=32,
                 flop=136.715e9, gemm="bf16"),
    "cfg5": dict(model=dict(d_model=1024, num_emotions=7, n_heads=8, num_layers_fusion=4, num_layers_decoder=2), T_a=400, T_t=128, batch=32,
                 flop=227.115e9, gemm="bf16"),
    "cfg5_fp8": dict(model=dict(d_model=1024, num_emotions=7, n_heads=8, num_layers_fusion=4, num_layers_decoder=2), T_a=400, T_t=128,
                     batch=32, flop=227.115e9, gemm="mx_fp8"),
}
CFG = dict(WORKLOADS["cfg2"]["model"], beta_hidden=256,
           dropout=0.1)                   # 0.1 = reference default (the headline); --dropout changes it
T_A, T_T = 400, 128
FLOP_PER_UTT_FWD_BWD = 65.378e9           # SURVEY.md 8(d), closed form == FlopCounterMode
PEAK_BF16_TFLOPS = 2500.0                 # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_FP8_TFLOPS = 5000.0                  # dense MX-fp8 (scaled MFMA 16x16x128)
PEAK_HBM_GBS = 8000.0
GRAD_SAMPLE = 1 << 22                     # --dump-outputs: gradient entries kept (16 MB of float32; cfg 2 has 54.6 M)


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-per-gpu", type=int, default=None, help="default: the workload's batch (64 for cfg2)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2",
                    help="cfg2 = BASELINE configs[1] (the metric's configuration, default); cfg4 / cfg5 / cfg5_fp8: configs[3] / [4] per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of one hipGraph replay per step")
    ap.add_argument("--graph-dp", action="store_true", help="N>1: replay a captured step and all-reduce afterwards (no overlap)")
    ap.add_argument("--dropout", type=float, default=0.1, help="dropout probability of the benchmark model (0.1 = the reference default)")
    ap.add_argument("--captured-exchange", action="store_true",
                    help="N>1: also probe the replay whose graph holds the gradient exchange (capture(collectives=True)) as a third mode")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run the secondary measurements: ragged / packed masks, optimizer, host -> device "
                         "copy, cross-attention cores, per-kernel-class roofline (--no-roofline drops these) and the CPU baseline "
                         "(--no-cpu-baseline drops it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the loss and a seeded sample of the gradients of the last timed step to DIR/*.npy (float32)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


def dump_outputs(out_dir, loss, model):
    """what the last timed step handed its caller: the loss it returned and the parameters' gradients (sampled, see the module
    docstring).  Called right after the timed region, before anything else runs a step."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    grads = [p.grad.reshape(-1) for p in model.parameters() if p.requires_grad]
    n = sum(g.numel() for g in grads)
    flat = torch.cat(grads).float()
    if n > GRAD_SAMPLE:
        idx = torch.randint(0, n, (GRAD_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
        flat = flat[idx.to(flat.device)]
    np.save(os.path.join(out_dir, "loss.npy"), loss.detach().float().reshape(1).cpu().numpy())
    np.save(os.path.join(out_dir, "grads.npy"), flat.cpu().numpy())
    log(f"outputs of the last timed step written to {out_dir}: loss.npy, grads.npy ({flat.numel()} of {n} gradient entries)")


def synth(B, rank, device):
    g = torch.Generator().manual_seed(1234 + rank)
    h_a = torch.randn(B, T_A, CFG["d_model"], generator=g).to(device=device, dtype=torch.bfloat16)
    h_t = torch.randn(B, T_T, CFG["d_model"], generator=g).to(device=device, dtype=torch.bfloat16)
    m_a = torch.zeros(B, T_A, dtype=torch.bool, device=device)      # all-False masks, as the reference's tests
    m_t = torch.zeros(B, T_T, dtype=torch.bool, device=device)
    y = (torch.rand(B, CFG["num_emotions"], generator=g) < 0.3).float().to(device)
    return h_a, h_t, m_a, m_t, y


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for ln in fh:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline():
    """CPU oracle (fp32, train mode, dropout 0.1), same shapes: B=16 on all host cores of this GPU's share (1 warm-up + up to
    6 timed steps), then B=2 steps on ONE thread (SURVEY 8d asks both); bounded to ~10-30 s of CPU work."""
    from oracle import hri_emo_oracle as O
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))          # the GPU box gives one GPU a 16-core CPU share
    torch.manual_seed(1234)
    m = O.FusionWithEmotionDecoder(**CFG).train()

    def timed(B, threads, nsteps):
        torch.set_num_threads(threads)
        g = torch.Generator().manual_seed(1234)
        h_a, h_t = torch.randn(B, T_A, CFG["d_model"], generator=g), torch.randn(B, T_T, CFG["d_model"], generator=g)
        m_a, m_t = torch.zeros(B, T_A, dtype=torch.bool), torch.zeros(B, T_T, dtype=torch.bool)
        y = (torch.rand(B, CFG["num_emotions"], generator=g) < 0.3).float()
        times = []
        for i in range(nsteps + 1):
            t0 = time.perf_counter()
            logits, beta, _ = m(h_a, h_t, m_a, m_t)
            O.train_step_loss(logits, beta, y).backward()
            m.zero_grad()
            el = time.perf_counter() - t0
            if i:
                times.append(el)
            log(f"cpu_baseline B={B} step {i}: {el:.2f} s on {threads} thread(s)")
            if i == 0 and el > 12.0:        # keep the whole bench within minutes
                times.append(el)
                break
        times.sort()
        return B / times[len(times) // 2]

    heavy = FLOP_PER_UTT_FWD_BWD > 100e9          # cfg 4 / cfg 5: a smaller sample keeps the CPU leg at ~20-30 s
    b_all, n_all = (8, 3) if heavy else (16, 6)
    v_all = timed(b_all, cores, n_all)
    v_one = timed(1 if heavy else 2, 1, 1 if heavy else 2)
    return {"value": round(v_all, 3), "unit": "utterances/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(),
            "one_thread_value": round(v_one, 3),
            "sample": f"CPU oracle fp32 train-mode fwd+bwd, d={CFG['d_model']} T_a={T_A} T_t={T_T} N_e={CFG['num_emotions']}: B={b_all} on {cores} "
                      f"threads, median of the timed steps (<={n_all}) after 1 warm-up; one_thread_value: B={1 if heavy else 2}, 1 thread"}


def relaunch_under_torchrun(n):
    """`python bench.py --gpus N` without a launcher: start `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a
    CHILD process (one rank per GPU) and hand its output and exit code through.  Nothing in this process has touched the GPU
    yet (no HIP call, no torch.cuda.is_available()): it stays a plain launcher, and the ranks are children, never an exec."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("no WORLD_SIZE in the environment: launching " + " ".join(cmd[1:]))
    return subprocess.run(cmd, env=env).returncode


def main():
    global CFG, T_A, T_T, FLOP_PER_UTT_FWD_BWD
    a = parse()
    wl = WORKLOADS[a.workload]
    CFG = dict(wl["model"], beta_hidden=256, dropout=float(a.dropout))
    T_A, T_T, FLOP_PER_UTT_FWD_BWD = wl["T_a"], wl["T_t"], wl["flop"]
    if a.batch_per_gpu is None:
        a.batch_per_gpu = wl["batch"]
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_under_torchrun(a.gpus))          # `python bench.py --gpus N` run plainly: becomes the launcher
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}")
    # rehearsal on a one-GPU box (control flow of the N>1 path only, never a measurement): HRIEMO_DIST_BACKEND=gloo lets
    # several ranks share device 0 and exchange gradients through the host
    backend = os.environ.get("HRIEMO_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local = min(local, torch.cuda.device_count() - 1)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    import hri_emo_amd as H
    from hri_emo_amd import _lib
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss

    H.set_gemm_mode(wl["gemm"])
    torch.manual_seed(1234)                       # same weights and same dropout-seed stream on every rank
    model = H.FusionWithEmotionDecoder(**CFG).to(device).train()
    # one GPU: the whole step is one hipGraph replay.  Several GPUs: eager launches (the step is GPU-bound either way:
    # 9.0 ms eager vs 9.0 ms replayed at N=1) so that every matrix-gradient bucket is all-reduced over RCCL from a
    # gradient-ready hook while backward is still running; a captured graph could only start the exchange after it
    # N>1 without a forced mode: both are warmed up and the faster one (max over ranks) runs the timed region -- eager
    # overlap wins unless the host cannot keep the launches ahead of the GPU, the replay is immune to that.
    auto_mode = world > 1 and not a.no_graph and not a.graph_dp
    use_graph = not a.no_graph and (world == 1 or a.graph_dp)
    exchange_mode = None
    dp = DataParallelStep(model, fusion_step_loss, overlap=not use_graph)
    from hri_emo_amd.optim import FusedClipAdamW
    opt = FusedClipAdamW(dp.buckets, lr=1e-4, weight_decay=1e-2, max_norm=5.0)     # before capture: re-homes the parameters
    B = a.batch_per_gpu
    dp.set_global_batch(B * world)
    batch = synth(B, rank, device)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    log(f"rank {rank}/{world}: model + batch resident, warming up")
    dp.step(*batch)                                # eager once: sizes workspaces, sets kernel attributes
    if use_graph:
        dp.capture(*batch)
        log("step captured into a hipGraph (zero-grad + fwd + loss + bwd)")
    if auto_mode:
        def probe(n=3):
            dp.step(*batch)
            sync()
            t = time.perf_counter()
            for _ in range(n):
                dp.step(*batch)
            sync()
            tt = torch.tensor([(time.perf_counter() - t) / n], device=device, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return tt.item()
        t_eager = probe()
        # two optional replay modes; a capture that fails on this node (every rank takes the same branch) just drops its mode:
        #   "replay+captured exchange": the bucket all-reduces are part of the graph, launched where their gradients are ready
        #                               (overlaps backward like the eager mode, without ~450 host launches per step)
        #   "replay, exchange after":   the PR-safe form: collectives stay outside the graph and follow the replay
        modes = {"eager": t_eager}

        def try_capture(name, **kw):
            ok = 1
            try:
                dp.capture(*batch, **kw)
                dp.use_graph(True)
            except Exception as e:                 # noqa: BLE001
                ok = 0
                log(f"rank {rank}: capturing the step ({name}) failed ({type(e).__name__}: {e})")
            flag = torch.tensor([ok], device=device, dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 1:
                modes[name] = probe()
            return int(flag.item()) == 1

        # (opt-in: --captured-exchange.  It is rehearsed on one rank over RCCL in the GPU suite, but it has never run
        # on more than one GPU -- no multi-GPU node was available to the builder -- and a collective that hangs inside a
        # capture would take the whole scaling run with it; the two modes below are the measured-safe defaults)
        if a.captured_exchange:
            try_capture("replay+captured exchange", collectives=True)
        dp.buckets.suspended = True
        try_capture("replay, exchange after")
        best = min(modes, key=modes.get)
        if best == "replay+captured exchange":
            dp.capture(*batch, collectives=True)       # the later capture replaced it
            dp.use_graph(True)
        use_graph = best != "eager"
        dp.use_graph(use_graph)
        if not use_graph:
            dp.buckets.suspended = False
        exchange_mode = best
        log(f"N={world}: " + ", ".join(f"{k} {v * 1e3:.3f} ms/step" for k, v in modes.items()) + f" -> {best}")
    for _ in range(a.warmup):
        dp.step(*batch)
    sync()
    log("warm-up done, timing")
    # the contract's number: wall clock around EXACTLY a.steps steps between two sync points (max over ranks below);
    # beside it HIP events around every step on the launch stream -> median / min / max per step
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for k in range(a.steps):
        loss = dp.step(*batch)
        evs[k + 1].record()
    host_ms = (time.perf_counter() - t0) / a.steps * 1e3       # time to ENQUEUE a step (diagnostic)
    sync()
    dt = time.perf_counter() - t0
    per_step = sorted(evs[k].elapsed_time(evs[k + 1]) for k in range(a.steps))
    step_stats = {"median": round(per_step[len(per_step) // 2], 3), "min": round(per_step[0], 3), "max": round(per_step[-1], 3),
                  "source": "HIP events on the launch stream around each step"}
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    ms = dt / a.steps * 1e3
    value = B * world / (ms * 1e-3)
    log(f"{ms:.3f} ms/step -> {value:.1f} utt/s (host enqueue {host_ms:.3f} ms/step)")
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, loss, model)

    # secondary number: the same step with ragged key-padding masks, valid length ~U[0.5 L, L] per sample and
    # modality.  PAD keys are masked, PAD query rows are still computed (as in the reference), so the first number mainly shows
    # that masks cost nothing; the second is the packed (varlen) encoder, which computes the valid rows only.
    ragged = None
    if a.full and rank == 0 and world == 1 and not a.no_roofline:
        g = torch.Generator().manual_seed(4321)
        la = torch.randint(T_A // 2, T_A + 1, (B,), generator=g)
        lt = torch.randint(T_T // 2, T_T + 1, (B,), generator=g)
        rb = (batch[0], batch[1], (torch.arange(T_A)[None] >= la[:, None]).to(device), (torch.arange(T_T)[None] >= lt[:, None]).to(device), batch[4])
        for _ in range(3):
            dp.step(*rb)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(10):
            dp.step(*rb)
        torch.cuda.synchronize()
        rms = (time.perf_counter() - t1) / 10 * 1e3
        ragged = {"ms_per_step": round(rms, 3), "value": round(B / (rms * 1e-3), 1), "valid_fraction": round(float((la.sum() / T_A + lt.sum() / T_T) / (2 * B)), 3)}
        log(f"ragged masks: {rms:.3f} ms/step")
        # the same ragged batch through the packed (varlen) encoder, SURVEY 8(f) rank 4: rows of PAD positions are not computed.
        # Its graph bakes this batch's lengths in, so it is captured for this leg and the headline capture restored afterwards.
        if not a.no_graph:
            import hri_emo_amd as _H
            _H.set_varlen(True)
            try:
                dp.capture(*rb)
                for _ in range(3):
                    dp.step(*rb)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(10):
                    dp.step(*rb)
                torch.cuda.synchronize()
                pms = (time.perf_counter() - t1) / 10 * 1e3
                ragged["packed_ms_per_step"] = round(pms, 3)
                ragged["packed_value"] = round(B / (pms * 1e-3), 1)
                log(f"ragged masks, packed (varlen) encoder: {pms:.3f} ms/step")
                # the same capture fed a DIFFERENT length pattern every step (lengths handed over as host lists, as a collate
                # would): the lengths are device data of the graph, the packed row counts pick a bucket graph (captured on first
                # sight, outside the timed loop)
                fresh = []
                for j in range(8):
                    la_j = torch.randint(T_A // 2, T_A + 1, (B,), generator=g)
                    lt_j = torch.randint(T_T // 2, T_T + 1, (B,), generator=g)
                    fresh.append(((batch[0], batch[1], (torch.arange(T_A)[None] >= la_j[:, None]).to(device),
                                   (torch.arange(T_T)[None] >= lt_j[:, None]).to(device), batch[4]), (la_j.tolist(), lt_j.tolist())))
                for fb, fl in fresh:
                    dp.step(*fb, lengths=fl)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(2):
                    for fb, fl in fresh:
                        dp.step(*fb, lengths=fl)
                torch.cuda.synchronize()
                fms = (time.perf_counter() - t1) / 16 * 1e3
                ragged["packed_fresh_masks_ms_per_step"] = round(fms, 3)
                ragged["packed_bucket_graphs"] = len(dp._pb["graphs"])
                log(f"packed encoder, new masks every step: {fms:.3f} ms/step over {len(dp._pb['graphs'])} bucket graphs")
            finally:
                _H.set_varlen(False)
            dp.capture(*batch)
        dp.step(*batch)                              # gradients of the headline batch again for the legs below

    # optimizer step, timed separately: the trainer's clip_grad_norm_(5.0) + AdamW(lr 1e-4, wd 1e-2) on the
    # flat fp32 parameter buffer with the gradients of the last step (train_fusion_seq_level_decoder.py:332-334).
    # Never in `value`.
    opt_ms = None
    if a.full and rank == 0:
        snap = opt.flat_p.clone()
        for i in range(6):
            if i == 1:
                torch.cuda.synchronize()
                t1 = time.perf_counter()
            opt.step()
        torch.cuda.synchronize()
        opt_ms = (time.perf_counter() - t1) / 5 * 1e3
        opt.flat_p.copy_(snap)                      # leave the weights as they were for the legs below
        del snap
        log(f"optimizer (clip 5.0 + AdamW, hri_emo_amd.optim.FusedClipAdamW) {opt_ms:.3f} ms/step, reported separately")

    # host -> device hand-over of one batch (features + masks + labels from pinned host memory), timed separately: `value` is
    # quoted with the inputs resident in HBM; this is the PCIe-inclusive rate DESIGN.md notes (copy not overlapped with compute)
    h2d = None
    if a.full and rank == 0 and not a.no_roofline:
        host = [t.cpu().pin_memory() for t in batch]
        dst = [torch.empty_like(t) for t in batch]
        for i in range(6):
            if i == 1:
                torch.cuda.synchronize()
                t1 = time.perf_counter()
            for h_, d_ in zip(host, dst):
                d_.copy_(h_, non_blocking=True)
        torch.cuda.synchronize()
        h2d_ms = (time.perf_counter() - t1) / 5 * 1e3
        nbytes = sum(t.numel() * t.element_size() for t in batch)
        h2d = {"h2d_ms_per_batch": round(h2d_ms, 3), "bytes": nbytes, "gb_per_s": round(nbytes / h2d_ms / 1e6, 1),
               "value_with_serial_h2d": round(B / ((ms + h2d_ms) * 1e-3), 1)}
        log(f"host->device batch copy {h2d_ms:.3f} ms ({nbytes / 1e6:.1f} MB): {h2d['value_with_serial_h2d']} utt/s if not overlapped")
        del dst
        # the same hand-over the way a trainer on this package does it (hri_emo_amd.data.DevicePrefetcher: pinned double
        # buffers, copy stream, the copy of batch k+1 beside the step on batch k): every step takes a FRESH host batch
        from hri_emo_amd.data import DevicePrefetcher
        nst = max(a.steps, 10) if world == 1 else 0     # (rank-local leg: dp.step exchanges gradients, so one rank only)
        if nst:
            pf = DevicePrefetcher((host for _ in range(nst + 3)), device, depth=3)
            it = iter(pf)
            for _ in range(3):
                dp.step(*next(it))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for bt in it:
                dp.step(*bt)
            torch.cuda.synchronize()
            ov_ms = (time.perf_counter() - t1) / nst * 1e3
            h2d["ms_per_step_with_prefetched_h2d"] = round(ov_ms, 3)
            h2d["value_with_prefetched_h2d"] = round(B / (ov_ms * 1e-3), 1)
            log(f"steps fed by the prefetcher (fresh pinned host batch per step, copy overlapped): {ov_ms:.3f} ms/step")
            del pf, it
        del host

    # north_star sub-target: the cross-attention QK^T / AV cores alone (both directions, dropout as in the step),
    # algorithmic FLOPs (fwd 4*B*H*Lq*Lk*hd, bwd 2x) over the kernels' own time, against the dense bf16 MFMA peak and
    # against the attention roofline min(MFMA peak, AI * HBM) with AI = Lq*Lk/(Lq+Lk) flop/B
    xattn = None
    if a.full and rank == 0 and not a.no_roofline:
        from hri_emo_amd import _ops
        Hh, hd = CFG["n_heads"], CFG["d_model"] // CFG["n_heads"]
        pd = CFG["dropout"]

        def t_us(fn, reps=20):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3

        xattn = {"dropout": pd, "peak_tflops": PEAK_BF16_TFLOPS, "directions": {}}
        tot_fl, tot_us = 0.0, 0.0
        for name, Lq, Lk in (("audio_queries_text", T_A, T_T), ("text_queries_audio", T_T, T_A)):
            q = torch.randn(B * Lq, CFG["d_model"], device=device).bfloat16()
            k = torch.randn(B * Lk, CFG["d_model"], device=device).bfloat16()
            v = torch.randn(B * Lk, CFG["d_model"], device=device).bfloat16()
            wb = _ops.attn_mask_bits(B, Hh, Lk, hd, Lq)    # what the step itself does: bit words where the backward is one kernel
            o, lse, mbits = _ops.attn_fwd(q, k, v, B, Hh, Lq, Lk, hd, None, pd, 1234, 5, 0, want_bits=True)
            if not wb:
                mbits = None
            do, dq, dk, dv = torch.randn_like(o), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            tf = t_us(lambda: _ops.attn_fwd(q, k, v, B, Hh, Lq, Lk, hd, None, pd, 1234, 5, 0, want_bits=wb))
            tb = t_us(lambda: _ops.attn_bwd(q, k, v, o, do, dq, dk, dv, lse, B, Hh, Lq, Lk, hd, None, pd, 1234, 5, 0, mask_bits=mbits))
            fl = 4.0 * B * Hh * Lq * Lk * hd
            roofl = min(PEAK_BF16_TFLOPS, Lq * Lk / (Lq + Lk) * 8.0)
            xattn["directions"][name] = {"fwd_us": round(tf, 1), "bwd_us": round(tb, 1),
                                         "fwd_tflops": round(fl / tf / 1e6, 1), "fwd_bwd_tflops": round(3 * fl / (tf + tb) / 1e6, 1),
                                         "attention_roofline_tflops": round(roofl, 1)}
            tot_fl += 3 * fl
            tot_us += tf + tb
        xattn["fwd_bwd_tflops"] = round(tot_fl / tot_us / 1e6, 1)
        xattn["frac_of_mfma_peak"] = round(tot_fl / tot_us / 1e6 / PEAK_BF16_TFLOPS, 4)
        xattn["frac_of_attention_roofline"] = round(tot_fl / tot_us / 1e6 / min(PEAK_BF16_TFLOPS, T_A * T_T / (T_A + T_T) * 8.0), 4)
        log(f"cross-attention cores fwd+bwd: {xattn['fwd_bwd_tflops']} TFLOP/s = {100 * xattn['frac_of_mfma_peak']:.1f} % of MFMA peak, "
            f"{100 * xattn['frac_of_attention_roofline']:.1f} % of the attention roofline")

    roof = None
    if a.full and rank == 0 and not a.no_roofline:
        L = _lib.lib()
        from hri_emo_amd import _ops
        two = _ops.side_stream(device) is not None
        _ops.TWO_STREAMS = False          # time each kernel ALONE: with the text branch on a second stream the
        L.hriemo_prof_enable(1)           # event pairs would also count the time a kernel shares the chip
        nprof = min(a.steps, 5)
        dp.buckets.suspended = True                     # rank-local steps: no gradient exchange may be launched
        for _ in range(nprof):                          # instrumented steps run eagerly (events per launch)
            dp._fwd_bwd(*batch)
        dp.buckets.suspended = False
        torch.cuda.synchronize()
        rows = []
        for c in range(L.hriemo_prof_nclass()):
            msum, n, work = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
            L.hriemo_prof_collect(c, ctypes.byref(msum), ctypes.byref(n), ctypes.byref(work))
            rows.append((L.hriemo_prof_name(c).decode(), msum.value, n.value, work.value))
        L.hriemo_prof_enable(0)
        _ops.TWO_STREAMS = two
        rows.sort(key=lambda r: -r[1])
        name, msum, n, work = rows[0]                      # dominant kernel class by device time
        avg_ms = msum / max(n, 1)
        achieved = work / max(n, 1) / (avg_ms * 1e-3) / 1e12
        traffic, traffic_src = None, None
        tj = os.path.join(REPO, "profiles", "hbm_traffic.json")      # PMC passes cannot run inside bench.py;
        if os.path.exists(tj):                                       # the committed rocprofv3 summary is reported
            with open(tj) as fh:
                k = json.load(fh).get("kernels", {}).get(name)
            if k:
                traffic = round(k["fetch_bytes_per_launch"] + k["write_bytes_per_launch"])
                traffic_src = "profiles/hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 / WRITE_SIZE, bytes per launch)"
        peak_of = lambda nm: PEAK_FP8_TFLOPS if "mx8" in nm else PEAK_BF16_TFLOPS          # noqa: E731
        if a.workload != "cfg2":
            traffic, traffic_src = None, None            # the committed PMC passes were taken on the headline workload
        roof = {"bound": "mfma", "kernel": name, "achieved": round(achieved, 1), "peak": peak_of(name),
                "unit": "TFLOP/s", "frac": round(achieved / peak_of(name), 4), "traffic": traffic, "traffic_source": traffic_src,
                "algorithmic_flop_per_launch": round(work / max(n, 1)),
                "avg_launch_us": round(avg_ms * 1e3, 2), "launches_per_step": n // nprof,
                "timing": "HIP events around each launch, 5 eager steps, single stream (kernels not overlapped)",
                "device_ms_per_step_by_class": {r[0]: round(r[1] / nprof, 3) for r in rows},
                # every class against its own bound: MFMA classes in TFLOP/s of algorithmic FLOPs over the dense bf16
                # peak, the row kernels in GB/s of algorithmic bytes over HBM (8 TB/s)
                "achieved_by_class": {r[0]: ({"achieved": round(r[3] / (r[1] * 1e-3) / 1e9, 1), "unit": "GB/s", "frac": round(r[3] / (r[1] * 1e-3) / 8e12, 4)}
                                             if r[0] == "rowops" else
                                             {"achieved": round(r[3] / (r[1] * 1e-3) / 1e12, 1), "unit": "TFLOP/s", "frac": round(r[3] / (r[1] * 1e-3) / 1e12 / peak_of(r[0]), 4)})
                                      for r in rows if r[1] > 0}}
    if world > 1:
        dist.barrier()

    if rank == 0:
        out = {"metric": f"utterances/sec fwd+bwd, d={CFG['d_model']} T_a={T_A} T_t={T_T} N_e={CFG['num_emotions']}", "value": round(value, 1),
               "unit": "utterances/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
               "ms_per_step": round(ms, 3), "ms_per_step_events": step_stats, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "bf16" if wl["gemm"] == "bf16" else "fp8 (MX e4m3 forward GEMM operands) + bf16", "data": "synthetic",
               "config": {"workload": f"FusionWithEmotionDecoder fwd+bwd (train mode, dropout {CFG['dropout']}), d={CFG['d_model']} T_a={T_A} "
                                      f"T_t={T_T} N_e={CFG['num_emotions']} H=8, {CFG['num_layers_fusion']} fusion + {CFG['num_layers_decoder']} decoder layers, "
                                      f"all-False masks (BASELINE {a.workload})",
                          "global_batch": B * world, "batch_per_gpu": B, "parallelism": f"dp{world}",
                          "grad_allreduce": ("fp32 flat buckets 32MiB, RCCL, " + (exchange_mode or ("after the replay" if use_graph else "launched from gradient-ready hooks during backward"))) if world > 1 else "none",
                          "launch": "hipGraph replay" if use_graph else "eager",
                          "streams": 2 if os.environ.get("HRIEMO_TWO_STREAMS", "1") != "0" else 1},
               "host_enqueue_ms_per_step": round(host_ms, 3), "optimizer_ms_per_step": None if opt_ms is None else round(opt_ms, 3), "cross_attention": xattn, "ragged_masks": ragged, "pcie": h2d,
               "model_tflops": round(value * FLOP_PER_UTT_FWD_BWD / 1e12, 1),
               "model_mfma_frac": round(value * FLOP_PER_UTT_FWD_BWD / 1e12 / world / PEAK_BF16_TFLOPS, 4)}
        if roof is not None:
            out["roofline"] = roof
        if a.full and world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
