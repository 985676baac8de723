"""A/B of hriemo_ingest_rows against the launches it replaces, in ONE process, arms alternated, timed by device events.

kernel sites (default): for one modality, arm A = what the parent enqueues -- as_pair's torch cast(s) + hriemo_pack_rows, and
hriemo_quant_mx8 of the packed rows in fp8 mode -- arm B = one hriemo_ingest_rows.  20 launches per timed window, 7 rounds, the
median per arm and its round-to-round spread (max - min) / median.  Sites: cfg-2 audio 64 x 400 x 768 and text 64 x 128 x 768 at
valid fractions 0.72 and 1.0 with fp32 and fp16 sources (bf16 as well: there the cast is free and only the gather remains), and
cfg 5 (d = 1024, B = 32) with the fp8 copy.  Bytes per arm are the algorithm's, from the shapes.

step: captured ragged steps (DataParallelStep, varlen + packed tail) with _ops.INGEST_ROWS off and on, two models from one seed,
replays interleaved round by round: cfg 2 (B = 64) at valid fraction ~0.72 and cfg 5 in its fp8 form (B = 32).  The bench's
synthetic inputs are bf16; `step ... fp32` feeds the same batch as fp32 (what a trainer that does not cast on the host hands over).

usage: python scripts_dev/bench_ingest.py [rounds] [launches]  |  step cfg2|cfg5_fp8 [bf16|fp32] [rounds] [replays]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import hri_emo_amd as H  # noqa: E402
from hri_emo_amd import _ops  # noqa: E402

dev = torch.device("cuda", 0)
argv = sys.argv[1:]


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per call


def alternate(arms, rounds, n):
    """{name: fn} -> {name: (median us, spread = (max - min) / median)}; every round times every arm once, in turn"""
    for fn in arms.values():                       # warm-up: code objects, the allocator's blocks
        window(fn, 3)
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(window(fn, n))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in t.items()}


def kernel_sites(rounds, n):
    H.set_varlen(True)
    sites = [(f"cfg2 {mod} {B}x{L}x{d} v={v} {kind}", B, L, d, v, kind, False)
             for mod, B, L, d in (("audio", 64, 400, 768), ("text", 64, 128, 768)) for v in (0.72, 1.0) for kind in ("fp32", "fp16", "bf16")]
    sites += [(f"cfg5 {mod} {B}x{L}x{d} v={v} {kind} +fp8", B, L, d, v, kind, True)
              for mod, B, L, d in (("audio", 32, 400, 1024), ("text", 32, 128, 1024)) for v in (0.72, 1.0) for kind in ("fp32", "bf16")]
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    print(f"{'site':44s} {'valid':>6s} {'A us':>8s} {'spread':>7s} {'B us':>8s} {'spread':>7s} {'B/A':>6s} {'A MB':>7s} {'B MB':>7s} {'B GB/s':>7s}")
    for name, B, L, d, v, kind, fp8 in sites:
        g = torch.Generator().manual_seed(4321)
        lens = torch.full((B,), L) if v == 1.0 else torch.randint(int(0.44 * L), L + 1, (B,), generator=g)
        mask = (torch.arange(L)[None] >= lens[:, None]).to(dev)
        seq = _ops.seq_plan(mask, B, L)
        x = torch.randn(B, L, d, generator=g).to(dtype=dt[kind]).to(dev)
        N, frac = seq.N, seq.N / (B * L)
        H.set_gemm_mode("mx_fp8" if fp8 else "bf16")
        mx = _ops.want_mx_copy(N, d)
        assert mx == fp8, (name, N)
        twin = kind != "bf16"

        def parent():
            x16, x32 = _ops.as_pair(x)
            p16, p32 = _ops._pack_pair(x16, x32, seq, d, seq.idx)
            return (p16, p32) + (_ops.quant_mx8(p16.view(N, d)) if mx else ())

        def ingest():
            return _ops._ingest_rows(x, seq, False, want32=twin)

        a, b = parent(), ingest()                  # the two arms write the same bits
        assert torch.equal(a[0], b[0]) and (not twin or torch.equal(a[1], b[1]))
        assert not mx or (torch.equal(a[2], b[2][0]) and torch.equal(a[3][:, :N], b[2][1][:, :N]))
        res = alternate({"A": parent, "B": ingest}, rounds, n)
        es = x.element_size()
        per = B * L * d
        # A: casts over the padded tensor (read + write per cast), the pack's read + write of both members, the quantiser's pass
        bytes_a = per * ((es + 2 if twin else 0) + (es + 4 if kind == "fp16" else 0)) + N * d * (12 if twin else 4) + (N * d * 3 if mx else 0)
        bytes_b = N * d * (es + 2 + (4 if twin else 0) + (1 if mx else 0))
        (ta, sa), (tb, sb) = res["A"], res["B"]
        print(f"{name:44s} {frac:6.3f} {ta:8.1f} {sa:7.3f} {tb:8.1f} {sb:7.3f} {tb / ta:6.3f} {bytes_a / 1e6:7.1f} {bytes_b / 1e6:7.1f} {bytes_b / tb / 1e3:7.0f}")
    H.set_gemm_mode("bf16")


def step_ab(which, kind, rounds, n):
    from hri_emo_amd.dp import DataParallelStep
    from hri_emo_amd.train import fusion_step_loss
    wl = bench.WORKLOADS[which]
    B = wl["batch"]
    bench.CFG = dict(wl["model"], beta_hidden=256, dropout=0.1)
    bench.T_A, bench.T_T = wl["T_a"], wl["T_t"]
    H.set_gemm_mode(wl["gemm"])
    H.set_varlen(True)
    _ops.PACKED_TAIL = _ops.PACKED_TAIL_MX8 = True
    g = torch.Generator().manual_seed(4321)
    la = torch.randint(bench.T_A // 2, bench.T_A + 1, (B,), generator=g)
    lt = torch.randint(bench.T_T // 2, bench.T_T + 1, (B,), generator=g)
    batch = bench.synth(B, 0, dev)
    cast = (lambda t: t.float()) if kind == "fp32" else (lambda t: t)
    rb = (cast(batch[0]), cast(batch[1]), (torch.arange(bench.T_A)[None] >= la[:, None]).to(dev),
          (torch.arange(bench.T_T)[None] >= lt[:, None]).to(dev), batch[4])
    valid = float((la.sum() / bench.T_A + lt.sum() / bench.T_T) / (2 * B))

    def arm(on):
        H.set_ingest(on)
        torch.manual_seed(1234)
        model = H.FusionWithEmotionDecoder(**bench.CFG).to(dev).train()
        dp = DataParallelStep(model, fusion_step_loss, overlap=False)
        dp.set_global_batch(B)
        dp.step(*rb)
        dp.capture(*rb)
        for _ in range(5):
            dp.step(*rb)
        torch.cuda.synchronize()
        return dp

    arms = {"off": arm(False), "on": arm(True)}
    H.set_ingest(False)
    t = {k: [] for k in arms}
    for r in range(rounds):
        for k, dp in arms.items():
            t[k].append(window(lambda: dp.step(*rb), n) / 1e3)
        print(f"round {r}: " + ", ".join(f"INGEST_ROWS {k} {t[k][-1]:.3f} ms/step" for k in arms))
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"{which} ragged captured step, B={B}, {kind} inputs, valid fraction {valid:.3f}: median of {rounds} rounds x {n} replays: "
          + "; ".join(f"{k} {med[k]:.3f} ms (spread {(max(t[k]) - min(t[k])) / med[k]:.4f})" for k in arms)
          + f"; on / off = {med['on'] / med['off']:.4f}, difference {med['off'] - med['on']:+.3f} ms"
          " (dropout on: each capture draws its own seed; equality is the tests' business)")


if argv and argv[0] == "step":
    kind = argv[2] if len(argv) > 2 and argv[2] in ("bf16", "fp32") else "bf16"
    rest = [a for a in argv[2:] if a not in ("bf16", "fp32")]
    step_ab(argv[1], kind, int(rest[0]) if rest else 7, int(rest[1]) if len(rest) > 1 else 20)
else:
    kernel_sites(int(argv[0]) if argv else 7, int(argv[1]) if len(argv) > 1 else 20)
