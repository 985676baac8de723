"""GPU suite, fp32-mode row kernels (hri-emo_amd/csrc/fp32mode.hip) through the C ABI against fp32_reference.py: the operand splits
(bit for bit, and hi + mid + lo == x), the element-wise dropout (exact against the hash), column sums, LayerNorm(x + drop(g))
forward and backward with their _rows forms, the padded gate pieces and the head's rowdot backward -- at the widths, row counts
and lengths where each kernel changes path (fp32_reference's tables), with every operand and output between 0xFF guards (NaN as
fp32), strided where the ABI has a leading dimension, and every workspace of exactly the queried size.

Limits: F v mag from the float64 reference alone (fp32_reference.py; test_fp32_bound_host.py proves their teeth).  Each test
prints its worst error / limit (profiles/2026-10-19_fp32_kernel_limits.log is one run of them)."""
import pytest
import torch

import fp32_reference as F
import rowops_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
V = F.V


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib.lib()


def call(L, name, *args):
    rc = getattr(L, name)(*args)
    assert rc == 0, (name, rc, L.hriemo_last_error().decode())


def refused(L, name, *args):
    rc = getattr(L, name)(*args)
    msg = L.hriemo_last_error().decode()
    assert rc != 0 and msg, (name, rc, msg)
    torch.cuda.synchronize()
    return msg


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(b):
    return None if b is None else b.ptr


def mat(x, j=0, **kw):
    return None if x is None else F.Guarded.of(x, j=j, guard=16, device=DEV, **kw)


def vec(x):
    return None if x is None else F.GuardedVec.of(x.contiguous(), device=DEV)


def out_vec(n, dtype=torch.float32):
    return F.GuardedVec(n, dtype, device=DEV)


class Strided:
    """[rows, cols] of any width inside a GuardedVec with row stride ld >= cols; the pad columns stay 0xFF"""

    def __init__(self, x, ld):
        self.buf = F.GuardedVec(x.shape[0] * ld, x.dtype, device=DEV)
        self.ld, self.shape = ld, tuple(x.shape)
        self.buf.view.view(x.shape[0], ld)[:, :x.shape[1]].copy_(x)
        self.ptr = self.buf.ptr

    def assert_intact(self, name):
        self.buf.assert_intact(name)


def intact(bufs, name):
    torch.cuda.synchronize()
    for n, b in bufs.items():
        if b is not None:
            b.assert_intact(f"{name}: {n}")


def untouched(b):
    return bool((b.view.contiguous().view(torch.uint8) == 0xFF).all())


def bits16(x):
    return x.contiguous().view(torch.int16)


def bits32(x):
    return x.contiguous().view(torch.int32)


# ================================================================================================ operand splits
def run_split(L, x, form, relu, mask, legacy=False, name="split"):
    """one launch: X with ldx = K + 8, the mask with ldmask = K + 16, Y exactly filling its guarded allocation -> Y on the CPU"""
    M, K = x.shape
    n = 6 if form >= 4 else 3
    rows, cols = (M, n * K) if form in (0, 1, 4, 5) else (n * M, K)
    bufs = {"X": mat(x, j=1), "mask": mat(mask, j=2), "Y": out_vec(rows * cols, torch.bfloat16)}
    if mask is not None:
        assert bufs["mask"].ld != bufs["X"].ld
    if legacy:
        call(L, "hriemo_split_bf16x3", bufs["X"].ptr, bufs["X"].ld, M, K, bufs["Y"].ptr, form, int(relu), stream())
    else:
        call(L, "hriemo_split3_f32", bufs["X"].ptr, bufs["X"].ld, M, K, bufs["Y"].ptr, form, int(relu), ptr(bufs["mask"]),
             bufs["mask"].ld if mask is not None else 0, stream())
    intact(bufs, name)
    return bufs["Y"].view.cpu().reshape(rows, cols)


def check_split(got, x, form, relu, mask, name):
    t, hi, mid, lo = F.split_host(x, relu, mask)
    want = F.split_layout(form, hi, mid, lo)
    assert got.shape == want.shape
    if relu:
        # max(-0, 0) may return either zero (IEEE 754 maxNum); everything else is compared bit for bit
        assert torch.equal(bits32(got.float() + 0.0), bits32(want.float() + 0.0)), f"{name}: hi / mid / lo differ from the host's"
    else:
        assert torch.equal(bits16(got), bits16(want)), f"{name}: hi / mid / lo differ from the host's bit for bit"
    if form >= 4:
        assert F.split_sum_exact(form, got, t) == 0, f"{name}: hi + mid + lo != x"


@pytest.mark.parametrize("form", range(8))
def test_split3_f32_forms(L, form):
    """all eight layouts at K in {4, 12, 264}, M in {1, 5}: plain, masked, and relu together with a mask; inputs with +-0,
    subnormals, hi that rounds up (mid < 0) and 1e-30 .. 1e30"""
    for M in F.SPLIT_M:
        for K in F.SPLIT_K:
            x = F.split_inputs(M, K)
            g = torch.Generator().manual_seed(M + K)
            mask = torch.randn(M, K, generator=g)
            for relu, mk in ((False, None), (False, mask), (True, mask)):
                name = f"split3_f32 form {form} {M}x{K} relu={relu} mask={mk is not None}"
                check_split(run_split(L, x, form, relu, mk, name=name), x, form, relu, mk, name)


@pytest.mark.parametrize("layout", [0, 1])
def test_split_bf16x3_layouts(L, layout):
    for M in F.SPLIT_M:
        for relu in (False, True):
            x = F.split_inputs(M, 8, seed=layout)
            name = f"split_bf16x3 layout {layout} {M}x8 relu={relu}"
            check_split(run_split(L, x, layout, relu, None, legacy=True, name=name), x, layout, relu, None, name)


def test_split_second_trip(L):
    """M K / 4 just above 8192 * 256 vectors: the grid-stride loop takes its second trip; compared on the device"""
    M, K = F.SPLIT_SECOND_TRIP
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3))
    bufs = {"X": mat(x, j=1), "Y": out_vec(M * 3 * K, torch.bfloat16)}
    call(L, "hriemo_split3_f32", bufs["X"].ptr, bufs["X"].ld, M, K, bufs["Y"].ptr, 0, 0, None, 0, stream())
    intact(bufs, "split second trip")
    _, hi, mid, lo = F.split_host(x)
    want = F.split_layout(0, hi, mid, lo).to(DEV)
    assert torch.equal(bits16(bufs["Y"].view.reshape(M, 3 * K)), bits16(want))


# ================================================================================================ element-wise dropout
def run_dropout(L, X, relu, gate, p, row_off, name):
    M, N = X.shape
    bufs = {"X": mat(X), "gate": mat(gate), "Y": F.Guarded(M, N, torch.float32, j=0, guard=16, device=DEV)}
    call(L, "hriemo_dropout_f32", bufs["X"].ptr, bufs["Y"].ptr, M, N, int(relu), ptr(bufs["gate"]), p, F.SEED, None, F.SITE, row_off, stream())
    intact(bufs, name)
    return bufs["Y"].view


@pytest.mark.parametrize("M,N,relu,gated,p,row_off", [(5, 4, False, False, 0.25, 0), (5, 264, True, False, 0.25, 1000), (3, 12, False, True, 0.25, 77),
                                                      (4, 260, True, True, 0.5, 1 << 20), (5, 264, False, False, 0.0, 0)])
def test_dropout_f32_exact(L, M, N, relu, gated, p, row_off):
    g = torch.Generator().manual_seed(M * N)
    X = torch.randn(M, N, generator=g)
    gate = torch.randn(M, N, generator=g) if gated else None
    got = run_dropout(L, X, relu, gate, p, row_off, "dropout_f32").cpu()
    want = F.dropout_host(X, relu, gate, p, F.SEED, F.SITE, row_off)
    assert torch.equal(bits32(got), bits32(want))
    if p > 0:
        assert 0 < int((got == 0).sum()) < got.numel()


def test_dropout_f32_second_trip(L):
    M, N = F.DROPOUT_SECOND_TRIP
    X = torch.randn(M, N, generator=torch.Generator().manual_seed(4))
    got = run_dropout(L, X, True, None, 0.1, 5, "dropout second trip")
    want = F.dropout_host(X, True, None, 0.1, F.SEED, F.SITE, 5).to(DEV)
    assert torch.equal(bits32(got), bits32(want))


# ================================================================================================ column sums
@pytest.mark.parametrize("M", F.COLSUM_M)
def test_colsum_f32(L, M):
    """every regrouping of the row slices (rows_per 1, 33, 64, 65, a short last slice) x N around one 256-column block; ldx > N, a
    mask with its own stride, accumulation onto a non-zero destination; the workspace of exactly the queried size"""
    worst = 0.0
    for i, N in enumerate(F.COLSUM_N):
        g = torch.Generator().manual_seed(M * 1000 + N)
        X = torch.randn(M, N, generator=g)
        masked, acc = i % 2 == 1, (i + M) % 2 == 0
        mask = torch.randn(M, N, generator=g) if masked else None
        init = F.far_init(N, g)
        bufs = {"X": Strided(X, N + 3), "mask": Strided(mask, N + 5) if masked else None, "out": vec(init) if acc else out_vec(N),
                "workspace": out_vec(L.hriemo_colsum_f32_workspace_bytes(M, N) // 4)}
        call(L, "hriemo_colsum_f32", bufs["X"].ptr, bufs["X"].ld, M, N, ptr(bufs["mask"]), bufs["mask"].ld if masked else 0, bufs["out"].ptr,
             int(acc), bufs["workspace"].ptr, stream())
        intact(bufs, f"colsum_f32 {M}x{N}")
        t = X if mask is None else X * (mask > 0)
        ref, mag = R.colsum_ref(t, init if acc else None)
        worst = max(worst, R.check_sum(bufs["out"].view.cpu(), ref, mag, M + (1 if acc else 0), f"colsum_f32 {M}x{N} mask={masked} acc={acc}"))
    print(f"fp32 limits colsum_f32 M={M}: {worst:.3f}")


# ================================================================================================ LayerNorm(x + drop(g))
@pytest.mark.parametrize("c", F.LN32_FWD_CASES, ids=F.ln32_id)
def test_add_ln_f32_forward(L, c):
    M, d, fam, p, resid, roff, rows, y16 = c
    case = F.ln32_case(c)
    f, _ = F.ln32_refs(case)
    bufs = {"G": mat(case["G"]), "X": mat(case["X32"]), "gamma": vec(case["gamma"]), "beta": vec(case["beta"]),
            "Y32": F.Guarded(M, d, torch.float32, j=0, guard=16, device=DEV), "Y16": out_vec(M * d, torch.bfloat16) if y16 else None,
            "row_index": vec(torch.from_numpy(case["row_index"])) if rows else None}
    head = (bufs["G"].ptr, ptr(bufs["X"]), bufs["gamma"].ptr, bufs["beta"].ptr, bufs["Y32"].ptr, ptr(bufs["Y16"]), M, d, case["eps"], p, F.SEED, None,
            F.SITE, roff)
    if rows:
        call(L, "hriemo_add_ln_f32_rows", *head, bufs["row_index"].ptr, stream())
    else:
        call(L, "hriemo_add_ln_f32", *head, stream())
    intact(bufs, F.ln32_id(c))
    r = F.check_ln32_fwd(bufs["Y32"].view.cpu(), bufs["Y16"].view.cpu().reshape(M, d) if y16 else None, f, "add_ln_f32 " + F.ln32_id(c))
    print(f"fp32 limits add_ln_f32 {F.ln32_id(c)}: y {r['y32']:.3f}")


def test_add_ln_f32_device_seed_word(L):
    """seed split between the argument and the device word: the masks of their sum"""
    c = (5, 260, "unit", 0.25, "x32", 77, False, False)
    case = F.ln32_case(c)
    f, _ = F.ln32_refs(case)
    word = 0x1122334455
    bufs = {"G": mat(case["G"]), "X": mat(case["X32"]), "gamma": vec(case["gamma"]), "beta": vec(case["beta"]),
            "Y32": F.Guarded(5, 260, torch.float32, j=0, guard=16, device=DEV), "word": vec(torch.tensor([word], dtype=torch.int64))}
    call(L, "hriemo_add_ln_f32", bufs["G"].ptr, bufs["X"].ptr, bufs["gamma"].ptr, bufs["beta"].ptr, bufs["Y32"].ptr, None, 5, 260, case["eps"], 0.25,
         F.SEED - word, bufs["word"].ptr, F.SITE, 77, stream())
    intact(bufs, "seed word")
    F.check_ln32_fwd(bufs["Y32"].view.cpu(), None, f, "add_ln_f32 seed word")


@pytest.mark.parametrize("c", F.LN32_BWD_CASES, ids=F.ln32_id)
def test_add_ln_f32_backward(L, c):
    """dS, dG (its own matrix under dropout, NULL without), dgamma, dbeta and dbias (NULL: the two-segment reduce grid), overwriting
    or accumulating onto non-zero destinations; M up to 2053 at d = 260: the row loop's second trip, with waves that own no row in it"""
    M, d, fam, p, resid, roff, rows, dbias, acc = c
    case = F.ln32_case(c)
    g = torch.Generator().manual_seed(M + d)
    init = {n: F.far_init(d, g) for n in ("dgamma", "dbeta", "dbias")}
    _, ref = F.ln32_refs(case, init if acc else None)
    nbytes = L.hriemo_add_ln_bwd_f32_workspace_bytes(M, d)
    assert nbytes == min((M + 3) // 4, 512) * 3 * d * 4
    bufs = {"dY": mat(case["dY"]), "G": mat(case["G"]), "X": mat(case["X32"]), "gamma": vec(case["gamma"]),
            "dS": F.Guarded(M, d, torch.float32, j=0, guard=16, device=DEV), "dG": F.Guarded(M, d, torch.float32, j=0, guard=16, device=DEV) if p > 0 else None,
            "workspace": out_vec(nbytes // 4), "row_index": vec(torch.from_numpy(case["row_index"])) if rows else None}
    for n in ("dgamma", "dbeta", "dbias"):
        bufs[n] = None if (n == "dbias" and not dbias) else (vec(init[n]) if acc else out_vec(d))
    head = (bufs["dY"].ptr, bufs["G"].ptr, ptr(bufs["X"]), bufs["gamma"].ptr, bufs["dS"].ptr, ptr(bufs["dG"]), bufs["dgamma"].ptr, bufs["dbeta"].ptr,
            ptr(bufs["dbias"]), int(acc), M, d, case["eps"], p, F.SEED, None, F.SITE, roff, bufs["workspace"].ptr)
    if rows:
        call(L, "hriemo_add_ln_bwd_f32_rows", *head, bufs["row_index"].ptr, stream())
    else:
        call(L, "hriemo_add_ln_bwd_f32", *head, stream())
    intact(bufs, F.ln32_id(c))
    got = {n: (None if bufs[n] is None else bufs[n].view.cpu()) for n in ("dS", "dG", "dgamma", "dbeta", "dbias")}
    if not dbias:
        ref = {k: v for k, v in ref.items() if "dbias" not in k}
    r = F.check_ln32_bwd(got, case, ref, "add_ln_bwd_f32 " + F.ln32_id(c), acc)
    print(f"fp32 limits add_ln_bwd_f32 {F.ln32_id(c)}: " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))


# ================================================================================================ refusals
def test_row_kernel_refusals(L):
    """d = 1028 into add_ln_bwd_f32, d % 4 != 0, K % 4 != 0, a misaligned mask: non-zero return, hriemo_last_error() set, every output
    byte still 0xFF"""
    g = torch.Generator().manual_seed(1)
    # LayerNorm backward wider than its registers hold
    M, d = 3, 1028
    b = {"dY": vec(torch.randn(M * d, generator=g)), "G": vec(torch.randn(M * d, generator=g)), "gamma": vec(torch.ones(d)), "dS": out_vec(M * d),
         "dgamma": out_vec(d), "dbeta": out_vec(d), "dbias": out_vec(d), "workspace": out_vec(3 * d)}
    msg = refused(L, "hriemo_add_ln_bwd_f32", b["dY"].ptr, b["G"].ptr, None, b["gamma"].ptr, b["dS"].ptr, None, b["dgamma"].ptr, b["dbeta"].ptr,
                  b["dbias"].ptr, 0, M, d, 1e-5, 0.0, 0, None, 0, 0, b["workspace"].ptr, stream())
    assert all(untouched(b[n]) for n in ("dS", "dgamma", "dbeta", "dbias", "workspace")), msg
    intact(b, "add_ln_bwd_f32 d=1028")
    # d % 4 != 0
    M, d = 3, 6
    b = {"G": vec(torch.randn(M * d, generator=g)), "gamma": vec(torch.ones(d)), "beta": vec(torch.zeros(d)), "Y32": out_vec(M * d),
         "Y16": out_vec(M * d, torch.bfloat16)}
    refused(L, "hriemo_add_ln_f32", b["G"].ptr, None, b["gamma"].ptr, b["beta"].ptr, b["Y32"].ptr, b["Y16"].ptr, M, d, 1e-5, 0.0, 0, None, 0, 0, stream())
    assert untouched(b["Y32"]) and untouched(b["Y16"])
    intact(b, "add_ln_f32 d=6")
    # p = 1
    refused(L, "hriemo_add_ln_f32", b["G"].ptr, None, b["gamma"].ptr, b["beta"].ptr, b["Y32"].ptr, b["Y16"].ptr, 3, 4, 1e-5, 1.0, 0, None, 0, 0, stream())
    assert untouched(b["Y32"]) and untouched(b["Y16"])
    # K % 4 != 0, and a mask off by 4 bytes
    M, K = 3, 8
    x = {"X": vec(torch.randn(M * K, generator=g)), "mask": vec(torch.randn(M * K + 4, generator=g)), "Y": out_vec(6 * M * K, torch.bfloat16)}
    refused(L, "hriemo_split3_f32", x["X"].ptr, 8, M, 6, x["Y"].ptr, 4, 0, None, 0, stream())
    assert untouched(x["Y"])
    refused(L, "hriemo_split3_f32", x["X"].ptr, K, M, K, x["Y"].ptr, 4, 0, x["mask"].ptr + 4, K, stream())
    assert untouched(x["Y"])
    refused(L, "hriemo_split3_f32", x["X"].ptr, K, M, K, x["Y"].ptr, 4, 0, x["mask"].ptr, 6, stream())        # ldmask % 4 != 0
    assert untouched(x["Y"])
    refused(L, "hriemo_split3_f32", x["X"].ptr, K, M, K, x["Y"].ptr, 8, 0, None, 0, stream())                 # no such form
    assert untouched(x["Y"])
    refused(L, "hriemo_split_bf16x3", x["X"].ptr, K, M, 4, x["Y"].ptr, 0, 0, stream())                        # the legacy entry wants K % 8 == 0
    assert untouched(x["Y"])
    y = out_vec(M * K)
    refused(L, "hriemo_dropout_f32", x["X"].ptr, y.ptr, M, 6, 0, None, 0.1, 0, None, 0, 0, stream())
    refused(L, "hriemo_dropout_f32", x["X"].ptr, y.ptr, M, K, 0, x["mask"].ptr + 4, 0.1, 0, None, 0, 0, stream())
    assert untouched(y)
    intact(x, "split3_f32 refusals")


# ================================================================================================ padded fp32 gate pieces
def check(got, ref, mag, factor, name):
    return R.check_elem(got, ref, mag, factor, True, name)


@pytest.mark.parametrize("mask", ("none", "prefix", "scattered", "full"))
def test_masked_mean_f32(L, mask):
    worst = 0.0
    for Ln in F.MEAN_LENGTHS:
        for d in F.GATE_WIDTHS:
            B = 3
            X = torch.randn(B, Ln, d, generator=torch.Generator().manual_seed(Ln * d))
            m = F.gate_mask(mask, B, Ln)
            bufs = {"X": vec(X.reshape(-1)), "mask": None if m is None else vec(m.view(torch.uint8).reshape(-1)), "pooled": out_vec(B * d)}
            call(L, "hriemo_masked_mean_f32", bufs["X"].ptr, ptr(bufs["mask"]), bufs["pooled"].ptr, B, Ln, d, stream())
            intact(bufs, f"masked_mean_f32 {mask} L={Ln} d={d}")
            ref, mag, n = F.masked_mean32_ref(X, m)
            got = bufs["pooled"].view.cpu().reshape(B, d)
            worst = max(worst, check(got, ref, mag, Ln + 1, f"masked_mean_f32 {mask} L={Ln} d={d}"))     # L - 1 additions, the division
            if mask == "full":
                assert float(got[0].abs().max()) == 0.0        # every row PAD: 0 / max(0, 1)
    print(f"fp32 limits masked_mean_f32 {mask}: {worst:.3f}")


@pytest.mark.parametrize("d", F.GATE_WIDTHS + (1024,))
def test_gate_input_f32_and_backward(L, d):
    """[a, t, |a - t|, a t]: single fp32 operations, bit for bit; the backward with columns where a == t (sign(0) = 0)"""
    B = 3
    c = F.G.gin_bwd_case(B, d)
    a, t = c["a"], c["t"]
    dgin = c["dgin"].float() * (1 + 2.0 ** -9 * torch.randn(B, 4 * d, generator=torch.Generator().manual_seed(d)))
    bufs = {"a": vec(a.reshape(-1)), "t": vec(t.reshape(-1)), "gin": out_vec(B * 4 * d), "dgin": vec(dgin.reshape(-1)), "da": out_vec(B * d),
            "dt": out_vec(B * d)}
    call(L, "hriemo_gate_input_f32", bufs["a"].ptr, bufs["t"].ptr, bufs["gin"].ptr, B, d, stream())
    call(L, "hriemo_gate_input_bwd_f32", bufs["dgin"].ptr, bufs["a"].ptr, bufs["t"].ptr, bufs["da"].ptr, bufs["dt"].ptr, B, d, stream())
    intact(bufs, f"gate_input_f32 d={d}")
    want = torch.cat([a, t, (a - t).abs(), a * t], 1)
    assert torch.equal(bits32(bufs["gin"].view.cpu().reshape(B, 4 * d)), bits32(want))
    assert int((a == t).sum()) >= B * (d // 3)
    ref = F.gate_in_bwd32_ref(dgin, a, t)
    r = {n: check(bufs[n].view.cpu().reshape(B, d), ref[n], ref["mag_" + n], F.GIN_BWD_ROUNDINGS, f"gate_input_bwd_f32 d={d} {n}") for n in ("da", "dt")}
    print(f"fp32 limits gate_input_bwd_f32 d={d}: da {r['da']:.3f} dt {r['dt']:.3f}")


@pytest.mark.parametrize("d", F.GATE_WIDTHS + (1024,))
def test_sigmoid_beta_f32(L, d):
    B = 3
    pre = F.G.sigmoid_inputs(B, d)
    assert float(pre.abs().max()) <= F.G.PRE_MAX
    bufs = {"pre": vec(pre.reshape(-1)), "w": out_vec(B * d), "beta": out_vec(B)}
    call(L, "hriemo_sigmoid_beta_f32", bufs["pre"].ptr, bufs["w"].ptr, bufs["beta"].ptr, B, d, stream())
    intact(bufs, f"sigmoid_beta_f32 d={d}")
    ref = F.G.sigmoid_ref(pre)
    rw = check(bufs["w"].view.cpu().reshape(B, d), ref["w"], ref["w"], F.SIGMOID32_FACTOR, f"sigmoid_beta_f32 d={d} w")
    rb = check(bufs["beta"].view.cpu(), ref["beta"], ref["beta"], d + F.SIGMOID32_FACTOR, f"sigmoid_beta_f32 d={d} beta")
    print(f"fp32 limits sigmoid_beta_f32 d={d}: w {rw:.3f} beta {rb:.3f}")


def run_fuse(L, B, Ln, La, Lt, d, h16, name):
    g = torch.Generator().manual_seed(B * Ln + d)
    w = torch.sigmoid(2 * torch.randn(B, d, generator=g))
    Aa, T = torch.randn(B, La, d, generator=g), torch.randn(B, Lt, d, generator=g)
    bufs = {"w": vec(w.reshape(-1)), "A": vec(Aa.reshape(-1)), "T": vec(T.reshape(-1)), "H32": out_vec(B * Ln * d),
            "H16": out_vec(B * Ln * d, torch.bfloat16) if h16 else None}
    call(L, "hriemo_fuse_f32", bufs["w"].ptr, bufs["A"].ptr, La, bufs["T"].ptr, Lt, bufs["H32"].ptr, ptr(bufs["H16"]), B, Ln, d, stream())
    intact(bufs, name)
    ref, mag = F.fuse32_ref(w, Aa, T, Ln)
    h32 = bufs["H32"].view.cpu().reshape(B, Ln, d)
    r = check(h32, ref, mag, F.FUSE_ROUNDINGS, name)
    if h16:
        assert torch.equal(bits16(bufs["H16"].view.cpu()), bits16(h32.bfloat16().reshape(-1))), f"{name}: H16 is not bf16(H32)"
    return r


@pytest.mark.parametrize("B,Ln,La,Lt,d,h16", [(3, 1, 2, 4, 4, True), (2, 5, 9, 6, 252, False), (2, 33, 40, 34, 256, True), (3, 2, 3, 3, 260, False)])
def test_fuse_f32(L, B, Ln, La, Lt, d, h16):
    r = run_fuse(L, B, Ln, La, Lt, d, h16, f"fuse_f32 B={B} L={Ln} La={La} Lt={Lt} d={d}")
    print(f"fp32 limits fuse_f32 d={d}: {r:.3f}")


def test_fuse_f32_second_trip(L):
    B, Ln, d = F.FUSE_SECOND_TRIP
    r = run_fuse(L, B, Ln, Ln + 1, Ln + 2, d, True, "fuse_f32 second trip")
    print(f"fp32 limits fuse_f32 second trip: {r:.3f}")


@pytest.mark.parametrize("Ln", F.DPRE_LENGTHS)
def test_gate_dpre_f32(L, Ln):
    worst = 0.0
    for i, d in enumerate(F.GATE_WIDTHS):
        B, La, Lt = 3, Ln + 2, Ln + 1
        has_dbeta = (i + Ln) % 2 == 0
        g = torch.Generator().manual_seed(Ln * d)
        dH, Aa, T = torch.randn(B, Ln, d, generator=g), torch.randn(B, La, d, generator=g), torch.randn(B, Lt, d, generator=g)
        w = torch.sigmoid(2 * torch.randn(B, d, generator=g))
        dbeta = torch.randn(B, generator=g) * d ** 0.5 if has_dbeta else None
        bufs = {"dH": vec(dH.reshape(-1)), "A": vec(Aa.reshape(-1)), "T": vec(T.reshape(-1)), "w": vec(w.reshape(-1)), "dbeta": vec(dbeta),
                "dpre": out_vec(B * d)}
        call(L, "hriemo_gate_dpre_f32", bufs["dH"].ptr, bufs["A"].ptr, La, bufs["T"].ptr, Lt, bufs["w"].ptr, ptr(bufs["dbeta"]), bufs["dpre"].ptr, B,
             Ln, d, stream())
        intact(bufs, f"gate_dpre_f32 L={Ln} d={d}")
        ref, mag = F.gate_dpre32_ref(dH, Aa, T, w, dbeta, Ln)
        worst = max(worst, check(bufs["dpre"].view.cpu().reshape(B, d), ref, mag, F.dpre32_factor(Ln, has_dbeta), f"gate_dpre_f32 L={Ln} d={d}"))
    print(f"fp32 limits gate_dpre_f32 L={Ln}: {worst:.3f}")


@pytest.mark.parametrize("is_a", [1, 0])
@pytest.mark.parametrize("mask", ("none", "scattered", "full"))
def test_gate_dy_f32(L, is_a, mask):
    worst = 0.0
    for Ln, Lx, d in ((1, 3, 4), (5, 9, 252), (33, 70, 260), (2, 2, 256)):
        B = 3
        g = torch.Generator().manual_seed(Ln * d + Lx)
        dH, dpool = torch.randn(B, Ln, d, generator=g), torch.randn(B, d, generator=g)
        w = torch.sigmoid(2 * torch.randn(B, d, generator=g))
        m = F.gate_mask(mask, B, Lx)
        bufs = {"dH": vec(dH.reshape(-1)), "w": vec(w.reshape(-1)), "dpool": vec(dpool.reshape(-1)),
                "mask": None if m is None else vec(m.view(torch.uint8).reshape(-1)), "dY": out_vec(B * Lx * d)}
        call(L, "hriemo_gate_dy_f32", bufs["dH"].ptr, bufs["w"].ptr, is_a, bufs["dpool"].ptr, ptr(bufs["mask"]), bufs["dY"].ptr, B, Ln, Lx, d, stream())
        intact(bufs, f"gate_dy_f32 {mask} L={Ln} Lx={Lx} d={d}")
        ref, mag = F.gate_dy32_ref(dH, w, bool(is_a), dpool, m, Ln, Lx)
        worst = max(worst, check(bufs["dY"].view.cpu().reshape(B, Lx, d), ref, mag, F.DY_ROUNDINGS, f"gate_dy_f32 {mask} L={Ln} Lx={Lx} d={d}"))
    print(f"fp32 limits gate_dy_f32 {mask} is_a={is_a}: {worst:.3f}")


@pytest.mark.parametrize("M", F.ROWDOT_M)
@pytest.mark.parametrize("acc", [False, True])
def test_rowdot_bwd_f32(L, M, acc):
    worst = 0.0
    for d in F.ROWDOT_D:
        g = torch.Generator().manual_seed(M * d)
        dl, Z, w = torch.randn(M, generator=g), torch.randn(M, d, generator=g), torch.randn(d, generator=g)
        dw0, db0 = F.far_init(d, g), F.far_init(1, g)
        bufs = {"dl": vec(dl), "Z": vec(Z.reshape(-1)), "w": vec(w), "dZ": out_vec(M * d), "dw": vec(dw0) if acc else out_vec(d),
                "db": vec(db0) if acc else out_vec(1)}
        call(L, "hriemo_rowdot_bwd_f32", bufs["dl"].ptr, bufs["Z"].ptr, bufs["w"].ptr, bufs["dZ"].ptr, bufs["dw"].ptr, bufs["db"].ptr, int(acc), M, d,
             stream())
        intact(bufs, f"rowdot_bwd_f32 {M}x{d}")
        assert torch.equal(bits32(bufs["dZ"].view.cpu().reshape(M, d)), bits32(dl[:, None] * w[None, :]))          # one fp32 product
        _, (dw, mdw), (db, mdb) = R.rowdot_bwd_ref(dl, Z, w, dw0 if acc else None, db0 if acc else None)
        n = 1 if acc else 0
        worst = max(worst, R.check_sum(bufs["dw"].view.cpu(), dw, mdw, M + 1 + n, f"rowdot_bwd_f32 {M}x{d} dw"),
                    R.check_sum(bufs["db"].view.cpu(), db, mdb, M + n, f"rowdot_bwd_f32 {M}x{d} db"))
    print(f"fp32 limits rowdot_bwd_f32 M={M} acc={acc}: {worst:.3f}")
