"""GPU suite, row kernels (hri-emo_amd/csrc/rowops.hip) through the C-ABI against rowops_reference.py: float64 references, limits
from the reference and the fp32 yardstick orders alone.  Every input sits in a poisoned buffer between guard rows, every output is
pre-filled with 0xFF between guards and compared with them afterwards:

  1. LayerNorm(x + dropout(g)) forward and backward, both mappings, at the widths where the per-lane chunk count changes, around one
     4-row block, at 65 partial rows and at 16389 rows (every grid-stride loop takes a second trip); unit-variance, offset,
     constant and all-zero rows; rows that lose every element of g; every operand form; accumulation into non-zero destinations
  2. row maps, the device seed word, the partial-only form, the error returns
  3. hriemo_colreduce_batch on a table of 64 jobs; hriemo_colsum_bf16; hriemo_rowdot_fwd / _bwd

test_rowops_bound_host.py proves on the CPU that these limits pass correct kernels in four summation orders and fail faulty ones."""
import numpy as np
import pytest
import torch

import rowops_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES3 = ("dgamma", "dbeta", "dbias")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib.lib()


@pytest.fixture
def variant(L):
    """force(v): 0 = quad-mapped add_ln kernels where built, 1 = chunk-mapped (the default), restored afterwards"""
    try:
        yield L.hriemo_rowops_force_variant
    finally:
        L.hriemo_rowops_force_variant(1)


def call(name, *args):
    from hri_emo_amd import _lib
    _lib.call(name, *args)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(b):
    return None if b is None else b.ptr


def mat(x, **kw):
    return None if x is None else R.Guarded.of(x, j=0, device=DEV, **kw)


def vec(x):
    return None if x is None else R.GuardedVec.of(x, device=DEV)


def intact(bufs, name):
    torch.cuda.synchronize()
    for n, b in bufs.items():
        if b is not None:
            b.assert_intact(f"{name}: {n}")


def untouched(b):
    return bool((b.view.contiguous().view(torch.uint8) == 0xFF).all())


# ------------------------------------------------------------------------------------------------ add_ln launches
def run_fwd(case, name, want32=True, rows_entry=False, seed=None, seed_word=None, row_offset=None, row_index=None):
    """one forward launch on guarded buffers -> {y, y32, mean, rstd} on the CPU.  row_index / row_offset / seed override the case's."""
    M, d = case["G"].shape
    row_index = case["row_index"] if row_index is None else row_index
    bufs = {"G": mat(case["G"]), "X": mat(case["X"]), "X32": mat(case["X32"]), "gamma": vec(case["gamma"]), "beta": vec(case["beta"]),
            "Y": R.Guarded(M, d, torch.bfloat16, j=0, device=DEV), "Y32": R.Guarded(M, d, torch.float32, j=0, device=DEV) if want32 else None,
            "mean": R.GuardedVec(M, torch.float32, device=DEV), "rstd": R.GuardedVec(M, torch.float32, device=DEV),
            "row_index": None if row_index is None else vec(torch.from_numpy(np.asarray(row_index, dtype=np.int64))),
            "seed word": None if seed_word is None else vec(torch.tensor([seed_word], dtype=torch.int64))}
    b = bufs
    head = (b["G"].ptr, ptr(b["X"]), ptr(b["X32"]), b["gamma"].ptr, b["beta"].ptr, b["Y"].ptr, ptr(b["Y32"]), b["mean"].ptr, b["rstd"].ptr,
            M, d, case["eps"], case["p"], case["seed"] if seed is None else seed, ptr(b["seed word"]), case["site"],
            case["row_offset"] if row_offset is None else row_offset)
    if rows_entry or row_index is not None:
        call("hriemo_add_ln_fwd_rows", *head, None, None, 0, ptr(b["row_index"]), stream())
    else:
        call("hriemo_add_ln_fwd", *head, stream())
    intact(bufs, name)
    return {"y": b["Y"].view.cpu(), "y32": b["Y32"].view.cpu() if want32 else None, "mean": b["mean"].view.cpu(), "rstd": b["rstd"].view.cpu()}


def run_bwd(L, case, m32, r32, name, dX=True, dG=True, dbias=True, reduce=True, accumulate=False, init=None, rows_entry=False,
            seed=None, seed_word=None, row_offset=None, row_index=None):
    """one backward launch on guarded buffers -> {dX, dG, dgamma, dbeta, dbias, partials} on the CPU (None where not asked for).
    reduce=False: the partial-only form (dgamma == NULL) on a workspace of exactly the documented partial rows."""
    M, d = case["G"].shape
    row_index = case["row_index"] if row_index is None else row_index
    nb = L.hriemo_add_ln_bwd_partial_rows(M, d)
    if reduce:
        ws = R.GuardedVec(L.hriemo_add_ln_bwd_workspace_bytes(M, d) // 4, torch.float32, guard=1024, device=DEV)
    else:
        ws = R.Guarded(nb, 3 * d, torch.float32, j=0, guard=16, device=DEV)
    outs = {}
    for n in NAMES3:
        if reduce and (n != "dbias" or dbias):
            outs[n] = vec(init[n]) if accumulate else R.GuardedVec(d, torch.float32, device=DEV)
        else:
            outs[n] = None
    bufs = {"dY": mat(case["dY"]), "G": mat(case["G"]), "X": mat(case["X"]), "X32": mat(case["X32"]), "gamma": vec(case["gamma"]),
            "mean": vec(m32), "rstd": vec(r32), "dX": R.Guarded(M, d, torch.bfloat16, j=0, device=DEV) if dX else None,
            "dG": R.Guarded(M, d, torch.bfloat16, j=0, device=DEV) if dG else None, "workspace": ws,
            "row_index": None if row_index is None else vec(torch.from_numpy(np.asarray(row_index, dtype=np.int64))),
            "seed word": None if seed_word is None else vec(torch.tensor([seed_word], dtype=torch.int64))}
    bufs.update(outs)
    b = bufs
    head = (b["dY"].ptr, b["G"].ptr, ptr(b["X"]), ptr(b["X32"]), b["gamma"].ptr, b["mean"].ptr, b["rstd"].ptr, ptr(b["dX"]), ptr(b["dG"]),
            ptr(b["dgamma"]), ptr(b["dbeta"]), ptr(b["dbias"]), int(accumulate), M, d, case["p"], case["seed"] if seed is None else seed,
            ptr(b["seed word"]), case["site"], case["row_offset"] if row_offset is None else row_offset, ws.ptr)
    if rows_entry or row_index is not None:
        call("hriemo_add_ln_bwd_rows", *head, ptr(b["row_index"]), stream())
    else:
        call("hriemo_add_ln_bwd", *head, stream())
    intact(bufs, name)
    got = {n: (None if b[n] is None else b[n].view.cpu()) for n in ("dX", "dG") + NAMES3}
    got["partials"] = None if reduce else ws.view.cpu()
    got["nb"] = nb
    return got


def make(c, row_index=None):
    M, d, fam, p, res, quad, roff = c
    case = R.ln_case(M, d, fam, p, res, roff, row_index)
    fwd = R.ln_fwd_ref(case)
    m32, r32 = R.stats32(fwd)
    return case, fwd, m32, r32


def judge(case, fwd, m32, r32, name, got_f=None, got_b=None, init=None, accumulate=False):
    fw, bw = R.ln_yardsticks(case, m32 if got_b is not None else None, r32, cols=False)
    out = {}
    if got_f is not None:
        out.update(R.check_ln_fwd(got_f, case, fwd, fw, name))
    if got_b is not None:
        ref = R.ln_bwd_ref(case, m32, r32, init if accumulate else None)
        out.update(R.check_ln_bwd(got_b, case, ref, bw, name, accumulate))
    print(name, {k: round(v, 3) for k, v in out.items()})
    return out


# ------------------------------------------------------------------------------------------------ 1. add_ln at its edges
@pytest.mark.parametrize("c", R.LN_CASES, ids=R.case_id)
def test_add_ln_forward_and_backward(L, variant, c):
    """gap 1: d = 2056 and 4096 run the NCH = 8 (gamma / beta reloaded per row) instances; gap 2: 16389 rows stride every row loop;
    gap 4: rstd and mean are judged, on offset, constant, all-zero and fully dropped rows too"""
    M, d, fam, p, res, quad, roff = c
    variant(0 if quad else 1)
    case, fwd, m32, r32 = make(c)
    name = R.case_id(c)
    got_f = run_fwd(case, name)
    got_b = run_bwd(L, case, m32, r32, name)
    judge(case, fwd, m32, r32, name, got_f, got_b)
    if fam in ("const", "zero"):        # gap 4: zero variance -- y is beta to fp32 rounding, rstd is eps^-1/2, the backward finite
        assert (got_f["y32"].double() - case["beta"].double()).abs().max() <= R.V * case["beta"].abs().max()
        assert torch.equal(got_f["y"], case["beta"].bfloat16().expand(M, d))
        assert (got_f["rstd"].double() * R.EPS ** 0.5 - 1).abs().max() <= 4 * R.V
    if p == 0.9:                        # gap 4: rows with every element of g dropped
        dead = (~case["keep"]).all(1)
        assert int(dead.sum()) >= 1
        assert (got_b["dG"][dead] == 0).all() and (got_b["dG"][~case["keep"]] == 0).all()
    if M == R.M_STRIDE:                 # gap 2: the second trip is proven, not assumed
        assert got_b["nb"] * 4 < M, (got_b["nb"], "the backward grid covers every row in one trip")
        assert M > 4 * 4096 and M > 2 * 4 * 8 * 256, "forward grids: 4096 blocks (chunk), at most 8 blocks x 256 CUs resident (quad)"


@pytest.mark.parametrize("M", [5, 257])
@pytest.mark.parametrize("d,quad", [(520, False), (768, True)])
def test_add_ln_operand_forms(L, variant, M, d, quad):
    """gap 5: Y32 absent, dX / dG / dbias absent in turn (two segments in a 3d stride), accumulate = 1 into non-zero destinations on
    both sides of the 64-partial threshold of the two-level reduce (M = 257: 65 partial rows).
    With the quad mapping selected (d = 768) only the dbias-absent and the accumulating calls run the quad kernels: the library takes
    them with Y32, dX and dG all present and otherwise falls back to the chunk-mapped kernels at d = 768, which is what the calls
    without Y32, dX or dG check there (the fall-back under the quad setting, not the quad kernels)."""
    variant(0 if quad else 1)
    c = (M, d, "unit", 0.1, "x32", quad, 500)
    case, fwd, m32, r32 = make(c)
    name = f"forms {R.case_id(c)}"
    judge(case, fwd, m32, r32, name + " no Y32", run_fwd(case, name, want32=False))
    for form in ({"dX": False}, {"dG": False}, {"dbias": False}, {"dX": False, "dG": False}):
        got = run_bwd(L, case, m32, r32, f"{name} {form}", **form)
        judge(case, fwd, m32, r32, f"{name} {form}", None, got)
        assert all(got[k] is None for k, v in form.items() if not v)
    g = torch.Generator().manual_seed(M + d)
    init = {n: 1.0 + torch.rand(d, generator=g) for n in NAMES3}
    for form in ({}, {"dbias": False}):
        got = run_bwd(L, case, m32, r32, f"{name} accumulate {form}", accumulate=True, init=init, **form)
        judge(case, fwd, m32, r32, f"{name} accumulate {form}", None, got, init, True)
    if M == 257:
        assert got["nb"] == 65


@pytest.mark.parametrize("M", [5, 257])
def test_add_ln_quad_without_dropout_writes_dx_once(L, variant, M):
    """gap 5: the quad path's dG = dX alias (p = 0, dG == NULL), plain and accumulating"""
    variant(0)
    c = (M, 512, "unit", 0.0, "x32", True, 0)
    case, fwd, m32, r32 = make(c)
    init = {n: torch.full((512,), -2.0) for n in NAMES3}
    for acc in (False, True):
        got = run_bwd(L, case, m32, r32, f"alias M={M} acc={acc}", dG=False, accumulate=acc, init=init)
        judge(case, fwd, m32, r32, f"alias M={M} acc={acc}", None, got, init, acc)
    full = run_bwd(L, case, m32, r32, "alias, both outputs")
    assert torch.equal(full["dX"], got["dX"]) and torch.equal(full["dG"], full["dX"])


# ------------------------------------------------------------------------------------------------ 2. row maps, seed word, partials, errors
@pytest.mark.parametrize("d,quad", [(520, False), (2056, False), (256, True), (768, True)])
def test_add_ln_row_index_keys_the_mask(L, variant, d, quad):
    """gap 3: the _rows entry points on both mappings (the quad kernels' hash_row) with a permuted, gappy row_index: the mask is
    the one rows_mask_at predicts, seen through dG == 0 exactly where dropped and through y against the reference built with it;
    row_index = arange(M) + k equals the plain entry point with row_offset + k bit for bit"""
    variant(0 if quad else 1)
    M, k = 37, 4242
    rows = np.random.RandomState(d).permutation(3 * M)[:M].astype(np.int64)
    c = (M, d, "unit", 0.3, "x32", quad, 1000)
    case, fwd, m32, r32 = make(c, rows)
    plain = R.ln_case(M, d, "unit", 0.3, "x32", 1000)
    assert not torch.equal(plain["keep"], case["keep"])
    name = f"row_index {R.case_id(c)}"
    got_f = run_fwd(case, name)
    got_b = run_bwd(L, case, m32, r32, name)
    judge(case, fwd, m32, r32, name, got_f, got_b)
    assert (got_b["dG"][~case["keep"]] == 0).all()
    assert (got_b["dG"][case["keep"]] != 0).float().mean() > 0.99
    shifted_f = run_fwd(plain, name + " arange + k", rows_entry=True, row_index=np.arange(M) + k)
    plain_f = run_fwd(plain, name + " offset + k", row_offset=1000 + k)
    shifted_b = run_bwd(L, plain, m32, r32, name + " arange + k", rows_entry=True, row_index=np.arange(M) + k)
    plain_b = run_bwd(L, plain, m32, r32, name + " offset + k", row_offset=1000 + k)
    for n in ("y", "y32", "mean", "rstd"):
        assert torch.equal(shifted_f[n], plain_f[n]), n
    for n in ("dX", "dG") + NAMES3:
        assert torch.equal(shifted_b[n], plain_b[n]), n
    assert not torch.equal(plain_f["y"], run_fwd(plain, name + " offset")["y"])


@pytest.mark.parametrize("d,quad", [(520, False), (512, True)])
def test_add_ln_device_seed_word(L, variant, d, quad):
    """gap 10: with a private device word holding k the kernels draw the mask of seed + k"""
    variant(0 if quad else 1)
    k = 0x9E3779B97F4A7C15 >> 1
    c = (9, d, "unit", 0.3, "x32", quad, 1000)
    case, fwd, m32, r32 = make(c)
    name = f"seed word {R.case_id(c)}"
    a_f = run_fwd(case, name + " word", seed_word=k)
    b_f = run_fwd(case, name + " NULL", seed=case["seed"] + k)
    a_b = run_bwd(L, case, m32, r32, name + " word", seed_word=k)
    b_b = run_bwd(L, case, m32, r32, name + " NULL", seed=case["seed"] + k)
    for n in ("y", "y32", "mean", "rstd"):
        assert torch.equal(a_f[n], b_f[n]), n
    for n in ("dX", "dG") + NAMES3:
        assert torch.equal(a_b[n], b_b[n]), n
    assert not torch.equal(a_f["y"], run_fwd(case, name + " seed alone")["y"])
    moved = dict(case, seed=case["seed"] + k, keep=R.keep_mask(9, d, 0.3, case["seed"] + k, case["site"], R.row_keys(9, 1000)))
    f2 = R.ln_fwd_ref(moved)
    judge(moved, f2, *R.stats32(f2), name + " against the host mask", a_f)


@pytest.mark.parametrize("M,d,quad", [(5, 520, False), (257, 520, False), (257, 2056, False), (257, 768, True), (R.M_STRIDE, 256, True)])
def test_add_ln_partial_only_form(L, variant, M, d, quad):
    """gap 7: dgamma == NULL leaves exactly hriemo_add_ln_bwd_partial_rows rows of 3d floats, every element written, nothing behind
    them; their float64 sum obeys the dgamma / dbeta / dbias limits"""
    variant(0 if quad else 1)
    c = (M, d, "unit", 0.1, "x32", quad, 77)
    case, fwd, m32, r32 = make(c)
    got = run_bwd(L, case, m32, r32, f"partials {R.case_id(c)}", reduce=False)
    P = got["partials"]
    assert P.shape == (got["nb"], 3 * d) and torch.isfinite(P).all()
    ref = R.ln_bwd_ref(case, m32, r32)
    total = P.double().sum(0)
    for i, n in enumerate(NAMES3):
        R.check_elem(total[i * d:(i + 1) * d], ref[n], ref["mag_" + n], R.bwd_sum_factor(n, M), True, n)
    if M == R.M_STRIDE:
        assert got["nb"] * 4 < M


def test_add_ln_error_returns_leave_the_outputs_alone(L):
    M, d = 4, 520
    case, fwd, m32, r32 = make((M, d, "unit", 0.0, "x16", False, 0))
    G, X, dY, gam, bet = mat(case["G"]), mat(case["X"]), mat(case["dY"]), vec(case["gamma"]), vec(case["beta"])
    mean, rstd = vec(m32), vec(r32)
    for Mb, db, ws_null in ((M, 12, False), (M, 4104, False), (0, d, False), (M, d, True)):
        outs = {"Y": R.Guarded(M, d, torch.bfloat16, j=0, device=DEV), "Y32": R.Guarded(M, d, torch.float32, j=0, device=DEV),
                "mean": R.GuardedVec(M, torch.float32, device=DEV), "rstd": R.GuardedVec(M, torch.float32, device=DEV),
                "dX": R.Guarded(M, d, torch.bfloat16, j=0, device=DEV), "dG": R.Guarded(M, d, torch.bfloat16, j=0, device=DEV),
                "ws": R.GuardedVec(L.hriemo_add_ln_bwd_workspace_bytes(M, d) // 4, torch.float32, device=DEV)}
        outs.update({n: R.GuardedVec(d, torch.float32, device=DEV) for n in NAMES3})
        o = outs
        if not ws_null:
            with pytest.raises(RuntimeError, match=r"hriemo_add_ln_fwd failed \(\d+\): \S+"):
                call("hriemo_add_ln_fwd", G.ptr, X.ptr, None, gam.ptr, bet.ptr, o["Y"].ptr, o["Y32"].ptr, o["mean"].ptr, o["rstd"].ptr,
                     Mb, db, R.EPS, 0.0, 1, None, 1, 0, stream())
        with pytest.raises(RuntimeError, match=r"hriemo_add_ln_bwd failed \(\d+\): \S+"):
            call("hriemo_add_ln_bwd", dY.ptr, G.ptr, X.ptr, None, gam.ptr, mean.ptr, rstd.ptr, o["dX"].ptr, o["dG"].ptr, o["dgamma"].ptr,
                 o["dbeta"].ptr, o["dbias"].ptr, 0, Mb, db, 0.0, 1, None, 1, 0, None if ws_null else o["ws"].ptr, stream())
        intact(outs, "error return")
        assert all(untouched(b) for b in outs.values()), (Mb, db, ws_null)


# ------------------------------------------------------------------------------------------------ 3. reduce, column sum, rowdot
def test_colreduce_batch_table_of_64_jobs(L):
    """gap 6: hriemo_colreduce_batch alone -- the binary search on first_block, w that is no multiple of 32, the four-way unrolled
    row loop and its tail, 1 / 2 / 3 segments in a wider stride, mixed accumulate bits, two argument uploads (64 > 48 jobs)"""
    g = torch.Generator().manual_seed(64)
    shapes = [(w, n) for w in R.REDUCE_W for n in R.REDUCE_NP] * 2
    jobs = []
    for j, (w, n) in enumerate(shapes):
        nseg, integer, acc = 1 + j % 3, j < len(shapes) // 2, (j // 2) % 2 == 1
        P = torch.randint(-8, 9, (n, nseg * w), generator=g).float() if integer else torch.randn(n, nseg * w, generator=g)
        inits = [(torch.randint(-8, 9, (w,), generator=g).float() if integer else torch.randn(w, generator=g)) for _ in range(nseg)]
        jobs.append({"w": w, "np": n, "nseg": nseg, "integer": integer, "acc": acc, "P": P, "inits": inits,
                     "part": R.Guarded.of(P, j=1, guard=4, device=DEV),            # pstride = nseg * w + 8, the gap poisoned
                     "outs": [vec(i) if acc else R.GuardedVec(w, torch.float32, device=DEV) for i in inits]})
    first, nblocks = R.first_blocks([(jb["w"], jb["nseg"]) for jb in jobs])
    table = torch.zeros(len(jobs), 8, dtype=torch.int64)
    for j, jb in enumerate(jobs):
        assert jb["part"].ld > jb["nseg"] * jb["w"]
        table[j, :5] = torch.tensor([jb["part"].ptr, jb["part"].ld, jb["np"], jb["w"], jb["nseg"] | (int(jb["acc"]) << 8) | (first[j] << 32)])
        for sg, o in enumerate(jb["outs"]):
            table[j, 5 + sg] = o.ptr
    assert len(jobs) == 64 and {jb["nseg"] for jb in jobs} == {1, 2, 3}
    dev = R.GuardedVec(len(jobs) * 8, torch.int64, device=DEV)
    call("hriemo_colreduce_batch", table.data_ptr(), len(jobs), dev.ptr, nblocks, stream())
    torch.cuda.synchronize()
    dev.assert_intact("job table")
    assert torch.equal(dev.view.cpu().view(-1, 8), table)
    for j, jb in enumerate(jobs):
        name = f"job {j}: w={jb['w']} np={jb['np']} nseg={jb['nseg']} acc={jb['acc']} {'integer' if jb['integer'] else 'real'}"
        jb["part"].assert_intact(name + " partials")
        refs = R.reduce_ref(jb["P"], jb["w"], jb["nseg"], jb["inits"] if jb["acc"] else None)
        for sg, (o, (ref, mag)) in enumerate(zip(jb["outs"], refs)):
            o.assert_intact(f"{name} segment {sg}")
            got = o.view.cpu()
            R.check_sum(got, ref, mag, jb["np"] + int(jb["acc"]), f"{name} segment {sg}")
            if jb["np"] == 1 and not jb["acc"]:
                assert torch.equal(got, jb["P"][0, sg * jb["w"]:(sg + 1) * jb["w"]]), f"{name} segment {sg}: one partial row is a copy"
            if jb["integer"]:
                assert torch.equal(got.double(), ref), f"{name} segment {sg}: integer partials must sum exactly"


@pytest.mark.parametrize("N", R.COLSUM_N)
@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum_bf16(L, M, N):
    """gap 8: ldx > N with poisoned padding (column slices of projection buffers), M < 16, a second column group (N = 520),
    rows_per_slice > 16 (M = 32785), accumulate on and off; gap 7: out == NULL leaves exactly hriemo_colsum_partial_rows rows"""
    g = torch.Generator().manual_seed(M * 1000 + N)
    rows = L.hriemo_colsum_partial_rows(M, N)
    if M == 32785:
        assert (M + rows - 1) // rows > 16
    for integer in (True, False):
        X = (torch.randint(-4, 5, (M, N), generator=g).float() if integer else torch.randn(M, N, generator=g)).bfloat16()
        for j in (1, 0):                                   # ldx = N + 8 | N
            Xb = R.Guarded.of(X, j=j, device=DEV)
            for acc in (False, True):
                name = f"colsum {M}x{N} ld={Xb.ld} acc={acc} {'integer' if integer else 'real'}"
                init = torch.randint(-8, 9, (N,), generator=g).float() if integer else torch.randn(N, generator=g)
                out = vec(init) if acc else R.GuardedVec(N, torch.float32, device=DEV)
                ws = R.GuardedVec(L.hriemo_colsum_workspace_bytes(M, N) // 4, torch.float32, guard=1024, device=DEV)
                call("hriemo_colsum_bf16", Xb.ptr, Xb.ld, M, N, out.ptr, int(acc), ws.ptr, stream())
                intact({"X": Xb, "out": out, "workspace": ws}, name)
                ref, mag = R.colsum_ref(X, init if acc else None)
                got = out.view.cpu()
                R.check_sum(got, ref, mag, M + int(acc), name)
                if M == 1 and not acc:
                    assert torch.equal(got, X[0].float()), name + ": one row is a convert"
                if integer:
                    assert torch.equal(got.double(), ref), name
            part = R.Guarded(rows, N, torch.float32, j=0, guard=16, device=DEV)
            call("hriemo_colsum_bf16", Xb.ptr, Xb.ld, M, N, None, 0, part.ptr, stream())
            intact({"X": Xb, "partials": part}, "colsum partials")
            P = part.view.cpu()
            ref, mag = R.colsum_ref(X)
            R.check_sum(P.double().sum(0), ref, mag, M, f"colsum {M}x{N} partial rows")      # (non-finite: a row never written)


@pytest.mark.parametrize("d", R.ROWDOT_D)
@pytest.mark.parametrize("M", R.ROWDOT_M)
def test_rowdot_forward_and_backward(L, M, d):
    """gap 9: more than 32 rows (the second trip of the backward's row loop; 385 rows: a ragged 13th), Z32, accumulate, b == NULL,
    d that is no multiple of 32"""
    g = torch.Generator().manual_seed(M * 1000 + d)
    Z32 = torch.randn(M, d, generator=g)
    w, b, dl = torch.randn(d, generator=g), torch.randn(1, generator=g), torch.randn(M, generator=g)
    dw0, db0 = torch.randn(d, generator=g), torch.randn(1, generator=g)
    for twin in (False, True):
        Z = Z32 if twin else Z32.bfloat16()
        Zb, wb, bb, dlb = mat(Z), vec(w), vec(b), vec(dl)
        z16, z32 = (None, Zb.ptr) if twin else (Zb.ptr, None)
        for bias in (True, False):
            name = f"rowdot {M}x{d} {'Z32' if twin else 'Z'} {'b' if bias else 'no b'}"
            out = R.GuardedVec(M, torch.float32, device=DEV)
            call("hriemo_rowdot_fwd", z16, z32, wb.ptr, bb.ptr if bias else None, out.ptr, M, d, stream())
            intact({"Z": Zb, "w": wb, "b": bb, "logits": out}, name)
            ref, mag = R.rowdot_fwd_ref(Z, w, b if bias else None)
            R.check_sum(out.view.cpu(), ref, mag, d + int(bias), name + " logits")
        for acc in (False, True):
            name = f"rowdot {M}x{d} {'Z32' if twin else 'Z'} acc={acc}"
            dZ = R.Guarded(M, d, torch.bfloat16, j=0, device=DEV)
            dw = vec(dw0) if acc else R.GuardedVec(d, torch.float32, device=DEV)
            db = vec(db0) if acc else R.GuardedVec(1, torch.float32, device=DEV)
            call("hriemo_rowdot_bwd", dlb.ptr, z16, z32, wb.ptr, dZ.ptr, dw.ptr, db.ptr, int(acc), M, d, stream())
            intact({"Z": Zb, "w": wb, "dl": dlb, "dZ": dZ, "dw": dw, "db": db}, name)
            rZ, (rw, mw), (rb, mb) = R.rowdot_bwd_ref(dl, Z, w, dw0 if acc else None, db0 if acc else None)
            assert torch.equal(dZ.view.cpu(), rZ), name + ": dZ is not bf16(dl * w)"
            R.check_sum(dw.view.cpu(), rw, mw, M + int(acc), name + " dw")
            R.check_sum(db.view.cpu(), rb, mb, M + int(acc), name + " db")
