"""GPU suite, fp32-mode attention (hri-emo_amd/csrc/fp32mode.hip) through the C ABI against fp32_reference.py: hriemo_attn_fwd_f32,
hriemo_attn_bwd_f32 (both of its kernels), hriemo_attn_probs_f32 and their three _varlen forms, at every case of
fp32_reference.ATTN_CASES -- every head width, the 16-row sub-tile and 64-row tile edges in both sequence lengths, every
key-padding pattern, dropout off and on.

Every operand and every output sits in a guarded buffer filled with 0xFF (NaN as fp32): Q, O, dO, dQ with ld = d + 8; K | V and
dK | dV as the halves of one [rows, 2d] buffer with ld = 2d + 8; lse, delta and the maps between guards.  A guard that is read
poisons the result, a guard that is written fails the test.  PAD key rows hold ordinary finite values (the padded path's contract).
The limits come from the float64 reference and the fp32 yardsticks on the CPU alone (test_fp32_bound_host.py proves their teeth);
each test prints its worst error / limit per output (profiles/2026-10-19_fp32_kernel_limits.log is one run of them)."""
import pytest
import torch

import attn_reference as A
import fp32_reference as F
import rowops_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def mat(x, **kw):
    return F.Guarded.of(x, j=1, guard=GUARD, device=DEV, **kw)


def out_mat(rows, cols):
    return F.Guarded(rows, cols, torch.float32, j=1, guard=GUARD, device=DEV)


def vec(x):
    return F.GuardedVec.of(x, device=DEV)


def out_vec(n):
    return F.GuardedVec(n, torch.float32, device=DEV)


def untouched(b, rows=None):
    v = b.view if rows is None else b.view[rows]
    return bool((v.contiguous().view(torch.uint8) == 0xFF).all())


class Launch:
    """the buffers of one problem and its launches.  rows_q / rows_k: the rows of the padded layout that a packed launch owns
    (followed by PACKED_SURPLUS rows that stay 0xFF); cu: (cu_q, cu_k) int32 lists of a packed launch."""

    def __init__(self, L, c, packed=False, seed=None, seed_word=None, out_l=None):
        self.L, self.c, self.packed = L, c, packed
        B, H, Lq, Lk, d = c["B"], c["H"], c["Lq"], c["Lk"], c["d"]
        q, kv, do = c["q"], c["kv"], c["do"]
        self.nq, self.nk = B * Lq, B * Lk
        b = {}
        if packed:
            q, kv, do = q[c["rows_q"]], kv[c["rows_k"]], do[c["rows_q"]]
            self.nq, self.nk = q.shape[0], kv.shape[0]
            sq, sk = self.nq + F.PACKED_SURPLUS, self.nk + F.PACKED_SURPLUS
            for n, x, rows in (("Q", q, sq), ("KV", kv, sk), ("dO", do, sq)):
                b[n] = F.Guarded(rows, x.shape[1], torch.float32, j=1, guard=GUARD, device=DEV)
                b[n].view[:x.shape[0]].copy_(x)
            cuq = torch.cat([torch.zeros(1, dtype=torch.long), c["lens_q"].cumsum(0)]).int()
            cuk = torch.cat([torch.zeros(1, dtype=torch.long), c["lens_k"].cumsum(0)]).int()
            b["cu_q"], b["cu_k"] = vec(cuq), vec(cuk)
            b["kpm"] = None
        else:
            sq, sk = self.nq, self.nk
            b["Q"], b["KV"], b["dO"] = mat(q), mat(kv), mat(do)
            b["kpm"] = None if c["kpm"] is None else vec(c["kpm"].view(torch.uint8).reshape(-1))
        self.out_lq, self.out_lk = (Lq, Lk) if out_l is None else out_l
        b["O"], b["dQ"], b["dKV"] = out_mat(sq, d), out_mat(sq, d), out_mat(sk, 2 * d)
        b["lse"], b["delta"], b["map"] = out_vec(B * H * Lq), out_vec(B * H * Lq), out_vec(B * self.out_lq * self.out_lk)
        b["seed word"] = None if seed_word is None else vec(torch.tensor([seed_word], dtype=torch.int64))
        self.b = b
        self.seed = F.SEED if seed is None else seed
        self.outputs = ("O", "dQ", "dKV", "lse", "delta", "map")

    # ---- argument lists (o: overrides for the refusal tests)
    def _drop(self, o):
        sw = self.b["seed word"]
        return (o.get("p", self.c["p"]), self.seed, None if sw is None else sw.ptr, F.SITE, F.B_OFFSET, stream())

    def _dims(self, o):
        c = self.c
        return (c["B"], c["H"], c["Lq"], c["Lk"], o.get("hd", c["hd"]))

    def _mask_or_cu(self, o):
        b = self.b
        if self.packed:
            return (o.get("cu_q", b["cu_q"].ptr), o.get("cu_k", b["cu_k"].ptr))
        return (o.get("kpm", None if b["kpm"] is None else b["kpm"].ptr),)

    def fwd(self, **o):
        b, d = self.b, self.c["d"]
        ldq, ldkv = o.get("ldq", b["Q"].ld), b["KV"].ld
        args = (b["Q"].ptr + o.get("q_off", 0), ldq, b["KV"].ptr, ldkv, b["KV"].ptr + 4 * d, ldkv, b["O"].ptr, b["O"].ld) + self._mask_or_cu(o) \
            + (b["lse"].ptr,) + self._dims(o) + self._drop(o)
        return getattr(self.L, "hriemo_attn_fwd_f32_varlen" if self.packed else "hriemo_attn_fwd_f32")(*args)

    def bwd(self, **o):
        b, d = self.b, self.c["d"]
        ldq, ldkv = o.get("ldq", b["Q"].ld), b["KV"].ld
        args = (b["Q"].ptr + o.get("q_off", 0), ldq, b["KV"].ptr, ldkv, b["KV"].ptr + 4 * d, ldkv, b["O"].ptr, b["O"].ld, b["dO"].ptr, b["dO"].ld) \
            + self._mask_or_cu(o) + (b["lse"].ptr, b["dQ"].ptr, b["dQ"].ld, b["dKV"].ptr, b["dKV"].ld, b["dKV"].ptr + 4 * d, b["dKV"].ld,
                                     b["delta"].ptr) + self._dims(o) + self._drop(o)
        return getattr(self.L, "hriemo_attn_bwd_f32_varlen" if self.packed else "hriemo_attn_bwd_f32")(*args)

    def probs(self, **o):
        b = self.b
        args = (b["Q"].ptr + o.get("q_off", 0), o.get("ldq", b["Q"].ld), b["KV"].ptr, b["KV"].ld) + self._mask_or_cu(o) + (b["lse"].ptr, b["map"].ptr)
        c = self.c
        if self.packed:
            args += (c["B"], c["H"], c["Lq"], c["Lk"], o.get("out_lq", self.out_lq), self.out_lk, o.get("hd", c["hd"]))
            return self.L.hriemo_attn_probs_f32_varlen(*(args + self._drop(o)))
        return self.L.hriemo_attn_probs_f32(*(args + self._dims(o) + self._drop(o)))

    def ok(self, rc, what):
        assert rc == 0, (what, self.L.hriemo_last_error().decode())

    def run_all(self):
        self.ok(self.fwd(), "fwd")
        self.ok(self.probs(), "probs")
        self.ok(self.bwd(), "bwd")
        torch.cuda.synchronize()
        return self

    def intact(self, name):
        torch.cuda.synchronize()
        for n, buf in self.b.items():
            if buf is not None:
                buf.assert_intact(f"{name}: {n}")

    # ---- results in the PADDED layout on the CPU: rows a packed launch does not own are 0
    def _rows(self, x, rows, n):
        if not self.packed:
            return x.cpu()
        full = torch.zeros(n, x.shape[1])
        full[rows] = x[:rows.numel()].cpu()
        return full

    def results(self):
        c, b = self.c, self.b
        B, H, Lq, Lk, hd, d = c["B"], c["H"], c["Lq"], c["Lk"], c["hd"], c["d"]
        r = {"O": self._rows(b["O"].view, c.get("rows_q"), B * Lq), "dQ": self._rows(b["dQ"].view, c.get("rows_q"), B * Lq)}
        dkv = self._rows(b["dKV"].view, c.get("rows_k"), B * Lk)
        out = {"O": A.heads(r["O"], B, Lq, H, hd), "dQ": A.heads(r["dQ"], B, Lq, H, hd), "dK": A.heads(dkv[:, :d], B, Lk, H, hd),
               "dV": A.heads(dkv[:, d:], B, Lk, H, hd), "lse": b["lse"].view.cpu().reshape(B, H, Lq, 1).double(),
               "delta": b["delta"].view.cpu().reshape(B, H, Lq).double(),
               "Pmean": b["map"].view.cpu().reshape(B, 1, self.out_lq, self.out_lk).double()}
        return out


def report(name, ratios):
    print(f"fp32 limits {name}: " + "  ".join(f"{o} {e:.3f}/{t:.3f}" if isinstance(v, tuple) else f"{o} {v:.3f}"
                                              for o, v in ratios.items() for e, t in [v if isinstance(v, tuple) else (v, v)]))


def check_live(run, c, name, valid_q=None):
    """the live samples against the limits of fp32_reference; returns the ratios"""
    got = run.results()
    lv = c["live"]
    g = {o: got[o][lv] for o in F.ATTN_OUTPUTS}
    g["Pmean"] = g["Pmean"][:, :, :c["Lq"], :c["Lk"]]
    if valid_q is not None:                       # rows a packed launch never writes: lse / delta slots stay 0xFF
        w = valid_q[:, None, :, None]
        assert bool(torch.isnan(g["lse"][~w.expand_as(g["lse"])]).all()), f"{name}: lse slots past a sample's length were written"
        g["lse"] = torch.where(w, g["lse"], torch.zeros((), dtype=torch.float64))
    ratios = F.check_attn_all(g, c, name, valid_q=valid_q)
    dref, dmag = F.delta_ref(c)
    dl = got["delta"][lv]
    if valid_q is not None:
        w = valid_q[:, None, :]
        dl, dref, dmag = torch.where(w, dl, torch.zeros((), dtype=torch.float64)), dref * w, dmag * w
    ratios["delta"] = R.check_elem(dl, dref, dmag, F.delta_factor(c["hd"]), True, f"{name} delta")
    return ratios, got


# ------------------------------------------------------------------------------------------------ padded launches
@pytest.mark.parametrize("case", [c for c in F.ATTN_CASES if c[0] == "padded"], ids=F.attn_id)
def test_attention_f32_padded(L, case):
    """O, lse, dQ, dK, dV, delta and the head-mean map of the padded entries inside their limits; PAD keys' dK / dV rows and the
    map's PAD columns exactly 0 (their magnitude is 0); a sample with every key PAD: O, dQ and its map rows NaN, lse -inf"""
    c = F.attn_case(case)
    name = F.attn_id(case)
    run = Launch(L, c).run_all()
    run.intact(name)
    ratios, got = check_live(run, c, name)
    report(name, ratios)
    if c["kpm"] is not None and c["kpm"][c["live"]].any():
        pad = c["kpm"][:, None, :, None].expand_as(got["dK"])
        live = c["live"][:, None, None, None]
        assert float(got["dK"][pad & live].abs().max()) == 0.0 and float(got["dV"][pad & live].abs().max()) == 0.0
        pm = got["Pmean"][c["live"]][:, 0]
        assert float(pm.transpose(1, 2)[c["kpm"][c["live"]]].abs().max()) == 0.0
    for b in (~c["live"]).nonzero().reshape(-1).tolist():
        assert bool(torch.isnan(got["O"][b]).all()) and bool(torch.isnan(got["dQ"][b]).all()) and bool(torch.isnan(got["Pmean"][b]).all())
        assert bool((got["lse"][b] == float("-inf")).all())


def test_attention_f32_device_seed_word(L):
    """the dropout seed split between the immediate argument and the device word draws the masks of their sum"""
    case = ("padded", 3, 17, 65, 32, "prefix", 0.1)
    c = F.attn_case(case)
    word = 0x0123456789
    run = Launch(L, c, seed=F.SEED - word, seed_word=word).run_all()
    run.intact("seed word")
    ratios, _ = check_live(run, c, "seed word")
    report("device seed word", ratios)
    other = Launch(L, c, seed=F.SEED - word, seed_word=word + 1).run_all()        # another word, another draw
    assert not torch.equal(other.b["O"].view, run.b["O"].view)


# ------------------------------------------------------------------------------------------------ packed launches
@pytest.mark.parametrize("case", [c for c in F.ATTN_CASES if c[0] == "packed"], ids=F.attn_id)
def test_attention_f32_packed(L, case):
    """the _varlen entries on cu_seqlens built from the edge lengths (q and k independently, one empty sample in the middle):
    inside the float64 limits, bit-identical to the padded launch under the equivalent prefix mask, surplus rows behind cu[B]
    untouched, and the map -- asked for with out_lq > max_len_q, out_lk > max_len_k -- written everywhere, exact zeros past the lengths"""
    c = F.attn_case(case)
    name = F.attn_id(case)
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    run = Launch(L, c, packed=True, out_l=(Lq + 3, Lk + 7)).run_all()
    run.intact(name)
    for n in ("O", "dQ", "dKV"):
        rows = run.nk if n == "dKV" else run.nq
        assert untouched(run.b[n], slice(rows, None)), f"{name}: surplus rows of {n} were written"
        assert bool(torch.isfinite(run.b[n].view[:rows]).all()), f"{name}: {n} has rows that were not written"
    valid_q = (torch.arange(Lq)[None] < c["lens_q"][:, None])
    ratios, got = check_live(run, c, name, valid_q[c["live"]])
    report(name, ratios)
    # the map: every element written, zeros outside [lens_q, lens_k]
    pm = got["Pmean"][:, 0]
    assert bool(torch.isfinite(pm).all()), f"{name}: map elements that were not written"
    inside = valid_q[:, :, None] & (torch.arange(Lk)[None, None] < c["lens_k"][:, None, None])
    outside = torch.ones_like(pm, dtype=torch.bool)
    outside[:, :Lq, :Lk] = ~inside
    assert float(pm[outside].abs().max()) == 0.0
    # == the padded launch, bit for bit, on every row the packed launch owns
    ref = Launch(L, c).run_all()
    rq, rk = c["rows_q"].to(DEV), c["rows_k"].to(DEV)
    for n, rows, cnt in (("O", rq, run.nq), ("dQ", rq, run.nq), ("dKV", rk, run.nk)):
        assert torch.equal(run.b[n].view[:cnt], ref.b[n].view.index_select(0, rows)), f"{name}: packed {n} differs from the padded launch"
    vq = valid_q[:, None, :].expand(B, H, Lq).reshape(-1).to(DEV)
    for n in ("lse", "delta"):
        assert torch.equal(run.b[n].view[vq], ref.b[n].view[vq]), f"{name}: packed {n} differs from the padded launch"
    pmap = ref.b["map"].view.reshape(B, Lq, Lk)
    ins = inside.to(DEV)
    assert torch.equal(run.b["map"].view.reshape(B, Lq + 3, Lk + 7)[:, :Lq, :Lk][ins], pmap[ins]), f"{name}: packed map differs from the padded launch"


# ------------------------------------------------------------------------------------------------ refusals
REFUSALS = [  # (id, packed, entries, overrides)
    ("hd48", False, ("fwd", "bwd", "probs"), {"hd": 48}),
    ("hd48-packed", True, ("fwd", "bwd", "probs"), {"hd": 48}),
    ("ld-not-multiple-of-4", False, ("fwd", "bwd", "probs"), {"ldq": 42}),
    ("ld-not-multiple-of-4-packed", True, ("fwd", "bwd", "probs"), {"ldq": 42}),
    ("pointer-off-by-4-bytes", False, ("fwd", "bwd", "probs"), {"q_off": 4}),
    ("pointer-off-by-4-bytes-packed", True, ("fwd", "bwd", "probs"), {"q_off": 4}),
    ("p1", False, ("fwd", "bwd", "probs"), {"p": 1.0}),
    ("p1-packed", True, ("fwd", "bwd", "probs"), {"p": 1.0}),
    ("packed-null-cu_q", True, ("fwd", "bwd", "probs"), {"cu_q": None}),
    ("packed-null-cu_k", True, ("fwd", "bwd", "probs"), {"cu_k": None}),
    ("map-smaller-than-max_len_q", True, ("probs",), {"out_lq": 4}),
]


@pytest.mark.parametrize("rid,packed,entries,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_attention_f32_refusals(L, rid, packed, entries, over):
    """each refused call returns non-zero, sets hriemo_last_error() and leaves every output byte 0xFF.  (The C ABI of the packed
    entries has no key_padding_mask argument, so 'a packed entry given a mask' cannot be expressed through it; the Python wrapper's
    refusal of that combination is test_attention_f32_wrapper_refuses_a_mask_on_packed_rows.)"""
    if packed:
        c = F.attn_case(("packed", len(F.PACKED_LQ), max(F.PACKED_LQ), max(F.PACKED_LK), 16, "lengths", 0.1))
    else:
        c = F.attn_case(("padded", 3, 5, 7, 16, "prefix", 0.1))
    run = Launch(L, c, packed=packed)
    if packed:
        assert run.out_lq > 4
    for e in entries:
        rc = getattr(run, e)(**over)
        msg = L.hriemo_last_error().decode()
        assert rc != 0 and msg, (rid, e, rc, msg)
        torch.cuda.synchronize()
        for n in run.outputs:
            assert untouched(run.b[n]), f"{rid}: {e} was refused but wrote {n}"
    run.intact(rid)
    print(f"{rid}: {msg}")


def test_attention_f32_wrapper_refuses_a_mask_on_packed_rows(L):
    """hri_emo_amd._fp32.attn / attn_bwd / probs with cu_seqlens AND a key_padding_mask: refused before any launch, nothing written"""
    from hri_emo_amd import _fp32
    d, hd = 32, 16
    q, kv = torch.randn(6, d, device=DEV), torch.randn(6, 2 * d, device=DEV)
    cu = torch.tensor([0, 2, 6], dtype=torch.int32, device=DEV)
    kpm = torch.zeros(2, 4, dtype=torch.uint8, device=DEV)
    lse = torch.zeros(2, 2, 4, device=DEV)
    outs = [torch.full((6, d), 7.0, device=DEV) for _ in range(3)]
    with pytest.raises(RuntimeError, match="key_padding_mask"):
        _fp32.attn(q, kv[:, :d], kv[:, d:], 2, 2, 4, 4, hd, kpm, want_lse=True, drop=None, cu=(cu, cu))
    with pytest.raises(RuntimeError, match="key_padding_mask"):
        _fp32.attn_bwd(q, kv[:, :d], kv[:, d:], q, q, lse, outs[0], outs[1], outs[2], 2, 2, 4, 4, hd, kpm, drop=None, cu=(cu, cu))
    with pytest.raises(RuntimeError, match="key_padding_mask"):
        _fp32.probs(q, kv[:, :d], 2, 2, 4, 4, hd, kpm, lse, drop=None, cu=(cu, cu), out_l=(4, 4))
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
