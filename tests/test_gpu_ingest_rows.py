"""GPU suite of hriemo_ingest_rows, through the C ABI: the module inputs (fp32 / bf16 / fp16; padded and gathered, already packed,
or kept padded) -> bf16 rows, fp32 twin, MX-fp8 copy and row index from ONE launch.  Everything is compared BIT FOR BIT: the twin
with the source, the bf16 rows with torch's CPU cast, the fp8 copy with hriemo_quant_mx8 of the bf16 rows (the kernel that ran
before) and with tests/mx8_emul, the row index with hriemo_pack_rows'.  Every buffer is 0xFF-filled with guard rows on both sides
(and a leading dimension wider than the payload where the ABI has one); PAD rows of a padded source and rows past cu[B] of a packed
one hold 0xFF (NaN in all three formats), so a read of them poisons a result."""
import pytest
import torch

import mx8_emul

pytestmark = pytest.mark.gpu

SENTINEL = 0xFF
GUARD = 4
DT = {"fp32": (torch.float32, 0), "bf16": (torch.bfloat16, 1), "fp16": (torch.float16, 2)}
BITS = {4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}


def ST():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """rows x cols payload of `dtype` in a 0xFF-filled allocation: GUARD rows before and after, leading dimension ld >= cols.
    .t is the (strided) payload, .intact() compares every guard byte, .bits() the payload as CPU integers."""

    def __init__(self, rows, cols, dtype, ld=None, fill=None):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.ld = rows, cols, ld
        self.item = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((rows + 2 * GUARD) * ld * self.item,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.raw.view(dtype).view(rows + 2 * GUARD, ld)[GUARD:GUARD + rows, :cols]
        assert self.t.data_ptr() % 16 == 0
        if fill is not None:
            self.t.copy_(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        by = self.raw.cpu().numpy().reshape(self.rows + 2 * GUARD, self.ld * self.item)
        return bool((by[:GUARD] == SENTINEL).all() and (by[GUARD + self.rows:] == SENTINEL).all() and
                    (by[GUARD:GUARD + self.rows, self.cols * self.item:] == SENTINEL).all())

    def bits(self):
        return self.t.contiguous().view(BITS[self.item]).cpu()

    def untouched(self):
        return bool((self.raw == SENTINEL).all())


def _bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def _plan(lens, L, n_rows):
    """(cu list, [(b, l) | None per destination row])"""
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    rows = [(b, l) for b, n in enumerate(lens) for l in range(n)]
    assert n_rows >= len(rows)
    return cu, rows + [None] * (n_rows - len(rows))


def _values(n, d, kind, seed):
    """[n, d] fp32 values, exactly representable in the source format `kind`, with the edge cases planted in EVERY row:
    columns 0..6 = +0.0, -0.0, 2^-126 (fp16: 2^-14), 1 + 2^-8 and 1 + 3 * 2^-8 (halfway between two bf16 numbers, the even one
    below / above), and for fp16 65504 and its smallest subnormal 2^-24 (else two ordinary values); from d = 64 on, 32-column
    block 1 is all zero in every row and block 2 has one element 2^20 times the rest (at d = 32 there is one block: all zero in
    every fourth row, the spike beside the planted columns in the others).  |x| < 1e30, finite."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    if kind == "fp32":
        x[:, 7::8] *= 1e12                                   # (fp32 only: large and tiny magnitudes across blocks)
        x[:, 5::16] *= 1e-20
    x[:, 0], x[:, 1] = 0.0, -0.0
    x[:, 2] = 2.0 ** -14 if kind == "fp16" else 2.0 ** -126
    x[:, 3], x[:, 4] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8
    if kind == "bf16":
        x[:, 3], x[:, 4] = 1 + 2.0 ** -7, 1 + 3 * 2.0 ** -7  # (a bf16 source holds no halfway case: its two neighbours)
    if kind == "fp16":
        x[:, 5], x[:, 6] = 65504.0, 2.0 ** -24
    spike = lambda col: (torch.randn(n, 32, generator=g) * 2.0 ** -12).index_fill_(1, torch.tensor([col]), 256.0)  # noqa: E731
    if d >= 96:
        x[:, 32:64] = 0.0
        x[:, 64:96] = spike(13)
    elif d == 32:
        x[:, 8:] = spike(21)[:, 8:]
        x[3::4] = 0.0
    planted = x[:, :7].clone()
    x = x.half().float() if kind == "fp16" else x.bfloat16().float() if kind == "bf16" else x
    assert torch.equal(x[:, :5], planted[:, :5]) and (kind != "fp16" or torch.equal(x[:, :7], planted)), "a planted value is not exact"
    assert bool(torch.signbit(x[0, 1])) and not bool(torch.signbit(x[0, 0]))
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 1e30
    return x


def _quant_parent(p16, n_rows, d):
    """hriemo_quant_mx8 of bf16 rows [n_rows, d] -> (bytes [n_rows, d], scale bytes [d/32, n_rows]) on the CPU"""
    from hri_emo_amd import _lib
    ld = _lib.lib().hriemo_mx8_scale_ld(n_rows)
    q = torch.empty((n_rows, d), dtype=torch.uint8, device="cuda")
    sc = torch.empty((d // 32, ld), dtype=torch.uint8, device="cuda")
    _lib.call("hriemo_quant_mx8", p16.data_ptr(), d, 0, n_rows, d, q.data_ptr(), d, sc.data_ptr(), ld, ST())
    return q.cpu(), sc[:, :n_rows].cpu()


def _pack_index(cu_dev, B, L, n_rows):
    """row_index of hriemo_pack_rows for the same plan"""
    from hri_emo_amd import _lib
    x = torch.zeros((B * L, 8), dtype=torch.bfloat16, device="cuda")
    p = torch.empty((n_rows, 8), dtype=torch.bfloat16, device="cuda")
    idx = torch.full((n_rows,), -1, dtype=torch.int64, device="cuda")
    _lib.call("hriemo_pack_rows", x.data_ptr(), None, cu_dev.data_ptr(), B, L, 8, n_rows, p.data_ptr(), None, idx.data_ptr(), ST())
    return idx.cpu()


class Case:
    """one launch configuration: the guarded source, the plan, and fresh guarded outputs per launch"""

    def __init__(self, lens, L, d, kind, layout, n_rows=None, seed=0):
        self.B, self.L, self.d, self.kind, self.layout = len(lens), L, d, kind, layout
        dtype, self.xt = DT[kind]
        total = sum(lens)
        if layout == "nocu":                                  # the padded layout kept: every row is a source row
            self.n_rows = self.B * L
            self.cu, self.rows = None, [(r // L, r % L) for r in range(self.n_rows)]
            src_rows, valid = self.n_rows, list(range(self.n_rows))
        else:
            self.n_rows = total if n_rows is None else n_rows
            self.cu, self.rows = _plan(lens, L, self.n_rows)
            if layout == "gather":
                src_rows, valid = self.B * L, [b * L + l for b, l in self.rows[:total]]
            else:                                             # packed source: cu[B] real rows, then rows nobody may read
                src_rows, valid = total + 3, list(range(total))
        self.vals = _values(len(valid), d, kind, seed)        # fp32, exact in the source format
        self.ldx = d + 8
        self.src = Guarded(src_rows, d, dtype, ld=self.ldx)
        self.src.t[torch.tensor(valid, device="cuda")] = self.vals.to(dtype).cuda()
        self.cu_dev = None if self.cu is None else torch.tensor(self.cu, dtype=torch.int32, device="cuda")
        self.real = [i for i, r in enumerate(self.rows) if r is not None]

    def launch(self, outs=("p16", "p32", "mx", "idx"), raw=False, **over):
        """fresh outputs, one launch -> dict of Guarded (None where not asked for); raw: return the status instead of raising"""
        from hri_emo_amd import _lib
        n, d = self.n_rows, self.d
        o = {k: None for k in ("p16", "p32", "pq", "ps", "idx")}
        if "p16" in outs:
            o["p16"] = Guarded(n, d, torch.bfloat16)
        if "p32" in outs:
            o["p32"] = Guarded(n, d, torch.float32)
        lds = 0
        if "mx" in outs:
            lds = _lib.lib().hriemo_mx8_scale_ld(n)
            o["pq"], o["ps"] = Guarded(n, d, torch.uint8), Guarded(d // 32, n, torch.uint8, ld=lds)
        if "idx" in outs and self.cu is not None:
            o["idx"] = Guarded(n, 1, torch.int64)
        ptr = lambda k: None if o[k] is None else o[k].ptr    # noqa: E731
        a = dict(X=self.src.ptr, xt=self.xt, ldx=self.ldx, cu=None if self.cu_dev is None else self.cu_dev.data_ptr(),
                 sp=int(self.layout == "packed"), B=self.B, L=self.L, d=d, n=n, p16=ptr("p16"), p32=ptr("p32"), pq=ptr("pq"),
                 ps=ptr("ps"), lds=lds, idx=ptr("idx"))
        a.update(over)
        args = (a["X"], a["xt"], a["ldx"], a["cu"], a["sp"], a["B"], a["L"], a["d"], a["n"], a["p16"], a["p32"], a["pq"], a["ps"],
                a["lds"], a["idx"], ST())
        if raw:
            return _lib.lib().hriemo_ingest_rows(*args), o
        _lib.call("hriemo_ingest_rows", *args)
        torch.cuda.synchronize()
        return o

    def check(self, o):
        """every output given in `o` against its reference, bit for bit; every guard byte; the source unchanged"""
        n, d = self.n_rows, self.d
        exp32 = torch.zeros(n, d)
        exp32[self.real] = self.vals
        exp16 = exp32.to(torch.bfloat16)                      # torch's CPU cast: round to nearest even
        if self.kind == "bf16":
            assert torch.equal(_bits(exp16.float()), _bits(exp32))
        for k in ("p16", "p32", "pq", "ps", "idx"):
            assert o[k] is None or o[k].intact(), f"{k}: a guard byte was written"
        assert self.src.intact()
        if o["p32"] is not None:
            assert torch.equal(o["p32"].bits(), _bits(exp32)), "fp32 twin != source values"
        if o["p16"] is not None:
            assert torch.equal(o["p16"].bits(), _bits(exp16)), "bf16 rows != torch's round-to-nearest-even cast"
        if o["pq"] is not None:
            q_par, s_par = _quant_parent(exp16.cuda(), n, d)
            q_emu, s_emu = mx8_emul.mx8_quantize(exp16)
            got_q, got_s = o["pq"].bits(), o["ps"].bits()
            assert torch.equal(got_q, q_par) and torch.equal(got_s, s_par), "MX-fp8 copy != hriemo_quant_mx8 of the bf16 rows"
            assert torch.equal(got_q, q_emu) and torch.equal(got_s, s_emu.t().contiguous()), "MX-fp8 copy != the host emulation"
            surplus = [i for i, r in enumerate(self.rows) if r is None]
            assert bool((got_q[surplus] == 0).all()) and bool((got_s[:, surplus] == 0).all())
        if o["idx"] is not None:
            ref = _pack_index(self.cu_dev, self.B, self.L, n)
            assert torch.equal(o["idx"].bits().reshape(-1), ref), "row_index != hriemo_pack_rows'"
            assert ref[self.real].tolist() == [b * self.L + l for b, l in (self.rows[i] for i in self.real)]

    def run(self, outs=("p16", "p32", "mx", "idx")):
        if self.d % 32 != 0:
            outs = tuple(k for k in outs if k != "mx")
        first = self.launch(outs)
        self.check(first)
        second = self.launch(outs)                            # a second launch is bit-identical, guard bytes and all
        for k, g in first.items():
            assert g is None or torch.equal(g.raw, second[k].raw), f"{k}: second launch differs"


LENS5 = [70, 33, 32, 1, 17]


@pytest.mark.parametrize("layout", ["gather", "packed", "nocu"])
@pytest.mark.parametrize("kind", list(DT))
@pytest.mark.parametrize("d", [8, 32, 40, 520, 768])
def test_ingest_rows_every_width_dtype_and_layout(d, kind, layout):
    """B = 5, L = 70, lengths [70, 33, 32, 1, 17], n_rows = sum + 11 (surplus rows, a row count that is no multiple of 4); d = 8
    (one chunk), 32 (one MX block), 40 (no fp8), 520 (a second 512-column pass with a one-chunk tail), 768 (24 MX blocks); all
    outputs of the launch at once"""
    Case(LENS5, 70, d, kind, layout, n_rows=sum(LENS5) + 11, seed=d).run()


@pytest.mark.parametrize("layout", ["gather", "packed", "nocu"])
@pytest.mark.parametrize("name,lens,L,n_rows", [
    ("one row", [1], 1, None),
    ("three", [17, 1, 9], 17, None),
    ("search over 68 entries", [1 + i % 3 for i in range(67)], 3, None),
    ("scale byte of row 256 in the second 256-column segment", [70, 70, 70, 50], 70, 260),
])
def test_ingest_rows_length_sets(name, lens, L, n_rows, layout):
    for kind, d in (("fp32", 32), ("fp16", 96)):
        c = Case(lens, L, d, kind, layout, n_rows=n_rows, seed=len(lens))
        if n_rows == 260 and layout != "nocu":
            from hri_emo_amd import _lib
            assert c.n_rows == 260 and _lib.lib().hriemo_mx8_scale_ld(260) == 512
        c.run()


@pytest.mark.parametrize("outs", [("p16", "p32", "idx"), ("p16", "idx"), ("p16", "p32", "mx", "idx"), ("p16", "mx", "idx"), ("mx",),
                                  ("p16", "p32"), ("p32",)])
def test_ingest_rows_output_subsets(outs):
    """the subsets the host wiring asks for (pair with and without twin, with and without the fp8 copy, the fp8 copy alone for a
    bf16 tensor that keeps its layout) and the twin alone: what is not asked for is not written, what is asked for is the same"""
    for kind, layout in (("fp16", "gather"), ("bf16", "nocu"), ("fp32", "packed")):
        Case([17, 1, 9], 17, 96, kind, layout, n_rows=None if layout == "nocu" else 30, seed=5).run(outs)


def test_ingest_rows_refusals():
    """one per documented check: non-zero status, hriemo_last_error set, nothing launched (the 0xFF-filled outputs unchanged);
    the same arguments unchanged are accepted"""
    from hri_emo_amd import _lib
    c = Case([17, 1, 9], 17, 96, "fp32", "gather", n_rows=30, seed=9)
    n = Case([17, 1, 9], 17, 96, "fp32", "nocu", seed=9)
    bad = [
        ("empty shape (B)", c, dict(B=0)), ("empty shape (L)", c, dict(L=0)), ("empty shape (d)", c, dict(d=0)),
        ("empty shape (n_rows)", c, dict(n=0)),
        ("d % 8", c, dict(d=100, pq=None, ps=None)),
        ("Pq without Ps", c, dict(ps=None)),
        ("Pq with d % 32 != 0", c, dict(d=40)),
        ("lds < n_rows", c, dict(lds=0)), ("lds % 256", c, dict(lds=300)),
        ("X alignment", c, dict(X=c.src.ptr + 4)),
        ("ldx < d", c, dict(ldx=88)), ("source row stride not a multiple of 16 bytes", c, dict(ldx=98)),
        ("unknown x_dtype", c, dict(xt=3)), ("negative x_dtype", c, dict(xt=-1)),
        ("row_index without cu", c, dict(cu=None, n=17 * 3, sp=0)),
        ("src_packed without cu", n, dict(sp=1)),
        ("n_rows != B * L without cu", n, dict(n=30)),
        ("no output", c, dict(p16=None, p32=None, pq=None, ps=None)),
    ]
    for what, case, over in bad:
        rc, o = case.launch(raw=True, **over)
        torch.cuda.synchronize()
        assert rc != 0, what
        msg = _lib.lib().hriemo_last_error().decode()
        assert "ingest_rows" in msg, (what, msg)
        for k, g in o.items():
            assert g is None or g.untouched(), (what, k)
    for k in ("p16", "p32", "pq"):                            # a misaligned output base
        rc, o = c.launch(raw=True)
        assert rc == 0
        rc, o = c.launch(raw=True, **{k: o[k].ptr + 8})
        torch.cuda.synchronize()
        assert rc != 0 and "unaligned" in _lib.lib().hriemo_last_error().decode(), k
        assert all(g is None or g.untouched() for g in o.values()), k
    for case in (c, n):                                       # the same arguments, unchanged, are accepted
        rc, o = case.launch(raw=True)
        torch.cuda.synchronize()
        assert rc == 0
        case.check(o)
