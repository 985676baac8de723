"""Host proof of what tests/test_gpu_attention_variants_packed.py accepts (tests/attn_reference.py: make_packed / check_packed): on
packed (varlen) rows the bf16 yardstick of every sample passes check(), and the mistakes only the packed layout allows -- a bound
taken from the tile instead of the sample, a side buffer indexed the wrong way -- fail it when planted into the yardstick.  The table
of the GPU test is held to the launch plan and to its coverage here as well, for a 256-CU device.  No GPU; float64 on the CPU."""
import pytest
import torch

import attn_reference as R
import hashrng
import test_gpu_attention_variants_packed as V

SEED, SITE, BOFF = V.SEED, V.SITE, V.BOFF
CUS = 256
HEAD_DIMS = (16, 32, 64, 96, 128)
CASES = [  # B, H, max_lq, max_lk, hd, length pattern, p: rows of the GPU table (fewer heads), same lengths and generator seed
    (None, 2, 130, 130, 32, "edges", 0.1),
    (None, 1, 200, 128, 128, "edges", 0.0),
    (4, 2, 100, 65, 96, "bucket", 0.1),
    (4, 2, 130, 150, 64, "bucket", 0.0),
    (None, 1, 6, 200, 96, "edges", 0.1),
    (3, 2, 100, 65, 32, "ones", 0.1),
    (1, 2, 64, 200, 96, "single", 0.1),
]
MUTANTS = ("one_key_leaked_from_the_next_sample", "last_key_dropped", "query_rows_one_packed_row_late", "keep_mask_keyed_by_packed_row",
           "delta_from_the_compact_slot", "lse_from_the_compact_slot", "mask_words_with_the_stride_of_max_lk", "last_key_row_of_dK_dV_unwritten")


def _case(B, H, Lq, Lk, hd, pattern, p):
    lq, lk, filler = R.packed_lengths(pattern, Lq, Lk, B)
    return R.make_packed_decidable(lq, lk, filler, H, hd, V.data_seed(Lq, Lk), p, (SEED, SITE, BOFF))[0]


def _keep(c, b, lq, lk):
    return R.sample_keep(SEED, SITE, b, c.H, lq, lk, c.p, BOFF) if c.p > 0 else None


def _padded_slots(c, Lq, values):
    """the [B, H, max_lq] side buffer the kernels keep (zeros where nothing is written), flat, and for every sample the values a
    COMPACT reader finds: element (b, h, r) taken from H * cu_q[b] + h * lq[b] + r instead of (b * H + h) * max_lq + r"""
    flat = torch.zeros(c.B * c.H * Lq, dtype=torch.float64)
    for b in range(c.B):
        for h in range(c.H):
            at = (b * c.H + h) * Lq
            flat[at:at + c.lq[b]] = values[b][0, h]
    return [torch.stack([flat[c.H * c.cu_q[b] + h * c.lq[b]:][:c.lq[b]] for h in range(c.H)])[None] for b in range(c.B)]


def _strided_keep(keep, Lq, Lk):
    """the keep-mask a backward decodes when the forward wrote the words of a (b, h) compactly (word (q, kt) at q * nkt(lk) + kt of
    the slot) and it reads them with the stride of the launch maximum (q * nkt(max_lk) + kt); unwritten words read as zero"""
    _, H, lq, lk = keep.shape
    nkt_b, nkt = (lk + 63) // 64, (Lk + 63) // 64
    out = torch.zeros_like(keep)
    for h in range(H):
        slot = torch.zeros(Lq * nkt + nkt, 64, dtype=torch.bool)
        for kt in range(nkt_b):
            n = min(64, lk - 64 * kt)
            slot[torch.arange(lq) * nkt_b + kt, :n] = keep[0, h, :, 64 * kt:64 * kt + n]
        for kt in range(nkt_b):
            n = min(64, lk - 64 * kt)
            out[0, h, :, 64 * kt:64 * kt + n] = slot[torch.arange(lq) * nkt + kt, :n]
    return out


def mutant(name, c, b, Lq, Lk, side):
    """the outputs {O, dQ, dK, dV} of sample b under the planted mistake, or None where it changes nothing at this sample"""
    q, k, v, dO = c.sample(b)
    lq, lk, keep, inv = c.lq[b], c.lk[b], c.keep[b], c.inv_keep
    yard = c.yard[b]
    backward_only = lambda out: dict(out, O=yard["O"])            # noqa: E731  (the forward is right, the stored O is the yardstick's)
    if name == "one_key_leaked_from_the_next_sample":
        if b == c.B - 1:
            return None
        _, k1, v1, _ = c.sample(b, extra_k=1)
        out = R.yardstick(q, k1, v1, dO, None, _keep(c, b, lq, lk + 1), inv)
        return dict(out, dK=out["dK"][:, :, :lk], dV=out["dV"][:, :, :lk])
    if name == "last_key_dropped":
        if lk < 2:
            return None
        _, k1, v1, _ = c.sample(b, extra_k=-1)
        out = R.yardstick(q, k1, v1, dO, None, None if keep is None else keep[..., :lk - 1], inv)
        grow = lambda x: torch.cat([x, torch.zeros_like(x[:, :, :1])], 2)         # noqa: E731
        return dict(out, dK=grow(out["dK"]), dV=grow(out["dV"]))
    if name == "query_rows_one_packed_row_late":
        return R.yardstick(c.sample(b, dq=1)[0], k, v, dO, None, keep, inv)
    if name == "keep_mask_keyed_by_packed_row":
        if c.p == 0 or c.cu_q[b] == 0:
            return None
        return R.yardstick(q, k, v, dO, None, _keep(c, b, c.cu_q[b] + lq, lk)[:, :, c.cu_q[b]:], inv)
    if name == "delta_from_the_compact_slot":
        wrong = side["delta"][b]
        if torch.equal(wrong, side["delta_true"][b]):
            return None
        return backward_only(R.yardstick(q, k, v, dO, None, keep, inv, hooks={"delta": lambda x: wrong}))
    if name == "lse_from_the_compact_slot":
        wrong, true = side["lse"][b], c.ref[b]["lse"]
        if torch.equal(wrong, true):
            return None
        # the backward recomputes P = exp(S - lse) from the lse it reads
        return backward_only(R.yardstick(q, k, v, dO, None, keep, inv, hooks={"P": lambda x: x * torch.exp(true - wrong)[..., None],
                                                                             "delta": lambda x: side["delta_true"][b]}))
    if name == "mask_words_with_the_stride_of_max_lk":
        if c.p == 0:
            return None
        wrong = _strided_keep(keep, Lq, Lk)
        if torch.equal(wrong, keep):
            return None
        return backward_only(R.yardstick(q, k, v, dO, None, wrong, inv, hooks={"delta": lambda x: side["delta_true"][b]}))
    if name == "last_key_row_of_dK_dV_unwritten":
        out = {n: yard[n].clone() for n in R.OUTPUTS}
        out["dK"][:, :, -1], out["dV"][:, :, -1] = 0.0, 0.0          # what a zero-filled buffer holds where no store arrives
        return out if bool((yard["dK"][:, :, -1] != 0).any()) else None
    raise ValueError(name)


def _side_buffers(c, Lq):
    delta_true = [(c.yard[b]["O"] * c.sample(b)[3]).sum(-1) for b in range(c.B)]
    return {"delta_true": delta_true, "delta": _padded_slots(c, Lq, delta_true),
            "lse": _padded_slots(c, Lq, [c.ref[b]["lse"] for b in range(c.B)])}


def exercised(c, Lq, Lk):
    """the mutants that change something at this case, decided from the lengths alone"""
    B, nkt = c.B, (Lk + 63) // 64
    out = {"query_rows_one_packed_row_late", "last_key_row_of_dK_dV_unwritten"}
    if B > 1:
        out.add("one_key_leaked_from_the_next_sample")
    if max(c.lk) >= 2:
        out.add("last_key_dropped")
    if c.p > 0 and B > 1:
        out.add("keep_mask_keyed_by_packed_row")
    if any(c.cu_q[b] != b * Lq or (c.H > 1 and c.lq[b] < Lq) for b in range(B)):     # a compact slot that is not the padded slot
        out.update({"delta_from_the_compact_slot", "lse_from_the_compact_slot"})
    if c.p > 0 and any((c.lk[b] + 63) // 64 < nkt and c.lq[b] >= 2 for b in range(B)):
        out.add("mask_words_with_the_stride_of_max_lk")
    return out


@pytest.mark.parametrize("B,H,Lq,Lk,hd,pattern,p", CASES)
def test_packed_yardstick_passes_and_every_packed_mutant_fails(B, H, Lq, Lk, hd, pattern, p):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    c = _case(B, H, Lq, Lk, hd, pattern, p)
    for n, s in zip(R.OUTPUTS, "qqkk"):
        yard2d = torch.cat([R.rows(c.yard[b][n]) for b in range(c.B)])
        elem, tile = R.check_packed(yard2d, c, n, s)
        print(f"  yardstick {n}: elementwise {elem:.3f}, per tile {tile:.3f} of the limit")
        assert elem <= 0.5                                       # the kernels get the other half, as on padded rows
        assert R.packed_ratios(yard2d, c, n, s) == (elem, tile)
    if c.filler:                                                 # the all-zero filler: zero magnitude, so exact zeros are demanded
        assert all(bool((c.mag[-1][n] == 0).all()) and bool((c.ref[-1][n] == 0).all()) for n in R.OUTPUTS)
    side = _side_buffers(c, Lq)
    seen = set()
    for name in MUTANTS:
        worst = {n: (0.0, 0.0) for n in R.OUTPUTS}
        for b in range(c.B):
            mut = mutant(name, c, b, Lq, Lk, side)
            if mut is None:
                continue
            seen.add(name)
            for n in R.OUTPUTS:
                r = R.ratios(mut[n], c.ref[b][n], c.yard[b][n], c.mag[b][n])
                worst[n] = (max(worst[n][0], r[0]), max(worst[n][1], r[1]))
        if name not in seen:
            continue
        top = max(max(r) for r in worst.values())
        print(f"  mutant {name}: fails by {top:.3g} x its limit; " + ", ".join(f"{n} {e:.2f}/{t:.2f}" for n, (e, t) in worst.items()))
        assert top > 1.0, f"mutant {name} passes check() on every tensor of every sample: {worst}"
    assert seen == exercised(c, Lq, Lk), (seen, exercised(c, Lq, Lk))


def test_every_packed_mutant_is_exercised():
    seen = set()
    for B, H, Lq, Lk, hd, pattern, p in CASES:
        lq, lk, filler = R.packed_lengths(pattern, Lq, Lk, B)
        seen |= exercised(R.make_packed(lq, lk, filler, H, hd, 1, p, (SEED, SITE, BOFF), with_reference=False), Lq, Lk)
    assert seen == set(MUTANTS), set(MUTANTS) - seen
    # and by the GPU table: every case above is a row of it, up to the head count
    rows = {(B, Lq, Lk, hd, pattern, p) for B, _, Lq, Lk, hd, pattern, p, _, _ in V.VARIANTS}
    assert all((B, Lq, Lk, hd, pattern, p) in rows for B, _, Lq, Lk, hd, pattern, p in CASES)


def test_length_patterns():
    for Lq, Lk in ((400, 400), (130, 128), (33, 17), (6, 200), (16, 16), (1, 1), (18, 200)):
        lq, lk, filler = R.packed_lengths("edges", Lq, Lk)
        assert not filler and min(lq) >= 1 and min(lk) >= 1 and max(lq) == Lq and max(lk) == Lk
        assert set(lq) == {min(max(n, 1), Lq) for n in R.EDGE_LENGTHS + (Lq - 1, Lq)} and len(lq) >= len(set(lk))
        assert set(lk) == {min(max(n, 1), Lk) for n in R.EDGE_LENGTHS + (Lk - 1, Lk)}
        assert (lq[0], lk[0]) == (1, Lk)                         # the shortest queries meet the longest keys
        lq, lk, filler = R.packed_lengths("bucket", Lq, Lk)
        assert filler and len(lq) == len(lk) == 5 and min(lq) >= 1 and min(lk) >= 1
        for L, lens in ((Lq, lq), (Lk, lk)):
            assert max(lens) <= (L - 17 if L > 17 else max(1, L - 1)) or L == 1
            assert L == 1 or max(lens) < L                       # nobody reaches the launch maximum, the filler neither
        lq, lk, filler = R.packed_lengths("ones", Lq, Lk)
        assert (lq, lk, filler) == ([1, Lq, 1], [1, Lk, 1], False)
        assert R.packed_lengths("single", Lq, Lk) == ([Lq], [Lk], False)


def test_packed_inputs_and_keep_mask_are_those_of_the_padded_shape():
    """the packed keep-mask of sample b is the padded launch's mask cut to the sample: hashrng.attn_mask(...)[b, :, :lq[b], :lk[b]]"""
    B, H, Lq, Lk, p = None, 2, 70, 130, 0.1
    lq, lk, filler = R.packed_lengths("bucket", Lq, Lk, B)
    c = R.make_packed(lq, lk, filler, H, 16, 3, p, (SEED, SITE, BOFF), with_reference=False)
    full = torch.from_numpy(hashrng.attn_mask(SEED, SITE, c.B, H, Lq, Lk, p, BOFF))
    for b in range(c.B):
        assert torch.equal(c.keep[b][0], full[b, :, :lq[b], :lk[b]])
    assert c.cu_q[-1] == sum(lq) == c.qb.shape[0] == c.dob.shape[0] and c.cu_k[-1] == sum(lk) == c.kvb.shape[0]
    assert not c.qb[c.rows_q(c.B - 1)].any() and not c.kvb[c.rows_k(c.B - 1)].any() and not c.dob[c.rows_q(c.B - 1)].any()
    assert c.qb[:c.cu_q[-2]].any() and c.kvb[:c.cu_k[-2]].any()


def test_every_row_of_the_gpu_table_gets_inputs_that_check_can_judge():
    """The per-tile rule measures a kernel's error with the yardstick's own: 3 * ||yard - ref||.  On a tile of one query row over three
    keys that is one draw of a handful of roundings, and the OTHER float64 realisation of the same documented rounding points
    (attn_reference.yardstick_unnormalised: P rounded before its normalisation, as attn_fwd_kernel rounds it) can miss the limit
    -- here, with no kernel in sight.  Every row of the GPU table therefore takes the first data seed on which both realisations agree
    within the limits (make_packed_decidable); all but a few rows keep their first seed, and every row finds one."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    stepped = []
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd in V.VARIANTS:
        lq, lk, filler = V.resolve(L_(), B, H, Lq, Lk, hd, pattern, bwd, CUS)
        c, k = R.make_packed_decidable(lq, lk, filler, H, hd, V.data_seed(Lq, Lk), p, (SEED, SITE, BOFF))
        assert c.gap <= 1.0
        if k:
            first = R.make_packed(lq, lk, filler, H, hd, V.data_seed(Lq, Lk), p, (SEED, SITE, BOFF))
            stepped.append((Lq, Lk, hd, pattern, k))
            print(f"  max_lq={Lq} max_lk={Lk} hd={hd} {pattern}: data seed #{k}; on the first the two float64 realisations stand "
                  f"{R.realisation_gap(first):.2f} x the limit apart, on this one {c.gap:.2f}")
    assert len(stepped) <= len(V.VARIANTS) // 6, stepped            # the criterion sorts out a few inputs, it does not pick them all


# ---- the GPU test's variant table, held to the launch plan of a 256-CU device and to the coverage it promises

def L_():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib.lib()


def resolved():
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd in V.VARIANTS:
        lq, lk, filler = V.resolve(L_(), B, H, Lq, Lk, hd, pattern, bwd, CUS)
        assert H in (2, 4) or B == V.W                           # 8 heads only where the scan for the wide tile needs them
        yield len(lq), H, Lq, Lk, hd, pattern, p, fwd, bwd, lq, lk


def test_every_packed_row_takes_the_form_the_table_names():
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd, lq, lk in resolved():
        assert V.backward_form(L_(), B, H, Lq, Lk, hd, CUS) == bwd, (B, H, Lq, Lk, hd)
        assert V.forward_form(L_(), B, H, Lq, Lk, hd, CUS) == fwd, (Lq, Lk)
        assert hd in HEAD_DIMS and 0.0 <= p < 1.0
        assert 1 <= min(lq) and max(lq) <= Lq and 1 <= min(lk) and max(lk) <= Lk


def test_every_packed_arm_head_dim_and_length_pattern_is_reached():
    arms, dims, patterns, fwds = set(), {}, {}, set()
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd, lq, lk in resolved():
        fwds.add((fwd, p > 0))
        group = bwd if not bwd.startswith("two-kernel") else "two-kernel"
        parts = [bwd] if group != "two-kernel" else bwd[len("two-kernel("):-1].split(",")
        for part in parts + [group]:
            arms.add((part, "dropout" if p > 0 else "no dropout"))
            dims.setdefault(part, set()).add(hd)
            patterns.setdefault(part, set()).add(pattern)
        if group == "two-kernel":
            # blocks whose whole tile lies past their sample's end, on both sides of the two-kernel form
            rows = {"1w": 16, "n64": 64, "w128": 128}
            dq_rows, dkv_rows = (rows[part.split("=")[1]] for part in parts)
            if Lq > dq_rows:
                assert any(-(-n // dq_rows) < -(-Lq // dq_rows) for n in lq), (Lq, Lk, hd, "no empty dQ tile")
            if Lk > dkv_rows:
                assert any(-(-n // dkv_rows) < -(-Lk // dkv_rows) for n in lk), (Lq, Lk, hd, "no empty dK|dV tile")
    for fwd in ("fwd<4,2>", "fwd<4,1>", "fwd<1,1>"):
        assert (fwd, True) in fwds and (fwd, False) in fwds, fwd
    every = ("fused-KW1", "fused-KW2", "qres", "two-kernel", "dq=1w", "dq=n64", "dq=w128", "dkv=1w", "dkv=n64", "dkv=w128")
    for part in every:
        assert (part, "dropout") in arms and (part, "no dropout") in arms, part
        assert patterns[part] >= {"edges", "bucket"}, (part, patterns[part])
    for part, built in (("fused-KW1", HEAD_DIMS[1:]), ("fused-KW2", HEAD_DIMS[1:]), ("qres", HEAD_DIMS[1:]), ("two-kernel", HEAD_DIMS)):
        assert dims[part] >= set(built), (part, dims[part])
    assert all(16 not in dims[part] for part in ("fused-KW1", "fused-KW2", "qres"))
    used = [r[5] for r in V.VARIANTS]
    assert used.count("ones") == 1 and used.count("single") == 1
    # the query-resident form's second branch, and fwd<1,1> together with the 64-row dK | dV tile
    assert any(bwd == "qres" and Lk <= 16 for _, _, _, Lk, _, _, _, _, bwd in V.VARIANTS)
    assert any(fwd == "fwd<1,1>" and "dkv=n64" in bwd for *_, fwd, bwd in V.VARIANTS)
