"""Host check of the variant table of tests/test_gpu_attention_variants.py and of the launch plan behind it: hriemo_attn_plan
(hri-emo_amd/csrc/attention.hip; host code, the plan attn_fwd_impl / attn_bwd_impl launch), asked for a 256-CU device, sends every
row where the table says, and the rows together reach every launch arm of the padded path with the bit-word mask, with the hash
replay and without dropout, at every head dim the arm is built for and under every mask pattern.  A sweep then holds the plan's
fields to their contract with each other and the older size queries to the plan."""
import itertools

import test_gpu_attention_variants as V

CUS = 256
HEAD_DIMS = (16, 32, 64, 96, 128)


def L_():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    return _lib.lib()


def backward_form(B, H, Lq, Lk, hd):
    return V.backward_form(L_(), B, H, Lq, Lk, hd, CUS)


def bwd_wide(L, B, H, hd):
    """the 128-row backward tile on a side of length L (L_q = L_k = L > 128: the two-kernel form)"""
    return V.plan(L_(), B, H, L, L, hd, CUS)[2:4] == (128, 128)


def resolved():
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd in V.VARIANTS:
        if B == V.W:
            B = next(b for b in range(1, 129) if backward_form(b, H, Lq, Lk, hd) == bwd)
        yield B, H, Lq, Lk, hd, pattern, p, fwd, bwd


def test_every_row_takes_the_form_the_table_names():
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd in resolved():
        assert backward_form(B, H, Lq, Lk, hd) == bwd, (B, H, Lq, Lk, hd)
        assert V.forward_form(L_(), B, H, Lq, Lk, hd, CUS) == fwd, (Lq, Lk)
        assert hd in HEAD_DIMS and 0.0 <= p < 1.0
        assert V.R.key_padding_mask(pattern, B, Lk) is None or pattern != "none"      # B is large enough for the pattern


def test_the_wide_tile_batch_sizes_on_256_cus():
    first = lambda L: next(b for b in range(1, 129) if bwd_wide(L, b, 8, 96))
    assert first(400) == 15 and first(256) == 29 and first(200) == 29
    assert [b for b in range(1, 33) if bwd_wide(400, b, 8, 96)] == [15, 16, 29, 30]     # the headline batch over 4 GPUs: 16
    assert [b for b in range(1, 33) if bwd_wide(256, b, 8, 96)] == [29, 30, 31, 32]
    assert [b for b in range(1, 33) if bwd_wide(512, b, 8, 96)] == [15, 16] and bwd_wide(1000, 8, 8, 96)
    assert not any(bwd_wide(400, b, 4, 128) for b in range(1, 129))                  # head_dim 128 is never wide


def test_every_launch_arm_head_dim_and_mask_pattern_is_reached():
    arms, dims, patterns = set(), {}, {}
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd in resolved():
        arms.add((fwd, "bit words written" if p > 0 else "no bit words"))
        parts = [bwd] if not bwd.startswith("two-kernel") else bwd[len("two-kernel("):-1].split(",")
        for part in parts:
            # p > 0: the test runs the backward with the bit words AND with mask_bits = NULL (hash replay); p = 0: thr16 == 0
            arms.update({(part, "bit words"), (part, "hash replay")} if p > 0 else {(part, "no dropout")})
            dims.setdefault(part, set()).add(hd)
        group = bwd if not bwd.startswith("two-kernel") else "two-kernel"
        patterns.setdefault(group, set()).add(pattern)
    for fwd in ("fwd<4,2>", "fwd<4,1>", "fwd<1,1>"):
        assert (fwd, "bit words written") in arms and (fwd, "no bit words") in arms, fwd
    for part in ("fused-KW1", "fused-KW2", "qres", "dq=1w", "dq=n64", "dq=w128", "dkv=1w", "dkv=n64", "dkv=w128"):
        assert (part, "bit words") in arms and (part, "hash replay") in arms, part
    assert all((g, "no dropout") in arms for g in ("qres", "dq=1w", "dq=n64", "dq=w128", "dkv=1w", "dkv=n64", "dkv=w128"))
    for part, built in (("fused-KW1", HEAD_DIMS[1:]), ("fused-KW2", HEAD_DIMS[1:]), ("qres", HEAD_DIMS[1:]), ("dq=n64", HEAD_DIMS),
                        ("dkv=n64", HEAD_DIMS), ("dq=w128", HEAD_DIMS[:4]), ("dkv=w128", HEAD_DIMS[:4]), ("dq=1w", HEAD_DIMS),
                        ("dkv=1w", HEAD_DIMS)):
        assert dims[part] >= set(built), (part, dims[part])
    for group in ("fused-KW1", "fused-KW2", "qres", "two-kernel"):
        assert patterns[group] >= {"none", "edges", "leading", "allpad"}, (group, patterns[group])


def test_plan_fields_keep_their_contract_and_the_older_queries_read_the_plan():
    lib = L_()
    lengths = (1, 16, 17, 64, 65, 128, 129, 200, 256, 400, 1000)
    ceil = lambda a, b: -(-a // b)
    for B, H, Lq, Lk, hd in itertools.product(range(1, 41), (1, 2, 4, 8), lengths, lengths, HEAD_DIMS):
        for cus in (256, 304):
            fwd_rows, form, dq_rows, dkv_rows, rq, rk = V.plan(lib, B, H, Lq, Lk, hd, cus)
            assert fwd_rows in (128, 64, 16) and form in (0, 1, 2), (B, H, Lq, Lk, hd, cus)
            if form == 0:       # the kernels index the partials as b * tiles + tile
                assert dq_rows in (128, 64, 16) and dkv_rows in (128, 64, 16)
                assert (rq, rk) == (B * ceil(Lq, dq_rows), B * ceil(Lk, dkv_rows)), (B, H, Lq, Lk, hd, cus)
            else:               # one block per (batch, head): one row per batch on both sides
                assert (rq, rk) == (B, B) and hd != 16 and dq_rows == 0, (B, H, Lq, Lk, hd, cus)
                assert dkv_rows == (0 if form == 2 else 64 if Lk <= 64 else 128) and (form == 2 or Lk <= dkv_rows)
            assert hd != 128 or form != 0 or 128 not in (dq_rows, dkv_rows), (B, H, Lq, Lk, cus)
        _, form, _, _, rq, rk = V.plan(lib, B, H, Lq, Lk, hd, 0)            # this device, as the older queries ask
        assert lib.hriemo_attn_bwd_single_pass_q(B, H, Lq, Lk, hd) == (form != 0)
        assert lib.hriemo_attn_bwd_dq_colsum_rows(B, H, Lq, Lk, hd) == rq and lib.hriemo_attn_bwd_kv_colsum_rows(B, H, Lq, Lk, hd) == rk
        # the two queries without L_q: the key-resident form and the dK | dV rows do not depend on it, except that a one-row
        # query side keeps the query-resident form out
        rk1 = rk if form != 2 else V.plan(lib, B, H, 1, Lk, hd, 0)[5]
        assert lib.hriemo_attn_bwd_single_pass(B, H, Lk, hd) == (form == 1) and lib.hriemo_attn_bwd_colsum_rows(B, H, Lk, hd) == rk1
    for hd in (0, 8, 48, 100, 256):
        assert V.plan(lib, 2, 2, 64, 64, hd, CUS) is None and b"head_dim" in lib.hriemo_last_error()
    assert V.plan(lib, 0, 2, 64, 64, 64, CUS) is None and V.plan(lib, 2, 2, 64, 0, 64, CUS) is None
