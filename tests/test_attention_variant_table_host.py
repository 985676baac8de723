"""Host check of the variant table of tests/test_gpu_attention_variants.py: the dispatch rules of attn_fwd_impl / attn_bwd_impl
(hri-emo_amd/csrc/attention.hip), replayed for a 256-CU device, send every row where the table says, and the rows together reach
every launch arm of the padded path with the bit-word mask, with the hash replay and without dropout, at every head dim the arm
is built for and under every mask pattern.  (On the GPU the test asserts each row's form through the ABI instead of this replica.)"""
import test_gpu_attention_variants as V

CUS = 256
HEAD_DIMS = (16, 32, 64, 96, 128)


def bwd_wide(L, BH, hd):
    if L <= 64 or hd > 96:
        return False
    sn, sw = 3 * CUS, 2 * CUS
    nn, nw = -(-L // 64) * BH, -(-L // 128) * BH
    return nn / (-(-nn // sn) * sn) < 0.75 and nw / (-(-nw // sw) * sw) >= 0.9


def bwd_fused(Lk, hd):
    return 16 < Lk <= 128 and hd >= 32


def bwd_qres(Lq, Lk, hd):
    return not bwd_fused(Lk, hd) and 16 < Lq <= 128 and hd >= 32


def backward_form(B, H, Lq, Lk, hd):
    if bwd_fused(Lk, hd):
        return "fused-KW1" if Lk <= 64 else "fused-KW2"
    if bwd_qres(Lq, Lk, hd):
        return "qres"
    side = lambda L: "w128" if bwd_wide(L, B * H, hd) else ("n64" if L > 16 else "1w")
    return f"two-kernel(dq={side(Lq)},dkv={side(Lk)})"


def resolved():
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd in V.VARIANTS:
        if B == V.W:
            B = next(b for b in range(1, 129) if backward_form(b, H, Lq, Lk, hd) == bwd)
        yield B, H, Lq, Lk, hd, pattern, p, fwd, bwd


def test_every_row_takes_the_form_the_table_names():
    for B, H, Lq, Lk, hd, pattern, p, fwd, bwd in resolved():
        assert backward_form(B, H, Lq, Lk, hd) == bwd, (B, H, Lq, Lk, hd)
        assert V.forward_form(Lq, Lk) == fwd, (Lq, Lk)
        assert hd in HEAD_DIMS and 0.0 <= p < 1.0
        assert V.R.key_padding_mask(pattern, B, Lk) is None or pattern != "none"      # B is large enough for the pattern


def test_the_wide_tile_batch_sizes_on_256_cus():
    first = lambda L: next(b for b in range(1, 129) if bwd_wide(L, b * 8, 96))
    assert first(400) == 15 and first(256) == 29 and first(200) == 29
    assert [b for b in range(1, 33) if bwd_wide(400, b * 8, 96)] == [15, 16, 29, 30]     # the headline batch over 4 GPUs: 16
    assert [b for b in range(1, 33) if bwd_wide(256, b * 8, 96)] == [29, 30, 31, 32]
    assert [b for b in range(1, 33) if bwd_wide(512, b * 8, 96)] == [15, 16] and bwd_wide(1000, 8 * 8, 96)
    assert not any(bwd_wide(400, b * 4, 128) for b in range(1, 129))                  # head_dim 128 is never wide


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
