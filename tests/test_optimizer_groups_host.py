"""CPU suite of DeviceAdamW's parameter groups (hri_emo_amd.optim): the segment table the grouped update kernel reads
(optim.group_segments, a pure host function), optim.decay_groups, every refusal of DeviceAdamW(buckets, param_groups=...) with its
message -- each BEFORE any parameter storage moves --, and the two new ABI entries in header, library and binding with the limits
their launchers enforce before they launch anything."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world():
    """the d = 128 model on CPU buckets: (model, buckets, parameters in flat-buffer order)"""
    import hri_emo_amd as H
    from hri_emo_amd.dp import GradBuckets
    torch.manual_seed(0)
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.0)
    buckets = GradBuckets(m.parameters(), overlap=False)
    order = sorted(buckets.params, key=lambda p: buckets._offsets[id(p)])
    return m, buckets, order


def _pad64(n):
    return (n + 63) // 64 * 64


def _check_table(buckets, seg, seg_group, G):
    assert len(seg) == len(seg_group) + 1 and seg[0] == 0 and seg[-1] == buckets.flat.numel()
    assert all(isinstance(x, int) for x in seg + seg_group)
    assert all(b > a for a, b in zip(seg, seg[1:])), "ascending, no empty segment"
    assert all(x % 64 == 0 for x in seg), "every boundary is a multiple of 64 elements"
    assert all(0 <= g < G for g in seg_group)
    assert all(a != b for a, b in zip(seg_group, seg_group[1:])), "neighbours of one group are merged"


def test_decay_split_is_one_boundary_in_the_flat_buffer(world):
    from hri_emo_amd.optim import decay_groups, group_segments
    m, buckets, order = world
    groups = decay_groups(m.named_parameters(), 1e-2)
    assert len(groups) == 2 and groups[0]["weight_decay"] == 1e-2 and groups[1]["weight_decay"] == 0.0
    assert all(p.dim() >= 2 for p in groups[0]["params"]) and all(p.dim() < 2 for p in groups[1]["params"])
    assert len(groups[0]["params"]) + len(groups[1]["params"]) == len(buckets.params)
    seg, seg_group = group_segments(buckets, groups)
    _check_table(buckets, seg, seg_group, 2)
    # GradBuckets lays every matrix in front of every vector: two segments, cut where the first vector starts
    first_vec = min(buckets._offsets[id(p)] for p in buckets.params if p.dim() < 2)
    assert seg == [0, first_vec, buckets.flat.numel()] and seg_group == [0, 1]
    # a predicate on names: LayerNorm and biases by name
    by_name = decay_groups(m.named_parameters(), 5e-2, no_decay=lambda name, p: name.endswith("bias") or "norm" in name)
    seg2, sg2 = group_segments(buckets, by_name)
    _check_table(buckets, seg2, sg2, 2)
    # a predicate nothing satisfies leaves the empty group out
    assert len(decay_groups(m.named_parameters(), 1e-2, no_decay=lambda name, p: False)) == 1


def test_interleaved_groups_give_one_segment_per_run(world):
    from hri_emo_amd.optim import group_segments
    m, buckets, order = world
    # every other parameter of the FLAT order: no two neighbours share a group, one segment per parameter
    groups = [{"params": order[0::2]}, {"params": order[1::2]}]
    seg, seg_group = group_segments(buckets, groups)
    _check_table(buckets, seg, seg_group, 2)
    assert len(seg_group) == len(order) and seg_group == [i % 2 for i in range(len(order))]
    assert seg[:-1] == [buckets._offsets[id(p)] for p in order]
    # every other parameter of the MODEL order, three groups: the runs counted here from the offsets
    params = list(buckets.params)
    groups3 = [{"params": params[k::3]} for k in range(3)]
    owner = {id(p): k for k in range(3) for p in params[k::3]}
    runs = [owner[id(order[0])]]
    starts = [0]
    for p in order[1:]:
        if owner[id(p)] != runs[-1]:
            runs.append(owner[id(p)])
            starts.append(buckets._offsets[id(p)])
    seg3, sg3 = group_segments(buckets, groups3)
    _check_table(buckets, seg3, sg3, 3)
    assert sg3 == runs and seg3 == starts + [buckets.flat.numel()]


def test_a_parameters_padding_belongs_to_its_segment(world):
    from hri_emo_amd.optim import group_segments
    m, buckets, order = world
    odd = [i for i, p in enumerate(order[:-1]) if p.numel() % 64 != 0]
    assert odd, "the d = 128 model has parameters whose size is no multiple of 64 (the 4-class head)"
    i = odd[0]
    p = order[i]
    groups = [{"params": [p]}, {"params": [q for q in order if q is not p]}]
    seg, seg_group = group_segments(buckets, groups)
    _check_table(buckets, seg, seg_group, 2)
    off = buckets._offsets[id(p)]
    k = seg.index(off)
    assert seg_group[k] == 0 and seg[k + 1] == off + _pad64(p.numel()) == buckets._offsets[id(order[i + 1])]


def test_refusals_name_the_parameter_and_move_nothing(world):
    from hri_emo_amd.optim import DeviceAdamW, MAX_GROUPS, group_segments
    m, buckets, order = world
    params = list(buckets.params)
    homes = [p.data_ptr() for p in m.parameters()]
    grads = [p.grad.data_ptr() for p in buckets.params]
    stranger = torch.nn.Parameter(torch.zeros(3, 5))
    cases = [
        ([{"params": params[:5]}, {"params": params[6:]}], r"buckets\.params\[5\] \(shape .*\) is missing"),
        ([{"params": params[:5]}, {"params": params[4:]}], r"buckets\.params\[4\] \(shape .*\) is repeated.*param_groups\[0\].*param_groups\[1\]"),
        ([{"params": params[:3] + [params[1]]}, {"params": params[3:]}], r"buckets\.params\[1\] .* is repeated"),
        ([{"params": params}, {"params": [stranger]}], r"param_groups\[1\]\['params'\]\[0\] \(shape \(3, 5\)\) is foreign"),
        ([{"params": [p]} for p in params[:MAX_GROUPS]] + [{"params": params[MAX_GROUPS:]}], r"17 param groups.*at most 16"),
        ([{"params": params[:5], "max_norm": 1.0}, {"params": params[5:]}], r"param_groups\[0\] names max_norm=1\.0.*clip is global"),
        ([{"params": params[:5]}, {"params": params[5:], "lr": -1.0}], r"lr, eps, weight_decay >= 0.*param_groups\[1\]"),
        ([{"params": params[:5]}, {"params": params[5:], "betas": (0.9, 1.0)}], r"betas in \[0, 1\).*param_groups\[1\]"),
        ([], r"non-empty list of dicts"),
        ([params], r"non-empty list of dicts"),
    ]
    for groups, msg in cases:
        with pytest.raises(ValueError, match=msg):
            DeviceAdamW(buckets, param_groups=groups, lr=1e-3, max_norm=5.0)
    for groups, msg in cases[:4]:                                # the partition check is group_segments' own
        with pytest.raises(ValueError, match=msg):
            group_segments(buckets, groups)
    # a group that repeats the global max_norm is no refusal; valid groups on host buckets end at the loud GPU check, as ever
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceAdamW(buckets, param_groups=[{"params": params[:5], "max_norm": 5.0}, {"params": params[5:]}], max_norm=5.0)
    assert homes == [p.data_ptr() for p in m.parameters()], "a refused construction must not have moved the parameters"
    assert grads == [p.grad.data_ptr() for p in buckets.params]


def test_groups_given_as_generators_are_read_once(monkeypatch):
    """torch's idiom {"params": model.backbone.parameters(), "lr": 3e-5}: a generator must not be spent by the validation and leave
    the optimizer with empty groups.  The GPU check is stubbed out so that the constructor runs through on host buckets (nothing is
    launched by a construction); group_segments alone takes generators too and leaves the caller's dicts as they were."""
    import hri_emo_amd as H
    from hri_emo_amd import optim
    from hri_emo_amd.dp import GradBuckets
    torch.manual_seed(0)
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.0)
    buckets = GradBuckets(m.parameters(), overlap=False)
    ps = list(buckets.params)
    want = optim.group_segments(buckets, [{"params": ps[:5]}, {"params": ps[5:]}])
    gen_groups = [{"params": (p for p in ps[:5])}, {"params": iter(ps[5:]), "lr": 3e-5}]
    kept = [g["params"] for g in gen_groups]
    assert optim.group_segments(buckets, gen_groups) == want
    assert [g["params"] for g in gen_groups] == kept and set(gen_groups[1]) == {"params", "lr"}, "the caller's dicts are not rewritten"
    # a missing parameter hidden in a generator is still named
    with pytest.raises(ValueError, match=r"buckets\.params\[5\] .* is missing"):
        optim.DeviceAdamW(buckets, param_groups=[{"params": (p for p in ps[:5])}, {"params": iter(ps[6:])}])
    monkeypatch.setattr(optim, "_require_gpu", lambda t: None)
    values = [p.detach().clone() for p in ps]
    opt = optim.DeviceAdamW(buckets, param_groups=[{"params": (p for p in ps[:5])}, {"params": iter(ps[5:]), "lr": 3e-5}], lr=1e-4)
    assert [len(g["params"]) for g in opt.param_groups] == [5, len(ps) - 5]
    assert all(a is b for a, b in zip([p for g in opt.param_groups for p in g["params"]], ps))
    assert opt.param_groups[1]["lr"] == 3e-5 and opt.param_groups[0]["lr"] == 1e-4
    assert (opt._seg.tolist(), opt._seg_group.tolist()) == want
    assert len(opt.state) == len(ps) and len(opt.state_dict()["state"]) == len(ps)
    for p, old in zip(ps, values):                              # every parameter was re-homed into the flat buffer, values kept
        off = buckets._offsets[id(p)]
        assert p.data_ptr() == opt.flat_p.data_ptr() + 4 * off and torch.equal(p.detach(), old)


def test_too_many_segments_is_refused_before_anything_moves():
    """2050 one-element vectors, alternating groups: 2050 segments, the kernel's table holds 2048"""
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW, MAX_SEGMENTS, group_segments
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in range(MAX_SEGMENTS + 2)]
    buckets = GradBuckets(ps, overlap=False)
    order = sorted(buckets.params, key=lambda p: buckets._offsets[id(p)])
    groups = [{"params": order[0::2]}, {"params": order[1::2]}]
    seg, seg_group = group_segments(buckets, groups)
    assert len(seg_group) == MAX_SEGMENTS + 2 and seg[1] == 64
    homes = [p.data_ptr() for p in ps]
    with pytest.raises(ValueError, match=r"2050 segments.*at most 2048"):
        DeviceAdamW(buckets, param_groups=groups)
    assert homes == [p.data_ptr() for p in ps]


def test_new_entries_in_header_library_and_binding():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hriemo.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)

    def args_of(name):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    assert args_of("hriemo_adamw_flat_groups") == [
        "float* p", "const float* g", "float* m", "float* v", "long n", "const long long* seg", "const int* seg_group", "int S",
        "const float* hyper", "const float* state", "int G", "hriemo_stream_t stream"]
    assert args_of("hriemo_optim_finalize_groups") == [
        "const float* partial", "int nblocks", "const float* hyper", "int G", "const float* grad_scale", "const float* found_inf",
        "float* state", "const int* ctl", "hriemo_stream_t stream"]
    assert _lib._SIGS["hriemo_adamw_flat_groups"] == ("pppplppippip", "i") and hasattr(L, "hriemo_adamw_flat_groups")
    assert _lib._SIGS["hriemo_optim_finalize_groups"] == ("pipippppp", "i") and hasattr(L, "hriemo_optim_finalize_groups")
    assert L.hriemo_abi_version() == 1


def test_launchers_refuse_their_limits_before_launching():
    """the checks run on the host in front of the launch: with no device in reach a refused call still returns its message.  The
    pointers are never dereferenced by a refused call (aligned dummy addresses)."""
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    a = 1 << 20                                                  # 16-byte aligned, non-null
    ok = dict(n=64, S=2, G=2)

    def update(n=64, S=2, G=2, p=a, seg=a, seg_group=a):
        _lib.call("hriemo_adamw_flat_groups", p, a, a, a, n, seg, seg_group, S, a, a, G, None)

    for kw, msg in ((dict(S=2049), r"S=2049 segments \(1 \.\. 2048\)"), (dict(S=0), r"S=0 segments"), (dict(G=17), r"G=17 groups \(1 \.\. 16\)"),
                    (dict(G=0), r"G=0 groups"), (dict(n=6), r"n=6 must be a positive multiple of 4"), (dict(n=0), "positive multiple of 4"),
                    (dict(p=a + 4), "unaligned buffer"), (dict(seg=None), "are required"), (dict(seg_group=None), "are required"),
                    (dict(seg=a + 4), "seg .* is not 8-byte aligned"), (dict(seg_group=a + 2), "seg_group .* is not 4-byte aligned")):
        with pytest.raises(RuntimeError, match="adamw_flat_groups.*" + msg):
            update(**{**ok, **kw})
    for G, msg in ((17, r"G=17 groups \(1 \.\. 16\)"), (0, "G=0 groups")):
        with pytest.raises(RuntimeError, match="optim_finalize_groups.*" + msg):
            _lib.call("hriemo_optim_finalize_groups", a, 1024, a, G, None, None, a, None, None)
    with pytest.raises(RuntimeError, match="optim_finalize_groups.*nblocks"):
        _lib.call("hriemo_optim_finalize_groups", a, 0, a, 2, None, None, a, None, None)
    with pytest.raises(RuntimeError, match="optim_finalize_groups.*ctl"):
        _lib.call("hriemo_optim_finalize_groups", a, 1024, a, 2, None, None, a, a + 2, None)
