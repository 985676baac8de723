"""CPU suite of DeviceAdamW's unit clip modes (hri_emo_amd.optim): the tables optim.clip_units builds for clip="group" and
clip="parameter" (pure host code), every refusal with its message -- each BEFORE any parameter storage moves --, the shape of the
state dict, and the new ABI entries in header, library and binding with the limits their launchers enforce before they launch."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 32768


def _pad64(n):
    return (n + 63) // 64 * 64


@pytest.fixture()
def small():
    """host buckets over parameters of 64, 40 (a vector, padded to 64), exactly one chunk, one chunk plus 64, and 64 elements:
    -> (buckets, the parameters in flat-buffer order)"""
    from hri_emo_amd.dp import GradBuckets
    ps = [torch.nn.Parameter(torch.zeros(8, 8)), torch.nn.Parameter(torch.zeros(40)), torch.nn.Parameter(torch.zeros(128, 256)),
          torch.nn.Parameter(torch.zeros(513, 64)), torch.nn.Parameter(torch.zeros(64))]
    buckets = GradBuckets(ps, overlap=False)
    order = sorted(buckets.params, key=lambda p: buckets._offsets[id(p)])
    return buckets, order


def _check(buckets, t, U):
    """what every table promises"""
    n = buckets.flat.numel()
    seg, S = t["seg"], len(t["seg_group"])
    assert len(seg) == S + 1 == len(t["seg_unit"]) + 1 and seg[0] == 0 and seg[-1] == n and all(b > a for a, b in zip(seg, seg[1:]))
    assert len(t["unit_group"]) == U and len(t["unit_chunks"]) == U + 1 and t["unit_chunks"][0] == 0 and t["unit_chunks"][-1] == len(t["chunks"])
    assert all(isinstance(x, int) for key in ("seg", "seg_group", "seg_unit", "unit_group", "unit_chunks") for x in t[key])
    hit = torch.zeros(n, dtype=torch.int32)
    for start, length, unit, group in t["chunks"]:
        assert start % 64 == 0 and length % 64 == 0 and 0 < length <= CHUNK and 0 <= start and start + length <= n
        assert group == t["unit_group"][unit]
        hit[start:start + length] += 1
    assert bool((hit == 1).all()), "every element is in exactly one chunk"
    keys = [(unit, start) for start, _, unit, _ in t["chunks"]]
    assert keys == sorted(keys), "chunks are ordered by unit, then by offset"
    for u in range(U):
        rows = t["chunks"][t["unit_chunks"][u]:t["unit_chunks"][u + 1]]
        assert rows and all(r[2] == u for r in rows)
    # a chunk never crosses a segment, and the segment's unit is the chunk's
    for start, length, unit, _ in t["chunks"]:
        s = max(i for i in range(S) if seg[i] <= start)
        assert start + length <= seg[s + 1] and t["seg_unit"][s] == unit


def test_parameter_mode_tables(small):
    from hri_emo_amd.optim import clip_units
    buckets, order = small
    groups = [{"params": [order[0], order[2], order[4]]}, {"params": [order[1], order[3]]}]
    t = clip_units(buckets, groups, "parameter")
    P = len(order)
    _check(buckets, t, P)
    assert t["seg"][:-1] == [buckets._offsets[id(p)] for p in order], "one segment per parameter slot, neighbours never merged"
    assert t["seg_unit"] == list(range(P)) and t["unit_group"] == t["seg_group"]
    owner = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    assert t["seg_group"] == [owner[id(p)] for p in order]
    per_unit = [t["unit_chunks"][u + 1] - t["unit_chunks"][u] for u in range(P)]
    sizes = {_pad64(p.numel()): k for p, k in zip(order, per_unit)}
    assert sizes[CHUNK] == 1, "a slot of exactly one chunk is one row"
    assert sizes[CHUNK + 64] == 2 and sizes[64] == 1
    u = [_pad64(p.numel()) for p in order].index(CHUNK + 64)
    assert [r[1] for r in t["chunks"] if r[2] == u] == [CHUNK, 64], "the slot of a chunk plus 64 elements ends in a 64-element row"
    # one group over everything (what the constructor builds without param_groups): the same segments, every unit in group 0
    t1 = clip_units(buckets, [{"params": list(buckets.params)}], "parameter")
    _check(buckets, t1, P)
    assert t1["seg"] == t["seg"] and t1["unit_group"] == [0] * P
    # neighbours of ONE group stay apart
    assert any(a == b for a, b in zip(t1["seg_group"], t1["seg_group"][1:]))


def test_group_mode_tables_with_non_adjacent_slots(small):
    from hri_emo_amd.optim import clip_units, group_segments
    buckets, order = small
    groups = [{"params": [order[0], order[2], order[4]]}, {"params": [order[1], order[3]]}]       # every other slot
    t = clip_units(buckets, groups, "group")
    _check(buckets, t, 2)
    assert (t["seg"], t["seg_group"]) == group_segments(buckets, groups) and t["seg_unit"] == t["seg_group"] and t["unit_group"] == [0, 1]
    assert len(t["seg_group"]) == len(order), "no two neighbours share a group here: one segment per slot"
    # the rows of unit 0 come first although its slots alternate with unit 1's in the buffer
    starts0 = [r[0] for r in t["chunks"] if r[2] == 0]
    starts1 = [r[0] for r in t["chunks"] if r[2] == 1]
    assert starts0 == sorted(starts0) and starts1 == sorted(starts1) and min(starts1) < max(starts0)
    # neighbours of one group merge, and the cut then runs over the merged segment
    merged = clip_units(buckets, [{"params": order[:3]}, {"params": order[3:]}], "group")
    _check(buckets, merged, 2)
    assert len(merged["seg_group"]) == 2
    with pytest.raises(ValueError, match="the unit modes are 'group' and 'parameter'"):
        clip_units(buckets, groups, "global")


def test_64_element_slots():
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import clip_units
    ps = [torch.nn.Parameter(torch.zeros(k)) for k in (64, 1, 64, 63)]
    buckets = GradBuckets(ps, overlap=False)
    t = clip_units(buckets, [{"params": ps}], "parameter")
    _check(buckets, t, 4)
    assert t["seg"] == [0, 64, 128, 192, 256] and [r[:3] for r in t["chunks"]] == [(0, 64, 0), (64, 64, 1), (128, 64, 2), (192, 64, 3)]
    assert t["unit_chunks"] == [0, 1, 2, 3, 4]


def test_refusals_by_name_move_nothing(small):
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW, MAX_GROUPS, MAX_SEGMENTS, clip_units
    buckets, order = small
    params = list(buckets.params)
    homes = [p.data_ptr() for p in params]
    stranger = torch.nn.Parameter(torch.zeros(3, 5))
    with pytest.raises(ValueError, match=r"clip='units'; the modes are 'global', 'group' and 'parameter'"):
        DeviceAdamW(buckets, clip="units")
    # the global mode refuses a group's own max_norm by name (it used to be a silent no-op only where it equalled the optimizer's)
    with pytest.raises(ValueError, match=r"param_groups\[1\] names max_norm=0\.5, the optimizer 5\.0.*clip is global.*clip='group'"):
        DeviceAdamW(buckets, param_groups=[{"params": params[:2]}, {"params": params[2:], "max_norm": 0.5}], max_norm=5.0)
    for mode in ("group", "parameter"):
        cases = [
            ([{"params": params[:2]}, {"params": params[3:]}], r"buckets\.params\[2\] \(shape .*\) is missing"),
            ([{"params": params[:3]}, {"params": params[2:]}], r"buckets\.params\[2\] .* is repeated"),
            ([{"params": params}, {"params": [stranger]}], r"is foreign"),
            ([{"params": params}, {"params": []}], r"param_groups\[1\] holds no parameter.*clip unit of nothing"),
            ([{"params": params[:2], "max_norm": "5"}, {"params": params[2:]}], r"param_groups\[0\] names max_norm='5'; a number"),
            ([{"params": params[:2]}, {"params": params[2:], "lr": -1.0}], r"lr, eps, weight_decay >= 0.*param_groups\[1\]"),
        ]
        for groups, msg in cases:
            with pytest.raises(ValueError, match=msg):
                DeviceAdamW(buckets, param_groups=groups, clip=mode)
        for groups, msg in cases[:4]:
            with pytest.raises(ValueError, match=msg):
                clip_units(buckets, groups, mode)
        # valid groups with their own max_norm on host buckets end at the loud GPU check, as ever
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DeviceAdamW(buckets, param_groups=[{"params": params[:2], "max_norm": 0.5}, {"params": params[2:], "max_norm": 0.0}], clip=mode)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DeviceAdamW(buckets, clip=mode)
    assert homes == [p.data_ptr() for p in params], "a refused construction must not have moved the parameters"
    # the limits: 2049 parameters are 2049 units in parameter mode and fine as one group; 17 groups are refused as ever
    many = [torch.nn.Parameter(torch.zeros(1)) for _ in range(MAX_SEGMENTS + 1)]
    big = GradBuckets(many, overlap=False)
    with pytest.raises(ValueError, match=r"clip='parameter' makes 2049 clip units.*at most 2048"):
        DeviceAdamW(big, clip="parameter")
    with pytest.raises(ValueError, match=r"2049 clip units"):
        clip_units(big, [{"params": many}], "parameter")
    assert len(clip_units(big, [{"params": many}], "group")["chunks"]) == 5, "one unit of 2049 * 64 elements: four full chunks and 64"


def test_limits_of_groups_and_segments():
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import MAX_GROUPS, MAX_SEGMENTS, clip_units
    many = [torch.nn.Parameter(torch.zeros(1)) for _ in range(MAX_SEGMENTS + 2)]
    big = GradBuckets(many, overlap=False)
    order = sorted(big.params, key=lambda p: big._offsets[id(p)])
    with pytest.raises(ValueError, match=r"2050 segments.*at most 2048"):
        clip_units(big, [{"params": order[0::2]}, {"params": order[1::2]}], "group")
    with pytest.raises(ValueError, match=r"17 param groups.*at most 16"):
        clip_units(big, [{"params": [p]} for p in order[:MAX_GROUPS]] + [{"params": order[MAX_GROUPS:]}], "group")


def test_state_dict_shape_and_mode_check(small, monkeypatch):
    """the GPU check is stubbed out so that the constructor runs through on host buckets (a construction launches nothing)"""
    from hri_emo_amd import optim
    buckets, order = small
    params = list(buckets.params)
    monkeypatch.setattr(optim, "_require_gpu", lambda t: None)
    groups = [{"params": params[:2], "max_norm": 0.05}, {"params": params[2:]}]
    opt = optim.DeviceAdamW(buckets, param_groups=groups, max_norm=5.0, clip="group")
    assert [g["max_norm"] for g in opt.param_groups] == [0.05, 5.0], "a missing key takes the constructor's value"
    assert opt._clip_state.shape == (4,) and opt._partial.numel() == len(optim.clip_units(buckets, groups, "group")["chunks"])
    sd = opt.state_dict()
    assert sd["clip"] == {"mode": "group"} and [g["max_norm"] for g in sd["param_groups"]] == [0.05, 5.0]
    assert set(sd) == {"state", "param_groups", "clip"}
    opt.load_state_dict(sd)
    plain = {k: v for k, v in sd.items() if k != "clip"}                     # what a torch.optim.AdamW (or the global mode) writes
    opt.load_state_dict(plain)
    for other in ("parameter", "global"):
        with pytest.raises(ValueError, match=rf"written with clip='{other}', this optimizer was built with clip='group'"):
            opt.load_state_dict({**sd, "clip": {"mode": other}})
    with pytest.raises(ValueError, match=r"name_parameters: parameter 0 of the optimizer \(shape .*\) has no name"):
        opt.name_parameters([])


def test_global_mode_keeps_its_state_dict_and_refuses_unit_dicts(monkeypatch):
    from hri_emo_amd import optim
    from hri_emo_amd.dp import GradBuckets
    ps = [torch.nn.Parameter(torch.zeros(8, 8)), torch.nn.Parameter(torch.zeros(40))]
    buckets = GradBuckets(ps, overlap=False)
    monkeypatch.setattr(optim, "_require_gpu", lambda t: None)
    opt = optim.DeviceAdamW(buckets, param_groups=[{"params": ps}], max_norm=5.0)
    assert opt.clip == "global" and not hasattr(opt, "_clip_state") and opt._partial.numel() == 1024
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}, "the default mode adds no key"
    with pytest.raises(ValueError, match=r"written with clip='parameter', this optimizer was built with clip='global'"):
        opt.load_state_dict({**sd, "clip": {"mode": "parameter"}})
    with pytest.raises(RuntimeError, match=r"clip_arrays\(\): built with clip='global'"):
        opt.clip_arrays()


def test_new_entries_in_header_library_and_binding():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hriemo.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)

    def args_of(name):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    assert args_of("hriemo_sumsq_units") == ["const float* g", "long n", "const long long* chunks", "int C", "float* partial", "hriemo_stream_t stream"]
    assert args_of("hriemo_optim_finalize_units") == [
        "const float* partial", "int C", "const int* unit_chunks", "const int* unit_group", "int U", "const float* hyper", "int G",
        "const float* grad_scale", "const float* found_inf", "float* state", "const int* ctl", "float* clip_state",
        "const float* avg_hyper", "float* avg_state", "hriemo_stream_t stream"]
    upd = ["float* p", "const float* g", "float* m", "float* v", "long n", "const long long* seg", "const int* seg_group",
           "const int* seg_unit", "int S", "const float* hyper", "const float* state", "int G", "const float* clip_state", "int U"]
    assert args_of("hriemo_adamw_flat_units") == upd + ["hriemo_stream_t stream"]
    assert args_of("hriemo_adamw_flat_units_avg") == upd + ["float* avg", "const float* avg_state", "hriemo_stream_t stream"]
    code = {"float*": "p", "const float*": "p", "const int*": "p", "const long long*": "p", "hriemo_stream_t": "p", "int": "i", "long": "l"}
    for name in ("hriemo_sumsq_units", "hriemo_optim_finalize_units", "hriemo_adamw_flat_units", "hriemo_adamw_flat_units_avg"):
        want = "".join(code[a.rsplit(" ", 1)[0]] for a in args_of(name))
        assert _lib._SIGS[name] == (want, "i") and hasattr(L, name), name
    assert L.hriemo_abi_version() == 1


def test_launchers_refuse_their_limits_before_launching():
    """the checks run on the host in front of the launch: with no device in reach a refused call still returns its message.  The
    pointers are never dereferenced by a refused call (aligned dummy addresses far apart)."""
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    a = [(k + 1) << 24 for k in range(12)]                        # 16-byte aligned, non-null, no two spans overlap

    def update(n=4096, S=2, G=2, U=2, p=a[0], seg=a[4], seg_unit=a[6], clip=a[9], name="hriemo_adamw_flat_units", tail=()):
        _lib.call(name, p, a[1], a[2], a[3], n, seg, a[5], seg_unit, S, a[7], a[8], G, clip, U, *tail, None)

    for kw, msg in ((dict(U=2049, S=2048), r"U=2049 units \(1 \.\. 2048\)"), (dict(U=0), r"U=0 units"), (dict(U=3), r"U=3 units over S=2 segments"),
                    (dict(S=2049), r"S=2049 segments \(1 \.\. 2048\)"), (dict(G=17), r"G=17 groups \(1 \.\. 16\)"),
                    (dict(n=6), r"n=6 must be a positive multiple of 4"), (dict(n=4), r"S=2 segments over n=4 elements"),
                    (dict(p=a[0] + 4), "unaligned buffer"), (dict(seg=a[4] + 4), "seg .* is not 8-byte aligned"),
                    (dict(seg_unit=a[6] + 2), "seg_group / seg_unit .* is not 4-byte aligned"), (dict(seg_unit=None), "seg .* are required"),
                    (dict(clip=None), "clip_state .* is required")):
        with pytest.raises(RuntimeError, match="adamw_flat_units: .*" + msg):
            update(**kw)
    with pytest.raises(RuntimeError, match="adamw_flat_units_avg: avg is required"):
        update(name="hriemo_adamw_flat_units_avg", tail=(None, a[11]))
    with pytest.raises(RuntimeError, match="adamw_flat_units_avg: avg overlaps p, g, m or v"):
        update(name="hriemo_adamw_flat_units_avg", tail=(a[0] + 16, a[11]))

    def finalize(C=8, U=2, G=2, ctl=None, clip=a[5], avg_hyper=None, avg_state=None, unit_chunks=a[1]):
        _lib.call("hriemo_optim_finalize_units", a[0], C, unit_chunks, a[2], U, a[3], G, None, None, a[4], ctl, clip, avg_hyper, avg_state, None)

    for kw, msg in ((dict(U=2049, C=4096), r"U=2049 units \(1 \.\. 2048\)"), (dict(U=9), r"U=9 units over C=8 chunks"), (dict(C=0), r"C=0 chunks"),
                    (dict(C=(1 << 20) + 1), r"C=1048577 chunks \(1 \.\. 1048576\)"), (dict(G=17), r"G=17 groups"), (dict(ctl=a[6] + 2), "ctl is the int32"),
                    (dict(clip=None), "clip_state .* is required"), (dict(clip=a[4] + 8), "clip_state overlaps"),
                    (dict(avg_hyper=a[7]), "come together or not at all"), (dict(unit_chunks=a[1] + 2), "4-byte aligned")):
        with pytest.raises(RuntimeError, match="optim_finalize_units: .*" + msg):
            finalize(**kw)

    def sumsq(n=4096, C=8, g=a[0], chunks=a[1], partial=a[2]):
        _lib.call("hriemo_sumsq_units", g, n, chunks, C, partial, None)

    for kw, msg in ((dict(n=6), "positive multiple of 4"), (dict(g=a[0] + 4), "16-byte aligned"), (dict(C=0), r"C=0 chunks"),
                    (dict(C=1025), r"C=1025 chunks over n=4096 elements"), (dict(chunks=a[1] + 4), "8-byte aligned"),
                    (dict(chunks=None), "chunks .* is required"), (dict(partial=None), "partial .* is required"),
                    (dict(partial=a[0] + 64), "partial overlaps g or chunks")):
        with pytest.raises(RuntimeError, match="sumsq_units: .*" + msg):
            sumsq(**kw)
