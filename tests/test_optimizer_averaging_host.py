"""CPU suite of DeviceAdamW's weight averaging (hri_emo_amd.optim): every refusal of the averaging arguments BEFORE anything is
allocated or re-homed, the averaging-step predicate and the weight sequence against torch.optim.swa_utils.AveragedModel's own
bookkeeping, the four new ABI entries in header, library and binding with what their launchers refuse before they launch, and the
host side of the checkpoint format (the "averaging" key, the restart on a dict without it, refusals) on host buckets."""
import copy
import ctypes
import os
import re

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from avg_reference import walk, weight32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _world():
    import hri_emo_amd as H
    from hri_emo_amd.dp import GradBuckets
    torch.manual_seed(0)
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4, n_heads=8, dropout=0.0)
    return m, GradBuckets(m.parameters(), overlap=False)


def test_averaging_arguments_are_refused_before_anything_moves():
    from hri_emo_amd.optim import DeviceAdamW
    m, buckets = _world()
    homes = [p.data_ptr() for p in m.parameters()]
    cases = [
        (dict(averaging="polyak"), r"averaging='polyak'.*None, 'ema' and 'swa'"),
        (dict(averaging=True), r"averaging=True"),
        (dict(averaging="ema", avg_decay=1.0), r"avg_decay=1\.0 must lie in \[0, 1\)"),
        (dict(averaging="ema", avg_decay=-0.1), r"avg_decay=-0\.1"),
        (dict(averaging="swa", avg_start=-1), r"avg_start=-1 must be an integer >= 0"),
        (dict(averaging="swa", avg_start=1.5), r"avg_start=1\.5 must be an integer"),
        (dict(averaging="swa", avg_every=0), r"avg_every=0 must be an integer >= 1"),
        (dict(averaging="ema", avg_every=2 ** 24), r"avg_every=16777216"),
        (dict(avg_decay=0.99), r"without averaging="),
        (dict(avg_start=3), r"without averaging="),
        (dict(avg_every=2), r"without averaging="),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            DeviceAdamW(buckets, lr=1e-3, **kw)
        with pytest.raises(ValueError, match=msg):          # the same refusals in front of the groups' own
            DeviceAdamW(buckets, lr=1e-3, param_groups=[{"params": list(buckets.params)}], **kw)
    # valid averaging arguments on host buckets end at the loud GPU check, as every construction does
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceAdamW(buckets, averaging="ema", avg_decay=0.99, avg_start=2, avg_every=2)
    assert homes == [p.data_ptr() for p in m.parameters()], "a refused construction must not have moved the parameters"


@pytest.mark.parametrize("mode", ["ema", "swa"])
@pytest.mark.parametrize("start,every", [(0, 1), (1, 2), (2, 2), (3, 5), (20, 1)])
def test_predicate_and_weights_against_averaged_model(mode, start, every):
    """12 real updates of a tiny module, two skipped steps and a held micro-step between them: torch's loop calls
    update_parameters on exactly the updates is_averaging_step names; the device's bookkeeping (avg_reference.walk, the rule of
    csrc/optim.hip) must give AveragedModel's n_averaged after every event, and its fp32 weights must reproduce AveragedModel's
    parameters (2 roundings per update on either side: 1e-6 on values of order 1)"""
    from hri_emo_amd.optim import averaging_weight, is_averaging_step
    decay = 0.9
    torch.manual_seed(1)
    net = torch.nn.Linear(3, 2)
    am = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay)) if mode == "ema" else AveragedModel(net)
    events = ["update", "update", "skip", "update", "hold", "update", "update", "skip"] + ["update"] * 7
    records = walk(mode, decay, start, every, events)
    mine, t, n_seen = None, 0, 0
    for ev, (t_dev, kind, n_dev, w) in zip(events, records):
        if ev == "update":
            t += 1
            with torch.no_grad():
                for p in net.parameters():
                    p.add_(torch.randn_like(p) * 0.1)
            cur = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
            if is_averaging_step(t, start, every):
                am.update_parameters(net)
                assert kind == ("first" if n_seen == 0 else "update")
                assert abs(float(w) - averaging_weight(mode, n_seen, decay)) <= 2.0 ** -24, "the fp32 weight is the float64 one, rounded"
                assert torch.equal(w, weight32(mode, n_seen, decay))
                mine = cur.clone() if n_seen == 0 else mine + w * (cur - mine)
                n_seen += 1
            else:
                assert kind == "none" and w is None
        else:
            assert kind == "untouched" and w is None
        assert t_dev == t and n_dev == n_seen == int(am.n_averaged), (ev, t, n_dev, n_seen, int(am.n_averaged))
        if mine is not None:
            ref = torch.cat([p.detach().reshape(-1) for p in am.module.parameters()])
            assert float((mine - ref).abs().max()) <= 1e-6
    assert n_seen == sum(1 for t in range(1, 13) if t > start and (t - start) % every == 0)


def test_new_entries_in_header_library_and_binding():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hriemo.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)

    def args_of(name):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    update = ["float* p", "const float* g", "float* m", "float* v", "long n"]
    assert args_of("hriemo_optim_finalize_avg") == [
        "const float* partial", "int nblocks", "const float* hyper", "int G", "const float* grad_scale", "const float* found_inf",
        "float* state", "const int* ctl", "const float* avg_hyper", "float* avg_state", "hriemo_stream_t stream"]
    assert args_of("hriemo_adamw_flat_dev_avg") == update + [
        "const float* hyper", "const float* state", "float* avg", "const float* avg_state", "hriemo_stream_t stream"]
    assert args_of("hriemo_adamw_flat_groups_avg") == update + [
        "const long long* seg", "const int* seg_group", "int S", "const float* hyper", "const float* state", "int G", "float* avg",
        "const float* avg_state", "hriemo_stream_t stream"]
    assert args_of("hriemo_swap_fp32") == ["float* a", "float* b", "long n", "hriemo_stream_t stream"]
    for name, sig in (("hriemo_optim_finalize_avg", "pipippppppp"), ("hriemo_adamw_flat_dev_avg", "pppplppppp"),
                      ("hriemo_adamw_flat_groups_avg", "pppplppippippp"), ("hriemo_swap_fp32", "pplp")):
        assert _lib._SIGS[name] == (sig, "i") and hasattr(L, name), name
    assert L.hriemo_abi_version() == 1


def test_launchers_refuse_before_launching():
    """the checks run on the host in front of the launch (aligned dummy addresses that a refused call never dereferences)"""
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    a, far = 1 << 20, 1 << 24                                    # 16-byte aligned, non-null, 16 MiB apart

    for n, x, y, msg in ((6, a, far, "n=6 must be a positive multiple of 4"), (0, a, far, "positive multiple of 4"),
                         (64, a, a, "overlap"), (64, a, a + 16, "overlap"), (64, a + 255, a, "aligned"), (64, a + 240, a, "overlap"),
                         (64, a, a - 240, "overlap"), (64, None, far, "required"), (64, a, None, "required"), (64, a + 4, far, "aligned")):
        with pytest.raises(RuntimeError, match="swap_fp32.*" + msg):
            _lib.call("hriemo_swap_fp32", x, y, n, None)

    def dev(n=64, p=a, avg=far, avg_state=a):
        _lib.call("hriemo_adamw_flat_dev_avg", p, a + 4096, a + 8192, a + 12288, n, a, a, avg, avg_state, None)

    def grouped(n=64, S=2, G=2, avg=far, avg_state=a):
        _lib.call("hriemo_adamw_flat_groups_avg", a, a + 4096, a + 8192, a + 12288, n, a, a, S, a, a, G, avg, avg_state, None)

    for fn, name in ((dev, "adamw_flat_dev_avg"), (grouped, "adamw_flat_groups_avg")):
        for kw, msg in ((dict(n=6), "n=6 must be a positive multiple of 4"), (dict(avg=None), "avg are required"),
                        (dict(avg=far + 4), "unaligned buffer"), (dict(avg_state=None), "avg_state are required"),
                        (dict(avg=a), "avg overlaps"), (dict(avg=a + 4096 + 240), "avg overlaps"), (dict(avg=a + 12288 - 16), "avg overlaps")):
            with pytest.raises(RuntimeError, match=name + ".*" + msg):
                fn(**kw)
    for kw, msg in ((dict(S=2049), r"S=2049 segments"), (dict(G=17), r"G=17 groups"), (dict(G=0), "G=0 groups")):
        with pytest.raises(RuntimeError, match="adamw_flat_groups_avg.*" + msg):
            grouped(**kw)

    def finalize(nblocks=1024, G=1, ctl=None, avg_hyper=a, avg_state=a):
        _lib.call("hriemo_optim_finalize_avg", a, nblocks, a, G, None, None, a, ctl, avg_hyper, avg_state, None)

    for kw, msg in ((dict(nblocks=0), "nblocks"), (dict(G=17), r"G=17 groups \(1 \.\. 16\)"), (dict(G=0), "G=0 groups"),
                    (dict(ctl=a + 2), "ctl"), (dict(avg_hyper=None), "avg_hyper and avg_state"), (dict(avg_state=None), "avg_hyper and avg_state"),
                    (dict(avg_state=a + 2), "avg_hyper and avg_state")):
        with pytest.raises(RuntimeError, match="optim_finalize_avg.*" + msg):
            finalize(**kw)


def test_checkpoint_format_on_host_buckets(monkeypatch):
    """the GPU check stubbed out (a construction and a state dict launch nothing): the "averaging" key and only it is new, the
    average starts as a bit copy of the parameters, a dict without the key restarts the average from the CURRENT parameters, and
    another mode or other shapes are refused before anything is written"""
    from hri_emo_amd import optim
    monkeypatch.setattr(optim, "_require_gpu", lambda t: None)
    m, buckets = _world()
    plain = optim.DeviceAdamW(buckets, lr=1e-3)
    assert not hasattr(plain, "avg") and plain.averaging is None and plain._hyper.shape == (8,)
    sd_plain = plain.state_dict()
    assert set(sd_plain) == {"state", "param_groups"}, "without averaging= the dict is the dict of before"
    with pytest.raises(RuntimeError, match="built without averaging="):
        plain.averaged_weights().__enter__()
    with pytest.raises(RuntimeError, match="built without averaging="):
        plain.averaged_state_dict(m)

    m2, buckets2 = _world()
    opt = optim.DeviceAdamW(buckets2, lr=1e-3, averaging="ema", avg_decay=0.99, avg_start=2, avg_every=3)
    assert opt._hyper.shape == (8,) and opt._avg_hyper.shape == (4,) and opt._avg_hyper.data_ptr() == opt._hyper.data_ptr() + 32
    assert torch.equal(opt.avg.view(torch.int32), opt.flat_p.view(torch.int32)) and opt.avg.data_ptr() != opt.flat_p.data_ptr()
    assert opt.n_averaged.dim() == 0 and float(opt.n_averaged) == 0.0 and opt.n_averaged.data_ptr() == opt._avg_state.data_ptr()
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "averaging"} and set(sd["state"]) == set(sd_plain["state"])
    av = sd["averaging"]
    assert set(av) == {"mode", "decay", "start", "every", "n_averaged", "avg"}
    assert (av["mode"], av["decay"], av["start"], av["every"]) == ("ema", 0.99, 2, 3) and set(av["avg"]) == set(sd["state"])
    order = [p for g in opt.param_groups for p in g["params"]]
    assert all(av["avg"][k].shape == p.shape and torch.equal(av["avg"][k], p.detach()) for k, p in enumerate(order))
    # averaged_state_dict: the model's keys, the averages' values, clones
    with torch.no_grad():
        opt.avg.mul_(2.0)
    asd = opt.averaged_state_dict(m2)
    assert list(asd) == list(m2.state_dict())
    assert all(torch.equal(asd[k], 2.0 * v) and asd[k].data_ptr() != v.data_ptr() for k, v in m2.state_dict().items())
    # a round trip restores values, counter and the host attributes
    saved = copy.deepcopy(sd)
    saved["averaging"]["n_averaged"] = torch.tensor(5.0)
    saved["averaging"]["decay"], saved["averaging"]["start"], saved["averaging"]["every"] = 0.5, 7, 1
    opt.load_state_dict(saved)
    assert float(opt.n_averaged) == 5.0 and (opt.avg_decay, opt.avg_start, opt.avg_every) == (0.5, 7, 1)
    assert all(torch.equal(opt._avg_view(p), saved["averaging"]["avg"][k]) for k, p in enumerate(order))
    # refusals: nothing written
    before = (opt.avg.clone(), opt.m.clone(), float(opt.n_averaged))
    other = copy.deepcopy(saved)
    other["averaging"]["mode"] = "swa"
    with pytest.raises(ValueError, match="average is 'swa'.*averaging='ema'"):
        opt.load_state_dict(other)
    other = copy.deepcopy(saved)
    other["averaging"]["avg"][3] = torch.zeros(5, 7)
    other["state"] = {}
    with pytest.raises(ValueError, match="averages' shapes do not match"):
        opt.load_state_dict(other)
    other = copy.deepcopy(saved)
    del other["averaging"]["avg"][0]
    with pytest.raises(ValueError, match="averages' shapes do not match"):
        opt.load_state_dict(other)
    with pytest.raises(ValueError, match="average is 'ema'.*averaging=None"):
        plain.load_state_dict(saved)
    assert torch.equal(opt.avg, before[0]) and torch.equal(opt.m, before[1]) and float(opt.n_averaged) == before[2]
    # a dict without the key (a torch optimizer's): the average restarts from the parameters as they are NOW
    with torch.no_grad():
        opt.flat_p.add_(1.0)
    opt.load_state_dict(sd_plain)
    assert float(opt.n_averaged) == 0.0 and torch.equal(opt.avg, opt.flat_p) and torch.equal(opt._avg_state, torch.zeros(4))
