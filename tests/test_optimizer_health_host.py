"""CPU suite of DeviceAdamW's health log (hri_emo_amd.optim.HealthLog, csrc/health.hip): the chunk table, the decoding of the
device buffer (arrays / blame / ratios) from hand-written images, naming, what is fixed at construction, the unchanged state dict,
the two ABI entries in header, library and binding with what their launchers refuse before they launch, and the float64 reference
of health_reference.py against a real torch.optim.AdamW."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import health_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 2048


def _tiny(monkeypatch, numels=(6, 200, 64), **kw):
    """a host optimizer over three vectors (the GPU check stubbed out: a construction launches nothing) -> (params, buckets, opt)"""
    from hri_emo_amd import optim
    from hri_emo_amd.dp import GradBuckets
    monkeypatch.setattr(optim, "_require_gpu", lambda t: None)
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n)) for n in numels]
    buckets = GradBuckets(params, overlap=False)
    return params, buckets, optim.DeviceAdamW(buckets, lr=1e-3, **kw)


# ------------------------------------------------------------------------------------------------------------ the chunk table
def test_health_chunks_cover_every_slot_once_in_order():
    from hri_emo_amd.optim import health_chunks
    lengths = [64, CHUNK, CHUNK + 64, 3 * CHUNK + 128, 64, 2 * CHUNK]
    groups = [0, 0, 1, 1, 0, 2]
    slots, start = [], 0
    for n, g in zip(lengths, groups):
        slots.append((start, n, g))
        start += n + (256 if g == 1 else 0)                    # a gap behind some slots: the table follows the slots, not a running sum
    rows = health_chunks(slots, CHUNK)
    assert [sum(1 for r in rows if r[2] == i) for i in range(6)] == [1, 1, 2, 4, 1, 2]
    assert [r[1] for r in rows if r[2] == 2] == [CHUNK, 64] and [r[1] for r in rows if r[2] == 3] == [CHUNK, CHUNK, CHUNK, 128]
    covered = np.zeros(start, dtype=np.int32)
    for s, n, i, g in rows:
        assert 0 < n <= CHUNK and s % 64 == 0 and n % 64 == 0 and g == groups[i], (s, n, i, g)
        assert slots[i][0] <= s and s + n <= slots[i][0] + slots[i][1]
        covered[s:s + n] += 1
    want = np.zeros(start, dtype=np.int32)
    for s, n, _ in slots:
        want[s:s + n] = 1
    assert np.array_equal(covered, want), "every element of every slot in exactly one chunk, nothing outside the slots"
    assert [r[2] for r in rows] == sorted(r[2] for r in rows), "the chunks of a parameter are neighbours"
    for i in range(6):
        starts = [r[0] for r in rows if r[2] == i]
        assert starts == sorted(starts) and all(b - a == CHUNK for a, b in zip(starts, starts[1:])), "ascending within a parameter"
    for bad in (1000, 0, -1024, 1536, True, 2048.0):
        with pytest.raises(ValueError, match="multiple of 1024"):
            health_chunks(slots, bad)
    for bad in ([(32, 64, 0)], [(0, 60, 0)], [(0, 0, 0)], [(0, 128, 0), (64, 64, 0)], []):
        with pytest.raises(ValueError, match="health_chunks"):
            health_chunks(bad, CHUNK)


def test_the_optimizer_builds_its_table_from_the_buckets(monkeypatch):
    from hri_emo_amd import optim
    params, buckets, opt = _tiny(monkeypatch, numels=(6, 200, 64), health=True)
    log = opt.health
    assert isinstance(log, optim.HealthLog) and (log.capacity, log.every) == (64, 1) and log.n_params == 3
    order = sorted(params, key=lambda q: buckets._offsets[id(q)])
    assert log._chunks.tolist() == [[buckets._offsets[id(q)], R.pad64(q.numel()), i, 0] for i, q in enumerate(order)]
    assert log._buf.dtype == torch.int32 and log._buf.numel() == 4 + 64 * (4 + 4 * 3) and int(log._buf.abs().sum()) == 0
    assert log._partial.numel() == 4 * 3
    # groups are carried through: the table names the group that owns each parameter
    monkeypatch.undo()
    params, buckets, opt = _tiny(monkeypatch, param_groups=None, health=None)
    assert opt.health is None
    monkeypatch.undo()
    from hri_emo_amd.dp import GradBuckets
    monkeypatch.setattr(optim, "_require_gpu", lambda t: None)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (6, 200, 64)]
    b = GradBuckets(ps, overlap=False)
    o = optim.DeviceAdamW(b, param_groups=[{"params": [ps[1]]}, {"params": [ps[0], ps[2]], "lr": 3e-5}], health=optim.HealthLog(4, 2))
    by_param = {id(q): gi for gi, g in enumerate(o.param_groups) for q in g["params"]}
    order = sorted(ps, key=lambda q: b._offsets[id(q)])
    assert [r[3] for r in o.health._chunks.tolist()] == [by_param[id(q)] for q in order]
    # refusals, in front of any allocation
    homes = [q.data_ptr() for q in ps]
    ps2 = [torch.nn.Parameter(torch.randn(8))]
    b2 = GradBuckets(ps2, overlap=False)
    with pytest.raises(ValueError, match="already attached"):
        optim.DeviceAdamW(b2, health=o.health)
    with pytest.raises(ValueError, match="health='on'"):
        optim.DeviceAdamW(b2, health="on")
    assert ps2[0].data_ptr() != 0 and homes == [q.data_ptr() for q in ps]
    for kw, msg in ((dict(capacity=0), "capacity=0"), (dict(every=0), "every=0"), (dict(capacity=1.5), "capacity=1.5"),
                    (dict(every=True), "every=True"), (dict(capacity=2 ** 20 + 1), "capacity=")):
        with pytest.raises(ValueError, match=msg):
            optim.HealthLog(**kw)


# ------------------------------------------------------------------------------------------------------------------- decoding
def _image(P, capacity, records, n_recorded, fill=0x5A5A5A5A):
    """the device buffer as csrc/health.hip lays it out; records = {slot: (step, kind, grad_norm, grad_sq, nonfinite, weight_sq,
    update_sq)}; slots that hold no record keep `fill`"""
    Rw = 4 + 4 * P
    img = np.full(4 + capacity * Rw, fill, dtype=np.int32)
    img[:4] = [n_recorded, 0, 0, 0]
    f = lambda x: np.asarray(x, dtype=np.float32).view(np.int32)  # noqa: E731
    for slot, (step, kind, norm, gsq, bad, wsq, usq) in records.items():
        rec = img[4 + slot * Rw:4 + (slot + 1) * Rw]
        rec[0], rec[1], rec[2], rec[3] = f(step), kind, f(norm), 0
        rec[4:4 + P], rec[4 + P:4 + 2 * P], rec[4 + 2 * P:4 + 3 * P], rec[4 + 3 * P:] = f(gsq), bad, f(wsq), f(usq)
    return img


def _rec(step, kind, seed, bad=(0, 0, 0)):
    rng = np.random.default_rng(seed)
    gsq, wsq, usq = (rng.random(3).astype(np.float32) + 0.5 for _ in range(3))
    if kind != 0:
        wsq, usq = np.zeros(3, np.float32), np.zeros(3, np.float32)
    return (float(step), kind, float(np.sqrt(gsq.sum())) if kind != 1 else float("inf"), gsq, np.asarray(bad, np.int32), wsq, usq)


def test_arrays_blame_and_ratios_decode_the_ring(monkeypatch):
    from hri_emo_amd import optim
    params, buckets, opt = _tiny(monkeypatch, health=optim.HealthLog(capacity=3, every=2))
    log = opt.health
    a = log.arrays()
    assert a["n_recorded"] == 0 and a["step"].shape == (0,) and a["grad_sq"].shape == (0, 3) and a["nonfinite"].dtype == np.int32
    assert log.blame() is None and a["names"] == ["param0", "param1", "param2"]
    with pytest.raises(IndexError):
        log.ratios()
    # two records in a ring of three: no wrap, no skipped record
    recs = {0: _rec(2, 0, 1), 1: _rec(4, 0, 2)}
    log._buf.copy_(torch.from_numpy(_image(3, 3, recs, 2)))
    a = log.arrays()
    assert a["n_recorded"] == 2 and a["step"].tolist() == [2.0, 4.0] and a["kind"].tolist() == [0, 0]
    assert a["grad_sq"].dtype == a["weight_sq"].dtype == a["update_sq"].dtype == np.float32 and a["grad_sq"].shape == (2, 3)
    for i, slot in enumerate((0, 1)):
        for key, col in (("grad_sq", 3), ("nonfinite", 4), ("weight_sq", 5), ("update_sq", 6)):
            assert np.array_equal(a[key][i], recs[slot][col]), (key, i)
        assert a["grad_norm"][i] == np.float32(recs[slot][2])
    assert log.blame() is None, "no skipped record in the ring"
    want = {f"param{j}": float(np.sqrt(np.float64(recs[1][6][j]) / np.float64(recs[1][5][j]))) for j in range(3)}
    assert log.ratios() == want and log.ratios(0) != want and log.ratios(-2) == log.ratios(0)
    # a wrapped ring: 7 records ever written, slots hold records 6 (slot 0), 4 (slot 1), 5 (slot 2) -> oldest first 4, 5, 6
    recs = {1: _rec(8, 0, 4), 2: _rec(8, 1, 5, bad=(0, 3, 1)), 0: _rec(10, 0, 6)}
    log._buf.copy_(torch.from_numpy(_image(3, 3, recs, 7)))
    a = log.arrays()
    assert a["n_recorded"] == 7 and a["step"].tolist() == [8.0, 8.0, 10.0] and a["kind"].tolist() == [0, 1, 0]
    assert np.isinf(a["grad_norm"][1]) and not a["weight_sq"][1].any() and not a["update_sq"][1].any()
    assert np.array_equal(a["grad_sq"][2], recs[0][3]) and np.array_equal(a["grad_sq"][0], recs[1][3])
    assert log.blame() == [("param1", 3), ("param2", 1)]
    with pytest.raises(ValueError, match="skipped step"):
        log.ratios(1)
    assert set(log.ratios()) == {"param0", "param1", "param2"}
    # the newest skipped record wins; a found_inf-only skip with finite gradients blames nobody
    recs = {1: _rec(8, 1, 4, bad=(9, 0, 0)), 2: _rec(8, 2, 5), 0: _rec(9, 0, 6)}
    log._buf.copy_(torch.from_numpy(_image(3, 3, recs, 10)))
    assert log.arrays()["kind"].tolist() == [1, 2, 0] and log.blame() == []
    # names
    log.name_parameters([("w.a", params[0]), ("stranger", torch.nn.Parameter(torch.zeros(2))), ("w.b", params[1]), ("w.c", params[2])])
    order = sorted(range(3), key=lambda j: buckets._offsets[id(params[j])])
    assert log.arrays()["names"] == [["w.a", "w.b", "w.c"][j] for j in order]
    recs = {0: _rec(1, 1, 4, bad=(1, 0, 2))}
    log._buf.copy_(torch.from_numpy(_image(3, 3, recs, 1)))
    assert log.blame() == [(log.names[0], 1), (log.names[2], 2)]
    with pytest.raises(ValueError, match=r"has no name.*shape \(200,\)|shape \(200,\).*has no name"):
        log.name_parameters([("w.a", params[0]), ("w.c", params[2])])
    assert log.names == [["w.a", "w.b", "w.c"][j] for j in order], "a refused naming changes nothing"
    # reset: the counters, one slice write
    log.reset()
    assert log.arrays()["n_recorded"] == 0 and log.blame() is None
    # the decoder refuses an image of another shape
    with pytest.raises(ValueError, match="decode_health"):
        optim.decode_health(np.zeros(10, np.int32), 3, 3)


def test_capacity_and_every_are_fixed_and_the_state_dict_does_not_change(monkeypatch):
    from hri_emo_amd import optim
    log = optim.HealthLog(capacity=5, every=3)
    for name in ("capacity", "every"):
        with pytest.raises(AttributeError, match="fixed at construction"):
            setattr(log, name, 7)
    assert (log.capacity, log.every) == (5, 3)
    for what in (log.arrays, log.reset, lambda: log.name_parameters([])):
        with pytest.raises(RuntimeError, match="not attached"):
            what()
    _, _, plain = _tiny(monkeypatch)
    monkeypatch.undo()
    _, _, logged = _tiny(monkeypatch, health=log)
    a, b = plain.state_dict(), logged.state_dict()
    assert set(a) == set(b) == {"state", "param_groups"} and a["param_groups"] == b["param_groups"] and set(a["state"]) == set(b["state"])
    for k in a["state"]:
        assert set(a["state"][k]) == set(b["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert all(torch.equal(a["state"][k][w], b["state"][k][w]) for w in a["state"][k])
    plain.load_state_dict(b)
    logged.load_state_dict(a)


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_health_entries_in_header_library_and_binding():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hriemo.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)

    def args_of(name):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    assert args_of("hriemo_health_sweep") == [
        "const float* g", "const float* p", "const float* m", "const float* v", "long n", "const long long* chunks", "int C",
        "const float* hyper", "const float* state", "int G", "const int* ctl", "int every", "float* partial", "hriemo_stream_t stream"]
    assert args_of("hriemo_health_fold") == [
        "const float* partial", "const long long* chunks", "int C", "int P", "const float* state", "const int* ctl",
        "const float* grad_scale", "int every", "int capacity", "int* log", "hriemo_stream_t stream"]
    for name, sig in (("hriemo_health_sweep", "pppplpippipipp"), ("hriemo_health_fold", "ppiipppiipp")):
        assert _lib._SIGS[name] == (sig, "i") and hasattr(L, name), name
    mk = open(os.path.join(REPO, "hri-emo_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bhealth\.hip\b", mk, flags=re.M)


def test_health_launchers_refuse_before_launching():
    """the checks run on the host in front of the launch (aligned dummy addresses that a refused call never dereferences)"""
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    a, far = 1 << 20, 1 << 26
    n = 4096

    def sweep(n=n, g=a, p=a + (1 << 16), partial=far, chunks=far + (1 << 16), C=4, G=2, ctl=None, every=1, state=far + (1 << 20)):
        _lib.call("hriemo_health_sweep", g, p, a + (2 << 16), a + (3 << 16), n, chunks, C, far + (1 << 21), state, G, ctl, every, partial, None)

    for kw, msg in ((dict(n=6), "n=6 must be a positive multiple of 4"), (dict(n=0), "positive multiple of 4"), (dict(g=None), "are required"),
                    (dict(partial=None), "are required"), (dict(p=a + (1 << 16) + 4), "unaligned buffer"), (dict(partial=far + 8), "unaligned buffer"),
                    (dict(C=0), "C=0 chunks"), (dict(C=(1 << 20) + 1), "chunks"), (dict(chunks=None), "chunks"), (dict(chunks=far + 4), "chunks"),
                    (dict(G=0), "G=0 groups"), (dict(G=17), "G=17 groups"), (dict(ctl=a + 2), "ctl"), (dict(every=0), "every=0"),
                    (dict(every=-3), "every=-3"), (dict(state=None), "hyper and state"),
                    (dict(partial=a), "partial overlaps"), (dict(partial=a + 4 * n - 16), "partial overlaps"),
                    (dict(partial=a + (1 << 16) - 16), "partial overlaps"), (dict(partial=far + (1 << 16) - 32), "partial overlaps"),
                    (dict(partial=far + (1 << 20) + 16), "partial overlaps")):
        with pytest.raises(RuntimeError, match="health_sweep.*" + msg):
            sweep(**kw)

    def fold(partial=far, chunks=far + (1 << 16), C=4, P=3, state=far + (1 << 20), ctl=None, gs=None, every=1, capacity=2, log=a):
        _lib.call("hriemo_health_fold", partial, chunks, C, P, state, ctl, gs, every, capacity, log, None)

    words = 4 + 2 * (4 + 4 * 3)                                 # the log of P = 3, capacity = 2
    for kw, msg in ((dict(capacity=0), "capacity=0"), (dict(capacity=-1), "capacity=-1"), (dict(every=0), "every=0"), (dict(P=0), "P=0 parameters"),
                    (dict(P=4097), "P=4097 parameters"), (dict(C=0), "C=0 chunks"), (dict(partial=None), "partial"), (dict(partial=far + 4), "partial"),
                    (dict(chunks=far + (1 << 16) + 4), "chunks"), (dict(state=None), "state is required"), (dict(ctl=a + 2), "ctl"),
                    (dict(log=None), "log"), (dict(log=a + 2), "log"),
                    (dict(log=far), "log overlaps"), (dict(log=far + 4 * 16 - 4), "log overlaps"), (dict(log=far - 4 * words + 4), "log overlaps"),
                    (dict(log=far + (1 << 16) + 16), "log overlaps"), (dict(log=far + (1 << 20) + 28), "log overlaps"),
                    (dict(gs=a + 4 * words - 4), "log overlaps"), (dict(ctl=a + 8), "log overlaps")):
        with pytest.raises(RuntimeError, match="health_fold.*" + msg):
            fold(**kw)


# ------------------------------------------------------------------------------------------------------------ the reference
def test_reference_replay_agrees_with_a_real_torch_adamw():
    """health_reference's two independent routes: a float64 torch.optim.AdamW stepped three times on float64 parameters, its state
    read by from_torch_adamw -- against replay_adamw64 + record_ref64 + scalars_adamw64 on the flat buffers.  Both are float64
    evaluations of the same formulas: 1e-10 relative."""
    torch.manual_seed(5)
    numels, groups_of = [6, 300, 64, 1000], [0, 0, 1, 1]
    hyper = [(1e-3, 0.9, 0.999, 1e-8, 1e-2), (3e-4, 0.8, 0.99, 1e-6, 0.0)]
    params = [torch.nn.Parameter(torch.randn(n, dtype=torch.float64) * 10.0 ** (i - 2)) for i, n in enumerate(numels)]
    opt = torch.optim.AdamW([{"params": [q for q, g in zip(params, groups_of) if g == gi], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3],
                              "weight_decay": h[4]} for gi, h in enumerate(hyper)])
    slots, total = R.slots_of(numels)
    flat = {k: torch.zeros(total, dtype=torch.float64) for k in "pmv"}
    for (s, _), q in zip(slots, params):
        flat["p"][s:s + q.numel()] = q.detach()
    for t in (1, 2, 3):
        grads = [torch.randn(n, dtype=torch.float64) * 10.0 ** (-i) for i, n in enumerate(numels)]
        g = torch.zeros(total, dtype=torch.float64)
        for (s, _), q, gr in zip(slots, params, grads):
            q.grad = gr.clone()
            g[s:s + q.numel()] = gr
        opt.step()
        flat["p"], flat["m"], flat["v"], norm = R.replay_adamw64(flat["p"], g, flat["m"], flat["v"], slots, groups_of, hyper, t, max_norm=0.0)
        mine = R.record_ref64(g, flat["p"], flat["m"], flat["v"], slots, groups_of, R.scalars_adamw64([h[:4] for h in hyper], t))
        theirs = R.from_torch_adamw(opt, params, grads)
        assert abs(norm - float(torch.cat(grads).norm())) <= 1e-12 * norm
        for key in ("grad_sq", "weight_sq", "update_sq"):
            err = ((mine[key] - theirs[key]).abs() / theirs[key]).max()
            assert float(err) <= 1e-10, (t, key, float(err))
        assert int(mine["nonfinite"].sum()) == 0
    # the bound's counts for the layouts the GPU tests use
    assert R.thread_roundings(64) == 4 and R.thread_roundings(32768) == 128 and R.thread_roundings(1028) == 8
    assert R.roundings(64, 32768) == (4 + 9 + 3, 4 + 9, 4 + 9 + 14) and R.roundings(3 * 32768 + 128, 32768) == (128 + 9 + 3 + 3, 128 + 9 + 3, 128 + 9 + 3 + 14)
    # a non-finite gradient element is counted and left out of the sum
    g = torch.ones(64)
    g[3], g[9] = float("nan"), float("-inf")
    rec = R.record_ref64(g, None, None, None, [(0, 64)], [0], None, grad_scale=2.0, real=False)
    assert int(rec["nonfinite"][0]) == 2 and float(rec["grad_sq"][0]) == 62 / 4.0 and float(rec["weight_sq"][0]) == 0.0
