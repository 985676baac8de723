"""CPU suite of the step-control block of the captured ragged step (capture_packed(partial_batches=, grad_accum=)): the ghost
bookkeeping against a small model of the rule written out here, the micro-step counter and flush_accumulated on a DataParallelStep
whose device work is replaced by recorders, the CPU formulas of the three losses with n_valid against slicing, the TypeError for a
loss without n_valid, the new C-ABI entries in header, library and binding, and the prefetcher's pass-through of a short batch."""
import ctypes
import functools
import os
import random
import re
import types

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- ghosts
def _model_of_the_rule(la, lt, B, La, Lt, buckets):
    """written independently of dp.ghost_plan: every missing utterance is one row of each modality, appended behind the batch; the
    bucket of a modality is the smallest multiple of its granule GREATER than the rows of batch and ghosts together"""
    out = []
    for own, L in ((la, La), (lt, Lt)):
        lens = [int(x) for x in own]
        while len(lens) < B:
            lens.append(1)
        g = (B * L) // buckets
        g -= g % 8
        g = min(max(g, 8), L)
        rows = sum(lens) + 1
        while rows % g:
            rows += 1
        out.append((lens, rows, sum(int(x) for x in own)))
    return out


def test_ghost_plan_lengths_key_and_ctl_words():
    from hri_emo_amd import dp
    rnd = random.Random(3)
    for trial in range(300):
        B = rnd.choice([1, 2, 5, 8, 64])
        La = rnd.choice([3, 8, 37, 70, 400])
        Lt = rnd.randint(1, La)
        n = rnd.randint(1, B) if trial % 7 else B
        la, lt = [rnd.randint(1, La) for _ in range(n)], [rnd.randint(1, Lt) for _ in range(n)]
        (ea, ka, oa), (et, kt, ot) = _model_of_the_rule(la, lt, B, La, Lt, dp._VARLEN_BUCKETS)
        fa, ft, key, own = dp.ghost_plan(la, lt, B, La, Lt)
        assert (fa, ft, key, own) == (ea, et, (ka, kt), (oa, ot)), (B, La, Lt, la, lt)
        assert len(fa) == len(ft) == B and fa[:n] == la and ft[:n] == lt
        # the ghosts' rows lie inside the region that is zeroed behind the batch's own rows, and the surplus sequence is not empty
        assert own[0] + (B - n) < key[0] and own[1] + (B - n) < key[1]
        # every bucket a short batch can need fits the static row sources (sized for the full batch of full-length utterances)
        assert key[0] <= dp.bucket_rows(B * La, B, La) and key[1] <= dp.bucket_rows(B * Lt, B, Lt)
        if n == B:
            assert key == (dp.bucket_rows(sum(la), B, La), dp.bucket_rows(sum(lt), B, Lt)), "a full batch keeps its key"
    assert dp.ctl_words(3, True, False) == [3, 1, 0, 0] and dp.ctl_words(5, 0, 1) == [5, 0, 1, 0]
    assert [dp.micro_flags(i, 3) for i in range(3)] == [(True, False), (False, False), (False, True)]
    assert dp.micro_flags(0, 1) == (True, True)


# ----------------------------------------------------------------------------- the micro-step counter
class _Recorder:
    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.log.append(name)
        return call


def _stub_step(k, partial, optimizer=True):
    """a DataParallelStep whose device work (loading the static state, the graph, the exchange, the optimizer) is recorded, not run"""
    from hri_emo_amd import _ops, dp
    s = object.__new__(dp.DataParallelStep)
    s.ctx = _ops.StepContext()
    s.events = []
    s._static = [torch.zeros(8, 16), torch.zeros(8, 16), None, None, torch.zeros(5, 4)]
    front = dp._RaggedFront(lens=None, masks=(), same_width=True, partial=partial, accum=k, ctl=object())
    s._pb = dp._PackedState(5, 7, 4, "cpu", front)
    s._record, s._replay, s._exchange_in_graph, s._micro = None, True, False, 0
    s.buckets = _Recorder()
    s.buckets.suspended = False
    s._optimizer = _Recorder() if optimizer else None
    graph = types.SimpleNamespace(replay=lambda: s.events.append("replay"))
    s._pb.graphs[(8, 8)] = dp._GraphRecord(graph, torch.zeros(()), [])          # the one bucket graph: the step counts as captured
    s._load_packed = lambda ra, rt, la, lt, y, ctl=None: s.events.append(("load", len(la), tuple(bool(c) for c in ctl))) or (8, 8)
    s._packed_graph = lambda key: s._pb.graphs[key]
    return s


def _batch(n):
    la, lt = [2] * n, [1] * n
    return torch.zeros(sum(la), 16), torch.zeros(sum(lt), 16), la, lt, torch.zeros(n, 4)


def test_micro_step_counter_and_flush():
    s = _stub_step(3, partial=True)
    for _ in range(2):                                         # two whole groups
        for i in range(3):
            assert s.micro_step == i
            s.step_packed(*_batch(5 if i < 2 else 3))
        assert s.micro_step == 0
    loads = [e for e in s.events if e != "replay"]
    assert loads == [("load", 5, (True, False)), ("load", 5, (False, False)), ("load", 3, (False, True))] * 2
    assert s.events.count("replay") == 6
    # the exchange, the hyper-parameter upload and nothing else of the optimizer: once per group
    assert s.buckets.log == ["finish"] * 2 and s._optimizer.log == ["_upload_hyper"] * 2
    # a group cut short: flush_accumulated() finishes the exchange and runs one eager optimizer step; nothing is replayed
    s.step_packed(*_batch(5))
    assert s.micro_step == 1 and s.events[-2:] == [("load", 5, (True, False)), "replay"]
    n_events = len(s.events)
    assert s.flush_accumulated() == 1 and s.micro_step == 0 and len(s.events) == n_events
    assert s.buckets.log == ["finish"] * 3 and s._optimizer.log == ["_upload_hyper"] * 2 + ["step"]
    assert s.flush_accumulated() == 0 and s._optimizer.log[-1] == "step" and len(s._optimizer.log) == 3, "nothing pending: nothing done"
    s.step_packed(*_batch(5))
    assert s.events[-2] == ("load", 5, (True, False)), "the next call opens a new group"


def test_refusals_come_before_any_load():
    s = _stub_step(1, partial=True)
    for args in (_batch(6), _batch(3)[:4] + (torch.zeros(5, 4),), (torch.zeros(0, 16), torch.zeros(0, 16), [], [], torch.zeros(0, 4))):
        with pytest.raises(ValueError):
            s.step_packed(*args)
    assert s.events == [] and s.micro_step == 0
    s = _stub_step(1, partial=False)
    with pytest.raises(ValueError, match="B = 5"):
        s.step_packed(*_batch(4))
    assert s.events == []
    s.step_packed(*_batch(5))
    assert s.events == [("load", 5, (True, True)), "replay"]


def test_loss_without_n_valid_is_a_type_error():
    from hri_emo_amd import _ops, dp, train
    for fn in (train.fusion_step_loss, train.fusion_step_loss_single_label, train.mosei_step_loss,
               functools.partial(train.mosei_step_loss, beta_entropy=0.01, grad_accum=2), lambda a, b, c, **kw: 0):
        assert dp._accepts_n_valid(fn)
    assert not dp._accepts_n_valid(lambda logits, beta, y: 0)
    s = object.__new__(dp.DataParallelStep)
    s.ctx = _ops.StepContext()
    s.model = types.SimpleNamespace(_forward_rows=None)
    s.loss_fn = lambda logits, beta, y: 0
    with pytest.raises(TypeError, match="n_valid"):
        s.capture_packed(None, None, None, None, None, pad_to=(7, 4), partial_batches=True)
    with pytest.raises(ValueError, match="grad_accum"):
        s.capture_packed(None, None, None, None, None, pad_to=(7, 4), grad_accum=0)


# ----------------------------------------------------------------------------- the CPU formulas
def test_cpu_losses_with_n_valid_equal_the_losses_of_the_slice():
    from hri_emo_amd import train
    g = torch.Generator().manual_seed(4)
    B, Ne = 6, 5
    x, beta = torch.randn(B, Ne, generator=g), torch.rand(B, 1, generator=g)
    y = (torch.rand(B, Ne, generator=g) < 0.3).float()
    lab = torch.randint(0, Ne, (B,), generator=g)
    pw = 0.5 + torch.rand(Ne, generator=g)
    for n in (1, 4, 6):
        nv = torch.tensor([n], dtype=torch.int32)
        xg, bg, yg = x.clone(), beta.clone(), y.clone()
        xg[n:], bg[n:], yg[n:] = float("nan"), float("nan"), float("nan")       # ghosts may hold anything
        assert torch.equal(train.fusion_step_loss(xg, bg, yg, n_valid=nv), train.fusion_step_loss(x[:n], beta[:n], y[:n]))
        assert torch.equal(train.fusion_step_loss_single_label(xg, bg, lab, n_valid=nv),
                           train.fusion_step_loss_single_label(x[:n], beta[:n], lab[:n]))
        kw = dict(pos_weight=pw, beta_entropy=0.01, grad_accum=2)
        assert torch.equal(train.mosei_step_loss(xg, bg, yg, n_valid=nv.view(()), **kw), train.mosei_step_loss(x[:n], beta[:n], y[:n], **kw))
        ref = F.binary_cross_entropy_with_logits(x[:n], y[:n]) - 0.01 * (beta[:n] * (1 - beta[:n])).mean()
        assert torch.equal(train.fusion_step_loss(xg, bg, yg, n_valid=nv), ref)
    assert torch.equal(train.fusion_step_loss(x, beta, y), train.fusion_step_loss(x, beta, y, n_valid=None))
    for bad in (0, 7):
        with pytest.raises(ValueError, match="n_valid"):
            train.fusion_step_loss(x, beta, y, n_valid=torch.tensor(bad, dtype=torch.int32))


# ----------------------------------------------------------------------------- ABI
def test_new_entries_in_header_library_and_binding():
    import hri_emo_amd  # noqa: F401
    from hri_emo_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hriemo.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    want = {"hriemo_fusion_loss_n": ("hriemo_fusion_loss", "const int* n_valid"), "hriemo_fusion_loss_ce_n": ("hriemo_fusion_loss_ce", "const int* n_valid"),
            "hriemo_optim_finalize_ctl": ("hriemo_optim_finalize", "const int* ctl")}
    for name, (base, extra) in want.items():
        m, mb = (re.search(r"int\s+" + nm + r"\s*\(([^)]*)\)\s*;", hdr) for nm in (name, base))
        assert m and mb, name
        args, base_args = ([" ".join(a.split()) for a in mm.group(1).split(",")] for mm in (m, mb))
        assert args == base_args[:-1] + [extra] + base_args[-1:], f"{name} is {base} plus `{extra}` in front of the stream"
        assert _lib._SIGS[name] == (_lib._SIGS[base][0][:-1] + "pp", "i") and hasattr(L, name)
    assert re.search(r"int\s+hriemo_grad_begin\s*\(\s*float\*\s*flat,\s*long\s+n,\s*const\s+int\*\s*ctl,\s*hriemo_stream_t\s+stream\s*\)\s*;", hdr)
    assert _lib._SIGS["hriemo_grad_begin"] == ("plpp", "i") and hasattr(L, "hriemo_grad_begin")
    assert L.hriemo_abi_version() == 1


# ----------------------------------------------------------------------------- the prefetcher
def test_prefetcher_passes_a_short_last_batch_through_on_cpu():
    from hri_emo_amd.data import DevicePrefetcher
    full = (torch.zeros(10, 16), [5, 5], torch.zeros(6, 16), [3, 3], torch.zeros(2, 4))
    short = (torch.zeros(4, 16), [4], torch.zeros(2, 16), [2], torch.zeros(1, 4))
    out = list(DevicePrefetcher([full, short], "cpu", ragged={0: 10, 2: 6}))
    assert len(out) == 2 and all(a is b for a, b in zip(out[1], short))
