"""Host side of the kernels: thin tensor->pointer wrappers over the C ABI (include/hriemo.h) and the
``torch.autograd.Function``s the mirrored nn.Modules (``models/``) are built from.

One Function per residual sub-layer of the reference (each is "LayerNorm(x + dropout(sub(x)))"):
  SelfAttnLN   models/cross_modal_block_tacfn.py:74-81,85-92 ; models/emotion_decoder.py:42-43
  CrossAttnLN  models/cross_modal_block_tacfn.py:98-105,111-118 ; models/emotion_decoder.py:48-55
  FFNLN        models/cross_modal_block_tacfn.py:106,119 ; models/emotion_decoder.py:58-59
  BetaGateFn   models/beta_gate_tacfn.py:68-118
  ExpandFn / RowDotFn  models/emotion_decoder.py:127,155
torch is used for device memory, streams and autograd bookkeeping only; all arithmetic on the path is in
libhriemo.so.  Activations are bf16, statistics/parameter gradients fp32.  No CPU fallback exists.
"""
import itertools
import os as _os
import threading
from collections import namedtuple

import torch

from . import _lib

BF16 = torch.bfloat16
_EPS = 1e-5
_apply_tls = threading.local()


# ----------------------------------------------------------------------------- plumbing
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _require_fp32_master(p):
    """Parameters stay fp32 (what AMP / the reference trainer keeps): the kernels read biases and LayerNorm affines as
    fp32 and cast weights to their bf16 shadows themselves.  model.half() / model.bfloat16() is refused loudly."""
    if p.dtype != torch.float32:
        raise TypeError(f"hri_emo_amd: parameter of dtype {p.dtype}; keep the module's parameters in fp32 "
                        "(the bf16 compute copies are made internally, as under torch.autocast)")


def _require_fp32_masters(*ps):
    for p in ps:
        if p is not None:
            _require_fp32_master(p)


def _require_gpu(t):
    if not t.is_cuda:
        raise RuntimeError(
            "hri_emo_amd runs on MI355X only: got a CPU tensor. There is no CPU fallback for this path "
            "(move the module and its inputs to 'cuda').")


_ws_cache = {}
_ws_retired = []           # outgrown workspaces a captured hipGraph may still point into: never freed
GRAPHS_ALIVE = 0           # number of captured steps that bake workspace pointers (dp.DataParallelStep.capture)


def workspace(nbytes, device, slot=0):
    """Caller-owned scratch for the C ABI (split-K slabs, column-sum partials); grows monotonically.
    One per (device, slot, stream): the audio and text branches may run on two streams concurrently.
    Once a step has been captured into a hipGraph the pointers of the workspaces it used are frozen inside the graph:
    an outgrown buffer is then retired (kept alive), never handed back to the allocator."""
    key = (device.index, slot, torch.cuda.current_stream(device).cuda_stream)
    t = _ws_cache.get(key)
    if t is None or t.numel() * 4 < nbytes:
        if t is not None and GRAPHS_ALIVE > 0:
            _ws_retired.append(t)
        n = max(int(nbytes), 64 << 20) // 4 + 16
        t = torch.empty(n, dtype=torch.float32, device=device)
        _ws_cache[key] = t
    return t


_side_streams = {}
TWO_STREAMS = _os_env_flag = None


def side_stream(device):
    """Second stream for the text branch of a CrossModalBlock (independent of the audio branch between the
    joins); None when disabled (HRIEMO_TWO_STREAMS=0)."""
    global TWO_STREAMS
    if TWO_STREAMS is None:
        import os
        TWO_STREAMS = os.environ.get("HRIEMO_TWO_STREAMS", "1") != "0"
    if not TWO_STREAMS:
        return None
    s = _side_streams.get(device.index)
    if s is None:
        s = torch.cuda.Stream(device=device)
        _side_streams[device.index] = s
    return s


class StepContext:
    """State of ONE model's step in flight -- what used to be module globals, so that two models (or two DataParallelSteps) in one
    process cannot see each other's capture flag, packed plan or gradient-join scope.  dp.DataParallelStep owns one and installs
    it around capture() / step() (use_context); models used on their own run on the module's default context.
      capturing      set by DataParallelStep.capture(): weight shadows are re-cast inside the graph, buffers are kept, not freed
      capture_origin the stream the capture runs on (every helper-stream fork must start there: fork())
      seq_override   (Seq audio, Seq text, Seq fused) injected for the bucketed packed graphs (models/cross_modal_block_tacfn.py)
      join_scope     > 0 inside a forward whose outputs ALL depend on both encoder branches (grad_join)
      half_reports   id(parameter) -> SharedProjFn nodes that have written their half of its gradient in this step
      stationary     set by dp.EvalStep(stationary=True) around the passes of a bucket graph: a capture derives no weight form
                     (form_stale), the step's weights pass keeps them fresh
      forms          a FormLog while such a step looks for the forms its forward asks for; None otherwise
      prologue       such a step's hand-over of the decoder's query prologue: prologue(decoder, B) -> the static (tgt, tgt32) layer 0
                     starts its cross-attention on (models/emotion_decoder.py); None otherwise
      act_log        a train.ActivationLog whose probes the sub-layers launch (probe()); None: no launch anywhere"""
    __slots__ = ("capturing", "capture_origin", "seq_override", "join_scope", "half_reports", "stationary", "forms", "prologue",
                 "act_log")

    def __init__(self):
        self.capturing, self.capture_origin, self.seq_override, self.join_scope, self.half_reports = False, None, None, 0, {}
        self.stationary, self.forms, self.prologue = False, None, None
        self.act_log = None


CTX = StepContext()        # the context in force


class use_context:
    """`with use_context(ctx):` -- ctx is the step context in force inside the block (re-entrant: the previous one comes back)"""

    def __init__(self, ctx):
        self.ctx, self.prev = ctx, None

    def __enter__(self):
        global CTX
        self.prev, CTX = CTX, self.ctx
        return self.ctx

    def __exit__(self, *exc):
        global CTX
        CTX = self.prev
        return False


def probe(key, half, x, seq):
    """A site of the activation log in force (train.ActivationLog): the statistics of x, whose rows are laid out as `seq`, go to the
    forward (half 0) or gradient (half 1) half of the site `key` names -- a sub-layer's dropout site id, or the site's name.  One
    launch of hriemo_act_probe on the current stream; nothing at all without a log or for a site the log does not keep.  No
    autograd node: x is only read."""
    log = CTX.act_log
    if log is None or not log.open[half]:
        # (no pass of the log is open: a sub-module called on its own inside log.watch(), or a backward behind close_backward() --
        # a probe without its plan launch in front would run under the window of the pass before)
        return
    site = log.index.get(key)
    if site is not None:
        log.probe(site, half, x.detach(), seq)


def fork(child, parent):
    """`child` starts to depend on `parent`: a stream fork.  While a step is being captured, every fork has to start at the
    capture's origin stream: a helper stream forked from an already forked stream (a fork nested inside a fork) makes
    hipStreamEndCapture segfault on ROCm 7.2 (gpurun_out/seg.log of round 2) -- raw HIP events or torch streams
    alike -- so that shape is refused here, as a Python exception, before anything reaches the runtime."""
    if CTX.capturing and CTX.capture_origin is not None and parent != CTX.capture_origin and child != CTX.capture_origin:
        raise RuntimeError("hri_emo_amd: a stream was forked from a stream that is itself a fork of the capture stream; ROCm 7.2 "
                           "crashes in hipStreamEndCapture on nested forks -- fork helper streams from the capturing stream only "
                           "(join the side stream back first), or run this step eagerly")
    child.wait_stream(parent)


_main_streams = {}


def note_main_stream(stream):
    """the stream a fusion block was entered on (its audio branch runs there, the text branch on the side stream)"""
    _main_streams[stream.device.index] = stream


def branch_streams(device):
    """streams the fusion blocks run on: the main one (as last noted) and the text-branch side stream if it exists"""
    out = [_main_streams.get(device.index, torch.cuda.current_stream(device))]
    side = _side_streams.get(device.index)
    if side is not None:
        out.append(side)
    return out


def share(t, stream):
    """tensor (or Seq: its index and mask tensors) produced on another stream is about to be read on `stream`"""
    if t is not None:
        t.record_stream(stream)
    return t


class TextBranch:
    """The text branch of a fusion block beside its audio branch: on `side` (side_stream()) while the audio branch runs on `main`,
    or, with side None, in line on main -- then all three operations do nothing and the block reads as one sequence of calls.
    Every fork starts at main (fork() refuses a nested one during capture), so a branch is joined before it is forked again."""

    def __init__(self, side, main):
        self.side, self.main = side, main

    def fork(self, *handed):
        """the branch starts behind everything enqueued on main; `handed`: what it will read of main's tensors (or Seqs)"""
        if self.side is not None:
            fork(self.side, self.main)
            for x in handed:
                share(x, self.side)

    def run(self):
        """`with branch.run():` -- the calls inside are enqueued on the branch"""
        return torch.cuda.stream(self.side)          # (a no-op context for None)

    def join(self, *back):
        """main goes on behind the branch; `back`: what main will read of the branch's tensors"""
        if self.side is not None:
            self.main.wait_stream(self.side)
            for x in back:
                share(x, self.main)


_site_counter = itertools.count(1)


def new_site_base():
    """Unique dropout-site id base for a module instance (3 sites per sub-layer)."""
    return next(_site_counter) * 4


_seed_words = {}
STEP_ID = 0                # bumped at the top of every model step (begin_step): "this shadow was already cast in this step"


def begin_step():
    global STEP_ID
    STEP_ID += 1
    CTX.half_reports.clear()

WEIGHTS_EPOCH = 0          # bumped by anything that rewrites parameter storage behind autograd's back (optim.FusedClipAdamW
                           # updates the flat buffer through raw pointers: p._version and p.data_ptr() do not move)


def bump_weights_epoch():
    """Invalidate every bf16 weight shadow: the next forward re-casts from the fp32 masters."""
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1


def seed_word(device):
    """Device-resident u64 added to every dropout seed (see include/hriemo.h): a captured step bumps it
    in-graph so each replay draws fresh masks while kernel arguments stay frozen."""
    t = _seed_words.get(device.index)
    if t is None:
        t = torch.zeros(1, dtype=torch.int64, device=device)
        _seed_words[device.index] = t
    return t


DROP_LOG = None          # tests: a list that receives every dropout site of a forward in call order --
                         # ("attn", seed, site, B, H, Lq, Lk, p, b_off) / ("rows", seed, site, M, N, p, row_off); the effective seed
                         # is seed + the device seed word (tests/hashrng.py rebuilds the keep-masks from these)
_ones = {}


def one(device):
    """the constant 1.0 a training loop may hand to ``loss.backward(gradient=...)``: the fused losses recognise this very tensor
    and skip the multiplication by the incoming gradient (two elementwise launches and a fill on the step's serial chain)"""
    t = _ones.get(device.index)
    if t is None:
        t = _ones[device.index] = torch.ones((), dtype=torch.float32, device=device)
    return t


def _is_one(g):
    t = _ones.get(g.device.index) if g.is_cuda else None
    return t is not None and g.data_ptr() == t.data_ptr() and g.dim() == 0


def bump_seed_word(device):
    _lib.call("hriemo_seed_bump", _p(seed_word(device)), _stream())      # golden-ratio increment (mod 2^64)


def next_seed(training):
    """Per-call dropout seed drawn from torch's CPU generator (reproducible under torch.manual_seed;
    identical on every DP rank that seeded identically)."""
    if not training:
        return 0
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def form_stale(ent, ver, device=None, once_per_step=True):
    """THE staleness rule of every cached weight form (bf16 shadows, concatenations, padded and MX-fp8 copies, the fp32 mode's
    splits): must the form be derived from its fp32 master(s) now?  ent: the cache entry (version key, form[, STEP_ID of its
    derivation]) or None; ver: the masters' version key now; device: where the form has to live (None: the site does not ask).
    Outside a capture: when there is no entry, the version key differs or the device does.  Inside a capture additionally whenever
    the form was not derived in this step yet -- the replayed graph must honour optimizer updates -- or, for a site that keeps no
    step id (once_per_step=False), always.  Inside a capture of a stationary step (CTX.stationary) nothing is derived: the step's
    weights pass has refreshed every form, so a stale one is an error, not a cast to record."""
    fresh = ent is not None and ent[0] == ver and (device is None or ent[1].device == device)
    if not CTX.capturing:
        return not fresh
    if CTX.stationary:
        if not fresh:
            raise RuntimeError("hri_emo_amd: a weight form is stale inside the capture of a stationary step (internal error: the "
                               "weights pass should have refreshed it) -- no cast is recorded")
        return False
    return not once_per_step or not fresh or len(ent) < 3 or ent[2] != STEP_ID


class FormLog:
    """The weight forms a forward asked for, in call order, as (key, getter, arguments): what a stationary dp.EvalStep replays as its
    weights pass.  A request whose key was known before the pass in flight is not kept again; within one pass every request is."""

    def __init__(self):
        self.known, self.new = set(), []

    def take(self):
        """the requests of the pass just run whose keys were not known before it"""
        new, self.new = self.new, []
        self.known.update(k for k, _, _ in new)
        return new


def _note_form(key, fn, *args):
    log = CTX.forms
    if log is not None and key not in log.known:
        log.new.append((key, fn, args))


class Shadows:
    """bf16 copies of fp32 master weights, refreshed when the master changes (optimizer step,
    load_state_dict, .to())."""

    def __init__(self):
        self._d = {}

    def get(self, p):
        key = id(p)
        _note_form(("get", id(self), key), self.get, p)
        ent = self._d.get(key)
        ver = (p._version, p.data_ptr(), WEIGHTS_EPOCH)
        # inside a capture every step re-casts (the replayed graph must honour optimizer updates), but only once per step:
        # a shadow prefetched at the top of the step (prefetch()) is not cast again on the decoder's serial chain
        if form_stale(ent, ver, p.device):
            s = ent[1] if ent is not None and ent[1].device == p.device and ent[1].shape == p.shape else \
                torch.empty(p.shape, dtype=BF16, device=p.device)
            _require_gpu(p)
            _require_fp32_master(p)
            src = p.detach()
            if not src.is_contiguous():
                src = src.contiguous()
            _lib.call("hriemo_cast_f32_to_bf16", _p(src), _p(s), src.numel(), _stream())
            ent = (ver, s, STEP_ID)
            self._d[key] = ent
        return ent[1]

    def prefetch(self, params):
        for p in params:
            self.get(p)

    def stale(self, p):
        """would get(p) cast now?  -> (needs a cast, destination tensor, version key)"""
        ent = self._d.get(id(p))
        ver = (p._version, p.data_ptr(), WEIGHTS_EPOCH)
        need = form_stale(ent, ver, p.device)
        dst = ent[1] if ent is not None and ent[1].device == p.device and ent[1].shape == p.shape else None
        return need, dst, ver

    def get_cat(self, parts):
        """bf16 shadow of the row-wise concatenation of master slices: parts = ((param, r0, r1), ...) -> [sum(r1 - r0), K].
        One GEMM per shared input (SharedProjFn) reads it; refreshed when any of the masters changes, like get()."""
        key = ("cat",) + tuple((id(p), r0, r1) for p, r0, r1 in parts)
        _note_form(("get_cat", id(self), key), self.get_cat, parts)
        ent = self._d.get(key)
        ver = tuple((p._version, p.data_ptr()) for p, _, _ in parts) + (WEIGHTS_EPOCH,)
        dev = parts[0][0].device
        if form_stale(ent, ver, dev):
            rows = sum(r1 - r0 for _, r0, r1 in parts)
            K = parts[0][0].shape[1]
            s = ent[1] if ent is not None and ent[1].device == dev else torch.empty((rows, K), dtype=BF16, device=dev)
            at = 0
            for p, r0, r1 in parts:
                _require_gpu(p)
                _require_fp32_master(p)
                src = p.detach()
                if not src.is_contiguous():
                    src = src.contiguous()
                _lib.call("hriemo_cast_f32_to_bf16", _p(src[r0:r1]), _p(s[at:at + (r1 - r0)]), (r1 - r0) * K, _stream())
                at += r1 - r0
            ent = (ver, s, STEP_ID)
            self._d[key] = ent
        return ent[1]

    def get_cat_wb(self, wparts, bparts):
        """get_cat(wparts) and get_cat_vec(bparts) refreshed together by ONE launch (hriemo_cast_copy_batch) -- a shared
        projection's [3d, d] bf16 weight shadow and [3d] fp32 bias; before: two casts, a torch.cat and a copy per refresh."""
        kw = ("cat",) + tuple((id(p), r0, r1) for p, r0, r1 in wparts)
        kb = ("catv",) + tuple((id(p), r0, r1) for p, r0, r1 in bparts)
        _note_form(("get_cat_wb", id(self), kw, kb), self.get_cat_wb, wparts, bparts)
        ew, eb = self._d.get(kw), self._d.get(kb)
        vw = tuple((p._version, p.data_ptr()) for p, _, _ in wparts) + (WEIGHTS_EPOCH,)
        vb = tuple((p._version, p.data_ptr()) for p, _, _ in bparts) + (WEIGHTS_EPOCH,)
        dev = wparts[0][0].device
        stale_w, stale_b = form_stale(ew, vw, dev), form_stale(eb, vb, dev)
        if not (stale_w or stale_b):
            return ew[1], eb[1]
        if not all(p.is_contiguous() for p, _, _ in wparts + bparts):
            return self.get_cat(wparts), self.get_cat_vec(bparts)
        K = wparts[0][0].shape[1]
        rows = sum(r1 - r0 for _, r0, r1 in wparts)
        nb = sum(r1 - r0 for _, r0, r1 in bparts)
        sw = ew[1] if ew is not None and ew[1].device == dev and ew[1].shape == (rows, K) else torch.empty((rows, K), dtype=BF16, device=dev)
        sb = eb[1] if eb is not None and eb[1].device == dev and eb[1].shape == (nb,) else torch.empty((nb,), dtype=torch.float32, device=dev)
        jobs, at = [], 0
        for p, r0, r1 in wparts:
            _require_gpu(p)
            _require_fp32_master(p)
            jobs.append((p.data_ptr() + r0 * K * 4, sw.data_ptr() + at * K * 2, (r1 - r0) * K, 0))
            at += r1 - r0
        at = 0
        for p, r0, r1 in bparts:
            _require_fp32_master(p)
            jobs.append((p.data_ptr() + r0 * 4, sb.data_ptr() + at * 4, r1 - r0, 1))
            at += r1 - r0
        if any(j[0] % 16 or j[1] % 16 for j in jobs):
            return self.get_cat(wparts), self.get_cat_vec(bparts)
        host = torch.tensor(jobs, dtype=torch.int64)
        _lib.call("hriemo_cast_copy_batch", host.data_ptr(), len(jobs), _stream())
        self._d[kw] = (vw, sw, STEP_ID)
        self._d[kb] = (vb, sb, STEP_ID)
        return sw, sb

    def get_cat_mx8(self, parts):
        """MX-fp8 form (bytes [rows, K], scales [K/32, ld]) of the row-wise concatenation of master slices, refreshed like
        mx8_shadow: every slice is quantised from its fp32 master straight into its rows of ONE buffer (the scale matrix is
        k-block major with one column per row, so a slice owns a column range of it)"""
        key = ("catmx",) + tuple((id(p), r0, r1) for p, r0, r1 in parts)
        _note_form(("get_cat_mx8", id(self), key), self.get_cat_mx8, parts)
        ent = self._d.get(key)
        ver = tuple((p._version, p.data_ptr()) for p, _, _ in parts) + (WEIGHTS_EPOCH,)
        if form_stale(ent, ver, once_per_step=False):
            rows = sum(r1 - r0 for _, r0, r1 in parts)
            K = parts[0][0].shape[1]
            dev = parts[0][0].device
            L_ = _lib.lib()
            ld = L_.hriemo_mx8_scale_ld(rows)
            if ent is not None and ent[1][0].shape == (rows, K) and ent[1][0].device == dev:
                q, sc = ent[1]
            else:
                q = torch.empty((rows, K), dtype=torch.uint8, device=dev)
                sc = torch.zeros((K // 32, ld), dtype=torch.uint8, device=dev)
            at = 0
            for p, r0, r1 in parts:
                _require_gpu(p)
                _require_fp32_master(p)
                src = p.detach()
                if not src.is_contiguous():
                    src = src.contiguous()
                src = src[r0:r1]
                _lib.call("hriemo_quant_mx8", _p(src), src.stride(0), 1, r1 - r0, K, q.data_ptr() + at * K, K, sc.data_ptr() + at, ld,
                          _stream())
                at += r1 - r0
            ent = (ver, (q, sc))
            self._d[key] = ent
        return ent[1]

    def get_cat_vec(self, parts):
        """fp32 concatenation of bias slices ((param, r0, r1), ...), cached like the weight shadows"""
        key = ("catv",) + tuple((id(p), r0, r1) for p, r0, r1 in parts)
        _note_form(("get_cat_vec", id(self), key), self.get_cat_vec, parts)
        ent = self._d.get(key)
        ver = tuple((p._version, p.data_ptr()) for p, _, _ in parts) + (WEIGHTS_EPOCH,)
        if form_stale(ent, ver):
            v = torch.cat([p.detach()[r0:r1] for p, r0, r1 in parts])
            if ent is not None and ent[1].shape == v.shape and ent[1].device == v.device:
                ent[1].copy_(v)           # same storage: a captured graph keeps pointing at it
                v = ent[1]
            ent = (ver, v, STEP_ID)
            self._d[key] = ent
        return ent[1]


FUSED_WGRAD = True


def enable_fused_wgrad(params, on=True):
    """Opt the given parameters into in-place gradient accumulation (GradSink below).  dp.GradBuckets does this for
    the parameters whose .grad it owns.  The contract changes for them: the Functions return None for these gradients
    and write ``p.grad`` directly, bias / LayerNorm gradients are final only when backward() returns (launch-boundary
    reduce), ``torch.autograd.grad(loss, params)`` yields nothing for them, and tensor / post-accumulate hooks of other
    libraries (torch DDP, optimizer-in-backward) never see them -- do not combine with foreign gradient hooks."""
    for p in params:
        p._hriemo_fused_grad = bool(on)


class GradSink:
    """Where a Function's parameter gradients go.  Default: fresh tensors returned to autograd (hooks, autograd.grad and
    foreign reducers work as usual).  If every parameter of the sub-layer was opted in (enable_fused_wgrad; dp.GradBuckets
    does it for its flat-buffer views) and owns a dense fp32 ``.grad``, the kernels accumulate straight into it (GEMM /
    column-reduce ``accumulate`` flag) and the Function returns None for it: no temporary, no autograd add kernel."""

    def __init__(self, params):
        self.params = params
        self.fused = FUSED_WGRAD and all(
            getattr(p, "_hriemo_fused_grad", False)
            and p.grad is not None and p.grad.dtype == torch.float32 and p.grad.is_contiguous()
            and p.grad.device == p.device and p.grad.shape == p.shape for p in params)
        if self.fused:
            for p in params:
                if hasattr(p, "_hriemo_grad_ready"):
                    p._hriemo_sink_managed = True      # dp.GradBuckets: only done() below reports this gradient

    def buf(self, p):
        return p.grad if self.fused else torch.empty(p.shape, dtype=torch.float32, device=p.device)

    def ret(self, t):
        return None if self.fused else t

    def done(self, skip=(), after_flush=()):
        """skip: parameters another Function still adds to in this backward (it reports them); after_flush: matrices whose
        gradient is a column sum finished by the launch-boundary reduce, like the vectors"""
        if self.fused:
            for p in self.params:
                if any(p is q for q in skip):
                    continue
                hook = getattr(p, "_hriemo_grad_ready", None)
                if hook is not None:
                    if (p.dim() < 2 or any(p is q for q in after_flush)) and _small_dw.touches(p.grad):
                        _small_dw.add_hook(hook, p, True)     # its column sum is still queued (decoder / gate sized bias gradient)
                    elif (p.dim() < 2 or any(p is q for q in after_flush)) and DEFER_REDUCE and _in_backward():
                        _deferred.add_hook(hook, p)       # bias / LayerNorm gradients are final only after the flush
                    elif p.dim() >= 2 and _small_dw.touches(p.grad):
                        _small_dw.add_hook(hook, p)       # its weight-gradient GEMM is still queued
                    else:
                        hook(p)


def prefetch_batch(pairs):
    """bf16 shadows of many masters in ONE launch per 64 matrices (hriemo_cast_f32_to_bf16_batch): pairs = ((Shadows, param), ...).
    The gate's and the decoder's fourteen matrices at the top of a step: one ~25 us launch instead of a chain of fourteen
    dependent ~5 us ones in front of whatever runs next on that stream."""
    _note_form(("prefetch_batch",) + tuple((id(sh), id(p)) for sh, p in pairs), prefetch_batch, pairs)
    jobs, upd = [], []
    for sh, p in pairs:
        need, dst, ver = sh.stale(p)
        if not need:
            continue
        _require_gpu(p)
        _require_fp32_master(p)
        if not p.is_contiguous() or p.data_ptr() % 16:
            sh.get(p)
            continue
        if dst is None:
            dst = torch.empty(p.shape, dtype=BF16, device=p.device)
        jobs.append((p.data_ptr(), dst.data_ptr(), p.numel()))
        upd.append((sh, id(p), ver, dst))
    if jobs:
        host = torch.tensor(jobs, dtype=torch.int64)
        _lib.call("hriemo_cast_f32_to_bf16_batch", host.data_ptr(), len(jobs), _stream())
        for sh, key, ver, dst in upd:
            sh._d[key] = (ver, dst, STEP_ID)


def padded_shadow(sh, p, kp):
    """bf16 shadow of a [N,K] weight zero-padded to [N,kp] (kp = K rounded up to 8: 16-byte rows)"""
    key = (id(p), "pad")
    _note_form(("padded_shadow", id(sh), key), padded_shadow, sh, p, kp)
    ent = sh._d.get(key)
    ver = (p._version, p.data_ptr(), WEIGHTS_EPOCH)
    if form_stale(ent, ver, p.device, once_per_step=False):
        _require_gpu(p)
        _require_fp32_master(p)
        s_ = ent[1] if ent is not None and ent[1].device == p.device else \
            torch.zeros((p.shape[0], kp), dtype=BF16, device=p.device)
        s_[:, :p.shape[1]].copy_(p.detach())
        ent = (ver, s_)
        sh._d[key] = ent
    return ent[1]


def to_bf16(x):
    return x if x.dtype == BF16 else x.to(BF16)


def mask_u8(mask, B, L):
    if mask is None:
        return None
    if mask.shape != (B, L):
        raise ValueError(f"key_padding_mask shape {tuple(mask.shape)} != {(B, L)}")
    m = mask.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)


# ----------------------------------------------------------------------------- raw kernel wrappers
def gemm(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, c_f32=False, bias=None, epi=0, aux=None, ldaux=0, accumulate=False):
    ws = workspace(64 << 20, C.device) if c_f32 else None
    _lib.call("hriemo_gemm_bf16", ta, tb, M, N, K, _p(A), lda, _p(B), ldb, _p(C), ldc, int(c_f32), _p(bias), epi,
              _p(aux), ldaux, int(accumulate), _p(ws), ws.numel() * 4 if ws is not None else 0, _stream())


def linear_fwd(x, w16, bias, relu=False, out_f32=False):
    """x [M,K] bf16 (row stride free), w16 [N,K] bf16 -> [M,N]"""
    M, K = x.shape
    N = w16.shape[0]
    y = torch.empty((M, N), dtype=torch.float32 if out_f32 else BF16, device=x.device)
    gemm(0, 0, M, N, K, x, x.stride(0), w16, w16.stride(0), y, N, c_f32=out_f32, bias=bias, epi=1 if relu else 0)
    return y


def linear_dx(dy, w16, epi=0, aux=None):
    """dX[M,K] = dY[M,N] . W[N,K]  (optionally * (aux>0) or + aux)"""
    M, N = dy.shape
    K = w16.shape[1]
    dx = torch.empty((M, K), dtype=BF16, device=dy.device)
    gemm(0, 1, M, K, N, dy, dy.stride(0), w16, w16.stride(0), dx, K, epi=epi, aux=aux,
         ldaux=aux.stride(0) if aux is not None else 0)
    return dx


FOLD_FFN_BIAS = True       # the first FFN Linear's bias gradient out of the dX GEMM's epilogue (hriemo_gemm_bf16_colsum)


def fold_ffn_bias():
    return FOLD_FFN_BIAS


def linear_dx_masked_colsum(dy, w16, aux, bias_out, accumulate):
    """dX[M,K] = (dY . W) * (aux > 0) and bias_out[K] (+)= colsum(dX) in one pass: the GEMM's epilogue leaves per-row-block
    partial sums of the tile it stores, finished by the launch-boundary reduce inside backward (fused path) or right here"""
    M, N = dy.shape
    K = w16.shape[1]
    dx = torch.empty((M, K), dtype=BF16, device=dy.device)
    rows = _lib.lib().hriemo_gemm_colsum_rows(0, 1, M, K, N)
    part = torch.empty(rows * K, dtype=torch.float32, device=dy.device)
    _lib.call("hriemo_gemm_bf16_colsum", 0, 1, M, K, N, _p(dy), dy.stride(0), _p(w16), w16.stride(0), _p(dx), K, _p(aux), aux.stride(0),
              _p(part), _stream())
    if accumulate and DEFER_REDUCE and _in_backward():
        _deferred.add(part, K, rows, K, 1, [bias_out], True)
    else:
        red = _DeferredReduce()
        red.device = dy.device
        red.add(part, K, rows, K, 1, [bias_out], accumulate, schedule=False)
        red.flush()
    return dx


def linear_dw(dy, x, out, accumulate=False):
    """out[N,K] (fp32, row stride free) (+)= dY[M,N]^T . X[M,K]"""
    M, N = dy.shape
    K = x.shape[1]
    if accumulate and M <= SMALL_DW_ROWS and _small_dw.enabled():
        _small_dw.add(dy, x, out)          # decoder / gate sized: issued later, beside the encoder's backward (class below)
        return
    gemm(1, 1, N, K, M, dy, dy.stride(0), x, x.stride(0), out, out.stride(0), c_f32=True, accumulate=accumulate)


def linear_dw_split(dy, x, out, out2, split, accumulate=False):
    """[out ; out2] (+)= dY[M,N]^T . X[M,K]: rows [0, split) of the [N, K] result to `out`, the rest to `out2` (one launch)"""
    M, N = dy.shape
    K = x.shape[1]
    ws = workspace(64 << 20, out.device)
    _lib.call("hriemo_gemm_bf16_split", 1, 1, N, K, M, _p(dy), dy.stride(0), _p(x), x.stride(0), _p(out), out.stride(0), _p(out2),
              out2.stride(0), split, int(accumulate), _p(ws), ws.numel() * 4, _stream())


# ---- MX-fp8 operand path (forward projection / FFN GEMMs; include/hriemo.h "MX-fp8 operand path")
GEMM_MODE = None           # 'bf16' | 'mx_fp8'; read from HRIEMO_GEMM at first use, set_gemm_mode() changes it at run time


def set_gemm_mode(mode):
    """'bf16' (default) or 'mx_fp8': forward nn.Linear / in-proj / out-proj GEMMs on block-scaled fp8 operands (BASELINE.json
    configs[4]); attention cores, backward GEMMs, masters and gradients are unchanged."""
    global GEMM_MODE
    if mode not in ("bf16", "mx_fp8"):
        raise ValueError(f"gemm mode {mode!r}: expected 'bf16' or 'mx_fp8'")
    GEMM_MODE = mode


def gemm_mode():
    global GEMM_MODE
    if GEMM_MODE is None:
        import os
        GEMM_MODE = os.environ.get("HRIEMO_GEMM", "bf16")
        if GEMM_MODE not in ("bf16", "mx_fp8"):
            raise ValueError(f"HRIEMO_GEMM={GEMM_MODE!r}: expected 'bf16' or 'mx_fp8'")
    return GEMM_MODE


# ---- arithmetic of the whole path: 'bf16' (product path: bf16 GEMM operands, fp32 accumulate, fp32 residual twins) or 'fp32'
# (hri-emo_amd/_fp32.py: the reference's fp32 arithmetic to 1e-3, forward and backward).  HRIEMO_PRECISION at
# first use, set_precision().
PRECISION = None


def set_precision(mode):
    global PRECISION
    if mode not in ("bf16", "fp32"):
        raise ValueError(f"set_precision: {mode!r} (expected 'bf16' or 'fp32')")
    PRECISION = mode


def precision():
    global PRECISION
    if PRECISION is None:
        import os
        mode = os.environ.get("HRIEMO_PRECISION", "bf16")
        if mode not in ("bf16", "fp32"):
            raise ValueError(f"HRIEMO_PRECISION={mode!r} (expected 'bf16' or 'fp32')")
        PRECISION = mode
    return PRECISION


def _fp32():
    from . import _fp32 as m
    return m


MX_MIN_ROWS = 1024     # below this a GEMM is latency-bound (decoder queries, gate MLP): fp8 operands buy nothing there


def mx8_ok(K, N, M):
    """shapes the scaled-MFMA path takes (a 128-deep step per MFMA, enough rows to be throughput-bound); anything else stays on
    the bf16 GEMM"""
    return K % 128 == 0 and N % 8 == 0 and M >= MX_MIN_ROWS


def want_mx_copy(M, d):
    """should a LayerNorm also emit the MX-fp8 copy of its [M, d] output (it feeds projection / FFN GEMMs)?"""
    return gemm_mode() == "mx_fp8" and d % 128 == 0 and M >= MX_MIN_ROWS


def quant_mx8(x, out=None):
    """x [M,K] bf16 or fp32 (row stride free) -> (e4m3 bytes [M,K], E8M0 scales [K/32, ld]); out: a pair of that form and device to
    write into (anything else: fresh buffers)"""
    M, K = x.shape
    L_ = _lib.lib()
    ld = L_.hriemo_mx8_scale_ld(M)
    if out is not None and out[0].shape == (M, K) and out[1].shape == (K // 32, ld) and out[0].device == out[1].device == x.device:
        q, sc = out
    else:
        q = torch.empty((M, K), dtype=torch.uint8, device=x.device)
        sc = torch.empty((K // 32, ld), dtype=torch.uint8, device=x.device)
    _lib.call("hriemo_quant_mx8", _p(x), x.stride(0), int(x.dtype == torch.float32), M, K, _p(q), K, _p(sc), ld, _stream())
    return q, sc


def linear_fwd_mx8(xq, xs, wq, ws, bias, relu=False, out_f32=False, want_q=False):
    """(xq, xs) [M,K] and (wq, ws) [N,K] quantised operands -> y [M,N] = x . w^T + bias; want_q: the epilogue also leaves the
    MX-fp8 form of y (the next GEMM's operand) attached to y (tag_mx): no quantisation pass over [M, N]"""
    M, K = xq.shape
    N = wq.shape[0]
    y = torch.empty((M, N), dtype=torch.float32 if out_f32 else BF16, device=xq.device)
    if want_q and not out_f32 and N % 128 == 0:
        ld = _lib.lib().hriemo_mx8_scale_ld(M)
        q = torch.empty((M, N), dtype=torch.uint8, device=xq.device)
        sc = torch.empty((N // 32, ld), dtype=torch.uint8, device=xq.device)
        _lib.call("hriemo_gemm_mx8_q", M, N, K, _p(xq), xq.stride(0), _p(xs), xs.stride(0), _p(wq), wq.stride(0), _p(ws), ws.stride(0),
                  _p(y), N, _p(bias), 1 if relu else 0, _p(q), N, _p(sc), ld, _stream())
        return tag_mx(y, (q, sc))
    _lib.call("hriemo_gemm_mx8", M, N, K, _p(xq), xq.stride(0), _p(xs), xs.stride(0), _p(wq), wq.stride(0), _p(ws), ws.stride(0),
              _p(y), N, int(out_f32), _p(bias), 1 if relu else 0, None, 0, _stream())
    return y


def mx8_shadow(sh, p, rows=None):
    """MX-fp8 copy (bytes, scales) of an fp32 master weight [N,K] (or of its row slice `rows`), refreshed like the bf16 shadow"""
    key = (id(p), "mx8", rows)
    _note_form(("mx8_shadow", id(sh), key), mx8_shadow, sh, p, rows)
    ent = sh._d.get(key)
    ver = (p._version, p.data_ptr(), WEIGHTS_EPOCH)
    if form_stale(ent, ver, once_per_step=False):
        _require_gpu(p)
        _require_fp32_master(p)
        src = p.detach()
        if rows is not None:
            src = src[rows[0]:rows[1]]
        if not src.is_contiguous():
            src = src.contiguous()
        # a refresh writes into the buffers the form already has: a captured graph (and a stationary evaluation, whose bucket
        # graphs never derive it themselves) keeps pointing at them
        ent = (ver, quant_mx8(src, out=ent[1] if ent is not None else None))
        sh._d[key] = ent
    return ent[1]


class Operand:
    """A GEMM input in the formats the forward may want: the bf16 rows and, lazily and at most once, their MX-fp8 form
    (handed over by the producing LayerNorm when it emitted one)."""
    __slots__ = ("x", "_q")

    def __init__(self, x, q=None):
        self.x, self._q = x, q

    def q(self):
        if self._q is None:
            self._q = quant_mx8(self.x)
        return self._q


def mx_of(t):
    """the MX-fp8 copy a producing LayerNorm attached to its output tensor (None if there is none)"""
    return getattr(t, "_hriemo_mx", None)


def tag_mx(t, mx):
    if mx is not None:
        t._hriemo_mx = mx
    return t


def proj_fwd(xop, sh, w, w16, bias, rows=None, relu=False, out_f32=False, want_q=False):
    """y = x . W[rows]^T + bias[rows] on the configured operand format.  xop: Operand or bf16 tensor; want_q (fp8 mode): y is the
    operand of another GEMM -- its MX-fp8 form comes out of this GEMM's epilogue, attached to y"""
    x = xop.x if isinstance(xop, Operand) else xop
    K = x.shape[1]
    N = (rows[1] - rows[0]) if rows is not None else w.shape[0]
    b = bias if rows is None or bias is None else bias[rows[0]:rows[1]]
    if gemm_mode() == "mx_fp8" and mx8_ok(K, N, x.shape[0]):
        xq, xs = xop.q() if isinstance(xop, Operand) else quant_mx8(x)
        wq, ws = mx8_shadow(sh, w, rows)
        return linear_fwd_mx8(xq, xs, wq, ws, b, relu=relu, out_f32=out_f32, want_q=want_q)
    wv = w16 if rows is None else w16[rows[0]:rows[1]]
    return linear_fwd(x, wv, b, relu=relu, out_f32=out_f32)


_GEMM_FLAGS_EXPLICIT = False


def gemm_flags():
    """the tuning word of hriemo_gemm_debug_flags that is in force right now (read back from the library)"""
    L = _lib.lib()
    cur = L.hriemo_gemm_debug_flags(0)
    L.hriemo_gemm_debug_flags(cur)
    return cur


def set_gemm_flags(word):
    """Set the GEMM tuning word (include/hriemo.h: hriemo_gemm_debug_flags) for good: gemm_contended() then leaves it alone, so a
    caller's choice of the tile walk (bit 3) is what runs.  None hands bit 3 back to gemm_contended.  Returns the previous word."""
    global _GEMM_FLAGS_EXPLICIT
    _GEMM_FLAGS_EXPLICIT = word is not None
    return _lib.lib().hriemo_gemm_debug_flags(word) if word is not None else gemm_flags()


def gemm_contended(on, force=False):
    """Will other kernels (RCCL collectives) hold CUs while the GEMMs run?  True: the loader / consumer GEMM draws its tiles from
    the per-XCD work queue (with 32 CUs held a 25600x3072x768 launch takes 140 us, 184 on the static walk; 118-124 alone); False
    (default): static walk, 5-8 % faster per launch on a chip the kernel has to itself, the same step time
    (profiles/r04_gemm_ws.log).  Bit 3 of hriemo_gemm_debug_flags and nothing else of that word; a word set through
    set_gemm_flags() is kept as it is unless `force` (DataParallelStep(force_queue=...)).  No-op without a GPU."""
    if not torch.cuda.is_available() or (_GEMM_FLAGS_EXPLICIT and not force):
        return
    cur = gemm_flags()
    want = (cur & ~8) if on else (cur | 8)
    if want != cur:
        _lib.lib().hriemo_gemm_debug_flags(want)


FUSE_LN = None             # Linear + bias + dropout + residual + LayerNorm in one launch (csrc/gemm_ln.hip); HRIEMO_FUSE_LN=1
FUSE_LN_MIN_ROWS = 1024    # a full-row tile is one workgroup per 64 rows: the decoder's M = 384 would use 6 CUs


def fuse_ln(M, d):
    """should this sub-layer's output projection run fused with its LayerNorm?"""
    global FUSE_LN
    if FUSE_LN is None:
        import os
        FUSE_LN = os.environ.get("HRIEMO_FUSE_LN", "0") == "1"
    return FUSE_LN and gemm_mode() == "bf16" and M >= FUSE_LN_MIN_ROWS and bool(_lib.lib().hriemo_gemm_ln_supported(d))


def proj_add_ln_fwd(a, w16, bias, x, x32, gamma, beta, p, seed, site, row_off, want32, rows=None):
    """g = a . W^T + bias (bf16, kept for the backward); y = LN(x + drop(g)) -> (g, y, y32 | None, mean, rstd): the results of
    proj_fwd + add_ln_fwd from ONE kernel (full-row tiles, row statistics reduced across the waves of a workgroup)"""
    M, K = a.shape
    d = w16.shape[0]
    dev = a.device
    g = torch.empty((M, d), dtype=BF16, device=dev)
    y = torch.empty((M, d), dtype=BF16, device=dev)
    y32 = torch.empty((M, d), dtype=torch.float32, device=dev) if want32 else None
    mean = torch.empty(M, dtype=torch.float32, device=dev)
    rstd = torch.empty(M, dtype=torch.float32, device=dev)
    if DROP_LOG is not None and p > 0 and rows is None:
        DROP_LOG.append(("rows", seed, site, M, d, float(p), row_off))
    _lib.call("hriemo_gemm_ln_fwd", M, d, K, _p(a), a.stride(0), _p(w16), w16.stride(0), _p(bias), _p(x), _p(x32), _p(gamma), _p(beta),
              _p(g), _p(y), _p(y32), _p(mean), _p(rstd), _EPS, float(p), seed, _p(seed_word(dev)), site, row_off, _p(rows), _stream())
    return g, y, y32, mean, rstd


def colsum(x, out, accumulate=False):
    M, N = x.shape
    L_ = _lib.lib()
    if accumulate and M <= SMALL_DW_ROWS and not _small_dw.flushing and _small_dw.enabled():
        _small_dw.add(x, None, out)        # decoder / gate sized bias gradient: off the serial chain, like the weight gradients
        return
    if accumulate and DEFER_REDUCE and _in_backward() and not _small_dw.in_final:
        rows = L_.hriemo_colsum_partial_rows(M, N)
        part = torch.empty(rows * N, dtype=torch.float32, device=x.device)
        _lib.call("hriemo_colsum_bf16", _p(x), x.stride(0), M, N, None, 0, _p(part), _stream())
        _deferred.add(part, N, rows, N, 1, [out], True)
        return
    ws = workspace(L_.hriemo_colsum_workspace_bytes(M, N), x.device, slot=1)
    _lib.call("hriemo_colsum_bf16", _p(x), x.stride(0), M, N, _p(out), int(accumulate), _p(ws), _stream())


def _in_backward():
    """True while the autograd engine is running a backward pass on this thread (final callbacks can be queued)."""
    try:
        return torch._C._current_graph_task_id() != -1
    except AttributeError:
        return False


# Dropout keep-mask as bit words from the forward to the backward (include/hriemo.h, drop_mask_bits).  Measured at cfg 2: in the
# two-kernel backward the bit words save the hash but cost three registers in the dK/dV kernel (a wave per SIMD at head_dim 96)
# and a 2-byte store per lane and key tile in the forward -- no gain; in the single-pass backward (16 < L_k <= 128) they pay
# (profiles/r02_attention.log).  So a site asks for them exactly when its backward is the single kernel.
def attn_mask_bits(B, H, Lk, hd, Lq=None):
    if Lq is not None:
        return bool(_lib.lib().hriemo_attn_bwd_single_pass_q(B, H, Lq, Lk, hd))
    return bool(_lib.lib().hriemo_attn_bwd_single_pass(B, H, Lk, hd))


# fp8 GEMM mode on packed rows: the attention forward leaves the MX-fp8 copy of O itself (hriemo_attn_fwd_q_varlen), as the padded
# launch does.  False: the previous launches (hriemo_attn_fwd_varlen, then hriemo_quant_mx8 in front of the out-projection) -- the
# A/B handle; the results are bit-identical.
ATTN_Q_VARLEN = True


def attn_fwd(q, k, v, B, H, Lq, Lk, hd, kpm, p, seed, site, b_off, want_bits=False, cu=None):
    """-> (o, lse) or, with want_bits, (o, lse, mask_bits|None): the dropout keep-mask as bit words for the backward.
    cu = (cu_seqlens_q, cu_seqlens_k) int32 device tensors: q / k / v hold packed rows, Lq / Lk are the longest sequences, kpm is None"""
    o = torch.empty((q.shape[0], H * hd), dtype=BF16, device=q.device)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    if DROP_LOG is not None and p > 0:
        DROP_LOG.append(("attn", seed, site, B, H, Lq, Lk, float(p), b_off))
    mb = None
    if want_bits and p > 0:
        mb = torch.empty(_lib.lib().hriemo_attn_mask_bytes(B, H, Lq, Lk) // 8, dtype=torch.int64, device=q.device)
    if (cu is None or ATTN_Q_VARLEN) and hd % 32 == 0 and want_mx_copy(q.shape[0], H * hd):
        # fp8 GEMM mode: the out-projection's operand leaves the attention kernel already quantised (tagged onto o)
        n = q.shape[0]
        ld = _lib.lib().hriemo_mx8_scale_ld(n)
        oq = torch.empty((n, H * hd), dtype=torch.uint8, device=q.device)
        so = torch.empty((H * hd // 32, ld), dtype=torch.uint8, device=q.device)
        if cu is not None:        # packed rows: the scale byte of packed row r is column r
            _lib.call("hriemo_attn_fwd_q_varlen", _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                      _p(cu[0]), _p(cu[1]), _p(lse), B, H, Lq, Lk, hd, float(p), seed, _p(seed_word(q.device)), site, b_off, _p(mb),
                      _p(oq), H * hd, _p(so), ld, n, _stream())
        else:
            _lib.call("hriemo_attn_fwd_q", _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                      _p(kpm), _p(lse), B, H, Lq, Lk, hd, float(p), seed, _p(seed_word(q.device)), site, b_off, _p(mb), _p(oq), H * hd,
                      _p(so), ld, _stream())
        tag_mx(o, (oq, so))
        return (o, lse, mb) if want_bits else (o, lse)
    if cu is not None:
        _lib.call("hriemo_attn_fwd_varlen", _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                  _p(cu[0]), _p(cu[1]), _p(lse), B, H, Lq, Lk, hd, float(p), seed, _p(seed_word(q.device)), site, b_off, _p(mb),
                  _stream())
    else:
        _lib.call("hriemo_attn_fwd", _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                  _p(kpm), _p(lse), B, H, Lq, Lk, hd, float(p), seed, _p(seed_word(q.device)), site, b_off, _p(mb), _stream())
    return (o, lse, mb) if want_bits else (o, lse)


def attn_bwd(q, k, v, o, do, dq, dk, dv, lse, B, H, Lq, Lk, hd, kpm, p, seed, site, b_off, bias_grad=None, mask_bits=None, cu=None):
    """bias_grad = (db_q [d], db_kv [2d]) fp32 views the column sums of dQ and dK|dV go to: the kernels leave per-block partial
    sums behind (fp32 values before the bf16 rounding of dQ/dK/dV); inside backward with the fused path they are finished by the
    launch-boundary reduce (accumulating), otherwise by one reduce launch right here (overwriting).  Returns True if it took
    care of them."""
    delta = torch.empty_like(lse)
    pq = pkv = None
    fold = bias_grad is not None and FOLD_ATTN_BIAS
    if fold:
        L_ = _lib.lib()
        rq, rk = L_.hriemo_attn_bwd_dq_colsum_rows(B, H, Lq, Lk, hd), L_.hriemo_attn_bwd_kv_colsum_rows(B, H, Lq, Lk, hd)
        pq = torch.empty(rq * H * hd, dtype=torch.float32, device=q.device)
        pkv = torch.empty(rk * 2 * H * hd, dtype=torch.float32, device=q.device)
    if cu is not None:
        _lib.call("hriemo_attn_bwd_varlen", _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                  _p(do), do.stride(0), _p(dq), dq.stride(0), _p(dk), dk.stride(0), _p(dv), dv.stride(0), _p(cu[0]), _p(cu[1]),
                  _p(lse), _p(delta), B, H, Lq, Lk, hd, float(p), seed, _p(seed_word(q.device)), site, b_off,
                  _p(pq), _p(pkv), _p(mask_bits), _stream())
    else:
        _lib.call("hriemo_attn_bwd", _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                  _p(do), do.stride(0), _p(dq), dq.stride(0), _p(dk), dk.stride(0), _p(dv), dv.stride(0), _p(kpm),
                  _p(lse), _p(delta), B, H, Lq, Lk, hd, float(p), seed, _p(seed_word(q.device)), site, b_off,
                  _p(pq), _p(pkv), _p(mask_bits), _stream())
    if fold:
        d = H * hd
        deferred = bias_grad[2] if len(bias_grad) > 2 else False
        if deferred and DEFER_REDUCE and _in_backward():
            _deferred.add(pq, d, rq, d, 1, [bias_grad[0]], True)
            _deferred.add(pkv, 2 * d, rk, 2 * d, 1, [bias_grad[1]], True)
        else:
            red = _DeferredReduce()
            red.device = q.device
            red.add(pq, d, rq, d, 1, [bias_grad[0]], deferred, schedule=False)
            red.add(pkv, 2 * d, rk, 2 * d, 1, [bias_grad[1]], deferred, schedule=False)
            red.flush()
    attn_bwd.last_delta = delta          # scratch of the last call (diagnostics: scripts_dev/dbg_attn.py)
    return fold


class LogSite:
    """Where the maps of ONE attention site go when a train.AttentionLog takes them: the site's log tensor [capacity, Lq, Lk], the
    log's window word {slot0, n_take, 0, 0} (device memory, written by hriemo_attn_log_plan at the top of the pass) and the capacity.
    A site is handed this in the place of its need flag (it is truthy) and then returns no map: the samples inside the window are
    in the log.  B: the number of samples of the pass -- a bucket plan's filler sequence has no sample to export."""
    __slots__ = ("maps", "window", "capacity", "B")

    def __init__(self, maps, window, capacity, B):
        self.maps, self.window, self.capacity, self.B = maps, window, int(capacity), int(B)

    def take(self, B, Lq, Lk):
        """the number of samples to launch for, after checking that this site's maps are [., Lq, Lk]"""
        if tuple(self.maps.shape[1:]) != (Lq, Lk):
            raise ValueError(f"attention log: a site exports maps [{Lq}, {Lk}]; its log holds {tuple(self.maps.shape[1:])}")
        return min(B, self.B)


def _log_append(out, site):
    """a map [B, Lq, Lk] that a padded export produced, into the site's log under the window (hriemo_attn_log_append)"""
    n = site.take(out.shape[0], out.shape[1], out.shape[2])
    _lib.call("hriemo_attn_log_append", _p(out), n, out.shape[1] * out.shape[2], _p(site.window), _p(site.maps), site.capacity, _stream())


def attn_probs(q, k, B, H, Lq, Lk, hd, kpm, lse, p, seed, site, b_off, cu=None, out_l=None, log=None):
    """head-averaged probabilities [B, Lq, Lk].  cu = (cu_seqlens_q, cu_seqlens_k): q / k hold packed rows, Lq / Lk are the longest
    sequences and out_l = (L_q, L_k) the padded lengths of the two layouts: the padded map [B, L_q, L_k] comes back, zeros in the
    PAD key columns and the PAD query rows (every element is written by the kernel).
    log (a LogSite): the maps go to the site's log and None comes back -- straight from the packed export (hriemo_attn_probs_varlen_log),
    or from the padded export through one append."""
    if cu is not None and log is not None:
        n = log.take(B, out_l[0], out_l[1])
        _lib.call("hriemo_attn_probs_varlen_log", _p(q), q.stride(0), _p(k), k.stride(0), _p(cu[0]), _p(cu[1]), _p(lse), _p(log.maps), n, H,
                  Lq, Lk, out_l[0], out_l[1], hd, float(p), seed, _p(seed_word(q.device)), site, b_off, _p(log.window), log.capacity, _stream())
        return None
    if cu is not None:
        out = torch.empty((B,) + tuple(out_l), dtype=torch.float32, device=q.device)
        _lib.call("hriemo_attn_probs_varlen", _p(q), q.stride(0), _p(k), k.stride(0), _p(cu[0]), _p(cu[1]), _p(lse), _p(out), B, H,
                  Lq, Lk, out_l[0], out_l[1], hd, float(p), seed, _p(seed_word(q.device)), site, b_off, _stream())
        return out
    out = torch.empty((B, Lq, Lk), dtype=torch.float32, device=q.device)
    _lib.call("hriemo_attn_probs_mfma" if MFMA_MAPS else "hriemo_attn_probs", _p(q), q.stride(0), _p(k), k.stride(0), _p(kpm), _p(lse), _p(out), B, H, Lq, Lk,
              hd, float(p), seed, _p(seed_word(q.device)), site, b_off, _stream())
    if log is not None:
        _log_append(out, log)
        return None
    return out


def add_ln_fwd(g, x, gamma, beta, p, seed, site, row_off, x32=None, want32=False, want_mx=False, rows=None):
    """y = LN(x + drop(g)); x32 = fp32 twin of the residual stream (used instead of x when given);
    want32 -> also return the fp32 twin of y; want_mx -> also the MX-fp8 copy (bytes, scales) of y as a 5th result."""
    M, d = g.shape
    y = torch.empty((M, d), dtype=BF16, device=g.device)
    y32 = torch.empty((M, d), dtype=torch.float32, device=g.device) if want32 else None
    mean = torch.empty(M, dtype=torch.float32, device=g.device)
    rstd = torch.empty(M, dtype=torch.float32, device=g.device)
    if DROP_LOG is not None and p > 0 and rows is None:
        DROP_LOG.append(("rows", seed, site, M, d, float(p), row_off))
    if rows is not None:          # packed rows: the dropout hash is keyed by the row of the padded layout
        yq = ys = None
        ld = 0
        if want_mx:
            ld = _lib.lib().hriemo_mx8_scale_ld(M)
            yq = torch.empty((M, d), dtype=torch.uint8, device=g.device)
            ys = torch.empty((d // 32, ld), dtype=torch.uint8, device=g.device)
        _lib.call("hriemo_add_ln_fwd_rows", _p(g), _p(x), _p(x32), _p(gamma), _p(beta), _p(y), _p(y32), _p(mean), _p(rstd), M, d,
                  _EPS, float(p), seed, _p(seed_word(g.device)), site, row_off, _p(yq), _p(ys), ld, _p(rows), _stream())
        return (y, y32, mean, rstd, (yq, ys)) if want_mx else (y, y32, mean, rstd)
    if want_mx:
        ld = _lib.lib().hriemo_mx8_scale_ld(M)
        yq = torch.empty((M, d), dtype=torch.uint8, device=g.device)
        ys = torch.empty((d // 32, ld), dtype=torch.uint8, device=g.device)
        _lib.call("hriemo_add_ln_fwd_mx8", _p(g), _p(x), _p(x32), _p(gamma), _p(beta), _p(y), _p(y32), _p(mean), _p(rstd), M, d,
                  _EPS, float(p), seed, _p(seed_word(g.device)), site, row_off, _p(yq), _p(ys), ld, _stream())
        return y, y32, mean, rstd, (yq, ys)
    _lib.call("hriemo_add_ln_fwd", _p(g), _p(x), _p(x32), _p(gamma), _p(beta), _p(y), _p(y32), _p(mean), _p(rstd), M, d,
              _EPS, float(p), seed, _p(seed_word(g.device)), site, row_off, _stream())
    return y, y32, mean, rstd


def add_ln_bwd(dy, g, x, gamma, mean, rstd, p, seed, site, row_off, want_dx=True, outs=None, accumulate=False, x32=None, rows=None):
    """outs = (dgamma, dbeta, dbias) destination tensors (fp32 [d]); fresh ones when None.  rows: the row index that keys the
    dropout hash (packed sequences), see add_ln_fwd."""
    M, d = g.shape
    dev = g.device
    dx = torch.empty((M, d), dtype=BF16, device=dev) if want_dx else None
    dg = torch.empty((M, d), dtype=BF16, device=dev) if (p > 0 or not want_dx) else None
    if outs is None:
        stats = torch.empty((3, d), dtype=torch.float32, device=dev)
        outs = (stats[0], stats[1], stats[2])
    L_ = _lib.lib()
    defer = accumulate and DEFER_REDUCE and _in_backward()
    if defer:             # the kernel leaves its partial sums in a buffer of their own, finished by the launch-boundary reduce
        nparts = L_.hriemo_add_ln_bwd_partial_rows(M, d)
        ws = torch.empty(nparts * 3 * d, dtype=torch.float32, device=dev)
        dests = (None, None, None, 0)
    else:
        ws = workspace(L_.hriemo_add_ln_bwd_workspace_bytes(M, d), dev, slot=1)
        dests = (_p(outs[0]), _p(outs[1]), _p(outs[2]), int(accumulate))
    _lib.call("hriemo_add_ln_bwd_rows", _p(dy), _p(g), _p(x), _p(x32), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dg), *dests, M, d,
              float(p), seed, _p(seed_word(dev)), site, row_off, _p(ws), _p(rows), _stream())
    if defer:
        _deferred.add(ws, 3 * d, nparts, d, 3 if outs[2] is not None else 2, [o for o in outs if o is not None], True)
    if dg is None:
        dg = dx           # no dropout: both branches get the same gradient
    return dx, dg, outs[0], outs[1], outs[2]


# The gate's row kernels: each picks the padded or the packed entry point itself from the layouts (Seq) of its buffers -- sx one
# modality's rows, sf the fused buffers' (An, Tn, H, dH); all padded or all packed.
def ln_pool_fwd(x, x32, sx, gamma, beta, Yn, mean, rstd, part, sf, d):
    """Yn = LayerNorm(x) on the rows the fused layout keeps, row statistics, per-chunk partial sums of the masked pooling"""
    if sf.packed:
        _lib.call("hriemo_ln_pool_fwd_packed", _p(x), _p(x32), _p(sx.cu), sx.B, sx.N, _p(gamma), _p(beta), _p(Yn), _p(mean), _p(rstd),
                  _p(part), sx.L, _p(sf.cu), sf.N, sx.Breal, d, _EPS, _stream())
    else:
        _lib.call("hriemo_ln_pool_fwd", _p(x), _p(x32), _p(sx.kpm), _p(gamma), _p(beta), _p(Yn), _p(mean), _p(rstd), _p(part),
                  sx.B, sx.L, sf.L, d, _EPS, _stream())


def ln_pool_fwd_pair(a, t, sf, d):
    """ln_pool_fwd of both modalities from one launch; a / t = (x, x32, sx, gamma, beta, Yn, mean, rstd, part) of each"""
    if sf.packed:
        side = lambda x, x32, sx, *rest: (_p(x), _p(x32), _p(sx.cu), sx.B, sx.N, *map(_p, rest), sx.L)          # noqa: E731
        _lib.call("hriemo_ln_pool_fwd_packed_pair", *side(*a), *side(*t), _p(sf.cu), sf.N, a[2].Breal, d, _EPS, _stream())
    else:
        side = lambda x, x32, sx, *rest: (_p(x), _p(x32), _p(sx.kpm), *map(_p, rest), sx.L)          # noqa: E731
        _lib.call("hriemo_ln_pool_fwd_pair", *side(*a), *side(*t), a[2].B, sf.L, d, _EPS, _stream())


def fuse_fwd(w, An, Tn, H, sf, d):
    """H = w * An + (1 - w) * Tn on the rows of the fused layout (the surplus rows of a packed one: zeros).  fp8 GEMM mode on the
    packed layout: the same launch leaves the MX-fp8 copy of H (the decoder's memory operand), tagged onto H (tag_mx)"""
    if sf.packed and want_mx_copy(sf.N, d):
        ld = _lib.lib().hriemo_mx8_scale_ld(sf.N)
        hq = torch.empty((sf.N, d), dtype=torch.uint8, device=H.device)
        hs = torch.empty((d // 32, ld), dtype=torch.uint8, device=H.device)
        _lib.call("hriemo_fuse_fwd_packed_q", _p(w), _p(An), _p(Tn), _p(H), _p(sf.cu), sf.N, sf.Breal, sf.L, d, _p(hq), _p(hs), ld,
                  _stream())
        tag_mx(H, (hq, hs))
    elif sf.packed:
        _lib.call("hriemo_fuse_fwd_packed", _p(w), _p(An), _p(Tn), _p(H), _p(sf.cu), sf.N, sf.Breal, sf.L, d, _stream())
    else:
        _lib.call("hriemo_fuse_fwd", _p(w), _p(An), _p(Tn), _p(H), sf.B, sf.L, d, _stream())


def fuse_bwd_dw(dH, An, Tn, part, sf, d):
    """per-chunk partial sums of dL/dw = sum over the fused rows of dH * (An - Tn)"""
    if sf.packed:
        _lib.call("hriemo_fuse_bwd_dw_packed", _p(dH), _p(An), _p(Tn), _p(part), _p(sf.cu), sf.N, sf.Breal, sf.L, d, _stream())
    else:
        _lib.call("hriemo_fuse_bwd_dw", _p(dH), _p(An), _p(Tn), _p(part), sf.B, sf.L, d, _stream())


def ln_pool_bwd(dH, sf, w, is_a, dpool, x, x32, sx, gamma, mean, rstd, dx, dgamma, dbeta, accumulate, ws, d):
    """backward of ln_pool_fwd and the fusion for one modality; dgamma / dbeta None: the partial sums stay in ws (deferred reduce)"""
    if sf.packed:
        _lib.call("hriemo_ln_pool_bwd_packed", _p(dH), _p(sf.cu), sf.N, _p(w), is_a, _p(dpool), _p(x), _p(x32), _p(sx.cu), sx.B, sx.N,
                  _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta), accumulate, sx.Breal, sx.L, d, _p(ws), _stream())
    else:
        _lib.call("hriemo_ln_pool_bwd", _p(dH), sf.L, _p(w), is_a, _p(dpool), _p(sx.kpm), _p(x), _p(x32), _p(gamma), _p(mean),
                  _p(rstd), _p(dx), _p(dgamma), _p(dbeta), accumulate, sx.B, sx.L, d, _p(ws), _stream())


def ln_pool_bwd_pair(dH, sf, w, a, t, accumulate, d):
    """ln_pool_bwd of both modalities from one launch; a / t = (ws, dpool, x, x32, sx, gamma, mean, rstd, dx, dgamma, dbeta)"""
    if sf.packed:
        side = lambda ws, dpool, x, x32, sx, *rest: (_p(dpool), _p(x), _p(x32), _p(sx.cu), sx.B, sx.N, *map(_p, rest), sx.L, _p(ws))  # noqa: E731
        _lib.call("hriemo_ln_pool_bwd_packed_pair", _p(dH), _p(sf.cu), sf.N, _p(w), *side(*a), *side(*t), accumulate, a[4].Breal, d, _stream())
    else:
        side = lambda ws, dpool, x, x32, sx, *rest: (_p(dpool), _p(sx.kpm), _p(x), _p(x32), *map(_p, rest), sx.L, _p(ws))  # noqa: E731
        _lib.call("hriemo_ln_pool_bwd_pair", _p(dH), sf.L, _p(w), *side(*a), *side(*t), accumulate, a[4].B, d, _stream())


TWIN = _os.environ.get("HRIEMO_FP32_TWIN", "1") != "0"      # carry the fp32 twin of the residual stream (LayerNorm outputs)


DEFER_REDUCE = True        # bias / LayerNorm column sums finished by ONE launch at the end of backward (_DeferredReduce)
FOLD_ATTN_BIAS = True      # in-proj bias grads from the attention backward kernels' own column sums


class _DeferredReduce:
    """Launch-boundary reduce (include/hriemo.h, hriemo_colreduce_batch): producers that accumulate straight into a
    parameter's .grad leave their per-block partial sums behind and ONE launch at the end of backward finishes all of
    them (85 five-microsecond launches per step otherwise).  The flush is an autograd-engine final callback: it runs
    on the caller's stream after the engine has joined every stream backward used."""

    def __init__(self):
        self.jobs, self.keep, self.scheduled, self.blocks, self.hooks = [], [], False, 0, []

    def _schedule(self):
        if not self.scheduled:
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)
            self.scheduled = True

    def add_hook(self, hook, p):
        self.hooks.append((hook, p))
        self._schedule()

    def add(self, part, pstride, np_, w, nseg, outs, accumulate, schedule=True):
        gx = (w + 31) // 32
        self.jobs.append([part.data_ptr(), pstride, np_, w, nseg | (int(bool(accumulate)) << 8) | (self.blocks << 32)]
                         + [o.data_ptr() for o in outs] + [0] * (3 - len(outs)))
        self.blocks += gx * nseg
        self.keep.append(part)
        self.keep.extend(outs)
        self.device = part.device
        if schedule:
            self._schedule()

    def flush(self):
        jobs, n, nblocks = self.jobs, len(self.jobs), self.blocks
        self.jobs, self.scheduled, self.blocks = [], False, 0
        if n:
            host = torch.tensor(jobs, dtype=torch.int64)
            dev = torch.empty((n, 8), dtype=torch.int64, device=self.device)
            _lib.call("hriemo_colreduce_batch", host.data_ptr(), n, _p(dev), nblocks, _stream())
            self.keep.append(dev)
        if not CTX.capturing and self.keep:     # a captured graph keeps using these buffers on every replay
            cur = torch.cuda.current_stream(self.device)
            for t in self.keep:     # partials of the text branch were allocated on the side stream
                t.record_stream(cur)
            self.keep = []
        hooks, self.hooks = self.hooks, []
        for hook, p in hooks:       # gradient-ready notifications held back until the values are final
            hook(p)


_deferred = _DeferredReduce()


# Deferred small weight-gradient GEMMs.  The decoder's and the gate's backward is a serial chain of latency-bound launches that
# runs before the encoder's backward starts; its 16 weight-gradient GEMMs (M = B*N_e = 384 or B rows of reduction) sit on that
# chain at ~20 us each although nothing downstream needs them.  When they accumulate straight into .grad (fused path) they are
# queued instead and issued in one go where the device has room: behind the LAST text-branch Function of backward (layer-0 text
# self-attention, on the side stream, while the audio branch still has ~0.5 ms of its own backward to run), or from an
# autograd-engine final callback if no such point comes.  Measured at cfg 2: 8.87 -> 8.7 ms per step (skipping them altogether:
# 8.65).  Off while gradient-ready hooks drive an overlapped exchange (the decoder's bucket would leave last instead of first);
# round 4: the same sites' bias-gradient column sums (five 5-7 us launches on the chain) are queued with them.
GATE_TWO_STREAMS = True    # the gate's text-side LayerNorm + pooling on the side stream
GATE_PAIR = True           # ... superseded for d <= 1024: both modalities' LayerNorm + pooling (forward and backward) from ONE launch
DEFER_SMALL_DW = True
GROUP_SMALL_DW = True      # the queued weight gradients leave as one grouped GEMM launch
SMALL_DW_ROWS = 1024
FLUSH_SITES = set()                # dropout-site ids of the sub-layers whose backward ends a model's text branch (one per CrossModalTransformer)
FORCE_INPUT_GRAD = False           # tests: SelfAttnLN.backward computes its input gradient even where autograd does not ask for it
_hook_predicates = []              # one per live dp.GradBuckets with gradient-ready hooks (register_hook_predicate)


def register_hook_predicate(fn):
    """dp.GradBuckets: `fn()` is True while its gradient-ready hooks drive an overlapped exchange"""
    _hook_predicates.append(fn)
    return fn


def unregister_hook_predicate(fn):
    if fn in _hook_predicates:
        _hook_predicates.remove(fn)


def grad_hooks_active():
    return any(f() for f in _hook_predicates)


class _DeferredWgrad:
    def __init__(self):
        self.jobs, self.hooks, self.keep, self.scheduled = [], [], [], False
        self.flushing = self.in_final = False

    def enabled(self):
        return DEFER_SMALL_DW and _in_backward() and not grad_hooks_active()

    def add(self, dy, x, out):
        self.jobs.append((dy, x, out))
        if not self.scheduled:
            torch.autograd.Variable._execution_engine.queue_callback(self.final)
            self.scheduled = True

    def add_hook(self, hook, p, column_sum=False):
        self.hooks.append((hook, p, column_sum))

    def touches(self, g):
        if not self.jobs or g is None:
            return False
        a = g.data_ptr()
        b = a + g.numel() * g.element_size()
        return any(a <= j[2].data_ptr() < b for j in self.jobs)

    def flush(self):
        alljobs, self.jobs = self.jobs, []
        sums = [j for j in alljobs if j[1] is None]          # queued column sums (x is None): (dy, None, out)
        jobs = [j for j in alljobs if j[1] is not None]
        if sums:
            cur = torch.cuda.current_stream(sums[0][0].device)
            self.flushing = True
            try:
                for dy, _, out in sums:
                    colsum(dy, out, True)
                    if CTX.capturing:
                        self.keep.extend((dy, out))
                    else:
                        dy.record_stream(cur); out.record_stream(cur)
            finally:
                self.flushing = False
        if jobs:
            cur = torch.cuda.current_stream(jobs[0][0].device)
            grouped = GROUP_SMALL_DW and all(dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0 for dy, x, _ in jobs)
            if grouped:
                # ONE launch per 16 queued weight gradients (hriemo_gemm_bf16_group_tn) instead of one ~20 us launch each
                table = [(dy.shape[1], x.shape[1], dy.shape[0], dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), out.data_ptr(),
                          out.stride(0)) for dy, x, out in jobs]
                host = torch.tensor(table, dtype=torch.int64)
                _lib.call("hriemo_gemm_bf16_group_tn", host.data_ptr(), len(table), 1, _stream())
            for dy, x, out in jobs:
                M, N = dy.shape
                if not grouped:
                    gemm(1, 1, N, x.shape[1], M, dy, dy.stride(0), x, x.stride(0), out, out.stride(0), c_f32=True, accumulate=True)
                if CTX.capturing:
                    self.keep.extend((dy, x, out))      # a captured graph keeps reading these buffers on every replay
                else:
                    dy.record_stream(cur); x.record_stream(cur); out.record_stream(cur)
        hooks, self.hooks = self.hooks, []
        for hook, p, column_sum in hooks:
            if column_sum and DEFER_REDUCE and not self.in_final and _in_backward():
                _deferred.add_hook(hook, p)          # the column sum just issued is finished by the launch-boundary reduce
            else:
                hook(p)

    def final(self):
        self.scheduled = False
        self.in_final = True             # engine final callback: column sums finish in their own call, nothing is queued any more
        try:
            self.flush()
        finally:
            self.in_final = False


_small_dw = _DeferredWgrad()


def as_pair(x):
    """(bf16 copy for the GEMMs, fp32 twin for the residual path or None)"""
    if x.dtype == BF16:
        return x, None
    return x.to(BF16), (x if x.dtype == torch.float32 else x.float()) if TWIN else None


def from_pair(y16, y32, dtype):
    if dtype == BF16:
        return y16
    return (y32 if y32 is not None else y16).to(dtype)


def _sum_grads(d16, d32):
    """total upstream gradient of a (bf16, fp32-twin) output pair, as bf16"""
    if d32 is None:
        return d16
    if d16 is None:
        return d32.to(BF16)
    return (d16.float() + d32).to(BF16)


def _c32(t):
    return None if t is None else (t if t.is_contiguous() else t.contiguous())


def _heads(d, H):
    if d % H != 0:
        raise ValueError(f"d_model={d} not divisible by n_heads={H}")
    hd = d // H
    if hd not in (16, 32, 64, 96, 128):
        raise ValueError(f"head_dim={hd} is not built (supported: 16, 32, 64, 96, 128)")
    return hd


def _contig_bf16(t):
    t = to_bf16(t)
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------- packed (varlen) sequences, SURVEY 8(f) rank 4
# The reference pads every sample to the batch maximum and computes the PAD rows too (train_fusion_seq_level_decoder.py:191-232).
# Opt-in (HRIEMO_VARLEN=1 / set_varlen(True)): the cross-modal encoder -- 9/10 of the FLOPs -- runs on the VALID rows only: the
# row-wise kernels (GEMM, LayerNorm, FFN) see [N_valid, d] matrices, the attention kernels take cu_seqlens
# (hriemo_attn_*_varlen); the rows are scattered back to the padded layout before the gate, whose pooling, fusion and the
# decoder's masks only ever read valid positions -- so logits, beta and z are those of the padded path.  The packing needs the
# lengths on the host (one sync per distinct mask tensor); a step captured into a hipGraph bakes them in and may only be
# replayed with the same masks (dp.DataParallelStep checks).
VARLEN = None


def set_varlen(on):
    global VARLEN
    VARLEN = bool(on)


def varlen():
    global VARLEN
    if VARLEN is None:
        VARLEN = _os.environ.get("HRIEMO_VARLEN", "0") == "1"
    return VARLEN


# The tail of the model on packed rows: with the encoder packed, the gate reads its packed output and hands the decoder a packed
# fused memory (BetaGateFn on packed layouts, hriemo_*_packed), so no unpack / pack launch runs behind the encoder.  False: the encoder's output
# is scattered back to the padded layout in front of the gate (exactly the launches from before the packed tail) -- the A/B handle.
# Opt-in until the step has been measured against the False arm (scripts_dev/ab_packed_tail.sh).
PACKED_TAIL = False
# The same for the fp32 precision mode (_fp32.beta_gate with a plan, hriemo_*_f32_packed): a switch of its own, because PACKED_TAIL
# alone must keep meaning "the bf16 tail" (with only PACKED_TAIL set, the fp32 mode issues exactly its previous launches) and
# because each arm becomes the default only after its own measurement (scripts_dev/ab_packed_tail.sh fp32).
PACKED_TAIL_FP32 = False
# And for the MX-fp8 GEMM mode (bf16 precision): the gate's fuse kernel leaves the quantised memory (hriemo_fuse_fwd_packed_q), the
# decoder's K | V projections run in fp8 over the N_f packed rows.  Its own switch for the same two reasons
# (scripts_dev/ab_packed_tail.sh mx8).
PACKED_TAIL_MX8 = False


# Attention maps (return_attention=True) from the packed path: the export runs on cu_seqlens (hriemo_attn_probs_varlen,
# hriemo_attn_probs_f32_varlen) and hands back the padded maps, so asking for the maps no longer sends the forward to the padded
# layout.  False: the maps are exported by the padded path only (the launches from before the packed export).  Opt-in; a module
# constant with a setter, not an environment switch.
PACKED_MAPS = False


def set_varlen_maps(on):
    global PACKED_MAPS
    PACKED_MAPS = bool(on)


def varlen_maps():
    return bool(PACKED_MAPS)


# Attention maps of PADDED rows from the matrix cores: attn_probs picks hriemo_attn_probs_mfma (the contract of hriemo_attn_probs
# under any key-padding mask: PAD query rows computed, PAD key columns exact zeros, an all-PAD sample NaN; the result is equal up
# to fp32 summation order) wherever it would launch the VALU export -- every encoder site, the decoder's padded maps (those of
# varlen + packed maps with the packed tail off included), the legacy block, the classifier's transformer.  False: exactly the
# launches from before.  The fp32 precision is unaffected: _fp32.probs already runs an fp32 MFMA loop.  Opt-in; a module constant
# with a setter, not an environment switch.
MFMA_MAPS = False


def set_mfma_maps(on):
    global MFMA_MAPS
    MFMA_MAPS = bool(on)


def mfma_maps():
    return bool(MFMA_MAPS)


def packed_tail():
    """the tail stays packed: the switch of the mode in force -- PACKED_TAIL for bf16 operands in bf16 precision, PACKED_TAIL_FP32
    for the fp32 precision (bf16 GEMM mode), PACKED_TAIL_MX8 for MX-fp8 operands in bf16 precision"""
    if gemm_mode() == "mx_fp8":
        return bool(PACKED_TAIL_MX8 and precision() == "bf16")
    return bool(PACKED_TAIL_FP32) if precision() == "fp32" else bool(PACKED_TAIL and precision() == "bf16")


class Seq:
    """How the rows of one activation buffer are laid out -- the ONE value every Function and kernel wrapper takes for it.
    Padded (Seq.padded): the buffer is [B, L, d], cu and idx are None, N = B * L, kpm is the uint8 key-padding mask [B, L] or None.
    Packed: the buffer is [1, N, d]; cu int32 [B+1] (device), idx int64 [N] packed row -> row of the padded [Breal*L] layout, kpm
    None (the lengths are in cu; only the copies the gate gets carry the masks, with_kpm).
    Bucketed form (seq_bucket, one captured graph for every batch): N = the bucket's row count, the rows beyond the last real
    sequence form ONE extra sequence (B = Breal + 1, cu has B+1 entries) of zeros, so every kernel writes every row.
    surplus: rows behind the last sequence that belong to NO sequence of the plan (the fused memory of a bucket, seq_bucket_fused):
    the attention kernels never see them, the kernels that write such a buffer write them as zeros.
    idx None: the rows are the padded rows themselves (the decoder's queries, query_seq)."""
    __slots__ = ("cu", "idx", "B", "L", "Lmax", "N", "Breal", "surplus", "kpm")

    def __init__(self, cu, idx, B, L, Lmax, N, Breal=None, surplus=False, kpm=None):
        self.cu, self.idx, self.B, self.L, self.Lmax, self.N = cu, idx, B, L, Lmax, N
        self.Breal = B if Breal is None else Breal
        self.surplus = bool(surplus)
        self.kpm = kpm

    @classmethod
    def padded(cls, B, L, mask=None):
        """the padded layout [B, L] with its key-padding mask (bool or uint8 [B, L], True = PAD; a bool mask is viewed, not copied)"""
        return cls(None, None, B, L, L, B * L, kpm=mask_u8(mask, B, L))

    @property
    def packed(self):
        return self.cu is not None

    def shape(self, d):          # of a buffer of these rows
        return (1, self.N, d) if self.packed else (self.Breal, self.L, d)

    def holds(self, x):          # x [., ., d] is a buffer of these rows, or the kernels would be handed row counts that are not x's
        if x.shape[0] * x.shape[1] != self.N:
            raise ValueError(f"activation of shape {tuple(x.shape)} does not have the {self.N} rows of its layout")

    def with_kpm(self, mask):
        """this layout with the padded [Breal, L] mask riding along: the gate reads its valid counts from the masks in either form"""
        return Seq(self.cu, self.idx, self.B, self.L, self.Lmax, self.N, self.Breal, self.surplus, mask_u8(mask, self.Breal, self.L))

    def record_stream(self, stream):
        for t in (self.cu, self.idx, self.kpm):
            if t is not None:
                t.record_stream(stream)


# What two layouts mean to an attention sub-layer (attn_rows): B sequences of up to Lq / Lk rows with the keys' uint8 mask kpm (padded)
# or cu = (cu_seqlens_q, cu_seqlens_k) (packed); the LayerNorm dropout is keyed by `stride` rows per padded sample and by `rows`, the
# padded row of every packed query row (None: the rows are the padded ones); kv_surplus: key rows of no sequence, whose dK | dV the
# attention backward leaves unwritten.
AttnRows = namedtuple("AttnRows", "B Lq Lk kpm cu stride rows kv_surplus")


def attn_rows(seq_q, seq_k, need_w):
    """AttnRows of a sub-layer whose queries are laid out as seq_q and whose keys as seq_k (the same Seq for a self-attention).
    Packed: the attention sees Seq.B sequences of up to Seq.Lmax rows, the LayerNorm dropout stays keyed by the padded rows.
    need_w on packed rows: only with the packed export switched on (set_varlen_maps) and a plan without a filler sequence -- or a
    LogSite, whose launch covers the plan's real samples only (LogSite.B)."""
    if not (seq_q.packed or seq_k.packed):
        return AttnRows(seq_q.B, seq_q.L, seq_k.L, seq_k.kpm, None, seq_q.L, None, False)
    if isinstance(need_w, LogSite):
        if not varlen_maps():
            raise ValueError("attention maps are exported by the padded path only")
        if need_w.B > min(seq_q.Breal, seq_k.Breal):
            raise ValueError(f"attention log: a pass of {need_w.B} samples, but the plan holds {min(seq_q.Breal, seq_k.Breal)}")
    elif need_w and not (varlen_maps() and seq_q.B == seq_q.Breal and seq_k.B == seq_k.Breal):
        # (with the packed export on, a bucketed plan is still refused: its filler sequence has no sample to export)
        raise ValueError("attention maps are exported by the padded path only")
    if not (seq_q.packed and seq_k.packed) or seq_q.kpm is not None or seq_k.kpm is not None:
        raise ValueError("attn_fwd: packed sequences carry their lengths; no key_padding_mask")
    return AttnRows(seq_q.B, seq_q.Lmax, seq_k.Lmax, None, (seq_q.cu, seq_k.cu), seq_q.L, seq_q.idx, seq_k.surplus)


def seq_bucket(cu, B, L, n_rows):
    """Seq over `n_rows` packed rows whose lengths live in DEVICE memory: cu int32 [B+2] = [0, cumulative valid lengths of the B
    sequences ..., n_rows] (the caller refreshes it per batch; cu[B] < n_rows, n_rows - cu[B] <= L).  Nothing here depends on
    the lengths, so a step captured with it replays for every batch that fits the bucket."""
    idx = torch.empty(n_rows, dtype=torch.int64, device=cu.device)      # written by the first pack of the step (hriemo_pack_rows)
    return Seq(cu, idx, B + 1, L, L, n_rows, Breal=B)


def seq_bucket_fused(cu_f, B, L, n_rows):
    """Seq of the fused memory (sample b: min(audio length, text length) rows) over `n_rows` packed rows, lengths in DEVICE memory:
    cu_f int32 [B+2] = [0, cumulative fused lengths ..., n_rows].  n_rows is the text bucket's row count (sum of the fused lengths
    <= sum of the text lengths), so the fused plan adds no bucket dimension.  The rows behind cu_f[B] are surplus, not a sequence:
    the decoder's attention runs the B real sequences only."""
    return Seq(cu_f, None, B, L, L, n_rows, surplus=True)


_QUERY_SEQS = {}


def query_seq(B, n, device):
    """the trivial Seq of the decoder's queries: n rows for every sample, the packed rows are the padded rows (idx None)"""
    key = (B, n, str(device))
    s = _QUERY_SEQS.get(key)
    if s is None:
        s = _QUERY_SEQS[key] = Seq(torch.arange(B + 1, dtype=torch.int32, device=device) * n, None, B, n, n, B * n)
    return s


_FUSED_PLANS = {}


def fused_seq(sa, st):
    """Seq of the fused memory for the plans of two prefix masks (seq_plan): lf[b] = min(la[b], lt[b]) -- the reference ORs the two
    masks cut to L_t (models/fusion_with_emotion_decoder.py:62-79), both are prefix masks, and lf >= 1 because seq_plan refuses
    empty sequences.  One device -> host read per distinct pair of plans."""
    key = (id(sa), id(st))
    hit = _FUSED_PLANS.get(key)
    if hit is not None:
        return hit[0]
    if CTX.capturing:
        raise RuntimeError("varlen: the sequence lengths must be known before the step is captured (run one eager step first)")
    B = sa.Breal
    la, lt = sa.cu[1:B + 1] - sa.cu[:B], st.cu[1:B + 1] - st.cu[:B]
    lf = torch.minimum(la, lt)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=lf.device)
    cu[1:] = torch.cumsum(lf, 0)
    L = min(sa.L, st.L)
    # Lmax = the padded fused length, not the longest sample: the decoder's attention launches then pick the kernel variant of the
    # padded call, whatever the batch's lengths (its grid is N_e query rows per sample either way)
    sf = Seq(cu, None, B, L, L, int(lf.sum()))
    if len(_FUSED_PLANS) > 64:
        _FUSED_PLANS.clear()
    _FUSED_PLANS[key] = (sf, sa, st)          # the plans stay referenced: their ids are the key
    return sf


_SEQ_PLANS = {}


def seq_plan(mask, B, L):
    """Seq for a [B, L] padding mask (True = PAD) whose valid positions are a prefix of every row with at least one valid
    position (what the collate produces); None when the mask does not have that form (the padded path then runs)."""
    if mask is None:
        return None
    key = (mask.data_ptr(), tuple(mask.shape), mask._version, str(mask.device))
    hit = _SEQ_PLANS.get(key)
    if hit is not None:
        return hit[0]
    if CTX.capturing:
        raise RuntimeError("varlen: the sequence lengths must be known before the step is captured (run one eager step first)")
    valid = ~mask.bool()
    lens = valid.sum(1)
    prefix = bool((valid == (torch.arange(L, device=mask.device)[None, :] < lens[:, None])).all()) and bool((lens > 0).all())
    plan = None
    if prefix:
        cu = torch.zeros(B + 1, dtype=torch.int32, device=mask.device)
        cu[1:] = torch.cumsum(lens, 0)
        idx = valid.reshape(-1).nonzero().reshape(-1)
        plan = Seq(cu, idx, B, L, int(lens.max()), int(idx.numel()))
    if len(_SEQ_PLANS) > 64:
        _SEQ_PLANS.clear()
    _SEQ_PLANS[key] = (plan, mask)            # the mask stays referenced: its address is the key
    return plan


def seq_plans(mask_a, mask_t, B, La, Lt):
    """(Seq audio, Seq text, Seq fused) for the two padding masks of a batch, or None when either is not a prefix mask"""
    sa, st = seq_plan(mask_a, B, La), seq_plan(mask_t, B, Lt)
    if sa is None or st is None:
        return None
    return sa, st, fused_seq(sa, st)


def _pack_pair(x16, x32, seq, d, idx):
    """padded [Breal, L, d] pair (either member may be None) -> packed [1, N, d] pair: ONE gather launch, bucket padding rows written
    as zeros; idx: the tensor that receives the padded row of every packed row (seq.idx), or None"""
    dev = (x16 if x16 is not None else x32).device
    p16 = torch.empty((1, seq.N, d), dtype=BF16, device=dev) if x16 is not None else None
    p32 = torch.empty((1, seq.N, d), dtype=torch.float32, device=dev) if x32 is not None else None
    x16c = None if x16 is None else _contig_bf16(x16)
    _lib.call("hriemo_pack_rows", _p(x16c), _p(_c32(x32)), _p(seq.cu), seq.Breal, seq.L, d, seq.N, _p(p16), _p(p32), _p(idx), _stream())
    return p16, p32


class PackFn(torch.autograd.Function):
    """(x16 [B, L, d], x32 | None) -> packed ([1, N, d], twin | None): ONE gather launch for the pair (hriemo_pack_rows), bucket
    padding rows written as zeros; also fills seq.idx (padded row of every packed row)."""

    @staticmethod
    def forward(ctx, x16, x32, seq):
        ctx.set_materialize_grads(False)
        d = x16.shape[2]
        if tuple(x16.shape[:2]) != (seq.Breal, seq.L):
            raise ValueError(f"pack: activation of shape {tuple(x16.shape)} is not the padded [{seq.Breal}, {seq.L}] layout of its plan")
        ctx.seq, ctx.d, ctx.has32 = seq, d, x32 is not None
        return _pack_pair(x16, x32, seq, d, seq.idx)

    @staticmethod
    def backward(ctx, d16, d32):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) or (d16 is None and d32 is None):
            return None, None, None
        y16, y32 = _unpack_pair(d16, d32, ctx.seq, ctx.d)
        return y16, (y32 if ctx.has32 else None), None


def _unpack_pair(p16, p32, seq, d):
    dev = (p16 if p16 is not None else p32).device
    y16 = torch.empty((seq.Breal, seq.L, d), dtype=BF16, device=dev) if p16 is not None else None
    y32 = torch.empty((seq.Breal, seq.L, d), dtype=torch.float32, device=dev) if p32 is not None else None
    p16c = None if p16 is None else _contig_bf16(p16)
    _lib.call("hriemo_unpack_rows", _p(p16c), _p(_c32(p32)), _p(seq.cu), seq.Breal, seq.L, d, _p(y16), _p(y32), _stream())
    return y16, y32


class UnpackFn(torch.autograd.Function):
    """packed ([1, N, d], twin | None) -> padded ([B, L, d], twin | None) with zeros at the PAD positions: one scatter launch
    (hriemo_unpack_rows); backward = the gather of the pair's gradients (bucket padding rows get zeros)."""

    @staticmethod
    def forward(ctx, p16, p32, seq):
        ctx.set_materialize_grads(False)
        d = p16.shape[-1]
        ctx.seq, ctx.d = seq, d
        return _unpack_pair(p16, p32, seq, d)

    @staticmethod
    def backward(ctx, d16, d32):
        if d16 is None and d32 is None:
            return None, None, None
        return _pack_pair(d16, d32, ctx.seq, ctx.d, None) + (None,)


def pack_rows(x, seq):
    """[B, L, d] -> [1, N, d] by torch indexing: what PackFn computes, stated on seq.idx (host-logic tests; the model calls pack_pair)"""
    if x is None:
        return None
    B, L, d = x.shape
    return x.reshape(B * L, d).index_select(0, seq.idx).view(1, seq.N, d)


def unpack_rows(x, seq):
    """[1, N, d] -> [B, L, d] with zeros at the PAD positions by torch indexing (see pack_rows)"""
    if x is None:
        return None
    d = x.shape[-1]
    out = torch.zeros((seq.B * seq.L, d), dtype=x.dtype, device=x.device)
    return out.index_copy(0, seq.idx, x.reshape(seq.N, d)).view(seq.B, seq.L, d)


def pack_pair(x16, x32, seq):
    """[B, L, d] pair -> packed [1, N, d] pair (valid rows only)"""
    return PackFn.apply(x16, x32, seq)


def unpack_pair(p16, p32, seq):
    """packed [1, N, d] pair -> [B, L, d] pair with zeros at the PAD positions"""
    return UnpackFn.apply(p16, p32, seq)


# ----------------------------------------------------------------------------- module inputs in one launch (hriemo_ingest_rows)
# The front door of every model: the caller's tensor (fp32 / bf16 / fp16) -> the (bf16, fp32-twin) pair the first encoder layer
# reads, gathered straight into the packed rows where the encoder packs, with seq.idx and -- in MX-fp8 mode -- the quantised copy
# of the rows from the same launch.  Replaces as_pair's torch casts + hriemo_pack_rows (+ the first layer's hriemo_quant_mx8): PAD
# rows are neither read nor converted.  Opt-in (set_ingest) until the step has been measured against the launches it replaces
# (scripts_dev/bench_ingest.py); forward_packed (rows that arrive packed) uses the kernel regardless.
INGEST_ROWS = False
_XT = {torch.float32: 0, BF16: 1, torch.float16: 2}       # x_dtype of hriemo_ingest_rows


def set_ingest(on):
    global INGEST_ROWS
    INGEST_ROWS = bool(on)


def ingest():
    return bool(INGEST_ROWS)


def ingestible(*xs):
    """the module entries take these tensors through hriemo_ingest_rows (switch on, a source dtype the kernel converts)"""
    return bool(INGEST_ROWS) and all(x.dtype in _XT for x in xs)


def _ingest_rows(x, seq, src_packed, want16=True, want32=False):
    """x: the padded [Breal, L, d] tensor, or (src_packed) the packed [rows, d] one -> (bf16 rows | None, fp32 twin | None, MX-fp8
    copy (bytes, scales) | None -- made when want_mx_copy(seq.N, d)) in the layout of `seq` ([1, N, d] packed: fills seq.idx,
    surplus rows zero; a padded Seq: [Breal, L, d], the rows stay where they are)."""
    _require_gpu(x)
    d = x.shape[-1]
    if not (x.is_contiguous() and x.data_ptr() % 16 == 0):
        x = x.contiguous()
    N, shape = seq.N, seq.shape(d)
    p16 = torch.empty(shape, dtype=BF16, device=x.device) if want16 else None
    p32 = torch.empty(shape, dtype=torch.float32, device=x.device) if want32 else None
    q = sc = None
    ld = 0
    if want_mx_copy(N, d):
        ld = _lib.lib().hriemo_mx8_scale_ld(N)
        q = torch.empty((N, d), dtype=torch.uint8, device=x.device)
        sc = torch.empty((d // 32, ld), dtype=torch.uint8, device=x.device)
    _lib.call("hriemo_ingest_rows", _p(x), _XT[x.dtype], d, _p(seq.cu), int(bool(src_packed)), seq.Breal, seq.L, d, N, _p(p16), _p(p32),
              _p(q), _p(sc), ld, _p(seq.idx), _stream())
    return p16, p32, ((q, sc) if q is not None else None)


class IngestFn(torch.autograd.Function):
    """x (fp32 / bf16 / fp16) -> the (bf16, fp32 twin | None) pair of its rows laid out as `seq`: ONE launch (hriemo_ingest_rows).
    seq packed: x is the padded [Breal, L, d] tensor (gathered; what as_pair + PackFn give) or, src_packed, the valid rows
    [N, d] back to back; also fills seq.idx.  seq padded: x [B, L, d] keeps its layout (what as_pair gives).  The twin is None
    where as_pair's is (bf16 sources, HRIEMO_FP32_TWIN=0); in MX-fp8 mode the quantised copy rides on the bf16 member (tag_mx).
    Backward: the pair's gradients scattered back to x's layout (hriemo_unpack_rows for a gathered source), each cast to x's
    dtype and summed there -- what autograd computes for as_pair + PackFn."""

    @staticmethod
    def forward(ctx, x, seq, src_packed=False):
        ctx.set_materialize_grads(False)
        if x.dtype not in _XT:
            raise TypeError(f"ingest: inputs of dtype {x.dtype} (expected float32, bfloat16 or float16)")
        d = x.shape[-1]
        if src_packed:
            if not seq.packed or x.dim() != 2 or (seq.B == seq.Breal and x.shape[0] != seq.N):
                raise ValueError(f"ingest: packed rows of shape {tuple(x.shape)} do not match the {seq.N} rows of their plan")
        elif x.dim() != 3 or tuple(x.shape[:2]) != (seq.Breal, seq.L):
            raise ValueError(f"ingest: activation of shape {tuple(x.shape)} is not the padded [{seq.Breal}, {seq.L}] layout of its plan")
        ctx.seq, ctx.src_packed, ctx.shape, ctx.dtype = seq, bool(src_packed), tuple(x.shape), x.dtype
        p16, p32, mx = _ingest_rows(x, seq, src_packed, want32=TWIN and x.dtype != BF16)
        return tag_mx(p16, mx), p32

    @staticmethod
    def backward(ctx, d16, d32):
        if not ctx.needs_input_grad[0] or (d16 is None and d32 is None):
            return None, None, None
        seq, d = ctx.seq, ctx.shape[-1]
        if seq.packed and not ctx.src_packed:
            d16, d32 = _unpack_pair(d16, d32, seq, d)
        g = None
        for y in (d16, d32):
            if y is not None:
                y = y.reshape(-1, d)[:ctx.shape[0]] if ctx.src_packed else y
                y = y.to(ctx.dtype)
                g = y if g is None else g + y
        return g.reshape(ctx.shape), None, None


def ingest_pair(x, seq, src_packed=False):
    """IngestFn; a bf16 tensor that keeps its padded layout is its own pair (as_pair): no launch unless the MX-fp8 copy is wanted,
    which then rides on a fresh view of x"""
    if x.dtype == BF16 and not seq.packed:
        if not want_mx_copy(seq.N, x.shape[-1]):
            return x, None
        return tag_mx(x.view(x.shape), _ingest_rows(x.detach(), seq, False, want16=False)[2]), None
    return IngestFn.apply(x, seq, src_packed)


def entry_pair(x):
    """as_pair at a module entry that keeps the padded layout; with INGEST_ROWS on, its one-launch form"""
    if x.dim() != 3 or not ingestible(x):
        return as_pair(x)
    return ingest_pair(x, Seq.padded(x.shape[0], x.shape[1]))


def packed_lengths(rows_a, rows_t, lengths_a, lengths_t, pad_to=None, same_width=True):
    """Argument check of forward_packed, on the host only: -> (audio lengths, text lengths) as Python lists and (L_a, L_t).
    ValueError for lengths outside [1, L], rows that do not add up to the lengths or tensors of the wrong form; RuntimeError for
    L_t > L_a (the reference's gate slices h_a[:, :L_t], beta_gate_tacfn.py:98-112).  same_width False: the two modalities may differ
    in width (the MOSEI wrapper, in front of its projections)."""
    la, lt = ([int(v) for v in (l.tolist() if isinstance(l, torch.Tensor) else l)] for l in (lengths_a, lengths_t))
    for l in (lengths_a, lengths_t):
        if isinstance(l, torch.Tensor) and l.is_cuda:
            raise ValueError("forward_packed: lengths are host sequences or CPU int tensors (no device read)")
    if len(la) == 0 or len(la) != len(lt):
        raise ValueError(f"forward_packed: {len(la)} audio and {len(lt)} text lengths")
    La, Lt = (max(la), max(lt)) if pad_to is None else (int(pad_to[0]), int(pad_to[1]))
    for name, ls, L in (("audio", la, La), ("text", lt, Lt)):
        bad = [v for v in ls if v < 1 or v > L]
        if bad:
            raise ValueError(f"forward_packed: {name} length {bad[0]} outside [1, {L}]")
    for name, rows, ls in (("rows_a", rows_a, la), ("rows_t", rows_t, lt)):
        if rows.dim() != 2 or rows.shape[0] != sum(ls):
            raise ValueError(f"forward_packed: {name} of shape {tuple(rows.shape)} is not [sum(lengths) = {sum(ls)}, d]")
        if rows.dtype not in _XT:
            raise ValueError(f"forward_packed: {name} of dtype {rows.dtype} (expected float32, bfloat16 or float16)")
    if (same_width and rows_a.shape[1] != rows_t.shape[1]) or rows_a.dtype != rows_t.dtype or rows_a.device != rows_t.device:
        raise ValueError("forward_packed: rows_a and rows_t differ in width, dtype or device")
    if Lt > La:
        raise RuntimeError(f"forward_packed: L_t={Lt} > L_a={La}: the gate fuses over the text length and needs L_a >= L_t")
    return la, lt, (La, Lt)


_LENGTH_PLANS = {}


def plans_from_lengths(la, lt, La, Lt, device):
    """(Seq audio, Seq text, Seq fused) and the padded bool masks (True = PAD) [B, La], [B, Lt] of a batch given by its lengths (host
    lists): what seq_plans makes of the masks, without a device -> host read.  idx of the two modality plans is written by the
    ingest launch (hriemo_ingest_rows' row_index)."""
    key = (tuple(la), tuple(lt), La, Lt, str(device))
    hit = _LENGTH_PLANS.get(key)
    if hit is not None:
        return hit
    B = len(la)

    def plan(ls, L, Lmax, with_idx):
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(torch.tensor(ls, dtype=torch.int64), 0)
        n = int(cu[B])
        return Seq(cu.to(device), torch.empty(n, dtype=torch.int64, device=device) if with_idx else None, B, L, Lmax, n)

    lf = [min(x, y) for x, y in zip(la, lt)]
    Lf = min(La, Lt)
    plans = (plan(la, La, max(la), True), plan(lt, Lt, max(lt), True), plan(lf, Lf, Lf, False))     # (fused: Lmax as fused_seq)
    masks = tuple((torch.arange(L)[None, :] >= torch.tensor(ls)[:, None]).to(device) for ls, L in ((la, La), (lt, Lt)))
    if len(_LENGTH_PLANS) > 64:
        _LENGTH_PLANS.clear()
    _LENGTH_PLANS[key] = (plans, masks)
    return plans, masks


def seq_tables(lens, La, Lt, rows=(0, 0), cu=(None, None, None), masks=(None, None, None)):
    """The tables of a ragged batch from its lengths in DEVICE memory, ONE launch (hriemo_seq_tables): lens int32 [2, B] (audio row,
    text row; already checked on the host, packed_lengths) -> cu = (cu_a, cu_t, cu_f) int32 [B+2] each, closed by the bucket row
    counts rows = (audio, text), and masks = (mask_a [B, La], mask_t [B, Lt], mask_f [B, Lt]) uint8, 1 = PAD.  Every output is
    optional; the ones given are overwritten in place, so a captured step that starts with this launch follows the lengths."""
    _require_gpu(lens)
    B = lens.shape[1]
    if lens.dtype != torch.int32 or lens.dim() != 2 or lens.shape[0] != 2 or not lens.is_contiguous():
        raise ValueError(f"seq_tables: lengths of shape {tuple(lens.shape)} / {lens.dtype} (expected contiguous int32 [2, B])")
    for t, n, size in zip(tuple(cu) + tuple(masks), (B + 2,) * 3 + (B * La, B * Lt, B * Lt), (4,) * 3 + (1,) * 3):
        if t is not None and not (t.is_contiguous() and t.numel() == n and t.element_size() == size):
            raise ValueError(f"seq_tables: an output of shape {tuple(t.shape)} / {t.dtype} does not hold its {n} elements")
    _lib.call("hriemo_seq_tables", _p(lens[0]), _p(lens[1]), B, int(La), int(Lt), int(rows[0]), int(rows[1]), _p(cu[0]), _p(cu[1]), _p(cu[2]),
              _p(masks[0]), _p(masks[1]), _p(masks[2]), _stream())


# ----------------------------------------------------------------------------- sub-layer Functions
class _GradModeAware:
    """Function.forward always runs with grad mode off, and ctx.needs_input_grad mirrors the inputs' requires_grad even under
    torch.no_grad(): a forward that must know whether autograd is RECORDING this call (the fp32 mode saves its activations
    only then) reads the grad mode noted here at apply() time (thread-local)."""

    @classmethod
    def apply(cls, *args, **kwargs):
        prev = getattr(_apply_tls, "grad_mode", None)
        _apply_tls.grad_mode = torch.is_grad_enabled()
        try:
            return super().apply(*args, **kwargs)
        finally:
            _apply_tls.grad_mode = prev


def recording(ctx):
    """autograd will call this node's backward"""
    return bool(getattr(_apply_tls, "grad_mode", True)) and any(ctx.needs_input_grad)


def _proj_ln(a, sh, w, w16, b, x2, x32v, gamma, beta, p, seed, site, row_off, rows):
    """the tail of every sub-layer: g = a . W^T + b, y = LN(x + drop(g)) -> (g, y, y32, mean, rstd, MX-fp8 copy of y | None)"""
    M, d = x2.shape
    if fuse_ln(M, d):
        return proj_add_ln_fwd(a, w16, b, x2, x32v, gamma, beta, p, seed, site, row_off, TWIN, rows) + (None,)
    g = proj_fwd(Operand(a, mx_of(a)), sh, w, w16, b)
    y, y32, mean, rstd, *mx = add_ln_fwd(g, x2, gamma, beta, p, seed, site, row_off, x32=x32v, want32=TWIN, want_mx=want_mx_copy(M, d),
                                         rows=rows)
    return g, y, y32, mean, rstd, (mx[0] if mx else None)


def _attn_ln_fwd(ctx, head, q, k, v, x2, x32v, ar, H, hd, sh, w_in16, w_out16, drop, need_w, out_l, shape):
    """What both attention sub-layers do behind their in-projections: the attention core (its dropout keep-mask as bit words
    exactly when the backward is the single-pass kernel: attn_mask_bits), out-projection + dropout + residual + LayerNorm
    (_proj_ln), the head-averaged map if asked for, and the node's bookkeeping.  x2 / x32v: the residual rows [M, d] and their
    fp32 twin; drop = (p, seed, site, b_off); out_l: the padded lengths of a packed map; ctx.params = (w_in, b_in, w_out, b_out,
    gamma, beta) as set by the caller.  Saved for the backward: `head` (the in-projection's tensors), then o, lse, g, mean, rstd,
    w_in16, w_out16, gamma, mask bits.  -> the Function's results (y, y32 | None, probs | None), y shaped `shape`."""
    p, seed, site, b_off = drop
    _, _, w_out, b_out, gamma, beta = ctx.params
    o, lse, *mbits = attn_fwd(q, k, v, ar.B, H, ar.Lq, ar.Lk, hd, ar.kpm, p, seed, site, b_off,
                              want_bits=attn_mask_bits(ar.B, H, ar.Lk, hd, ar.Lq), cu=ar.cu)
    g, y, y32, mean, rstd, mx = _proj_ln(o, sh, w_out, w_out16, b_out, x2, x32v, gamma, beta, p, seed, site + 1, b_off * ar.stride,
                                         ar.rows)
    probe(site, 0, y, ctx.seq_q)
    probs = attn_probs(q, k, ar.B, H, ar.Lq, ar.Lk, hd, ar.kpm, lse, p, seed, site, b_off, ar.cu, out_l,
                       log=need_w if isinstance(need_w, LogSite) else None) if need_w else None
    ctx.save_for_backward(*head, o, lse, g, mean, rstd, w_in16, w_out16, gamma, mbits[0] if mbits else None)
    ctx.rows = ar
    ctx.mark_non_differentiable(*([probs] if probs is not None else []))
    return tag_mx(y.view(shape), mx), (y32.view(shape) if y32 is not None else None), probs


def _ln_bwd(params, dy, dy32, g, x2, x32v, gamma, mean, rstd, p, seed, site, row_off, rows, want_dx=True, seq=None):
    """How every sub-layer's backward opens: the gradients of its output pair summed, the GradSink of `params` = (..., bias of the
    last Linear, gamma, beta), LayerNorm + residual + dropout backward into the sink's buffers.
    -> (sink, dS: the residual path's gradient (None unless want_dx), dG: the last Linear's output gradient, dgamma, dbeta, dbias)
    seq: the Seq of the rows -- the summed gradient is the gradient half of the sub-layer's site in an activation log (probe)"""
    dy2 = _contig_bf16(_sum_grads(dy, dy32)).view(x2.shape)
    if seq is not None:
        probe(site - 1, 1, dy2, seq)
    sink = GradSink(params)
    return (sink,) + add_ln_bwd(dy2, g, x2, gamma, mean, rstd, p, seed, site, row_off, want_dx=want_dx,
                                outs=(sink.buf(params[-2]), sink.buf(params[-1]), sink.buf(params[-3])),
                                accumulate=sink.fused, x32=x32v, rows=rows)


def _attn_ln_bwd(ctx, params, dy, dy32, x2, x32v, tail, want_dx=True):
    """_ln_bwd and the out-projection's backward of an attention sub-layer; params = (..., w_out, b_out, gamma, beta), tail: the
    saved tensors behind the in-projection's (_attn_ln_fwd).
    -> (sink, dS (None unless want_dx), dO: the attention output's gradient, dw_out, db_out, dgamma, dbeta)"""
    o, lse, g, mean, rstd, w_in16, w_out16, gamma, mbits = tail
    p, seed, site, b_off = ctx.cfg[-4:]
    sink, ds, dg, dgamma, dbeta, db_out = _ln_bwd(params, dy, dy32, g, x2, x32v, gamma, mean, rstd, p, seed, site + 1,
                                                  b_off * ctx.rows.stride, ctx.rows.rows, want_dx, seq=ctx.seq_q)
    dw_out = sink.buf(params[-4])
    linear_dw(dg, o, dw_out, sink.fused)
    return sink, ds, linear_dx(dg, w_out16), dw_out, db_out, dgamma, dbeta


class SelfAttnLN(_GradModeAware, torch.autograd.Function):
    """y = LN(x + drop(out_proj(MHA_core(in_proj(x))))) ; returns (y, probs|None)"""

    @staticmethod
    def forward(ctx, x, x32, w_in, b_in, w_out, b_out, gamma, beta, sh, H, seq, p, seed, site, b_off, need_w):
        """seq: the Seq of x's rows ([B, L, d] padded with its mask, or [1, N_valid, d] packed)"""
        seq.holds(x)
        if precision() == "fp32":
            return _fp32().self_attn_ln(ctx, x, x32, w_in, b_in, w_out, b_out, gamma, beta, sh, H, seq, need_w, p, seed, site, b_off)
        _require_fp32_masters(w_in, b_in, w_out, b_out, gamma, beta)
        ctx.set_materialize_grads(False)      # an unused twin output must arrive as None, not as zeros
        _require_gpu(x)
        B, L, d = x.shape
        hd = _heads(d, H)
        M = B * L
        ar = attn_rows(seq, seq, need_w)
        x2 = _contig_bf16(x).view(M, d)
        x32 = _c32(x32)
        x32v = x32.view(M, d) if x32 is not None else None
        w_in16, w_out16 = sh.get(w_in), sh.get(w_out)
        ctx.cfg = (B, L, d, H, hd, p, seed, site, b_off)
        ctx.params = (w_in, b_in, w_out, b_out, gamma, beta)
        ctx.seq_q = seq
        qkv = proj_fwd(Operand(x2, mx_of(x)), sh, w_in, w_in16, b_in)
        return _attn_ln_fwd(ctx, (x2, x32v, qkv), qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], x2, x32v, ar, H, hd, sh, w_in16,
                            w_out16, (p, seed, site, b_off), need_w, (seq.L, seq.L), (B, L, d))

    @staticmethod
    def backward(ctx, dy, dy32, _dprobs):
        if getattr(ctx, "fp32", False):
            return _fp32().self_attn_ln_bwd(ctx, dy, dy32)
        x2, x32v, qkv, o, lse, _, _, _, w_in16, _, _, mbits = saved = ctx.saved_tensors
        B, L, d, H, hd, p, seed, site, b_off = ctx.cfg
        ar = ctx.rows
        M = B * L
        p_w_in, p_b_in = ctx.params[:2]
        # x is the model's input in the first encoder layer: where autograd asks for neither x's nor its twin's gradient, the
        # residual gradient dS (its only reader is the dX GEMM below) and that GEMM are not computed at all
        want_dx = ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or FORCE_INPUT_GRAD
        sink, ds, do, dw_out, db_out, dgamma, dbeta = _attn_ln_bwd(ctx, ctx.params, dy, dy32, x2, x32v, saved[-9:], want_dx)
        acc = sink.fused
        dqkv = torch.empty((M, 3 * d), dtype=BF16, device=x2.device)
        db_in = sink.buf(p_b_in)
        folded = attn_bwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, do, dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:],
                          lse, ar.B, H, ar.Lq, ar.Lk, hd, ar.kpm, p, seed, site, b_off, bias_grad=(db_in[:d], db_in[d:], acc), mask_bits=mbits,
                          cu=ar.cu)
        dw_in = sink.buf(p_w_in)
        linear_dw(dqkv, x2, dw_in, acc)
        if not folded:
            colsum(dqkv, db_in, acc)
        dx = linear_dx(dqkv, w_in16, epi=3, aux=ds).view(B, L, d) if want_dx else None
        if CTX.act_log is not None and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            probe(("input", site), 1, dx, ctx.seq_q)      # layer 0 only (the log's keys): x is the rows the encoder starts from
        sink.done()
        if site in FLUSH_SITES:
            _small_dw.flush()                 # the text branch's backward ends here: queued decoder / gate weight gradients go out now
        r = sink.ret
        return (dx, None, r(dw_in), r(db_in), r(dw_out), r(db_out), r(dgamma), r(dbeta)) + (None,) * 8


class CrossAttnLN(_GradModeAware, torch.autograd.Function):
    """y = LN(xq + drop(out_proj(MHA_core(Wq xq, Wkv xkv)))) ; returns (y, probs|None)"""

    @staticmethod
    def forward(ctx, xq, xq32, xkv, w_in, b_in, w_out, b_out, gamma, beta, sh, H, seq_q, seq_k, p, seed, site, b_off, need_w,
                kv_pre=None, join_q=None, q_pre=None, slots=None):
        """seq_q / seq_k: the Seq of xq's and of xkv's rows (both padded, the keys' mask on seq_k, or both packed).
        kv_pre: the K | V projection of xkv computed by KVProjFn ahead of time (the decoder hoists it onto the side stream); its
        weight-gradient and dX then belong to that Function, this one returns dK | dV for it.
        q_pre: likewise the Q projection of xq (SharedProjFn: one GEMM per shared input); this Function then only returns dQ for it
        and hands the residual-path gradient of xq to join_q.  slots = (SharedGrad of dQ, SharedGrad of dK|dV): where the attention
        backward writes those gradients, so that they arrive at the projection's backward as column slices of ONE buffer.
        This node owns its Q projection unless q_pre is given and its K | V projection unless kv_pre is; the combinations in use
        are: neither given, kv_pre, and kv_pre + q_pre + slots (both projections belong to SharedProjFn nodes)."""
        if (q_pre is None) != (slots is None) or (q_pre is not None and kv_pre is None):
            raise ValueError("CrossAttnLN: q_pre and slots come together, and only with kv_pre (both projections made by SharedProjFn)")
        seq_q.holds(xq)
        seq_k.holds(xkv)
        if precision() == "fp32":
            return _fp32().cross_attn_ln(ctx, xq, xq32, xkv, w_in, b_in, w_out, b_out, gamma, beta, sh, H, seq_q, seq_k, need_w, p, seed,
                                         site, b_off)
        _require_fp32_masters(w_in, b_in, w_out, b_out, gamma, beta)
        ctx.set_materialize_grads(False)      # an unused twin output must arrive as None, not as zeros
        _require_gpu(xq)
        B, Lq, d = xq.shape
        Lk = xkv.shape[1]
        hd = _heads(d, H)
        ar = attn_rows(seq_q, seq_k, need_w)
        xq2 = _contig_bf16(xq).view(B * Lq, d)
        xq32 = _c32(xq32)
        x32v = xq32.view(B * Lq, d) if xq32 is not None else None
        ctx.cfg = (B, Lq, Lk, d, H, hd, p, seed, site, b_off)
        ctx.params = (w_in, b_in, w_out, b_out, gamma, beta)
        ctx.seq_q = seq_q
        ctx.own_q, ctx.own_kv, ctx.slots, ctx.join_q = q_pre is None, kv_pre is None, slots, join_q
        w_out16 = sh.get(w_out)
        w_in16 = sh.get(w_in) if (ctx.own_q or ctx.own_kv) else None
        q = q_pre if q_pre is not None else proj_fwd(Operand(xq2, mx_of(xq)), sh, w_in, w_in16, b_in, rows=(0, d))
        if kv_pre is not None:
            xkv2, kv = None, kv_pre
        else:
            xkv2 = _contig_bf16(xkv).view(B * Lk, d)
            kv = proj_fwd(Operand(xkv2, mx_of(xkv)), sh, w_in, w_in16, b_in, rows=(d, 3 * d))
        return _attn_ln_fwd(ctx, (xq2, x32v, xkv2, q, kv), q, kv[:, :d], kv[:, d:], xq2, x32v, ar, H, hd, sh, w_in16,
                            w_out16, (p, seed, site, b_off), need_w, (seq_q.L, seq_k.L), (B, Lq, d))

    @staticmethod
    def backward(ctx, dy, dy32, _dprobs):
        """One body for the three owners of the projections.  Always here: LayerNorm / out-projection backward, the attention core's
        backward with the in-projection's bias gradients from its column sums, and the residual-path gradient of xq.  A projection
        this node owns gets its weight gradient and dX here; one it does not own gets dQ / dK | dV returned for its node (written
        straight into the SharedProjFn nodes' gradient buffers: slots), which also writes and reports its rows of dW_in."""
        if getattr(ctx, "fp32", False):
            return _fp32().cross_attn_ln_bwd(ctx, dy, dy32)
        xq2, x32v, xkv2, q, kv, o, lse, _, _, _, w_in16, _, _, mbits = saved = ctx.saved_tensors
        B, Lq, Lk, d, H, hd, p, seed, site, b_off = ctx.cfg
        ar = ctx.rows
        own_q, own_kv = ctx.own_q, ctx.own_kv
        p_w_in, p_b_in = ctx.params[:2]
        sink, ds, do, dw_out, db_out, dgamma, dbeta = _attn_ln_bwd(ctx, ctx.params if own_q else ctx.params[1:], dy, dy32, xq2, x32v, saved[-9:])
        acc = sink.fused
        if own_q:
            dq = torch.empty((B * Lq, d), dtype=BF16, device=xq2.device)
            dkv = (torch.zeros if ar.kv_surplus else torch.empty)((B * Lk, 2 * d), dtype=BF16, device=xq2.device)
        else:
            dq, dkv = ctx.slots[0].buf(), ctx.slots[1].buf()
        db_in = sink.buf(p_b_in)
        folded = attn_bwd(q, kv[:, :d], kv[:, d:], o, do, dq, dkv[:, :d], dkv[:, d:], lse, ar.B, H, ar.Lq, ar.Lk, hd, ar.kpm, p, seed,
                          site, b_off, bias_grad=(db_in[:d], db_in[d:], acc), mask_bits=mbits, cu=ar.cu)
        dw_in = None
        if own_q:
            dw_in = sink.buf(p_w_in)
            linear_dw(dq, xq2, dw_in[:d], acc)
        if not folded:
            colsum(dq, db_in[:d], acc)
            colsum(dkv, db_in[d:], acc)
        dxq = linear_dx(dq, w_in16[:d], epi=3, aux=ds) if own_q else ds
        if ctx.join_q is not None:            # xq has another consumer (GradJoin): deposit for it, or finish the sum if it came first
            last, dep = ctx.join_q.arrive()   # (the Q projection's own node folds the deposit into its dX GEMM's epilogue)
            if dep is not None:
                dxq = dxq + dep.view(B * Lq, d)          # this GEMM's aux slot carries the residual gradient: explicit add
            if not last:
                ctx.join_q.deposit(dxq)
                dxq = None
        dxq = dxq.view(B, Lq, d) if dxq is not None else None
        dxkv = None
        if own_kv:
            linear_dw(dkv, xkv2, dw_in[d:], acc)
            dxkv = linear_dx(dkv, w_in16[d:]).view(B, Lk, d)
        elif own_q and not acc:
            dw_in[d:].zero_()                 # KVProjFn adds its rows of dW_in
        sink.done(skip=() if own_kv else (p_w_in,))          # (and reports the parameter)
        r = sink.ret
        return (dxq, None, dxkv, r(dw_in), r(db_in), r(dw_out), r(db_out), r(dgamma), r(dbeta)) + (None,) * 9 + \
            (None if own_kv else dkv, None, None if own_q else dq, None)


class GradJoin:
    """One tensor, n consumers that are Functions of this file (the audio self-attention output feeds the a2t queries AND the t2a
    keys / values; the decoder's memory feeds every layer): autograd would sum their gradients with an elementwise add launch per
    pair.  Here every consumer but the last DEPOSITS its gradient and returns None, the last folds the deposit into its dX
    GEMM's add-aux epilogue (epi = 3) and returns the total.  "Last" is decided by arrival, so any execution order of the
    consumers' backward is correct; a consumer that cannot fold (its GEMM's aux slot is taken) adds explicitly.  If a consumer's
    backward never runs, the deposit would be lost: an engine final callback checks that every join was completed."""

    def __init__(self, n=2):
        self.n, self.seen, self.dep, self.ev = n, 0, None, None

    def arrive(self):
        """-> (is_last, deposit | None): the deposit is ordered before the caller's stream on return"""
        if self.seen == 0:
            torch.autograd.Variable._execution_engine.queue_callback(self._check)
        self.seen += 1
        last = self.seen == self.n
        dep, ev = self.dep, self.ev
        self.dep = self.ev = None
        if last:
            self.seen = 0
        if dep is not None:
            cur = torch.cuda.current_stream(dep.device)
            if ev != cur:                      # `ev` is the depositor's stream
                cur.wait_stream(ev)
                dep.record_stream(cur)         # also inside a capture: the depositor's stream must not reuse it under the reader
        return last, dep

    def deposit(self, t):
        self.dep = t
        self.ev = torch.cuda.current_stream(t.device)

    def _check(self):
        if self.seen != 0 or self.dep is not None:
            self.seen, self.dep, self.ev = 0, None, None
            raise RuntimeError("GradJoin: a consumer of a shared activation did not run its backward; its partner's gradient was "
                               "deposited for it (_ops.GRAD_JOIN = False lets autograd sum the gradients)")


GRAD_JOIN = True           # (False: autograd sums the gradients of a shared activation -- what the tests hold the joins against)
SHARED_PROJ = True         # one N = 3d projection GEMM per shared encoder input (SharedProjFn); False: Q and K | V apart


def shared_proj():
    return SHARED_PROJ


def grad_join(n=2, always=False):
    """a GradJoin where every consumer is certain to run its backward: the encoder's joins only inside the fusion model's forward
    (a stand-alone CrossModalBlock may be trained on one of its two outputs, and the unused branch's consumers never run), the
    decoder's (its layers are a chain) always"""
    return GradJoin(n) if (GRAD_JOIN and torch.is_grad_enabled() and (always or CTX.join_scope > 0)) else None


class SharedGrad:
    """[M, 3d] gradient buffer of one SharedProjFn output, filled by two attention backward launches (dQ by the cross-attention
    this input queries, dK | dV by the one it serves as keys / values -- different streams), so that the projection's backward
    reads ONE dY operand.  A slot is a column range of it; the buffer is allocated by whichever slot is asked first."""

    def __init__(self, M, d, device):
        # Allocated HERE, in the forward, on the stream of its projection and before the branches exchange their K | V halves
        # (a point both streams are ordered behind): never in backward by whichever attention core comes first.  A buffer born
        # in backward on one stream can be written by the OTHER stream before the allocating stream has run the kernels that
        # still read the block's previous occupant -- the allocator only orders reuse within the allocating stream.  That was a
        # real race: the text branch's dQ landed in a block the audio branch's pending FFN dX GEMM still read its residual
        # operand from (scripts_dev/soak_step.py 500 16 ragged: a handful of dirty replays in 500, first differing word always
        # layer 1's attn_a2t.out_proj gradient).  Cost: (M_a + M_t) x 3d bf16 per layer held from forward to backward (312 MB
        # at cfg 2).
        self.M, self.d, self.device = M, d, device
        self.t = torch.empty((M, 3 * d), dtype=BF16, device=device) if torch.is_grad_enabled() else None
        self.stream = torch.cuda.current_stream(device) if self.t is not None else None

    def slot(self, c0, c1):
        return _SharedSlot(self, c0, c1)

    def guard(self, cur):
        """the buffer is used on `cur`, possibly not the stream it was allocated on: the allocator must not hand its memory to a
        later allocation of the allocating stream while `cur` still works on it.  Also inside a capture (there the block simply
        stays reserved until the capture ends): without it a replayed step raced -- the determinism test caught it."""
        if self.t is not None and self.stream != cur:
            self.t.record_stream(cur)

    def take(self):
        self.guard(torch.cuda.current_stream(self.device))          # the projection's backward reads it on its own stream
        t, self.t = self.t, None
        return t


class _SharedSlot:
    def __init__(self, owner, c0, c1):
        self.owner, self.c0, self.c1 = owner, c0, c1

    def buf(self):
        o = self.owner
        cur = torch.cuda.current_stream(o.device)
        if o.t is None:                       # (forward ran under no_grad, or the buffer was already consumed: a second backward)
            o.t = torch.empty((o.M, 3 * o.d), dtype=BF16, device=o.device)
            o.stream = cur
            o.late = True
        else:
            o.guard(cur)
            if getattr(o, "late", False) and o.stream != cur:
                cur.wait_stream(o.stream)     # born in backward after all: order this stream behind the allocating one first
        return o.t[:, self.c0:self.c1]


def _report_half(p, sink):
    """an in-projection weight's gradient is written by TWO SharedProjFn nodes (rows [:d] by the projection of the tensor it
    queries, rows [d:] by the one it serves as keys / values): the gradient-ready notification goes out with the second"""
    hook = getattr(p, "_hriemo_grad_ready", None)
    if not sink.fused or hook is None:
        return
    n = CTX.half_reports.get(id(p), 0) + 1
    if n == 2:
        CTX.half_reports.pop(id(p), None)
        hook(p)
    else:
        CTX.half_reports[id(p)] = n


class SharedProjFn(torch.autograd.Function):
    """[q | kv][M, 3d] = x . [W_q ; W_kv]^T + [b_q ; b_kv] -- ONE N = 3d GEMM per shared input (reference call
    sites models/cross_modal_block_tacfn.py:98-104,111-117): each self-attention output is the query input of its own
    cross-attention (rows [:d] of that module's in_proj_weight) and the key / value input of the other one (rows [d:] of the
    other module's).  Forward: one GEMM on the row-concatenated bf16 shadow; backward: one K = 3d dX GEMM (the residual-path
    gradient of x from the cross-attention's LayerNorm arrives through `join` and is added in the epilogue) and the weight
    gradients from the same [M, 3d] dY buffer.  state_dict is untouched: the parameters stay where the reference has them."""

    @staticmethod
    def forward(ctx, x, wq, bq, wkv, bkv, sh, join, shared):
        _require_fp32_masters(wq, bq, wkv, bkv)
        _require_gpu(x)
        ctx.set_materialize_grads(False)      # a half nobody differentiated must arrive as None, not as zeros
        B, L, d = x.shape
        x2 = _contig_bf16(x).view(B * L, d)
        wcat, bcat = sh.get_cat_wb(((wq, 0, d), (wkv, d, 3 * d)), ((bq, 0, d), (bkv, d, 3 * d)))
        if gemm_mode() == "mx_fp8" and mx8_ok(d, 3 * d, B * L):
            # cfg 5: the same ONE N = 3d launch on MX-fp8 operands (the LayerNorm that produced x left its fp8 copy; the
            # concatenated weight is quantised slice by slice into one buffer); the backward below is the bf16 one either way
            xq, xs = Operand(x2, mx_of(x)).q()
            wq8, ws8 = sh.get_cat_mx8(((wq, 0, d), (wkv, d, 3 * d)))
            out = linear_fwd_mx8(xq, xs, wq8, ws8, bcat)
        else:
            out = linear_fwd(x2, wcat, bcat)
        ctx.save_for_backward(x2, wcat)
        ctx.cfg = (B, L, d)
        ctx.join, ctx.shared = join, shared
        ctx.params = (wq, wkv)
        return out[:, :d], out[:, d:]

    @staticmethod
    def backward(ctx, dq, dkv):
        x2, wcat = ctx.saved_tensors
        B, L, d = ctx.cfg
        M = B * L
        dcat = ctx.shared.take()
        if dq is None and dkv is None:
            return (None,) * 8
        ok = (dcat is not None and dq is not None and dkv is not None and dq.data_ptr() == dcat.data_ptr()
              and dkv.data_ptr() == dcat.data_ptr() + 2 * d and dq.stride(0) == 3 * d and dkv.stride(0) == 3 * d)
        if not ok:                                # gradients that did not come through the shared buffer (or only one of them)
            dcat = torch.zeros((M, 3 * d), dtype=BF16, device=x2.device)
            if dq is not None:
                dcat[:, :d].copy_(dq)
            if dkv is not None:
                dcat[:, d:].copy_(dkv)
        wq, wkv = ctx.params
        sq, skv = GradSink((wq,)), GradSink((wkv,))
        dwq = dwkv = None                         # a half whose gradient never arrived leaves its weight's .grad alone (None, like
        if dq is not None:                        # autograd would for a cross-attention that took no part in the loss)
            dwq = sq.buf(wq)
            if not sq.fused:
                dwq[d:].zero_()
        if dkv is not None:
            dwkv = skv.buf(wkv)
            if not skv.fused:
                dwkv[:d].zero_()
        if dwq is not None and dwkv is not None and sq.fused == skv.fused:
            linear_dw_split(dcat, x2, dwq[:d], dwkv[d:], d, sq.fused)        # one 3d x d x M weight-gradient GEMM, two destinations
        else:
            if dwq is not None:
                linear_dw(dcat[:, :d], x2, dwq[:d], sq.fused)
            if dwkv is not None:
                linear_dw(dcat[:, d:], x2, dwkv[d:], skv.fused)
        dep = None
        if ctx.join is not None:
            _, dep = ctx.join.arrive()
        dx = linear_dx(dcat, wcat, epi=3, aux=dep.view(M, d)) if dep is not None else linear_dx(dcat, wcat)
        _report_half(wq, sq)
        _report_half(wkv, skv)
        return dx.view(B, L, d), (sq.ret(dwq) if dwq is not None else None), None, (skv.ret(dwkv) if dwkv is not None else None), None, None, None, None


class KVProjFn(torch.autograd.Function):
    """kv[B*L_k, 2d] = x_kv . W_in[d:3d]^T + b_in[d:3d]: the key / value half of a cross-attention's packed in-projection as a node
    of its own, so that the decoder can run it (forward and backward) on the side stream beside its serial chain of
    latency-bound launches -- the memory does not depend on the queries (models/emotion_decoder.py:48-54).  The bias gradient
    stays with CrossAttnLN (it comes out of the attention backward's column sums)."""

    @staticmethod
    def forward(ctx, xkv, w_in, b_in, sh, join=None):
        _require_fp32_masters(w_in, b_in)
        _require_gpu(xkv)
        ctx.join = join
        B, Lk, d = xkv.shape
        xkv2 = _contig_bf16(xkv).view(B * Lk, d)
        w_in16 = sh.get(w_in)
        kv = proj_fwd(Operand(xkv2, mx_of(xkv)), sh, w_in, w_in16, b_in, rows=(d, 3 * d))
        ctx.save_for_backward(xkv2, w_in16)
        ctx.cfg = (B, Lk, d)
        ctx.params = (w_in,)
        return kv

    @staticmethod
    def backward(ctx, dkv):
        xkv2, w_in16 = ctx.saved_tensors
        B, Lk, d = ctx.cfg
        dkv = _contig_bf16(dkv)
        sink = GradSink(ctx.params)
        acc = sink.fused
        dw_in = sink.buf(ctx.params[0])
        if not acc:
            dw_in[:d].zero_()
        linear_dw(dkv, xkv2, dw_in[d:], acc)
        last, dep = ctx.join.arrive() if ctx.join is not None else (True, None)
        dxkv = linear_dx(dkv, w_in16[d:], epi=3, aux=dep.view(B * Lk, d)) if dep is not None else linear_dx(dkv, w_in16[d:])
        sink.done()
        if not last:
            ctx.join.deposit(dxkv)
            return None, sink.ret(dw_in), None, None, None
        return dxkv.view(B, Lk, d), sink.ret(dw_in), None, None, None


class FFNLN(_GradModeAware, torch.autograd.Function):
    """y = LN(x + drop(W2 . drop_mid(relu(W1 x + b1)) + b2))"""

    @staticmethod
    def forward(ctx, x, x32, w1, b1, w2, b2, gamma, beta, sh, p, p_mid, seed, site, b_off, seq):
        """seq: the Seq of x's rows; packed (x is [1, N_valid, d]) it keys the LayerNorm dropout by the rows of the padded layout"""
        seq.holds(x)
        if seq.packed and p_mid > 0:
            raise ValueError("FFNLN: packed rows with a mid-FFN dropout are not built (the encoder's FFNs have none)")
        if precision() == "fp32":
            return _fp32().ffn_ln(ctx, x, x32, w1, b1, w2, b2, gamma, beta, sh, p, p_mid, seed, site, b_off, seq)
        _require_fp32_masters(w1, b1, w2, b2, gamma, beta)
        ctx.set_materialize_grads(False)      # an unused twin output must arrive as None, not as zeros
        _require_gpu(x)
        B, L, d = x.shape
        M = B * L
        x2 = _contig_bf16(x).view(M, d)
        x32 = _c32(x32)
        x32v = x32.view(M, d) if x32 is not None else None
        w1_16, w2_16 = sh.get(w1), sh.get(w2)
        h = proj_fwd(Operand(x2, mx_of(x)), sh, w1, w1_16, b1, relu=True, want_q=p_mid == 0)
        hd_ = h
        if p_mid > 0:
            hd_ = torch.empty_like(h)
            if DROP_LOG is not None:
                DROP_LOG.append(("rows", seed, site + 2, M, h.shape[1], float(p_mid), b_off * L))
            _lib.call("hriemo_dropout_bf16", _p(h), _p(hd_), M, h.shape[1], float(p_mid), seed, _p(seed_word(h.device)),
                      site + 2, b_off * L, _stream())
        g, y, y32, mean, rstd, mx = _proj_ln(hd_, sh, w2, w2_16, b2, x2, x32v, gamma, beta, p, seed, site + 1, b_off * seq.L, seq.idx)
        probe(site, 0, y, seq)
        ctx.save_for_backward(x2, x32v, h, hd_, g, mean, rstd, w1_16, w2_16, gamma)
        ctx.cfg = (B, L, d, p, p_mid, seed, site, b_off)
        ctx.seq = seq
        ctx.params = (w1, b1, w2, b2, gamma, beta)
        return tag_mx(y.view(B, L, d), mx), (y32.view(B, L, d) if y32 is not None else None)

    @staticmethod
    def backward(ctx, dy, dy32):
        if getattr(ctx, "fp32", False):
            return _fp32().ffn_ln_bwd(ctx, dy, dy32)
        x2, x32v, h, hd_, g, mean, rstd, w1_16, w2_16, gamma = ctx.saved_tensors
        B, L, d, p, p_mid, seed, site, b_off = ctx.cfg
        M, F = h.shape
        dev = x2.device
        p_w1, p_b1, p_w2 = ctx.params[:3]
        sink, ds, dg, dgamma, dbeta, db2 = _ln_bwd(ctx.params, dy, dy32, g, x2, x32v, gamma, mean, rstd, p, seed, site + 1,
                                                   b_off * ctx.seq.L, ctx.seq.idx, seq=ctx.seq)
        acc = sink.fused
        dw2 = sink.buf(p_w2)
        linear_dw(dg, hd_, dw2, acc)
        db1 = sink.buf(p_b1)
        fold = p_mid == 0 and fold_ffn_bias()
        if fold:                                         # db1 = colsum(da) out of the GEMM that writes da
            da = linear_dx_masked_colsum(dg, w2_16, h, db1, acc)
        else:
            da = linear_dx(dg, w2_16, epi=2, aux=h)          # * relu'(h)
        if p_mid > 0:
            _lib.call("hriemo_dropout_bf16", _p(da), _p(da), M, F, float(p_mid), seed, _p(seed_word(dev)), site + 2, b_off * L,
                      _stream())
        dw1 = sink.buf(p_w1)
        linear_dw(da, x2, dw1, acc)
        if not fold:
            colsum(da, db1, acc)
        dx = linear_dx(da, w1_16, epi=3, aux=ds)
        sink.done()
        r = sink.ret
        return (dx.view(B, L, d), None, r(dw1), r(db1), r(dw2), r(db2), r(dgamma), r(dbeta)) + (None,) * 7


def _gate_align(La, Lt):
    """the fused length: both streams aligned to the text length (beta_gate_tacfn.py:98-104, beta_gate.py:97-101)"""
    L = La if La == Lt else Lt
    if La < L:
        raise RuntimeError(f"BetaGate: audio length {La} < text length {Lt}; the reference cannot fuse this either")
    return L


def _gate_prologue(h_a, h_a32, h_t, h_t32, params, sa, st):
    """what both gate forwards do before their first launch -> (L, xa, h_a32, xt, h_t32, (mean, rstd, masked-pool partials) of the
    audio side, the same of the text side)"""
    L = _gate_align(sa.L, st.L)
    _require_fp32_masters(*params)
    _require_gpu(h_a)
    d = h_a.shape[-1]
    f32 = dict(dtype=torch.float32, device=h_a.device)
    chunks = _lib.lib().hriemo_pool_chunks
    bufs = lambda s: (torch.empty(s.N, **f32), torch.empty(s.N, **f32), torch.empty((s.Breal, chunks(s.L), d), **f32))  # noqa: E731
    return L, _contig_bf16(h_a), _c32(h_a32), _contig_bf16(h_t), _c32(h_t32), bufs(sa), bufs(st)


def _both_sides(d, dev, pair, single, side_a, side_t, two_streams=False, shared=()):
    """One step of the gate for both modalities.  pair(side_a, side_t): both from ONE launch, no fork / join around the step (two graph
    edges and 10-27 us of idle device each) -- where the library has it (d <= 1024) and the caller offers it (pair not None).  Else
    single(*side) per modality; the two are independent: with two_streams the (small) text one runs on the side stream beside the audio
    one -- `shared`: what the side stream touched of this stream's tensors -- else behind it."""
    main = torch.cuda.current_stream(dev)
    side = side_stream(dev) if two_streams else None
    if pair is not None and _lib.lib().hriemo_ln_pool_pair_supported(d):
        pair(side_a, side_t)
    elif side is not None and side != main:
        fork(side, main)
        with torch.cuda.stream(side):
            single(*side_t)
        single(*side_a)
        main.wait_stream(side)
        if not CTX.capturing:
            for t_ in shared:
                share(t_, side)
    else:
        single(*side_a)
        single(*side_t)


class _LnAffine:
    """The LayerNorm-affine gradients grads = (dga, dba, dgt, dbt) of a gate backward.  They are finished by the launch-boundary reduce
    when they accumulate into .grad inside backward (defer: the kernels' partial sums then live in buffers of their own and outs is all
    None), else by the launch's own reduce, out of the shared workspace slot."""

    def __init__(self, sink, grads, B, La, Lt, d, dev):
        L_ = _lib.lib()
        self.defer = sink.fused and DEFER_REDUCE and _in_backward()
        self.grads, self.outs, self.acc = grads, (None,) * 4 if self.defer else grads, int(sink.fused)
        self.nbytes = tuple(L_.hriemo_ln_pool_bwd_workspace_bytes(B, L, d) for L in (La, Lt))
        self.rows = tuple(B * L_.hriemo_ln_pool_bwd_chunks(L) for L in (La, Lt))
        self.d, self.dev = d, dev

    def workspaces(self):
        """(audio, text) for launches on ONE stream: own buffers when deferring, else one slot split at a 64-float boundary"""
        if self.defer:
            return tuple(torch.empty(n // 4 + 16, dtype=torch.float32, device=self.dev) for n in self.nbytes)
        wsa = workspace(sum(self.nbytes) + 256, self.dev, slot=1)
        return wsa, wsa[(self.nbytes[0] // 4 + 63) // 64 * 64:]

    def queue(self, ws, text):
        """behind the launch that left the partial sums of one side (text = 0 | 1) in ws"""
        if self.defer:
            _deferred.add(ws, 2 * self.d, self.rows[text], self.d, 2, list(self.grads[2 * text:2 * text + 2]), True)


def _gate_weights(pa, pt, sa, st, B, La, Lt, d, w1, b1, w2, b2, sh):
    """the vector gate from the pooled partial sums of both modalities (beta_gate_tacfn.py:83-95): masked means, gate input
    [a, t, |a-t|, a*t], the two-layer MLP, w = sigmoid, beta = mean(w) -> (gin, a_pool, t_pool, cnt, hid, w, beta, w1_16, w2_16).
    Shared by BetaGateFn and PooledGateFn."""
    dev = pa.device
    f32 = dict(dtype=torch.float32, device=dev)
    st_ = _stream()
    gin = torch.empty((B, 4 * d), dtype=BF16, device=dev)
    a_pool, t_pool = torch.empty((B, d), **f32), torch.empty((B, d), **f32)
    cnt = torch.empty((B, 2), **f32)
    _lib.call("hriemo_gate_input", _p(pa), _p(pt), _p(sa.kpm), _p(st.kpm), B, La, Lt, d, _p(gin), _p(a_pool),
              _p(t_pool), _p(cnt), st_)
    w1_16, w2_16 = sh.get(w1), sh.get(w2)
    hid = linear_fwd(gin, w1_16, b1, relu=True)
    pre = linear_fwd(hid, w2_16, b2, out_f32=True)
    w = torch.empty((B, d), **f32)
    beta = torch.empty((B, 1), **f32)
    _lib.call("hriemo_sigmoid_beta", _p(pre), _p(w), _p(beta), B, d, st_)
    return gin, a_pool, t_pool, cnt, hid, w, beta, w1_16, w2_16


def _gate_weights_bwd(part, Lp, dbeta2, w, hid, gin, a_pool, t_pool, cnt, w1_16, w2_16, sink, params, B, d):
    """backward of _gate_weights: part = the dw partial sums [B, hriemo_pool_chunks(Lp), d] -> (da, dt: the gradients of the masked
    means, already divided by the valid counts; dw1, db1, dw2, db2 in the sink's buffers)"""
    p_w1, p_b1, p_w2, p_b2 = params
    dev = w.device
    f32 = dict(dtype=torch.float32, device=dev)
    st_ = _stream()
    acc = sink.fused
    dpre = torch.empty((B, d), dtype=BF16, device=dev)
    _lib.call("hriemo_gate_dpre", _p(part), Lp, _p(dbeta2), _p(w), _p(dpre), B, d, st_)
    dw2 = sink.buf(p_w2)
    linear_dw(dpre, hid, dw2, acc)
    db2 = sink.buf(p_b2)
    colsum(dpre, db2, acc)
    dhid = linear_dx(dpre, w2_16, epi=2, aux=hid)
    dw1 = sink.buf(p_w1)
    linear_dw(dhid, gin, dw1, acc)
    db1 = sink.buf(p_b1)
    colsum(dhid, db1, acc)
    dgin = linear_dx(dhid, w1_16)
    da, dt = torch.empty((B, d), **f32), torch.empty((B, d), **f32)
    _lib.call("hriemo_gate_input_bwd", _p(dgin), _p(a_pool), _p(t_pool), _p(cnt), _p(da), _p(dt), B, d, st_)
    return da, dt, dw1, db1, dw2, db2


def _fused_rows(sa, st, sf):
    """the fused memory's layout as an activation log counts its rows: the packed plan as it is; padded, the rows both modalities
    hold (the reference ORs the two padding masks cut to the fused length)"""
    if sf.packed or (sa.kpm is None and st.kpm is None):
        return sf
    ma = sa.kpm[:, :sf.L] if sa.kpm is not None else None
    m = ma.contiguous() if st.kpm is None else (st.kpm if ma is None else (ma | st.kpm))
    return sf.with_kpm(m)


class BetaGateFn(_GradModeAware, torch.autograd.Function):
    """(h_fusion, beta) = BetaGate(h_a, h_t, masks)  -- models/beta_gate_tacfn.py:68-118
    sa / st / sf: the Seq of h_a's rows, of h_t's rows and of the fused memory's -- all padded ([B, L_a, d], [B, L_t, d], h_fusion
    [B, L_t, d]) or all packed (the encoder's packed rows [1, N, d]; h_fusion comes back as the packed fused memory [1, N_f, d], sample
    b: min(la, lt) rows, surplus rows zero, and backward returns the packed dX of both modalities).  sa and st carry the padding
    masks in both forms (Seq.with_kpm): the valid counts are read from them."""

    @staticmethod
    def forward(ctx, h_a, h_a32, h_t, h_t32, ga, ba, gt, bt, w1, b1, w2, b2, sh, sa, st, sf):
        if not (sa.packed == st.packed == sf.packed):
            raise ValueError("BetaGate: the three layouts must be all padded or all packed")
        B, La, Lt, d = sa.Breal, sa.L, st.L, h_a.shape[-1]
        Ra, Rt = h_a.shape[0] * h_a.shape[1], h_t.shape[0] * h_t.shape[1]
        if Ra != sa.N or Rt != st.N:
            raise ValueError(f"BetaGate: packed rows {Ra} / {Rt} do not match the plan ({sa.N} / {st.N})")
        _gate_align(La, Lt)                  # the refusal comes before the fp32 dispatch; the prologue aligns again for its L
        if precision() == "fp32":           # -> (h_fusion as the fp32 tensor itself, beta)
            return _fp32().beta_gate(ctx, h_a, h_a32, h_t, h_t32, ga, ba, gt, bt, w1, b1, w2, b2, sh, sa, st, sf)
        _, xa, h_a32, xt, h_t32, (mean_a, rstd_a, pa), (mean_t, rstd_t, pt) = _gate_prologue(h_a, h_a32, h_t, h_t32,
                                                                                              (ga, ba, gt, bt, w1, b1, w2, b2), sa, st)
        dev = h_a.device
        An = torch.empty(sf.shape(d), dtype=BF16, device=dev)
        Tn = torch.empty(sf.shape(d), dtype=BF16, device=dev)
        _both_sides(d, dev, (lambda a, t: ln_pool_fwd_pair(a, t, sf, d)) if GATE_PAIR else None, lambda *s: ln_pool_fwd(*s, sf, d),
                    (xa, h_a32, sa, ga, ba, An, mean_a, rstd_a, pa), (xt, h_t32, st, gt, bt, Tn, mean_t, rstd_t, pt),
                    GATE_TWO_STREAMS, (xt, h_t32, st.kpm, Tn, mean_t, rstd_t, pt))
        gin, a_pool, t_pool, cnt, hid, w, beta, w1_16, w2_16 = _gate_weights(pa, pt, sa, st, B, La, Lt, d, w1, b1, w2, b2, sh)
        H = torch.empty(sf.shape(d), dtype=BF16, device=dev)
        fuse_fwd(w, An, Tn, H, sf, d)
        ctx.fused_rows = None
        if CTX.act_log is not None and CTX.act_log.open[0]:
            # (padded rows with masks: ONE elementwise launch of torch's, the OR of the two masks; the backward reuses the layout)
            ctx.fused_rows = _fused_rows(sa, st, sf)
            probe("gate.w", 0, w, Seq.padded(B, 1))
            probe("gate.fused", 0, H, ctx.fused_rows)
        ctx.save_for_backward(xa, xt, An, Tn, mean_a, rstd_a, mean_t, rstd_t, gin, a_pool, t_pool, cnt, hid, w, w1_16,
                              w2_16, ga, gt, h_a32, h_t32)
        ctx.seqs = (sa, st, sf)
        ctx.params = (ga, ba, gt, bt, w1, b1, w2, b2)
        return H, beta

    @staticmethod
    def backward(ctx, dH, dbeta):
        if getattr(ctx, "fp32", False):
            return _fp32().beta_gate_bwd(ctx, dH, dbeta)
        (xa, xt, An, Tn, mean_a, rstd_a, mean_t, rstd_t, gin, a_pool, t_pool, cnt, hid, w, w1_16, w2_16, ga, gt,
         h_a32, h_t32) = ctx.saved_tensors
        sa, st, sf = ctx.seqs
        B, La, Lt, L, d = sa.Breal, sa.L, st.L, st.L, xa.shape[-1]
        dev = xa.device
        f32 = dict(dtype=torch.float32, device=dev)
        p_ga, p_ba, p_gt, p_bt, p_w1, p_b1, p_w2, p_b2 = ctx.params
        # parameter gradients go straight into .grad when the parameters were opted in (dp.GradBuckets): no autograd accumulate
        # launches on the serial chain between the decoder's and the encoder's backward
        sink = GradSink(ctx.params)
        dH2 = _contig_bf16(dH) if dH is not None else torch.zeros(An.shape, dtype=BF16, device=dev)
        if ctx.fused_rows is not None and dH is not None:
            probe("gate.fused", 1, dH2, ctx.fused_rows)
        dbeta2 = dbeta.contiguous().float() if dbeta is not None else None
        part = torch.empty((B, _lib.lib().hriemo_pool_chunks(L), d), **f32)
        fuse_bwd_dw(dH2, An, Tn, part, sf, d)
        da, dt, dw1, db1, dw2, db2 = _gate_weights_bwd(part, L, dbeta2, w, hid, gin, a_pool, t_pool, cnt, w1_16, w2_16, sink,
                                                       (p_w1, p_b1, p_w2, p_b2), B, d)
        dxa = torch.empty(sa.shape(d), dtype=BF16, device=dev)
        dxt = torch.empty(st.shape(d), dtype=BF16, device=dev)
        dga, dba, dgt, dbt = sink.buf(p_ga), sink.buf(p_ba), sink.buf(p_gt), sink.buf(p_bt)
        aff = _LnAffine(sink, (dga, dba, dgt, dbt), B, La, Lt, d, dev)

        def pair(a, t):
            wsa, wst = aff.workspaces()
            ln_pool_bwd_pair(dH2, sf, w, (wsa,) + a[1:] + aff.outs[:2], (wst,) + t[1:] + aff.outs[2:], aff.acc, d)
            aff.queue(wsa, 0)
            aff.queue(wst, 1)

        def one_side(text, *rest):
            # a workspace per side, taken on the stream the side runs on (the text side's may be the side stream)
            wsx = torch.empty(aff.nbytes[text] // 4 + 16, **f32) if aff.defer else workspace(aff.nbytes[text], dev, slot=1)
            ln_pool_bwd(dH2, sf, w, 1 - text, *rest, *aff.outs[2 * text:2 * text + 2], aff.acc, wsx, d)
            aff.queue(wsx, text)

        # (two streams: joined before the gradients are handed back)
        _both_sides(d, dev, pair if GATE_PAIR else None, one_side, (0, da, xa, h_a32, sa, ga, mean_a, rstd_a, dxa),
                    (1, dt, xt, h_t32, st, gt, mean_t, rstd_t, dxt), GATE_TWO_STREAMS, (dH2, w, dt, dxt, dgt, dbt))
        sink.done()
        r = sink.ret
        return dxa, None, dxt, None, r(dga), r(dba), r(dgt), r(dbt), r(dw1), r(db1), r(dw2), r(db2), None, None, None, None


class LegacyBetaGateFn(torch.autograd.Function):
    """(h_fusion, beta) of the legacy scalar gate, models/beta_gate.py:60-114: masked-mean pools of the raw features,
    [a, t, |a-t|, a*t] -> Linear(4d,h) -> ReLU -> Linear(h,1) -> sigmoid = beta[B,1], h = beta*h_a[:, :L] + (1-beta)*h_t[:, :L].
    Everything runs in libhriemo.so: pooling / gate input / fusion row kernels, the MLP on hriemo_gemm_bf16 (first layer) and
    hriemo_rowdot_* (the h -> 1 layer), like the vector gate; only [B]- and [B,h]-sized casts / masks are torch plumbing."""

    @staticmethod
    def forward(ctx, h_a, h_t, w1, b1, w2, b2, sh, kpm_a, kpm_t):
        if precision() == "fp32":
            raise NotImplementedError("HRIEMO_PRECISION=fp32 covers the tacfn model family (FusionWithEmotionDecoder); the legacy "
                                      "scalar gate (models/beta_gate.py) runs on the bf16 path only")
        _require_fp32_masters(w1, b1, w2, b2)
        _require_gpu(h_a)
        B, La, d = h_a.shape
        Lt = h_t.shape[1]
        L = _gate_align(La, Lt)
        dev = h_a.device
        xa, xt = _contig_bf16(h_a), _contig_bf16(h_t)
        f32 = dict(dtype=torch.float32, device=dev)
        st = _stream()
        a_pool, t_pool = torch.empty((B, d), **f32), torch.empty((B, d), **f32)
        cnt_a, cnt_t = torch.empty(B, **f32), torch.empty(B, **f32)
        _lib.call("hriemo_masked_mean_fwd", _p(xa), _p(kpm_a), _p(a_pool), _p(cnt_a), B, La, d, st)
        _lib.call("hriemo_masked_mean_fwd", _p(xt), _p(kpm_t), _p(t_pool), _p(cnt_t), B, Lt, d, st)
        gin = torch.empty((B, 4 * d), dtype=BF16, device=dev)
        _lib.call("hriemo_gate_input_pooled", _p(a_pool), _p(t_pool), _p(gin), B, d, st)
        w1_16 = sh.get(w1)
        hid = linear_fwd(gin, w1_16, b1, relu=True)                                        # [B, h] bf16
        w2f, b2f = w2.detach().float().contiguous(), b2.detach().float().contiguous()
        pre = torch.empty(B, **f32)
        _lib.call("hriemo_rowdot_fwd", _p(hid), None, _p(w2f), _p(b2f), _p(pre), B, hid.shape[1], st)
        beta = torch.empty((B, 1), **f32)
        wfull1 = torch.empty((B, 1), **f32)
        _lib.call("hriemo_sigmoid_beta", _p(pre), _p(wfull1), _p(beta), B, 1, st)          # d = 1: w == beta == sigmoid(pre)
        A = xa if La == L else xa[:, :L].contiguous()
        T = xt
        wfull = beta.expand(B, d).contiguous()
        H = torch.empty((B, L, d), dtype=BF16, device=dev)
        fuse_fwd(wfull, A, T, H, Seq.padded(B, L), d)
        ctx.save_for_backward(A, T, cnt_a, cnt_t, kpm_a, kpm_t, a_pool, t_pool, gin, hid, beta, w1_16, w2f)
        ctx.cfg = (B, La, Lt, L, d)
        return H, beta

    @staticmethod
    def backward(ctx, dH, dbeta):
        A, T, cnt_a, cnt_t, kpm_a, kpm_t, a_pool, t_pool, gin, hid, beta, w1_16, w2f = ctx.saved_tensors
        B, La, Lt, L, d = ctx.cfg
        dev = A.device
        f32 = dict(dtype=torch.float32, device=dev)
        st = _stream()
        L_ = _lib.lib()
        dH2 = _contig_bf16(dH) if dH is not None else torch.zeros((B, L, d), dtype=BF16, device=dev)
        nc = L_.hriemo_pool_chunks(L)
        part = torch.empty((B, nc, d), **f32)
        fuse_bwd_dw(dH2, A, T, part, Seq.padded(B, L), d)
        dbeta_h = torch.empty(B, **f32)
        _lib.call("hriemo_rowsum_f32", _p(part), _p(dbeta_h), B, nc * d, st)               # d loss / d beta through the fusion
        dbeta2 = dbeta.contiguous().float() if dbeta is not None else None
        dpre16 = torch.empty((B, 1), dtype=BF16, device=dev)
        # gate_dpre with d = 1: (dbeta_h + dbeta) * beta * (1 - beta)
        _lib.call("hriemo_gate_dpre", _p(dbeta_h), 1, _p(dbeta2), _p(beta), _p(dpre16), B, 1, st)
        dpre = dpre16.float().view(B)                                                      # [B]-sized plumbing
        Hd = hid.shape[1]
        dhid = torch.empty((B, Hd), dtype=BF16, device=dev)
        dw2 = torch.empty((1, Hd), **f32)
        db2 = torch.empty(1, **f32)
        _lib.call("hriemo_rowdot_bwd", _p(dpre), _p(hid), None, _p(w2f), _p(dhid), _p(dw2), _p(db2), 0, B, Hd, st)
        dhid = dhid * (hid > 0)                                                            # ReLU mask, [B,h]-sized plumbing
        dw1 = torch.empty((Hd, 4 * d), **f32)
        linear_dw(dhid, gin, dw1)
        db1 = torch.empty(Hd, **f32)
        colsum(dhid, db1)
        dgin = linear_dx(dhid, w1_16)
        dpa, dpt = torch.empty((B, d), **f32), torch.empty((B, d), **f32)
        ones = torch.ones((B, 2), **f32)           # scalar_gate_dx divides by the valid counts itself
        _lib.call("hriemo_gate_input_bwd", _p(dgin), _p(a_pool), _p(t_pool), _p(ones), _p(dpa), _p(dpt), B, d, st)
        bflat = beta.reshape(B).contiguous()
        dxa = torch.empty((B, La, d), dtype=BF16, device=dev)
        dxt = torch.empty((B, Lt, d), dtype=BF16, device=dev)
        _lib.call("hriemo_scalar_gate_dx", _p(dH2), L, _p(bflat), 1, _p(dpa), _p(cnt_a), _p(kpm_a), _p(dxa), B, La, d, st)
        _lib.call("hriemo_scalar_gate_dx", _p(dH2), L, _p(bflat), 0, _p(dpt), _p(cnt_t), _p(kpm_t), _p(dxt), B, Lt, d, st)
        return dxa, dxt, dw1, db1, dw2, db2, None, None, None


# ----------------------------------------------------------------------------- pooled gate (FusionClassifier)
# FusionClassifier.forward through PooledGateFn: opt-in, like the packed-tail switches (forward_packed always takes the pooled path)
POOLED_GATE = False


def pooled_gate():
    return bool(POOLED_GATE)


# The pooled gate in the fp32 precision mode (_fp32.pooled_gate, hriemo_pool32_*): with it FusionClassifier's ragged path --
# forward_packed, the captured steps, EvalStep, forward() under POOLED_GATE -- runs in fp32.  A switch of its own, for the reason
# PACKED_TAIL_FP32 has one: an arm becomes a default only after it has been measured as a step (DESIGN 3.5,
# scripts_dev/bench_classifier_fp32.py).  False: the pooled path refuses the fp32 precision, as it did before the fp32 gate existed.
POOLED_GATE_FP32 = False


def set_pooled_gate_fp32(on):
    global POOLED_GATE_FP32
    POOLED_GATE_FP32 = bool(on)


def pooled_gate_fp32():
    return bool(POOLED_GATE_FP32)


def _require_pooled_path(who):
    """the pooled gate serves bf16 GEMM operands in bf16 precision, and in fp32 precision once POOLED_GATE_FP32 is set"""
    if gemm_mode() != "bf16":
        raise NotImplementedError(f"{who}: built for the bf16 GEMM mode only (precision {precision()!r}, GEMM mode {gemm_mode()!r})")
    if precision() == "fp32" and not POOLED_GATE_FP32:
        raise NotImplementedError(f"{who}: the fp32 precision takes the pooled gate only with _ops.POOLED_GATE_FP32 set "
                                  f"(hri_emo_amd.set_pooled_gate_fp32(True)); precision {precision()!r}, GEMM mode {gemm_mode()!r}")


class IngestPaddedFn(torch.autograd.Function):
    """packed rows x [n, d] (fp32 / bf16 / fp16) + the plan's cu_seqlens -> the PADDED (bf16 [Breal, L, d], fp32 twin | None) pair, PAD
    rows zero: ONE launch (hriemo_ingest_padded), no source row behind cu[Breal] is read.  The twin is None where as_pair's is.
    Backward: the pair's gradients gathered back to the packed rows (hriemo_pack_rows), cast to x's dtype and summed."""

    @staticmethod
    def forward(ctx, x, seq):
        ctx.set_materialize_grads(False)
        if x.dtype not in _XT:
            raise TypeError(f"ingest: inputs of dtype {x.dtype} (expected float32, bfloat16 or float16)")
        if not seq.packed or x.dim() != 2 or (seq.B == seq.Breal and x.shape[0] != seq.N):
            raise ValueError(f"ingest: packed rows of shape {tuple(x.shape)} do not match the {seq.N} rows of their plan")
        _require_gpu(x)
        if not (x.is_contiguous() and x.data_ptr() % 16 == 0):
            x = x.contiguous()
        n, d = x.shape
        B, L = seq.Breal, seq.L
        y16 = torch.empty((B, L, d), dtype=BF16, device=x.device)
        y32 = torch.empty((B, L, d), dtype=torch.float32, device=x.device) if (TWIN and x.dtype != BF16) else None
        _lib.call("hriemo_ingest_padded", _p(x), _XT[x.dtype], d, _p(seq.cu), n, B, L, d, _p(y16), _p(y32), _stream())
        ctx.seq, ctx.shape, ctx.dtype = seq, (n, d), x.dtype
        return y16, y32

    @staticmethod
    def backward(ctx, d16, d32):
        if not ctx.needs_input_grad[0] or (d16 is None and d32 is None):
            return None, None
        seq, (n, d) = ctx.seq, ctx.shape
        g = None
        for y, is32 in ((d16, False), (d32, True)):
            if y is None:
                continue
            y = y.contiguous().float() if is32 else _contig_bf16(y)
            out = torch.empty((n, d), dtype=y.dtype, device=y.device)
            _lib.call("hriemo_pack_rows", None if is32 else _p(y), _p(y) if is32 else None, _p(seq.cu), seq.Breal, seq.L, d, n,
                      None if is32 else _p(out), _p(out) if is32 else None, None, _stream())
            out = out.to(ctx.dtype)
            g = out if g is None else g + out
        return g, None


def ln_pool2_fwd(x, x32, sx, gamma, beta, mean, rstd, part, part_keep, Lkeep, d):
    """row statistics, the masked-pooling partials of ln_pool_fwd and the partials over rows l < Lkeep; no Yn (padded rows)"""
    _lib.call("hriemo_ln_pool2_fwd", _p(x), _p(x32), _p(sx.kpm), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(part), _p(part_keep),
              sx.B, sx.L, Lkeep, d, _EPS, _stream())


def ln_pool2_fwd_pair(a, t, Lkeep, d):
    """ln_pool2_fwd of both modalities from one launch; a / t = (x, x32, sx, gamma, beta, mean, rstd, part, part_keep)"""
    side = lambda x, x32, sx, *rest: (_p(x), _p(x32), _p(sx.kpm), *map(_p, rest), sx.L)          # noqa: E731
    _lib.call("hriemo_ln_pool2_fwd_pair", *side(*a), *side(*t), a[2].B, Lkeep, d, _EPS, _stream())


def ln_pool_vec_bwd(g, Lkeep, dpool, x, x32, sx, gamma, mean, rstd, dx, dgamma, dbeta, accumulate, ws, d):
    """backward of ln_pool2_fwd for one modality; dgamma / dbeta None: the partial sums stay in ws (deferred reduce)"""
    _lib.call("hriemo_ln_pool_vec_bwd", _p(g), Lkeep, _p(dpool), _p(sx.kpm), _p(x), _p(x32), _p(gamma), _p(mean), _p(rstd), _p(dx),
              _p(dgamma), _p(dbeta), accumulate, sx.B, sx.L, d, _p(ws), _stream())


def ln_pool_vec_bwd_pair(Lkeep, a, t, accumulate, d):
    """ln_pool_vec_bwd of both modalities from one launch; a / t = (ws, g, dpool, x, x32, sx, gamma, mean, rstd, dx, dgamma, dbeta)"""
    side = lambda ws, g, dpool, x, x32, sx, *rest: (_p(g), _p(dpool), _p(sx.kpm), _p(x), _p(x32), *map(_p, rest), sx.L, _p(ws))  # noqa: E731
    _lib.call("hriemo_ln_pool_vec_bwd_pair", Lkeep, *side(*a), *side(*t), accumulate, a[5].B, d, _stream())


class PooledGateFn(_GradModeAware, torch.autograd.Function):
    """(pooled fp32 [B, d], beta [B, 1]) = mean over the L fused positions of BetaGate(h_a, h_t, masks)'s h_fusion
    -- models/fusion_classifier.py:142-145 on the PADDED pairs (sa / st: padded Seq with the key-padding masks).
    pooled = w * Abar + (1 - w) * Tbar with Abar / Tbar the unmasked means of the LayerNorm outputs over l < L (PAD rows included, as
    the reference's h_fusion.mean(dim=1)); the gate weights come from _gate_weights, the code of the vector gate.  Neither the
    LayerNorm outputs, h_fusion nor a [B, L, d] gradient of it is formed."""

    @staticmethod
    def forward(ctx, h_a, h_a32, h_t, h_t32, ga, ba, gt, bt, w1, b1, w2, b2, sh, sa, st):
        if sa.packed or st.packed:
            raise ValueError("PooledGate: the pooled mean includes PAD rows -- padded layouts only")
        _require_pooled_path("PooledGate")
        B, La, Lt, d = sa.Breal, sa.L, st.L, h_a.shape[-1]
        sa.holds(h_a)
        st.holds(h_t)
        _gate_align(La, Lt)                  # the refusal comes before the fp32 dispatch, as in BetaGateFn
        if precision() == "fp32":           # -> (pooled fp32, beta)
            return _fp32().pooled_gate(ctx, h_a, h_a32, h_t, h_t32, ga, ba, gt, bt, w1, b1, w2, b2, sh, sa, st)
        L, xa, h_a32, xt, h_t32, (mean_a, rstd_a, pa), (mean_t, rstd_t, pt) = _gate_prologue(h_a, h_a32, h_t, h_t32,
                                                                                              (ga, ba, gt, bt, w1, b1, w2, b2), sa, st)
        dev = h_a.device
        f32 = dict(dtype=torch.float32, device=dev)
        ka, kt = torch.empty_like(pa), torch.empty_like(pt)
        _both_sides(d, dev, lambda a, t: ln_pool2_fwd_pair(a, t, L, d), lambda *s: ln_pool2_fwd(*s, L, d),
                    (xa, h_a32, sa, ga, ba, mean_a, rstd_a, pa, ka), (xt, h_t32, st, gt, bt, mean_t, rstd_t, pt, kt))
        gin, a_pool, t_pool, cnt, hid, w, beta, w1_16, w2_16 = _gate_weights(pa, pt, sa, st, B, La, Lt, d, w1, b1, w2, b2, sh)
        abar, tbar, pooled = torch.empty((B, d), **f32), torch.empty((B, d), **f32), torch.empty((B, d), **f32)
        _lib.call("hriemo_pooled_fuse_fwd", _p(ka), La, _p(kt), Lt, _p(w), L, _p(abar), _p(tbar), _p(pooled), B, d, _stream())
        ctx.save_for_backward(xa, xt, mean_a, rstd_a, mean_t, rstd_t, gin, a_pool, t_pool, cnt, hid, w, w1_16, w2_16, ga, gt,
                              h_a32, h_t32, abar, tbar)
        ctx.seqs = (sa, st)
        ctx.params = (ga, ba, gt, bt, w1, b1, w2, b2)
        return pooled, beta

    @staticmethod
    def backward(ctx, dpooled, dbeta):
        if getattr(ctx, "fp32", False):
            return _fp32().pooled_gate_bwd(ctx, dpooled, dbeta)
        (xa, xt, mean_a, rstd_a, mean_t, rstd_t, gin, a_pool, t_pool, cnt, hid, w, w1_16, w2_16, ga, gt, h_a32, h_t32,
         abar, tbar) = ctx.saved_tensors
        sa, st = ctx.seqs
        B, La, Lt, L, d = sa.Breal, sa.L, st.L, st.L, xa.shape[-1]
        dev = xa.device
        f32 = dict(dtype=torch.float32, device=dev)
        p_ga, p_ba, p_gt, p_bt, p_w1, p_b1, p_w2, p_b2 = ctx.params
        sink = GradSink(ctx.params)
        dpooled2 = dpooled.contiguous().float() if dpooled is not None else None
        dbeta2 = dbeta.contiguous().float() if dbeta is not None else None
        dwf, g_a, g_t = torch.empty((B, d), **f32), torch.empty((B, d), **f32), torch.empty((B, d), **f32)
        _lib.call("hriemo_pooled_fuse_bwd", _p(dpooled2), _p(abar), _p(tbar), _p(w), L, _p(dwf), _p(g_a), _p(g_t), B, d, _stream())
        # (dwf: ONE chunk of dw partials, [B, 1, d])
        da, dt, dw1, db1, dw2, db2 = _gate_weights_bwd(dwf, 1, dbeta2, w, hid, gin, a_pool, t_pool, cnt, w1_16, w2_16, sink,
                                                       (p_w1, p_b1, p_w2, p_b2), B, d)
        dxa = torch.empty(sa.shape(d), dtype=BF16, device=dev)
        dxt = torch.empty(st.shape(d), dtype=BF16, device=dev)
        dga, dba, dgt, dbt = sink.buf(p_ga), sink.buf(p_ba), sink.buf(p_gt), sink.buf(p_bt)
        aff = _LnAffine(sink, (dga, dba, dgt, dbt), B, La, Lt, d, dev)
        ws = aff.workspaces()
        _both_sides(d, dev,
                    lambda a, t: ln_pool_vec_bwd_pair(L, (ws[0],) + a[1:] + aff.outs[:2], (ws[1],) + t[1:] + aff.outs[2:], aff.acc, d),
                    lambda text, g, *rest: ln_pool_vec_bwd(g, L, *rest, *aff.outs[2 * text:2 * text + 2], aff.acc, ws[text], d),
                    (0, g_a, da, xa, h_a32, sa, ga, mean_a, rstd_a, dxa), (1, g_t, dt, xt, h_t32, st, gt, mean_t, rstd_t, dxt))
        aff.queue(ws[0], 0)
        aff.queue(ws[1], 1)
        sink.done()
        r = sink.ret
        return dxa, None, dxt, None, r(dga), r(dba), r(dgt), r(dbt), r(dw1), r(db1), r(dw2), r(db2), None, None, None


class DropoutF32Fn(torch.autograd.Function):
    """y = drop(x) on fp32 [M, N] rows by the counter hash (hriemo_dropout_f32): the classifier head's Dropout as a hash site -- it
    follows the device seed word inside a captured step, and tests/hashrng.py rebuilds its mask.  Backward: the same keep / (1 - p)."""

    @staticmethod
    def forward(ctx, x, p, seed, site, row_off):
        _require_gpu(x)
        x = x.contiguous()
        M, N = x.shape
        if DROP_LOG is not None and p > 0:
            DROP_LOG.append(("rows", seed, site, M, N, float(p), row_off))
        y = torch.empty_like(x)
        _lib.call("hriemo_dropout_f32", _p(x), _p(y), M, N, 0, None, float(p), seed, _p(seed_word(x.device)), site, row_off, _stream())
        ctx.drop = (float(p), seed, site, row_off)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed, site, row_off = ctx.drop
        dy = dy.contiguous().float()
        M, N = dy.shape
        dx = torch.empty_like(dy)
        _lib.call("hriemo_dropout_f32", _p(dy), _p(dx), M, N, 0, None, p, seed, _p(seed_word(dy.device)), site, row_off, _stream())
        return dx, None, None, None, None


def _n_valid_word(n_valid, like):
    """the optional trailing argument of the loss Functions -> one int32 word on `like`'s device, or None"""
    if not n_valid or n_valid[0] is None:
        return None
    nv = n_valid[0]
    if not (isinstance(nv, torch.Tensor) and nv.dtype == torch.int32 and nv.numel() == 1 and nv.device == like.device):
        raise TypeError("n_valid is a 0-dim or 1-element int32 tensor on the logits' device (the count is device data: a captured "
                        f"step reads it on every replay), got {nv!r}")
    return nv


class FusionLossFn(torch.autograd.Function):
    """Trainer loss with its gradients from ONE kernel (hriemo_fusion_loss): mean BCEWithLogits(logits, targets; pos_weight) +
    reg(beta).  reg_mode 1 = -coef*mean(beta(1-beta)) (train_fusion_seq_level_decoder.py:318-326), 2 = +coef*entropy(beta)
    (train_mosei_fusion_seq_level_decoder.py:340-347,385-386); `scale` = 1/grad_accum (:387).  An eighth argument n_valid (one int32
    on the device) routes to hriemo_fusion_loss_n: only the first n_valid samples count, the others get zero gradients."""

    @staticmethod
    def forward(ctx, logits, beta, targets, pos_weight, reg_mode, reg_coef, scale, *n_valid):
        _require_gpu(logits)
        nv = _n_valid_word(n_valid, logits)
        ctx.n_extra = len(n_valid)
        B, Ne = logits.shape
        x, y = logits.contiguous().float(), targets.contiguous().float()
        bt = beta.contiguous().float().view(B) if beta is not None else None
        pw = pos_weight.contiguous().float() if pos_weight is not None else None
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dx = torch.empty((B, Ne), dtype=torch.float32, device=x.device)
        db = torch.empty(B, dtype=torch.float32, device=x.device) if bt is not None else None
        if nv is None:
            _lib.call("hriemo_fusion_loss", _p(x), _p(y), _p(pw), _p(bt), B, Ne, int(reg_mode) if bt is not None else 0, float(reg_coef),
                      float(scale), _p(loss), _p(dx), _p(db), _stream())
        else:
            _lib.call("hriemo_fusion_loss_n", _p(x), _p(y), _p(pw), _p(bt), B, Ne, int(reg_mode) if bt is not None else 0, float(reg_coef),
                      float(scale), _p(loss), _p(dx), _p(db), _p(nv), _stream())
        ctx.save_for_backward(dx, db)
        ctx.shapes = (logits.shape, beta.shape if beta is not None else None, logits.dtype, beta.dtype if beta is not None else None)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        dx, db = ctx.saved_tensors
        ls, bs, ld, bd = ctx.shapes
        rest = (None,) * (5 + ctx.n_extra)
        if _is_one(g):                       # loss.backward(gradient=_ops.one(device)): the kernel's gradients are the answer
            return (dx.to(ld).view(ls), (db.to(bd).view(bs) if db is not None else None)) + rest
        gl = (dx * g).to(ld).view(ls)
        gb = (db * g).to(bd).view(bs) if db is not None else None
        return (gl, gb) + rest


class FusionLossCEFn(torch.autograd.Function):
    """Single-label trainer loss (train_fusion_seq_level_decoder.py:312-314,325-326,413-414): CrossEntropyLoss(logits, labels) +
    reg(beta), value and gradients from ONE kernel (hriemo_fusion_loss_ce; with a seventh argument n_valid, hriemo_fusion_loss_ce_n)."""

    @staticmethod
    def forward(ctx, logits, beta, labels, reg_mode, reg_coef, scale, *n_valid):
        _require_gpu(logits)
        nv = _n_valid_word(n_valid, logits)
        ctx.n_extra = len(n_valid)
        B, C = logits.shape
        x = logits.contiguous().float()
        lb = labels.contiguous().to(torch.int64)
        bt = beta.contiguous().float().view(B) if beta is not None else None
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dx = torch.empty((B, C), dtype=torch.float32, device=x.device)
        db = torch.empty(B, dtype=torch.float32, device=x.device) if bt is not None else None
        if nv is None:
            _lib.call("hriemo_fusion_loss_ce", _p(x), _p(lb), _p(bt), B, C, int(reg_mode) if bt is not None else 0, float(reg_coef),
                      float(scale), _p(loss), _p(dx), _p(db), _stream())
        else:
            _lib.call("hriemo_fusion_loss_ce_n", _p(x), _p(lb), _p(bt), B, C, int(reg_mode) if bt is not None else 0, float(reg_coef),
                      float(scale), _p(loss), _p(dx), _p(db), _p(nv), _stream())
        ctx.save_for_backward(dx, db)
        ctx.shapes = (logits.shape, beta.shape if beta is not None else None, logits.dtype, beta.dtype if beta is not None else None)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        dx, db = ctx.saved_tensors
        ls, bs, ld, bd = ctx.shapes
        rest = (None,) * (4 + ctx.n_extra)
        if _is_one(g):
            return (dx.to(ld).view(ls), (db.to(bd).view(bs) if db is not None else None)) + rest
        gl = (dx * g).to(ld).view(ls)
        gb = (db * g).to(bd).view(bs) if db is not None else None
        return (gl, gb) + rest


class LinearFn(_GradModeAware, torch.autograd.Function):
    """y[..., N] (fp32) = x[..., K] . W[N,K]^T + b for any K (MOSEI projections: K = 74 / 300, padded to a
    multiple of 8 internally) -- models/mosei_fusion_with_emotion_decoder.py:41-42,63-65."""

    @staticmethod
    def forward(ctx, x, w, b, sh):
        if precision() == "fp32":
            return _fp32().linear_any_k(ctx, x, w, b, sh)
        _require_fp32_masters(w, b)
        _require_gpu(x)
        K = x.shape[-1]
        N = w.shape[0]
        M = x.numel() // K
        kp = (K + 7) // 8 * 8
        xb = torch.zeros((M, kp), dtype=BF16, device=x.device)
        xb[:, :K].copy_(x.reshape(M, K))
        w16 = padded_shadow(sh, w, kp)
        y = linear_fwd(xb, w16, b, out_f32=True)
        ctx.save_for_backward(xb, w16)
        ctx.cfg = (tuple(x.shape), x.dtype, K, N, M, kp)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        if getattr(ctx, "fp32", False):
            return _fp32().linear_any_k_bwd(ctx, dy)
        xb, w16 = ctx.saved_tensors
        shape, xdtype, K, N, M, kp = ctx.cfg
        dyb = dy.reshape(M, N).to(BF16).contiguous()
        dx = linear_dx(dyb, w16)[:, :K].to(xdtype).reshape(shape) if ctx.needs_input_grad[0] else None
        dwp = torch.empty((N, kp), dtype=torch.float32, device=dyb.device)
        linear_dw(dyb, xb, dwp)
        db = torch.empty(N, dtype=torch.float32, device=dyb.device)
        colsum(dyb, db)
        return dx, dwp[:, :K].contiguous(), db, None


class ExpandFn(_GradModeAware, torch.autograd.Function):
    """queries[N_e,d] -> [B,N_e,d] bf16   (models/emotion_decoder.py:127)"""

    @staticmethod
    def forward(ctx, q, B, twin=False):
        """twin: also return the fp32 copy [B,N_e,d] (the residual twin of the first decoder layer; not differentiable)"""
        _require_gpu(q)
        Ne, d = q.shape
        out = torch.empty((B, Ne, d), dtype=BF16, device=q.device)
        out32 = torch.empty((B, Ne, d), dtype=torch.float32, device=q.device) if twin else None
        src = q.detach().float().contiguous()
        _lib.call("hriemo_expand_rows", _p(src), _p(out), _p(out32), B, Ne * d, _stream())
        ctx.cfg = (B, Ne, d)
        ctx.params = (q,)
        ctx.fp32 = precision() == "fp32"      # fp32 mode: the decoder reads the fp32 copy and its gradient comes back through it
        if ctx.fp32:
            ctx.set_materialize_grads(False)
        if twin:
            if not ctx.fp32:
                ctx.mark_non_differentiable(out32)
            return out, out32
        return out

    @staticmethod
    def backward(ctx, dout, _d32=None):
        B, Ne, d = ctx.cfg
        if ctx.fp32:
            return _fp32().expand_bwd(dout, _d32, B, Ne, d, ctx.params[0]), None, None
        g = _contig_bf16(dout).view(B, Ne * d)
        sink = GradSink(ctx.params)
        dq = sink.buf(ctx.params[0])
        colsum(g, dq.view(Ne * d), sink.fused)
        sink.done(after_flush=ctx.params)
        return sink.ret(dq), None, None


class RowDotFn(_GradModeAware, torch.autograd.Function):
    """logits[M] = z[M,d] . w[1,d] + b   (models/emotion_decoder.py:155)"""

    @staticmethod
    def forward(ctx, z, z32, w, b):
        _require_fp32_masters(w, b)
        _require_gpu(z)
        B, Ne, d = z.shape
        z2 = _contig_bf16(z).view(B * Ne, d)
        z32 = _c32(z32)
        z32v = z32.view(B * Ne, d) if z32 is not None else None
        wf = w.detach().float().contiguous()
        bf = b.detach().float().contiguous()
        out = torch.empty(B * Ne, dtype=torch.float32, device=z.device)
        _lib.call("hriemo_rowdot_fwd", _p(z2), _p(z32v), _p(wf), _p(bf), _p(out), B * Ne, d, _stream())
        if CTX.act_log is not None:
            probe("logits", 0, out.view(B, Ne), Seq.padded(B, 1))
        ctx.save_for_backward(z2, z32v, wf)
        ctx.cfg = (B, Ne, d)
        ctx.params = (w, b)
        ctx.fp32 = precision() == "fp32" and z32v is not None
        return out.view(B, Ne)

    @staticmethod
    def backward(ctx, dl):
        z2, z32v, wf = ctx.saved_tensors
        B, Ne, d = ctx.cfg
        if ctx.fp32:                            # gradient of z in fp32, through the fp32 slot
            dz32, dw, db = _fp32().rowdot_bwd(dl, z32v, wf, B, Ne, d)
            return None, dz32, dw.view_as(ctx.params[0]), db.view_as(ctx.params[1])
        dl2 = dl.contiguous().float().view(-1)
        if CTX.act_log is not None:
            probe("logits", 1, dl2.view(B, Ne), Seq.padded(B, 1))
        dz = torch.empty((B * Ne, d), dtype=BF16, device=z2.device)
        sink = GradSink(ctx.params)
        dw, db = sink.buf(ctx.params[0]), sink.buf(ctx.params[1])
        _lib.call("hriemo_rowdot_bwd", _p(dl2), _p(z2), _p(z32v), _p(wf), _p(dz), _p(dw), _p(db), int(sink.fused), B * Ne, d, _stream())
        sink.done()
        return dz.view(B, Ne, d), None, sink.ret(dw), sink.ret(db)
