"""Data-parallel driver for the fusion path: one process per GPU, utterances sharded contiguously across
ranks, ONE exchange step per iteration -- a sum/avg all-reduce of the parameter gradients (RCCL over xGMI
when the backend is "nccl"; gloo on CPU for tests).  The reference has no distributed code;
the contract here is "N-rank step on shards == 1-rank step on the concatenated batch".

MI355X-first layout: every parameter gradient is a VIEW into one flat fp32 buffer, ordered in reverse
parameter order (the order backward produces them: decoder first, fusion layer 0 last).  Buckets are
contiguous slices of that buffer, so a bucket is all-reduced in place -- no flatten/unflatten copies -- and
is launched from a post-accumulate-grad hook as soon as its last gradient has been written, overlapping the
collective with the rest of backward.  xGMI is point-to-point (7 links x ~153 GB/s), so few large buckets
(default 32 MiB) beat many small ones.
"""
import collections
import itertools
import logging
import os

import torch
import torch.distributed as dist

log = logging.getLogger("hri_emo_amd.dp")

# packed (varlen) graphs: the packed row count of a modality is rounded up to a multiple of (padded rows / this): finer = fewer
# wasted rows, more distinct graphs over a run (DataParallelStep.capture)
_VARLEN_BUCKETS = max(1, int(os.environ.get("HRIEMO_VARLEN_BUCKETS", "64")))
# packed (varlen) graphs kept alive per captured step: one hipGraph + the buffers its kernels point into per distinct
# (audio rows, text rows) bucket pair; beyond the cap the least recently replayed one is released (and re-captured if it returns)
_VARLEN_MAX_GRAPHS = max(1, int(os.environ.get("HRIEMO_VARLEN_MAX_GRAPHS", "48")))


def bucket_rows(n, B, L):
    """Row count of the packed (varlen) bucket that holds `n` valid rows of a modality padded to [B, L]: the next multiple of the
    granule g = max(8, B*L / _VARLEN_BUCKETS rounded down to a multiple of 8), g capped at L -- always > n (the surplus rows form
    ONE extra sequence, which is never empty and never longer than L).  The one place this arithmetic lives: packed_tables, which
    the mask-fed (_packed_key) and the ragged (step_packed) front doors of DataParallelStep share, is built on it."""
    g = max(8, (B * L) // _VARLEN_BUCKETS // 8 * 8)
    g = min(g, L)                         # the surplus rows are ONE sequence of at most L rows
    return (n // g + 1) * g               # > n: the extra sequence is never empty


def packed_tables(la, lt, B, La, Lt):
    """Host arithmetic of a packed batch, lists in and lists out: the lengths of B utterances per modality, padded to [B, La] / [B, Lt]
    -> (bucket key, cu_a, cu_t, cu_f).  key = (audio rows, text rows) of the bucket (bucket_rows); every cu is
    [0, inclusive prefix sums ..., bucket row count], B + 2 entries: the surplus rows are the last sequence.  cu_f is the fused memory
    of the packed tail (min of the two lengths per utterance: the reference ORs the two prefix masks); it rides in the text bucket
    (sum lf <= sum lt < its row count): no bucket dimension, no graph of its own."""
    key = (bucket_rows(sum(la), B, La), bucket_rows(sum(lt), B, Lt))
    cu = lambda lens, rows: list(itertools.accumulate(lens, initial=0)) + [rows]          # noqa: E731
    return key, cu(la, key[0]), cu(lt, key[1]), cu([min(x, y) for x, y in zip(la, lt)], key[1])


def mask_lengths(m_a, m_t, lengths, B, La, Lt):
    """-> (audio lengths, text lengths) as host lists: `lengths` checked, or read from the padding masks (one device -> host read;
    the masks must be prefix masks with no empty sequence, the collate's form)"""
    if lengths is not None:
        la, lt = [int(x) for x in lengths[0]], [int(x) for x in lengths[1]]
        if len(la) != B or len(lt) != B or min(la) < 1 or min(lt) < 1 or max(la) > La or max(lt) > Lt:
            raise ValueError("DataParallelStep (packed mode): lengths must hold one value in [1, L] per utterance and modality")
        return la, lt
    va, vt = ~m_a.bool(), ~m_t.bool()
    la, lt = va.sum(1), vt.sum(1)
    ok = ((va == (torch.arange(La, device=m_a.device)[None, :] < la[:, None])).all()
          & (vt == (torch.arange(Lt, device=m_t.device)[None, :] < lt[:, None])).all() & (la > 0).all() & (lt > 0).all())
    host = torch.cat([la, lt, ok.long().view(1)]).tolist()
    if not host[-1]:
        raise RuntimeError("DataParallelStep (packed mode): padding masks must mark a suffix of every row and leave at least "
                           "one valid position -- use_graph(False) runs such a batch on the padded path")
    return host[:B], host[B:2 * B]


def ghost_plan(la, lt, B, La, Lt):
    """A short batch of n = len(la) <= B utterances, as a captured step of B utterances sees it (capture_packed(partial_batches=True)):
    -> (audio lengths, text lengths, bucket key, (own audio rows, own text rows)).  The B - n missing utterances are ghosts of length
    1 in both modalities -- the shortest sequence every kernel of the step accepts; their rows lie directly behind the batch's own
    rows, inside the region _load_ragged's fill zeroes up to the bucket's end, and the bucket key counts them.  n == B: the batch itself."""
    own = (sum(la), sum(lt))
    ghosts = [1] * (B - len(la))
    la, lt = list(la) + ghosts, list(lt) + ghosts
    return la, lt, packed_tables(la, lt, B, La, Lt)[0], own


def ctl_words(n_valid, first, last):
    """host image of the step-control block a captured step reads from device memory: int32 {n_valid, first, last, spare}"""
    return [int(n_valid), 1 if first else 0, 1 if last else 0, 0]


def micro_flags(micro, k):
    """(first, last) of micro-step `micro` in an accumulation group of k: the flat gradient buffer starts from zero on the first,
    the optimizer (and the exchange outside the graph) runs on the last"""
    return micro == 0, micro == k - 1


def _accepts_n_valid(fn):
    import inspect
    try:
        params = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        return False
    return any(p.name == "n_valid" or p.kind is inspect.Parameter.VAR_KEYWORD for p in params)


class GradBuckets:
    """comm_dtype: torch.float32 (default: the flat buffer is all-reduced in place) or torch.bfloat16: every bucket is cast to a
    bf16 staging buffer (half the bytes on the xGMI links: 109 MB instead of 218 MB per step at cfg 2), summed by the collective in
    bf16 and cast back into the fp32 flat buffer (the 1/N average is applied in fp32).  A bf16 sum over N <= 8 ranks adds
    ~2^-9 relative rounding per addition on top of the bf16 backward that produced the gradients."""

    def __init__(self, params, bucket_bytes=32 << 20, group=None, overlap=True, comm_dtype=torch.float32, force_exchange=False,
                 launch_from="notify"):
        """force_exchange: install the hooks and run the collectives at world size 1 too (a one-rank all-reduce is the identity:
        rehearses the exchange -- also captured inside a hipGraph -- on a one-GPU box)
        launch_from: the stream an EAGER step launches a bucket's collective from -- "notify": the stream the gradient-ready
        notification came in on (it first waits for the other branch stream); "main": always the model's main stream (which first
        waits for the notifying one and the side stream).  A captured step always uses the capture's origin stream."""
        if launch_from not in ("notify", "main"):
            raise ValueError("GradBuckets: launch_from is 'notify' or 'main'")
        self.launch_from = launch_from
        self._snap = None           # test hook (enable_launch_snapshots): the flat buffer as every collective saw it at launch
        self.params = [p for p in params if p.requires_grad]
        self.force_exchange = bool(force_exchange) and dist.is_initialized()
        self.group = group
        self.comm_dtype = comm_dtype
        self._stage = None
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # matrices first, in the order backward produces them (decoder first, fusion layer 0 last); every vector
        # parameter (biases, LayerNorm gain/bias) behind them: their gradients are finished by the launch-boundary
        # reduce at the END of backward (_ops._DeferredReduce), so they share the last bucket(s) and the matrix
        # buckets can be all-reduced while backward is still running
        rev = list(reversed(self.params))
        order = [p for p in rev if p.dim() >= 2] + [p for p in rev if p.dim() < 2]
        pad = lambda n: (n + 63) // 64 * 64          # every view starts 256-B aligned (16-B vector stores)
        total = sum(pad(p.numel()) for p in order)
        dev = order[0].device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.buckets = []           # (start, end, n_params)
        self._bucket_of = {}
        self._offsets = {}
        off, b_start, b_n = 0, 0, 0
        for p in order:
            n = p.numel()
            p.grad = self.flat[off:off + n].view_as(p)
            p._hriemo_fused_grad = True          # the kernels may accumulate straight into this view (_ops.GradSink)
            self._offsets[id(p)] = off
            self._bucket_of[id(p)] = len(self.buckets)
            off += pad(n)
            b_n += 1
            if (off - b_start) * 4 >= bucket_bytes:
                self.buckets.append((b_start, off, b_n))
                b_start, b_n = off, 0
        if b_n:
            self.buckets.append((b_start, off, b_n))
        self._pending = [0] * len(self.buckets)
        self._launched = [False] * len(self.buckets)
        self._reported = set()
        self.suspended = False      # True: gradient-ready notifications are ignored (rank-local diagnostic steps: no collectives)
        self._works = []
        self._hooks = []
        self._predicate = None
        if overlap and (self.world > 1 or self.force_exchange):
            from . import _ops
            # an overlapped exchange wants gradients in production order; one predicate per GradBuckets (a second instance --
            # an eval or EMA wrapper -- must not switch the first one's deferral of small weight-gradient GEMMs on or off)
            self._predicate = _ops.register_hook_predicate(lambda: bool(self._hooks) and not self.suspended)
            for p in self.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad))
                p._hriemo_grad_ready = self._on_grad_sink     # gradients the kernels accumulate in place (_ops.GradSink)

    def close(self):
        """remove the gradient-ready hooks and this instance's predicate (the parameters keep their flat-buffer views)"""
        from . import _ops
        for h in self._hooks:
            h.remove()
        self._hooks = []
        if self._predicate is not None:
            _ops.unregister_hook_predicate(self._predicate)
            self._predicate = None
        for p in self.params:
            if getattr(p, "_hriemo_grad_ready", None) == self._on_grad_sink:
                del p._hriemo_grad_ready

    # -- test hook: is every collective launched behind the kernels that produce its bucket? ------------
    def enable_launch_snapshots(self, on=True):
        """Test hook.  While enabled, every bucket is copied to a side buffer at the exact point its collective
        is enqueued -- on the launching stream, in front of the all-reduce, eager and inside a capture alike.  At world size 1
        the all-reduce is the identity, so after the step the side buffer must equal the flat gradient buffer bit for bit; a
        collective launched before one of its gradients was produced leaves the words that were written later different
        (``launch_snapshot_mismatches``).  That makes the ORDERING of the exchange testable on one GPU, which the values of a
        one-rank exchange alone are not.  fp32 buckets only.  Enable BEFORE capture() to have the copies recorded in the graph."""
        if on and self.comm_dtype != torch.float32:
            raise ValueError("launch snapshots compare fp32 buckets")
        self._snap = torch.zeros_like(self.flat) if on else None

    def launch_snapshot_mismatches(self):
        """after a finished step at world size 1 -> [(bucket, words that differ, first differing word's parameter name or index)];
        empty = every collective saw the final gradients of its bucket"""
        if self._snap is None:
            raise RuntimeError("enable_launch_snapshots() first")
        if self.world != 1:
            raise RuntimeError("launch snapshots are compared at world size 1 (the all-reduce must be the identity)")
        out = []
        for bi, (s, e, _) in enumerate(self.buckets):
            a, b = self._snap[s:e], self.flat[s:e]
            ne = (a != b) & ~(torch.isnan(a) & torch.isnan(b))
            n = int(ne.sum())
            if n:
                first = s + int(ne.nonzero()[0])
                owner = next((i for i, p in enumerate(self.params)
                              if self._offsets[id(p)] <= first < self._offsets[id(p)] + p.numel()), None)
                out.append((bi, n, owner))
        return out

    # -- hooks ---------------------------------------------------------------------------------
    def _launch(self, bi):
        s, e, _ = self.buckets[bi]
        self._launched[bi] = True
        ctx = None
        if self.flat.is_cuda:
            # a bucket holds gradients written on both branch streams: the collective is ordered after the launching stream
            # only, so that stream first waits for the other one.  Eager steps launch from the stream the gradient-ready
            # notification came in on.  (Round 3 also tried "always from the main stream, which first waits for the notifying
            # one"; in the two-rank rehearsal over gloo that form sporadically sent a bucket out with a wrong half of an
            # in-projection gradient -- scripts_dev/dbg_dp_overlap.py.  The experiment predates the fix of the SharedGrad
            # first-touch race (_ops.SharedGrad) and may have been that fault; the form measured correct stays for eager steps.)
            # Inside a capture the launch MUST come from the capture's origin stream: the
            # process group forks its communication stream from the launching one, and a fork off the side stream would be a
            # fork nested in a fork (_ops.fork; hipStreamEndCapture crashes on those).
            from . import _ops
            streams = _ops.branch_streams(self.flat.device)
            cur = torch.cuda.current_stream(self.flat.device)
            capturing = _ops.CTX.capturing and _ops.CTX.capture_origin is not None
            if capturing or self.launch_from == "main":
                main = _ops.CTX.capture_origin if capturing else streams[0]
                for st in streams:
                    if st != main:
                        main.wait_stream(st)
                if cur != main:
                    main.wait_stream(cur)
                    ctx = torch.cuda.stream(main)
                    ctx.__enter__()
            else:
                for st in streams:
                    if st != cur:
                        cur.wait_stream(st)
        try:
            if self._snap is not None:
                # what the collective is about to read, copied on the launching stream directly in front of it: a launch that
                # precedes the production of one of the bucket's gradients shows as a difference to the final buffer
                self._snap[s:e].copy_(self.flat[s:e])
            if self.comm_dtype == torch.float32:
                self._works.append((dist.all_reduce(self.flat[s:e], op=dist.ReduceOp.SUM, group=self.group, async_op=True), None))
            else:
                if self._stage is None:
                    self._stage = torch.empty(self.flat.numel(), dtype=self.comm_dtype, device=self.flat.device)
                st = self._stage[s:e]
                st.copy_(self.flat[s:e])                    # fp32 -> bf16 on the launching stream, ordered before the collective
                self._works.append((dist.all_reduce(st, op=dist.ReduceOp.SUM, group=self.group, async_op=True), (s, e)))
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)

    def _on_grad(self, p, from_sink=False):
        """gradient of `p` is final.  Sources: autograd's post-accumulate hook (gradients returned as tensors) and
        _ops.GradSink (gradients the kernels wrote in place).  While a parameter is sink-managed in this backward pass
        only the sink's notification counts -- it comes after the producing kernels were issued, for bias / LayerNorm
        vectors after the launch-boundary reduce -- and every parameter counts once per step."""
        if self.suspended or (getattr(p, "_hriemo_sink_managed", False) and not from_sink) or id(p) in self._reported:
            return
        self._reported.add(id(p))
        bi = self._bucket_of[id(p)]
        self._pending[bi] += 1
        if self._pending[bi] == self.buckets[bi][2] and not self._launched[bi]:
            self._launch(bi)

    def _on_grad_sink(self, p):
        self._on_grad(p, from_sink=True)

    # -- per-step API --------------------------------------------------------------------------
    def _rebind(self):
        for p in self.params:
            off, n = self._offsets[id(p)], p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat.data_ptr() + off * 4:
                p.grad = self.flat[off:off + n].view_as(p)

    def zero_grad(self):
        self.flat.zero_()
        self._rebind()                   # keep the views even if someone set grads to None

    def finish(self):
        """Complete the gradient exchange of this step and average over ranks."""
        if self.world > 1 or self.force_exchange:
            for bi in range(len(self.buckets)):
                if not self._launched[bi]:          # no hooks, or a parameter got no gradient this step
                    self._launch(bi)
            for w, rng in self._works:
                w.wait()
                if rng is not None:                     # summed bf16 bucket back into the fp32 flat buffer
                    self.flat[rng[0]:rng[1]].copy_(self._stage[rng[0]:rng[1]])
            self._works = []
            self._pending = [0] * len(self.buckets)
            self._launched = [False] * len(self.buckets)
            self._reported = set()
            for p in self.params:
                p._hriemo_sink_managed = False
            if self.world > 1:
                self.flat.mul_(1.0 / self.world)

    def grad_norm(self):
        return self.flat.norm()


def shard_bounds(global_batch, rank, world):
    """Contiguous shard [lo, hi) of rank `rank` (rank r gets utterances [r*B/W, (r+1)*B/W))."""
    if global_batch % world != 0:
        raise ValueError(f"global batch {global_batch} is not divisible by world size {world}")
    per = global_batch // world
    return rank * per, (rank + 1) * per


def _in_step_context(fn):
    """run a DataParallelStep method with the step's own _ops.StepContext in force"""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        from . import _ops
        with _ops.use_context(self.ctx):
            return fn(self, *a, **k)
    return wrapper


class _GraphRecord:
    """One captured graph and what lives exactly as long as it: the loss tensor its replay writes, the buffers its kernels point
    into (column-sum partials, queued weight-gradient operands), the packed plans of a bucket graph (None: the plain step), the
    output tensors of a captured evaluation (EvalStep; None for a trainer step).  A record has ONE owner -- DataParallelStep._record
    or a _PackedState.graphs entry -- and dies through release()."""
    __slots__ = ("graph", "loss", "keep", "seqs", "out")

    def __init__(self, graph, loss, keep, seqs=None, out=None):
        self.graph, self.loss, self.keep, self.seqs, self.out = graph, loss, keep, seqs, out

    def release(self):
        """the one way down for _ops.GRAPHS_ALIVE (the way up: _record_graph); the caller has synchronized the device"""
        from . import _ops
        self.graph = self.loss = self.keep = self.seqs = self.out = None
        _ops.GRAPHS_ALIVE -= 1
        if _ops.GRAPHS_ALIVE == 0:
            del _ops._ws_retired[:]   # no graph points into the outgrown workspaces any more


class _HostBlock:
    """a small int32 block a captured step reads from device memory (`dev`) and its host twin (`host`, pinned beside a GPU)"""
    __slots__ = ("dev", "host", "copied")

    def __init__(self, values, device):
        self.dev = torch.tensor(values, dtype=torch.int32, device=device)
        self.host = torch.tensor(values, dtype=torch.int32, pin_memory=self.dev.is_cuda)
        self.copied = None           # event behind the latest upload: until it has passed the twin is still being read

    def upload(self, values):
        """values -> twin -> device, in stream order"""
        if self.copied is not None:
            self.copied.synchronize()         # the previous upload has left the pinned twin
        self.host.copy_(torch.tensor(values, dtype=torch.int32))
        self.dev.copy_(self.host, non_blocking=True)
        self.copied = torch.cuda.Event()
        self.copied.record()


class _RaggedFront:
    """what capture_packed adds in front of the packed step: the lengths as one [2, B] block, the three mask buffers
    hriemo_seq_tables fills (uint8, and the same memory as bool), and the step-control block {n_valid, first, last, spare} --
    None unless the step was captured with partial_batches or grad_accum > 1"""
    __slots__ = ("lens", "masks", "bool", "same_width", "partial", "accum", "ctl")

    def __init__(self, lens, masks, same_width, partial=False, accum=1, ctl=None):
        self.lens, self.masks, self.bool = lens, masks, tuple(m.view(torch.bool) for m in masks)
        self.same_width, self.partial, self.accum, self.ctl = same_width, bool(partial), int(accum), ctl


# the mask-fed packed step's memory of its last batch: the identity of the mask tensors, their bucket key and cu_seqlens, the masks
_MaskSeen = collections.namedtuple("_MaskSeen", "ident key cu masks")


class _PackedState:
    """a step captured in packed (varlen) mode: the baked-in shapes, the three cu_seqlens buffers every bucket graph reads, the
    bucket graphs {(rows audio, rows text): _GraphRecord} in LRU order with their one memory pool, and the ragged front door
    (capture_packed) or None (mask-fed, capture)"""
    __slots__ = ("B", "La", "Lt", "cu_a", "cu_t", "cu_f", "graphs", "pool", "front")

    def __init__(self, B, La, Lt, device, front=None):
        self.B, self.La, self.Lt, self.front = B, La, Lt, front
        self.cu_a, self.cu_t, self.cu_f = (torch.zeros(B + 2, dtype=torch.int32, device=device) for _ in range(3))
        self.graphs = collections.OrderedDict()
        self.pool = None              # the bucket graphs never run concurrently: one pool for all

    def __getitem__(self, name):      # bench.py reads _pb["graphs"]
        return getattr(self, name)

    def graph(self, key, cap, capture, label):
        """The record of bucket `key`, the least recently used one last.  A bucket not seen yet is captured on the spot, on the static
        state (already this batch): at most `cap` graphs stay alive, the three bucket plans are built, ``capture(seqs)`` -> the
        bucket's _GraphRecord does whatever the step records (and sets aside whatever its warm-up passes would disturb), and the
        record is kept only once capture() has returned.  label: the step, as the log names it."""
        from . import _ops
        rec = self.graphs.get(key)
        if rec is not None:
            self.graphs.move_to_end(key)
            return rec
        # a bucket met inside a step runs two eager warm-up passes + the capture pass; a trainer's draw dropout seeds from torch's
        # CPU generator (an evaluation's draw nothing).  Ranks meet new buckets at different steps, so the generator is put back:
        # its stream stays the one the caller (and every other rank) sees, as _ops.next_seed documents.  (The step's first capture
        # keeps its draws.)
        rng = torch.get_rng_state() if self.graphs else None
        try:
            while len(self.graphs) >= cap:
                # bounded: a corpus with a wide length spread would otherwise accumulate a graph + its buffers per bucket pair
                old_key, old = self.graphs.popitem(last=False)
                torch.cuda.synchronize()
                old.release()
                log.info("%s: released the graph of bucket %s (cap %d)", label, old_key, cap)
            seqs = (_ops.seq_bucket(self.cu_a, self.B, self.La, key[0]), _ops.seq_bucket(self.cu_t, self.B, self.Lt, key[1]),
                    _ops.seq_bucket_fused(self.cu_f, self.B, min(self.La, self.Lt), key[1]))
            if self.pool is None:
                self.pool = torch.cuda.graph_pool_handle()
            rec = self.graphs[key] = capture(seqs)
        finally:
            if rng is not None:
                torch.set_rng_state(rng)
        log.info("%s: captured the graph of bucket (audio rows, text rows) = %s (%d alive)", label, key, len(self.graphs))
        return rec


def _load_ragged(pb, static, fill, la, lt, ctl=None):
    """A checked ragged batch into the static state of a step captured from ragged batches (static = [src_a, src_t, -, -, y]) -> its
    bucket key.  What every front door shares lives here: a short batch is completed with ghosts first (ghost_plan); then
    ``fill(static, n_utt, (own audio rows, own text rows), key)`` -- _caller_rows or _StoreFeed.fill -- puts the rows at the head of
    each source with zeros from there to the bucket's end (the MOSEI projections read every bucket row) and the targets into the first
    n_utt rows of y; then the lengths go up as one [2, B] block through the pinned twin.  ctl = (first, last): the step-control block
    goes up with n_valid = the batch's own number of utterances, by the protocol of the lengths block."""
    front = pb.front
    n_utt = len(la)
    la, lt, key, own = ghost_plan(la, lt, pb.B, pb.La, pb.Lt)
    fill(static, n_utt, own, key)
    front.lens.upload([la, lt])
    if front.ctl is not None:
        front.ctl.upload(ctl_words(n_utt, *(ctl if ctl is not None else (1, 1))))
    return key


def _caller_rows(rows_a, rows_t, y):
    """the fill of a batch whose rows the caller holds (capture_packed / step_packed / eval_packed): copies, then the zero tail;
    y None: the step holds no targets"""
    def fill(static, n_utt, own, key):
        for src, rows, n, n_rows in ((static[0], rows_a, own[0], key[0]), (static[1], rows_t, own[1], key[1])):
            if rows.data_ptr() != src.data_ptr():
                src[:n].copy_(rows, non_blocking=True)
            src[n:n_rows].zero_()
        if y is not None and y.data_ptr() != static[4].data_ptr():
            static[4][:n_utt].copy_(y, non_blocking=True)      # a short batch: rows of an earlier batch stay behind it (ghosts)
    return fill


def _check_count(who, n, B, partial):
    """ValueError for a batch of n utterances that a step captured for B cannot take: more than B, or another number than B
    unless short batches are served (partial)"""
    if n > B:
        raise ValueError(f"{who}: a batch of {n} utterances; the captured step holds at most B = {B}")
    if n != B and not partial:
        raise ValueError(f"{who}: a batch of {n} utterances; the captured step holds B = {B} (drop the batch, run it with "
                         "use_graph(False), or capture with partial_batches=True)")


class _StoreFeed:
    """what capture_store adds in front of the ragged front door: the data.DeviceFeatureStore the step reads and its version at
    capture, and the plan block -- int32 [3, 2B + 1]: {ids[n], dst_cu[n + 1]} for the audio rows, the text rows and the targets, zero
    padded -- with its pinned twin (_HostBlock), uploaded once per batch.  The gather itself is three eager launches on the step's
    stream in front of the replay; the captured graphs do not know where their static rows came from.  While the feed is alive the
    store refuses append().  augment: the data.StoreAugment of a trainer step (None: the plain gather, always so for an evaluation);
    every fill gathers at ``augment.draw`` as it stands, the step that owns the feed advances it."""
    __slots__ = ("store", "version", "B", "pad", "stride", "block", "augment", "__weakref__")

    def __init__(self, store, B, pad, device, augment=None):
        self.store, self.version, self.B, self.pad = store, store.version, int(B), (int(pad[0]), int(pad[1]))
        self.augment = augment
        self.stride = 2 * self.B + 1
        self.block = _HostBlock([0] * (3 * self.stride), device)
        store._holders.add(self)

    def close(self):
        self.store._holders.discard(self)

    def batch(self, ids, partial, who):
        """every host check of a batch of ids -> (ids, audio lengths, text lengths) as lists.  RuntimeError: the store changed since
        the capture.  ValueError: an id outside the store, more than B utterances (or another number than B without
        partial_batches), a length outside [1, L].  Nothing has been enqueued when it raises."""
        st = self.store
        if st.version != self.version:
            raise RuntimeError(f"{who}: the store changed since the capture (append): capture_store() again")
        ids = st.check_ids(ids)
        _check_count(who, len(ids), self.B, partial)
        return (ids,) + _store_batch(st, ids, self.pad, who)

    def fill(self, ids, targets=True):
        """the fill of a checked batch of ids (_load_ragged): one plan upload, one hriemo_gather_rows launch per operand -- the rows to
        the head of each source and zeros up to the bucket's end in the same launch, the targets into the first n rows of y"""
        def fill(static, n_utt, own, key):
            self.block.upload(self.store.plan_words(ids, self.stride))
            self.store.gather_into(self.block.dev, self.stride, n_utt, static[0], key[0], static[1], key[1], static[4] if targets else None,
                                   self.augment)
        return fill


def _store_batch(store, ids, pad, who):
    """checked ids -> (audio lengths, text lengths) of the batch from the store's host lists; ValueError for a length outside [1, L]"""
    la, lt = [store.lengths_a[i] for i in ids], [store.lengths_t[i] for i in ids]
    for name, ls, L in (("audio", la, pad[0]), ("text", lt, pad[1])):
        bad = [v for v in ls if v < 1 or v > L]
        if bad:
            raise ValueError(f"{who}: {name} length {bad[0]} outside [1, {L}]")
    return la, lt


_capture_streams = {}         # device index -> the one stream every capture of this process records on


def _record_graph(dev, seqs, pool, warm, body, warmed=None, settle=0.0):
    """The capture mechanics every captured step of the process shares: two eager warm-up passes (`warm()`) on the process's one
    capture stream of `dev`, then `body()` -> (loss, out) recorded into a fresh graph on that stream (pool: the memory pool of a
    bucket graph, or None) with CTX.capturing / capture_origin / seq_override in force.  -> the graph's _GraphRecord with that loss
    and those outputs (None: a trainer step has none).  The one way up for _ops.GRAPHS_ALIVE.  warmed(): called behind the warm-up
    passes, in front of the capture (drop what they left).  settle: seconds to wait between the
    warm-up passes and the capture (eager collectives in the warm-up, DataParallelStep._capture_graph)."""
    from . import _ops
    # ONE capture stream per device for every capture of the process: workspaces are keyed by stream, a fresh stream per
    # capture would allocate (and, with a graph alive, retire instead of free) a fresh 64 MB+ set each time
    side = _capture_streams.get(dev.index)
    if side is None:
        side = _capture_streams[dev.index] = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    _ops.CTX.seq_override = seqs
    try:
        with torch.cuda.stream(side):                 # warm-up off the default stream, as graph capture wants
            for _ in range(2):
                warm()
            if warmed is not None:
                warmed()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if settle:
            import time
            time.sleep(settle)
        graph = torch.cuda.CUDAGraph()
        _ops.CTX.capturing = True
        _ops.CTX.capture_origin = side        # every helper-stream fork of the step must start here (_ops.fork refuses nested forks)
        _ops.begin_step()
        try:
            # capture on the stream the warm-up ran on: its workspaces (keyed by stream) exist already, so nothing the
            # graph points into comes from the graph's private pool or is first sized during capture.
            # thread_local: the RCCL watchdog thread may query events while we capture
            kw = {"pool": pool} if pool is not None else {}
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local", **kw):
                loss, out = body()
        finally:
            _ops.CTX.capturing = False
            _ops.CTX.capture_origin = None
    finally:
        _ops.CTX.seq_override = None
    _ops.GRAPHS_ALIVE += 1            # from now on outgrown workspaces are retired, not freed (_ops.workspace)
    # buffers the captured kernels point into (column-sum partials, queued weight-gradient operands) live exactly as long as
    # this graph: they move from the process-wide lists to the graph's owner
    keep = _ops._deferred.keep + _ops._small_dw.keep
    _ops._deferred.keep, _ops._small_dw.keep = [], []
    return _GraphRecord(graph, loss, keep, seqs, out)


def _ragged_state(model, B, pad, widths, dtype, y_static, partial, accum, ctl):
    """The static state of a step captured from ragged batches -> (its _PackedState, the static list [src_a, src_t, None, None, y]):
    one zero-initialised row source per modality, `widths` wide, in `dtype` and as long as the LARGEST bucket (a full batch of B*L
    rows still gets its surplus sequence, bucket_rows); the lengths as one int32 [2, B] block; the three masks; y_static (or None:
    a prediction-only evaluation); the _RaggedFront with the step-control block when `ctl` says there is one."""
    dev = next(model.parameters()).device
    La, Lt = pad
    src_a = torch.zeros(bucket_rows(B * La, B, La), widths[0], dtype=dtype, device=dev)
    src_t = torch.zeros(bucket_rows(B * Lt, B, Lt), widths[1], dtype=dtype, device=dev)
    masks = tuple(torch.ones(B, L, dtype=torch.uint8, device=dev) for L in (La, Lt, Lt))
    front = _RaggedFront(_HostBlock([[1] * B] * 2, dev), masks, not hasattr(model, "audio_proj"), partial, accum,
                         _HostBlock(ctl_words(B, 1, 1), dev) if ctl else None)
    return _PackedState(B, La, Lt, dev, front), [src_a, src_t, None, None, y_static]


class _RaggedStep:
    """What a captured trainer step (DataParallelStep) and a captured evaluation (EvalStep) are alike: a model whose static state
    (_static, _pb) ragged batches are loaded into -- rows the caller holds, or ids of a data.DeviceFeatureStore behind a feed
    (_feed) -- and one graph per bucket, picked or captured on the spot and replayed.  A subclass adds what its graphs record
    (_capture_bucket; _label names it in the log), how its old step goes, and its entry points with their own refusals."""

    max_graphs = None             # bucket graphs kept alive; None: _VARLEN_MAX_GRAPHS (EvalStep takes its own)

    def __init__(self, model, loss_fn):
        from . import _ops
        self.model, self.loss_fn = model, loss_fn
        self.ctx = _ops.StepContext()      # this step's capture flag / packed plan / join scope: not shared with another step's
        self._pb = None               # _PackedState of a step captured in packed (varlen) mode: shapes, cu_seqlens, bucket graphs, front
        self._static = None           # the static batch the captured step reads: [h_a | src_a, h_t | src_t, m_a, m_t, y | None]
        self._feed = None             # _StoreFeed of a step captured on a data.DeviceFeatureStore (capture_store)
        self._replay = True           # use_graph(False) runs a captured step eagerly

    @property
    def captured(self):
        """bucket graphs exist (use_graph decides whether they are replayed)"""
        return self._pb is not None and len(self._pb.graphs) > 0

    @property
    def _replaying(self):
        return self._replay and self.captured

    @property
    def store(self):
        """the data.DeviceFeatureStore this step was captured on (capture_store) and the ids of step_store / eval_store refer to;
        None otherwise"""
        return None if self._feed is None else self._feed.store

    def _packed_graph(self, key):
        """the record of bucket `key`: captured on the static state (already this batch) when the bucket is new"""
        return self._pb.graph(key, self.max_graphs if self.max_graphs is not None else _VARLEN_MAX_GRAPHS, self._capture_bucket, self._label)

    def _release_buckets(self):
        """every bucket graph goes, with the buffers its kernels point into, and the feed closes: the store may grow again"""
        if self._pb is not None and self._pb.graphs:
            torch.cuda.synchronize()
            for rec in self._pb.graphs.values():
                rec.release()
        if self._feed is not None:
            self._feed.close()
            self._feed = None

    def _need_forward_packed(self, who):
        if not hasattr(self.model, "_forward_rows"):
            raise TypeError(f"{who}: the model has no forward_packed entry")

    def _need_n_valid(self, who):
        if not _accepts_n_valid(self.loss_fn):
            raise TypeError(f"{who}: loss_fn takes no n_valid= keyword -- the ghost utterances of a short batch must stay out of "
                            "the loss (hri_emo_amd.train's losses accept it)")

    def _store_capture(self, who, store, ids, pad_to, targets=True):
        """the host checks of capture_store, before the old step is given up -> (ids, audio lengths, text lengths, (La, Lt), the
        static targets: zeros in the store's form, or None without `targets`)"""
        from .data import DeviceFeatureStore
        if not isinstance(store, DeviceFeatureStore):
            raise TypeError(f"{who}: store is a data.DeviceFeatureStore")
        ids = store.check_ids(ids)
        dev = next(self.model.parameters()).device
        if store.device != dev:
            raise ValueError(f"{who}: the store lives on {store.device}, the model on {dev}")
        La, Lt = (int(v) for v in (pad_to if pad_to is not None else store.pad_to))
        if Lt > La:
            raise RuntimeError(f"{who}: L_t={Lt} > L_a={La}: the gate fuses over the text length and needs L_a >= L_t")
        if not hasattr(self.model, "audio_proj") and store.widths[0] != store.widths[1]:
            raise ValueError(f"{who}: the store's rows differ in width {store.widths}")
        la, lt = _store_batch(store, ids, (La, Lt), who)
        y_static = torch.zeros((len(ids),) + tuple(store.y.shape[1:]), dtype=store.y.dtype, device=dev) if targets else None
        return ids, la, lt, (La, Lt), y_static

    def _capture_ragged(self, begin, widths, dtype, y_static, la, lt, pad, load, store=None, partial=True, accum=1, ctl=True, augment=None):
        """What every capture from ragged batches does behind its entry's checks: begin() -- the old step goes (behind the refusals
        that need it untouched) and the subclass's facts of the new one are set --, the static state is built (_ragged_state), a
        step that reads `store` gets its _StoreFeed (made after the old step and its feed have gone), the first batch is loaded by
        load() -> bucket key and its bucket graph is captured."""
        from . import _ops
        _ops._require_gpu(next(self.model.parameters()))
        begin()
        self._pb, self._static = _ragged_state(self.model, len(la), pad, widths, dtype, y_static, partial, accum, ctl)
        try:
            if store is not None:
                self._feed = _StoreFeed(store, len(la), pad, self._static[0].device, augment)
            self._packed_graph(load())
        except BaseException:
            self.release_graph()          # a failed capture leaves no graph behind -- and no feed that would keep the store from growing
            raise

    def _check_batch(self, who, rows_a, rows_t, n, y):
        """the refusals of a ragged batch whose rows the caller holds, before anything is enqueued: the number of utterances, row
        width / dtype against the static sources, the targets' shape against the static targets (when the step holds any)"""
        B, sy = self._pb.B, self._static[4]
        _check_count(who, n, B, self._pb.front.partial)
        for name, rows, src in (("rows_a", rows_a, self._static[0]), ("rows_t", rows_t, self._static[1])):
            if rows.shape[1] != src.shape[1] or rows.dtype != src.dtype:
                raise ValueError(f"{who}: {name} of width {rows.shape[1]} / {rows.dtype}; captured with width {src.shape[1]} / {src.dtype}")
        if sy is not None:
            want = (n,) + tuple(sy.shape[1:])
            if tuple(y.shape) != want:
                raise ValueError(f"{who}: targets of shape {tuple(y.shape)}; captured with {tuple(sy.shape)}"
                                 + (f", this batch needs {want}" if n != B else ""))

    def _load_packed(self, rows_a, rows_t, la, lt, y, ctl=None):
        """a checked ragged batch whose rows the caller holds into the static state -> its bucket key (_load_ragged)"""
        return _load_ragged(self._pb, self._static, _caller_rows(rows_a, rows_t, y), la, lt, ctl)

    def _load_store(self, ids, la, lt, ctl=None):
        """a checked batch of ids of the captured store into the static state -> its bucket key (_load_ragged)"""
        return _load_ragged(self._pb, self._static, self._feed.fill(ids, self._static[4] is not None), la, lt, ctl)


class DataParallelStep(_RaggedStep):
    """fwd -> loss -> bwd -> gradient all-reduce for one shard; mirrors the order of operations of
    train_one_epoch (scripts/fusion/train_fusion_seq_level_decoder.py:310-334) minus the optimizer.

    ``capture()`` records zero-grad + forward + loss + backward of one step into a hipGraph (the eager step
    costs ~10 ms of host time for ~150 launches; a replay costs microseconds).  Dropout stays fresh per
    replay through the device-resident seed word the graph bumps itself (``_ops.seed_word``); bf16 weight
    shadows are re-cast inside the graph so optimizer updates between replays are honoured.  The gradient
    all-reduce runs after the replay on the flat buffer.  ``capture(..., optimizer=opt)`` with an ``optim.DeviceAdamW``
    records the optimizer's three launches at the end of the graph as well: one ``step()`` is then the whole trainer step."""

    _label = "packed step"

    def __init__(self, model, loss_fn, group=None, bucket_bytes=32 << 20, overlap=True, comm_dtype=torch.float32, force_exchange=False,
                 launch_from="notify", force_queue=None):
        super().__init__(model, loss_fn)
        self.force_queue = force_queue    # None: the loader / consumer GEMMs draw from the work queue when collectives run beside backward; True / False: always / never
        self._exchange_in_graph = False   # capture(collectives=True): the bucket all-reduces are part of the captured step
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.buckets = GradBuckets(model.parameters(), bucket_bytes, group, overlap, comm_dtype, force_exchange, launch_from)
        # a captured graph has one owner: _record (the plain step) or _pb.graphs (the packed modes, one record per bucket)
        self._record = None
        self._mask_seen = None        # mask-fed packed step: (mask identity, bucket key, cu_seqlens clones, the masks) of the last step
        self._optimizer = None        # optim.DeviceAdamW whose update closes the captured step (capture(optimizer=...))
        self._micro = 0               # micro-steps of the open accumulation group (capture_packed(grad_accum=k)): 0 .. k-1
        self._stats = None            # train.EpochStats fed by every executed (micro-)step (attach_stats)
        self._stats_scale = 1.0
        self._outputs = None          # with statistics attached: what the latest _fwd_bwd pass hands to _update_stats
        self._act_log = None          # train.ActivationLog fed by every executed (micro-)step (attach_activations)

    @property
    def captured(self):
        """a captured step exists (use_graph decides whether step() replays it)"""
        return self._record is not None or (self._pb is not None and len(self._pb.graphs) > 0)

    def set_global_batch(self, global_batch):
        lo, hi = shard_bounds(global_batch, self.rank, self.world)
        if hasattr(self.model, "set_batch_offset"):
            self.model.set_batch_offset(lo)
        return lo, hi

    def attach_stats(self, stats, loss_scale=1.0):
        """Feed a ``train.EpochStats`` from this step: every executed trainer step or micro-step -- a replay, an eager step, a
        micro-batch of step_accumulated -- updates it exactly once, with the pass's logits, beta, targets and loss (and n_valid after
        capture_packed(partial_batches=True)); nothing is read back.  Call it BEFORE capture() / capture_packed(): the update
        (hriemo_stats_update, one block) is recorded inside the graph, behind forward + loss + backward and in front of the
        optimizer's launches.  The warm-up passes of a capture never count -- those of a bucket graph captured in the middle of an
        epoch included: they run without the update exactly as they run without the optimizer.  loss_scale: what the logged loss is
        multiplied by -- grad_accum where the loss function divides by it (mosei_step_loss(grad_accum=k)): the reference logs the
        undivided loss (train_mosei_fusion_seq_level_decoder.py:385-388,406).  stats=None detaches.  Without statistics attached
        every path launches exactly what it launched before."""
        if self.captured:
            raise RuntimeError("attach_stats() comes before capture() / capture_packed(): the update is part of the captured step "
                               "(release_graph() first to change it)")
        self._stats, self._stats_scale, self._outputs = stats, float(loss_scale), None

    def attach_activations(self, log):
        """Feed a ``train.ActivationLog`` from this step: every executed trainer step or micro-step -- a replay, an eager step, a
        micro-batch of step_accumulated or of a captured accumulation group -- is one pass of the log: its plan launch at the top of
        the forward in front of every fork, a probe behind every sub-layer the log keeps (forward) and at the top of its backward
        (gradient), the forward fold at the end of the forward and the gradient fold behind backward, in front of the statistics
        and the optimizer.  Nothing is read back.  Call it BEFORE capture() / capture_packed() / capture_store(), as attach_stats:
        the launches are part of the captured step.  The warm-up passes of a capture -- those of a bucket graph met in the middle
        of an epoch included -- run under the closed window and leave no trace.  After capture_packed(partial_batches=True) the
        ghost utterances of a short batch never count.  log=None detaches.  Without a log attached every path launches exactly what
        it launched before."""
        if self.captured:
            raise RuntimeError("attach_activations() comes before capture() / capture_packed(): the probes are part of the captured "
                               "step (release_graph() first to change it)")
        if log is not None:
            log._guard()
        self._act_log = self.ctx.act_log = log

    def _update_stats(self):
        """one hriemo_stats_update launch on the outputs of the latest _fwd_bwd pass (no-op without statistics attached)"""
        out, self._outputs = self._outputs, None
        if self._stats is not None and out is not None:
            logits, beta, y, loss, n_valid = out
            self._stats.update(logits, beta, y, loss, n_valid=n_valid, loss_scale=self._stats_scale)

    def _fwd_bwd(self, h_a, h_t, m_a, m_t, y, zero=True, scale=None, ragged=None):
        """ragged = (audio lengths, text lengths, pad_to): h_a / h_t are a ragged batch's own rows (the eager forward_packed step).
        After capture_packed, without `ragged`: h_a / h_t are the static row sources and the step starts with hriemo_seq_tables."""
        from . import _ops
        pb = self._pb
        front = pb.front if (pb is not None and ragged is None) else None
        if front is not None:
            # the first launch of the packed arm, warm-up passes included: the lengths [2, B] -> the three cu_seqlens of the bucket
            # in force and the three masks; everything behind it reads those static buffers
            seqs = _ops.CTX.seq_override
            if seqs is None:
                raise RuntimeError("DataParallelStep: after capture_packed() the static rows are fed by step_packed() only")
            _ops.seq_tables(front.lens.dev, pb.La, pb.Lt, rows=(seqs[0].N, seqs[1].N), cu=(pb.cu_a, pb.cu_t, pb.cu_f), masks=front.masks)
        # collectives launched from the gradient-ready hooks run BESIDE backward (eagerly, or baked into a capture): the loader /
        # consumer GEMMs then draw their tiles from the work queue (a block whose CU a collective holds late draws fewer); with
        # the chip to itself they walk statically, which is 5-8 % faster per launch alone and equal inside the step
        b = self.buckets
        if self.force_queue is None:
            _ops.gemm_contended(bool(b._hooks) and not b.suspended and b.world > 1)
        else:
            _ops.gemm_contended(bool(self.force_queue), force=True)
        ctl = front.ctl.dev if (front is not None and front.ctl is not None) else None
        if ctl is not None and front.accum > 1:
            # a step captured with gradient accumulation: whether the flat buffer starts from zero is device data (ctl.first)
            from . import _lib
            _lib.call("hriemo_grad_begin", self.buckets.flat.data_ptr(), self.buckets.flat.numel(), ctl.data_ptr(), _ops._stream())
            self.buckets._rebind()
        elif zero:
            self.buckets.zero_grad()
        act = self._act_log
        if act is not None:
            act.n_valid = ctl[:1] if (ctl is not None and front.partial) else None
        if ragged is not None:
            logits, beta, _ = self.model.forward_packed(h_a, h_t, ragged[0], ragged[1], pad_to=ragged[2])
        elif front is not None:
            logits, beta, _ = self.model._forward_rows(h_a, h_t, tuple(seqs), front.bool, (pb.La, pb.Lt))
        else:
            logits, beta, _ = self.model(h_a, h_t, m_a, m_t)
        if ctl is not None and front.partial:
            loss = self.loss_fn(logits, beta, y, n_valid=ctl[:1])      # ctl.n_valid: the ghosts behind it add nothing and get zero gradients
        else:
            loss = self.loss_fn(logits, beta, y)
        if self._stats is not None:
            # handed to _update_stats by the caller that executes (or records) a real step; a warm-up pass drops them.  The loss
            # as loss_fn returned it: step_accumulated's own 1/k below is not part of what the reference logs
            self._outputs = (logits.detach(), None if beta is None else beta.detach(), y, loss.detach(),
                             ctl[:1] if (ctl is not None and front.partial) else None)
        if scale is not None:
            loss = loss * scale
        if loss.is_cuda and scale is None:
            loss.backward(gradient=_ops.one(loss.device))      # the fused losses skip the multiply by this very tensor
        else:
            loss.backward()
        if act is not None:
            act.close_backward()              # the gradient half's fold: behind backward, in front of statistics and optimizer
        return loss.detach()

    @_in_step_context
    def step_accumulated(self, micro_batches, pad_to=None):
        """Gradient accumulation (train_mosei_fusion_seq_level_decoder.py:387-396: loss / grad_accum, optimizer every grad_accum
        micro-steps) under data parallelism WITHOUT a gradient exchange per micro-step: the flat buffer is zeroed once, every
        micro-batch accumulates into it (the kernels add in place), gradient-ready notifications stay suspended until the LAST
        micro-batch, whose backward launches the bucket all-reduces as usual.  Returns the mean of the micro-losses.
        pad_to=(L_a, L_t): the micro-batches are ragged, (rows_a, rows_t, lengths_a, lengths_t, y) each, of any number of
        utterances, and run through the model's forward_packed (the eager counterpart of capture_packed(grad_accum=k))."""
        from . import _ops
        k = len(micro_batches)
        was = self.buckets.suspended
        total = None
        for i, mb in enumerate(micro_batches):
            self.buckets.suspended = True if i + 1 < k else was
            if pad_to is not None:
                ra, rt, la, lt, y = mb
                la, lt, pad = _ops.packed_lengths(ra, rt, la, lt, pad_to, same_width=not hasattr(self.model, "audio_proj"))
                l = self._fwd_bwd(ra, rt, None, None, y, zero=(i == 0), scale=1.0 / k, ragged=(la, lt, pad))
            else:
                l = self._fwd_bwd(*mb, zero=(i == 0), scale=1.0 / k)
            self._update_stats()
            total = l if total is None else total + l
        self.buckets.suspended = was
        self.buckets.finish()
        return total

    @_in_step_context
    def capture(self, h_a, h_t, m_a, m_t, y, collectives=False, lengths=None, optimizer=None):
        """Record one step on static copies of the batch tensors; later ``step()`` calls replay it.

        collectives=True: the gradient exchange is captured INSIDE the graph -- every bucket's all-reduce is launched from its
        gradient-ready hook while backward is being recorded (on the capture's origin stream; the process group forks its
        communication stream from there), the waits and the 1/N average close the graph -- so a replay overlaps the exchange
        with backward exactly like the eager mode does, without the host enqueueing ~450 launches per step.  Needs a backend
        whose collectives can be stream-captured (RCCL can); the hooks must be installed (overlap=True) and not suspended.

        Packed (varlen) mode (``hri_emo_amd.set_varlen(True)`` and both padding masks given): the sequence lengths are DEVICE
        data of the captured step (cu_seqlens buffers refreshed before every replay), only the packed row counts are baked in,
        rounded up to a bucket (1/64 of the padded rows; the surplus rows form one extra all-zero sequence).  The fused memory of
        the packed tail (min of the two lengths per utterance) has a third cu_seqlens buffer and the text bucket's row count.  ``step()`` then
        serves EVERY batch of these shapes: a batch whose row counts fall into a bucket not seen yet captures that bucket's
        graph on the spot (same static inputs, one memory pool).  ``lengths`` = (audio lengths, text lengths) as host lists /
        CPU tensors spares the device -> host read of the masks' row sums (one sync per step otherwise).

        optimizer: an ``optim.DeviceAdamW`` built on this step's buckets.  Its three launches (sum of squares, finalize, update) are
        recorded at the END of the captured step -- behind the captured exchange with collectives=True -- and in no warm-up pass,
        so capture() itself moves neither parameters nor moments nor the step count.  ``step()`` then uploads the optimizer's
        hyper-parameters (lr as a scheduler left it) before the replay and is the whole trainer step: no ``opt.step()`` after it.
        Every scalar of the update is device data, so packed bucket graphs captured later share the one step count.  At world
        size > 1 this needs collectives=True: an exchange after the replay would run behind the update."""
        from . import _ops
        packed = _ops.varlen() and m_a is not None and m_t is not None
        self._begin_capture("capture", optimizer, collectives, packed)
        self._static = [None if t is None else t.clone() for t in (h_a, h_t, m_a, m_t, y)]
        if packed:
            self._pb = _PackedState(h_a.shape[0], h_a.shape[1], h_t.shape[1], self._static[0].device)
            self._packed_graph(self._packed_key(m_a, m_t, lengths))
        else:
            self._record = self._capture_graph(None)
        self._end_capture()

    def _begin_capture(self, entry, optimizer, collectives, packed):
        """the refusals capture() and capture_packed() share, then the old step goes and the new one's facts are set"""
        if optimizer is not None:
            from .optim import DeviceAdamW
            if not isinstance(optimizer, DeviceAdamW) or optimizer.buckets is not self.buckets:
                raise TypeError(f"{entry}(optimizer=...) takes an optim.DeviceAdamW built on this step's buckets (every scalar of its "
                                "update is device data; FusedClipAdamW passes lr and the step count by value)")
            if self.world > 1 and not collectives:
                raise RuntimeError(f"{entry}(optimizer=...) at world size > 1 needs collectives=True: the gradient exchange after the "
                                   "replay would run behind the captured update" + (" (and packed mode captures none)" if packed else ""))
        if packed and collectives and self.world > 1:
            raise RuntimeError(f"{entry}(collectives=True) in packed (varlen) mode: ranks meet new buckets at different steps and a "
                               "bucket's capture runs eager warm-up exchanges -- capture without collectives (exchange after the "
                               "replay) or run the padded path")
        if collectives and not self.buckets._hooks:
            raise RuntimeError(f"{entry}(collectives=True) needs the gradient-ready hooks: GradBuckets(overlap=True) at world size > 1 "
                               "(or force_exchange=True)")
        if not collectives and self.buckets._hooks and not self.buckets.suspended:
            raise RuntimeError(f"{entry}() needs GradBuckets(overlap=False) or buckets.suspended = True, or collectives=True to "
                               "capture the exchange as well")
        if collectives:
            self.buckets.suspended = False
        self.release_graph()              # a re-capture replaces the old graph(s): their pinned buffers go first
        self._exchange_in_graph = bool(collectives)
        self._optimizer = optimizer
        self._mask_seen = None

    def _end_capture(self):
        self._replay = True
        if self._exchange_in_graph:
            self.buckets.suspended = True         # from now on hooks fire only inside replays (they are baked into the graph)

    @_in_step_context
    def capture_packed(self, rows_a, rows_t, lengths_a, lengths_t, y, pad_to, optimizer=None, collectives=False, partial_batches=False,
                       grad_accum=1):
        """capture() for batches that arrive ragged (data.collate_seq_packed): rows_a / rows_t [sum(lengths), d] (fp32, bf16 or fp16; on
        the device or in pinned host memory) hold the valid rows of all utterances back to back, lengths_a / lengths_t are host
        sequences or CPU int tensors, pad_to = (L_a, L_t) the padded lengths: they size the static buffers, key the dropout hash and fix
        the gate's L.  pad_to and the number of utterances are fixed from here on; ``step_packed`` then serves every batch.

        Static state: one row source per modality in the rows' dtype, zero-initialised and as long as the LARGEST bucket (a full
        batch of B*L rows still gets its surplus sequence, bucket_rows); the lengths as ONE int32 [2, B] block on the device with a
        pinned host twin; the three cu_seqlens buffers and three mask buffers of packed mode; y.  The captured step starts with
        hriemo_seq_tables, which derives the cu_seqlens and the masks from the lengths block, then runs the model's forward_packed
        body on a bucket plan (hriemo_ingest_rows on the packed source): no padded tensor exists on the host or on the device, and
        the lengths cross to the device once.  Behind the front door everything is the mask-fed packed step: the bucket graphs
        (one per (audio rows, text rows) bucket, LRU-capped, one memory pool), packed_tail(), fp32 precision, mx_fp8,
        optimizer=DeviceAdamW.  The encoder runs packed whatever set_varlen says, as in forward_packed.  collectives=True at world
        size > 1 is refused for the reason capture() gives in packed mode.

        Two opt-in arguments let the captured step run a whole epoch of the reference's trainers (their loaders keep the short last
        batch; the MOSEI trainer accumulates gradients, train_mosei_fusion_seq_level_decoder.py:383-402).  Both turn a fact of the
        step that is otherwise baked into the graph into DEVICE data: one int32 step-control block ctl[4] = {n_valid, first, last,
        spare} with a pinned host twin, uploaded in stream order before every replay like the lengths block.  With neither given the
        captured step consists of exactly the launches it had before them (memset, hriemo_fusion_loss(_ce), hriemo_optim_finalize).

        partial_batches=True: ``step_packed`` accepts 1 <= n <= B utterances.  The B - n missing ones become GHOSTS on the host:
        length 1 in both modalities, their rows the zero rows that are written behind the batch's own rows anyway, counted in the
        bucket key.  ctl.n_valid = n; ``loss_fn`` is called with ``n_valid=`` (a 1-element int32 device tensor) and must ignore the
        ghosts: hri_emo_amd.train's three losses do (hriemo_fusion_loss_n / _ce_n: means over the first n samples, exactly zero
        gradients for the ghosts, so nothing of a ghost reaches a parameter gradient).  y is copied into the first n rows of the
        static targets; rows of an earlier batch may stay behind them.  A ``loss_fn`` without an ``n_valid`` keyword is a TypeError
        here.  Each rank normalises by its OWN n_valid, as torch's DistributedDataParallel does with a short last batch: the
        exchange averages per-rank means, it does not re-weight them by sample counts.

        grad_accum=k > 1: the captured step starts with hriemo_grad_begin (zeroes the flat gradient buffer when ctl.first is set,
        leaves every bit in place otherwise) instead of the memset, and the optimizer's finalize launch becomes
        hriemo_optim_finalize_ctl (holds the update unless ctl.last is set: parameters, moments, step count, ``skipped`` and
        ``grad_norm`` stay as they are).  ``step_packed`` counts micro-steps: first on micro-step 0, last on micro-step k - 1; the
        exchange outside the graph, the weights-epoch bump and the hyper-parameter upload happen for the last micro-step only.  The
        1/k loss scale stays the caller's, by value (``mosei_step_loss(grad_accum=k)``): it is constant per run.
        ``flush_accumulated()`` closes a group that the end of an epoch cut short."""
        from . import _ops
        self._check_ragged_capture("capture_packed", partial_batches, grad_accum)
        same_width = not hasattr(self.model, "audio_proj")
        la, lt, pad = _ops.packed_lengths(rows_a, rows_t, lengths_a, lengths_t, pad_to, same_width=same_width)
        if pad_to is None:
            raise ValueError("capture_packed: pad_to=(L_a, L_t) is required")
        dev = next(self.model.parameters()).device
        self._capture_ragged(lambda: self._begin_ragged("capture_packed", optimizer, collectives), (rows_a.shape[1], rows_t.shape[1]),
                             rows_a.dtype, y.to(dev, copy=True), la, lt, pad, lambda: self._load_packed(rows_a, rows_t, la, lt, y),
                             partial=partial_batches, accum=grad_accum, ctl=partial_batches or grad_accum > 1)
        self._end_capture()

    def _check_ragged_capture(self, entry, partial_batches, grad_accum):
        self._need_forward_packed(entry)
        if int(grad_accum) != grad_accum or grad_accum < 1:
            raise ValueError(f"{entry}: grad_accum = {grad_accum!r} (an integer >= 1)")
        if partial_batches:
            self._need_n_valid(f"{entry}(partial_batches=True)")

    def _begin_ragged(self, entry, optimizer, collectives):
        """_capture_ragged's begin(): the refusals capture() shares, the old step goes, a new accumulation group opens"""
        self._begin_capture(entry, optimizer, collectives, packed=True)
        self._micro = 0

    @_in_step_context
    def capture_store(self, store, ids, pad_to=None, optimizer=None, collectives=False, partial_batches=False, grad_accum=1, augment=None):
        """capture_packed() for batches that are lists of utterance ids of a ``data.DeviceFeatureStore`` on this step's device: the
        batch `ids` fixes B, pad_to = (L_a, L_t) defaults to ``store.pad_to`` (the store's longest utterances).  Everything behind the
        static row sources is capture_packed unchanged -- bucket graphs and their LRU cap, ghosts and the control block
        (partial_batches), grad_accum, optimizer=DeviceAdamW, attach_stats, fp32 and mx_fp8 modes -- and the captured graphs hold the
        launches they hold after capture_packed, in the same order.  What changes is how a batch reaches the static state
        (``step_store``): one upload of the plan block {ids, dst_cu} x 3 (written by the host from the store's host lengths, pinned
        twin like the lengths block) and one hriemo_gather_rows launch per operand -- audio rows, text rows, targets -- on the
        step's stream in front of the replay; the kernel writes the zero tail up to the bucket's end as well.  No row crosses
        PCIe, nothing is read back, no device memory is allocated.
        While the step is captured the store refuses ``append``.  Data parallel: every rank holds the whole store (a few GB) and
        passes ITS slice of the global batch's ids (``shard_bounds``); ``set_batch_offset`` / ``set_global_batch`` are untouched.

        augment (a ``data.StoreAugment``): the audio and text gathers of every ``step_store`` become hriemo_gather_rows_aug launches
        -- time masks, noise, modality dropout, all seeded by (augment.seed, augment.draw, store id) -- and nothing else changes: the
        graphs, the plan block and the targets gather are the same.  The warm-up and capture fills here use ``augment.draw`` as it
        stands and leave it alone.  Every rank passes an augment with the same seed and keeps the same draw (lockstep); a sample's
        augmentation then does not depend on the rank that holds it.  Evaluation takes no augment."""
        self._check_ragged_capture("capture_store", partial_batches, grad_accum)
        ids, la, lt, pad, y_static = self._store_capture("capture_store", store, ids, pad_to)
        if augment is not None:
            store._check_augment("capture_store", augment)
        self._capture_ragged(lambda: self._begin_ragged("capture_store", optimizer, collectives), store.widths, store.dtype, y_static, la, lt,
                             pad, lambda: self._load_store(ids, la, lt), store, partial=partial_batches, accum=grad_accum,
                             ctl=partial_batches or grad_accum > 1, augment=augment)
        self._end_capture()

    @_in_step_context
    def step_store(self, ids):
        """One trainer step on the utterances `ids` of the captured store (capture_store): step_packed with "copy the caller's rows"
        replaced by "gather by id".  The ids ALWAYS refer to the store given to capture_store -- ``self.store``; a caller that
        keeps several stores (train / val / test) keeps one step per store or captures again, and checks ``step.store is store``
        where the two could be confused (train.evaluate_store does).  Host checks first -- the store as it was at capture (RuntimeError after an append), every id
        inside it, n <= B (n == B without partial_batches), lengths inside pad_to (ValueError) -- and nothing is enqueued when one
        fails.  Then: plan block up, at most three hriemo_gather_rows launches, lengths (and control) block up, replay.  After
        use_graph(False) this is the eager step_packed on ``store.fetch(ids)``.  Micro-steps, flush_accumulated() and the
        optimizer in the graph behave as after capture_packed.
        After capture_store(augment=aug) the rows are gathered with ``draw = aug.draw`` -- captured, or eager through
        ``store.fetch(ids, augment=aug)``: both see identical rows -- and ``aug.draw`` goes up by one per call that got through (every
        micro-step is a draw of its own); a refused call leaves it alone.  Ghost utterances are not in the plan and stay zero rows."""
        feed = self._feed
        if feed is None or self._pb is None or self._pb.front is None:
            raise RuntimeError("step_store needs capture_store() first")
        ids, la, lt = feed.batch(ids, self._pb.front.partial or not self._replaying, "step_store")
        aug = feed.augment
        if self._replaying:
            loss = self._replay_ragged(lambda ctl: self._load_store(ids, la, lt, ctl=ctl))
        else:
            rows_a, _, rows_t, _, y = feed.store.fetch(ids, augment=aug)
            loss = self._eager_ragged(rows_a, rows_t, la, lt, y)
        if aug is not None:
            aug.draw += 1
        return loss

    @_in_step_context
    def step_packed(self, rows_a, rows_t, lengths_a, lengths_t, y):
        """One trainer step on a ragged batch (capture_packed): the arguments are checked on the host (_ops.packed_lengths; a
        ValueError leaves the static state untouched), the rows, the lengths block and y are copied into the static buffers, the
        batch's bucket graph is picked -- or captured on the spot -- and replayed.  A batch with another number of utterances than
        captured is refused: drop it, or run it with use_graph(False), which makes this the eager forward_packed step.  After
        capture_packed(partial_batches=True) a batch of 1 <= n <= B utterances is served by the same graphs (ghosts, n_valid as
        device data); after capture_packed(grad_accum=k) every call is one MICRO-step and the k-th one carries the update."""
        from . import _ops
        pb = self._pb
        front = pb.front if pb is not None else None
        if front is None:
            raise RuntimeError("step_packed needs capture_packed() first")
        la, lt, _ = _ops.packed_lengths(rows_a, rows_t, lengths_a, lengths_t, (pb.La, pb.Lt), same_width=front.same_width)
        if self._replaying:
            self._check_batch("step_packed", rows_a, rows_t, len(la), y)
            return self._replay_ragged(lambda ctl: self._load_packed(rows_a, rows_t, la, lt, y, ctl=ctl))
        return self._eager_ragged(rows_a, rows_t, la, lt, y)

    def _replay_ragged(self, load):
        """a checked batch through the captured step, for every ragged front door: hyper-parameters up when this micro-step carries
        the update, the batch into the static state (load(ctl) -> bucket key: _load_packed or _load_store), the bucket graph
        picked -- or captured on the spot -- and replayed"""
        first, last = micro_flags(self._micro, self._pb.front.accum)
        if self._optimizer is not None and self._optimizer._swapped is True:
            # inside opt.averaged_weights(): a held micro-step uploads nothing (so _upload_hyper cannot refuse it), but its
            # gradients must not come from the average either
            self._optimizer._refuse_while_averaged("a training replay")
        if self._optimizer is not None and last:
            # the update of this group reads lr & co. as the scheduler left them after the previous update; a held micro-step
            # reads none of them (the finalize returns in front of hyper[], the update kernel in front of everything)
            self._optimizer._upload_hyper()
        key = load((first, last))
        rec = self._packed_graph(key)                 # captures on the static state (already this batch) if the bucket is new
        rec.graph.replay()
        self._micro = 0 if last else self._micro + 1
        if last:
            self._after_replay()
        return rec.loss

    def _eager_ragged(self, rows_a, rows_t, la, lt, y):
        """use_graph(False): the eager forward_packed step on a checked ragged batch"""
        pb = self._pb
        first, last = micro_flags(self._micro, pb.front.accum)
        dev = self._static[0].device
        was = self.buckets.suspended
        if not last:
            self.buckets.suspended = True                 # as step_accumulated: the exchange belongs to the group's last backward
        try:
            loss = self._fwd_bwd(rows_a.to(dev, non_blocking=True), rows_t.to(dev, non_blocking=True), None, None, y.to(dev, non_blocking=True),
                                 zero=first, ragged=(la, lt, (pb.La, pb.Lt)))
        finally:
            self.buckets.suspended = was
        self._update_stats()
        self._micro = 0 if last else self._micro + 1
        if last:
            self.buckets.finish()
            if self._optimizer is not None:
                self._optimizer.step()
        return loss

    @property
    def micro_step(self):
        """micro-steps taken in the open accumulation group (0: none pending)"""
        return self._micro

    @_in_step_context
    def flush_accumulated(self):
        """Close an accumulation group that the end of an epoch cut short (capture_packed(grad_accum=k), fewer than k micro-steps
        since the last update): the update runs on what HAS been accumulated -- nothing is rerun.  The form chosen is the simplest
        correct one: no replay with last = 1 and an empty batch, but the gradient exchange (when it is outside the graph) followed
        by one eager ``DeviceAdamW.step()`` on the flat buffer -- the same three launches the graph holds, with the plain finalize.
        The sum is NOT rescaled by k / micro-steps: every term carries the caller's 1/k, as in the reference trainer, whose loss
        scale does not know about the epoch's end either.  Without an optimizer in the graph only the exchange is finished and the
        caller's own ``opt.step()`` follows.  Returns the number of micro-steps the update covers (0: nothing was pending, nothing
        is done)."""
        n = self._micro
        if n == 0:
            return 0
        self._micro = 0
        if not self._exchange_in_graph or not self._replaying:
            self.buckets.finish()
        if self._optimizer is not None:
            self._optimizer.step()                        # uploads hyper[], bumps the weights epoch
        return n

    # ---- packed (varlen) bucket graphs
    def _packed_key(self, m_a, m_t, lengths):
        """host-side: the batch's cu_seqlens written to the static device buffers + the bucket (rows audio, rows text) it needs"""
        pb = self._pb
        la, lt = mask_lengths(m_a, m_t, lengths, pb.B, pb.La, pb.Lt)
        key, *tables = packed_tables(la, lt, pb.B, pb.La, pb.Lt)
        for buf, cu in zip((pb.cu_a, pb.cu_t, pb.cu_f), tables):
            buf.copy_(torch.tensor(cu, dtype=torch.int32))
        return key

    def _capture_bucket(self, seqs):
        """the bucket graph of the plans `seqs` (_PackedState.graph)"""
        # inside an accumulation group the warm-up passes run with ctl.first = 0 and would add to the running gradient sum:
        # it is set aside and put back (a copy of the flat buffer, paid only when a bucket is met for the first time)
        front = self._pb.front
        held = self.buckets.flat.clone() if (front is not None and front.accum > 1 and self._micro > 0) else None
        try:
            return self._capture_graph(seqs)
        finally:
            if held is not None:
                self.buckets.flat.copy_(held)

    def _capture_graph(self, seqs):
        """warm-up + capture of one step on self._static; seqs = the packed plans of a bucket graph (or None) -> its _GraphRecord"""
        from . import _ops
        collectives = self._exchange_in_graph

        def warm():
            if self._act_log is not None:
                with self._act_log.paused():      # under the closed window: a warm-up pass leaves no trace in the log
                    self._fwd_bwd(*self._static)
            else:
                self._fwd_bwd(*self._static)
            if collectives:
                self.buckets.finish()         # the warm-up steps exchange eagerly (every rank alike) and leave the buckets reset

        def warmed():
            self._outputs = None                  # warm-up passes never reach the statistics

        def body():
            _ops.bump_seed_word(self._static[0].device)
            loss = self._fwd_bwd(*self._static)
            self._update_stats()              # recorded, not run: one block behind backward, in front of the optimizer
            if collectives:
                self.buckets.finish()         # waits on the captured collectives + the average: part of the graph
            if self._optimizer is not None:
                front = self._pb.front if self._pb is not None else None
                ctl = front.ctl.dev if (front is not None and front.accum > 1) else None
                self._optimizer._enqueue(ctl=ctl)    # recorded, not run: norm, skip / hold / clip / bias corrections, update
            return loss, None

        # The process group's watchdog thread polls the end event of every EAGER collective until it has seen it complete
        # (every 100 ms).  The warm-up exchanges are complete when the capture starts, but not necessarily reaped -- and once the
        # capture pulls the group's communication stream into the capture, ROCm 7.2 answers a query of an event that was
        # recorded on that stream with hipErrorCapturedEvent, which the watchdog turns into std::terminate (sporadic: 1 run
        # in 8 aborted).  Two watchdog periods let it drain its list first.
        return _record_graph(self._static[0].device, seqs, self._pb.pool if seqs is not None else None, warm, body, warmed,
                             settle=0.25 if collectives else 0.0)

    def release_graph(self):
        """drop the captured step (before a re-capture, or to free its buffers): the graph(s), the buffers their kernels point into"""
        was = self.captured
        if self._record is not None:
            torch.cuda.synchronize()
            self._record.release()
        self._release_buckets()
        if was:
            self._record = self._pb = self._optimizer = None

    def use_graph(self, on):
        """Switch between the captured replay (gradient exchange after it) and eager launches (exchange from the
        gradient-ready hooks during backward, if installed)."""
        self._replay = bool(on) and self.captured
        self.buckets.suspended = self._replay     # eager steps: the hooks drive the exchange; replays: it follows / is inside the graph

    def _after_replay(self):
        """what follows the replay that carries the update: the exchange unless the graph holds it, the optimizer's host side"""
        if not self._exchange_in_graph:
            self.buckets.finish()
        if self._optimizer is not None:
            from . import _ops
            _ops.bump_weights_epoch()                 # the replay rewrote the parameters through raw pointers
            self._optimizer._opt_called = True        # torch's lr schedulers warn about a scheduler.step() before any optimizer step

    @_in_step_context
    def step(self, h_a, h_t, m_a, m_t, y, lengths=None):
        if self._replaying:
            pb = self._pb
            if self._optimizer is not None:
                self._optimizer._upload_hyper()           # host -> device only; the replay reads lr & co. from that block
            if pb is not None and pb.front is not None:
                raise RuntimeError("DataParallelStep: this step was captured by capture_packed(); feed it with step_packed()")
            if pb is not None:
                # packed mode: any padding masks of the captured shapes; the lengths travel as device data (cu_seqlens), the row
                # counts pick the bucket graph (captured now if this bucket was not seen before)
                if m_a is None or m_t is None:
                    raise RuntimeError("DataParallelStep (packed mode): both padding masks are needed")
                ident = (m_a.data_ptr(), m_a._version, m_t.data_ptr(), m_t._version)
                seen = self._mask_seen
                if lengths is None and seen is not None and seen.ident == ident:
                    key = seen.key                        # the same mask tensors as last step: no second device -> host read
                    for buf, saved in zip((pb.cu_a, pb.cu_t, pb.cu_f), seen.cu):
                        buf.copy_(saved)
                else:
                    key = self._packed_key(m_a, m_t, lengths)
                    # the entry HOLDS the masks: while it is the cache entry their addresses cannot be handed to the next batch's
                    # masks (same address + version 0 would otherwise pass for "the same tensors" with other lengths inside)
                    self._mask_seen = _MaskSeen(ident, key, (pb.cu_a.clone(), pb.cu_t.clone(), pb.cu_f.clone()), (m_a, m_t))
            for s, t in zip(self._static, (h_a, h_t, m_a, m_t, y)):
                if s is not None and t is not None and s.data_ptr() != t.data_ptr():
                    s.copy_(t)
            # packed: captures on self._static (already this batch) if the bucket is new
            rec = self._packed_graph(key) if pb is not None else self._record
            rec.graph.replay()
            self._after_replay()
            return rec.loss
        loss = self._fwd_bwd(h_a, h_t, m_a, m_t, y)
        self._update_stats()
        self.buckets.finish()
        if self._optimizer is not None:
            self._optimizer.step()                        # use_graph(False): still the whole trainer step
        return loss


# the switches a captured forward bakes in: name -> how it reads now (eval_packed refuses a replay under another setting)
# POOLED_GATE_FP32 is read by the fp32 precision alone and is recorded only there: in bf16 precision the recorded switches stay the six
# of before (a replay under another precision is refused by the first entry, whatever follows)
def _mode_switches():
    from . import _ops
    six = (("precision", _ops.precision()), ("gemm_mode", _ops.gemm_mode()), ("PACKED_TAIL", bool(_ops.PACKED_TAIL)),
           ("PACKED_TAIL_FP32", bool(_ops.PACKED_TAIL_FP32)), ("PACKED_TAIL_MX8", bool(_ops.PACKED_TAIL_MX8)), ("ingest", _ops.ingest()))
    if _ops.precision() != "fp32":
        return six
    return six + (("POOLED_GATE_FP32", bool(_ops.POOLED_GATE_FP32)),)


class _WeightsPass:
    """What a stationary EvalStep keeps beside its bucket graphs: everything that depends on the parameters alone.
      log      the _ops.FormLog of the weight forms the step's forwards asked for
      records  _GraphRecords replayed in order.  The first holds the forms of the first bucket's forward and the decoder's query
               prologue (its `out`: the static (tgt, tgt32) layer 0 reads, None for a model without a decoder); a later one the
               forms a later bucket asked for first.  Each is recorded by the default capture rule with the step's context not
               stationary: every form once per pass, in the order the forward asked.
      seen     (_ops.WEIGHTS_EPOCH, every parameter's _version) when the pass last ran; ptrs: every parameter's data_ptr() at the
               capture; forms: (Shadows, key) -> the data_ptr()s of that cached form at the capture"""

    def __init__(self, model, B):
        from . import _ops
        from .models.emotion_decoder import EmotionDecoder
        self.model, self.params = model, list(model.parameters())
        self.shadows = [m._sh for m in model.modules() if hasattr(m, "_sh")]
        decoders = [m for m in model.modules() if isinstance(m, EmotionDecoder)]
        self.decoder, self.B = (decoders[0] if decoders else None), B
        self.log, self.records, self.entries = _ops.FormLog(), [], []
        self.seen, self.ptrs, self.forms = None, tuple(p.data_ptr() for p in self.params), {}

    def _body(self, entries, prologue):
        from . import _ops
        ctx = _ops.CTX
        held, ctx.act_log = ctx.act_log, None     # the weights pass is no pass of an activation log: no probe in its graphs
        try:
            with torch.no_grad():
                for _, fn, args in entries:
                    fn(*args)
                out = self.decoder.prologue(self.B) if prologue else None
        finally:
            ctx.act_log = held
        return None, out

    def eager(self):
        """the whole pass as plain launches, by the eager rule: every form whose masters moved, then the prologue (tests, and the
        measurement of what an evaluation behind an update pays)"""
        from . import _ops
        was = self.model.training
        self.model.eval()
        try:
            _ops.begin_step()
            return self._body(self.entries, self.decoder is not None)[1]
        finally:
            self.model.train(was)

    def record(self, dev, new):
        """one more graph: the derivation of the forms `new`, and, in the first, the prologue"""
        prologue = not self.records and self.decoder is not None
        self.records.append(_record_graph(dev, None, None, lambda: self._body(new, prologue), lambda: self._body(new, prologue)))
        self.entries += new
        self.replay()

    def handed(self, decoder, B):
        """_ops.StepContext.prologue of the step's bucket passes"""
        if decoder is not self.decoder or B != self.B or not self.records:
            raise RuntimeError("EvalStep (stationary): the decoder asks for a prologue the weights pass did not record")
        return self.records[0].out

    def state(self):
        from . import _ops
        return (_ops.WEIGHTS_EPOCH, tuple(p._version for p in self.params))

    def moved(self):
        return self.seen != self.state()

    def replay(self):
        for rec in self.records:
            rec.graph.replay()
        self.seen = self.state()

    def _form_ptrs(self):
        out = {}
        for sh in self.shadows:
            for key, ent in sh._d.items():
                form = ent[1]
                out[(id(sh), key)] = tuple(t.data_ptr() for t in (form if isinstance(form, tuple) else (form,)))
        return out

    def note(self):
        """the forms as they lie in memory now, behind a capture: what the bucket graphs point at"""
        self.forms = self._form_ptrs()

    def rehomed(self, forms):
        """None, or what lives elsewhere than at the capture: a parameter, or (looked at with `forms` only: a form's storage
        changes in a refresh, and a refresh needs moved weights) a weight form"""
        if tuple(p.data_ptr() for p in self.params) != self.ptrs:
            return "a parameter"
        if forms:
            now = self._form_ptrs()
            for key, ptrs in self.forms.items():
                if now.get(key) != ptrs:
                    return "a weight form"
        return None

    def release(self):
        for rec in self.records:
            rec.release()
        self.records, self.entries = [], []


class EvalStep(_RaggedStep):
    """The evaluation half of an epoch as graph replays: capture_packed / step_packed of DataParallelStep for the FORWARD alone --
    the reference's evaluate() bodies (train_fusion_seq_level_decoder.py:342-372, train_mosei_fusion_seq_level_decoder.py:432-495)
    and the loop of scripts/infer/mosei_eval_infer.py.  An eager forward is ~150 launches issued from Python; one ``eval_packed``
    is the copies of the batch into the static buffers and one replay.

    EvalStep(model, loss_fn=None, stats=None, log=None, max_graphs=None, attn_log=None, stationary=False, act_log=None): loss_fn(logits, beta, y, n_valid=...) as
    hri_emo_amd.train's losses; stats a ``train.EpochStats``, log a ``train.PredictionLog`` -- both are fed INSIDE the graph, one
    launch each, and never by a warm-up pass.  max_graphs: bucket graphs kept alive (default HRIEMO_VARLEN_MAX_GRAPHS), least
    recently replayed one released first.  The step has its own ``_ops.StepContext`` and its own graph pool, creates no gradient
    buffers and leaves the module's training flag, torch's CPU generator and the device seed word as it found them.

    What a bucket graph holds, in this order: hriemo_seq_tables (lengths block -> cu_seqlens and masks), the model's
    ``_forward_rows`` in eval mode under no_grad, the loss (when a loss_fn and targets were given at capture), stats.update,
    log.update -- each with n_valid read from the control block, so a batch of 1 <= n <= B utterances is served by the graphs
    captured for B (ghost utterances of length 1, ghost_plan).  No seed bump, no zero-grad, no backward, no optimizer.  The bf16 /
    MX weight shadows are re-cast inside the graph: an evaluation that follows optimizer replays sees the new weights.
    attn_log: a ``train.AttentionLog`` -- the attention maps of the split's first `capacity` samples from the same replays.  The
    graph then holds, directly behind hriemo_seq_tables and so in front of every fork, the log's plan launch (hriemo_attn_log_plan
    on the step's n_valid word and lengths block), and every attention site the log keeps exports under the window that launch
    wrote: the varlen sites straight into their log slots (hriemo_attn_probs_varlen_log / _log_fp32), the decoder's padded
    map -- packed tail off -- through one append.  Once the log is full those launches are blocks that read the window and exit, so
    one family of bucket graphs serves the whole split.  Warm-up passes run with the closed window and leave the log bit-unchanged.
    Needs set_varlen_maps(True); varlen_maps() and mfma_maps() then join the switches recorded at capture.  ``return_attention``
    itself is not part of the captured step.
    act_log: a ``train.ActivationLog`` -- every evaluation is one pass of it, forward half only: the log's plan launch at the top of
    the model's forward (in front of every fork), a probe behind every sub-layer the log keeps, one fold at the forward's end; the
    ghosts behind n_valid never count.  Warm-up passes run under the closed window.  A stationary step's dec0.self runs in the
    weights pass, which is no pass of the log: that site stays absent.

    stationary=True: a bucket graph holds only what depends on the batch.  What depends on the parameters alone -- every weight
    form the forward asks for (bf16 shadows, concatenations, padded and MX-fp8 copies, the fp32 mode's splits) and the decoder's
    query prologue (EmotionDecoder.prologue: the broadcast queries and layer 0's self-attention sub-layer) -- lives in the step's
    WEIGHTS PASS: one more captured graph (a further one for forms a later bucket asks for first), recorded in front of the first
    bucket graph by the default capture rule, so its launches and the bucket graph's are together those of a default bucket
    graph, and the values are the same bits.  eval_packed / eval_store replay it in front of the bucket graph only when the
    weights moved since it last ran: _ops.WEIGHTS_EPOCH changed (captured optimizer replays, DeviceAdamW.step,
    FusedClipAdamW.step) or the _version of a parameter did (torch.optim, load_state_dict, in-place edits) -- host arithmetic,
    nothing is read back.  Every form is refreshed in the storage the bucket graphs point at; when a parameter or a form has
    moved to other memory since the capture (a DeviceAdamW built afterwards, .to()) the call raises RuntimeError("... capture
    again") before anything is enqueued.  The default, False, is launch for launch the step without the option; use_graph(False)
    ignores it."""

    _label = "eval step"

    def __init__(self, model, loss_fn=None, stats=None, log=None, max_graphs=None, attn_log=None, stationary=False, act_log=None):
        if max_graphs is not None and int(max_graphs) < 1:
            raise ValueError("EvalStep: max_graphs is a positive integer (or None)")
        super().__init__(model, loss_fn)
        self.stats, self.log, self.attn_log = stats, log, attn_log
        if act_log is not None:
            act_log._guard()
        self.act_log = self.ctx.act_log = act_log
        self.max_graphs = None if max_graphs is None else int(max_graphs)
        self.stationary = bool(stationary)
        self._modes = None                 # _mode_switches() at capture
        self._weights = None               # _WeightsPass of a stationary step, from its first bucket capture to release_graph()

    def use_graph(self, on):
        """False: eval_packed is the eager forward_packed evaluation (same outputs, same updates of stats and log)"""
        self._replay = bool(on) and self.captured

    def release_graph(self):
        """drop the captured step: the graphs (a stationary step's weights pass included), their outputs, the buffers their kernels
        point into, the static state"""
        self._release_buckets()
        if self._weights is not None:
            torch.cuda.synchronize()
            self._weights.release()
        self._pb = self._static = self._modes = self._weights = None

    def _switches(self):
        """the switches a replay depends on: with an attention log also the two that pick the export kernels"""
        from . import _ops
        if self.attn_log is None:
            return _mode_switches()
        return _mode_switches() + (("varlen_maps", _ops.varlen_maps()), ("mfma_maps", _ops.mfma_maps()))

    @_in_step_context
    def capture_packed(self, rows_a, rows_t, lengths_a, lengths_t, y=None, pad_to=None):
        """Capture the evaluation of ragged batches (data.collate_seq_packed): the arguments of DataParallelStep.capture_packed, y
        optional.  pad_to = (L_a, L_t) and B = the number of utterances of this batch are fixed from here on; ``eval_packed`` then
        serves every batch of 1 <= n <= B utterances.  With y (and a loss_fn) the graphs compute the loss and feed `stats`; with
        y=None they are prediction-only: logits, beta, z and the log.  Static state as capture_packed builds it: zero-initialised
        row sources of the largest bucket in the rows' dtype, the lengths as one int32 [2, B] block with a pinned twin, three
        cu_seqlens and three mask buffers, y, and the control block whose n_valid word the loss, the statistics and the log read.
        The switches in force now -- precision(), gemm_mode(), the three packed-tail flags, ingest(), with an attention log also
        varlen_maps() and mfma_maps() -- are recorded.  With an attention log, a capture without set_varlen_maps(True) or with a
        log whose pad_to, layer counts or num_emotions are not the model's and this call's is a ValueError that leaves the step
        (and the log) as it was."""
        from . import _ops
        self._need_forward_packed("EvalStep.capture_packed")
        if self.loss_fn is not None and y is not None:
            self._need_n_valid("EvalStep.capture_packed")
        if self.stats is not None and (self.loss_fn is None or y is None):
            raise ValueError("EvalStep.capture_packed: statistics need a loss_fn and targets (prediction-only graphs feed the log)")
        same_width = not hasattr(self.model, "audio_proj")
        la, lt, pad = _ops.packed_lengths(rows_a, rows_t, lengths_a, lengths_t, pad_to, same_width=same_width)
        if pad_to is None:
            raise ValueError("EvalStep.capture_packed: pad_to=(L_a, L_t) is required")
        if y is not None and y.shape[0] != len(la):
            raise ValueError(f"EvalStep.capture_packed: targets of shape {tuple(y.shape)} for {len(la)} utterances")
        dev = next(self.model.parameters()).device
        self._capture_ragged(lambda: self._begin_ragged("capture_packed", pad), (rows_a.shape[1], rows_t.shape[1]), rows_a.dtype,
                             None if y is None else y.to(dev, copy=True), la, lt, pad, lambda: self._load_packed(rows_a, rows_t, la, lt, y))

    def _begin_ragged(self, entry, pad):
        """_capture_ragged's begin(): the attention log's refusals, then the old graphs go and the switches in force are recorded"""
        from . import _ops
        if self.attn_log is not None:
            if not _ops.varlen_maps():
                raise ValueError(f"EvalStep.{entry}: attention maps of packed rows need set_varlen_maps(True)")
            why = self.attn_log.mismatch(self.model, pad)
            if why is not None:
                raise ValueError(f"EvalStep.{entry}: the attention log does not fit: {why}")
        self.release_graph()              # a re-capture replaces the old graphs
        self._modes = self._switches()
        self._replay = True

    @_in_step_context
    def capture_store(self, store, ids, pad_to=None):
        """capture_packed() for batches that are lists of utterance ids of a ``data.DeviceFeatureStore`` on the model's device, built as
        DataParallelStep.capture_store is: `ids` fixes B, pad_to defaults to ``store.pad_to``; the graphs are those of capture_packed
        (with the store's targets when the step has a loss_fn, prediction-only without); ``eval_store(ids)`` uploads one plan block
        and launches hriemo_gather_rows once per operand in front of the replay.  stats, log and attn_log work as before.  While the
        step is captured the store refuses ``append``."""
        self._need_forward_packed("EvalStep.capture_store")
        targets = self.loss_fn is not None
        if targets:
            self._need_n_valid("EvalStep.capture_store")
        if self.stats is not None and not targets:
            raise ValueError("EvalStep.capture_store: statistics need a loss_fn (prediction-only graphs feed the log)")
        ids, la, lt, pad, y_static = self._store_capture("EvalStep.capture_store", store, ids, pad_to, targets)
        self._capture_ragged(lambda: self._begin_ragged("capture_store", pad), store.widths, store.dtype, y_static, la, lt, pad,
                             lambda: self._load_store(ids, la, lt), store)

    @_in_step_context
    def eval_store(self, ids):
        """One evaluation of the utterances `ids` (1 <= n <= B) of the captured store -> (logits [n, C], beta, z, loss | None):
        eval_packed with "copy the caller's rows" replaced by "gather by id".  The ids ALWAYS refer to the store given to
        capture_store -- ``self.store``: a step captured on the validation store evaluates the validation store whatever the ids
        were meant for, so one step per store (or a new capture_store); train.evaluate_store refuses a step of another store.  Host checks first (the store as it was at capture:
        RuntimeError after an append or a mode switch; ids, n and lengths: ValueError), nothing is enqueued when one fails.  The
        returned tensors are views of the replayed graph's outputs, as eval_packed's.  After use_graph(False): the eager evaluation of
        ``store.fetch(ids)``."""
        pb, feed = self._pb, self._feed
        if pb is None or feed is None:
            raise RuntimeError("eval_store needs capture_store() first")
        ids, la, lt = feed.batch(ids, True, "eval_store")
        targets = self._static[4] is not None
        if not self._replaying:
            rows_a, _, rows_t, _, y = feed.store.fetch(ids)
            return self._eval_eager(rows_a, rows_t, la, lt, y if targets else None)
        self._check_modes("eval_store", "capture_store")
        moved = self.stationary and self._weights_moved("eval_store")
        return self._replay_bucket(self._load_store(ids, la, lt), len(ids), moved)

    def _pass(self, record):
        """one evaluation on the static state, as every warm-up pass runs it and the capture records it; record: the pass feeds
        stats, log and attention log (the capture pass only; a warm-up pass runs the exports under the closed window)
        -> (loss | None, (logits, beta, z)), the form _record_graph takes"""
        act = self.act_log
        if act is not None and not record:
            with act.paused():                    # the activation log's probes likewise
                return self._pass_body(record)
        return self._pass_body(record)

    def _pass_body(self, record):
        from . import _ops
        pb = self._pb
        front = pb.front
        seqs = _ops.CTX.seq_override
        y = self._static[4]
        with torch.no_grad():
            _ops.seq_tables(front.lens.dev, pb.La, pb.Lt, rows=(seqs[0].N, seqs[1].N), cu=(pb.cu_a, pb.cu_t, pb.cu_f), masks=front.masks)
            n_valid = front.ctl.dev[:1]
            if self.act_log is not None:
                self.act_log.n_valid = n_valid
            if self.attn_log is not None:
                self.attn_log.plan(front.lens.dev, n_valid, pb.B, record=record)
                logits, beta, z = self.model._forward_rows(self._static[0], self._static[1], tuple(seqs), front.bool, (pb.La, pb.Lt),
                                                           attn_log=self.attn_log)
            else:
                logits, beta, z = self.model._forward_rows(self._static[0], self._static[1], tuple(seqs), front.bool, (pb.La, pb.Lt))
            loss = self.loss_fn(logits, beta, y, n_valid=n_valid) if (self.loss_fn is not None and y is not None) else None
            if record and self.stats is not None:
                self.stats.update(logits, beta, y, loss, n_valid=n_valid)
            if record and self.log is not None:
                self.log.update(logits, beta, n_valid=n_valid)
        return loss, (logits, beta, z)

    def _capture_bucket(self, seqs):
        """the bucket graph of the plans `seqs` (_PackedState.graph): the module in eval mode while it is warmed up and recorded"""
        from . import _ops
        was = self.model.training
        self.model.eval()
        try:
            if not self.stationary:
                return _record_graph(self._static[0].device, seqs, self._pb.pool, lambda: self._pass(False), lambda: self._pass(True))
            # stationary: the weights pass first (the forms this bucket's forward asks for, the prologue), then the bucket's passes
            # with the rule switched -- the warm-up passes find every form fresh, the capture pass must (_ops.form_stale raises)
            self._prepare_weights(seqs)
            ctx = _ops.CTX
            ctx.stationary, ctx.prologue = True, self._weights.handed
            try:
                return _record_graph(self._static[0].device, seqs, self._pb.pool, lambda: self._pass(False), lambda: self._pass(True))
            finally:
                ctx.stationary, ctx.prologue = False, None
        finally:
            self.model.train(was)

    def _prepare_weights(self, seqs):
        """in front of a stationary bucket capture, module in eval mode: one eager default pass on the bucket's plans under a FormLog
        finds the weight forms this forward asks for; the ones not known yet are recorded, with the prologue the first time, as a
        further graph of the weights pass, which is then replayed once: its outputs are what the bucket graphs read"""
        from . import _ops
        dev = self._static[0].device
        if self._weights is None:
            self._weights = _WeightsPass(self.model, self._pb.B)
        wp, ctx = self._weights, _ops.CTX
        side = _capture_streams.get(dev.index)
        if side is None:
            side = _capture_streams[dev.index] = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        ctx.seq_override, ctx.forms = seqs, wp.log
        try:
            with torch.cuda.stream(side):
                self._pass(False)
        finally:
            ctx.seq_override, ctx.forms = None, None
        torch.cuda.current_stream().wait_stream(side)
        new = wp.log.take()
        if new or (not wp.records and wp.decoder is not None):
            wp.record(dev, new)
        wp.note()

    def _weights_moved(self, who):
        """host arithmetic in front of a stationary replay -> did the weights move since the weights pass last ran?  RuntimeError,
        before anything is enqueued, when a parameter or a weight form lives in other memory than at the capture"""
        wp = self._weights
        if wp is None:
            return False
        moved = wp.moved()
        why = wp.rehomed(forms=moved)
        if why is not None:
            raise RuntimeError(f"EvalStep.{who}: {why} moved to other memory since the capture (an optimizer built afterwards, .to()): "
                               "the stationary bucket graphs still point at the old one -- capture again")
        return moved

    def _replay_bucket(self, key, n, moved=False):
        """the graph of bucket `key` (captured now if it is new) replayed on the static state -> the outputs of its first n samples;
        moved: a stationary step whose weights moved (_weights_moved) -- its weights pass goes first"""
        if moved:
            self._weights.replay()                # the weights moved: every form and the prologue again, into the same storage
        rec = self._packed_graph(key)
        rec.graph.replay()
        logits, beta, z = rec.out
        return logits[:n], beta[:n], z[:n], rec.loss

    def _check_modes(self, entry="eval_packed", capture="capture_packed"):
        for (name, then), (_, now) in zip(self._modes, self._switches()):
            if then != now:
                raise RuntimeError(f"EvalStep.{entry}: the step was captured with {name} = {then!r}; it is {now!r} now -- "
                                   f"{capture}() again under the new setting, or switch back")

    @_in_step_context
    def eval_packed(self, rows_a, rows_t, lengths_a, lengths_t, y=None):
        """One evaluation of a ragged batch of 1 <= n <= B utterances -> (logits [n, C], beta, z, loss | None).  The arguments are
        checked on the host first -- a refusal (ValueError; RuntimeError for a mode switch that changed since the capture) leaves
        every static buffer untouched -- then rows, lengths, n_valid and y are copied into the static state and the batch's bucket
        graph is replayed (captured on the spot if the bucket is new).

        The returned tensors are VIEWS of the replayed graph's own output tensors, cut to the first n samples: they are valid until
        the graph of the same bucket is replayed again (clone what must outlive that).  loss is the 0-dim tensor the replay wrote:
        the mean over the batch's n utterances.  After use_graph(False) this is the eager model.eval() + forward_packed evaluation
        with the same outputs and the same updates of stats and log."""
        from . import _ops
        pb = self._pb
        if pb is None:
            raise RuntimeError("eval_packed needs capture_packed() first")
        la, lt, _ = _ops.packed_lengths(rows_a, rows_t, lengths_a, lengths_t, (pb.La, pb.Lt), same_width=pb.front.same_width)
        n = len(la)
        if not self._replaying:
            return self._eval_eager(rows_a, rows_t, la, lt, y)
        self._check_modes()
        sy = self._static[4]
        if sy is None and y is not None:
            raise ValueError("eval_packed: targets given, but the step was captured without (prediction-only graphs)")
        if sy is not None and y is None:
            raise ValueError("eval_packed: the step was captured with targets; this batch has none")
        self._check_batch("eval_packed", rows_a, rows_t, n, y)
        moved = self.stationary and self._weights_moved("eval_packed")
        return self._replay_bucket(self._load_packed(rows_a, rows_t, la, lt, y), n, moved)

    def _eval_eager(self, rows_a, rows_t, la, lt, y):
        pb = self._pb
        dev = self._static[0].device
        was = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                if self.act_log is not None:
                    self.act_log.n_valid = None
                extra = {} if self.attn_log is None else {"attn_log": self.attn_log}
                logits, beta, z = self.model.forward_packed(rows_a.to(dev, non_blocking=True), rows_t.to(dev, non_blocking=True), la, lt,
                                                            pad_to=(pb.La, pb.Lt), **extra)
                loss = None
                if self.loss_fn is not None and y is not None:
                    y = y.to(dev, non_blocking=True)
                    loss = self.loss_fn(logits, beta, y)
                    if self.stats is not None:
                        self.stats.update(logits, beta, y, loss)
                if self.log is not None:
                    self.log.update(logits, beta)
        finally:
            self.model.train(was)
        return logits, beta, z, loss
