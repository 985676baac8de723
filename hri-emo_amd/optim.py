"""clip_grad_norm_(max_norm) + AdamW for the fusion path as two HIP passes over flat buffers
(scripts/fusion/train_fusion_seq_level_decoder.py:332-334).

The gradients already live in ONE flat fp32 buffer (dp.GradBuckets).  This optimizer gives the parameters and both
Adam moments the same layout -- every ``p.data`` becomes a view into a flat parameter buffer -- so the whole update
is one elementwise kernel and the gradient norm one reduction, with the clip coefficient taken from device memory
(no host synchronisation, safe between hipGraph replays).  Construct it BEFORE ``DataParallelStep.capture()``:
it moves the parameter storage.  Results follow torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (fp32)."""
import contextlib

import torch

from . import _lib
from . import _ops
from ._ops import _p, _stream, _require_gpu


class FusedClipAdamW:
    def __init__(self, buckets, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=5.0):
        self.buckets = buckets
        flat_g = buckets.flat
        _require_gpu(flat_g)
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_norm
        self.flat_p = torch.zeros_like(flat_g)
        self.m = torch.zeros_like(flat_g)
        self.v = torch.zeros_like(flat_g)
        with torch.no_grad():
            for p in buckets.params:
                off, n = buckets._offsets[id(p)], p.numel()
                view = self.flat_p[off:off + n].view_as(p)
                view.copy_(p.data)
                p.data = view                       # same values, storage now inside the flat buffer
        self.nblocks = 1024
        self._partial = torch.empty(self.nblocks, dtype=torch.float32, device=flat_g.device)
        self._norm2 = torch.zeros(1, dtype=torch.float32, device=flat_g.device)
        self.steps = 0

    @torch.no_grad()
    def step(self):
        """One update from the gradients currently in the flat buffer; returns the pre-clip gradient norm (device)."""
        g = self.buckets.flat
        n = g.numel()
        st = _stream()
        self.steps += 1
        _lib.call("hriemo_sumsq_f32", _p(g), n, _p(self._partial), self.nblocks, st)
        _lib.call("hriemo_rowsum_f32", _p(self._partial), _p(self._norm2), 1, self.nblocks, st)
        _lib.call("hriemo_adamw_flat", _p(self.flat_p), _p(g), _p(self.m), _p(self.v), n, self.lr, self.betas[0], self.betas[1],
                  self.eps, self.wd, self.steps, self.max_norm if self.max_norm else 0.0, _p(self._norm2), st)
        # the update went through raw pointers: neither p._version nor p.data_ptr() moved, so tell the bf16 weight
        # shadows explicitly (eager steps would otherwise keep running on the initial weights)
        _ops.bump_weights_epoch()
        return self._norm2.sqrt()


MAX_GROUPS = 16            # hriemo_adamw_flat_groups: rows of hyper / state
MAX_SEGMENTS = 2048        # hriemo_adamw_flat_groups: entries of the segment table a block keeps in LDS
AVERAGING_MODES = {"ema": 1.0, "swa": 2.0}     # avg_hyper[0] of hriemo_optim_finalize_avg (0: off)


def is_averaging_step(t, avg_start, avg_every):
    """does the real update that brings the step count to ``t`` fold the parameters into the average?  The rule the finalize kernel
    evaluates on the device (host mirror: tests, logging)."""
    return t > avg_start and (t - avg_start) % avg_every == 0


def averaging_weight(mode, n_averaged, avg_decay):
    """the weight ``w`` of ``avg += w * (p - avg)`` for an averaging update that finds ``n_averaged`` >= 1 earlier ones, in float64
    (the device rounds ``1 - decay`` and ``1 / (n + 1)`` once, in fp32)"""
    return 1.0 - avg_decay if mode == "ema" else 1.0 / (n_averaged + 1)


def decay_groups(named_parameters, weight_decay, no_decay=lambda name, p: p.dim() < 2):
    """The usual two groups for ``DeviceAdamW(buckets, param_groups=...)`` from ``model.named_parameters()``: every trainable
    parameter for which ``no_decay(name, p)`` holds (default: vectors -- biases, LayerNorm gains and biases) gets
    ``weight_decay = 0.0``, the rest ``weight_decay``.  GradBuckets lays all matrices in front of all vectors, so the default
    split is ONE boundary in the flat buffer.  A group that would be empty is left out."""
    decay, rest = [], []
    for name, p in named_parameters:
        if p.requires_grad:
            (rest if no_decay(name, p) else decay).append(p)
    groups = [{"params": decay, "weight_decay": weight_decay}, {"params": rest, "weight_decay": 0.0}]
    return [g for g in groups if g["params"]]


def _describe(p):
    return f"shape {tuple(p.shape)}"


def _materialise(param_groups):
    """-> new group dicts whose 'params' are lists, each group's params read exactly ONCE: torch's idiom
    ``{"params": model.backbone.parameters(), "lr": 3e-5}`` hands over a generator, which a second reader would find empty.  The
    caller's dicts are not modified (a generator inside them is spent afterwards, as after torch.optim.AdamW(groups))."""
    groups = list(param_groups)
    if not groups or not all(isinstance(g, dict) and "params" in g for g in groups):
        raise ValueError("DeviceAdamW: param_groups is a non-empty list of dicts with a 'params' entry")
    return [{**g, "params": [g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])} for g in groups]


def _group_of_params(buckets, groups):
    """-> {id(p): group index} after checking that the materialised groups PARTITION buckets.params (ValueError names the offender)"""
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"DeviceAdamW: {len(groups)} param groups; the grouped update kernel takes at most {MAX_GROUPS}")
    index = {id(p): i for i, p in enumerate(buckets.params)}
    owner = {}
    for gi, g in enumerate(groups):
        for j, p in enumerate(g["params"]):
            if not isinstance(p, torch.Tensor) or id(p) not in index:
                what = _describe(p) if isinstance(p, torch.Tensor) else repr(type(p))
                raise ValueError(f"DeviceAdamW: param_groups[{gi}]['params'][{j}] ({what}) is foreign: not one of the buckets' parameters")
            if id(p) in owner:
                raise ValueError(f"DeviceAdamW: buckets.params[{index[id(p)]}] ({_describe(p)}) is repeated: it appears in "
                                 f"param_groups[{owner[id(p)]}] and again in param_groups[{gi}]")
            owner[id(p)] = gi
    for i, p in enumerate(buckets.params):
        if id(p) not in owner:
            raise ValueError(f"DeviceAdamW: buckets.params[{i}] ({_describe(p)}) is missing: it appears in no param group "
                             "(the groups must partition the buckets' parameters)")
    return owner


def group_segments(buckets, param_groups):
    """The segment table of hriemo_adamw_flat_groups for these groups over ``buckets.flat``: ``(seg, seg_group)``, two lists of host
    integers -- ``seg`` has S + 1 ascending element offsets (``seg[0] = 0``, ``seg[S] = buckets.flat.numel()``, multiples of 64),
    ``seg_group[s]`` is the group that owns elements ``seg[s] .. seg[s + 1] - 1``.  Parameters are walked in flat-buffer order;
    neighbours of one group are merged into one segment, and a parameter's padding up to its 64-element boundary belongs to that
    parameter's segment (it holds zeros in all four buffers and stays zero under any group's update).  Pure host code: works on
    buckets in host memory.  ValueError if the groups do not partition ``buckets.params``.  A group whose ``params`` is a generator
    is read once here and is spent afterwards: hand over lists when the groups go on to ``DeviceAdamW``."""
    owner = _group_of_params(buckets, _materialise(param_groups))
    seg, seg_group = [0], []
    for p in sorted(buckets.params, key=lambda q: buckets._offsets[id(q)]):
        off, g = buckets._offsets[id(p)], owner[id(p)]
        if seg_group and seg_group[-1] == g:
            continue
        if seg_group:
            seg.append(off)
        seg_group.append(g)
    seg.append(buckets.flat.numel())
    return seg, seg_group


HEALTH_CHUNK = 32768       # elements per block of hriemo_health_sweep (one resident round of blocks at cfg 2)
MAX_HEALTH_PARAMS = 4096   # hriemo_health_fold: parameters whose chunk ranges the one block keeps in LDS
MAX_HEALTH_CAPACITY = 1 << 20


def health_chunks(slots, chunk=HEALTH_CHUNK):
    """The chunk table of hriemo_health_sweep / hriemo_health_fold: ``slots`` is one ``(start, length, group)`` per parameter in
    flat-buffer order -- the parameter's slot of the flat buffers as GradBuckets lays it out (``start`` a multiple of 64 elements,
    ``length`` the element count padded to 64) and the param group that owns it.  -> a list of ``(start, length, parameter, group)``
    rows: every slot cut into pieces of at most ``chunk`` elements (a positive multiple of 1024), the pieces of one parameter
    neighbours in ascending order, every element of every slot in exactly one row.  Pure host code."""
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1024 or chunk % 1024:
        raise ValueError(f"health_chunks: chunk={chunk!r} must be a positive multiple of 1024")
    rows, end = [], 0
    for i, (start, length, group) in enumerate(slots):
        if start % 64 or length % 64 or length <= 0 or start < end:
            raise ValueError(f"health_chunks: slot {i} (start {start}, length {length}): slots start at multiples of 64 elements, are "
                             "padded to 64 and ascend without overlap")
        end = start + length
        for off in range(0, length, chunk):
            rows.append((start + off, min(chunk, length - off), i, group))
    if not rows:
        raise ValueError("health_chunks: no slots")
    return rows


CLIP_MODES = ("global", "group", "parameter")     # DeviceAdamW(clip=...)


def clip_units(buckets, param_groups, mode):
    """The tables of the unit clip modes (``DeviceAdamW(clip="group" | "parameter")``: hriemo_sumsq_units,
    hriemo_optim_finalize_units, hriemo_adamw_flat_units) for these groups over ``buckets.flat`` -- a dict of host integers:

    * ``seg`` [S + 1], ``seg_group`` [S]: the segment table of the update kernel.  ``mode="group"``: ``group_segments``' table
      (neighbours of one group merged).  ``mode="parameter"``: ONE segment per parameter slot, neighbours never merged.
    * ``seg_unit`` [S]: the clip unit of every segment -- the group index, or the parameter's index in flat-buffer order.
    * ``unit_group`` [U]: the group whose ``max_norm`` clips unit u.
    * ``chunks``: rows ``(start, length, unit, group)`` -- every segment cut the way ``health_chunks`` cuts a slot (pieces of at
      most 32768 elements, starts at 64-element boundaries), ordered by unit, then by start; every element of the flat buffer lies in
      exactly one row.  ``unit_chunks`` [U + 1]: unit u owns rows ``unit_chunks[u] .. unit_chunks[u + 1] - 1``.

    Pure host code: works on buckets in host memory.  ValueError (by name, before anything is allocated) for groups that do not
    partition ``buckets.params``, more than 16 groups, a group without parameters, more than 2048 units or 2048 segments."""
    if mode not in ("group", "parameter"):
        raise ValueError(f"clip_units: mode={mode!r}; the unit modes are 'group' and 'parameter'")
    groups = _materialise(param_groups)
    owner = _group_of_params(buckets, groups)
    for gi, g in enumerate(groups):
        if not g["params"]:
            raise ValueError(f"DeviceAdamW: param_groups[{gi}] holds no parameter: with clip={mode!r} it would be a clip unit of nothing")
    n = buckets.flat.numel()
    if mode == "group":
        seg, seg_group = group_segments(buckets, groups)
        seg_unit, unit_group = list(seg_group), list(range(len(groups)))
    else:
        order = sorted(buckets.params, key=lambda q: buckets._offsets[id(q)])
        seg = [buckets._offsets[id(p)] for p in order] + [n]
        seg_group = [owner[id(p)] for p in order]
        seg_unit, unit_group = list(range(len(order))), list(seg_group)
    S, U = len(seg_group), len(unit_group)
    if U > MAX_SEGMENTS:
        raise ValueError(f"DeviceAdamW: clip={mode!r} makes {U} clip units; the unit kernels take at most {MAX_SEGMENTS}")
    if S > MAX_SEGMENTS:
        raise ValueError(f"DeviceAdamW: the groups cut the flat buffer into {S} segments; the grouped update kernel takes at most "
                         f"{MAX_SEGMENTS} (group neighbouring parameters together)")
    chunks, unit_chunks = unit_chunk_table(seg, seg_unit, unit_group)
    return {"seg": seg, "seg_group": seg_group, "seg_unit": seg_unit, "unit_group": unit_group, "chunks": chunks, "unit_chunks": unit_chunks}


def unit_chunk_table(seg, seg_unit, unit_group):
    """``(chunks, unit_chunks)`` of ``clip_units`` from a segment table: every segment cut by ``health_chunks``, the rows
    ``(start, length, unit, group)`` ordered by unit, then by start.  The table addresses the gradient buffer, so it is checked
    here, where it is built: the rows tile ``[0, seg[-1])`` exactly once, start and end at 64-element boundaries, hold at most
    32768 elements, and every unit owns at least one row (ValueError otherwise)."""
    S, U, n = len(seg_unit), len(unit_group), seg[-1]
    if len(seg) != S + 1 or any(not 0 <= u < U for u in seg_unit):
        raise ValueError(f"unit_chunk_table: {len(seg)} offsets for {S} segments, or a segment's unit outside 0 .. {U - 1}")
    cut = health_chunks([(seg[s], seg[s + 1] - seg[s], seg_unit[s]) for s in range(S)])
    chunks = sorted(((start, length, unit, unit_group[unit]) for start, length, _, unit in cut), key=lambda r: (r[2], r[0]))
    unit_chunks = [0] * (U + 1)
    for row in chunks:
        unit_chunks[row[2] + 1] += 1
    for u in range(U):
        unit_chunks[u + 1] += unit_chunks[u]
    covered = sorted((start, start + length) for start, length, _, _ in chunks)
    if (covered[0][0] != 0 or covered[-1][1] != n or any(a[1] != b[0] for a, b in zip(covered, covered[1:]))
            or any(start % 64 or length % 64 or not 0 < length <= HEALTH_CHUNK for start, length, _, _ in chunks)
            or any(unit_chunks[u + 1] <= unit_chunks[u] for u in range(U))):
        raise ValueError("unit_chunk_table: the chunks do not tile the flat buffer once, or a unit owns none (segments start at "
                         "64-element boundaries, without gaps, and every unit owns a segment)")
    return chunks, unit_chunks


def decode_health(image, n_params, capacity):
    """One host image of the log's device buffer (int32 words, csrc/health.hip) -> the dict ``HealthLog.arrays()`` returns, without
    the names: the records still in the ring in chronological order, oldest first."""
    import numpy as np
    img = np.ascontiguousarray(np.asarray(image, dtype=np.int32))
    P, R = n_params, 4 + 4 * n_params
    if img.shape != (4 + capacity * R,):
        raise ValueError(f"decode_health: an image of {img.shape} words; {n_params} parameters and capacity {capacity} make {4 + capacity * R}")
    n_recorded = int(img[0]) & 0xFFFFFFFF
    kept = min(n_recorded, capacity)
    ring = img[4:].reshape(capacity, R)
    order = [(n_recorded - kept + i) % capacity for i in range(kept)]
    recs = ring[order]
    f32 = lambda a: np.ascontiguousarray(a).view(np.float32)  # noqa: E731
    return {"n_recorded": n_recorded, "step": f32(recs[:, 0]), "kind": recs[:, 1].copy(), "grad_norm": f32(recs[:, 2]),
            "grad_sq": f32(recs[:, 4:4 + P]), "nonfinite": recs[:, 4 + P:4 + 2 * P].copy(), "weight_sq": f32(recs[:, 4 + 2 * P:4 + 3 * P]),
            "update_sq": f32(recs[:, 4 + 3 * P:4 + 4 * P])}


class HealthLog:
    """Per-parameter statistics of DeviceAdamW's steps, recorded by the step itself -- eagerly or inside any captured step -- into a
    ring in device memory and read back once, when asked: ``DeviceAdamW(buckets, ..., health=HealthLog(capacity=64, every=1))``.

    A step writes a **record** when its update was SKIPPED (always) or when it was a real update whose new step count ``t``
    satisfies ``t % every == 0``; a held accumulation micro-step writes nothing.  A record holds ``step``, ``kind`` (0 real update,
    1 skipped on a non-finite norm, 2 skipped on ``found_inf`` alone), ``grad_norm`` and, per parameter tensor in flat-buffer order,
    ``grad_sq`` (sum of squares of the unscaled gradient over its finite elements), ``nonfinite`` (how many elements are NaN or
    +-Inf, exact), ``weight_sq`` (the parameter after the update) and ``update_sq`` (the Adam term subtracted in this step); the last
    two are zeros on a skipped record.  ``capacity`` records are kept, the newest overwrite the oldest.  ``capacity`` and ``every`` are
    baked into captured graphs: they are fixed at construction.  The log is a diagnostic: it never enters ``state_dict()``.

    ``arrays()`` is ONE device -> host copy; ``blame()`` and ``ratios()`` are built on it."""

    def __init__(self, capacity=64, every=1):
        for name, val, high in (("capacity", capacity, MAX_HEALTH_CAPACITY), ("every", every, 2 ** 24 - 1)):
            if isinstance(val, bool) or not isinstance(val, int) or not 1 <= val <= high:
                raise ValueError(f"HealthLog: {name}={val!r} must be an integer in 1 .. {high}")
        self._capacity, self._every = capacity, every
        self._opt = None
        self.names = None

    capacity = property(lambda self: self._capacity)
    every = property(lambda self: self._every)

    @capacity.setter
    def capacity(self, value):
        raise AttributeError("HealthLog.capacity is fixed at construction: captured graphs carry it (build a new log and optimizer)")

    @every.setter
    def every(self, value):
        raise AttributeError("HealthLog.every is fixed at construction: captured graphs carry it (build a new log and optimizer)")

    def _check_attach(self, buckets):
        """DeviceAdamW's constructor, in front of its first allocation"""
        if self._opt is not None:
            raise ValueError("HealthLog: this log is already attached to an optimizer; every DeviceAdamW takes its own")
        if len(buckets.params) > MAX_HEALTH_PARAMS:
            raise ValueError(f"HealthLog: {len(buckets.params)} parameter tensors; the fold kernel takes at most {MAX_HEALTH_PARAMS}")

    def _attach(self, opt, owner):
        """owner: {id(p): group index}.  Builds the chunk table (uploaded here, once), the partials and the zeroed ring."""
        buckets = opt.buckets
        self._opt = opt
        self._params = sorted(buckets.params, key=lambda q: buckets._offsets[id(q)])
        self.n_params = len(self._params)
        pad = lambda n: (n + 63) // 64 * 64  # noqa: E731
        rows = health_chunks([(buckets._offsets[id(p)], pad(p.numel()), owner[id(p)]) for p in self._params])
        dev = buckets.flat.device
        self._chunks = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.n_chunks = len(rows)
        self._partial = torch.zeros(self.n_chunks * 4, dtype=torch.float32, device=dev)
        self._buf = torch.zeros(4 + self._capacity * (4 + 4 * self.n_params), dtype=torch.int32, device=dev)
        self.names = [f"param{i}" for i in range(self.n_params)]

    def _require_attached(self, what):
        if self._opt is None:
            raise RuntimeError(f"HealthLog.{what}: the log is not attached (DeviceAdamW(buckets, health=log))")

    def _enqueue(self, opt, grad_scale, ctl):
        """the two launches behind the update kernel, on the current stream"""
        st = _stream()
        g = opt.buckets.flat
        G = len(opt.param_groups)
        _lib.call("hriemo_health_sweep", _p(g), _p(opt.flat_p), _p(opt.m), _p(opt.v), g.numel(), _p(self._chunks), self.n_chunks,
                  _p(opt._hyper), _p(opt._state), G, _p(ctl), self._every, _p(self._partial), st)
        _lib.call("hriemo_health_fold", _p(self._partial), _p(self._chunks), self.n_chunks, self.n_params, _p(opt._state), _p(ctl),
                  _p(grad_scale), self._every, self._capacity, _p(self._buf), st)

    def name_parameters(self, named_parameters):
        """names from ``model.named_parameters()``: parameters the optimizer does not own are ignored, a parameter of the optimizer
        that gets no name raises (nothing is changed then)"""
        self._require_attached("name_parameters()")
        given = {id(p): name for name, p in named_parameters}
        for i, p in enumerate(self._params):
            if id(p) not in given:
                raise ValueError(f"HealthLog.name_parameters: parameter {i} of the optimizer ({_describe(p)}) has no name")
        self.names = [given[id(p)] for p in self._params]

    def arrays(self):
        """ONE read-back -> dict of numpy arrays, the records still in the ring oldest first: ``step`` [n], ``kind`` [n],
        ``grad_norm`` [n], ``grad_sq`` / ``weight_sq`` / ``update_sq`` float32 [n, P], ``nonfinite`` int32 [n, P]; ``names`` (list of
        P) and ``n_recorded``, the records ever written (it can exceed ``capacity``)"""
        self._require_attached("arrays()")
        out = decode_health(self._buf.cpu().numpy(), self.n_params, self._capacity)
        out["names"] = list(self.names)
        return out

    def blame(self):
        """the newest SKIPPED record still in the ring -> ``[(name, nonfinite_count), ...]`` of the parameters whose gradient holds
        NaN or +-Inf, in flat-buffer order; ``[]`` when every gradient was finite (a ``found_inf``-only skip); ``None`` when the ring
        holds no skipped record"""
        a = self.arrays()
        skipped = [i for i, k in enumerate(a["kind"]) if k != 0]
        if not skipped:
            return None
        row = a["nonfinite"][skipped[-1]]
        return [(name, int(c)) for name, c in zip(a["names"], row) if c != 0]

    def ratios(self, record=-1):
        """``{name: sqrt(update_sq / weight_sq)}`` -- the update-to-weight ratio of every parameter -- of a real-update record
        (an index into ``arrays()``, default the newest record)"""
        import numpy as np
        a = self.arrays()
        if len(a["kind"]) == 0:
            raise IndexError("HealthLog.ratios: the ring holds no record")
        if a["kind"][record] != 0:
            raise ValueError(f"HealthLog.ratios: record {record} is a skipped step (kind {int(a['kind'][record])}): it carries no weight "
                             "or update norms")
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.sqrt(a["update_sq"][record].astype(np.float64) / a["weight_sq"][record].astype(np.float64))
        return {name: float(x) for name, x in zip(a["names"], r)}

    def reset(self):
        """zeroes the counters (the next record goes to slot 0); the ring's old rows are unreachable afterwards"""
        self._require_attached("reset()")
        self._buf[:4].zero_()


class DeviceAdamW(torch.optim.Optimizer):
    """FusedClipAdamW's update as a ``torch.optim.Optimizer`` whose every scalar lives in DEVICE memory -- what the reference's
    MOSEI trainer asks of its optimizer (scripts/fusion/train_mosei_fusion_seq_level_decoder.py:367-402, 564-584: AdamW under a
    ``LambdaLR`` warm-up + cosine schedule, ``GradScaler``, clip 5.0, NaN / Inf batches skipped), and what lets the update be
    recorded into the hipGraph of the step (``DataParallelStep.capture(..., optimizer=opt)``).

    * ``param_groups[0]`` is an ordinary torch group (``lr`` is a host float a scheduler mutates); ``step()`` uploads the 8-word
      ``hyper`` block when its host image changed (a tiny host -> device copy, nothing is read back) and enqueues three launches:
      sum of squares, finalize (norm, skip decision, clip coefficient, bias corrections, the step count: all written by the
      device), update.
    * ``param_groups=[{"params": [...], "weight_decay": 0.0}, {"params": [...], "lr": 3e-5}]`` gives up to 16 torch groups with
      their own ``lr``, ``betas``, ``eps`` and ``weight_decay`` (missing keys take the constructor's values;
      ``optim.decay_groups`` builds the usual no-decay split).  The groups must partition ``buckets.params``.  The step stays
      three launches: hyper is one [G, 8] block, the finalize writes every group's bias corrections, and ONE update kernel walks
      the flat buffer with a segment table (``optim.group_segments``) that tells it which group owns which elements.  The clip is
      global -- one norm over all groups, as ``clip_grad_norm_(model.parameters())`` -- and so are the skip decision, the step
      count and ``skipped``; a group that names another ``max_norm`` is refused.  ``LambdaLR(opt, [f0, f1])`` drives the groups.
      Without ``param_groups`` there is one group and the three single-group launches run, bit for bit as before.
    * ``clip="global"`` (default) is that one clip.  ``clip="group"`` makes every param group a CLIP UNIT, clipped by its own norm
      against its own ``max_norm`` (group key ``"max_norm"``; a missing key takes the constructor's, ``<= 0`` or ``None`` leaves the
      group unclipped): ``for g in groups: clip_grad_norm_(g["params"], g["max_norm"])``.  ``clip="parameter"`` makes every
      parameter tensor a unit, clipped against its group's ``max_norm``: ``clip_grad_norm_([p], g["max_norm"])`` per parameter.
      Per unit ``norm_u = sqrt(sum g^2) / grad_scale`` and ``coef_u = (max_norm > 0 ? min(1, max_norm / (norm_u + 1e-6)) : 1) /
      grad_scale``.  The step stays three launches (``hriemo_sumsq_units``, ``hriemo_optim_finalize_units``,
      ``hriemo_adamw_flat_units``; tables from ``optim.clip_units``), eagerly and inside every captured step, with averaging, a
      health log and ``GradScaler``, with or without ``param_groups``.  What stays global: the skip decision (any non-finite norm,
      or ``found_inf``), the step count, ``skipped``, the hold of accumulation micro-steps and ``grad_norm`` -- the norm over
      everything, formed as the fixed-order sum of the unit sums.  Word 2 of the state block (``coef``) holds the SMALLEST unit
      coefficient in these modes.  ``clip_state[U][2]`` = ``norm_u, coef_u`` lives on the device: a real update writes both, a
      skipped step the norms only (the non-finite unit shows without a health log), a held micro-step nothing;
      ``opt.clip_arrays()`` reads it back once.  ``state_dict()`` gains a top-level ``"clip"`` key in the unit modes (a dict of
      another mode is refused by name; a dict without the key -- ``torch.optim.AdamW``'s -- loads as ever).
    * A step whose gradient norm is not finite, or in which ``GradScaler`` found an inf, is SKIPPED on the device: parameters,
      moments and the step count stay bit-identical, ``skipped`` counts it.  ``max_norm=None`` disables the clip, not the norm.
    * ``GradScaler.step(opt)`` hands ``grad_scale`` / ``found_inf`` over as device tensors (``_step_supports_amp_scaling``):
      without ``unscale_`` the unscale is fused into the clip coefficient.
    * ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.AdamW``'s format in both directions, multi-group included
      (parameter ids follow group order).  What is compared on loading is what torch compares -- the number of groups and each
      group's parameter count -- plus the moment shapes where the dict carries state: a dict with other counts is refused, one
      whose groups hold the same counts with members swapped between them is not detected.
    * ``grad_norm`` (pre-clip, unscaled), ``device_step`` and ``skipped`` are 0-dim device tensors (views: read them when wanted).
    * ``averaging="ema"`` or ``"swa"`` keeps ``torch.optim.swa_utils.AveragedModel``'s running average of the parameters in one
      more flat fp32 buffer, ``opt.avg`` (laid out like ``flat_p``, a bit copy of the parameters at construction), updated INSIDE the
      update kernel: the step stays three launches and nothing is added behind a graph replay.  With ``t`` the device step count of
      a real update (neither skipped nor held by an accumulation micro-step), the update averages iff ``t > avg_start`` and
      ``(t - avg_start) % avg_every == 0`` -- the torch loop that calls ``update_parameters`` on exactly those steps: the first one
      copies, a later one is ``avg += w * (p - avg)`` with ``w = 1 - avg_decay`` (``"ema"``, ``get_ema_multi_avg_fn(decay)``) or
      ``1 / (n_averaged + 1)`` (``"swa"``, the default ``AveragedModel``).  A skipped or held step moves nothing of the average.
      ``avg_decay``, ``avg_start`` and ``avg_every`` are host attributes uploaded with ``hyper``; ``n_averaged`` is a 0-dim device
      view.  ``with opt.averaged_weights():`` exchanges parameters and average in place (one launch in, one out), so the eager
      forward, ``EvalStep`` and everything built on them evaluate the average without a second model; no step, replay or state dict
      is possible inside.  ``averaged_state_dict(model)`` is ``model.state_dict()`` with the averages in.  ``state_dict()`` gains one
      top-level key ``"averaging"`` (torch's ``load_state_dict`` ignores it); loading a dict WITHOUT it -- a torch optimizer's --
      restarts the average: ``n_averaged = 0`` and ``avg`` = the parameters as they are at that moment, so load the model first,
      then the optimizer.
    * ``health=HealthLog(capacity=64, every=1)`` (or ``health=True``) attaches a health log, ``opt.health``: two more launches behind
      the update kernel (``hriemo_health_sweep``, ``hriemo_health_fold``; they only read the buffers of the step) record the
      per-parameter gradient norm, non-finite count, weight norm and update norm of every ``every``-th real update and of EVERY
      skipped step into a ring in device memory -- eagerly and inside every captured step, with no read-back per step.
      ``opt.health.blame()`` names the parameters whose gradient made the device skip an update, ``opt.health.ratios()`` gives the
      update-to-weight ratios.  Without ``health=`` the launches are those of before; ``state_dict()`` never carries the log.

    Like FusedClipAdamW it re-homes every ``p.data`` into one flat fp32 buffer laid out like ``buckets.flat``: construct it BEFORE
    ``DataParallelStep.capture()``."""

    _step_supports_amp_scaling = True          # GradScaler.step: set opt.grad_scale / opt.found_inf and call step() directly

    def __init__(self, buckets, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=5.0, *, clip="global",
                 param_groups=None, averaging=None, avg_decay=0.999, avg_start=0, avg_every=1, health=None):
        flat_g = buckets.flat
        if clip not in CLIP_MODES:
            raise ValueError(f"DeviceAdamW: clip={clip!r}; the modes are 'global', 'group' and 'parameter'")
        if clip != "global" and param_groups is None:
            param_groups = [{"params": list(buckets.params)}]      # one group: its units share the constructor's max_norm
        self._check_averaging(averaging, avg_decay, avg_start, avg_every)
        if health is True:
            health = HealthLog()
        if health is not None:
            if not isinstance(health, HealthLog):
                raise ValueError(f"DeviceAdamW: health={health!r}; pass a HealthLog, True (HealthLog()) or None")
            health._check_attach(buckets)
        if param_groups is None:
            _require_gpu(flat_g)
        self._check_scalars(lr, betas, eps, weight_decay, "")
        # every refusal comes before the first allocation and before any p.data moves
        groups, seg, seg_group, units = None, None, None, None
        if param_groups is not None:
            groups = _materialise(param_groups)          # generators are read here, once; everything below sees lists
            if clip == "global":
                seg, seg_group = group_segments(buckets, groups)
            else:
                units = clip_units(buckets, groups, clip)
                seg, seg_group = units["seg"], units["seg_group"]
            if len(seg_group) > MAX_SEGMENTS:
                raise ValueError(f"DeviceAdamW: the groups cut the flat buffer into {len(seg_group)} segments; the grouped update "
                                 f"kernel takes at most {MAX_SEGMENTS} (group neighbouring parameters together)")
            for gi, g in enumerate(groups):
                if clip == "global" and "max_norm" in g and g["max_norm"] != max_norm:
                    raise ValueError(f"DeviceAdamW: param_groups[{gi}] names max_norm={g['max_norm']!r}, the optimizer {max_norm!r}: "
                                     "the clip is global (one norm over all groups); clip='group' or clip='parameter' gives every "
                                     "group its own max_norm")
                mn = g.get("max_norm")
                if clip != "global" and mn is not None and (isinstance(mn, bool) or not isinstance(mn, (int, float)) or mn != mn):
                    raise ValueError(f"DeviceAdamW: param_groups[{gi}] names max_norm={mn!r}; a number (<= 0 or None: no clipping)")
                self._check_scalars(g.get("lr", lr), g.get("betas", betas), g.get("eps", eps), g.get("weight_decay", weight_decay),
                                    f" (param_groups[{gi}])")
                if "betas" in g:
                    g["betas"] = tuple(g["betas"])
            _require_gpu(flat_g)
        self.buckets = buckets
        self._grouped = groups is not None          # the grouped launches run, whatever the number of groups
        G = len(groups) if self._grouped else 1
        dev = flat_g.device
        self.flat_p = torch.zeros_like(flat_g)
        self.m = torch.zeros_like(flat_g)
        self.v = torch.zeros_like(flat_g)
        self.nblocks = 1024
        self.clip = clip
        # the unit modes keep one partial per chunk of their own table instead of one per block of the fixed grid
        self._partial = torch.zeros(self.nblocks if units is None else len(units["chunks"]), dtype=torch.float32, device=dev)
        # G rows of 8 words each, kept flat: row 0 of _state is the single-group state block word for word
        self.averaging, self.avg_decay, self.avg_start, self.avg_every = averaging, avg_decay, avg_start, avg_every
        self._swapped = False                       # inside averaged_weights(): flat_p holds the average, avg the parameters
        if averaging is None:
            self._hyper = torch.zeros(G * 8, dtype=torch.float32, device=dev)
        else:
            # avg_hyper[4] rides behind hyper[G][8] in ONE block: one pinned, stream-ordered copy uploads both
            self._hyper_block = torch.zeros(G * 8 + 4, dtype=torch.float32, device=dev)
            self._hyper, self._avg_hyper = self._hyper_block[:G * 8], self._hyper_block[G * 8:]
            # device-written: n_averaged, w, flag, stamp (csrc/optim.hip)
            self._avg_state = torch.zeros(4, dtype=torch.float32, device=dev)
            self.n_averaged = self._avg_state[0]
        self._state = torch.zeros(G * 8, dtype=torch.float32, device=dev)
        self._hyper_host = None                     # the image last uploaded
        if self._grouped:
            self._seg = torch.tensor(seg, dtype=torch.int64, device=dev)
            self._seg_group = torch.tensor(seg_group, dtype=torch.int32, device=dev)
        if units is not None:
            # uploaded here, once; clip_state[U][2] = norm_u, coef_u is written by the finalize launch alone
            self._seg_unit = torch.tensor(units["seg_unit"], dtype=torch.int32, device=dev)
            self._unit_group = torch.tensor(units["unit_group"], dtype=torch.int32, device=dev)
            self._unit_chunks = torch.tensor(units["unit_chunks"], dtype=torch.int32, device=dev)
            self._chunks = torch.tensor(units["chunks"], dtype=torch.int64, device=dev)
            self._unit_group_host = list(units["unit_group"])
            self._clip_state = torch.zeros(2 * len(units["unit_group"]), dtype=torch.float32, device=dev)
            self._clip_params = sorted(buckets.params, key=lambda q: buckets._offsets[id(q)])
            self._clip_names = None
        # the group's keys are torch.optim.AdamW's (a state dict travels both ways) plus max_norm
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True, max_norm=max_norm)
        self._constructing = True
        try:
            super().__init__(groups if self._grouped else list(buckets.params), defaults)
        finally:
            self._constructing = False
        with torch.no_grad():
            for group in self.param_groups:         # group order: the state's keys ascend like torch.optim.AdamW's
                for p in group["params"]:
                    off, n = buckets._offsets[id(p)], p.numel()
                    view = self.flat_p[off:off + n].view_as(p)
                    view.copy_(p.data)
                    p.data = view                   # same values, storage now inside the flat buffer
                    self.state[p] = {"step": self._state[0], "exp_avg": self.m[off:off + n].view_as(p),
                                     "exp_avg_sq": self.v[off:off + n].view_as(p)}
        self.grad_norm, self.device_step, self.skipped = self._state[6], self._state[0], self._state[7]
        if averaging is not None:
            self.avg = self.flat_p.clone()          # the bits of the parameters, zeros in the padding
        self.health = health
        if health is not None:
            health._attach(self, {id(p): gi for gi, group in enumerate(self.param_groups) for p in group["params"]})

    @staticmethod
    def _check_scalars(lr, betas, eps, weight_decay, where):
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f"DeviceAdamW: lr, eps, weight_decay >= 0 and betas in [0, 1) are required{where}")

    @staticmethod
    def _check_averaging(averaging, avg_decay, avg_start, avg_every):
        """the constructor's refusals (before any allocation) and _upload_hyper's, for attributes changed afterwards"""
        if averaging is None:
            if (avg_decay, avg_start, avg_every) != (0.999, 0, 1):
                raise ValueError("DeviceAdamW: avg_decay / avg_start / avg_every are given without averaging= ('ema' or 'swa'): "
                                 "nothing would be averaged")
            return
        if averaging not in AVERAGING_MODES:
            raise ValueError(f"DeviceAdamW: averaging={averaging!r}; the modes are None, 'ema' and 'swa'")
        if not (isinstance(avg_decay, (int, float)) and 0 <= avg_decay < 1):
            raise ValueError(f"DeviceAdamW: avg_decay={avg_decay!r} must lie in [0, 1)")
        for name, val, low in (("avg_start", avg_start, 0), ("avg_every", avg_every, 1)):
            # whole numbers the device holds in fp32 next to the fp32 step count
            if isinstance(val, bool) or not isinstance(val, int) or not low <= val < 2 ** 24:
                raise ValueError(f"DeviceAdamW: {name}={val!r} must be an integer >= {low} (and below 2**24)")

    def _refuse_while_averaged(self, what):
        if self._swapped:
            raise RuntimeError(f"DeviceAdamW: {what} inside `with opt.averaged_weights():` -- the parameter buffer holds the AVERAGE "
                               "there; leave the block first")

    def add_param_group(self, param_group):
        if self.param_groups and not getattr(self, "_constructing", False):
            raise RuntimeError("DeviceAdamW updates ONE flat buffer laid out like its GradBuckets: its param groups are fixed at "
                               "construction (DeviceAdamW(buckets, param_groups=[...])) and partition the buckets' parameters")
        super().add_param_group(param_group)

    # -- the step ---------------------------------------------------------------------------------
    def _upload_hyper(self):
        """hyper[] follows the param groups (a scheduler's lr included): one host -> device copy of the [G, 8] block (32 bytes per
        group) when any group's image changed.  With averaging the 4 words of avg_hyper (mode, decay, start, every: the host
        attributes avg_decay, avg_start, avg_every as they are now) ride behind it in the same block and the same copy.  Every step
        and every replay that carries an update passes through here: inside ``averaged_weights()`` it raises before anything is
        enqueued."""
        self._refuse_while_averaged("step() / a replay that carries the update")
        img = []
        for g in self.param_groups:
            if g["amsgrad"] or g["maximize"]:
                raise RuntimeError("DeviceAdamW: amsgrad / maximize are not built; there is no fallback to torch.optim.AdamW")
            mn = g["max_norm"]
            if self.clip == "global" and mn != self.param_groups[0]["max_norm"]:
                raise RuntimeError("DeviceAdamW: the param groups carry different max_norm values; the clip is global")
            img += [float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                    float(mn) if mn else 0.0, 0.0, 0.0]
        block = self._hyper
        if self.averaging is not None:
            self._check_averaging(self.averaging, self.avg_decay, self.avg_start, self.avg_every)
            img += [AVERAGING_MODES[self.averaging], float(self.avg_decay), float(self.avg_start), float(self.avg_every)]
            block = self._hyper_block
        img = tuple(img)
        if img != self._hyper_host:
            # pinned staging + an asynchronous copy in stream order: the host neither waits for the step in flight nor can a
            # later image overtake this one (torch's host allocator keeps the block until the copy has run)
            block.copy_(torch.tensor(img, dtype=torch.float32).pin_memory(), non_blocking=True)
            self._hyper_host = img

    def _enqueue(self, grad_scale=None, found_inf=None, ctl=None):
        """the step on the current stream (eagerly, or while a step is being captured): the three launches of _enqueue_update and,
        with a health log attached, its two launches behind them -- in all four forms (plain, ctl, groups, averaging)"""
        self._enqueue_update(grad_scale, found_inf, ctl)
        if self.health is not None:
            self.health._enqueue(self, grad_scale, ctl)

    def _enqueue_update(self, grad_scale, found_inf, ctl):
        """the three launches on the current stream (eagerly, or while a step is being captured).  ctl: the int32 step-control block
        of a step captured with gradient accumulation (dp.capture_packed(grad_accum=k)): the finalize launch then holds the update
        on every micro-step whose ctl.last is 0 -- parameters, moments, step count, skipped and grad_norm stay as they are.
        Built with param_groups: the finalize for G groups and the one grouped update kernel take the places of the single-group
        launches.  Built with averaging: the averaging finalize (one entry for plain, ctl and groups) and the averaging form of the
        update kernel -- still three launches."""
        self._refuse_while_averaged("an update")
        g = self.buckets.flat
        n = g.numel()
        st = _stream()
        if self.clip != "global":
            # the unit modes: per-chunk sums of squares, ONE finalize for plain / ctl / averaging, the update with per-unit coef
            G, S, U, C = len(self.param_groups), self._seg_group.numel(), self._unit_group.numel(), self._partial.numel()
            avg = self.averaging is not None
            _lib.call("hriemo_sumsq_units", _p(g), n, _p(self._chunks), C, _p(self._partial), st)
            _lib.call("hriemo_optim_finalize_units", _p(self._partial), C, _p(self._unit_chunks), _p(self._unit_group), U, _p(self._hyper), G,
                      _p(grad_scale), _p(found_inf), _p(self._state), _p(ctl), _p(self._clip_state),
                      _p(self._avg_hyper) if avg else None, _p(self._avg_state) if avg else None, st)
            if avg:
                _lib.call("hriemo_adamw_flat_units_avg", _p(self.flat_p), _p(g), _p(self.m), _p(self.v), n, _p(self._seg), _p(self._seg_group),
                          _p(self._seg_unit), S, _p(self._hyper), _p(self._state), G, _p(self._clip_state), U, _p(self.avg),
                          _p(self._avg_state), st)
            else:
                _lib.call("hriemo_adamw_flat_units", _p(self.flat_p), _p(g), _p(self.m), _p(self.v), n, _p(self._seg), _p(self._seg_group),
                          _p(self._seg_unit), S, _p(self._hyper), _p(self._state), G, _p(self._clip_state), U, st)
            return
        _lib.call("hriemo_sumsq_f32", _p(g), n, _p(self._partial), self.nblocks, st)
        if self.averaging is not None:
            G = len(self.param_groups)
            _lib.call("hriemo_optim_finalize_avg", _p(self._partial), self.nblocks, _p(self._hyper), G, _p(grad_scale), _p(found_inf),
                      _p(self._state), _p(ctl), _p(self._avg_hyper), _p(self._avg_state), st)
            if self._grouped:
                _lib.call("hriemo_adamw_flat_groups_avg", _p(self.flat_p), _p(g), _p(self.m), _p(self.v), n, _p(self._seg),
                          _p(self._seg_group), self._seg_group.numel(), _p(self._hyper), _p(self._state), G, _p(self.avg),
                          _p(self._avg_state), st)
            else:
                _lib.call("hriemo_adamw_flat_dev_avg", _p(self.flat_p), _p(g), _p(self.m), _p(self.v), n, _p(self._hyper), _p(self._state),
                          _p(self.avg), _p(self._avg_state), st)
            return
        if self._grouped:
            G = len(self.param_groups)
            _lib.call("hriemo_optim_finalize_groups", _p(self._partial), self.nblocks, _p(self._hyper), G, _p(grad_scale), _p(found_inf),
                      _p(self._state), _p(ctl), st)
            _lib.call("hriemo_adamw_flat_groups", _p(self.flat_p), _p(g), _p(self.m), _p(self.v), n, _p(self._seg), _p(self._seg_group),
                      self._seg_group.numel(), _p(self._hyper), _p(self._state), G, st)
            return
        if ctl is None:
            _lib.call("hriemo_optim_finalize", _p(self._partial), self.nblocks, _p(self._hyper), _p(grad_scale), _p(found_inf),
                      _p(self._state), st)
        else:
            _lib.call("hriemo_optim_finalize_ctl", _p(self._partial), self.nblocks, _p(self._hyper), _p(grad_scale), _p(found_inf),
                      _p(self._state), _p(ctl), st)
        _lib.call("hriemo_adamw_flat_dev", _p(self.flat_p), _p(g), _p(self.m), _p(self.v), n, _p(self._hyper), _p(self._state), st)

    def _amp_word(self, name):
        t = getattr(self, name, None)
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
            raise RuntimeError(f"DeviceAdamW: {name} must be one fp32 value on the GPU (torch.amp.GradScaler's), got {t!r}")
        return t

    @torch.no_grad()
    def step(self, closure=None):
        """One update from the gradients currently in the flat buffer (skipped on the device if they are not finite)."""
        if closure is not None:
            raise RuntimeError("DeviceAdamW.step() takes no closure: the gradients are read from the flat buffer")
        self._upload_hyper()
        self._enqueue(self._amp_word("grad_scale"), self._amp_word("found_inf"))
        # the update went through raw pointers: neither p._version nor p.data_ptr() moved, so tell the bf16 weight shadows
        _ops.bump_weights_epoch()

    def zero_grad(self, set_to_none=True):
        """zeroes the flat gradient buffer; the gradients stay views into it whatever set_to_none says (the kernels and the
        optimizer address the flat buffer, a detached .grad would silently drop out of both)"""
        self.buckets.zero_grad()

    # -- the clip units ---------------------------------------------------------------------------
    def _require_units(self, what):
        if self.clip == "global":
            raise RuntimeError(f"DeviceAdamW.{what}: built with clip='global', there are no clip units (grad_norm is the one norm)")

    def name_parameters(self, named_parameters):
        """names for ``clip_arrays()["unit"]`` in parameter mode, from ``model.named_parameters()``: parameters the optimizer does
        not own are ignored, a parameter of the optimizer that gets no name raises (nothing is changed then)"""
        self._require_units("name_parameters()")
        given = {id(p): name for name, p in named_parameters}
        for i, p in enumerate(self._clip_params):
            if id(p) not in given:
                raise ValueError(f"DeviceAdamW.name_parameters: parameter {i} of the optimizer ({_describe(p)}) has no name")
        self._clip_names = [given[id(p)] for p in self._clip_params]

    def clip_arrays(self):
        """ONE read-back of ``clip_state`` -> ``{"mode", "unit", "norm", "coef", "max_norm"}``: per clip unit the pre-clip, unscaled
        gradient norm and the coefficient (``1 / grad_scale`` folded in) of the last real update -- after a skipped step ``norm`` is
        that step's and ``coef`` still the last real update's -- and the ``max_norm`` of the unit's group as the host holds it.
        ``unit``: the group indices in group mode; in parameter mode the names attached by ``name_parameters``, else the parameters'
        indices in flat-buffer order."""
        self._require_units("clip_arrays()")
        img = self._clip_state.cpu().numpy().reshape(-1, 2)
        if self.clip == "parameter" and self._clip_names is not None:
            unit = list(self._clip_names)
        else:
            unit = list(range(img.shape[0]))
        max_norm = [self.param_groups[gi]["max_norm"] for gi in self._unit_group_host]
        return {"mode": self.clip, "unit": unit, "norm": img[:, 0].copy(), "coef": img[:, 1].copy(), "max_norm": max_norm}

    # -- the average ------------------------------------------------------------------------------
    def _require_averaging(self, what):
        if self.averaging is None:
            raise RuntimeError(f"DeviceAdamW.{what}: built without averaging= ('ema' or 'swa'), there is no average")

    def _swap_avg(self):
        _lib.call("hriemo_swap_fp32", _p(self.flat_p), _p(self.avg), self.flat_p.numel(), _stream())
        # through raw pointers, like the update: tell the bf16 weight shadows and EvalStep's stationary weight forms
        _ops.bump_weights_epoch()

    @contextlib.contextmanager
    def averaged_weights(self):
        """``with opt.averaged_weights():`` -- the model's parameters ARE the average inside the block: ``flat_p`` and ``avg`` are
        exchanged in place by one launch (hriemo_swap_fp32, every bit crosses) and the weights epoch moves, so the eager forward,
        ``EvalStep`` (default and ``stationary=True``), ``evaluate_packed`` / ``evaluate_store`` and the logs built on them see the
        average without a second module.  The way out -- on an exception too -- exchanges them back: training continues from
        bit-identical parameters.  Inside the block ``step()``, a captured replay that carries the update, ``state_dict()``,
        ``load_state_dict()`` and a nested ``averaged_weights()`` raise."""
        self._require_averaging("averaged_weights()")
        self._refuse_while_averaged("a nested averaged_weights()")
        self._swap_avg()
        self._swapped = True
        try:
            yield self
        finally:
            self._swapped = False
            self._swap_avg()

    @torch.no_grad()
    def averaged_state_dict(self, model):
        """``model.state_dict()`` with a clone of the average in place of every parameter the buckets own (the models have no
        buffers, so there is no counterpart of ``update_bn``): the reference's checkpoint format, loadable by the reference model"""
        self._require_averaging("averaged_state_dict()")
        self._refuse_while_averaged("averaged_state_dict()")
        sd = model.state_dict()
        for name, p in model.named_parameters():
            off = self.buckets._offsets.get(id(p))
            if off is not None and name in sd:
                sd[name] = self.avg[off:off + p.numel()].view_as(p).clone()
        return sd

    # -- checkpoints ------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.AdamW's format.  The moments are the live views (as torch hands out its live state); every parameter gets
        its OWN copy of the step count, as torch keeps one per parameter: an optimizer that loads this and increments each entry
        must not find them all aliasing one word.  With averaging ONE more top-level key, ``"averaging"``: mode, decay, start,
        every, n_averaged (a 0-dim copy) and ``"avg"``, the per-parameter averages under the keys of ``"state"`` (live views, like
        the moments).  ``torch.optim.AdamW.load_state_dict`` ignores the key."""
        self._refuse_while_averaged("state_dict()")
        sd = super().state_dict()
        steps = self._state[0].expand(len(sd["state"])).clone().unbind(0)
        sd["state"] = {k: {**ent, "step": s} for (k, ent), s in zip(sd["state"].items(), steps)}
        if self.averaging is not None:
            keys = [k for g in sd["param_groups"] for k in g["params"]]
            params = [p for g in self.param_groups for p in g["params"]]
            sd["averaging"] = {"mode": self.averaging, "decay": self.avg_decay, "start": self.avg_start, "every": self.avg_every,
                               "n_averaged": self._avg_state[0].clone(), "avg": {k: self._avg_view(p) for k, p in zip(keys, params)}}
        if self.clip != "global":
            sd["clip"] = {"mode": self.clip}        # the groups carry their max_norm; clip_state is a diagnostic and stays out
        return sd

    def _avg_view(self, p):
        off = self.buckets._offsets[id(p)]
        return self.avg[off:off + p.numel()].view_as(p)

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """takes a state dict of this class or of torch.optim.AdamW over the same parameters: values are copied INTO the flat
        buffers (the views stay), `step` comes from the per-parameter entries (all equal, or this raises), lr and the other
        settings from the group.  The ``"averaging"`` block: a dict that carries one restores the average, ``n_averaged`` and the
        host attributes decay / start / every (another mode, other keys or other shapes are refused; so is any such block when this
        optimizer was built without averaging).  A dict WITHOUT one -- a torch optimizer's -- RESTARTS the average:
        ``n_averaged = 0`` and ``avg`` becomes a copy of the parameters as they are now.  So load the model first, then the
        optimizer.  The ``"clip"`` key: a dict that carries one must name this optimizer's ``clip`` mode (another mode is refused by
        name); a dict without one loads in every mode, each group keeping the ``max_norm`` the dict gives it, or its own."""
        self._refuse_while_averaged("load_state_dict()")
        groups, state = state_dict["param_groups"], state_dict["state"]
        mine_groups = self.param_groups
        n_params = len(self.buckets.params)
        if len(groups) != len(mine_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, mine_groups)):
            raise ValueError("DeviceAdamW.load_state_dict: a different grouping: the state dict has %d param group(s) over %s "
                             "parameters, this optimizer %d over %s"
                             % (len(groups), [len(a["params"]) for a in groups], len(mine_groups), [len(b["params"]) for b in mine_groups]))
        if any(src.get("amsgrad") or src.get("maximize") for src in groups):
            raise ValueError("DeviceAdamW.load_state_dict: amsgrad / maximize states cannot be continued here")
        cl = state_dict.get("clip")
        if cl is not None and cl.get("mode") != self.clip:
            raise ValueError(f"DeviceAdamW.load_state_dict: the state dict was written with clip={cl.get('mode')!r}, this optimizer was "
                             f"built with clip={self.clip!r}")
        if self.clip == "global" and any("max_norm" in src and src["max_norm"] != groups[0].get("max_norm") for src in groups):
            raise ValueError("DeviceAdamW.load_state_dict: the groups carry different max_norm values; the clip is global")
        if len(state) not in (0, n_params):
            raise ValueError("DeviceAdamW.load_state_dict: state for %d of %d parameters" % (len(state), n_params))
        pairs = [(key, p) for src, dst in zip(groups, mine_groups) for key, p in zip(src["params"], dst["params"])]
        steps = set()
        for key, p in pairs:
            ent = state.get(key)
            if ent is None:
                continue
            if tuple(ent["exp_avg"].shape) != tuple(p.shape) or tuple(ent["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError("DeviceAdamW.load_state_dict: moment shapes do not match the parameters (a different grouping or "
                                 "another model)")
            steps.add(float(ent["step"]))
        if len(steps) > 1:
            raise ValueError(f"DeviceAdamW.load_state_dict: the parameters carry different step counts {sorted(steps)}; "
                             "one flat update has one step count")
        av = state_dict.get("averaging")
        if av is not None:
            if av.get("mode") != self.averaging:
                raise ValueError(f"DeviceAdamW.load_state_dict: the state dict's average is {av.get('mode')!r}, this optimizer was built "
                                 f"with averaging={self.averaging!r}")
            self._check_averaging(av["mode"], av["decay"], av["start"], av["every"])
            if set(av["avg"]) != {key for key, _ in pairs} or any(tuple(av["avg"][key].shape) != tuple(p.shape) for key, p in pairs):
                raise ValueError("DeviceAdamW.load_state_dict: the averages' shapes do not match the parameters (a different grouping "
                                 "or another model)")
        # nothing has been written up to here
        for key, p in pairs:
            ent = state.get(key)
            mine = self.state[p]
            if ent is None:
                mine["exp_avg"].zero_(); mine["exp_avg_sq"].zero_()
            else:
                if ent["exp_avg"].data_ptr() != mine["exp_avg"].data_ptr():
                    mine["exp_avg"].copy_(ent["exp_avg"])
                if ent["exp_avg_sq"].data_ptr() != mine["exp_avg_sq"].data_ptr():
                    mine["exp_avg_sq"].copy_(ent["exp_avg_sq"])
        self._state[0].fill_(steps.pop() if steps else 0.0)
        for src, group in zip(groups, mine_groups):
            for k, val in src.items():
                if k != "params":
                    group[k] = val
            group.setdefault("max_norm", self.defaults["max_norm"])    # a torch dict has none: the group keeps its own
        self._hyper_host = None
        if self.averaging is not None:
            if av is None:
                self.avg.copy_(self.flat_p)                            # restart: the parameters as they are now
                self._avg_state.zero_()
            else:
                for key, p in pairs:
                    mine = self._avg_view(p)
                    if av["avg"][key].data_ptr() != mine.data_ptr():
                        mine.copy_(av["avg"][key])
                self.avg_decay, self.avg_start, self.avg_every = av["decay"], av["start"], av["every"]
                n_avg = float(av["n_averaged"])
                self._avg_state.zero_()                                # no flag, no stamp: the next finalize decides anew
                self._avg_state[0].fill_(n_avg)
