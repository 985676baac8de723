"""clip_grad_norm_(max_norm) + AdamW for the fusion path as two HIP passes over flat buffers
(scripts/fusion/train_fusion_seq_level_decoder.py:332-334).

The gradients already live in ONE flat fp32 buffer (dp.GradBuckets).  This optimizer gives the parameters and both
Adam moments the same layout -- every ``p.data`` becomes a view into a flat parameter buffer -- so the whole update
is one elementwise kernel and the gradient norm one reduction, with the clip coefficient taken from device memory
(no host synchronisation, safe between hipGraph replays).  Construct it BEFORE ``DataParallelStep.capture()``:
it moves the parameter storage.  Results follow torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (fp32)."""
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
    * A step whose gradient norm is not finite, or in which ``GradScaler`` found an inf, is SKIPPED on the device: parameters,
      moments and the step count stay bit-identical, ``skipped`` counts it.  ``max_norm=None`` disables the clip, not the norm.
    * ``GradScaler.step(opt)`` hands ``grad_scale`` / ``found_inf`` over as device tensors (``_step_supports_amp_scaling``):
      without ``unscale_`` the unscale is fused into the clip coefficient.
    * ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.AdamW``'s format in both directions, multi-group included
      (parameter ids follow group order).  What is compared on loading is what torch compares -- the number of groups and each
      group's parameter count -- plus the moment shapes where the dict carries state: a dict with other counts is refused, one
      whose groups hold the same counts with members swapped between them is not detected.
    * ``grad_norm`` (pre-clip, unscaled), ``device_step`` and ``skipped`` are 0-dim device tensors (views: read them when wanted).

    Like FusedClipAdamW it re-homes every ``p.data`` into one flat fp32 buffer laid out like ``buckets.flat``: construct it BEFORE
    ``DataParallelStep.capture()``."""

    _step_supports_amp_scaling = True          # GradScaler.step: set opt.grad_scale / opt.found_inf and call step() directly

    def __init__(self, buckets, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=5.0, *, param_groups=None):
        flat_g = buckets.flat
        if param_groups is None:
            _require_gpu(flat_g)
        self._check_scalars(lr, betas, eps, weight_decay, "")
        # every refusal comes before the first allocation and before any p.data moves
        groups, seg, seg_group = None, None, None
        if param_groups is not None:
            groups = _materialise(param_groups)          # generators are read here, once; everything below sees lists
            seg, seg_group = group_segments(buckets, groups)
            if len(seg_group) > MAX_SEGMENTS:
                raise ValueError(f"DeviceAdamW: the groups cut the flat buffer into {len(seg_group)} segments; the grouped update "
                                 f"kernel takes at most {MAX_SEGMENTS} (group neighbouring parameters together)")
            for gi, g in enumerate(groups):
                if "max_norm" in g and g["max_norm"] != max_norm:
                    raise ValueError(f"DeviceAdamW: param_groups[{gi}] names max_norm={g['max_norm']!r}, the optimizer {max_norm!r}: "
                                     "the clip is global (one norm over all groups), per-group clipping is not built")
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
        self._partial = torch.zeros(self.nblocks, dtype=torch.float32, device=dev)
        # G rows of 8 words each, kept flat: row 0 of _state is the single-group state block word for word
        self._hyper = torch.zeros(G * 8, dtype=torch.float32, device=dev)
        self._state = torch.zeros(G * 8, dtype=torch.float32, device=dev)
        self._hyper_host = None                     # the image last uploaded
        if self._grouped:
            self._seg = torch.tensor(seg, dtype=torch.int64, device=dev)
            self._seg_group = torch.tensor(seg_group, dtype=torch.int32, device=dev)
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

    @staticmethod
    def _check_scalars(lr, betas, eps, weight_decay, where):
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f"DeviceAdamW: lr, eps, weight_decay >= 0 and betas in [0, 1) are required{where}")

    def add_param_group(self, param_group):
        if self.param_groups and not getattr(self, "_constructing", False):
            raise RuntimeError("DeviceAdamW updates ONE flat buffer laid out like its GradBuckets: its param groups are fixed at "
                               "construction (DeviceAdamW(buckets, param_groups=[...])) and partition the buckets' parameters")
        super().add_param_group(param_group)

    # -- the step ---------------------------------------------------------------------------------
    def _upload_hyper(self):
        """hyper[] follows the param groups (a scheduler's lr included): one host -> device copy of the [G, 8] block (32 bytes per
        group) when any group's image changed"""
        img = []
        for g in self.param_groups:
            if g["amsgrad"] or g["maximize"]:
                raise RuntimeError("DeviceAdamW: amsgrad / maximize are not built; there is no fallback to torch.optim.AdamW")
            mn = g["max_norm"]
            if mn != self.param_groups[0]["max_norm"]:
                raise RuntimeError("DeviceAdamW: the param groups carry different max_norm values; the clip is global")
            img += [float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                    float(mn) if mn else 0.0, 0.0, 0.0]
        img = tuple(img)
        if img != self._hyper_host:
            # pinned staging + an asynchronous copy in stream order: the host neither waits for the step in flight nor can a
            # later image overtake this one (torch's host allocator keeps the block until the copy has run)
            self._hyper.copy_(torch.tensor(img, dtype=torch.float32).pin_memory(), non_blocking=True)
            self._hyper_host = img

    def _enqueue(self, grad_scale=None, found_inf=None, ctl=None):
        """the three launches on the current stream (eagerly, or while a step is being captured).  ctl: the int32 step-control block
        of a step captured with gradient accumulation (dp.capture_packed(grad_accum=k)): the finalize launch then holds the update
        on every micro-step whose ctl.last is 0 -- parameters, moments, step count, skipped and grad_norm stay as they are.
        Built with param_groups: the finalize for G groups and the one grouped update kernel take the places of the single-group
        launches."""
        g = self.buckets.flat
        n = g.numel()
        st = _stream()
        _lib.call("hriemo_sumsq_f32", _p(g), n, _p(self._partial), self.nblocks, st)
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

    # -- checkpoints ------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.AdamW's format.  The moments are the live views (as torch hands out its live state); every parameter gets
        its OWN copy of the step count, as torch keeps one per parameter: an optimizer that loads this and increments each entry
        must not find them all aliasing one word."""
        sd = super().state_dict()
        steps = self._state[0].expand(len(sd["state"])).clone().unbind(0)
        sd["state"] = {k: {**ent, "step": s} for (k, ent), s in zip(sd["state"].items(), steps)}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """takes a state dict of this class or of torch.optim.AdamW over the same parameters: values are copied INTO the flat
        buffers (the views stay), `step` comes from the per-parameter entries (all equal, or this raises), lr and the other
        settings from the group"""
        groups, state = state_dict["param_groups"], state_dict["state"]
        mine_groups = self.param_groups
        n_params = len(self.buckets.params)
        if len(groups) != len(mine_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, mine_groups)):
            raise ValueError("DeviceAdamW.load_state_dict: a different grouping: the state dict has %d param group(s) over %s "
                             "parameters, this optimizer %d over %s"
                             % (len(groups), [len(a["params"]) for a in groups], len(mine_groups), [len(b["params"]) for b in mine_groups]))
        if any(src.get("amsgrad") or src.get("maximize") for src in groups):
            raise ValueError("DeviceAdamW.load_state_dict: amsgrad / maximize states cannot be continued here")
        if any("max_norm" in src and src["max_norm"] != groups[0].get("max_norm") for src in groups):
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
