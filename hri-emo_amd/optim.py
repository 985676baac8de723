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


class DeviceAdamW(torch.optim.Optimizer):
    """FusedClipAdamW's update as a ``torch.optim.Optimizer`` whose every scalar lives in DEVICE memory -- what the reference's
    MOSEI trainer asks of its optimizer (scripts/fusion/train_mosei_fusion_seq_level_decoder.py:367-402, 564-584: AdamW under a
    ``LambdaLR`` warm-up + cosine schedule, ``GradScaler``, clip 5.0, NaN / Inf batches skipped), and what lets the update be
    recorded into the hipGraph of the step (``DataParallelStep.capture(..., optimizer=opt)``).

    * ``param_groups[0]`` is an ordinary torch group (``lr`` is a host float a scheduler mutates); ``step()`` uploads the 8-word
      ``hyper`` block when its host image changed (a tiny host -> device copy, nothing is read back) and enqueues three launches:
      sum of squares, finalize (norm, skip decision, clip coefficient, bias corrections, the step count: all written by the
      device), update.
    * A step whose gradient norm is not finite, or in which ``GradScaler`` found an inf, is SKIPPED on the device: parameters,
      moments and the step count stay bit-identical, ``skipped`` counts it.  ``max_norm=None`` disables the clip, not the norm.
    * ``GradScaler.step(opt)`` hands ``grad_scale`` / ``found_inf`` over as device tensors (``_step_supports_amp_scaling``):
      without ``unscale_`` the unscale is fused into the clip coefficient.
    * ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.AdamW(model.parameters())``'s format in both directions.
    * ``grad_norm`` (pre-clip, unscaled), ``device_step`` and ``skipped`` are 0-dim device tensors (views: read them when wanted).

    Like FusedClipAdamW it re-homes every ``p.data`` into one flat fp32 buffer laid out like ``buckets.flat``: construct it BEFORE
    ``DataParallelStep.capture()``."""

    _step_supports_amp_scaling = True          # GradScaler.step: set opt.grad_scale / opt.found_inf and call step() directly

    def __init__(self, buckets, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=5.0):
        flat_g = buckets.flat
        _require_gpu(flat_g)
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("DeviceAdamW: lr, eps, weight_decay >= 0 and betas in [0, 1) are required")
        self.buckets = buckets
        dev = flat_g.device
        self.flat_p = torch.zeros_like(flat_g)
        self.m = torch.zeros_like(flat_g)
        self.v = torch.zeros_like(flat_g)
        self.nblocks = 1024
        self._partial = torch.zeros(self.nblocks, dtype=torch.float32, device=dev)
        self._hyper = torch.zeros(8, dtype=torch.float32, device=dev)
        self._state = torch.zeros(8, dtype=torch.float32, device=dev)
        self._hyper_host = None                     # the image last uploaded
        # the group's keys are torch.optim.AdamW's (a state dict travels both ways) plus max_norm
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True, max_norm=max_norm)
        super().__init__(list(buckets.params), defaults)
        with torch.no_grad():
            for p in buckets.params:
                off, n = buckets._offsets[id(p)], p.numel()
                view = self.flat_p[off:off + n].view_as(p)
                view.copy_(p.data)
                p.data = view                       # same values, storage now inside the flat buffer
                self.state[p] = {"step": self._state[0], "exp_avg": self.m[off:off + n].view_as(p),
                                 "exp_avg_sq": self.v[off:off + n].view_as(p)}
        self.grad_norm, self.device_step, self.skipped = self._state[6], self._state[0], self._state[7]

    def add_param_group(self, param_group):
        if self.param_groups:
            raise RuntimeError("DeviceAdamW updates ONE flat buffer laid out like its GradBuckets: it has exactly one param group")
        super().add_param_group(param_group)

    # -- the step ---------------------------------------------------------------------------------
    def _upload_hyper(self):
        """hyper[] follows the param group (a scheduler's lr included): one 32-byte host -> device copy when the image changed"""
        g = self.param_groups[0]
        if g["amsgrad"] or g["maximize"]:
            raise RuntimeError("DeviceAdamW: amsgrad / maximize are not built; there is no fallback to torch.optim.AdamW")
        mn = g["max_norm"]
        img = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
               float(mn) if mn else 0.0, 0.0, 0.0)
        if img != self._hyper_host:
            # pinned staging + an asynchronous copy in stream order: the host neither waits for the step in flight nor can a
            # later image overtake this one (torch's host allocator keeps the block until the copy has run)
            self._hyper.copy_(torch.tensor(img, dtype=torch.float32).pin_memory(), non_blocking=True)
            self._hyper_host = img

    def _enqueue(self, grad_scale=None, found_inf=None, ctl=None):
        """the three launches on the current stream (eagerly, or while a step is being captured).  ctl: the int32 step-control block
        of a step captured with gradient accumulation (dp.capture_packed(grad_accum=k)): the finalize launch then holds the update
        on every micro-step whose ctl.last is 0 -- parameters, moments, step count, skipped and grad_norm stay as they are."""
        g = self.buckets.flat
        n = g.numel()
        st = _stream()
        _lib.call("hriemo_sumsq_f32", _p(g), n, _p(self._partial), self.nblocks, st)
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
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.buckets.params):
            raise ValueError("DeviceAdamW.load_state_dict: expected one param group over %d parameters" % len(self.buckets.params))
        src, state = groups[0], state_dict["state"]
        if src.get("amsgrad") or src.get("maximize"):
            raise ValueError("DeviceAdamW.load_state_dict: amsgrad / maximize states cannot be continued here")
        if len(state) not in (0, len(self.buckets.params)):
            raise ValueError("DeviceAdamW.load_state_dict: state for %d of %d parameters" % (len(state), len(self.buckets.params)))
        steps = set()
        for key, p in zip(src["params"], self.buckets.params):
            ent = state.get(key)
            if ent is None:
                continue
            if tuple(ent["exp_avg"].shape) != tuple(p.shape) or tuple(ent["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError("DeviceAdamW.load_state_dict: moment shapes do not match the parameters")
            steps.add(float(ent["step"]))
        if len(steps) > 1:
            raise ValueError(f"DeviceAdamW.load_state_dict: the parameters carry different step counts {sorted(steps)}; "
                             "one flat update has one step count")
        for key, p in zip(src["params"], self.buckets.params):
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
        group = self.param_groups[0]
        for k, val in src.items():
            if k != "params":
                group[k] = val
        group.setdefault("max_norm", self.defaults["max_norm"])
        self._hyper_host = None
