"""Host-side batch plumbing of the seq-level trainer (scripts/fusion/train_fusion_seq_level_decoder.py:137-232):
the on-disk feature format {"hidden": [L, d], "attention_mask": [L] (1 = valid)} -> padded batch + key-padding
masks (True = PAD), plus what the reference leaves on the table:

* ``trim_padding`` drops the columns that are PAD for EVERY sample of the batch (feature files are usually stored
  padded to a dataset-wide length, so the reference computes -- and this path would otherwise compute -- all of those
  query rows).  Outputs (logits, beta, z) are unchanged: PAD keys are masked, PAD query rows feed nothing.
* ``length_bucketed_batches`` groups utterances of similar length so a batch's padding (= wasted rows in every
  GEMM / LayerNorm / attention of the path) stays small.
"""
import itertools
import math
import weakref

import torch


def load_seq_feat(obj):
    """{"hidden": [L,d], "attention_mask": [L] 1=valid} -> (hidden fp32 [L,d], mask bool [L] True=PAD)   (:137-154)"""
    return obj["hidden"].float(), obj["attention_mask"].long() == 0


def collate_seq_batch(batch, loss_type="multi_label", pad_to=None):
    """list of (h_a[L_a,d], m_a[L_a], h_t[L_t,d], m_t[L_t], label) -> (h_a[B,La,d], mask_a[B,La], h_t[B,Lt,d],
    mask_t[B,Lt], labels); zero padding, padded positions masked True; labels [B] long (single_label) or [B,C]
    float (multi_label)   (:191-232).  pad_to=(La, Lt): pad to these lengths instead of the batch maxima -- every batch then
    has one shape, which is what a captured step wants; in packed (varlen) mode the extra PAD rows cost nothing
    (DataParallelStep.capture)."""
    B = len(batch)
    d = batch[0][0].shape[-1]
    La = max(s[0].shape[0] for s in batch)
    Lt = max(s[2].shape[0] for s in batch)
    if pad_to is not None:
        if pad_to[0] < La or pad_to[1] < Lt:
            raise ValueError(f"collate_seq_batch: pad_to={tuple(pad_to)} is shorter than this batch's longest sequences ({La}, {Lt})")
        La, Lt = int(pad_to[0]), int(pad_to[1])
    h_a, h_t = torch.zeros(B, La, d), torch.zeros(B, Lt, d)
    m_a, m_t = torch.ones(B, La, dtype=torch.bool), torch.ones(B, Lt, dtype=torch.bool)
    for i, (xa, ka, xt, kt, _) in enumerate(batch):
        h_a[i, :xa.shape[0]], m_a[i, :xa.shape[0]] = xa, ka
        h_t[i, :xt.shape[0]], m_t[i, :xt.shape[0]] = xt, kt
    if loss_type == "single_label":
        labels = torch.tensor([s[4] for s in batch], dtype=torch.long)
    else:
        labels = torch.stack([s[4] for s in batch], dim=0)
    return h_a, m_a, h_t, m_t, labels


def collate_seq_packed(batch, loss_type="multi_label"):
    """The samples of collate_seq_batch for a model's forward_packed: -> (rows_a [sum(lengths_a), d], lengths_a [B] int64,
    rows_t [sum(lengths_t), d], lengths_t [B] int64, labels) -- the valid rows (mask False) of every utterance back to back, nothing
    padded on the host and no PAD row on its way to the device.  The padded batch collate_seq_batch builds, gathered at its valid
    rows, is exactly (rows_a, rows_t); pad_to of forward_packed defaults to the lengths collate_seq_batch would pad to when every
    utterance's stored rows are valid."""
    rows_a = torch.cat([xa[~ka] for xa, ka, _, _, _ in batch], dim=0)
    rows_t = torch.cat([xt[~kt] for _, _, xt, kt, _ in batch], dim=0)
    len_a = torch.tensor([int((~ka).sum()) for _, ka, _, _, _ in batch], dtype=torch.int64)
    len_t = torch.tensor([int((~kt).sum()) for _, _, _, kt, _ in batch], dtype=torch.int64)
    if loss_type == "single_label":
        labels = torch.tensor([s[4] for s in batch], dtype=torch.long)
    else:
        labels = torch.stack([s[4] for s in batch], dim=0)
    return rows_a, len_a, rows_t, len_t, labels


def _valid_extent(mask):
    """1 + index of the last position that is valid for at least one sample (0 if everything is PAD)."""
    any_valid = (~mask).any(dim=0)
    idx = torch.nonzero(any_valid)
    return int(idx[-1]) + 1 if idx.numel() else 0


def trim_padding(h_a, mask_a, h_t, mask_t):
    """Cut the trailing columns that are PAD in every sample.  The audio side is never cut below the text side:
    BetaGate fuses over the text length and slices h_a[:, :L_t] (beta_gate_tacfn.py:98-112)."""
    Lt = max(1, _valid_extent(mask_t))
    La = max(1, _valid_extent(mask_a), min(Lt, h_a.shape[1]))
    return h_a[:, :La].contiguous(), mask_a[:, :La].contiguous(), h_t[:, :Lt].contiguous(), mask_t[:, :Lt].contiguous()


def length_bucketed_batches(lengths, batch_size, shuffle=True, generator=None, bucket_mult=50):
    """Index batches in which lengths are similar: shuffle, cut into chunks of bucket_mult*batch_size, sort each chunk
    by length, slice it into batches, shuffle the batches.  Every index appears exactly once."""
    n = len(lengths)
    order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
    chunk = max(batch_size, bucket_mult * batch_size)
    batches = []
    for s in range(0, n, chunk):
        part = sorted(order[s:s + chunk], key=lambda i: lengths[i])
        batches += [part[k:k + batch_size] for k in range(0, len(part), batch_size)]
    if shuffle:
        perm = torch.randperm(len(batches), generator=generator).tolist()
        batches = [batches[i] for i in perm]
    return batches


class StoreAugment:
    """Seeded train-time augmentation of the rows a ``DeviceFeatureStore`` hands to a TRAINER step, applied inside the gather
    (hriemo_gather_rows_aug, csrc/store.hip): no buffer, no upload, nothing inside the captured graphs changes.

    ``time_mask=dict(spans=1..4, max_width=W >= 1, max_frac=0 < f <= 1)`` (one dict for both modalities, or a pair (audio, text)
    whose entries may be None): per utterance `spans` spans of rows become zero, each of a width uniform in [0, min(W, f * L)] at
    a uniform place (SpecAugment's time mask on frames).  ``noise_std=(sigma_a, sigma_t)``: zero-mean noise of that standard
    deviation is added to every kept element (a sum of four 8-bit uniforms: bounded by 3.45 sigma).  ``modality_drop=(p_a, p_t)``:
    with probability p_a an utterance's audio rows are all zero, with p_t its text rows -- never both (one draw decides), so
    p_a + p_t < 1.  Noise first, then the zeros.

    Everything is a function of (seed, draw, modality, the utterance's id in the store, row, column) through the counter hash of
    csrc/common.h: not of the batch an utterance is in, its position there, or the data-parallel shard that holds it
    (tests/augment_reference.py is the host replica).  ``draw`` is a host int that starts at 0: ``step_store`` uses it and adds one
    per accepted call (every micro-step of an accumulation group is a draw of its own); ``fetch`` reads it and never advances it.
    A caller that resumes sets it, e.g. ``aug.draw = epoch * steps_per_epoch + step``.  Data parallel: every rank constructs the same
    object and steps in lockstep -- ``seed`` and ``draw`` MUST agree across ranks; then a sample's augmentation does not depend
    on which rank holds it.  Evaluation is never augmented: EvalStep and train.evaluate_store take no augment."""

    NOISE_VAR = 21845.0              # variance of the sum of four uniform bytes: 4 * (256^2 - 1) / 12

    def __init__(self, seed, time_mask=None, noise_std=None, modality_drop=None):
        seed = int(seed)
        if seed < 0 or seed >= 1 << 64:
            raise ValueError(f"StoreAugment: seed {seed} (an unsigned 64-bit integer)")
        if time_mask is None or isinstance(time_mask, dict):
            time_mask = (time_mask, time_mask)
        if len(time_mask) != 2:
            raise ValueError("StoreAugment: time_mask is one dict(spans=, max_width=, max_frac=) or a pair (audio, text) of them")
        masks = []
        for name, tm in zip(("audio", "text"), time_mask):
            if tm is None:
                masks.append((0, 0, 0.0))
                continue
            if not isinstance(tm, dict) or set(tm) != {"spans", "max_width", "max_frac"}:
                raise ValueError(f"StoreAugment: time_mask ({name}) is dict(spans=, max_width=, max_frac=)")
            spans, width, frac = tm["spans"], tm["max_width"], float(tm["max_frac"])
            if int(spans) != spans or not 1 <= spans <= 4:
                raise ValueError(f"StoreAugment: time_mask ({name}) spans = {spans!r} (1 .. 4)")
            if int(width) != width or not 1 <= width < 1 << 31:
                raise ValueError(f"StoreAugment: time_mask ({name}) max_width = {width!r} (an integer >= 1)")
            if not 0.0 < frac <= 1.0:
                raise ValueError(f"StoreAugment: time_mask ({name}) max_frac = {frac!r} (0 < max_frac <= 1)")
            masks.append((int(spans), int(width), frac))
        sigma = (0.0, 0.0) if noise_std is None else tuple(float(v) for v in noise_std)
        if len(sigma) != 2 or not all(0.0 <= v < float("inf") for v in sigma):
            raise ValueError(f"StoreAugment: noise_std = {noise_std!r} (a pair (audio, text) of finite sigma >= 0)")
        drop = (0.0, 0.0) if modality_drop is None else tuple(float(v) for v in modality_drop)
        if len(drop) != 2 or not all(v >= 0.0 for v in drop) or not drop[0] + drop[1] < 1.0:
            raise ValueError(f"StoreAugment: modality_drop = {modality_drop!r} (a pair p_a, p_t >= 0 with p_a + p_t < 1)")
        if not any(m[0] for m in masks) and not any(sigma) and not any(drop):
            raise ValueError("StoreAugment: no transform is enabled (time_mask, noise_std and modality_drop are all off): "
                             "an augment that does nothing is refused; pass augment=None")
        self.seed, self.draw = seed, 0
        self.time_mask, self.noise_std, self.modality_drop = tuple(masks), sigma, drop

    @staticmethod
    def _thr16(p):
        """round(p * 65536) in [0, 65535], as make_drop (csrc/common.h) counts a dropout rate"""
        return max(0, min(65535, int(p * 65536.0 + 0.5)))

    def config(self):
        """the configuration as plain Python values (what state_dict carries beside seed and draw)"""
        return {"time_mask": [list(m) for m in self.time_mask], "noise_std": list(self.noise_std), "modality_drop": list(self.modality_drop)}

    def state_dict(self):
        return {"seed": self.seed, "draw": self.draw, "config": self.config()}

    def load_state_dict(self, state):
        """seed and draw of a saved run; a dict saved from another configuration is refused (ValueError), nothing is changed then"""
        if state.get("config") != self.config():
            raise ValueError(f"StoreAugment.load_state_dict: the state was saved with another configuration ({state.get('config')!r}; "
                             f"this object has {self.config()!r})")
        seed, draw = int(state["seed"]), int(state["draw"])
        if seed < 0 or seed >= 1 << 64 or draw < 0:
            raise ValueError(f"StoreAugment.load_state_dict: seed {seed}, draw {draw}")
        self.seed, self.draw = seed, draw

    def launch_args(self, which, draw=None):
        """the scalar arguments of hriemo_gather_rows_aug behind max_rows for the audio (which = 0) or the text (1) launch:
        (seed, draw, modality, thr_lo, thr_hi, spans, max_width, frac16, noise_scale); the draw is taken modulo 2^32"""
        draw = self.draw if draw is None else int(draw)
        if draw < 0:
            raise ValueError(f"StoreAugment: draw = {draw} (a counter >= 0)")
        thr_a, thr_t = self._thr16(self.modality_drop[0]), self._thr16(self.modality_drop[1])
        lo, hi = ((0, thr_a), (thr_a, thr_a + thr_t))[which]
        spans, width, frac = self.time_mask[which]
        frac16 = min(65536, int(frac * 65536.0 + 0.5))
        scale = torch.tensor(self.noise_std[which] / math.sqrt(self.NOISE_VAR), dtype=torch.float64).float().item()      # fp32(sigma / sqrt(var))
        return (self.seed, draw & 0xFFFFFFFF, which + 1, lo, hi, spans, min(width, 0xFFFFFFFF), frac16, scale)


class DeviceFeatureStore:
    """One split of a corpus resident on ONE device: every utterance's valid rows back to back, so that a batch is a list of utterance
    ids and nothing but those ids and their lengths crosses to the device per step (the corpora of this model are a few GB; an
    MI355X has 288 GB).  Built from whatever ``Dataset`` the user has (``from_samples``); ``DataParallelStep.capture_store`` /
    ``step_store`` and ``EvalStep.capture_store`` / ``eval_store`` feed a captured step from it (one hriemo_gather_rows launch per
    operand in front of the replay), ``fetch`` is the eager and test entry.

    Device state: ``rows_a`` [N_a, d_a] and ``rows_t`` [N_t, d_t] in the store's dtype (fp32, bf16 or fp16), ``off_a`` / ``off_t``
    int64 [N + 1] (utterance u owns the rows off[u] .. off[u + 1]), ``y`` [N, C] float or [N] int64 (single_label) and ``off_y`` =
    0 .. N (the targets are a store in which every utterance owns one row).  Host state: ``lengths_a`` / ``lengths_t`` and
    ``offsets_a`` / ``offsets_t`` as Python lists -- every bucket key, every plan and every check is computed from these; nothing is
    ever read back from the device.

    On a CPU ``device`` the store works with torch indexing in place of the kernel (host tests, gloo rehearsals), as
    ``DevicePrefetcher`` passes batches through there; the captured front doors themselves need the GPU like every product path.
    Under data parallelism every rank holds the whole store and passes its own slice of the global batch's ids."""

    _DTYPES = (torch.float32, torch.bfloat16, torch.float16)

    def __init__(self, device, dtype=None, max_len=None, sanitize=True, loss_type="multi_label", chunk_bytes=64 << 20):
        if dtype is not None and dtype not in self._DTYPES:
            raise ValueError(f"DeviceFeatureStore: dtype {dtype} (float32, bfloat16 or float16)")
        if max_len is not None and (len(max_len) != 2 or min(int(v) for v in max_len) < 1):
            raise ValueError("DeviceFeatureStore: max_len=(L_a, L_t), both positive")
        self.device, self.dtype, self.sanitize, self.loss_type = torch.device(device), dtype, bool(sanitize), loss_type
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())      # comparable with a module's device
        self.max_len = None if max_len is None else (int(max_len[0]), int(max_len[1]))
        self.chunk_bytes = int(chunk_bytes)
        self.lengths_a, self.lengths_t, self.offsets_a, self.offsets_t = [], [], [0], [0]
        self.rows_a = self.rows_t = self.off_a = self.off_t = self.off_y = self.y = None
        self.widths = None                    # (d_a, d_t), fixed by the first sample
        self.version = 0                     # bumped by every append: a step captured on an earlier version refuses the store
        self._holders = weakref.WeakSet()     # the captured steps that read this store (capture_store .. release_graph)

    @classmethod
    def from_samples(cls, samples, device, dtype=None, max_len=None, sanitize=True, loss_type="multi_label", chunk_bytes=64 << 20):
        """samples yields the reference datasets' items (h_a [L_a, d_a], m_a [L_a], h_t [L_t, d_t], m_t [L_t], y), the form
        collate_seq_packed takes.  Per item, on the host: the rows with mask False are kept (the mask is honoured row by row, PAD rows
        inside the stored length included); sanitize: nan_to_num(nan=0, posinf=0, neginf=0) as _load_feat of the MOSEI trainer;
        max_len=(L_a, L_t): the trainers' crop_center on the kept rows -- rows (L - max_len) // 2 .. + max_len, only when L > max_len;
        then the cast to `dtype` (default: the samples' own).  Rows are uploaded in chunks of about chunk_bytes, so host memory holds one
        chunk beside the samples' source, never the whole split."""
        store = cls(device, dtype, max_len, sanitize, loss_type, chunk_bytes)
        store.append(samples)
        return store

    def __len__(self):
        return len(self.lengths_a)

    @property
    def pad_to(self):
        """(max L_a, max L_t) over the store: the padded lengths a step captured on it needs at least"""
        return (max(self.lengths_a), max(self.lengths_t)) if len(self) else (0, 0)

    @property
    def nbytes(self):
        """bytes of device memory the store holds"""
        return sum(t.numel() * t.element_size() for t in (self.rows_a, self.rows_t, self.off_a, self.off_t, self.off_y, self.y) if t is not None)

    def _item_rows(self, x, mask, limit):
        x = x[~mask.bool()]
        if self.sanitize:
            x = torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
        if limit is not None and x.shape[0] > limit:
            s = (x.shape[0] - limit) // 2
            x = x[s:s + limit]
        return x.to(self.dtype)

    def append(self, samples):
        """more utterances behind the ones held (ids continue).  Allowed only while no captured step reads the store (RuntimeError
        otherwise: the graphs' front door has the store's addresses and sizes; release_graph() first)."""
        if len(self._holders):
            raise RuntimeError("DeviceFeatureStore.append: a captured step reads this store (release_graph() it first)")
        la, lt, ys = [], [], []
        dev_a, dev_t = ([] if self.rows_a is None else [self.rows_a]), ([] if self.rows_t is None else [self.rows_t])
        host_a, host_t, held = [], [], 0

        def flush():
            nonlocal host_a, host_t, held
            if host_a:
                dev_a.append(torch.cat(host_a).to(self.device))
                dev_t.append(torch.cat(host_t).to(self.device))
            host_a, host_t, held = [], [], 0

        for xa, ka, xt, kt, y in samples:
            if self.dtype is None:
                self.dtype = xa.dtype
                if self.dtype not in self._DTYPES:
                    raise ValueError(f"DeviceFeatureStore: samples of dtype {self.dtype} (float32, bfloat16 or float16)")
            ra = self._item_rows(xa, ka, None if self.max_len is None else self.max_len[0])
            rt = self._item_rows(xt, kt, None if self.max_len is None else self.max_len[1])
            if ra.dim() != 2 or rt.dim() != 2:
                raise ValueError("DeviceFeatureStore: a sample's features are [L, d] per modality")
            if self.widths is None:
                self.widths = (ra.shape[1], rt.shape[1])
            if (ra.shape[1], rt.shape[1]) != self.widths:
                raise ValueError(f"DeviceFeatureStore: rows of widths {(ra.shape[1], rt.shape[1])}; the store holds {self.widths}")
            host_a.append(ra)
            host_t.append(rt)
            la.append(ra.shape[0])
            lt.append(rt.shape[0])
            ys.append(y)
            held += ra.numel() * ra.element_size() + rt.numel() * rt.element_size()
            if held >= self.chunk_bytes:
                flush()
        flush()
        if not la:
            return self
        if self.loss_type == "single_label":
            y = torch.tensor([int(v) for v in ys], dtype=torch.long)
        else:
            y = torch.stack(ys, dim=0)
        y = y.to(self.device)
        if self.y is not None and (y.dtype != self.y.dtype or y.shape[1:] != self.y.shape[1:]):
            raise ValueError(f"DeviceFeatureStore: targets of shape {tuple(y.shape[1:])} / {y.dtype}; the store holds {tuple(self.y.shape[1:])} / {self.y.dtype}")
        # one concatenation per append: the device briefly holds the old rows and the new ones twice
        self.rows_a = dev_a[0] if len(dev_a) == 1 else torch.cat(dev_a)
        self.rows_t = dev_t[0] if len(dev_t) == 1 else torch.cat(dev_t)
        self.y = y if self.y is None else torch.cat([self.y, y])
        for lens, offs, new in ((self.lengths_a, self.offsets_a, la), (self.lengths_t, self.offsets_t, lt)):
            for v in new:
                lens.append(v)
                offs.append(offs[-1] + v)
        self.off_a = torch.tensor(self.offsets_a, dtype=torch.int64).to(self.device)
        self.off_t = torch.tensor(self.offsets_t, dtype=torch.int64).to(self.device)
        self.off_y = torch.arange(len(self) + 1, dtype=torch.int64).to(self.device)
        self.version += 1
        return self

    # ---- host arithmetic
    def check_ids(self, ids):
        """-> ids as a list of Python ints; ValueError for an empty list or an id outside [0, len(store)) -- checked here, on the host,
        before anything is enqueued: the gather kernel cannot know how long the store is"""
        ids = [int(v) for v in (ids.tolist() if isinstance(ids, torch.Tensor) else ids)]
        if not ids:
            raise ValueError("DeviceFeatureStore: an empty id list")
        n = len(self)
        bad = [v for v in ids if v < 0 or v >= n]
        if bad:
            raise ValueError(f"DeviceFeatureStore: utterance id {bad[0]} outside [0, {n})")
        return ids

    def plan_words(self, ids, stride):
        """The plan block of a batch, as the host writes it from its own lengths: three plans {ids[n], dst_cu[n + 1]} -- audio rows,
        text rows, targets (one row per utterance) -- `stride` >= 2 n + 1 int32 words apart, zero padded: what hriemo_gather_rows
        reads for each of the three operands.  ids: checked (check_ids)."""
        n = len(ids)
        if stride < 2 * n + 1:
            raise ValueError(f"DeviceFeatureStore.plan_words: {n} ids do not fit a plan of {stride} words")
        words = []
        for lens in ([self.lengths_a[i] for i in ids], [self.lengths_t[i] for i in ids], [1] * n):
            words += ids + list(itertools.accumulate(lens, initial=0)) + [0] * (stride - 2 * n - 1)
        return words

    _DTYPE_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}

    def _check_augment(self, who, augment):
        """the refusals of an augment, before anything is allocated or enqueued"""
        if not isinstance(augment, StoreAugment):
            raise TypeError(f"{who}: augment is a data.StoreAugment (or None)")
        if self.device.type != "cuda":
            raise RuntimeError(f"{who}: augment= on a store that lives on {self.device}: the augmentation is part of the gather kernel "
                               "(hriemo_gather_rows_aug) and has no CPU fallback; the lengths do not change, so the host needs nothing from it")
        if max(self.pad_to) >= 65536:
            raise ValueError(f"{who}: augment= on a store with an utterance of {max(self.pad_to)} rows (the span arithmetic is 16-bit: < 65536)")

    def gather_into(self, plan_dev, stride, n, dst_a, rows_a, dst_t, rows_t, dst_y, augment=None, draw=None):
        """The batch of a plan block on the device (plan_words(ids, stride), n = len(ids)) into three destinations on the current
        stream: rows 0 .. rows_a of dst_a and 0 .. rows_t of dst_t (the batch's rows, zeros behind them), the first n rows of dst_y
        (None: no targets wanted).  One hriemo_gather_rows launch each; no allocation, no synchronisation.  augment (a
        StoreAugment; draw None: its own counter, which is never advanced here): the audio and the text rows go through
        hriemo_gather_rows_aug instead, the targets stay with the plain kernel."""
        from . import _lib
        if augment is not None:
            self._check_augment("DeviceFeatureStore.gather_into", augment)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        base = plan_dev.data_ptr()
        for p, (src, off, dst, rows) in enumerate(((self.rows_a, self.off_a, dst_a, rows_a), (self.rows_t, self.off_t, dst_t, rows_t),
                                                   (self.y, self.off_y, dst_y, n))):
            if dst is None:
                continue
            row_bytes = src[0].numel() * src.element_size()
            if dst.dtype != src.dtype or dst[0].numel() * dst.element_size() != row_bytes or dst.shape[0] < rows or not dst.is_contiguous():
                raise ValueError(f"DeviceFeatureStore.gather_into: destination {tuple(dst.shape)} / {dst.dtype} for {rows} rows of "
                                 f"{tuple(src.shape[1:])} / {src.dtype}")
            if augment is not None and p < 2:
                _lib.call("hriemo_gather_rows_aug", src.data_ptr(), src[0].numel(), self._DTYPE_CODES[src.dtype], off.data_ptr(),
                          base + 4 * p * stride, n, dst.data_ptr(), rows, self.pad_to[p], *augment.launch_args(p, draw), stream)
                continue
            _lib.call("hriemo_gather_rows", src.data_ptr(), row_bytes, off.data_ptr(), base + 4 * p * stride, n, dst.data_ptr(), rows, stream)

    # ---- batches
    def fetch(self, ids, augment=None, draw=None):
        """-> (rows_a, lengths_a, rows_t, lengths_t, y): exactly what collate_seq_packed gives for the samples `ids` (after the
        store's mask / sanitise / crop / cast), as fresh tensors with rows and targets on the store's device.  The two lengths
        tensors stay int64 HOST tensors, as the collate makes them: every consumer (forward_packed, step_packed, eval_packed) wants
        them on the host and refuses device lengths.  On a GPU the rows come through hriemo_gather_rows, on a CPU device through
        torch indexing.  augment (a StoreAugment): the rows as a trainer step with that augment sees them at `draw` (None:
        ``augment.draw``, which fetch never advances); GPU stores only (RuntimeError on a CPU device)."""
        if augment is not None:
            self._check_augment("DeviceFeatureStore.fetch", augment)
        ids = self.check_ids(ids)
        la, lt = [self.lengths_a[i] for i in ids], [self.lengths_t[i] for i in ids]
        len_a, len_t = torch.tensor(la, dtype=torch.int64), torch.tensor(lt, dtype=torch.int64)
        if self.device.type != "cuda":
            rows_a = torch.cat([self.rows_a[self.offsets_a[i]:self.offsets_a[i + 1]] for i in ids], dim=0)
            rows_t = torch.cat([self.rows_t[self.offsets_t[i]:self.offsets_t[i + 1]] for i in ids], dim=0)
            return rows_a, len_a, rows_t, len_t, self.y[torch.tensor(ids, dtype=torch.int64)]
        n, na, nt = len(ids), sum(la), sum(lt)
        rows_a = torch.empty((max(na, 1),) + tuple(self.rows_a.shape[1:]), dtype=self.dtype, device=self.device)
        rows_t = torch.empty((max(nt, 1),) + tuple(self.rows_t.shape[1:]), dtype=self.dtype, device=self.device)
        y = torch.empty((n,) + tuple(self.y.shape[1:]), dtype=self.y.dtype, device=self.device)
        stride = 2 * n + 1
        plan = torch.tensor(self.plan_words(ids, stride), dtype=torch.int32).to(self.device)
        self.gather_into(plan, stride, n, rows_a, rows_a.shape[0], rows_t, rows_t.shape[0], y, augment, draw)
        return rows_a[:na], len_a, rows_t[:nt], len_t, y

    def batches(self, batch_size, shuffle=True, generator=None, bucket_mult=50):
        """The id lists of one epoch: every id exactly once, the short last batch kept.  Through length_bucketed_batches on the audio
        lengths (batches of similar length; their row counts then repeat, and with them the bucket graphs of a captured step);
        bucket_mult=0: plain consecutive (shuffle=False) or shuffled slices."""
        if int(batch_size) < 1:
            raise ValueError("DeviceFeatureStore.batches: batch_size is positive")
        if bucket_mult:
            return length_bucketed_batches(self.lengths_a, int(batch_size), shuffle, generator, bucket_mult)
        n = len(self)
        order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
        return [order[k:k + int(batch_size)] for k in range(0, n, int(batch_size))]


class DevicePrefetcher:
    """Host -> device hand-over of the batches of a loader, overlapped with the step that runs on the previous batch.

    The reference copies every batch synchronously at the top of its step (``.to(device)``,
    scripts/fusion/train_fusion_seq_level_decoder.py:306-308): at cfg 2 that is 52 MB per batch, 1-4 ms of PCIe time in front
    of an 8 ms step.  Here a batch is staged in pinned host buffers (a ring of ``depth`` sets, allocated once per shape) and
    copied on a dedicated copy stream while the caller's stream still computes on the previous batch; ``__next__`` makes the
    caller's stream wait for the copy's event and hands out device tensors.  A set of staging and device buffers is reused
    only after the step that consumed it has been enqueued ``depth`` batches ago AND its copy event / the consumer stream's
    event recorded at hand-out have completed, so the ring is safe for any consumer that stays on the stream it called
    ``__next__`` on.

    ``convert`` maps the loader's item to a tuple of tensors (None entries pass through); ``dtypes`` optionally casts on the
    host before the copy (bf16 features halve the PCIe bytes).  On a CPU ``device`` the batches pass through unchanged
    (tests, gloo rehearsals).  ``mask_slots=(i, j)``: the tuple entries that are the audio / text padding masks -- the batch is
    handed out with one more element, ``(audio lengths, text lengths)`` as Python lists counted on the HOST copy of the masks, which
    is what ``DataParallelStep.step(..., lengths=)`` wants in packed (varlen) mode instead of reading the masks back from the
    device.

    ``ragged={slot: capacity_rows}``: the tuple entries whose FIRST dimension changes from batch to batch (the packed rows of
    ``collate_seq_packed``).  Their pinned staging and device buffers are allocated once, ``capacity_rows`` long (B * L covers any
    batch); a batch copies only its own ``n`` rows and is handed out as the ``[:n]`` view of the device buffer, so the buffers --
    and their addresses -- stay put while the row count changes with every batch.  Entries not named keep the behaviour above
    (buffers per shape, except that a batch whose entry is SHORTER in the first dimension only -- the labels of an epoch's short last
    batch -- is staged in the same buffers and handed out as their ``[:n]`` view).  An entry that is no tensor (the lengths as Python lists, which ``DataParallelStep.step_packed`` wants
    on the host) passes through like None."""

    def __init__(self, loader, device, depth=2, convert=None, dtypes=None, mask_slots=None, ragged=None):
        self.loader, self.device, self.depth = loader, torch.device(device), max(2, int(depth))
        self.convert, self.dtypes, self.mask_slots = convert, dtypes, mask_slots
        self.ragged = {int(k): int(v) for k, v in (ragged or {}).items()}
        self.cuda = self.device.type == "cuda"
        self._ring = [None] * self.depth          # slot -> {"host": [...], "dev": [...], "copied": event, "released": event}
        self._copy_stream = torch.cuda.Stream(device=self.device) if self.cuda else None

    def __len__(self):
        return len(self.loader)

    def _stage(self, slot, item):
        tensors = self.convert(item) if self.convert is not None else tuple(item)
        if self.dtypes is not None:
            tensors = tuple(t if (t is None or dt is None) else t.to(dt) for t, dt in zip(tensors, self.dtypes))
        extra = ()
        if self.mask_slots is not None:
            extra = (tuple((~tensors[i].bool()).sum(1).tolist() for i in self.mask_slots),)
        if not self.cuda:
            return tensors + extra, None
        ent = self._ring[slot]
        is_t = [isinstance(t, torch.Tensor) for t in tensors]
        for i, cap in self.ragged.items():
            if is_t[i] and tensors[i].shape[0] > cap:
                raise ValueError(f"DevicePrefetcher: entry {i} has {tensors[i].shape[0]} rows, its ragged capacity is {cap}")
        # a ragged entry is keyed (and its buffers are sized) by its capacity, not by the batch's row count
        full = [None if not ok else ((self.ragged[i],) + tuple(t.shape[1:]) if i in self.ragged else tuple(t.shape))
                for i, (t, ok) in enumerate(zip(tensors, is_t))]
        shapes = [None if f is None else (f, t.dtype) for f, t in zip(full, tensors)]

        def holds(have, want):
            """a buffer set serves every batch whose entries differ from it in the FIRST dimension only and are no longer there: the
            short last batch of an epoch (its labels and lengths tensors shrink with the number of utterances) is staged in the
            buffers of the full batches, like a ragged entry in its capacity"""
            if have is None or want is None:
                return have is None and want is None
            (hf, hd), (wf, wd) = have, want
            return hd == wd and len(hf) == len(wf) and hf[1:] == wf[1:] and (not wf or wf[0] <= hf[0])

        if ent is None or len(ent["shapes"]) != len(shapes) or not all(holds(h, w) for h, w in zip(ent["shapes"], shapes)):
            ent = {"shapes": shapes,
                   "host": [None if f is None else torch.empty(f, dtype=t.dtype).pin_memory() for f, t in zip(full, tensors)],
                   "dev": [None if f is None else torch.empty(f, dtype=t.dtype, device=self.device) for f, t in zip(full, tensors)],
                   "copied": torch.cuda.Event(), "released": None}
            self._ring[slot] = ent
        if ent["released"] is not None:
            ent["released"].synchronize()          # the step that read this slot's device buffers has finished
        src, out = [], []
        for i, (h, d_, t) in enumerate(zip(ent["host"], ent["dev"], tensors)):
            if not is_t[i]:
                src.append(None)
                out.append(t)
                continue
            if t.dim() and t.shape[0] != h.shape[0]:      # this batch's rows only; the views keep the buffers' base addresses
                h, d_ = h[:t.shape[0]], d_[:t.shape[0]]
            if t.is_pinned():                      # a loader with pin_memory=True hands pinned tensors over: copied from there
                src.append(t)
            else:
                h.copy_(t)                         # pageable -> pinned staging (host memcpy)
                src.append(h)
            out.append(d_)
        ent["src"] = src                           # referenced until the slot is staged again: the copy below is asynchronous
        with torch.cuda.stream(self._copy_stream):
            for h, d_ in zip(src, out):
                if h is not None:
                    d_.copy_(h, non_blocking=True)
            ent["copied"].record(self._copy_stream)
        return tuple(out) + extra, ent

    def __iter__(self):
        it = iter(self.loader)
        pending = []                               # staged batches, oldest first
        k = 0

        def stage_next():
            nonlocal k
            try:
                item = next(it)
            except StopIteration:
                return
            pending.append(self._stage(k % self.depth, item))
            k += 1

        for _ in range(self.depth - 1):
            stage_next()
        while pending:
            batch, ent = pending.pop(0)
            if ent is not None:
                torch.cuda.current_stream(self.device).wait_event(ent["copied"])
            yield batch
            # resumed when the caller asks for the next batch, i.e. AFTER it has enqueued its step on this one: the host-side
            # staging of a later batch (pageable -> pinned memcpy) and its copy now run beside that step on the GPU
            if ent is not None:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                ent["released"] = ev
            stage_next()
