"""Drop-in for the reference's models/fusion_with_emotion_decoder.py (FusionWithEmotionDecoder :10-197)."""
import torch
import torch.nn as nn

try:
    from .. import _ops
except ImportError:            # imported as top-level `models` (PYTHONPATH=<repo>/hri-emo_amd, the reference's import path)
    from hri_emo_amd import _ops
from .cross_modal_block_tacfn import CrossModalTransformer
from .beta_gate_tacfn import BetaGate
from .emotion_decoder import EmotionDecoder


def _check_attn_log(model, attn_log, return_attention, pad):
    """the argument check of forward_packed(attn_log=...) / _forward_rows(attn_log=...): ValueError before anything is launched"""
    if attn_log is None:
        return
    if return_attention:
        raise ValueError("forward_packed: return_attention=True and attn_log= exclude each other (with a log the maps live in the log)")
    why = attn_log.mismatch(model, pad)
    if why is not None:
        raise ValueError(f"forward_packed: the attention log does not fit: {why}")


class FusionWithEmotionDecoder(nn.Module):
    def __init__(self, d_model: int = 768, num_emotions: int = 4, n_heads: int = 8, num_layers_fusion: int = 2,
                 num_layers_decoder: int = 2, beta_hidden: int = 256, dropout: float = 0.1):
        super().__init__()
        self.cross_modal = CrossModalTransformer(num_layers=num_layers_fusion, d_model=d_model, n_heads=n_heads,
                                                 dropout=dropout)
        self.beta_gate = BetaGate(d_model=d_model, hidden_dim=beta_hidden)
        self.emotion_decoder = EmotionDecoder(d_model=d_model, num_emotions=num_emotions, n_heads=n_heads,
                                              num_layers=num_layers_decoder, dropout=dropout, use_output_layer=True)

    def set_batch_offset(self, offset: int):
        """Global index of this shard's first utterance: keeps dropout masks independent of how the
        batch is sharded across GPUs (hri_emo_amd.dp)."""
        for m in self.modules():
            if hasattr(m, "batch_offset"):
                m.batch_offset = int(offset)

    def _prefetch_shadows(self, device):
        """bf16 copies of the gate's and the decoder's weight matrices, cast on the side stream at the top of the step, beside the
        first fusion layer, instead of one ~5 us launch in front of every GEMM of the decoder's latency-bound chain.  Returns the
        event the consumer stream waits for, or None (one stream / fp32 / fp8 mode)."""
        if _ops.precision() != "bf16" or not device.type == "cuda":
            return None
        side = _ops.side_stream(device)
        if side is None:
            return None
        main = torch.cuda.current_stream(device)
        _ops.fork(side, main)                       # the masters may have just been updated on the caller's stream
        with torch.cuda.stream(side):
            g = self.beta_gate
            pairs = [(g._sh, g.mlp[0].weight), (g._sh, g.mlp[2].weight)]
            for layer in self.emotion_decoder.layers:
                pairs += [(layer._sh, w) for w in (layer.self_attn.in_proj_weight, layer.self_attn.out_proj.weight,
                                                   layer.cross_attn.in_proj_weight, layer.cross_attn.out_proj.weight,
                                                   layer.linear1.weight, layer.linear2.weight)]
            _ops.prefetch_batch(pairs)          # one launch for the fourteen matrices (the step time is the same as with fourteen:
            #                                     7.45 vs 7.45 ms -- the graph runtime starts the branches late either way)
            ev = torch.cuda.Event()
            ev.record(side)
        return ev

    def _ensure_3d(self, x):
        if x.dim() == 2:
            return x.unsqueeze(1)
        if x.dim() == 3:
            return x
        raise ValueError(f"Expected 2D or 3D tensor, got {x.shape}")

    def _build_fused_mask(self, mask_a, mask_t, L_fused):
        if mask_a is None and mask_t is None:
            return None

        def fit(m):
            if m is None:
                return None
            if m.size(1) < L_fused:
                pad = torch.ones(m.size(0), L_fused - m.size(1), dtype=torch.bool, device=m.device)
                return torch.cat([m, pad], dim=1)
            return m[:, :L_fused]

        ma, mt = fit(mask_a), fit(mask_t)
        if ma is None:
            return mt
        if mt is None:
            return ma
        return ma | mt

    def forward(self, h_a, h_t, mask_a=None, mask_t=None, return_attention=False):
        h_a, h_t = self._ensure_3d(h_a), self._ensure_3d(h_t)
        if _ops.CTX.act_log is not None:
            _ops.CTX.act_log._guard()          # an activation log in fp32 precision: refused before anything is enqueued
        # one cast at the boundary; between the sub-modules activations travel as (bf16, fp32-twin) pairs
        # (_ops.INGEST_ROWS: the pairs are made by the encoder's entry, one launch each, packed where it packs)
        raw = _ops.ingestible(h_a, h_t)
        a, a32 = (h_a, None) if raw else _ops.as_pair(h_a)
        t, t32 = (h_t, None) if raw else _ops.as_pair(h_t)
        return self._run(a, a32, t, t32, mask_a, mask_t, h_t.size(1), h_a.dtype, return_attention, raw=raw)

    def forward_packed(self, rows_a, rows_t, lengths_a, lengths_t, pad_to=None, return_attention=False, attn_log=None):
        """forward for a batch that is already ragged: rows_a / rows_t [sum(lengths), d] (fp32, bf16 or fp16) hold the valid rows of
        all utterances back to back, lengths_a / lengths_t are host sequences or CPU int tensors.  pad_to = (L_a, L_t), default the
        batch maxima: the padded lengths the reference's collate would produce -- they key the dropout hash and size the returned
        attention maps.  One launch per modality takes the rows in (hriemo_ingest_rows); the encoder always runs packed, whatever
        set_varlen says; packed_tail() decides whether the gate and the decoder stay packed; return_attention needs
        set_varlen_maps(True).  Returns what forward returns for the padded batch and its masks.
        attn_log: a train.AttentionLog -- the maps of the samples its window takes go straight into the log (one plan launch, fed by
        one small int32 upload of the lengths, then every site exports into its slots); the 3-tuple comes back.  Needs
        set_varlen_maps(True) as return_attention does, and excludes it."""
        la, lt, (La, Lt) = _ops.packed_lengths(rows_a, rows_t, lengths_a, lengths_t, pad_to)
        _check_attn_log(self, attn_log, return_attention, (La, Lt))
        if (return_attention or attn_log is not None) and not _ops.varlen_maps():
            raise ValueError("forward_packed: attention maps of packed rows need set_varlen_maps(True)")
        _ops._require_gpu(rows_a)
        plan, masks = _ops.plans_from_lengths(la, lt, La, Lt, rows_a.device)
        if attn_log is not None:
            attn_log.plan(torch.tensor([la, lt], dtype=torch.int32).to(rows_a.device, non_blocking=True))
        return self._forward_rows(rows_a, rows_t, plan, masks, (La, Lt), return_attention, attn_log)

    def _forward_rows(self, rows_a, rows_t, plan, masks, pad, return_attention=False, attn_log=None):
        """forward_packed behind its argument check: the packed rows, their plan (Seq audio, Seq text, Seq fused), the padded bool
        masks (mask_a [B, L_a], mask_t [B, L_t] and optionally the fused mask [B, L_t], which then stands in for _build_fused_mask
        when the tail is unpacked) and pad = (L_a, L_t).  dp.DataParallelStep.step_packed calls it with a BUCKET plan (_ops.seq_bucket,
        _ops.seq_bucket_fused) and masks in device memory that hriemo_seq_tables wrote: rows_a / rows_t may then hold more rows than
        the batch has (the ingest launch never reads past cu[B]).  attn_log: the caller has run the log's plan launch for this pass
        (AttentionLog.plan); the sites export under the window it wrote."""
        _check_attn_log(self, attn_log, return_attention, pad)
        if attn_log is not None and not _ops.varlen_maps():
            raise ValueError("forward_packed: attention maps of packed rows need set_varlen_maps(True)")
        if _ops.CTX.act_log is not None:
            _ops.CTX.act_log._guard()          # an activation log in fp32 precision: refused before anything is enqueued
        a, a32 = _ops.ingest_pair(rows_a, plan[0], src_packed=True)
        t, t32 = _ops.ingest_pair(rows_t, plan[1], src_packed=True)
        return self._run(a, a32, t, t32, masks[0], masks[1], pad[1], rows_a.dtype, return_attention, plan=plan,
                         fused_mask=masks[2] if len(masks) > 2 else None, attn_log=attn_log)

    def _run(self, a, a32, t, t32, mask_a, mask_t, Lt, out_dtype, return_attention, raw=False, plan=None, fused_mask=None, attn_log=None):
        """the model behind its entry: a / t as pairs (raw: still the caller's tensors; plan: the packed pairs of that plan;
        fused_mask: the decoder's memory mask [B, L_t] where the caller has it already; attn_log: with a plan only -- the sites are
        visited in a fixed order, encoder layers first, each taking its tensor from the log; a half the log does not keep is not
        exported at all)"""
        need = need_enc = need_dec = bool(return_attention)
        if attn_log is not None:
            # (B: the plan's real samples -- a bucket plan's filler sequence has no map)
            enc_sites, dec_sites = attn_log.sites(plan[0].Breal)
            need, need_enc, need_dec = True, enc_sites or False, dec_sites or False
        act_log = _ops.CTX.act_log
        if act_log is not None:
            # a train.ActivationLog: its plan launch comes in front of every fork of the pass (the only writer of the window the
            # probes of the sub-layers read), its forward fold behind every join
            act_log.begin_pass()
        _ops.begin_step()
        # the decoder's memory mask needs the two padding masks only (L_fused = T_t, beta_gate_tacfn.py:98-116): built here, not on
        # the decoder's serial chain behind the gate
        # (not needed when the tail stays packed: the fused Seq carries the lengths; masks without a plan build it late)
        may_pack = (plan is not None or (_ops.varlen() and (not need or _ops.varlen_maps()) and mask_a is not None
                                         and mask_t is not None)) and _ops.packed_tail()
        fused_early = None if may_pack else (fused_mask if fused_mask is not None else self._build_fused_mask(mask_a, mask_t, Lt))
        ready = self._prefetch_shadows(a.device)
        _ops.CTX.join_scope += 1          # logits, beta and z all depend on both branches: the encoder's gradient joins are safe
        try:                              # seqs: the layouts of a, t and the fused memory (the packed plan when the tail stays packed)
            a, a32, t, t32, encoder_attns, seqs = self.cross_modal._fwd_pair(a, a32, t, t32, mask_a, mask_t, need_enc, tail=True, raw=raw,
                                                                             plan=plan)
        finally:
            _ops.CTX.join_scope -= 1
        if ready is not None:
            torch.cuda.current_stream(a.device).wait_event(ready)
        h_fusion, beta = self.beta_gate._fwd_pair(a, a32, t, t32, mask_a, mask_t, seqs)
        sm = seqs[2]                      # packed tail: the gate read the packed rows, the decoder reads a packed fused memory
        if not sm.packed and fused_mask is not None:
            sm = sm.with_kpm(fused_mask)
        elif not sm.packed:
            sm = sm.with_kpm(fused_early if (fused_early is not None and h_fusion.size(1) == Lt) else
                             self._build_fused_mask(mask_a, mask_t, h_fusion.size(1)))
        z, logits, decoder_attns = self.emotion_decoder._fwd(h_fusion, sm, need_dec, out_dtype)
        if act_log is not None:
            act_log.end_forward()
        if return_attention:
            return logits, beta, z, {"encoder": encoder_attns, "decoder": decoder_attns}
        return logits, beta, z
