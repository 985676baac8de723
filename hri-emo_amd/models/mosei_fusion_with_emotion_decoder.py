"""Drop-in for the reference's models/mosei_fusion_with_emotion_decoder.py (MoseiFusionWithEmotionDecoder
:8-79): two input projections (COVAREP d=74, GloVe d=300 -> d_model) in front of the fusion backbone; same
constructor arguments, return tuples and state_dict keys (``audio_proj.*``, ``text_proj.*``, ``backbone.*``), so
the reference's MOSEI checkpoints load."""
import torch
import torch.nn as nn

try:
    from .. import _ops
except ImportError:            # imported as top-level `models` (PYTHONPATH=<repo>/hri-emo_amd, the reference's import path)
    from hri_emo_amd import _ops
from .fusion_with_emotion_decoder import FusionWithEmotionDecoder, _check_attn_log


class MoseiFusionWithEmotionDecoder(nn.Module):
    def __init__(self, d_audio: int, d_text: int, d_model: int = 256, num_emotions: int = 6, n_heads: int = 4,
                 num_layers_fusion: int = 2, num_layers_decoder: int = 2, beta_hidden: int = 128,
                 dropout: float = 0.2):
        super().__init__()
        self.audio_proj = nn.Linear(d_audio, d_model)      # parameter containers (reference keys / init)
        self.text_proj = nn.Linear(d_text, d_model)
        self.backbone = FusionWithEmotionDecoder(d_model=d_model, num_emotions=num_emotions, n_heads=n_heads,
                                                 num_layers_fusion=num_layers_fusion,
                                                 num_layers_decoder=num_layers_decoder, beta_hidden=beta_hidden,
                                                 dropout=dropout)
        self._sh = _ops.Shadows()

    def set_batch_offset(self, offset: int):
        self.backbone.set_batch_offset(offset)

    def forward(self, h_a, h_t, mask_a=None, mask_t=None, return_attention=False):
        if _ops.CTX.act_log is not None:
            _ops.CTX.act_log._guard()          # refused before the projections are enqueued
        h_a_proj = _ops.LinearFn.apply(h_a, self.audio_proj.weight, self.audio_proj.bias, self._sh)   # :63
        h_t_proj = _ops.LinearFn.apply(h_t, self.text_proj.weight, self.text_proj.bias, self._sh)     # :65
        return self.backbone(h_a_proj, h_t_proj, mask_a, mask_t, return_attention=return_attention)   # :68-79

    def forward_packed(self, rows_a, rows_t, lengths_a, lengths_t, pad_to=None, return_attention=False, attn_log=None):
        """forward for ragged data (FusionWithEmotionDecoder.forward_packed): rows_a [sum(lengths_a), d_audio] and rows_t
        [sum(lengths_t), d_text]; the two input projections run over the valid rows only; attn_log as there"""
        la, lt, (La, Lt) = _ops.packed_lengths(rows_a, rows_t, lengths_a, lengths_t, pad_to, same_width=False)
        _check_attn_log(self.backbone, attn_log, return_attention, (La, Lt))
        if (return_attention or attn_log is not None) and not _ops.varlen_maps():
            raise ValueError("forward_packed: attention maps of packed rows need set_varlen_maps(True)")
        _ops._require_gpu(rows_a)
        plan, masks = _ops.plans_from_lengths(la, lt, La, Lt, rows_a.device)
        if attn_log is not None:
            attn_log.plan(torch.tensor([la, lt], dtype=torch.int32).to(rows_a.device, non_blocking=True))
        return self._forward_rows(rows_a, rows_t, plan, masks, (La, Lt), return_attention, attn_log)

    def _forward_rows(self, rows_a, rows_t, plan, masks, pad, return_attention=False, attn_log=None):
        """forward_packed behind its argument check (FusionWithEmotionDecoder._forward_rows): the projections run over the first
        plan.N rows of each source -- all of them for a batch's own plan; for a bucket plan the bucket's row count, a slice that is
        static per bucket graph (the caller keeps the rows between the batch's last row and plan.N finite: their gradient is zero,
        and zero times a NaN would not be)"""
        if _ops.CTX.act_log is not None:
            _ops.CTX.act_log._guard()          # refused before the projections are enqueued
        a = _ops.LinearFn.apply(rows_a[:plan[0].N], self.audio_proj.weight, self.audio_proj.bias, self._sh)
        t = _ops.LinearFn.apply(rows_t[:plan[1].N], self.text_proj.weight, self.text_proj.bias, self._sh)
        return self.backbone._forward_rows(a, t, plan, masks, pad, return_attention, attn_log)
