"""Drop-in for the reference's models/cross_modal_block_tacfn.py (CrossModalBlock :6-125,
CrossModalTransformer :130-166): same constructor arguments, forward signature, return tuples and
state_dict keys; the arithmetic runs in the gfx950 kernels of libhriemo.so.

The torch.nn modules created here (MultiheadAttention, LayerNorm, Linear) are PARAMETER CONTAINERS only
-- identical key names and default initialisation as the reference, their forward() is never called.

Internally every activation of the residual stream travels as a pair (bf16 copy for the GEMM operands,
fp32 twin for the residual/LayerNorm path): see _ops.as_pair and DESIGN.md (precision)."""
import torch
import torch.nn as nn

try:
    from .. import _ops
except ImportError:            # imported as top-level `models` (PYTHONPATH=<repo>/hri-emo_amd, the reference's import path)
    from hri_emo_amd import _ops


class CrossModalBlock(nn.Module):
    def __init__(self, d_model=768, n_heads=8, dropout=0.1):
        super().__init__()
        self.d_model, self.n_heads, self.p = d_model, n_heads, float(dropout)
        self.self_attn_a = nn.MultiheadAttention(d_model, n_heads, dropout=dropout, batch_first=True)
        self.self_attn_t = nn.MultiheadAttention(d_model, n_heads, dropout=dropout, batch_first=True)
        self.self_norm_a = nn.LayerNorm(d_model)
        self.self_norm_t = nn.LayerNorm(d_model)
        self.attn_a2t = nn.MultiheadAttention(d_model, n_heads, dropout=dropout, batch_first=True)
        self.attn_t2a = nn.MultiheadAttention(d_model, n_heads, dropout=dropout, batch_first=True)
        self.ffn_a = nn.Sequential(nn.Linear(d_model, 4 * d_model), nn.ReLU(), nn.Linear(4 * d_model, d_model))
        self.ffn_t = nn.Sequential(nn.Linear(d_model, 4 * d_model), nn.ReLU(), nn.Linear(4 * d_model, d_model))
        self.norm_a1 = nn.LayerNorm(d_model)
        self.norm_a2 = nn.LayerNorm(d_model)
        self.norm_t1 = nn.LayerNorm(d_model)
        self.norm_t2 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self._sh = _ops.Shadows()
        self._site = [_ops.new_site_base() for _ in range(6)]
        self.batch_offset = 0          # global index of this shard's first utterance (data parallel)

    def _self(self, x, x32, mha, ln, seq, p, seed, site, need_w):
        return _ops.SelfAttnLN.apply(x, x32, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight,
                                     mha.out_proj.bias, ln.weight, ln.bias, self._sh, self.n_heads, seq, p, seed, site,
                                     self.batch_offset, need_w)

    def _cross(self, xq, xq32, xkv, mha, ln, seq_q, seq_k, p, seed, site, need_w, kv_pre=None, join_q=None, q_pre=None, slots=None):
        return _ops.CrossAttnLN.apply(xq, xq32, xkv, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight,
                                      mha.out_proj.bias, ln.weight, ln.bias, self._sh, self.n_heads, seq_q, seq_k, p, seed,
                                      site, self.batch_offset, need_w, kv_pre, join_q, q_pre, slots)

    def _shared_proj(self, x, mha_q, mha_kv, join):
        """[Q of the cross-attention `x` queries | K, V of the one it serves] from ONE N = 3d GEMM (_ops.SharedProjFn);
        -> (q, kv, SharedGrad the two attention backwards write dQ and dK | dV into)"""
        sg = _ops.SharedGrad(x.shape[0] * x.shape[1], x.shape[2], x.device)
        q, kv = _ops.SharedProjFn.apply(x, mha_q.in_proj_weight, mha_q.in_proj_bias, mha_kv.in_proj_weight, mha_kv.in_proj_bias,
                                        self._sh, join, sg)
        return q, kv, sg

    def _kv(self, xkv, mha, join):
        """K | V projection of a cross-attention as its own node (_ops.KVProjFn): the gradient it returns for `xkv` meets the
        gradient the OTHER cross-attention returns for the same tensor as its query side in a GradJoin"""
        return _ops.KVProjFn.apply(xkv, mha.in_proj_weight, mha.in_proj_bias, self._sh, join)

    def _ffn(self, x, x32, ffn, ln, p, seed, site, seq):
        return _ops.FFNLN.apply(x, x32, ffn[0].weight, ffn[0].bias, ffn[2].weight, ffn[2].bias, ln.weight, ln.bias,
                                self._sh, p, 0.0, seed, site, self.batch_offset, seq)

    def _fwd_pair(self, a, a32, t, t32, sa, st, need):
        """(bf16, fp32-twin) pairs in and out; returns (a, a32, t, t32, maps|None).
        sa / st: the _ops.Seq of a's and of t's rows -- padded [B, L, d] with the padding masks, or the packed valid rows
        ([1, N, d], _ops.pack_pair), for which the attention kernels get cu_seqlens instead of padding masks.
        need: a bool, or {site name: _ops.LogSite} -- the four maps then go to a train.AttentionLog and none is returned."""
        logged = isinstance(need, dict)
        nw = need if logged else dict.fromkeys(("audio_self", "text_self", "audio_queries_text", "text_queries_audio"), need)
        p = self.p if self.training else 0.0
        seed = _ops.next_seed(self.training and p > 0)
        s = self._site
        _ops._require_gpu(a)
        # fp32 inference mode: the key/value side of a cross-attention reads the fp32 twin of the other branch, not its bf16 copy
        fp32 = _ops.precision() == "fp32"
        kv = lambda x16, x32: x32 if (fp32 and x32 is not None) else x16          # noqa: E731
        main = torch.cuda.current_stream(a.device)
        _ops.note_main_stream(main)
        side = _ops.side_stream(a.device)
        # Each self-attention output has two consumers -- the queries of its own cross-attention and the keys / values of the
        # other one.  With the K | V projections as their own nodes, created BEFORE both cross-attention cores, the engine runs
        # the cores' backward first (they deposit the query-side gradients) and the projections' backward last, where one
        # dX GEMM adds the deposit in its epilogue: no elementwise add launches on [B*L, d] (_ops.GradJoin).
        # A join exists only where BOTH consumers are certain to get a backward node that must produce the shared activation's
        # gradient, i.e. where that activation requires grad: with a frozen cross-attention and inputs that need no gradient the
        # partner's node never runs and a deposit would be stranded (autograd then sums whatever gradients there are).
        use_kv = not fp32
        join_for = lambda x: _ops.grad_join(2) if (use_kv and x.requires_grad) else None          # noqa: E731
        d = a.shape[2]
        shared = use_kv and _ops.shared_proj()
        # The audio and text branches only meet at the two cross-attentions (each reads the OTHER branch's self-attention output),
        # so the text branch runs on a second stream (_ops.TextBranch; in line on main without one): its small grids (B*T_t rows)
        # fill the CUs the audio branch leaves idle.  Tensors that cross streams are recorded on the consumer stream (allocator
        # safety); autograd replays the same streams in backward.  The audio branch -- three times the rows, the critical path --
        # is ENQUEUED first at every fork (the reference's order of sub-layers, :74-119): the order of capture decides which
        # branch the graph runtime starts first.
        tb = _ops.TextBranch(side, main)
        tb.fork(t, t32, st, sa)
        # stage 1, nothing of the other branch needed yet: self-attention and, shared, ONE N = 3d GEMM that projects its output to
        # [Q of the branch's own cross-attention | K, V of the other one]
        q_a2t = q_t2a = kv_t2a = kv_a2t = slots_a = slots_t = None
        a_s, a_s32, w_a = self._self(a, a32, self.self_attn_a, self.self_norm_a, sa, p, seed, s[0], nw["audio_self"])         # :74-81
        ja = join_for(a_s)
        if shared:
            q_a2t, kv_t2a, sga = self._shared_proj(a_s, self.attn_a2t, self.attn_t2a, ja)
        with tb.run():
            t_s, t_s32, w_t = self._self(t, t32, self.self_attn_t, self.self_norm_t, st, p, seed, s[1], nw["text_self"])     # :85-92
            jt = join_for(t_s)
            if shared:
                q_t2a, kv_a2t, sgt = self._shared_proj(t_s, self.attn_t2a, self.attn_a2t, jt)
        # the exchange: the K | V halves cross streams, or the self-attention outputs do (in fp32 mode their twins too) and each
        # stream projects the K | V of the cross-attention it runs
        if shared:
            tb.join(kv_a2t)
            tb.fork(kv_t2a)
            slots_a, slots_t = (sga.slot(0, d), sgt.slot(d, 3 * d)), (sgt.slot(0, d), sga.slot(d, 3 * d))
        else:
            tb.join(t_s, t_s32 if fp32 else None)
            tb.fork(a_s, a_s32 if fp32 else None)
            if use_kv:
                with tb.run():
                    kv_t2a = self._kv(a_s, self.attn_t2a, ja)
                kv_a2t = self._kv(t_s, self.attn_a2t, jt)
        # stage 2: cross-attention + FFN
        x, x32, w_a2t = self._cross(a_s, a_s32, kv(t_s, t_s32), self.attn_a2t, self.norm_a1, sa, st, p, seed, s[2], nw["audio_queries_text"],
                                    kv_a2t, ja, q_a2t, slots_a)                                                    # :98-105
        a_cm, a_cm32 = self._ffn(x, x32, self.ffn_a, self.norm_a2, p, seed, s[3], sa)                              # :106
        with tb.run():
            x, x32, w_t2a = self._cross(t_s, t_s32, kv(a_s, a_s32), self.attn_t2a, self.norm_t1, st, sa, p, seed, s[4], nw["text_queries_audio"],
                                        kv_t2a, jt, q_t2a, slots_t)                                                # :111-118
            t_cm, t_cm32 = self._ffn(x, x32, self.ffn_t, self.norm_t2, p, seed, s[5], st)                          # :119
        tb.join(t_cm, t_cm32, w_t, w_t2a)
        maps = {"audio_self": w_a, "text_self": w_t, "audio_queries_text": w_a2t, "text_queries_audio": w_t2a} if (need and not logged) else None
        return a_cm, a_cm32, t_cm, t_cm32, maps

    def forward(self, h_a, h_t, mask_a=None, mask_t=None, return_attention=False):
        out_dtype = h_a.dtype          # outputs come back in the caller's dtype
        a, a32 = _ops.as_pair(h_a)
        t, t32 = _ops.as_pair(h_t)
        sa, st = _ops.Seq.padded(a.shape[0], a.shape[1], mask_a), _ops.Seq.padded(t.shape[0], t.shape[1], mask_t)
        a, a32, t, t32, maps = self._fwd_pair(a, a32, t, t32, sa, st, bool(return_attention))
        h_a_cm, h_t_cm = _ops.from_pair(a, a32, out_dtype), _ops.from_pair(t, t32, out_dtype)
        if return_attention:
            return h_a_cm, h_t_cm, maps
        return h_a_cm, h_t_cm


class CrossModalTransformer(nn.Module):
    def __init__(self, num_layers=2, d_model=768, n_heads=8, dropout=0.1):
        super().__init__()
        self.layers = nn.ModuleList([CrossModalBlock(d_model, n_heads, dropout) for _ in range(num_layers)])

    def _fwd_pair(self, a, a32, t, t32, mask_a, mask_t, need, tail=False, raw=False, plan=None, padded=False):
        """-> (a, a32, t, t32, maps, (sa, st, sf)): the outputs, the _ops.Seq of their rows and the Seq of the fused memory the gate
        makes of them.  tail: the caller can take the packed tail (_ops.PACKED_TAIL).  When the encoder ran packed, its outputs then
        STAY packed ([1, N, d] pairs) and the layouts are the plan (Seq audio, Seq text, Seq fused) -- the gate and the decoder read
        the packed rows, nothing is scattered back.  Otherwise (and always for forward() below, whose public output is padded) the
        outputs are unpacked as before and the layouts are the padded ones.
        raw (_ops.INGEST_ROWS): a / t are still the caller's tensors (a32 / t32 None); ONE launch each makes the pairs here, gathered
        straight into the packed rows where the encoder packs (_ops.ingest_pair).  plan: the caller's packed plan, a / t are already
        its packed pairs (forward_packed): the encoder runs packed whatever set_varlen says.
        need: a bool, or a train.AttentionLog's encoder sites (per layer {name: _ops.LogSite}): the maps go to the log, `maps` is [].
        padded: the encoder stays on the padded layout whatever set_varlen says (FusionClassifier's pooled path: its unmasked mean
        reads the PAD rows of the output, which the unpack of a packed run writes as zeros)."""
        all_layers_attn = []
        given = plan is not None
        B, La, Lt = (plan[0].Breal, plan[0].L, plan[1].L) if given else (a.shape[0], a.shape[1], t.shape[1])
        _ops.FLUSH_SITES.add(self.layers[0]._site[1])        # layer-0 text self-attention: the last text-branch backward (_ops._DeferredWgrad)
        if not given and not padded and _ops.varlen() and (not need or _ops.varlen_maps()) and mask_a is not None and mask_t is not None:
            # the encoder on the valid rows only (prefix masks, as the collate builds them); anything else
            # takes the padded path.  dp.DataParallelStep injects bucketed plans whose lengths are device data (_ops.CTX.seq_override).
            if _ops.CTX.seq_override is not None:
                plan = tuple(_ops.CTX.seq_override)
            else:
                plan = _ops.seq_plans(mask_a, mask_t, B, La, Lt)
            if plan is not None:
                if raw:
                    (a, a32), (t, t32) = _ops.ingest_pair(a, plan[0]), _ops.ingest_pair(t, plan[1])
                else:
                    (a, a32), (t, t32) = _ops.pack_pair(a, a32, plan[0]), _ops.pack_pair(t, t32, plan[1])
        if raw and plan is None:
            (a, a32), (t, t32) = _ops.ingest_pair(a, _ops.Seq.padded(B, La)), _ops.ingest_pair(t, _ops.Seq.padded(B, Lt))
        if _ops.CTX.act_log is not None:          # the rows the encoder starts from (train.ActivationLog: input.audio, input.text)
            s0 = plan[:2] if plan is not None else (_ops.Seq.padded(B, La, mask_a), _ops.Seq.padded(B, Lt, mask_t))
            _ops.probe("input.audio", 0, a, s0[0])
            _ops.probe("input.text", 0, t, s0[1])
        for i, layer in enumerate(self.layers):
            # (padded: every layer converts the masks itself, as it always did -- a view for bool masks)
            sa, st = plan[:2] if plan is not None else (_ops.Seq.padded(B, La, mask_a), _ops.Seq.padded(B, Lt, mask_t))
            a, a32, t, t32, maps = layer._fwd_pair(a, a32, t, t32, sa, st, need[i] if isinstance(need, list) else need)
            if maps is not None:
                all_layers_attn.append(maps)
        if plan is not None:
            if tail and len(plan) == 3 and _ops.packed_tail():
                return a, a32, t, t32, all_layers_attn, plan
            (a, a32), (t, t32) = _ops.unpack_pair(a, a32, plan[0]), _ops.unpack_pair(t, t32, plan[1])
        return a, a32, t, t32, all_layers_attn, (_ops.Seq.padded(B, La), _ops.Seq.padded(B, Lt), _ops.Seq.padded(B, Lt))

    def forward(self, h_a, h_t, mask_a=None, mask_t=None, return_attention=False):
        out_dtype = h_a.dtype
        raw = h_a.dim() == 3 and h_t.dim() == 3 and _ops.ingestible(h_a, h_t)
        a, a32 = (h_a, None) if raw else _ops.as_pair(h_a)
        t, t32 = (h_t, None) if raw else _ops.as_pair(h_t)
        a, a32, t, t32, maps, _ = self._fwd_pair(a, a32, t, t32, mask_a, mask_t, bool(return_attention), raw=raw)
        h_a, h_t = _ops.from_pair(a, a32, out_dtype), _ops.from_pair(t, t32, out_dtype)
        if return_attention:
            return h_a, h_t, maps
        return h_a, h_t
