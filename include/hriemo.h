/* hriemo.h -- C ABI of libhriemo.so: the MI355X (gfx950) kernels behind HRI-EMO's cross-modal fusion +
 * beta-gate + emotion-decoder forward/backward path.
 *
 * The reference (Makiato1999/HRI-EMO) has no FFI layer: every FLOP of this path is a stock torch.nn
 * call inside models/ (SURVEY.md section 8b).  Each entry point below therefore names the reference
 * nn.Module arithmetic it replaces (file:line under the reference tree); the Python mirror of the
 * reference's nn.Module API (hri-emo_amd/models/) binds these symbols with ctypes.
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller (outputs and
 *    workspaces included); nothing is allocated, freed or synchronised inside (graph-capturable);
 *  - activations are bf16 (uint16 storage) row-major with an explicit leading dimension in ELEMENTS;
 *    statistics, parameters' masters, gradients of parameters are fp32;
 *  - masks are uint8 [B, L], 1 = PAD (the reference's key_padding_mask convention);
 *  - dropout is replayed from (seed, site, row/col) -- the backward takes the same triple, no mask is
 *    stored; p_drop = 0 disables it; the effective seed is seed + *seed_dev (device word, may be NULL) so a
 *    captured hipGraph can draw fresh masks per replay by bumping that word inside the graph;  b_offset / row_offset = global index of the first utterance/row
 *    of this shard so masks do not depend on how the batch is sharded over GPUs;
 *  - `stream` is a hipStream_t; return 0 = ok, otherwise hriemo_last_error() explains.
 */
#ifndef HRIEMO_H_
#define HRIEMO_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hriemo_stream_t;

const char* hriemo_last_error(void);
int hriemo_abi_version(void);

/* ---- GEMM: every nn.Linear / packed in-projection / out-projection on the path and their backward.
 * C[M,N] = opA(A) . opB(B) (+bias) with fp32 accumulation on MFMA 16x16x32 bf16.
 *   ta=0: A is [M,K] (K contiguous)      ta=1: A is [K,M] (dW = dY^T . X)
 *   tb=0: B is [N,K] (weight layout)     tb=1: B is [K,N] (dX = dY . W)
 * c_is_f32: 0 -> bf16 C, 1 -> fp32 C (weight gradients; split-K through `workspace`).
 * epilogue (bf16 C only): 0 none, 1 ReLU, 2 multiply by (aux > 0) (ReLU backward), 3 add aux
 *   (fuses the residual-branch gradient into the dX GEMM).
 * Replaces: F.linear in nn.MultiheadAttention in-proj/out-proj (models/cross_modal_block_tacfn.py:24-40,
 * 74-117; models/emotion_decoder.py:14,20,42-54), ffn_a/ffn_t (cross_modal_block_tacfn.py:43-52,106,119),
 * linear1/linear2 (emotion_decoder.py:25-27,58), gate MLP (models/beta_gate_tacfn.py:62-66,92). */
int hriemo_gemm_bf16(int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                     void* C, long ldc, int c_is_f32, const float* bias, int epilogue, const void* aux,
                     long ldaux, int accumulate, float* workspace, long workspace_bytes, hriemo_stream_t stream);

/* njobs independent weight-gradient GEMMs C_j[M_j, N_j] (+)= A_j[K_j, M_j]^T . B_j[K_j, N_j] (layout ta = 1, tb = 1 of
 * hriemo_gemm_bf16, fp32 results, no split-K) in ONE launch per 16 problems: jobs_host = HOST array of njobs x 9 int64
 * {M, N, K, A, lda, B, ldb, C, ldc}, passed through kernel arguments (capture-safe).  The decoder's and the gate's weight gradients
 * (models/emotion_decoder.py:14-27, models/beta_gate_tacfn.py:62-66: M = B*N_e or B reduction rows), 16 latency-bound launches
 * per step otherwise. */
int hriemo_gemm_bf16_group_tn(const void* jobs_host, int njobs, int accumulate, hriemo_stream_t stream);
/* hriemo_gemm_bf16 with an fp32 result written to TWO matrices: rows [0, split_m) of the [M, N] result to C, rows [split_m, M) to
 * C2 (from its row 0).  The weight gradient of a projection whose weight rows belong to two parameters -- one N = 3d GEMM per
 * shared input: rows [0, d) are the Q rows of one nn.MultiheadAttention.in_proj_weight, rows [d, 3d) the K | V rows of another
 * (models/cross_modal_block_tacfn.py:98-104,111-117) -- in one launch.  accumulate as in hriemo_gemm_bf16. */
int hriemo_gemm_bf16_split(int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                           void* C2, long ldc2, int split_m, int accumulate, float* workspace, long workspace_bytes,
                           hriemo_stream_t stream);
/* C[M,N] (bf16) = (A . B) * (aux > 0) as hriemo_gemm_bf16 with epilogue 2, plus the column sums of the stored (masked, rounded)
 * C as per-row-block partials [hriemo_gemm_colsum_rows(ta,tb,M,N,K)][N] fp32 -- summed over rows (hriemo_colreduce_batch) they
 * are the bias gradient of the FIRST Linear of a feed-forward block (dh = (dy . W2) * relu'(h), db1 = colsum(dh);
 * cross_modal_block_tacfn.py:43-52,106,119) without a second pass over dh. */
int hriemo_gemm_colsum_rows(int ta, int tb, int M, int N, int K);
int hriemo_gemm_bf16_colsum(int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                            const void* aux, long ldaux, float* colsum_partials, hriemo_stream_t stream);
/* tuning hook: force one of the built tile configurations (-1 = built-in heuristic); 0-8: work-queue kernels (128x128 ... 32x64
 * tiles), 9: the loader / consumer kernel (256x128 tile, 8 MFMA waves + 4 waves that only stage operands; round 4, the default for
 * encoder-sized projections and long weight-gradient reductions) */
int hriemo_gemm_force_config(int cfg);
/* Tuning word of every following GEMM launch (default 9); returns the previous value.  Bit 0: in the 3-stage 256x128 kernel the
 * first K-step after an epilogue counts that epilogue's stores in its retire wait instead of waiting for their acknowledgement;
 * bit 1: never pick configuration 9; bit 3: configuration 9 (and the MX-fp8 kernel of the same form) walk their tiles statically instead of drawing
 * them from the per-XCD work queue -- faster on a chip the launch has to itself; hri_emo_amd.dp clears it while collectives run
 * beside backward (a block whose CU is held late then draws fewer tiles). */
int hriemo_gemm_debug_flags(int flags);
/* Read-only: the launch plan hriemo_gemm_bf16 (and _split / _colsum) takes for this call on the current device, after every
 * fallback and with the forced configuration and flag word in force: tile configuration (0-9 as hriemo_gemm_force_config), number
 * of split-K slices (1: no workspace traffic) and the k of one slice.  workspace_bytes <= 0: no workspace.  The split-K launch
 * writes splitk * M * N floats of the workspace.  Launches nothing. */
int hriemo_gemm_plan(int ta, int tb, int M, int N, int K, int c_is_f32, long workspace_bytes, int* cfg, int* splitk,
                     int* k_per_split);

/* ---- MX-fp8 operand path (BASELINE.json configs[4], "fp8 MFMA path"): the same nn.Linear / in-projection / out-projection
 * sites as hriemo_gemm_bf16 in the FORWARD direction (models/cross_modal_block_tacfn.py:24-52, models/emotion_decoder.py:14-27),
 * with both operands as OCP e4m3 bytes + one E8M0 scale byte per 32 k-elements (OCP microscaling, block 32), multiplied on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with fp32 accumulation.  Attention cores, backward GEMMs, masters and gradients keep
 * their bf16 / fp32 formats.
 *   hriemo_quant_mx8: X[M,K] (bf16, or fp32 when src_is_f32: weight masters) -> Xq[M,K] bytes (row stride ldq) and scales
 *     S[K/32][lds] (k-block major; lds = hriemo_mx8_scale_ld(M), a multiple of 256 >= M).  Block scale = 2^ceil(log2(amax/448)):
 *     nothing saturates; elements round to nearest even.
 *   hriemo_gemm_mx8: C[M,N] = A[M,K] . B[N,K]^T (+bias) with the epilogues of hriemo_gemm_bf16; K % 128 == 0. */
long hriemo_mx8_scale_ld(int rows);
int hriemo_quant_mx8(const void* X, long ldx, int src_is_f32, int M, int K, void* Xq, long ldq, void* S, long lds,
                     hriemo_stream_t stream);
int hriemo_gemm_mx8(int M, int N, int K, const void* Aq, long lda, const void* SA, long ldsa, const void* Bq, long ldb,
                    const void* SB, long ldsb, void* C, long ldc, int c_is_f32, const float* bias, int epilogue,
                    const void* aux, long ldaux, hriemo_stream_t stream);
/* hriemo_gemm_mx8 with bf16 output (epilogue 0 / 1) whose epilogue ALSO writes the MX-fp8 form of the values it stores: bytes
 * CQ[M][ldcq] + E8M0 scales SC[N/32][ldsc] (ldsc >= M, a multiple of 256), bit-identical to hriemo_quant_mx8 of C -- the operand
 * of the next GEMM (FFN1 -> FFN2, models/cross_modal_block_tacfn.py:43-52) without a quantisation pass of its own.  N % 32 == 0. */
int hriemo_gemm_mx8_q(int M, int N, int K, const void* Aq, long lda, const void* SA, long ldsa, const void* Bq, long ldb,
                      const void* SB, long ldsb, void* C, long ldc, const float* bias, int epilogue, void* CQ, long ldcq,
                      void* SC, long ldsc, hriemo_stream_t stream);
int hriemo_gemm_mx8_force_config(int cfg);

/* ---- attention core: softmax(QK^T/sqrt(hd) + mask) -> dropout -> .V per (batch, head), flash style.
 * Q/K/V/O/dX are read/written in place inside the projection buffers: element (b, l, h, e) of X is
 * X[(b*L + l)*ldx + h*head_dim + e].  lse [B,H,Lq] (natural log) is written by fwd, read by bwd/probs;
 * delta [B,H,Lq] is bwd scratch.  Replaces the body of nn.MultiheadAttention.forward between the
 * projections (cross_modal_block_tacfn.py:74-80,85-91,98-104,111-117; emotion_decoder.py:42,48-54). */
int hriemo_attn_fwd(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                    const unsigned char* key_padding_mask, float* lse, int B, int H, int Lq, int Lk, int head_dim,
                    float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site, int b_offset,
                    void* drop_mask_bits, hriemo_stream_t stream);
int hriemo_attn_bwd(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, const void* O, long ldo,
                    const void* dO, long lddo, void* dQ, long lddq, void* dK, long lddk, void* dV, long lddv,
                    const unsigned char* key_padding_mask, const float* lse, float* delta, int B, int H, int Lq,
                    int Lk, int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev,
                    unsigned site, int b_offset, float* dq_colsum_partials, float* dkv_colsum_partials,
                    const void* drop_mask_bits, hriemo_stream_t stream);
/* drop_mask_bits (optional, hriemo_attn_mask_bytes(B,H,Lq,Lk) bytes, 8-byte aligned): the dropout keep-mask as bits, one
 * 64-bit word per (batch, head, query, 64-key tile), written by hriemo_attn_fwd when p_drop > 0 and read by hriemo_attn_bwd
 * instead of replaying the hash (NULL on either side: the hash is replayed; both give the same mask).
 * For 16 < Lk <= 128 hriemo_attn_bwd is ONE kernel (dQ, dK, dV together; HRIEMO_ATTN_FUSED_BWD=0 in the environment selects
 * the two-kernel path). */
long hriemo_attn_mask_bytes(int B, int H, int Lq, int Lk);
/* 1 when hriemo_attn_bwd runs as the single kernel for this problem (the bit words pay there; the two-kernel path is as fast
 * replaying the hash) -- what the host side asks before it requests drop_mask_bits from the forward */
int hriemo_attn_bwd_single_pass(int B, int H, int Lk, int head_dim);
/* Both lengths known: 1 if the backward of this shape is ONE kernel -- the key-resident form above (16 < L_k <= 128) or the
 * query-resident one (16 < L_q <= 128 < L_k: all queries of a (batch, head) in one block, dQ in registers, complete dK / dV tiles
 * per key tile) -- and the rows of the dK | dV column-sum partials hriemo_attn_bwd then leaves behind. */
int hriemo_attn_bwd_single_pass_q(int B, int H, int Lq, int Lk, int head_dim);
int hriemo_attn_bwd_kv_colsum_rows(int B, int H, int Lq, int Lk, int head_dim);
/* The launch plan of a shape (host code, no launch): what hriemo_attn_fwd / hriemo_attn_bwd launch for it on a device of `cus`
 * compute units (cus <= 0: this device).  fwd_rows: query rows per forward block (128 / 64 / 16); bwd_form: 0 two kernels, 1
 * key-resident single pass, 2 query-resident single pass; dq_rows / dkv_rows: rows per dQ and per dK | dV block (128 / 64 / 16;
 * form 1: dq_rows 0, dkv_rows 64 or 128 = the block's key capacity; form 2: both 0); dq_colsum_rows / kv_colsum_rows: rows of the
 * two column-sum partial buffers below.  Every query around it is one field of this plan.  Non-zero (hriemo_last_error) for an
 * empty problem or a head_dim that is not built. */
int hriemo_attn_plan(int B, int H, int Lq, int Lk, int head_dim, int cus, int* fwd_rows, int* bwd_form, int* dq_rows, int* dkv_rows,
                     int* dq_colsum_rows, int* kv_colsum_rows);
/* Packed (varlen) sequences, SURVEY 8(f) rank 4: the reference pads every sample to the batch maximum
 * (scripts/fusion/train_fusion_seq_level_decoder.py:191-232) and computes the PAD rows; here Q / O / dO / dQ hold the valid rows of
 * all samples back to back (sample b = rows cu_seqlens_q[b] .. cu_seqlens_q[b+1]-1) and K / V / dK / dV likewise with
 * cu_seqlens_k (int32 [B+1], separate arrays in device memory, every length >= 1).  max_len_q / max_len_k are upper bounds of the
 * lengths that NO sequence need reach (a captured step launches with the loader's padded length and appends its surplus rows as
 * one more sequence): they choose the kernel form (hriemo_attn_plan at the maxima), size the grid -- blocks whose tile lies past
 * their sample's end store nothing but zero column sums -- and size the side buffers, which are asked for with the maxima
 * (hriemo_attn_mask_bytes / *_colsum_rows) and keep padded slots.  With bh = b * H + h:
 *   lse, delta       element (b, h, q) at bh * max_len_q + q;
 *   drop_mask_bits   a slot of max_len_q * ceil(max_len_k / 64) words per (b, h), filled COMPACTLY with the sample's own key-tile
 *                    count: word (b, h, q, tile) at bh * max_len_q * ceil(max_len_k / 64) + q * ceil(len_k[b] / 64) + tile (the bits
 *                    inside a word as above); the rest of the slot is not written;
 *   partials         two-kernel form: row b * tiles(max_len) + tile on either side, single-pass forms: row b.
 * Rows of Q / K / V / dO past cu_seqlens[B] are never read and rows of O / dQ / dK / dV past it never written.  Same arithmetic,
 * same dropout mask (it is keyed by position within the sequence), results on the valid rows identical to the padded call with
 * a key_padding_mask (tests/test_gpu_attention_variants_packed.py holds every kernel form to all of this). */
/* hriemo_attn_fwd whose epilogue also writes the MX-fp8 form of O -- bytes Oq[B*Lq][ldoq], E8M0 scales So[H*hd/32][ldso] (ldso >=
 * B*Lq, a multiple of 256), bit-identical to hriemo_quant_mx8 of O -- for the out-projection GEMM of the fp8 mode.  head_dim % 32 == 0. */
int hriemo_attn_fwd_q(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                      const unsigned char* key_padding_mask, float* lse, int B, int H, int Lq, int Lk, int head_dim, float p_drop,
                      unsigned long long seed, const unsigned long long* seed_dev, unsigned site, int b_offset, void* drop_mask_bits,
                      void* Oq, long ldoq, void* So, long ldso, hriemo_stream_t stream);
int hriemo_attn_fwd_varlen(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                           const int* cu_seqlens_q, const int* cu_seqlens_k, float* lse, int B, int H, int max_len_q,
                           int max_len_k, int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev,
                           unsigned site, int b_offset, void* drop_mask_bits, hriemo_stream_t stream);
/* hriemo_attn_fwd_varlen whose epilogue also writes the MX-fp8 form of the packed O: bytes Oq[n_rows][ldoq], E8M0 scales
 * So[H*hd/32][ldso] with the scale byte of packed row r in column r (ldso >= n_rows, a multiple of 256), bit-identical to
 * hriemo_quant_mx8 of the packed O; O and lse are those of hriemo_attn_fwd_varlen bit for bit.  n_rows = cu_seqlens_q[B], the packed
 * row count of Q / O (the host cannot read cu_seqlens).  head_dim % 32 == 0. */
int hriemo_attn_fwd_q_varlen(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo,
                             const int* cu_seqlens_q, const int* cu_seqlens_k, float* lse, int B, int H, int max_len_q,
                             int max_len_k, int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev,
                             unsigned site, int b_offset, void* drop_mask_bits, void* Oq, long ldoq, void* So, long ldso,
                             long n_rows, hriemo_stream_t stream);
int hriemo_attn_bwd_varlen(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, const void* O, long ldo,
                           const void* dO, long lddo, void* dQ, long lddq, void* dK, long lddk, void* dV, long lddv,
                           const int* cu_seqlens_q, const int* cu_seqlens_k, const float* lse, float* delta, int B, int H,
                           int max_len_q, int max_len_k, int head_dim, float p_drop, unsigned long long seed,
                           const unsigned long long* seed_dev, unsigned site, int b_offset, float* dq_colsum_partials,
                           float* dkv_colsum_partials, const void* drop_mask_bits, hriemo_stream_t stream);
/* Optional by-product of hriemo_attn_bwd (either pointer may be NULL): per-block column sums of the dQ tiles,
 * [hriemo_attn_bwd_dq_colsum_rows(B, H, Lq, Lk, head_dim), H*head_dim] fp32, and of the dK | dV tiles,
 * [hriemo_attn_bwd_kv_colsum_rows(B, H, Lq, Lk, head_dim), 2*H*head_dim] fp32 (values before their bf16 rounding).  Summed over
 * rows (hriemo_colreduce_batch) they are the gradient of the packed in-projection bias (in_proj_bias of nn.MultiheadAttention,
 * cross_modal_block_tacfn.py:24-40) without re-reading dQ/dK/dV.  hriemo_attn_bwd_colsum_rows is the rule without L_q: it
 * names more rows than are written where the query-resident kernel leaves one row per batch. */
int hriemo_attn_bwd_colsum_rows(int B, int H, int L, int head_dim);
int hriemo_attn_bwd_dq_colsum_rows(int B, int H, int Lq, int Lk, int head_dim);
/* head-averaged attention probabilities [B,Lq,Lk] fp32 (need_weights=True; return_attention path,
 * cross_modal_block_tacfn.py:70-125, emotion_decoder.py:48-64) */
int hriemo_attn_probs(const void* Q, long ldq, const void* K, long ldk, const unsigned char* key_padding_mask,
                      const float* lse, float* probs, int B, int H, int Lq, int Lk, int head_dim, float p_drop,
                      unsigned long long seed, const unsigned long long* seed_dev, unsigned site, int b_offset,
                      hriemo_stream_t stream);
/* The export on packed (varlen) rows, on the matrix cores (v_mfma_f32_16x16x32_bf16): Q / K hold the packed rows of
 * hriemo_attn_fwd_varlen (sample b = rows cu_seqlens_q[b] .. cu_seqlens_q[b+1]-1 of Q, cu_seqlens_k likewise of K; int32 [B+1],
 * device memory, every length >= 1; own leading dimensions), lse is what that forward wrote ([B, H, max_len_q], padded indexing),
 * dropout (p_drop > 0) replays its mask (keyed by position within the sample).  probs is the PADDED map [B, out_lq, out_lk] fp32,
 * out_lq >= max_len_q, out_lk >= max_len_k (the padded lengths of the two layouts), and EVERY element of it is written, so no
 * memset precedes the call: probabilities where query and key are valid, exact 0.0 in the key columns at or past the sample's
 * key length (as hriemo_attn_probs does under a key_padding_mask) and exact 0.0 in the query rows at or past the sample's query
 * length.  That last part is the one difference to the padded export: hriemo_attn_probs computes the PAD query rows (a softmax
 * over the valid keys, which nothing reads), the packed path never has those rows.  Rows of K at or past cu_seqlens_k[B] (the
 * surplus rows of a fused bucket) are never read.  Non-zero (hriemo_last_error) for an empty problem, a head_dim that is not built,
 * unaligned operands, out_lq < max_len_q or out_lk < max_len_k, and a missing cu_seqlens pointer. */
int hriemo_attn_probs_varlen(const void* Q, long ldq, const void* K, long ldk, const int* cu_seqlens_q, const int* cu_seqlens_k,
                             const float* lse, float* probs, int B, int H, int max_len_q, int max_len_k, int out_lq, int out_lk,
                             int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site,
                             int b_offset, hriemo_stream_t stream);
/* hriemo_attn_probs on the matrix cores (v_mfma_f32_16x16x32_bf16): the same arguments and the same padded layout -- sample b owns
 * rows b*Lq .. b*Lq+Lq-1 of Q and b*Lk .. b*Lk+Lk-1 of K, lse is the [B, H, Lq] of hriemo_attn_fwd, probs the dense map
 * [B, Lq, Lk] fp32, of which EVERY element is written and nothing outside it.  key_padding_mask is uint8 [B, Lk], non-zero = PAD,
 * any pattern (not only prefixes), or NULL.  A PAD key's column is exact 0.0, chosen by a select: NaN / Inf in a PAD key's row
 * of K reach no output element.  PAD query rows are computed like any other row (the reference masks keys, not queries).  A
 * query whose lse is -inf (every key of the sample PAD) is NaN in its whole row, PAD columns and dropped elements included.
 * Dropout (p_drop > 0) replays the forward's mask, keyed by the padded indices.  Rows of K past a sample's Lk are never read, and
 * a 64-key tile whose keys are all PAD costs no fetch and no MFMA work.  The result is hriemo_attn_probs's up to fp32 summation
 * order.  Non-zero (hriemo_last_error), and nothing launched, for an empty problem or a NULL Q / K / lse / probs, a head_dim that
 * is not built, leading dimensions that are not multiples of 8, unaligned operands, p_drop outside [0, 1) and B > 65535. */
int hriemo_attn_probs_mfma(const void* Q, long ldq, const void* K, long ldk, const unsigned char* key_padding_mask,
                           const float* lse, float* probs, int B, int H, int Lq, int Lk, int head_dim, float p_drop,
                           unsigned long long seed, const unsigned long long* seed_dev, unsigned site, int b_offset,
                           hriemo_stream_t stream);

/* ---- y = LayerNorm(x + dropout(g)), eps, affine (X may be NULL: plain LayerNorm of g).
 * The residual stream has an optional fp32 twin: X32 (read instead of the bf16 X when non-NULL) and Y32
 * (written next to the bf16 Y when non-NULL).  bf16 rounding of the LayerNorm outputs is ~85 % of the
 * path's end-to-end error (scripts_dev/precision_study.py); GEMM operands stay bf16.
 * Replaces norm(h + self.dropout(sub(h))) (cross_modal_block_tacfn.py:81,92,105,106,118,119;
 * emotion_decoder.py:43,55,59).  bwd writes dX (residual branch), dG (sub-layer branch, dropout mask
 * applied) and the column sums dgamma, dbeta, dbias (= colsum dG, the producing Linear's bias grad);
 * accumulate=1 adds them into the destination (fused accumulation into existing .grad buffers). */
int hriemo_add_ln_fwd(const void* G, const void* X, const float* X32, const float* gamma, const float* beta, void* Y,
                      float* Y32, float* mean, float* rstd, int M, int d, float eps, float p_drop, unsigned long long seed,
                      const unsigned long long* seed_dev, unsigned site, long row_offset, hriemo_stream_t stream);
/* same, plus the MX-fp8 copy of Y (e4m3 bytes [M][d], E8M0 scales [d/32][ldsy], d % 32 == 0): the quantiser of hriemo_quant_mx8
 * fused into the LayerNorm that produces the next GEMM's operand (bit-identical to quantising the bf16 Y afterwards) */
int hriemo_add_ln_fwd_mx8(const void* G, const void* X, const float* X32, const float* gamma, const float* beta, void* Y,
                          float* Y32, float* mean, float* rstd, int M, int d, float eps, float p_drop, unsigned long long seed,
                          const unsigned long long* seed_dev, unsigned site, long row_offset, void* Yq, void* SY, long ldsy,
                          hriemo_stream_t stream);
/* hriemo_add_ln_fwd / _bwd for rows gathered from a larger layout (packed varlen sequences): the dropout hash is keyed by
 * row_index[row] (int64 [M], e.g. the row of the padded [B*L] layout) instead of row, so the packed launch drops exactly the
 * elements the padded one drops.  Yq / SY (MX-fp8 copy) may be NULL. */
int hriemo_add_ln_fwd_rows(const void* G, const void* X, const float* X32, const float* gamma, const float* beta, void* Y,
                           float* Y32, float* mean, float* rstd, int M, int d, float eps, float p_drop, unsigned long long seed,
                           const unsigned long long* seed_dev, unsigned site, long row_offset, void* Yq, void* SY, long ldsy,
                           const long long* row_index, hriemo_stream_t stream);
int hriemo_add_ln_bwd_rows(const void* dY, const void* G, const void* X, const float* X32, const float* gamma, const float* mean,
                           const float* rstd, void* dX, void* dG, float* dgamma, float* dbeta, float* dbias, int accumulate,
                           int M, int d, float p_drop, unsigned long long seed, const unsigned long long* seed_dev,
                           unsigned site, long row_offset, float* workspace, const long long* row_index, hriemo_stream_t stream);
/* Packed (varlen) sequences <-> padded layout, lengths read from DEVICE memory (one captured graph serves every batch whose valid
 * rows fit n_rows; replaces the reference's pad-to-the-batch-maximum, train_fusion_seq_level_decoder.py:191-232).  cu_seqlens:
 * int32 [B+1], sequence b = packed rows cu[b]..cu[b+1]-1 = its first positions of the padded [B, L, d] layout.  pack: packed rows
 * cu[B]..n_rows-1 (bucket padding) are written as zeros; row_index[r] (int64 [n_rows], may be NULL) = padded row of packed row r
 * (the row key of hriemo_add_ln_*_rows).  unpack: PAD positions are written as zeros.  X16/P16 (bf16) and X32/P32 (fp32 twin):
 * either pair may be NULL. */
int hriemo_pack_rows(const void* X16, const float* X32, const int* cu_seqlens, int B, int L, int d, int n_rows, void* P16, float* P32,
                     long long* row_index, hriemo_stream_t stream);
int hriemo_unpack_rows(const void* P16, const float* P32, const int* cu_seqlens, int B, int L, int d, void* Y16, float* Y32,
                       hriemo_stream_t stream);
/* Module inputs in one launch: the caller's tensor X (x_dtype 0 fp32, 1 bf16, 2 fp16; row stride ldx elements) -> the rows the
 * first encoder layer reads.  Destination rows r in [0, n_rows):
 *  - with cu_seqlens (int32 [B+1], device): b = the largest index with cu[b] <= r, l = r - cu[b]; the row is real when b < B (then
 *    l < cu[b+1] - cu[b]); rows from cu[B] on are the surplus of a bucket plan.  src_packed = 0: X is the padded [B, L, d] tensor,
 *    the source row is b*L + l (hriemo_pack_rows' gather).  src_packed = 1: X is already packed [cu[B], d], the source row is r.
 *  - cu_seqlens = NULL: the padded layout is kept, n_rows must equal B*L, the source row is r, row_index must be NULL.
 * Outputs, each optional, at least one given:
 *  - P32 [n_rows][d]: the exact fp32 value of the source element;  P16 [n_rows][d]: its round-to-nearest-even bf16 (a bf16 source
 *    is copied);
 *  - Pq / Ps: the MX-fp8 form of the ROUNDED bf16 values, bit-identical to hriemo_quant_mx8 of P16: e4m3 bytes [n_rows][d], E8M0
 *    scales [d/32][lds] with the scale byte of row r in column r; lds >= n_rows and a multiple of 256 (hriemo_mx8_scale_ld),
 *    d % 32 == 0; columns >= n_rows of Ps are not written;
 *  - row_index[r] (int64 [n_rows]): b*L + l, exactly what hriemo_pack_rows writes.
 * Surplus rows get zeros in P16 and P32, zero bytes in Pq and zero scale bytes in Ps.  A source row that is not real (a PAD row of
 * a padded source, a row past cu[B] of a packed one) is never read.
 * Refused (non-zero, hriemo_last_error set, nothing launched): an empty shape; d % 8 != 0; Pq without Ps (or Ps
 * without Pq) or with d % 32 != 0; lds < n_rows or lds % 256 != 0; a base pointer that is not 16-byte aligned; ldx < d or a
 * source row stride that is not a multiple of 16 bytes; an unknown x_dtype; row_index or src_packed without cu_seqlens; no
 * output at all. */
int hriemo_ingest_rows(const void* X, int x_dtype, long ldx, const int* cu_seqlens, int src_packed, int B, int L, int d, int n_rows,
                       void* P16, float* P32, void* Pq, void* Ps, long lds, long long* row_index, hriemo_stream_t stream);
/* The sequence tables of a ragged batch in one launch: the lengths (int32 [B] each, DEVICE memory) -> every table a packed step
 * reads, so the lengths are ONE piece of device data and a captured step derives the rest itself.  The kernel clamps a length to
 * [1, La] / [1, Lt] for memory safety only (the host has refused anything else).  Outputs, each optional, at least one given:
 *  - cu_a, cu_t (int32 [B+2]): [0, inclusive prefix sums of the lengths ..., n_rows_x] -- the cu_seqlens of a bucket plan whose
 *    row count is n_rows_x (hriemo_pack_rows / hriemo_ingest_rows read entries 0..B, the attention kernels all B+2);
 *  - cu_f (int32 [B+2]): the same over lf[b] = min(la[b], lt[b]) (the fused memory), last entry n_rows_t: the fused plan rides in
 *    the text bucket;
 *  - mask_a [B, La], mask_t [B, Lt], mask_f [B, Lt]: dense bytes, 1 = PAD: mask_x[b, l] = l >= length_x[b], mask_f[b, l] = l >= lf[b]
 *    (the OR of the two prefix masks cut to L_t).  Any byte alignment.
 * Every element of every given output is written, nothing outside it.
 * Refused (non-zero, hriemo_last_error set, nothing launched): B < 1, La < 1, Lt < 1 or Lt > La; a NULL lengths pointer; no output
 * at all; n_rows_a <= 0 with cu_a, n_rows_t <= 0 with cu_t or cu_f; an int32 operand that is not 4-byte aligned. */
int hriemo_seq_tables(const int* lengths_a, const int* lengths_t, int B, int La, int Lt, int n_rows_a, int n_rows_t, int* cu_a,
                      int* cu_t, int* cu_f, unsigned char* mask_a, unsigned char* mask_t, unsigned char* mask_f,
                      hriemo_stream_t stream);
/* A batch gathered from a device-resident feature store (data.DeviceFeatureStore) by utterance id, one launch per operand.
 *  - store: rows of row_bytes bytes each, every utterance's rows back to back; offsets (int64 [N+1], device): utterance u owns the
 *    rows offsets[u] .. offsets[u+1].  A store in which every utterance owns ONE row (the targets) has offsets = 0, 1, 2, ...
 *  - plan (int32 [2n+1], device): {ids[n], dst_cu[n+1]}, written by the host from its own lengths.
 *  - dst: dst_rows rows of row_bytes bytes.
 * Rows offsets[ids[i]] .. offsets[ids[i]+1] of the store go to rows dst_cu[i] .. dst_cu[i+1] of dst (ids may repeat); the rows
 * dst_cu[n] .. dst_rows of dst become zero (the tail a packed step's row sources carry); rows in front of dst_cu[0] are left as
 * they are; nothing at or behind row dst_rows is written.  The values are copied bit for bit: the kernel sees bytes, any element
 * type and any row_bytes >= 1 (10-byte rows included), any byte alignment of store and dst.  Destination chunks of 16 aligned
 * bytes are written with 16-byte stores; their source is read 16 bytes wide where source and destination agree modulo 16 and in
 * 8-, 4-, 2- or 1-byte pieces where they do not; chunks on a segment boundary go byte by byte.
 * The caller guarantees 0 <= ids[i] < N: the kernel cannot know N.  For memory safety alone dst_cu is clamped to [0, dst_rows] and
 * a segment longer than its utterance is completed with zeros instead of reading on.
 * Refused (non-zero, hriemo_last_error set, nothing launched): a null pointer; n < 1 or n > 2048; row_bytes < 1; dst_rows < 1; a
 * plan that is not 4-byte or offsets that are not 8-byte aligned. */
int hriemo_gather_rows(const void* store, long row_bytes, const long long* offsets, const int* plan, int n, void* dst, long dst_rows,
                       hriemo_stream_t stream);
/* hriemo_gather_rows with seeded train-time augmentation of the rows it moves (data.StoreAugment): same store / offsets / plan /
 * dst / zero tail / clamps, but typed: rows of row_elems elements of dtype (0 fp32, 1 bf16, 2 fp16), store and dst aligned to the
 * element.  max_rows: the host's bound on the rows of any utterance of the store (the kernel cannot read it without a round trip).
 * Everything random is the counter hash of csrc/common.h keyed by the utterance's STORE id u = ids[i], so it depends neither on the
 * batch's composition nor on the data-parallel shard; L = the utterance's rows, AUG_SITE = 0x41554700:
 *   ku = fmix32(site_key(seed, AUG_SITE + modality, draw) + u * DROP_CA), modality 1 = audio, 2 = text;
 *   modality drop: rd = fmix32(site_key(seed, AUG_SITE, draw) + u * DROP_CA) & 0xffff: all rows of the utterance are zero iff
 *     thr_lo <= rd < thr_hi (audio launch [0, thr_a), text launch [thr_a, thr_a + thr_t): never both);
 *   time spans j = 0 .. spans-1: h = fmix32(ku + (j+1) * DROP_CB), W = min(max_width, (L * frac16) >> 16),
 *     w = ((h & 0xffff) * (W+1)) >> 16, s = ((h >> 16) * (L - w + 1)) >> 16: rows [s, s+w) are zero;
 *   noise (noise_scale != 0): element (r, c) of the utterance: h = mix24(fmix32(ku + 0x27d4eb2f) + r * DROP_CA + c * DROP_CB),
 *     k = sum of the four bytes of h - 510 (mean 0, variance 21845), out = rne_dtype(x + noise_scale * k) with the product and the
 *     sum each rounded to fp32 (no FMA).  The caller passes noise_scale = sigma / sqrt(21845).
 * Noise first, then the zeros (+0.0 bits; masked rows are not read).  With noise_scale == 0 kept elements are bit copies.
 * Refused (non-zero, hriemo_last_error set, nothing launched): a null pointer; n < 1 or n > 512; a dtype code outside 0..2;
 * row_elems outside 1..65535; dst_rows < 1; max_rows >= 65536; modality outside {1, 2}; thr_lo > thr_hi or thr_hi > 65536;
 * spans outside 0..4; frac16 > 65536; a negative or non-finite noise_scale; a plan that is not 4-byte or offsets that are not
 * 8-byte aligned; store or dst not aligned to the element. */
int hriemo_gather_rows_aug(const void* store, int row_elems, int dtype, const long long* offsets, const int* plan, int n, void* dst,
                           long dst_rows, long max_rows, unsigned long long seed, unsigned draw, int modality, unsigned thr_lo,
                           unsigned thr_hi, int spans, unsigned max_width, unsigned frac16, float noise_scale,
                           hriemo_stream_t stream);
long hriemo_add_ln_bwd_workspace_bytes(int M, int d);
int hriemo_add_ln_bwd(const void* dY, const void* G, const void* X, const float* X32, const float* gamma, const float* mean,
                      const float* rstd, void* dX, void* dG, float* dgamma, float* dbeta, float* dbias, int accumulate,
                      int M, int d, float p_drop, unsigned long long seed, const unsigned long long* seed_dev,
                      unsigned site, long row_offset, float* workspace, hriemo_stream_t stream);

/* ---- small glue on the path */
long hriemo_colsum_workspace_bytes(int M, int N);
int hriemo_colsum_bf16(const void* X, long ldx, int M, int N, float* out, int accumulate, float* workspace,
                       hriemo_stream_t stream);                                   /* bias gradients */
int hriemo_cast_f32_to_bf16(const float* src, void* dst, long n, hriemo_stream_t stream);   /* bf16 shadows */
int hriemo_cast_bf16_to_f32(const void* src, float* dst, long n, hriemo_stream_t stream);
/* njobs casts in one launch (64 per launch): jobs_host = HOST array of njobs x 3 int64 {src fp32, dst bf16, n elements}, 16-byte
 * aligned pointers; the table is passed through kernel arguments (capture-safe).  The bf16 shadows of all weights of a step. */
int hriemo_cast_f32_to_bf16_batch(const void* jobs_host, int njobs, hriemo_stream_t stream);
/* the same with a kind per job: jobs_host = njobs x 4 int64 {src fp32, dst, n elements, kind}; kind 0 = fp32 -> bf16 (dst bf16),
 * 1 = fp32 -> fp32 copy.  One launch refreshes a shared projection's concatenated weight shadow and bias vector
 * (nn.MultiheadAttention.in_proj_weight / in_proj_bias slices of two modules, cross_modal_block_tacfn.py:98-117). */
int hriemo_cast_copy_batch(const void* jobs_host, int njobs, hriemo_stream_t stream);
int hriemo_dropout_bf16(const void* X, void* Y, long M, int N, float p_drop, unsigned long long seed,
                        const unsigned long long* seed_dev, unsigned site, long row_offset, hriemo_stream_t stream);                  /* emotion_decoder.py:58 */
/* emotion_decoder.py:127: out[b] = q for b < B, as bf16 and (out32 != NULL) as the fp32 twin of the residual stream */
int hriemo_expand_rows(const float* q, void* out, float* out32, int B, long n, hriemo_stream_t stream);
/* the device-resident dropout seed word of a captured step += 0x9E3779B97F4A7C15 (one launch per replay, inside the graph) */
int hriemo_seed_bump(unsigned long long* seed_dev, hriemo_stream_t stream);
int hriemo_rowdot_fwd(const void* Z, const float* Z32, const float* w, const float* b, float* out, int M, int d,
                      hriemo_stream_t stream);                                     /* emotion_decoder.py:155 */
/* dw[d], db[1]: overwritten, or added to when accumulate != 0 (gradients accumulated straight into .grad) */
int hriemo_rowdot_bwd(const float* dl, const void* Z, const float* Z32, const float* w, void* dZ, float* dw, float* db, int accumulate,
                      int M, int d, hriemo_stream_t stream);

/* ---- beta gate (models/beta_gate_tacfn.py:68-118): LayerNorm + masked mean-pool (:6-24,79-84),
 * gate input [a,t,|a-t|,a*t] (:87-89), w = sigmoid(MLP), beta = mean(w) (:92-95), fuse over the first
 * L positions (:98-116).  partials buffers are [B, hriemo_pool_chunks(L), d] fp32. */
int hriemo_pool_chunks(int L);
int hriemo_ln_pool_fwd(const void* X, const float* X32, const unsigned char* mask, const float* gamma, const float* beta, void* Yn,
                       float* mean, float* rstd, float* partials, int B, int L, int Lkeep, int d, float eps,
                       hriemo_stream_t stream);
int hriemo_gate_input(const float* partials_a, const float* partials_t, const unsigned char* mask_a,
                      const unsigned char* mask_t, int B, int La, int Lt, int d, void* gate_in, float* a_pool,
                      float* t_pool, float* cnt, hriemo_stream_t stream);
int hriemo_sigmoid_beta(const float* pre, float* w, float* beta, int B, int d, hriemo_stream_t stream);
int hriemo_fuse_fwd(const float* w, const void* A, const void* T, void* H, int B, int L, int d, hriemo_stream_t stream);
int hriemo_fuse_bwd_dw(const void* dH, const void* A, const void* T, float* partials, int B, int L, int d,
                       hriemo_stream_t stream);
int hriemo_gate_dpre(const float* partials, int L, const float* dbeta, const float* w, void* dpre, int B, int d,
                     hriemo_stream_t stream);
int hriemo_gate_input_bwd(const void* dgin, const float* a_pool, const float* t_pool, const float* cnt, float* da,
                          float* dt, int B, int d, hriemo_stream_t stream);
/* Legacy scalar gate, models/beta_gate.py:6-32,60-114 (what the reference's tests/test_beta_gate.py exercises):
 * masked mean pooling of the raw [B,L,d] features (pooled[B,d], cnt[B] = max(#valid,1)); the [B,4d]->h->1 MLP and
 * its sigmoid are [B]-sized host-side plumbing; h_fusion = beta*h_a[:, :L] + (1-beta)*h_t[:, :L] reuses
 * hriemo_fuse_fwd with beta broadcast over d, hriemo_fuse_bwd_dw + hriemo_rowsum_f32 give dbeta, and
 * hriemo_scalar_gate_dx writes dX = coef*dH (first Lf rows) + valid*dpool/cnt in one pass. */
int hriemo_masked_mean_fwd(const void* X, const unsigned char* mask, float* pooled, float* cnt, int B, int L, int d,
                           hriemo_stream_t stream);
int hriemo_rowsum_f32(const float* x, float* out, int B, long n, hriemo_stream_t stream);
/* gate input [a, t, |a-t|, a*t] (bf16 [B,4d]) from already pooled means: the legacy gate's MLP then runs on hriemo_gemm_bf16 +
 * hriemo_rowdot_* like the vector gate's (models/beta_gate.py:82-93) */
int hriemo_gate_input_pooled(const float* a_pool, const float* t_pool, void* gate_in, int B, int d, hriemo_stream_t stream);
/* Trainer losses, value and gradients in one launch ([B,N_e]-sized): mean BCEWithLogits(logits, targets; pos_weight (may be NULL))
 * + reg(beta) (reg_mode 0 none; 1: -coef*mean(beta(1-beta)), scripts/fusion/train_fusion_seq_level_decoder.py:318-326; 2: +coef*mean
 * binary entropy of clamp(beta,1e-8,1-1e-8), train_mosei_fusion_seq_level_decoder.py:340-347,385-386,569), everything times `scale`
 * (1/grad_accum).  Writes loss[1], dlogits[B,N_e], dbeta[B] (dbeta may be NULL). */
int hriemo_fusion_loss(const float* logits, const float* targets, const float* pos_weight, const float* beta, int B, int Ne,
                       int reg_mode, float reg_coef, float scale, float* loss, float* dlogits, float* dbeta, hriemo_stream_t stream);
/* Single-label variant, torch.nn.CrossEntropyLoss() as scripts/fusion/train_fusion_seq_level_decoder.py:413-414 builds it (mean
 * over the labelled samples, no class weights, no label smoothing, ignore_index = -100), plus the same beta regulariser (:325-326,
 * a mean over all B): labels[B] are int64 class indices in [0, C), or -100 for a sample the criterion skips (no loss term, zero
 * gradient, not counted in the mean; all of them skipped: NaN, as torch); any other index outside [0, C) poisons the loss with NaN
 * instead of reading out of bounds.  Writes loss[1], dlogits[B,C] = (softmax - onehot)/n_labelled * scale, dbeta[B] (may be NULL). */
int hriemo_fusion_loss_ce(const float* logits, const long long* labels, const float* beta, int B, int C, int reg_mode,
                          float reg_coef, float scale, float* loss, float* dlogits, float* dbeta, hriemo_stream_t stream);
/* The two losses with the number of samples that count in DEVICE memory (a captured step that serves the short last batch of an
 * epoch, DataParallelStep.capture_packed(partial_batches=True)): nv = clamp(*n_valid, 1, B) on the device.  Samples b >= nv are
 * ghosts: their rows of logits, targets / labels and beta are never read (they may hold NaN), they add no loss term, and every
 * element of their dlogits row and their dbeta is stored as +0.  The BCE mean runs over nv * N_e, the CE mean over the labelled
 * samples among the first nv, the regulariser mean over nv.  *n_valid == B: bit-identical to the entries above. */
int hriemo_fusion_loss_n(const float* logits, const float* targets, const float* pos_weight, const float* beta, int B, int Ne,
                         int reg_mode, float reg_coef, float scale, float* loss, float* dlogits, float* dbeta, const int* n_valid,
                         hriemo_stream_t stream);
int hriemo_fusion_loss_ce_n(const float* logits, const long long* labels, const float* beta, int B, int C, int reg_mode,
                            float reg_coef, float scale, float* loss, float* dlogits, float* dbeta, const int* n_valid,
                            hriemo_stream_t stream);
/* Epoch statistics in device memory (csrc/metrics.hip): what the reference's trainers report per epoch
 * (scripts/fusion/train_fusion_seq_level_decoder.py:300-372: mean loss, accuracy, mean beta;
 * train_mosei_fusion_seq_level_decoder.py:119-171,367-495: mean loss with non-finite batches skipped, micro / macro F1, macro AUC,
 * the 19-threshold calibration sweep) without a read-back per step.  State of one epoch, owned by the caller, zeroed to reset:
 *   probs   fp32  [C, capacity]   class-major log of p = 1 / (1 + expf(-logit))
 *   truth   uint8 [C, capacity]   [target > 0]
 *   counters int32[8]  {cursor, n_samples, n_batches, n_skipped, n_correct, n_nonfinite, overflow, spare}
 *   sums    float64[4] {sum_loss, sum_beta, n_beta, spare}
 * hriemo_stats_update: ONE block, meant to be recorded right behind the loss launch of a (captured) step -- every input is a device
 * pointer; launches are stream-ordered, so the block owns the cursor and nothing is atomic.  Exactly one of targets (float [B, C],
 * multi-label) and labels (int64 [B], single-label; nothing is logged, probs / truth may be NULL) is given.  loss: the scalar the
 * loss kernel wrote; loss_scale by value (grad_accum, to undo the 1/k of hriemo_fusion_loss's scale: the reference logs the raw
 * loss).  beta: NULL or B * beta_per_sample values.  n_valid: NULL or one aligned int32, nv = clamp(*n_valid, 1, B) as in
 * hriemo_fusion_loss_n; rows b >= nv are never read.  skip_nonfinite != 0 and a NaN / Inf loss: n_skipped += 1 and nothing else.
 * Otherwise, over the first nv samples: the log is appended at the cursor (multi-label), sum_loss += loss * loss_scale * nv,
 * sum_beta / n_beta, n_correct (multi-label: every label of the sample has [p > 0.5] == [target > 0]; single-label: the first
 * maximal logit's index equals the label, as torch.argmax), n_samples += nv, n_batches += 1, n_nonfinite += the non-finite logits
 * that were logged.  cursor + nv > capacity: overflow = 1 and nothing is appended; the sums and counters are still updated.
 * hriemo_stats_counts: out int32 [C, S, 3] = {tp, fp, fn} of the prediction p >= thresholds[s] (fp32 [S], S <= 64) over the first
 * `cursor` log entries; the entry zeroes out first.  The reference compares fp32 p with float64 thresholds: hand in every
 * threshold rounded UP to fp32 and the decisions are the same.
 * hriemo_stats_auc: per class, 2U = sum over (positive i, negative j) of 2 [p_i > p_j] + [p_i == p_j], as partial sums
 * partial uint64 [C, hriemo_stats_auc_tiles(capacity)] (256 rows i per tile; every tile is stored, tiles past the cursor as 0;
 * the caller adds them), and npn int32 [C, 2] = {n_pos, n_neg}.  AUC = 2U / (2 n_pos n_neg), formed on the host.
 * hriemo_stats_rank: the ranking metrics of the reference's reporting layer (tools/mosei_export_per_class_metrics.py:10-17,
 * scripts/infer/mosei_plot_metrics.py:44-80,130-148: average precision, precision-recall and ROC curves) as integers.  With
 * n = clamp(cursor, 0, capacity), rank int32 [C, 2, capacity]: for i < n, rank[c, 0, i] = the number of j < n with truth[c, j] != 0
 * and probs[c, j] >= probs[c, i], rank[c, 1, i] the same over truth[c, j] == 0; entry i counts itself in the plane of its own kind.
 * Elements n <= i < capacity of both planes are stored as 0: every element of rank is written by every call.  Log entries at or
 * past the cursor are never read (they may hold NaN); a NaN probs[c, i] compares false with everything and gets 0 / 0.  No sort, no
 * floating-point sum and no atomics on the device; the host forms precision = ge_pos / (ge_pos + ge_neg), recall = ge_pos / n_pos,
 * fpr = ge_neg / n_neg at every distinct probability, and average precision = sum over the positives of their precision / n_pos.
 * Refused (non-zero, nothing launched): capacity < 1, C < 1 or C > 65535 (the grid's second dimension), a NULL pointer, probs /
 * counters / rank not 4-byte aligned.
 * hriemo_stats_confusion: ONE block of 256, meant to be recorded directly behind hriemo_stats_update of the same single-label step
 * (stream order makes it the only writer of cm).  cm int32 [C * C + 2], owned by the caller, zeroed to reset: the confusion matrix
 * (row = label, column = prediction), then {n_ignored, n_bad}.  nv = clamp(*n_valid, 1, B) (NULL: B); rows b >= nv are never read.
 * skip_nonfinite != 0 and a NaN / Inf loss[0]: cm is left untouched (the batch hriemo_stats_update only counts in n_skipped).
 * Otherwise, for each of the first nv samples, pred = the first maximal logit's index (a NaN counts as maximal: the rule of
 * hriemo_stats_update) and cm[label * C + pred] += 1 for 0 <= label < C; label == -100 (the criterion's ignore_index): cm[C * C]
 * += 1; any other label: cm[C * C + 1] += 1, and nothing is indexed with it.  Refused (non-zero, nothing launched): B < 1, C < 1
 * or C > 64, NULL logits / labels / loss / cm, n_valid / cm not 4-byte aligned. */
int hriemo_stats_update(const float* logits, const float* targets, const long long* labels, const float* loss, float loss_scale,
                        const float* beta, int beta_per_sample, const int* n_valid, int B, int C, int skip_nonfinite,
                        float* probs, unsigned char* truth, int capacity, int* counters, double* sums, hriemo_stream_t stream);
int hriemo_stats_counts(const float* probs, const unsigned char* truth, int capacity, int C, const int* counters,
                        const float* thresholds, int S, int* out, hriemo_stream_t stream);
int hriemo_stats_auc_tiles(int capacity);
int hriemo_stats_auc(const float* probs, const unsigned char* truth, int capacity, int C, const int* counters,
                     unsigned long long* partial, int* npn, hriemo_stream_t stream);
int hriemo_stats_rank(const float* probs, const unsigned char* truth, int capacity, int C, const int* counters, int* rank,
                      hriemo_stream_t stream);
int hriemo_stats_confusion(const float* logits, const long long* labels, const float* loss, int skip_nonfinite, const int* n_valid,
                           int B, int C, int* cm, hriemo_stream_t stream);
/* Prediction log in device memory (csrc/metrics.hip): the products of the reference's inference driver
 * (scripts/infer/mosei_eval_infer.py: {split}_y_prob.npy, {split}_beta_mean.npy) without targets and without a read-back per batch.
 * State, owned by the caller, counters zeroed to reset:
 *   probs     fp32  [C, capacity]  class-major, as the statistics' log
 *   beta_mean fp32  [capacity]     (optional)
 *   pred      int32 [capacity]     (optional, single-label only)
 *   counters  int32 [4]            {cursor, n_samples, overflow, n_nonfinite}
 * hriemo_predict_log: ONE block of 256, meant to be recorded behind the forward of a (captured) step -- every input is a device
 * pointer; launches are stream-ordered, so the block owns the cursor and nothing is atomic.  nv = clamp(*n_valid, 1, B) (NULL: B)
 * as in hriemo_fusion_loss_n; rows b >= nv of logits and beta are never read.  kind 0 (multi-label): probs[c, cursor + b] =
 * 1 / (1 + expf(-logit)), the expression of hriemo_stats_update: equal logits give equal bits in both logs.  kind 1
 * (single-label): the fp32 softmax over C with the row maximum subtracted (the difference carried with its rounding error, the
 * sum over the classes in index order), and pred[cursor + b] = the first maximal logit's index (torch.argmax's rule; pred may
 * be NULL).  beta: NULL or B * beta_per_sample values; beta_mean[cursor + b] = the mean of the
 * sample's values, summed in index order in float64, stored as fp32 (beta_mean may be NULL).  cursor + nv > capacity: overflow = 1
 * and nothing is appended; n_samples still counts.  Otherwise the cursor moves by nv and n_nonfinite gains the number of non-finite
 * logits logged.  Refused (non-zero, nothing launched): B, C or capacity < 1, kind outside {0, 1}, NULL logits / probs / counters,
 * beta with beta_per_sample < 1, n_valid / counters / pred not 4-byte aligned. */
int hriemo_predict_log(const float* logits, const float* beta, int beta_per_sample, const int* n_valid, int B, int C, int kind,
                       float* probs, float* beta_mean, int* pred, int capacity, int* counters, hriemo_stream_t stream);
/* Attention log in device memory (csrc/metrics.hip, csrc/attention.hip, csrc/fp32mode.hip): the --dump_attn --attn_max_samples K
 * product of the same driver -- the attention maps of the FIRST `capacity` samples of a split -- from a captured evaluation whose
 * launch list is fixed.  State, owned by the caller, counters zeroed to reset:
 *   one fp32 [capacity, Lq, Lk] tensor per attention site (the log of that site)
 *   lengths   int32 [2, capacity]  audio row, text row: the lengths of the logged samples (optional)
 *   counters  int32 [4]            {cursor, n_offered, n_batches, spare}
 *   window    int32 [4]            {slot0, n_take, 0, 0}: samples 0 .. n_take-1 of the current pass go to slots slot0 ..
 * hriemo_attn_log_plan: ONE block, recorded once per pass in front of every export launch (in a captured step: directly behind
 * hriemo_seq_tables, in front of every fork).  nv = clamp(*n_valid, 1, B) (NULL: B) as in hriemo_fusion_loss_n.  slot0 = cursor,
 * n_take = clamp(capacity - cursor, 0, nv), lengths[:, slot0 + b] = lens[:, b] for b < n_take (lens: the pass's int32 [2, B]
 * lengths block; lens and lengths are both given or both NULL), cursor += n_take, n_offered += nv, n_batches += 1.  A cursor
 * outside [0, capacity] counts as full: n_take = 0 and only n_offered, n_batches and the window are written.  A full log is the
 * normal end state, not an overflow.
 * hriemo_attn_log_close: writes the window {0, 0, 0, 0} and touches nothing else -- the plan of a pass that must leave no trace
 * (the warm-up passes of a capture): every export launch behind it exits.
 * hriemo_attn_probs_varlen_log / hriemo_attn_probs_varlen_log_fp32: hriemo_attn_probs_varlen and hriemo_attn_probs_f32_varlen (same kernels, same
 * arguments, same values) with probs = the site's log [capacity, out_lq, out_lk] and the window: the blocks of sample b return
 * before their first barrier when b >= n_take, slot0 < 0 or slot0 + b >= capacity; otherwise the sample's map goes to slot
 * slot0 + b, every element of the slot written.  capacity travels by value, so a stale window cannot send a store past the log.
 * hriemo_attn_log_append: the same window rule as a copy of maps fp32 [B, map_elems] into log [capacity, map_elems], for a site
 * whose map a padded export produced.
 * Refused (non-zero, nothing launched): B or capacity < 1, map_elems < 1, a NULL or misaligned counters / window / log / maps
 * pointer, lens without lengths or the reverse, and everything the two varlen exports refuse. */
int hriemo_attn_log_plan(const int* lens, const int* n_valid, int B, int capacity, int* counters, int* window, int* lengths,
                         hriemo_stream_t stream);
int hriemo_attn_log_close(int* window, hriemo_stream_t stream);
int hriemo_attn_log_append(const float* maps, int B, int map_elems, const int* window, float* log, int capacity,
                           hriemo_stream_t stream);
int hriemo_attn_probs_varlen_log(const void* Q, long ldq, const void* K, long ldk, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                 const float* lse, float* probs, int B, int H, int max_len_q, int max_len_k, int out_lq, int out_lk,
                                 int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site,
                                 int b_offset, const int* window, int capacity, hriemo_stream_t stream);
int hriemo_attn_probs_varlen_log_fp32(const float* Q, long ldq, const float* K, long ldk, const int* cu_seqlens_q,
                                     const int* cu_seqlens_k, const float* lse, float* probs, int B, int H, int max_len_q, int max_len_k,
                                     int out_lq, int out_lk, int head_dim, float p_drop, unsigned long long seed,
                                     const unsigned long long* seed_dev, unsigned site, int b_offset, const int* window, int capacity,
                                     hriemo_stream_t stream);
int hriemo_scalar_gate_dx(const void* dH, int Lf, const float* beta, int is_a, const float* dpool, const float* cnt,
                          const unsigned char* mask, void* dX, int B, int L, int d, hriemo_stream_t stream);
/* Trainer step off the timed path, scripts/fusion/train_fusion_seq_level_decoder.py:332-334: clip_grad_norm_(5.0) +
 * AdamW(lr 1e-4, weight_decay 1e-2) as two passes over flat fp32 buffers that share one layout (parameters,
 * gradients, first and second moments; hri-emo_amd/optim.py lays them out): hriemo_sumsq_f32 writes nblocks partial
 * sums of squares (reduce them with hriemo_rowsum_f32), hriemo_adamw_flat reads the squared norm from device memory
 * (coef = min(1, max_norm/(norm+1e-6)); max_norm <= 0: no clipping) and applies torch.optim.AdamW's update. */
int hriemo_sumsq_f32(const float* x, long n, float* partial, int nblocks, hriemo_stream_t stream);
int hriemo_adamw_flat(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, float max_norm, const float* norm2, hriemo_stream_t stream);
/* The same trainer step with EVERY scalar in device memory (hri-emo_amd/optim.py: DeviceAdamW), so the update can be recorded
 * into the hipGraph of the step and still follow torch's LambdaLR, GradScaler and the NaN / Inf batch guard of
 * scripts/fusion/train_mosei_fusion_seq_level_decoder.py:367-402,564-584 without a host read:
 *   hyper[8] (host-written fp32):   lr, beta1, beta2, eps, weight_decay, max_norm (<= 0: no clipping), two spare words;
 *   state[8] (device-written fp32): step, skip, coef, step_size = lr/bc1, 1/sqrt(bc2), decay = 1 - lr*wd, grad_norm (pre-clip,
 *                                   unscaled), skipped (count of skipped steps); bcN = 1 - betaN^step.
 * hriemo_optim_finalize (one block) sums the nblocks partials of hriemo_sumsq_f32 in a fixed order, norm = sqrt(sum)/grad_scale,
 * skip = (found_inf != 0) || !isfinite(norm); a step that is not skipped increments `step` and writes
 * coef = min(1, max_norm/(norm+1e-6))/grad_scale and the bias-correction terms of the new step; a skipped one increments `skipped`
 * only.  grad_scale / found_inf (one fp32 each, torch.amp.GradScaler's device tensors) may be NULL: scale 1, nothing found.
 * hriemo_adamw_flat_dev is hriemo_adamw_flat's arithmetic with its scalars read from hyper / state; a skipped step leaves p, m, v
 * untouched. */
int hriemo_optim_finalize(const float* partial, int nblocks, const float* hyper, const float* grad_scale, const float* found_inf,
                          float* state, hriemo_stream_t stream);
int hriemo_adamw_flat_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, const float* state,
                          hriemo_stream_t stream);
/* Gradient accumulation inside a captured step (DataParallelStep.capture_packed(grad_accum=k)).  ctl is the step-control block,
 * int32[4] in device memory, written by the host before every replay: {n_valid, first, last, spare}.
 * hriemo_grad_begin opens a micro-step: ctl[1] (first) != 0 writes +0 over flat[0, n) (n % 4 == 0, flat 16-byte aligned);
 * first == 0 leaves every bit of flat in place (nothing is loaded or stored: NaN payloads and -0 survive).
 * hriemo_optim_finalize_ctl is hriemo_optim_finalize for the micro-step with ctl[2] (last) != 0, bit for bit; with last == 0 it
 * HOLDS the update: state[1] (skip) = 1 so that hriemo_adamw_flat_dev returns early, and no other word of state changes -- step,
 * skipped and grad_norm stay as they were. */
int hriemo_grad_begin(float* flat, long n, const int* ctl, hriemo_stream_t stream);
int hriemo_optim_finalize_ctl(const float* partial, int nblocks, const float* hyper, const float* grad_scale, const float* found_inf,
                              float* state, const int* ctl, hriemo_stream_t stream);
/* Parameter groups (DeviceAdamW(param_groups=...)): the same step with per-group lr, betas, eps and weight decay, still three
 * launches (hriemo_sumsq_f32 -> hriemo_optim_finalize_groups -> hriemo_adamw_flat_groups).  Layout, 1 <= G <= 16 groups:
 *   hyper[G][8] (host-written fp32):   row g = {lr, beta1, beta2, eps, weight_decay, max_norm, 2 spare words} of group g;
 *                                      max_norm is GLOBAL and read from row 0 only (one clip over the whole flat buffer, as
 *                                      clip_grad_norm_(model.parameters()) gives);
 *   state[G][8] (device-written fp32): row 0 = the state[8] above, word for word: step, skip, coef, step_size, 1/sqrt(bc2), decay
 *                                      (those three of group 0), grad_norm, skipped -- one norm, one skip decision, one step count
 *                                      and one `skipped` counter serve all groups;
 *                                      row g >= 1: words 3, 4, 5 = step_size = lr_g/bc1_g, 1/sqrt(bc2_g), decay_g = 1 - lr_g*wd_g
 *                                      from group g's own lr, betas and weight decay; its other five words are never written;
 *   seg   int64 [S+1] (device):        ascending element offsets into the flat buffer, seg[0] = 0, seg[S] = n, every entry a
 *                                      multiple of 4; 1 <= S <= 2048;
 *   seg_group int32 [S] (device):      the group in [0, G) that owns elements seg[s] .. seg[s+1]-1; a group may own several
 *                                      segments, adjacent or not.
 * hriemo_optim_finalize_groups is hriemo_optim_finalize for G groups; with G = 1 all 8 words of state are those of
 * hriemo_optim_finalize bit for bit.  ctl may be NULL; otherwise it is the step-control block and the launch HOLDS the update as
 * hriemo_optim_finalize_ctl does (ctl[2] == 0: state[0][1] (skip) = 1 and no other word of any row changes).
 * hriemo_adamw_flat_groups is hriemo_adamw_flat_dev with the scalars of the group that owns each 16-byte vector, in ONE launch over
 * the flat buffer: the per-element arithmetic is the same inline function, so on a group's elements the result equals
 * hriemo_adamw_flat_dev run with that group's hyper row, bit for bit.  Each block copies the tables into LDS ((S+1)*8 + G*32 + S
 * bytes) and every thread keeps its current segment in registers.  The tables only select scalars and address nothing: a lookup
 * that falls outside them is clamped to the last segment, a group outside [0, G) to the nearest valid one, so hyper and state are
 * never indexed out of range, and nothing at or beyond element n is written whatever seg holds.  A skipped or held step
 * (state[0][1] != 0) leaves p, m, v untouched.
 * Refused (non-zero, hriemo_last_error set, nothing launched): G outside 1..16, S outside 1..2048, n <= 0 or n % 4 != 0, a NULL
 * p / g / m / v / hyper / state / seg / seg_group, buffers that are not 16-byte aligned, seg not 8-byte or seg_group / ctl not
 * 4-byte aligned. */
int hriemo_optim_finalize_groups(const float* partial, int nblocks, const float* hyper, int G, const float* grad_scale,
                                 const float* found_inf, float* state, const int* ctl, hriemo_stream_t stream);
int hriemo_adamw_flat_groups(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group, int S,
                             const float* hyper, const float* state, int G, hriemo_stream_t stream);
/* Weight averaging inside the step (DeviceAdamW(averaging="ema" | "swa")): torch.optim.swa_utils.AveragedModel's running average
 * as one more flat fp32 buffer `avg`, laid out like p, updated by the update kernel itself.  Two blocks beside hyper / state:
 *   avg_hyper[4] (host-written fp32):   mode (0 off, 1 ema, 2 swa), decay, start, every (whole numbers below 2^24);
 *   avg_state[4] (device-written fp32): n_averaged, w, flag (0 none, 1 averaging update, 2 first averaging update), stamp.
 * hriemo_optim_finalize_avg is hriemo_optim_finalize_groups (G = 1 and ctl == NULL: hriemo_optim_finalize; G = 1 with ctl:
 * hriemo_optim_finalize_ctl -- state comes out bit for bit) that also writes avg_state.  With t the step count a real update
 * (neither skipped nor held) has just written: the update averages iff t > start and (t - start) % every == 0; then
 * w = 1 - decay (ema) or 1 / (n_averaged + 1) (swa), in fp32, flag = 2 if n_averaged was 0 and 1 otherwise, n_averaged += 1,
 * stamp = t.  A real update that does not average writes flag = 0 and stamp = t and leaves n_averaged and w alone.  A skipped or
 * held step writes no word of avg_state.
 * hriemo_adamw_flat_dev_avg / hriemo_adamw_flat_groups_avg are hriemo_adamw_flat_dev / hriemo_adamw_flat_groups -- p, m, v bit
 * for bit -- that fold each freshly written 16-byte vector of p into avg when flag != 0 AND stamp == state[0] (a flag left by
 * another step is no update): flag 2 stores the bits of p, flag 1 stores fmaf(w, p - avg, avg).  On every other step, skipped and
 * held ones included, avg is neither loaded nor stored.  Nothing at or beyond element n is written.
 * Refused besides what the plain entries refuse: NULL avg_hyper / avg_state / avg, avg not 16-byte aligned, avg overlapping p, g,
 * m or v.
 * hriemo_swap_fp32 exchanges a[0, n) and b[0, n) bit for bit (16-byte vectors; NaN payloads, -0 and denormals cross unchanged).
 * Refused: n <= 0 or n % 4 != 0, NULL or unaligned buffers, buffers that overlap or are one buffer. */
int hriemo_optim_finalize_avg(const float* partial, int nblocks, const float* hyper, int G, const float* grad_scale,
                              const float* found_inf, float* state, const int* ctl, const float* avg_hyper, float* avg_state,
                              hriemo_stream_t stream);
int hriemo_adamw_flat_dev_avg(float* p, const float* g, float* m, float* v, long n, const float* hyper, const float* state, float* avg,
                              const float* avg_state, hriemo_stream_t stream);
int hriemo_adamw_flat_groups_avg(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group, int S,
                                 const float* hyper, const float* state, int G, float* avg, const float* avg_state,
                                 hriemo_stream_t stream);
int hriemo_swap_fp32(float* a, float* b, long n, hriemo_stream_t stream);
/* Per-group and per-parameter gradient clipping (DeviceAdamW(clip="group" | "parameter")): every CLIP UNIT -- a param group, or one
 * parameter tensor -- is clipped by its own norm against its group's max_norm, hyper[g][5] of EVERY row (<= 0: that group's units
 * are not clipped).  Still three launches: hriemo_sumsq_units -> hriemo_optim_finalize_units -> hriemo_adamw_flat_units(_avg).
 *   chunks int64 [C][4] (host-written, once): {start, length, unit, group} -- the segments cut into pieces of at most 32768 elements
 *                       (start a multiple of 64 elements, length a multiple of 64), rows ordered by unit, then by start; the
 *                       kernels read start and length only.  1 <= C <= 2^20.
 *   unit_chunks int32 [U+1]:   unit u owns the rows unit_chunks[u] .. unit_chunks[u+1]-1; unit_chunks[0] = 0, unit_chunks[U] = C.
 *   unit_group int32 [U]:      the group in [0, G) whose max_norm clips unit u.  1 <= U <= 2048.
 *   seg_unit int32 [S]:        the unit in [0, U) of segment s, beside seg / seg_group of the grouped update.
 *   clip_state fp32 [U][2] (device-written): norm_u = sqrt(sum of g^2 over the unit) / grad_scale and
 *                       coef_u = (max_norm_g > 0 ? min(1, max_norm_g / (norm_u + 1e-6)) : 1) / grad_scale.
 * hriemo_sumsq_units: one block of 256 threads per chunk, partial[c] = the chunk's sum of squares in one fixed order (16-byte loads;
 * per thread fmaf over its vectors in ascending order, the xor butterfly over the wave, the four wave sums in index order; no
 * atomics).  Nothing is masked: a NaN / Inf element makes its chunk's partial NaN / Inf.  Rows are clamped into [0, n) before use.
 * hriemo_optim_finalize_units is hriemo_optim_finalize_groups (ctl may be NULL; HOLD as there) and, with avg_hyper / avg_state given
 * (both or neither), hriemo_optim_finalize_avg: one entry for every form.  It adds each unit's partials in ONE order that depends on
 * the tables alone (lane l of a wave adds the unit's partials l, l + 64, ... ascending, then the xor butterfly), forms the global
 * sum as the fixed-order sum of the unit sums, and decides the skip from it as before (any non-finite unit makes it non-finite).
 * A real update writes both columns of clip_state and state[0][2] (coef) = the SMALLEST unit coefficient; a skipped step writes the
 * norms only (which unit was not finite can be read without a health log); a held step writes no word of clip_state.  Everything
 * else of state[G][8] is as hriemo_optim_finalize_groups leaves it.
 * hriemo_adamw_flat_units / _avg are hriemo_adamw_flat_groups / _avg whose every 16-byte vector takes coef from clip_state of its
 * segment's unit instead of state[0][2]: the same inline arithmetic, so a unit's elements equal hriemo_adamw_flat_dev run with the
 * group's hyper row and a state block whose coef is coef_u, bit for bit.  LDS grows by 4 U + 2 S bytes.  seg_unit only selects a
 * scalar and is clamped to [0, U).
 * Refused besides what the grouped entries refuse: U outside 1..2048 (or U > S, U > C), C outside 1..2^20 or more chunks /
 * segments than 16-byte vectors in n, NULL or misaligned chunks / unit_chunks / unit_group / seg_unit / clip_state / partial,
 * partial or clip_state overlapping the buffers read beside them, one of avg_hyper / avg_state without the other. */
int hriemo_sumsq_units(const float* g, long n, const long long* chunks, int C, float* partial, hriemo_stream_t stream);
int hriemo_optim_finalize_units(const float* partial, int C, const int* unit_chunks, const int* unit_group, int U, const float* hyper,
                                int G, const float* grad_scale, const float* found_inf, float* state, const int* ctl, float* clip_state,
                                const float* avg_hyper, float* avg_state, hriemo_stream_t stream);
int hriemo_adamw_flat_units(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group,
                            const int* seg_unit, int S, const float* hyper, const float* state, int G, const float* clip_state, int U,
                            hriemo_stream_t stream);
int hriemo_adamw_flat_units_avg(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group,
                                const int* seg_unit, int S, const float* hyper, const float* state, int G, const float* clip_state, int U,
                                float* avg, const float* avg_state, hriemo_stream_t stream);
/* The health log of the device-state optimizer (DeviceAdamW(health=HealthLog(capacity, every))): per-parameter statistics of a
 * step, written by two launches BEHIND the update kernel into a ring in device memory.  They only read g, p, m, v, hyper, state
 * and ctl; no existing launch changes.
 *   chunks int64 [C][4] (host-written, once): {start, length, parameter, group} -- the parameters' slots of the flat buffers (start a
 *                       multiple of 64 elements, length padded to 64, zeros in the padding of g, p, m, v) cut into pieces of at most
 *                       `chunk` elements, in flat-buffer order: the chunks of one parameter are neighbours and ascend.
 *                       1 <= C <= 2^20; parameter in [0, P), group in [0, G).
 *   partial fp32 [C][4] (device-written):     {grad_sq, nonfinite (the bits of an int32), weight_sq, update_sq} of chunk c.
 *   log int32 [4 + capacity * (4 + 4 P)]:     word 0 = n_recorded, the records ever written (words 1..3 spare); record r lives in
 *                       slot r % capacity: {step (fp32 bits), kind, grad_norm (fp32 bits), spare}, grad_sq[P] (fp32 bits),
 *                       nonfinite[P] (int32), weight_sq[P], update_sq[P] (fp32 bits).  1 <= P <= 4096, 1 <= capacity <= 2^20.
 * Both kernels take the same block-uniform decision from state, ctl and every, in front of any barrier:
 *   ctl != NULL and ctl[2] (last) == 0: a held micro-step records NOTHING -- every block returns with nothing loaded or stored;
 *   state[1] (skip) != 0: ALWAYS a record, kind 1 if state[6] (grad_norm) is not finite, else kind 2 (found_inf alone); only g is
 *                       read, weight_sq and update_sq are zeros;
 *   otherwise (a real update, t = state[0]): a record of kind 0 iff t % every == 0; g, p, m and v are read.
 * hriemo_health_sweep: one block of 256 threads per chunk.  grad_sq = sum of g^2 over the FINITE elements of the chunk (as the
 * buffer holds them: still scaled by grad_scale), nonfinite = the number of NaN / +-Inf elements (exact), weight_sq = sum of p^2,
 * update_sq = sum of (step_size * m / (sqrt(v) * isb2 + eps))^2 with step_size = state[group][3], isb2 = state[group][4],
 * eps = hyper[group][3]: the Adam term the update kernel has just subtracted, from the moments it has just written.  Fixed-order
 * sums: per thread over its vectors tid, tid + 256, ... element by element, the wave's xor butterfly, the four wave sums in index
 * order; no floating-point atomics.  A row of the table is clamped before use (start into [0, n] and down to a multiple of 4, the
 * length into [0, n - start] likewise, the group into [0, G)): a table that breaks its contract cannot make a buffer be read out of
 * range.  The only store is partial[c].
 * hriemo_health_fold: one block.  Adds the partials of every parameter in chunk order (the chunk range of a parameter is rebuilt
 * from the table's parameter column, indices clamped to [0, P)), multiplies grad_sq by 1 / grad_scale^2 (grad_scale may be NULL:
 * 1), writes the record into slot n_recorded % capacity and then n_recorded + 1: it is the only writer of the counter.  Nothing at
 * or beyond the end of log is written whatever the table holds.
 * Refused (non-zero, hriemo_last_error set, nothing launched): n <= 0 or n % 4 != 0, C, P, G, capacity outside their ranges,
 * every < 1, NULL or unaligned buffers (16 bytes: g, p, m, v, partial; 8: chunks; 4: ctl, log), partial overlapping g, p, m, v,
 * chunks, hyper or state, log overlapping partial, chunks, state, ctl or grad_scale. */
int hriemo_health_sweep(const float* g, const float* p, const float* m, const float* v, long n, const long long* chunks, int C,
                        const float* hyper, const float* state, int G, const int* ctl, int every, float* partial,
                        hriemo_stream_t stream);
int hriemo_health_fold(const float* partial, const long long* chunks, int C, int P, const float* state, const int* ctl,
                       const float* grad_scale, int every, int capacity, int* log, hriemo_stream_t stream);
/* Activation log in device memory (csrc/actlog.hip; train.ActivationLog): per-site statistics of the activations of a pass and of
 * the gradients that arrive at them, written by the pass itself, so that a captured step can say in which sub-layer, sample and
 * position a non-finite value first appeared.  S sites, two halves (0: forward, 1: gradient).  State, owned by the caller:
 *   counters int32 [4]    {n_passes, n_recorded, 0, 0}; zeroed to reset
 *   window   int32 [4]    {open, slot, pass, 0}: written by the plan, read by every probe and fold behind it
 *   counts   int32 [2 S]  the chunk count of the latest probe of (half, site), at half * S + site
 *   partial  fp32 [2 S][chunk_cap][8]  one row per chunk of hriemo_act_probe_rows() rows: {sumsq, absmax, n_bad (int32 bits),
 *                         first_bad_row (int32 bits, -1: none), n_rows (int32 bits), 0, 0, 0}
 *   ring     int32        `capacity` records of 4 + 16 S words: {pass, halves (bit 0: forward folded, bit 1: gradient folded), 0, 0},
 *                         then for (half, site), at word 4 + (half * S + site) * 8: {have, n_rows, n_bad, first_bad_row,
 *                         absmax (fp32 bits), sumsq (fp32 bits), 0, 0}; record r of the run lives in slot r % capacity
 * hriemo_act_log_plan: ONE block, recorded once at the top of a pass, in front of every fork; the only writer of counters and
 * window.  record = 0 (a warm-up pass): writes the closed window {0, 0, 0, 0} and touches nothing else.  record = 1: the pass is
 * counted (pass = n_passes, n_passes += 1); if pass % every == 0 the window {1, n_recorded % capacity, pass, 0} opens, that record
 * is cleared (every have 0, header {pass, 0, 0, 0}), counts is cleared and n_recorded += 1; otherwise the window closes.
 * hriemo_act_probe: the sweep over one activation buffer x [n_rows, d] with leading dimension ld (dtype 0: bf16, 1: fp32), one
 * block of 256 threads per chunk of rows.  A block that finds the window closed returns before its first load of x and before any
 * barrier.  Which rows count, with nv = clamp(*n_valid, 1, B) (n_valid NULL: B):
 *   cu_seqlens != NULL (packed rows, int32 [B + 1] or longer): row r counts iff it lies in a sequence b < nv of the B real ones,
 *                         cu[b] <= r < cu[b + 1], at a position l = r - cu[b] < L; its index is b * L + l
 *   otherwise (padded rows [B, L], n_rows <= B * L): row r = b * L + l counts iff b < nv and (kpm == NULL or kpm[r] == 0)
 * so the filler sequence of a bucket plan, surplus rows behind the last sequence, PAD rows and the ghost utterances of a short
 * batch never count and may hold anything.  Per chunk: sumsq = the sum of x^2 over the FINITE elements of the counted rows (fp32,
 * fmaf, fixed order: per thread over its vectors tid, tid + 256, ... of the chunk element by element, the wave's xor butterfly,
 * the four wave sums in index order), absmax over the same elements, n_bad = the number of NaN / +-Inf elements (exact),
 * first_bad_row = the smallest index b * L + l of a counted row that holds one, n_rows = the counted rows.  Block 0 also stores
 * the launch's chunk count.  d % 8 == 0 (bf16) or d % 4 == 0 (fp32) with ld likewise and x 16-byte aligned reads 16-byte vectors,
 * anything else element by element.  Whatever cu_seqlens holds, x is read at rows below n_rows only.
 * hriemo_act_log_fold: once per half, one block per site; returns if the window is closed.  Folds the site's chunk partials (sum,
 * max, integer sums, min; fixed order: per thread over the chunks tid, tid + 256, ..., butterfly, four wave sums) and writes the
 * site's entry of the open record with have = 1; a site whose chunk count is 0 keeps have = 0.  Thread 0 of site 0 writes the
 * record's pass and sets the half's bit.  The slot is clamped into [0, capacity) and a chunk count into [0, chunk_cap] before
 * they address anything.  No floating-point atomics anywhere: the same pass from the same state gives the same bits.
 * Refused (non-zero, hriemo_last_error set, nothing launched): record, half or dtype outside {0, 1}, every, capacity, n_sites,
 * chunk_cap, B, L, n_rows or d < 1 (or above their limits), ld < d, B * L >= 2^31, site outside [0, n_sites), more chunks than
 * chunk_cap, padded rows beyond B * L, cu_seqlens together with kpm, NULL or misaligned state pointers (16 bytes: counters,
 * window, partial, ring; 4: counts, cu_seqlens, n_valid), state blocks that overlap each other or x. */
int hriemo_act_probe_rows(void);
int hriemo_act_log_plan(int record, int every, int capacity, int n_sites, int* counters, int* window, int* counts, int* ring,
                        hriemo_stream_t stream);
int hriemo_act_probe(const void* x, int dtype, int n_rows, int d, long ld, const int* cu_seqlens, const unsigned char* kpm, int B, int L,
                     const int* n_valid, const int* window, int site, int half, int n_sites, int chunk_cap, float* partial, int* counts,
                     hriemo_stream_t stream);
int hriemo_act_log_fold(const float* partial, const int* counts, const int* window, int half, int n_sites, int chunk_cap, int capacity,
                        int* ring, hriemo_stream_t stream);
/* Launch-boundary reduce.  hriemo_add_ln_bwd with dgamma == NULL and hriemo_colsum_bf16 with out == NULL stop after
 * their per-block partial sums ([hriemo_add_ln_bwd_partial_rows(M,d)][3*d] resp. [hriemo_colsum_partial_rows(M,N)][N]
 * fp32 at the start of the caller's workspace); hriemo_colreduce_batch finishes any number of such jobs in one launch
 * at the end of backward.  jobs_host: HOST array of njobs records (copied into the caller's device buffer jobs_dev,
 * njobs*64 bytes, through kernel arguments: capture-safe) of 8 x int64 = {partials, pstride (floats), np, w,
 * nseg | accumulate << 8 | first_block << 32, out0, out1, out2} with first_block the running sum of
 * nseg * ceil(w/32) over the preceding jobs and nblocks the total.  Deterministic (fixed summation order). */
int hriemo_add_ln_bwd_partial_rows(int M, int d);
/* Tuning / test hook: 1 (default) = LayerNorm(x + dropout(g)) forward and backward run the chunk-mapped kernels; 0 = the quad-mapped,
 * software-pipelined kernels where they are built (d = 256, 512, 768 or 1024, fp32 twin in and out, no MX copy).  Both mappings
 * draw the same dropout masks and differ by the summation order of the row statistics only.  Set it before any workspace is sized
 * (hriemo_add_ln_bwd_workspace_bytes / _partial_rows follow the variant). */
int hriemo_rowops_force_variant(int variant);
int hriemo_colsum_partial_rows(int M, int N);
int hriemo_colreduce_batch(const void* jobs_host, int njobs, void* jobs_dev, int nblocks, hriemo_stream_t stream);
/* tuning hook: `blocks` CUs made unavailable for ~`micros` us (stands in for a collective running beside the step) */
int hriemo_debug_hog(int blocks, int micros, float* sink, hriemo_stream_t stream);
/* The gate's two modalities from ONE launch (d <= 1024: hriemo_ln_pool_pair_supported): side a = audio (gate coefficient w), side t =
 * text (1 - w); the blocks are those of the single calls, so are the results.  Replaces two launches on two streams and the fork /
 * join around them (models/beta_gate_tacfn.py:79-84 forward, its autograd backward). */
int hriemo_ln_pool_pair_supported(int d);
int hriemo_ln_pool_fwd_pair(const void* Xa, const float* Xa32, const unsigned char* mask_a, const float* gamma_a, const float* beta_a,
                            void* Yna, float* mean_a, float* rstd_a, float* partials_a, int La,
                            const void* Xt, const float* Xt32, const unsigned char* mask_t, const float* gamma_t, const float* beta_t,
                            void* Ynt, float* mean_t, float* rstd_t, float* partials_t, int Lt,
                            int B, int Lkeep, int d, float eps, hriemo_stream_t stream);
int hriemo_ln_pool_bwd_pair(const void* dH, int Lf, const float* w,
                            const float* dpool_a, const unsigned char* mask_a, const void* Xa, const float* Xa32, const float* gamma_a,
                            const float* mean_a, const float* rstd_a, void* dXa, float* dgamma_a, float* dbeta_a, int La, float* workspace_a,
                            const float* dpool_t, const unsigned char* mask_t, const void* Xt, const float* Xt32, const float* gamma_t,
                            const float* mean_t, const float* rstd_t, void* dXt, float* dgamma_t, float* dbeta_t, int Lt, float* workspace_t,
                            int accumulate, int B, int d, hriemo_stream_t stream);
/* row chunks per sample of hriemo_ln_pool_bwd: its partial sums are [B * chunks][2 d] floats at the head of `workspace` */
int hriemo_ln_pool_bwd_chunks(int L);
long hriemo_ln_pool_bwd_workspace_bytes(int B, int L, int d);
int hriemo_ln_pool_bwd(const void* dH, int Lf, const float* w, int is_a, const float* dpool, const unsigned char* mask,
                       const void* X, const float* X32, const float* gamma, const float* mean, const float* rstd, void* dX,
                       float* dgamma, float* dbeta, int accumulate, int B, int L, int d, float* workspace, hriemo_stream_t stream);
/* (dgamma / dbeta: overwritten, or added to when accumulate != 0; both NULL: the per-block partial sums stay in `workspace`, rows
 * [B * ceil(L/32)] of [dgamma | dbeta] (2d floats each), for hriemo_colreduce_batch at the end of backward) */

/* ---- the pooled gate (models/fusion_classifier.py:142-145): the classifier reads the fused sequence only through its UNMASKED mean
 * over the L fused positions, so   pooled[b] = w[b] * Abar[b] + (1 - w[b]) * Tbar[b],   Abar[b] = (1/Lkeep) sum_{l < Lkeep} LN_a(h_a)[b, l]
 * (Tbar likewise; PAD rows l < Lkeep are part of the sum, as in the reference), and neither Yn, h_fusion nor a [B, L, d] gradient
 * is ever formed.  Padded rows only; d % 8 == 0, d <= 2048 (pairs: d <= 1024); 1 <= Lkeep <= L.
 *  - hriemo_ln_pool2_fwd: ONE pass over X (bf16, or its fp32 twin X32 when non-NULL; key-padding mask optional) with the blocks and
 *    the wave walk of hriemo_ln_pool_fwd.  mean, rstd [B*L] and `partials` [B, hriemo_pool_chunks(L), d] (sums over the VALID rows
 *    of every 32-row chunk) equal hriemo_ln_pool_fwd's bit for bit, so hriemo_gate_input runs unchanged; `partials_keep` (same
 *    shape) holds the sums over rows l < Lkeep whatever the mask says, zeros in chunks behind Lkeep.  No Yn is written.
 *  - hriemo_pooled_fuse_fwd: partials_keep of both sides + gate weights w [B, d] -> Abar, Tbar, pooled (fp32 [B, d]).
 *  - hriemo_pooled_fuse_bwd: dpooled (NULL: zero) -> dw = dpooled * (Abar - Tbar) [B, d] (one chunk of dw partials: hriemo_gate_dpre
 *    with L <= 32) and the row gradients g_a = w * dpooled / Lkeep, g_t = (1 - w) * dpooled / Lkeep [B, d].
 *  - hriemo_ln_pool_vec_bwd: hriemo_ln_pool_bwd with the fp32 vector g[b, :] (NULL: zero) standing in for coef * dH[b, l, :] on
 *    rows l < Lkeep:  dYn[b, l] = (l < Lkeep ? g[b] : 0) + (valid ? dpool[b] : 0),  dX = LayerNorm'(dYn).  Same workspace
 *    (hriemo_ln_pool_bwd_workspace_bytes), same dgamma | dbeta partial layout and the same dgamma / dbeta / accumulate rules.
 *  - *_pair: both modalities from one launch, the blocks -- and the results -- of the single calls. */
int hriemo_ln_pool2_fwd(const void* X, const float* X32, const unsigned char* mask, const float* gamma, const float* beta,
                        float* mean, float* rstd, float* partials, float* partials_keep, int B, int L, int Lkeep, int d, float eps,
                        hriemo_stream_t stream);
int hriemo_ln_pool2_fwd_pair(const void* Xa, const float* Xa32, const unsigned char* mask_a, const float* gamma_a, const float* beta_a,
                             float* mean_a, float* rstd_a, float* partials_a, float* partials_keep_a, int La,
                             const void* Xt, const float* Xt32, const unsigned char* mask_t, const float* gamma_t, const float* beta_t,
                             float* mean_t, float* rstd_t, float* partials_t, float* partials_keep_t, int Lt,
                             int B, int Lkeep, int d, float eps, hriemo_stream_t stream);
int hriemo_pooled_fuse_fwd(const float* partials_keep_a, int La, const float* partials_keep_t, int Lt, const float* w, int Lkeep,
                           float* abar, float* tbar, float* pooled, int B, int d, hriemo_stream_t stream);
int hriemo_pooled_fuse_bwd(const float* dpooled, const float* abar, const float* tbar, const float* w, int Lkeep, float* dw,
                           float* g_a, float* g_t, int B, int d, hriemo_stream_t stream);
int hriemo_ln_pool_vec_bwd(const float* g, int Lkeep, const float* dpool, const unsigned char* mask, const void* X, const float* X32,
                           const float* gamma, const float* mean, const float* rstd, void* dX, float* dgamma, float* dbeta,
                           int accumulate, int B, int L, int d, float* workspace, hriemo_stream_t stream);
int hriemo_ln_pool_vec_bwd_pair(int Lkeep,
                                const float* g_a, const float* dpool_a, const unsigned char* mask_a, const void* Xa, const float* Xa32, const float* gamma_a,
                                const float* mean_a, const float* rstd_a, void* dXa, float* dgamma_a, float* dbeta_a, int La, float* workspace_a,
                                const float* g_t, const float* dpool_t, const unsigned char* mask_t, const void* Xt, const float* Xt32, const float* gamma_t,
                                const float* mean_t, const float* rstd_t, void* dXt, float* dgamma_t, float* dbeta_t, int Lt, float* workspace_t,
                                int accumulate, int B, int d, hriemo_stream_t stream);
/* Packed rows in, PADDED rows out (the classifier's front door): X packed [n_rows, d] (x_dtype 0 fp32, 1 bf16, 2 fp16; row stride
 * ldx elements) with cu_seqlens int32 [>= B + 1] in device memory -> Y16 bf16 [B, L, d] and the fp32 twin Y32 (either may be NULL).
 * Row (b, l) is source row cu[b] + l for l < cu[b+1] - cu[b] and zeros behind it; no source row at or behind min(cu[B], n_rows) is
 * read.  A valid row equals hriemo_ingest_rows followed by hriemo_unpack_rows bit for bit. */
int hriemo_ingest_padded(const void* X, int x_dtype, long ldx, const int* cu_seqlens, int n_rows, int B, int L, int d, void* Y16,
                         float* Y32, hriemo_stream_t stream);

/* ---- the gate on packed (varlen) rows: the encoder's packed output feeds the gate and the gate's h_fusion stays packed for the
 * decoder, so no hriemo_unpack_rows / hriemo_pack_rows runs between the encoder and the loss.
 *  - A modality's X / X32 / mean / rstd / dX are packed [n_rows, d] buffers with cu_seqlens (int32 [nseq + 1], device memory):
 *    sample b = rows cu[b] .. cu[b+1]-1, every row valid.  nseq = B, or B + 1 when the rows behind the last sample form the
 *    bucket's surplus sequence (hriemo_pack_rows' zero rows): those rows get mean = rstd = 0 and dX = 0, and pool nothing.
 *  - Yn / H / dH live in the packed FUSED layout [n_fused, d] with cu_fused (int32 [B + 1]): sample b has
 *    lf[b] = min(audio length, text length) rows (the reference ORs the two prefix masks cut to L_t,
 *    models/fusion_with_emotion_decoder.py:62-79).  Rows cu_fused[B] .. n_fused-1 are surplus: every kernel here that writes a
 *    fused buffer writes them as zeros (the decoder's K | V weight-gradient GEMM multiplies every row).
 *  - L is the padded length of that side (it sizes the grid and the partial-sum layouts; lengths are clamped to it and to the
 *    buffers).  The pooled partials stay [B, hriemo_pool_chunks(L), d], the dw partials [B, hriemo_pool_chunks(L), d] and the
 *    dgamma | dbeta partials [B * hriemo_ln_pool_bwd_chunks(L)][2d], chunks behind a sample's end hold zeros: hriemo_gate_input,
 *    hriemo_gate_dpre, hriemo_colreduce_batch and the gate MLP run unchanged, and a block adds the rows the padded kernel adds in
 *    the same order -- pooled sums, Yn, H, dw partials and dX equal the padded launch's bit for bit on the valid rows.
 *  - hriemo_ln_pool_bwd_packed: dH may be NULL (no gradient through h_fusion); rows l >= lf[b] of a sample get the pooled
 *    gradient only.  workspace as hriemo_ln_pool_bwd (hriemo_ln_pool_bwd_workspace_bytes(B, L, d)).
 *  - *_pair: both modalities from one launch (d <= 1024), the blocks -- and the results -- of the single calls. */
int hriemo_ln_pool_fwd_packed(const void* X, const float* X32, const int* cu_seqlens, int nseq, int n_rows, const float* gamma,
                              const float* beta, void* Yn, float* mean, float* rstd, float* partials, int L,
                              const int* cu_fused, int n_fused, int B, int d, float eps, hriemo_stream_t stream);
int hriemo_ln_pool_fwd_packed_pair(const void* Xa, const float* Xa32, const int* cu_a, int nseq_a, int n_rows_a, const float* gamma_a,
                                   const float* beta_a, void* Yna, float* mean_a, float* rstd_a, float* partials_a, int La,
                                   const void* Xt, const float* Xt32, const int* cu_t, int nseq_t, int n_rows_t, const float* gamma_t,
                                   const float* beta_t, void* Ynt, float* mean_t, float* rstd_t, float* partials_t, int Lt,
                                   const int* cu_fused, int n_fused, int B, int d, float eps, hriemo_stream_t stream);
/* H = w * A + (1 - w) * T on the packed fused rows (the sample of a row comes from cu_fused); dw partials of the same rows */
int hriemo_fuse_fwd_packed(const float* w, const void* A, const void* T, void* H, const int* cu_fused, int n_fused, int B, int L, int d,
                           hriemo_stream_t stream);
/* hriemo_fuse_fwd_packed that also leaves the MX-fp8 form of H for the decoder's memory K | V projection (fp8 GEMM mode): bytes
 * Hq[n_fused][d], E8M0 scales Hs[d/32][lds] with the scale byte of row r in column r (lds >= n_fused, a multiple of 256),
 * bit-identical to hriemo_quant_mx8(H); the surplus rows get zero bytes and zero scale bytes.  d % 32 == 0. */
int hriemo_fuse_fwd_packed_q(const float* w, const void* A, const void* T, void* H, const int* cu_fused, int n_fused, int B, int L, int d,
                             void* Hq, void* Hs, long lds, hriemo_stream_t stream);
int hriemo_fuse_bwd_dw_packed(const void* dH, const void* A, const void* T, float* partials, const int* cu_fused, int n_fused, int B,
                              int L, int d, hriemo_stream_t stream);
int hriemo_ln_pool_bwd_packed(const void* dH, const int* cu_fused, int n_fused, const float* w, int is_a, const float* dpool,
                              const void* X, const float* X32, const int* cu_seqlens, int nseq, int n_rows, const float* gamma,
                              const float* mean, const float* rstd, void* dX, float* dgamma, float* dbeta, int accumulate, int B, int L,
                              int d, float* workspace, hriemo_stream_t stream);
int hriemo_ln_pool_bwd_packed_pair(const void* dH, const int* cu_fused, int n_fused, const float* w,
                                   const float* dpool_a, const void* Xa, const float* Xa32, const int* cu_a, int nseq_a, int n_rows_a,
                                   const float* gamma_a, const float* mean_a, const float* rstd_a, void* dXa, float* dgamma_a,
                                   float* dbeta_a, int La, float* workspace_a,
                                   const float* dpool_t, const void* Xt, const float* Xt32, const int* cu_t, int nseq_t, int n_rows_t,
                                   const float* gamma_t, const float* mean_t, const float* rstd_t, void* dXt, float* dgamma_t,
                                   float* dbeta_t, int Lt, float* workspace_t, int accumulate, int B, int d, hriemo_stream_t stream);

/* ---- fp32-tolerance mode, forward (csrc/fp32mode.hip; host side hri-emo_amd/_fp32.py, HRIEMO_PRECISION=fp32).
 * The reference's modules are fp32 nn.Modules throughout (models/cross_modal_block_tacfn.py:70-125, beta_gate_tacfn.py:68-118,
 * emotion_decoder.py:30-64,116-162); this mode reproduces them to 1e-3 (no dropout; the backward follows below):
 *  - hriemo_split_bf16x3: X fp32 [M,K] (row stride ldx) -> Y bf16 [M,3K], x = hi + mid + ..: layout 0 (activations) [hi|mid|hi],
 *    layout 1 (weights) [hi|hi|mid]; relu != 0 applies max(x,0) first.  hriemo_gemm_bf16 over the 3K-long contraction with fp32
 *    output then gives hi.hi + mid.hi + hi.mid, the fp32 product to 2^-16 relative (nn.Linear, nn.MultiheadAttention in/out-proj);
 *  - hriemo_attn_fwd_f32 / hriemo_attn_probs_f32: softmax(Q K^T / sqrt(hd) + key padding) V on the fp32 MFMA
 *    (v_mfma_f32_16x16x4_f32), operands and outputs fp32 with row strides; lse = log-sum-exp of the scaled scores per
 *    (batch, head, query), probs = head-averaged probabilities [B,Lq,Lk] (need_weights=True);
 *  - hriemo_add_ln_f32: Y32 (and the bf16 copy Y16 when non-NULL) = LayerNorm(drop(G) + X) (X may be NULL), fp32 in and out;
 *  - dropout (round 4): every fp32 kernel that sits where the reference drops takes (p_drop, seed, seed_dev, site, offset) like its
 *    bf16 counterpart and draws the SAME mask from the same counter hash (hriemo_add_ln_fwd / hriemo_attn_fwd / hriemo_dropout_bf16):
 *    attention weights after the softmax (the exported probabilities too, as nn.MultiheadAttention returns them in training mode),
 *    the sub-layer output before the residual add, and hriemo_dropout_f32 for the FFN's hidden layer: Y = drop(relu ? max(X,0) : X)
 *    [* (gate > 0) when gate is non-NULL: the backward form, X = gradient, gate = pre-activations]; p_drop = 0 drops nothing;
 *  - gate pieces of models/beta_gate_tacfn.py in fp32: masked mean (:6-24), gate input [a,t,|a-t|,a*t] (:87-89),
 *    w = sigmoid(pre) / beta = mean(w) (:92-95), h = w*a + (1-w)*t over the first L positions (:98-116; A, T are [B,La,d], [B,Lt,d]). */
int hriemo_split_bf16x3(const float* X, long ldx, int M, int K, void* Y, int layout, int relu, hriemo_stream_t stream);
int hriemo_attn_fwd_f32(const float* Q, long ldq, const float* K, long ldk, const float* V, long ldv, float* O, long ldo,
                        const unsigned char* key_padding_mask, float* lse, int B, int H, int Lq, int Lk, int head_dim,
                        float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site, int b_offset,
                        hriemo_stream_t stream);
int hriemo_attn_probs_f32(const float* Q, long ldq, const float* K, long ldk, const unsigned char* key_padding_mask,
                          const float* lse, float* probs, int B, int H, int Lq, int Lk, int head_dim, float p_drop,
                          unsigned long long seed, const unsigned long long* seed_dev, unsigned site, int b_offset,
                          hriemo_stream_t stream);
int hriemo_add_ln_f32(const float* G, const float* X, const float* gamma, const float* beta, float* Y32, void* Y16, int M, int d,
                      float eps, float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site,
                      long row_offset, hriemo_stream_t stream);
int hriemo_dropout_f32(const float* X, float* Y, long M, int N, int relu, const float* gate, float p_drop, unsigned long long seed,
                       const unsigned long long* seed_dev, unsigned site, long row_offset, hriemo_stream_t stream);
int hriemo_masked_mean_f32(const float* X, const unsigned char* mask, float* pooled, int B, int L, int d, hriemo_stream_t stream);
int hriemo_gate_input_f32(const float* a_pool, const float* t_pool, float* gate_in, int B, int d, hriemo_stream_t stream);
int hriemo_sigmoid_beta_f32(const float* pre, float* w, float* beta, int B, int d, hriemo_stream_t stream);
int hriemo_fuse_f32(const float* w, const float* A, int La, const float* T, int Lt, float* H32, void* H16, int B, int L, int d,
                    hriemo_stream_t stream);

/* ---- fp32-tolerance TRAINING step: the backward of the pieces above in the same arithmetic (round 4).  The IEMOCAP trainer runs
 * the reference in fp32 without autocast (scripts/fusion/train_fusion_seq_level_decoder.py:310-334); with HRIEMO_PRECISION=fp32 the
 * modules of hri-emo_amd/models keep every activation and every gradient in fp32 (host side hri-emo_amd/_fp32.py).  Dropout 0 only.
 *  - hriemo_split3_f32: the operand split in four forms.  X fp32 [M,K] (row stride ldx), optionally times (mask > 0) (mask fp32
 *    [M, ldmask]: ReLU's derivative) and / or clamped at 0 (relu) -> bf16
 *      form 0: Y[M][3K] = [hi | mid | hi]      form 1: Y[M][3K] = [hi | hi | mid]       contraction along the columns of X
 *      form 2: Y[3M][K] = [hi ; mid ; hi]      form 3: Y[3M][K] = [hi ; hi ; mid]       contraction along the rows of X
 *      form 4: Y[M][6K] = [hi|mid|lo|hi|mid|hi]  form 5: Y[M][6K] = [hi|hi|hi|mid|mid|lo]  (x = hi + mid + lo exactly: six products,
 *      form 6: Y[6M][K] = [hi;mid;lo;hi;mid;hi]  form 7: Y[6M][K] = [hi;hi;hi;mid;mid;lo]   2^-24 relative; what _fp32.py uses: no
 *              ReLU pre-activation changes sign against fp32, ill-conditioned weights keep every gradient within 1e-3)
 *    dX = dY . W is hriemo_gemm_bf16(ta 0, tb 1) on form 0 (4) of dY and form 3 (7) of W (K = 3 (6) N_out); dW = dY^T . X is
 *    (ta 1, tb 1) on form 2 (6) of dY and form 3 (7) of X (K = 3 (6) M); fp32 output.
 *  - hriemo_colsum_f32: out[n] (+)= sum_m X[m][n] * (mask[m][n] > 0) (bias gradients; mask fp32 [M, ldmask] or NULL), fixed
 *    summation order; workspace >= hriemo_colsum_f32_workspace_bytes.
 *  - hriemo_add_ln_bwd_f32: backward of Y = LayerNorm(drop(G) + X) * gamma + beta (X may be NULL): dS = d loss / d (drop(G) + X)
 *    [M,d] (= dX; = dG as well when p_drop = 0, dG may then be NULL; with dropout dG = dS * keep / (1 - p) is written to its own
 *    matrix), dgamma / dbeta / dbias (= column sums of dG; may be NULL) overwritten or added to (accumulate); the row statistics
 *    are recomputed from drop(G) + X.  d <= 1024.  workspace >= hriemo_add_ln_bwd_f32_workspace_bytes(M, d).
 *  - hriemo_attn_bwd_f32: dQ, dK, dV of O = softmax(Q K^T / sqrt(hd) + key padding) V from Q, K, V, O, dO and the forward's lse, on
 *    v_mfma_f32_16x16x4_f32; two kernels (dQ per 64 queries, dK / dV per 64 keys), no atomics, fixed order; delta: scratch
 *    [B, H, Lq] floats (rowsum(dO * O), written by the first kernel for the second).  nn.MultiheadAttention, cross_modal_block_
 *    tacfn.py:74-80,98-117, emotion_decoder.py:42,48-54.
 *  - gate backward (beta_gate_tacfn.py:79-116): hriemo_gate_dpre_f32: dpre[B,d] = (sum_{l<L} dH (A - T) + dbeta / d) w (1 - w)
 *    (dbeta [B] may be NULL); hriemo_gate_input_bwd_f32: gradients of the pooled means from d [a, t, |a-t|, a*t];
 *    hriemo_gate_dy_f32: the gradient that reaches LayerNorm_x's output of one modality, dY[B,Lx,d] = (l < L ? wsel dH : 0) +
 *    (valid ? dpool / max(#valid, 1) : 0), wsel = w (is_a) or 1 - w; the LayerNorm itself goes through hriemo_add_ln_bwd_f32.
 *  - hriemo_rowdot_bwd_f32: logits = z . w + b (emotion_decoder.py:155): dZ[M,d] = dl w, dw[d] (+)= sum_m dl z, db[1] (+)= sum dl. */
int hriemo_split3_f32(const float* X, long ldx, int M, int K, void* Y, int form, int relu, const float* mask, long ldmask,
                      hriemo_stream_t stream);
long hriemo_colsum_f32_workspace_bytes(int M, int N);
int hriemo_colsum_f32(const float* X, long ldx, int M, int N, const float* mask, long ldmask, float* out, int accumulate,
                      float* workspace, hriemo_stream_t stream);
long hriemo_add_ln_bwd_f32_workspace_bytes(int M, int d);
int hriemo_add_ln_bwd_f32(const float* dY, const float* G, const float* X, const float* gamma, float* dS, float* dG, float* dgamma,
                          float* dbeta, float* dbias, int accumulate, int M, int d, float eps, float p_drop, unsigned long long seed,
                          const unsigned long long* seed_dev, unsigned site, long row_offset, float* workspace, hriemo_stream_t stream);
int hriemo_attn_bwd_f32(const float* Q, long ldq, const float* K, long ldk, const float* V, long ldv, const float* O, long ldo,
                        const float* dO, long lddo, const unsigned char* key_padding_mask, const float* lse, float* dQ, long lddq,
                        float* dK, long lddk, float* dV, long lddv, float* delta, int B, int H, int Lq, int Lk, int head_dim,
                        float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site, int b_offset,
                        hriemo_stream_t stream);
int hriemo_gate_dpre_f32(const float* dH, const float* A, int La, const float* T, int Lt, const float* w, const float* dbeta, float* dpre,
                         int B, int L, int d, hriemo_stream_t stream);
int hriemo_gate_input_bwd_f32(const float* dgin, const float* a_pool, const float* t_pool, float* da, float* dt, int B, int d,
                              hriemo_stream_t stream);
int hriemo_gate_dy_f32(const float* dH, const float* w, int is_a, const float* dpool, const unsigned char* mask, float* dY, int B, int L,
                       int Lx, int d, hriemo_stream_t stream);
int hriemo_rowdot_bwd_f32(const float* dl, const float* Z, const float* w, float* dZ, float* dw, float* db, int accumulate, int M, int d,
                          hriemo_stream_t stream);

/* ---- the pooled gate in the fp32-tolerance mode (FusionClassifier; "the pooled gate" above is its bf16 form): fp32 in and out,
 * padded rows only, d % 4 == 0 and d <= 1024 (the limit of the mode's LayerNorm backward), 1 <= Lkeep <= L; anything else is
 * refused with a message.  Every sum has a fixed order (no float atomics): two launches on the same inputs agree bit for bit.
 *  - hriemo_pool32_ln_fwd: ONE pass over X fp32 [B, L, d] (mask uint8 [B, L], 1 = PAD, or NULL).  Per row the LayerNorm of
 *    hriemo_add_ln_f32 (two-pass variance, 1 / sqrt(var + eps)), kept in registers and never stored.  part_valid / part_keep are
 *    fp32 [B, hriemo_pool_chunks(L), d]: per 32-row chunk the sums of the LayerNorm outputs over the VALID rows, and over the rows
 *    l < Lkeep whatever the mask says (chunks behind Lkeep: zeros).  Within a chunk wave w of four adds rows w, w + 4, ... in that
 *    order, then the four waves are added in wave order.  No Yn, mean or rstd is written.
 *  - hriemo_pool32_gate_input: the chunk sums of both modalities added in chunk order and divided by max(#valid, 1) -> a_pool,
 *    t_pool [B, d] and gate_in [B, 4d] = [a, t, |a - t|, a * t], bit-equal to hriemo_gate_input_f32 of those pools.  One launch in
 *    place of two masked means and the gate-input kernel.
 *  - hriemo_pool32_ln_bwd: dYn[b, l] = (l < Lkeep ? g[b] : 0) + (valid ? dpool[b] / max(#valid_b, 1) : 0) with g, dpool fp32 [B, d]
 *    (g NULL: zero; the count is formed in the kernel), dX fp32 [B, L, d] = LayerNorm'(dYn) with the row statistics recomputed
 *    from X.  dgamma / dbeta [d]: column sums over all B * L rows (per-block partials in `workspace`,
 *    hriemo_pool32_ln_bwd_workspace_bytes(B, L, d), then one fixed-order reduce); overwritten, or added to when accumulate != 0;
 *    both NULL (no affine gradients, workspace unused), or neither.  No [B, L, d] gradient other than dX is formed.
 *  The [B, d]-sized pieces are the existing exports: hriemo_pooled_fuse_fwd / _bwd (fp32 arithmetic), hriemo_sigmoid_beta_f32,
 *  hriemo_gate_dpre_f32 with L = 1 (dH = dpooled, A = Abar, T = Tbar) and hriemo_gate_input_bwd_f32. */
int hriemo_pool32_ln_fwd(const float* X, const unsigned char* mask, const float* gamma, const float* beta, float* part_valid,
                         float* part_keep, int B, int L, int Lkeep, int d, float eps, hriemo_stream_t stream);
int hriemo_pool32_gate_input(const float* part_valid_a, const unsigned char* mask_a, int La, const float* part_valid_t,
                             const unsigned char* mask_t, int Lt, float* a_pool, float* t_pool, float* gate_in, int B, int d,
                             hriemo_stream_t stream);
long hriemo_pool32_ln_bwd_workspace_bytes(int B, int L, int d);
int hriemo_pool32_ln_bwd(const float* g, int Lkeep, const float* dpool, const unsigned char* mask, const float* X, const float* gamma,
                         float* dX, float* dgamma, float* dbeta, int accumulate, int B, int L, int d, float eps, float* workspace,
                         hriemo_stream_t stream);

/* ---- fp32-tolerance mode on packed (varlen) sequences: the encoder on the valid rows only (hriemo_attn_*_varlen's contract).
 *  - hriemo_attn_fwd_f32_varlen / hriemo_attn_bwd_f32_varlen: hriemo_attn_fwd_f32 / _bwd_f32 with cu_seqlens_q / cu_seqlens_k
 *    (int32 [B+1], device memory, every length >= 1) in place of the key padding mask: sample b = rows cu[b] .. cu[b+1]-1 of
 *    Q / O / dO / dQ (cu_seqlens_q) and K / V / dK / dV (cu_seqlens_k); max_len_q / max_len_k are the longest sequences (grid, and
 *    the row stride of lse / delta, which keep their padded [B, H, max_len_q] slots).  The dropout hash is keyed by position within
 *    the sequence, i.e. the padded (batch, query, key): a packed launch drops what the padded one drops.
 *  - hriemo_add_ln_f32_rows / hriemo_add_ln_bwd_f32_rows: hriemo_add_ln_f32 / _bwd_f32 on rows gathered from a larger layout; the
 *    residual-dropout hash is keyed by row_index[row] + row_offset (int64 [M], the padded row hriemo_pack_rows writes). */
int hriemo_attn_fwd_f32_varlen(const float* Q, long ldq, const float* K, long ldk, const float* V, long ldv, float* O, long ldo,
                               const int* cu_seqlens_q, const int* cu_seqlens_k, float* lse, int B, int H, int max_len_q, int max_len_k,
                               int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site,
                               int b_offset, hriemo_stream_t stream);
int hriemo_attn_bwd_f32_varlen(const float* Q, long ldq, const float* K, long ldk, const float* V, long ldv, const float* O, long ldo,
                               const float* dO, long lddo, const int* cu_seqlens_q, const int* cu_seqlens_k, const float* lse, float* dQ,
                               long lddq, float* dK, long lddk, float* dV, long lddv, float* delta, int B, int H, int max_len_q,
                               int max_len_k, int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev,
                               unsigned site, int b_offset, hriemo_stream_t stream);
/*  - hriemo_attn_probs_f32_varlen: hriemo_attn_probs_f32 on those packed rows, the contract of hriemo_attn_probs_varlen (padded map
 *    [B, out_lq, out_lk], every element written, zeros in PAD key columns and PAD query rows, no row of K past cu_seqlens_k[B] read). */
int hriemo_attn_probs_f32_varlen(const float* Q, long ldq, const float* K, long ldk, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                 const float* lse, float* probs, int B, int H, int max_len_q, int max_len_k, int out_lq, int out_lk,
                                 int head_dim, float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site,
                                 int b_offset, hriemo_stream_t stream);
int hriemo_add_ln_f32_rows(const float* G, const float* X, const float* gamma, const float* beta, float* Y32, void* Y16, int M, int d,
                           float eps, float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site,
                           long row_offset, const long long* row_index, hriemo_stream_t stream);
int hriemo_add_ln_bwd_f32_rows(const float* dY, const float* G, const float* X, const float* gamma, float* dS, float* dG, float* dgamma,
                               float* dbeta, float* dbias, int accumulate, int M, int d, float eps, float p_drop, unsigned long long seed,
                               const unsigned long long* seed_dev, unsigned site, long row_offset, float* workspace,
                               const long long* row_index, hriemo_stream_t stream);

/* ---- fp32-tolerance mode, the gate on packed (varlen) rows: the packed arm of the four gate kernels that index by sequence
 * position (same kernel bodies, so the arithmetic and its order are the padded launch's).  Three layouts meet: the audio rows
 * (cu_a [B+1], n_a rows), the text rows (cu_t, n_t) and the fused rows (cu_fused, n_fused; sample b owns min(la, lt) rows); sample
 * b of a layout = rows cu[b] .. cu[b+1]-1.  The cu arrays are int32 DEVICE memory: grids depend on (B, L, d) only, the lengths are
 * read by the blocks and clamped to the buffers and to the padded lengths La / Lt / L (a stale cu cannot send a block out of
 * bounds), so one captured graph serves every batch of a bucket.  Rows of a buffer behind its last sample (the surplus rows of a
 * fused bucket plan, the all-zero filler sequence of a modality's) are written as ZEROS.  The LayerNorms of the gate are
 * row-wise: hriemo_add_ln_f32 / hriemo_add_ln_bwd_f32 run on the packed rows as they are.
 *  - hriemo_masked_mean_f32_packed: pooled[b] = sum of the sample's rows of X [n_rows, d] / max(len, 1), in position order.
 *  - hriemo_fuse_f32_packed: H[cu_fused[b] + j] = w[b] A[cu_a[b] + j] + (1 - w[b]) T[cu_t[b] + j] for j < cu_fused[b+1] -
 *    cu_fused[b]; rows cu_fused[B] .. n_fused-1 of H32 and (when given) H16 are zeros.
 *  - hriemo_gate_dpre_f32_packed: hriemo_gate_dpre_f32 with the sum over j < lf[b] (dH on the fused rows, A / T on their own).
 *  - hriemo_gate_dy_f32_packed: dY[cu_x[b] + i] = dpool[b] / max(len_x[b], 1) + (i < lf[b] ? wsel dH[cu_fused[b] + i] : 0) on
 *    the modality's n_x packed rows; rows cu_x[B] .. n_x-1 are zeros. */
int hriemo_masked_mean_f32_packed(const float* X, const int* cu_seqlens, int n_rows, float* pooled, int B, int L, int d,
                                  hriemo_stream_t stream);
int hriemo_fuse_f32_packed(const float* w, const float* A, const int* cu_a, int n_a, int La, const float* T, const int* cu_t, int n_t, int Lt,
                           float* H32, void* H16, const int* cu_fused, int n_fused, int B, int L, int d, hriemo_stream_t stream);
int hriemo_gate_dpre_f32_packed(const float* dH, const int* cu_fused, int n_fused, const float* A, const int* cu_a, int n_a, int La,
                                const float* T, const int* cu_t, int n_t, int Lt, const float* w, const float* dbeta, float* dpre, int B,
                                int L, int d, hriemo_stream_t stream);
int hriemo_gate_dy_f32_packed(const float* dH, const int* cu_fused, int n_fused, const float* w, int is_a, const float* dpool,
                              const int* cu_x, int n_x, float* dY, int B, int L, int Lx, int d, hriemo_stream_t stream);

/* ---- per-kernel-class HIP-event timing on the launch stream (bench.py roofline leg) */
int hriemo_prof_enable(int on);
int hriemo_prof_nclass(void);
const char* hriemo_prof_name(int cls);
int hriemo_prof_collect(int cls, double* ms_total, long* launches, double* work);

/* ---- Linear + bias + dropout + residual + LayerNorm in one kernel (round 4, csrc/gemm_ln.hip) ---------------------------------
 * north_star's "fused bias + LayerNorm + residual epilogue" for the post-LN sites of a fusion layer (cross_modal_block_tacfn.py:
 * 81,92,105,106,118,119):  G = A[M,K] . W[d,K]^T + bias (bf16; kept because the backward reads it; may be NULL),
 * Y16 / Y32 (may be NULL) = LayerNorm(X + drop(G)) * gamma + beta, mean / rstd [M] as hriemo_add_ln_fwd leaves them.  X = X32 (fp32
 * twin) when non-NULL, else X16 (bf16).  A workgroup owns 64 FULL rows (LayerNorm needs them), d in {256, 512, 768}
 * (hriemo_gemm_ln_supported).  Dropout mask and keys = hriemo_add_ln_fwd(_rows); row_index as there (packed sequences) or NULL.
 * G is bit-identical to hriemo_gemm_bf16's output, Y to hriemo_add_ln_fwd's within the summation order of the row statistics. */
int hriemo_gemm_ln_supported(int d);
int hriemo_gemm_ln_fwd(int M, int d, int K, const void* A, long lda, const void* W, long ldw, const float* bias, const void* X16,
                       const float* X32, const float* gamma, const float* beta, void* G, void* Y16, float* Y32, float* mean, float* rstd,
                       float eps, float p_drop, unsigned long long seed, const unsigned long long* seed_dev, unsigned site,
                       long row_offset, const long long* row_index, hriemo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HRIEMO_H_ */
