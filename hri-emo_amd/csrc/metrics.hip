// Epoch statistics of the reference's trainers, kept in device memory so that a captured trainer step never reads anything back:
//   scripts/fusion/train_fusion_seq_level_decoder.py:300-372         sample-weighted mean loss, accuracy, mean beta
//   scripts/fusion/train_mosei_fusion_seq_level_decoder.py:119-171,367-495   mean loss (non-finite batches skipped), mean beta,
//                                                                    micro / macro F1, macro AUC, the 19-threshold calibration sweep
//   hriemo_stats_update   one block behind the loss launch of a step: appends sigmoid(logits) and [target > 0] of the batch's own
//                         samples to the epoch's log, adds to the sums and counters
//   hriemo_stats_counts   tp / fp / fn per class and threshold over the log                     (once per epoch)
//   hriemo_stats_auc      2 [p_i > p_j] + [p_i == p_j] over all (positive i, negative j) pairs   (once per epoch, the O(N^2) part)
//   hriemo_stats_rank     per logged sample the number of positives / negatives with p_j >= p_i: average precision, PR and ROC
//                         curves of the reference's reporting layer (tools/mosei_export_per_class_metrics.py,
//                         scripts/infer/mosei_plot_metrics.py) from integers                    (on demand, O(N^2) as well)
//   hriemo_stats_confusion  one block behind hriemo_stats_update of a single-label step: the confusion matrix of the epoch
//                         (macro / weighted F1, recall per class: train_text_baseline.py:59-61, linear_probe_baseline.py:132-133)
// and the products of the reference's inference driver (scripts/infer/mosei_eval_infer.py: {split}_y_prob.npy, {split}_beta_mean.npy):
//   hriemo_predict_log    one block behind the forward of a (captured) evaluation step: appends the batch's probabilities (sigmoid
//                         or softmax), its per-sample mean beta and -- single-label -- its argmax to a log that needs no targets
// and its --dump_attn --attn_max_samples K product, the attention maps of the split's first K samples:
//   hriemo_attn_log_plan  one block at the top of a (captured) pass: moves the log's cursor and writes the window {slot0, n_take}
//                         that the export launches of the pass read (hriemo_attn_probs_varlen_log, csrc/attention.hip; its fp32
//                         twin, csrc/fp32mode.hip); hriemo_attn_log_close writes the closed window of a warm-up pass
//   hriemo_attn_log_append  the window rule as a copy, for a map that a padded export produced
// The device hands back integers only; every ratio is formed on the host in float64 (train.EpochStats.result).
// Plain C++, vector stores only.  Built with -fno-slp-vectorize like loss.hip: the scalar tails of the one-block kernel are where
// hipcc produces the packed fp32 operand-select form `make check-isa` forbids.
#include "common.h"

// counters[8] (int32) and sums[4] (float64) of one epoch: the layout include/hriemo.h documents
enum { SC_CURSOR = 0, SC_SAMPLES, SC_BATCHES, SC_SKIPPED, SC_CORRECT, SC_NONFINITE, SC_OVERFLOW, SC_SPARE };
enum { SS_LOSS = 0, SS_BETA, SS_NBETA, SS_SPARE };
#define STATS_MAX_THRESHOLDS 64
#define AUC_TILE 256

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One block of 256.  Launches are stream-ordered, so this block is the only writer of the cursor, the counters and the sums: no
// atomics.  Only the first nv = clamp(*n_valid, 1, B) samples are ever loaded (the ghosts of a short batch may hold NaN).
// SINGLE: labels are int64 class indices, nothing is logged, correct = the FIRST maximal logit's index equals the label
// (torch.argmax: a NaN counts as maximal).  Otherwise: targets are float [B, C], p = 1 / (1 + expf(-x)) and [target > 0] go to
// column cursor + b of the class-major log, correct = every label of the sample has [p > 0.5] == [target > 0].
template <bool SINGLE>
__global__ __launch_bounds__(256) void stats_update_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const long long* __restrict__ label, const float* __restrict__ loss,
                                                           float loss_scale, const float* __restrict__ beta, int bps,
                                                           const int* __restrict__ n_valid, int B, int C, int skip_nonfinite,
                                                           float* __restrict__ probs, unsigned char* __restrict__ truth, int capacity,
                                                           int* __restrict__ counters, double* __restrict__ sums) {
  __shared__ int red_i[2][4];
  __shared__ double red_d[4];
  const int nv = n_valid != nullptr ? min(max(n_valid[0], 1), B) : B;
  const float lv = loss[0];
  if (skip_nonfinite && !isfinite(lv)) {            // the MOSEI trainer's `continue`: the batch leaves no other trace
    if (threadIdx.x == 0) counters[SC_SKIPPED] += 1;
    return;
  }
  const int cursor = counters[SC_CURSOR];           // every thread reads it here; thread 0 writes it behind the last barrier
  const bool fits = SINGLE || (cursor >= 0 && (long)cursor + nv <= (long)capacity);
  int correct = 0, nonfinite = 0;
  for (int b = threadIdx.x; b < nv; b += 256) {
    const float* xr = x + (long)b * C;
    if (SINGLE) {
      int best = 0;
      float bv = xr[0];
      for (int c = 1; c < C; ++c) {
        const float v = xr[c];
        if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
      }
      correct += (long long)best == label[b] ? 1 : 0;
    } else {
      bool all = true;
      for (int c = 0; c < C; ++c) {
        const float xv = xr[c];
        const float p = 1.f / (1.f + expf(-xv));
        const bool t = y[(long)b * C + c] > 0.f;
        all = all && ((p > 0.5f) == t);
        if (fits) {
          const long at = (long)c * capacity + cursor + b;
          probs[at] = p;
          truth[at] = t ? 1 : 0;
          nonfinite += isfinite(xv) ? 0 : 1;
        }
      }
      correct += all ? 1 : 0;
    }
  }
  double bsum = 0.0;
  const int nb = beta != nullptr ? nv * bps : 0;
  for (int i = threadIdx.x; i < nb; i += 256) bsum += (double)beta[i];
  correct = wave_sum_i(correct);
  nonfinite = wave_sum_i(nonfinite);
  bsum = wave_sum_d(bsum);
  if ((threadIdx.x & 63) == 0) {
    red_i[0][threadIdx.x >> 6] = correct;
    red_i[1][threadIdx.x >> 6] = nonfinite;
    red_d[threadIdx.x >> 6] = bsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counters[SC_CORRECT] += (red_i[0][0] + red_i[0][1]) + (red_i[0][2] + red_i[0][3]);
    counters[SC_NONFINITE] += (red_i[1][0] + red_i[1][1]) + (red_i[1][2] + red_i[1][3]);
    counters[SC_SAMPLES] += nv;
    counters[SC_BATCHES] += 1;
    if (!SINGLE) {
      if (fits) counters[SC_CURSOR] = cursor + nv;
      else counters[SC_OVERFLOW] = 1;
    }
    sums[SS_LOSS] += (double)lv * (double)loss_scale * (double)nv;
    if (nb > 0) {
      sums[SS_BETA] += (red_d[0] + red_d[1]) + (red_d[2] + red_d[3]);
      sums[SS_NBETA] += (double)nb;
    }
  }
}

// counters[4] (int32) of one prediction log: the layout include/hriemo.h documents
enum { PL_CURSOR = 0, PL_SAMPLES, PL_OVERFLOW, PL_NONFINITE };

// One block of 256, the only writer of its log and counters (stream order): no atomics.  Only the first nv = clamp(*n_valid, 1, B)
// rows of x and beta are ever loaded.  KIND 0 (multi-label): one (sample, class) element per thread and trip, p = 1 / (1 + expf(-x))
// -- stats_update_kernel's expression, so both logs hold the same bits for equal logits.  KIND 1 (single-label): one sample per
// thread and trip; the first maximal logit's index (torch.argmax: a NaN counts as maximal) goes to pred, the fp32 softmax with that
// maximum subtracted (exp_below_max; the sum over the classes in index order) to the log.  beta_mean: one sample per thread, its bps values summed in index order in float64.
// exp(x - m) for x <= m with the difference carried exactly: d = fl(x - m) and its rounding error (TwoSum), exp(d + err) =
// exp(d) (1 + err) up to err^2 < 2^-34.  Plain expf(x - m) loses |x - m| * 2^-24 relative -- 30 to 60 ulp for a logit 80 below the
// row maximum.  x = -inf or an infinite difference: err is NaN and exp(d) (0, or NaN from NaN) stands.
__device__ __forceinline__ float exp_below_max(float x, float m) {
  const float d = x - m;
  const float t = d - x;
  const float err = (x - (d - t)) + (-m - t);
  const float e = expf(d);
  return err == err ? fmaf(e, err, e) : e;
}

template <int KIND>
__global__ __launch_bounds__(256) void predict_log_kernel(const float* __restrict__ x, const float* __restrict__ beta, int bps,
                                                          const int* __restrict__ n_valid, int B, int C, float* __restrict__ probs,
                                                          float* __restrict__ beta_mean, int* __restrict__ pred, int capacity,
                                                          int* __restrict__ counters) {
  __shared__ int red_i[4];
  const int nv = n_valid != nullptr ? min(max(n_valid[0], 1), B) : B;
  const int cursor = counters[PL_CURSOR];           // every thread reads it here; thread 0 writes it behind the barrier
  const bool fits = cursor >= 0 && (long)cursor + nv <= (long)capacity;
  int nonfinite = 0;
  if (fits) {
    if (KIND == 0) {
      const int n = nv * C;                         // B * C fits an int: the entry checks it
      for (int i = threadIdx.x; i < n; i += 256) {
        const int b = i / C, c = i - b * C;
        const float xv = x[i];
        probs[(long)c * capacity + cursor + b] = 1.f / (1.f + expf(-xv));
        nonfinite += isfinite(xv) ? 0 : 1;
      }
    } else {
      for (int b = threadIdx.x; b < nv; b += 256) {
        const float* xr = x + (long)b * C;
        int best = 0;
        float bv = xr[0];
        nonfinite += isfinite(bv) ? 0 : 1;
        for (int c = 1; c < C; ++c) {
          const float v = xr[c];
          nonfinite += isfinite(v) ? 0 : 1;
          if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
        }
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += exp_below_max(xr[c], bv);
        for (int c = 0; c < C; ++c) probs[(long)c * capacity + cursor + b] = exp_below_max(xr[c], bv) / s;
        if (pred != nullptr) pred[cursor + b] = best;
      }
    }
    if (beta != nullptr && beta_mean != nullptr) {
      for (int b = threadIdx.x; b < nv; b += 256) {
        const float* br = beta + (long)b * bps;
        double s = 0.0;
        for (int k = 0; k < bps; ++k) s += (double)br[k];
        beta_mean[cursor + b] = (float)(s / (double)bps);
      }
    }
  }
  nonfinite = wave_sum_i(nonfinite);
  if ((threadIdx.x & 63) == 0) red_i[threadIdx.x >> 6] = nonfinite;
  __syncthreads();
  if (threadIdx.x == 0) {
    counters[PL_SAMPLES] += nv;
    if (fits) {
      counters[PL_CURSOR] = cursor + nv;
      counters[PL_NONFINITE] += (red_i[0] + red_i[1]) + (red_i[2] + red_i[3]);
    } else {
      counters[PL_OVERFLOW] = 1;
    }
  }
}

// counters[4] (int32) of one attention log: the layout include/hriemo.h documents.  window[4] = {slot0, n_take, 0, 0}.
enum { AL_CURSOR = 0, AL_OFFERED, AL_BATCHES, AL_SPARE };

// One block of 256, recorded once per pass in front of every fork: the only writer of the cursor, the counters and the window
// (stream order), no atomics.  It decides which samples of the pass the export launches behind it log -- slots slot0 ..
// slot0 + n_take - 1 for samples 0 .. n_take - 1 -- and writes their lengths.  A full log takes nothing: the normal end state.
__global__ __launch_bounds__(256) void attn_log_plan_kernel(const int* __restrict__ lens, const int* __restrict__ n_valid, int B,
                                                            int capacity, int* __restrict__ counters, int* __restrict__ window,
                                                            int* __restrict__ lengths) {
  const int nv = n_valid != nullptr ? min(max(n_valid[0], 1), B) : B;
  const int cursor = counters[AL_CURSOR];           // every thread reads it here; thread 0 writes it behind the barrier
  const bool sane = cursor >= 0 && cursor <= capacity;          // anything else counts as full
  const int n_take = sane ? min(capacity - cursor, nv) : 0;
  if (lens != nullptr && lengths != nullptr)
    for (int b = threadIdx.x; b < n_take; b += 256) {
      lengths[(long)cursor + b] = lens[b];
      lengths[(long)capacity + cursor + b] = lens[(long)B + b];
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    window[0] = cursor;
    window[1] = n_take;
    window[2] = 0;
    window[3] = 0;
    if (n_take > 0) counters[AL_CURSOR] = cursor + n_take;
    counters[AL_OFFERED] += nv;
    counters[AL_BATCHES] += 1;
  }
}

// the closed window of a pass that must leave no trace (warm-up): {0, 0, 0, 0}, nothing else touched
__global__ __launch_bounds__(64) void attn_log_close_kernel(int* __restrict__ window) {
  if (threadIdx.x < 4) window[threadIdx.x] = 0;
}

// The window rule as a plain copy: maps [B, map_elems] fp32 -> log[slot0 + b] for the samples inside the window.  Grid (chunks, B);
// a block whose sample lies outside the window returns before it touches anything; the capacity is a launch argument.
__global__ __launch_bounds__(256) void attn_log_append_kernel(const float* __restrict__ maps, int map_elems, const int* __restrict__ window,
                                                              float* __restrict__ log, int capacity) {
  const int b = blockIdx.y;
  const int slot0 = window[0], n_take = window[1];
  if (b >= n_take || slot0 < 0 || (long)slot0 + b >= (long)capacity) return;
  const float* src = maps + (long)b * map_elems;
  float* dst = log + ((long)slot0 + b) * map_elems;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < map_elems; e += gridDim.x * 256) dst[e] = src[e];
}

// tp / fp / fn of `p >= thr[s]` per class and threshold over the first n = clamp(cursor, 0, capacity) log entries.  Grid
// (ceil(capacity / 256), C): one entry per thread, blocks past the cursor exit; a block adds its S * 3 integers to out[C, S, 3]
// (zeroed by the entry in front of the launch) with integer atomics -- integer sums do not depend on the order.
__global__ __launch_bounds__(256) void stats_counts_kernel(const float* __restrict__ probs, const unsigned char* __restrict__ truth,
                                                           int capacity, const int* __restrict__ counters, const float* __restrict__ thr,
                                                           int S, int* __restrict__ out) {
  __shared__ int acc[STATS_MAX_THRESHOLDS * 3];
  const int n = min(max(counters[SC_CURSOR], 0), capacity);
  if ((int)blockIdx.x * 256 >= n) return;
  const int c = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < n;
  const float p = valid ? probs[(long)c * capacity + i] : 0.f;
  const bool t = valid && truth[(long)c * capacity + i] != 0;
  for (int k = threadIdx.x; k < S * 3; k += 256) acc[k] = 0;
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const bool pred = valid && p >= thr[s];
    const int tp = __popcll(__ballot(pred && t));
    const int fp = __popcll(__ballot(pred && !t));
    const int fn = __popcll(__ballot(valid && !pred && t));
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&acc[s * 3 + 0], tp);
      atomicAdd(&acc[s * 3 + 1], fp);
      atomicAdd(&acc[s * 3 + 2], fn);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < S * 3; k += 256)
    if (acc[k] != 0) atomicAdd(&out[(long)c * S * 3 + k], acc[k]);
}

// Mann-Whitney count of one class, twice over so that a tie is an integer: 2 U = sum over (positive i, negative j) of
// 2 [p_i > p_j] + [p_i == p_j].  Grid (ceil(capacity / 256), C): a block owns 256 rows i and walks every j through LDS, 256 at a
// time; an entry that is no negative (a positive, or past the cursor) is staged as NaN, against which both comparisons are false.
// uint32 per thread (<= 2 * capacity), uint64 per block, ONE ordinary store per (class, tile): partial[C, tiles].  A tile past the
// cursor stores 0.  Tile 0 of every class also stores the class's n_pos, n_neg to npn[C, 2].
__global__ __launch_bounds__(256) void stats_auc_kernel(const float* __restrict__ probs, const unsigned char* __restrict__ truth,
                                                        int capacity, const int* __restrict__ counters,
                                                        unsigned long long* __restrict__ partial, int* __restrict__ npn) {
  __shared__ float pj[AUC_TILE];
  __shared__ unsigned long long red[4];
  __shared__ int red_n[2][4];
  const int n = min(max(counters[SC_CURSOR], 0), capacity);
  const int c = blockIdx.y, tiles = gridDim.x;
  if ((int)blockIdx.x * AUC_TILE >= n && blockIdx.x != 0) {
    if (threadIdx.x == 0) partial[(long)c * tiles + blockIdx.x] = 0ull;
    return;
  }
  const float* pc = probs + (long)c * capacity;
  const unsigned char* tc = truth + (long)c * capacity;
  const int i = blockIdx.x * AUC_TILE + threadIdx.x;
  const bool pos_i = i < n && tc[i] != 0;
  const float pi = pos_i ? pc[i] : 0.f;
  unsigned int cnt = 0;
  int n_pos = 0, n_neg = 0;
  for (int j0 = 0; j0 < n; j0 += AUC_TILE) {
    const int j = j0 + threadIdx.x;
    const bool in = j < n;
    const bool tj = in && tc[j] != 0;
    n_pos += tj ? 1 : 0;
    n_neg += (in && !tj) ? 1 : 0;
    __syncthreads();                                 // the previous chunk has been read
    pj[threadIdx.x] = (in && !tj) ? pc[j] : __builtin_nanf("");
    __syncthreads();
    if (pos_i) {
      const int m = min(AUC_TILE, n - j0);
      for (int k = 0; k < m; ++k) {
        const float q = pj[k];
        cnt += (pi > q ? 2u : 0u) + (pi == q ? 1u : 0u);
      }
    }
  }
  unsigned long long s = wave_sum_u64((unsigned long long)cnt);
  n_pos = wave_sum_i(n_pos);
  n_neg = wave_sum_i(n_neg);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = s;
    red_n[0][threadIdx.x >> 6] = n_pos;
    red_n[1][threadIdx.x >> 6] = n_neg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[(long)c * tiles + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (blockIdx.x == 0) {
      npn[c * 2 + 0] = (red_n[0][0] + red_n[0][1]) + (red_n[0][2] + red_n[0][3]);
      npn[c * 2 + 1] = (red_n[1][0] + red_n[1][1]) + (red_n[1][2] + red_n[1][3]);
    }
  }
}

// The ranks of one class: for entry i < n, rank[c, 0, i] = #{j < n : truth_j != 0, p_j >= p_i} and rank[c, 1, i] the same over
// truth_j == 0 (entry i counts itself in its own plane).  Grid (ceil(capacity / 256), C): a thread owns entry i, the block walks
// every j through LDS 256 at a time as stats_auc_kernel does -- the positives in one array, the negatives in the other, NaN where
// the entry is of the other kind (both comparisons with NaN are false; a NaN p_i gets 0 / 0).  Entries at or past the cursor are
// never read.  Two uint32 per thread (<= capacity), ordinary stores of the thread's own two results, no atomics; elements at or
// past n are stored as 0, so every element of rank is written by every launch.  A block wholly past the cursor stores its zeros
// and leaves before the first barrier.
__global__ __launch_bounds__(256) void stats_rank_kernel(const float* __restrict__ probs, const unsigned char* __restrict__ truth,
                                                         int capacity, const int* __restrict__ counters, int* __restrict__ rank) {
  __shared__ float qp[AUC_TILE];
  __shared__ float qn[AUC_TILE];
  const int n = min(max(counters[SC_CURSOR], 0), capacity);
  const int c = blockIdx.y;
  const int i = blockIdx.x * AUC_TILE + threadIdx.x;
  int* r_pos = rank + (long)c * 2 * capacity;
  int* r_neg = r_pos + capacity;
  if ((int)blockIdx.x * AUC_TILE >= n) {
    if (i < capacity) {
      r_pos[i] = 0;
      r_neg[i] = 0;
    }
    return;
  }
  const float* pc = probs + (long)c * capacity;
  const unsigned char* tc = truth + (long)c * capacity;
  const float pi = i < n ? pc[i] : __builtin_nanf("");
  unsigned int ge_pos = 0, ge_neg = 0;
  for (int j0 = 0; j0 < n; j0 += AUC_TILE) {
    const int j = j0 + threadIdx.x;
    float vp = __builtin_nanf(""), vn = __builtin_nanf("");
    if (j < n) {
      const float v = pc[j];
      if (tc[j] != 0) vp = v;
      else vn = v;
    }
    __syncthreads();                                 // the previous chunk has been read
    qp[threadIdx.x] = vp;
    qn[threadIdx.x] = vn;
    __syncthreads();
    const int m = min(AUC_TILE, n - j0);
    for (int k = 0; k < m; ++k) {
      ge_pos += qp[k] >= pi ? 1u : 0u;
      ge_neg += qn[k] >= pi ? 1u : 0u;
    }
  }
  if (i < capacity) {
    r_pos[i] = i < n ? (int)ge_pos : 0;
    r_neg[i] = i < n ? (int)ge_neg : 0;
  }
}

// cm[C * C + 2] (int32) of one epoch: the confusion matrix, rows = label, columns = prediction, then {n_ignored, n_bad}
#define CONFUSION_MAX_CLASSES 64
#define CONFUSION_IGNORE (-100LL)

// One block of 256 behind stats_update_kernel<true> of the same step: the only writer of cm (stream order), so the final adds are
// ordinary read-modify-writes by one thread per cell.  The same nv, the same skip on a non-finite loss, the same first-maximum
// rule (a NaN counts as maximal).  The block's counts are formed in LDS with integer atomics -- integer sums do not depend on the
// order -- and then added to cm in cell order.  A label outside [0, C) indexes nothing: -100 (the criterion's ignore_index) counts
// in cm[C * C], anything else in cm[C * C + 1].
__global__ __launch_bounds__(256) void stats_confusion_kernel(const float* __restrict__ x, const long long* __restrict__ label,
                                                              const float* __restrict__ loss, int skip_nonfinite,
                                                              const int* __restrict__ n_valid, int B, int C, int* __restrict__ cm) {
  __shared__ int acc[CONFUSION_MAX_CLASSES * CONFUSION_MAX_CLASSES + 2];
  if (skip_nonfinite && !isfinite(loss[0])) return;  // block-uniform: in front of every barrier
  const int nv = n_valid != nullptr ? min(max(n_valid[0], 1), B) : B;
  const int cells = C * C + 2;
  for (int k = threadIdx.x; k < cells; k += 256) acc[k] = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < nv; b += 256) {
    const float* xr = x + (long)b * C;
    int best = 0;
    float bv = xr[0];
    for (int c = 1; c < C; ++c) {
      const float v = xr[c];
      if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }
    }
    const long long lab = label[b];
    const int cell = (lab >= 0 && lab < (long long)C) ? (int)lab * C + best : (lab == CONFUSION_IGNORE ? C * C : C * C + 1);
    atomicAdd(&acc[cell], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < cells; k += 256)
    if (acc[k] != 0) cm[k] += acc[k];
}

extern "C" int hriemo_stats_update(const float* logits, const float* targets, const long long* labels, const float* loss, float loss_scale,
                                   const float* beta, int beta_per_sample, const int* n_valid, int B, int C, int skip_nonfinite,
                                   float* probs, unsigned char* truth, int capacity, int* counters, double* sums, hipStream_t st) {
  HRIEMO_CHECK(B > 0 && C > 0 && logits != nullptr && loss != nullptr && counters != nullptr && sums != nullptr, "stats_update: bad arguments");
  HRIEMO_CHECK((targets != nullptr) != (labels != nullptr), "stats_update: float targets [B, C] (multi-label) or int64 labels [B] (single-label), not both");
  HRIEMO_CHECK(beta == nullptr || beta_per_sample >= 1, "stats_update: beta_per_sample %d", beta_per_sample);
  HRIEMO_CHECK(n_valid == nullptr || ((uintptr_t)n_valid % 4) == 0, "stats_update: n_valid is one aligned int32 in device memory");
  HRIEMO_CHECK(((uintptr_t)counters % 4) == 0 && ((uintptr_t)sums % 8) == 0, "stats_update: counters / sums are not aligned");
  if (labels != nullptr) {
    hipLaunchKernelGGL(stats_update_kernel<true>, dim3(1), dim3(256), 0, st, logits, targets, labels, loss, loss_scale, beta, beta_per_sample,
                       n_valid, B, C, skip_nonfinite, probs, truth, capacity, counters, sums);
  } else {
    HRIEMO_CHECK(probs != nullptr && truth != nullptr && capacity > 0, "stats_update: the multi-label kind needs the log (probs, truth, capacity > 0)");
    hipLaunchKernelGGL(stats_update_kernel<false>, dim3(1), dim3(256), 0, st, logits, targets, labels, loss, loss_scale, beta, beta_per_sample,
                       n_valid, B, C, skip_nonfinite, probs, truth, capacity, counters, sums);
  }
  HRIEMO_LAUNCH_CHECK("stats_update_kernel");
  return 0;
}

extern "C" int hriemo_predict_log(const float* logits, const float* beta, int beta_per_sample, const int* n_valid, int B, int C, int kind,
                                  float* probs, float* beta_mean, int* pred, int capacity, int* counters, hipStream_t st) {
  HRIEMO_CHECK(B >= 1 && C >= 1 && capacity >= 1, "predict_log: B = %d, C = %d, capacity = %d (all >= 1)", B, C, capacity);
  HRIEMO_CHECK((long)B * C <= 0x7fffffffL, "predict_log: B * C = %ld does not fit an int", (long)B * C);
  HRIEMO_CHECK(kind == 0 || kind == 1, "predict_log: kind %d (0 multi-label, 1 single-label)", kind);
  HRIEMO_CHECK(logits != nullptr && probs != nullptr && counters != nullptr, "predict_log: logits, probs and counters are required");
  HRIEMO_CHECK(beta == nullptr || beta_per_sample >= 1, "predict_log: beta_per_sample %d", beta_per_sample);
  HRIEMO_CHECK(n_valid == nullptr || ((uintptr_t)n_valid % 4) == 0, "predict_log: n_valid is one aligned int32 in device memory");
  HRIEMO_CHECK(((uintptr_t)counters % 4) == 0 && ((uintptr_t)pred % 4) == 0, "predict_log: counters / pred are not aligned");
  if (kind == 0) {
    hipLaunchKernelGGL(predict_log_kernel<0>, dim3(1), dim3(256), 0, st, logits, beta, beta_per_sample, n_valid, B, C, probs, beta_mean, pred,
                       capacity, counters);
  } else {
    hipLaunchKernelGGL(predict_log_kernel<1>, dim3(1), dim3(256), 0, st, logits, beta, beta_per_sample, n_valid, B, C, probs, beta_mean, pred,
                       capacity, counters);
  }
  HRIEMO_LAUNCH_CHECK("predict_log_kernel");
  return 0;
}

extern "C" int hriemo_attn_log_plan(const int* lens, const int* n_valid, int B, int capacity, int* counters, int* window, int* lengths,
                                    hipStream_t st) {
  HRIEMO_CHECK(B >= 1 && capacity >= 1, "attn_log_plan: B = %d, capacity = %d (both >= 1)", B, capacity);
  HRIEMO_CHECK(counters != nullptr && window != nullptr, "attn_log_plan: counters and window are required");
  HRIEMO_CHECK((lens == nullptr) == (lengths == nullptr), "attn_log_plan: the lengths block [2, B] and the logged lengths [2, capacity] come together");
  HRIEMO_CHECK(((uintptr_t)counters % 4) == 0 && ((uintptr_t)window % 4) == 0 && ((uintptr_t)lens % 4) == 0 && ((uintptr_t)lengths % 4) == 0 &&
                   ((uintptr_t)n_valid % 4) == 0, "attn_log_plan: an int32 operand is not 4-byte aligned");
  hipLaunchKernelGGL(attn_log_plan_kernel, dim3(1), dim3(256), 0, st, lens, n_valid, B, capacity, counters, window, lengths);
  HRIEMO_LAUNCH_CHECK("attn_log_plan_kernel");
  return 0;
}

extern "C" int hriemo_attn_log_close(int* window, hipStream_t st) {
  HRIEMO_CHECK(window != nullptr && ((uintptr_t)window % 4) == 0, "attn_log_close: window is int32[4] in device memory, 4-byte aligned");
  hipLaunchKernelGGL(attn_log_close_kernel, dim3(1), dim3(64), 0, st, window);
  HRIEMO_LAUNCH_CHECK("attn_log_close_kernel");
  return 0;
}

extern "C" int hriemo_attn_log_append(const float* maps, int B, int map_elems, const int* window, float* log, int capacity, hipStream_t st) {
  HRIEMO_CHECK(B >= 1 && B <= 65535 && map_elems >= 1 && capacity >= 1, "attn_log_append: B = %d (1 .. 65535), map_elems = %d, capacity = %d (>= 1)",
               B, map_elems, capacity);
  HRIEMO_CHECK(maps != nullptr && window != nullptr && log != nullptr, "attn_log_append: maps, window and log are required");
  HRIEMO_CHECK(((uintptr_t)maps % 4) == 0 && ((uintptr_t)log % 4) == 0 && ((uintptr_t)window % 4) == 0, "attn_log_append: an operand is not 4-byte aligned");
  const int chunks = (map_elems + 255) / 256;
  hipLaunchKernelGGL(attn_log_append_kernel, dim3(chunks < 64 ? chunks : 64, B), dim3(256), 0, st, maps, map_elems, window, log, capacity);
  HRIEMO_LAUNCH_CHECK("attn_log_append_kernel");
  return 0;
}

extern "C" int hriemo_stats_counts(const float* probs, const unsigned char* truth, int capacity, int C, const int* counters,
                                   const float* thresholds, int S, int* out, hipStream_t st) {
  HRIEMO_CHECK(probs != nullptr && truth != nullptr && counters != nullptr && thresholds != nullptr && out != nullptr && capacity > 0 && C > 0,
               "stats_counts: bad arguments");
  HRIEMO_CHECK(S >= 1 && S <= STATS_MAX_THRESHOLDS, "stats_counts: %d thresholds (1 .. %d)", S, STATS_MAX_THRESHOLDS);
  HRIEMO_CHECK(C <= 65535, "stats_counts: %d classes", C);
  hipError_t e = hipMemsetAsync(out, 0, (size_t)C * S * 3 * sizeof(int), st);
  HRIEMO_CHECK(e == hipSuccess, "stats_counts: memset failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(stats_counts_kernel, dim3((capacity + 255) / 256, C), dim3(256), 0, st, probs, truth, capacity, counters, thresholds, S, out);
  HRIEMO_LAUNCH_CHECK("stats_counts_kernel");
  return 0;
}

extern "C" int hriemo_stats_auc_tiles(int capacity) { return capacity > 0 ? (capacity + AUC_TILE - 1) / AUC_TILE : 0; }

extern "C" int hriemo_stats_auc(const float* probs, const unsigned char* truth, int capacity, int C, const int* counters,
                                unsigned long long* partial, int* npn, hipStream_t st) {
  HRIEMO_CHECK(probs != nullptr && truth != nullptr && counters != nullptr && partial != nullptr && npn != nullptr && capacity > 0 && C > 0,
               "stats_auc: bad arguments");
  HRIEMO_CHECK(C <= 65535 && ((uintptr_t)partial % 8) == 0, "stats_auc: %d classes / partial not 8-byte aligned", C);
  hipLaunchKernelGGL(stats_auc_kernel, dim3(hriemo_stats_auc_tiles(capacity), C), dim3(256), 0, st, probs, truth, capacity, counters, partial, npn);
  HRIEMO_LAUNCH_CHECK("stats_auc_kernel");
  return 0;
}

extern "C" int hriemo_stats_rank(const float* probs, const unsigned char* truth, int capacity, int C, const int* counters, int* rank,
                                 hipStream_t st) {
  HRIEMO_CHECK(capacity >= 1 && C >= 1 && C <= 65535, "stats_rank: capacity = %d (>= 1), C = %d (1 .. 65535)", capacity, C);
  HRIEMO_CHECK(probs != nullptr && truth != nullptr && counters != nullptr && rank != nullptr, "stats_rank: probs, truth, counters and rank are required");
  HRIEMO_CHECK(((uintptr_t)counters % 4) == 0 && ((uintptr_t)rank % 4) == 0 && ((uintptr_t)probs % 4) == 0,
               "stats_rank: probs / counters / rank are not 4-byte aligned");
  hipLaunchKernelGGL(stats_rank_kernel, dim3((capacity + AUC_TILE - 1) / AUC_TILE, C), dim3(256), 0, st, probs, truth, capacity, counters, rank);
  HRIEMO_LAUNCH_CHECK("stats_rank_kernel");
  return 0;
}

extern "C" int hriemo_stats_confusion(const float* logits, const long long* labels, const float* loss, int skip_nonfinite,
                                      const int* n_valid, int B, int C, int* cm, hipStream_t st) {
  HRIEMO_CHECK(B >= 1 && C >= 1 && C <= CONFUSION_MAX_CLASSES, "stats_confusion: B = %d (>= 1), C = %d (1 .. %d)", B, C, CONFUSION_MAX_CLASSES);
  HRIEMO_CHECK(logits != nullptr && labels != nullptr && loss != nullptr && cm != nullptr, "stats_confusion: logits, labels, loss and cm are required");
  HRIEMO_CHECK(((uintptr_t)n_valid % 4) == 0 && ((uintptr_t)cm % 4) == 0, "stats_confusion: n_valid / cm are not 4-byte aligned");
  hipLaunchKernelGGL(stats_confusion_kernel, dim3(1), dim3(256), 0, st, logits, labels, loss, skip_nonfinite, n_valid, B, C, cm);
  HRIEMO_LAUNCH_CHECK("stats_confusion_kernel");
  return 0;
}
