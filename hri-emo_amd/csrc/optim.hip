// Device-state AdamW (hri-emo_amd/optim.py: DeviceAdamW): clip_grad_norm_ + torch.optim.AdamW with EVERY scalar of the update in
// device memory, so the whole optimizer step can be recorded into the hipGraph of the trainer step and still follow a learning-
// rate schedule, a GradScaler and its own step count (scripts/fusion/train_mosei_fusion_seq_level_decoder.py:367-402, 564-584).
//   hyper[8]  written by the host:   lr, beta1, beta2, eps, weight_decay, max_norm (<= 0: no clipping), 2 spare words
//   state[8]  written by the device: step, skip, coef, step_size = lr / bc1, 1 / sqrt(bc2), decay = 1 - lr * wd,
//                                    grad_norm (pre-clip, unscaled), skipped (number of skipped steps)
// A step is hriemo_sumsq_f32 (rowops.hip) -> hriemo_optim_finalize (one block) -> hriemo_adamw_flat_dev (streaming).
// Gradient accumulation inside a captured step (dp.capture_packed(grad_accum=k)) adds the step-control block
//   ctl[4]    written by the host (int32): n_valid (read by the masked losses, loss.hip), first, last, one spare word
// hriemo_grad_begin zeroes the flat gradient buffer when ctl.first is set and leaves every bit of it in place otherwise;
// hriemo_optim_finalize_ctl holds the update (state.skip = 1, nothing else) on every micro-step but the one with ctl.last set.
// Parameter groups (DeviceAdamW(param_groups=...)): hyper[G][8] and state[G][8], one row per group, and a segment table over the
// flat buffer that says which group owns which elements.  Row 0 of state keeps the meaning above word for word (one norm, one clip
// coefficient, one skip decision, one step count for all groups); rows g >= 1 carry step_size, 1 / sqrt(bc2) and decay of their
// group (words 3, 4, 5) and nothing else.  max_norm is read from row 0 of hyper.  A step is hriemo_sumsq_f32 ->
// hriemo_optim_finalize_groups (one block) -> hriemo_adamw_flat_groups (streaming): three launches, as with one group.
// Weight averaging (DeviceAdamW(averaging="ema" | "swa")): torch.optim.swa_utils.AveragedModel's average as one more streaming
// operand of the update, `avg`, a flat fp32 buffer laid out like p.  Two more blocks, outside hyper[] / state[]:
//   avg_hyper[4]  written by the host:   mode (0 off, 1 ema, 2 swa), decay, start, every
//   avg_state[4]  written by the device: n_averaged, w (this update's weight), flag (0 none, 1 averaging update, 2 first
//                                        averaging update: avg = p), stamp (the step count the flag belongs to)
// A step is hriemo_sumsq_f32 -> hriemo_optim_finalize_avg (one block; G groups, ctl or none: the one finalize of all three forms)
// -> hriemo_adamw_flat_dev_avg or hriemo_adamw_flat_groups_avg: three launches.  With t the step count of a real update (neither
// skipped nor held), the update averages iff t > start and (t - start) % every == 0; the finalize then writes
// w = 1 - decay (ema) or 1 / (n + 1) (swa), n += 1, flag and stamp = t, once, in fp32; a real update that does not average writes
// flag = 0 and stamp = t and leaves n and w alone; a skipped or held step writes NO word of avg_state.
// How the update kernel tells "this step averages" from a stale flag: (1) a skipped or held step returns on state.skip before it
// reads avg_state at all, and every real update rewrites flag; (2) the flag only counts when stamp == state.step, so a flag left by
// an earlier step -- the state block advanced by a finalize that knows nothing of averaging, a loaded checkpoint -- is not an
// update.  On a step that does not average, avg is neither loaded nor stored.
// hriemo_swap_fp32 exchanges two flat fp32 buffers bit for bit (DeviceAdamW.averaged_weights(): evaluation on the average).
// Clip units (DeviceAdamW(clip="group" | "parameter")): every param group, or every parameter tensor, is clipped by its own norm
// against its group's max_norm (hyper[g][HY_MAX_NORM] of every row).  A step is hriemo_sumsq_units -> hriemo_optim_finalize_units
// -> hriemo_adamw_flat_units(_avg): three launches; the tables and clip_state[U][2] are described at the launchers below.
#include "common.h"

enum { HY_LR = 0, HY_BETA1, HY_BETA2, HY_EPS, HY_WD, HY_MAX_NORM };
enum { ST_STEP = 0, ST_SKIP, ST_COEF, ST_STEP_SIZE, ST_ISB2, ST_DECAY, ST_GRAD_NORM, ST_SKIPPED };
enum { CTL_N_VALID = 0, CTL_FIRST, CTL_LAST };
enum { AG_MAX_GROUPS = 16, AG_MAX_SEGS = 2048 };
enum { AH_MODE = 0, AH_DECAY, AH_START, AH_EVERY };
enum { AS_N = 0, AS_W, AS_FLAG, AS_STAMP };
enum { AV_NONE = 0, AV_UPDATE = 1, AV_FIRST = 2, AV_EMA = 1, AV_SWA = 2 };

// One block.  Sums the sumsq_f32 partials in a fixed order (deterministic), forms the unscaled gradient norm, decides whether
// the step is skipped (GradScaler found an inf / the norm is not finite: torch's GradScaler.step and the reference trainer's
// NaN guard, without the host reading anything back) and leaves every per-step scalar of the update in state[]: the only
// powf of the optimizer runs here, once, not per element.
// HOLD (hriemo_optim_finalize_ctl): a micro-step of an accumulation group that is not its last one (ctl.last == 0) sets
// state.skip so that adamw_flat_dev_kernel returns early, and touches nothing else: step, skipped and grad_norm stay those of the last
// real step -- a held micro-step is not a skipped step.  With ctl.last != 0 the kernel runs the instructions of the plain one.
template <bool HOLD>
__global__ __launch_bounds__(256) void optim_finalize_kernel(const float* __restrict__ partial, int nblocks, const float* __restrict__ hyper,
                                                             const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                             float* __restrict__ state, const int* __restrict__ ctl) {
  __shared__ float red[4];
  if (HOLD && ctl[CTL_LAST] == 0) {                // block-uniform: nobody reaches the barrier below
    if (threadIdx.x == 0) state[ST_SKIP] = 1.f;
    return;
  }
  float s = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float sum = red[0] + red[1] + red[2] + red[3];
  const float gs = grad_scale != nullptr ? grad_scale[0] : 1.f;
  const float norm = sqrtf(sum) / gs;
  const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
  const bool skip = !finite || (found_inf != nullptr && !(found_inf[0] == 0.f));
  state[ST_GRAD_NORM] = norm;
  if (skip) {
    state[ST_SKIP] = 1.f;
    state[ST_SKIPPED] += 1.f;
    return;
  }
  const float lr = hyper[HY_LR], b1 = hyper[HY_BETA1], b2 = hyper[HY_BETA2], wd = hyper[HY_WD], max_norm = hyper[HY_MAX_NORM];
  const float step = state[ST_STEP] + 1.f;
  const float bc1 = 1.f - powf(b1, step), bc2 = 1.f - powf(b2, step);
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(1.f, max_norm / (norm + 1e-6f));
  state[ST_STEP] = step;
  state[ST_SKIP] = 0.f;
  state[ST_COEF] = coef / gs;
  state[ST_STEP_SIZE] = lr / bc1;
  state[ST_ISB2] = 1.f / sqrtf(bc2);
  state[ST_DECAY] = 1.f - lr * wd;
}

// One 16-byte vector of the update: torch.optim.AdamW's arithmetic on the clipped, unscaled gradient coef * g.  The ONE place the
// per-element arithmetic of the device-state optimizer lives: adamw_flat_dev_kernel and adamw_flat_groups_kernel both call it, so
// a group's elements get, bit for bit, what the single-group kernel gives them under that group's scalars.  Returns the new p
// vector (the averaging forms fold it into avg without reading it back).
struct AdamScalars { float b1, b2, eps, coef, step, isb2, decay; };

__device__ __forceinline__ f32x4 adamw_vec4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           long i, const AdamScalars& s) {
  const float b1 = s.b1, b2 = s.b2, eps = s.eps, coef = s.coef, step = s.step, isb2 = s.isb2, decay = s.decay;
  f32x4 pp = *(const f32x4*)(p + i * 4), mm = *(const f32x4*)(m + i * 4), vv = *(const f32x4*)(v + i * 4);
  const f32x4 gg = *(const f32x4*)(g + i * 4) * coef;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    pp[e] *= decay;
    mm[e] += (gg[e] - mm[e]) * (1.f - b1);
    vv[e] = vv[e] * b2 + gg[e] * gg[e] * (1.f - b2);
    pp[e] -= step * mm[e] / (sqrtf(vv[e]) * isb2 + eps);
  }
  *(f32x4*)(p + i * 4) = pp; *(f32x4*)(m + i * 4) = mm; *(f32x4*)(v + i * 4) = vv;
  return pp;
}

// What this step does to avg, read once per block behind the skip test: AV_NONE unless the finalize of THIS step (stamp ==
// state.step) flagged an averaging update.  Block-uniform (scalar loads), so the branches on it in the sweep are uniform too.
struct AvgStep { int kind; float w; };

__device__ __forceinline__ AvgStep avg_step(const float* __restrict__ state, const float* __restrict__ avg_state) {
  const float flag = avg_state[AS_FLAG];
  AvgStep a = {AV_NONE, 0.f};
  if (avg_state[AS_STAMP] == state[ST_STEP] && (flag == (float)AV_UPDATE || flag == (float)AV_FIRST)) {
    a.kind = flag == (float)AV_FIRST ? AV_FIRST : AV_UPDATE;
    a.w = avg_state[AS_W];
  }
  return a;
}

// One 16-byte vector of the average from the freshly updated p vector: the first averaging update copies the bits of p (torch's
// first AveragedModel.update_parameters), a later one is avg += w * (p - avg) with one rounding of the difference and one of the fma.
__device__ __forceinline__ void avg_vec4(float* __restrict__ avg, long i, const f32x4 pp, const AvgStep a) {
  if (a.kind == AV_FIRST) {
    *(f32x4*)(avg + i * 4) = pp;
    return;
  }
  f32x4 aa = *(const f32x4*)(avg + i * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) aa[e] = __builtin_fmaf(a.w, pp[e] - aa[e], aa[e]);
  *(f32x4*)(avg + i * 4) = aa;
}

// adamw_flat_kernel (rowops.hip) with its scalars read from hyper[] / state[].  A skipped step returns before it touches p, m or v.
// AVG: the averaging form (hriemo_adamw_flat_dev_avg) -- the same sweep, avg_vec4 behind adamw_vec4 on an averaging update and
// neither a load nor a store of avg on any other step; AVG = false is the kernel of before, avg and avg_state unused.
template <bool AVG>
__device__ __forceinline__ void adamw_flat_dev_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, const float* __restrict__ hyper,
                                                    const float* __restrict__ state, float* __restrict__ avg,
                                                    const float* __restrict__ avg_state) {
  if (state[ST_SKIP] != 0.f) return;
  const AdamScalars s = {hyper[HY_BETA1], hyper[HY_BETA2], hyper[HY_EPS], state[ST_COEF], state[ST_STEP_SIZE], state[ST_ISB2], state[ST_DECAY]};
  const long nv = n >> 2;
  if (AVG) {
    const AvgStep a = avg_step(state, avg_state);
    if (a.kind != AV_NONE) {
      for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) avg_vec4(avg, i, adamw_vec4(p, g, m, v, i, s), a);
      return;
    }
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) adamw_vec4(p, g, m, v, i, s);
}

__global__ __launch_bounds__(256) void adamw_flat_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, long n, const float* __restrict__ hyper,
                                                             const float* __restrict__ state) {
  adamw_flat_dev_body<false>(p, g, m, v, n, hyper, state, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void adamw_flat_dev_avg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, long n, const float* __restrict__ hyper,
                                                                 const float* __restrict__ state, float* __restrict__ avg,
                                                                 const float* __restrict__ avg_state) {
  adamw_flat_dev_body<true>(p, g, m, v, n, hyper, state, avg, avg_state);
}

// optim_finalize_kernel for G parameter groups.  One norm over the whole flat buffer, one clip coefficient, one skip decision, one
// step count and one `skipped` counter, all in row 0 of state exactly as optim_finalize_kernel leaves them (G = 1: the same bits
// in all 8 words); thread g < G then writes its group's step_size = lr_g / bc1_g, 1 / sqrt(bc2_g) and decay_g = 1 - lr_g * wd_g
// into row g, each from that group's own lr, betas and weight decay.  Rows g >= 1: words 3, 4, 5 and nothing else.
// ctl == nullptr: the plain finalize; otherwise the HOLD of optim_finalize_kernel<true> (ctl.last == 0: state[0][ST_SKIP] = 1, nothing else).
// AVG: the averaging finalize (hriemo_optim_finalize_avg): thread 0 of a REAL update also writes avg_state -- the decision of the
// header comment, w once per step in fp32 -- behind the words of state; a held or skipped step returns in front of it and writes
// no word of avg_state.  AVG = false is the kernel of before, avg_hyper and avg_state unused.
// UNITS: the finalize of the unit clip modes (hriemo_optim_finalize_units).  partial then holds ONE sum of squares per chunk of
// hriemo_sumsq_units (nblocks = C) and units describes the U clip units; the global sum is the fixed-order sum of the unit sums,
// every unit gets its own norm and coefficient in clip_state, and row 0's coef is the smallest of them.  UNITS = false is the
// kernel of before, units unused.
struct ClipUnits {
  const int* __restrict__ unit_chunks;             // [U + 1] ascending chunk ranges: unit u owns partial[unit_chunks[u] .. unit_chunks[u + 1])
  const int* __restrict__ unit_group;              // [U] the group whose max_norm clips unit u
  int U;
  float* __restrict__ clip_state;                  // [U][2] norm_u, coef_u
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

template <bool AVG, bool UNITS>
__device__ __forceinline__ void optim_finalize_groups_body(const float* __restrict__ partial, int nblocks, const float* __restrict__ hyper,
                                                           int G, const float* __restrict__ grad_scale,
                                                           const float* __restrict__ found_inf, float* __restrict__ state,
                                                           const int* __restrict__ ctl, const float* __restrict__ avg_hyper,
                                                           float* __restrict__ avg_state, const ClipUnits units) {
  __shared__ float red[4];
  extern __shared__ float unit_sum[];              // [U] (UNITS)
  if (ctl != nullptr && ctl[CTL_LAST] == 0) {      // block-uniform: nobody reaches the barrier below
    if (threadIdx.x == 0) state[ST_SKIP] = 1.f;
    return;
  }
  const float step = state[ST_STEP] + 1.f;         // read by every thread in front of the barrier, written by thread 0 behind it
  if (UNITS) {
    // one wave per unit: lane l adds partials c0 + l, c0 + l + 64, ... in ascending order, then the xor butterfly -- an order that
    // the chunk table fixes and no launch parameter changes.  A range is clamped into [0, C]: it selects partials, nothing else.
    // A wave takes UF units at a time so that their loads and butterflies are in flight together: this block is the step's serial
    // chain, and one global round trip per unit (119 units at cfg 2 in parameter mode) would be what it costs.
    constexpr int UF = 8, UW = 8;
    const int lane = threadIdx.x & 63;
    for (int u0 = (threadIdx.x >> 6) * UF; u0 < units.U; u0 += 4 * UF) {
      int c1[UF], c[UF];
      float a[UF];
#pragma unroll
      for (int k = 0; k < UF; ++k) {
        const int u = u0 + k < units.U ? u0 + k : units.U - 1;           // past the end: the last unit again, never stored
        int lo = units.unit_chunks[u], hi = units.unit_chunks[u + 1];
        lo = lo < 0 ? 0 : (lo > nblocks ? nblocks : lo);
        hi = hi < lo ? lo : (hi > nblocks ? nblocks : hi);
        c[k] = lo + lane; c1[k] = hi;
      }
#pragma unroll
      for (int k = 0; k < UF; ++k) {
        a[k] = c[k] < c1[k] ? partial[c[k]] : 0.f;                       // 0 + x is exact: the first partial of the lane
        c[k] += 64;
      }
      // the lane's further partials, UW loads in flight at a time, added one after the other in ascending order; a slot past the
      // range adds +0, which changes no bit of a sum of squares
#pragma unroll
      for (int k = 0; k < UF; ++k)
        for (; c[k] < c1[k]; c[k] += 64 * UW) {
          float x[UW];
#pragma unroll
          for (int j = 0; j < UW; ++j) x[j] = c[k] + 64 * j < c1[k] ? partial[c[k] + 64 * j] : 0.f;
#pragma unroll
          for (int j = 0; j < UW; ++j) a[k] += x[j];
        }
#pragma unroll
      for (int k = 0; k < UF; ++k) a[k] = wave_sum(a[k]);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < UF; ++k)
          if (u0 + k < units.U) unit_sum[u0 + k] = a[k];
      }
    }
    __syncthreads();
  }
  const float* __restrict__ terms = UNITS ? unit_sum : partial;
  const int nterms = UNITS ? units.U : nblocks;
  float s = 0.f;
  for (int i = threadIdx.x; i < nterms; i += 256) s += terms[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const int grp = threadIdx.x;
  if (!UNITS && grp >= G) return;
  const float sum = red[0] + red[1] + red[2] + red[3];
  const float gs = grad_scale != nullptr ? grad_scale[0] : 1.f;
  const float norm = sqrtf(sum) / gs;
  const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
  const bool skip = !finite || (found_inf != nullptr && !(found_inf[0] == 0.f));
  float min_coef = 0.f;
  if (UNITS) {
    // thread t owns units t, t + 256, ...: the norm always (a skipped step shows which unit was not finite), the coefficient on a
    // real update only.  A unit's group only selects a max_norm and is clamped to [0, G).
    float lo = __builtin_inff();
    for (int u = threadIdx.x; u < units.U; u += 256) {
      const float norm_u = sqrtf(unit_sum[u]) / gs;
      units.clip_state[2 * u] = norm_u;
      if (skip) continue;
      const int q = units.unit_group[u];
      const float mn = hyper[(q < 0 ? 0 : (q >= G ? G - 1 : q)) * 8 + HY_MAX_NORM];
      float c = 1.f;
      if (mn > 0.f) c = fminf(1.f, mn / (norm_u + 1e-6f));
      c /= gs;
      units.clip_state[2 * u + 1] = c;
      lo = fminf(lo, c);
    }
    if (!skip) {                                   // block-uniform: skip is the same in every thread
      lo = wave_min(lo);
      __syncthreads();                             // every thread has read red[] as the sum
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lo;
      __syncthreads();
      min_coef = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    }
    if (grp >= G) return;
  }
  if (grp == 0) state[ST_GRAD_NORM] = norm;
  if (skip) {
    if (grp == 0) {
      state[ST_SKIP] = 1.f;
      state[ST_SKIPPED] += 1.f;
    }
    return;
  }
  const float* hy = hyper + grp * 8;
  float* stg = state + grp * 8;
  const float lr = hy[HY_LR], b1 = hy[HY_BETA1], b2 = hy[HY_BETA2], wd = hy[HY_WD], max_norm = hyper[HY_MAX_NORM];
  const float bc1 = 1.f - powf(b1, step), bc2 = 1.f - powf(b2, step);
  if (grp == 0) {
    float coef = 1.f;
    if (max_norm > 0.f) coef = fminf(1.f, max_norm / (norm + 1e-6f));
    state[ST_STEP] = step;
    state[ST_SKIP] = 0.f;
    state[ST_COEF] = UNITS ? min_coef : coef / gs;
  }
  stg[ST_STEP_SIZE] = lr / bc1;
  stg[ST_ISB2] = 1.f / sqrtf(bc2);
  stg[ST_DECAY] = 1.f - lr * wd;
  if (AVG && grp == 0) {
    // step counts and the schedule are whole numbers below 2^24 held in fp32: the difference and fmodf are exact.  every = 0 or a
    // NaN word gives NaN != 0: no averaging, never a fault.
    const float mode = avg_hyper[AH_MODE], since = step - avg_hyper[AH_START];
    float flag = (float)AV_NONE;
    if ((mode == (float)AV_EMA || mode == (float)AV_SWA) && since > 0.f && fmodf(since, avg_hyper[AH_EVERY]) == 0.f) {
      const float n_avg = avg_state[AS_N];
      flag = n_avg == 0.f ? (float)AV_FIRST : (float)AV_UPDATE;
      avg_state[AS_W] = mode == (float)AV_EMA ? 1.f - avg_hyper[AH_DECAY] : 1.f / (n_avg + 1.f);
      avg_state[AS_N] = n_avg + 1.f;
    }
    avg_state[AS_FLAG] = flag;
    avg_state[AS_STAMP] = step;
  }
}

__global__ __launch_bounds__(256) void optim_finalize_groups_kernel(const float* __restrict__ partial, int nblocks, const float* __restrict__ hyper,
                                                                    int G, const float* __restrict__ grad_scale,
                                                                    const float* __restrict__ found_inf, float* __restrict__ state,
                                                                    const int* __restrict__ ctl) {
  optim_finalize_groups_body<false, false>(partial, nblocks, hyper, G, grad_scale, found_inf, state, ctl, nullptr, nullptr, ClipUnits{});
}

__global__ __launch_bounds__(256) void optim_finalize_avg_kernel(const float* __restrict__ partial, int nblocks, const float* __restrict__ hyper,
                                                                 int G, const float* __restrict__ grad_scale,
                                                                 const float* __restrict__ found_inf, float* __restrict__ state,
                                                                 const int* __restrict__ ctl, const float* __restrict__ avg_hyper,
                                                                 float* __restrict__ avg_state) {
  optim_finalize_groups_body<true, false>(partial, nblocks, hyper, G, grad_scale, found_inf, state, ctl, avg_hyper, avg_state, ClipUnits{});
}

// The one finalize of the unit clip modes: plain, ctl, G groups and -- AVG -- the averaging decision, all in this body.
template <bool AVG>
__global__ __launch_bounds__(256) void optim_finalize_units_kernel(const float* __restrict__ partial, int C, const int* __restrict__ unit_chunks,
                                                                   const int* __restrict__ unit_group, int U, const float* __restrict__ hyper,
                                                                   int G, const float* __restrict__ grad_scale,
                                                                   const float* __restrict__ found_inf, float* __restrict__ state,
                                                                   const int* __restrict__ ctl, float* __restrict__ clip_state,
                                                                   const float* __restrict__ avg_hyper, float* __restrict__ avg_state) {
  const ClipUnits units = {unit_chunks, unit_group, U, clip_state};
  optim_finalize_groups_body<AVG, true>(partial, C, hyper, G, grad_scale, found_inf, state, ctl, avg_hyper, avg_state, units);
}

// hriemo_sumsq_f32 for the unit clip modes: one block per row of chunks[C][4] = {start, length, unit, group} (the last two columns
// are the host's; the kernel reads the first two), one fp32 sum of squares per chunk.  A thread adds the elements of its vectors
// tid, tid + 256, ... of the chunk one after the other (fmaf(x, x, acc), no masking: a NaN or Inf element makes the partial NaN or
// Inf, which is what the skip decision rests on), the wave adds its 64 lanes by the xor butterfly, thread 0 adds the four wave sums
// in index order.  The table addresses g, so a row is clamped before it is used: start into [0, n] and down to a multiple of 4, the
// length into [0, n - start] likewise -- a table that breaks its contract changes what a partial holds and cannot make g be read out
// of range.  The only store is this block's partial.
__global__ __launch_bounds__(256) void sumsq_units_kernel(const float* __restrict__ g, long n, const long long* __restrict__ chunks,
                                                          float* __restrict__ partial) {
  __shared__ float red[4];
  const long long* row = chunks + (long)blockIdx.x * 4;
  long long start = row[0], len = row[1];
  start = (start < 0 ? 0 : (start > n ? n : start)) & ~3LL;
  len = (len < 0 ? 0 : (len > n - start ? n - start : len)) & ~3LL;
  const long nv = (long)(len >> 2);
  const float* gb = g + start;
  float s = 0.f;
#pragma unroll 4
  for (long i = threadIdx.x; i < nv; i += 256) {
    const f32x4 t = *(const f32x4*)(gb + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_fmaf(t[e], t[e], s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// adamw_flat_dev_kernel with per-segment scalars: ONE launch over the whole flat buffer.  seg[S + 1] (ascending element offsets,
// seg[0] = 0, seg[S] = n, multiples of 4) and seg_group[S] say which group owns which elements; a group may own several segments.
// How a vector finds its group: the table is copied into LDS once per block ((S + 1) int64 + the 7 scalars of every group + S group
// bytes: at most 19 KiB) and every thread keeps its CURRENT segment -- bounds and scalars -- in registers, as gather_rows_kernel
// (store.hip) does.  A vector inside the current segment costs two compares; one outside it a binary search in LDS (<= 11 probes)
// and 7 LDS reads, once per sweep of the capped grid at worst.  The table only ever selects scalars, it addresses nothing: the
// search result is clamped to [0, S) and the group to [0, G), so a table that breaks its contract changes which hyper-parameters
// an element gets and cannot make hyper, state, p, g, m or v be read or written out of range.  Nothing at or beyond n is written.
// AVG: the averaging form (hriemo_adamw_flat_groups_avg): avg_vec4 behind adamw_vec4 on an averaging update (avg is indexed by the
// vector index alone, like p), nothing of avg touched on any other step; AVG = false is the kernel of before.
// UNITS: the update of the unit clip modes (hriemo_adamw_flat_units, hriemo_adamw_flat_units_avg): seg_unit[S] names the clip unit
// of every segment and clip_state[U][2] holds the units' coefficients (hriemo_optim_finalize_units); the LDS table grows by
// coef[U] and seg_unit[S] (4 U + 2 S bytes, at most 12 KiB) and a thread that changes segment takes the coefficient of that
// segment's unit instead of state[ST_COEF].  Units, like groups, only select a scalar and are clamped to [0, U).  UNITS = false is
// the kernel of before, seg_unit, clip_state and U unused and the LDS layout unchanged.
template <bool AVG, bool UNITS>
__device__ __forceinline__ void adamw_flat_groups_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long n, const long long* __restrict__ seg,
                                                       const int* __restrict__ seg_group, int S, const float* __restrict__ hyper,
                                                       const float* __restrict__ state, int G, float* __restrict__ avg,
                                                       const float* __restrict__ avg_state, const int* __restrict__ seg_unit,
                                                       const float* __restrict__ clip_state, int U) {
  if (state[ST_SKIP] != 0.f) return;               // block-uniform: nobody reaches the barrier below
  AvgStep a = {AV_NONE, 0.f};
  if (AVG) a = avg_step(state, avg_state);
  extern __shared__ __attribute__((aligned(16))) long long ag_lds[];
  long long* segb = ag_lds;                        // [S + 1]
  float* sc = (float*)(segb + (S + 1));            // [G][8]: b1, b2, eps, coef, step_size, isb2, decay, spare
  float* uc = sc + G * 8;                          // [U] coefficient of unit u (UNITS)
  unsigned short* su = (unsigned short*)(uc + (UNITS ? U : 0));   // [S] unit of segment s, clamped to [0, U) (UNITS)
  unsigned char* sg = (unsigned char*)(su + (UNITS ? S : 0));     // [S] group of segment s, clamped to [0, G)
  for (int i = threadIdx.x; i <= S; i += 256) {
    segb[i] = seg[i];
    if (i < S) {
      const int q = seg_group[i];
      sg[i] = (unsigned char)(q < 0 ? 0 : (q >= G ? G - 1 : q));
      if (UNITS) {
        const int w = seg_unit[i];
        su[i] = (unsigned short)(w < 0 ? 0 : (w >= U ? U - 1 : w));
      }
    }
  }
  if (UNITS)
    for (int u = threadIdx.x; u < U; u += 256) uc[u] = clip_state[2 * u + 1];
  if (threadIdx.x < G) {
    const float* hy = hyper + threadIdx.x * 8;
    const float* stg = state + threadIdx.x * 8;
    float* o = sc + threadIdx.x * 8;
    o[0] = hy[HY_BETA1]; o[1] = hy[HY_BETA2]; o[2] = hy[HY_EPS]; o[3] = state[ST_COEF];
    o[4] = stg[ST_STEP_SIZE]; o[5] = stg[ST_ISB2]; o[6] = stg[ST_DECAY]; o[7] = 0.f;
  }
  __syncthreads();
  AdamScalars s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  long long cur_lo = 0, cur_hi = 0;                // empty: the first vector searches
  const long nv = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    const long long x = (long long)i * 4;
    if (x < cur_lo || x >= cur_hi) {
      // upper bound: the first k in [1, S] with segb[k] > x (S if there is none); the owner is k - 1, in [0, S)
      int lo = 1, hi = S;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (segb[mid] > x) hi = mid; else lo = mid + 1;
      }
      cur_lo = segb[lo - 1]; cur_hi = segb[lo];
      const float* o = sc + (int)sg[lo - 1] * 8;
      s.b1 = o[0]; s.b2 = o[1]; s.eps = o[2]; s.coef = UNITS ? uc[su[lo - 1]] : o[3]; s.step = o[4]; s.isb2 = o[5]; s.decay = o[6];
    }
    const f32x4 pp = adamw_vec4(p, g, m, v, i, s);
    if (AVG && a.kind != AV_NONE) avg_vec4(avg, i, pp, a);   // block-uniform branch
  }
}

__global__ __launch_bounds__(256) void adamw_flat_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, long n, const long long* __restrict__ seg,
                                                                const int* __restrict__ seg_group, int S, const float* __restrict__ hyper,
                                                                const float* __restrict__ state, int G) {
  adamw_flat_groups_body<false, false>(p, g, m, v, n, seg, seg_group, S, hyper, state, G, nullptr, nullptr, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(256) void adamw_flat_groups_avg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                    float* __restrict__ v, long n, const long long* __restrict__ seg,
                                                                    const int* __restrict__ seg_group, int S, const float* __restrict__ hyper,
                                                                    const float* __restrict__ state, int G, float* __restrict__ avg,
                                                                    const float* __restrict__ avg_state) {
  adamw_flat_groups_body<true, false>(p, g, m, v, n, seg, seg_group, S, hyper, state, G, avg, avg_state, nullptr, nullptr, 0);
}

template <bool AVG>
__global__ __launch_bounds__(256) void adamw_flat_units_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, long n, const long long* __restrict__ seg,
                                                               const int* __restrict__ seg_group, const int* __restrict__ seg_unit, int S,
                                                               const float* __restrict__ hyper, const float* __restrict__ state, int G,
                                                               const float* __restrict__ clip_state, int U, float* __restrict__ avg,
                                                               const float* __restrict__ avg_state) {
  adamw_flat_groups_body<AVG, true>(p, g, m, v, n, seg, seg_group, S, hyper, state, G, avg, avg_state, seg_unit, clip_state, U);
}

// Exact exchange of two fp32 buffers that do not overlap: 16-byte vector loads and stores, grid capped like the update's.  Every
// bit crosses (NaN payloads, -0, denormals: nothing is computed), nothing at or beyond n is touched.
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__global__ __launch_bounds__(256) void swap_fp32_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
  const long nv = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    const u32x4 x = *(const u32x4*)(a + i * 4), y = *(const u32x4*)(b + i * 4);
    *(u32x4*)(a + i * 4) = y; *(u32x4*)(b + i * 4) = x;
  }
}

// The conditional start of an accumulation group: ctl.first != 0 -> +0 over flat[0, n) (16-byte stores, grid capped like the update's);
// ctl.first == 0 -> the kernel returns without a load or a store, so NaN payloads, -0 and denormals of the running sum survive.
__global__ __launch_bounds__(256) void grad_begin_kernel(float* __restrict__ flat, long n, const int* __restrict__ ctl) {
  if (ctl[CTL_FIRST] == 0) return;
  const long nv = n >> 2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) *(f32x4*)(flat + i * 4) = zero;
}

extern "C" int hriemo_grad_begin(float* flat, long n, const int* ctl, hipStream_t st) {
  HRIEMO_CHECK(flat != nullptr && n > 0 && n % 4 == 0, "grad_begin: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(((uintptr_t)flat % 16) == 0, "grad_begin: unaligned buffer");
  HRIEMO_CHECK(ctl != nullptr && ((uintptr_t)ctl % 4) == 0, "grad_begin: ctl is the int32 step-control block in device memory");
  long gsz = (n / 4 + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  hipLaunchKernelGGL(grad_begin_kernel, dim3((int)gsz), dim3(256), 0, st, flat, n, ctl);
  HRIEMO_LAUNCH_CHECK("grad_begin_kernel");
  return 0;
}

extern "C" int hriemo_optim_finalize(const float* partial, int nblocks, const float* hyper, const float* grad_scale, const float* found_inf,
                                     float* state, hipStream_t st) {
  HRIEMO_CHECK(partial != nullptr && hyper != nullptr && state != nullptr, "optim_finalize: partial, hyper and state are required");
  HRIEMO_CHECK(nblocks > 0 && nblocks <= 4096, "optim_finalize: nblocks=%d out of range (1..4096)", nblocks);
  hipLaunchKernelGGL(optim_finalize_kernel<false>, dim3(1), dim3(256), 0, st, partial, nblocks, hyper, grad_scale, found_inf, state,
                     (const int*)nullptr);
  HRIEMO_LAUNCH_CHECK("optim_finalize_kernel");
  return 0;
}

extern "C" int hriemo_optim_finalize_ctl(const float* partial, int nblocks, const float* hyper, const float* grad_scale,
                                         const float* found_inf, float* state, const int* ctl, hipStream_t st) {
  HRIEMO_CHECK(partial != nullptr && hyper != nullptr && state != nullptr, "optim_finalize_ctl: partial, hyper and state are required");
  HRIEMO_CHECK(nblocks > 0 && nblocks <= 4096, "optim_finalize_ctl: nblocks=%d out of range (1..4096)", nblocks);
  HRIEMO_CHECK(ctl != nullptr && ((uintptr_t)ctl % 4) == 0, "optim_finalize_ctl: ctl is the int32 step-control block in device memory");
  hipLaunchKernelGGL(optim_finalize_kernel<true>, dim3(1), dim3(256), 0, st, partial, nblocks, hyper, grad_scale, found_inf, state, ctl);
  HRIEMO_LAUNCH_CHECK("optim_finalize_kernel<hold>");
  return 0;
}

extern "C" int hriemo_adamw_flat_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, const float* state,
                                     hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "adamw_flat_dev: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0,
               "adamw_flat_dev: unaligned buffer");
  HRIEMO_CHECK(hyper != nullptr && state != nullptr, "adamw_flat_dev: hyper and state are required");
  long gsz = (n / 4 + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  hipLaunchKernelGGL(adamw_flat_dev_kernel, dim3((int)gsz), dim3(256), 0, st, p, g, m, v, n, hyper, state);
  HRIEMO_LAUNCH_CHECK("adamw_flat_dev_kernel");
  return 0;
}

extern "C" int hriemo_optim_finalize_groups(const float* partial, int nblocks, const float* hyper, int G, const float* grad_scale,
                                            const float* found_inf, float* state, const int* ctl, hipStream_t st) {
  HRIEMO_CHECK(partial != nullptr && hyper != nullptr && state != nullptr, "optim_finalize_groups: partial, hyper and state are required");
  HRIEMO_CHECK(nblocks > 0 && nblocks <= 4096, "optim_finalize_groups: nblocks=%d out of range (1..4096)", nblocks);
  HRIEMO_CHECK(G >= 1 && G <= AG_MAX_GROUPS, "optim_finalize_groups: G=%d groups (1 .. %d)", G, (int)AG_MAX_GROUPS);
  HRIEMO_CHECK(((uintptr_t)ctl % 4) == 0, "optim_finalize_groups: ctl is the int32 step-control block in device memory (or NULL)");
  hipLaunchKernelGGL(optim_finalize_groups_kernel, dim3(1), dim3(256), 0, st, partial, nblocks, hyper, G, grad_scale, found_inf, state, ctl);
  HRIEMO_LAUNCH_CHECK("optim_finalize_groups_kernel");
  return 0;
}

extern "C" int hriemo_adamw_flat_groups(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group,
                                        int S, const float* hyper, const float* state, int G, hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "adamw_flat_groups: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(p != nullptr && g != nullptr && m != nullptr && v != nullptr, "adamw_flat_groups: p, g, m and v are required");
  HRIEMO_CHECK(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0,
               "adamw_flat_groups: unaligned buffer");
  HRIEMO_CHECK(hyper != nullptr && state != nullptr, "adamw_flat_groups: hyper and state are required");
  HRIEMO_CHECK(G >= 1 && G <= AG_MAX_GROUPS, "adamw_flat_groups: G=%d groups (1 .. %d)", G, (int)AG_MAX_GROUPS);
  HRIEMO_CHECK(S >= 1 && S <= AG_MAX_SEGS, "adamw_flat_groups: S=%d segments (1 .. %d)", S, (int)AG_MAX_SEGS);
  HRIEMO_CHECK(seg != nullptr && seg_group != nullptr, "adamw_flat_groups: seg (int64 [S + 1]) and seg_group (int32 [S]) are required");
  HRIEMO_CHECK(((uintptr_t)seg % 8) == 0, "adamw_flat_groups: seg (int64 [S + 1]) is not 8-byte aligned");
  HRIEMO_CHECK(((uintptr_t)seg_group % 4) == 0, "adamw_flat_groups: seg_group (int32 [S]) is not 4-byte aligned");
  long gsz = (n / 4 + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  const size_t lds = (size_t)(S + 1) * sizeof(long long) + (size_t)G * 8 * sizeof(float) + (size_t)S;
  hipLaunchKernelGGL(adamw_flat_groups_kernel, dim3((int)gsz), dim3(256), lds, st, p, g, m, v, n, seg, seg_group, S, hyper, state, G);
  HRIEMO_LAUNCH_CHECK("adamw_flat_groups_kernel");
  return 0;
}

// [x, x + bytes) and [y, y + bytes) share a byte
static bool ranges_overlap(const void* x, const void* y, size_t bytes) {
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
  return a < b ? b - a < bytes : a - b < bytes;
}

extern "C" int hriemo_optim_finalize_avg(const float* partial, int nblocks, const float* hyper, int G, const float* grad_scale,
                                         const float* found_inf, float* state, const int* ctl, const float* avg_hyper, float* avg_state,
                                         hipStream_t st) {
  HRIEMO_CHECK(partial != nullptr && hyper != nullptr && state != nullptr, "optim_finalize_avg: partial, hyper and state are required");
  HRIEMO_CHECK(nblocks > 0 && nblocks <= 4096, "optim_finalize_avg: nblocks=%d out of range (1..4096)", nblocks);
  HRIEMO_CHECK(G >= 1 && G <= AG_MAX_GROUPS, "optim_finalize_avg: G=%d groups (1 .. %d)", G, (int)AG_MAX_GROUPS);
  HRIEMO_CHECK(((uintptr_t)ctl % 4) == 0, "optim_finalize_avg: ctl is the int32 step-control block in device memory (or NULL)");
  HRIEMO_CHECK(avg_hyper != nullptr && avg_state != nullptr && ((uintptr_t)avg_hyper % 4) == 0 && ((uintptr_t)avg_state % 4) == 0,
               "optim_finalize_avg: avg_hyper and avg_state (fp32 [4] each, device memory) are required");
  hipLaunchKernelGGL(optim_finalize_avg_kernel, dim3(1), dim3(256), 0, st, partial, nblocks, hyper, G, grad_scale, found_inf, state, ctl,
                     avg_hyper, avg_state);
  HRIEMO_LAUNCH_CHECK("optim_finalize_avg_kernel");
  return 0;
}

extern "C" int hriemo_adamw_flat_dev_avg(float* p, const float* g, float* m, float* v, long n, const float* hyper, const float* state,
                                         float* avg, const float* avg_state, hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "adamw_flat_dev_avg: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(p != nullptr && g != nullptr && m != nullptr && v != nullptr && avg != nullptr, "adamw_flat_dev_avg: p, g, m, v and avg are required");
  HRIEMO_CHECK(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                   ((uintptr_t)avg % 16) == 0, "adamw_flat_dev_avg: unaligned buffer");
  HRIEMO_CHECK(hyper != nullptr && state != nullptr && avg_state != nullptr, "adamw_flat_dev_avg: hyper, state and avg_state are required");
  HRIEMO_CHECK(!ranges_overlap(avg, p, (size_t)n * 4) && !ranges_overlap(avg, g, (size_t)n * 4) && !ranges_overlap(avg, m, (size_t)n * 4) &&
                   !ranges_overlap(avg, v, (size_t)n * 4), "adamw_flat_dev_avg: avg overlaps p, g, m or v");
  long gsz = (n / 4 + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  hipLaunchKernelGGL(adamw_flat_dev_avg_kernel, dim3((int)gsz), dim3(256), 0, st, p, g, m, v, n, hyper, state, avg, avg_state);
  HRIEMO_LAUNCH_CHECK("adamw_flat_dev_avg_kernel");
  return 0;
}

extern "C" int hriemo_adamw_flat_groups_avg(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group,
                                            int S, const float* hyper, const float* state, int G, float* avg, const float* avg_state,
                                            hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "adamw_flat_groups_avg: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(p != nullptr && g != nullptr && m != nullptr && v != nullptr && avg != nullptr,
               "adamw_flat_groups_avg: p, g, m, v and avg are required");
  HRIEMO_CHECK(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                   ((uintptr_t)avg % 16) == 0, "adamw_flat_groups_avg: unaligned buffer");
  HRIEMO_CHECK(hyper != nullptr && state != nullptr && avg_state != nullptr, "adamw_flat_groups_avg: hyper, state and avg_state are required");
  HRIEMO_CHECK(G >= 1 && G <= AG_MAX_GROUPS, "adamw_flat_groups_avg: G=%d groups (1 .. %d)", G, (int)AG_MAX_GROUPS);
  HRIEMO_CHECK(S >= 1 && S <= AG_MAX_SEGS, "adamw_flat_groups_avg: S=%d segments (1 .. %d)", S, (int)AG_MAX_SEGS);
  HRIEMO_CHECK(seg != nullptr && seg_group != nullptr, "adamw_flat_groups_avg: seg (int64 [S + 1]) and seg_group (int32 [S]) are required");
  HRIEMO_CHECK(((uintptr_t)seg % 8) == 0, "adamw_flat_groups_avg: seg (int64 [S + 1]) is not 8-byte aligned");
  HRIEMO_CHECK(((uintptr_t)seg_group % 4) == 0, "adamw_flat_groups_avg: seg_group (int32 [S]) is not 4-byte aligned");
  HRIEMO_CHECK(!ranges_overlap(avg, p, (size_t)n * 4) && !ranges_overlap(avg, g, (size_t)n * 4) && !ranges_overlap(avg, m, (size_t)n * 4) &&
                   !ranges_overlap(avg, v, (size_t)n * 4), "adamw_flat_groups_avg: avg overlaps p, g, m or v");
  long gsz = (n / 4 + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  const size_t lds = (size_t)(S + 1) * sizeof(long long) + (size_t)G * 8 * sizeof(float) + (size_t)S;
  hipLaunchKernelGGL(adamw_flat_groups_avg_kernel, dim3((int)gsz), dim3(256), lds, st, p, g, m, v, n, seg, seg_group, S, hyper, state, G, avg,
                     avg_state);
  HRIEMO_LAUNCH_CHECK("adamw_flat_groups_avg_kernel");
  return 0;
}

// ---------------------------------------------------------------------------------------------- the unit clip modes
// DeviceAdamW(clip="group" | "parameter"): every clip unit -- a param group, or a parameter tensor -- is clipped by its own norm
// against its group's max_norm (hyper[g][HY_MAX_NORM], every row read).  Still three launches: hriemo_sumsq_units ->
// hriemo_optim_finalize_units -> hriemo_adamw_flat_units(_avg).  The skip decision, the step count, `skipped`, grad_norm and the
// HOLD stay global, in row 0 of state; state[0][ST_COEF] holds the smallest unit coefficient.
//   clip_state[U][2]  written by the finalize: norm_u, coef_u -- both on a real update, the norms alone on a skipped step, nothing
//                     on a held micro-step
enum { CU_MAX_UNITS = 2048, CU_MAX_CHUNKS = 1 << 20 };

static bool spans_overlap(const void* x, size_t nx, const void* y, size_t ny) {
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
  return a < b ? b - a < nx : a - b < ny;
}

extern "C" int hriemo_sumsq_units(const float* g, long n, const long long* chunks, int C, float* partial, hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "sumsq_units: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(g != nullptr && ((uintptr_t)g % 16) == 0, "sumsq_units: g is required, 16-byte aligned");
  HRIEMO_CHECK(C >= 1 && C <= CU_MAX_CHUNKS, "sumsq_units: C=%d chunks (1 .. %d)", C, (int)CU_MAX_CHUNKS);
  HRIEMO_CHECK((long)C <= n / 4, "sumsq_units: C=%d chunks over n=%ld elements: more chunks than 16-byte vectors", C, n);
  HRIEMO_CHECK(chunks != nullptr && ((uintptr_t)chunks % 8) == 0, "sumsq_units: chunks (int64 [C][4]) is required, 8-byte aligned");
  HRIEMO_CHECK(partial != nullptr && ((uintptr_t)partial % 4) == 0, "sumsq_units: partial (fp32 [C]) is required, 4-byte aligned");
  HRIEMO_CHECK(!spans_overlap(partial, (size_t)C * 4, g, (size_t)n * 4) && !spans_overlap(partial, (size_t)C * 4, chunks, (size_t)C * 32),
               "sumsq_units: partial overlaps g or chunks");
  hipLaunchKernelGGL(sumsq_units_kernel, dim3(C), dim3(256), 0, st, g, n, chunks, partial);
  HRIEMO_LAUNCH_CHECK("sumsq_units_kernel");
  return 0;
}

extern "C" int hriemo_optim_finalize_units(const float* partial, int C, const int* unit_chunks, const int* unit_group, int U,
                                           const float* hyper, int G, const float* grad_scale, const float* found_inf, float* state,
                                           const int* ctl, float* clip_state, const float* avg_hyper, float* avg_state, hipStream_t st) {
  HRIEMO_CHECK(partial != nullptr && hyper != nullptr && state != nullptr, "optim_finalize_units: partial, hyper and state are required");
  HRIEMO_CHECK(C >= 1 && C <= CU_MAX_CHUNKS, "optim_finalize_units: C=%d chunks (1 .. %d)", C, (int)CU_MAX_CHUNKS);
  HRIEMO_CHECK(U >= 1 && U <= CU_MAX_UNITS, "optim_finalize_units: U=%d units (1 .. %d)", U, (int)CU_MAX_UNITS);
  HRIEMO_CHECK(U <= C, "optim_finalize_units: U=%d units over C=%d chunks: every unit owns at least one chunk", U, C);
  HRIEMO_CHECK(G >= 1 && G <= AG_MAX_GROUPS, "optim_finalize_units: G=%d groups (1 .. %d)", G, (int)AG_MAX_GROUPS);
  HRIEMO_CHECK(unit_chunks != nullptr && unit_group != nullptr && ((uintptr_t)unit_chunks % 4) == 0 && ((uintptr_t)unit_group % 4) == 0,
               "optim_finalize_units: unit_chunks (int32 [U + 1]) and unit_group (int32 [U]) are required, 4-byte aligned");
  HRIEMO_CHECK(clip_state != nullptr && ((uintptr_t)clip_state % 4) == 0, "optim_finalize_units: clip_state (fp32 [U][2]) is required, 4-byte aligned");
  HRIEMO_CHECK(((uintptr_t)ctl % 4) == 0, "optim_finalize_units: ctl is the int32 step-control block in device memory (or NULL)");
  HRIEMO_CHECK((avg_hyper == nullptr) == (avg_state == nullptr) && ((uintptr_t)avg_hyper % 4) == 0 && ((uintptr_t)avg_state % 4) == 0,
               "optim_finalize_units: avg_hyper and avg_state (fp32 [4] each, device memory) come together or not at all");
  const size_t cb = (size_t)U * 8;
  HRIEMO_CHECK(!spans_overlap(clip_state, cb, partial, (size_t)C * 4) && !spans_overlap(clip_state, cb, state, (size_t)G * 32) &&
                   !spans_overlap(clip_state, cb, hyper, (size_t)G * 32) && !spans_overlap(clip_state, cb, unit_chunks, (size_t)(U + 1) * 4) &&
                   !spans_overlap(clip_state, cb, unit_group, (size_t)U * 4),
               "optim_finalize_units: clip_state overlaps partial, state, hyper, unit_chunks or unit_group");
  const size_t lds = (size_t)U * sizeof(float);
  if (avg_hyper != nullptr)
    hipLaunchKernelGGL(optim_finalize_units_kernel<true>, dim3(1), dim3(256), lds, st, partial, C, unit_chunks, unit_group, U, hyper, G,
                       grad_scale, found_inf, state, ctl, clip_state, avg_hyper, avg_state);
  else
    hipLaunchKernelGGL(optim_finalize_units_kernel<false>, dim3(1), dim3(256), lds, st, partial, C, unit_chunks, unit_group, U, hyper, G,
                       grad_scale, found_inf, state, ctl, clip_state, avg_hyper, avg_state);
  HRIEMO_LAUNCH_CHECK("optim_finalize_units_kernel");
  return 0;
}

// avg == NULL: hriemo_adamw_flat_units; otherwise hriemo_adamw_flat_units_avg
static int adamw_flat_units_launch(const char* who, float* p, const float* g, float* m, float* v, long n, const long long* seg,
                                   const int* seg_group, const int* seg_unit, int S, const float* hyper, const float* state, int G,
                                   const float* clip_state, int U, float* avg, const float* avg_state, hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "%s: n=%ld must be a positive multiple of 4", who, n);
  HRIEMO_CHECK(p != nullptr && g != nullptr && m != nullptr && v != nullptr, "%s: p, g, m and v are required", who);
  HRIEMO_CHECK(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                   ((uintptr_t)avg % 16) == 0, "%s: unaligned buffer", who);
  HRIEMO_CHECK(hyper != nullptr && state != nullptr, "%s: hyper and state are required", who);
  HRIEMO_CHECK(G >= 1 && G <= AG_MAX_GROUPS, "%s: G=%d groups (1 .. %d)", who, G, (int)AG_MAX_GROUPS);
  HRIEMO_CHECK(S >= 1 && S <= AG_MAX_SEGS, "%s: S=%d segments (1 .. %d)", who, S, (int)AG_MAX_SEGS);
  HRIEMO_CHECK(U >= 1 && U <= CU_MAX_UNITS, "%s: U=%d units (1 .. %d)", who, U, (int)CU_MAX_UNITS);
  HRIEMO_CHECK(U <= S, "%s: U=%d units over S=%d segments: every unit owns at least one segment", who, U, S);
  HRIEMO_CHECK((long)S <= n / 4, "%s: S=%d segments over n=%ld elements: more segments than 16-byte vectors", who, S, n);
  HRIEMO_CHECK(seg != nullptr && seg_group != nullptr && seg_unit != nullptr,
               "%s: seg (int64 [S + 1]), seg_group and seg_unit (int32 [S]) are required", who);
  HRIEMO_CHECK(((uintptr_t)seg % 8) == 0, "%s: seg (int64 [S + 1]) is not 8-byte aligned", who);
  HRIEMO_CHECK(((uintptr_t)seg_group % 4) == 0 && ((uintptr_t)seg_unit % 4) == 0, "%s: seg_group / seg_unit (int32 [S]) is not 4-byte aligned", who);
  HRIEMO_CHECK(clip_state != nullptr && ((uintptr_t)clip_state % 4) == 0, "%s: clip_state (fp32 [U][2]) is required, 4-byte aligned", who);
  long gsz = (n / 4 + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  const size_t lds = (size_t)(S + 1) * sizeof(long long) + (size_t)G * 8 * sizeof(float) + (size_t)U * sizeof(float) + (size_t)S * 2 + (size_t)S;
  if (avg != nullptr) {
    HRIEMO_CHECK(avg_state != nullptr, "%s: avg_state is required", who);
    HRIEMO_CHECK(!ranges_overlap(avg, p, (size_t)n * 4) && !ranges_overlap(avg, g, (size_t)n * 4) && !ranges_overlap(avg, m, (size_t)n * 4) &&
                     !ranges_overlap(avg, v, (size_t)n * 4), "%s: avg overlaps p, g, m or v", who);
    hipLaunchKernelGGL(adamw_flat_units_kernel<true>, dim3((int)gsz), dim3(256), lds, st, p, g, m, v, n, seg, seg_group, seg_unit, S, hyper, state,
                       G, clip_state, U, avg, avg_state);
  } else {
    hipLaunchKernelGGL(adamw_flat_units_kernel<false>, dim3((int)gsz), dim3(256), lds, st, p, g, m, v, n, seg, seg_group, seg_unit, S, hyper, state,
                       G, clip_state, U, (float*)nullptr, (const float*)nullptr);
  }
  HRIEMO_LAUNCH_CHECK("adamw_flat_units_kernel");
  return 0;
}

extern "C" int hriemo_adamw_flat_units(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group,
                                       const int* seg_unit, int S, const float* hyper, const float* state, int G, const float* clip_state,
                                       int U, hipStream_t st) {
  return adamw_flat_units_launch("adamw_flat_units", p, g, m, v, n, seg, seg_group, seg_unit, S, hyper, state, G, clip_state, U, nullptr,
                                 nullptr, st);
}

extern "C" int hriemo_adamw_flat_units_avg(float* p, const float* g, float* m, float* v, long n, const long long* seg, const int* seg_group,
                                           const int* seg_unit, int S, const float* hyper, const float* state, int G,
                                           const float* clip_state, int U, float* avg, const float* avg_state, hipStream_t st) {
  HRIEMO_CHECK(avg != nullptr, "adamw_flat_units_avg: avg is required");
  return adamw_flat_units_launch("adamw_flat_units_avg", p, g, m, v, n, seg, seg_group, seg_unit, S, hyper, state, G, clip_state, U, avg,
                                 avg_state, st);
}

extern "C" int hriemo_swap_fp32(float* a, float* b, long n, hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "swap_fp32: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(a != nullptr && b != nullptr && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0, "swap_fp32: two 16-byte aligned buffers are required");
  HRIEMO_CHECK(!ranges_overlap(a, b, (size_t)n * 4), "swap_fp32: the buffers overlap (or are one buffer)");
  long gsz = (n / 4 + 255) / 256;
  if (gsz > 4096) gsz = 4096;
  hipLaunchKernelGGL(swap_fp32_kernel, dim3((int)gsz), dim3(256), 0, st, a, b, n);
  HRIEMO_LAUNCH_CHECK("swap_fp32_kernel");
  return 0;
}
