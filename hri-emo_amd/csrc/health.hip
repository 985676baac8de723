// The health log of the device-state AdamW (hri-emo_amd/optim.py: HealthLog): per-parameter statistics of a step -- gradient sum of
// squares, the number of non-finite gradient elements, weight sum of squares, sum of squares of the Adam term -- written by the
// step itself into a ring in device memory, so that a skipped update inside a captured step can be blamed on a parameter and the
// per-layer norms and update-to-weight ratios can be read without giving up the graph.  Two launches BEHIND the update kernel of
// optim.hip (the update does not change the gradient buffer, so one sweep behind it sees everything); they only read hyper[],
// state[], ctl, g, p, m and v.
//   chunks[C][4]  written by the host, once (int64): {start, length, parameter, group} -- every parameter's slot of the flat buffers
//                 (256-byte aligned start, padded to 64 elements, zeros in the padding of g, p, m and v) cut into pieces of at most
//                 `chunk` elements, in flat-buffer order; all chunks of a parameter are neighbours and ascend
//   partial[C][4] written by the sweep: {grad_sq, nonfinite (int32 bits), weight_sq, update_sq} of chunk c
//   log           int32 words: [0] n_recorded (records ever written), [1..3] spare, then `capacity` records of 4 + 4 P words:
//                 {step (fp32), kind (int32), grad_norm (fp32), spare}, grad_sq[P] (fp32), nonfinite[P] (int32), weight_sq[P] (fp32),
//                 update_sq[P] (fp32); record r of the run lives in slot r % capacity
// Which steps record, decided by every block of both kernels from state[], ctl and `every`, in front of any barrier:
//   ctl != NULL and ctl.last == 0 (a held accumulation micro-step)  -> nothing: no load, no store, no word of the log moves
//   state.skip != 0 (the finalize skipped the update)               -> always: kind 1 if state.grad_norm is not finite, else kind 2
//                                                                      (found_inf alone); only g is read, weight_sq = update_sq = 0
//   a real update with step count t = state.step                    -> kind 0 iff t % every == 0; g, p, m and v are read
// Every sum has ONE fixed order (no floating-point atomics anywhere): a thread adds the elements of its vectors i = tid, tid + 256,
// ... of the chunk one after the other (fmaf(x, x, acc), 4 per vector), the wave adds its 64 lanes by the xor butterfly, thread 0
// adds the four wave sums in index order; the fold adds a parameter's chunk partials in chunk order.  The same step from the same
// state gives the same bits.
#include "common.h"

enum { HY_EPS = 3 };                                             // hyper[g][8] and state[g][8] of optim.hip
enum { ST_STEP = 0, ST_SKIP = 1, ST_STEP_SIZE = 3, ST_ISB2 = 4, ST_GRAD_NORM = 6 };
enum { CTL_LAST = 2 };
enum { HL_MAX_GROUPS = 16, HL_MAX_PARAMS = 4096, HL_MAX_CHUNKS = 1 << 20, HL_MAX_CAPACITY = 1 << 20 };
enum { HL_HEADER = 4, HL_REC_HEADER = 4 };
enum { HK_NONE = -1, HK_UPDATE = 0, HK_SKIP_NORM = 1, HK_SKIP_INF = 2 };

__device__ __forceinline__ bool is_finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// Block-uniform (scalar loads of words no launch of this step writes any more): every thread of both kernels gets the same answer.
// The step count is a whole number below 2^24 held in fp32; every >= 1 is the launchers' check.
__device__ __forceinline__ int health_kind(const float* __restrict__ state, const int* __restrict__ ctl, int every) {
  if (ctl != nullptr && ctl[CTL_LAST] == 0) return HK_NONE;
  if (state[ST_SKIP] != 0.f) return is_finite_bits(state[ST_GRAD_NORM]) ? HK_SKIP_INF : HK_SKIP_NORM;
  return (int)state[ST_STEP] % every == 0 ? HK_UPDATE : HK_NONE;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One block per chunk.  The table addresses g, p, m and v, so a row is clamped before it is used: start into [0, n] and down to a
// multiple of 4, the length into [0, n - start] likewise, the group into [0, G) -- a table that breaks its contract changes what a
// partial holds and cannot make any buffer be read out of range.  The only store is the 16-byte partial of this block's chunk.
__global__ __launch_bounds__(256) void health_sweep_kernel(const float* __restrict__ g, const float* __restrict__ p, const float* __restrict__ m,
                                                           const float* __restrict__ v, long n, const long long* __restrict__ chunks,
                                                           const float* __restrict__ hyper, const float* __restrict__ state, int G,
                                                           const int* __restrict__ ctl, int every, float* __restrict__ partial) {
  const int kind = health_kind(state, ctl, every);
  if (kind == HK_NONE) return;                                   // block-uniform: nobody reaches the barrier below
  __shared__ float red[4][4];
  const long long* row = chunks + (long)blockIdx.x * 4;
  long long start = row[0], len = row[1];
  int grp = (int)row[3];
  start = (start < 0 ? 0 : (start > n ? n : start)) & ~3LL;
  len = (len < 0 ? 0 : (len > n - start ? n - start : len)) & ~3LL;
  grp = grp < 0 ? 0 : (grp >= G ? G - 1 : grp);
  const long nv = (long)(len >> 2);
  const float* gb = g + start;
  float gsq = 0.f, wsq = 0.f, usq = 0.f;
  int bad = 0;
  if (kind == HK_UPDATE) {
    const float* pb = p + start;
    const float* mb = m + start;
    const float* vb = v + start;
    const float step = state[grp * 8 + ST_STEP_SIZE], isb2 = state[grp * 8 + ST_ISB2], eps = hyper[grp * 8 + HY_EPS];
    for (long i = threadIdx.x; i < nv; i += 256) {
      const f32x4 gg = *(const f32x4*)(gb + i * 4), pp = *(const f32x4*)(pb + i * 4), mm = *(const f32x4*)(mb + i * 4),
                  vv = *(const f32x4*)(vb + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool fin = is_finite_bits(gg[e]);
        const float x = fin ? gg[e] : 0.f;
        bad += fin ? 0 : 1;
        gsq = __builtin_fmaf(x, x, gsq);
        wsq = __builtin_fmaf(pp[e], pp[e], wsq);
        const float d = step * mm[e] / (sqrtf(vv[e]) * isb2 + eps);     // the term adamw_vec4 subtracted, from the new moments
        usq = __builtin_fmaf(d, d, usq);
      }
    }
  } else {
    for (long i = threadIdx.x; i < nv; i += 256) {
      const f32x4 gg = *(const f32x4*)(gb + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool fin = is_finite_bits(gg[e]);
        const float x = fin ? gg[e] : 0.f;
        bad += fin ? 0 : 1;
        gsq = __builtin_fmaf(x, x, gsq);
      }
    }
  }
  gsq = wave_sum(gsq); wsq = wave_sum(wsq); usq = wave_sum(usq);
  bad = wave_sum_int(bad);
  if ((threadIdx.x & 63) == 0) {
    float* r = red[threadIdx.x >> 6];
    r[0] = gsq; r[1] = __int_as_float(bad); r[2] = wsq; r[3] = usq;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  f32x4 out;
  out[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
  out[1] = __int_as_float(__float_as_int(red[0][1]) + __float_as_int(red[1][1]) + __float_as_int(red[2][1]) + __float_as_int(red[3][1]));
  out[2] = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
  out[3] = ((red[0][3] + red[1][3]) + red[2][3]) + red[3][3];
  *(f32x4*)(partial + (long)blockIdx.x * 4) = out;
}

// One block.  The chunk ranges of the parameters are rebuilt from the table's parameter column: a chunk whose left neighbour names
// another parameter opens its parameter's range, one whose right neighbour does closes it (LDS, 8 P bytes).  The column only selects
// ranges: the index is clamped to [0, P) and a range lies in [0, C] by construction, so a table that breaks its contract moves sums
// between parameters and cannot make partial or the log be read or written out of range.  Thread q then adds the partials of parameter
// q in chunk order, scales grad_sq by 1 / grad_scale^2 and writes its four words of the record in slot n_recorded % capacity; thread 0
// writes the record's header and, last, n_recorded + 1.  n_recorded is read by every thread in front of the first barrier and written
// behind the last one.  Nothing at or beyond log[4 + capacity * (4 + 4 P)] is written.
__global__ __launch_bounds__(256) void health_fold_kernel(const float* __restrict__ partial, const long long* __restrict__ chunks, int C, int P,
                                                          const float* __restrict__ state, const int* __restrict__ ctl,
                                                          const float* __restrict__ grad_scale, int every, int capacity,
                                                          int* __restrict__ log) {
  const int kind = health_kind(state, ctl, every);
  if (kind == HK_NONE) return;                                   // block-uniform: nobody reaches the barriers below
  extern __shared__ int hf_lds[];
  int* first = hf_lds;                                           // [P]
  int* last = hf_lds + P;                                        // [P]
  const unsigned n_rec = (unsigned)log[0];
  const float step = state[ST_STEP], norm = state[ST_GRAD_NORM];
  for (int q = threadIdx.x; q < P; q += 256) first[q] = last[q] = 0;
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const long long par = chunks[(long)c * 4 + 2];
    const int q = par < 0 ? 0 : (par >= P ? P - 1 : (int)par);
    if (c == 0 || chunks[(long)(c - 1) * 4 + 2] != par) first[q] = c;
    if (c == C - 1 || chunks[(long)(c + 1) * 4 + 2] != par) last[q] = c + 1;
  }
  __syncthreads();
  const long R = HL_REC_HEADER + 4 * (long)P;
  int* rec = log + HL_HEADER + (long)(n_rec % (unsigned)capacity) * R;
  const float gs = grad_scale != nullptr ? grad_scale[0] : 1.f;
  const float inv = 1.f / (gs * gs);
  for (int q = threadIdx.x; q < P; q += 256) {
    const int c0 = first[q], c1 = last[q];
    float gsq = 0.f, wsq = 0.f, usq = 0.f;
    int bad = 0;
#pragma unroll 8
    for (int c = c0; c < c1; ++c) {
      const f32x4 x = *(const f32x4*)(partial + (long)c * 4);
      gsq += x[0]; bad += __float_as_int(x[1]); wsq += x[2]; usq += x[3];
    }
    rec[HL_REC_HEADER + q] = __float_as_int(gsq * inv);
    rec[HL_REC_HEADER + P + q] = bad;
    rec[HL_REC_HEADER + 2 * P + q] = __float_as_int(wsq);
    rec[HL_REC_HEADER + 3 * P + q] = __float_as_int(usq);
  }
  if (threadIdx.x == 0) {
    rec[0] = __float_as_int(step); rec[1] = kind; rec[2] = __float_as_int(norm); rec[3] = 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) log[0] = (int)(n_rec + 1u);
}

// [x, x + nx) and [y, y + ny) share a byte
static bool spans_overlap(const void* x, size_t nx, const void* y, size_t ny) {
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
  return a < b ? b - a < nx : a - b < ny;
}

extern "C" int hriemo_health_sweep(const float* g, const float* p, const float* m, const float* v, long n, const long long* chunks, int C,
                                   const float* hyper, const float* state, int G, const int* ctl, int every, float* partial,
                                   hipStream_t st) {
  HRIEMO_CHECK(n > 0 && n % 4 == 0, "health_sweep: n=%ld must be a positive multiple of 4", n);
  HRIEMO_CHECK(g != nullptr && p != nullptr && m != nullptr && v != nullptr && partial != nullptr, "health_sweep: g, p, m, v and partial are required");
  HRIEMO_CHECK(((uintptr_t)g % 16) == 0 && ((uintptr_t)p % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                   ((uintptr_t)partial % 16) == 0, "health_sweep: unaligned buffer");
  HRIEMO_CHECK(C >= 1 && C <= HL_MAX_CHUNKS, "health_sweep: C=%d chunks (1 .. %d)", C, (int)HL_MAX_CHUNKS);
  HRIEMO_CHECK(chunks != nullptr && ((uintptr_t)chunks % 8) == 0, "health_sweep: chunks (int64 [C][4]) is required, 8-byte aligned");
  HRIEMO_CHECK(hyper != nullptr && state != nullptr, "health_sweep: hyper and state are required");
  HRIEMO_CHECK(G >= 1 && G <= HL_MAX_GROUPS, "health_sweep: G=%d groups (1 .. %d)", G, (int)HL_MAX_GROUPS);
  HRIEMO_CHECK(((uintptr_t)ctl % 4) == 0, "health_sweep: ctl is the int32 step-control block in device memory (or NULL)");
  HRIEMO_CHECK(every >= 1, "health_sweep: every=%d must be >= 1", every);
  const size_t nb = (size_t)n * 4, pb = (size_t)C * 16;
  HRIEMO_CHECK(!spans_overlap(partial, pb, g, nb) && !spans_overlap(partial, pb, p, nb) && !spans_overlap(partial, pb, m, nb) &&
                   !spans_overlap(partial, pb, v, nb) && !spans_overlap(partial, pb, chunks, (size_t)C * 32) &&
                   !spans_overlap(partial, pb, state, (size_t)G * 32) && !spans_overlap(partial, pb, hyper, (size_t)G * 32),
               "health_sweep: partial overlaps g, p, m, v, chunks, hyper or state");
  hipLaunchKernelGGL(health_sweep_kernel, dim3(C), dim3(256), 0, st, g, p, m, v, n, chunks, hyper, state, G, ctl, every, partial);
  HRIEMO_LAUNCH_CHECK("health_sweep_kernel");
  return 0;
}

extern "C" int hriemo_health_fold(const float* partial, const long long* chunks, int C, int P, const float* state, const int* ctl,
                                  const float* grad_scale, int every, int capacity, int* log, hipStream_t st) {
  HRIEMO_CHECK(partial != nullptr && ((uintptr_t)partial % 16) == 0, "health_fold: partial (fp32 [C][4]) is required, 16-byte aligned");
  HRIEMO_CHECK(C >= 1 && C <= HL_MAX_CHUNKS, "health_fold: C=%d chunks (1 .. %d)", C, (int)HL_MAX_CHUNKS);
  HRIEMO_CHECK(P >= 1 && P <= HL_MAX_PARAMS, "health_fold: P=%d parameters (1 .. %d)", P, (int)HL_MAX_PARAMS);
  HRIEMO_CHECK(chunks != nullptr && ((uintptr_t)chunks % 8) == 0, "health_fold: chunks (int64 [C][4]) is required, 8-byte aligned");
  HRIEMO_CHECK(state != nullptr, "health_fold: state is required");
  HRIEMO_CHECK(((uintptr_t)ctl % 4) == 0, "health_fold: ctl is the int32 step-control block in device memory (or NULL)");
  HRIEMO_CHECK(every >= 1, "health_fold: every=%d must be >= 1", every);
  HRIEMO_CHECK(capacity >= 1 && capacity <= HL_MAX_CAPACITY, "health_fold: capacity=%d records (1 .. %d)", capacity, (int)HL_MAX_CAPACITY);
  HRIEMO_CHECK(log != nullptr && ((uintptr_t)log % 4) == 0, "health_fold: log (int32 words) is required, 4-byte aligned");
  const size_t lb = ((size_t)HL_HEADER + (size_t)capacity * (HL_REC_HEADER + 4 * (size_t)P)) * 4;
  HRIEMO_CHECK(!spans_overlap(log, lb, partial, (size_t)C * 16) && !spans_overlap(log, lb, chunks, (size_t)C * 32) &&
                   !spans_overlap(log, lb, state, 32) && (grad_scale == nullptr || !spans_overlap(log, lb, grad_scale, 4)) &&
                   (ctl == nullptr || !spans_overlap(log, lb, ctl, 16)),
               "health_fold: log overlaps partial, chunks, state, ctl or grad_scale");
  hipLaunchKernelGGL(health_fold_kernel, dim3(1), dim3(256), (size_t)P * 8, st, partial, chunks, C, P, state, ctl, grad_scale, every, capacity, log);
  HRIEMO_LAUNCH_CHECK("health_fold_kernel");
  return 0;
}
