// The activation log (hri-emo_amd/train.py: ActivationLog): per-site statistics of the activations of a pass and of the gradients
// that arrive at them -- sum of squares and abs-max over the finite elements, the number of non-finite elements and the first row
// that holds one -- written by the pass itself into a ring in device memory, so that a skipped update inside a captured step can
// be blamed on the sub-layer, sample and position where a non-finite value first appeared, without giving up the graph.
//   counters int32 [4]   {n_passes, n_recorded, 0, 0}: passes counted (record = 1) and records ever opened; zeroed to reset
//   window   int32 [4]   {open, slot, pass, 0}: written by the plan at the top of a pass, read by everything behind it
//   counts   int32 [2 S] chunk count of the latest probe of (half, site), index half * S + site; cleared by an opening plan
//   partial  fp32 [2 S][chunk_cap][8]  per chunk of AL_ROWS rows: {sumsq, absmax, n_bad (int32 bits), first_bad_row (int32 bits,
//                        -1: none), n_rows (int32 bits: the rows of the chunk that count), 0, 0, 0}
//   ring     int32       `capacity` records of 4 + 2 S * 8 words: {pass, halves (bit 0 forward, bit 1 gradient), 0, 0}, then for
//                        (half, site) at 4 + (half * S + site) * 8: {have, n_rows, n_bad, first_bad_row, absmax (fp32 bits),
//                        sumsq (fp32 bits), 0, 0}; record r of the run lives in slot r % capacity
// The plan is the only writer of counters and window and runs in front of every fork of the pass, so stream order alone keeps every
// reader behind it.  A probe or fold block that finds the window closed returns before its first load of data and before any
// barrier: one family of graphs serves recording and non-recording passes alike.
// Every sum has ONE fixed order (no floating-point atomics anywhere): a thread adds the elements of its vectors i = tid, tid + 256,
// ... of the chunk one after the other (fmaf(x, x, acc)), the wave adds its 64 lanes by the xor butterfly, thread 0 adds the four
// wave sums in index order; the fold does the same over the chunk partials c = tid, tid + 256, ....  The same pass from the same
// state gives the same bits.
#include "common.h"

enum { AL_ROWS = 32, AL_PARTIAL = 8, AL_ENTRY = 8, AL_REC_HEADER = 4 };
enum { AL_MAX_SITES = 1024, AL_MAX_CAPACITY = 1 << 20, AL_MAX_CHUNKS = 1 << 22 };
enum { AL_NONE = 0x7fffffff };

__device__ __forceinline__ bool al_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ int al_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int al_wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float al_wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

struct AlAcc {
  float sq, am;
  int bad, first, rows;
};

// the block's five values from its 256 threads' (fixed order: butterfly, then the four waves in index order); valid in thread 0
__device__ __forceinline__ AlAcc al_block_reduce(AlAcc a, float (*redf)[2], int (*redi)[3]) {
  a.sq = wave_sum(a.sq);
  a.am = al_wave_max(a.am);
  a.bad = al_wave_sum_int(a.bad);
  a.first = al_wave_min_int(a.first);
  a.rows = al_wave_sum_int(a.rows);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    redf[w][0] = a.sq; redf[w][1] = a.am;
    redi[w][0] = a.bad; redi[w][1] = a.first; redi[w][2] = a.rows;
  }
  __syncthreads();
  AlAcc o;
  o.sq = ((redf[0][0] + redf[1][0]) + redf[2][0]) + redf[3][0];
  o.am = fmaxf(fmaxf(redf[0][1], redf[1][1]), fmaxf(redf[2][1], redf[3][1]));
  o.bad = redi[0][0] + redi[1][0] + redi[2][0] + redi[3][0];
  o.first = min(min(redi[0][1], redi[1][1]), min(redi[2][1], redi[3][1]));
  o.rows = redi[0][2] + redi[1][2] + redi[2][2] + redi[3][2];
  return o;
}

// One block.  record = 0: the closed window and nothing else.  record = 1: the pass is counted; pass % every == 0 opens the window
// on slot n_recorded % capacity, clears that record and the chunk counts and advances n_recorded.  Both counters are read by every
// thread in front of the barrier and written by thread 0 behind it.
__global__ __launch_bounds__(256) void act_plan_kernel(int record, int every, int capacity, int S, int* __restrict__ counters,
                                                       int* __restrict__ window, int* __restrict__ counts, int* __restrict__ ring) {
  typedef __attribute__((ext_vector_type(4))) int i32x4;
  if (record == 0) {
    if (threadIdx.x == 0) *(i32x4*)window = (i32x4){0, 0, 0, 0};
    return;
  }
  const unsigned pass = (unsigned)counters[0], n_rec = (unsigned)counters[1];
  __syncthreads();
  const bool open = pass % (unsigned)every == 0u;
  const int slot = (int)(n_rec % (unsigned)capacity);
  const int RW = AL_REC_HEADER + 2 * S * AL_ENTRY;
  int* rec = ring + (long)slot * RW;
  if (open) {
    for (int i = threadIdx.x; i < RW; i += 256) rec[i] = i == 0 ? (int)pass : 0;
    for (int i = threadIdx.x; i < 2 * S; i += 256) counts[i] = 0;
  }
  if (threadIdx.x == 0) {
    *(i32x4*)window = (i32x4){open ? 1 : 0, open ? slot : 0, (int)pass, 0};
    counters[0] = (int)(pass + 1u);
    if (open) counters[1] = (int)(n_rec + 1u);
  }
}

// One block per chunk of AL_ROWS rows.  The first AL_ROWS threads decide for their row whether it counts and what its index in the
// padded numbering b * L + l is (LDS, -1: not counted):
//   packed (cu != NULL): b = the last of the B sequences with cu[b] <= r (binary search); counted iff b < nv, r < cu[b + 1] and
//                        l = r - cu[b] < L -- the filler sequence of a bucket plan, surplus rows and ghosts never count
//   padded:              b = r / L, l = r % L; counted iff b < nv and (kpm == NULL or kpm[r] == 0)
// with nv = clamp(*n_valid, 1, B) (NULL: B).  Whatever cu holds, the only addresses formed from it are indices into prow's values,
// which are compared, never dereferenced: x is read at rows < n_rows only.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void act_probe_kernel(const T* __restrict__ x, int n_rows, int d, long ld, const int* __restrict__ cu,
                                                        const unsigned char* __restrict__ kpm, int B, int L, const int* __restrict__ n_valid,
                                                        const int* __restrict__ window, int k, float* __restrict__ partial,
                                                        int* __restrict__ counts) {
  if (window[0] == 0) return;                                    // block-uniform: nobody reaches a load of x or a barrier
  __shared__ int prow[AL_ROWS];
  __shared__ float redf[4][2];
  __shared__ int redi[4][3];
  int nv = B;
  if (n_valid != nullptr) {
    nv = n_valid[0];
    nv = nv < 1 ? 1 : (nv > B ? B : nv);
  }
  const int r0 = blockIdx.x * AL_ROWS;
  AlAcc a;
  a.sq = 0.f; a.am = 0.f; a.bad = 0; a.first = AL_NONE; a.rows = 0;
  if (threadIdx.x < AL_ROWS) {
    const int r = r0 + threadIdx.x;
    int pr = -1;
    if (r < n_rows) {
      if (cu != nullptr) {
        int lo = 0, hi = B;
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (cu[mid] <= r) lo = mid; else hi = mid;
        }
        const int c0 = cu[lo], c1 = cu[lo + 1], l = r - c0;
        if (lo < nv && l >= 0 && r < c1 && l < L) pr = lo * L + l;
      } else {
        const int b = r / L;
        if (b < nv && (kpm == nullptr || kpm[r] == 0)) pr = r;
      }
    }
    prow[threadIdx.x] = pr;
    a.rows = pr >= 0 ? 1 : 0;
  }
  __syncthreads();
  const int nvr = d / VEC;
  const int rows_here = min((int)AL_ROWS, n_rows - r0);
  const int total = rows_here * nvr;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int rr = i / nvr, c = i - rr * nvr;
    const int pr = prow[rr];
    if (pr < 0) continue;
    const T* src = x + (long)(r0 + rr) * ld + (long)c * VEC;
    float f[VEC];
    if constexpr (VEC == 8) {
      bf8_to_f32(*(const bf16x8*)src, f);
    } else if constexpr (VEC == 4) {
      const f32x4 v = *(const f32x4*)src;
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = v[e];
    } else {
      f[0] = (float)src[0];
    }
    int bad = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const bool fin = al_finite(f[e]);
      const float v = fin ? f[e] : 0.f;
      bad += fin ? 0 : 1;
      a.sq = __builtin_fmaf(v, v, a.sq);
      a.am = fmaxf(a.am, fabsf(v));
    }
    a.bad += bad;
    if (bad != 0) a.first = min(a.first, pr);
  }
  const AlAcc o = al_block_reduce(a, redf, redi);
  if (threadIdx.x != 0) return;
  float* out = partial + (long)blockIdx.x * AL_PARTIAL;
  f32x4 w0, w1;
  w0[0] = o.sq; w0[1] = o.am; w0[2] = __int_as_float(o.bad); w0[3] = __int_as_float(o.first == AL_NONE ? -1 : o.first);
  w1[0] = __int_as_float(o.rows); w1[1] = 0.f; w1[2] = 0.f; w1[3] = 0.f;
  *(f32x4*)out = w0;
  *(f32x4*)(out + 4) = w1;
  if (blockIdx.x == 0) counts[k] = (int)gridDim.x;
}

// One block per site.  The slot and the chunk count are device data and are clamped (slot into [0, capacity), the count into
// [0, chunk_cap]) before they address the ring or partial.
__global__ __launch_bounds__(256) void act_fold_kernel(const float* __restrict__ partial, const int* __restrict__ counts,
                                                       const int* __restrict__ window, int half, int S, int chunk_cap, int capacity,
                                                       int* __restrict__ ring) {
  typedef __attribute__((ext_vector_type(4))) int i32x4;
  if (window[0] == 0) return;                                    // block-uniform
  __shared__ float redf[4][2];
  __shared__ int redi[4][3];
  const int site = blockIdx.x, k = half * S + site;
  int slot = window[1];
  slot = slot < 0 ? 0 : (slot >= capacity ? capacity - 1 : slot);
  int C = counts[k];
  C = C < 0 ? 0 : (C > chunk_cap ? chunk_cap : C);
  int* rec = ring + (long)slot * (AL_REC_HEADER + 2 * S * AL_ENTRY);
  if (site == 0 && threadIdx.x == 0) {
    rec[0] = window[2];
    rec[1] = rec[1] | (1 << half);
  }
  if (C == 0) return;                                            // block-uniform: the site keeps have = 0
  const float* p = partial + (long)k * chunk_cap * AL_PARTIAL;
  AlAcc a;
  a.sq = 0.f; a.am = 0.f; a.bad = 0; a.first = AL_NONE; a.rows = 0;
  for (int c = threadIdx.x; c < C; c += 256) {
    const f32x4 w0 = *(const f32x4*)(p + (long)c * AL_PARTIAL);
    const int rows = __float_as_int(p[(long)c * AL_PARTIAL + 4]);
    const int first = __float_as_int(w0[3]);
    a.sq += w0[0];
    a.am = fmaxf(a.am, w0[1]);
    a.bad += __float_as_int(w0[2]);
    if (first >= 0) a.first = min(a.first, first);
    a.rows += rows;
  }
  const AlAcc o = al_block_reduce(a, redf, redi);
  if (threadIdx.x != 0) return;
  int* e = rec + AL_REC_HEADER + (long)k * AL_ENTRY;
  *(i32x4*)e = (i32x4){1, o.rows, o.bad, o.first == AL_NONE ? -1 : o.first};
  *(i32x4*)(e + 4) = (i32x4){__float_as_int(o.am), __float_as_int(o.sq), 0, 0};
}

static bool al_overlap(const void* x, size_t nx, const void* y, size_t ny) {
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
  return a < b ? b - a < nx : a - b < ny;
}

static size_t al_ring_bytes(int capacity, int S) { return (size_t)capacity * (AL_REC_HEADER + 2 * (size_t)S * AL_ENTRY) * 4; }

extern "C" int hriemo_act_probe_rows(void) { return AL_ROWS; }

extern "C" int hriemo_act_log_plan(int record, int every, int capacity, int n_sites, int* counters, int* window, int* counts, int* ring,
                                   hipStream_t st) {
  HRIEMO_CHECK(record == 0 || record == 1, "act_log_plan: record=%d (0 | 1)", record);
  HRIEMO_CHECK(every >= 1, "act_log_plan: every=%d must be >= 1", every);
  HRIEMO_CHECK(capacity >= 1 && capacity <= AL_MAX_CAPACITY, "act_log_plan: capacity=%d records (1 .. %d)", capacity, (int)AL_MAX_CAPACITY);
  HRIEMO_CHECK(n_sites >= 1 && n_sites <= AL_MAX_SITES, "act_log_plan: n_sites=%d (1 .. %d)", n_sites, (int)AL_MAX_SITES);
  HRIEMO_CHECK(counters != nullptr && window != nullptr && counts != nullptr && ring != nullptr,
               "act_log_plan: counters, window, counts and ring are required");
  HRIEMO_CHECK(((uintptr_t)counters % 16) == 0 && ((uintptr_t)window % 16) == 0 && ((uintptr_t)counts % 4) == 0 && ((uintptr_t)ring % 16) == 0,
               "act_log_plan: counters, window and ring are 16-byte aligned int32 blocks, counts 4-byte aligned");
  const size_t rb = al_ring_bytes(capacity, n_sites), cb = (size_t)2 * n_sites * 4;
  HRIEMO_CHECK(!al_overlap(ring, rb, counters, 16) && !al_overlap(ring, rb, window, 16) && !al_overlap(ring, rb, counts, cb) &&
                   !al_overlap(counts, cb, counters, 16) && !al_overlap(counts, cb, window, 16) && !al_overlap(counters, 16, window, 16),
               "act_log_plan: counters, window, counts and ring overlap");
  hipLaunchKernelGGL(act_plan_kernel, dim3(1), dim3(256), 0, st, record, every, capacity, n_sites, counters, window, counts, ring);
  HRIEMO_LAUNCH_CHECK("act_plan_kernel");
  return 0;
}

extern "C" int hriemo_act_probe(const void* x, int dtype, int n_rows, int d, long ld, const int* cu_seqlens, const unsigned char* kpm, int B,
                                int L, const int* n_valid, const int* window, int site, int half, int n_sites, int chunk_cap, float* partial,
                                int* counts, hipStream_t st) {
  HRIEMO_CHECK(x != nullptr && window != nullptr && partial != nullptr && counts != nullptr, "act_probe: x, window, partial and counts are required");
  HRIEMO_CHECK(dtype == 0 || dtype == 1, "act_probe: dtype=%d (0: bf16, 1: fp32)", dtype);
  HRIEMO_CHECK(n_rows >= 1 && d >= 1 && ld >= d, "act_probe: n_rows=%d, d=%d, ld=%ld (n_rows, d >= 1, ld >= d)", n_rows, d, ld);
  HRIEMO_CHECK(B >= 1 && L >= 1 && (long)B * L < 0x7fffffffL, "act_probe: B=%d sequences of up to L=%d rows (B, L >= 1, B * L < 2^31)", B, L);
  HRIEMO_CHECK(cu_seqlens == nullptr || kpm == nullptr, "act_probe: packed rows carry their lengths; no key_padding_mask");
  HRIEMO_CHECK(cu_seqlens != nullptr || (long)n_rows <= (long)B * L, "act_probe: %d padded rows, but B * L = %ld", n_rows, (long)B * L);
  HRIEMO_CHECK(n_sites >= 1 && n_sites <= AL_MAX_SITES && site >= 0 && site < n_sites && (half == 0 || half == 1),
               "act_probe: site=%d of n_sites=%d (1 .. %d), half=%d (0 | 1)", site, n_sites, (int)AL_MAX_SITES, half);
  const int chunks = (n_rows + AL_ROWS - 1) / AL_ROWS;
  HRIEMO_CHECK(chunk_cap >= 1 && chunk_cap <= AL_MAX_CHUNKS && chunks <= chunk_cap, "act_probe: %d rows are %d chunks, the log holds %d per site",
               n_rows, chunks, chunk_cap);
  HRIEMO_CHECK(((uintptr_t)window % 16) == 0 && ((uintptr_t)partial % 16) == 0 && ((uintptr_t)counts % 4) == 0 &&
                   ((uintptr_t)cu_seqlens % 4) == 0 && ((uintptr_t)n_valid % 4) == 0 && ((uintptr_t)x % (dtype == 0 ? 2 : 4)) == 0,
               "act_probe: unaligned buffer");
  const size_t es = dtype == 0 ? 2 : 4;
  const size_t xb = ((size_t)(n_rows - 1) * (size_t)ld + (size_t)d) * es, pb = (size_t)2 * n_sites * chunk_cap * AL_PARTIAL * 4;
  HRIEMO_CHECK(!al_overlap(partial, pb, x, xb) && !al_overlap(partial, pb, window, 16) && !al_overlap(partial, pb, counts, (size_t)2 * n_sites * 4) &&
                   !al_overlap(counts, (size_t)2 * n_sites * 4, x, xb),
               "act_probe: partial or counts overlaps x, window or each other");
  const int k = half * n_sites + site;
  float* part = partial + (size_t)k * chunk_cap * AL_PARTIAL;
  const bool vec = ((uintptr_t)x % 16) == 0;
#define AL_LAUNCH(T, VEC)                                                                                                              \
  hipLaunchKernelGGL((act_probe_kernel<T, VEC>), dim3(chunks), dim3(256), 0, st, (const T*)x, n_rows, d, ld, cu_seqlens, kpm, B, L, \
                     n_valid, window, k, part, counts)
  if (dtype == 0) {
    if (vec && d % 8 == 0 && ld % 8 == 0) AL_LAUNCH(bf16_t, 8); else AL_LAUNCH(bf16_t, 1);
  } else {
    if (vec && d % 4 == 0 && ld % 4 == 0) AL_LAUNCH(float, 4); else AL_LAUNCH(float, 1);
  }
#undef AL_LAUNCH
  HRIEMO_LAUNCH_CHECK("act_probe_kernel");
  return 0;
}

extern "C" int hriemo_act_log_fold(const float* partial, const int* counts, const int* window, int half, int n_sites, int chunk_cap,
                                   int capacity, int* ring, hipStream_t st) {
  HRIEMO_CHECK(partial != nullptr && counts != nullptr && window != nullptr && ring != nullptr, "act_log_fold: partial, counts, window and ring are required");
  HRIEMO_CHECK(half == 0 || half == 1, "act_log_fold: half=%d (0 | 1)", half);
  HRIEMO_CHECK(n_sites >= 1 && n_sites <= AL_MAX_SITES, "act_log_fold: n_sites=%d (1 .. %d)", n_sites, (int)AL_MAX_SITES);
  HRIEMO_CHECK(chunk_cap >= 1 && chunk_cap <= AL_MAX_CHUNKS, "act_log_fold: chunk_cap=%d (1 .. %d)", chunk_cap, (int)AL_MAX_CHUNKS);
  HRIEMO_CHECK(capacity >= 1 && capacity <= AL_MAX_CAPACITY, "act_log_fold: capacity=%d records (1 .. %d)", capacity, (int)AL_MAX_CAPACITY);
  HRIEMO_CHECK(((uintptr_t)partial % 16) == 0 && ((uintptr_t)counts % 4) == 0 && ((uintptr_t)window % 16) == 0 && ((uintptr_t)ring % 16) == 0,
               "act_log_fold: unaligned buffer");
  const size_t rb = al_ring_bytes(capacity, n_sites), pb = (size_t)2 * n_sites * chunk_cap * AL_PARTIAL * 4;
  HRIEMO_CHECK(!al_overlap(ring, rb, partial, pb) && !al_overlap(ring, rb, counts, (size_t)2 * n_sites * 4) && !al_overlap(ring, rb, window, 16),
               "act_log_fold: ring overlaps partial, counts or window");
  hipLaunchKernelGGL(act_fold_kernel, dim3(n_sites), dim3(256), 0, st, partial, counts, window, half, n_sites, chunk_cap, capacity, ring);
  HRIEMO_LAUNCH_CHECK("act_fold_kernel");
  return 0;
}
