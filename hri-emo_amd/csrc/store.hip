// hriemo_gather_rows: a batch assembled from a device-resident feature store (data.DeviceFeatureStore) in one launch per operand.
// The store holds every utterance's valid rows back to back; a batch is a list of utterance ids.  Segment i of the plan copies the
// rows offsets[ids[i]] .. offsets[ids[i]+1] of the store to the rows dst_cu[i] .. dst_cu[i+1] of the destination; the rows from
// dst_cu[n] to dst_rows become zero (the tail the packed step's static row sources carry), nothing at or behind row dst_rows is
// written.  A pure copy: memory bound, no arithmetic on the values, any element type (the kernel sees bytes).
//
// Work is cut by the DESTINATION: chunk c is the 16-byte-aligned piece of destination memory at absolute address
// (dst & ~15) + 16 c, so a chunk that lies inside one segment is always written with ONE 16-byte store, whatever the phase of its
// source.  The source of such a chunk is read at the widest width its address allows: 16 bytes when source and destination agree
// modulo 16 (every row a multiple of 16 bytes: 768 x bf16, 300 x fp32), two 8-byte loads, four 4-byte loads, ... when they do not
// (74 x fp32 is 296 bytes a row: utterance starts fall on 8-byte boundaries and the phase changes from segment to segment; 5 x fp16
// is 10 bytes a row).  A chunk that straddles a segment boundary, the destination's first or last byte or the end of the copied
// rows goes byte by byte; there are at most n + 2 of those per launch unless the rows themselves are shorter than a chunk.
//
// The owning segment of a destination byte is found by a binary search of the segment boundaries (bytes, in LDS: n is a few
// hundred at most).  A thread's chunks lie 4 KiB apart and a segment is hundreds of rows, so the segment found for one chunk is
// kept in registers and the search runs again only when a chunk leaves it.
//
// The plan is device data written by the host from its own lengths.  For memory safety only, every dst_cu entry is clamped to
// [0, dst_rows] and a segment never reads past the rows its utterance owns in the store (the bytes behind them become zero); the
// ids themselves are checked by the host before anything is enqueued -- the kernel has no way to know how long `offsets` is.
#include "common.h"

#define GR_THREADS 256
#define GR_CHUNKS 8            // 16-byte destination chunks per thread, in two groups of four (four loads in flight per lane)
#define GR_MAX_N 2048          // segments per launch: 3 int64 tables of LDS, (3 n + 1) x 8 bytes = 49 160 at the cap

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

enum { GR_SKIP = 0, GR_SEG = 1, GR_ZERO = 2 };

// the segment a thread is in: destination bytes [lo, hi), source byte = destination byte + delta, the first src_len bytes of it exist
struct GrSeg {
  long long lo, hi, delta, src_len;
  int kind;
};

__device__ __forceinline__ void gr_locate(long long x, const long long* segb, const long long* delta, const long long* slen, int n,
                                          long long total, GrSeg& s) {
  // upper bound: the first k in [0, n] with segb[k] > x; the owner is k - 1
  int lo = 0, hi = n + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (segb[mid] > x) hi = mid; else lo = mid + 1;
  }
  const int seg = lo - 1;
  if (seg < 0) {                       // in front of dst_cu[0]: not part of the plan, left as it is
    s.kind = GR_SKIP; s.lo = 0; s.hi = segb[0]; s.delta = 0; s.src_len = 0;
  } else if (seg >= n) {               // behind the last segment: the zero tail
    s.kind = GR_ZERO; s.lo = segb[n]; s.hi = total; s.delta = 0; s.src_len = 0;
  } else {
    s.kind = GR_SEG; s.lo = segb[seg]; s.hi = segb[seg + 1]; s.delta = delta[seg]; s.src_len = slen[seg];
  }
}

// 16 source bytes at the widest width the address allows
__device__ __forceinline__ u32x4 gr_load16(const unsigned char* __restrict__ p) {
  const uintptr_t a = (uintptr_t)p;
  u32x4 v;
  if ((a & 15) == 0) {
    v = *(const u32x4*)p;
  } else if ((a & 7) == 0) {
    const u32x2 q0 = *(const u32x2*)p, q1 = *(const u32x2*)(p + 8);
    v = (u32x4){q0.x, q0.y, q1.x, q1.y};
  } else if ((a & 3) == 0) {
    const unsigned int* q = (const unsigned int*)p;
    v = (u32x4){q[0], q[1], q[2], q[3]};
  } else if ((a & 1) == 0) {
    const unsigned short* q = (const unsigned short*)p;
    v = (u32x4){q[0] | ((unsigned)q[1] << 16), q[2] | ((unsigned)q[3] << 16), q[4] | ((unsigned)q[5] << 16), q[6] | ((unsigned)q[7] << 16)};
  } else {
#pragma unroll
    for (int w = 0; w < 4; ++w)
      v[w] = p[4 * w] | ((unsigned)p[4 * w + 1] << 8) | ((unsigned)p[4 * w + 2] << 16) | ((unsigned)p[4 * w + 3] << 24);
  }
  return v;
}

__global__ __launch_bounds__(GR_THREADS) void gather_rows_kernel(const unsigned char* __restrict__ store, long long row_bytes,
                                                                 const long long* __restrict__ offsets, const int* __restrict__ plan, int n,
                                                                 unsigned char* __restrict__ dst, long long dst_rows, int head) {
  extern __shared__ __attribute__((aligned(16))) long long gr_lds[];
  long long* segb = gr_lds;                  // [n + 1] destination byte at which segment i starts; [n]: where the zero tail starts
  long long* delta = segb + (n + 1);         // [n] source byte - destination byte
  long long* slen = delta + n;               // [n] bytes the utterance owns in the store
  const int* ids = plan;
  const int* cu = plan + n;
  for (int i = threadIdx.x; i <= n; i += GR_THREADS) {
    long long c0 = cu[i];
    c0 = c0 < 0 ? 0 : (c0 > dst_rows ? dst_rows : c0);
    segb[i] = c0 * row_bytes;
    if (i < n) {
      const long long id = ids[i];
      const long long o0 = offsets[id], o1 = offsets[id + 1];
      delta[i] = (o0 - c0) * row_bytes;
      slen[i] = (o1 > o0 ? o1 - o0 : 0) * row_bytes;
    }
  }
  __syncthreads();
  const long long total = dst_rows * row_bytes;
  GrSeg s;
  s.kind = GR_SKIP; s.lo = 0; s.hi = 0; s.delta = 0; s.src_len = 0;     // empty: the first chunk searches

  // one chunk: destination bytes [x, x + 16), dst + x is 16-byte aligned
  auto chunk = [&](long long x) {
    if (x >= 0 && x + 16 <= total) {
      if (x < s.lo || x >= s.hi) gr_locate(x, segb, delta, slen, n, total, s);
      if (x >= s.lo && x + 16 <= s.hi) {
        if (s.kind == GR_SKIP) return;
        if (s.kind == GR_ZERO) {
          *(u32x4*)(dst + x) = (u32x4){0u, 0u, 0u, 0u};
          return;
        }
        if (x - s.lo + 16 <= s.src_len) {
          *(u32x4*)(dst + x) = gr_load16(store + (x + s.delta));
          return;
        }
      }
    }
    for (int b = 0; b < 16; ++b) {            // a boundary chunk: every byte finds its own segment
      const long long xb = x + b;
      if (xb < 0 || xb >= total) continue;
      if (xb < s.lo || xb >= s.hi) gr_locate(xb, segb, delta, slen, n, total, s);
      if (s.kind == GR_SKIP) continue;
      unsigned char v = 0;
      if (s.kind == GR_SEG && xb >= s.lo && xb - s.lo < s.src_len) v = store[xb + s.delta];
      dst[xb] = v;
    }
  };

  const long long c0 = (long long)blockIdx.x * (GR_THREADS * GR_CHUNKS) + threadIdx.x;
#pragma unroll 1
  for (int g = 0; g < GR_CHUNKS; g += 4) {
    const long long x0 = (c0 + (long long)g * GR_THREADS) * 16 - head;
    const long long step = (long long)GR_THREADS * 16;
    if (x0 >= total) break;
    const long long x3 = x0 + 3 * step;
    if (x0 >= 0 && x3 + 16 <= total) {
      if (x0 < s.lo || x0 >= s.hi) gr_locate(x0, segb, delta, slen, n, total, s);
      const unsigned char* p = store + (x0 + s.delta);
      if (s.kind == GR_SEG && x0 >= s.lo && x3 + 16 <= s.hi && x3 - s.lo + 16 <= s.src_len && ((uintptr_t)p & 15) == 0) {
        // the common case: four chunks of one segment whose source agrees with the destination modulo 16
        const u32x4 v0 = *(const u32x4*)p, v1 = *(const u32x4*)(p + step), v2 = *(const u32x4*)(p + 2 * step), v3 = *(const u32x4*)(p + 3 * step);
        *(u32x4*)(dst + x0) = v0;
        *(u32x4*)(dst + x0 + step) = v1;
        *(u32x4*)(dst + x0 + 2 * step) = v2;
        *(u32x4*)(dst + x3) = v3;
        continue;
      }
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const long long x = x0 + j * step;
      if (x < total) chunk(x);
    }
  }
}

}  // namespace

extern "C" int hriemo_gather_rows(const void* store, long row_bytes, const long long* offsets, const int* plan, int n, void* dst,
                                  long dst_rows, hipStream_t st) {
  HRIEMO_CHECK(store != nullptr && offsets != nullptr && plan != nullptr && dst != nullptr, "gather_rows: a null pointer");
  HRIEMO_CHECK(n >= 1 && n <= GR_MAX_N, "gather_rows: n=%d segments (1 .. %d)", n, GR_MAX_N);
  HRIEMO_CHECK(row_bytes >= 1 && row_bytes <= (1L << 30), "gather_rows: row_bytes=%ld", row_bytes);
  HRIEMO_CHECK(dst_rows >= 1 && dst_rows <= (1L << 31), "gather_rows: dst_rows=%ld", dst_rows);
  HRIEMO_CHECK(((uintptr_t)plan % 4) == 0 && ((uintptr_t)offsets % 8) == 0, "gather_rows: unaligned plan or offsets");
  const int head = (int)((uintptr_t)dst & 15);
  const long long chunks = ((long long)dst_rows * row_bytes + head + 15) / 16;
  const long long blocks = (chunks + GR_THREADS * GR_CHUNKS - 1) / (GR_THREADS * GR_CHUNKS);
  HRIEMO_CHECK(blocks <= 0x7fffffffLL, "gather_rows: destination of %ld rows x %ld bytes is too large", dst_rows, row_bytes);
  const size_t lds = (size_t)(3 * n + 1) * sizeof(long long);
  hriemo_prof_begin(HP_ROWOPS, st);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(GR_THREADS), lds, st, (const unsigned char*)store, (long long)row_bytes,
                     offsets, plan, n, (unsigned char*)dst, (long long)dst_rows, head);
  HRIEMO_LAUNCH_CHECK("gather_rows_kernel");
  hriemo_prof_end(HP_ROWOPS, st, 2.0 * (double)dst_rows * (double)row_bytes);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// hriemo_gather_rows_aug: the gather above with seeded train-time augmentation of the rows it moves (data.StoreAugment): time
// masking, additive noise, modality dropout.  Same division of work -- 16-byte destination chunks, segment tables in LDS, gr_locate,
// the widest source load the address allows, boundary chunks piece by piece, the zero tail, the clamps -- but the kernel is typed
// on the element (fp32, bf16, fp16): a row and a column are needed per element, and the noise is arithmetic on the value.
//
// Everything random comes from the counter hash of common.h and is keyed by the utterance's STORE id u, never by its position in
// the batch, so an utterance's augmentation does not depend on what else is in the batch or on the data-parallel shard:
//   ku = fmix32(site_key(seed, AUG_SITE + modality, draw) + u * DROP_CA)                  modality: 1 audio, 2 text
//   drop:  rd = fmix32(site_key(seed, AUG_SITE, draw) + u * DROP_CA) & 0xffff; every row of the utterance is zero iff
//          thr_lo <= rd < thr_hi.  One draw for both modalities: the audio launch takes [0, thr_a), the text launch
//          [thr_a, thr_a + thr_t), so the two are never dropped together.
//   spans: j = 0 .. spans - 1: h = fmix32(ku + (j + 1) * DROP_CB); W = min(max_width, (L * frac16) >> 16);
//          w = ((h & 0xffff) * (W + 1)) >> 16; s = ((h >> 16) * (L - w + 1)) >> 16; rows [s, s + w) are zero.  L: the utterance's rows.
//   noise: kn = fmix32(ku + 0x27d4eb2f); element (r, c): h = mix24(kn + r * DROP_CA + c * DROP_CB), k = the sum of h's four bytes
//          - 510 (Irwin-Hall of four 8-bit uniforms: mean 0 exactly, variance 21845, |k| <= 510);
//          out = rne(x + noise_scale * k), product and sum rounded separately in fp32 (tests/augment_reference.py forms the same
//          two roundings in numpy.float32).  noise_scale == 0: no hash, kept elements are bit copies (NaN patterns pass).
// Noise first, then the zeros: a masked row is +0.0 bits and needs no source read.  The per-segment facts -- four spans as
// (s << 16 | w), a dropped utterance being the span [0, L), and kn -- are worked out once per block in the LDS prologue with
// fmix32; per element there is one mix24 (24-bit multiplies, full rate), one v_sad_u8 and the two fp32 operations.
#define GA_MAX_N 512           // segments per launch: the three int64 tables and 5 words per segment, 22 536 bytes of LDS at the cap
// gr_locate is reused as it is; it does not say WHICH segment it found, so the slen table carries the segment's index above the
// byte count (a destination is at most 2^31 rows x 2^18 bytes = 2^49 bytes, so a count clamped to 50 bits compares as before)
#define GA_OWNER_SHIFT 50
#define GA_LEN_MASK ((1LL << GA_OWNER_SHIFT) - 1)
#define AUG_SITE 0x41554700u   // far from the sites modules draw (_ops.new_site_base(): 4, 8, 12, ...)

namespace {

enum { GA_F32 = 0, GA_BF16 = 1, GA_F16 = 2 };

template <int DT> struct GaElem;
template <> struct GaElem<GA_F32> {
  static constexpr int ES = 4;
  static __device__ __forceinline__ float up(uint32_t b) { return __uint_as_float(b); }
  static __device__ __forceinline__ uint32_t down(float f) { return __float_as_uint(f); }
};
template <> struct GaElem<GA_BF16> {
  static constexpr int ES = 2;
  static __device__ __forceinline__ float up(uint32_t b) { return __uint_as_float(b << 16); }
  static __device__ __forceinline__ uint32_t down(float f) {            // round to nearest even; a NaN stays a (quiet) NaN
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
};
template <> struct GaElem<GA_F16> {
  static constexpr int ES = 2;
  static __device__ __forceinline__ float up(uint32_t b) { return (float)__builtin_bit_cast(_Float16, (unsigned short)b); }
  static __device__ __forceinline__ uint32_t down(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
};

// what a thread keeps of its current segment beside GrSeg: the masked row ranges and the noise key
struct GaSeg {
  uint32_t sp[4];              // (first row << 16) | rows; rows == 0: no span
  uint32_t kn;
};

__device__ __forceinline__ bool ga_masked(const GaSeg& a, uint32_t r) {
  return (r - (a.sp[0] >> 16)) < (a.sp[0] & 0xffffu) || (r - (a.sp[1] >> 16)) < (a.sp[1] & 0xffffu) ||
         (r - (a.sp[2] >> 16)) < (a.sp[2] & 0xffffu) || (r - (a.sp[3] >> 16)) < (a.sp[3] & 0xffffu);
}

// element bits + noise_scale * k(hash input hb), the two roundings apart
template <int DT>
__device__ __forceinline__ uint32_t ga_noise(uint32_t bits, uint32_t hb, float scale) {
#pragma clang fp contract(off)       // __fmul_rn / __fadd_rn are plain operators to this compiler and fuse into an FMA when inlined
  const uint32_t h = mix24(hb);
  const int k = (int)__builtin_amdgcn_sad_u8(h, 0u, 0u) - 510;
  const float nz = scale * (float)k;                   // rounded here,
  return GaElem<DT>::down(GaElem<DT>::up(bits) + nz);  // and here: two v_*_f32, never an FMA
}

template <int DT>
__device__ __forceinline__ uint32_t ga_get(const u32x4& v, int e) {
  if (GaElem<DT>::ES == 4) return v[e];
  return (v[e >> 1] >> (16 * (e & 1))) & 0xffffu;
}

// the 16 / ES elements of a chunk that lies in ONE segment, its first element being (row r, column c) of the utterance.
// ONE_ROW: the chunk cannot leave row r (rows a multiple of 16 bytes, destination 16-byte aligned).
template <int DT, bool ONE_ROW>
__device__ __forceinline__ u32x4 ga_chunk(const u32x4& v, uint32_t r, uint32_t c, uint32_t row_elems, const GaSeg& a, bool noise, float scale) {
  constexpr int E = 16 / GaElem<DT>::ES;
  bool m = ga_masked(a, r);
  uint32_t hb = a.kn + r * DROP_CA + c * DROP_CB;
  u32x4 out = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (e > 0) {
      hb += DROP_CB;
      if (!ONE_ROW && ++c == row_elems) {
        c = 0;
        ++r;
        m = ga_masked(a, r);
        hb = a.kn + r * DROP_CA;
      }
    }
    uint32_t b = ga_get<DT>(v, e);
    if (noise) b = ga_noise<DT>(b, hb, scale);
    if (m) b = 0u;
    if (GaElem<DT>::ES == 4) out[e] = b; else out[e >> 1] |= b << (16 * (e & 1));
  }
  return out;
}

template <int DT>
__global__ __launch_bounds__(GR_THREADS) void gather_rows_aug_kernel(const unsigned char* __restrict__ store, int row_elems_i,
                                                                     const long long* __restrict__ offsets, const int* __restrict__ plan, int n,
                                                                     unsigned char* __restrict__ dst, long long dst_rows, int head, uint32_t key_m,
                                                                     uint32_t key_d, uint32_t thr_lo, uint32_t thr_hi, int spans, uint32_t max_width,
                                                                     uint32_t frac16, float scale) {
  constexpr int ES = GaElem<DT>::ES, E = 16 / ES;
  extern __shared__ __attribute__((aligned(16))) long long ga_lds[];
  long long* segb = ga_lds;                  // the three tables of gather_rows_kernel
  long long* delta = segb + (n + 1);
  long long* slen = delta + n;
  uint32_t* spt = (uint32_t*)(slen + n);     // [n][4] spans
  uint32_t* knt = spt + 4 * n;               // [n] noise keys
  const uint32_t row_elems = (uint32_t)row_elems_i;
  const long long row_bytes = (long long)row_elems * ES;
  const int* ids = plan;
  const int* cu = plan + n;
  for (int i = threadIdx.x; i <= n; i += GR_THREADS) {
    long long c0 = cu[i];
    c0 = c0 < 0 ? 0 : (c0 > dst_rows ? dst_rows : c0);
    segb[i] = c0 * row_bytes;
    if (i < n) {
      const long long id = ids[i];
      const long long o0 = offsets[id], o1 = offsets[id + 1];
      const long long rows = o1 > o0 ? o1 - o0 : 0;
      delta[i] = (o0 - c0) * row_bytes;
      const long long own = rows * row_bytes;
      slen[i] = (own < GA_LEN_MASK ? own : GA_LEN_MASK) | ((long long)i << GA_OWNER_SHIFT);      // gr_locate hands it back in src_len
      const uint32_t L = rows > 65535 ? 65535u : (uint32_t)rows;      // the host refuses stores with longer utterances
      const uint32_t u = (uint32_t)id;
      const uint32_t ku = fmix32(key_m + u * DROP_CA);
      const uint32_t rd = fmix32(key_d + u * DROP_CA) & 0xffffu;
      uint32_t sp[4] = {0u, 0u, 0u, 0u};
      if (rd >= thr_lo && rd < thr_hi) {
        sp[0] = L;                                                     // modality drop: rows [0, L)
      } else {
        const uint32_t frac = (L * frac16) >> 16;
        const uint32_t W = max_width < frac ? max_width : frac;
        for (int j = 0; j < spans; ++j) {
          const uint32_t h = fmix32(ku + (uint32_t)(j + 1) * DROP_CB);
          const uint32_t w = ((h & 0xffffu) * (W + 1u)) >> 16;
          const uint32_t s0 = ((h >> 16) * (L - w + 1u)) >> 16;
          sp[j] = (s0 << 16) | w;
        }
      }
      for (int j = 0; j < 4; ++j) spt[4 * i + j] = sp[j];
      knt[i] = fmix32(ku + 0x27d4eb2fu);
    }
  }
  __syncthreads();
  const long long total = dst_rows * row_bytes;
  const bool noise = scale != 0.0f;
  GrSeg s;
  s.kind = GR_SKIP; s.lo = 0; s.hi = 0; s.delta = 0; s.src_len = 0;     // empty: the first chunk searches
  GaSeg a;
  a.sp[0] = a.sp[1] = a.sp[2] = a.sp[3] = 0u; a.kn = 0u;

  auto locate = [&](long long x) {
    gr_locate(x, segb, delta, slen, n, total, s);
    if (s.kind == GR_SEG) {
      const int owner = (int)(s.src_len >> GA_OWNER_SHIFT);
      s.src_len &= GA_LEN_MASK;
      for (int j = 0; j < 4; ++j) a.sp[j] = spt[4 * owner + j];      // word reads: the table behind 3 n + 1 int64 is 8-byte aligned only
      a.kn = knt[owner];
    }
  };

  // one chunk: destination bytes [x, x + 16), dst + x is 16-byte aligned; x and every segment boundary are multiples of ES
  auto chunk = [&](long long x) {
    if (x >= 0 && x + 16 <= total) {
      if (x < s.lo || x >= s.hi) locate(x);
      if (x >= s.lo && x + 16 <= s.hi) {
        if (s.kind == GR_SKIP) return;
        if (s.kind == GR_ZERO) {
          *(u32x4*)(dst + x) = (u32x4){0u, 0u, 0u, 0u};
          return;
        }
        if (x - s.lo + 16 <= s.src_len) {
          const uint32_t ei = (uint32_t)((x - s.lo) / ES);            // < 65536 rows x 65535 elements
          const uint32_t r = ei / row_elems, c = ei - r * row_elems;
          *(u32x4*)(dst + x) = ga_chunk<DT, false>(gr_load16(store + (x + s.delta)), r, c, row_elems, a, noise, scale);
          return;
        }
      }
    }
    for (int e = 0; e < E; ++e) {             // a boundary chunk: every element finds its own segment
      const long long xb = x + e * ES;
      if (xb < 0 || xb >= total) continue;
      if (xb < s.lo || xb >= s.hi) locate(xb);
      if (s.kind == GR_SKIP) continue;
      uint32_t b = 0u;
      if (s.kind == GR_SEG && xb >= s.lo && xb - s.lo + ES <= s.src_len) {
        const uint32_t ei = (uint32_t)((xb - s.lo) / ES);
        const uint32_t r = ei / row_elems, c = ei - r * row_elems;
        if (!ga_masked(a, r)) {
          const unsigned char* p = store + (xb + s.delta);
          b = ES == 4 ? *(const uint32_t*)p : (uint32_t)*(const unsigned short*)p;
          if (noise) b = ga_noise<DT>(b, a.kn + r * DROP_CA + c * DROP_CB, scale);
        }
      }
      if (ES == 4) *(uint32_t*)(dst + xb) = b; else *(unsigned short*)(dst + xb) = (unsigned short)b;
    }
  };

  const bool one_row = head == 0 && (row_bytes & 15) == 0;     // every chunk inside a segment lies in one row
  const uint32_t row_chunks = (uint32_t)(row_bytes >> 4);
  const long long c0 = (long long)blockIdx.x * (GR_THREADS * GR_CHUNKS) + threadIdx.x;
#pragma unroll 1
  for (int g = 0; g < GR_CHUNKS; g += 4) {
    const long long x0 = (c0 + (long long)g * GR_THREADS) * 16 - head;
    const long long step = (long long)GR_THREADS * 16;
    if (x0 >= total) break;
    const long long x3 = x0 + 3 * step;
    if (one_row && x0 >= 0 && x3 + 16 <= total) {
      if (x0 < s.lo || x0 >= s.hi) locate(x0);
      const unsigned char* p = store + (x0 + s.delta);
      if (s.kind == GR_SEG && x0 >= s.lo && x3 + 16 <= s.hi && x3 - s.lo + 16 <= s.src_len && ((uintptr_t)p & 15) == 0) {
        // the common case: four chunks of one segment whose source agrees with the destination modulo 16; the row is needed once
        // per chunk, a masked chunk is not read, and the four loads are in flight together
        const uint32_t ci = (uint32_t)((x0 - s.lo) >> 4);             // < 65536 rows x 16384 chunks
        uint32_t r[4], c[4];
        bool m[4];
        u32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t cj = ci + (uint32_t)j * GR_THREADS;
          r[j] = cj / row_chunks;
          c[j] = (cj - r[j] * row_chunks) * E;
          m[j] = ga_masked(a, r[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = m[j] ? (u32x4){0u, 0u, 0u, 0u} : *(const u32x4*)(p + j * step);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (noise && !m[j]) v[j] = ga_chunk<DT, true>(v[j], r[j], c[j], row_elems, a, true, scale);
          *(u32x4*)(dst + x0 + j * step) = v[j];
        }
        continue;
      }
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const long long x = x0 + j * step;
      if (x < total) chunk(x);
    }
  }
}

}  // namespace

extern "C" int hriemo_gather_rows_aug(const void* store, int row_elems, int dtype, const long long* offsets, const int* plan, int n,
                                      void* dst, long dst_rows, long max_rows, unsigned long long seed, unsigned draw, int modality,
                                      unsigned thr_lo, unsigned thr_hi, int spans, unsigned max_width, unsigned frac16,
                                      float noise_scale, hipStream_t st) {
  HRIEMO_CHECK(store != nullptr && offsets != nullptr && plan != nullptr && dst != nullptr, "gather_rows_aug: a null pointer");
  HRIEMO_CHECK(n >= 1 && n <= GA_MAX_N, "gather_rows_aug: n=%d segments (1 .. %d)", n, GA_MAX_N);
  HRIEMO_CHECK(dtype == GA_F32 || dtype == GA_BF16 || dtype == GA_F16, "gather_rows_aug: dtype code %d (0 fp32, 1 bf16, 2 fp16)", dtype);
  HRIEMO_CHECK(row_elems >= 1 && row_elems <= 65535, "gather_rows_aug: row_elems=%d (1 .. 65535)", row_elems);
  HRIEMO_CHECK(dst_rows >= 1 && dst_rows <= (1L << 31), "gather_rows_aug: dst_rows=%ld", dst_rows);
  HRIEMO_CHECK(max_rows >= 0 && max_rows < 65536, "gather_rows_aug: an utterance of %ld rows (the span arithmetic is 16-bit: < 65536)", max_rows);
  HRIEMO_CHECK(modality == 1 || modality == 2, "gather_rows_aug: modality %d (1 audio, 2 text)", modality);
  HRIEMO_CHECK(thr_lo <= thr_hi && thr_hi <= 65536u, "gather_rows_aug: drop thresholds [%u, %u) (lo <= hi <= 65536)", thr_lo, thr_hi);
  HRIEMO_CHECK(spans >= 0 && spans <= 4, "gather_rows_aug: spans=%d (0 .. 4)", spans);
  HRIEMO_CHECK(frac16 <= 65536u, "gather_rows_aug: frac16=%u (a 16-bit fraction, at most 65536)", frac16);
  HRIEMO_CHECK(noise_scale == noise_scale && noise_scale >= 0.0f && noise_scale <= 3.0e38f, "gather_rows_aug: noise_scale=%g", (double)noise_scale);
  HRIEMO_CHECK(((uintptr_t)plan % 4) == 0 && ((uintptr_t)offsets % 8) == 0, "gather_rows_aug: unaligned plan or offsets");
  const long es = dtype == GA_F32 ? 4 : 2;
  HRIEMO_CHECK(((uintptr_t)store % es) == 0 && ((uintptr_t)dst % es) == 0, "gather_rows_aug: store or dst not aligned to the element");
  const long row_bytes = (long)row_elems * es;
  const int head = (int)((uintptr_t)dst & 15);
  const long long chunks = ((long long)dst_rows * row_bytes + head + 15) / 16;
  const long long blocks = (chunks + GR_THREADS * GR_CHUNKS - 1) / (GR_THREADS * GR_CHUNKS);
  HRIEMO_CHECK(blocks <= 0x7fffffffLL, "gather_rows_aug: destination of %ld rows x %ld bytes is too large", dst_rows, row_bytes);
  const size_t lds = (size_t)(3 * n + 1) * sizeof(long long) + (size_t)n * 5 * sizeof(uint32_t);
  const uint32_t key_m = site_key(seed, AUG_SITE + (uint32_t)modality, draw), key_d = site_key(seed, AUG_SITE, draw);
  auto kernel = dtype == GA_F32 ? gather_rows_aug_kernel<GA_F32> : dtype == GA_BF16 ? gather_rows_aug_kernel<GA_BF16> : gather_rows_aug_kernel<GA_F16>;
  hriemo_prof_begin(HP_ROWOPS, st);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(GR_THREADS), lds, st, (const unsigned char*)store, row_elems, offsets, plan, n,
                     (unsigned char*)dst, (long long)dst_rows, head, key_m, key_d, (uint32_t)thr_lo, (uint32_t)thr_hi, spans, (uint32_t)max_width,
                     (uint32_t)frac16, noise_scale);
  HRIEMO_LAUNCH_CHECK("gather_rows_aug_kernel");
  hriemo_prof_end(HP_ROWOPS, st, 2.0 * (double)dst_rows * (double)row_bytes);
  return 0;
}
