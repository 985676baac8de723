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
