// bf16 MFMA GEMM for gfx950 with the three operand layouts the fusion path needs:
//   NT  C[M,N] = A[M,K]  . B[N,K]^T   forward projections / FFN (weights are [out,in])
//   NN  C[M,N] = A[M,K]  . B[K,N]     dX = dY . W
//   TN  C[M,N] = A[K,M]^T. B[K,N]     dW = dY^T . X   (reduction over the B*L rows, split-K)
// One kernel template, parameterised by block tile BMxBN (BK = 64), wave grid WMxWN (each wave owns
// (BM/WM)x(BN/WN) as MFMA 16x16x32 tiles) and NS LDS stages:
//  * operand tiles go HBM -> LDS with 16-byte buffer_load ... lds (LDS-DMA, no VGPR round trip; per-lane
//    offsets are loop-invariant, out-of-matrix lanes are zero-filled by the buffer range check) into an
//    NS-deep ring; the prefetch runs NS-1 K-steps ahead and is retired with a COUNTED s_waitcnt vmcnt(N)
//    + raw s_barrier (never vmcnt(0) in the steady state), one barrier per K-step;
//  * LDS images are lane-linear (LDS-DMA rule) and XOR-swizzled through the per-lane SOURCE address +
//    the same XOR on the fragment read:
//      K-contiguous operand: [rows][64 k] bf16, 128-B rows, 16-B chunk ^= row&7      -> ds_read_b128
//      K-strided operand:    [64 k][cols] bf16, 256/512-B rows, 32-B pair ^= key(k)  -> ds_read_b64_tr_b16
//    both conflict-free for the lane groups of those instructions;
//  * accumulators are produced transposed (mfma(Bfrag, Afrag)) so a lane owns 4 consecutive columns of one
//    row; bias / ReLU / ReLU-mask / residual-add are fused in the epilogue; bf16 tiles leave through LDS as
//    full-line 16-byte stores, fp32 (weight-gradient) tiles as 16-byte stores from registers;
//  * blockIdx is remapped (bijectively) so each XCD's L2 sees a contiguous range of tiles.
#include "gemm_common.h"
#include <string.h>
#include <stdlib.h>

// Persistent kernel: the grid is one (or two) blocks per CU; block b belongs to XCD b & 7 and walks that XCD's
// contiguous range of work units, so neighbouring tiles (same A row-panel) share an L2.  The operand ring is
// one continuous stream over (tile, K-step): the first NS-1 stages of the NEXT tile are issued during the last
// K-steps of the current one, the epilogue does not touch the ring and does not wait for its stores, so a
// tile boundary costs neither a block launch, nor a cold prologue, nor a store drain.
// (the body is a device function: gemm_kernel runs it on its one problem, gemm_group_kernel on problem blockIdx.y of a list)
template <int TA, int TB, int OUTF32, int BM, int BN, int WM, int WN, int NS, int BK>
__device__ __forceinline__ void gemm_body(const GemmArgs& p) {
  constexpr int NWAVE = WM * WN;
  // 32-deep stages: 8-wave blocks run the staggered two-group schedule; 4-wave blocks (two per CU, whose waves pair
  // up on the SIMDs and drift apart on their own) the same K-step body without the second barrier
  constexpr bool K32 = (BK == 32), STAG = K32 && (WM * WN == 8);
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
  constexpr int A_PW = A_BYTES / 1024 / NWAVE, B_PW = B_BYTES / 1024 / NWAVE, LPT = A_PW + B_PW;
  constexpr int MT = BM / WM / 16, NTL = BN / WN / 16;
  static_assert(A_PW * NWAVE * 1024 == A_BYTES && B_PW * NWAVE * 1024 == B_BYTES, "tile must split evenly over waves");
  static_assert(NS >= 2 && NS <= 8 && (NS - 1) * LPT < 64, "ring depth / vmcnt range");
  static_assert(!STAG || NS == 4, "staggered schedule: 4 ring slots");
  static_assert(!K32 || NS >= 3, "32-deep stages need a ring of 3");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: LDS-DMA bases stay scalar
  const int wm = wave / WN, wn = wave % WN;
  char* scratch = smem + NS * STAGE + wave * 2048;

  // this block's work units: wg = beg + lb, beg + lb + nx, ... < end
  // hardware places block b on XCD b % 8: an XCD with nx of the G blocks gets the matching share of the units
  const int G = gridDim.x, nxcd = min(8, G), q = G / nxcd, r = G - q * nxcd;
  const int xcd = blockIdx.x % nxcd, lb = blockIdx.x / nxcd, nx = q + (xcd < r ? 1 : 0);
  const int before = xcd * q + min(xcd, r);            // blocks on lower-numbered XCDs
  const int tiles = p.tiles_m * p.tiles_n;
  const long total = (long)tiles * p.splitk;
  const int end = (int)(total * (before + nx) / G);
  const int beg = (int)(total * before / G);
  // Work queue (p.sched != nullptr): the blocks of an XCD draw that XCD's units from one atomic counter instead of
  // owning every nx-th one, so a block that gets its CU late (another kernel -- an RCCL collective, the other branch's
  // GEMM -- is holding it) simply draws fewer units and the launch is not stretched by the blocks that started last.
  // Ids travel two units ahead: `wg` is being computed, `nwg` is already streaming into the ring, and the id after that
  // is drawn by lane 0 of wave 0 right before the epilogue (behind the counted wait, so no vmcnt arithmetic changes),
  // parked in the first word of wave 0's epilogue scratch and read by all waves after the next tile-start barrier.
  const bool dyn = p.sched != nullptr;
  unsigned* const qctr = p.sched + xcd;
  int* const qslot = (int*)(smem + NS * STAGE);          // wave 0's scratch: free between its epilogues
  auto leave = [&]() {                                    // every block, exactly once, on its way out
    if (dyn && tid == 0) {
      const unsigned done = atomicAdd(p.sched + 8, 1u);
      if (done == gridDim.x - 1) {                        // last one out resets the queue for the next launch
#pragma unroll
        for (int k = 0; k < 9; ++k) __hip_atomic_store(p.sched + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  };
  int wg, nwg;
  if (dyn) {
    if (tid == 0) {
      const int first = (int)atomicAdd(qctr, 2u);
      qslot[0] = beg + first;
      qslot[1] = beg + first + 1;
    }
    __syncthreads();
    wg = __builtin_amdgcn_readfirstlane(qslot[0]);
    nwg = __builtin_amdgcn_readfirstlane(qslot[1]);
    __syncthreads();                                      // both read before anyone's epilogue reuses the scratch
  } else {
    wg = beg + lb;
    nwg = wg + nx;
  }
  if (wg >= end) { leave(); return; }

  const long astep = TA == 0 ? BK : BK * p.lda, bstep = TB == 0 ? BK : BK * p.ldb;
  const LaneOff aoff = operand_lane<TA, BM, BK>(p.lda, lane), boff = operand_lane<TB, BN, BK>(p.ldb, lane);

  auto decode = [&](int w) {
    TileInfo t;
    t.slice = w / tiles;
    const int r = w - t.slice * tiles;
    const int tm = r / p.tiles_n, tn = r - tm * p.tiles_n;
    t.m0 = tm * BM; t.n0 = tn * BN;
    const int kbeg = t.slice * p.k_per_split;
    t.kext = min(p.K, kbeg + p.k_per_split) - kbeg;
    t.nk = (t.kext + BK - 1) / BK;
    t.abase = TA == 0 ? p.A + (long)t.m0 * p.lda + kbeg : p.A + (long)kbeg * p.lda + t.m0;
    t.bbase = TB == 0 ? p.B + (long)t.n0 * p.ldb + kbeg : p.B + (long)kbeg * p.ldb + t.n0;
    t.a_valid = p.M - t.m0; t.b_valid = p.N - t.n0;
    return t;
  };
  // The 128x64 wave tile runs at the 256-VGPR limit: there the per-lane offsets are rebuilt from the lane id at
  // every K-step (a dozen VALU ops) instead of living in registers that the allocator would spill to scratch.
  constexpr bool REBUILD = (MT * NTL > 16);
  auto stage = [&](int s, const TileInfo& t, int kstep) {
    char* sa = smem + s * STAGE;
    const int krem = t.kext - kstep * BK;
    if (REBUILD) {
      int l2 = lane;
      asm volatile("" : "+v"(l2));        // opaque: keeps the rebuild inside the loop
      const LaneOff ao = operand_lane<TA, BM, BK>(p.lda, l2), bo = operand_lane<TB, BN, BK>(p.ldb, l2);
      stage_operand<TA, BM, A_PW, BK>(sa, t.abase + kstep * astep, ao, p.lda, t.a_valid, krem, wave, lane);
      stage_operand<TB, BN, B_PW, BK>(sa + A_BYTES, t.bbase + kstep * bstep, bo, p.ldb, t.b_valid, krem, wave, lane);
    } else {
      stage_operand<TA, BM, A_PW, BK>(sa, t.abase + kstep * astep, aoff, p.lda, t.a_valid, krem, wave, lane);
      stage_operand<TB, BN, B_PW, BK>(sa + A_BYTES, t.bbase + kstep * bstep, boff, p.ldb, t.b_valid, krem, wave, lane);
    }
  };

  f32x4 acc[MT][NTL];
  auto load_frags = [&](const char* sa, int ks, bf16x8 (&af)[MT], bf16x8 (&bfr)[NTL]) {
    const char* sb = sa + A_BYTES;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
      af[mi] = TA == 0 ? lds_row_frag<BK>(sa, wm * MT * 16 + mi * 16, ks, lane) : lds_tr_frag<BM * 2>(sa, wm * MT * 16 + mi * 16, ks, lane);
#pragma unroll
    for (int ni = 0; ni < NTL; ++ni)
      bfr[ni] = TB == 0 ? lds_row_frag<BK>(sb, wn * NTL * 16 + ni * 16, ks, lane) : lds_tr_frag<BN * 2>(sb, wn * NTL * 16 + ni * 16, ks, lane);
  };
  auto mma_rows = [&](const bf16x8 (&af)[MT], const bf16x8 (&bfr)[NTL], int lo, int hi) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
      if (mi >= lo && mi < hi) {
#pragma unroll
        for (int ni = 0; ni < NTL; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
      }
  };
  auto mma = [&](const bf16x8 (&af)[MT], const bf16x8 (&bfr)[NTL]) { mma_rows(af, bfr, 0, MT); };

  // The host guarantees nk >= NS-1 for every work unit, so stream positions it+NS-1 of a tile fall either in
  // the tile itself or in the first NS-1 stages of the next one.
  TileInfo T = decode(wg);
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) stage(s, T, s);
  wait_vmcnt<(NS - 2) * LPT>();
  int cur = 0, nxt = NS - 1;          // ring slots of the stage being computed / being filled

  bool parked = false;                  // wave 0 parked the next-next id in qslot[0] at the end of the last tile
  bool relax_first = false;             // this wave's last epilogue stored a full bf16 sub-tile (see First below)
  for (;;) {
    __builtin_amdgcn_s_barrier();       // stage 0 of this tile (confirmed per wave before its last epilogue) is visible
    if (parked) nwg = __builtin_amdgcn_readfirstlane(qslot[0]);
    const bool has_next = nwg < end;
    const int nk = T.nk;
    // stream position it+NS-1: issue it if it exists; returns whether a stage group went out.  The next
    // unit is decoded on the spot (scalar ALU, NS-1 times per tile) instead of living in SGPRs all loop long.
    auto prefetch = [&](int it) -> bool {
      const int ps = it + NS - 1;
      if (ps < nk) { stage(nxt, T, ps); return true; }
      if (has_next) { const TileInfo NX = decode(nwg); stage(nxt, NX, ps - nk); return true; }
      return false;
    };
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NTL; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // groups of LPT loads younger than stage it+1 when iteration `it` retires it
    auto retire_next = [&](int it) {
      const int young = has_next ? NS - 2 : min(NS - 2, max(0, nk - it - 2));
      if (NS >= 8 && young >= 6) wait_vmcnt<(NS >= 8 ? 6 : 0) * LPT>();
      else if (NS >= 7 && young >= 5) wait_vmcnt<(NS >= 7 ? 5 : 0) * LPT>();
      else if (NS >= 6 && young >= 4) wait_vmcnt<(NS >= 6 ? 4 : 0) * LPT>();
      else if (NS >= 5 && young >= 3) wait_vmcnt<(NS >= 5 ? 3 : 0) * LPT>();
      else if (NS >= 4 && young >= 2) wait_vmcnt<(NS >= 4 ? 2 : 0) * LPT>();
      else if (NS >= 3 && young >= 1) wait_vmcnt<(NS >= 3 ? 1 : 0) * LPT>();
      else wait_vmcnt<0>();
    };
    // A K-step far enough from the tile's end needs no decisions: the stage it+NS-1 belongs to this tile, stage
    // it+1 has NS-2 younger groups behind it, and there is a next K-step.  The loops below run that STEADY body for
    // it < nk-(NS-1) and the general body for the last NS-1 K-steps (stage stream crossing into the next tile).
    const int n_steady = max(0, nk - (NS - 1));
    auto prefetch_s = [&](int it, auto steady) {
      if constexpr (decltype(steady)::value) stage(nxt, T, it + NS - 1);
      else prefetch(it);
    };
    constexpr int NST = OUTF32 ? 0 : MT * 2;            // 16-byte line stores of one wave's bf16 sub-tile
    auto retire_s = [&](int it, auto steady) {
      if constexpr (decltype(steady)::value) {
        // (NS >= 3 only: with two ring slots the stage this wait needs is the one this very K-step issued, YOUNGER than the stores)
        if (NS >= 3 && NST > 0 && relax_first && it == 0) wait_vmcnt<((NS - 2) * LPT + NST) < 63 ? ((NS - 2) * LPT + NST) : 63>();
        else wait_vmcnt<(NS - 2) * LPT>();
      } else retire_next(it);
    };
    typedef std::integral_constant<bool, true> Steady;
    typedef std::integral_constant<bool, false> Tail;
    // First K-step (it == 0, steady body) of a tile that follows an epilogue of THIS wave (round 4).  CDNA counts stores in vmcnt like loads and
    // retires them in order, so the standard wait of that K-step -- "at most the NS-2 youngest stage groups outstanding", i.e. the
    // stage that is needed next has landed -- also waited for the acknowledgement of every store of the epilogue, which sits in
    // the queue between that (older) stage and the group this K-step has just issued: the store drain was 40-60 % of the
    // epilogue's cost (round 3's ablation: 44.1 / 41.9 / 38.7 us full / no stores / no epilogue on 25600x768x768).  The stage it
    // waits for is OLDER than the stores, so the exact count is (NS-2) groups + the NST stores of a full bf16 tile; the stores
    // then have a whole K-step to be acknowledged before the next wait needs them gone.  Only when this wave's sub-tile was
    // stored unpredicated (full tile, no column-sum stores): a skipped store would make the count too permissive.

    if constexpr (K32) {
      // Staggered two-group schedule (256x256 tile, 32-deep stages).  A SIMD hosts wave w (group 0) and wave
      // w + 4 (group 1).  Every K-step is an S-phase (LDS-DMA issue for stream position it+3, the 12 fragment
      // reads of stage it, counted retire of stage it+1) and an M-phase (32 MFMAs), each closed by one barrier;
      // group 1 runs one phase behind, so on every SIMD one wave feeds the matrix pipe while its partner pays
      // the DMA-issue / LDS-read time (measured on the ingredient probe, scripts_dev/mfma_probe.hip: 1.85 of
      // 2.0 PFLOP/s MFMA-only, against 1.49 for the same work with both waves in phase).
      //   stage it is read in barrier slot 2it (g0) / 2it+1 (g1); every wave confirms its share of stage it at
      //   the end of S(it-1), i.e. before either group reads it; ring slot (it+3)%4 == (it-1)%4 is restaged in
      //   S(it), after the barrier that follows the last read of stage it-1 (slot 2it-1).
      bf16x8 af[MT], bfr[NTL];
      const bool g1 = STAG && wave >= NWAVE / 2;
      if (g1) __builtin_amdgcn_s_barrier();
      auto kstep = [&](int it, auto steady) {
        prefetch_s(it, steady);
        load_frags(smem + cur * STAGE, 0, af, bfr);
        retire_s(it, steady);
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): fragments in registers, slot released
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        mma(af, bfr);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        if (STAG) __builtin_amdgcn_s_barrier();
        cur = (cur + 1 == NS) ? 0 : cur + 1;
        nxt = (nxt + 1 == NS) ? 0 : nxt + 1;
      };
      for (int it = 0; it < n_steady; ++it) kstep(it, Steady());
      for (int it = n_steady; it < nk; ++it) kstep(it, Tail());
      if (STAG && !g1) __builtin_amdgcn_s_barrier();
    } else {
    bf16x8 afA[MT], bfA[NTL], afB[MT], bfB[NTL];
      // Software pipeline across the barrier: while the MFMAs of one 32-deep half-step run, the fragments of
      // the next half-step are already being read (two register sets), and the retire-wait + barrier for
      // stage it+1 sits in the MIDDLE of iteration it, so its first fragments load under the second cluster.
      // Order inside an iteration (pinned with sched_barrier(0): hipcc otherwise moves the register-only MFMA
      // clusters across the waits and the barrier, rule 18):
      //   DMA(it+NS-1) | MFMA(A, rows 0..MT/2) | read B-set | MFMA(A, rest) | retire stage it+1 + barrier |
      //   read next A-set | MFMA(B-set)
      // so every fragment read has >= half a cluster of MFMAs to land, and the LDS-read retire before the
      // barrier is a builtin s_waitcnt (lgkmcnt(0) only) the compiler can see, so it adds no wait of its own
      // in front of the B cluster.
      // fragment reads of the NEXT half-step are interleaved with the MFMAs of the current one in four
      // equal groups (sched_group_barrier), so the LDS sees a steady trickle instead of 8 waves bursting
      // 12 reads each right after the barrier.
      constexpr int RD_A = (TA == 0 ? 1 : 2) * MT, RD_B = (TB == 0 ? 1 : 2) * NTL;     // ds_read instrs per set
      auto interleave = [&]() {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          __builtin_amdgcn_sched_group_barrier(0x008, MT * NTL / 4, 0);               // MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, (RD_A + RD_B + 3) / 4, 0);      // DS read
        }
      };
      constexpr bool ILV = (MT * NTL <= 16) || (MT % 2 != 0);
      constexpr bool HALF = !ILV && !OUTF32;
      if constexpr (ILV) {
        // 64x64 wave tiles: two full fragment sets, reads of the next half-step trickle between the MFMAs
        load_frags(smem + cur * STAGE, 0, afA, bfA);
        auto kstep = [&](int it, auto steady) {
          prefetch_s(it, steady);
          __builtin_amdgcn_sched_barrier(0);
          load_frags(smem + cur * STAGE, 1, afB, bfB);
          mma(afA, bfA);
          interleave();
          __builtin_amdgcn_sched_barrier(0);
          cur = (cur + 1 == NS) ? 0 : cur + 1;
          nxt = (nxt + 1 == NS) ? 0 : nxt + 1;
          if (decltype(steady)::value || it + 1 < nk) {
            // stage it+1 must have landed for every wave; our own reads of stage `it` must be retired before
            // any wave may restage that slot (WAR).
            retire_s(it, steady);
            __builtin_amdgcn_s_waitcnt(0xC07F);       // lgkmcnt(0) alone
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);        // reads + MFMAs in ONE scheduling region
            load_frags(smem + cur * STAGE, 0, afA, bfA);
            mma(afB, bfB);
            interleave();
            __builtin_amdgcn_sched_barrier(0);
          } else {
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_sched_barrier(0);
            mma(afB, bfB);
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        for (int it = 0; it < n_steady; ++it) kstep(it, Steady());
        for (int it = n_steady; it < nk; ++it) kstep(it, Tail());
      } else if constexpr (!HALF) {
        // 128x64 wave tile, fp32 output (weight gradients: both operands K-strided, twice the fragment reads, no
        // aux epilogue): two full fragment sets, each 32-deep half-step = two clusters of 16 MFMAs.
        //   DMA | MFMA(A, rows 0..MT/2) | read B-set | MFMA(A, rest) | retire stage it+1 + barrier |
        //   read next A-set | MFMA(B-set)
        load_frags(smem + cur * STAGE, 0, afA, bfA);
        auto kstep = [&](int it, auto steady) {
          prefetch_s(it, steady);
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
          mma_rows(afA, bfA, 0, MT / 2);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
          load_frags(smem + cur * STAGE, 1, afB, bfB);
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
          mma_rows(afA, bfA, MT / 2, MT);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
          cur = (cur + 1 == NS) ? 0 : cur + 1;
          nxt = (nxt + 1 == NS) ? 0 : nxt + 1;
          if (decltype(steady)::value || it + 1 < nk) {
            retire_s(it, steady);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_s_barrier();
            load_frags(smem + cur * STAGE, 0, afA, bfA);
          } else {
            __builtin_amdgcn_s_waitcnt(0xC07F);
          }
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(1);
          mma(afB, bfB);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
        };
        for (int it = 0; it < n_steady; ++it) kstep(it, Steady());
        for (int it = n_steady; it < nk; ++it) kstep(it, Tail());
      } else {
        // 128x64 wave tile (128 accumulator registers): the A fragments are double-buffered in HALVES (rows
        // 0..63 / 64..127 of the wave tile) and B in two sets, 64 fragment registers instead of 96, so the loop
        // stays clear of the 256-register limit.  Each 32-deep half-step is two clusters of 16 MFMAs; the reads
        // for the cluster after next are issued right before a cluster and land underneath it:
        //   L(a1,ks0) A(0) | L(a0,ks1) L(b',ks1) B(0) | L(a1,ks1) A(1) | retire + barrier |
        //   L(a0,next) L(b,next) B(1)
        constexpr int MH = MT / 2;
        bf16x8 a0[MH], a1[MH], b0[NTL], b1[NTL];
        auto load_a = [&](const char* sa, int ks, int half, bf16x8 (&af)[MH]) {
#pragma unroll
          for (int mi = 0; mi < MH; ++mi)
            af[mi] = TA == 0 ? lds_row_frag<BK>(sa, wm * MT * 16 + (half * MH + mi) * 16, ks, lane)
                             : lds_tr_frag<BM * 2>(sa, wm * MT * 16 + (half * MH + mi) * 16, ks, lane);
        };
        auto load_b = [&](const char* sa, int ks, bf16x8 (&bfr)[NTL]) {
          const char* sb = sa + A_BYTES;
#pragma unroll
          for (int ni = 0; ni < NTL; ++ni)
            bfr[ni] = TB == 0 ? lds_row_frag<BK>(sb, wn * NTL * 16 + ni * 16, ks, lane) : lds_tr_frag<BN * 2>(sb, wn * NTL * 16 + ni * 16, ks, lane);
        };
        auto cluster = [&](int half, const bf16x8 (&af)[MH], const bf16x8 (&bfr)[NTL]) {
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int mi = 0; mi < MH; ++mi)
#pragma unroll
            for (int ni = 0; ni < NTL; ++ni)
              acc[half * MH + mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[half * MH + mi][ni], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
        };
        load_a(smem + cur * STAGE, 0, 0, a0);
        load_b(smem + cur * STAGE, 0, b0);
        auto kstep = [&](int it, auto steady) {
          prefetch_s(it, steady);
          const char* sa = smem + cur * STAGE;
          __builtin_amdgcn_sched_barrier(0);
          load_a(sa, 0, 1, a1);
          cluster(0, a0, b0);
          load_a(sa, 1, 0, a0);
          load_b(sa, 1, b1);
          cluster(1, a1, b0);
          load_a(sa, 1, 1, a1);
          cluster(0, a0, b1);
          cur = (cur + 1 == NS) ? 0 : cur + 1;
          nxt = (nxt + 1 == NS) ? 0 : nxt + 1;
          if (decltype(steady)::value || it + 1 < nk) {
            retire_s(it, steady);
            __builtin_amdgcn_s_waitcnt(0xC07F);       // lgkmcnt(0): a1 is in, slot released
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            load_a(smem + cur * STAGE, 0, 0, a0);
            load_b(smem + cur * STAGE, 0, b0);
          }
          cluster(1, a1, b1);
        };
        for (int it = 0; it < n_steady; ++it) kstep(it, Steady());
        for (int it = n_steady; it < nk; ++it) kstep(it, Tail());
      }
    }
    // This wave's share of the next tile's stage 0 must have landed BEFORE its stores join the queue: loads
    // complete in order among themselves, so a counted wait stays exact only while nothing but loads is older.
    if (has_next) wait_vmcnt<(NS - 2) * LPT>();
    int drawn = end;                    // id of the unit after next (lane 0 of wave 0 only)
    if (dyn && has_next && tid == 0) drawn = beg + (int)atomicAdd(qctr, 1u);
#if defined(HRIEMO_GEMM_ABL) && (HRIEMO_GEMM_ABL & 8)
    bool skip_epilogue;                 // timing-only build: no epilogue (stores only on an impossible value)
    {
      float sum = 0.f;
#pragma unroll
      for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NTL; ++b) sum += acc[a][b][0] + acc[a][b][1] + acc[a][b][2] + acc[a][b][3];
      skip_epilogue = sum != 12345.678f;
    }
    if (skip_epilogue) {
    } else
#endif
    if (OUTF32) {
      store_tile<1, 0, MT, NTL>(acc, p, T, scratch, wm, wn, lane);
    } else {
      switch (p.epi) {        // wave-uniform; one specialised copy of the epilogue each
        case 1: store_tile<0, 1, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
        case 2: store_tile<0, 2, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
        case 3: store_tile<0, 3, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
        default: store_tile<0, 0, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
      }
    }
    if (!has_next) break;
    if (!OUTF32) {
      const int rows_valid = p.M - (T.m0 + wm * MT * 16), cols_valid = p.N - (T.n0 + wn * 64);
      relax_first = (p.flags & 1) && rows_valid >= MT * 16 && cols_valid >= 64 && p.cs == nullptr;
    }
    T = decode(nwg);
    wg = nwg;
    if (dyn) {
      if (tid == 0) qslot[0] = drawn;   // wave 0's epilogue is over: its scratch is free until the next one
      __builtin_amdgcn_s_waitcnt(0xC07F);          // landed before the tile-start barrier publishes it
      parked = true;
    } else {
      nwg = wg + nx;
    }
  }
  leave();
}

template <int TA, int TB, int OUTF32, int BM, int BN, int WM, int WN, int NS, int BK>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 ? 2 : 1)) void gemm_kernel(const GemmArgs p) {
  gemm_body<TA, TB, OUTF32, BM, BN, WM, WN, NS, BK>(p);
}

// ---------------------------------------------------------------------------------------------- config 9: loader / consumer waves
// The same 256x128 tile, 64-deep stages and three-slot ring as config 1, with the LDS-DMA issue taken OFF the MFMA waves: a
// workgroup is 8 consumer waves (4x2, 64x64 each: fragment reads, MFMAs, epilogue) + 4 loader waves, one per SIMD, that do nothing
// but stage operands (12 of a stage's 48 one-KiB pieces each) and confirm them with counted vmcnt waits.  Why: an LDS-DMA
// wave-instruction holds its wave for 60-185 cycles (MI355X guide), six per K-step and wave in config 1 -- as long as the 32
// MFMAs (512 cycles) the same wave issues per K-step -- and because both waves of a SIMD sit in the same phase behind the
// K-step's barrier, nobody feeds the matrix pipe meanwhile (round 4 counters: MFMA busy 25 %, waves parked 36 %, issue-stalled
// 35 %).  Three waves per SIMD need <= 168 registers each: one accumulator set (64) + two fragment sets (64).
// Protocol, one workgroup barrier per K-step: position s of the (tile, K-step) stream lives in ring slot s % 3;
//   loaders:   wait until their pieces of position s have landed (position s+1 may be in flight) | barrier(s) | issue s+2
//   consumers: wait for their own fragment reads of position s-1                                  | barrier(s) | read + multiply s
// barrier(s) therefore publishes position s and frees the slot of s-1 = the slot position s+2 goes to.  The stream runs across
// tile boundaries, so the consumers' epilogue overlaps the next tile's first two stages with no extra logic.
template <int TA, int TB, int OUTF32>
__global__ __launch_bounds__(768) void gemm_ws_kernel(const GemmArgs p) {
  constexpr int BM = 256, BN = 128, BK = 64, NS = 3, WN = 2, NCW = 8, NLW = 4, MT = 4, NTL = 4;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
  constexpr int A_PL = A_BYTES / 1024 / NLW, B_PL = B_BYTES / 1024 / NLW, LPL = A_PL + B_PL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = gridDim.x, nxcd = min(8, G), q = G / nxcd, r = G - q * nxcd;
  const int xcd = blockIdx.x % nxcd, lb = blockIdx.x / nxcd, nx = q + (xcd < r ? 1 : 0);
  const int before = xcd * q + min(xcd, r);
  const int tiles = p.tiles_m * p.tiles_n;
  const long total = (long)tiles * p.splitk;
  const int end = (int)(total * (before + nx) / G), beg = (int)(total * before / G);
  // Work queue (p.sched != nullptr), as gemm_body: the blocks of an XCD draw that XCD's units from one atomic counter, so a block
  // that gets its CU late (another kernel holds it) draws fewer units.  Twelve waves have to agree on the ids and there is no LDS
  // left for a mailbox -- but consumer wave 0's epilogue scratch is idle while the tile's K loop runs: during tile t wave 0
  // (lane 0) draws the id of tile t+2 and, in front of the barrier of the tile's last-but-one position, writes the id of tile
  // t+1 (drawn one tile earlier) into the first word of that scratch; every wave reads it right behind that barrier -- exactly
  // when the loaders are about to issue tile t+1's first stage -- and the barrier of the last position then separates all
  // reads from wave 0's next epilogue.  (Every unit has >= 2 K-steps: host.)
  const bool dyn = p.sched != nullptr;
  unsigned* const qctr = p.sched + xcd;
  int* const qslot = (int*)(smem + NS * STAGE);
  // A block's FIRST unit is its static one (beg + lb: the operand stream starts at once, no round trip to the counter in front
  // of it); the counter hands out the units from beg + nx on.
  const int wg0 = beg + lb, wg1 = wg0 + nx;              // (wg1: the static walk's second unit; the queue draws its own)
  auto leave = [&]() {                                    // every block, exactly once (its thread 0), on its way out
    if (dyn && tid == 0) {
      const unsigned done = atomicAdd(p.sched + 8, 1u);
      if (done == gridDim.x - 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) __hip_atomic_store(p.sched + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  };
  if (wg0 >= end) { leave(); return; }
  auto decode = [&](int w) {
    TileInfo t;
    t.slice = w / tiles;
    const int rr = w - t.slice * tiles;
    const int tm = rr / p.tiles_n, tn = rr - tm * p.tiles_n;
    t.m0 = tm * BM; t.n0 = tn * BN;
    const int kbeg = t.slice * p.k_per_split;
    t.kext = min(p.K, kbeg + p.k_per_split) - kbeg;
    t.nk = (t.kext + BK - 1) / BK;
    t.abase = TA == 0 ? p.A + (long)t.m0 * p.lda + kbeg : p.A + (long)kbeg * p.lda + t.m0;
    t.bbase = TB == 0 ? p.B + (long)t.n0 * p.ldb + kbeg : p.B + (long)kbeg * p.ldb + t.n0;
    t.a_valid = p.M - t.m0; t.b_valid = p.N - t.n0;
    return t;
  };
  if (wave >= NCW) {
    // ------------------------------------------------------------------ loader wave
    __builtin_amdgcn_s_setprio(3);             // its few instructions go out as soon as they are ready (priority 0: the same step time)
    const int lw = wave - NCW;
    const long astep = TA == 0 ? BK : BK * p.lda, bstep = TB == 0 ? BK : BK * p.ldb;
    const LaneOff aoff = operand_lane<TA, BM, BK>(p.lda, lane), boff = operand_lane<TB, BN, BK>(p.ldb, lane);
    int ik = 0, islot = 0;
    int known_next = dyn ? end : wg1;          // id of the tile after the one being handed over (queue: read at its position nk-2)
    bool more = true, crossed = false;         // crossed: the issue cursor has left its tile; the next id is decoded lazily
    TileInfo IT = decode(wg0);
    auto issue_next = [&]() -> bool {
      if (crossed) {                           // (only now is the next id certain to have been read)
        crossed = false;
        if (known_next < end) IT = decode(known_next); else more = false;
      }
      if (!more) return false;
      char* sa = smem + islot * STAGE;
      const int krem = IT.kext - ik * BK;
      stage_operand<TA, BM, A_PL, BK>(sa, IT.abase + ik * astep, aoff, p.lda, IT.a_valid, krem, lw, lane);
      stage_operand<TB, BN, B_PL, BK>(sa + A_BYTES, IT.bbase + ik * bstep, boff, p.ldb, IT.b_valid, krem, lw, lane);
      islot = (islot + 1 == NS) ? 0 : islot + 1;
      if (++ik == IT.nk) { ik = 0; crossed = true; }
      return true;
    };
    int pending = 0;                           // positions issued and not yet handed over
    if (issue_next()) ++pending;
    if (issue_next()) ++pending;
    for (int w = wg0; w < end;) {
      const int nk = decode(w).nk;
      for (int it = 0; it < nk; ++it) {
        if (pending >= 2) wait_vmcnt<LPL>(); else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (dyn && it == nk - 2) {             // the id of the next tile has just been published
          const int v = *(LDS_PTR(const int))qslot;
          __builtin_amdgcn_s_waitcnt(0xC07F);
          known_next = __builtin_amdgcn_readfirstlane(v);
        }
        --pending;
        if (issue_next()) ++pending;
      }
      w = known_next;
      if (!dyn) known_next = w + nx;
    }
    return;
  }
  // -------------------------------------------------------------------- consumer wave
  const int wm = wave / WN, wn = wave % WN;
  char* scratch = smem + NS * STAGE + wave * 2048;
  f32x4 acc[MT][NTL];
  auto load_frags = [&](const char* sa, int ks, bf16x8 (&af)[MT], bf16x8 (&bfr)[NTL]) {
    const char* sb = sa + A_BYTES;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
      af[mi] = TA == 0 ? lds_row_frag<BK>(sa, wm * MT * 16 + mi * 16, ks, lane) : lds_tr_frag<BM * 2>(sa, wm * MT * 16 + mi * 16, ks, lane);
#pragma unroll
    for (int ni = 0; ni < NTL; ++ni)
      bfr[ni] = TB == 0 ? lds_row_frag<BK>(sb, wn * NTL * 16 + ni * 16, ks, lane) : lds_tr_frag<BN * 2>(sb, wn * NTL * 16 + ni * 16, ks, lane);
  };
  auto mma = [&](const bf16x8 (&af)[MT], const bf16x8 (&bfr)[NTL]) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NTL; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
  };
  constexpr int RD = (TA == 0 ? 1 : 2) * MT + (TB == 0 ? 1 : 2) * NTL;     // ds_read instructions per fragment set
  int cur = 0;
  const bool drawer = dyn && wave == 0;        // consumer wave 0 (lane 0) draws and publishes the ids
  // `drawn` (lane 0 of wave 0): the counter value behind the id published during the CURRENT tile; it is overwritten by the draw
  // at the end of the tile's loop, i.e. after its use.  The RAW return value is kept and turned into an id only at the publish
  // point: any arithmetic on it right after the atomic makes hipcc wait for the round trip on the spot (wave 0 late at every
  // tile's first barrier, and every wave with it: 5-8 % per launch), and a copy after the epilogue made it drain the epilogue's
  // stores first.  The one wait on the atomic now sits most of a tile after the draw.
  int drawn = end, nextv = dyn ? end : wg1;
  if (drawer && lane == 0) drawn = (int)atomicAdd(qctr, 1u);     // the block's second unit, needed at tile 0's position nk-2
  for (int w = wg0; w < end;) {
    const TileInfo T = decode(w);
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NTL; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Software pipeline across the barrier: the second 32-deep half of a position is multiplied AFTER the next barrier, under the
    // next position's first fragment reads -- every read has a cluster of 16 MFMAs to land under (reading both halves right
    // after the barrier left all eight consumers reading, and nobody multiplying, at the start of every K-step):
    //   barrier(s) | read half 0 of s -> A | MFMA(B: half 1 of s-1) | read half 1 of s -> B | MFMA(A) | wait reads | barrier(s+1)
    // No branch inside the steady body (a fragment set that is conditionally loaded makes hipcc take the bf16x8 vectors apart).
    bf16x8 afA[MT], bfA[NTL], afB[MT], bfB[NTL];
    auto interleave = [&]() {
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        __builtin_amdgcn_sched_group_barrier(0x008, MT * NTL / 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, (RD + 3) / 4, 0);
      }
    };
    {                                          // the tile's first position: nothing pending from before
      if (drawer && T.nk == 2 && lane == 0) qslot[0] = beg + nx + drawn;
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (dyn && T.nk == 2) nextv = *(LDS_PTR(const int))qslot;
      const char* sa = smem + cur * STAGE;
      load_frags(sa, 0, afA, bfA);
      load_frags(sa, 1, afB, bfB);
      mma(afA, bfA);
      __builtin_amdgcn_sched_group_barrier(0x100, RD, 0);
      interleave();
      __builtin_amdgcn_sched_barrier(0);
      cur = (cur + 1 == NS) ? 0 : cur + 1;
    }
    for (int it = 1; it < T.nk; ++it) {
      if (drawer && it == T.nk - 2 && lane == 0) qslot[0] = beg + nx + drawn;
      __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0): this wave's reads of the previous position are in registers
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (dyn && it == T.nk - 2) nextv = *(LDS_PTR(const int))qslot;
      const char* sa = smem + cur * STAGE;
      load_frags(sa, 0, afA, bfA);
      mma(afB, bfB);                           // second half of the previous position
      interleave();
      __builtin_amdgcn_sched_barrier(0);
      load_frags(sa, 1, afB, bfB);
      mma(afA, bfA);
      interleave();
      __builtin_amdgcn_sched_barrier(0);
      cur = (cur + 1 == NS) ? 0 : cur + 1;
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    mma(afB, bfB);                             // second half of the tile's last position
    // the id of the tile after next: drawn here so that the atomic's round trip passes under the epilogue (drawn at the top of
    // the tile, hipcc parked wave 0 -- and with it every barrier -- on the returning value: 44.8 vs 38.7 us on 25600x768x768)
    if (drawer && lane == 0) drawn = (int)atomicAdd(qctr, 1u);
    if (OUTF32) {
      store_tile<1, 0, MT, NTL>(acc, p, T, scratch, wm, wn, lane);
    } else {
      switch (p.epi) {
        case 1: store_tile<0, 1, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
        case 2: store_tile<0, 2, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
        case 3: store_tile<0, 3, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
        default: store_tile<0, 0, MT, NTL>(acc, p, T, scratch, wm, wn, lane); break;
      }
    }
    w = __builtin_amdgcn_readfirstlane(nextv);
    nextv = dyn ? end : w + nx;
  }
  leave();
}

// Grouped launch: up to 16 independent problems of one layout / tile configuration, problem blockIdx.y walked statically by its
// gridDim.x blocks (blocks beyond a problem's tile count leave at once).  The decoder's and the gate's weight-gradient GEMMs --
// 16 latency-bound ~20 us launches for ~0.1 GFLOP each, queued by the host until the encoder's backward has room for them -- go
// out as ONE launch.  The problem table travels in the kernel arguments (capture-safe).
struct GemmGroup { GemmArgs p[16]; };
template <int TA, int TB, int OUTF32, int BM, int BN, int WM, int WN, int NS, int BK>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 ? 2 : 1)) void gemm_group_kernel(const GemmGroup grp) {
  gemm_body<TA, TB, OUTF32, BM, BN, WM, WN, NS, BK>(grp.p[blockIdx.y]);
}

// out[m][n] (+)= sum_s ws[s][m][n], slabs summed in slice order (bit-identical from run to run).  Four slabs' loads are in
// flight per lane before the first add (the k-loop is latency-bound otherwise: 0.5 TB/s measured on the 66 MB of a
// 3072x768x7 reduction in round 1's form, profiles/r02_bench_kernel_stats.csv).
// (Tried in round 2: no separate launch at all -- the wave that stores the last slab of its 64-column sub-tile reduces it,
// arrival counters in device memory.  The slabs come from other XCDs, so the hand-over needs agent-scope release/acquire
// fences, i.e. an L2 write-back and invalidate per wave: 156 us instead of 56 for the 768x768x25600 weight gradient.  Dropped.)
// Rows >= split_m go to a second matrix (C2, row split_m first): the weight gradient of a projection whose weight rows live in
// two parameters (SharedProjFn: rows [0, d) of one in_proj_weight, rows [d, 3d) of another one) comes out of ONE GEMM.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ C, long ldc, int M, int N,
                                                            int splitk, int accumulate, float* __restrict__ C2, long ldc2, int split_m) {
  const long nv = (long)M * N / 4, slab = (long)M * N;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (long)gridDim.x * blockDim.x) {
    const long e = v * 4;
    const int m = (int)(e / N), n = (int)(e - (long)m * N);
    const float* src = ws + e;
    float* dst = m < split_m ? C + (long)m * ldc + n : C2 + (long)(m - split_m) * ldc2 + n;
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    if (accumulate) c = *(const f32x4*)dst;
    f32x4 s = *(const f32x4*)src;
    int k = 1;
    for (; k + 4 <= splitk; k += 4) {
      const f32x4 a0 = *(const f32x4*)(src + (k + 0) * slab), a1 = *(const f32x4*)(src + (k + 1) * slab);
      const f32x4 a2 = *(const f32x4*)(src + (k + 2) * slab), a3 = *(const f32x4*)(src + (k + 3) * slab);
      s += a0; s += a1; s += a2; s += a3;
    }
    for (; k < splitk; ++k) s += *(const f32x4*)(src + k * slab);
    if (accumulate) s += c;
    *(f32x4*)dst = s;
  }
}

// ---------------------------------------------------------------------------------------------- host
struct TileCfg { int bm, bn, threads, lds, ns, bk; };   // lds = bytes of the operand ring (ns stages of bk k)
static const TileCfg kCfg[] = {
    {128, 128, 256, 2 * 32768, 2, 64},   // 0: 128x128, 2x2 waves (64x64 per wave), 2 stages, two blocks per CU
    {256, 128, 512, 3 * 49152, 3, 64},   // 1: 256x128, 4x2 waves (64x64 per wave), 3 stages
    {256, 256, 512, 2 * 65536, 2, 64},   // 2: 256x256, 2x4 waves (128x64 per wave), 2 stages
    {64, 128, 256, 4 * 24576, 4, 64},    // 3: 64x128, 2x2 waves (32x64 per wave), 4 stages: small-M, latency-bound problems
    {256, 256, 512, 4 * 32768, 4, 32},   // 4: 256x256, 2x4 waves, 4 stages of 32 k, staggered two-group schedule
    {320, 128, 512, 2 * 57344, 2, 64},   // 5: 320x128, 4x2 waves (80x64 per wave), 2 stages: tile count for M = 25600, N = 768
    {64, 128, 256, 6 * 24576, 6, 64},    // 6: config 3 with a 6-deep ring: the M = 384 decoder chain is bound by memory latency / prefetch depth
    {32, 128, 256, 7 * 20480, 7, 64},    // 7: 32x128, 2x2 waves (16x64 per wave), 7-deep ring: twice the blocks, deeper prefetch
    {32, 64, 128, 6 * 12288, 6, 64},     // 8: 32x64, 2x1 waves (16x64 per wave): least operand bytes per CU
    {256, 128, 768, 3 * 49152, 3, 64},   // 9: config 1's tile with 8 consumer + 4 loader waves (gemm_ws_kernel)
};
static const int kNumCfg = sizeof(kCfg) / sizeof(kCfg[0]);
int hriemo_num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  }
  return n;
}
static int g_gemm_flags = 9;        // bit 0: count the epilogue's stores in the next tile's first wait (configs 0-8); bit 1: no config 9;
                                    // bit 3 (default on; dp.py clears it while collectives run beside backward): config 9 walks its tiles statically
extern "C" int hriemo_gemm_debug_flags(int flags) {   // tuning hook (A/B in one process): returns the previous value
  const int prev = g_gemm_flags;
  g_gemm_flags = flags;
  return prev;
}
int hriemo_gemm_debug_flags_get() { return g_gemm_flags; }
static int g_force_cfg = -1;
extern "C" int hriemo_gemm_force_config(int cfg) {   // tuning hook (scripts_dev/bench_gemm.py); -1 = heuristic
  g_force_cfg = (cfg >= 0 && cfg < kNumCfg) ? cfg : -1;
  return 0;
}

// Work-queue words for the persistent kernels: one 16-word slot per (device, stream) -- launches on one stream are
// serialised and every launch leaves its slot zeroed (last block out), launches on different streams never share one.
// Allocated once, outside any stream capture; until then the kernels walk statically.
unsigned* hriemo_gemm_sched_slot(hipStream_t st) {
  constexpr int MAXDEV = 16, MAXSLOT = 64;
  static unsigned* base[MAXDEV] = {nullptr};
  static hipStream_t owner[MAXDEV][MAXSLOT];
  static int nslot[MAXDEV] = {0};
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (base[dev] == nullptr) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    unsigned* b = nullptr;
    if (hipMalloc(&b, MAXSLOT * 16 * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(b, 0, MAXSLOT * 16 * sizeof(unsigned)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return nullptr;
    base[dev] = b;
  }
  for (int i = 0; i < nslot[dev]; ++i)
    if (owner[dev][i] == st) return base[dev] + i * 16;
  if (nslot[dev] == MAXSLOT) return nullptr;
  owner[dev][nslot[dev]] = st;
  return base[dev] + (nslot[dev]++) * 16;
}

template <int TA, int TB, int OUTF32, int BM, int BN, int WM, int WN, int NS, int BK = 64>
static void launch_one(const GemmArgs& a, int ring, hipStream_t st) {
  const int lds = ring + WM * WN * 2048;          // operand ring + 2 KB epilogue scratch per wave
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute((const void*)gemm_kernel<TA, TB, OUTF32, BM, BN, WM, WN, NS, BK>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_set = true;
  }
  const long units = (long)a.tiles_m * a.tiles_n * a.splitk;
  const long slots = (long)hriemo_num_cus() * (lds <= 80 * 1024 ? 2 : 1);      // persistent: one block per resident slot
  const int grid = (int)(units < slots ? units : slots);
  GemmArgs q = a;
  q.sched = units > slots ? hriemo_gemm_sched_slot(st) : nullptr;       // a queue only pays when blocks own several units
  hipLaunchKernelGGL((gemm_kernel<TA, TB, OUTF32, BM, BN, WM, WN, NS, BK>), dim3(grid), dim3(WM * WN * 64), lds, st, q);
}

template <int TA, int TB, int OUTF32>
static void launch_gemm(const GemmArgs& a, int cfg, hipStream_t st) {
  const int lds = kCfg[cfg].lds;
  switch (cfg) {
    case 0: launch_one<TA, TB, OUTF32, 128, 128, 2, 2, 2>(a, lds, st); break;
    case 1: launch_one<TA, TB, OUTF32, 256, 128, 4, 2, 3>(a, lds, st); break;
    case 2: launch_one<TA, TB, OUTF32, 256, 256, 2, 4, 2>(a, lds, st); break;
    case 4: launch_one<TA, TB, OUTF32, 256, 256, 2, 4, 4, 32>(a, lds, st); break;
    case 5:
      if constexpr (TA == 0 && OUTF32 == 0) launch_one<TA, TB, OUTF32, 320, 128, 4, 2, 2>(a, lds, st);   // row-major A only
      break;
    case 6:
      if constexpr (TA == 0) launch_one<TA, TB, OUTF32, 64, 128, 2, 2, 6>(a, lds, st);
      break;
    case 7:
      if constexpr (TA == 0) launch_one<TA, TB, OUTF32, 32, 128, 2, 2, 7>(a, lds, st);
      break;
    case 8:
      if constexpr (TA == 0 && TB == 0) launch_one<TA, TB, OUTF32, 32, 64, 2, 1, 6>(a, lds, st);   // 128-B k-rows cannot hold the K-strided swizzle
      break;
    case 9: {
      const int wlds = lds + 8 * 2048;
      static bool ws_attr = false;
      if (!ws_attr) {
        hipFuncSetAttribute((const void*)gemm_ws_kernel<TA, TB, OUTF32>, hipFuncAttributeMaxDynamicSharedMemorySize, wlds);
        ws_attr = true;
      }
      const long units = (long)a.tiles_m * a.tiles_n * a.splitk;
      const long slots = hriemo_num_cus();
      GemmArgs qa = a;
      qa.sched = (units > slots && !(a.flags & 8)) ? hriemo_gemm_sched_slot(st) : nullptr;     // (bit 3 of the debug flags: static walk)
      hipLaunchKernelGGL((gemm_ws_kernel<TA, TB, OUTF32>), dim3((int)(units < slots ? units : slots)), dim3(768), wlds, st, qa);
      break;
    }
    default: launch_one<TA, TB, OUTF32, 64, 128, 2, 2, 4>(a, lds, st); break;
  }
}

// Tile choice from the measured sweep on MI355X (scripts_dev/bench_gemm.py, profiles/r01_gemm_tile_sweep.log):
// the 256x256 tile halves LDS-DMA issues and fragment reads per MFMA and wins when the output is wide enough
// to give every CU several of them; narrower outputs take 256x128 (forward) or 128x128 at two blocks per CU.
static int pick_config(int ta, int tb, int M, int N, int K) {
  if (g_force_cfg >= 0) return g_force_cfg;
  // Round 4: the loader / consumer kernel (config 9) replaces the 256x128 kernel for the encoder-sized projections and the
  // 256x256 / 128x128 kernels for the long weight-gradient reductions (profiles/r04_gemm_ws.log: 7-22 % per launch, the step
  // 7.87 -> 7.39 ms in one process).  Wide outputs of the audio branch stay on the 256x256 kernel (equal alone; 7.39 vs 7.54 ms
  // per step with a tile-cost model that moved more shapes to the queue kernels).  Bit 1 of hriemo_gemm_debug_flags: never config 9.
  if ((g_gemm_flags & 2) == 0) {
    if (ta == 1 && (long)K >= 4096 && M >= 768 && N >= 768) return 9;
    if (ta == 0 && M >= 1024 && N >= 256 && !(N >= 2048 && M >= 16384)) return 9;
  }
  if (ta == 1) return ((long)M * N >= 768L * 2304 && (long)K >= 4096) ? 2 : 0;   // dW: split-K fills the chip
  if (M < 1024 || N < 256) {                                                    // decoder / gate sized problems
    // one block per CU pulls ~68 GB/s of operands whatever the ring depth (scripts_dev/bench_small_gemm.py: 0.375 us per 24 KB
    // K-step on the 64x128 tile, the same with a 6-deep ring), so these launches are as fast as their largest block's operand
    // bytes are small: 32-row tiles, 64 columns where that still fits one round of CUs and the B operand is K-contiguous
    if (!(M <= 512 && N >= 256)) return 0;
    if (K <= 384) return 3;
    return (tb == 0 && N <= 1024) ? 8 : 7;
  }
  // (config 5, 320x128: 480 instead of 600 tiles for the 25600 x 768 outputs, is 3-8 % faster on those launches alone
  // but 0.1 ms slower inside the two-stream step -- kept as a tuning configuration for hriemo_gemm_force_config, never picked)
  if (tb == 0) return (N >= 2048 && M >= 16384) ? 2 : 1;                       // NT
  return (N >= 2048 && M >= 16384) ? 2 : 1;                                    // NN
}

// rows of the column-sum partials of hriemo_gemm_bf16_colsum: one per wave row-block of the tile configuration the launch takes
static int wave_rows(int cfg) {
  static const int waves_m[] = {2, 4, 2, 2, 2, 4, 2, 2, 2, 4};
  return kCfg[cfg].bm / waves_m[cfg];
}
// The launch plan of one GEMM call: the tile configuration after EVERY fallback, the number of split-K slices and the k of a
// slice.  gemm_impl launches exactly this; hriemo_gemm_plan reports it (the tests pin which kernel a shape runs on).
struct GemmPlan { int cfg, splitk, k_per_split; };
static GemmPlan plan_gemm(int ta, int tb, int M, int N, int K, int c_is_f32, long workspace_bytes) {
  int cfg = pick_config(ta, tb, M, N, K);
  if (cfg == 8 && tb == 1) cfg = 7;
  if ((cfg == 3 || (cfg >= 6 && cfg <= 8)) && ta == 1) cfg = 0;   // the 64- / 32-row tiles have no K-strided A image (128-B rows cannot hold the swizzle)
  if (cfg == 5 && (ta == 1 || c_is_f32)) cfg = 0;   // the 320-row tile exists for row-major A and bf16 output only
  int splitk = 1;
  if (c_is_f32) {
    const long tiles = (long)((M + kCfg[cfg].bm - 1) / kCfg[cfg].bm) * ((N + kCfg[cfg].bn - 1) / kCfg[cfg].bn);
    const int ksteps = (K + 63) / 64;
    const long slots = (long)hriemo_num_cus() * (kCfg[cfg].lds + kCfg[cfg].threads * 32 <= 80 * 1024 ? 2 : 1);
    long want = slots / tiles;                         // persistent grid: one work unit per resident block
    if (want > ksteps / 4) want = ksteps / 4;          // >= 4 K-steps (256 of K) per slice
    const long fit = workspace_bytes > 0 ? workspace_bytes / ((long)M * N * 4) : 0;
    if (want > fit) want = fit;
    if (want > 1) splitk = (int)want;
  }
  const int kper = ((K + splitk - 1) / splitk + 63) / 64 * 64;
  splitk = (K + kper - 1) / kper;
  // an NS-deep ring streams NS-1 K-steps ahead across work units: every unit needs >= NS-1 K-steps
  if (K - (splitk - 1) * kper <= (kCfg[cfg].ns - 2) * kCfg[cfg].bk) cfg = 0;
  return {cfg, splitk, kper};
}
// read-only: what hriemo_gemm_bf16 would launch for this call (workspace_bytes <= 0: no workspace)
extern "C" int hriemo_gemm_plan(int ta, int tb, int M, int N, int K, int c_is_f32, long workspace_bytes, int* cfg, int* splitk,
                                int* k_per_split) {
  HRIEMO_CHECK(M > 0 && N > 0 && K > 0 && cfg != nullptr && splitk != nullptr && k_per_split != nullptr, "gemm_plan: bad arguments");
  HRIEMO_CHECK(!(ta == 1 && tb == 0), "gemm: layout (ta=1,tb=0) is not used by this path and not built");
  const GemmPlan pl = plan_gemm(ta, tb, M, N, K, c_is_f32, workspace_bytes);
  *cfg = pl.cfg; *splitk = pl.splitk; *k_per_split = pl.k_per_split;
  return 0;
}
extern "C" int hriemo_gemm_colsum_rows(int ta, int tb, int M, int N, int K) {
  const int wr = wave_rows(plan_gemm(ta, tb, M, N, K, 0, 0).cfg);
  return (M + wr - 1) / wr;
}

static int gemm_impl(int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                     void* C, long ldc, int c_is_f32, const float* bias, int epilogue, const void* aux,
                     long ldaux, int accumulate, float* workspace, long workspace_bytes, float* colsum_partials, hipStream_t st,
                     void* C2 = nullptr, long ldc2 = 0, int split_m = 0) {
  HRIEMO_CHECK(M > 0 && N > 0 && K > 0, "gemm: empty problem M=%d N=%d K=%d", M, N, K);
  HRIEMO_CHECK(C2 == nullptr || (c_is_f32 && split_m > 0 && split_m < M && ldc2 % 4 == 0 && ((uintptr_t)C2 % 16) == 0),
               "gemm: a split output needs fp32 results, 0 < split_m < M and a 16-byte aligned second matrix");
  HRIEMO_CHECK(!(ta == 1 && tb == 0), "gemm: layout (ta=1,tb=0) is not used by this path and not built");
  HRIEMO_CHECK(N % 8 == 0, "gemm: N=%d must be a multiple of 8", N);
  HRIEMO_CHECK(lda % 8 == 0 && ldb % 8 == 0 && ldc % (c_is_f32 ? 4 : 8) == 0, "gemm: leading dims must keep 16-byte alignment");
  HRIEMO_CHECK(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0 && ((uintptr_t)C % 16) == 0, "gemm: unaligned operand");
  HRIEMO_CHECK(lda < (1L << 21) && ldb < (1L << 21), "gemm: leading dimension too large for 32-bit tile offsets");
  if (ta == 0) HRIEMO_CHECK(K % 8 == 0, "gemm: K=%d must be a multiple of 8 for a K-contiguous operand", K);
  if (ta == 1) HRIEMO_CHECK(M % 8 == 0, "gemm: M=%d must be a multiple of 8 for a transposed A", M);
  HRIEMO_CHECK(c_is_f32 || (epilogue >= 0 && epilogue <= 3), "gemm: bad epilogue");
  HRIEMO_CHECK(epilogue < 2 || (aux != nullptr && ldaux % 8 == 0 && ((uintptr_t)aux % 16) == 0), "gemm: epilogue 2/3 needs a 16-byte aligned aux");
  HRIEMO_CHECK(!(c_is_f32 && epilogue != 0), "gemm: fp32 output has no activation epilogue");
  HRIEMO_CHECK(c_is_f32 || !accumulate, "gemm: accumulate needs fp32 output");

  const GemmPlan pl = plan_gemm(ta, tb, M, N, K, c_is_f32, workspace != nullptr ? workspace_bytes : 0);
  const int cfg = pl.cfg, splitk = pl.splitk;
  GemmArgs a = {};
  a.M = M; a.N = N; a.K = K;
  a.A = (const bf16_t*)A; a.lda = lda; a.B = (const bf16_t*)B; a.ldb = ldb;
  a.C = C; a.ldc = ldc; a.bias = bias; a.aux = (const bf16_t*)aux; a.ldaux = ldaux; a.epi = epilogue;
  a.tiles_m = (M + kCfg[cfg].bm - 1) / kCfg[cfg].bm; a.tiles_n = (N + kCfg[cfg].bn - 1) / kCfg[cfg].bn;
  a.ws = workspace; a.accumulate = accumulate; a.sched = nullptr;
  a.flags = g_gemm_flags;
  a.cs = colsum_partials;
  HRIEMO_CHECK(colsum_partials == nullptr || (epilogue == 2 && !c_is_f32), "gemm: column sums are built for the masked epilogue (2) with bf16 output");
  a.splitk = splitk; a.k_per_split = pl.k_per_split;
  if (C2 != nullptr && splitk == 1) {
    // the split is applied by the split-K reduce; a problem that is not split along K runs as two launches instead
    const char* A2 = (const char*)A + (size_t)split_m * 2;      // ta == 1: A is [K][M], its column m is output row m
    HRIEMO_CHECK(ta == 1, "gemm: a split output without split-K is built for the weight-gradient layout only");
    int rc = gemm_impl(ta, tb, split_m, N, K, A, lda, B, ldb, C, ldc, 1, nullptr, 0, nullptr, 0, accumulate, workspace, workspace_bytes, nullptr, st);
    if (rc != 0) return rc;
    return gemm_impl(ta, tb, M - split_m, N, K, A2, lda, B, ldb, C2, ldc2, 1, nullptr, 0, nullptr, 0, accumulate, workspace, workspace_bytes, nullptr, st);
  }

  const int cls = ta ? HP_GEMM_TN : (tb ? HP_GEMM_NN : HP_GEMM_NT);
  hriemo_prof_begin(cls, st);
  if (ta == 0 && tb == 0) {
    if (c_is_f32) launch_gemm<0, 0, 1>(a, cfg, st); else launch_gemm<0, 0, 0>(a, cfg, st);
  } else if (ta == 0 && tb == 1) {
    if (c_is_f32) launch_gemm<0, 1, 1>(a, cfg, st); else launch_gemm<0, 1, 0>(a, cfg, st);
  } else {
    if (c_is_f32) launch_gemm<1, 1, 1>(a, cfg, st); else launch_gemm<1, 1, 0>(a, cfg, st);
  }
  HRIEMO_LAUNCH_CHECK("gemm_kernel");
  if (splitk > 1) {
    const long nv = (long)M * N / 4;
    int grid = (int)((nv + 255) / 256);
    if (grid > 16 * hriemo_num_cus()) grid = 16 * hriemo_num_cus();
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid), dim3(256), 0, st, workspace, (float*)C, ldc, M, N, splitk,
                       accumulate, (float*)C2, ldc2, C2 != nullptr ? split_m : M);
    HRIEMO_LAUNCH_CHECK("splitk_reduce_kernel");
  }
  hriemo_prof_end(cls, st, 2.0 * M * N * K);
  return 0;
}

extern "C" int hriemo_gemm_bf16(int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                                void* C, long ldc, int c_is_f32, const float* bias, int epilogue, const void* aux,
                                long ldaux, int accumulate, float* workspace, long workspace_bytes, hipStream_t st) {
  return gemm_impl(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, c_is_f32, bias, epilogue, aux, ldaux, accumulate, workspace, workspace_bytes,
                   nullptr, st);
}
// fp32 output whose rows [0, split_m) go to C and rows [split_m, M) to C2 (row split_m = row 0 of C2); ta / tb as hriemo_gemm_bf16
extern "C" int hriemo_gemm_bf16_split(int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                                      void* C, long ldc, void* C2, long ldc2, int split_m, int accumulate, float* workspace,
                                      long workspace_bytes, hipStream_t st) {
  HRIEMO_CHECK(C2 != nullptr, "gemm_split: second output missing");
  return gemm_impl(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, 1, nullptr, 0, nullptr, 0, accumulate, workspace, workspace_bytes, nullptr, st,
                   C2, ldc2, split_m);
}
// Weight-gradient GEMMs C_j[N_j, K_j] (+)= dY_j[M_j, N_j]^T . X_j[M_j, K_j] (fp32 results) of njobs independent problems in one launch
// per 16 problems.  jobs_host: njobs x 9 int64 {M (output rows), N (output columns), K (reduction rows), A, lda, B, ldb, C, ldc}
// in hriemo_gemm_bf16's (ta = 1, tb = 1) convention.  No split-K: meant for short reductions (K <= a few thousand rows).
extern "C" int hriemo_gemm_bf16_group_tn(const void* jobs_host, int njobs, int accumulate, hipStream_t st) {
  HRIEMO_CHECK(jobs_host != nullptr && njobs > 0, "gemm_group: empty job table");
  const long long* h = (const long long*)jobs_host;
  constexpr int BM = 128, BN = 128;
  using KernelT = void (*)(const GemmGroup);
  KernelT kern = gemm_group_kernel<1, 1, 1, BM, BN, 2, 2, 2, 64>;
  const int lds = kCfg[0].lds + 4 * 2048;
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_set = true;
  }
  for (int j0 = 0; j0 < njobs; j0 += 16) {

    GemmGroup g = {};
    const int nj = njobs - j0 < 16 ? njobs - j0 : 16;
    int gx = 1;
    double flops = 0.0;
    for (int j = 0; j < nj; ++j) {
      const long long* r = h + (long)(j0 + j) * 9;
      GemmArgs& a = g.p[j];
      a.M = (int)r[0]; a.N = (int)r[1]; a.K = (int)r[2];
      a.A = (const bf16_t*)r[3]; a.lda = (long)r[4]; a.B = (const bf16_t*)r[5]; a.ldb = (long)r[6]; a.C = (void*)r[7]; a.ldc = (long)r[8];
      HRIEMO_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.M % 8 == 0 && a.N % 8 == 0, "gemm_group: job %d: bad shape %dx%dx%d", j0 + j, a.M, a.N, a.K);
      HRIEMO_CHECK(a.lda % 8 == 0 && a.ldb % 8 == 0 && a.ldc % 4 == 0 && ((uintptr_t)a.A % 16) == 0 && ((uintptr_t)a.B % 16) == 0 &&
                       ((uintptr_t)a.C % 16) == 0 && a.lda < (1L << 21) && a.ldb < (1L << 21), "gemm_group: job %d: alignment", j0 + j);
      HRIEMO_CHECK(a.K > (kCfg[0].ns - 2) * kCfg[0].bk, "gemm_group: job %d: reduction too short for the operand ring", j0 + j);
      a.tiles_m = (a.M + BM - 1) / BM; a.tiles_n = (a.N + BN - 1) / BN;
      a.splitk = 1; a.k_per_split = (a.K + 63) / 64 * 64;
      a.accumulate = accumulate; a.sched = nullptr;
      const int tiles = a.tiles_m * a.tiles_n;
      if (tiles > gx) gx = tiles;
      flops += 2.0 * a.M * a.N * a.K;
    }
    for (int j = nj; j < 16; ++j) { g.p[j] = g.p[0]; g.p[j].tiles_m = 0; g.p[j].tiles_n = 0; }      // never launched (grid.y = nj)
    const int cap = 2 * hriemo_num_cus();                 // a problem's tiles beyond its blocks are walked statically
    if (gx > cap) gx = cap;
    hriemo_prof_begin(HP_GEMM_TN, st);
    hipLaunchKernelGGL(kern, dim3(gx, nj), dim3(256), lds, st, g);
    HRIEMO_LAUNCH_CHECK("gemm_group_kernel");
    hriemo_prof_end(HP_GEMM_TN, st, flops);
  }
  return 0;
}
extern "C" int hriemo_gemm_bf16_colsum(int ta, int tb, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                                       void* C, long ldc, const void* aux, long ldaux, float* colsum_partials, hipStream_t st) {
  HRIEMO_CHECK(colsum_partials != nullptr, "gemm_colsum: partials buffer missing");
  return gemm_impl(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, 0, nullptr, 2, aux, ldaux, 0, nullptr, 0, colsum_partials, st);
}
