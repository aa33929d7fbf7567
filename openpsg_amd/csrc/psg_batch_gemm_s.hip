// Batched decode-step projections of the fp32s mode over UNQUANTISED weights: part[s][m][n] = split-K slices of
// x[M][K] . W[N][K]^T for 33 <= M <= 160 fp32 rows given as the fp16 planes [2][M][K] + inv_scale[M] of psg_split_f16x2,
// where W is held as 16-bit planes - the kernel shape of psg_batch_gemm_q.hip's PAIR form over 2-byte weight rows:
//   psg_batch_split_gemm_w16  W an fp16 value (frozen fp16 checkpoint), w16[N][K] + col_scale[N]:
//       part = (xh . w + xl . w) inv_scale[m] col_scale[n]                  - psg_split_gemm_w16's arithmetic above 32 rows
//   psg_batch_split_gemm_w32  W 2^s = wh + wl, both planes read IN PLACE from one fp16 image (row stride, lo_off = the
//       element offset of wl inside a row: the prompt pass's [wh | wl | wh] image with stride 3 K and lo_off K, or a packed
//       [wh | wl] image) + col_scale[N] = 2^-s:
//       part = (xh . wh + xh . wl + xl . wh) inv_scale[m] col_scale[n]      - psg_split.hip's three products, 4 bytes per weight
// Every product of two fp16 values is exact in fp32; all products of an output element go into ONE fp32 accumulator.
//
// Layout:
//   * K step 64: an x row and a weight-plane row of a step are both 128 bytes = 8 pieces of 16 bytes, XOR-swizzled on the
//     SOURCE address with (row >> 1) & 7 (psg_batch_gemm.hip's x image); one LDS-DMA instruction fetches 8 rows;
//   * the x image of a step is 2 planes x MT x 32 rows (MT = 2 / 3 / 5 for M <= 64 / 96 / 160): 16 / 24 / 40 KB;
//   * the weight image of a step is 256 rows x 128 B = 32 KB in both forms: w16 a slab of 256 weight rows, w32 a slab of
//     128 weight rows x its two planes [wh rows | wl rows].  A unit streams 32 KB of weights either way;
//   * a step is ONE stage [x | w] of the ring: 48 / 56 / 72 KB -> 3 / 2 / 2 stages, counted vmcnt;
//   * w16: 8 waves x one 32-row weight tile, every wave walks all MT x tiles (16 MT <= 80 accumulator registers).
//     w32: 4 weight tiles x 2 groups of x tiles (tiles g, g + 2, ...: <= 3 per wave, 48 accumulator registers), so that both
//     planes' fragments of a wave's weight tile stay in registers through the step and xh is read once for its two products.
//     A group with one tile less repeats its last product on a copy and does not store it: the step ends at the barrier
//     with the full group anyway;
//   * per x tile and step the order is xh.wh, xh.wl, xl.wh (w16: xh.w, xl.w), each 4 matrix instructions over K = 16;
//   * ranges, slots, plan and launch: psg_streamk.h.
// Row independence: the plan is a function of (N, K, form, mode) ONLY and is made for 160 rows; M picks MT, which decides
// what is staged and which tiles a wave multiplies, never a slot's k range nor the order of a row's sum.
#include "psg_common.h"
#include "psg_streamk.h"
#include "psg_wave.h"

#define BS_BK 64
#define BS_WAVES 8
#define BS_WROWS 256                                          // rows of a step's weight image (w32: 128 weight rows x 2 planes)
#define BS_LDS_MAX (160 * 1024)

__host__ __device__ constexpr int bs_stage_bytes(int mt) { return (2 * mt * 32 + BS_WROWS) * 128; }
__host__ __device__ constexpr int bs_nst(int mt) { return BS_LDS_MAX / bs_stage_bytes(mt) > 4 ? 4 : BS_LDS_MAX / bs_stage_bytes(mt); }

// NP: weight planes (1: w16, 2: w32).  S_al > 0: aligned ranges, 0: stream-K (psg_streamk.h)
template <int NP, int MT>
__global__ void __launch_bounds__(BS_WAVES * 64, 1)
bs_gemm_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w, float* __restrict__ part, int M, int N, int K,
               int64_t wstride, int64_t lo_off, int S, int S_al, const float* __restrict__ row_scale,
               const float* __restrict__ col_scale) {
  using v8 = EF16::v8;
  constexpr int NST = bs_nst(MT);
  constexpr int XG = NP, WT = BS_WAVES / XG, BN = WT * 32;     // x-tile groups, weight tiles and weight rows of a slab
  constexpr int MTG = (MT + XG - 1) / XG;                      // x tiles of a wave
  constexpr int XR = 2 * MT * 32, XB = XR * 128;               // the x image: plane 0's MT tiles, then plane 1's
  constexpr int STAGE = bs_stage_bytes(MT);
  constexpr int XI = XB / 1024, NI = STAGE / 1024;             // 16-byte DMA instructions (1 KB = 8 rows each): x / x and w
  constexpr int PER = NI / BS_WAVES;
  static_assert(XI % BS_WAVES == 0 && NI % BS_WAVES == 0, "every wave issues the same DMAs of x and of w");
  static_assert(NST >= 2 && NST * STAGE <= BS_LDS_MAX, "LDS of a CU");
  static_assert((NST - 1) * PER <= 63, "vmcnt field");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t smem_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int nk = K / BS_BK, NB = (N + BN - 1) / BN;
  const int64_t T = (int64_t)NB * nk;
  const int G = gridDim.x;
  const psg_sk_span span = psg_sk_range(nk, T, G, S_al);
  const int64_t g0 = span.g0, g1 = span.g1;
  if (g0 >= g1) return;

  // instruction idx of a step: 1 KB idx of the step's [x | w] image = 8 rows x 8 pieces; a wave issues idx = wid + 8 q,
  // q < PER: XI is a multiple of 8, so q alone says which operand an instruction fetches
  auto stage = [&](int slab, int ks, int buf) {              // this wave's DMAs of one step: PER instructions
    unsigned char* sb = smem + buf * STAGE;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int idx = wid + BS_WAVES * q;
      const int r = idx * 8 + (lane >> 3);                   // row of the stage (XR is a multiple of 16: the row's own swizzle)
      const int piece = (lane & 7) ^ ((r >> 1) & 7);
      if (q < XI / BS_WAVES) {
        const int plane = r / (MT * 32), xr = r - plane * (MT * 32);
        const int64_t gr = (int64_t)plane * M + (xr < M ? xr : M - 1);   // (rows past M: a copy of the last row, never stored)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(x + gr * K + ks * BS_BK + piece * 8),
            (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 0);
      } else {
        const int wr_ = r - XR, plane = wr_ / BN;
        int gr = slab * BN + (wr_ - plane * BN);
        gr = gr < N ? gr : N - 1;                            // (rows past N: a copy of the last row, never stored)
        __builtin_amdgcn_global_load_lds(                    // a weight byte is read once by one CU: non-temporal
            (const __attribute__((address_space(1))) void*)(w + (int64_t)gr * wstride + plane * lo_off + ks * BS_BK + piece * 8),
            (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 2);
      }
    }
  };

  const int l31 = lane & 31, hi = lane >> 5;
  const int wt = wid % WT, xg = wid / WT;                    // this wave's weight tile and x-tile group
  const uint32_t swz = (uint32_t)((l31 >> 1) & 7);           // (tile bases are multiples of 32 rows)
  const uint32_t brow = (uint32_t)XB + (uint32_t)(wt * 32 + l31) * 128;

  union Frag {
    psg_u32x4 u;
    v8 v;
  };
  psg_f32x16 acc[MTG];
#pragma unroll
  for (int i = 0; i < MTG; ++i) acc[i] = (psg_f32x16){0};

  int slab = (int)(g0 / nk), ks = (int)(g0 - (int64_t)slab * nk);
  int pslab = slab, pks = ks;                                // the step the next DMA stage fetches
  int issued = 0;                                            // steps in flight (prologue: NST - 1)
#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (g0 + p < g1) {
      stage(pslab, pks, p);
      psg_sk_advance(pslab, pks, nk);
      ++issued;
    }
  const int S_fill = S_al == 0 ? S : 0;
  bool after_flush = false;
  int buf = 0;
  for (int64_t u = g0; u < g1; ++u) {
    // step u landed?  loads complete in order: the younger steps' loads may stay outstanding
    const int ahead = issued - 1;                            // younger steps in flight (<= NST - 2)
    if (after_flush) psg_vmwait<0>();                         // (stores of a flush may complete out of order with loads)
    else PsgDmaWait<PER, NST - 1>::go(ahead);
    after_flush = false;
    psg_lds_barrier();                                        // step u is in LDS; nobody reads the buffer of step u - 1 any more
    --issued;
    const bool pf = u + (NST - 1) < g1;
    int nb_ = buf + (NST - 1);
    nb_ = nb_ >= NST ? nb_ - NST : nb_;
    const uint32_t base = smem_lds + (uint32_t)(buf * STAGE);

    // matrix instruction j of a step covers K 16 j .. + 15: a lane's 8 values = piece 2 j + hi of its x row / weight row
    Frag af[2][4], bh[4], bl[NP == 2 ? 4 : 1];
    auto read_x = [&](int t, Frag (&a_)[4]) {                 // t = 2 i + plane: tile i of this wave's group, hi / lo plane
      int ti = (t >> 1) * XG + xg;
      ti = ti < MT ? ti : MT - 1;
      const uint32_t xrow = base + (uint32_t)((((t & 1) * MT + ti) * 32 + l31) * 128);
#pragma unroll
      for (int j = 0; j < 4; ++j) a_[j].u = psg_lds_read128(xrow + ((((uint32_t)(2 * j + hi)) ^ swz) << 4));
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) bh[j].u = psg_lds_read128(base + brow + ((((uint32_t)(2 * j + hi)) ^ swz) << 4));
    if (NP == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bl[j].u = psg_lds_read128(base + brow + (uint32_t)(BN * 128) + ((((uint32_t)(2 * j + hi)) ^ swz) << 4));
    }
    read_x(0, af[0]);
    if (pf) {
      stage(pslab, pks, nb_);
      psg_sk_advance(pslab, pks, nk);
      ++issued;
    }
    psg_lgkmwait<4>();                                        // (LDS reads return in order: the weight fragments are here)
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2 * MTG; ++t) {
      if (t + 1 < 2 * MTG) {
        read_x(t + 1, af[(t + 1) & 1]);
        psg_lgkmwait<4>();                                    // (tile t is here, tile t + 1 in flight under its products)
      } else {
        psg_lgkmwait<0>();
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t >> 1] = EF16::mfma32(af[t & 1][j].v, bh[j].v, acc[t >> 1]);   // D[m][n]
      if (NP == 2 && (t & 1) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t >> 1] = EF16::mfma32(af[t & 1][j].v, bl[j].v, acc[t >> 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);

    const bool slab_end = ks == nk - 1;
    if (slab_end || u == g1 - 1) {                           // the segment ends: one fp32 slice
      const int slot = psg_sk_slot(slab, nk, T, G, S_al);
      const int nslots = slab_end && S_fill > slot ? S_fill : slot + 1;   // ending a slab (stream-K): zero the slots it did not use
      // D[m][n]: register r of a lane = row 8 (r >> 2) + 4 hi + (r & 3) of the tile, column lane & 31
      const int n0 = slab * BN + wt * 32;
      if (n0 + l31 < N) {
        const float cs = col_scale[n0 + l31];
        asm volatile("" ::"v"(cs));                        // retired HERE on every path: a load the compiler still counts as
                                                           // pending at the loop head costs the DMA ring a vmcnt(0) per step
        float* ps = part + (int64_t)slot * M * N + n0 + l31;
#pragma unroll
        for (int i = 0; i < MTG; ++i) {
          const int ti = i * XG + xg;
          if (ti < MT) {                                     // (wave-uniform; the group's repeated last tile is not stored)
            // the lane's element offset walks down its rows: one register.  The asm statement keeps the offsets and row
            // masks - invariants of the step loop - from being hoisted out of it and held across the matrix instructions
            int off = (ti * 32 + 4 * hi) * N, Mf = M;
            asm volatile("" : "+v"(off), "+s"(Mf));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int m_ = ti * 32 + 8 * (r >> 2) + (r & 3) + 4 * hi;
              if (m_ < Mf) ps[off] = acc[i][r] * (row_scale[m_] * cs);
              off += (r & 3) == 3 ? 5 * N : N;               // rows 8 g + 4 hi + 0..3, then the next group of 8
            }
          }
        }
        if (xg == 0)
          for (int s_ = slot + 1; s_ < nslots; ++s_) {       // the slots this slab did not use: this lane's column, every
            float* pz = part + (int64_t)s_ * M * N + n0 + l31;   // second row
            for (int m_ = hi; m_ < M; m_ += 2) pz[(int64_t)m_ * N] = 0.f;
          }
      }
#pragma unroll
      for (int i = 0; i < MTG; ++i) acc[i] = (psg_f32x16){0};
      after_flush = true;
    }
    psg_sk_advance(slab, ks, nk);
    buf = buf + 1 == NST ? 0 : buf + 1;
  }
}

// ---- host side: plan and launch --------------------------------------------------------------------------------------
// psg_sk_make_plan's estimate with this step's cost: L2 -> LDS staging at ~40 B/clk/CU, the matrix instructions of the
// busiest wave at 32 clk on two waves per SIMD, or the unit's share of the HBM stream.  Made for 160 rows whatever M is.
static psg_sk_plan bs_make_plan(const psg_ctx* ctx, int N, int K, int np, int forced_mode) {
  const int G = ctx->num_cu < 1024 ? ctx->num_cu : 1024;
  const int bn = 256 / np, nk = K / BS_BK, NB = (N + bn - 1) / bn;
  const double mfma_us = (np == 1 ? 5 * 2 : 3 * 3) * 4 * 2 * 32 / 2.4e3;
  const double unit_us = fmax(fmax((double)bs_stage_bytes(5) / (40.0 * 2.4e3), mfma_us), (double)BS_WROWS * 128 * G / 5.8e6);
  return psg_sk_make_plan(G, NB, nk, N, unit_us, 160, forced_mode);
}

static int bs_plan_checked(const char* name, psg_ctx* ctx, int M, int N, int K, int np, int mode, psg_sk_plan* p, int* slots) {
  const int rc = psg_sk_check_args(name, ctx, slots, M, 33, 160, N, K, BS_BK, mode);
  if (rc != PSG_OK) return rc;
  *p = bs_make_plan(ctx, N, K, np, mode);
  return psg_sk_plan_ok(name, *p, N, K, mode, slots);
}

template <int NP, int MT>
static int bs_launch_mt(const char* name, const psg_sk_plan& p, const void* x2, const void* w, float* part, int M, int N, int K,
                        int64_t wstride, int64_t lo_off, const float* row_scale, const float* col_scale, void* stream) {
  constexpr int LDS = bs_nst(MT) * bs_stage_bytes(MT);
  return psg_sk_launch(name, bs_gemm_kernel<NP, MT>, p.grid, LDS, stream, x2, w, part, M, N, K, wstride, lo_off, p.slots, p.s_al,
                       row_scale, col_scale);
}

// x2 / w: 16-byte-aligned rows (the LDS-DMA pieces); w32: the low plane lies behind the high one inside a row
template <int NP>
static int bs_pair(const char* name, psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w, int64_t wstride,
                   int64_t lo_off, const float* col_scale, float* part, int M, int N, int K, int slots, int mode, void* stream) {
  PSG_REQUIRE(ctx && x2 && inv_scale && w && col_scale && part, PSG_ERR_INVALID, "%s: NULL argument", name);
  psg_sk_plan p;
  int want = 0;
  int rc = bs_plan_checked(name, ctx, M, N, K, NP, mode, &p, &want);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE((uintptr_t)x2 % 16 == 0 && (uintptr_t)w % 16 == 0 && wstride % 8 == 0 && wstride >= (int64_t)NP * K &&
                  (NP == 1 || (lo_off % 8 == 0 && lo_off >= K && lo_off + K <= wstride)),
              PSG_ERR_UNSUPPORTED, "%s: rows must be 16-byte aligned: x2=%p w=%p row stride=%lld lo_off=%lld (K=%d)", name, x2, w,
              (long long)wstride, (long long)lo_off, K);
  rc = psg_sk_check_slots(name, slots, want, N, K);
  if (rc != PSG_OK) return rc;
  // M picks the x tiles that are staged and multiplied (2 / 3 / 5), nothing else
  if (M <= 64) return bs_launch_mt<NP, 2>(name, p, x2, w, part, M, N, K, wstride, lo_off, inv_scale, col_scale, stream);
  if (M <= 96) return bs_launch_mt<NP, 3>(name, p, x2, w, part, M, N, K, wstride, lo_off, inv_scale, col_scale, stream);
  return bs_launch_mt<NP, 5>(name, p, x2, w, part, M, N, K, wstride, lo_off, inv_scale, col_scale, stream);
}

extern "C" int psg_batch_split_gemm_w16_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  psg_sk_plan p;
  return bs_plan_checked("psg_batch_split_gemm_w16_plan", ctx, M, N, K, 1, mode, &p, slots);
}
extern "C" int psg_batch_split_gemm_w16(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w16, int64_t row_stride,
                                        const float* col_scale, float* part, int M, int N, int K, int slots, int mode,
                                        void* stream) {
  return bs_pair<1>("psg_batch_split_gemm_w16", ctx, x2, inv_scale, w16, row_stride, 0, col_scale, part, M, N, K, slots, mode,
                    stream);
}
extern "C" int psg_batch_split_gemm_w32_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  psg_sk_plan p;
  return bs_plan_checked("psg_batch_split_gemm_w32_plan", ctx, M, N, K, 2, mode, &p, slots);
}
extern "C" int psg_batch_split_gemm_w32(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w_img,
                                        int64_t row_stride, int64_t lo_off, const float* col_scale, float* part, int M, int N,
                                        int K, int slots, int mode, void* stream) {
  return bs_pair<2>("psg_batch_split_gemm_w32", ctx, x2, inv_scale, w_img, row_stride, lo_off, col_scale, part, M, N, K, slots, mode,
                    stream);
}
