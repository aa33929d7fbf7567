// Batched decode-step projections of the fp32s mode over bf16-VALUED weights held as their bf16 copy ONLY:
// part[s][m][n] = split-K slices of x[M][K] . W[N][K]^T for 33 <= M <= 160 fp32 rows given as the three bf16 planes
// [3][M][K] of psg_split_b16x3 (x = x0 + x1 + x2 exactly, psg_split_b16.h), W a bf16 value w[N][K]:
//   psg_batch_split_gemm_wb16   part = x2 . w + x1 . w + x0 . w           - psg_split_gemm_wb16's products above 32 rows
// Every product of two bf16 values is exact in fp32; all three planes' products of an output element go into ONE fp32
// accumulator, per K step from the smallest plane up (x2, x1, x0).  No row scale, no column scale.
//
// Layout - psg_batch_gemm_s.hip's kernel shape (bs_gemm_kernel) with a third x plane:
//   * K step 64: an x row and a weight row of a step are both 128 bytes = 8 pieces of 16 bytes, XOR-swizzled on the SOURCE
//     address with (row >> 1) & 7; one LDS-DMA instruction fetches 8 rows;
//   * the x image of a step is 3 planes x MT x 32 rows (MT = 2 / 3 / 5 for M <= 64 / 96 / 160): 24 / 36 / 60 KB;
//   * the weight image of a step is a slab of 128 weight rows x 128 B = 16 KB at EVERY MT: with the 256-row slab of the w16
//     form a stage of MT = 5 is 92 KB and only one fits the 160 KB of a CU; a slab height that changed with MT would change
//     the plan - and with it the k range of every slot - with the row count;
//   * a step is ONE stage [x | w] of the ring: 40 / 52 / 76 KB -> 3 / 3 / 2 stages, counted vmcnt.  40 / 52 / 76 DMA
//     instructions are no multiple of the 8 waves at MT = 3 / 5: waves 0..3 issue one more, and count one more per stage;
//   * the waves are dealt as the w32 form deals them: 4 weight tiles x 2 groups of x tiles (tiles g, g + 2, ...: <= 3 per
//     wave, 48 accumulator registers); the wave's weight fragments stay in registers through the step.  A group with one
//     tile less repeats its last product on a copy and does not store it: the step ends at the barrier with the full group;
//   * per x tile and step the order is x2.w, x1.w, x0.w, each 4 matrix instructions (v_mfma_f32_32x32x16_bf16) over K = 16;
//   * ranges, slots, plan and launch: psg_streamk.h.
// Row independence: the plan is a function of (N, K, mode) ONLY and is made for 160 rows; M picks MT, which decides what is
// staged and which tiles a wave multiplies, never a slot's k range nor the order of a row's sum.
#include "psg_common.h"
#include "psg_streamk.h"
#include "psg_wave.h"

#define B3_BK 64
#define B3_WAVES 8
#define B3_BN 128                                             // weight rows of a slab
#define B3_XG 2                                               // x-tile groups
#define B3_LDS_MAX (160 * 1024)

__host__ __device__ constexpr int b3_stage_bytes(int mt) { return (3 * mt * 32 + B3_BN) * 128; }
__host__ __device__ constexpr int b3_nst(int mt) { return B3_LDS_MAX / b3_stage_bytes(mt) > 3 ? 3 : B3_LDS_MAX / b3_stage_bytes(mt); }

// S_al > 0: aligned ranges, 0: stream-K (psg_streamk.h)
template <int MT>
__global__ void __launch_bounds__(B3_WAVES * 64, 1)
b3_gemm_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w, float* __restrict__ part, int M, int N, int K,
               int S, int S_al) {
  using v8 = EBf16::v8;
  constexpr int NST = b3_nst(MT);
  constexpr int XG = B3_XG, WT = B3_WAVES / XG, BN = B3_BN;    // x-tile groups, weight tiles and weight rows of a slab
  static_assert(WT * 32 == BN, "one 32-row weight tile per wave of a group");
  constexpr int MTG = (MT + XG - 1) / XG;                      // x tiles of a wave
  constexpr int XR = 3 * MT * 32, XB = XR * 128;               // the x image: plane 0's MT tiles, then plane 1's, plane 2's
  constexpr int STAGE = b3_stage_bytes(MT);
  constexpr int XI = XB / 1024, NI = STAGE / 1024;             // 16-byte DMA instructions (1 KB = 8 rows each): x / x and w
  constexpr int PER = NI / B3_WAVES, REM = NI % B3_WAVES;      // per wave; waves 0 .. REM - 1 issue one more
  static_assert(NST >= 2 && NST * STAGE <= B3_LDS_MAX, "LDS of a CU");
  static_assert((NST - 1) * (PER + 1) <= 63, "vmcnt field");
  static_assert(XR % 16 == 0, "a weight row's swizzle is its stage row's");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t smem_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int nk = K / B3_BK, NB = (N + BN - 1) / BN;
  const int64_t T = (int64_t)NB * nk;
  const int G = gridDim.x;
  const psg_sk_span span = psg_sk_range(nk, T, G, S_al);
  const int64_t g0 = span.g0, g1 = span.g1;
  if (g0 >= g1) return;

  // instruction idx of a step: 1 KB idx of the step's [x | w] image = 8 rows x 8 pieces; a wave issues idx = wid + 8 q
  auto stage = [&](int slab, int ks, int buf) {              // this wave's DMAs of one step: PER (+ 1) instructions
    unsigned char* sb = smem + buf * STAGE;
#pragma unroll
    for (int q = 0; q < PER + (REM ? 1 : 0); ++q) {
      const int idx = wid + B3_WAVES * q;
      if (idx >= NI) continue;                               // (wave-uniform: the last round belongs to waves 0 .. REM - 1)
      const int r = idx * 8 + (lane >> 3);                   // row of the stage
      const int piece = (lane & 7) ^ ((r >> 1) & 7);
      if (idx < XI) {                                        // (MT x 32 is a multiple of 8: an instruction's rows share a plane)
        const int plane = r / (MT * 32), xr = r - plane * (MT * 32);
        const int64_t gr = (int64_t)plane * M + (xr < M ? xr : M - 1);   // (rows past M: a copy of the last row, never stored)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(x + gr * K + ks * B3_BK + piece * 8),
            (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 0);
      } else {
        int gr = slab * BN + (r - XR);
        gr = gr < N ? gr : N - 1;                            // (rows past N: a copy of the last row, never stored)
        __builtin_amdgcn_global_load_lds(                    // a weight byte is read once by one CU: non-temporal
            (const __attribute__((address_space(1))) void*)(w + (int64_t)gr * K + ks * B3_BK + piece * 8),
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
    else if (REM && wid < REM) PsgDmaWait<PER + 1, NST - 1>::go(ahead);
    else PsgDmaWait<PER, NST - 1>::go(ahead);
    after_flush = false;
    psg_lds_barrier();                                        // step u is in LDS; nobody reads the buffer of step u - 1 any more
    --issued;
    const bool pf = u + (NST - 1) < g1;
    int nb_ = buf + (NST - 1);
    nb_ = nb_ >= NST ? nb_ - NST : nb_;
    const uint32_t base = smem_lds + (uint32_t)(buf * STAGE);

    // matrix instruction j of a step covers K 16 j .. + 15: a lane's 8 values = piece 2 j + hi of its x row / weight row
    Frag af[2][4], bw[4];
    auto read_x = [&](int t, Frag (&a_)[4]) {                 // t = 3 i + s: tile i of this wave's group, plane 2 - s
      int ti = (t / 3) * XG + xg;
      ti = ti < MT ? ti : MT - 1;
      const uint32_t xrow = base + (uint32_t)((((2 - t % 3) * MT + ti) * 32 + l31) * 128);
#pragma unroll
      for (int j = 0; j < 4; ++j) a_[j].u = psg_lds_read128(xrow + ((((uint32_t)(2 * j + hi)) ^ swz) << 4));
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) bw[j].u = psg_lds_read128(base + brow + ((((uint32_t)(2 * j + hi)) ^ swz) << 4));
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
    for (int t = 0; t < 3 * MTG; ++t) {
      if (t + 1 < 3 * MTG) {
        read_x(t + 1, af[(t + 1) & 1]);
        psg_lgkmwait<4>();                                    // (operand t is here, operand t + 1 in flight under its products)
      } else {
        psg_lgkmwait<0>();
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t / 3] = EBf16::mfma32(af[t & 1][j].v, bw[j].v, acc[t / 3]);   // D[m][n]
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
              if (m_ < Mf) ps[off] = acc[i][r];
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
// busiest wave (3 tiles x 3 planes x 4 instructions) at 32 clk on two waves per SIMD, or the unit's share of the HBM stream.
// Made for 160 rows whatever M is.
static psg_sk_plan b3_make_plan(const psg_ctx* ctx, int N, int K, int forced_mode) {
  const int G = ctx->num_cu < 1024 ? ctx->num_cu : 1024;
  const int nk = K / B3_BK, NB = (N + B3_BN - 1) / B3_BN;
  const double mfma_us = 3 * 3 * 4 * 2 * 32 / 2.4e3;
  const double unit_us = fmax(fmax((double)b3_stage_bytes(5) / (40.0 * 2.4e3), mfma_us), (double)B3_BN * 128 * G / 5.8e6);
  return psg_sk_make_plan(G, NB, nk, N, unit_us, 160, forced_mode);
}

static int b3_plan_checked(const char* name, psg_ctx* ctx, int M, int N, int K, int mode, psg_sk_plan* p, int* slots) {
  const int rc = psg_sk_check_args(name, ctx, slots, M, 33, 160, N, K, B3_BK, mode);
  if (rc != PSG_OK) return rc;
  *p = b3_make_plan(ctx, N, K, mode);
  return psg_sk_plan_ok(name, *p, N, K, mode, slots);
}

template <int MT>
static int b3_launch_mt(const char* name, const psg_sk_plan& p, const void* x3, const void* w, float* part, int M, int N, int K,
                        void* stream) {
  constexpr int LDS = b3_nst(MT) * b3_stage_bytes(MT);
  return psg_sk_launch(name, b3_gemm_kernel<MT>, p.grid, LDS, stream, x3, w, part, M, N, K, p.slots, p.s_al);
}

extern "C" int psg_batch_split_gemm_wb16_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  psg_sk_plan p;
  return b3_plan_checked("psg_batch_split_gemm_wb16_plan", ctx, M, N, K, mode, &p, slots);
}

// x3 / wb16: 16-byte-aligned contiguous rows (the LDS-DMA pieces)
extern "C" int psg_batch_split_gemm_wb16(psg_ctx* ctx, const void* x3, const void* wb16, float* part, int M, int N, int K,
                                         int slots, int mode, void* stream) {
  const char* name = "psg_batch_split_gemm_wb16";
  PSG_REQUIRE(ctx && x3 && wb16 && part, PSG_ERR_INVALID, "%s: NULL argument", name);
  psg_sk_plan p;
  int want = 0;
  int rc = b3_plan_checked(name, ctx, M, N, K, mode, &p, &want);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(((uintptr_t)x3 | (uintptr_t)wb16 | (uintptr_t)part) % 16 == 0, PSG_ERR_UNSUPPORTED,
              "%s: x3, w and part must be 16-byte aligned: x3=%p w=%p part=%p", name, x3, wb16, (void*)part);
  rc = psg_sk_check_slots(name, slots, want, N, K);
  if (rc != PSG_OK) return rc;
  // M picks the x tiles that are staged and multiplied (2 / 3 / 5), nothing else
  if (M <= 64) return b3_launch_mt<2>(name, p, x3, wb16, part, M, N, K, stream);
  if (M <= 96) return b3_launch_mt<3>(name, p, x3, wb16, part, M, N, K, stream);
  return b3_launch_mt<5>(name, p, x3, wb16, part, M, N, K, stream);
}
