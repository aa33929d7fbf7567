// The 32-row weight-streaming GEMM over a QUANTISED weight, written once for psg_gemm_w8.hip (FP8), psg_gemm_w4.hip
// (MXFP4) and psg_gemm_int4.hip (group-wise INT4): part[s][m][n] = split-K slices of x[M][K] . W'[N][K]^T, M <= 32.
// The weight streams from HBM in its packed form, is widened to the x operand's 16-bit type in registers and multiplied
// on v_mfma_f32_32x32x16 with fp32 accumulation.
//   PAIR   : x is the two fp16 planes [2][M][K] + inv_scale[M] of psg_split_f16x2 / psg_rmsnorm_split2 (fp32s mode);
//   single : x is [M][K] bf16 or fp16.
// The schedule is the pair form of psg_batch_gemm.hip's: ranges of (slab, K step) units (psg_streamk.h) dealt to one
// workgroup per CU, LDS-DMA into a ring of units with counted vmcnt, 8 waves x one 32-row weight tile, k-ordered slices
// without atomics.
//   * a unit is 256 weight rows x Fmt::BK K, and BK is chosen so that a packed weight row of it is 128 bytes - the row
//     the 2-byte kernel stages per K step of 64: the weight image keeps that kernel's 16-byte pieces, its XOR swizzle on
//     the source address and its conflict-free ds_read_b128.  ONE read per lane is weight piece p = 16 bytes = BK / 8 K;
//   * x is staged as BK / 64 [rows][128 B] images per unit (K halves / quarters), each exactly the 2-byte kernel's x image;
//   * the matrix instruction sums over 16 K and does not care WHICH 16 as long as both operands agree: the lane that holds
//     weight piece p feeds it, 8 K at a time, to BK / 64 matrix instructions against x pieces (BK / 64) p .. of the same
//     lane half.  No shuffling;
//   * a format with per-row side data (block exponents, group scales: Fmt::SIDE = 8 bytes per row and unit) passes it
//     re-laid-out as side[K / BK][N][8].  It arrives by LDS-DMA too (no global_load beside the ring, which would drain
//     it): a wave's 32 rows of a unit are 256 contiguous bytes - one 4-byte DMA per wave and unit, into the wave's own 256
//     bytes of the stage - and a lane reads its row's with ONE ds_read per unit;
//   * a unit is four sub-steps (weight pieces 2 s2 + hi); the fragment reads run one sub-step ahead of the matrix
//     instructions and the next unit's DMAs are issued between them.
// A row's result does not depend on the other rows (nor on M: the plan is made for 32 rows whatever M is).
//
// What a format supplies (struct Fmt):
//   BK                      K of a unit: 128 (one byte per weight) or 256 (half a byte)
//   SIDE                    bytes of side data per weight row and unit: 0 or 8
//   SIDE_HI                 where in its row's SIDE bytes lane half 1 (lanes 32-63) reads, lane half 0 reading at 0
//   nst(pair)               ring depth
//   COL_SCALE               whether col_scale[n] multiplies what a slice stores
//   ALIGNED                 the operands of the 16-byte alignment check, for its message
//   Acc<E, XT>              the accumulator state of a lane:
//     zero()                  before the first unit and after every flush
//     unit(side_addr)         the lane's LDS read of its side data, once per unit, before the fragment reads
//     step(s2, a, b)          sub-step s2: widen weight piece b and multiply it with the x pieces a[XT][BK / 64]
//     out(r)                  accumulator register r as a slice stores it, before the row and column scales
#pragma once
#include "psg_common.h"
#include "psg_streamk.h"
#include "psg_wave.h"

#define Q32_BN 256
#define Q32_WAVES 8

template <typename E>
union PsgQ32Frag {                                           // a ds_read_b128 as the matrix instruction's 8 x 16-bit operand
  psg_u32x4 u;
  typename E::v8 v;
};

template <typename Fmt>
__host__ __device__ constexpr int psg_q32_stage_bytes(bool pair) {   // one unit: [x: BK / 64 images | w: 256 rows x 128 B | side]
  return Fmt::BK / 64 * (pair ? 64 : 32) * 128 + Q32_BN * 128 + Q32_BN * Fmt::SIDE;
}

template <typename Fmt, typename E, bool PAIR>
__global__ void __launch_bounds__(Q32_WAVES * 64, 1)
psg_q32_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const uint8_t* __restrict__ side,
                    float* __restrict__ part, int M, int N, int K, int S, int S_al, const float* __restrict__ row_scale,
                    const float* __restrict__ col_scale) {
  constexpr int BK = Fmt::BK, NST = Fmt::nst(PAIR);
  constexpr int NJ = BK / 64;                                // x images per unit = x pieces per weight piece
  constexpr int XT = PAIR ? 2 : 1, XR = XT * 32;             // x tiles of 32 rows (PAIR: plane 0, plane 1)
  constexpr int XQ = XR * 128, XB = NJ * XQ;                 // one x image / all of them
  constexpr int WB = Q32_BN * 128;                           // the weight image
  constexpr int STAGE = psg_q32_stage_bytes<Fmt>(PAIR);
  constexpr int XI = XB / 1024, NI = (XB + WB) / 1024;       // 16-byte DMA instructions (8 rows x 128 B each): x / x and w
  constexpr int EX = Fmt::SIDE ? 1 : 0;
  constexpr int PER = NI / Q32_WAVES + EX;                   // per wave and unit: its share of x and w + its rows' side data
  static_assert(BK == 128 || BK == 256, "a packed weight row of a unit is 128 bytes");
  static_assert(Fmt::SIDE == 0 || Fmt::SIDE == 8, "side data: one 4-byte DMA per lane pair and row");
  static_assert(STAGE == XB + WB + Q32_BN * Fmt::SIDE && NST * STAGE <= 160 * 1024, "LDS of a CU");
  static_assert(NI % Q32_WAVES == 0 && XR % 16 == 0, "uniform DMA counts, operand-local swizzle");
  static_assert(NST >= 2 && NST <= 3 && (NST - 1) * PER <= 63, "the wait ladder below, vmcnt field");
  constexpr int NR = 1 + NJ * XT;                            // LDS reads of one sub-step
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t smem_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int nk = K / BK, NB = (N + Q32_BN - 1) / Q32_BN;
  const int64_t T = (int64_t)NB * nk;
  const int G = gridDim.x;
  const psg_sk_span span = psg_sk_range(nk, T, G, S_al);
  const int64_t g0 = span.g0, g1 = span.g1;
  if (g0 >= g1) return;

  const int srow = lane >> 3, sslot = lane & 7;
  const int Kb = K >> (BK / 256);                            // bytes of a weight row (128 per K step)
  // instruction idx of a unit: 128-byte rows 8 idx .. + 7 of the unit's image; a wave issues idx = wid, wid + 8, ...
  auto stage_one = [&](int slab, int kt, unsigned char* sb, int idx) {
    const int r = idx * 8 + srow;
    const int piece = sslot ^ ((r >> 1) & 7);                // (XR and XI * 8 are multiples of 16: the operand-local row's swizzle)
    if (idx < XI) {
      const int img = r / XR, xr = r - img * XR;
      int gr = xr < M ? xr : M - 1;
      if (PAIR) gr = (xr >> 5) * M + ((xr & 31) < M ? (xr & 31) : M - 1);   // plane xr >> 5, row xr & 31 of [2][M][K]
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(x + (int64_t)gr * K + kt * BK + img * 64 + piece * 8),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 0);
    } else {
      int gr = slab * Q32_BN + (r - XI * 8);
      gr = gr < N ? gr : N - 1;
      __builtin_amdgcn_global_load_lds(                      // a weight byte is read once by one CU: non-temporal
          (const __attribute__((address_space(1))) void*)(w + (int64_t)gr * Kb + kt * 128 + piece * 16),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 2);
    }
  };
  // the side data of this wave's 32 rows of the unit: lane -> dword lane & 1 of row lane >> 1, LDS = its slot + 4 lane
  auto stage_side = [&](int slab, int kt, unsigned char* sb) {
    int gr = slab * Q32_BN + wid * 32 + (lane >> 1);
    gr = gr < N ? gr : N - 1;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(side + ((int64_t)kt * N + gr) * 8 + (lane & 1) * 4),
        (__attribute__((address_space(3))) void*)(sb + XB + WB + wid * 256), 4, 0, 2);
  };
  auto stage = [&](int slab, int kt, int buf, int q0, int q1) {   // this wave's instructions q0 .. q1 - 1 of the unit
    unsigned char* sb = smem + buf * STAGE;
    for (int q = q0; q < q1; ++q) {
      if (q < PER - EX) stage_one(slab, kt, sb, wid + Q32_WAVES * q);
      else if (EX && q == PER - 1) stage_side(slab, kt, sb);
    }
  };

  const int l31 = lane & 31, hi = lane >> 5;
  uint32_t arow[XT];
#pragma unroll
  for (int i = 0; i < XT; ++i) arow[i] = (uint32_t)((i * 32 + l31) * 128);
  const uint32_t aswz = (uint32_t)((l31 >> 1) & 7);          // (tile bases are multiples of 32 rows)
  const uint32_t brow = (uint32_t)(XB + (wid * 32 + l31) * 128), bswz = aswz;
  const uint32_t srow_lds = (uint32_t)(XB + WB + (wid * 32 + l31) * 8 + hi * Fmt::SIDE_HI);   // this lane's side data

  using Frag = PsgQ32Frag<E>;
  typename Fmt::template Acc<E, XT> acc;
  acc.zero();

  int slab = (int)(g0 / nk), kt = (int)(g0 - (int64_t)slab * nk);
  int pslab = slab, pkt = kt;                                // the unit the next DMA stage fetches
  int issued = 0;                                            // units in flight (prologue: NST - 1)
#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (g0 + p < g1) {
      stage(pslab, pkt, p, 0, PER);
      psg_sk_advance(pslab, pkt, nk);
      ++issued;
    }
  bool after_flush = false;
  int buf = 0;
  constexpr int QH = (PER + 1) / 2;                          // DMA instructions issued beside the first sub-step
  for (int64_t u = g0; u < g1; ++u) {
    // unit u landed?  loads complete in order: the younger units' loads may stay outstanding
    const int ahead = issued - 1;                            // younger units in flight (<= NST - 2)
    if (after_flush || ahead <= 0) psg_vmwait<0>();           // (stores of a flush may complete out of order with loads)
    else if (ahead == 1) psg_vmwait<PER>();
    else psg_vmwait<2 * PER>();
    after_flush = false;
    psg_lds_barrier();                                        // unit u is in LDS; nobody reads the buffer of unit u - 1 any more
    --issued;
    const bool pf = u + (NST - 1) < g1;
    int nb_ = buf + (NST - 1);
    nb_ = nb_ >= NST ? nb_ - NST : nb_;
    const uint32_t base = smem_lds + (uint32_t)(buf * STAGE);
    Frag af[2][XT][NJ];
    psg_u32x4 bq[2];
    acc.unit(base + srow_lds);
    // sub-step s2: weight piece p = 2 s2 + hi (K BK / 8 p .. of the unit), x pieces NJ p .. NJ p + NJ - 1 of the unit's K
    auto read_frags = [&](int s2, Frag (&a_)[XT][NJ], psg_u32x4& b_) {
      const uint32_t p = (uint32_t)(2 * s2 + hi);
      b_ = psg_lds_read128(base + brow + ((p ^ bswz) << 4));
      const uint32_t xq = base + (p / (8 / NJ)) * XQ, x0 = (NJ * p) & 7;
#pragma unroll
      for (int i = 0; i < XT; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) a_[i][j].u = psg_lds_read128(xq + arow[i] + (((x0 + j) ^ aswz) << 4));
    };
    read_frags(0, af[0], bq[0]);
    read_frags(1, af[1], bq[1]);
    if (pf) stage(pslab, pkt, nb_, 0, QH);
    psg_lgkmwait<NR>();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    acc.step(0, af[0], bq[0]);
    __builtin_amdgcn_sched_barrier(0);
    read_frags(2, af[0], bq[0]);
    if (pf) stage(pslab, pkt, nb_, QH, PER);
    psg_lgkmwait<NR>();
    __builtin_amdgcn_sched_barrier(0);
    acc.step(1, af[1], bq[1]);
    __builtin_amdgcn_sched_barrier(0);
    read_frags(3, af[1], bq[1]);
    psg_lgkmwait<NR>();
    __builtin_amdgcn_sched_barrier(0);
    acc.step(2, af[0], bq[0]);
    psg_lgkmwait<0>();
    __builtin_amdgcn_sched_barrier(0);
    acc.step(3, af[1], bq[1]);
    __builtin_amdgcn_s_setprio(0);
    if (pf) {
      psg_sk_advance(pslab, pkt, nk);
      ++issued;
    }

    const bool slab_end = kt == nk - 1;
    if (slab_end || u == g1 - 1) {                           // the segment ends: one fp32 slice
      const int slot = psg_sk_slot(slab, nk, T, G, S_al);
      const int nslots = (slab_end && S_al == 0) ? S : slot + 1;   // ending a slab (stream-K): zero the slots it did not use
      // D[m][n]: register r of a lane = row 8 (r >> 2) + 4 hi + (r & 3) of the tile, column lane & 31
      const int n0 = slab * Q32_BN + wid * 32;
      if (n0 + l31 < N) {
        const float cs = Fmt::COL_SCALE ? col_scale[n0 + l31] : 1.f;
        const int lane_off = 4 * hi * N + l31;
        float rs[16];                                        // (all sixteen loads in flight before the first store waits)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m_ = 8 * (r >> 2) + (r & 3) + 4 * hi;
          rs[r] = PAIR ? row_scale[m_ < M ? m_ : M - 1] * cs : cs;
        }
        for (int s_ = slot; s_ < nslots; ++s_) {
          float* ps = part + (int64_t)s_ * M * N;
          const bool real = s_ == slot;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int mrow = 8 * (r >> 2) + (r & 3);
            float* rowp = ps + (int64_t)mrow * N + n0;
            if (mrow + 4 * hi < M) {
              float val = 0.f;
              if (real) val = acc.out(r) * rs[r];
              rowp[lane_off] = val;
            }
          }
        }
      }
      acc.zero();
      after_flush = true;
    }
    psg_sk_advance(slab, kt, nk);
    buf = buf + 1 == NST ? 0 : buf + 1;
  }
}

// ---- host side: plan and launch --------------------------------------------------------------------------------------
// The unit's cost: L2 -> LDS staging at ~40 B/clk/CU, or the unit's share of the HBM stream.  Made for 32 rows whatever M
// is: a row's k ranges must not follow the row count.
template <typename Fmt>
static psg_sk_plan psg_q32_make_plan(const psg_ctx* ctx, int N, int K, int forced_mode, bool pair) {
  const int G = ctx->num_cu < 1024 ? ctx->num_cu : 1024;
  const int nk = K / Fmt::BK, NB = (N + Q32_BN - 1) / Q32_BN;
  const int stage = psg_q32_stage_bytes<Fmt>(pair);
  const double unit_us = fmax((double)stage / (40.0 * 2.4e3), (double)Q32_BN * (128 + Fmt::SIDE) * G / 5.8e6);
  return psg_sk_make_plan(G, NB, nk, N, unit_us, 32, forced_mode);
}

template <typename Fmt>
static int psg_q32_plan_checked(const char* name, psg_ctx* ctx, int M, int N, int K, int mode, bool pair, psg_sk_plan* p,
                                int* slots) {
  const int rc = psg_sk_check_args(name, ctx, slots, M, 1, 32, N, K, Fmt::BK, mode);
  if (rc != PSG_OK) return rc;
  *p = psg_q32_make_plan<Fmt>(ctx, N, K, mode, pair);
  return psg_sk_plan_ok(name, *p, N, K, mode, slots);
}

// An entry point after its NULL check: plan, the slot count the caller allocated, the operands' alignment (every
// operand is fetched by 16-byte LDS-DMA), x's type, launch.  PAIR: x is fp16 planes, dtype is not looked at.
template <typename Fmt, bool PAIR>
static int psg_q32_run(const char* name, psg_ctx* ctx, const void* x, const void* w, const void* side, const float* row_scale,
                       const float* col_scale, float* part, int M, int N, int K, int slots, int dtype, int mode, void* stream) {
  psg_sk_plan p;
  int want = 0;
  int rc = psg_q32_plan_checked<Fmt>(name, ctx, M, N, K, mode, PAIR, &p, &want);
  if (rc == PSG_OK) rc = psg_sk_check_slots(name, slots, want, N, K);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)side & 15) == 0, PSG_ERR_UNSUPPORTED,
              "%s: %s must be 16-byte aligned", name, Fmt::ALIGNED);
  constexpr int LDS = Fmt::nst(PAIR) * psg_q32_stage_bytes<Fmt>(PAIR);
#define Q32_GO(E_) \
  return psg_sk_launch(name, psg_q32_gemm_kernel<Fmt, E_, PAIR>, p.grid, LDS, stream, x, w, side, part, M, N, K, p.slots, p.s_al, \
                       row_scale, col_scale)
  if constexpr (PAIR) Q32_GO(EF16);
  else PSG_DISPATCH_E16(dtype, name, Q32_GO(E));
#undef Q32_GO
  return PSG_ERR_INVALID;
}
