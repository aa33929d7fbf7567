// Batched decode-step projections over QUANTISED weights: part[s][m][n] = split-K slices of
// x[M][K] . W'[N][K]^T for 33 <= M <= 160 rows (`head.forward_batch`: 2 / 4 / 8 images = 40 / 80 / 160 decode rows), where
// W' is the model's weight of psg_gemm_w8.hip (e4m3 bytes x col_scale[n]) or of psg_gemm_w4.hip (e2m1 nibbles x
// 2^(e - 127) per 32 x col_scale[n]).  The arithmetic is exactly that of those two families: the bytes / nibbles are
// widened to the x operand's 16-bit type in registers (v_cvt_scalef32_pk_{f16,bf16}_fp8 at scale 1.0,
// v_cvt_scalef32_pk_{f16,bf16}_fp4 at the block's 2^(e - 127): both exact), multiplied on v_mfma_f32_32x32x16 with fp32
// accumulation, and the scales are applied once, in fp32, where a slice is stored:
//   single (psg_batch_gemm_w8 / _w4, bf16 / fp16 x[M][K]):                   part = (x . q) col_scale[n]
//   PAIR   (psg_batch_split_gemm_w8 / _w4, fp16 planes [2][M][K] + inv_scale): part = (xh . q + xl . q) inv_scale[m] col_scale[n]
// No fp8 / MX matrix instruction, no activation quantisation.
//
// Layout (the 32-row tile shape does not scale: 160 rows of x under a 128-byte weight row are 40 / 80 KB per unit):
//   * the K step is 64 for every format, so an x row of a step is 128 bytes - psg_batch_gemm.hip's x image, its 16-byte
//     pieces and its XOR swizzle - and the x image of a step is MT x 32 rows (PAIR: both planes): 8 / 12 / 20 KB, PAIR twice;
//   * a step's weight image is 256 rows x 64 bytes (fp8) or x 32 bytes (fp4): 16 / 8 KB.  One LDS-DMA instruction fetches
//     16 (32) weight rows x 4 (2) pieces of 16 bytes, lane-linear in LDS; the piece is swizzled on the SOURCE address with
//     (row >> 2) & 3 (fp8) / (row >> 3) & 1 (fp4), which spreads the 16 rows of a quarter-wave ds_read_b128 over all banks;
//   * fp4: the step's block exponents ride along as in psg_gemm_w4.hip (one 4-byte DMA per wave: the dword [h][0..3] of
//     e_img[K / 256][N][2][4] of its 32 rows); the step K/64 = 4 kt + q uses byte q;
//   * a step is ONE stage of the ring: [x | w | e], 18-56 KB.  The ring is as deep as 160 KiB hold, at most 4 and at least
//     2 stages (fp8 PAIR at 160 rows: 2 x 56 KB; fp4 PAIR at 160 rows: 3 x 50 KB; everything else: 4), counted vmcnt;
//   * 8 waves x one 32-row weight tile; every wave walks all MT x tiles (PAIR: 2 MT, the low plane's products are added
//     to the SAME fp32 accumulators as the high plane's: 16 MT <= 80 accumulator registers in both forms).  Fragment reads
//     of the next x tile are in flight under the MFMAs of this one;
//   * ranges of (slab, K step) units, stream-K or slab-aligned, k-ordered fp32 slices without atomics, unused slots
//     zero-filled: psg_batch_gemm.hip's.
// Row independence: the plan - grid, ranges, slots - is a function of (N, K, format, form, mode) ONLY.  M picks MT (2 / 3 /
// 5 x tiles), which decides what is staged and multiplied, never which k a slot covers or in what order a row's products
// are summed: rows 0..32 of a 160-row call are bit-equal to the same rows of a 33-row call.
#include "psg_common.h"
#include "psg_streamk.h"
#include "psg_wave.h"

#define BQ_BK 64
#define BQ_BN 256
#define BQ_WAVES 8
#define BQ_LDS_MAX (160 * 1024)

__host__ __device__ constexpr int bq_wrow_bytes(int fmt) { return fmt == 8 ? 64 : 32; }
__host__ __device__ constexpr int bq_stage_bytes(int fmt, bool pair, int mt) {
  return mt * 32 * (pair ? 2 : 1) * 128 + BQ_BN * bq_wrow_bytes(fmt) + (fmt == 4 ? BQ_BN * 8 : 0);
}
__host__ __device__ constexpr int bq_nst(int fmt, bool pair, int mt) {
  return BQ_LDS_MAX / bq_stage_bytes(fmt, pair, mt) > 4 ? 4 : BQ_LDS_MAX / bq_stage_bytes(fmt, pair, mt);
}

template <typename E>
struct BqCvt;
template <>
struct BqCvt<EF16> {
  static __device__ __forceinline__ EF16::v2 fp8(uint32_t v, bool hi) {
    return hi ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, false);
  }
  template <int SEL>
  static __device__ __forceinline__ EF16::v2 fp4(uint32_t v, float scale) {
    return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, scale, SEL);
  }
};
template <>
struct BqCvt<EBf16> {
  static __device__ __forceinline__ EBf16::v2 fp8(uint32_t v, bool hi) {
    return hi ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, false);
  }
  template <int SEL>
  static __device__ __forceinline__ EBf16::v2 fp4(uint32_t v, float scale) {
    return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, SEL);
  }
};
// 8 e4m3 bytes (two dwords, K ascending with the address) -> 8 values of E's type
template <typename E>
__device__ __forceinline__ typename E::v8 bq_widen8(uint32_t d0, uint32_t d1) {
  const typename E::v2 a = BqCvt<E>::fp8(d0, false), b = BqCvt<E>::fp8(d0, true), c = BqCvt<E>::fp8(d1, false),
                       d = BqCvt<E>::fp8(d1, true);
  return (typename E::v8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// 8 e2m1 nibbles (one dword, K ascending with the address, low nibble first) -> 8 scaled values of E's type
template <typename E>
__device__ __forceinline__ typename E::v8 bq_widen4(uint32_t d, float scale) {
  const typename E::v2 a = BqCvt<E>::template fp4<0>(d, scale), b = BqCvt<E>::template fp4<1>(d, scale),
                       c = BqCvt<E>::template fp4<2>(d, scale), e = BqCvt<E>::template fp4<3>(d, scale);
  return (typename E::v8){a[0], a[1], b[0], b[1], c[0], c[1], e[0], e[1]};
}

// S_al > 0: aligned ranges (workgroup i = slab i / S_al, slice i % S_al of its K walk); 0: stream-K
template <typename E, int FMT, bool PAIR, int MT>
__global__ void __launch_bounds__(BQ_WAVES * 64, 1)
bq_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const uint8_t* __restrict__ e_img,
               float* __restrict__ part, int M, int N, int K, int S, int S_al, const float* __restrict__ row_scale,
               const float* __restrict__ col_scale) {
  using v8 = typename E::v8;
  constexpr int NST = bq_nst(FMT, PAIR, MT);
  constexpr int XP = PAIR ? 2 : 1, NT = MT * XP, XR = NT * 32;   // x tiles of 32 rows (PAIR: plane 0's MT, then plane 1's)
  constexpr int XB = XR * 128;                                    // the x image: XR rows x 128 B
  constexpr int WRB = bq_wrow_bytes(FMT), WB = BQ_BN * WRB;       // the weight image: 256 rows x WRB bytes
  constexpr int WPR = WRB / 16, WRI = 64 / WPR;                   // 16-byte pieces of a weight row / weight rows per DMA
  constexpr int STAGE = bq_stage_bytes(FMT, PAIR, MT);            // one step: [x | w | e: 256 x 8 B (fp4)]
  constexpr int XI = XB / 1024, NI = (XB + WB) / 1024;            // 16-byte DMA instructions (1 KB each): x / x and w
  constexpr int PER = NI / BQ_WAVES, REM = NI % BQ_WAVES;         // per wave (the first REM waves: one more)
  constexpr int EX = FMT == 4 ? 1 : 0;                            // + its rows' exponents
  static_assert(NST >= 2 && NST * STAGE <= BQ_LDS_MAX, "LDS of a CU");
  static_assert(XR % 16 == 0 && XB % 1024 == 0 && WB % 1024 == 0, "operand-local swizzle, whole DMA instructions");
  static_assert((NST - 1) * (PER + 1 + EX) <= 63, "vmcnt field");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t smem_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int nk = K / BQ_BK, NB = (N + BQ_BN - 1) / BQ_BN;
  const int64_t T = (int64_t)NB * nk;
  const int G = gridDim.x;
  const psg_sk_span span = psg_sk_range(nk, T, G, S_al);
  const int64_t g0 = span.g0, g1 = span.g1;
  if (g0 >= g1) return;

  const int my_cnt = PER + (wid < REM ? 1 : 0);
  const int64_t Kw = FMT == 8 ? (int64_t)K : (int64_t)(K >> 1);   // bytes of a weight row
  // instruction idx of a step: 1 KB idx of the step's [x | w] image; a wave issues idx = wid, wid + 8, ...
  auto stage_one = [&](int slab, int ks, unsigned char* sb, int idx) {
    if (idx < XI) {                                          // 8 x rows x 8 pieces
      const int r = idx * 8 + (lane >> 3);
      const int piece = (lane & 7) ^ ((r >> 1) & 7);         // (tile bases are multiples of 32 rows: the row's own swizzle)
      const int plane = r / (MT * 32), xr = r - plane * (MT * 32);
      const int64_t gr = (int64_t)plane * M + (xr < M ? xr : M - 1);   // (rows past M: a copy of the last row, never stored)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(x + gr * K + ks * BQ_BK + piece * 8),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 0);
    } else {                                                 // WRI weight rows x WPR pieces
      const int r = (idx - XI) * WRI + lane / WPR;
      const int piece = (lane % WPR) ^ (FMT == 8 ? (r >> 2) & 3 : (r >> 3) & 1);
      int gr = slab * BQ_BN + r;
      gr = gr < N ? gr : N - 1;
      __builtin_amdgcn_global_load_lds(                      // a weight byte is read once by one CU: non-temporal
          (const __attribute__((address_space(1))) void*)(w + (int64_t)gr * Kw + ks * WRB + piece * 16),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 2);
    }
  };
  // the exponents of this wave's 32 rows: lane -> dword lane & 1 of row lane >> 1 of unit ks / 4, LDS = its slot + 4 lane
  auto stage_exp = [&](int slab, int ks, unsigned char* sb) {
    int gr = slab * BQ_BN + wid * 32 + (lane >> 1);
    gr = gr < N ? gr : N - 1;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(e_img + ((int64_t)(ks >> 2) * N + gr) * 8 + (lane & 1) * 4),
        (__attribute__((address_space(3))) void*)(sb + XB + WB + wid * 256), 4, 0, 0);
  };
  auto stage = [&](int slab, int ks, int buf) {              // this wave's DMAs of one step: my_cnt + EX instructions
    unsigned char* sb = smem + buf * STAGE;
#pragma unroll
    for (int q = 0; q <= PER; ++q)
      if (q < my_cnt) stage_one(slab, ks, sb, wid + BQ_WAVES * q);
    if (EX) stage_exp(slab, ks, sb);
  };

  const int l31 = lane & 31, hi = lane >> 5;
  const uint32_t aswz = (uint32_t)((l31 >> 1) & 7);          // (tile bases are multiples of 32 rows)
  const uint32_t wr = (uint32_t)(wid * 32 + l31);            // this lane's weight row of the slab
  const uint32_t brow = (uint32_t)XB + wr * WRB;
  const uint32_t bswz = FMT == 8 ? (wr >> 2) & 3 : (wr >> 3) & 1;
  const uint32_t erow = (uint32_t)(XB + WB) + wr * 8 + hi * 4;

  union Frag {
    psg_u32x4 u;
    v8 v;
  };
  psg_f32x16 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = (psg_f32x16){0};

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
  bool after_flush = false;
  int buf = 0;
  for (int64_t u = g0; u < g1; ++u) {
    // step u landed?  loads complete in order: the younger steps' loads may stay outstanding
    const int ahead = issued - 1;                            // younger steps in flight (<= NST - 2)
    if (after_flush) psg_vmwait<0>();                         // (stores of a flush may complete out of order with loads)
    else if (wid < REM) PsgDmaWait<PER + 1 + EX, NST - 1>::go(ahead);
    else PsgDmaWait<PER + EX, NST - 1>::go(ahead);
    after_flush = false;
    psg_lds_barrier();                                        // step u is in LDS; nobody reads the buffer of step u - 1 any more
    --issued;
    const bool pf = u + (NST - 1) < g1;
    int nb_ = buf + (NST - 1);
    nb_ = nb_ >= NST ? nb_ - NST : nb_;
    const uint32_t base = smem_lds + (uint32_t)(buf * STAGE);

    // x pieces (8 K each) a lane multiplies, in MFMA order, and the weight values against them:
    //   fp8: weight piece p = 2 s + hi (K 16 p .. + 15), s = 0, 1: its low 8 against x piece 2 p, its high 8 against 2 p + 1
    //   fp4: weight piece hi (K 32 hi .. + 31 = one MX block): dword j against x piece 4 hi + j
    Frag af[2][4];
    psg_u32x4 bq0, bq1 = (psg_u32x4){0};
    uint32_t ev = 0;
    auto read_x = [&](int t, Frag (&a_)[4]) {
      const uint32_t xrow = base + (uint32_t)((t * 32 + l31) * 128);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t c = FMT == 8 ? (uint32_t)(2 * (2 * (j >> 1) + hi) + (j & 1)) : (uint32_t)(4 * hi + j);
        a_[j].u = psg_lds_read128(xrow + ((c ^ aswz) << 4));
      }
    };
    if (FMT == 8) {
      bq0 = psg_lds_read128(base + brow + ((((uint32_t)hi) ^ bswz) << 4));
      bq1 = psg_lds_read128(base + brow + ((((uint32_t)(2 + hi)) ^ bswz) << 4));
    } else {
      bq0 = psg_lds_read128(base + brow + ((((uint32_t)hi) ^ bswz) << 4));
      ev = psg_lds_read32(base + erow);
    }
    read_x(0, af[0]);
    if (pf) {
      stage(pslab, pks, nb_);
      psg_sk_advance(pslab, pks, nk);
      ++issued;
    }
    psg_lgkmwait<4>();
    __builtin_amdgcn_sched_barrier(0);
    v8 b[4];
    if (FMT == 8) {
      b[0] = bq_widen8<E>(bq0[0], bq0[1]);
      b[1] = bq_widen8<E>(bq0[2], bq0[3]);
      b[2] = bq_widen8<E>(bq1[0], bq1[1]);
      b[3] = bq_widen8<E>(bq1[2], bq1[3]);
    } else {
      const float sc = __uint_as_float(((ev >> (8 * (ks & 3))) & 0xffu) << 23);   // 2^(e - 127)
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = bq_widen4<E>(bq0[j], sc);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t + 1 < NT) {
        read_x(t + 1, af[(t + 1) & 1]);
        psg_lgkmwait<4>();
      } else {
        psg_lgkmwait<0>();
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t % MT] = E::mfma32(af[t & 1][j].v, b[j], acc[t % MT]);   // D[m][n]
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);

    const bool slab_end = ks == nk - 1;
    if (slab_end || u == g1 - 1) {                           // the segment ends: one fp32 slice
      const int slot = psg_sk_slot(slab, nk, T, G, S_al);
      const int nslots = (slab_end && S_al == 0) ? S : slot + 1;   // ending a slab (stream-K): zero the slots it did not use
      // D[m][n]: register r of a lane = row 8 (r >> 2) + 4 hi + (r & 3) of the tile, column lane & 31
      const int n0 = slab * BQ_BN + wid * 32;
      if (n0 + l31 < N) {
        const float cs = col_scale[n0 + l31];
        float* ps = part + (int64_t)slot * M * N + n0 + l31;
        // the lane's element offset walks down its rows: one register, not one scalar row pointer per store.  Both asm
        // statements keep the 16 MT offsets and row masks - invariants of the step loop - from being hoisted out of it
        // and held in registers across the matrix instructions
        int off = 4 * hi * N, Mf = M;
        asm volatile("" : "+v"(off), "+s"(Mf));
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m_ = i * 32 + 8 * (r >> 2) + (r & 3) + 4 * hi;
            if (m_ < Mf) ps[off] = PAIR ? acc[i][r] * (row_scale[m_] * cs) : acc[i][r] * cs;
            off += (r & 3) == 3 ? 5 * N : N;                 // rows 8 g + 4 hi + 0..3, then the next group of 8
          }
        }
        for (int s_ = slot + 1; s_ < nslots; ++s_) {         // the slots this slab did not use: this lane's column, every
          float* pz = part + (int64_t)s_ * M * N + n0 + l31; // second row
          for (int m_ = hi; m_ < M; m_ += 2) pz[(int64_t)m_ * N] = 0.f;
        }
      }
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i] = (psg_f32x16){0};
      after_flush = true;
    }
    psg_sk_advance(slab, ks, nk);
    buf = buf + 1 == NST ? 0 : buf + 1;
  }
}

// ---- host side: plan and launch --------------------------------------------------------------------------------------
// psg_sk_make_plan's estimate with this step's cost: L2 -> LDS staging at ~40 B/clk/CU, its matrix instructions at 32 clk
// on two waves per SIMD, or its share of the HBM stream.  mode 1: ranges aligned to the slabs, 2: stream-K, 0: the cheaper
// estimate.  Made for 160 rows whatever M is: a row's k ranges must not follow the row count.
static psg_sk_plan bq_make_plan(const psg_ctx* ctx, int N, int K, int fmt, int forced_mode, bool pair) {
  const int G = ctx->num_cu < 1024 ? ctx->num_cu : 1024;
  const int nk = K / BQ_BK, NB = (N + BQ_BN - 1) / BQ_BN;
  const int stage = bq_stage_bytes(fmt, pair, 5);
  const double mfma_us = 5.0 * (pair ? 2 : 1) * 4 * 2 * 32 / 2.4e3;
  const double unit_us = fmax(fmax((double)stage / (40.0 * 2.4e3), mfma_us), (double)BQ_BN * bq_wrow_bytes(fmt) * G / 5.8e6);
  return psg_sk_make_plan(G, NB, nk, N, unit_us, 160, forced_mode);
}

static int bq_plan_checked(const char* name, psg_ctx* ctx, int M, int N, int K, int fmt, int mode, bool pair, psg_sk_plan* p,
                           int* slots) {
  const int kq = fmt == 8 ? 128 : 256;                       // the 32-row families' K granule: the images they already use
  const int rc = psg_sk_check_args(name, ctx, slots, M, 33, 160, N, K, kq, mode);
  if (rc != PSG_OK) return rc;
  *p = bq_make_plan(ctx, N, K, fmt, mode, pair);
  return psg_sk_plan_ok(name, *p, N, K, mode, slots);
}

template <typename E, int FMT, bool PAIR, int MT>
static int bq_launch_mt(const char* name, const psg_sk_plan& p, const void* x, const void* wq, const void* e_img, float* part, int M,
                        int N, int K, const float* row_scale, const float* col_scale, void* stream) {
  constexpr int LDS = bq_nst(FMT, PAIR, MT) * bq_stage_bytes(FMT, PAIR, MT);
  return psg_sk_launch(name, bq_gemm_kernel<E, FMT, PAIR, MT>, p.grid, LDS, stream, x, wq, e_img, part, M, N, K, p.slots, p.s_al,
                       row_scale, col_scale);
}

// M picks the x tiles that are staged and multiplied (2 / 3 / 5), nothing else
template <typename E, int FMT, bool PAIR>
static int bq_launch(const char* name, const psg_sk_plan& p, const void* x, const void* wq, const void* e_img, float* part, int M,
                     int N, int K, const float* row_scale, const float* col_scale, void* stream) {
  if (M <= 64) return bq_launch_mt<E, FMT, PAIR, 2>(name, p, x, wq, e_img, part, M, N, K, row_scale, col_scale, stream);
  if (M <= 96) return bq_launch_mt<E, FMT, PAIR, 3>(name, p, x, wq, e_img, part, M, N, K, row_scale, col_scale, stream);
  return bq_launch_mt<E, FMT, PAIR, 5>(name, p, x, wq, e_img, part, M, N, K, row_scale, col_scale, stream);
}

template <int FMT>
static int bq_single(const char* name, psg_ctx* ctx, const void* x, const void* wq, const void* e_img, const float* col_scale,
                     float* part, int M, int N, int K, int slots, int dtype, int mode, void* stream) {
  PSG_REQUIRE(ctx && x && wq && (FMT == 8 || e_img) && col_scale && part, PSG_ERR_INVALID, "%s: NULL argument", name);
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "%s: dtype %d (bf16 / fp16)", name, dtype);
  psg_sk_plan p;
  int want = 0;
  int rc = bq_plan_checked(name, ctx, M, N, K, FMT, mode, false, &p, &want);
  if (rc == PSG_OK) rc = psg_sk_check_slots(name, slots, want, N, K);
  if (rc != PSG_OK) return rc;
  PSG_DISPATCH_E16(dtype, name,
                   return (bq_launch<E, FMT, false>(name, p, x, wq, e_img, part, M, N, K, nullptr, col_scale, stream)));
  return PSG_ERR_INVALID;
}

template <int FMT>
static int bq_pair(const char* name, psg_ctx* ctx, const void* x2, const float* inv_scale, const void* wq, const void* e_img,
                   const float* col_scale, float* part, int M, int N, int K, int slots, int mode, void* stream) {
  PSG_REQUIRE(ctx && x2 && inv_scale && wq && (FMT == 8 || e_img) && col_scale && part, PSG_ERR_INVALID, "%s: NULL argument", name);
  psg_sk_plan p;
  int want = 0;
  int rc = bq_plan_checked(name, ctx, M, N, K, FMT, mode, true, &p, &want);
  if (rc == PSG_OK) rc = psg_sk_check_slots(name, slots, want, N, K);
  if (rc != PSG_OK) return rc;
  return bq_launch<EF16, FMT, true>(name, p, x2, wq, e_img, part, M, N, K, inv_scale, col_scale, stream);
}

extern "C" int psg_batch_gemm_w8_plan(psg_ctx* ctx, int M, int N, int K, int dtype, int mode, int* slots) {
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "psg_batch_gemm_w8_plan: dtype %d (bf16 / fp16)", dtype);
  psg_sk_plan p;
  return bq_plan_checked("psg_batch_gemm_w8_plan", ctx, M, N, K, 8, mode, false, &p, slots);
}
extern "C" int psg_batch_gemm_w8(psg_ctx* ctx, const void* x, const void* w8, const float* col_scale, float* part, int M, int N,
                                 int K, int slots, int dtype, int mode, void* stream) {
  return bq_single<8>("psg_batch_gemm_w8", ctx, x, w8, nullptr, col_scale, part, M, N, K, slots, dtype, mode, stream);
}
extern "C" int psg_batch_split_gemm_w8_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  psg_sk_plan p;
  return bq_plan_checked("psg_batch_split_gemm_w8_plan", ctx, M, N, K, 8, mode, true, &p, slots);
}
extern "C" int psg_batch_split_gemm_w8(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w8,
                                       const float* col_scale, float* part, int M, int N, int K, int slots, int mode,
                                       void* stream) {
  return bq_pair<8>("psg_batch_split_gemm_w8", ctx, x2, inv_scale, w8, nullptr, col_scale, part, M, N, K, slots, mode, stream);
}
extern "C" int psg_batch_gemm_w4_plan(psg_ctx* ctx, int M, int N, int K, int dtype, int mode, int* slots) {
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "psg_batch_gemm_w4_plan: dtype %d (bf16 / fp16)", dtype);
  psg_sk_plan p;
  return bq_plan_checked("psg_batch_gemm_w4_plan", ctx, M, N, K, 4, mode, false, &p, slots);
}
extern "C" int psg_batch_gemm_w4(psg_ctx* ctx, const void* x, const void* w4, const void* e_img, const float* col_scale,
                                 float* part, int M, int N, int K, int slots, int dtype, int mode, void* stream) {
  return bq_single<4>("psg_batch_gemm_w4", ctx, x, w4, e_img, col_scale, part, M, N, K, slots, dtype, mode, stream);
}
extern "C" int psg_batch_split_gemm_w4_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  psg_sk_plan p;
  return bq_plan_checked("psg_batch_split_gemm_w4_plan", ctx, M, N, K, 4, mode, true, &p, slots);
}
extern "C" int psg_batch_split_gemm_w4(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w4, const void* e_img,
                                       const float* col_scale, float* part, int M, int N, int K, int slots, int mode,
                                       void* stream) {
  return bq_pair<4>("psg_batch_split_gemm_w4", ctx, x2, inv_scale, w4, e_img, col_scale, part, M, N, K, slots, mode, stream);
}
