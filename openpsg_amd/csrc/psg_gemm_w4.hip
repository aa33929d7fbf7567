// Decode-step projections over MXFP4-quantised weights: part[s][m][n] = split-K slices of x[M][K] . W'[N][K]^T,
// M <= 32 rows, where the model's weight is W'[n][k] = e2m1(q[n][k]) * 2^(e[n][k / 32] - 127) * col_scale[n]
// (openpsg_amd/weights.py, quantize_mxfp4_rows).  q streams from HBM as HALF a byte per weight plus one exponent byte per
// 32, is widened to the x operand's 16-bit type in registers (v_cvt_scalef32_pk_{f16,bf16}_fp4 with the block's
// 2^(e - 127) as the instruction's scale: exact, and a normal fp16 number or zero for e >= 114) and multiplied on the
// 16-bit matrix cores with fp32 accumulation; col_scale is applied once, in fp32, where a slice is stored.
//   PAIR   (psg_split_gemm_w4, fp32s mode): x is the two fp16 planes [2][M][K] + inv_scale[M] of psg_split_f16x2 /
//          psg_rmsnorm_split2: part = (xh . w + xl . w) inv_scale[m] col_scale[n] with w = e2m1(q) 2^(e - 127);
//   single (psg_skinny_gemm_w4, bf16 / fp16 / mixed): x is [M][K] bf16 or fp16: part = (x . w) col_scale[n].
// The kernel is psg_gemm_w8.hip's with the K step widened to 256:
//   * a unit is 256 weight rows x 256 K.  An fp4 row of it is 128 bytes - the row psg_gemm_w8.hip and the 2-byte kernel
//     stage - so the weight image keeps their 16-byte pieces, the XOR swizzle on the source address and the conflict-free
//     ds_read_b128.  ONE read per lane is 32 nibbles = one MX block: one scale per read;
//   * x is staged as four [rows][128 B] images per unit (K quarters), each exactly the 2-byte kernel's x image.  The x
//     image of a unit is now as large as the weight's (PAIR: 32 KB + 32 KB), so the PAIR form runs a ring of two units
//     (132 KB) where the single form keeps three (150 KB);
//   * the lane that holds weight piece p (K 32p .. 32p + 31 of the unit) feeds its four dwords to four
//     v_mfma_f32_32x32x16 against x pieces 4p .. 4p + 3 of the same lane half.  No shuffling, 16 conversions per read;
//   * the block exponents arrive by LDS-DMA too (no global_load beside the ring, which would drain it): the caller passes
//     them re-laid-out as e_img[K / 256][N][2][4] (ops.mxfp4_exp_image), byte [h][j] = the exponent of block 2 j + h of
//     the row's 8 blocks in the unit.  A wave's 32 rows of a unit are then 256 contiguous bytes - one 4-byte DMA per wave
//     and unit, into the wave's own 256 bytes of the stage - and a lane's four scales are ONE ds_read_b32.
// A row's result does not depend on the other rows (nor on M: the plan is made for 32 rows whatever M is).
#include "psg_common.h"
#include "psg_wave.h"

#define W4_BK 256
#define W4_BN 256
#define W4_WAVES 8

__host__ __device__ static inline int w4_owner(int64_t u, int64_t T, int G) { return (int)(((u + 1) * G - 1) / T); }
__host__ __device__ constexpr int w4_nst(bool pair) { return pair ? 2 : 3; }
__host__ __device__ constexpr int w4_stage_bytes(bool pair) { return (pair ? 64 : 32) * 512 + W4_BN * 128 + W4_BN * 8; }

// byte SEL of v = two e2m1 nibbles -> two values of E's type, times `scale` (a power of two: only its exponent is used).
// Element 0 is the LOW nibble (the even k of the storage order); tests/test_gpu_gemm_w4.py pins it
template <typename E>
struct W4Cvt;
template <>
struct W4Cvt<EF16> {
  template <int SEL>
  static __device__ __forceinline__ EF16::v2 go(uint32_t v, float scale) {
    return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, scale, SEL);
  }
};
template <>
struct W4Cvt<EBf16> {
  template <int SEL>
  static __device__ __forceinline__ EBf16::v2 go(uint32_t v, float scale) {
    return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, SEL);
  }
};
// 8 e2m1 nibbles (one dword, K ascending with the address, low nibble first) -> 8 scaled values of E's type
template <typename E>
__device__ __forceinline__ typename E::v8 w4_widen(uint32_t d, float scale) {
  const typename E::v2 a = W4Cvt<E>::template go<0>(d, scale), b = W4Cvt<E>::template go<1>(d, scale),
                       c = W4Cvt<E>::template go<2>(d, scale), e = W4Cvt<E>::template go<3>(d, scale);
  return (typename E::v8){a[0], a[1], b[0], b[1], c[0], c[1], e[0], e[1]};
}

// S_al > 0: aligned ranges (workgroup i = slab i / S_al, slice i % S_al of its K walk); 0: stream-K
template <typename E, bool PAIR>
__global__ void __launch_bounds__(W4_WAVES * 64, 1)
w4_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const uint8_t* __restrict__ e_img,
               float* __restrict__ part, int M, int N, int K, int S, int S_al, const float* __restrict__ row_scale,
               const float* __restrict__ col_scale) {
  using v8 = typename E::v8;
  constexpr int NST = w4_nst(PAIR);
  constexpr int XT = PAIR ? 2 : 1, XR = XT * 32;             // x tiles of 32 rows (PAIR: plane 0, plane 1)
  constexpr int XQ = XR * 128, XB = 4 * XQ;                  // one K quarter of the x image / all four
  constexpr int WB = W4_BN * 128;                            // the weight image
  constexpr int STAGE = w4_stage_bytes(PAIR);                // one unit: [x: K quarters 0..3 | w: 256 rows x 128 B | e: 256 x 8 B]
  constexpr int XI = XB / 1024, NI = (XB + WB) / 1024;       // 16-byte DMA instructions (8 rows x 128 B each): x / x and w
  constexpr int PER = NI / W4_WAVES + 1;                     // per wave and unit: its share of x and w + its rows' exponents
  static_assert(STAGE == XB + WB + W4_BN * 8 && NST * STAGE <= 160 * 1024, "LDS of a CU");
  static_assert(NI % W4_WAVES == 0 && XR % 16 == 0, "uniform DMA counts, operand-local swizzle");
  static_assert(2 * PER <= 63, "vmcnt field");
  constexpr int NR = 1 + 4 * XT;                             // LDS reads of one sub-step
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t smem_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int nk = K / W4_BK, NB = (N + W4_BN - 1) / W4_BN;
  const int64_t T = (int64_t)NB * nk;
  const int G = gridDim.x;
  int64_t g0, g1;
  if (S_al > 0) {
    const int sb = blockIdx.x / S_al, sl = blockIdx.x - sb * S_al;
    g0 = (int64_t)sb * nk + (int64_t)sl * nk / S_al;
    g1 = (int64_t)sb * nk + (int64_t)(sl + 1) * nk / S_al;
  } else {
    g0 = (int64_t)blockIdx.x * T / G;
    g1 = ((int64_t)blockIdx.x + 1) * T / G;
  }
  if (g0 >= g1) return;

  const int srow = lane >> 3, sslot = lane & 7;
  const int Kb = K >> 1;                                     // bytes of a weight row
  // instruction idx of a unit: 128-byte rows 8 idx .. + 7 of the unit's image; a wave issues idx = wid, wid + 8, ...
  auto stage_one = [&](int slab, int kt, unsigned char* sb, int idx) {
    const int r = idx * 8 + srow;
    const int piece = sslot ^ ((r >> 1) & 7);                // (XR and XI * 8 are multiples of 16: the operand-local row's swizzle)
    if (idx < XI) {
      const int quarter = r / XR, xr = r - quarter * XR;
      int gr = xr < M ? xr : M - 1;
      if (PAIR) gr = (xr >> 5) * M + ((xr & 31) < M ? (xr & 31) : M - 1);   // plane xr >> 5, row xr & 31 of [2][M][K]
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(x + (int64_t)gr * K + kt * W4_BK + quarter * 64 + piece * 8),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 0);
    } else {
      int gr = slab * W4_BN + (r - XI * 8);
      gr = gr < N ? gr : N - 1;
      __builtin_amdgcn_global_load_lds(                      // a weight byte is read once by one CU: non-temporal
          (const __attribute__((address_space(1))) void*)(w + (int64_t)gr * Kb + kt * 128 + piece * 16),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 2);
    }
  };
  // the exponents of this wave's 32 rows of the unit: lane -> dword lane & 1 of row lane >> 1, LDS = its slot + 4 lane
  auto stage_exp = [&](int slab, int kt, unsigned char* sb) {
    int gr = slab * W4_BN + wid * 32 + (lane >> 1);
    gr = gr < N ? gr : N - 1;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(e_img + ((int64_t)kt * N + gr) * 8 + (lane & 1) * 4),
        (__attribute__((address_space(3))) void*)(sb + XB + WB + wid * 256), 4, 0, 2);
  };
  auto stage = [&](int slab, int kt, int buf, int q0, int q1) {   // this wave's instructions q0 .. q1 - 1 of the unit
    unsigned char* sb = smem + buf * STAGE;
    for (int q = q0; q < q1; ++q) {
      if (q < PER - 1) stage_one(slab, kt, sb, wid + W4_WAVES * q);
      else if (q == PER - 1) stage_exp(slab, kt, sb);
    }
  };

  const int l31 = lane & 31, hi = lane >> 5;
  uint32_t arow[XT];
#pragma unroll
  for (int i = 0; i < XT; ++i) arow[i] = (uint32_t)((i * 32 + l31) * 128);
  const uint32_t aswz = (uint32_t)((l31 >> 1) & 7);          // (tile bases are multiples of 32 rows)
  const uint32_t brow = (uint32_t)(XB + (wid * 32 + l31) * 128), bswz = aswz;
  const uint32_t erow = (uint32_t)(XB + WB + (wid * 32 + l31) * 8 + hi * 4);

  union Frag {
    psg_u32x4 u;
    v8 v;
  };
  psg_f32x16 acc[XT];
#pragma unroll
  for (int i = 0; i < XT; ++i) acc[i] = (psg_f32x16){0};

  int slab = (int)(g0 / nk), kt = (int)(g0 - (int64_t)slab * nk);
  int pslab = slab, pkt = kt;                                // the unit the next DMA stage fetches
  auto advance = [&](int& s_, int& k_) {
    if (++k_ == nk) {
      k_ = 0;
      ++s_;
    }
  };
  int issued = 0;                                            // units in flight (prologue: NST - 1)
#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (g0 + p < g1) {
      stage(pslab, pkt, p, 0, PER);
      advance(pslab, pkt);
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
    Frag af[2][XT][4];
    psg_u32x4 bq[2];
    const uint32_t ev = psg_lds_read32(base + erow);          // this lane's four block exponents: byte s2 = sub-step s2's
    // sub-step s2: weight piece p = 2 s2 + hi (K 32 p .. + 31 of the unit), x pieces 4 p .. 4 p + 3 of the 512-byte row
    auto read_frags = [&](int s2, Frag (&a_)[XT][4], psg_u32x4& b_) {
      const uint32_t p = (uint32_t)(2 * s2 + hi);
      b_ = psg_lds_read128(base + brow + ((p ^ bswz) << 4));
      const uint32_t xq = base + (p >> 1) * XQ, x0 = 4 * (p & 1);
#pragma unroll
      for (int i = 0; i < XT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) a_[i][j].u = psg_lds_read128(xq + arow[i] + (((x0 + j) ^ aswz) << 4));
    };
    auto mma = [&](int s2, Frag (&a_)[XT][4], psg_u32x4& b_) {
      const float sc = __uint_as_float(((ev >> (8 * s2)) & 0xffu) << 23);   // 2^(e - 127)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const v8 b = w4_widen<E>(b_[j], sc);
#pragma unroll
        for (int i = 0; i < XT; ++i) acc[i] = E::mfma32(a_[i][j].v, b, acc[i]);         // D[m][n]
      }
    };
    read_frags(0, af[0], bq[0]);
    read_frags(1, af[1], bq[1]);
    if (pf) stage(pslab, pkt, nb_, 0, QH);
    psg_lgkmwait<NR>();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mma(0, af[0], bq[0]);
    __builtin_amdgcn_sched_barrier(0);
    read_frags(2, af[0], bq[0]);
    if (pf) stage(pslab, pkt, nb_, QH, PER);
    psg_lgkmwait<NR>();
    __builtin_amdgcn_sched_barrier(0);
    mma(1, af[1], bq[1]);
    __builtin_amdgcn_sched_barrier(0);
    read_frags(3, af[1], bq[1]);
    psg_lgkmwait<NR>();
    __builtin_amdgcn_sched_barrier(0);
    mma(2, af[0], bq[0]);
    psg_lgkmwait<0>();
    __builtin_amdgcn_sched_barrier(0);
    mma(3, af[1], bq[1]);
    __builtin_amdgcn_s_setprio(0);
    if (pf) {
      advance(pslab, pkt);
      ++issued;
    }

    const bool slab_end = kt == nk - 1;
    if (slab_end || u == g1 - 1) {                           // the segment ends: one fp32 slice
      int slot;
      if (S_al > 0) slot = (int)blockIdx.x % S_al;
      else slot = (int)blockIdx.x - w4_owner((int64_t)slab * nk, T, G);
      const int nslots = (slab_end && S_al == 0) ? S : slot + 1;   // ending a slab (stream-K): zero the slots it did not use
      // D[m][n]: register r of a lane = row 8 (r >> 2) + 4 hi + (r & 3) of the tile, column lane & 31
      const int n0 = slab * W4_BN + wid * 32;
      if (n0 + l31 < N) {
        const float cs = col_scale[n0 + l31];
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
              if (real) val = PAIR ? (acc[0][r] + acc[XT - 1][r]) * rs[r] : acc[0][r] * rs[r];
              rowp[lane_off] = val;
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < XT; ++i) acc[i] = (psg_f32x16){0};
      after_flush = true;
    }
    advance(slab, kt);
    buf = buf + 1 == NST ? 0 : buf + 1;
  }
}

// ---- host side: plan and launch --------------------------------------------------------------------------------------
struct w4_plan {
  int grid, slots, s_al;
};

static int w4_streamk_slots(int N, int K, int G) {
  const int nk = K / W4_BK, NB = (N + W4_BN - 1) / W4_BN;
  const int64_t T = (int64_t)NB * nk;
  int smax = 1;
  for (int b = 0; b < NB; ++b) {
    const int i0 = w4_owner((int64_t)b * nk, T, G), i1 = w4_owner((int64_t)(b + 1) * nk - 1, T, G);
    if (i1 - i0 + 1 > smax) smax = i1 - i0 + 1;
  }
  return smax;
}

// psg_gemm_w8.hip's estimate: the longest range's units x the unit's cost (L2 -> LDS staging at ~40 B/clk/CU, or the unit's
// share of the HBM stream) + the fp32 slices it leaves (written here, read by the consumer).  mode 1: ranges aligned to
// the slabs, 2: stream-K, 0: the cheaper estimate.  Made for 32 rows whatever M is: a row's k ranges must not follow
// the row count.
static w4_plan w4_make_plan(const psg_ctx* ctx, int N, int K, int forced_mode, bool pair) {
  w4_plan best{0, 0, 0};
  double best_t = 1e300;
  const int G = ctx->num_cu < 1024 ? ctx->num_cu : 1024;
  const int nk = K / W4_BK, NB = (N + W4_BN - 1) / W4_BN;
  const int64_t T = (int64_t)NB * nk;
  const int stage = w4_stage_bytes(pair);
  const double unit_us = fmax((double)stage / (40.0 * 2.4e3), (double)W4_BN * 136 * G / 5.8e6);
  for (int mode = 1; mode <= 2; ++mode) {
    if (forced_mode && forced_mode != mode) continue;
    w4_plan p{0, 0, 0};
    double units;
    if (mode == 1) {
      int s_al = G / NB;
      if (s_al < 1) continue;
      if (s_al > nk) s_al = nk;
      if (s_al > PSG_MAX_SPLITS) s_al = PSG_MAX_SPLITS;      // what a consumer kernel sums
      p.s_al = p.slots = s_al;
      p.grid = NB * s_al;
      units = (double)((nk + s_al - 1) / s_al);
    } else {
      p.grid = T < G ? (int)T : G;                           // every workgroup gets at least one unit: slot ranks are contiguous
      p.slots = w4_streamk_slots(N, K, p.grid);
      while (p.slots > PSG_MAX_SPLITS && p.grid > NB) {      // few slabs, long K walks: fewer workgroups = longer segments
        p.grid = p.grid * 7 / 8 > NB ? p.grid * 7 / 8 : NB;
        p.slots = w4_streamk_slots(N, K, p.grid);
      }
      if (p.slots > PSG_MAX_SPLITS) continue;
      units = (double)((T + p.grid - 1) / p.grid);
    }
    const double slice_bytes = (double)p.slots * 32 * N * 4;
    const double t = units * unit_us + slice_bytes / 3.5e6 + slice_bytes / 8e6 + (mode == 2 ? 3.0 : 0.0);
    if (t < best_t) {
      best_t = t;
      best = p;
    }
  }
  return best;
}

static int w4_plan_checked(const char* name, psg_ctx* ctx, int M, int N, int K, int mode, bool pair, w4_plan* p, int* slots) {
  PSG_REQUIRE(ctx && slots, PSG_ERR_INVALID, "%s: NULL argument", name);
  PSG_REQUIRE(M >= 1 && M <= 32 && N >= 16 && N % 16 == 0 && K >= W4_BK && K % W4_BK == 0 && mode >= 0 && mode <= 2,
              PSG_ERR_UNSUPPORTED, "%s: M=%d (1..32), N=%d (multiple of 16), K=%d (multiple of %d), mode=%d", name, M, N, K,
              W4_BK, mode);
  *p = w4_make_plan(ctx, N, K, mode, pair);
  PSG_REQUIRE(p->grid > 0 && p->slots <= PSG_MAX_SPLITS, PSG_ERR_UNSUPPORTED, "%s: no plan with <= %d slices for N=%d K=%d mode=%d",
              name, PSG_MAX_SPLITS, N, K, mode);
  *slots = p->slots;
  return PSG_OK;
}

template <typename E, bool PAIR>
static int w4_launch(const char* name, const w4_plan& p, const void* x, const void* w4, const void* e_img, float* part, int M,
                     int N, int K, const float* row_scale, const float* col_scale, void* stream) {
  constexpr int LDS = w4_nst(PAIR) * w4_stage_bytes(PAIR);
  auto k = w4_gemm_kernel<E, PAIR>;
  hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  if (e != hipSuccess) {
    psg_set_error("%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
    return PSG_ERR_HIP;
  }
  k<<<(unsigned)p.grid, W4_WAVES * 64, LDS, (hipStream_t)stream>>>((const uint16_t*)x, (const uint8_t*)w4, (const uint8_t*)e_img,
                                                                   part, M, N, K, p.slots, p.s_al, row_scale, col_scale);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

extern "C" int psg_split_gemm_w4_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  w4_plan p;
  return w4_plan_checked("psg_split_gemm_w4_plan", ctx, M, N, K, mode, true, &p, slots);
}

extern "C" int psg_split_gemm_w4(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w4, const void* e_img,
                                 const float* col_scale, float* part, int M, int N, int K, int slots, int mode, void* stream) {
  PSG_REQUIRE(ctx && x2 && inv_scale && w4 && e_img && col_scale && part, PSG_ERR_INVALID, "psg_split_gemm_w4: NULL argument");
  w4_plan p;
  int want = 0;
  const int rc = w4_plan_checked("psg_split_gemm_w4", ctx, M, N, K, mode, true, &p, &want);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(slots == want, PSG_ERR_INVALID, "psg_split_gemm_w4: slots=%d, the plan for N=%d K=%d writes %d", slots, N, K, want);
  return w4_launch<EF16, true>("psg_split_gemm_w4", p, x2, w4, e_img, part, M, N, K, inv_scale, col_scale, stream);
}

extern "C" int psg_skinny_gemm_w4_plan(psg_ctx* ctx, int M, int N, int K, int dtype, int mode, int* slots) {
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "psg_skinny_gemm_w4_plan: dtype %d (bf16 / fp16)", dtype);
  w4_plan p;
  return w4_plan_checked("psg_skinny_gemm_w4_plan", ctx, M, N, K, mode, false, &p, slots);
}

extern "C" int psg_skinny_gemm_w4(psg_ctx* ctx, const void* x, const void* w4, const void* e_img, const float* col_scale,
                                  float* part, int M, int N, int K, int slots, int dtype, int mode, void* stream) {
  PSG_REQUIRE(ctx && x && w4 && e_img && col_scale && part, PSG_ERR_INVALID, "psg_skinny_gemm_w4: NULL argument");
  w4_plan p;
  int want = 0;
  const int rc = w4_plan_checked("psg_skinny_gemm_w4", ctx, M, N, K, mode, false, &p, &want);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(slots == want, PSG_ERR_INVALID, "psg_skinny_gemm_w4: slots=%d, the plan for N=%d K=%d writes %d", slots, N, K, want);
  PSG_DISPATCH_E16(dtype, "psg_skinny_gemm_w4",
                   return (w4_launch<E, false>("psg_skinny_gemm_w4", p, x, w4, e_img, part, M, N, K, nullptr, col_scale, stream)));
  return PSG_ERR_INVALID;
}
