// Decode-step projections over MXFP4-quantised weights: part[s][m][n] = split-K slices of x[M][K] . W'[N][K]^T,
// M <= 32 rows, where the model's weight is W'[n][k] = e2m1(q[n][k]) * 2^(e[n][k / 32] - 127) * col_scale[n]
// (openpsg_amd/weights.py, quantize_mxfp4_rows).  q streams from HBM as HALF a byte per weight plus one exponent byte per
// 32, is widened to the x operand's 16-bit type in registers (v_cvt_scalef32_pk_{f16,bf16}_fp4 with the block's
// 2^(e - 127) as the instruction's scale: exact, and a normal fp16 number or zero for e >= 114) and multiplied on the
// 16-bit matrix cores with fp32 accumulation; col_scale is applied once, in fp32, where a slice is stored.
//   PAIR   (psg_split_gemm_w4, fp32s mode): x is the two fp16 planes [2][M][K] + inv_scale[M] of psg_split_f16x2 /
//          psg_rmsnorm_split2: part = (xh . w + xl . w) inv_scale[m] col_scale[n] with w = e2m1(q) 2^(e - 127);
//   single (psg_skinny_gemm_w4, bf16 / fp16 / mixed): x is [M][K] bf16 or fp16: part = (x . w) col_scale[n].
// The kernel is psg_gemm_q32.h's - the one psg_gemm_w8.hip runs - with a K step of 256 and the block exponents as its side
// image; this file holds the format: the widening and the sub-step.
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
#include "psg_gemm_q32.h"

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

// the format of psg_gemm_q32.h's kernel
struct W4Fmt {
  static constexpr int BK = 256, SIDE = 8, SIDE_HI = 4;      // four x images per unit (K quarters); e_img: 2 x 4 exponents per row
  static constexpr bool COL_SCALE = true;
  static constexpr const char* ALIGNED = "x, w4 and e_img";
  __host__ __device__ static constexpr int nst(bool pair) { return pair ? 2 : 3; }   // 132 KB / 150 KB
  template <typename E, int XT>
  struct Acc {
    psg_f32x16 acc[XT];
    uint32_t ev;                                             // this lane's four block exponents: byte s2 = sub-step s2's
    __device__ __forceinline__ void zero() {
#pragma unroll
      for (int i = 0; i < XT; ++i) acc[i] = (psg_f32x16){0};
    }
    __device__ __forceinline__ void unit(uint32_t a) { ev = psg_lds_read32(a); }
    // weight piece p (K 32 p .. + 31 of the unit = one MX block): dword j against x piece 4 p + j, one scale
    __device__ __forceinline__ void step(int s2, PsgQ32Frag<E> (&a_)[XT][4], psg_u32x4& b_) {
      const float sc = __uint_as_float(((ev >> (8 * s2)) & 0xffu) << 23);   // 2^(e - 127)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const typename E::v8 b = w4_widen<E>(b_[j], sc);
#pragma unroll
        for (int i = 0; i < XT; ++i) acc[i] = E::mfma32(a_[i][j].v, b, acc[i]);         // D[m][n]
      }
    }
    __device__ __forceinline__ float out(int r) const { return XT == 2 ? acc[0][r] + acc[XT - 1][r] : acc[0][r]; }
  };
};

extern "C" int psg_split_gemm_w4_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  psg_sk_plan p;
  return psg_q32_plan_checked<W4Fmt>("psg_split_gemm_w4_plan", ctx, M, N, K, mode, true, &p, slots);
}

extern "C" int psg_split_gemm_w4(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w4, const void* e_img,
                                 const float* col_scale, float* part, int M, int N, int K, int slots, int mode, void* stream) {
  PSG_REQUIRE(ctx && x2 && inv_scale && w4 && e_img && col_scale && part, PSG_ERR_INVALID, "psg_split_gemm_w4: NULL argument");
  return psg_q32_run<W4Fmt, true>("psg_split_gemm_w4", ctx, x2, w4, e_img, inv_scale, col_scale, part, M, N, K, slots, PSG_F16,
                                  mode, stream);
}

extern "C" int psg_skinny_gemm_w4_plan(psg_ctx* ctx, int M, int N, int K, int dtype, int mode, int* slots) {
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "psg_skinny_gemm_w4_plan: dtype %d (bf16 / fp16)", dtype);
  psg_sk_plan p;
  return psg_q32_plan_checked<W4Fmt>("psg_skinny_gemm_w4_plan", ctx, M, N, K, mode, false, &p, slots);
}

extern "C" int psg_skinny_gemm_w4(psg_ctx* ctx, const void* x, const void* w4, const void* e_img, const float* col_scale,
                                  float* part, int M, int N, int K, int slots, int dtype, int mode, void* stream) {
  PSG_REQUIRE(ctx && x && w4 && e_img && col_scale && part, PSG_ERR_INVALID, "psg_skinny_gemm_w4: NULL argument");
  return psg_q32_run<W4Fmt, false>("psg_skinny_gemm_w4", ctx, x, w4, e_img, nullptr, col_scale, part, M, N, K, slots, dtype, mode,
                                   stream);
}
