// Decode-step projections over FP8-quantised weights: part[s][m][n] = split-K slices of x[M][K] . W'[N][K]^T,
// M <= 32 rows, where the model's weight is W'[n][k] = e4m3(q[n][k]) * col_scale[n] (openpsg_amd/weights.py,
// quantize_fp8_rows).  q streams from HBM as ONE byte per weight, is widened to the x operand's 16-bit type in registers
// (v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1.0: e4m3 is a subset of both, the widening is exact) and multiplied on
// the 16-bit matrix cores with fp32 accumulation; col_scale is applied once, in fp32, where a slice is stored.
//   PAIR   (psg_split_gemm_w8, fp32s mode): x is the two fp16 planes [2][M][K] + inv_scale[M] of psg_split_f16x2 /
//          psg_rmsnorm_split2: part = (xh . q + xl . q) inv_scale[m] col_scale[n] - psg_split_gemm_w16's arithmetic over
//          a weight that has a scale;
//   single (psg_skinny_gemm_w8, bf16 / fp16 / mixed): x is [M][K] bf16 or fp16: part = (x . q) col_scale[n].
// The kernel is psg_gemm_q32.h's - the pair form of psg_batch_gemm.hip's (stream-K or slab-aligned ranges of (slab, K step)
// units dealt to one workgroup per CU, LDS-DMA into a 3-unit ring with counted vmcnt, 8 waves x one 32-row weight tile,
// k-ordered slices without atomics) - with a K step of 128; this file holds the format: the widening and the sub-step.
//   * a unit is 256 weight rows x 128 K.  An fp8 row of it is 128 bytes - the row length the 2-byte kernel stages per
//     K step of 64 - so the weight image keeps that kernel's 16-byte pieces, its XOR swizzle on the source address and
//     its conflict-free ds_read_b128: ONE read per lane and 32 K (16 fp8) where the 2-byte kernel needs two;
//   * x is staged as two [rows][128 B] images per unit (K halves), each exactly the 2-byte kernel's x image;
//   * the matrix instruction sums over 16 K and does not care WHICH 16 as long as both operands agree: the lane that
//     holds weight piece p (K 16p .. 16p + 15 of the unit) feeds its low 8 values to one v_mfma_f32_32x32x16 and its high
//     8 to the next, against x pieces 2p and 2p + 1 of the same lane half.  No byte shuffling, 8 conversions per read.
// A row's result does not depend on the other rows (nor on M: the plan is made for 32 rows whatever M is).
#include "psg_gemm_q32.h"

template <typename E>
struct W8Cvt;
template <>
struct W8Cvt<EF16> {
  static __device__ __forceinline__ EF16::v2 go(uint32_t v, bool hi) {
    return hi ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, false);
  }
};
template <>
struct W8Cvt<EBf16> {
  static __device__ __forceinline__ EBf16::v2 go(uint32_t v, bool hi) {
    return hi ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, false);
  }
};
// 8 e4m3 bytes (two dwords, K ascending with the address) -> 8 values of E's type
template <typename E>
__device__ __forceinline__ typename E::v8 w8_widen(uint32_t d0, uint32_t d1) {
  const typename E::v2 a = W8Cvt<E>::go(d0, false), b = W8Cvt<E>::go(d0, true), c = W8Cvt<E>::go(d1, false),
                       d = W8Cvt<E>::go(d1, true);
  return (typename E::v8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// the format of psg_gemm_q32.h's kernel
struct W8Fmt {
  static constexpr int BK = 128, SIDE = 0, SIDE_HI = 0;      // two x images per unit (K halves), no side image
  static constexpr bool COL_SCALE = true;
  static constexpr const char* ALIGNED = "x and w8";
  __host__ __device__ static constexpr int nst(bool) { return 3; }
  template <typename E, int XT>
  struct Acc {
    psg_f32x16 acc[XT];
    __device__ __forceinline__ void zero() {
#pragma unroll
      for (int i = 0; i < XT; ++i) acc[i] = (psg_f32x16){0};
    }
    __device__ __forceinline__ void unit(uint32_t) {}
    // weight piece p (K 16 p .. + 15 of the unit): its low 8 values against x piece 2 p, its high 8 against 2 p + 1
    __device__ __forceinline__ void step(int, PsgQ32Frag<E> (&a_)[XT][2], psg_u32x4& b_) {
      const typename E::v8 b0 = w8_widen<E>(b_[0], b_[1]), b1 = w8_widen<E>(b_[2], b_[3]);
#pragma unroll
      for (int i = 0; i < XT; ++i) acc[i] = E::mfma32(a_[i][0].v, b0, acc[i]);          // D[m][n]
#pragma unroll
      for (int i = 0; i < XT; ++i) acc[i] = E::mfma32(a_[i][1].v, b1, acc[i]);
    }
    __device__ __forceinline__ float out(int r) const { return XT == 2 ? acc[0][r] + acc[XT - 1][r] : acc[0][r]; }
  };
};

extern "C" int psg_split_gemm_w8_plan(psg_ctx* ctx, int M, int N, int K, int mode, int* slots) {
  psg_sk_plan p;
  return psg_q32_plan_checked<W8Fmt>("psg_split_gemm_w8_plan", ctx, M, N, K, mode, true, &p, slots);
}

extern "C" int psg_split_gemm_w8(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* w8, const float* col_scale,
                                 float* part, int M, int N, int K, int slots, int mode, void* stream) {
  PSG_REQUIRE(ctx && x2 && inv_scale && w8 && col_scale && part, PSG_ERR_INVALID, "psg_split_gemm_w8: NULL argument");
  return psg_q32_run<W8Fmt, true>("psg_split_gemm_w8", ctx, x2, w8, nullptr, inv_scale, col_scale, part, M, N, K, slots, PSG_F16,
                                  mode, stream);
}

extern "C" int psg_skinny_gemm_w8_plan(psg_ctx* ctx, int M, int N, int K, int dtype, int mode, int* slots) {
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "psg_skinny_gemm_w8_plan: dtype %d (bf16 / fp16)", dtype);
  psg_sk_plan p;
  return psg_q32_plan_checked<W8Fmt>("psg_skinny_gemm_w8_plan", ctx, M, N, K, mode, false, &p, slots);
}

extern "C" int psg_skinny_gemm_w8(psg_ctx* ctx, const void* x, const void* w8, const float* col_scale, float* part, int M, int N,
                                  int K, int slots, int dtype, int mode, void* stream) {
  PSG_REQUIRE(ctx && x && w8 && col_scale && part, PSG_ERR_INVALID, "psg_skinny_gemm_w8: NULL argument");
  return psg_q32_run<W8Fmt, false>("psg_skinny_gemm_w8", ctx, x, w8, nullptr, nullptr, col_scale, part, M, N, K, slots, dtype, mode,
                                   stream);
}
