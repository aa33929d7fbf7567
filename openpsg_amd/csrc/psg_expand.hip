// Dense operands rebuilt from a quantised LLM matrix: the engine that keeps ONLY the bytes resident
// (llm_weight_resident='quantised') expands a matrix into a scratch buffer right before the one large-M product that reads it.
//   psg_expand_w8: q e4m3fn bytes [N][K]                      -> out[n][k] = e4m3(q)                       (s == NULL, fp16)
//   psg_expand_w4: q fp4 nibbles [N][K / 2], e uint8 [N][K / 32] -> out[n][k] = e2m1(q) 2^(e - 127)          (s == NULL, fp16)
//   with s fp32 [N]:  out[n][k] = round_to_out_dtype(float32(unscaled) * s[n])   - ONE fp32 multiply, ONE rounding to the
//   output type: weights.dequantize_fp8_rows / dequantize_mxfp4_rows bit for bit.  (A non-power-of-two s must NOT go into the
//   scale operand of a v_cvt_scalef32_* conversion straight to 16 bits: that rounds once where the model rounds twice.)
// A streaming kernel, no LDS, no matrix cores.  A lane takes one UNIT = 16 bytes of q (16 fp8 values, or exactly one
// 32-element MXFP4 block and its single exponent byte) with a non-temporal 16-byte load - the bytes are read once - widens it
// with the conversions of psg_gemm_w8.hip / psg_gemm_w4.hip (v_cvt_scalef32_pk_f16_fp8 at scale 1.0,
// v_cvt_scalef32_pk_f16_fp4 with the block's power of two: both exact in fp16, e >= 114 keeps the latter normal) and writes
// 16-byte ORDINARY stores: the consumer is the very next launch and should find the operand in the L2 / Infinity Cache.
// Units are dealt by a grid-stride loop over a grid sized from the device's CU count.
#include "psg_common.h"

#define XP_THREADS 256
#define XP_WG_PER_CU 8

typedef _Float16 xp_h2 __attribute__((ext_vector_type(2)));

// 16 bytes of q -> the unit's values as fp16, K ascending
template <int FMT>
struct XpUnit;
template <>
struct XpUnit<8> {
  static constexpr int VALS = 16;
  static __device__ __forceinline__ void widen(const psg_u32x4 d, float, _Float16 (&h)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const xp_h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d[i], 1.0f, false);
      const xp_h2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(d[i], 1.0f, true);
      h[4 * i] = a[0]; h[4 * i + 1] = a[1]; h[4 * i + 2] = b[0]; h[4 * i + 3] = b[1];
    }
  }
};
template <>
struct XpUnit<4> {
  static constexpr int VALS = 32;
  static __device__ __forceinline__ void widen(const psg_u32x4 d, float bs, _Float16 (&h)[32]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {                              // byte SEL of a dword: element 0 is the LOW nibble (the even k)
      const xp_h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d[i], bs, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d[i], bs, 1),
                  c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d[i], bs, 2), e = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(d[i], bs, 3);
      h[8 * i] = a[0]; h[8 * i + 1] = a[1]; h[8 * i + 2] = b[0]; h[8 * i + 3] = b[1];
      h[8 * i + 4] = c[0]; h[8 * i + 5] = c[1]; h[8 * i + 6] = e[0]; h[8 * i + 7] = e[1];
    }
  }
};

__device__ __forceinline__ uint32_t xp_pack(uint16_t lo, uint16_t hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }

// FMT 8 / 4; OUT = psg_dtype of the result; SCALED: multiply by s[row] in fp32 first (unscaled results are fp16 only)
template <int FMT, int OUT, bool SCALED>
__global__ void __launch_bounds__(XP_THREADS)
xp_expand_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ e, const float* __restrict__ s, void* __restrict__ out,
                 uint64_t units, uint32_t units_per_row) {
  constexpr int V = XpUnit<FMT>::VALS;
  const uint64_t stride = (uint64_t)gridDim.x * XP_THREADS;
  for (uint64_t u = (uint64_t)blockIdx.x * XP_THREADS + threadIdx.x; u < units; u += stride) {
    const psg_u32x4 d = __builtin_nontemporal_load(reinterpret_cast<const psg_u32x4*>(q) + u);
    float bs = 1.0f;
    if (FMT == 4) bs = __uint_as_float((uint32_t)__builtin_nontemporal_load(e + u) << 23);   // 2^(e - 127): one block per unit
    float sc = 1.0f;
    if (SCALED) {
      const uint64_t row = units <= 0xffffffffull ? (uint64_t)((uint32_t)u / units_per_row) : u / units_per_row;
      sc = s[row];
    }
    _Float16 h[V];
    XpUnit<FMT>::widen(d, bs, h);
    if (OUT == PSG_F32) {
      psg_f32x4* o = reinterpret_cast<psg_f32x4*>(out) + u * (V / 4);
#pragma unroll
      for (int i = 0; i < V / 4; ++i) {
        const psg_f32x4 v = {(float)h[4 * i] * sc, (float)h[4 * i + 1] * sc, (float)h[4 * i + 2] * sc, (float)h[4 * i + 3] * sc};
        o[i] = v;
      }
    } else {
      psg_u32x4* o = reinterpret_cast<psg_u32x4*>(out) + u * (V / 8);
#pragma unroll
      for (int i = 0; i < V / 8; ++i) {
        uint16_t r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (!SCALED) r[j] = __builtin_bit_cast(uint16_t, h[8 * i + j]);
          else if (OUT == PSG_F16) r[j] = f32_to_f16((float)h[8 * i + j] * sc);
          else r[j] = f32_to_bf16((float)h[8 * i + j] * sc);
        }
        const psg_u32x4 v = {xp_pack(r[0], r[1]), xp_pack(r[2], r[3]), xp_pack(r[4], r[5]), xp_pack(r[6], r[7])};
        o[i] = v;
      }
    }
  }
}

template <int FMT>
static int xp_launch(const char* name, psg_ctx* ctx, const void* q, const void* e, const float* s, void* out, int N, int K,
                     int out_dtype, void* stream) {
  constexpr int V = XpUnit<FMT>::VALS;
  PSG_REQUIRE(ctx && q && out && (FMT == 8 || e), PSG_ERR_INVALID, "%s: NULL argument", name);
  PSG_REQUIRE(out_dtype == PSG_F32 || out_dtype == PSG_BF16 || out_dtype == PSG_F16, PSG_ERR_INVALID, "%s: out_dtype %d", name,
              out_dtype);
  PSG_REQUIRE(s || out_dtype == PSG_F16, PSG_ERR_INVALID, "%s: the unscaled form (s == NULL) is fp16 only, got out_dtype %d", name,
              out_dtype);
  PSG_REQUIRE(N >= 1 && K >= 32 && K % 32 == 0, PSG_ERR_UNSUPPORTED, "%s: N=%d (>= 1), K=%d (a multiple of 32)", name, N, K);
  PSG_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)out & 15) == 0, PSG_ERR_UNSUPPORTED,
              "%s: q and out must be 16-byte aligned (16-byte accesses)", name);
  const uint32_t upr = (uint32_t)(K / V);
  const uint64_t units = (uint64_t)N * upr;
  const uint64_t want = (units + XP_THREADS - 1) / XP_THREADS, cap = (uint64_t)ctx->num_cu * XP_WG_PER_CU;
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  const hipStream_t st = (hipStream_t)stream;
  const uint8_t *q8 = (const uint8_t*)q, *e8 = (const uint8_t*)e;
#define XP_GO(OUT, SC) xp_expand_kernel<FMT, OUT, SC><<<grid, XP_THREADS, 0, st>>>(q8, e8, s, out, units, upr)
  if (!s) XP_GO(PSG_F16, false);
  else if (out_dtype == PSG_F32) XP_GO(PSG_F32, true);
  else if (out_dtype == PSG_BF16) XP_GO(PSG_BF16, true);
  else XP_GO(PSG_F16, true);
#undef XP_GO
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

extern "C" int psg_expand_w8(psg_ctx* ctx, const void* q, const float* s, void* out, int N, int K, int out_dtype, void* stream) {
  return xp_launch<8>("psg_expand_w8", ctx, q, nullptr, s, out, N, K, out_dtype, stream);
}

extern "C" int psg_expand_w4(psg_ctx* ctx, const void* q, const void* e, const float* s, void* out, int N, int K, int out_dtype,
                             void* stream) {
  return xp_launch<4>("psg_expand_w4", ctx, q, e, s, out, N, K, out_dtype, stream);
}
