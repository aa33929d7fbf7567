// Decode-step projections over group-wise INT4 weights (GPTQ / AWQ checkpoints): part[s][m][n] = split-K slices
// of x[M][K] . W'[N][K]^T, M <= 32 rows, where the model's weight is W'[n][k] = float(gs[n][k / 128]) * (q[n][k] - gz[n][k /
// 128]) (openpsg_amd/weights.py, dequantize_int4_groups): 4-bit codes q, one fp16 scale gs and one 4-bit zero point gz per
// 128 weights of a row.  The codes stream from HBM as HALF a byte per weight plus 8 bytes per row and 256 k (4.25 bits per
// weight), are widened in registers to the EXACT integers q - z in the x operand's 16-bit type and multiplied on the
// 16-bit matrix cores with fp32 accumulation.  gs is an arbitrary fp16 number: gs (q - z) is no 16-bit value, so the
// scale is applied in fp32 to each group's partial sum, inside the K loop - never to the 16-bit operand.
//   PAIR   (psg_split_gemm_int4, fp32s mode): x is the two fp16 planes [2][M][K] + inv_scale[M] of psg_split_f16x2 /
//          psg_rmsnorm_split2: part = sum_g gs_g (xh . (q - z) + xl . (q - z))_g inv_scale[m];
//   single (psg_skinny_gemm_int4, bf16 / fp16 / mixed): x is [M][K] bf16 or fp16: part = sum_g gs_g (x . (q - z))_g.
// The kernel is psg_gemm_q32.h's with psg_gemm_w4.hip's schedule - a unit of 256 weight rows x 256 K, 128-byte weight rows
// in 16-byte pieces, the XOR swizzle on the source address, the counted vmcnt ladder, a ring of two units (PAIR) / three
// (single) - with
//   * the GROUP image in place of the exponent image: a unit holds two groups of a row, and the caller passes (gs, gz)
//     re-laid-out as g_img[K / 256][N][8 bytes] (ops.int4_group_image): bytes 0-1 the fp16 scale of the unit's first group,
//     2-3 of its second, byte 4 / 5 their zero points, 6-7 zero.  A wave's 32 rows of a unit are 256 contiguous bytes: one
//     4-byte DMA per wave and unit, and ONE ds_read_b64 per lane and unit;
//   * the widening.  q_img is the project's own image of q (ops.int4_q_image): of the 8 codes of a dword, k = 8 d + e sits
//     in nibble (0, 4, 1, 5, 2, 6, 3, 7)[e], so that the mask-and-shift unpack, which yields the nibble pairs (j, j + 4) in
//     the two halves of a register, comes out in the K order of the x fragments: registers (n0 n4)(n1 n5)(n2 n6)(n3 n7) =
//     k 0..7.  fp16: a nibble in bits 0-3 of a half ORed into 0x6400 is 1024 + q, in bits 4-7 ORed into 0x5400 is 64 + q
//     (no shift for half of them); one v_pk_add_f16 of -(1024 + z) / -(64 + z) gives q - z: 5 + 4 instructions per 8 codes.
//     bf16 has no packed arithmetic here: nibble k of a word ORed into the fp32 2^(23 - 4 k) is 2^(23 - 4 k) + q for k <= 4
//     (one shift by 12 reaches nibbles 5..7), an fp32 subtraction of 2^(23 - 4 k) + z gives q - z, whose upper 16 bits are
//     its bf16 exactly; v_perm_b32 packs two: 1 + 8 + 8 + 4 instructions per 8 codes.  |q - z| <= 15 is exact in both;
//   * the scale: sub-steps 0-1 of a unit are one group, 2-3 the other, for both lane halves.  A group accumulates into
//     temporary fp32 fragments from zero and is folded with acc = fma(float(gs), tmp, acc): 16 FMAs per x tile and group
//     (a lane's 16 accumulator registers all belong to weight row lane & 31).  The PAIR form folds both planes into ONE
//     accumulator fragment (16 + 2 x 16 registers instead of psg_gemm_w4.hip's 2 x 16).
// inv_scale[m] (PAIR) is applied where a slice is stored; there is no column scale.
// A row's result does not depend on the other rows (nor on M: the plan is made for 32 rows whatever M is).
#include "psg_gemm_q32.h"

#define I4_GROUP 128

// the zero point of a group, in the form the widening of E subtracts
template <typename E>
struct I4Zero;
template <>
struct I4Zero<EF16> {
  EF16::v2 c0, c1;                                           // (1024 + z, 1024 + z), (64 + z, 64 + z)
  __device__ __forceinline__ explicit I4Zero(uint32_t z) {
    c0 = __builtin_bit_cast(EF16::v2, (0x6400u | z) * 0x10001u);
    c1 = __builtin_bit_cast(EF16::v2, (0x5400u | (z << 4)) * 0x10001u);
  }
};
template <>
struct I4Zero<EBf16> {
  float c[5];                                                // 2^(23 - 4 k) + z
  __device__ __forceinline__ explicit I4Zero(uint32_t z) {
    const float zf = (float)z;
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] = __uint_as_float((uint32_t)(150 - 4 * k) << 23) + zf;
  }
};

// 8 codes of q_img (one dword, nibble order of the header) -> the 8 exact values q - z of E's type, K ascending
__device__ __forceinline__ EF16::v8 i4_widen(uint32_t d, const I4Zero<EF16>& z) {
  using v2 = EF16::v2;
  const uint32_t s = d >> 8;
  union {
    v2 p[4];
    EF16::v8 v;
  } o;
  o.p[0] = __builtin_bit_cast(v2, (d & 0x000F000Fu) | 0x64006400u) - z.c0;
  o.p[1] = __builtin_bit_cast(v2, (d & 0x00F000F0u) | 0x54005400u) - z.c1;
  o.p[2] = __builtin_bit_cast(v2, (s & 0x000F000Fu) | 0x64006400u) - z.c0;
  o.p[3] = __builtin_bit_cast(v2, (s & 0x00F000F0u) | 0x54005400u) - z.c1;
  return o.v;
}
template <int KN>
__device__ __forceinline__ uint32_t i4_f32(uint32_t v, const I4Zero<EBf16>& z) {   // nibble KN of v: q - z as fp32 bits
  return __float_as_uint(__uint_as_float((v & (0xFu << (4 * KN))) | ((uint32_t)(150 - 4 * KN) << 23)) - z.c[KN]);
}
__device__ __forceinline__ EBf16::v8 i4_widen(uint32_t d, const I4Zero<EBf16>& z) {
  const uint32_t s = d >> 12;                                // nibbles 3..7 of d in places 0..4
  union {
    uint32_t p[4];
    EBf16::v8 v;
  } o;
  // v_perm_b32: the upper halves of (odd element, even element) = two bf16, exact (q - z has at most 4 significant bits)
  o.p[0] = __builtin_amdgcn_perm(i4_f32<4>(d, z), i4_f32<0>(d, z), 0x07060302u);
  o.p[1] = __builtin_amdgcn_perm(i4_f32<2>(s, z), i4_f32<1>(d, z), 0x07060302u);
  o.p[2] = __builtin_amdgcn_perm(i4_f32<3>(s, z), i4_f32<2>(d, z), 0x07060302u);
  o.p[3] = __builtin_amdgcn_perm(i4_f32<4>(s, z), i4_f32<3>(d, z), 0x07060302u);
  return o.v;
}

// the format of psg_gemm_q32.h's kernel
struct I4Fmt {
  static constexpr int BK = 256, SIDE = 8, SIDE_HI = 0;      // four x images per unit (K quarters); g_img: two groups per row
  static constexpr bool COL_SCALE = false;
  static constexpr const char* ALIGNED = "x, q_img and g_img";
  __host__ __device__ static constexpr int nst(bool pair) { return pair ? 2 : 3; }
  static_assert(BK == 2 * I4_GROUP, "a unit is two groups: sub-steps 0-1 and 2-3");
  template <typename E, int XT>
  struct Acc {
    psg_f32x16 acc;                                          // sum over groups of gs * (the group's integer products)
    psg_f32x16 tmp[XT];                                      // the current group's, per x tile
    psg_u32x2 gv;                                            // this row's two groups: [gs0 | gs1 << 16], [z0 | z1 << 8]
    __device__ __forceinline__ void zero() { acc = (psg_f32x16){0}; }
    __device__ __forceinline__ void unit(uint32_t a) { gv = psg_lds_read64(a); }
    // sub-steps 2 g, 2 g + 1 are group g: the first starts tmp from zero, the second folds it into acc with the group's scale
    __device__ __forceinline__ void step(int s2, PsgQ32Frag<E> (&a_)[XT][4], psg_u32x4& b_) {
      const int g = s2 >> 1;
      const I4Zero<E> z((gv[1] >> (8 * g)) & 0xfu);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const typename E::v8 b = i4_widen(b_[j], z);
#pragma unroll
        for (int i = 0; i < XT; ++i)
          tmp[i] = E::mfma32(a_[i][j].v, b, ((s2 & 1) == 0 && j == 0) ? (psg_f32x16){0} : tmp[i]);   // D[m][n]
      }
      if (s2 & 1) {
        const float gs = (float)__builtin_bit_cast(_Float16, (uint16_t)(gv[0] >> (16 * g)));
#pragma unroll
        for (int i = 0; i < XT; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = __builtin_fmaf(gs, tmp[i][r], acc[r]);
      }
    }
    __device__ __forceinline__ float out(int r) const { return acc[r]; }
  };
};

// the families' argument check + the group size
static int i4_check_args(const char* name, const void* ctx, const int* slots, int M, int N, int K, int group, int mode) {
  PSG_REQUIRE(ctx && slots, PSG_ERR_INVALID, "%s: NULL argument", name);
  PSG_REQUIRE(M >= 1 && M <= 32 && N >= 16 && N % 16 == 0 && K >= I4Fmt::BK && K % I4Fmt::BK == 0 && group == I4_GROUP &&
                  mode >= 0 && mode <= 2,
              PSG_ERR_UNSUPPORTED, "%s: M=%d (1..32), N=%d (multiple of 16), K=%d (multiple of %d), group=%d (%d), mode=%d", name,
              M, N, K, I4Fmt::BK, group, I4_GROUP, mode);
  return PSG_OK;
}

static int i4_plan(const char* name, psg_ctx* ctx, int M, int N, int K, int group, int mode, bool pair, int* slots) {
  const int rc = i4_check_args(name, ctx, slots, M, N, K, group, mode);
  psg_sk_plan p;
  return rc != PSG_OK ? rc : psg_q32_plan_checked<I4Fmt>(name, ctx, M, N, K, mode, pair, &p, slots);
}

extern "C" int psg_split_gemm_int4_plan(psg_ctx* ctx, int M, int N, int K, int group, int mode, int* slots) {
  return i4_plan("psg_split_gemm_int4_plan", ctx, M, N, K, group, mode, true, slots);
}

extern "C" int psg_split_gemm_int4(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* q_img, const void* g_img,
                                   float* part, int M, int N, int K, int group, int slots, int mode, void* stream) {
  PSG_REQUIRE(ctx && x2 && inv_scale && q_img && g_img && part, PSG_ERR_INVALID, "psg_split_gemm_int4: NULL argument");
  const int rc = i4_check_args("psg_split_gemm_int4", ctx, &slots, M, N, K, group, mode);
  if (rc != PSG_OK) return rc;
  return psg_q32_run<I4Fmt, true>("psg_split_gemm_int4", ctx, x2, q_img, g_img, inv_scale, nullptr, part, M, N, K, slots, PSG_F16,
                                  mode, stream);
}

extern "C" int psg_skinny_gemm_int4_plan(psg_ctx* ctx, int M, int N, int K, int group, int dtype, int mode, int* slots) {
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "psg_skinny_gemm_int4_plan: dtype %d (bf16 / fp16)", dtype);
  return i4_plan("psg_skinny_gemm_int4_plan", ctx, M, N, K, group, mode, false, slots);
}

extern "C" int psg_skinny_gemm_int4(psg_ctx* ctx, const void* x, const void* q_img, const void* g_img, float* part, int M, int N,
                                    int K, int group, int slots, int dtype, int mode, void* stream) {
  PSG_REQUIRE(ctx && x && q_img && g_img && part, PSG_ERR_INVALID, "psg_skinny_gemm_int4: NULL argument");
  const int rc = i4_check_args("psg_skinny_gemm_int4", ctx, &slots, M, N, K, group, mode);
  if (rc != PSG_OK) return rc;
  return psg_q32_run<I4Fmt, false>("psg_skinny_gemm_int4", ctx, x, q_img, g_img, nullptr, nullptr, part, M, N, K, slots, dtype,
                                   mode, stream);
}
