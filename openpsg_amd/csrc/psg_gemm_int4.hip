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
// The schedule is psg_gemm_w4.hip's - a unit of 256 weight rows x 256 K, 128-byte weight rows in 16-byte pieces, the XOR
// swizzle on the source address, the counted vmcnt ladder, a ring of two units (PAIR) / three (single) - with
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
#include "psg_common.h"
#include "psg_wave.h"

#define I4_BK 256
#define I4_BN 256
#define I4_WAVES 8
#define I4_GROUP 128

__host__ __device__ static inline int i4_owner(int64_t u, int64_t T, int G) { return (int)(((u + 1) * G - 1) / T); }
__host__ __device__ constexpr int i4_nst(bool pair) { return pair ? 2 : 3; }
__host__ __device__ constexpr int i4_stage_bytes(bool pair) { return (pair ? 64 : 32) * 512 + I4_BN * 128 + I4_BN * 8; }

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

// S_al > 0: aligned ranges (workgroup i = slab i / S_al, slice i % S_al of its K walk); 0: stream-K
template <typename E, bool PAIR>
__global__ void __launch_bounds__(I4_WAVES * 64, 1)
i4_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const uint8_t* __restrict__ g_img,
               float* __restrict__ part, int M, int N, int K, int S, int S_al, const float* __restrict__ row_scale) {
  using v8 = typename E::v8;
  constexpr int NST = i4_nst(PAIR);
  constexpr int XT = PAIR ? 2 : 1, XR = XT * 32;             // x tiles of 32 rows (PAIR: plane 0, plane 1)
  constexpr int XQ = XR * 128, XB = 4 * XQ;                  // one K quarter of the x image / all four
  constexpr int WB = I4_BN * 128;                            // the weight image
  constexpr int STAGE = i4_stage_bytes(PAIR);                // one unit: [x: K quarters 0..3 | w: 256 rows x 128 B | g: 256 x 8 B]
  constexpr int XI = XB / 1024, NI = (XB + WB) / 1024;       // 16-byte DMA instructions (8 rows x 128 B each): x / x and w
  constexpr int PER = NI / I4_WAVES + 1;                     // per wave and unit: its share of x and w + its rows' groups
  static_assert(STAGE == XB + WB + I4_BN * 8 && NST * STAGE <= 160 * 1024, "LDS of a CU");
  static_assert(NI % I4_WAVES == 0 && XR % 16 == 0, "uniform DMA counts, operand-local swizzle");
  static_assert(2 * PER <= 63, "vmcnt field");
  static_assert(I4_BK == 2 * I4_GROUP, "a unit is two groups: sub-steps 0-1 and 2-3");
  constexpr int NR = 1 + 4 * XT;                             // LDS reads of one sub-step
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t smem_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int nk = K / I4_BK, NB = (N + I4_BN - 1) / I4_BN;
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
          (const __attribute__((address_space(1))) void*)(x + (int64_t)gr * K + kt * I4_BK + quarter * 64 + piece * 8),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 0);
    } else {
      int gr = slab * I4_BN + (r - XI * 8);
      gr = gr < N ? gr : N - 1;
      __builtin_amdgcn_global_load_lds(                      // a weight byte is read once by one CU: non-temporal
          (const __attribute__((address_space(1))) void*)(w + (int64_t)gr * Kb + kt * 128 + piece * 16),
          (__attribute__((address_space(3))) void*)(sb + idx * 1024), 16, 0, 2);
    }
  };
  // the groups of this wave's 32 rows of the unit: lane -> dword lane & 1 of row lane >> 1, LDS = its slot + 4 lane
  auto stage_grp = [&](int slab, int kt, unsigned char* sb) {
    int gr = slab * I4_BN + wid * 32 + (lane >> 1);
    gr = gr < N ? gr : N - 1;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(g_img + ((int64_t)kt * N + gr) * 8 + (lane & 1) * 4),
        (__attribute__((address_space(3))) void*)(sb + XB + WB + wid * 256), 4, 0, 2);
  };
  auto stage = [&](int slab, int kt, int buf, int q0, int q1) {   // this wave's instructions q0 .. q1 - 1 of the unit
    unsigned char* sb = smem + buf * STAGE;
    for (int q = q0; q < q1; ++q) {
      if (q < PER - 1) stage_one(slab, kt, sb, wid + I4_WAVES * q);
      else if (q == PER - 1) stage_grp(slab, kt, sb);
    }
  };

  const int l31 = lane & 31, hi = lane >> 5;
  uint32_t arow[XT];
#pragma unroll
  for (int i = 0; i < XT; ++i) arow[i] = (uint32_t)((i * 32 + l31) * 128);
  const uint32_t aswz = (uint32_t)((l31 >> 1) & 7);          // (tile bases are multiples of 32 rows)
  const uint32_t brow = (uint32_t)(XB + (wid * 32 + l31) * 128), bswz = aswz;
  const uint32_t grow = (uint32_t)(XB + WB + (wid * 32 + l31) * 8);

  union Frag {
    psg_u32x4 u;
    v8 v;
  };
  psg_f32x16 acc = (psg_f32x16){0};                          // sum over groups of gs * (the group's integer products)
  psg_f32x16 tmp[XT];                                        // the current group's, per x tile

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
    const psg_u32x2 gv = psg_lds_read64(base + grow);         // this row's two groups: [gs0 | gs1 << 16], [z0 | z1 << 8]
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
    // sub-steps 2 g, 2 g + 1 are group g: the first starts tmp from zero, the second folds it into acc with the group's scale
    auto mma = [&](int s2, Frag (&a_)[XT][4], psg_u32x4& b_) {
      const int g = s2 >> 1;
      const I4Zero<E> z((gv[1] >> (8 * g)) & 0xfu);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const v8 b = i4_widen(b_[j], z);
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
      else slot = (int)blockIdx.x - i4_owner((int64_t)slab * nk, T, G);
      const int nslots = (slab_end && S_al == 0) ? S : slot + 1;   // ending a slab (stream-K): zero the slots it did not use
      // D[m][n]: register r of a lane = row 8 (r >> 2) + 4 hi + (r & 3) of the tile, column lane & 31
      const int n0 = slab * I4_BN + wid * 32;
      if (n0 + l31 < N) {
        const int lane_off = 4 * hi * N + l31;
        float rs[16];                                        // (all sixteen loads in flight before the first store waits)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m_ = 8 * (r >> 2) + (r & 3) + 4 * hi;
          rs[r] = PAIR ? row_scale[m_ < M ? m_ : M - 1] : 1.f;
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
              if (real) val = PAIR ? acc[r] * rs[r] : acc[r];
              rowp[lane_off] = val;
            }
          }
        }
      }
      acc = (psg_f32x16){0};
      after_flush = true;
    }
    advance(slab, kt);
    buf = buf + 1 == NST ? 0 : buf + 1;
  }
}

// ---- host side: plan and launch (psg_gemm_w4.hip's: the unit, its bytes and its slices are the same) --------------------
struct i4_plan {
  int grid, slots, s_al;
};

static int i4_streamk_slots(int N, int K, int G) {
  const int nk = K / I4_BK, NB = (N + I4_BN - 1) / I4_BN;
  const int64_t T = (int64_t)NB * nk;
  int smax = 1;
  for (int b = 0; b < NB; ++b) {
    const int i0 = i4_owner((int64_t)b * nk, T, G), i1 = i4_owner((int64_t)(b + 1) * nk - 1, T, G);
    if (i1 - i0 + 1 > smax) smax = i1 - i0 + 1;
  }
  return smax;
}

// mode 1: ranges aligned to the slabs, 2: stream-K, 0: the cheaper estimate (the longest range's units x the unit's cost +
// the fp32 slices it leaves).  Made for 32 rows whatever M is: a row's k ranges must not follow the row count.
static i4_plan i4_make_plan(const psg_ctx* ctx, int N, int K, int forced_mode, bool pair) {
  i4_plan best{0, 0, 0};
  double best_t = 1e300;
  const int G = ctx->num_cu < 1024 ? ctx->num_cu : 1024;
  const int nk = K / I4_BK, NB = (N + I4_BN - 1) / I4_BN;
  const int64_t T = (int64_t)NB * nk;
  const int stage = i4_stage_bytes(pair);
  const double unit_us = fmax((double)stage / (40.0 * 2.4e3), (double)I4_BN * 136 * G / 5.8e6);
  for (int mode = 1; mode <= 2; ++mode) {
    if (forced_mode && forced_mode != mode) continue;
    i4_plan p{0, 0, 0};
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
      p.slots = i4_streamk_slots(N, K, p.grid);
      while (p.slots > PSG_MAX_SPLITS && p.grid > NB) {      // few slabs, long K walks: fewer workgroups = longer segments
        p.grid = p.grid * 7 / 8 > NB ? p.grid * 7 / 8 : NB;
        p.slots = i4_streamk_slots(N, K, p.grid);
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

static int i4_plan_checked(const char* name, psg_ctx* ctx, int M, int N, int K, int group, int mode, bool pair, i4_plan* p,
                           int* slots) {
  PSG_REQUIRE(ctx && slots, PSG_ERR_INVALID, "%s: NULL argument", name);
  PSG_REQUIRE(M >= 1 && M <= 32 && N >= 16 && N % 16 == 0 && K >= I4_BK && K % I4_BK == 0 && group == I4_GROUP && mode >= 0 &&
                  mode <= 2,
              PSG_ERR_UNSUPPORTED, "%s: M=%d (1..32), N=%d (multiple of 16), K=%d (multiple of %d), group=%d (%d), mode=%d", name,
              M, N, K, I4_BK, group, I4_GROUP, mode);
  *p = i4_make_plan(ctx, N, K, mode, pair);
  PSG_REQUIRE(p->grid > 0 && p->slots <= PSG_MAX_SPLITS, PSG_ERR_UNSUPPORTED, "%s: no plan with <= %d slices for N=%d K=%d mode=%d",
              name, PSG_MAX_SPLITS, N, K, mode);
  *slots = p->slots;
  return PSG_OK;
}

template <typename E, bool PAIR>
static int i4_launch(const char* name, const i4_plan& p, const void* x, const void* q_img, const void* g_img, float* part, int M,
                     int N, int K, const float* row_scale, void* stream) {
  PSG_REQUIRE(((uintptr_t)q_img & 15) == 0 && ((uintptr_t)g_img & 15) == 0 && ((uintptr_t)x & 15) == 0, PSG_ERR_UNSUPPORTED,
              "%s: x, q_img and g_img must be 16-byte aligned", name);
  constexpr int LDS = i4_nst(PAIR) * i4_stage_bytes(PAIR);
  auto k = i4_gemm_kernel<E, PAIR>;
  hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  if (e != hipSuccess) {
    psg_set_error("%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
    return PSG_ERR_HIP;
  }
  k<<<(unsigned)p.grid, I4_WAVES * 64, LDS, (hipStream_t)stream>>>((const uint16_t*)x, (const uint8_t*)q_img,
                                                                   (const uint8_t*)g_img, part, M, N, K, p.slots, p.s_al, row_scale);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

extern "C" int psg_split_gemm_int4_plan(psg_ctx* ctx, int M, int N, int K, int group, int mode, int* slots) {
  i4_plan p;
  return i4_plan_checked("psg_split_gemm_int4_plan", ctx, M, N, K, group, mode, true, &p, slots);
}

extern "C" int psg_split_gemm_int4(psg_ctx* ctx, const void* x2, const float* inv_scale, const void* q_img, const void* g_img,
                                   float* part, int M, int N, int K, int group, int slots, int mode, void* stream) {
  PSG_REQUIRE(ctx && x2 && inv_scale && q_img && g_img && part, PSG_ERR_INVALID, "psg_split_gemm_int4: NULL argument");
  i4_plan p;
  int want = 0;
  const int rc = i4_plan_checked("psg_split_gemm_int4", ctx, M, N, K, group, mode, true, &p, &want);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(slots == want, PSG_ERR_INVALID, "psg_split_gemm_int4: slots=%d, the plan for N=%d K=%d writes %d", slots, N, K, want);
  return i4_launch<EF16, true>("psg_split_gemm_int4", p, x2, q_img, g_img, part, M, N, K, inv_scale, stream);
}

extern "C" int psg_skinny_gemm_int4_plan(psg_ctx* ctx, int M, int N, int K, int group, int dtype, int mode, int* slots) {
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED, "psg_skinny_gemm_int4_plan: dtype %d (bf16 / fp16)", dtype);
  i4_plan p;
  return i4_plan_checked("psg_skinny_gemm_int4_plan", ctx, M, N, K, group, mode, false, &p, slots);
}

extern "C" int psg_skinny_gemm_int4(psg_ctx* ctx, const void* x, const void* q_img, const void* g_img, float* part, int M, int N,
                                    int K, int group, int slots, int dtype, int mode, void* stream) {
  PSG_REQUIRE(ctx && x && q_img && g_img && part, PSG_ERR_INVALID, "psg_skinny_gemm_int4: NULL argument");
  i4_plan p;
  int want = 0;
  const int rc = i4_plan_checked("psg_skinny_gemm_int4", ctx, M, N, K, group, mode, false, &p, &want);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(slots == want, PSG_ERR_INVALID, "psg_skinny_gemm_int4: slots=%d, the plan for N=%d K=%d writes %d", slots, N, K, want);
  PSG_DISPATCH_E16(dtype, "psg_skinny_gemm_int4",
                   return (i4_launch<E, false>("psg_skinny_gemm_int4", p, x, q_img, g_img, part, M, N, K, nullptr, stream)));
  return PSG_ERR_INVALID;
}
