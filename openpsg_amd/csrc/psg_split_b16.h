// An fp32 value as the EXACT sum of three bf16 values: the operand of psg_split_gemm_wb16 (psg_batch_gemm.hip), whose weight
// is a bf16 value (a bf16 checkpoint upcast on load).
//
//     x0 = bf16(x)   x1 = bf16(x - x0)   x2 = bf16(x - x0 - x1)          (round to nearest even, f32_to_bf16)
//
// x has 24 significant bits; x0 keeps the top 8, the remainder x - x0 is exact in fp32 and has <= 16, x1 keeps 8 of those,
// the second remainder is exact and has <= 8: x2 holds it whole.  bf16 has fp32's exponent range, so nothing is scaled and
// no row maximum is needed - the planes are written element by element by whichever kernel produces x.  (The sum is exact
// as long as x's lowest set bit is >= 2^-133, bf16's smallest subnormal: every |x| >= 2^-110.)
#pragma once
#include "psg_common.h"

struct sp_b16x3_t {
  uint16_t p[3];
};
__device__ __forceinline__ sp_b16x3_t sp_b16x3(float x) {
  // x is often the product that ends a row kernel's arithmetic (RMSNorm's g * (v * inv), SwiGLU's silu(gate) * up): as an
  // opaque register it cannot be contracted with the subtraction below into an fma of the UNROUNDED product
  asm("" : "+v"(x));
  sp_b16x3_t o;
  o.p[0] = f32_to_bf16(x);
  const float r1 = x - bf16_to_f32(o.p[0]);                  // exact
  o.p[1] = f32_to_bf16(r1);
  const float r2 = r1 - bf16_to_f32(o.p[1]);                 // exact
  o.p[2] = f32_to_bf16(r2);
  return o;
}

// four consecutive columns c .. c + 3 of one row into the three planes (8-byte stores); wt (option wt_stores, bit 4): written
// through the L2 as sp_store2's
__device__ __forceinline__ void sp_store3(uint16_t* o0, uint16_t* o1, uint16_t* o2, int64_t c, const float (&x)[4], int wt) {
  uint64_t w[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const sp_b16x3_t s = sp_b16x3(x[i]);
#pragma unroll
    for (int p = 0; p < 3; ++p) w[p] |= (uint64_t)s.p[p] << (16 * i);
  }
  uint16_t* o[3] = {o0, o1, o2};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    if (wt) __hip_atomic_store(reinterpret_cast<uint64_t*>(o[p] + c), w[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *reinterpret_cast<uint64_t*>(o[p] + c) = w[p];
  }
}
