// Wave-level device primitives of the hand-scheduled kernels (gfx950, wave = 64): counted waits, the LDS-only barrier,
// LDS accesses that stay out of the compiler's sight, the wait ladder behind an LDS-DMA ring and the permlane row
// reductions.  Device code only; psg_common.h stays the host + device header.  Everything here is __forceinline__ and
// emits exactly the instruction text it shows: a variant that differs in one s_nop or one trailing wait is another
// function, because each count was chosen for its call sites.
//
// Three facts about hipcc (ROCm 7.2) that the code below works around, stated here once:
//   (1) LDS-DMA aliasing.  To the compiler a pending global_load_lds is an LDS write that may alias ANY ds access it
//       generates itself, so it puts s_waitcnt vmcnt(0) in front of that access (and of __syncthreads()): the whole
//       prefetch ring is drained.  LDS traffic and barriers that run next to a ring are therefore inline asm, and the
//       ring is synchronised by the issuing wave's own counted vmcnt only.
//   (2) No hazard padding for asm operands.  The wait states between a matrix-core (or VALU) result and an asm
//       statement that consumes it are NOT inserted by the compiler; the s_nop in front of such a consumer supplies them.
//   (3) __builtin_amdgcn_permlane16_swap returns its FIRST result in both vector elements (v_add_f32 v1, v1, v1 in the
//       ISA), so v_permlane16_swap is inline asm.  __builtin_amdgcn_permlane32_swap is correct and is used as a builtin
//       where no hazard of (2) is involved.
#pragma once
#include "psg_common.h"

// ---- counted waits, LDS-only barrier -----------------------------------------------------------------------------------
template <int N_>
__device__ __forceinline__ void psg_vmwait() {        // at most N_ vector-memory operations (LDS-DMAs, loads, stores) pending
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}
template <int N_>
__device__ __forceinline__ void psg_lgkmwait() {      // at most N_ LDS / scalar-memory operations pending
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N_) : "memory");
}
// Workgroup barrier for LDS traffic only: __syncthreads() would also drain the vector-memory counter, see (1)
__device__ __forceinline__ void psg_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Wait ladder of a per-wave LDS-DMA ring: run-time "blocks issued after the wanted one that may stay in flight" ->
// compile-time vmcnt.  PER = DMA instructions per block, MAXN = ring slots - 1 (the counter saturates at 63).
template <int PER, int MAXN>
struct PsgDmaWait {
  static __device__ __forceinline__ void go(int newer) {
    if (newer >= MAXN) psg_vmwait<(MAXN * PER < 63 ? MAXN * PER : 63)>();
    else PsgDmaWait<PER, MAXN - 1>::go(newer);
  }
};
template <int PER>
struct PsgDmaWait<PER, 0> {
  static __device__ __forceinline__ void go(int) { psg_vmwait<0>(); }
};

// ---- LDS accesses by byte address, invisible to the compiler (1) --------------------------------------------------------
// plain forms: the caller waits (psg_lgkmwait) where it needs the value - fragment reads of the dense / batch GEMMs and
// the cross-attention slots, which issue several before one wait
__device__ __forceinline__ psg_u32x4 psg_lds_read128(uint32_t a) {
  psg_u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a) : "memory");
  return v;
}
__device__ __forceinline__ uint32_t psg_lds_read32(uint32_t a) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(a) : "memory");
  return v;
}
__device__ __forceinline__ psg_u32x2 psg_lds_read64(uint32_t a) {
  psg_u32x2 v;
  asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(a) : "memory");
  return v;
}
__device__ __forceinline__ void psg_lds_write64(uint32_t a, psg_u32x2 v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(v) : "memory");
}
__device__ __forceinline__ void psg_lds_write32(uint32_t a, uint32_t v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory");
}
// read that retires itself: the partial-tile read-out of the skinny GEMMs, one read per global store
__device__ __forceinline__ psg_f32x4 psg_lds_read128_wait(uint32_t a) {
  psg_f32x4 v;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
  return v;
}
// write of matrix-core results: s_nop 15 covers MFMA result -> LDS store (2); the skinny GEMMs' partial tiles
__device__ __forceinline__ void psg_lds_write128_mfma(uint32_t a, psg_f32x4 v) {
  asm volatile("s_nop 15\n\tds_write_b128 %0, %1" ::"v"(a), "v"(v) : "memory");
}

// ---- lane exchanges on the VALU (no LDS round trip) ---------------------------------------------------------------------
// max / sum of a lane's value and its partner's (lane ^ 32), in both: the two halves of a 32-row MFMA tile
__device__ __forceinline__ float psg_xchg32_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float psg_xchg32_sum(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// sum / max over the four 16-lane rows of a wave, in every lane, associated (r0 + r1) + (r2 + r3).  v_permlane16_swap
// exchanges the odd rows of its first operand with the even rows of its second, v_permlane32_swap the upper half of the
// first with the lower half of the second; fed two copies of a value they leave "this row pair's first" / "second" in
// the two registers.  Inline asm for (3); NOP16 / NOP32 are the wait states of (2) in front of the two swaps:
//   <3, 3>  VALU write -> permlane read: the fp32 attention's softmax statistics (psg_attn_f32)
//   <7, 1>  psg_rows4_sum_mfma: the value is a matrix-core result (2-pass MFMA -> VALU read: 5 wait states) - the four
//           kq partials of the fp32 skinny GEMM's 4-row groups (psg_gemm_f32, psg_decode_layer)
template <int NOP16 = 3, int NOP32 = 3>
__device__ __forceinline__ float psg_rows4_sum(float v) {
  float a = v, b = v;
  asm volatile("s_nop %2\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b) : "n"(NOP16));   // [r0 r0 r2 r2], [r1 r1 r3 r3]
  const float s = a + b;
  float c = s, d = s;
  asm volatile("s_nop %2\n\tv_permlane32_swap_b32 %0, %1" : "+v"(c), "+v"(d) : "n"(NOP32));   // [lo lo], [hi hi]
  return c + d;
}
__device__ __forceinline__ float psg_rows4_sum_mfma(float v) { return psg_rows4_sum<7, 1>(v); }
__device__ __forceinline__ float psg_rows4_max(float v) {
  float a = v, b = v;
  asm volatile("s_nop 3\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  const float s = fmaxf(a, b);
  float c = s, d = s;
  asm volatile("s_nop 3\n\tv_permlane32_swap_b32 %0, %1" : "+v"(c), "+v"(d));
  return fmaxf(c, d);
}
