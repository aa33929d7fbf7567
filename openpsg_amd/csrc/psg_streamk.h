// The schedule bookkeeping of the weight-streaming GEMMs (psg_batch_gemm.hip, psg_batch_gemm_q.hip and the 32-row quantised
// kernel of psg_gemm_q32.h), written once for host and device.  The work is NB slabs of weight rows x nk K steps = T units
// in slab-major order, dealt to the workgroups as contiguous ranges:
//   stream-K (S_al == 0): workgroup i owns [i T / G, (i + 1) T / G) - every workgroup streams the same number of weight
//       bytes whatever N is; a range may cross slab boundaries;
//   aligned  (S_al  > 0): workgroup i owns slice i % S_al of slab i / S_al's K walk - one segment per workgroup.
// A segment (the part of a range inside one slab) ends in ONE fp32 slice part[slot]: slot = the rank of the segment inside
// its slab, so a slab's slices are k-ordered without atomics; the workgroup that ends a slab under stream-K zero-fills
// the slots the slab did not use.  The host plans the mode, the grid and the slot count by walking the same integer
// arithmetic.  The plan decides which k range a slot covers: its arithmetic is visible in the low bits of every result.
#pragma once
#include "psg_common.h"

#define PSG_SK_THREADS 512  // 8 waves: every kernel of the family

// first workgroup whose unit range [i T / G, (i + 1) T / G) holds unit u
__host__ __device__ static inline int psg_sk_owner(int64_t u, int64_t T, int G) { return (int)(((u + 1) * G - 1) / T); }

// ---- device side: the range of a workgroup, the slot of a segment end, the walk ------------------------------------------
struct psg_sk_span {
  int64_t g0, g1;
};
// the units [g0, g1) of this workgroup (G = gridDim.x, read once by the kernel)
__device__ __forceinline__ psg_sk_span psg_sk_range(int nk, int64_t T, int G, int S_al) {
  psg_sk_span r;
  if (S_al > 0) {
    const int sb = blockIdx.x / S_al, sl = blockIdx.x - sb * S_al;
    r.g0 = (int64_t)sb * nk + (int64_t)sl * nk / S_al;
    r.g1 = (int64_t)sb * nk + (int64_t)(sl + 1) * nk / S_al;
  } else {
    r.g0 = (int64_t)blockIdx.x * T / G;
    r.g1 = ((int64_t)blockIdx.x + 1) * T / G;
  }
  return r;
}
// the slice a segment of `slab` that ends in this workgroup is stored to.  It writes slots [slot, nslots): nslots = slot + 1,
// or S where it ends the slab under stream-K and zero-fills the slots the slab did not use
__device__ __forceinline__ int psg_sk_slot(int slab, int nk, int64_t T, int G, int S_al) {
  if (S_al > 0) return (int)blockIdx.x % S_al;
  return (int)blockIdx.x - psg_sk_owner((int64_t)slab * nk, T, G);
}
__device__ __forceinline__ void psg_sk_advance(int& slab, int& kt, int nk) {   // the next unit of the walk
  if (++kt == nk) {
    kt = 0;
    ++slab;
  }
}

// ---- host side: plan, argument checks, launch -----------------------------------------------------------------------------
struct psg_sk_plan {
  int grid, slots, s_al;
};

// slices the fullest slab gets when G workgroups share the T units as stream-K ranges
static int psg_sk_streamk_slots(int NB, int nk, int G) {
  const int64_t T = (int64_t)NB * nk;
  int smax = 1;
  for (int b = 0; b < NB; ++b) {
    const int i0 = psg_sk_owner((int64_t)b * nk, T, G), i1 = psg_sk_owner((int64_t)(b + 1) * nk - 1, T, G);
    if (i1 - i0 + 1 > smax) smax = i1 - i0 + 1;
  }
  return smax;
}

// Candidates {aligned slices, stream-K} for NB slabs x nk steps on G workgroups (the CU count, clamped by the caller).
// Estimated time = the longest range's units x unit_us (the caller's: L2 -> LDS staging at ~40 B/clk/CU, the unit's matrix
// instructions or its share of the HBM stream) + the fp32 slices of `rows` rows it leaves (written here, read by the
// consumer).  Aligned ranges need slabs x slices ~ the grid; stream-K balances any shape at the price of a second flush
// per workgroup and the zero-filled slots.  forced_mode 1: aligned, 2: stream-K, 0: the cheaper estimate (ties: aligned).
// Returns grid 0 (and 1e300 in *t_out) when no candidate stays within PSG_MAX_SPLITS slices.
static psg_sk_plan psg_sk_make_plan(int G, int NB, int nk, int N, double unit_us, int64_t rows, int forced_mode,
                                    double* t_out = nullptr) {
  psg_sk_plan best{0, 0, 0};
  double best_t = 1e300;
  const int64_t T = (int64_t)NB * nk;
  for (int mode = 1; mode <= 2; ++mode) {
    if (forced_mode && forced_mode != mode) continue;
    psg_sk_plan p{0, 0, 0};
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
      p.slots = psg_sk_streamk_slots(NB, nk, p.grid);
      while (p.slots > PSG_MAX_SPLITS && p.grid > NB) {      // few slabs, long K walks: fewer workgroups = longer segments
        p.grid = p.grid * 7 / 8 > NB ? p.grid * 7 / 8 : NB;
        p.slots = psg_sk_streamk_slots(NB, nk, p.grid);
      }
      if (p.slots > PSG_MAX_SPLITS) continue;
      units = (double)((T + p.grid - 1) / p.grid);
    }
    const double slice_bytes = (double)p.slots * rows * N * 4;
    const double t = units * unit_us + slice_bytes / 3.5e6 + slice_bytes / 8e6 + (mode == 2 ? 3.0 : 0.0);
    if (t < best_t) {
      best_t = t;
      best = p;
    }
  }
  if (t_out) *t_out = best_t;
  return best;
}

// the argument check of the quantised families: rows m_lo..m_hi, K in granules of kq
static int psg_sk_check_args(const char* name, const void* ctx, const int* slots, int M, int m_lo, int m_hi, int N, int K, int kq,
                             int mode) {
  PSG_REQUIRE(ctx && slots, PSG_ERR_INVALID, "%s: NULL argument", name);
  PSG_REQUIRE(M >= m_lo && M <= m_hi && N >= 16 && N % 16 == 0 && K >= kq && K % kq == 0 && mode >= 0 && mode <= 2,
              PSG_ERR_UNSUPPORTED, "%s: M=%d (%d..%d), N=%d (multiple of 16), K=%d (multiple of %d), mode=%d", name, M, m_lo, m_hi,
              N, K, kq, mode);
  return PSG_OK;
}
// a plan a consumer kernel can sum?  -> *slots
static int psg_sk_plan_ok(const char* name, const psg_sk_plan& p, int N, int K, int mode, int* slots) {
  PSG_REQUIRE(p.grid > 0 && p.slots <= PSG_MAX_SPLITS, PSG_ERR_UNSUPPORTED, "%s: no plan with <= %d slices for N=%d K=%d mode=%d",
              name, PSG_MAX_SPLITS, N, K, mode);
  *slots = p.slots;
  return PSG_OK;
}
// the caller allocated what the plan writes?
static int psg_sk_check_slots(const char* name, int slots, int want, int N, int K) {
  PSG_REQUIRE(slots == want, PSG_ERR_INVALID, "%s: slots=%d, the plan for N=%d K=%d writes %d", name, slots, N, K, want);
  return PSG_OK;
}

// set the dynamic-LDS attribute, launch on PSG_SK_THREADS threads, check
template <typename... P, typename... A>
static int psg_sk_launch(const char* name, void (*kernel)(P...), int grid, int lds, void* stream, A... args) {
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) {
    psg_set_error("%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
    return PSG_ERR_HIP;
  }
  kernel<<<(unsigned)grid, PSG_SK_THREADS, lds, (hipStream_t)stream>>>((P)args...);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}
