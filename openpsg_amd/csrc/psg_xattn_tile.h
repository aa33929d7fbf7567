// K6: what the two generations of the 16-bit relation-query cross-attention share, written once.
//
// psg_xattn_mfma.hip (first generation: Q fragments loaded straight into the MFMA layout, direct context stores) and
// psg_xattn_dma.hip (second generation: Q and context through per-wave LDS-DMA slots) are bit-equal wherever both run
// (tests/test_gpu_parity.py).  They are because everything that decides a result lives here: the LDS image of a head
// (K_h rows, V_h^T rows, mean of V_h, object bit table), the order of the row tiles, the K/V staging, the mask analysis
// of a unit and the loop over its key tiles (scores, additive mask, online softmax, P.V).  How a unit's Q tile gets in,
// how its context tile gets out and which wave computes it is each file's own business.
// The mean of V_h is NOT here: the first generation sums a V^T row with one thread per dim, the second with 8 lanes per
// dim plus shuffles; the two orders round differently in fp32, so merging them would change one kernel's bits.
#pragma once
#include "psg_common.h"
#include "psg_wave.h"

// ---- internal launchers (psg_qformer_cross_attn dispatches to them) ----
int psg_cross_attn_dma_launch(psg_ctx* ctx, const void* q, const void* k, const void* v, const uint64_t* bits,
                              int words, const int32_t* pair_index, int N, int P, int L, int nq, int heads, int policy,
                              void* out, int dtype, hipStream_t st, const int32_t* q_index, const void* q_cls);
extern "C" int psg_cross_attn_dma_lds_bytes(int N, int words, int L);
int psg_cross_attn_simple_launch(const void* q, const void* k, const void* v, const uint64_t* bits, int words,
                                 const int32_t* pair_index, int N, int P, int L, int nq, int heads, int policy,
                                 void* out, int dtype, hipStream_t st);
int psg_cross_attn_f32_launch(const void* q, const void* k, const void* v, const uint64_t* bits, int words,
                              const int32_t* pair_index, int N, int P, int L, int nq, int heads, int policy, void* out,
                              hipStream_t st);

// ---- LDS image of one head: K_h [Lpad][64] | V_h^T [64][Lpad] | mean of V_h | object bit rows [N][words] ----
// Row strides are padded by 16 B => conflict-free ds_read_b128.  Keys [L, Lpad) are padding and hold zeros.
constexpr int XATTN_KSTRIDE = 144;   // bytes per K row: 64 x 16 bit + 16 B pad

struct XattnImage {
  int Lpad;        // L rounded up to whole 32-key tiles
  int NT;          // 32-key tiles
  int VS;          // bytes per V^T row
  int vt_off;      // byte offsets from the start of the image (K_h is at 0)
  int mean_off;    // 64 floats
  int bits_off;
  size_t bytes;    // whole image, a multiple of 16: what follows it is 16-byte aligned
};

__host__ __device__ inline XattnImage xattn_image(int N, int words, int L) {
  XattnImage im;
  im.Lpad = (L + 31) & ~31;
  im.NT = im.Lpad >> 5;
  im.VS = im.Lpad * 2 + 16;
  im.vt_off = im.Lpad * XATTN_KSTRIDE;
  im.mean_off = im.vt_off + 64 * im.VS;
  im.bits_off = im.mean_off + 256;
  im.bytes = (size_t)im.bits_off + (((size_t)N * words * 8 + 15) & ~(size_t)15);   // N, words: unchecked caller input
  return im;
}

inline size_t xattn_image_bytes(int N, int words, int L) { return xattn_image(N, words, L).bytes; }

// ---- row tiles (32 query rows each) ----
// nq == 33: the NCLS tiles that batch the cls rows (row 0) of 32 consecutive pairs come FIRST - they carry per-row
// masks and need most key tiles; then tile NCLS + p = rows 1..32 of pair p, which share ONE pair mask.  Other nq: flat
// 32-row tiles over the R = P nq rows.
__host__ __device__ inline int64_t xattn_ntile(int64_t P, int nq) {
  return nq == 33 ? P + ((P + 31) >> 5) : (P * nq + 31) >> 5;
}

struct XattnTiles {
  bool aligned;    // nq == 33
  int nq;
  int64_t P, R, NCLS, ntile;
};

__device__ __forceinline__ XattnTiles xattn_tiles(int64_t R, int nq) {
  XattnTiles g;
  g.aligned = nq == 33;
  g.nq = nq;
  g.R = R;
  g.P = R / nq;
  g.NCLS = g.aligned ? (g.P + 31) >> 5 : 0;
  g.ntile = xattn_ntile(g.P, nq);
  return g;
}

// row rr (0..31) of a tile: global row, validity (a row past the end is clamped to the last one), pair
__device__ __forceinline__ void xattn_tile_row(const XattnTiles& g, int64_t tile, int rr, int64_t& row, bool& valid,
                                               int64_t& pair) {
  if (g.aligned) {
    if (tile >= g.NCLS) {
      pair = tile - g.NCLS;
      row = pair * 33 + 1 + rr;
      valid = true;
    } else {
      const int64_t pr = tile * 32 + rr;
      valid = pr < g.P;
      pair = valid ? pr : g.P - 1;
      row = pair * 33;
    }
  } else {
    row = tile * 32 + rr;
    valid = row < g.R;
    if (!valid) row = g.R - 1;
    pair = row / g.nq;
  }
}

// ---- K/V staging, once per workgroup of THREADS threads, in two halves ----
// All global loads of a thread are issued before the first LDS write (a load -> write loop paid one L2 round trip per
// iteration).  A thread owns the key PAIR (2m, 2m+1) of one 8-dim chunk c: the two keys are neighbours in the V^T row,
// so the transposed writes are 32-bit.  IT >= (Lpad / 2 key pairs * 8 chunks) / THREADS.
template <int THREADS, int IT>
__device__ __forceinline__ void xattn_kv_load(uint4 (&kv)[IT][2], uint4 (&vv)[IT][2], const uint16_t* __restrict__ k,
                                              const uint16_t* __restrict__ v, int tid, int L, int hidden, int h) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int e = tid + it * THREADS;
    const int m = e >> 3, c = e & 7;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int key = 2 * m + u;
      kv[it][u] = make_uint4(0, 0, 0, 0);
      vv[it][u] = make_uint4(0, 0, 0, 0);
      if (key < L) {
        kv[it][u] = *reinterpret_cast<const uint4*>(k + (int64_t)key * hidden + h * 64 + c * 8);
        vv[it][u] = *reinterpret_cast<const uint4*>(v + (int64_t)key * hidden + h * 64 + c * 8);
      }
    }
  }
}

// V^T is stored with key bits 2 <-> 3 swapped inside every 16-key group, which makes the accumulator registers of the
// S^T tile line up with the B-operand slots of the P.V MFMA without any cross-lane shuffle.
template <int THREADS, int IT>
__device__ __forceinline__ void xattn_kv_store(unsigned char* smem, const XattnImage& im, const uint4 (&kv)[IT][2],
                                               const uint4 (&vv)[IT][2], int tid) {
  unsigned char* vt_lds = smem + im.vt_off;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int e = tid + it * THREADS;
    const int m = e >> 3, c = e & 7;
    if (2 * m < im.Lpad) {
      *reinterpret_cast<uint4*>(smem + (2 * m) * XATTN_KSTRIDE + c * 16) = kv[it][0];
      *reinterpret_cast<uint4*>(smem + (2 * m + 1) * XATTN_KSTRIDE + c * 16) = kv[it][1];
      const int o = (2 * m) & 15;
      const int pos = (o & 3) | ((o & 8) >> 1) | ((o & 4) << 1);  // swap bits 2 <-> 3 (bit 0 stays: pair adjacent)
      const int kcol = (((2 * m) & ~15) | pos) * 2;
      const uint32_t a[4] = {vv[it][0].x, vv[it][0].y, vv[it][0].z, vv[it][0].w};
      const uint32_t bq[4] = {vv[it][1].x, vv[it][1].y, vv[it][1].z, vv[it][1].w};
#pragma unroll
      for (int d2 = 0; d2 < 4; ++d2) {
        const uint32_t lo = (a[d2] & 0xffffu) | (bq[d2] << 16);            // dim 2 d2    of keys 2m, 2m+1
        const uint32_t hi2 = (a[d2] >> 16) | (bq[d2] & 0xffff0000u);      // dim 2 d2 + 1
        *reinterpret_cast<uint32_t*>(vt_lds + (c * 8 + 2 * d2) * im.VS + kcol) = lo;
        *reinterpret_cast<uint32_t*>(vt_lds + (c * 8 + 2 * d2 + 1) * im.VS + kcol) = hi2;
      }
    }
  }
}

// ---- one unit = (row tile, head) ----
// pair id p = i * N + j -> (i, j); rcpN = 1 / N.  Exact in fp32 for p < 2^24 and N <= 1024.
__device__ __forceinline__ void xattn_pair_objects(int pidx, int N, float rcpN, int& oi, int& oj) {
  if (N <= 1024) {
    oi = (int)(((float)pidx + 0.5f) * rcpN);
    oj = pidx - oi * N;
  } else {
    oi = pidx / N;
    oj = pidx % N;
  }
}

// Which 32-key tiles does this row tile need?  wi / wj: the two object bit rows of this lane's pair as 32-bit words
// (word t = keys [32 t, 32 t + 32), 1 = attend).  A key tile no row attends to contributes exactly 0: skipped.
//  AL (a pair tile: rows 1..32 of ONE pair): the words are wave-uniform.  An empty union means plain attention over the
//     L real keys under the "unmasked" policy (force_all), and under the "uniform" policy the mean of V: the function
//     returns true and leaves needmask 0 - what to do with the mean is the caller's.
//  generic (cls tiles, other nq): per-row masks; a row whose pair mask is empty attends to every key (uniform softmax),
//     so the tile needs all key tiles.
template <bool AL>
__device__ __forceinline__ bool xattn_mask_analysis(const uint32_t* wi, const uint32_t* wj, int NT, int policy,
                                                    uint32_t& needmask, bool& force_all) {
  const uint32_t all = NT >= 32 ? 0xffffffffu : (1u << NT) - 1u;
  needmask = 0;      // wave-uniform
  force_all = false;
  if constexpr (AL) {
    for (int t = 0; t < NT; ++t)
      needmask |= ((__builtin_amdgcn_readfirstlane(wi[t] | wj[t]) != 0u) ? 1u : 0u) << t;
    if (needmask == 0u) {
      if (policy == PSG_EMPTY_UNIFORM) return true;
      force_all = true;
      needmask = all;
    }
  } else {
    bool row_empty = true;
    for (int t = 0; t < NT; ++t) {
      const uint32_t w = wi[t] | wj[t];
      row_empty = row_empty && (w == 0u);
      needmask |= (__any(w != 0u) ? 1u : 0u) << t;
    }
    if (__any(row_empty)) needmask = all;
  }
  return false;
}

// The key tiles of a unit, a dynamic loop over the set bits of needmask with a per-tile online softmax.
//   S^T = K . Q^T (A = K fragment from LDS, B = q0..q3: lane (row = lane&31, hi) holds Q[row][16 s + 8 hi .. +7]), so a
//   lane owns ONE query row and 16 keys per tile; O^T += V^T . P^T the same way (B = this lane's exponentiated scores
//   packed to 16 bit), so the rescale and the final 1/l are lane-local: lane (q, hi) ends with
//   O[q][32 dt + (r&3) + 8 (r>>2) + 4 hi] in o<dt>[r], unnormalised, and the softmax denominator in l_run.
//  AL: the additive mask is applied by the matrix core: one extra MFMA per key tile adds A'[key][0] * B'[0][row] =
//     bias(key) * 1 to S^T, which replaces three VALU instructions per score.  No bias has to absorb the scores here
//     (the empty union never gets this far under "uniform"), so a moderate bias (-2^15, exact in bf16) and the fused
//     exp2(fma(s, C, -m C)) are safe.
//  generic: per-row masks in VALU, absorbing finfo.min bias as in the reference (HF additive mask; masked key => score
//     + finfo.min, so an all-masked row is a UNIFORM softmax over the L real keys), exp2((s - m) * C) so that equal
//     scores give exactly 2^0.  Padding keys get weight 0.
// kfrag_base / vfrag_base: this lane's K and V^T fragment addresses in key tile 0 (K_h + l31 KSTRIDE + 16 hi, V_h^T +
// l31 VS + 16 hi).  The caller carries them across its units: recomputed here per unit, they cost the ten-wave LDS-DMA
// kernel, which sits 2 VGPRs under its cap, a spilled register.
template <typename E, bool AL>
__device__ __forceinline__ void xattn_key_tiles(typename E::v8 q0, typename E::v8 q1, typename E::v8 q2,
                                                typename E::v8 q3, const uint32_t* wi, const uint32_t* wj,
                                                uint32_t needmask, bool force_all, const unsigned char* kfrag_base,
                                                const unsigned char* vfrag_base, int VS, int L, int policy, int l31,
                                                int hi, psg_f32x16& o0, psg_f32x16& o1, float& m_run, float& l_run) {
  const typename E::v8 qf[4] = {q0, q1, q2, q3};
  const float C8 = 0.125f * 1.4426950408889634f;
  const float bias_raw = policy == PSG_EMPTY_UNIFORM ? -3.4028234663852886e38f : -80000.0f;  // generic path, pre-scale
  while (needmask != 0u) {
    const int t = __builtin_ctz(needmask);
    needmask &= needmask - 1u;
    uint32_t word = wi[t] | wj[t];
    const int left = L - 32 * t;                       // real keys in this tile (>= 1)
    psg_f32x16 acc;
    const unsigned char* kp = kfrag_base + t * 32 * XATTN_KSTRIDE;
    if constexpr (AL) {
      if (force_all) word = left >= 32 ? 0xffffffffu : (1u << left) - 1u;
      // A'[key = lane&31][k = 0] = 0 if the pair attends to this key, else -2^15; B'[k = 0][row] = 1 for every row, all
      // other k-slots 0
      union {
        uint32_t u[4];
        typename E::v8 v;
      } a_bias, b_one;
      a_bias.u[0] = (((word >> l31) & 1u) | (uint32_t)hi) ? 0u : E::NEG_2_15;
      a_bias.u[1] = a_bias.u[2] = a_bias.u[3] = 0u;
      b_one.u[0] = hi ? 0u : E::ONE;
      b_one.u[1] = b_one.u[2] = b_one.u[3] = 0u;
      acc = E::mfma32(a_bias.v, b_one.v, (psg_f32x16){0});
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const typename E::v8 a = *reinterpret_cast<const typename E::v8*>(kp + s * 32);
        acc = E::mfma32(a, qf[s], acc);
      }
    } else {
      {
        const typename E::v8 a = *reinterpret_cast<const typename E::v8*>(kp);
        acc = E::mfma32(a, qf[0], (psg_f32x16){0});
      }
#pragma unroll
      for (int s = 1; s < 4; ++s) {
        const typename E::v8 a = *reinterpret_cast<const typename E::v8*>(kp + s * 32);
        acc = E::mfma32(a, qf[s], acc);
      }
      // additive mask per (row, key): register r of a lane is key (r&3) + 8 (r>>2) + 4 hi of the tile
      const uint32_t inv = ~word >> (4 * hi);
      const bool has_pad = left < 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int koff = (r & 3) + 8 * (r >> 2);
        const int mb = __builtin_amdgcn_sbfe((int)inv, koff, 1);  // -1 if masked
        float y = acc[r] + __uint_as_float((uint32_t)mb & __float_as_uint(bias_raw));
        if (has_pad && (koff + 4 * hi >= left)) y = -INFINITY;
        acc[r] = y;
      }
    }
    // online softmax over the raw scores (the scale is positive)
    float cmax = acc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) cmax = fmaxf(cmax, acc[r]);
    cmax = psg_xchg32_max(cmax);
    const float m_new = fmaxf(m_run, cmax);
    float alpha, csum = 0.f;
    if constexpr (AL) {
      const float mc = m_new * C8;
      alpha = __builtin_amdgcn_exp2f(fmaf(m_run, C8, -mc));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(acc[r], C8, -mc));
        acc[r] = pv;
        csum += pv;
      }
    } else {
      alpha = __builtin_amdgcn_exp2f((m_run - m_new) * C8);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f((acc[r] - m_new) * C8);
        acc[r] = pv;
        csum += pv;
      }
    }
    csum = psg_xchg32_sum(csum);
    l_run = l_run * alpha + csum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      o0[r] *= alpha;
      o1[r] *= alpha;
    }
    // O^T += V^T . P^T : A = V^T fragment (LDS), B = this lane's P values packed to 16 bit
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
      union {
        uint32_t u[4];
        typename E::v8 v;
      } pf;
#pragma unroll
      for (int e = 0; e < 4; ++e) pf.u[e] = E::pack(acc[8 * gg + 2 * e], acc[8 * gg + 2 * e + 1]);
      const unsigned char* vp = vfrag_base + (t * 32 + 16 * gg) * 2;
      const typename E::v8 a0 = *reinterpret_cast<const typename E::v8*>(vp);
      const typename E::v8 a1 = *reinterpret_cast<const typename E::v8*>(vp + 32 * VS);
      o0 = E::mfma32(a0, pf.v, o0);
      o1 = E::mfma32(a1, pf.v, o1);
    }
  }
}
