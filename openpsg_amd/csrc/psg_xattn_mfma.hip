// K6: relation-query cross-attention on the CDNA4 matrix cores (primary kernel of the path).
//
// Replaces HF-IB:464-466, 487-496 as driven by V4:168-170, 179-185: the reference expands the SAME
// [L,256] patch tensor to all B = N^2 pairs and re-projects K/V per pair; here K/V [L,768] are
// projected once per image and every pair reads them from LDS.  The pair mask
// (mask_i | mask_j, V4:430-433) is never materialised: each lane ORs two rows of the per-object
// bitmask table and tests bits in registers.
//
// Work layout (gfx950, wave = 64):
//   * a workgroup (4 waves, 2 per CU) owns one head h: it stages the head's LDS image (K_h, V_h^T, the mean of V_h
//     and the whole object bit table) once, then its waves walk row tiles in a static round-robin order;
//   * row tiles (nq == 33): first the tiles that batch the cls rows (row 0) of 32 consecutive pairs - they
//     carry per-row masks - then one tile per pair = its rows 1..32, which share ONE mask, so the mask words
//     are wave-uniform, 32-key tiles nobody attends to are skipped (they contribute exactly 0), and an empty
//     union under the "uniform" policy is just the mean of V;
//   * the image layout, the tile order, the K/V staging, the mask analysis and the loop over a unit's key tiles
//     (S^T = K . Q^T and O^T = V^T . P^T on v_mfma_f32_32x32x16, mask bias as one more MFMA, online softmax) are
//     shared with the second-generation kernel (psg_xattn_dma.hip) and live in psg_xattn_tile.h;
//   * this file's own: the Q fragments go straight from global memory into the MFMA B-operand layout, the Q
//     fragments and pair ids of the next two units are in flight while one is computed, and the context rows
//     are stored directly from the accumulator layout.
// The kernel moves Q in and the context out once each (PMC: 126 MB + 124 MB at N = 50) and is bound by that
// traffic, 128 bytes per row per head; see DESIGN.md for the timeline that led here.
//
// Mask semantics: masked key => score + finfo.min (== finfo.min in fp32) so an
// all-masked row is a UNIFORM softmax over the L real keys; keys in [L, Lpad) are padding (weight 0).
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "psg_xattn_tile.h"

template <typename E, int NC>   // NC = key chunks of 128 (L <= 128 NC): sizes the staging registers
__global__ void __launch_bounds__(256, 2)
cross_attn_mfma_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                       const uint64_t* __restrict__ bits, int words, const int32_t* __restrict__ pair_index, int N,
                       int64_t R, int L, int nq, int heads, int policy,
                       uint16_t* __restrict__ out, long long* __restrict__ trace) {
  // trace != nullptr (psg_set_trace_buffer(PSG_TRACE_CROSS_ATTN), debugging only): 32 timestamps per wave
  long long* tr = trace ? trace + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 : nullptr;
  if (tr && (threadIdx.x & 63) == 0) tr[0] = __builtin_readcyclecounter();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const XattnImage im = xattn_image(N, words, L);
  unsigned char* vt_lds = smem + im.vt_off;
  unsigned char* mean_lds = smem + im.mean_off;
  uint64_t* bits_lds = reinterpret_cast<uint64_t*>(smem + im.bits_off);
  const int h = blockIdx.x % heads;
  const int g = blockIdx.x / heads;
  const int G = gridDim.x / heads;
  const int hidden = heads * 64;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const XattnTiles tg = xattn_tiles(R, nq);           // cls tiles first, then one tile per pair (psg_xattn_tile.h)
  const bool aligned = tg.aligned;
  const int64_t NCLS = tg.NCLS, ntile = tg.ntile;
  const unsigned char* kfrag_base = smem + l31 * XATTN_KSTRIDE + hi * 16;
  const unsigned char* vfrag_base = vt_lds + l31 * im.VS + hi * 16;

  // One unit of work = (row tile, head h).  Its operands sit behind a chain of dependent global loads
  // (pair_index -> object bit rows -> mask words); most key tiles are skipped, so a unit is short (~1 us)
  // and that chain must be off the critical path.  Three units are in flight: unit A is computed while
  // the Q fragments and mask words of unit B are loading (its pair id arrived during the previous unit)
  // and the pair id of unit C is loading.  Nothing in a fetch waits on a load issued in the same step.
  struct XUnit {
    typename E::v8 qf[4];
    int pidx;                          // pair id p = i * N + j of this lane's row
    int64_t row;
    bool rvalid;
  };
  // A fetch only ISSUES loads (Q fragments and the pair id); the object bit rows live in LDS, so nothing
  // in the unit's operand chain depends on another global load.
  auto fetch = [&](int64_t tile, XUnit& u) {
    int64_t pair;
    xattn_tile_row(tg, tile, l31, u.row, u.rvalid, pair);
    // Q fragments: B operand of S^T = K.Q^T; lane (q = lane&31, hi) holds Q[q][16 s + 8 hi .. +7]
    const uint16_t* qp = q + u.row * hidden + h * 64 + hi * 8;
#pragma unroll
    for (int s = 0; s < 4; ++s) u.qf[s] = *reinterpret_cast<const typename E::v8*>(qp + s * 16);
    u.pidx = pair_index[pair];
  };
  const float rcpN = 1.0f / (float)N;
  // Static round-robin distribution over the waves that own head h (wave w of G*4 takes tiles w, w + 4G, ...).
  // The expensive cls tiles come first in the order, so every wave gets at most one or two of them, and a
  // pair with an empty mask union costs less than an average pair (mean-of-V shortcut), so the remaining
  // cost spread averages out over the ~15 units of a wave.  (A global atomic work queue was measured here:
  // 2048 waves x 2 returning atomics on 12 words cost 44 us of start-up plus a round trip every 4 units.)
  const int64_t wstride = (int64_t)G * 4;
  int64_t wnext = (int64_t)g * 4 + wid;
  auto next_tile = [&]() -> int64_t {
    const int64_t t = wnext;
    wnext += wstride;
    return t;
  };
  // One unit = (row tile, head): AL = a pair tile (nq == 33, rows 1..32 of ONE pair, wave-uniform mask words, mask
  // bias on the matrix core), otherwise per-row masks in VALU; the arithmetic is psg_xattn_tile.h's.
  auto run_unit = [&](const XUnit& cur, auto al_tag) {
    constexpr bool AL = decltype(al_tag)::value;
    const int64_t row = cur.row;
    const bool rvalid = cur.rvalid;
    int oi, oj;
    xattn_pair_objects(cur.pidx, N, rcpN, oi, oj);
    const uint32_t* wi = reinterpret_cast<const uint32_t*>(bits_lds + (int64_t)oi * words);
    const uint32_t* wj = reinterpret_cast<const uint32_t*>(bits_lds + (int64_t)oj * words);
    uint32_t needmask;
    bool force_all;
    if (xattn_mask_analysis<AL>(wi, wj, im.NT, policy, needmask, force_all)) {
      // empty union, uniform softmax over the L real keys: out = mean_k V[k]
      const float* mean = reinterpret_cast<const float*>(mean_lds);
      uint16_t* op = out + row * hidden + h * 64 + 4 * hi;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float4 m0 = *reinterpret_cast<const float4*>(mean + 8 * rr + 4 * hi);
        const float4 m1 = *reinterpret_cast<const float4*>(mean + 32 + 8 * rr + 4 * hi);
        uint2 w0, w1;
        w0.x = E::pack(m0.x, m0.y);
        w0.y = E::pack(m0.z, m0.w);
        w1.x = E::pack(m1.x, m1.y);
        w1.y = E::pack(m1.z, m1.w);
        *reinterpret_cast<uint2*>(op + 8 * rr) = w0;
        *reinterpret_cast<uint2*>(op + 32 + 8 * rr) = w1;
      }
      return;
    }
    psg_f32x16 o0 = {0}, o1 = {0};
    float m_run = -INFINITY, l_run = 0.f;
    xattn_key_tiles<E, AL>(cur.qf[0], cur.qf[1], cur.qf[2], cur.qf[3], wi, wj, needmask, force_all, kfrag_base,
                           vfrag_base, im.VS, L, policy, l31, hi, o0, o1, m_run, l_run);
    // epilogue: lane (q, hi) holds O[q][32 dt + (r&3) + 8 (r>>2) + 4 hi]
    if (AL || rvalid) {
      const float inv_l = 1.0f / l_run;
      uint16_t* op = out + row * hidden + h * 64 + 4 * hi;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        uint2 w0, w1;
        w0.x = E::pack(o0[4 * rr] * inv_l, o0[4 * rr + 1] * inv_l);
        w0.y = E::pack(o0[4 * rr + 2] * inv_l, o0[4 * rr + 3] * inv_l);
        w1.x = E::pack(o1[4 * rr] * inv_l, o1[4 * rr + 1] * inv_l);
        w1.y = E::pack(o1[4 * rr + 2] * inv_l, o1[4 * rr + 3] * inv_l);
        *reinterpret_cast<uint2*>(op + 8 * rr) = w0;
        *reinterpret_cast<uint2*>(op + 32 + 8 * rr) = w1;
      }
    }
  };

  int nun = 0;
  auto stamp = [&]() {
    if (tr && lane == 0) {
      if (nun < 28) tr[3 + nun] = __builtin_readcyclecounter();
      ++nun;
      tr[31] = nun;
    }
  };
  // The first units' operands are requested BEFORE the K/V staging: the first touch of Q by 2048 waves at
  // once takes 15-25 us, which now overlaps the staging and the cls unit instead of following them.
  const int64_t tlast = ntile - 1;
  int64_t t = next_tile();
  int64_t tal = t;                     // first pair tile of this wave
  if (aligned) {
    while (tal < NCLS) tal += wstride;
  } else {
    tal = ntile;
  }
  XUnit uf, u0, u1, u2;
  fetch(t < tlast ? t : tlast, uf);
  fetch(tal < tlast ? tal : tlast, u0);
  fetch(tal + wstride < tlast ? tal + wstride : tlast, u1);

  for (int e = threadIdx.x; e < N * words; e += 256) bits_lds[e] = bits[e];
  // ---- stage K_h and V_h^T (once per workgroup) ----
  {
    constexpr int IT = 2 * NC;                           // (Lpad/2 key pairs * 8 chunks) / 256 threads <= 2 NC
    uint4 kv[IT][2], vv[IT][2];
    xattn_kv_load<256, IT>(kv, vv, k, v, tid, L, hidden, h);
    xattn_kv_store<256, IT>(smem, im, kv, vv, tid);
  }
  __syncthreads();
  if (tid < 64) {                                       // pad keys hold zeros: sum over all Lpad slots
    float sum = 0.f;
    const uint16_t* vr = reinterpret_cast<const uint16_t*>(vt_lds + tid * im.VS);
    for (int kk = 0; kk < im.Lpad; kk += 8) {
      const uint4 x = *reinterpret_cast<const uint4*>(vr + kk);
      const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += E::to_f32((uint16_t)(xs[e] & 0xffffu)) + E::to_f32((uint16_t)(xs[e] >> 16));
    }
    reinterpret_cast<float*>(mean_lds)[tid] = sum / (float)L;
  }
  __syncthreads();
  if (tr && lane == 0) tr[1] = __builtin_readcyclecounter();
  if (tr && lane == 0) tr[2] = __builtin_readcyclecounter();
  // Phase 1: tiles with per-row masks (the cls tiles at the head of the order: at most one or two per wave;
  // every tile when nq != 33).
  {
    bool first = true;
    while (t < ntile && t < tal) {
      if (!first) fetch(t, uf);
      first = false;
      run_unit(uf, std::false_type{});
      stamp();
      t = next_tile();
    }
  }
  if (t >= ntile) return;
  // Phase 2: pair tiles.  Three units in flight - one is computed, the operands of the next have been
  // loading for one unit time, the loads of the third are issued now.  The three register sets rotate by
  // unrolling (a copy `a = b` would have to wait for b's loads); fetches are unconditional (tile clamped to
  // the last one) because a branch around them makes the compiler wait for the fresh loads at the join.
  // The compiler's s_waitcnt counts at the loop header are the minimum over the entry edge and the back edge
  // of "memory operations issued after the load".  In steady state 8 output stores sit between two fetches;
  // with fewer operations on the entry edge every unit would wait for the previous unit's stores to be
  // acknowledged.  Volatile (harmless) loads stand in for them.
#pragma unroll
  for (int e = 0; e < 16; ++e) (void)*reinterpret_cast<const volatile int*>(pair_index);
#define XA_STEP(COMPUTE, FILL)                                                  \
  {                                                                             \
    const int64_t t2 = t + 2 * wstride;                                         \
    fetch(t2 < tlast ? t2 : tlast, FILL);                                       \
    run_unit(COMPUTE, std::true_type{});                                        \
    stamp();                                                                    \
    t += wstride;                                                               \
    if (t >= ntile) break;                                                      \
  }
  for (;;) {
    XA_STEP(u0, u2)
    XA_STEP(u1, u0)
    XA_STEP(u2, u1)
  }
#undef XA_STEP
}

template <typename E>
static int xa_v1_launch(psg_ctx* ctx, const void* q, const void* k, const void* v, const uint64_t* bits, int words,
                        const int32_t* pair_index, int N, int P, int L, int nq, int heads, int empty_policy, void* out,
                        hipStream_t st) {
  const size_t lds = xattn_image_bytes(N, words, L);
  PSG_REQUIRE(lds <= 160 * 1024, PSG_ERR_UNSUPPORTED, "psg_qformer_cross_attn: L=%d needs %zu B of LDS (> 160 KiB)", L,
              lds);
  const int NC = (xattn_image(N, words, L).NT + 3) / 4;   // template parameter: staging passes / 128 keys
  PSG_REQUIRE(NC >= 1 && NC <= 4, PSG_ERR_UNSUPPORTED, "psg_qformer_cross_attn: L=%d (MFMA variant handles L <= 512)", L);
  const void* kfn = NC == 1 ? (const void*)cross_attn_mfma_kernel<E, 1>
                  : NC == 2 ? (const void*)cross_attn_mfma_kernel<E, 2>
                  : NC == 3 ? (const void*)cross_attn_mfma_kernel<E, 3> : (const void*)cross_attn_mfma_kernel<E, 4>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      psg_set_error("psg_qformer_cross_attn: hipFuncSetAttribute(%zu): %s", lds, hipGetErrorString(e));
      return PSG_ERR_HIP;
    }
  }
  const int64_t R = (int64_t)P * nq;
  const int64_t ntile = xattn_ntile(P, nq);
  // persistent grid: ~2 workgroups per CU, at least one tile per wave
  int blocks_per_cu = lds * 2 <= 160 * 1024 ? 2 : 1;
  int64_t G = ((int64_t)ctx->num_cu * blocks_per_cu + heads - 1) / heads;
  const int64_t maxG = (ntile + 3) / 4;
  if (G > maxG) G = maxG;
  if (G < 1) G = 1;
  const int64_t trace_n = G * heads * 4 * 32;
  long long* trace = (ctx->trace_kind == PSG_TRACE_CROSS_ATTN && ctx->trace_words >= trace_n) ? ctx->trace : nullptr;
#define XLAUNCH(NC_)                                                                                           \
  cross_attn_mfma_kernel<E, NC_><<<(unsigned)(G * heads), 256, lds, st>>>(                                        \
      (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, bits, words, pair_index, N, R, L, nq, heads, \
      empty_policy, (uint16_t*)out, trace)
  if (NC == 1) XLAUNCH(1);
  else if (NC == 2) XLAUNCH(2);
  else if (NC == 3) XLAUNCH(3);
  else XLAUNCH(4);
#undef XLAUNCH
  PSG_CHECK_LAUNCH("psg_qformer_cross_attn");
  return PSG_OK;
}

extern "C" int psg_qformer_cross_attn(psg_ctx* ctx, const void* q, const void* k, const void* v, const uint64_t* bits,
                                      int words, const int32_t* pair_index, int N, int P, int L, int nq, int heads,
                                      int empty_policy, int variant, void* out, int dtype, void* stream) {
  PSG_REQUIRE(ctx && q && k && v && bits && pair_index && out, PSG_ERR_INVALID, "psg_qformer_cross_attn: NULL argument");
  PSG_REQUIRE(N > 0 && P >= 0 && L > 0 && nq > 0 && heads > 0 && words * 64 >= L, PSG_ERR_INVALID,
              "psg_qformer_cross_attn: N=%d P=%d L=%d nq=%d heads=%d words=%d", N, P, L, nq, heads, words);
  PSG_REQUIRE(empty_policy == PSG_EMPTY_UNIFORM || empty_policy == PSG_EMPTY_UNMASKED, PSG_ERR_INVALID,
              "psg_qformer_cross_attn: empty_policy=%d", empty_policy);
  if (P == 0) return PSG_OK;
  hipStream_t st = (hipStream_t)stream;
  if (variant == PSG_XATTN_SIMPLE)
    return psg_cross_attn_simple_launch(q, k, v, bits, words, pair_index, N, P, L, nq, heads, empty_policy, out, dtype,
                                        st);
  PSG_REQUIRE(variant == PSG_XATTN_MFMA || variant == PSG_XATTN_MFMA_V1, PSG_ERR_INVALID,
              "psg_qformer_cross_attn: variant=%d", variant);
  // fp32 activations: exact f32 matrix instructions over the compacted key list (psg_attn_f32.hip)
  if (dtype == PSG_F32 && variant == PSG_XATTN_MFMA)
    return psg_cross_attn_f32_launch(q, k, v, bits, words, pair_index, N, P, L, nq, heads, empty_policy, out, st);
  PSG_REQUIRE(dtype == PSG_BF16 || dtype == PSG_F16, PSG_ERR_UNSUPPORTED,
              "psg_qformer_cross_attn: PSG_XATTN_MFMA_V1 computes in bf16 / fp16");
  // second-generation kernel (full-line Q / context traffic through LDS-DMA) whenever its LDS image fits
  if (variant == PSG_XATTN_MFMA && ctx->opt.xattn_dma && psg_cross_attn_dma_lds_bytes(N, words, L) <= 160 * 1024 &&
      L <= 384)
    return psg_cross_attn_dma_launch(ctx, q, k, v, bits, words, pair_index, N, P, L, nq, heads, empty_policy, out, dtype,
                                     st, nullptr, nullptr);
  PSG_DISPATCH_E16(dtype, "psg_qformer_cross_attn", return xa_v1_launch<E>(ctx, q, k, v, bits, words, pair_index, N, P, L, nq,
                                                                            heads, empty_policy, out, st));
}


// psg_qformer_cross_attn with the queries stored ONCE PER PROMPT (HF-IB:464-496 over the prompt-deduplicated layer 0):
// q_u [U][33][hidden] = the projected query rows of the U distinct prompts, q_index [P] = the prompt of each pair, q_cls
// [P][hidden] = row 0 of every pair (gathered by the caller: P rows).  Saves the [P x 33][hidden] expansion of q (127 MB
// written and read again at BASELINE C2).  Only the LDS-DMA kernel takes the index: PSG_ERR_UNSUPPORTED when it cannot run
// (fp32, L > 384, LDS image too large, option xattn_dma = 0) - the caller then expands q and calls psg_qformer_cross_attn.
extern "C" int psg_qformer_cross_attn_indexed(psg_ctx* ctx, const void* q_u, const int32_t* q_index, const void* q_cls,
                                              const void* k, const void* v, const uint64_t* bits, int words,
                                              const int32_t* pair_index, int N, int P, int L, int heads, int empty_policy,
                                              void* out, int dtype, void* stream) {
  PSG_REQUIRE(ctx && q_u && q_index && q_cls && k && v && bits && pair_index && out, PSG_ERR_INVALID,
              "psg_qformer_cross_attn_indexed: NULL argument");
  PSG_REQUIRE(N > 0 && P >= 0 && L > 0 && heads > 0 && words * 64 >= L, PSG_ERR_INVALID,
              "psg_qformer_cross_attn_indexed: N=%d P=%d L=%d heads=%d words=%d", N, P, L, heads, words);
  PSG_REQUIRE(empty_policy == PSG_EMPTY_UNIFORM || empty_policy == PSG_EMPTY_UNMASKED, PSG_ERR_INVALID,
              "psg_qformer_cross_attn_indexed: empty_policy=%d", empty_policy);
  PSG_REQUIRE((dtype == PSG_BF16 || dtype == PSG_F16) && ctx->opt.xattn_dma && L <= 384 &&
                  psg_cross_attn_dma_lds_bytes(N, words, L) <= 160 * 1024,
              PSG_ERR_UNSUPPORTED, "psg_qformer_cross_attn_indexed: needs the LDS-DMA kernel (16-bit, L <= 384, image in LDS)");
  if (P == 0) return PSG_OK;
  return psg_cross_attn_dma_launch(ctx, q_u, k, v, bits, words, pair_index, N, P, L, 33, heads, empty_policy, out, dtype,
                                   (hipStream_t)stream, q_index, q_cls);
}
