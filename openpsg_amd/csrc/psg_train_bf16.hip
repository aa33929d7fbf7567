// Training branch in bf16 (train_precision='bf16'): the row / attention entry points of psg_train_bwd.hip for
// activations stored as bf16, in the precision model torch.autocast(bfloat16) gives the reference:
//   * activations that a product, an attention or a pointwise kernel reads (and saves for its backward) are bf16;
//   * the two residual streams (the Q-Former's LayerNorm inputs, the Llama x), the LayerNorm / RMSNorm / softmax
//     statistics and LayerNorm's dgamma / dbeta are fp32;
//   * every kernel computes in fp32 from its bf16 inputs and rounds once (RNE) where it stores bf16.
//
//   psg_train_bf16_layernorm_fwd / _bwd   x fp32 (residual stream) -> y bf16; dy bf16 -> dx fp32, dgamma / dbeta fp32
//   psg_train_bf16_rmsnorm_fwd / _bwd     x fp32 -> y bf16; dy bf16 -> dx fp32 (weight frozen)
//   psg_train_bf16_gelu_fwd / _bwd, psg_train_bf16_silu_mul_fwd / _bwd, psg_train_bf16_rope   bf16 in, bf16 out
//   psg_train_bf16_attn_fwd / _bwd        attention on v_mfma_f32_32x32x16_bf16, keys walked in tiles of 32, the row
//                                         log-sum-exp saved instead of the probabilities; the backward recomputes P
//
// Row and pointwise kernels: the templates of psg_train_rows.h with the TrBf16 access policy - one wave per row, 16-byte
// accesses (8 bf16 / 2 x 4 fp32 per lane and step), hidden % 8 == 0.  Only LayerNorm's dgamma / dbeta kernel is written here.
//
// Attention.  One wave per workgroup.  Every product is computed TRANSPOSED, so that a lane owns one column of the
// 32 x 32 result tile (lane & 31) and 16 of its rows ((r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 0..15):
//   forward / dQ kernel:  S^T = K Q^T, dP^T = V dO^T    a lane owns a QUERY: its softmax statistics are per lane, the
//                                                       two halves of a row meet in one lane ^ 32 exchange
//   dK / dV kernel:       S = Q K^T, dP = dO V^T        a lane owns a KEY: dK^T / dV^T accumulate in its registers over
//                                                       every query tile (and every sequence when the keys are shared)
// Operands that are bf16 in memory (Q, K, V, dO) enter the matrix cores as they are.  P and dS are fp32 values made in
// registers: they enter as hi + lo bf16 pairs (two MFMAs), |p - hi - lo| <= 2^-18 |p|, so the fused attention keeps P
// at fp32 accuracy as far as the result is concerned.  sum_j p_j dP_j is accumulated from the recomputed tiles (a first
// pass of the dQ kernel, handed to the dK / dV kernel in `delta`) rather than taken from the bf16-rounded output.
// Masking as psg_train_attn_fwd: additive finfo(float32).min in fp32; an all-masked row is a uniform softmax.  Its
// log-sum-exp is finfo.min + log(Sk) == finfo.min in fp32: the backward recognises the row by that value and uses 1 / Sk.
#include "psg_train_rows.h"

#define TB_FMIN (-3.4028234663852886e38f)

typedef EBf16::v8 tb_v8;
union TbPack8 {                                   // 8 bf16 = one 16-byte access = one MFMA operand
  uint4 u;
  uint32_t w[4];
  tb_v8 v;
};

// dgamma[c] = sum_rows dy xhat, dbeta[c] = sum_rows dy: one thread per (column, row group), the 16 row groups of a
// column summed in a fixed order - no atomics, the same bits on every run
__global__ void __launch_bounds__(1024) tb_layernorm_dgb_kernel(const float* __restrict__ x, const uint16_t* __restrict__ dy,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                int64_t rows, int hidden, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta) {
  __shared__ float s_g[16][64], s_b[16][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float g = 0.f, b = 0.f;
  if (c < hidden)
    for (int64_t r = rg; r < rows; r += 16) {
      const float d = bf16_to_f32(dy[r * hidden + c]);
      g += d * ((x[r * hidden + c] - mean[r]) * rstd[r]);
      b += d;
    }
  s_g[rg][cl] = g;
  s_b[rg][cl] = b;
  __syncthreads();
  if (rg == 0 && c < hidden) {
    g = 0.f;
    b = 0.f;
    for (int t = 0; t < 16; ++t) {
      g += s_g[t][cl];
      b += s_b[t][cl];
    }
    dgamma[c] = g;
    dbeta[c] = b;
  }
}

#define TB_ALIGNED16(p) ((((uintptr_t)(p)) & 15u) == 0)

// ---- LayerNorm, RMSNorm: x fp32 -> y bf16; dy bf16 -> dx fp32 (psg_train_rows.h at 16-byte accesses) ---------------------
extern "C" int psg_train_bf16_layernorm_fwd(psg_ctx* ctx, const float* x, const float* gamma, const float* beta, float eps,
                                            int64_t rows, int hidden, void* y, float* mean, float* rstd, void* stream) {
  return tr_layernorm_fwd_launch<TrBf16>("psg_train_bf16_layernorm_fwd", ctx, x, gamma, beta, eps, rows, hidden, y, mean, rstd,
                                         stream);
}

extern "C" int psg_train_bf16_layernorm_bwd(psg_ctx* ctx, const float* x, const void* dy, const float* gamma,
                                            const float* mean, const float* rstd, int64_t rows, int hidden, float* dx,
                                            float* dgamma, float* dbeta, void* stream) {
  PSG_REQUIRE(!dgamma == !dbeta, PSG_ERR_INVALID, "psg_train_bf16_layernorm_bwd: bad argument");
  const int rc = tr_layernorm_bwd_launch<TrBf16>("psg_train_bf16_layernorm_bwd", ctx, x, dy, gamma, mean, rstd, rows, hidden, dx,
                                                 nullptr, nullptr, stream);
  if (rc != PSG_OK) return rc;
  if (dgamma) {                                              // written, not accumulated (zero rows: zeros)
    tb_layernorm_dgb_kernel<<<(unsigned)((hidden + 63) / 64), 1024, 0, (hipStream_t)stream>>>(x, (const uint16_t*)dy, mean,
                                                                                             rstd, rows, hidden, dgamma, dbeta);
    PSG_CHECK_LAUNCH("psg_train_bf16_layernorm_bwd (dgamma / dbeta)");
  }
  return PSG_OK;
}

extern "C" int psg_train_bf16_rmsnorm_fwd(psg_ctx* ctx, const float* x, const float* w, float eps, int64_t rows, int hidden,
                                          void* y, float* rstd, void* stream) {
  return tr_rmsnorm_fwd_launch<TrBf16>("psg_train_bf16_rmsnorm_fwd", ctx, x, w, eps, rows, hidden, y, rstd, stream);
}

extern "C" int psg_train_bf16_rmsnorm_bwd(psg_ctx* ctx, const float* x, const void* dy, const float* w, const float* rstd,
                                          int64_t rows, int hidden, float* dx, void* stream) {
  return tr_rmsnorm_bwd_launch<TrBf16>("psg_train_bf16_rmsnorm_bwd", ctx, x, dy, w, rstd, rows, hidden, dx, stream);
}

// ---- element-wise: GELU, SwiGLU gate, rotary: bf16 in, bf16 out (psg_train_rows.h) -----------------------------------------
extern "C" int psg_train_bf16_gelu_fwd(psg_ctx* ctx, const void* x, int64_t n, void* y, void* stream) {
  return tr_gelu_launch<TrBf16>("psg_train_bf16_gelu_fwd", ctx, x, nullptr, false, n, y, stream);
}
extern "C" int psg_train_bf16_gelu_bwd(psg_ctx* ctx, const void* x, const void* dy, int64_t n, void* dx, void* stream) {
  return tr_gelu_launch<TrBf16>("psg_train_bf16_gelu_bwd", ctx, x, dy, true, n, dx, stream);
}

extern "C" int psg_train_bf16_silu_mul_fwd(psg_ctx* ctx, const void* gu, int64_t rows, int inter, void* y, void* stream) {
  return tr_silu_mul_launch<TrBf16>("psg_train_bf16_silu_mul_fwd", ctx, gu, nullptr, false, rows, inter, y, nullptr, stream);
}
extern "C" int psg_train_bf16_silu_mul_bwd(psg_ctx* ctx, const void* gu, const void* dy, int64_t rows, int inter, void* dgu,
                                           void* stream) {
  return tr_silu_mul_launch<TrBf16>("psg_train_bf16_silu_mul_bwd", ctx, gu, dy, true, rows, inter, nullptr, dgu, stream);
}

extern "C" int psg_train_bf16_rope(psg_ctx* ctx, const void* x, const int32_t* pos, const float* rope_cos,
                                   const float* rope_sin, int table_rows, int64_t rows, int heads, int head_dim, float sign,
                                   void* y, void* stream) {
  return tr_rope_launch<TrBf16>("psg_train_bf16_rope", ctx, x, pos, rope_cos, rope_sin, table_rows, rows, heads, head_dim, sign,
                                y, stream);
}

// ---- attention on the matrix cores ---------------------------------------------------------------------------------------
// q / dout / out / dq [B][Sq][H*D], k / v / dk / dv [Bk][Sk][H*D] bf16; keep uint8 [B][Mq][Sk]; drop uint8 [B][H][Sq][Sk] or
// NULL; lse / delta fp32 [B][H][Sq].
__device__ __forceinline__ int tb_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }   // row of result register r

template <int NS>
__device__ __forceinline__ void tb_ld_frag(const uint16_t* p, tb_v8 (&f)[NS]) {   // p: the row's head + 8 (lane >> 5)
#pragma unroll
  for (int s = 0; s < NS; ++s) f[s] = *reinterpret_cast<const tb_v8*>(p + 16 * s);
}
template <int NS>
__device__ __forceinline__ psg_f32x16 tb_dot(const tb_v8 (&a)[NS], const tb_v8 (&b)[NS]) {
  psg_f32x16 c = (psg_f32x16){0};
#pragma unroll
  for (int s = 0; s < NS; ++s) c = EBf16::mfma32(a[s], b[s], c);
  return c;
}
// registers 8 g .. 8 g + 7 of an fp32 result tile as the hi + lo bf16 operand pair of the next product (its k index m of
// half `hi` is the tile row 16 g + tb_row(m, hi): whoever supplies the other operand gathers in that order)
__device__ __forceinline__ void tb_split(const psg_f32x16& t, int g, tb_v8& hi_, tb_v8& lo_) {
  TbPack8 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a = t[8 * g + 2 * e], b = t[8 * g + 2 * e + 1];
    h.w[e] = EBf16::pack(a, b);
    l.w[e] = EBf16::pack(a - __uint_as_float(h.w[e] << 16), b - __uint_as_float(h.w[e] & 0xffff0000u));
  }
  hi_ = h.v;
  lo_ = l.v;
}
// the other operand: column `col` (+ 32 dt) of the 8 rows 16 g + tb_row(m, hi) of a [rows][hid] matrix, rows clamped
template <int NT>
__device__ __forceinline__ void tb_gather_t(const uint16_t* base, int64_t hid, int row0, int nrows, int g, int hi,
                                            tb_v8 (&f)[NT]) {
  uint16_t e[NT][8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    int r = row0 + 16 * g + tb_row(m, hi);
    r = r < nrows ? r : nrows - 1;
    const uint16_t* p = base + (int64_t)r * hid;
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) e[dt][m] = p[32 * dt];
  }
#pragma unroll
  for (int dt = 0; dt < NT; ++dt) {
    TbPack8 t;
#pragma unroll
    for (int w = 0; w < 4; ++w) t.w[w] = (uint32_t)e[dt][2 * w] | ((uint32_t)e[dt][2 * w + 1] << 16);
    f[dt] = t.v;
  }
}
// a lane's 32 x 32 transposed result (its column = row `row` of the output, 16 dims per 32-dim tile) as bf16
template <int NT>
__device__ __forceinline__ void tb_store_t(uint16_t* rowp, int hi, const psg_f32x16 (&o)[NT], float mul) {
#pragma unroll
  for (int dt = 0; dt < NT; ++dt)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      uint2 w;
      w.x = EBf16::pack(o[dt][4 * rr] * mul, o[dt][4 * rr + 1] * mul);
      w.y = EBf16::pack(o[dt][4 * rr + 2] * mul, o[dt][4 * rr + 3] * mul);
      *reinterpret_cast<uint2*>(rowp + 32 * dt + 8 * rr + 4 * hi) = w;
    }
}

template <int D>
__global__ void __launch_bounds__(64)
tb_attn_fwd_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                   const uint8_t* __restrict__ keep, int B, int Bk, int H, int Sq, int Sk, int Mq, float scale,
                   const uint8_t* __restrict__ drop, float drop_scale, uint16_t* __restrict__ out, float* __restrict__ lse) {
  constexpr int NS = D / 16, NT = D / 32;
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int nqt = (Sq + 31) / 32;
  const int qt = blockIdx.x % nqt, h = (blockIdx.x / nqt) % H, b = blockIdx.x / (nqt * H);
  const int64_t hid = (int64_t)H * D;
  const int qrow = qt * 32 + l31, qi = qrow < Sq ? qrow : Sq - 1;
  tb_v8 qf[NS];
  tb_ld_frag<NS>(q + ((int64_t)b * Sq + qi) * hid + h * D + hi * 8, qf);
  const int64_t kvb = (int64_t)(Bk == 1 ? 0 : b) * Sk * hid + h * D;
  const uint8_t* mk = keep + ((int64_t)b * Mq + (Mq == 1 ? 0 : qi)) * Sk;
  const uint8_t* dr = drop ? drop + (((int64_t)b * H + h) * Sq + qi) * Sk : nullptr;
  float m = -INFINITY, l = 0.f;
  psg_f32x16 o[NT];
#pragma unroll
  for (int dt = 0; dt < NT; ++dt) o[dt] = (psg_f32x16){0};
  for (int j0 = 0; j0 < Sk; j0 += 32) {
    const int kj = j0 + l31 < Sk ? j0 + l31 : Sk - 1;
    tb_v8 kf[NS];
    tb_ld_frag<NS>(k + kvb + (int64_t)kj * hid + hi * 8, kf);
    psg_f32x16 sc = tb_dot<NS>(kf, qf);                              // S^T: this lane's query, keys j0 + tb_row(r, hi)
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = j0 + tb_row(r, hi);
      float y = -INFINITY;                                           // past the last key: no part of the row
      if (key < Sk) {
        y = sc[r] * scale;
        if (!mk[key]) y = y + TB_FMIN;                               // additive finfo.min (absorbs the score)
      }
      sc[r] = y;
      tmax = fmaxf(tmax, y);
    }
    const float mn = fmaxf(m, psg_xchg32_max(tmax));                 // finite: a walked tile holds at least one key
    const float alpha = expf(m - mn);
    float ts = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = j0 + tb_row(r, hi);
      const float e = expf(sc[r] - mn);
      ts += e;
      sc[r] = (dr && key < Sk) ? (dr[key] ? e * drop_scale : 0.f) : e;
    }
    l = l * alpha + psg_xchg32_sum(ts);
    m = mn;
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) o[dt] *= alpha;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      tb_v8 ph, pl, vt[NT];
      tb_split(sc, g, ph, pl);
      tb_gather_t<NT>(v + kvb + l31, hid, j0, Sk, g, hi, vt);       // V^T: head dim l31 + 32 dt of the slice's 8 keys
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) {
        o[dt] = EBf16::mfma32(vt[dt], ph, o[dt]);
        o[dt] = EBf16::mfma32(vt[dt], pl, o[dt]);
      }
    }
  }
  if (qrow < Sq) {
    tb_store_t<NT>(out + ((int64_t)b * Sq + qrow) * hid + h * D, hi, o, 1.0f / l);
    if (hi == 0) lse[((int64_t)b * H + h) * Sq + qrow] = m + logf(l);
  }
}

// P and the masked / dropped dP of one tile from the raw products; p is exactly what the forward normalised to
__device__ __forceinline__ float tb_prob(float s, float scale, bool kept, float lse_, float inv_sk) {
  float y = s * scale;
  if (!kept) y = y + TB_FMIN;
  return lse_ == TB_FMIN ? inv_sk : expf(y - lse_);
}

// dQ per query tile; first pass: delta = sum_j p_j dP_j of every row from the recomputed tiles
template <int D>
__global__ void __launch_bounds__(64)
tb_attn_bwd_dq_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                      const uint8_t* __restrict__ keep, const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                      int B, int Bk, int H, int Sq, int Sk, int Mq, float scale, const uint8_t* __restrict__ drop,
                      float drop_scale, uint16_t* __restrict__ dq, float* __restrict__ delta) {
  constexpr int NS = D / 16, NT = D / 32;
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int nqt = (Sq + 31) / 32;
  const int qt = blockIdx.x % nqt, h = (blockIdx.x / nqt) % H, b = blockIdx.x / (nqt * H);
  const int64_t hid = (int64_t)H * D;
  const int qrow = qt * 32 + l31, qi = qrow < Sq ? qrow : Sq - 1;
  tb_v8 qf[NS], dof[NS];
  tb_ld_frag<NS>(q + ((int64_t)b * Sq + qi) * hid + h * D + hi * 8, qf);
  tb_ld_frag<NS>(dout + ((int64_t)b * Sq + qi) * hid + h * D + hi * 8, dof);
  const int64_t kvb = (int64_t)(Bk == 1 ? 0 : b) * Sk * hid + h * D;
  const uint8_t* mk = keep + ((int64_t)b * Mq + (Mq == 1 ? 0 : qi)) * Sk;
  const uint8_t* dr = drop ? drop + (((int64_t)b * H + h) * Sq + qi) * Sk : nullptr;
  const float my_lse = lse[((int64_t)b * H + h) * Sq + qi], inv_sk = 1.0f / (float)Sk;
  float c = 0.f;
  psg_f32x16 acc[NT];
#pragma unroll
  for (int dt = 0; dt < NT; ++dt) acc[dt] = (psg_f32x16){0};
  for (int pass = 0; pass < 2; ++pass) {
    for (int j0 = 0; j0 < Sk; j0 += 32) {
      const int kj = j0 + l31 < Sk ? j0 + l31 : Sk - 1;
      tb_v8 kf[NS], vf[NS];
      tb_ld_frag<NS>(k + kvb + (int64_t)kj * hid + hi * 8, kf);
      tb_ld_frag<NS>(v + kvb + (int64_t)kj * hid + hi * 8, vf);
      psg_f32x16 sc = tb_dot<NS>(kf, qf), dp = tb_dot<NS>(vf, dof);  // S^T, dP^T: this lane's query, keys j0 + tb_row(r, hi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = j0 + tb_row(r, hi), kc = key < Sk ? key : Sk - 1;
        const float p = key < Sk ? tb_prob(sc[r], scale, mk[kc] != 0, my_lse, inv_sk) : 0.f;
        const float d = dr ? (dr[kc] ? dp[r] * drop_scale : 0.f) : dp[r];
        if (pass == 0) c += p * d;
        else sc[r] = p * (d - c) * scale;                            // dS^T
      }
      if (pass == 0) continue;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        tb_v8 sh, sl, kt[NT];
        tb_split(sc, g, sh, sl);
        tb_gather_t<NT>(k + kvb + l31, hid, j0, Sk, g, hi, kt);     // K^T
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) {
          acc[dt] = EBf16::mfma32(kt[dt], sh, acc[dt]);
          acc[dt] = EBf16::mfma32(kt[dt], sl, acc[dt]);
        }
      }
    }
    if (pass == 0) c = psg_xchg32_sum(c);
  }
  if (qrow < Sq) {
    tb_store_t<NT>(dq + ((int64_t)b * Sq + qrow) * hid + h * D, hi, acc, 1.0f);
    if (hi == 0) delta[((int64_t)b * H + h) * Sq + qrow] = c;
  }
}

// dK / dV per (key tile, head, key batch): loops over the query tiles - and over every sequence when the keys are shared -
// in a fixed order, one writer per element
template <int D>
__global__ void __launch_bounds__(64)
tb_attn_bwd_dkv_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                       const uint8_t* __restrict__ keep, const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                       const float* __restrict__ delta, int B, int Bk, int H, int Sq, int Sk, int Mq, float scale,
                       const uint8_t* __restrict__ drop, float drop_scale, uint16_t* __restrict__ dk,
                       uint16_t* __restrict__ dv) {
  constexpr int NS = D / 16, NT = D / 32;
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
  const int nkt = (Sk + 31) / 32;
  const int kt = blockIdx.x % nkt, h = (blockIdx.x / nkt) % H, kb = blockIdx.x / (nkt * H);
  const int64_t hid = (int64_t)H * D;
  const int krow = kt * 32 + l31, kj = krow < Sk ? krow : Sk - 1;
  tb_v8 kf[NS], vf[NS];
  tb_ld_frag<NS>(k + ((int64_t)kb * Sk + kj) * hid + h * D + hi * 8, kf);
  tb_ld_frag<NS>(v + ((int64_t)kb * Sk + kj) * hid + h * D + hi * 8, vf);
  const float inv_sk = 1.0f / (float)Sk;
  psg_f32x16 dka[NT], dva[NT];
#pragma unroll
  for (int dt = 0; dt < NT; ++dt) dka[dt] = dva[dt] = (psg_f32x16){0};
  const int b_lo = Bk == 1 ? 0 : kb, b_hi = Bk == 1 ? B : kb + 1;
  for (int b = b_lo; b < b_hi; ++b) {
    const float* lrow = lse + ((int64_t)b * H + h) * Sq;
    const float* crow = delta + ((int64_t)b * H + h) * Sq;
    const uint16_t* qb = q + (int64_t)b * Sq * hid + h * D;
    const uint16_t* ob = dout + (int64_t)b * Sq * hid + h * D;
    for (int i0 = 0; i0 < Sq; i0 += 32) {
      const int qi = i0 + l31 < Sq ? i0 + l31 : Sq - 1;
      tb_v8 qf[NS], dof[NS];
      tb_ld_frag<NS>(qb + (int64_t)qi * hid + hi * 8, qf);
      tb_ld_frag<NS>(ob + (int64_t)qi * hid + hi * 8, dof);
      psg_f32x16 pd = tb_dot<NS>(qf, kf), ds = tb_dot<NS>(dof, vf);  // S, dP: this lane's key, queries i0 + tb_row(r, hi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = i0 + tb_row(r, hi), ic = i < Sq ? i : Sq - 1;
        const bool kept = keep[((int64_t)b * Mq + (Mq == 1 ? 0 : ic)) * Sk + kj] != 0;
        const float p = i < Sq ? tb_prob(pd[r], scale, kept, lrow[ic], inv_sk) : 0.f;
        const float dm = drop ? (drop[(((int64_t)b * H + h) * Sq + ic) * Sk + kj] ? drop_scale : 0.f) : 1.0f;
        ds[r] = p * (ds[r] * dm - crow[ic]) * scale;                 // dS
        pd[r] = p * dm;                                              // P after the dropout
      }
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        tb_v8 ph, pl, sh, sl, qt[NT], ot[NT];
        tb_split(pd, g, ph, pl);
        tb_split(ds, g, sh, sl);
        tb_gather_t<NT>(ob + l31, hid, i0, Sq, g, hi, ot);          // dO^T
        tb_gather_t<NT>(qb + l31, hid, i0, Sq, g, hi, qt);          // Q^T
#pragma unroll
        for (int dt = 0; dt < NT; ++dt) {
          dva[dt] = EBf16::mfma32(ot[dt], ph, dva[dt]);
          dva[dt] = EBf16::mfma32(ot[dt], pl, dva[dt]);
          dka[dt] = EBf16::mfma32(qt[dt], sh, dka[dt]);
          dka[dt] = EBf16::mfma32(qt[dt], sl, dka[dt]);
        }
      }
    }
  }
  if (krow < Sk) {
    tb_store_t<NT>(dk + ((int64_t)kb * Sk + krow) * hid + h * D, hi, dka, 1.0f);
    tb_store_t<NT>(dv + ((int64_t)kb * Sk + krow) * hid + h * D, hi, dva, 1.0f);
  }
}

static int tb_attn_check(const char* name, int B, int Bk, int H, int Sq, int Sk, int D, int Mq) {
  PSG_REQUIRE(B >= 0 && (Bk == B || Bk == 1) && H > 0 && Sq > 0 && Sk > 0 && (D == 64 || D == 128) && (Mq == 1 || Mq == Sq) &&
                  (int64_t)(B > 0 ? B : 1) * H * ((Sq + 31) / 32) < (1ll << 31) && (int64_t)Bk * H * ((Sk + 31) / 32) < (1ll << 31),
              PSG_ERR_UNSUPPORTED, "%s: B=%d Bk=%d H=%d Sq=%d Sk=%d D=%d Mq=%d (head dims 64 and 128)", name, B, Bk, H, Sq, Sk, D,
              Mq);
  return PSG_OK;
}

extern "C" int psg_train_bf16_attn_fwd(psg_ctx* ctx, const void* q, const void* k, const void* v, const uint8_t* keep, int B,
                                       int Bk, int H, int Sq, int Sk, int D, int Mq, float scale, const uint8_t* drop,
                                       float drop_scale, void* out, float* lse, void* stream) {
  PSG_REQUIRE(ctx && q && k && v && keep && out && lse, PSG_ERR_INVALID, "psg_train_bf16_attn_fwd: NULL argument");
  const int rc = tb_attn_check("psg_train_bf16_attn_fwd", B, Bk, H, Sq, Sk, D, Mq);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(TB_ALIGNED16(q) && TB_ALIGNED16(k) && TB_ALIGNED16(v) && TB_ALIGNED16(out), PSG_ERR_UNSUPPORTED,
              "psg_train_bf16_attn_fwd: q / k / v / out must be 16-byte aligned");
  if (B == 0) return PSG_OK;
  const unsigned grid = (unsigned)(B * H * ((Sq + 31) / 32));
#define TB_FWD(D_)                                                                                                          \
  tb_attn_fwd_kernel<D_><<<grid, 64, 0, (hipStream_t)stream>>>((const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,  \
                                                               keep, B, Bk, H, Sq, Sk, Mq, scale, drop, drop_scale,         \
                                                               (uint16_t*)out, lse)
  if (D == 64) TB_FWD(64);
  else TB_FWD(128);
#undef TB_FWD
  PSG_CHECK_LAUNCH("psg_train_bf16_attn_fwd");
  return PSG_OK;
}

extern "C" int psg_train_bf16_attn_bwd(psg_ctx* ctx, const void* q, const void* k, const void* v, const uint8_t* keep,
                                       const void* dout, const float* lse, int B, int Bk, int H, int Sq, int Sk, int D, int Mq,
                                       float scale, const uint8_t* drop, float drop_scale, void* dq, void* dk, void* dv,
                                       float* delta, void* stream) {
  PSG_REQUIRE(ctx && q && k && v && keep && dout && lse && dq && dk && dv && delta, PSG_ERR_INVALID,
              "psg_train_bf16_attn_bwd: NULL argument");
  const int rc = tb_attn_check("psg_train_bf16_attn_bwd", B, Bk, H, Sq, Sk, D, Mq);
  if (rc != PSG_OK) return rc;
  PSG_REQUIRE(TB_ALIGNED16(q) && TB_ALIGNED16(k) && TB_ALIGNED16(v) && TB_ALIGNED16(dout) && TB_ALIGNED16(dq) &&
                  TB_ALIGNED16(dk) && TB_ALIGNED16(dv),
              PSG_ERR_UNSUPPORTED, "psg_train_bf16_attn_bwd: q / k / v / dout / dq / dk / dv must be 16-byte aligned");
  if (B == 0) return PSG_OK;
  const unsigned gq = (unsigned)(B * H * ((Sq + 31) / 32)), gk = (unsigned)(Bk * H * ((Sk + 31) / 32));
#define TB_BWD(D_)                                                                                                          \
  do {                                                                                                                      \
    tb_attn_bwd_dq_kernel<D_><<<gq, 64, 0, (hipStream_t)stream>>>(                                                          \
        (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, keep, (const uint16_t*)dout, lse, B, Bk, H, Sq, Sk, Mq, \
        scale, drop, drop_scale, (uint16_t*)dq, delta);                                                                     \
    tb_attn_bwd_dkv_kernel<D_><<<gk, 64, 0, (hipStream_t)stream>>>(                                                         \
        (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, keep, (const uint16_t*)dout, lse, delta, B, Bk, H, Sq,  \
        Sk, Mq, scale, drop, drop_scale, (uint16_t*)dk, (uint16_t*)dv);                                                     \
  } while (0)
  if (D == 64) TB_BWD(64);
  else TB_BWD(128);
#undef TB_BWD
  PSG_CHECK_LAUNCH("psg_train_bf16_attn_bwd");
  return PSG_OK;
}
