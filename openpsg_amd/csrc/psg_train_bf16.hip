// Training branch in bf16 (train_precision='bf16'): the row / attention kernels of psg_train_bwd.hip for
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
// Row kernels: one wave per row, 16-byte accesses (8 bf16 / 2 x 4 fp32 per lane and step), hidden % 8 == 0.
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
#include "psg_wave.h"

#define TB_FMIN (-3.4028234663852886e38f)

typedef EBf16::v8 tb_v8;
union TbPack8 {                                   // 8 bf16 = one 16-byte access = one MFMA operand
  uint4 u;
  uint32_t w[4];
  tb_v8 v;
};

__device__ __forceinline__ void tb_ld8(const uint16_t* p, float (&o)[8]) {
  TbPack8 t;
  t.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[2 * e] = __uint_as_float(t.w[e] << 16);
    o[2 * e + 1] = __uint_as_float(t.w[e] & 0xffff0000u);
  }
}
__device__ __forceinline__ void tb_st8(uint16_t* p, const float (&v)[8]) {
  TbPack8 t;
#pragma unroll
  for (int e = 0; e < 4; ++e) t.w[e] = EBf16::pack(v[2 * e], v[2 * e + 1]);
  *reinterpret_cast<uint4*>(p) = t.u;
}
__device__ __forceinline__ void tb_ld8f(const float* p, float (&o)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void tb_st8f(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// ---- LayerNorm: x fp32 -> y bf16 ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tb_layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, int64_t rows,
                                                               int hidden, uint16_t* __restrict__ y, float* __restrict__ mean,
                                                               float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float* xr = x + row * hidden;
  float a[8], s = 0.f;
  for (int c = lane * 8; c < hidden; c += 512) {
    tb_ld8f(xr + c, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += a[e];
  }
  const float mu = wave_sum(s) / (float)hidden;
  float v = 0.f;
  for (int c = lane * 8; c < hidden; c += 512) {
    tb_ld8f(xr + c, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) v += (a[e] - mu) * (a[e] - mu);
  }
  const float rs = 1.0f / sqrtf(wave_sum(v) / (float)hidden + eps);
  for (int c = lane * 8; c < hidden; c += 512) {
    float g[8], b[8], o[8];
    tb_ld8f(xr + c, a);
    tb_ld8f(gamma + c, g);
    tb_ld8f(beta + c, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (a[e] - mu) * rs * g[e] + b[e];
    tb_st8(y + row * hidden + c, o);
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma (dx fp32: the gradient of the residual stream)
__global__ void __launch_bounds__(256) tb_layernorm_bwd_kernel(const float* __restrict__ x, const uint16_t* __restrict__ dy,
                                                               const float* __restrict__ gamma, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, int64_t rows, int hidden,
                                                               float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float mu = mean[row], rs = rstd[row];
  const float* xr = x + row * hidden;
  const uint16_t* dr = dy + row * hidden;
  float xa[8], d[8], g[8], a = 0.f, b = 0.f;
  for (int c = lane * 8; c < hidden; c += 512) {
    tb_ld8f(xr + c, xa);
    tb_ld8(dr + c, d);
    tb_ld8f(gamma + c, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = d[e] * g[e];
      a += t;
      b += t * ((xa[e] - mu) * rs);
    }
  }
  a = wave_sum(a) / (float)hidden;
  b = wave_sum(b) / (float)hidden;
  for (int c = lane * 8; c < hidden; c += 512) {
    float o[8];
    tb_ld8f(xr + c, xa);
    tb_ld8(dr + c, d);
    tb_ld8f(gamma + c, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = rs * (d[e] * g[e] - a - (xa[e] - mu) * rs * b);
    tb_st8f(dx + row * hidden + c, o);
  }
}

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

extern "C" int psg_train_bf16_layernorm_fwd(psg_ctx* ctx, const float* x, const float* gamma, const float* beta, float eps,
                                            int64_t rows, int hidden, void* y, float* mean, float* rstd, void* stream) {
  PSG_REQUIRE(ctx && x && gamma && beta && y && mean && rstd && hidden > 0 && rows >= 0, PSG_ERR_INVALID,
              "psg_train_bf16_layernorm_fwd: bad argument");
  PSG_REQUIRE(hidden % 8 == 0 && TB_ALIGNED16(x) && TB_ALIGNED16(gamma) && TB_ALIGNED16(beta) && TB_ALIGNED16(y),
              PSG_ERR_UNSUPPORTED, "psg_train_bf16_layernorm_fwd: hidden=%d (a multiple of 8, 16-byte aligned rows)", hidden);
  if (rows == 0) return PSG_OK;
  tb_layernorm_fwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, gamma, beta, eps, rows, hidden,
                                                                                      (uint16_t*)y, mean, rstd);
  PSG_CHECK_LAUNCH("psg_train_bf16_layernorm_fwd");
  return PSG_OK;
}

extern "C" int psg_train_bf16_layernorm_bwd(psg_ctx* ctx, const float* x, const void* dy, const float* gamma,
                                            const float* mean, const float* rstd, int64_t rows, int hidden, float* dx,
                                            float* dgamma, float* dbeta, void* stream) {
  PSG_REQUIRE(ctx && x && dy && gamma && mean && rstd && dx && hidden > 0 && rows >= 0 && (!dgamma == !dbeta),
              PSG_ERR_INVALID, "psg_train_bf16_layernorm_bwd: bad argument");
  PSG_REQUIRE(hidden % 8 == 0 && TB_ALIGNED16(x) && TB_ALIGNED16(gamma) && TB_ALIGNED16(dy) && TB_ALIGNED16(dx),
              PSG_ERR_UNSUPPORTED, "psg_train_bf16_layernorm_bwd: hidden=%d (a multiple of 8, 16-byte aligned rows)", hidden);
  if (rows > 0) {
    tb_layernorm_bwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, (const uint16_t*)dy, gamma, mean,
                                                                                        rstd, rows, hidden, dx);
    PSG_CHECK_LAUNCH("psg_train_bf16_layernorm_bwd");
  }
  if (dgamma) {                                              // written, not accumulated (zero rows: zeros)
    tb_layernorm_dgb_kernel<<<(unsigned)((hidden + 63) / 64), 1024, 0, (hipStream_t)stream>>>(x, (const uint16_t*)dy, mean,
                                                                                             rstd, rows, hidden, dgamma, dbeta);
    PSG_CHECK_LAUNCH("psg_train_bf16_layernorm_bwd (dgamma / dbeta)");
  }
  return PSG_OK;
}

// ---- RMSNorm (weight frozen): x fp32 -> y bf16 -------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tb_rmsnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             float eps, int64_t rows, int hidden, uint16_t* __restrict__ y,
                                                             float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float* xr = x + row * hidden;
  float a[8], s = 0.f;
  for (int c = lane * 8; c < hidden; c += 512) {
    tb_ld8f(xr + c, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += a[e] * a[e];
  }
  const float rs = 1.0f / sqrtf(wave_sum(s) / (float)hidden + eps);
  for (int c = lane * 8; c < hidden; c += 512) {
    float g[8], o[8];
    tb_ld8f(xr + c, a);
    tb_ld8f(w + c, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = g[e] * (a[e] * rs);
    tb_st8(y + row * hidden + c, o);
  }
  if (lane == 0) rstd[row] = rs;
}

// y = w x r, r = (mean x^2 + eps)^-1/2:  dx = r (g - x r^2 mean(g x)), g = dy w
__global__ void __launch_bounds__(256) tb_rmsnorm_bwd_kernel(const float* __restrict__ x, const uint16_t* __restrict__ dy,
                                                             const float* __restrict__ w, const float* __restrict__ rstd,
                                                             int64_t rows, int hidden, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float rs = rstd[row];
  const float* xr = x + row * hidden;
  const uint16_t* dr = dy + row * hidden;
  float xa[8], d[8], g[8], a = 0.f;
  for (int c = lane * 8; c < hidden; c += 512) {
    tb_ld8f(xr + c, xa);
    tb_ld8(dr + c, d);
    tb_ld8f(w + c, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) a += d[e] * g[e] * xa[e];
  }
  a = wave_sum(a) / (float)hidden;
  for (int c = lane * 8; c < hidden; c += 512) {
    float o[8];
    tb_ld8f(xr + c, xa);
    tb_ld8(dr + c, d);
    tb_ld8f(w + c, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = rs * (d[e] * g[e] - xa[e] * rs * rs * a);
    tb_st8f(dx + row * hidden + c, o);
  }
}

extern "C" int psg_train_bf16_rmsnorm_fwd(psg_ctx* ctx, const float* x, const float* w, float eps, int64_t rows, int hidden,
                                          void* y, float* rstd, void* stream) {
  PSG_REQUIRE(ctx && x && w && y && rstd && hidden > 0 && rows >= 0, PSG_ERR_INVALID,
              "psg_train_bf16_rmsnorm_fwd: bad argument");
  PSG_REQUIRE(hidden % 8 == 0 && TB_ALIGNED16(x) && TB_ALIGNED16(w) && TB_ALIGNED16(y), PSG_ERR_UNSUPPORTED,
              "psg_train_bf16_rmsnorm_fwd: hidden=%d (a multiple of 8, 16-byte aligned rows)", hidden);
  if (rows == 0) return PSG_OK;
  tb_rmsnorm_fwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, w, eps, rows, hidden, (uint16_t*)y,
                                                                                    rstd);
  PSG_CHECK_LAUNCH("psg_train_bf16_rmsnorm_fwd");
  return PSG_OK;
}

extern "C" int psg_train_bf16_rmsnorm_bwd(psg_ctx* ctx, const float* x, const void* dy, const float* w, const float* rstd,
                                          int64_t rows, int hidden, float* dx, void* stream) {
  PSG_REQUIRE(ctx && x && dy && w && rstd && dx && hidden > 0 && rows >= 0, PSG_ERR_INVALID,
              "psg_train_bf16_rmsnorm_bwd: bad argument");
  PSG_REQUIRE(hidden % 8 == 0 && TB_ALIGNED16(x) && TB_ALIGNED16(w) && TB_ALIGNED16(dy) && TB_ALIGNED16(dx),
              PSG_ERR_UNSUPPORTED, "psg_train_bf16_rmsnorm_bwd: hidden=%d (a multiple of 8, 16-byte aligned rows)", hidden);
  if (rows == 0) return PSG_OK;
  tb_rmsnorm_bwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, (const uint16_t*)dy, w, rstd, rows,
                                                                                    hidden, dx);
  PSG_CHECK_LAUNCH("psg_train_bf16_rmsnorm_bwd");
  return PSG_OK;
}

// ---- element-wise: GELU, SwiGLU gate, rotary (8 bf16 per thread) -------------------------------------------------------
__global__ void tb_gelu_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, int64_t n8,
                               uint16_t* __restrict__ o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  float v[8], d[8], r[8];
  tb_ld8(x + i * 8, v);
  if (dy) tb_ld8(dy + i * 8, d);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float cdf = 0.5f * (1.0f + erff(v[e] * 0.70710678118654752f));
    r[e] = dy ? d[e] * (cdf + v[e] * 0.3989422804014327f * expf(-0.5f * v[e] * v[e])) : v[e] * cdf;
  }
  tb_st8(o + i * 8, r);
}

static int tb_gelu_launch(const char* name, psg_ctx* ctx, const void* x, const void* dy, bool bwd, int64_t n, void* o,
                          void* stream) {
  PSG_REQUIRE(ctx && x && o && (!bwd || dy) && n >= 0, PSG_ERR_INVALID, "%s: bad argument", name);
  PSG_REQUIRE(n % 8 == 0 && TB_ALIGNED16(x) && TB_ALIGNED16(o) && TB_ALIGNED16(dy), PSG_ERR_UNSUPPORTED,
              "%s: n=%lld (a multiple of 8, 16-byte aligned)", name, (long long)n);
  if (n == 0) return PSG_OK;
  tb_gelu_kernel<<<(unsigned)((n / 8 + 255) / 256), 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, (const uint16_t*)dy,
                                                                                  n / 8, (uint16_t*)o);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

extern "C" int psg_train_bf16_gelu_fwd(psg_ctx* ctx, const void* x, int64_t n, void* y, void* stream) {
  return tb_gelu_launch("psg_train_bf16_gelu_fwd", ctx, x, nullptr, false, n, y, stream);
}
extern "C" int psg_train_bf16_gelu_bwd(psg_ctx* ctx, const void* x, const void* dy, int64_t n, void* dx, void* stream) {
  return tb_gelu_launch("psg_train_bf16_gelu_bwd", ctx, x, dy, true, n, dx, stream);
}

// gu [rows][2 * inter] = gate | up; y = silu(gate) * up
__global__ void tb_silu_mul_kernel(const uint16_t* __restrict__ gu, const uint16_t* __restrict__ dy, int64_t rows, int inter,
                                   uint16_t* __restrict__ y, uint16_t* __restrict__ dgu) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = inter / 8;
  if (i >= rows * per) return;
  const int64_t r = i / per;
  const int c = (int)(i % per) * 8;
  float g[8], u[8], d[8], a[8], b[8];
  tb_ld8(gu + r * 2 * inter + c, g);
  tb_ld8(gu + r * 2 * inter + inter + c, u);
  if (dy) tb_ld8(dy + r * inter + c, d);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float sg = 1.0f / (1.0f + expf(-g[e]));
    if (!dy) {
      a[e] = g[e] * sg * u[e];
    } else {
      a[e] = d[e] * u[e] * sg * (1.0f + g[e] * (1.0f - sg));
      b[e] = d[e] * g[e] * sg;
    }
  }
  if (!dy) {
    tb_st8(y + r * inter + c, a);
  } else {
    tb_st8(dgu + r * 2 * inter + c, a);
    tb_st8(dgu + r * 2 * inter + inter + c, b);
  }
}

static int tb_silu_launch(const char* name, psg_ctx* ctx, const void* gu, const void* dy, bool bwd, int64_t rows, int inter,
                          void* y, void* dgu, void* stream) {
  PSG_REQUIRE(ctx && gu && (bwd ? (dy && dgu) : (y != nullptr)) && inter > 0 && rows >= 0, PSG_ERR_INVALID,
              "%s: bad argument", name);
  PSG_REQUIRE(inter % 8 == 0 && TB_ALIGNED16(gu) && TB_ALIGNED16(dy) && TB_ALIGNED16(y) && TB_ALIGNED16(dgu),
              PSG_ERR_UNSUPPORTED, "%s: inter=%d (a multiple of 8, 16-byte aligned rows)", name, inter);
  if (rows == 0) return PSG_OK;
  const int64_t n = rows * (inter / 8);
  tb_silu_mul_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>((const uint16_t*)gu, (const uint16_t*)dy,
                                                                                  rows, inter, (uint16_t*)y, (uint16_t*)dgu);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

extern "C" int psg_train_bf16_silu_mul_fwd(psg_ctx* ctx, const void* gu, int64_t rows, int inter, void* y, void* stream) {
  return tb_silu_launch("psg_train_bf16_silu_mul_fwd", ctx, gu, nullptr, false, rows, inter, y, nullptr, stream);
}
extern "C" int psg_train_bf16_silu_mul_bwd(psg_ctx* ctx, const void* gu, const void* dy, int64_t rows, int inter, void* dgu,
                                           void* stream) {
  return tb_silu_launch("psg_train_bf16_silu_mul_bwd", ctx, gu, dy, true, rows, inter, nullptr, dgu, stream);
}

// x [rows][heads * head_dim] bf16, pos int32 [rows], cos / sin fp32 [table_rows][head_dim / 2]:
// y = x cos + rotate_half(x) sin * sign (sign = -1: the adjoint).  A thread rotates 8 dims of the first half with their
// partners in the second.
__global__ void tb_rope_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ pos, const float* __restrict__ cs,
                               const float* __restrict__ sn, int table_rows, int64_t rows, int heads, int head_dim,
                               float sign, uint16_t* __restrict__ y) {
  const int half = head_dim / 2, per = half / 8;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * heads * per) return;
  const int d = (int)(i % per) * 8;
  const int h = (int)((i / per) % heads);
  const int64_t r = i / ((int64_t)per * heads);
  const int64_t base = (r * heads + h) * head_dim;
  int pr = pos[r];
  pr = pr < 0 ? 0 : (pr >= table_rows ? table_rows - 1 : pr);   // never read outside the tables (RopeFn checks the range)
  float c[8], s[8], a[8], b[8], oa[8], ob[8];
  tb_ld8f(cs + (int64_t)pr * half + d, c);
  tb_ld8f(sn + (int64_t)pr * half + d, s);
  tb_ld8(x + base + d, a);
  tb_ld8(x + base + d + half, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    oa[e] = a[e] * c[e] - b[e] * (s[e] * sign);                 // rotate_half(x) = [-x2, x1]
    ob[e] = b[e] * c[e] + a[e] * (s[e] * sign);
  }
  tb_st8(y + base + d, oa);
  tb_st8(y + base + d + half, ob);
}

extern "C" int psg_train_bf16_rope(psg_ctx* ctx, const void* x, const int32_t* pos, const float* rope_cos,
                                   const float* rope_sin, int table_rows, int64_t rows, int heads, int head_dim, float sign,
                                   void* y, void* stream) {
  PSG_REQUIRE(ctx && x && pos && rope_cos && rope_sin && y && heads > 0 && head_dim > 0 && table_rows > 0 && rows >= 0,
              PSG_ERR_INVALID, "psg_train_bf16_rope: bad argument");
  PSG_REQUIRE(head_dim % 16 == 0 && TB_ALIGNED16(x) && TB_ALIGNED16(y) && TB_ALIGNED16(rope_cos) && TB_ALIGNED16(rope_sin),
              PSG_ERR_UNSUPPORTED, "psg_train_bf16_rope: head_dim=%d (a multiple of 16, 16-byte aligned rows)", head_dim);
  if (rows == 0) return PSG_OK;
  const int64_t n = rows * heads * (head_dim / 16);
  tb_rope_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, pos, rope_cos, rope_sin,
                                                                              table_rows, rows, heads, head_dim, sign,
                                                                              (uint16_t*)y);
  PSG_CHECK_LAUNCH("psg_train_bf16_rope");
  return PSG_OK;
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
