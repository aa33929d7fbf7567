// Row and pointwise kernels of the training branch, written once for both precisions of the gradient path:
// LayerNorm and RMSNorm forward and dx, GELU, the SwiGLU gate and rotary.  Every kernel computes in fp32; an access
// policy F says how a lane reaches memory and what an activation is:
//   TrF32   one float per access, fp32 activations: any length, no alignment requirement (psg_train_*)
//   TrBf16  16-byte accesses (8 bf16 / 2 x 4 fp32 per lane and step), bf16 activations rounded once (RNE) where they are
//           stored: lengths a multiple of 8, 16-byte aligned rows (psg_train_bf16_*)
// The residual streams the norms read and write (x, dx), gamma / beta / w, the statistics and the rotary tables are
// fp32 in both.  The extern "C" entry points stay in psg_train_bwd.hip and psg_train_bf16.hip, one launcher call each.
#pragma once
#include "psg_wave.h"

struct TrF32 {
  static constexpr int W = 1;                  // elements a lane moves per access
  static constexpr bool DGB_ATOMIC = true;     // LayerNorm's dgamma / dbeta: added by the dx kernel into zeroed buffers
  typedef float act_t;
  static __device__ __forceinline__ void ldf(const float* p, float (&o)[1]) { o[0] = *p; }
  static __device__ __forceinline__ void stf(float* p, const float (&v)[1]) { *p = v[0]; }
  static __device__ __forceinline__ void lda(const float* p, float (&o)[1]) { o[0] = *p; }
  static __device__ __forceinline__ void sta(float* p, const float (&v)[1]) { *p = v[0]; }
};

struct TrBf16 {
  static constexpr int W = 8;
  static constexpr bool DGB_ATOMIC = false;    // written in a fixed order by tb_layernorm_dgb_kernel
  typedef uint16_t act_t;
  static __device__ __forceinline__ void ldf(const float* p, float (&o)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
  static __device__ __forceinline__ void stf(float* p, const float (&v)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  static __device__ __forceinline__ void lda(const uint16_t* p, float (&o)[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[2 * e] = __uint_as_float(w[e] << 16);
      o[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void sta(uint16_t* p, const float (&v)[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(EBf16::pack(v[0], v[1]), EBf16::pack(v[2], v[3]), EBf16::pack(v[4], v[5]),
                                              EBf16::pack(v[6], v[7]));
  }
};

// the pointers a W-wide access goes through lie on 16 bytes (NULL passes); nothing to ask at W = 1
template <class F, class... P>
static inline bool tr_aligned(P... p) {
  return F::W == 1 || ((... | (uintptr_t)p) & 15u) == 0;
}

// ---- LayerNorm: one wave per row ---------------------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(256) tr_layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, int64_t rows,
                                                               int hidden, typename F::act_t* __restrict__ y,
                                                               float* __restrict__ mean, float* __restrict__ rstd) {
  constexpr int W = F::W;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float* xr = x + row * hidden;
  float a[W], s = 0.f;
  for (int c = lane * W; c < hidden; c += 64 * W) {
    F::ldf(xr + c, a);
#pragma unroll
    for (int e = 0; e < W; ++e) s += a[e];
  }
  const float mu = wave_sum(s) / (float)hidden;
  float v = 0.f;
  for (int c = lane * W; c < hidden; c += 64 * W) {
    F::ldf(xr + c, a);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float d = a[e] - mu;
      v += d * d;
    }
  }
  const float rs = 1.0f / sqrtf(wave_sum(v) / (float)hidden + eps);
  for (int c = lane * W; c < hidden; c += 64 * W) {
    float g[W], b[W], o[W];
    F::ldf(xr + c, a);
    F::ldf(gamma + c, g);
    F::ldf(beta + c, b);
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = (a[e] - mu) * rs * g[e] + b[e];
    F::sta(y + row * hidden + c, o);
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma (dx fp32: the gradient of the residual stream);
// DGB_ATOMIC: dgamma += dy * xhat, dbeta += dy (atomics)
template <class F>
__global__ void __launch_bounds__(256) tr_layernorm_bwd_kernel(const float* __restrict__ x,
                                                               const typename F::act_t* __restrict__ dy,
                                                               const float* __restrict__ gamma, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, int64_t rows, int hidden,
                                                               float* __restrict__ dx, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
  constexpr int W = F::W;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float mu = mean[row], rs = rstd[row];
  const float* xr = x + row * hidden;
  const typename F::act_t* dr = dy + row * hidden;
  float xa[W], d[W], ga[W], a = 0.f, b = 0.f;
  for (int c = lane * W; c < hidden; c += 64 * W) {
    F::ldf(xr + c, xa);
    F::lda(dr + c, d);
    F::ldf(gamma + c, ga);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float g = d[e] * ga[e], xh = (xa[e] - mu) * rs;
      a += g;
      b += g * xh;
    }
  }
  a = wave_sum(a) / (float)hidden;
  b = wave_sum(b) / (float)hidden;
  for (int c = lane * W; c < hidden; c += 64 * W) {
    float o[W];
    F::ldf(xr + c, xa);
    F::lda(dr + c, d);
    F::ldf(gamma + c, ga);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float xh = (xa[e] - mu) * rs;
      o[e] = rs * (d[e] * ga[e] - a - xh * b);
      if constexpr (F::DGB_ATOMIC) {
        if (dgamma) atomicAdd(dgamma + c + e, d[e] * xh);
        if (dbeta) atomicAdd(dbeta + c + e, d[e]);
      }
    }
    F::stf(dx + row * hidden + c, o);
  }
}

template <class F>
static int tr_layernorm_fwd_launch(const char* name, psg_ctx* ctx, const float* x, const float* gamma, const float* beta,
                                   float eps, int64_t rows, int hidden, void* y, float* mean, float* rstd, void* stream) {
  PSG_REQUIRE(ctx && x && gamma && beta && y && mean && rstd && hidden > 0 && rows >= 0, PSG_ERR_INVALID, "%s: bad argument",
              name);
  PSG_REQUIRE(hidden % F::W == 0 && tr_aligned<F>(x, gamma, beta, y), PSG_ERR_UNSUPPORTED,
              "%s: hidden=%d (a multiple of %d, 16-byte aligned rows)", name, hidden, F::W);
  if (rows == 0) return PSG_OK;
  tr_layernorm_fwd_kernel<F><<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      x, gamma, beta, eps, rows, hidden, (typename F::act_t*)y, mean, rstd);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

// dgamma / dbeta: DGB_ATOMIC only (each may be NULL), into buffers handed in zeroed
template <class F>
static int tr_layernorm_bwd_launch(const char* name, psg_ctx* ctx, const float* x, const void* dy, const float* gamma,
                                   const float* mean, const float* rstd, int64_t rows, int hidden, float* dx, float* dgamma,
                                   float* dbeta, void* stream) {
  PSG_REQUIRE(ctx && x && dy && gamma && mean && rstd && dx && hidden > 0 && rows >= 0, PSG_ERR_INVALID, "%s: bad argument",
              name);
  PSG_REQUIRE(hidden % F::W == 0 && tr_aligned<F>(x, gamma, dy, dx), PSG_ERR_UNSUPPORTED,
              "%s: hidden=%d (a multiple of %d, 16-byte aligned rows)", name, hidden, F::W);
  if (rows == 0) return PSG_OK;
  tr_layernorm_bwd_kernel<F><<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      x, (const typename F::act_t*)dy, gamma, mean, rstd, rows, hidden, dx, dgamma, dbeta);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

// ---- RMSNorm (weight frozen: no weight gradient) -------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(256) tr_rmsnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             float eps, int64_t rows, int hidden,
                                                             typename F::act_t* __restrict__ y, float* __restrict__ rstd) {
  constexpr int W = F::W;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float* xr = x + row * hidden;
  float a[W], s = 0.f;
  for (int c = lane * W; c < hidden; c += 64 * W) {
    F::ldf(xr + c, a);
#pragma unroll
    for (int e = 0; e < W; ++e) s += a[e] * a[e];
  }
  const float rs = 1.0f / sqrtf(wave_sum(s) / (float)hidden + eps);
  for (int c = lane * W; c < hidden; c += 64 * W) {
    float g[W], o[W];
    F::ldf(xr + c, a);
    F::ldf(w + c, g);
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = g[e] * (a[e] * rs);
    F::sta(y + row * hidden + c, o);
  }
  if (lane == 0) rstd[row] = rs;
}

// y = w x r, r = (mean x^2 + eps)^-1/2:  dx = r (g - x r^2 mean(g x)), g = dy w
template <class F>
__global__ void __launch_bounds__(256) tr_rmsnorm_bwd_kernel(const float* __restrict__ x,
                                                             const typename F::act_t* __restrict__ dy,
                                                             const float* __restrict__ w, const float* __restrict__ rstd,
                                                             int64_t rows, int hidden, float* __restrict__ dx) {
  constexpr int W = F::W;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= rows) return;
  const float rs = rstd[row];
  const float* xr = x + row * hidden;
  const typename F::act_t* dr = dy + row * hidden;
  float xa[W], d[W], g[W], a = 0.f;
  for (int c = lane * W; c < hidden; c += 64 * W) {
    F::ldf(xr + c, xa);
    F::lda(dr + c, d);
    F::ldf(w + c, g);
#pragma unroll
    for (int e = 0; e < W; ++e) a += d[e] * g[e] * xa[e];
  }
  a = wave_sum(a) / (float)hidden;
  for (int c = lane * W; c < hidden; c += 64 * W) {
    float o[W];
    F::ldf(xr + c, xa);
    F::lda(dr + c, d);
    F::ldf(w + c, g);
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = rs * (d[e] * g[e] - xa[e] * rs * rs * a);
    F::stf(dx + row * hidden + c, o);
  }
}

template <class F>
static int tr_rmsnorm_fwd_launch(const char* name, psg_ctx* ctx, const float* x, const float* w, float eps, int64_t rows,
                                 int hidden, void* y, float* rstd, void* stream) {
  PSG_REQUIRE(ctx && x && w && y && rstd && hidden > 0 && rows >= 0, PSG_ERR_INVALID, "%s: bad argument", name);
  PSG_REQUIRE(hidden % F::W == 0 && tr_aligned<F>(x, w, y), PSG_ERR_UNSUPPORTED,
              "%s: hidden=%d (a multiple of %d, 16-byte aligned rows)", name, hidden, F::W);
  if (rows == 0) return PSG_OK;
  tr_rmsnorm_fwd_kernel<F><<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, w, eps, rows, hidden,
                                                                                       (typename F::act_t*)y, rstd);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

template <class F>
static int tr_rmsnorm_bwd_launch(const char* name, psg_ctx* ctx, const float* x, const void* dy, const float* w,
                                 const float* rstd, int64_t rows, int hidden, float* dx, void* stream) {
  PSG_REQUIRE(ctx && x && dy && w && rstd && dx && hidden > 0 && rows >= 0, PSG_ERR_INVALID, "%s: bad argument", name);
  PSG_REQUIRE(hidden % F::W == 0 && tr_aligned<F>(x, w, dy, dx), PSG_ERR_UNSUPPORTED,
              "%s: hidden=%d (a multiple of %d, 16-byte aligned rows)", name, hidden, F::W);
  if (rows == 0) return PSG_OK;
  tr_rmsnorm_bwd_kernel<F><<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(
      x, (const typename F::act_t*)dy, w, rstd, rows, hidden, dx);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

// ---- element-wise: GELU, SwiGLU gate, rotary (W elements per thread) -----------------------------------------------------
// exact-erf GELU; dy != NULL: its backward, d/dx [x Phi(x)] = Phi + x phi
template <class F>
__global__ void tr_gelu_kernel(const typename F::act_t* __restrict__ x, const typename F::act_t* __restrict__ dy,
                               int64_t items, typename F::act_t* __restrict__ o) {
  constexpr int W = F::W;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= items) return;
  float v[W], d[W], r[W];
  F::lda(x + i * W, v);
  if (dy) F::lda(dy + i * W, d);
#pragma unroll
  for (int e = 0; e < W; ++e) {
    const float cdf = 0.5f * (1.0f + erff(v[e] * 0.70710678118654752f));
    if (dy) r[e] = d[e] * (cdf + v[e] * 0.3989422804014327f * expf(-0.5f * v[e] * v[e]));
    else r[e] = v[e] * cdf;
  }
  F::sta(o + i * W, r);
}

template <class F>
static int tr_gelu_launch(const char* name, psg_ctx* ctx, const void* x, const void* dy, bool bwd, int64_t n, void* o,
                          void* stream) {
  PSG_REQUIRE(ctx && x && o && (!bwd || dy) && n >= 0, PSG_ERR_INVALID, "%s: bad argument", name);
  PSG_REQUIRE(n % F::W == 0 && tr_aligned<F>(x, o, dy), PSG_ERR_UNSUPPORTED, "%s: n=%lld (a multiple of %d, 16-byte aligned)",
              name, (long long)n, F::W);
  if (n == 0) return PSG_OK;
  tr_gelu_kernel<F><<<(unsigned)((n / F::W + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const typename F::act_t*)x, (const typename F::act_t*)dy, n / F::W, (typename F::act_t*)o);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

// gu [rows][2 * inter] = gate | up; y = silu(gate) * up; dy != NULL: the backward into dgu
template <class F>
__global__ void tr_silu_mul_kernel(const typename F::act_t* __restrict__ gu, const typename F::act_t* __restrict__ dy,
                                   int64_t rows, int inter, typename F::act_t* __restrict__ y,
                                   typename F::act_t* __restrict__ dgu) {
  constexpr int W = F::W;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = inter / W;
  if (i >= rows * per) return;
  const int64_t r = i / per;
  const int c = (int)(i % per) * W;
  float g[W], u[W], d[W], a[W], b[W];
  F::lda(gu + r * 2 * inter + c, g);
  F::lda(gu + r * 2 * inter + inter + c, u);
  if (dy) F::lda(dy + i * W, d);
#pragma unroll
  for (int e = 0; e < W; ++e) {
    const float sg = 1.0f / (1.0f + expf(-g[e]));
    if (!dy) {
      a[e] = g[e] * sg * u[e];
    } else {
      a[e] = d[e] * u[e] * sg * (1.0f + g[e] * (1.0f - sg));
      b[e] = d[e] * g[e] * sg;
    }
  }
  if (!dy) {
    F::sta(y + i * W, a);
  } else {
    F::sta(dgu + r * 2 * inter + c, a);
    F::sta(dgu + r * 2 * inter + inter + c, b);
  }
}

template <class F>
static int tr_silu_mul_launch(const char* name, psg_ctx* ctx, const void* gu, const void* dy, bool bwd, int64_t rows,
                              int inter, void* y, void* dgu, void* stream) {
  PSG_REQUIRE(ctx && gu && (bwd ? (dy && dgu) : (y != nullptr)) && inter > 0 && rows >= 0, PSG_ERR_INVALID, "%s: bad argument",
              name);
  PSG_REQUIRE(inter % F::W == 0 && tr_aligned<F>(gu, dy, y, dgu), PSG_ERR_UNSUPPORTED,
              "%s: inter=%d (a multiple of %d, 16-byte aligned rows)", name, inter, F::W);
  if (rows == 0) return PSG_OK;
  const int64_t n = rows * (inter / F::W);
  tr_silu_mul_kernel<F><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const typename F::act_t*)gu, (const typename F::act_t*)dy, rows, inter, (typename F::act_t*)y, (typename F::act_t*)dgu);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}

// x [rows][heads * head_dim], pos int32 [rows] (row of the fp32 cos / sin tables [table_rows][head_dim / 2]):
// y = x cos + rotate_half(x) sin * sign.  sign = +1: HF-LL:130-160; sign = -1: its adjoint (the rotation by -angle).
// A thread rotates W dims of the first half with their partners in the second.
template <class F>
__global__ void tr_rope_kernel(const typename F::act_t* __restrict__ x, const int32_t* __restrict__ pos,
                               const float* __restrict__ cs, const float* __restrict__ sn, int table_rows, int64_t rows,
                               int heads, int head_dim, float sign, typename F::act_t* __restrict__ y) {
  constexpr int W = F::W;
  const int half = head_dim / 2, per = half / W;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * heads * per) return;
  const int d = (int)(i % per) * W;
  const int h = (int)((i / per) % heads);
  const int64_t r = i / ((int64_t)per * heads);
  const int64_t base = (r * heads + h) * head_dim;
  int pr = pos[r];
  pr = pr < 0 ? 0 : (pr >= table_rows ? table_rows - 1 : pr);   // never read outside the tables (RopeFn checks the range)
  float c[W], s[W], a[W], b[W], oa[W], ob[W];
  F::ldf(cs + (int64_t)pr * half + d, c);
  F::ldf(sn + (int64_t)pr * half + d, s);
  F::lda(x + base + d, a);
  F::lda(x + base + d + half, b);
#pragma unroll
  for (int e = 0; e < W; ++e) {
    oa[e] = a[e] * c[e] - b[e] * (s[e] * sign);                 // rotate_half(x) = [-x2, x1]
    ob[e] = b[e] * c[e] + a[e] * (s[e] * sign);
  }
  F::sta(y + base + d, oa);
  F::sta(y + base + d + half, ob);
}

// an odd head_dim is PSG_ERR_INVALID; one whose halves W does not divide (W > 1) is PSG_ERR_UNSUPPORTED
template <class F>
static int tr_rope_launch(const char* name, psg_ctx* ctx, const void* x, const int32_t* pos, const float* rope_cos,
                          const float* rope_sin, int table_rows, int64_t rows, int heads, int head_dim, float sign, void* y,
                          void* stream) {
  PSG_REQUIRE(ctx && x && pos && rope_cos && rope_sin && y && heads > 0 && head_dim > 0 && table_rows > 0 && rows >= 0,
              PSG_ERR_INVALID, "%s: bad argument", name);
  PSG_REQUIRE((F::W == 1 || head_dim % (2 * F::W) == 0) && tr_aligned<F>(x, y, rope_cos, rope_sin), PSG_ERR_UNSUPPORTED,
              "%s: head_dim=%d (a multiple of %d, 16-byte aligned rows)", name, head_dim, 2 * F::W);
  PSG_REQUIRE(head_dim % 2 == 0, PSG_ERR_INVALID, "%s: head_dim=%d is odd", name, head_dim);
  if (rows == 0) return PSG_OK;
  const int64_t n = rows * heads * (head_dim / (2 * F::W));
  tr_rope_kernel<F><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (const typename F::act_t*)x, pos, rope_cos, rope_sin, table_rows, rows, heads, head_dim, sign, (typename F::act_t*)y);
  PSG_CHECK_LAUNCH(name);
  return PSG_OK;
}
