// SURVEY 8f rank 3, gradient path: the row / attention kernels of the TRAINING branch of RelationTransformerHeadV4 with
// their backward counterparts (the reference back-propagates binary_rel_cls_loss and rel_llm_loss, V4:327-351, 463-482,
// driven by tools/train.py:239-246; the LLM is frozen, CFG:65, so its weights need no gradient but its activations do:
// the loss reaches language_projection and the Q-Former THROUGH the 32 Llama layers).
//
// Training batches are tiny (<= 32 sampled pairs through the Q-Former, V4:29-30; <= 4 pairs through the LLM, V4:38),
// so these are plain fp32 kernels - one wave per row or per (sequence, head, query row) - written for exactness against
// autograd on the CPU oracle, not for speed; the dense projections and their weight gradients go through the library
// GEMM.  Every kernel is the exact adjoint of the forward kernel next to it.  The norms, GELU, the SwiGLU gate and rotary
// are the templates of psg_train_rows.h with the TrF32 access policy (one float per access; the bf16 path of
// psg_train_bf16.hip instantiates the same templates); the attention and the losses are written here:
//
//   psg_train_layernorm_fwd / _bwd     HF-IB LayerNorm (eps 1e-12): y = (x - mean) * rstd * gamma + beta
//   psg_train_rmsnorm_fwd / _bwd       HF-LL:53-67 (weight frozen: no weight gradient)
//   psg_train_attn_fwd / _bwd          softmax(q.k * scale + additive mask) v for Q-Former self- / cross-attention
//                                      (HF-IB:176-196, keys / values shared by all sequences when Bk == 1) and the Llama
//                                      attention (HF-LL:191-214); an all-masked row is a uniform softmax, and its score
//                                      gradient is p (dP - sum p dP) like any other row - what autograd computes for the
//                                      reference's additive finfo.min masks
//   psg_train_gelu_fwd / _bwd          exact-erf GELU (HF-IB:563-577)
//   psg_train_silu_mul_fwd / _bwd      SwiGLU gate (HF-LL:163-177)
//   psg_train_rope                     half-split rotary (HF-LL:130-160); sign = -1 is its adjoint
//   psg_train_ce_bwd / psg_train_bce_bwd   gradients of psg_cross_entropy_rows / psg_bce_with_logits
//   psg_train_mlcce_fwd / _bwd         multilabel categorical cross entropy of the multiclass head (V4:484-495)
#include "psg_train_rows.h"

#define TR_FMIN (-3.4028234663852886e38f)

// ---- LayerNorm, RMSNorm (psg_train_rows.h at one float per access) ------------------------------------------------------
// dgamma / dbeta (each may be NULL) are accumulated by atomics: the caller hands them in zeroed
extern "C" int psg_train_layernorm_fwd(psg_ctx* ctx, const float* x, const float* gamma, const float* beta, float eps,
                                       int64_t rows, int hidden, float* y, float* mean, float* rstd, void* stream) {
  return tr_layernorm_fwd_launch<TrF32>("psg_train_layernorm_fwd", ctx, x, gamma, beta, eps, rows, hidden, y, mean, rstd, stream);
}

extern "C" int psg_train_layernorm_bwd(psg_ctx* ctx, const float* x, const float* dy, const float* gamma, const float* mean,
                                       const float* rstd, int64_t rows, int hidden, float* dx, float* dgamma, float* dbeta,
                                       void* stream) {
  return tr_layernorm_bwd_launch<TrF32>("psg_train_layernorm_bwd", ctx, x, dy, gamma, mean, rstd, rows, hidden, dx, dgamma,
                                        dbeta, stream);
}

extern "C" int psg_train_rmsnorm_fwd(psg_ctx* ctx, const float* x, const float* w, float eps, int64_t rows, int hidden,
                                     float* y, float* rstd, void* stream) {
  return tr_rmsnorm_fwd_launch<TrF32>("psg_train_rmsnorm_fwd", ctx, x, w, eps, rows, hidden, y, rstd, stream);
}

extern "C" int psg_train_rmsnorm_bwd(psg_ctx* ctx, const float* x, const float* dy, const float* w, const float* rstd,
                                     int64_t rows, int hidden, float* dx, void* stream) {
  return tr_rmsnorm_bwd_launch<TrF32>("psg_train_rmsnorm_bwd", ctx, x, dy, w, rstd, rows, hidden, dx, stream);
}

// ---- attention -------------------------------------------------------------------------------------------------------
// q [B][Sq][H*D], k / v [Bk][Sk][H*D] (Bk = B, or 1 = shared by every sequence), keep uint8 [B][Mq][Sk] (Mq = Sq, or
// 1 = one key mask for all query rows; 1 = attend), p [B][H][Sq][Sk] (saved for the backward), out [B][Sq][H*D].
// drop (may be NULL) uint8 [B][H][Sq][Sk]: attention-probability dropout (HF-IB:176-196 `self.dropout(attention_probs)`,
// active when the reference trains): out = sum_j p_j drop_j drop_scale v_j with drop_scale = 1 / (1 - p_drop); p is saved
// BEFORE the dropout.  One wave per (b, h, query row); Sk <= 1024; D <= 128.
#define TR_MAXK 16   // keys per lane

__global__ void __launch_bounds__(64) tr_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                         const float* __restrict__ v, const uint8_t* __restrict__ keep,
                                                         int B, int Bk, int H, int Sq, int Sk, int D, int Mq, float scale,
                                                         const uint8_t* __restrict__ drop, float drop_scale,
                                                         float* __restrict__ p, float* __restrict__ out) {
  __shared__ float s_p[TR_MAXK * 64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x % Sq, h = (blockIdx.x / Sq) % H, b = blockIdx.x / (Sq * H);
  const int hid = H * D;
  const float* qr = q + ((int64_t)b * Sq + i) * hid + h * D;
  const float* kb = k + (int64_t)(Bk == 1 ? 0 : b) * Sk * hid + h * D;
  const float* vb = v + (int64_t)(Bk == 1 ? 0 : b) * Sk * hid + h * D;
  const uint8_t* mk = keep + ((int64_t)b * Mq + (Mq == 1 ? 0 : i)) * Sk;
  float s[TR_MAXK];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < TR_MAXK; ++t) {
    const int j = t * 64 + lane;
    s[t] = -INFINITY;
    if (j < Sk) {
      float acc = 0.f;
      for (int d = 0; d < D; ++d) acc += qr[d] * kb[(int64_t)j * hid + d];
      acc *= scale;
      if (!mk[j]) acc = acc + TR_FMIN;                     // additive finfo.min (absorbs the score), as the reference
      s[t] = acc;
      mx = fmaxf(mx, acc);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < TR_MAXK; ++t) {
    const int j = t * 64 + lane;
    if (j < Sk) {
      s[t] = expf(s[t] - mx);
      sum += s[t];
    }
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  float* pr = p + (((int64_t)b * H + h) * Sq + i) * Sk;
  const uint8_t* dr = drop ? drop + (((int64_t)b * H + h) * Sq + i) * Sk : nullptr;
#pragma unroll
  for (int t = 0; t < TR_MAXK; ++t) {
    const int j = t * 64 + lane;
    if (j < Sk) {
      const float pv = s[t] * inv;
      s_p[j] = dr ? (dr[j] ? pv * drop_scale : 0.f) : pv;
      pr[j] = pv;
    }
  }
  __syncthreads();
  for (int d = lane; d < D; d += 64) {
    float acc = 0.f;
    for (int j = 0; j < Sk; ++j) acc += s_p[j] * vb[(int64_t)j * hid + d];
    out[((int64_t)b * Sq + i) * hid + h * D + d] = acc;
  }
}

// dP_j = dO . v_j (x drop_j drop_scale under dropout); c = sum_j p_j dP_j; dS_j = p_j (dP_j - c); dq = scale sum_j dS_j k_j;
// dk_j += scale dS_j q; dv_j += p_j (drop_j drop_scale) dO  (dk / dv by atomics: rows of many queries - and, shared keys, of
// many sequences - add up)
__global__ void __launch_bounds__(64) tr_attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                         const float* __restrict__ v, const float* __restrict__ p,
                                                         const float* __restrict__ dout, int B, int Bk, int H, int Sq, int Sk,
                                                         int D, float scale, const uint8_t* __restrict__ drop,
                                                         float drop_scale, float* __restrict__ dq, float* __restrict__ dk,
                                                         float* __restrict__ dv) {
  __shared__ float s_ds[TR_MAXK * 64];
  __shared__ float s_p[TR_MAXK * 64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x % Sq, h = (blockIdx.x / Sq) % H, b = blockIdx.x / (Sq * H);
  const int hid = H * D;
  const int64_t qoff = ((int64_t)b * Sq + i) * hid + h * D;
  const int64_t kvoff = (int64_t)(Bk == 1 ? 0 : b) * Sk * hid + h * D;
  const float* pr = p + (((int64_t)b * H + h) * Sq + i) * Sk;
  const uint8_t* dr = drop ? drop + (((int64_t)b * H + h) * Sq + i) * Sk : nullptr;
  float dp[TR_MAXK];
  float c = 0.f;
#pragma unroll
  for (int t = 0; t < TR_MAXK; ++t) {
    const int j = t * 64 + lane;
    dp[t] = 0.f;
    if (j < Sk) {
      float acc = 0.f;
      for (int d = 0; d < D; ++d) acc += dout[qoff + d] * v[kvoff + (int64_t)j * hid + d];
      if (dr) acc = dr[j] ? acc * drop_scale : 0.f;
      dp[t] = acc;
      c += pr[j] * acc;
    }
  }
  c = wave_sum(c);
#pragma unroll
  for (int t = 0; t < TR_MAXK; ++t) {
    const int j = t * 64 + lane;
    if (j < Sk) {
      s_p[j] = dr ? (dr[j] ? pr[j] * drop_scale : 0.f) : pr[j];
      s_ds[j] = pr[j] * (dp[t] - c) * scale;
    }
  }
  __syncthreads();
  for (int d = lane; d < D; d += 64) {
    float acc = 0.f;
    const float qd = q[qoff + d], dod = dout[qoff + d];
    for (int j = 0; j < Sk; ++j) {
      const float ds = s_ds[j];
      acc += ds * k[kvoff + (int64_t)j * hid + d];
      if (ds != 0.f) atomicAdd(dk + kvoff + (int64_t)j * hid + d, ds * qd);
      const float pj = s_p[j];
      if (pj != 0.f) atomicAdd(dv + kvoff + (int64_t)j * hid + d, pj * dod);
    }
    dq[qoff + d] = acc;
  }
}

extern "C" int psg_train_attn_fwd(psg_ctx* ctx, const float* q, const float* k, const float* v, const uint8_t* keep, int B,
                                  int Bk, int H, int Sq, int Sk, int D, int Mq, float scale, const uint8_t* drop,
                                  float drop_scale, float* p, float* out, void* stream) {
  PSG_REQUIRE(ctx && q && k && v && keep && p && out, PSG_ERR_INVALID, "psg_train_attn_fwd: NULL argument");
  PSG_REQUIRE(B >= 0 && (Bk == B || Bk == 1) && H > 0 && Sq > 0 && Sk > 0 && Sk <= TR_MAXK * 64 && D > 0 && D <= 128 &&
                  (Mq == 1 || Mq == Sq),
              PSG_ERR_UNSUPPORTED, "psg_train_attn_fwd: B=%d Bk=%d H=%d Sq=%d Sk=%d D=%d Mq=%d", B, Bk, H, Sq, Sk, D, Mq);
  if (B == 0) return PSG_OK;
  tr_attn_fwd_kernel<<<(unsigned)(B * H * Sq), 64, 0, (hipStream_t)stream>>>(q, k, v, keep, B, Bk, H, Sq, Sk, D, Mq, scale,
                                                                           drop, drop_scale, p, out);
  PSG_CHECK_LAUNCH("psg_train_attn_fwd");
  return PSG_OK;
}

extern "C" int psg_train_attn_bwd(psg_ctx* ctx, const float* q, const float* k, const float* v, const float* p,
                                  const float* dout, int B, int Bk, int H, int Sq, int Sk, int D, float scale,
                                  const uint8_t* drop, float drop_scale, float* dq, float* dk, float* dv, void* stream) {
  PSG_REQUIRE(ctx && q && k && v && p && dout && dq && dk && dv, PSG_ERR_INVALID, "psg_train_attn_bwd: NULL argument");
  PSG_REQUIRE(B >= 0 && (Bk == B || Bk == 1) && H > 0 && Sq > 0 && Sk > 0 && Sk <= TR_MAXK * 64 && D > 0 && D <= 128,
              PSG_ERR_UNSUPPORTED, "psg_train_attn_bwd: B=%d Bk=%d H=%d Sq=%d Sk=%d D=%d", B, Bk, H, Sq, Sk, D);
  if (B == 0) return PSG_OK;
  // dk / dv are accumulated: the caller hands them in zeroed
  tr_attn_bwd_kernel<<<(unsigned)(B * H * Sq), 64, 0, (hipStream_t)stream>>>(q, k, v, p, dout, B, Bk, H, Sq, Sk, D, scale, drop,
                                                                           drop_scale, dq, dk, dv);
  PSG_CHECK_LAUNCH("psg_train_attn_bwd");
  return PSG_OK;
}

// ---- element-wise: GELU, SwiGLU gate, rotary (psg_train_rows.h) ----------------------------------------------------------
extern "C" int psg_train_gelu_fwd(psg_ctx* ctx, const float* x, int64_t n, float* y, void* stream) {
  return tr_gelu_launch<TrF32>("psg_train_gelu_fwd", ctx, x, nullptr, false, n, y, stream);
}
extern "C" int psg_train_gelu_bwd(psg_ctx* ctx, const float* x, const float* dy, int64_t n, float* dx, void* stream) {
  return tr_gelu_launch<TrF32>("psg_train_gelu_bwd", ctx, x, dy, true, n, dx, stream);
}

extern "C" int psg_train_silu_mul_fwd(psg_ctx* ctx, const float* gu, int64_t rows, int inter, float* y, void* stream) {
  return tr_silu_mul_launch<TrF32>("psg_train_silu_mul_fwd", ctx, gu, nullptr, false, rows, inter, y, nullptr, stream);
}
extern "C" int psg_train_silu_mul_bwd(psg_ctx* ctx, const float* gu, const float* dy, int64_t rows, int inter, float* dgu,
                                      void* stream) {
  return tr_silu_mul_launch<TrF32>("psg_train_silu_mul_bwd", ctx, gu, dy, true, rows, inter, nullptr, dgu, stream);
}

extern "C" int psg_train_rope(psg_ctx* ctx, const float* x, const int32_t* pos, const float* rope_cos, const float* rope_sin,
                              int table_rows, int64_t rows, int heads, int head_dim, float sign, float* y, void* stream) {
  return tr_rope_launch<TrF32>("psg_train_rope", ctx, x, pos, rope_cos, rope_sin, table_rows, rows, heads, head_dim, sign, y,
                               stream);
}

// ---- loss gradients ---------------------------------------------------------------------------------------------------
// dlogits[row] = dloss[row] * (softmax(logits[row]) - onehot(label)); rows with label < 0 (ignore_index) get zeros
__global__ void __launch_bounds__(256) tr_ce_bwd_kernel(const float* __restrict__ logits, int vocab,
                                                        const int32_t* __restrict__ labels, const float* __restrict__ dloss,
                                                        float* __restrict__ dlogits) {
  __shared__ float s_red[4];
  const int64_t row = blockIdx.x;
  const int lab = labels[row];
  const float* x = logits + row * vocab;
  float* dx = dlogits + row * vocab;
  if (lab < 0 || lab >= vocab) {
    for (int i = threadIdx.x; i < vocab; i += 256) dx[i] = 0.f;
    return;
  }
  float m = -INFINITY;
  for (int i = threadIdx.x; i < vocab; i += 256) m = fmaxf(m, x[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  float s = 0.f;
  for (int i = threadIdx.x; i < vocab; i += 256) s += expf(x[i] - m);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float inv = 1.0f / (s_red[0] + s_red[1] + s_red[2] + s_red[3]);
  const float g = dloss[row];
  for (int i = threadIdx.x; i < vocab; i += 256) dx[i] = g * (expf(x[i] - m) * inv - (i == lab ? 1.0f : 0.0f));
}

extern "C" int psg_train_ce_bwd(psg_ctx* ctx, const float* logits, int64_t rows, int vocab, const int32_t* labels,
                                const float* dloss, float* dlogits, void* stream) {
  PSG_REQUIRE(ctx && logits && labels && dloss && dlogits && vocab > 0, PSG_ERR_INVALID, "psg_train_ce_bwd: bad argument");
  if (rows == 0) return PSG_OK;
  tr_ce_bwd_kernel<<<(unsigned)rows, 256, 0, (hipStream_t)stream>>>(logits, vocab, labels, dloss, dlogits);
  PSG_CHECK_LAUNCH("psg_train_ce_bwd");
  return PSG_OK;
}

// loss = weight / n * sum_i bce(x_i, y_i):  dx_i = dloss * weight / n * (sigmoid(x_i) - y_i)
__global__ void tr_bce_bwd_kernel(const float* __restrict__ logit, const float* __restrict__ label, int n, float weight,
                                  const float* __restrict__ dloss, float* __restrict__ dlogit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dlogit[i] = dloss[0] * weight / (float)n * (1.0f / (1.0f + expf(-logit[i])) - label[i]);
}

extern "C" int psg_train_bce_bwd(psg_ctx* ctx, const float* logit, const float* label, int n, float weight,
                                 const float* dloss, float* dlogit, void* stream) {
  PSG_REQUIRE(ctx && logit && label && dloss && dlogit && n > 0, PSG_ERR_INVALID, "psg_train_bce_bwd: bad argument");
  tr_bce_bwd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(logit, label, n, weight, dloss, dlogit);
  PSG_CHECK_LAUNCH("psg_train_bce_bwd");
  return PSG_OK;
}

// ---- multilabel categorical cross entropy (V4:484-495, the multiclass head's row loss) ------------------------------
// Per row of R logits x with 0/1 labels y, exactly the reference's arithmetic in fp32:
//   z = (1 - 2y) x,  neg = z - 9999 y,  pos = z - 9999 (1 - y),  loss = lse([neg, 0]) + lse([pos, 0])
// (the concatenated zero is the extra class of both log-sum-exps).  Backward over the R real classes only:
//   dx = dloss (1 - 2y) (softmax([neg, 0])[:R] + softmax([pos, 0])[:R]).
// One wave per row; the self-weighting of the rows (loss / loss.max(), V4:473-476) is left to autograd on the caller side.
__device__ __forceinline__ void tr_mlcce_stats(const float* __restrict__ x, const float* __restrict__ y, int R, int lane,
                                               float& mn, float& ln, float& mp, float& lp) {
  float a = 0.f, b = 0.f;                              // the zero column takes part in both maxima
  for (int r = lane; r < R; r += 64) {
    const float yr = y[r], z = (1.0f - 2.0f * yr) * x[r];
    a = fmaxf(a, z - yr * 9999.0f);
    b = fmaxf(b, z - (1.0f - yr) * 9999.0f);
  }
  mn = wave_max(a);
  mp = wave_max(b);
  float sa = 0.f, sb = 0.f;
  for (int r = lane; r < R; r += 64) {
    const float yr = y[r], z = (1.0f - 2.0f * yr) * x[r];
    sa += expf(z - yr * 9999.0f - mn);
    sb += expf(z - (1.0f - yr) * 9999.0f - mp);
  }
  ln = wave_sum(sa) + expf(-mn);                       // sum of exp over [neg, 0] relative to its max
  lp = wave_sum(sb) + expf(-mp);
}

__global__ void __launch_bounds__(256) tr_mlcce_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                           int rows, int R, float* __restrict__ loss) {
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float mn, ln, mp, lp;
  tr_mlcce_stats(logits + (int64_t)row * R, labels + (int64_t)row * R, R, lane, mn, ln, mp, lp);
  if (lane == 0) loss[row] = (mn + logf(ln)) + (mp + logf(lp));
}

__global__ void __launch_bounds__(256) tr_mlcce_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                           int rows, int R, const float* __restrict__ dloss,
                                                           float* __restrict__ dlogits) {
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* x = logits + (int64_t)row * R;
  const float* y = labels + (int64_t)row * R;
  float mn, ln, mp, lp;
  tr_mlcce_stats(x, y, R, lane, mn, ln, mp, lp);
  const float g = dloss[row], in = 1.0f / ln, ip = 1.0f / lp;
  for (int r = lane; r < R; r += 64) {
    const float yr = y[r], s = 1.0f - 2.0f * yr, z = s * x[r];
    const float pn = expf(z - yr * 9999.0f - mn) * in, pp = expf(z - (1.0f - yr) * 9999.0f - mp) * ip;
    dlogits[(int64_t)row * R + r] = g * s * (pn + pp);
  }
}

extern "C" int psg_train_mlcce_fwd(psg_ctx* ctx, const float* logits, const float* labels, int rows, int R, float* loss,
                                   void* stream) {
  PSG_REQUIRE(ctx && rows >= 0 && R > 0, PSG_ERR_INVALID, "psg_train_mlcce_fwd: rows=%d R=%d", rows, R);
  if (rows == 0) return PSG_OK;
  PSG_REQUIRE(logits && labels && loss, PSG_ERR_INVALID, "psg_train_mlcce_fwd: NULL argument");
  tr_mlcce_fwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(logits, labels, rows, R, loss);
  PSG_CHECK_LAUNCH("psg_train_mlcce_fwd");
  return PSG_OK;
}

extern "C" int psg_train_mlcce_bwd(psg_ctx* ctx, const float* logits, const float* labels, int rows, int R,
                                   const float* dloss, float* dlogits, void* stream) {
  PSG_REQUIRE(ctx && rows >= 0 && R > 0, PSG_ERR_INVALID, "psg_train_mlcce_bwd: rows=%d R=%d", rows, R);
  if (rows == 0) return PSG_OK;
  PSG_REQUIRE(logits && labels && dloss && dlogits, PSG_ERR_INVALID, "psg_train_mlcce_bwd: NULL argument");
  tr_mlcce_bwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, (hipStream_t)stream>>>(logits, labels, rows, R, dloss,
                                                                                   dlogits);
  PSG_CHECK_LAUNCH("psg_train_mlcce_bwd");
  return PSG_OK;
}
