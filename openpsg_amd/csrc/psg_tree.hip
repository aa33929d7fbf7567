// Relation-likelihood pass of the LLM stage: every relation class of every selected pair scored by the
// decoder in ONE batched forward over a token trie of the candidate sequences.
//
//   psg_tree_attn       attention of trie rows: a row of pair p at trie node i attends to p's prompt keys (cache slots
//                       [0, prefix_len[p])) and to the slots of i's ancestors and i itself (trie_base + anc[i][d]).
//                       One wave per (row, query head).  Scores and softmax in fp32 for every storage type; the fp32
//                       variant is exact fp32 arithmetic (no split, no 16-bit products), like psg_attn_f32.hip.
//   psg_token_logprobs  per logit row: log-sum-exp in fp32 (one pass, running max and sum), then logit[tok] - lse for
//                       the row's trie children (CSR lists shared by all pairs).  Fixed reduction order, no atomics.
//
// Decode over the same trie only:
//   psg_trie_greedy_step  psg_greedy_step with the arg-max restricted to the children of the row's trie node; the node
//                       advances on the device, and the path's log-probability is accumulated with the log-sum-exp code
//                       of psg_token_logprobs (row_lse_256: one copy, both kernels call it).
//
// Beam decode over the same trie:
//   psg_trie_beam_step  one level of a width-B beam: per pair, every edge of every live hypothesis scored score + logit -
//                       lse (row_lse_256 again), the B best non-leaf edges become the next level's rows and the B best of
//                       (finished list + this level's EOS edges) the new finished list.  Ranked by counting under a total
//                       order: no atomics, bit-reproducible.
#include "psg_common.h"

namespace {

constexpr int TREE_WAVES = 4;

// One wave per (row, head).  Lane j of the score phase computes the full 128-wide dot product of key j (keys j, j + 64,
// ...; k-ordered fp32 sum), the softmax statistics are wave reductions (butterfly: every lane ends with the same
// value), and in the output phase lane l owns dims 2l, 2l + 1 and sums the keys in key order.
template <typename T>
__global__ void __launch_bounds__(64 * TREE_WAVES)
    tree_attn_kernel(const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc,
                     const int32_t* __restrict__ row_pair, const int32_t* __restrict__ row_node,
                     const int32_t* __restrict__ prefix_len, const int32_t* __restrict__ anc, int n_int, int max_depth,
                     int trie_base, int64_t rows, int heads, int kv_heads, int pairs, int ctx, T* __restrict__ out) {
  __shared__ float s_q[TREE_WAVES][128];
  __shared__ float s_p[TREE_WAVES][PSG_TREE_MAX_KEYS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t task = (int64_t)blockIdx.x * TREE_WAVES + w;
  const int64_t r = task / heads;
  const int h = (int)(task % heads);
  bool ok = r < rows;
  int p = 0, nd = 0;
  if (ok) {
    p = row_pair[r];
    nd = row_node[r];
    ok = p >= 0 && p < pairs && nd >= 0 && nd < n_int;
  }
  int plen = 0, depth = 0;
  if (ok) {
    plen = prefix_len[p];
    plen = plen < 0 ? 0 : (plen > trie_base ? trie_base : plen);       // the host keeps trie_base + max_depth <= MAX_KEYS
    for (; depth < max_depth; ++depth) {
      const int a = anc[(int64_t)nd * max_depth + depth];
      if (a < 0 || a >= n_int) break;
    }
  }
  const int nk = plen + depth;
  const int g = h / (heads / kv_heads);
  const int64_t hd = (int64_t)heads * 128;
  const T* kb = kc + ((int64_t)p * kv_heads + g) * ctx * 128;
  const T* vb = vc + ((int64_t)p * kv_heads + g) * ctx * 128;
  const int32_t* an = anc + (int64_t)nd * max_depth;
  if (ok) {
    s_q[w][2 * lane] = Act<T>::ld(q, r * hd + h * 128 + 2 * lane);
    s_q[w][2 * lane + 1] = Act<T>::ld(q, r * hd + h * 128 + 2 * lane + 1);
  }
  __syncthreads();
  for (int j = lane; j < nk; j += 64) {
    const int slot = j < plen ? j : trie_base + an[j - plen];
    const T* kr = kb + (int64_t)slot * 128;
    float acc = 0.f;
#pragma unroll 4
    for (int d = 0; d < 128; d += 4) {
      float kv4[4];
      Act<T>::ld4(kr, d, kv4);
      acc = fmaf(s_q[w][d], kv4[0], acc);
      acc = fmaf(s_q[w][d + 1], kv4[1], acc);
      acc = fmaf(s_q[w][d + 2], kv4[2], acc);
      acc = fmaf(s_q[w][d + 3], kv4[3], acc);
    }
    s_p[w][j] = acc * 0.08838834764831845f;                             // 1 / sqrt(128)
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = lane; j < nk; j += 64) m = fmaxf(m, s_p[w][j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float sum = 0.f;
  for (int j = lane; j < nk; j += 64) {
    const float e = expf(s_p[w][j] - m);
    s_p[w][j] = e;
    sum += e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  __syncthreads();
  if (!ok) return;
  float a0 = 0.f, a1 = 0.f;
  for (int j = 0; j < nk; ++j) {
    const int slot = j < plen ? j : trie_base + an[j - plen];
    const float pj = s_p[w][j] / sum;                                   // softmax first, then P.V (HF-LL:208-210)
    const T* vr = vb + (int64_t)slot * 128;
    a0 = fmaf(pj, Act<T>::ld(vr, 2 * lane), a0);
    a1 = fmaf(pj, Act<T>::ld(vr, 2 * lane + 1), a1);
  }
  Act<T>::st(out, r * hd + h * 128 + 2 * lane, a0);
  Act<T>::st(out, r * hd + h * 128 + 2 * lane + 1, a1);
}

__device__ __forceinline__ void lse_combine(float& m, float& s, float m2, float s2) {
  if (s2 == 0.f) return;
  if (s == 0.f) { m = m2; s = s2; return; }
  const float mn = fmaxf(m, m2);
  s = s * expf(m - mn) + s2 * expf(m2 - mn);
  m = mn;
}

template <typename T>
__device__ __forceinline__ float logit_at(const void* logits, int S, int64_t slice, int64_t i) {
  if (S <= 0) return Act<T>::ld(reinterpret_cast<const T*>(logits), i);
  const float* p = reinterpret_cast<const float*>(logits);
  float a = p[i];
  for (int s = 1; s < S; ++s) a += p[(int64_t)s * slice + i];        // slice order, as psg_greedy_step sums them
  return a;
}

// log-sum-exp of one logit row over the whole vocabulary, by a 256-thread workgroup (every thread calls it and gets the
// value): one pass with a running max and sum per thread, a butterfly per wave, then the 4 waves in wave order.  The one
// copy of this arithmetic: psg_token_logprobs and psg_trie_greedy_step both call it, so their results agree bit for bit.
template <typename T>
__device__ __forceinline__ float row_lse_256(const void* __restrict__ logits, int S, int64_t slice, int64_t base,
                                             int vocab) {
  __shared__ float s_m[4], s_s[4], s_lse;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float m = -INFINITY, s = 0.f;
  for (int v = tid; v < vocab; v += 256) {
    const float x = logit_at<T>(logits, S, slice, base + v);
    if (x == -INFINITY) continue;                                       // exp(-inf) = 0; keeps a -inf first entry from NaN
    if (x > m) {
      s = s * expf(m - x) + 1.f;                                        // (s == 0 on the first element: 0 * 0)
      m = x;
    } else {
      s += expf(x - m);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_combine(m, s, m2, s2);
  }
  if (lane == 0) { s_m[w] = m; s_s[w] = s; }
  __syncthreads();
  if (tid == 0) {
    float mm = s_m[0], ss = s_s[0];
    for (int i = 1; i < 4; ++i) lse_combine(mm, ss, s_m[i], s_s[i]);
    s_lse = mm + logf(ss);
  }
  __syncthreads();
  return s_lse;
}

// One workgroup per logit row.
template <typename T>
__global__ void __launch_bounds__(256)
    token_logprobs_kernel(const void* __restrict__ logits, int S, int64_t rows, int vocab,
                          const int32_t* __restrict__ row_node, const int64_t* __restrict__ row_out,
                          const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_tok, int n_nodes,
                          int n_edges, float* __restrict__ out, int64_t out_len) {
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t slice = rows * vocab;
  const int64_t base = r * vocab;
  const float lse = row_lse_256<T>(logits, S, slice, base, vocab);
  const int nd = row_node[r];
  if (nd < 0 || nd >= n_nodes) return;
  const int c0 = child_off[nd], c1 = child_off[nd + 1];
  const int64_t o0 = row_out[r];
  for (int c = c0 + tid; c < c1; c += 256) {
    if (c < 0 || c >= n_edges) continue;
    const int64_t oi = o0 + (c - c0);
    if (oi < 0 || oi >= out_len) continue;
    const int tok = child_tok[c];
    out[oi] = (tok >= 0 && tok < vocab) ? logit_at<T>(logits, S, slice, base + tok) - lse : NAN;
  }
}

// Candidate of the constrained arg-max: value (rounded to the activation type, as psg_greedy_step compares), token, edge.
struct TrieBest {
  float val;
  int tok, edge;
  int low_tok, low_edge;                                                // the child with the lowest token id (fallback)
  __device__ __forceinline__ void take(float v, int t, int e) {
    if (v > val || (v == val && t < tok)) { val = v; tok = t; edge = e; }
  }
  __device__ __forceinline__ void take_low(int t, int e) {
    if (t < low_tok) { low_tok = t; low_edge = e; }
  }
};

// One workgroup per decode row: the greedy step of psg_greedy_step with the arg-max restricted to the children of the
// row's trie node.  T: activation type the candidate values are rounded to; TE / TX as in greedy_step_kernel.
template <typename T, typename TE, typename TX>
__global__ void __launch_bounds__(256)
    trie_greedy_step_kernel(const void* __restrict__ logits, int S, int vocab, int step, int max_new, int eos,
                            const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_tok,
                            const int32_t* __restrict__ edge_node, int n_nodes, int n_edges, int32_t* __restrict__ node,
                            float* __restrict__ logp, int32_t* __restrict__ tokens, int32_t* __restrict__ done,
                            int32_t* __restrict__ next_ids, int32_t* __restrict__ tok_pos, const TE* __restrict__ embed,
                            int hidden, TX* __restrict__ x_out) {
  __shared__ float s_val[4];
  __shared__ int s_tok[4], s_edge[4], s_ltok[4], s_ledge[4];
  __shared__ int s_emit;
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t slice = (int64_t)gridDim.x * vocab;
  const int64_t base = (int64_t)k * vocab;
  const int nd = node[k];
  // workgroup-uniform: a finished row, or a state outside the tables, decodes nothing and reads no table
  const bool live = done[k] == 0 && nd >= 0 && nd < n_nodes;
  float lse = 0.f;
  if (logp && live) lse = row_lse_256<T>(logits, S, slice, base, vocab);
  TrieBest b = {-INFINITY, 0x7fffffff, -1, 0x7fffffff, -1};
  if (live) {
    int c0 = child_off[nd], c1 = child_off[nd + 1];
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 > n_edges ? n_edges : c1;
    for (int c = c0 + tid; c < c1; c += 256) {
      const int t = child_tok[c];
      if (t < 0 || t >= vocab) continue;                                // never a candidate: its logit does not exist
      b.take(Act<T>::rnd(logit_at<T>(logits, S, slice, base + t)), t, c);
      b.take_low(t, c);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(b.val, o, 64);
    const int ot = __shfl_xor(b.tok, o, 64), oe = __shfl_xor(b.edge, o, 64);
    const int lt = __shfl_xor(b.low_tok, o, 64), le = __shfl_xor(b.low_edge, o, 64);
    b.take(ov, ot, oe);
    b.take_low(lt, le);
  }
  if (lane == 0) { s_val[w] = b.val; s_tok[w] = b.tok; s_edge[w] = b.edge; s_ltok[w] = b.low_tok; s_ledge[w] = b.low_edge; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 4; ++i) {
      b.take(s_val[i], s_tok[i], s_edge[i]);
      b.take_low(s_ltok[i], s_ledge[i]);
    }
    // no child compared greater than -inf (all NaN or -inf): the child with the lowest token id
    if (b.edge < 0 || !(b.val > -INFINITY)) { b.tok = b.low_tok; b.edge = b.low_edge; }
    int emit = (eos >= 0 && eos < vocab) ? eos : 0;                     // a row that decodes nothing embeds EOS: harmless
    if (live && b.edge >= 0) {
      emit = b.tok;
      tokens[(int64_t)k * max_new + step] = emit;
      const int nx = edge_node[b.edge];
      if (nx < 0) done[k] = 1;
      else node[k] = nx + 1;
      if (logp) logp[k] += logit_at<T>(logits, S, slice, base + emit) - lse;   // psg_token_logprobs' value for this edge
    } else {
      tokens[(int64_t)k * max_new + step] = -1;
    }
    next_ids[k] = emit;
    tok_pos[k] += 1;
    s_emit = emit;
  }
  if (x_out) {                                                          // kernel-uniform
    __syncthreads();
    const TE* src = embed + (int64_t)s_emit * hidden;
    for (int c = tid * 4; c < hidden; c += 256 * 4) {
      float v[4];
      Act<TE>::ld4(src, c, v);
      Act<TX>::st4(x_out, (int64_t)k * hidden + c, v);
    }
  }
}

// One workgroup per PAIR: one level of the beam.  Candidate slot i = s_off[beam] + (edge - first edge of the
// beam's node), so the slot order is (beam, edge) ascending - the live pool's tie order; the B entries of the old finished
// list follow the edges.  s_cls: -2 = no candidate, -1 = live pool, >= 0 = finish pool (the class).
template <typename T, typename TE, typename TX>
__global__ void __launch_bounds__(256)
    trie_beam_step_kernel(const void* __restrict__ logits, int S, int vocab, int B, int beams_in, int eos,
                          const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_tok,
                          const int32_t* __restrict__ edge_node, const int32_t* __restrict__ edge_class,
                          const int32_t* __restrict__ node_tok, const int32_t* __restrict__ node_depth, int n_nodes,
                          int n_edges, int max_children, int trie_base, const int32_t* __restrict__ seq_len,
                          int32_t* __restrict__ node, float* __restrict__ logp, int32_t* __restrict__ fin_class,
                          float* __restrict__ fin_logp, int32_t* __restrict__ row_node, int32_t* __restrict__ tok_pos,
                          int32_t* __restrict__ rope_pos, const TE* __restrict__ embed, int hidden,
                          TX* __restrict__ x_out) {
  __shared__ float s_v[PSG_BEAM_MAX_CAND + PSG_BEAM_MAX_WIDTH];
  __shared__ int s_edge[PSG_BEAM_MAX_CAND + PSG_BEAM_MAX_WIDTH], s_cls[PSG_BEAM_MAX_CAND + PSG_BEAM_MAX_WIDTH];
  __shared__ float s_score[PSG_BEAM_MAX_WIDTH];
  __shared__ int s_c0[PSG_BEAM_MAX_WIDTH], s_cnt[PSG_BEAM_MAX_WIDTH], s_off[PSG_BEAM_MAX_WIDTH + 1];
  __shared__ int s_live[PSG_BEAM_MAX_WIDTH], s_fin[PSG_BEAM_MAX_WIDTH], s_emit[PSG_BEAM_MAX_WIDTH];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int n_int = n_nodes - 1;
  const int64_t slice = (int64_t)gridDim.x * beams_in * vocab;
  if (tid < B) {
    const int nd = tid < beams_in ? node[(int64_t)k * B + tid] : -1;
    int c0 = 0, cnt = 0;
    if (nd >= 0 && nd < n_nodes) {
      c0 = child_off[nd];
      int c1 = child_off[nd + 1];
      c0 = c0 < 0 ? 0 : c0;
      c1 = c1 > n_edges ? n_edges : c1;
      cnt = c1 - c0;
      cnt = cnt < 0 ? 0 : (cnt > max_children ? max_children : cnt);   // the host keeps B * max_children <= MAX_CAND
    }
    s_c0[tid] = c0;
    s_cnt[tid] = cnt;
    s_score[tid] = tid < beams_in ? logp[(int64_t)k * B + tid] : 0.f;
    s_live[tid] = -1;
    s_fin[tid] = -1;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int b = 0; b < B; ++b) { s_off[b] = o; o += s_cnt[b]; }
    s_off[B] = o;
  }
  __syncthreads();
  const int n_cand = s_off[B];
  for (int b = 0; b < beams_in; ++b) {
    const int cnt = s_cnt[b];
    if (cnt == 0) continue;                                             // workgroup-uniform: a dead beam reads no logit
    const int64_t base = ((int64_t)k * beams_in + b) * vocab;
    const float lse = row_lse_256<T>(logits, S, slice, base, vocab);
    const float score = s_score[b];
    for (int j = tid; j < cnt; j += 256) {
      const int c = s_c0[b] + j, tok = child_tok[c];
      float v = 0.f;
      int cls = -2;
      if (tok >= 0 && tok < vocab) {
        const float t = logit_at<T>(logits, S, slice, base + tok) - lse;   // psg_token_logprobs' value for this row and child
        v = score + t;
        if (!(v != v) && t != -INFINITY) {
          const int nx = edge_node[c];
          if (nx >= 0) cls = nx < n_int ? -1 : -2;
          else {
            const int r = edge_class[c];
            cls = r >= 0 ? r : -2;
          }
        }
      }
      s_v[s_off[b] + j] = v;
      s_edge[s_off[b] + j] = c;
      s_cls[s_off[b] + j] = cls;
    }
  }
  if (tid < B) {                                                        // the old finished list: behind the edges
    const float v = fin_logp[(int64_t)k * B + tid];
    const int r = fin_class[(int64_t)k * B + tid];
    s_v[n_cand + tid] = v;
    s_edge[n_cand + tid] = -1;
    s_cls[n_cand + tid] = (r >= 0 && !(v != v)) ? r : -2;
  }
  __syncthreads();
  const int total = n_cand + B;
  for (int i = tid; i < total; i += 256) {
    const int ci = s_cls[i];
    if (ci == -2) continue;
    const float vi = s_v[i];
    int rank = 0;
    for (int j = 0; j < total && rank < B; ++j) {
      const int cj = s_cls[j];
      if (cj == -2 || (cj < 0) != (ci < 0)) continue;                   // the other pool
      const float vj = s_v[j];
      // live pool: v descending, then (beam, edge) = slot ascending; finish pool: v descending, then class, then slot
      const bool first = vj > vi || (vj == vi && (ci < 0 ? j < i : (cj < ci || (cj == ci && j < i))));
      rank += first ? 1 : 0;
    }
    if (rank < B) (ci < 0 ? s_live : s_fin)[rank] = i;                  // a total order: one slot per rank
  }
  __syncthreads();
  if (tid < B) {
    const int64_t r = (int64_t)k * B + tid;
    const int li = s_live[tid], fi = s_fin[tid];
    int emit = (eos >= 0 && eos < vocab) ? eos : 0;                     // a dead row embeds EOS, as a finished greedy row
    if (li >= 0) {
      const int ni = edge_node[s_edge[li]];                             // in [0, n_int): checked when the slot was written
      const int tk = node_tok[ni];
      node[r] = ni + 1;
      logp[r] = s_v[li];
      row_node[r] = ni;
      tok_pos[r] = trie_base + ni;
      rope_pos[r] = seq_len[k] + node_depth[ni] - 1;
      if (tk >= 0 && tk < vocab) emit = tk;
    } else {
      node[r] = -1;
      logp[r] = -INFINITY;
      row_node[r] = -1;
      tok_pos[r] = -1;
      rope_pos[r] = 0;
    }
    fin_class[r] = fi >= 0 ? s_cls[fi] : -1;
    fin_logp[r] = fi >= 0 ? s_v[fi] : -INFINITY;
    s_emit[tid] = emit;
  }
  if (x_out) {                                                          // kernel-uniform
    __syncthreads();
    for (int b = 0; b < B; ++b) {
      const TE* src = embed + (int64_t)s_emit[b] * hidden;
      for (int c = tid * 4; c < hidden; c += 256 * 4) {
        float v[4];
        Act<TE>::ld4(src, c, v);
        Act<TX>::st4(x_out, ((int64_t)k * B + b) * hidden + c, v);
      }
    }
  }
}

}  // namespace

extern "C" int psg_tree_attn(psg_ctx* ctx_, const void* q, const void* k_cache, const void* v_cache,
                             const int32_t* row_pair, const int32_t* row_node, const int32_t* prefix_len,
                             const int32_t* anc, int n_int, int max_depth, int trie_base, int64_t rows, int heads,
                             int kv_heads, int pairs, int head_dim, int ctx, void* out, int dtype, void* stream) {
  PSG_REQUIRE(ctx_ && q && k_cache && v_cache && row_pair && row_node && prefix_len && anc && out, PSG_ERR_INVALID,
              "psg_tree_attn: NULL argument");
  PSG_REQUIRE(head_dim == 128, PSG_ERR_UNSUPPORTED, "psg_tree_attn: head_dim=%d (kernel is built for 128)", head_dim);
  PSG_REQUIRE(kv_heads > 0 && heads % kv_heads == 0 && heads / kv_heads <= PSG_GQA_MAX_GROUP, PSG_ERR_UNSUPPORTED,
              "psg_tree_attn: heads=%d kv_heads=%d (groups of 1..%d query heads per key / value head)", heads, kv_heads,
              PSG_GQA_MAX_GROUP);
  PSG_REQUIRE(n_int > 0 && max_depth > 0 && trie_base >= 0 && pairs > 0 && rows >= 0, PSG_ERR_INVALID,
              "psg_tree_attn: n_int=%d max_depth=%d trie_base=%d pairs=%d rows=%lld", n_int, max_depth, trie_base, pairs,
              (long long)rows);
  PSG_REQUIRE((int64_t)trie_base + n_int <= ctx, PSG_ERR_INVALID,
              "psg_tree_attn: trie slots [%d, %d) exceed the %d-slot cache", trie_base, trie_base + n_int, ctx);
  PSG_REQUIRE(trie_base + max_depth <= PSG_TREE_MAX_KEYS, PSG_ERR_UNSUPPORTED,
              "psg_tree_attn: %d prompt slots + depth %d exceed %d keys per row", trie_base, max_depth, PSG_TREE_MAX_KEYS);
  if (rows == 0) return PSG_OK;
  const int64_t tasks = rows * heads;
  const unsigned grid = (unsigned)((tasks + TREE_WAVES - 1) / TREE_WAVES);
  PSG_DISPATCH_DTYPE(dtype, "psg_tree_attn",
                     (tree_attn_kernel<T><<<grid, 64 * TREE_WAVES, 0, (hipStream_t)stream>>>(
                         (const T*)q, (const T*)k_cache, (const T*)v_cache, row_pair, row_node, prefix_len, anc, n_int,
                         max_depth, trie_base, rows, heads, kv_heads, pairs, ctx, (T*)out)));
  PSG_CHECK_LAUNCH("psg_tree_attn");
  return PSG_OK;
}

extern "C" int psg_token_logprobs(psg_ctx* ctx_, const void* logits, int splits, int64_t rows, int vocab,
                                  const int32_t* row_node, const int64_t* row_out, const int32_t* child_off,
                                  const int32_t* child_tok, int n_nodes, int n_edges, float* out, int64_t out_len,
                                  int dtype, void* stream) {
  PSG_REQUIRE(ctx_ && logits && row_node && row_out && child_off && child_tok && out, PSG_ERR_INVALID,
              "psg_token_logprobs: NULL argument");
  PSG_REQUIRE(rows >= 0 && vocab > 0 && n_nodes > 0 && n_edges >= 0 && out_len >= 0 && splits >= 0 && splits <= 64,
              PSG_ERR_INVALID, "psg_token_logprobs: rows=%lld vocab=%d n_nodes=%d n_edges=%d splits=%d", (long long)rows,
              vocab, n_nodes, n_edges, splits);
  if (rows == 0) return PSG_OK;
  PSG_REQUIRE(rows <= 0x7fffffff, PSG_ERR_UNSUPPORTED, "psg_token_logprobs: %lld rows", (long long)rows);
  if (splits > 0) dtype = PSG_F32;                                      // split-K partials are fp32 slices
  PSG_DISPATCH_DTYPE(dtype, "psg_token_logprobs",
                     (token_logprobs_kernel<T><<<(unsigned)rows, 256, 0, (hipStream_t)stream>>>(
                         logits, splits, rows, vocab, row_node, row_out, child_off, child_tok, n_nodes, n_edges, out,
                         out_len)));
  PSG_CHECK_LAUNCH("psg_token_logprobs");
  return PSG_OK;
}

extern "C" int psg_trie_greedy_step(psg_ctx* ctx_, const void* logits, int splits, int K, int vocab, int step, int max_new,
                                    int eos, const int32_t* child_off, const int32_t* child_tok, const int32_t* edge_node,
                                    int n_nodes, int n_edges, int32_t* node, float* logp, int32_t* tokens, int32_t* done,
                                    int32_t* next_ids, int32_t* tok_pos, const void* embed, int embed_dtype, int hidden,
                                    void* x_out, int x_dtype, int dtype, void* stream) {
  PSG_REQUIRE(ctx_ && logits && tokens && done && next_ids && tok_pos && node, PSG_ERR_INVALID,
              "psg_trie_greedy_step: NULL argument");
  PSG_REQUIRE(child_off && child_tok && edge_node, PSG_ERR_INVALID, "psg_trie_greedy_step: NULL trie table");
  PSG_REQUIRE(n_nodes >= 1 && n_edges >= 0, PSG_ERR_INVALID, "psg_trie_greedy_step: n_nodes=%d n_edges=%d", n_nodes,
              n_edges);
  PSG_REQUIRE(K > 0 && vocab > 0 && step >= 0 && step < max_new && splits >= 0 && splits <= 64, PSG_ERR_INVALID,
              "psg_trie_greedy_step: K=%d vocab=%d step=%d max_new=%d splits=%d", K, vocab, step, max_new, splits);
  PSG_REQUIRE(!x_out || (embed && hidden > 0 && hidden % 4 == 0), PSG_ERR_INVALID,
              "psg_trie_greedy_step: x_out needs the embedding table and hidden %% 4 == 0 (hidden=%d)", hidden);
  hipStream_t st = (hipStream_t)stream;
#define TGS(TE_, TX_)                                                                                                 \
  PSG_DISPATCH_DTYPE(dtype, "psg_trie_greedy_step",                                                                   \
                     (trie_greedy_step_kernel<T, TE_, TX_><<<K, 256, 0, st>>>(                                        \
                         logits, splits, vocab, step, max_new, eos, child_off, child_tok, edge_node, n_nodes, n_edges, \
                         node, logp, tokens, done, next_ids, tok_pos, (const TE_*)embed, hidden, (TX_*)x_out)))
  if (!x_out || (embed_dtype == PSG_F32 && x_dtype == PSG_F32)) TGS(float, float);
  else if (embed_dtype == PSG_BF16 && x_dtype == PSG_BF16) TGS(bf16_t, bf16_t);
  else if (embed_dtype == PSG_BF16 && x_dtype == PSG_F32) TGS(bf16_t, float);
  else if (embed_dtype == PSG_F16 && x_dtype == PSG_F16) TGS(f16_t, f16_t);
  else if (embed_dtype == PSG_F16 && x_dtype == PSG_F32) TGS(f16_t, float);
  else {
    psg_set_error("psg_trie_greedy_step: embedding dtype %d -> residual dtype %d unsupported", embed_dtype, x_dtype);
    return PSG_ERR_UNSUPPORTED;
  }
#undef TGS
  PSG_CHECK_LAUNCH("psg_trie_greedy_step");
  return PSG_OK;
}

extern "C" int psg_trie_beam_step(psg_ctx* ctx_, const void* logits, int splits, int K, int B, int beams_in, int vocab,
                                  int eos, const int32_t* child_off, const int32_t* child_tok, const int32_t* edge_node,
                                  const int32_t* edge_class, const int32_t* node_tok, const int32_t* node_depth,
                                  int n_nodes, int n_edges, int max_children, int trie_base, const int32_t* seq_len,
                                  int32_t* node, float* logp, int32_t* fin_class, float* fin_logp, int32_t* row_node,
                                  int32_t* tok_pos, int32_t* rope_pos, const void* embed, int embed_dtype, int hidden,
                                  void* x_out, int x_dtype, int dtype, void* stream) {
  PSG_REQUIRE(B >= 1 && B <= PSG_BEAM_MAX_WIDTH, PSG_ERR_INVALID, "psg_trie_beam_step: beam width B=%d (1..%d)", B,
              PSG_BEAM_MAX_WIDTH);
  PSG_REQUIRE(beams_in == 1 || beams_in == B, PSG_ERR_INVALID, "psg_trie_beam_step: beams_in=%d (1 or B=%d)", beams_in, B);
  PSG_REQUIRE(child_off && child_tok && edge_node && edge_class && node_tok && node_depth, PSG_ERR_INVALID,
              "psg_trie_beam_step: NULL trie table");
  PSG_REQUIRE(ctx_ && logits && seq_len && node && logp && fin_class && fin_logp && row_node && tok_pos && rope_pos,
              PSG_ERR_INVALID, "psg_trie_beam_step: NULL argument");
  PSG_REQUIRE(n_nodes >= 1 && n_edges >= 0, PSG_ERR_INVALID, "psg_trie_beam_step: n_nodes=%d n_edges=%d", n_nodes, n_edges);
  PSG_REQUIRE(!x_out || (embed && hidden > 0 && hidden % 4 == 0), PSG_ERR_INVALID,
              "psg_trie_beam_step: x_out needs the embedding table and hidden %% 4 == 0 (hidden=%d)", hidden);
  PSG_REQUIRE(K > 0 && vocab > 0 && splits >= 0 && splits <= 64 && trie_base >= 0, PSG_ERR_INVALID,
              "psg_trie_beam_step: K=%d vocab=%d splits=%d trie_base=%d", K, vocab, splits, trie_base);
  PSG_REQUIRE(max_children >= 0 && (int64_t)B * max_children <= PSG_BEAM_MAX_CAND, PSG_ERR_UNSUPPORTED,
              "psg_trie_beam_step: B=%d beams of up to %d children exceed %d candidates per pair", B, max_children,
              PSG_BEAM_MAX_CAND);
  if (splits > 0) dtype = PSG_F32;                                      // split-K partials are fp32 slices
  hipStream_t st = (hipStream_t)stream;
#define TBS(TE_, TX_)                                                                                                 \
  PSG_DISPATCH_DTYPE(dtype, "psg_trie_beam_step",                                                                     \
                     (trie_beam_step_kernel<T, TE_, TX_><<<K, 256, 0, st>>>(                                          \
                         logits, splits, vocab, B, beams_in, eos, child_off, child_tok, edge_node, edge_class, node_tok, \
                         node_depth, n_nodes, n_edges, max_children, trie_base, seq_len, node, logp, fin_class, fin_logp, \
                         row_node, tok_pos, rope_pos, (const TE_*)embed, hidden, (TX_*)x_out)))
  if (!x_out || (embed_dtype == PSG_F32 && x_dtype == PSG_F32)) TBS(float, float);
  else if (embed_dtype == PSG_BF16 && x_dtype == PSG_BF16) TBS(bf16_t, bf16_t);
  else if (embed_dtype == PSG_BF16 && x_dtype == PSG_F32) TBS(bf16_t, float);
  else if (embed_dtype == PSG_F16 && x_dtype == PSG_F16) TBS(f16_t, f16_t);
  else if (embed_dtype == PSG_F16 && x_dtype == PSG_F32) TBS(f16_t, float);
  else {
    psg_set_error("psg_trie_beam_step: embedding dtype %d -> residual dtype %d unsupported", embed_dtype, x_dtype);
    return PSG_ERR_UNSUPPORTED;
  }
#undef TBS
  PSG_CHECK_LAUNCH("psg_trie_beam_step");
  return PSG_OK;
}
