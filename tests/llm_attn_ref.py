"""Float64 restatements of the LLM stage's attention operations (HF-LL:191-214: scores = q . k / sqrt(128), causal and
padding mask, softmax, p . v; every query head h reads key / value head h // G), the derived error bound of their kernels
and the helpers that build their inputs.  CPU only: nothing here touches the GPU, and nothing here is written from the
kernels.  The inputs are the STORED tensors (bf16 / fp16 / fp32) converted to float64; nothing inside is rounded.

Every reference returns (ref, A, gx, n):
    ref  the attention output, [rows, heads * 128]
    A    sum_j p_j |v_j|, same shape
    gx   max_j sum_d |q_d k_jd| / sqrt(128) over the visible keys, [rows, heads]
    n    visible keys, [rows]
(with sum_v=True a fifth value, sum_j |v_j| over the visible keys, shaped like ref).  A row without a visible key has
ref = A = gx = n = 0.

The bound (attn_bound), u = 2^-8 for bf16, 2^-11 for fp16, 0 for fp32 (the unit roundoff of the storage type):

    bound = u |ref| + [u A] + [2^-25 sum_j |v_j|] + max(2e-5, (2 delta_s + (n + 4) 2^-24) A),   delta_s = 132 * 2^-24 * gx

  u |ref|   the output is rounded once to the storage type: every kernel does.
  u A       only for kernels that round their probabilities to the storage type before P.V (`p_rounded`: the two
            matrix-core prompt kernels): a relative error of at most u per probability.  The scalar, decode and trie
            kernels keep their probabilities in fp32 and do NOT get this term.
  2^-25 sum_j |v_j|   fp16 and `p_rounded` only.  The matrix-core kernels round UNNORMALISED probabilities exp(s - max)
            in (0, 1]; below 2^-14 those land on fp16's subnormal spacing 2^-24, an absolute error of up to 2^-25 each
            (the matrix cores do not flush subnormal inputs), and the row sum they are divided by is >= 1 (the maximum's
            own term).
  fp32 arithmetic   a score is 128 fp32 accumulations, the scale, the exponent's argument (s - max) and the exponential
            itself: at most 132 roundings of 2^-24 each, relative to sum_d |q_d k_jd| / sqrt(128) <= gx, so its absolute
            error is at most delta_s.  A probability moves relatively by at most twice the score error (its own score and
            the normaliser's), hence 2 delta_s A; the n accumulations of P.V, the rescales and the normalisation add
            (n + 4) 2^-24 A.  The floor 2e-5 is the figure the project's fp32 attention tests already hold.

The fused kernels (psg_decode_attn(_gqa), psg_prefill_attn_rope(_gqa)) round the rotated q / k to the storage type, and
the rotated q is never written anywhere: a float64 rotation can round the other way at a tie, and one flipped ulp of q
costs more than the whole bound.  The exact-rotation helpers below build inputs that leave no rounding choice: rotary
tables whose (cos, sin) entries come from EXACT_ROT, q and k on the grid of multiples of 1/16 in [-4, 4].  Then
x1 cos - x2 sin and x2 cos + x1 sin are sums of two multiples of 1/32 of magnitude <= 4: exact in fp32, fused or not,
and they carry at most 8 significant bits, so bf16 and fp16 hold them.  Split-K partials come from the same grid, so
their fp32 sum is exact in any order.  V needs no grid.
"""
import math

import torch

from tests import gqa_ref as R

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
RSQRT = 1.0 / math.sqrt(128.0)
EXACT_ROT = ((1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-1.0, 0.0), (0.5, 0.5), (0.5, -0.5), (-0.5, 0.5))
FAMILIES = ("random", "ascending_maximum", "descending_maximum", "last_key_matters", "probability_rounding_edge")


# ---- references ----
def attend_masked64(q, k, v, vis):
    """One key set: q [nq, H, 128], k / v [H, n, 128] (float64), vis bool [nq, n] -> ref, A, sv [nq, H, 128], gx [nq, H],
    n [nq].  Rows without a visible key: zeros."""
    vis = torch.as_tensor(vis, dtype=torch.bool)
    nq, H = q.shape[:2]
    n = vis.sum(-1)
    if k.shape[1] == 0:
        z = torch.zeros(nq, H, 128, dtype=torch.float64)
        return z, z.clone(), torch.zeros(nq, H, dtype=torch.float64), n, z.clone()
    s = torch.einsum("qhd,hnd->qhn", q, k) * RSQRT
    s = s.masked_fill(~vis[:, None, :], float("-inf"))
    some = n > 0
    s[~some] = 0.0                                                 # (softmax of an all -inf row is NaN)
    p = torch.softmax(s, -1) * some[:, None, None]
    ref = torch.einsum("qhn,hnd->qhd", p, v)
    A = torch.einsum("qhn,hnd->qhd", p, v.abs())
    sv = torch.einsum("qn,hnd->qhd", vis.double(), v.abs())
    g = torch.einsum("qhd,hnd->qhn", q.abs(), k.abs()) * RSQRT
    gx = g.masked_fill(~vis[:, None, :], 0.0).amax(-1)
    return ref, A, gx, n, sv


def _pack(parts, rows, heads, sum_v):
    ref, A, sv = (torch.zeros(rows, heads, 128, dtype=torch.float64) for _ in range(3))
    gx = torch.zeros(rows, heads, dtype=torch.float64)
    n = torch.zeros(rows, dtype=torch.int64)
    for idx, (r_, a_, g_, n_, s_) in parts:
        ref[idx], A[idx], gx[idx], n[idx], sv[idx] = r_, a_, g_, n_, s_
    out = (ref.reshape(rows, -1), A.reshape(rows, -1), gx, n)
    return out + (sv.reshape(rows, -1),) if sum_v else out


def causal64(q, kc, vc, tok_pos, pairs, S, heads, sum_v=False):
    """Causal attention of a pair-major prompt block: q [pairs * S, heads * 128], caches [pairs, kvh, ctx, 128] (key j of
    a pair in cache row j), tok_pos int [pairs * S] with -1 for padding.  Key j is visible to row i of its pair iff
    j <= i and j is a real token; a padding query row sees nothing."""
    kvh = kc.shape[1]
    G = heads // kvh
    tp = torch.as_tensor(tok_pos).reshape(pairs, S)
    parts = []
    for p in range(pairs):
        real = tp[p] >= 0
        vis = torch.ones(S, S, dtype=torch.bool).tril() & real[None, :] & real[:, None]
        # rows of padding keys may hold anything (NaN included): they are not part of the operation
        k = torch.where(real[None, :, None], kc[p, :, :S].double(), torch.zeros(())).repeat_interleave(G, 0)
        v = torch.where(real[None, :, None], vc[p, :, :S].double(), torch.zeros(())).repeat_interleave(G, 0)
        qq = q[p * S:(p + 1) * S].double().view(S, heads, 128)
        parts.append((slice(p * S, (p + 1) * S), attend_masked64(qq, k, v, vis)))
    return _pack(parts, pairs * S, heads, sum_v)


def rows64(q, kc, vc, row_pair, row_slots, heads, sum_v=False):
    """Row r of pair row_pair[r] attends the cache slots row_slots[r] (a list of ints; None or empty: nothing)."""
    kvh = kc.shape[1]
    G = heads // kvh
    rows = q.shape[0]
    parts = []
    for r in range(rows):
        sl = row_slots[r]
        if sl is None or len(sl) == 0:
            continue
        sl = torch.as_tensor(sl, dtype=torch.long)
        k = kc[int(row_pair[r])][:, sl].double().repeat_interleave(G, 0)
        v = vc[int(row_pair[r])][:, sl].double().repeat_interleave(G, 0)
        parts.append((slice(r, r + 1), attend_masked64(q[r:r + 1].double().view(1, heads, 128), k, v,
                                                       torch.ones(1, len(sl), dtype=torch.bool))))
    return _pack(parts, rows, heads, sum_v)


def prefix64(q, kc, vc, tok_pair, tok_pos, heads, sum_v=False):
    """Row r attends the slots [0, tok_pos[r]] of pair tok_pair[r] (tok_pos < 0: a padding row)."""
    return rows64(q, kc, vc, tok_pair, [range(int(t) + 1) if t >= 0 else None for t in tok_pos], heads, sum_v)


def decode64(q_rot, k_rot, v_new, kc, vc, tok_pair, tok_pos, heads, sum_v=False):
    """Decode step: the new token's rotated q [rows, heads, 128], rotated k and v [rows, kvh, 128] (float64) plus the
    cached keys [0, pos) of its pair; the new key / value sit at slot pos."""
    k64, v64 = kc.double().clone(), vc.double().clone()
    for r in range(q_rot.shape[0]):
        if tok_pos[r] >= 0:
            k64[int(tok_pair[r]), :, int(tok_pos[r])] = k_rot[r]
            v64[int(tok_pair[r]), :, int(tok_pos[r])] = v_new[r]
    return prefix64(q_rot.reshape(q_rot.shape[0], -1), k64, v64, tok_pair, tok_pos, heads, sum_v)


def tree_slots(row_pair, row_node, prefix_len, anc, trie_base):
    """The cache slots of every trie row: the pair's prompt slots, then trie_base + anc[node][d] (-1 ends the list)."""
    out = []
    for r in range(len(row_pair)):
        sl = list(range(int(prefix_len[int(row_pair[r])])))
        for a in anc[int(row_node[r])]:
            if a < 0:
                break
            sl.append(int(trie_base) + int(a))
        out.append(sl)
    return out


def tree64(q, kc, vc, row_pair, row_node, prefix_len, anc, trie_base, heads, sum_v=False):
    return rows64(q, kc, vc, row_pair, tree_slots(row_pair, row_node, prefix_len, anc, trie_base), heads, sum_v)


# ---- the bound ----
def attn_bound(ref, A, gx, n, dtype, p_rounded=False, sum_v=None):
    """Module docstring.  p_rounded: the kernel rounds its probabilities to `dtype` before P.V (needs sum_v for fp16)."""
    u = U[dtype]
    gxe = gx.repeat_interleave(128, dim=1)
    delta = 132 * 2.0 ** -24 * gxe
    b = u * ref.abs() + torch.clamp((2 * delta + (n.double()[:, None] + 4) * 2.0 ** -24) * A, min=2e-5)
    if p_rounded and u:
        b = b + u * A
        if dtype == torch.float16:
            b = b + 2.0 ** -25 * sum_v
    return b


def check(tag, got, ref, bound):
    """worst |got - ref| / bound; asserts it <= 1 (a NaN anywhere fails)"""
    err = (got.double() - ref).abs()
    ratio = float((err / bound).max()) if err.numel() else 0.0
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} of {err.numel()} elements miss the bound, worst err / bound "
                                 f"{ratio:.3f}, first at {tuple(bad.nonzero()[0].tolist())}")
    return ratio


# ---- exact-rotation inputs ----
def exact_rope_tables(ctx, g):
    """cos / sin fp32 [ctx, 64], every (cos, sin) drawn per (position, frequency) from EXACT_ROT"""
    pick = torch.randint(0, len(EXACT_ROT), (ctx, 64), generator=g)
    tab = torch.tensor(EXACT_ROT, dtype=torch.float32)
    return tab[pick, 0].contiguous(), tab[pick, 1].contiguous()


def grid(shape, g, lim=4.0):
    """float64 multiples of 1/16 in [-lim, lim]"""
    m = int(lim * 16)
    return torch.randint(-m, m + 1, shape, generator=g).double() / 16


def unrotate(x_rot, pos, cos, sin):
    """The x with rope64(x, pos) == x_rot, for tables of exact_rope_tables: the transposed rotation over cos^2 + sin^2 (1
    or 1/2).  On the grid whenever |x_rot| <= 2 is on it."""
    c = cos.double()[pos][:, None, :]
    s = sin.double()[pos][:, None, :]
    det = c * c + s * s
    r1, r2 = x_rot[..., :64], x_rot[..., 64:]
    return torch.cat([(r1 * c + r2 * s) / det, (r2 * c - r1 * s) / det], dim=-1)


def split_exact(x, splits, g):
    """fp32 [splits, *x.shape] on the grid whose sum (in any order, in fp32) is exactly x (x on the grid)"""
    parts = torch.empty(splits, *x.shape, dtype=torch.float64)
    parts[:-1] = grid((splits - 1,) + tuple(x.shape), g, lim=2.0)
    parts[-1] = x.double() - parts[:-1].sum(0)
    return parts.float()


# ---- directed inputs ----
def family_scores(family, n, dtype, g, window=64):
    """Target scores t [n] of the keys 0 .. n - 1 as the LAST query sees them (a causal row i sees t[:i + 1]).
    ascending_maximum: t grows with the key index, so every 64-key pass of an online softmax rescales (alpha < 1);
    descending_maximum: key 0 dominates and every later probability lies in [2^-24, 2^-14] (fp16's subnormal range);
    last_key_matters: t_j = t_{j-1} + ln 2 over the last `window` keys (flat before): the last visible key of a row holds
    half its mass, the one before a quarter - for every row that sees a prefix of the keys inside the window;
    probability_rounding_edge: key 0 scores exactly 0 (a zero key) and is the maximum; every other exp(t_j) sits 0.875
    ulp of bf16 (0.75 ulp of fp16, whose ulp is nearer the grid's score resolution) above a representable value with a
    small mantissa: rounding moves it by at most a quarter ulp, truncating by three quarters or more, always down."""
    j = torch.arange(n, dtype=torch.float64)
    if family == "ascending_maximum":
        step = min(0.25, 40.0 / max(n - 1, 1))
        return step * (j - (n - 1) / 2)
    if family == "descending_maximum":
        t = 12.0 - math.log(2.0) * (14.0 + 10.0 * torch.rand(n, generator=g, dtype=torch.float64))
        t[0] = 12.0
        return t
    if family == "last_key_matters":
        return math.log(2.0) * (torch.clamp(j - (n - 1), min=1.0 - window) + (min(window, n) - 1) / 2)
    assert family == "probability_rounding_edge"
    bits = 10 if dtype == torch.float16 else 7
    mant = torch.randint(0, 2 ** (bits - 3), (n,), generator=g).double() / 2 ** bits       # in [1, 1.125): the coarse ulp
    e = torch.randint(1, 6, (n,), generator=g).double()
    t = torch.log(2.0 ** -e * (1 + mant + (0.75 if bits == 10 else 0.875) * 2.0 ** -bits))
    t[0] = 0.0
    return t


def directed_qk(t, nq, g, same_q=False, kstep=1.0 / 16, kmax=2.0):
    """Grid vectors whose scores follow t: q [nq, 128], k [n, 128] (float64, multiples of 1/16, |q| <= 2, |k| <= 2: what
    `unrotate` keeps on the grid) with q_i . k_j / sqrt(128) within 2e-4 of m_i t_j (m_i in {1, 7/8, 3/4}; 1 with
    same_q) up to the vernier dims.  q = 2 m d on 120 main dims and d / 16 on 8 vernier dims (d a sign pattern); k_j is
    kappa_j d on the main dims, corrected by single grid steps on main dims and then on a vernier dim.  t_j == 0 exactly
    gives the zero key.  kstep < 1/16 (inputs that are not rotated, fp16 / fp32 only): the vernier dim of k moves in
    steps of kstep instead, and the scores land within kstep * 1.4e-3 of t."""
    n = t.numel()
    d = torch.randint(0, 2, (128,), generator=g).double() * 2 - 1
    perm = torch.randperm(128, generator=g)
    main, vern = perm[:120], perm[120:]
    m = torch.ones(nq, dtype=torch.float64) if same_q else \
        torch.tensor([1.0, 0.875, 0.75], dtype=torch.float64)[torch.randint(0, 3, (nq,), generator=g)]
    q = torch.zeros(nq, 128, dtype=torch.float64)
    q[:, main] = 2.0 * m[:, None] * d[main]
    q[:, vern] = d[vern] / 16
    k = torch.zeros(n, 128, dtype=torch.float64)
    kappa = torch.round(t / (240.0 * RSQRT) * 16) / 16
    assert float(kappa.abs().max()) <= kmax - 0.1, "target scores out of reach"     # (kmax > 2: not for `unrotate`)
    k[:, main] = kappa[:, None] * d[main]
    q0 = torch.zeros(128, dtype=torch.float64)
    q0[main], q0[vern] = 2.0 * d[main], d[vern] / 16
    coarse = torch.round((t - k @ q0 * RSQRT) / (2.0 / 16 * RSQRT)).long()                 # |.| <= 60 main-dim steps
    steps = (torch.arange(120)[None, :] < coarse.abs()[:, None]).double() * torch.sign(coarse.double())[:, None]
    k[:, main] += steps / 16 * d[main]
    fine = torch.round((t - k @ q0 * RSQRT) / (kstep / 16 * RSQRT))                        # at most 1 / kstep vernier steps
    k[:, vern[0]] += fine * kstep * d[vern[0]]
    assert float((k @ q0 * RSQRT - t).abs().max()) <= 2e-4 and float(k.abs().max()) <= kmax
    return q, k


def family_qk(family, n, nq, G, dtype, g, window=64, kstep=1.0 / 16, kmax=2.0):
    """The vectors of one (pair, key / value head) as the attention sees them (after the rotation): q [nq, G, 128] for the
    G query heads of the group, k [n, 128], float64 on the grid, |q| <= 2, |k| <= kmax.  "random": q uniform on the grid
    in [-2, 2], k in [-1, 1]; else directed_qk on family_scores."""
    if family == "random":
        return grid((nq, G, 128), g, lim=2.0), grid((n, 128), g, lim=1.0)
    t = family_scores(family, n, dtype, g, window=window)
    q, k = directed_qk(t, nq * G, g, same_q=family == "probability_rounding_edge", kstep=kstep, kmax=kmax)
    return q.view(nq, G, 128), k


def junk(shape, g):
    """finite junk of magnitude about 2^10 for the padding rows (representable in every storage type)"""
    return (torch.randint(0, 2, shape, generator=g).double() * 2 - 1) * (768.0 + 32 * torch.randint(0, 17, shape, generator=g))


def family_v(family, shape, g):
    """V [..., n, 128]: normal; for probability_rounding_edge positive (A == |ref|: the probability errors cannot cancel)
    with a zero row for key 0, whose probability 1 has no rounding error to show"""
    v = torch.randn(shape, generator=g)
    if family == "probability_rounding_edge":
        v = v.abs() + 0.25
        v[..., 0, :] = 0.0
    return v


def rope64(x, pos, cos, sin):
    return R.rope64(x, pos, cos, sin)
