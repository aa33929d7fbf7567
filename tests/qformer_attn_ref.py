"""Float64 restatements of the Q-Former attention operations (HF-IB:464-515 as driven by V4:158-170), the derived error
bounds of their 16-bit kernels and the helpers that build their inputs.  CPU only: nothing here touches the GPU, and
nothing here is written from the kernels.  The inputs are the STORED tensors (bf16 / fp16 / fp32) converted to float64;
nothing inside is rounded.

Every reference returns (ref, A) with A = sum_j p_j |v_j| (|x_j| for the input-space form): the bound needs it.

The bound of a 16-bit attention kernel (u = 2^-8 for bf16, 2^-11 for fp16: the unit roundoff of the storage type):

    bound = u |ref| + u A + 2e-5

  u |ref|  the output is rounded once to the storage type;
  u A      every kernel rounds its probabilities to the storage type before P.V (normalised ones in the scalar kernels,
           unnormalised ones in the matrix-core kernels): a relative error of at most u per probability;
  2e-5     the fp32 score and accumulation error at these magnitudes (the figure the fp32 attention tests hold);
fp32 instantiations get the 2e-5 alone.  Rows whose mask union is empty under the "unmasked" policy, computed by a path
that really adds the legacy constant (-10000 to the scaled score, or -80000 to the raw one) in fp32, get 2^-10 A more:
the sum rounds every score to half an ulp of the constant, 2^-11 in score units, and a probability moves by at most
twice the score error, relatively.
"""
import numpy as np
import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}


# ---- inputs ----
def pack_bits(om):
    """bool [N, L] -> int64 [N, ceil(L / 64)], bit l of a row = key l; the bits at and past L stay zero"""
    om = torch.as_tensor(om, dtype=torch.bool)
    N, L = om.shape
    words = (L + 63) // 64
    b = np.zeros((N, words * 64), dtype=np.uint8)
    b[:, :L] = om.numpy()
    return torch.from_numpy(np.packbits(b, axis=-1, bitorder="little").view(np.int64).reshape(N, words).copy())


def unpack_bits(bits, L):
    """the inverse of pack_bits (also tells whether a bit at or past L is set: second value)"""
    N, words = bits.shape
    b = np.unpackbits(bits.numpy().view(np.uint8).reshape(N, words * 8), axis=-1, bitorder="little")
    return torch.from_numpy(b[:, :L].astype(bool)), bool(b[:, L:].any())


def pair_masks(om, pair_index, N):
    """the key mask of pair id p = i * N + j: mask_i | mask_j (V4:430-433) -> bool [P, L]"""
    om = torch.as_tensor(om, dtype=torch.bool)
    pi = torch.as_tensor(pair_index).long()
    return om[pi // N] | om[pi % N]


# ---- references ----
def xattn64(q, k, v, pm, heads, nq, policy, chunk=64):
    """Cross-attention of the P * nq query rows over the L patch keys.  q [P * nq, hidden], k / v [L, hidden], pm bool
    [P, L] (True = attend).  scores = q . k / 8; "uniform": masked keys -inf, an empty union = all-equal scores (the mean
    of V); "unmasked": masked keys s - 10000 (an empty union = plain attention, exactly)."""
    assert policy in ("uniform", "unmasked")
    L, hidden = k.shape
    P = pm.shape[0]
    assert hidden == heads * 64 and q.shape == (P * nq, hidden) and pm.shape == (P, L)
    kh = k.double().view(L, heads, 64).permute(1, 0, 2)
    vh = v.double().view(L, heads, 64).permute(1, 0, 2)
    ref = torch.empty(P * nq, hidden, dtype=torch.float64)
    A = torch.empty_like(ref)
    for p0 in range(0, P, chunk):
        p1 = min(P, p0 + chunk)
        qh = q[p0 * nq:p1 * nq].double().view(p1 - p0, nq, heads, 64).permute(0, 2, 1, 3)
        s = torch.einsum("phqd,hld->phql", qh, kh) / 8.0
        on = pm[p0:p1, None, None, :]
        if policy == "uniform":
            s = torch.where(on, s, torch.full_like(s, float("-inf")))
            s[~pm[p0:p1].any(-1)] = 0.0
        else:
            empty = ~pm[p0:p1].any(-1)
            s = torch.where(on | empty[:, None, None, None], s, s - 10000.0)
        pr = torch.softmax(s, -1)
        ref[p0 * nq:p1 * nq] = torch.einsum("phql,hld->phqd", pr, vh).permute(0, 2, 1, 3).reshape(-1, hidden)
        A[p0 * nq:p1 * nq] = torch.einsum("phql,hld->phqd", pr, vh.abs()).permute(0, 2, 1, 3).reshape(-1, hidden)
    return ref, A


def selfattn64(src, text_mask, B, T, nq, heads, rows="all"):
    """Self-attention of the pairs' rows: the keys of pair p are its nq query rows plus its T text rows; masked text keys
    get -inf, query keys are always valid.  src = qkv [(B * nq + B * T), 3 * hidden] (query rows pair-major, then text rows
    pair-major), or (q_cls [B, hidden], kv [(B * nq + B * T), 2 * hidden]) for rows == "cls".
    rows: "all" -> [(B * nq + B * T), hidden] in the layout of qkv, "query" -> [B * nq, hidden], "cls" -> [B, hidden]."""
    assert rows in ("all", "query", "cls")
    if isinstance(src, (tuple, list)):
        q_cls, kv = src
        assert rows == "cls"
        H = kv.shape[1] // 2
        qa, ka, va = None, kv[:, :H].double(), kv[:, H:].double()
    else:
        H = src.shape[1] // 3
        q_cls = None
        qa, ka, va = src[:, :H].double(), src[:, H:2 * H].double(), src[:, 2 * H:].double()
    assert H == heads * 64 and ka.shape[0] == B * (nq + T)
    n_out = {"all": B * (nq + T), "query": B * nq, "cls": B}[rows]
    ref = torch.zeros(n_out, H, dtype=torch.float64)
    A = torch.zeros_like(ref)
    tm = torch.as_tensor(text_mask).bool().reshape(B, T) if T else torch.zeros(B, 0, dtype=torch.bool)
    for p in range(B):
        idx = torch.tensor(list(range(p * nq, (p + 1) * nq)) + list(range(B * nq + p * T, B * nq + (p + 1) * T)))
        sel = {"all": idx, "query": idx[:nq], "cls": idx[:1]}[rows]
        qq = q_cls[p:p + 1].double() if q_cls is not None else qa[sel]
        qh = qq.view(-1, heads, 64).permute(1, 0, 2)
        kh = ka[idx].view(-1, heads, 64).permute(1, 0, 2)
        vh = va[idx].view(-1, heads, 64).permute(1, 0, 2)
        valid = torch.cat([torch.ones(nq, dtype=torch.bool), tm[p]])
        s = (qh @ kh.transpose(1, 2) / 8.0).masked_fill(~valid[None, None, :], float("-inf"))
        pr = torch.softmax(s, -1)
        dst = sel if rows == "all" else (sel if rows == "query" else torch.tensor([p]))
        ref[dst] = (pr @ vh).permute(1, 0, 2).reshape(-1, H)
        A[dst] = (pr @ vh.abs()).permute(1, 0, 2).reshape(-1, H)
    return ref, A


def cls_input64(x_query, x_text, text_index, g, text_mask, B, T, nq, with_gx=False):
    """cls-row attention in the input space: xbar[h][p] = sum_j softmax_j(g_h . x_j / 8) x_j over the nq query rows of pair p
    (block p of x_query) and the T text rows of block text_index[p] of x_text (p when text_index is None), whose row of
    text_mask masks them (-inf).  g fp32 [heads, B, hidden].  -> ref, A [heads, B, hidden] (and, with_gx, max_j sum_c
    |g_c x_jc| / 8 per (head, pair): the score magnitude the bound of the kernel's split g needs)."""
    heads, Bg, H = g.shape
    assert Bg == B and x_query.shape == (B * nq, H)
    ti = torch.arange(B) if text_index is None else torch.as_tensor(text_index).long()
    tm = torch.as_tensor(text_mask).bool().reshape(-1, T) if T else None
    ref = torch.zeros(heads, B, H, dtype=torch.float64)
    A = torch.zeros_like(ref)
    gx = torch.zeros(heads, B, dtype=torch.float64)
    g64 = g.double()
    for p in range(B):
        X = x_query[p * nq:(p + 1) * nq].double()
        valid = torch.ones(nq, dtype=torch.bool)
        if T:
            t = int(ti[p])
            X = torch.cat([X, x_text[t * T:(t + 1) * T].double()])
            valid = torch.cat([valid, tm[t]])
        s = (g64[:, p] @ X.T / 8.0).masked_fill(~valid[None, :], float("-inf"))
        pr = torch.softmax(s, -1)
        ref[:, p] = pr @ X
        A[:, p] = pr @ X.abs()
        gx[:, p] = (g64[:, p].abs() @ X.abs().T / 8.0).max(-1).values
    return (ref, A, gx) if with_gx else (ref, A)


# ---- bounds ----
def attn_bound(ref, A, dtype, legacy_empty_rows=None):
    """u |ref| + u A + 2e-5 (module docstring); legacy_empty_rows: bool per output row, True where the row's mask union is
    empty under "unmasked" AND the path under test adds the legacy constant in fp32 (+ 2^-10 A)."""
    u = U[dtype]
    b = u * ref.abs() + u * A + 2e-5
    if legacy_empty_rows is not None:
        b = b + torch.where(torch.as_tensor(legacy_empty_rows)[:, None], 2.0 ** -10 * A, torch.zeros_like(A))
    return b


def cls_input_bound(A, gx, dtype):
    """The input-space kernel writes fp32 (no u |ref|): u A + 2 delta A + 1e-6.  delta bounds the score error: the kernel
    keeps a 16-bit head and a 16-bit remainder of g (what is left is at most 2^-16 |g| in bf16, 2^-22 in fp16) and
    accumulates 768 products in fp32 (768 * 2^-24), each relative to sum_c |g_c x_jc| / 8 of the largest key; a
    probability moves by at most twice the score error, relatively."""
    if dtype == torch.float32:                                     # fp32 instantiations: the fp32 attention figure alone
        return torch.full_like(A, 2e-5)
    split = {torch.bfloat16: 2.0 ** -16, torch.float16: 2.0 ** -22}[dtype]
    delta = (split + 768 * 2.0 ** -24) * gx
    return U[dtype] * A + 2 * delta[..., None] * A + 1e-6
