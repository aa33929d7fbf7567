"""Tensor-level wrappers over the C ABI (include/psg_hip.h).

torch is plumbing here: it owns the HBM allocations and the stream; every wrapper passes raw
device pointers + sizes to libpsg_hip.so on `torch.cuda.current_stream()`.  There is no host
fallback: tensors must be CUDA(HIP) tensors, contiguous, of the dtype the kernel expects.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import PSG_PRO_RMSNORM, PSG_PRO_DECODE_ATTN, PSG_PRO_SILU_MUL  # noqa: F401
from ._lib import (PSG_BF16, PSG_F16, PSG_F32, PSG_EMPTY_UNIFORM, PSG_EMPTY_UNMASKED, PSG_XATTN_MFMA,
                   PSG_XATTN_SIMPLE, PsgHipError, check)

_DT = {torch.float32: PSG_F32, torch.bfloat16: PSG_BF16, torch.float16: PSG_F16}


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise PsgHipError(f"unsupported activation dtype {t.dtype}") from None


def _p(t, dtype=None, name="tensor"):
    """device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise PsgHipError(f"{name} must live in HBM (got a {t.device} tensor); this path has no CPU fallback")
    if not t.is_contiguous():
        raise PsgHipError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise PsgHipError(f"{name} must be {dtype}, got {t.dtype}")
    return t.data_ptr()


def _env(t: torch.Tensor):
    if not t.is_cuda:
        raise PsgHipError(f"tensor lives on {t.device}: this path runs only on the GPU (no CPU fallback)")
    return _lib.load(), _lib.ctx(t.device.index or 0), torch.cuda.current_stream(t.device).cuda_stream


def patch_embed(feat: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, patch: int = 16) -> torch.Tensor:
    """feat [1,C,Hf,Wf] fp32, weight [Cout,C,16,16] fp32 -> patches [L, Cout] fp32 (V4:410)."""
    import ctypes
    lib, ctx, st = _env(feat)
    _, Cc, Hf, Wf = feat.shape
    Cout = weight.shape[0]
    nbytes = ctypes.c_int64(0)
    check(lib.psg_patch_embed_workspace(ctx, Cc, Hf, Wf, Cout, patch, ctypes.byref(nbytes)),
          "psg_patch_embed_workspace")
    ws = torch.empty(nbytes.value // 4, device=feat.device, dtype=torch.float32)
    out = torch.empty(((Hf // patch) * (Wf // patch), Cout), device=feat.device, dtype=torch.float32)
    check(lib.psg_patch_embed(ctx, _p(feat, torch.float32, "mask_features"), Cc, Hf, Wf,
                              _p(weight, torch.float32, "patch_embed.weight"), _p(bias, torch.float32), Cout, patch,
                              _p(out), _p(ws), nbytes.value, st), "psg_patch_embed")
    return out


def mask_grid(pan: torch.Tensor, img_hw, pad_hw, grid_hw) -> torch.Tensor:
    lib, ctx, st = _env(pan)
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    out = torch.empty(gh * gw, device=pan.device, dtype=torch.float32)
    check(lib.psg_mask_grid(ctx, _p(pan, torch.int32, "pan_results"), pan.shape[0], pan.shape[1], int(img_hw[0]),
                            int(img_hw[1]), int(pad_hw[0]), int(pad_hw[1]), gh, gw, _p(out), st), "psg_mask_grid")
    return out


def object_bitmasks(grid: torch.Tensor, object_ids: torch.Tensor) -> torch.Tensor:
    """-> int64 view of uint64 bits [N, ceil(L/64)]."""
    lib, ctx, st = _env(grid)
    L, N = grid.numel(), object_ids.numel()
    words = (L + 63) // 64
    bits = torch.empty((N, words), device=grid.device, dtype=torch.int64)
    check(lib.psg_object_bitmasks(ctx, _p(grid, torch.float32, "grid"), L, _p(object_ids, torch.int32, "object_ids"), N,
                                  _p(bits), words, st), "psg_object_bitmasks")
    return bits


def qformer_embed(ids, word_emb, pos_emb, query_rows, ln_w, ln_b, eps, out):
    lib, ctx, st = _env(out)
    B, T = ids.shape
    nq, hidden = query_rows.shape
    assert out.shape == (B * (nq + T), hidden)
    check(lib.psg_qformer_embed(ctx, _p(ids, torch.int32, "ids"), B, T, _p(word_emb, torch.float32),
                                _p(pos_emb, torch.float32), _p(query_rows, torch.float32), nq,
                                _p(ln_w, torch.float32), _p(ln_b, torch.float32), float(eps), hidden, _p(out), _dt(out),
                                st), "psg_qformer_embed")
    return out


def qformer_embed_split(ids, word_emb, pos_emb, query_rows, ln_w, ln_b, eps, out_query, out_text):
    """The same embedding, written as ONE block of query rows [nq, hidden] (identical for every pair) and the
    text rows [B*T, hidden]."""
    lib, ctx, st = _env(out_text)
    B, T = ids.shape
    nq, hidden = query_rows.shape
    assert out_query.shape == (nq, hidden) and out_text.shape == (B * T, hidden)
    common = (_p(word_emb, torch.float32), _p(pos_emb, torch.float32), _p(query_rows, torch.float32))
    tail = (_p(ln_w, torch.float32), _p(ln_b, torch.float32), float(eps), hidden)
    check(lib.psg_qformer_embed(ctx, None, 1, 0, *common, nq, *tail, _p(out_query), _dt(out_query), st),
          "psg_qformer_embed")
    check(lib.psg_qformer_embed(ctx, _p(ids, torch.int32, "ids"), B, T, *common, 0, *tail, _p(out_text), _dt(out_text),
                                st), "psg_qformer_embed")


def add_layernorm(x, residual, bias, gamma, beta, eps, out=None):
    lib, ctx, st = _env(x)
    out = x if out is None else out
    rows, hidden = x.shape
    if residual is not None:
        assert residual.shape == x.shape and residual.dtype == x.dtype
    check(lib.psg_add_layernorm(ctx, _p(x), _p(residual), _p(bias, torch.float32), _p(gamma, torch.float32),
                                _p(beta, torch.float32), float(eps), rows, hidden, _p(out, x.dtype), _dt(x), st),
          "psg_add_layernorm")
    return out


def add_layernorm_periodic(x, residual_table, bias, gamma, beta, eps, out=None):
    """LayerNorm(x + bias + residual_table[row % table_rows]); in place unless `out` is given."""
    lib, ctx, st = _env(x)
    out = x if out is None else out
    rows, hidden = x.shape
    assert residual_table.shape[1] == hidden and residual_table.dtype == x.dtype
    check(lib.psg_add_layernorm_periodic(ctx, _p(x), _p(residual_table), residual_table.shape[0],
                                         _p(bias, torch.float32), _p(gamma, torch.float32), _p(beta, torch.float32),
                                         float(eps), rows, hidden, _p(out, x.dtype), _dt(x), st),
          "psg_add_layernorm_periodic")
    return out


def add_layernorm_indexed(x, residual_table, block_index, group, bias, gamma, beta, eps, out=None):
    """LayerNorm(x + bias + residual_table[block_index[row // group] * group + row % group]); in place unless `out`."""
    lib, ctx, st = _env(x)
    out = x if out is None else out
    rows, hidden = x.shape
    assert residual_table.shape[1] == hidden and residual_table.dtype == x.dtype and rows % group == 0
    assert block_index.numel() == rows // group
    check(lib.psg_add_layernorm_indexed(ctx, _p(x), _p(residual_table), _p(block_index, torch.int32, "block_index"), group,
                                        _p(bias, torch.float32), _p(gamma, torch.float32), _p(beta, torch.float32),
                                        float(eps), rows, hidden, _p(out, x.dtype), _dt(x), st),
          "psg_add_layernorm_indexed")
    return out


def add_layernorm_res32(x, residual32, bias, gamma, beta, eps, out16=None, out32=None, period=0, index=None,
                        want16=True, want32=True):
    """Mixed mode: LayerNorm(x (16-bit) + bias + residual32 (fp32; plain, `period`-periodic table, or table blocks chosen
    by `index` per group of `period` rows)) -> (16-bit copy in place of x unless out16 is given, fp32 copy)."""
    lib, ctx, st = _env(x)
    rows, hidden = x.shape
    if want16 and out16 is None:
        out16 = x
    if want32 and out32 is None:
        out32 = torch.empty((rows, hidden), device=x.device, dtype=torch.float32)
    if residual32 is not None:
        assert residual32.dtype == torch.float32 and residual32.shape[1] == hidden
        assert period > 0 or residual32.shape[0] == rows
    check(lib.psg_add_layernorm_res32(ctx, _p(x), _p(residual32, torch.float32, "residual"), int(period),
                                      _p(index, torch.int32, "index"), _p(bias, torch.float32), _p(gamma, torch.float32),
                                      _p(beta, torch.float32), float(eps), rows, hidden,
                                      _p(out16, x.dtype) if want16 else None, _p(out32, torch.float32) if want32 else None,
                                      _dt(x), st), "psg_add_layernorm_res32")
    return (out16 if want16 else None), (out32 if want32 else None)


def bias_gelu(x, bias=None, out=None):
    lib, ctx, st = _env(x)
    out = x if out is None else out
    rows, cols = x.shape
    check(lib.psg_bias_gelu(ctx, _p(x), _p(bias, torch.float32), rows, cols, _p(out, x.dtype), _dt(x), st),
          "psg_bias_gelu")
    return out


def qformer_self_attn(qkv, text_mask, B, T, nq, heads, query_rows_only, out):
    lib, ctx, st = _env(qkv)
    hidden = qkv.shape[1] // 3
    assert qkv.shape[0] == B * (nq + T) and out.shape == (B * (nq + T), hidden) and out.dtype == qkv.dtype
    check(lib.psg_qformer_self_attn(ctx, _p(qkv), _p(text_mask, torch.uint8, "text_mask"), B, T, nq, heads,
                                    1 if query_rows_only else 0, _p(out), _dt(qkv), st), "psg_qformer_self_attn")
    return out


def qformer_self_attn_cls(q_cls, kv, text_mask, B, T, nq, heads):
    """Attention of the cls row (row 0) of every pair over its nq + T keys -> [B, hidden] (one row per pair).
    q_cls [B, hidden]: projected cls queries; kv [B*(nq+T), 2*hidden]: K | V of every row."""
    lib, ctx, st = _env(kv)
    hidden = kv.shape[1] // 2
    assert kv.shape[0] == B * (nq + T) and q_cls.shape == (B, hidden) and q_cls.dtype == kv.dtype
    out = torch.empty((B, hidden), device=kv.device, dtype=kv.dtype)
    check(lib.psg_qformer_self_attn_cls(ctx, _p(q_cls), _p(kv), _p(text_mask, torch.uint8, "text_mask"), B, T, nq,
                                        heads, _p(out), _dt(kv), st), "psg_qformer_self_attn_cls")
    return out


def qformer_cls_attn_input(x, g, text_mask, B, T, nq, heads, x_text=None, text_index=None):
    """cls-row attention in the input space (psg_qformer_cls_attn_input).  x [B*(nq+T), hidden]: the layer's input rows
    (query rows, then text rows) - or, with x_text [U*T, hidden] / text_index int32 [B], x [B*nq, hidden] holds the
    query rows only and pair p reads the text block (and text_mask row) text_index[p].
    g fp32 [heads, B, hidden] = W_k,h^T q_h  ->  xbar fp32 [heads, B, hidden] = sum_j p_j x_j."""
    lib, ctx, st = _env(x)
    hidden = x.shape[1]
    assert g.shape == (heads, B, hidden) and g.is_contiguous()
    if x_text is None:
        assert x.shape[0] == B * (nq + T) and text_index is None
        xt = x[B * nq:]
    else:
        assert x.shape[0] >= B * nq and x_text.dtype == x.dtype and x_text.shape[1] == hidden and text_index is not None
        xt = x_text
    xbar = torch.empty((heads, B, hidden), device=x.device, dtype=torch.float32)
    check(lib.psg_qformer_cls_attn_input(ctx, _p(x), _p(xt) if T > 0 else None,
                                         _p(text_index, torch.int32, "text_index") if text_index is not None else None,
                                         _p(g, torch.float32, "g"), _p(text_mask, torch.uint8, "text_mask"), B, T, nq,
                                         heads, hidden, _p(xbar), _dt(x), st), "psg_qformer_cls_attn_input")
    return xbar


def qformer_self_attn_shared(qkv_query, qkv_text, text_mask, B, T, nq, heads, out):
    """Layer-0 self-attention with ONE shared [nq, 3*hidden] projection of the query rows."""
    lib, ctx, st = _env(qkv_query)
    hidden = qkv_query.shape[1] // 3
    assert qkv_query.shape == (nq, 3 * hidden) and qkv_text.shape == (B * T, 3 * hidden)
    assert out.shape == (B * (nq + T), hidden) and out.dtype == qkv_query.dtype == qkv_text.dtype
    check(lib.psg_qformer_self_attn_shared(ctx, _p(qkv_query, name="qkv_query"), _p(qkv_text),
                                           _p(text_mask, torch.uint8, "text_mask"), B, T, nq, heads, _p(out),
                                           _dt(qkv_query), st), "psg_qformer_self_attn_shared")
    return out


def qformer_cross_attn(q, k, v, bits, pair_index, N, nq, heads, out=None, empty_policy=PSG_EMPTY_UNIFORM,
                       variant=None):
    lib, ctx, st = _env(q)
    P = pair_index.numel()
    L, hidden = k.shape
    assert q.shape == (P * nq, hidden) and v.shape == k.shape and k.dtype == q.dtype == v.dtype
    if variant is None:
        # the matrix-core kernel keeps all keys of one head in LDS (L <= 512 patches = images up to ~1450 px);
        # larger inputs take the row kernel (the reference runs them too)
        variant = PSG_XATTN_MFMA if L <= 512 else PSG_XATTN_SIMPLE
    out = torch.empty_like(q) if out is None else out
    check(lib.psg_qformer_cross_attn(ctx, _p(q), _p(k), _p(v), _p(bits, torch.int64, "bits"), bits.shape[1],
                                     _p(pair_index, torch.int32, "pair_index"), int(N), P, L, nq, heads,
                                     int(empty_policy), int(variant), _p(out, q.dtype), _dt(q), st),
          "psg_qformer_cross_attn")
    return out


def qformer_cross_attn_indexed(q_u, q_index, q_cls, k, v, bits, pair_index, N, heads, out=None,
                               empty_policy=PSG_EMPTY_UNIFORM):
    """`qformer_cross_attn` (33 query rows per pair) with the queries stored once per prompt: q_u [U * 33, hidden], q_index
    int32 [P] (prompt of each pair), q_cls [P, hidden] (row 0 of every pair).  Returns the context [P * 33, hidden], or
    None when the LDS-DMA kernel cannot run on these inputs (the caller then expands q)."""
    PSG_ERR_UNSUPPORTED = -2                                # include/psg_hip.h
    lib, ctx, st = _env(q_u)
    P = pair_index.numel()
    L, hidden = k.shape
    assert q_cls.shape == (P, hidden) and q_index.numel() == P and q_u.shape[1] == hidden and q_u.dtype == k.dtype == v.dtype
    out = torch.empty((P * 33, hidden), device=q_u.device, dtype=q_u.dtype) if out is None else out
    rc = lib.psg_qformer_cross_attn_indexed(ctx, _p(q_u), _p(q_index, torch.int32, "q_index"), _p(q_cls, q_u.dtype),
                                            _p(k), _p(v), _p(bits, torch.int64, "bits"), bits.shape[1],
                                            _p(pair_index, torch.int32, "pair_index"), int(N), P, L, heads, int(empty_policy),
                                            _p(out, q_u.dtype), _dt(q_u), st)
    if rc == PSG_ERR_UNSUPPORTED:
        return None
    check(rc, "psg_qformer_cross_attn_indexed")
    return out


def exist_head(x, w, b, P, nq):
    lib, ctx, st = _env(x)
    hidden = x.shape[1]
    logit = torch.empty(P, device=x.device, dtype=torch.float32)
    prob = torch.empty(P, device=x.device, dtype=torch.float32)
    check(lib.psg_exist_head(ctx, _p(x), _p(w, torch.float32), _p(b, torch.float32), P, nq, hidden, _p(logit),
                             _p(prob), _dt(x), st), "psg_exist_head")
    return logit, prob


def topk(score, k):
    lib, ctx, st = _env(score)
    idx = torch.empty(k, device=score.device, dtype=torch.int32)
    val = torch.empty(k, device=score.device, dtype=torch.float32)
    check(lib.psg_topk(ctx, _p(score, torch.float32, "score"), score.numel(), k, _p(idx), _p(val), st), "psg_topk")
    return idx, val


def multiclass_head(x, w, b, P, nq, pair_index=None, N=0, logit=None, prob=None):
    """Multiclass relation head (K8b): logits / probabilities [P, R] fp32 of the cls rows x[p*nq] (row stride nq*hidden).
    pair_index int32 [P] (global pair ids, None = p) and N mark the diagonal pairs, whose probabilities are 0.  logit /
    prob: caller-owned [P, R] fp32 outputs (e.g. slices of one [N^2, R] buffer); allocated when None."""
    lib, ctx, st = _env(x)
    hidden, R = x.shape[1], w.shape[0]
    if logit is None:
        logit = torch.empty((P, R), device=x.device, dtype=torch.float32)
    if prob is None:
        prob = torch.empty((P, R), device=x.device, dtype=torch.float32)
    if logit.shape != (P, R) or prob.shape != (P, R):
        raise PsgHipError(f"multiclass_head: outputs must be [{P}, {R}], got {tuple(logit.shape)} / {tuple(prob.shape)}")
    check(lib.psg_multiclass_head(ctx, _p(x), _p(w, torch.float32, "w"), _p(b, torch.float32, "b"), P, nq, hidden, R,
                                  _p(pair_index, torch.int32, "pair_index"), int(N), _p(logit, torch.float32, "logit"),
                                  _p(prob, torch.float32, "prob"), _dt(x), st), "psg_multiclass_head")
    return logit, prob


def topk_large_workspace_bytes(device, n, k):
    import ctypes
    out = ctypes.c_int64(0)
    check(_lib.load().psg_topk_large_workspace(_lib.ctx(torch.device(device).index or 0), int(n), int(k),
                                               ctypes.byref(out)),
          "psg_topk_large_workspace")
    return out.value


def topk_large(score, k, workspace=None, idx=None, val=None):
    """`topk` for large n (k <= 256; K9b): the same order and output.  workspace: uint8 device tensor of at least
    `topk_large_workspace_bytes(...)` bytes (allocated when None); idx int32 [k] / val fp32 [k]: caller-owned outputs."""
    lib, ctx, st = _env(score)
    n = score.numel()
    need = topk_large_workspace_bytes(score.device, n, k)
    if workspace is None:
        workspace = torch.empty(need, device=score.device, dtype=torch.uint8)
    if workspace.numel() * workspace.element_size() < need:
        raise PsgHipError(f"topk_large: workspace of {workspace.numel() * workspace.element_size()} bytes, {need} needed")
    if idx is None:
        idx = torch.empty(k, device=score.device, dtype=torch.int32)
    if val is None:
        val = torch.empty(k, device=score.device, dtype=torch.float32)
    if idx.numel() != k or val.numel() != k:
        raise PsgHipError(f"topk_large: outputs of {idx.numel()} / {val.numel()} elements for k={k}")
    check(lib.psg_topk_large(ctx, _p(score, torch.float32, "score"), n, k, _p(workspace, name="workspace"),
                             workspace.numel() * workspace.element_size(), _p(idx, torch.int32, "idx"),
                             _p(val, torch.float32, "val"), st), "psg_topk_large")
    return idx, val


def mlcce_rows(logits, labels):
    """Per-row multilabel categorical cross entropy (V4:484-495) of fp32 [S, R] logits with 0/1 fp32 labels."""
    lib, ctx, st = _env(logits)
    rows, R = logits.shape
    loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    check(lib.psg_train_mlcce_fwd(ctx, _p(logits, torch.float32, "logits"), _p(labels, torch.float32, "labels"), rows, R,
                                  _p(loss), st), "psg_train_mlcce_fwd")
    return loss


def mlcce_rows_bwd(logits, labels, dloss):
    lib, ctx, st = _env(logits)
    rows, R = logits.shape
    d = torch.empty_like(logits)
    check(lib.psg_train_mlcce_bwd(ctx, _p(logits, torch.float32, "logits"), _p(labels, torch.float32, "labels"), rows, R,
                                  _p(dloss, torch.float32, "dloss"), _p(d), st), "psg_train_mlcce_bwd")
    return d


def gather_rows(src, idx, dst):
    """dst[r] = src[idx[r]] (rows; idx < 0 -> zeros).  src/dst may be row-strided 2-D views."""
    lib, ctx, st = _env(src)
    assert src.dim() == 2 and dst.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
    if not src.is_cuda or not dst.is_cuda:
        raise PsgHipError("gather_rows: tensors must live in HBM")
    n, cols = dst.shape
    assert idx.numel() == n and src.shape[1] == cols
    check(lib.psg_gather_rows(ctx, src.data_ptr(), _dt(src), _p(idx, torch.int32, "idx"), n, cols, src.stride(0),
                              dst.data_ptr(), _dt(dst), dst.stride(0), st), "psg_gather_rows")
    return dst


def gather_pair_rows(xq, xt, text_index, text_mask, pair_index, sel, first, count, slot_off, nq, T, want_aux=True):
    """Rows of the selected pairs (global ids `sel`, int32 [K]) out of a selection-phase pass: see psg_gather_pair_rows.
    Returns (rows [K*(nq+T), cols], text mask [K, T] uint8, pair ids [K] int32, mine [K] uint8) - the last three None
    when want_aux is False (a second table of the same pass, e.g. the fp32 twins)."""
    lib, ctx, st = _env(xq)
    K = sel.numel()
    cols = xq.shape[1]
    out = torch.empty((K * (nq + T), cols), device=xq.device, dtype=xq.dtype)
    tm = torch.empty((K, T), device=xq.device, dtype=torch.uint8) if want_aux else None
    pi = torch.empty(K, device=xq.device, dtype=torch.int32) if want_aux else None
    mine = torch.empty(K, device=xq.device, dtype=torch.uint8) if want_aux else None
    check(lib.psg_gather_pair_rows(ctx, _p(xq), _p(xt, xq.dtype) if T > 0 else None, _p(text_index, torch.int32, "text_index"),
                                   _p(text_mask, torch.uint8, "text_mask") if want_aux and T > 0 else None,
                                   _p(pair_index, torch.int32, "pair_index") if want_aux else None,
                                   _p(sel, torch.int32, "sel"), K, int(first), int(count), int(slot_off), int(nq), int(T), cols,
                                   _p(out), _p(tm) if T > 0 else None, _p(pi), _p(mine), _dt(xq), st), "psg_gather_pair_rows")
    return out, tm, pi, mine


class Partials:
    """fp32 split-K slices [S, rows, cols] written by `skinny_gemm`; the consumer kernels
    (rmsnorm, rope_kvwrite, silu_mul, greedy_step) sum them while loading."""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        assert t.dim() == 3 and t.dtype == torch.float32 and t.is_contiguous()
        self.t = t

    @property
    def splits(self):
        return self.t.shape[0]

    @property
    def shape(self):
        return self.t.shape[1:]

    def reduce(self, dtype=torch.bfloat16):
        lib, ctx, st = _env(self.t)
        y = torch.empty(self.shape, device=self.t.device, dtype=dtype)
        check(lib.psg_reduce_partials(ctx, _p(self.t), self.splits, y.numel(), _p(y), _DT[dtype], st),
              "psg_reduce_partials")
        return y


def _in(x, dtype):
    """(pointer, splits) of a kernel input that is either an activation tensor or split-K partials."""
    if isinstance(x, Partials):
        return _p(x.t, torch.float32), x.splits
    return _p(x, dtype), 0


def rmsnorm(resid, delta, w, eps, out):
    """resid += delta; out = RMSNorm(resid) * w.  `out` has the activation dtype; `resid` has it too, or is fp32 with
    16-bit activations (mixed mode: the residual stream is never rounded to 16 bits)."""
    lib, ctx, st = _env(resid)
    rows, hidden = resid.shape
    dp, ds = (None, 0) if delta is None else _in(delta, out.dtype)
    if resid.dtype != out.dtype and resid.dtype != torch.float32:
        raise PsgHipError(f"rmsnorm: residual stream must be {out.dtype} or float32, got {resid.dtype}")
    check(lib.psg_rmsnorm(ctx, _p(resid), dp, ds, _p(w, torch.float32), float(eps), rows, hidden,
                          _p(out), _dt(out), _dt(resid), st), "psg_rmsnorm")
    return out


def _gqa(heads, kv_heads):
    """True when `kv_heads` names grouped-query attention (the *_gqa entry points); None / == heads: multi-head."""
    return kv_heads is not None and int(kv_heads) != int(heads)


def rope_kvwrite(qkv, tok_pair, tok_pos, rope, heads, head_dim, ctx_len, q_out, k_cache, v_cache, rope_pos=None,
                 kv_heads=None, rope_pos_bound=None):
    """rope = (cos, sin) fp32 tables [>= ctx_len, head_dim/2].  rope_pos int32 [rows]: rotary positions when they
    differ from the cache slots (training forward).  kv_heads < heads: grouped-query attention (psg_rope_kvwrite_gqa:
    qkv rows [q | k | v] of (heads + 2 kv_heads) * head_dim, caches [pairs, kv_heads, ctx, head_dim]).
    rope_pos_bound: a bound the caller knows on the host (every rope_pos < it) - no read-back, so the launch can be
    captured into a graph (the relation-likelihood pass)."""
    lib, ctx, st = _env(q_out)
    rows = q_out.shape[0]
    qp, qs = _in(qkv, q_out.dtype)
    assert rope[0].shape[0] >= ctx_len and rope[0].shape[1] == head_dim // 2
    if rope_pos is not None and rope_pos_bound is not None:
        if int(rope_pos_bound) > rope[0].shape[0]:
            raise PsgHipError(f"rope_kvwrite: rotary positions up to {int(rope_pos_bound) - 1} exceed the "
                              f"{rope[0].shape[0]}-row rotary table")
    elif rope_pos is not None:
        # positions of the reference's PADDED sequence may exceed the compact context length: the kernel indexes the
        # rotary tables with them unchecked, so bound them here (training forward only; one scalar read-back)
        top = int(rope_pos.max().item()) if rope_pos.numel() else -1
        if top >= rope[0].shape[0]:
            raise PsgHipError(f"rope_kvwrite: rotary position {top} exceeds the {rope[0].shape[0]}-row rotary table")
    if _gqa(heads, kv_heads):
        check(lib.psg_rope_kvwrite_gqa(ctx, qp, qs, _p(tok_pair, torch.int32), _p(tok_pos, torch.int32),
                                       _p(rope_pos, torch.int32), _p(rope[0], torch.float32), _p(rope[1], torch.float32),
                                       rows, heads, int(kv_heads), head_dim, ctx_len, _p(q_out), _p(k_cache, q_out.dtype),
                                       _p(v_cache, q_out.dtype), _dt(q_out), st), "psg_rope_kvwrite_gqa")
        return q_out
    check(lib.psg_rope_kvwrite(ctx, qp, qs, _p(tok_pair, torch.int32), _p(tok_pos, torch.int32),
                               _p(rope_pos, torch.int32), _p(rope[0], torch.float32), _p(rope[1], torch.float32), rows, heads, head_dim, ctx_len, _p(q_out),
                               _p(k_cache, q_out.dtype), _p(v_cache, q_out.dtype), _dt(q_out), st), "psg_rope_kvwrite")
    return q_out


def llm_attn(q, k_cache, v_cache, tok_pair, tok_pos, heads, head_dim, ctx_len, out, kv_heads=None):
    lib, ctx, st = _env(q)
    if _gqa(heads, kv_heads):
        check(lib.psg_llm_attn_gqa(ctx, _p(q), _p(k_cache, q.dtype), _p(v_cache, q.dtype), _p(tok_pair, torch.int32),
                                   _p(tok_pos, torch.int32), q.shape[0], heads, int(kv_heads), head_dim, ctx_len,
                                   _p(out, q.dtype), _dt(q), st), "psg_llm_attn_gqa")
        return out
    check(lib.psg_llm_attn(ctx, _p(q), _p(k_cache, q.dtype), _p(v_cache, q.dtype), _p(tok_pair, torch.int32),
                           _p(tok_pos, torch.int32), q.shape[0], heads, head_dim, ctx_len, _p(out, q.dtype), _dt(q),
                           st), "psg_llm_attn")
    return out


def prefill_attn(q, k_cache, v_cache, tok_pos, pairs, rows_per_pair, heads, head_dim, ctx_len, out, kv_heads=None):
    """Causal attention of a pair-major prompt batch on the matrix cores (bf16 / fp16 / exact fp32, rows_per_pair <= 64).
    kv_heads < heads: grouped-query attention over caches [pairs, kv_heads, ctx, head_dim] (psg_prefill_attn_gqa)."""
    lib, ctx, st = _env(q)
    assert q.shape[0] == pairs * rows_per_pair
    if _gqa(heads, kv_heads):
        check(lib.psg_prefill_attn_gqa(ctx, _p(q, name="q"), _p(k_cache, q.dtype), _p(v_cache, q.dtype),
                                       _p(tok_pos, torch.int32), pairs, rows_per_pair, heads, int(kv_heads), head_dim,
                                       ctx_len, _p(out, q.dtype), _dt(q), st), "psg_prefill_attn_gqa")
        return out
    check(lib.psg_prefill_attn(ctx, _p(q, name="q"), _p(k_cache, q.dtype), _p(v_cache, q.dtype),
                               _p(tok_pos, torch.int32), pairs, rows_per_pair, heads, head_dim, ctx_len,
                               _p(out, q.dtype), _dt(q), st), "psg_prefill_attn")
    return out


def tree_attn(q, k_cache, v_cache, row_pair, row_node, prefix_len, anc, trie_base, heads, head_dim, ctx_len, out,
              kv_heads=None):
    """Attention of token-trie rows (psg_tree_attn): row r of pair row_pair[r] at trie node row_node[r] attends to the
    pair's prompt slots [0, prefix_len[pair]) and to slots trie_base + anc[node][d] (ancestors, then the node itself;
    anc int32 [n_int, max_depth], -1 padded).  q / out [rows, heads * head_dim], caches [pairs, kv_heads, ctx, head_dim]:
    all fp32 (exact) or all 16-bit."""
    lib, ctx, st = _env(q)
    kv = heads if kv_heads is None else int(kv_heads)
    n_int, max_depth = anc.shape
    pairs = k_cache.shape[0]
    assert q.shape[1] == heads * head_dim and tuple(k_cache.shape) == (pairs, kv, ctx_len, head_dim)
    assert prefix_len.numel() == pairs and row_pair.numel() == q.shape[0] == row_node.numel()
    check(lib.psg_tree_attn(ctx, _p(q, name="q"), _p(k_cache, q.dtype), _p(v_cache, q.dtype), _p(row_pair, torch.int32),
                            _p(row_node, torch.int32), _p(prefix_len, torch.int32), _p(anc, torch.int32), n_int, max_depth,
                            int(trie_base), q.shape[0], heads, kv, pairs, head_dim, ctx_len, _p(out, q.dtype), _dt(q), st),
          "psg_tree_attn")
    return out


def token_logprobs(logits, row_node, row_out, child_off, child_tok, out, dtype=None):
    """logit[tok] - logsumexp(logit row) for the trie children of every logit row (psg_token_logprobs).  logits [rows,
    vocab] (fp32 / 16-bit) or `Partials` (summed in slice order); row_node int32 [rows], row_out int64 [rows] = flat index
    in `out` (fp32) of the row's first child; child_off int32 [n_nodes + 1] / child_tok int32 [n_edges]: CSR lists."""
    lib, ctx, st = _env(out)
    rows, vocab = logits.shape
    if isinstance(logits, Partials):
        lp, ls, dt = _p(logits.t), logits.splits, PSG_F32
    else:
        lp, ls, dt = _p(logits), 0, _dt(logits)
    assert row_node.numel() == rows == row_out.numel()
    check(lib.psg_token_logprobs(ctx, lp, ls, rows, vocab, _p(row_node, torch.int32), _p(row_out, torch.int64),
                                 _p(child_off, torch.int32), _p(child_tok, torch.int32), child_off.numel() - 1,
                                 child_tok.numel(), _p(out, torch.float32), out.numel(), dt, st), "psg_token_logprobs")
    return out


def prefill_attn_rope(qkv, tok_pos, rope, pairs, rows_per_pair, heads, head_dim, ctx_len, k_cache, v_cache, out,
                      kv_heads=None):
    """Rotary + KV-cache write + causal attention of a pair-major prompt batch in one launch (bf16 / fp16).
    kv_heads < heads: grouped-query attention (psg_prefill_attn_rope_gqa)."""
    lib, ctx, st = _env(out)
    kv = heads if kv_heads is None else int(kv_heads)
    assert qkv.shape == (pairs * rows_per_pair, (heads + 2 * kv) * head_dim) and rope[0].shape[1] == head_dim // 2
    assert rope[0].shape[0] >= rows_per_pair
    if _gqa(heads, kv_heads):
        check(lib.psg_prefill_attn_rope_gqa(ctx, _p(qkv, out.dtype, "qkv"), _p(tok_pos, torch.int32),
                                            _p(rope[0], torch.float32), _p(rope[1], torch.float32), pairs, rows_per_pair,
                                            heads, kv, head_dim, ctx_len, _p(k_cache, out.dtype), _p(v_cache, out.dtype),
                                            _p(out), _dt(out), st), "psg_prefill_attn_rope_gqa")
        return out
    check(lib.psg_prefill_attn_rope(ctx, _p(qkv, out.dtype, "qkv"), _p(tok_pos, torch.int32),
                                    _p(rope[0], torch.float32), _p(rope[1], torch.float32), pairs, rows_per_pair, heads,
                                    head_dim, ctx_len, _p(k_cache, out.dtype), _p(v_cache, out.dtype), _p(out),
                                    _dt(out), st), "psg_prefill_attn_rope")
    return out


def decode_attn(qkv, tok_pair, tok_pos, rope, heads, head_dim, ctx_len, k_cache, v_cache, out, kv_heads=None):
    """Fused rotary + KV append + attention for rows that each hold the newest token of their pair.
    kv_heads < heads: grouped-query attention (psg_decode_attn_gqa: one workgroup streams a key / value head's cache once
    for the query heads of its group)."""
    lib, ctx, st = _env(out)
    qp, qs = _in(qkv, out.dtype)
    assert rope[0].shape[0] >= ctx_len and rope[0].shape[1] == head_dim // 2
    if _gqa(heads, kv_heads):
        rows = out.shape[0]
        assert tuple(qkv.shape)[-2:] == (rows, (heads + 2 * int(kv_heads)) * head_dim)
        assert k_cache.shape[1] == int(kv_heads) and k_cache.shape[2] >= ctx_len and v_cache.shape == k_cache.shape
        check(lib.psg_decode_attn_gqa(ctx, qp, qs, _p(tok_pair, torch.int32), _p(tok_pos, torch.int32),
                                      _p(rope[0], torch.float32), _p(rope[1], torch.float32), rows, heads, int(kv_heads),
                                      head_dim, ctx_len, _p(k_cache, out.dtype), _p(v_cache, out.dtype), _p(out), _dt(out),
                                      st), "psg_decode_attn_gqa")
        return out
    check(lib.psg_decode_attn(ctx, qp, qs, _p(tok_pair, torch.int32), _p(tok_pos, torch.int32),
                              _p(rope[0], torch.float32), _p(rope[1], torch.float32), out.shape[0], heads, head_dim, ctx_len,
                              _p(k_cache, out.dtype), _p(v_cache, out.dtype), _p(out), _dt(out), st), "psg_decode_attn")
    return out


def decode_layer_supported(rows, hidden, inter, heads, dtype, device) -> bool:
    """Does psg_decode_layer (one persistent launch per decoder layer of the decode step) take this shape?"""
    if dtype not in _DT or not torch.device(device).type == "cuda":
        return False
    dev = torch.device(device)
    lib, ctx = _lib.load(), _lib.ctx(dev.index or 0)
    return bool(lib.psg_decode_layer_supported(ctx, int(rows), int(hidden), int(inter), int(heads), _DT[dtype]))


DL_TIMEOUT_WORD = 255 * 64         # csrc/psg_decode_layer.hip: PSG_DL_TIMEOUT * PSG_DL_SLOT - set by a hand-off poll that gave up


def decode_layer_counters(device) -> int:
    """int32 words of one psg_decode_layer launch's counter block (to be zeroed by the caller)."""
    import ctypes
    dev = torch.device(device)
    lib, ctx = _lib.load(), _lib.ctx(dev.index or 0)
    nf, nc = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.psg_decode_layer_workspace(ctx, 16, 4096, 11008, ctypes.byref(nf), ctypes.byref(nc)),
          "psg_decode_layer_workspace")
    return int(nc.value)


def decode_layer_workspace(rows, hidden, inter, device):
    """(workspace fp32 tensor, counter words per launch) of psg_decode_layer for `rows` decode rows."""
    import ctypes
    dev = torch.device(device)
    lib, ctx = _lib.load(), _lib.ctx(dev.index or 0)
    nf, nc = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.psg_decode_layer_workspace(ctx, int(rows), int(hidden), int(inter), ctypes.byref(nf), ctypes.byref(nc)),
          "psg_decode_layer_workspace")
    return torch.empty(nf.value, device=dev, dtype=torch.float32), int(nc.value)


def decode_layer(resid, delta, ln1, ln2, wqkv, wo, wgu, wdown, tok_pair, tok_pos, rope, heads, ctx_len, eps, k_cache,
                 v_cache, workspace, counters, down_part) -> Partials:
    """One decoder layer of the decode step in ONE persistent launch (psg_decode_layer), bit-identical to
    rmsnorm -> skinny_gemm -> decode_attn -> skinny_gemm -> rmsnorm -> skinny_gemm -> silu_mul -> skinny_gemm.
    resid [M, hidden] fp32 (updated in place); delta: the previous layer's down-projection Partials or None;
    counters: int32 [decode_layer_counters()], ZERO (word 255 * 64 != 0 afterwards: a bounded poll gave up); down_part fp32 [16, M, hidden] receives this layer's down partials (returned)."""
    lib, ctx, st = _env(resid)
    M, hidden = resid.shape
    inter = wdown.shape[1]
    assert wqkv.shape == (3 * hidden, hidden) and wo.shape == (hidden, hidden) and wgu.shape == (2 * inter, hidden)
    assert down_part.shape == (16, M, hidden) and counters.dtype == torch.int32
    assert counters.numel() >= decode_layer_counters(resid.device)
    dp, ds = (None, 0) if delta is None else _in(delta, resid.dtype)
    check(lib.psg_decode_layer(ctx, _p(resid, torch.float32, "resid"), dp, ds, _p(ln1, torch.float32), _p(ln2, torch.float32),
                               _p(wqkv, resid.dtype, "wqkv"), _p(wo, resid.dtype), _p(wgu, resid.dtype), _p(wdown, resid.dtype),
                               _p(tok_pair, torch.int32), _p(tok_pos, torch.int32), _p(rope[0], torch.float32),
                               _p(rope[1], torch.float32), M, hidden, inter, int(heads), int(ctx_len), float(eps),
                               _p(k_cache, resid.dtype), _p(v_cache, resid.dtype), _p(workspace, torch.float32),
                               _p(counters), _p(down_part, torch.float32), _dt(resid), st), "psg_decode_layer")
    return Partials(down_part)


def decode_layer_table(layers, k_caches, v_caches, device=None):
    """Table for `decode_layers`: one row of 8 pointers per decoder layer (the tensors must outlive it); on the layers'
    device unless `device` says otherwise (a caller inside a graph capture stages it through pinned memory)."""
    rows = [[L["ln1"].data_ptr(), L["ln2"].data_ptr(), L["wqkv"].data_ptr(), L["wo"].data_ptr(), L["wgu"].data_ptr(),
             L["wdown"].data_ptr(), k.data_ptr(), v.data_ptr()] for L, k, v in zip(layers, k_caches, v_caches)]
    return torch.tensor(rows, dtype=torch.int64, device=layers[0]["wqkv"].device if device is None else device)


def decode_layers(resid, delta, table, n_layers, tok_pair, tok_pos, rope, heads, ctx_len, eps, inter, workspace, counters,
                  down_parts) -> Partials:
    """All decoder layers of a decode step chained inside ONE persistent launch (psg_decode_layers).
    table: `decode_layer_table`; counters int32 [n_layers * decode_layer_counters()], ZERO; down_parts fp32 [2, 16, M, hidden].
    Returns the last layer's down-projection Partials (for the final rmsnorm)."""
    lib, ctx, st = _env(resid)
    M, hidden = resid.shape
    assert down_parts.shape == (2, 16, M, hidden) and counters.dtype == torch.int32
    assert counters.numel() >= n_layers * decode_layer_counters(resid.device) and table.shape == (n_layers, 8)
    dp, ds = (None, 0) if delta is None else _in(delta, resid.dtype)
    check(lib.psg_decode_layers(ctx, _p(resid, torch.float32, "resid"), dp, ds, _p(table), int(n_layers),
                                _p(tok_pair, torch.int32), _p(tok_pos, torch.int32), _p(rope[0], torch.float32),
                                _p(rope[1], torch.float32), M, hidden, int(inter), int(heads), int(ctx_len), float(eps),
                                _p(workspace, torch.float32), _p(counters), _p(down_parts, torch.float32), _dt(resid), st),
          "psg_decode_layers")
    return Partials(down_parts[(n_layers - 1) & 1])


def silu_mul(gate_up, out):
    lib, ctx, st = _env(out)
    rows, inter = out.shape
    gp, gs = _in(gate_up, out.dtype)
    check(lib.psg_silu_mul(ctx, gp, gs, rows, inter, _p(out), _dt(out), st), "psg_silu_mul")
    return out


def greedy_step(logits, step, max_new, eos, suppress_token, tokens, done, next_ids, tok_pos, dtype=None, embed=None,
                x_out=None):
    """embed [vocab, hidden] + x_out [K, hidden]: the chosen token's embedding row goes to x_out in the same launch (the
    next decode step's input; x_out may be fp32 next to a 16-bit table)."""
    lib, ctx, st = _env(tokens)
    K, vocab = logits.shape
    if isinstance(logits, Partials):
        lp, ls, dt = _p(logits.t), logits.splits, _DT[dtype or torch.bfloat16]
    else:
        lp, ls, dt = _p(logits), 0, _dt(logits)
    if x_out is not None:
        assert embed is not None and x_out.shape == (K, embed.shape[1])
        ep, ed, hid, xp, xd = _p(embed), _dt(embed), embed.shape[1], _p(x_out), _dt(x_out)
    else:
        ep, ed, hid, xp, xd = None, 0, 0, None, 0
    check(lib.psg_greedy_step(ctx, lp, ls, K, vocab, int(step), int(max_new), int(eos), int(suppress_token),
                              _p(tokens, torch.int32), _p(done, torch.int32), _p(next_ids, torch.int32),
                              _p(tok_pos, torch.int32), ep, ed, hid, xp, xd, dt, st), "psg_greedy_step")


def trie_greedy_step(logits, step, max_new, eos, tables, node, tokens, done, next_ids, tok_pos, logp=None, dtype=None,
                     embed=None, x_out=None):
    """`greedy_step` over the children of each row's trie node only (psg_trie_greedy_step).  tables: the device dict of a
    `rel_scores.RelationTrie` (child_off, child_tok, edge_node); node int32 [K]: the rows' trie nodes, advanced in place;
    logp fp32 [K] or None: gains logit[tok] - logsumexp(row) of the chosen edge, bit-equal to `token_logprobs`."""
    lib, ctx, st = _env(tokens)
    K, vocab = logits.shape
    if isinstance(logits, Partials):
        lp, ls, dt = _p(logits.t), logits.splits, _DT[dtype or torch.bfloat16]
    else:
        lp, ls, dt = _p(logits), 0, _dt(logits)
    if x_out is not None:
        assert embed is not None and x_out.shape == (K, embed.shape[1])
        ep, ed, hid, xp, xd = _p(embed), _dt(embed), embed.shape[1], _p(x_out), _dt(x_out)
    else:
        ep, ed, hid, xp, xd = None, 0, 0, None, 0
    co, ct, en = tables["child_off"], tables["child_tok"], tables["edge_node"]
    assert node.numel() == K and en.numel() == ct.numel() and (logp is None or logp.numel() == K)
    check(lib.psg_trie_greedy_step(ctx, lp, ls, K, vocab, int(step), int(max_new), int(eos), _p(co, torch.int32),
                                   _p(ct, torch.int32), _p(en, torch.int32), co.numel() - 1, ct.numel(),
                                   _p(node, torch.int32), None if logp is None else _p(logp, torch.float32),
                                   _p(tokens, torch.int32), _p(done, torch.int32), _p(next_ids, torch.int32),
                                   _p(tok_pos, torch.int32), ep, ed, hid, xp, xd, dt, st), "psg_trie_greedy_step")


BEAM_MAX_WIDTH = 8                 # include/psg_hip.h: PSG_BEAM_MAX_WIDTH


def trie_beam_step(logits, B, beams_in, eos, tables, trie_base, seq_len, node, logp, fin_class, fin_logp, row_node, tok_pos,
                   rope_pos, embed=None, x_out=None):
    """One level of a width-B beam over a relation trie (psg_trie_beam_step).  logits [K * beams_in, vocab]
    (fp32 / 16-bit) or `Partials`; beams_in = 1 (the pairs' root rows) or B.  tables: the device dict of a
    `rel_scores.RelationTrie` (child_off, child_tok, edge_node, edge_class, node_tok, node_depth, max_children).  State, read
    and written: node int32 [K * B] (CSR node, -1 = dead), logp fp32 [K * B], fin_class int32 [K, B], fin_logp fp32 [K, B].
    Written for the next level's rows: row_node / tok_pos / rope_pos int32 [K * B], x_out [K * B, hidden] = embed[token]."""
    lib, ctx, st = _env(node)
    rows, vocab = logits.shape
    B, beams_in = int(B), int(beams_in)
    if not 1 <= B <= BEAM_MAX_WIDTH:
        raise PsgHipError(f"trie_beam_step: beam width B={B} must be in 1..{BEAM_MAX_WIDTH}")
    if beams_in not in (1, B):
        raise PsgHipError(f"trie_beam_step: beams_in={beams_in} must be 1 or B={B}")
    if rows % beams_in:
        raise PsgHipError(f"trie_beam_step: {rows} logit rows are no multiple of beams_in={beams_in}")
    K = rows // beams_in
    if isinstance(logits, Partials):
        lp, ls, dt = _p(logits.t), logits.splits, PSG_F32
    else:
        lp, ls, dt = _p(logits), 0, _dt(logits)
    if x_out is not None:
        assert embed is not None and x_out.shape == (K * B, embed.shape[1])
        ep, ed, hid, xp, xd = _p(embed), _dt(embed), embed.shape[1], _p(x_out), _dt(x_out)
    else:
        ep, ed, hid, xp, xd = None, 0, 0, None, 0
    co, ct, en = tables["child_off"], tables["child_tok"], tables["edge_node"]
    ec, nt, ndp = tables.get("edge_class"), tables.get("node_tok"), tables.get("node_depth")
    assert en.numel() == ct.numel() and (ec is None or ec.numel() == ct.numel())
    assert nt is None or ndp is None or nt.numel() == ndp.numel() == co.numel() - 2
    assert seq_len.numel() == K and fin_class.numel() == K * B == fin_logp.numel()
    assert all(t.numel() == K * B for t in (node, logp, row_node, tok_pos, rope_pos))
    i32 = torch.int32
    check(lib.psg_trie_beam_step(ctx, lp, ls, K, B, beams_in, vocab, int(eos), _p(co, i32), _p(ct, i32), _p(en, i32),
                                 _p(ec, i32), _p(nt, i32), _p(ndp, i32), co.numel() - 1, ct.numel(), int(tables["max_children"]), int(trie_base),
                                 _p(seq_len, torch.int32), _p(node, torch.int32), _p(logp, torch.float32),
                                 _p(fin_class, torch.int32), _p(fin_logp, torch.float32), _p(row_node, torch.int32),
                                 _p(tok_pos, torch.int32), _p(rope_pos, torch.int32), ep, ed, hid, xp, xd, dt, st),
          "psg_trie_beam_step")


def skinny_gemm_plan(M, N, K, dtype, device) -> int:
    """Split count psg_skinny_gemm would use for x [M, K] of `dtype` against w [N, K]; raises PsgHipError where the kernel
    does not take the shape (psg_skinny_gemm_plan: row count, divisibility, the fp32 kernel's LDS bound)."""
    import ctypes
    lib = _lib.load()
    dev = torch.device(device)
    s = ctypes.c_int(0)
    check(lib.psg_skinny_gemm_plan(_lib.ctx(dev.index or 0), int(M), int(N), int(K), _DT[dtype], ctypes.byref(s)),
          "psg_skinny_gemm_plan")
    return s.value


def skinny_gemm(x, w, splits=None, part=None) -> Partials:
    """Decode-step projection: fp32 split-K partials of x @ w.T (x: <= 32 rows of bf16 / fp16 / fp32, w of the
    same type); every weight byte streams from HBM once.  Hand the result to a consumer kernel or call .reduce().
    part: the caller's [splits, M, N] fp32 buffer for the partials (contiguous, 16-byte aligned: the kernels store
    float4); None = a fresh allocation."""
    lib, ctx, st = _env(x)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    if x.dtype not in _DT or w.dtype != x.dtype:
        raise PsgHipError(f"skinny_gemm: x / w must both be bf16, fp16 or fp32, got {x.dtype} / {w.dtype}")
    if splits is None:
        import ctypes
        s = ctypes.c_int(0)
        check(lib.psg_skinny_gemm_plan(ctx, M, N, K, _dt(x), ctypes.byref(s)), "psg_skinny_gemm_plan")
        splits = s.value
    if part is None:
        part = torch.empty((splits, M, N), device=x.device, dtype=torch.float32)
    elif tuple(part.shape) != (splits, M, N) or part.device != x.device:
        raise PsgHipError(f"skinny_gemm: part must be [{splits}, {M}, {N}] on {x.device}, got {tuple(part.shape)} on "
                          f"{part.device}")
    elif _p(part, torch.float32, "part") % 16:
        raise PsgHipError("skinny_gemm: part must be 16-byte aligned")
    check(lib.psg_skinny_gemm(ctx, _p(x, name="x"), _p(w, name="w"), _p(part), M, N, K, splits, _dt(x), st),
          "psg_skinny_gemm")
    return Partials(part)


def skinny_gemm_w16(x, w16, splits=None) -> Partials:
    """`skinny_gemm` of fp32 rows against weights STORED as fp16 (values that are fp16 numbers: a frozen fp16 checkpoint
    upcast on load): bit-identical to skinny_gemm(x, w16.float()) at half the weight bytes (psg_skinny_gemm_w16)."""
    import ctypes
    lib, ctx, st = _env(x)
    M, K = x.shape
    N = w16.shape[0]
    assert w16.shape[1] == K
    if x.dtype != torch.float32 or w16.dtype != torch.float16:
        raise PsgHipError(f"skinny_gemm_w16: x must be fp32 and w fp16, got {x.dtype} / {w16.dtype}")
    if splits is None:
        s = ctypes.c_int(0)
        check(lib.psg_skinny_gemm_plan(ctx, M, N, K, _DT[torch.float32], ctypes.byref(s)), "psg_skinny_gemm_plan")
        splits = s.value
    part = torch.empty((splits, M, N), device=x.device, dtype=torch.float32)
    check(lib.psg_skinny_gemm_w16(ctx, _p(x, name="x"), _p(w16, name="w"), _p(part), M, N, K, splits, st),
          "psg_skinny_gemm_w16")
    return Partials(part)


def split_f16x2(x):
    """fp32 rows -> (fp16 planes [2, rows, K]: high and low parts, inv_scale fp32 [rows]) - the operand of `split_gemm_w16`."""
    lib, ctx, st = _env(x)
    assert x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1
    rows, K = x.shape
    out = torch.empty((2, rows, K), device=x.device, dtype=torch.float16)
    inv = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(lib.psg_split_f16x2(ctx, x.data_ptr(), rows, K, x.stride(0), _p(out), _p(inv), st), "psg_split_f16x2")
    return out, inv


def rmsnorm_split2(resid, delta, w, eps):
    """resid (fp32) += delta (Partials or None); RMSNorm(resid) * w as the two fp16 planes of `split_f16x2`:
    (fp16 [2, rows, hidden], inv_scale) - psg_rmsnorm + psg_split_f16x2 in one launch, bit-identical."""
    lib, ctx, st = _env(resid)
    rows, hidden = resid.shape
    assert resid.dtype == torch.float32 and (delta is None or isinstance(delta, Partials))
    out = torch.empty((2, rows, hidden), device=resid.device, dtype=torch.float16)
    inv = torch.empty(rows, device=resid.device, dtype=torch.float32)
    dp, ds = (None, 0) if delta is None else (_p(delta.t, torch.float32), delta.splits)
    check(lib.psg_rmsnorm_split2(ctx, _p(resid), dp, ds, _p(w, torch.float32), float(eps), rows, hidden, _p(out), _p(inv), st),
          "psg_rmsnorm_split2")
    return out, inv


def split_gemm_w16(x2, inv_scale, w16, mode=0) -> Partials:
    """Decode-step projection of fp32 rows against a weight that is an fp16 value (frozen fp16 checkpoint): two fp16
    products (high and low part of x) on the 16-bit matrix cores, fp32 slices [S, M, N] like `skinny_gemm`'s;
    2^-22 relative against the fp32 product (psg_split_gemm_w16).  x2, inv_scale from `split_f16x2`."""
    import ctypes
    lib, ctx, st = _env(x2)
    _, M, K = x2.shape
    N = w16.shape[0]
    assert x2.shape[0] == 2 and w16.shape[1] == K and x2.dtype == torch.float16 and w16.dtype == torch.float16
    s = ctypes.c_int(0)
    check(lib.psg_split_gemm_w16_plan(ctx, M, N, K, int(mode), ctypes.byref(s)), "psg_split_gemm_w16_plan")
    part = torch.empty((s.value, M, N), device=x2.device, dtype=torch.float32)
    check(lib.psg_split_gemm_w16(ctx, _p(x2), _p(inv_scale, torch.float32), _p(w16), _p(part), M, N, K, s.value, int(mode), st),
          "psg_split_gemm_w16")
    return Partials(part)


def _rows_f32(name, x):
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1):
        raise PsgHipError(f"{name}: x must be fp32 [rows, K] with contiguous rows, got "
                          f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    return x.shape


def split_b16x3(x):
    """fp32 rows -> bf16 planes [3, rows, K] with x == x0 + x1 + x2 EXACTLY (x0 = bf16(x), x1 = bf16(x - x0), x2 =
    bf16(x - x0 - x1), round to nearest even; no row scale) - the operand of `split_gemm_wb16` (psg_split_b16x3)."""
    rows, K = _rows_f32("split_b16x3", x)
    lib, ctx, st = _env(x)
    if K % 4 or x.stride(0) % 4 or x.data_ptr() % 16:
        raise PsgHipError(f"split_b16x3: K={K} and the row stride {x.stride(0)} must be multiples of 4, x 16-byte aligned")
    out = torch.empty((3, rows, K), device=x.device, dtype=torch.bfloat16)
    check(lib.psg_split_b16x3(ctx, x.data_ptr(), rows, K, x.stride(0), _p(out), st), "psg_split_b16x3")
    return out


def rmsnorm_split_b16x3(resid, delta, w, eps):
    """resid (fp32) += delta (Partials or None); RMSNorm(resid) * w as the three bf16 planes of `split_b16x3`, bf16
    [3, rows, hidden] - psg_rmsnorm + psg_split_b16x3 in one launch, bit-identical (psg_rmsnorm_split_b16x3)."""
    rows, hidden = _rows_f32("rmsnorm_split_b16x3", resid)
    lib, ctx, st = _env(resid)
    if not resid.is_contiguous() or not (delta is None or isinstance(delta, Partials)):
        raise PsgHipError("rmsnorm_split_b16x3: resid must be contiguous and delta a Partials (fp32 split-K slices) or None")
    if delta is not None and tuple(delta.t.shape[1:]) != (rows, hidden):
        raise PsgHipError(f"rmsnorm_split_b16x3: delta slices {tuple(delta.t.shape)} do not match resid [{rows}, {hidden}]")
    if w.numel() != hidden:
        raise PsgHipError(f"rmsnorm_split_b16x3: w has {w.numel()} elements, hidden is {hidden}")
    out = torch.empty((3, rows, hidden), device=resid.device, dtype=torch.bfloat16)
    dp, ds = (None, 0) if delta is None else (_p(delta.t, torch.float32), delta.splits)
    check(lib.psg_rmsnorm_split_b16x3(ctx, _p(resid), dp, ds, _p(w, torch.float32), float(eps), rows, hidden, _p(out), st),
          "psg_rmsnorm_split_b16x3")
    return out


def silu_mul_split_b16x3(gate_up):
    """silu(gate) * up of a gate|up projection result [rows, 2 inter] - Partials (fp32 split-K slices, summed in slice order)
    or a dense fp32 tensor - as the three bf16 planes of `split_b16x3`, bf16 [3, rows, inter]: `silu_mul` into fp32 rows +
    psg_split_b16x3 in one launch, bit-identical (psg_silu_mul_split_b16x3)."""
    t = gate_up.t if isinstance(gate_up, Partials) else gate_up
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()
            and t.dim() == (3 if isinstance(gate_up, Partials) else 2) and t.shape[-1] % 8 == 0):
        raise PsgHipError("silu_mul_split_b16x3: gate_up must be fp32 split-K slices [S, rows, 2 inter] (Partials) or dense "
                          f"fp32 rows [rows, 2 inter] with inter a multiple of 4, got {getattr(t, 'dtype', type(t))} "
                          f"{tuple(getattr(t, 'shape', ()))}")
    lib, ctx, st = _env(t)
    rows, inter = t.shape[-2], t.shape[-1] // 2
    out = torch.empty((3, rows, inter), device=t.device, dtype=torch.bfloat16)
    splits = gate_up.splits if isinstance(gate_up, Partials) else 0
    check(lib.psg_silu_mul_split_b16x3(ctx, _p(t), splits, rows, inter, _p(out), st), "psg_silu_mul_split_b16x3")
    return out


def split_gemm_wb16_plan(M, N, K, device, mode=0) -> int:
    """Slices `split_gemm_wb16` writes for x3 [3, M, K] against w [N, K]; raises where the kernel does not take the shape."""
    import ctypes
    lib = _lib.load()
    dev = torch.device(device)
    s = ctypes.c_int(0)
    check(lib.psg_split_gemm_wb16_plan(_lib.ctx(dev.index or 0), int(M), int(N), int(K), int(mode), ctypes.byref(s)),
          "psg_split_gemm_wb16_plan")
    return s.value


def split_gemm_wb16(x3, wb16, mode=0, part=None) -> Partials:
    """Decode-step projection of fp32 rows against a weight that is a bf16 value (a bf16 checkpoint upcast on load): three
    bf16 products (the planes of `split_b16x3`, x0 + x1 + x2 == x exactly) on the 16-bit matrix cores, fp32 slices
    [S, M, N] like `skinny_gemm`'s.  Every product is exact in fp32: only the fp32 accumulation separates the result from
    the exact one (psg_split_gemm_wb16).  M <= 32, N % 16 == 0, K % 64 == 0, 16-byte aligned operands.
    part: the caller's [S, M, N] fp32 buffer (S = `split_gemm_wb16_plan`); None = a fresh allocation."""
    if not (isinstance(x3, torch.Tensor) and x3.dim() == 3 and x3.shape[0] == 3 and x3.dtype == torch.bfloat16
            and x3.is_contiguous()):
        raise PsgHipError("split_gemm_wb16: x3 must be the contiguous bf16 planes [3, M, K] of split_b16x3, got "
                          f"{getattr(x3, 'dtype', type(x3))} {tuple(getattr(x3, 'shape', ()))}")
    _, M, K = x3.shape
    if not (isinstance(wb16, torch.Tensor) and wb16.dim() == 2 and wb16.dtype == torch.bfloat16 and wb16.shape[1] == K
            and wb16.is_contiguous() and wb16.device == x3.device):
        raise PsgHipError(f"split_gemm_wb16: w must be contiguous bf16 [N, {K}] on {x3.device}, got "
                          f"{getattr(wb16, 'dtype', type(wb16))} {tuple(getattr(wb16, 'shape', ()))}")
    lib, ctx, st = _env(x3)
    N = wb16.shape[0]
    S = split_gemm_wb16_plan(M, N, K, x3.device, mode)
    if part is None:
        part = torch.empty((S, M, N), device=x3.device, dtype=torch.float32)
    elif (tuple(part.shape) != (S, M, N) or part.dtype != torch.float32 or part.device != x3.device
          or not part.is_contiguous()):
        raise PsgHipError(f"split_gemm_wb16: part must be contiguous fp32 [{S}, {M}, {N}] on {x3.device} (slots = the plan's), "
                          f"got {part.dtype} {tuple(part.shape)}")
    check(lib.psg_split_gemm_wb16(ctx, _p(x3), _p(wb16), _p(part), M, N, K, S, int(mode), st), "psg_split_gemm_wb16")
    return Partials(part)


def _w8_args(name, w8, col_scale, K):
    if w8.dtype not in (torch.uint8, torch.float8_e4m3fn) or w8.dim() != 2 or w8.shape[1] != K:
        raise PsgHipError(f"{name}: w8 must be e4m3fn bytes [N, {K}] (uint8 / float8_e4m3fn), got {w8.dtype} {tuple(w8.shape)}")
    if col_scale.dtype != torch.float32 or tuple(col_scale.shape) != (w8.shape[0],):
        raise PsgHipError(f"{name}: col_scale must be fp32 [{w8.shape[0]}], got {col_scale.dtype} {tuple(col_scale.shape)}")
    return w8.shape[0]


def split_gemm_w8(x2, inv_scale, w8, col_scale, mode=0) -> Partials:
    """`split_gemm_w16` over an FP8-quantised weight W' = e4m3(w8) * col_scale[:, None] (weights.quantize_fp8_rows): one byte
    per weight from HBM, widened exactly to fp16 in registers; fp32 slices [S, M, N] of (xh . q + xl . q) * inv_scale *
    col_scale (psg_split_gemm_w8).  K % 128 == 0.  mode 1 / 2: slab-aligned / stream-K ranges, 0 = the library's estimate."""
    import ctypes
    lib, ctx, st = _env(x2)
    _, M, K = x2.shape
    assert x2.shape[0] == 2 and x2.dtype == torch.float16
    N = _w8_args("split_gemm_w8", w8, col_scale, K)
    s = ctypes.c_int(0)
    check(lib.psg_split_gemm_w8_plan(ctx, M, N, K, int(mode), ctypes.byref(s)), "psg_split_gemm_w8_plan")
    part = torch.empty((s.value, M, N), device=x2.device, dtype=torch.float32)
    check(lib.psg_split_gemm_w8(ctx, _p(x2), _p(inv_scale, torch.float32), _p(w8, name="w8"), _p(col_scale), _p(part), M, N, K,
                                s.value, int(mode), st), "psg_split_gemm_w8")
    return Partials(part)


def skinny_gemm_w8(x, w8, col_scale, mode=0) -> Partials:
    """`skinny_gemm` of <= 32 bf16 / fp16 rows over an FP8-quantised weight W' = e4m3(w8) * col_scale[:, None]: one byte per
    weight from HBM, widened exactly to x's type in registers; fp32 slices [S, M, N] of (x . q) * col_scale
    (psg_skinny_gemm_w8).  K % 128 == 0."""
    import ctypes
    lib, ctx, st = _env(x)
    M, K = x.shape
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise PsgHipError(f"skinny_gemm_w8: x must be bf16 or fp16, got {x.dtype}")
    N = _w8_args("skinny_gemm_w8", w8, col_scale, K)
    s = ctypes.c_int(0)
    check(lib.psg_skinny_gemm_w8_plan(ctx, M, N, K, _dt(x), int(mode), ctypes.byref(s)), "psg_skinny_gemm_w8_plan")
    part = torch.empty((s.value, M, N), device=x.device, dtype=torch.float32)
    check(lib.psg_skinny_gemm_w8(ctx, _p(x, name="x"), _p(w8, name="w8"), _p(col_scale), _p(part), M, N, K, s.value, _dt(x),
                                 int(mode), st), "psg_skinny_gemm_w8")
    return Partials(part)


def mxfp4_exp_image(e) -> torch.Tensor:
    """The block exponents e uint8 [N, K / 32] of an MXFP4 matrix (weights.quantize_mxfp4_rows), K % 256 == 0, re-laid-out
    for psg_gemm_w4.hip's K step of 256: uint8 [K / 256, N, 2, 4] with [t, n, h, j] = e[n, 8 t + 2 j + h].  The exponents
    of 32 consecutive rows of one step are then 256 contiguous bytes (one LDS-DMA per wave) and the four a lane needs
    one dword."""
    N, B = e.shape
    if e.dtype != torch.uint8 or B % 8:
        raise PsgHipError(f"mxfp4_exp_image: e must be uint8 [N, K / 32] with K % 256 == 0, got {e.dtype} {tuple(e.shape)}")
    return e.reshape(N, B // 8, 4, 2).permute(1, 0, 3, 2).contiguous()


def _expand_out(name, N, K, s, out, dtype, device):
    """The [N, K] result of an expansion: `out`'s first N * K elements (any contiguous buffer of the result's dtype that is
    large enough - the engine's scratch) or a fresh tensor.  The unscaled form (s None) is fp16."""
    dtype = torch.float16 if s is None else (dtype or (out.dtype if out is not None else torch.float32))
    if s is None and out is not None and out.dtype != torch.float16:
        raise PsgHipError(f"{name}: the unscaled form (s None) is fp16, out is {out.dtype}")
    if s is not None and (s.dtype != torch.float32 or tuple(s.shape) != (N,)):
        raise PsgHipError(f"{name}: s must be fp32 [{N}], got {s.dtype} {tuple(s.shape)}")
    if out is None:
        return torch.empty((N, K), device=device, dtype=dtype)
    if out.dtype != dtype or not out.is_contiguous() or out.numel() < N * K:
        raise PsgHipError(f"{name}: out must be a contiguous {dtype} buffer of >= {N * K} elements, got {out.dtype} "
                          f"{tuple(out.shape)}")
    return out.view(-1)[:N * K].view(N, K)


def expand_w8(q, s=None, out=None, dtype=None) -> torch.Tensor:
    """The dense operand of an FP8-quantised matrix (psg_expand_w8).  q: e4m3fn bytes [N, K] (uint8 /
    float8_e4m3fn), K % 32 == 0.  s None: float16(q), exact.  s fp32 [N]: W' = float32(q) * s[:, None] rounded once into
    `dtype` (fp32 / fp16 / bf16; default `out`'s, else fp32) - weights.dequantize_fp8_rows bit for bit.  Returns [N, K]: a
    view of `out`'s head when a buffer is given (elements behind N * K are not touched)."""
    lib, ctx, st = _env(q)
    if q.dtype not in (torch.uint8, torch.float8_e4m3fn) or q.dim() != 2:
        raise PsgHipError(f"expand_w8: q must be e4m3fn bytes [N, K] (uint8 / float8_e4m3fn), got {q.dtype} {tuple(q.shape)}")
    N, K = q.shape
    y = _expand_out("expand_w8", N, K, s, out, dtype, q.device)
    check(lib.psg_expand_w8(ctx, _p(q, name="q"), _p(s), _p(y), N, K, _dt(y), st), "psg_expand_w8")
    return y


def expand_w4(q, e, s=None, out=None, dtype=None) -> torch.Tensor:
    """`expand_w8` for an MXFP4-quantised matrix (psg_expand_w4): q fp4 nibbles uint8 [N, K / 2] (low nibble = even k), e the
    model's RAW block exponents uint8 [N, K / 32] in 114..127 (not `mxfp4_exp_image`).  s None: fp4(q) * 2^(e - 127) as
    fp16, exact.  s fp32 [N]: weights.dequantize_mxfp4_rows(q, e, s, dtype) bit for bit."""
    lib, ctx, st = _env(q)
    if q.dtype != torch.uint8 or q.dim() != 2:
        raise PsgHipError(f"expand_w4: q must be fp4 nibbles uint8 [N, K / 2], got {q.dtype} {tuple(q.shape)}")
    N, K = q.shape[0], 2 * q.shape[1]
    if e.dtype != torch.uint8 or e.dim() != 2 or e.shape[0] != N or e.shape[1] * 32 != K:
        raise PsgHipError(f"expand_w4: e must be uint8 [{N}, K / 32] with K = {K}, got {e.dtype} {tuple(e.shape)}")
    y = _expand_out("expand_w4", N, K, s, out, dtype, q.device)
    check(lib.psg_expand_w4(ctx, _p(q, name="q"), _p(e, name="e"), _p(s), _p(y), N, K, _dt(y), st), "psg_expand_w4")
    return y


def _w4_args(name, w4, e_img, col_scale, K):
    if w4.dtype != torch.uint8 or w4.dim() != 2 or w4.shape[1] * 2 != K:
        raise PsgHipError(f"{name}: w4 must be fp4 nibbles uint8 [N, {K // 2}], got {w4.dtype} {tuple(w4.shape)}")
    N = w4.shape[0]
    if K % 256 == 0 and (e_img.dtype != torch.uint8 or tuple(e_img.shape) != (K // 256, N, 2, 4) or not e_img.is_contiguous()):
        raise PsgHipError(f"{name}: e_img must be mxfp4_exp_image(e): uint8 [{K // 256}, {N}, 2, 4], got {e_img.dtype} "
                          f"{tuple(e_img.shape)}")
    if col_scale.dtype != torch.float32 or tuple(col_scale.shape) != (N,):
        raise PsgHipError(f"{name}: col_scale must be fp32 [{N}], got {col_scale.dtype} {tuple(col_scale.shape)}")
    return N


def split_gemm_w4(x2, inv_scale, w4, e_img, col_scale, mode=0) -> Partials:
    """`split_gemm_w8` over an MXFP4-quantised weight W' = fp4(w4) * 2^(e - 127) * col_scale[:, None]
    (weights.quantize_mxfp4_rows; `e_img` = mxfp4_exp_image(e)): 4.25 bits per weight from HBM, widened exactly to fp16 with
    the block scale in registers; fp32 slices [S, M, N] of (xh . w + xl . w) * inv_scale * col_scale (psg_split_gemm_w4).
    K % 256 == 0.  mode 1 / 2: slab-aligned / stream-K ranges, 0 = the library's estimate."""
    import ctypes
    lib, ctx, st = _env(x2)
    _, M, K = x2.shape
    assert x2.shape[0] == 2 and x2.dtype == torch.float16
    N = _w4_args("split_gemm_w4", w4, e_img, col_scale, K)
    s = ctypes.c_int(0)
    check(lib.psg_split_gemm_w4_plan(ctx, M, N, K, int(mode), ctypes.byref(s)), "psg_split_gemm_w4_plan")
    part = torch.empty((s.value, M, N), device=x2.device, dtype=torch.float32)
    check(lib.psg_split_gemm_w4(ctx, _p(x2), _p(inv_scale, torch.float32), _p(w4, name="w4"), _p(e_img, name="e_img"),
                                _p(col_scale), _p(part), M, N, K, s.value, int(mode), st), "psg_split_gemm_w4")
    return Partials(part)


def skinny_gemm_w4(x, w4, e_img, col_scale, mode=0) -> Partials:
    """`skinny_gemm_w8` of <= 32 bf16 / fp16 rows over an MXFP4-quantised weight (see `split_gemm_w4`): fp32 slices
    [S, M, N] of (x . w) * col_scale (psg_skinny_gemm_w4).  K % 256 == 0."""
    import ctypes
    lib, ctx, st = _env(x)
    M, K = x.shape
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise PsgHipError(f"skinny_gemm_w4: x must be bf16 or fp16, got {x.dtype}")
    N = _w4_args("skinny_gemm_w4", w4, e_img, col_scale, K)
    s = ctypes.c_int(0)
    check(lib.psg_skinny_gemm_w4_plan(ctx, M, N, K, _dt(x), int(mode), ctypes.byref(s)), "psg_skinny_gemm_w4_plan")
    part = torch.empty((s.value, M, N), device=x.device, dtype=torch.float32)
    check(lib.psg_skinny_gemm_w4(ctx, _p(x, name="x"), _p(w4, name="w4"), _p(e_img, name="e_img"), _p(col_scale), _p(part), M,
                                 N, K, s.value, _dt(x), int(mode), st), "psg_skinny_gemm_w4")
    return Partials(part)


INT4_NIBBLE_OF_K = (0, 4, 1, 5, 2, 6, 3, 7)     # psg_gemm_int4.hip: the nibble of a dword of q_img that holds k = 8 d + e


def int4_q_image(q) -> torch.Tensor:
    """The codes q uint8 [N, K / 2] of a group-wise INT4 matrix (weights.quantize_int4_groups: two codes per byte, the low
    nibble the even k), K % 8 == 0, re-laid-out for psg_gemm_int4.hip's unpack: uint8 [N, K / 2] in which the code of
    k = 8 d + e sits in nibble INT4_NIBBLE_OF_K[e] of little-endian dword d of the row (nibble i = bits 4 i .. 4 i + 3)."""
    if q.dtype != torch.uint8 or q.dim() != 2 or q.shape[1] % 4:
        raise PsgHipError(f"int4_q_image: q must be uint8 [N, K / 2] with K % 8 == 0, got {q.dtype} {tuple(q.shape)}")
    N, Kh = q.shape
    codes = torch.stack((q & 15, q >> 4), dim=2).reshape(N, Kh // 4, 8)           # [n, d, e] = the code of k = 8 d + e
    inv = sorted(range(8), key=lambda e: INT4_NIBBLE_OF_K[e])                      # nibble i holds e = inv[i]
    nib = codes[:, :, inv].reshape(N, Kh, 2)
    return (nib[:, :, 0] | (nib[:, :, 1] << 4)).contiguous()


def int4_group_image(gs, gz) -> torch.Tensor:
    """The group scales gs fp16 [N, K / 128] and zero points gz uint8 [N, K / 128] (0..15) of a group-wise INT4 matrix with
    groups of 128, K % 256 == 0, re-laid-out for psg_gemm_int4.hip's K step of 256: uint8 [K / 256, N, 8], a row's 8 bytes =
    the fp16 scales of groups 2 t and 2 t + 1 (little-endian), their zero points, two zero bytes.  The groups of 32
    consecutive rows of one step are then 256 contiguous bytes (one LDS-DMA per wave) and a lane's one 8-byte read."""
    if (gs.dtype != torch.float16 or gz.dtype != torch.uint8 or gs.dim() != 2 or gs.shape != gz.shape or gs.shape[1] % 2):
        raise PsgHipError("int4_group_image: gs fp16 / gz uint8 [N, K / 128] with K % 256 == 0, got "
                          f"{gs.dtype} {tuple(gs.shape)} / {gz.dtype} {tuple(gz.shape)}")
    N, B = gs.shape
    img = torch.zeros((B // 2, N, 8), dtype=torch.uint8, device=gs.device)
    img[:, :, 0:4] = gs.contiguous().view(torch.uint8).reshape(N, B // 2, 4).permute(1, 0, 2)
    img[:, :, 4:6] = gz.reshape(N, B // 2, 2).permute(1, 0, 2)
    return img


def _int4_args(name, q_img, g_img, K, group):
    if q_img.dtype != torch.uint8 or q_img.dim() != 2 or q_img.shape[1] * 2 != K:
        raise PsgHipError(f"{name}: q_img must be int4_q_image(q): uint8 [N, {K // 2}], got {q_img.dtype} {tuple(q_img.shape)}")
    N = q_img.shape[0]
    if K % 256 == 0 and group == 128 and (g_img.dtype != torch.uint8 or tuple(g_img.shape) != (K // 256, N, 8)):
        raise PsgHipError(f"{name}: g_img must be int4_group_image(gs, gz): uint8 [{K // 256}, {N}, 8], got {g_img.dtype} "
                          f"{tuple(g_img.shape)}")
    return N


def split_gemm_int4(x2, inv_scale, q_img, g_img, mode=0, group=128) -> Partials:
    """`split_gemm_w4` over a group-wise INT4 weight W' = float(gs) * (q - gz) per group of 128 (weights.quantize_int4_groups /
    a GPTQ or AWQ checkpoint; `q_img` = int4_q_image(q), `g_img` = int4_group_image(gs, gz)): 4.25 bits per weight from HBM,
    the codes widened to the exact integers q - z in fp16, each group's partial sum scaled in fp32; fp32 slices [S, M, N] of
    sum_g gs_g (xh . (q - z) + xl . (q - z))_g * inv_scale (psg_split_gemm_int4).  K % 256 == 0, group == 128.  mode 1 / 2:
    slab-aligned / stream-K ranges, 0 = the library's estimate."""
    import ctypes
    lib, ctx, st = _env(x2)
    _, M, K = x2.shape
    assert x2.shape[0] == 2 and x2.dtype == torch.float16
    N = _int4_args("split_gemm_int4", q_img, g_img, K, group)
    s = ctypes.c_int(0)
    check(lib.psg_split_gemm_int4_plan(ctx, M, N, K, int(group), int(mode), ctypes.byref(s)), "psg_split_gemm_int4_plan")
    part = torch.empty((s.value, M, N), device=x2.device, dtype=torch.float32)
    check(lib.psg_split_gemm_int4(ctx, _p(x2), _p(inv_scale, torch.float32), _p(q_img, name="q_img"), _p(g_img, name="g_img"),
                                  _p(part), M, N, K, int(group), s.value, int(mode), st), "psg_split_gemm_int4")
    return Partials(part)


def skinny_gemm_int4(x, q_img, g_img, mode=0, group=128) -> Partials:
    """`skinny_gemm_w4` of <= 32 bf16 / fp16 rows over a group-wise INT4 weight (see `split_gemm_int4`): fp32 slices
    [S, M, N] of sum_g gs_g (x . (q - z))_g (psg_skinny_gemm_int4).  K % 256 == 0, group == 128."""
    import ctypes
    lib, ctx, st = _env(x)
    M, K = x.shape
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise PsgHipError(f"skinny_gemm_int4: x must be bf16 or fp16, got {x.dtype}")
    N = _int4_args("skinny_gemm_int4", q_img, g_img, K, group)
    s = ctypes.c_int(0)
    check(lib.psg_skinny_gemm_int4_plan(ctx, M, N, K, int(group), _dt(x), int(mode), ctypes.byref(s)), "psg_skinny_gemm_int4_plan")
    part = torch.empty((s.value, M, N), device=x.device, dtype=torch.float32)
    check(lib.psg_skinny_gemm_int4(ctx, _p(x, name="x"), _p(q_img, name="q_img"), _p(g_img, name="g_img"), _p(part), M, N, K,
                                   int(group), s.value, _dt(x), int(mode), st), "psg_skinny_gemm_int4")
    return Partials(part)


def batch_gemm(x, w, slab_rows=0, mode=0) -> Partials:
    """Decode-step projection for 33..160 rows (several images' pairs decoded together): fp32 split-K slices of x @ w.T
    like `skinny_gemm`'s, the weight streamed from HBM once (psg_batch_gemm; bf16 / fp16).
    slab_rows 256 / 128, mode 1 (slab-aligned ranges) / 2 (stream-K): a variant; 0 = the library's estimate."""
    import ctypes
    lib, ctx, st = _env(x)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    if x.dtype not in (torch.bfloat16, torch.float16) or w.dtype != x.dtype:
        raise PsgHipError(f"batch_gemm: x / w must both be bf16 or fp16, got {x.dtype} / {w.dtype}")
    s = ctypes.c_int(0)
    check(lib.psg_batch_gemm_plan(ctx, M, N, K, _dt(x), int(slab_rows), int(mode), ctypes.byref(s)), "psg_batch_gemm_plan")
    part = torch.empty((s.value, M, N), device=x.device, dtype=torch.float32)
    check(lib.psg_batch_gemm(ctx, _p(x, name="x"), _p(w, name="w"), _p(part), M, N, K, s.value, _dt(x), int(slab_rows),
                             int(mode), st), "psg_batch_gemm")
    return Partials(part)


def _batch_q(entry, x, planes, args, M, N, K, mode):
    """Plan + launch of one psg_batch_*_w8 / _w4 or psg_batch_split_gemm_w16 / _w32 entry: `args` =
    what stands between ctx and `part`."""
    import ctypes
    lib, ctx, st = _env(x)
    s = ctypes.c_int(0)
    dt = () if planes else (_dt(x),)
    check(getattr(lib, f"psg_{entry}_plan")(ctx, M, N, K, *dt, int(mode), ctypes.byref(s)), f"psg_{entry}_plan")
    part = torch.empty((s.value, M, N), device=x.device, dtype=torch.float32)
    check(getattr(lib, f"psg_{entry}")(ctx, *args, _p(part), M, N, K, s.value, *dt, int(mode), st), f"psg_{entry}")
    return Partials(part)


def batch_gemm_w8(x, w8, col_scale, mode=0) -> Partials:
    """`batch_gemm` for 33..160 bf16 / fp16 rows over an FP8-quantised weight W' = e4m3(w8) * col_scale[:, None]: one byte
    per weight from HBM, `skinny_gemm_w8`'s arithmetic; fp32 slices [S, M, N] of (x . q) * col_scale (psg_batch_gemm_w8).
    K % 128 == 0.  A row's slices do not depend on M or on the other rows."""
    M, K = x.shape
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise PsgHipError(f"batch_gemm_w8: x must be bf16 or fp16, got {x.dtype}")
    N = _w8_args("batch_gemm_w8", w8, col_scale, K)
    return _batch_q("batch_gemm_w8", x, False, (_p(x, name="x"), _p(w8, name="w8"), _p(col_scale)), M, N, K, mode)


def _x2_args(name, x2, inv_scale):
    if x2.dim() != 3 or x2.shape[0] != 2 or x2.dtype != torch.float16 or not x2.is_contiguous():
        raise PsgHipError(f"{name}: x2 must be the fp16 planes [2, M, K] of split_f16x2, got {x2.dtype} {tuple(x2.shape)}")
    if inv_scale.dtype != torch.float32 or tuple(inv_scale.shape) != (x2.shape[1],):
        raise PsgHipError(f"{name}: inv_scale must be fp32 [{x2.shape[1]}], got {inv_scale.dtype} {tuple(inv_scale.shape)}")
    return x2.shape[1], x2.shape[2]


def batch_split_gemm_w8(x2, inv_scale, w8, col_scale, mode=0) -> Partials:
    """`split_gemm_w8` for 33..160 fp32 rows given as the planes of `split_f16x2`: fp32 slices [S, M, N] of
    (xh . q + xl . q) * inv_scale * col_scale (psg_batch_split_gemm_w8).  K % 128 == 0."""
    M, K = _x2_args("batch_split_gemm_w8", x2, inv_scale)
    N = _w8_args("batch_split_gemm_w8", w8, col_scale, K)
    return _batch_q("batch_split_gemm_w8", x2, True, (_p(x2), _p(inv_scale), _p(w8, name="w8"), _p(col_scale)), M, N, K, mode)


def batch_gemm_w4(x, w4, e_img, col_scale, mode=0) -> Partials:
    """`batch_gemm_w8` over an MXFP4-quantised weight (see `split_gemm_w4`; `e_img` = mxfp4_exp_image(e)): fp32 slices
    [S, M, N] of (x . w) * col_scale (psg_batch_gemm_w4).  K % 256 == 0."""
    M, K = x.shape
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise PsgHipError(f"batch_gemm_w4: x must be bf16 or fp16, got {x.dtype}")
    N = _w4_args("batch_gemm_w4", w4, e_img, col_scale, K)
    return _batch_q("batch_gemm_w4", x, False, (_p(x, name="x"), _p(w4, name="w4"), _p(e_img, name="e_img"), _p(col_scale)),
                    M, N, K, mode)


def batch_split_gemm_w4(x2, inv_scale, w4, e_img, col_scale, mode=0) -> Partials:
    """`batch_split_gemm_w8` over an MXFP4-quantised weight: fp32 slices [S, M, N] of (xh . w + xl . w) * inv_scale *
    col_scale (psg_batch_split_gemm_w4).  K % 256 == 0."""
    M, K = _x2_args("batch_split_gemm_w4", x2, inv_scale)
    N = _w4_args("batch_split_gemm_w4", w4, e_img, col_scale, K)
    return _batch_q("batch_split_gemm_w4", x2, True,
                    (_p(x2), _p(inv_scale), _p(w4, name="w4"), _p(e_img, name="e_img"), _p(col_scale)), M, N, K, mode)


def _rows16_args(name, what, w, K, col_scale, min_cols):
    """A 2-D fp16 weight in HBM whose rows are contiguous runs of >= min_cols elements (any row stride: a view is read in
    place) and its fp32 column scale [N].  Alignment is the library's check (PSG_ERR_UNSUPPORTED)."""
    if w.dtype != torch.float16 or w.dim() != 2 or w.shape[1] < min_cols or (w.shape[1] > 1 and w.stride(1) != 1):
        raise PsgHipError(f"{name}: {what} must be fp16 [N, >= {min_cols}] with contiguous rows (K = {K}), got {w.dtype} "
                          f"{tuple(w.shape)} strides {tuple(w.stride())}")
    N = w.shape[0]
    if col_scale.dtype != torch.float32 or tuple(col_scale.shape) != (N,):
        raise PsgHipError(f"{name}: col_scale must be fp32 [{N}], got {col_scale.dtype} {tuple(col_scale.shape)}")
    if not w.is_cuda:
        raise PsgHipError(f"{name}: {what} must live in HBM (got a {w.device} tensor); this path has no CPU fallback")
    return N


def batch_split_gemm_w16(x2, inv_scale, w16, col_scale=None, mode=0) -> Partials:
    """`split_gemm_w16` for 33..160 fp32 rows given as the planes of `split_f16x2`, over a weight that is an fp16 value:
    fp32 slices [S, M, N] of (xh . w + xl . w) * inv_scale * col_scale (psg_batch_split_gemm_w16).  w16 fp16
    [N, K], rows of any 16-byte-aligned stride (a column view is read in place); col_scale None = ones.  N % 16 == 0,
    K % 64 == 0.  A row's slices do not depend on M or on the other rows."""
    M, K = _x2_args("batch_split_gemm_w16", x2, inv_scale)
    if w16.dim() == 2 and w16.shape[1] != K:
        raise PsgHipError(f"batch_split_gemm_w16: w16 must be fp16 [N, {K}], got {tuple(w16.shape)}")
    if col_scale is None:
        col_scale = torch.ones(w16.shape[0], device=x2.device, dtype=torch.float32)
    N = _rows16_args("batch_split_gemm_w16", "w16", w16, K, col_scale, K)
    return _batch_q("batch_split_gemm_w16", x2, True,
                    (_p(x2), _p(inv_scale), w16.data_ptr(), int(w16.stride(0)) if N > 1 else K, _p(col_scale)), M, N, K, mode)


def batch_split_gemm_w32(x2, inv_scale, w_img, col_scale, K, lo_off=None, mode=0) -> Partials:
    """The fp32s product of 33..160 fp32 rows (planes of `split_f16x2`) with a generic fp32 weight held as two fp16 planes
    inside ONE image, read in place: fp32 slices [S, M, N] of (xh . wh + xh . wl + xl . wh) * inv_scale * col_scale
    (psg_batch_split_gemm_w32).  w_img fp16 [N, row]: wh at columns 0..K, wl at lo_off..lo_off + K (default K) -
    `split_f16x3(w, weights=True)`'s [wh | wl | wh] image as it stands, or a packed [wh | wl] image; col_scale = that split's
    inverse row scales.  N % 16 == 0, K % 64 == 0."""
    M, Kx = _x2_args("batch_split_gemm_w32", x2, inv_scale)
    K = int(K)
    lo_off = K if lo_off is None else int(lo_off)
    if Kx != K:
        raise PsgHipError(f"batch_split_gemm_w32: x2 has K = {Kx}, the weight image K = {K}")
    if lo_off < K or (w_img.dim() == 2 and lo_off + K > w_img.shape[1]):
        raise PsgHipError(f"batch_split_gemm_w32: the low plane [{lo_off}, {lo_off + K}) must lie behind the high plane "
                          f"[0, {K}) inside a row of {tuple(w_img.shape)}")
    N = _rows16_args("batch_split_gemm_w32", "w_img", w_img, K, col_scale, 2 * K)
    return _batch_q("batch_split_gemm_w32", x2, True,
                    (_p(x2), _p(inv_scale), w_img.data_ptr(), int(w_img.stride(0)) if N > 1 else w_img.shape[1], lo_off,
                     _p(col_scale)), M, N, K, mode)


def _x3_args(name, x3, wb16):
    if not (isinstance(x3, torch.Tensor) and x3.dim() == 3 and x3.shape[0] == 3 and x3.dtype == torch.bfloat16
            and x3.is_contiguous()):
        raise PsgHipError(f"{name}: x3 must be the contiguous bf16 planes [3, M, K] of split_b16x3, got "
                          f"{getattr(x3, 'dtype', type(x3))} {tuple(getattr(x3, 'shape', ()))}")
    K = x3.shape[2]
    if not (isinstance(wb16, torch.Tensor) and wb16.dim() == 2 and wb16.dtype == torch.bfloat16 and wb16.shape[1] == K
            and wb16.is_contiguous() and wb16.device == x3.device):
        raise PsgHipError(f"{name}: w must be contiguous bf16 [N, {K}] on {x3.device}, got "
                          f"{getattr(wb16, 'dtype', type(wb16))} {tuple(getattr(wb16, 'shape', ()))}")
    if not wb16.is_cuda:
        raise PsgHipError(f"{name}: w must live in HBM (got a {wb16.device} tensor); this path has no CPU fallback")
    return x3.shape[1], wb16.shape[0], K


def batch_split_gemm_wb16_plan(M, N, K, device, mode=0) -> int:
    """Slices `batch_split_gemm_wb16` writes for x3 [3, M, K] against w [N, K]: a function of (N, K, mode) only; raises
    where the kernel does not take the shape."""
    import ctypes
    lib = _lib.load()
    dev = torch.device(device)
    s = ctypes.c_int(0)
    check(lib.psg_batch_split_gemm_wb16_plan(_lib.ctx(dev.index or 0), int(M), int(N), int(K), int(mode), ctypes.byref(s)),
          "psg_batch_split_gemm_wb16_plan")
    return s.value


def batch_split_gemm_wb16(x3, w, mode=0) -> Partials:
    """`split_gemm_wb16` for 33..160 fp32 rows given as the planes of `split_b16x3`, over a weight that is a bf16 value: fp32
    slices [S, M, N] of x2 . w + x1 . w + x0 . w, every product exact, one fp32 accumulator per output element
    (psg_batch_split_gemm_wb16).  No scales.  N % 16 == 0, K % 64 == 0, 16-byte aligned operands.  A row's slices
    do not depend on M or on the other rows.  mode 1 / 2: slab-aligned / stream-K ranges, 0 = the library's estimate."""
    M, N, K = _x3_args("batch_split_gemm_wb16", x3, w)
    return _batch_q("batch_split_gemm_wb16", x3, True, (_p(x3), _p(w, name="w")), M, N, K, mode)


def skinny_gemm_fused(kind, x_out, w, sync, *, inp=None, resid=None, norm_w=None, eps=0.0, attn=None, splits=None):
    """Decode projection with its producer row operation in the same launch (psg_skinny_gemm_fused):
    the prologue `kind` computes x_out [M, K] from `inp` (Partials / activation tensor / None), then
    part = x_out @ w.T as in `skinny_gemm`.  sync: two zeroed int32 device words owned by this launch.
    attn = (tok_pair, tok_pos, rope, heads, ctx_len, k_cache, v_cache) for the decode-attention prologue."""
    import ctypes
    from ._lib import Prologue
    lib, ctx, st = _env(x_out)
    M, K = x_out.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.dtype == x_out.dtype and sync.dtype == torch.int32 and sync.numel() >= 2
    if splits is None:
        s = ctypes.c_int(0)
        check(lib.psg_skinny_gemm_plan(ctx, M, N, K, _dt(x_out), ctypes.byref(s)), "psg_skinny_gemm_plan")
        splits = s.value
    pro = Prologue()
    pro.kind = int(kind)
    if inp is not None:
        pro.input, pro.in_splits = _in(inp, x_out.dtype)
    if resid is not None:
        pro.resid = _p(resid, x_out.dtype)
        pro.norm_w = _p(norm_w, torch.float32)
        pro.eps = float(eps)
    if attn is not None:
        tok_pair, tok_pos, rope, heads, ctx_len, kc, vc = attn
        pro.tok_pair, pro.tok_pos = _p(tok_pair, torch.int32), _p(tok_pos, torch.int32)
        pro.rope_cos, pro.rope_sin = _p(rope[0], torch.float32), _p(rope[1], torch.float32)
        pro.heads, pro.ctx = int(heads), int(ctx_len)
        pro.k_cache, pro.v_cache = _p(kc, x_out.dtype), _p(vc, x_out.dtype)
    pro.sync = sync.data_ptr()
    part = torch.empty((splits, M, N), device=x_out.device, dtype=torch.float32)
    check(lib.psg_skinny_gemm_fused(ctx, ctypes.byref(pro), _p(x_out), _p(w), _p(part), M, N, K, splits, _dt(x_out), st),
          "psg_skinny_gemm_fused")
    return Partials(part)


def masked_mean_pool(feat, pan, img_hw, pad_hw, object_ids):
    """Masked-mean object embeddings of the v1-v3 detectors (openseed_relation.py:453-468).
    feat [1,C,Hf,Wf] fp32, pan [H0,W0] int32 id map, object_ids int32 [N] -> [N, C] fp32."""
    import ctypes
    lib, ctx, st = _env(feat)
    _, Cc, Hf, Wf = feat.shape
    N = object_ids.numel()
    nbytes = ctypes.c_int64(0)
    check(lib.psg_masked_mean_pool_workspace(ctx, Cc, Hf, Wf, N, ctypes.byref(nbytes)),
          "psg_masked_mean_pool_workspace")
    ws = torch.empty(nbytes.value // 4, device=feat.device, dtype=torch.int32)
    out = torch.empty((N, Cc), device=feat.device, dtype=torch.float32)
    check(lib.psg_masked_mean_pool(ctx, _p(feat, torch.float32), Cc, Hf, Wf, _p(pan, torch.int32, "pan_results"),
                                   pan.shape[0], pan.shape[1], int(img_hw[0]), int(img_hw[1]), int(pad_hw[0]),
                                   int(pad_hw[1]), _p(object_ids, torch.int32), N, _p(out), _p(ws), nbytes.value, st),
          "psg_masked_mean_pool")
    return out


def masked_split_mean_pool(feat, pan, img_hw, pad_hw, object_ids, output_size):
    """`_mask_pooling(output_size > 1)` of the v1 detector (openseed_relation.py:175-200): per object, its masked pixels in
    row-major order cut into `output_size` chunks, one mean per chunk -> [N, output_size, C] fp32."""
    import ctypes
    lib, ctx, st = _env(feat)
    _, Cc, Hf, Wf = feat.shape
    N = object_ids.numel()
    nbytes = ctypes.c_int64(0)
    check(lib.psg_masked_mean_pool_workspace(ctx, Cc, Hf, Wf, N, ctypes.byref(nbytes)), "psg_masked_mean_pool_workspace")
    ws = torch.empty(nbytes.value // 4, device=feat.device, dtype=torch.int32)
    out = torch.empty((N, int(output_size), Cc), device=feat.device, dtype=torch.float32)
    check(lib.psg_masked_split_mean_pool(ctx, _p(feat, torch.float32), Cc, Hf, Wf, _p(pan, torch.int32, "pan_results"),
                                         pan.shape[0], pan.shape[1], int(img_hw[0]), int(img_hw[1]), int(pad_hw[0]),
                                         int(pad_hw[1]), _p(object_ids, torch.int32), N, int(output_size), _p(out), _p(ws),
                                         nbytes.value, st), "psg_masked_split_mean_pool")
    return out


def bilinear_scores(sub, obj, num_relations):
    """einsum('nrsc,nroc->nrso') of the closed-set heads (relation_transformer_head_v2.py:204-209).
    sub / obj [B, N, R*C] fp32 (the Linear outputs before the reference's reshape + permute) -> [B, R, N, N] fp32."""
    lib, ctx, st = _env(sub)
    B, N, RC = sub.shape
    assert obj.shape == sub.shape and RC % num_relations == 0
    pred = torch.empty((B, num_relations, N, N), device=sub.device, dtype=torch.float32)
    check(lib.psg_bilinear_scores(ctx, _p(sub, torch.float32, "sub"), _p(obj, torch.float32, "obj"), B, N,
                                  num_relations, RC // num_relations, _p(pred), st), "psg_bilinear_scores")
    return pred


def train_object_bitmasks(thing_masks, sem, is_thing, category, thing_index, grid_hw):
    """V4:371-399.  thing_masks uint8 [n_thing,H,W], sem int32 [H,W], per-object int32 vectors -> int64 bits [N, words]."""
    lib, ctx, st = _env(sem)
    H, W = sem.shape
    N = is_thing.numel()
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    words = (gh * gw + 63) // 64
    bits = torch.empty((N, words), device=sem.device, dtype=torch.int64)
    n_thing = 0 if thing_masks is None else thing_masks.shape[0]
    if n_thing and tuple(thing_masks.shape[1:]) != (H, W):
        raise PsgHipError(f"train_object_bitmasks: thing masks are {tuple(thing_masks.shape[1:])}, the semantic map is "
                          f"{(H, W)}; both must be at the padded image resolution (V4:371-399)")
    check(lib.psg_train_object_bitmasks(ctx, _p(thing_masks, torch.uint8, "thing_masks") if n_thing else None, n_thing,
                                        _p(sem, torch.int32, "sem"), H, W, _p(is_thing, torch.int32),
                                        _p(category, torch.int32), _p(thing_index, torch.int32), N, gh, gw, _p(bits),
                                        words, st), "psg_train_object_bitmasks")
    return bits


def bce_with_logits(logit, label, weight=1.0):
    lib, ctx, st = _env(logit)
    out = torch.empty(1, device=logit.device, dtype=torch.float32)
    check(lib.psg_bce_with_logits(ctx, _p(logit, torch.float32, "logit"), _p(label, torch.float32, "label"),
                                  logit.numel(), float(weight), _p(out), st), "psg_bce_with_logits")
    return out[0]


def cross_entropy_rows(logits, labels):
    """per-row -log softmax(logits)[label] in fp32; label < 0 -> 0 (ignored)."""
    lib, ctx, st = _env(logits)
    rows, vocab = logits.shape
    loss = torch.empty(rows, device=logits.device, dtype=torch.float32)
    check(lib.psg_cross_entropy_rows(ctx, _p(logits), rows, vocab, _p(labels, torch.int32, "labels"), _p(loss),
                                     _dt(logits), st), "psg_cross_entropy_rows")
    return loss


TILES = {"auto": 0, "256x256": 1, "256x192": 2, "256x128": 3, "256x64": 4, "128x128": 5}      # enum psg_tile


def dense_gemm(x, w, bias=None, gelu=False, out=None, out_dtype=None, row_scale=None, col_scale=None, tile="256x256",
               swiglu=False):
    """out = [gelu](x @ w.T [* row_scale[:, None] * col_scale[None, :]] + bias) in one pass (bf16 / fp16 operands;
    N % 16 == 0, K % 64 == 0).  out_dtype=torch.float32: fp32 result (needed for the scales: the split-fp16 products of
    the fp32s mode).  Row-count invariant: a row's result does not depend on how many other rows the call has, nor on
    the tile ("auto": the geometry that fills the CUs in the fewest rounds for [M, N]).
    swiglu=True: w is a gate / up weight interleaved by `interleave_gate_up`; out [M, N / 2] = silu(gate) * up."""
    lib, ctx, st = _env(x)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.dtype == x.dtype
    odt = x.dtype if out_dtype is None else out_dtype
    out = torch.empty((M, N // 2 if swiglu else N), device=x.device, dtype=odt) if out is None else out
    assert out.shape == (M, N // 2 if swiglu else N)
    assert not (swiglu and gelu)
    check(lib.psg_dense_gemm_tiled(ctx, _p(x, name="x"), _p(w, name="w"), _p(bias, torch.float32, "bias"),
                                   2 if swiglu else 1 if gelu else 0, _p(out, odt), M, N, K, _dt(x), _DT[odt],
                                   _p(row_scale, torch.float32, "row_scale"), _p(col_scale, torch.float32, "col_scale"),
                                   TILES[tile], st), "psg_dense_gemm")
    return out


def dense_gemm_split(x2, w2, bias, row_scale, col_scale, gelu=False, out=None, tile="auto"):
    """fp32 out = [gelu]((xh.wh + xh.wl + xl.wh) * row_scale[:, None] * col_scale[None, :] + bias) for two fp32 matrices
    given as `split_f16i2` images ([rows, 2K] fp16: per 32 k the high parts, then the low parts): the fp32-grade product
    of the fp32s mode with every operand value staged once (psg_dense_gemm_split).  Row-count and tile invariant."""
    lib, ctx, st = _env(x2)
    M, K2 = x2.shape
    N = w2.shape[0]
    assert w2.shape[1] == K2 and x2.dtype == torch.float16 and w2.dtype == torch.float16
    out = torch.empty((M, N), device=x2.device, dtype=torch.float32) if out is None else out
    assert out.shape == (M, N) and out.dtype == torch.float32
    check(lib.psg_dense_gemm_split(ctx, _p(x2, name="x2"), _p(w2, name="w2"), _p(bias, torch.float32, "bias"),
                                   1 if gelu else 0, _p(out, torch.float32), M, N, K2, _p(row_scale, torch.float32, "row_scale"),
                                   _p(col_scale, torch.float32, "col_scale"), TILES[tile], st), "psg_dense_gemm_split")
    return out


def interleave_gate_up(w_gate_up):
    """[2 inter, K] (gate rows, then up rows) -> the row order the SwiGLU epilogue of `dense_gemm` reads: groups of 16
    rows = 8 gate rows, then the 8 up rows of the same columns."""
    lib, ctx, st = _env(w_gate_up)
    n2, K = w_gate_up.shape
    out = torch.empty_like(w_gate_up)
    check(lib.psg_interleave_gate_up(ctx, _p(w_gate_up, name="gate_up"), _p(out), n2 // 2, K, st), "psg_interleave_gate_up")
    return out


def split_f16x3(x, weights=False):
    """fp32 rows -> three fp16 K segments for an fp32-grade product on the 16-bit matrix cores (psg_split_f16x3):
    activations [hi | hi | lo], weights [hi | lo | hi].  Returns (fp16 [rows, 3K], inv_scale fp32 [rows])."""
    lib, ctx, st = _env(x)
    assert x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1
    rows, K = x.shape
    out = torch.empty((rows, 3 * K), device=x.device, dtype=torch.float16)
    inv = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(lib.psg_split_f16x3(ctx, x.data_ptr(), rows, K, x.stride(0), 1 if weights else 0, _p(out), _p(inv), st),
          "psg_split_f16x3")
    return out, inv


def split_f16i2(x):
    """fp32 rows -> (fp16 [rows, 2K]: per 32 k [hi(32) | lo(32)], inv_scale fp32 [rows]) - an operand of
    `dense_gemm_split` (activations and weights alike; psg_split_f16x3 order 2).  K % 32 == 0."""
    lib, ctx, st = _env(x)
    assert x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] % 32 == 0
    rows, K = x.shape
    out = torch.empty((rows, 2 * K), device=x.device, dtype=torch.float16)
    inv = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(lib.psg_split_f16x3(ctx, x.data_ptr(), rows, K, x.stride(0), 2, _p(out), _p(inv), st), "psg_split_f16x3")
    return out, inv


def scale_rows_cols(y, row_scale, col_scale):
    """y[m][n] *= row_scale[m] * col_scale[n] in place (fp32)."""
    lib, ctx, st = _env(y)
    rows, N = y.shape
    assert row_scale.numel() == rows and col_scale.numel() == N
    check(lib.psg_scale_rows_cols(ctx, _p(y, torch.float32, "y"), rows, N, _p(row_scale, torch.float32),
                                  _p(col_scale, torch.float32), st), "psg_scale_rows_cols")
    return y


class Scaled:
    """A raw split-fp16 GEMM result y [rows, N] fp32 with the power-of-two scales that turn it into the product:
    value = y * (row_scale[m] * col_scale[n]).  Consumed by rmsnorm_split / rope_kvwrite_scaled / silu_mul_split."""
    __slots__ = ("y", "row_scale", "col_scale")

    def __init__(self, y, row_scale, col_scale):
        # y [rows, N], or [slices, rows, N]: the K segments of the product as separate slices (rmsnorm_split sums them)
        assert y.dtype == torch.float32 and y.dim() in (2, 3) and y.is_contiguous()
        assert row_scale.numel() == y.shape[-2] and col_scale.numel() == y.shape[-1]
        self.y, self.row_scale, self.col_scale = y, row_scale, col_scale

    def dense(self):
        y = self.y if self.y.dim() == 2 else self.y.sum(0)
        return scale_rows_cols(y, self.row_scale, self.col_scale)


def rmsnorm_split(resid, delta, w, eps, planes=3):
    """resid += delta (a `Scaled` or None); RMSNorm(resid) * w as split-fp16 segments: (fp16 [rows, 3 hidden], inv_scale);
    planes=2: as two planes (fp16 [2, rows, hidden]: high, low) for a weight that is an fp16 value."""
    lib, ctx, st = _env(resid)
    rows, hidden = resid.shape
    out = torch.empty((rows, 3 * hidden) if planes == 3 else (2, rows, hidden), device=resid.device, dtype=torch.float16)
    inv = torch.empty(rows, device=resid.device, dtype=torch.float32)
    dp, rp, cp = (None, None, None) if delta is None else (_p(delta.y), _p(delta.row_scale, torch.float32),
                                                           _p(delta.col_scale, torch.float32))
    nsl = 1 if delta is None or delta.y.dim() == 2 else delta.y.shape[0]
    assert delta is None or delta.y.shape[-2:] == (rows, hidden)
    check(lib.psg_rmsnorm_split(ctx, _p(resid, torch.float32, "resid"), dp, rp, cp, nsl, _p(w, torch.float32), float(eps),
                                rows, hidden, _p(out), _p(inv), int(planes), st), "psg_rmsnorm_split")
    return out, inv


def rope_kvwrite_scaled(qkv, tok_pair, tok_pos, rope, heads, head_dim, ctx_len, q_out, k_cache, v_cache, kv_heads=None):
    lib, ctx, st = _env(q_out)
    rows = q_out.shape[0]
    kv = heads if kv_heads is None else int(kv_heads)
    assert isinstance(qkv, Scaled) and qkv.y.shape[-2:] == (rows, (heads + 2 * kv) * head_dim)
    nsl = 1 if qkv.y.dim() == 2 else qkv.y.shape[0]
    if _gqa(heads, kv_heads):
        check(lib.psg_rope_kvwrite_scaled_gqa(ctx, _p(qkv.y), _p(qkv.row_scale, torch.float32),
                                              _p(qkv.col_scale, torch.float32), _p(tok_pair, torch.int32),
                                              _p(tok_pos, torch.int32), _p(rope[0], torch.float32),
                                              _p(rope[1], torch.float32), nsl, rows, heads, kv, head_dim, ctx_len,
                                              _p(q_out, torch.float32), _p(k_cache, torch.float32),
                                              _p(v_cache, torch.float32), st), "psg_rope_kvwrite_scaled_gqa")
        return
    check(lib.psg_rope_kvwrite_scaled(ctx, _p(qkv.y), _p(qkv.row_scale, torch.float32), _p(qkv.col_scale, torch.float32),
                                      _p(tok_pair, torch.int32), _p(tok_pos, torch.int32), _p(rope[0], torch.float32),
                                      _p(rope[1], torch.float32), nsl, rows, heads, head_dim, ctx_len, _p(q_out, torch.float32),
                                      _p(k_cache, torch.float32), _p(v_cache, torch.float32), st), "psg_rope_kvwrite_scaled")


def silu_mul_split(gate_up, inter, planes=3):
    """silu(gate) * up of a `Scaled` gate|up result as split-fp16 segments: (fp16 [rows, 3 inter], inv_scale);
    planes=2: as two planes (fp16 [2, rows, inter])."""
    lib, ctx, st = _env(gate_up.y)
    rows = gate_up.y.shape[-2]
    nsl = 1 if gate_up.y.dim() == 2 else gate_up.y.shape[0]
    assert gate_up.y.shape[-1] == 2 * inter
    out = torch.empty((rows, 3 * inter) if planes == 3 else (2, rows, inter), device=gate_up.y.device, dtype=torch.float16)
    inv = torch.empty(rows, device=gate_up.y.device, dtype=torch.float32)
    check(lib.psg_silu_mul_split(ctx, _p(gate_up.y), _p(gate_up.row_scale, torch.float32), _p(gate_up.col_scale, torch.float32),
                                 nsl, rows, inter, _p(out), _p(inv), int(planes), st), "psg_silu_mul_split")
    return out, inv


# ---- the library product with a pinned algorithm (psg_lt_gemm) -------------------------------------------------
_LT_VERSION: dict = {}                                             # device index -> library version (int) or the error text


def lt_gemm_version(device):
    """The version number of the GEMM library copy this process runs (psg_lt_gemm_init: resolves its entry points and
    creates the context's handle on first use), or None when it cannot be used - `lt_gemm_error` then says why."""
    import ctypes
    dev_i = torch.device(device).index or 0
    if dev_i not in _LT_VERSION:
        try:
            v = ctypes.c_int(0)
            check(_lib.load().psg_lt_gemm_init(_lib.ctx(dev_i), ctypes.byref(v)), "psg_lt_gemm_init")
            _LT_VERSION[dev_i] = int(v.value)
        except PsgHipError as e:
            _LT_VERSION[dev_i] = str(e)
    v = _LT_VERSION[dev_i]
    return v if isinstance(v, int) else None


def lt_gemm_error(device):
    v = _LT_VERSION.get(torch.device(device).index or 0)
    return v if isinstance(v, str) else None


def _lt_operand(t, inner, name):
    """(batch, batch stride, leading dimension) of a [rows, inner] or [batch, rows, inner] view with unit inner stride."""
    assert t.dim() in (2, 3) and t.shape[-1] == inner and (t.stride(-1) == 1 or inner == 1), f"{name}: {t.shape} {t.stride()}"
    return (1, 0, t.stride(0)) if t.dim() == 2 else (t.shape[0], t.stride(0), t.stride(1))


def _lt_problem(a, w, y):
    rows, K = a.shape[-2:]
    N = w.shape[-2]
    assert w.shape[-1] == K and a.dtype == w.dtype == torch.float16, (a.shape, w.shape, a.dtype, w.dtype)
    (ba, sa, lda), (bw, sw, ldw) = _lt_operand(a, K, "a"), _lt_operand(w, K, "w")
    assert ba == bw
    if y is None:
        by, sy, ldy = ba, rows * N, N
    else:
        assert y.dtype == torch.float32 and y.shape[-2] == rows
        by, sy, ldy = _lt_operand(y, N, "y")
        assert by == ba
    return (int(rows), int(N), int(K), int(lda), int(ldw), int(ldy), int(ba), int(sa), int(sw), int(sy))


def lt_gemm_candidates(a, w, y=None, max_ws_bytes=0):
    """[(solution index, workspace bytes), ...] the library's heuristic lists for y = a . w^T (the operands' shapes and
    strides only; the first entry is its first choice) within max_ws_bytes of workspace."""
    import ctypes
    lib, ctx, _ = _env(a)
    if lt_gemm_version(a.device) is None:
        raise PsgHipError(lt_gemm_error(a.device))
    idx, ws, n = (ctypes.c_int * 64)(), (ctypes.c_int64 * 64)(), ctypes.c_int(0)
    check(lib.psg_lt_gemm_candidates(ctx, *_lt_problem(a, w, y), int(max_ws_bytes), 64, idx, ws, ctypes.byref(n)),
          "psg_lt_gemm_candidates")
    return [(int(idx[i]), int(ws[i])) for i in range(n.value)]


def lt_gemm(a, w, y, algo=-1, workspace=None):
    """y (fp32 [rows, N] or [batch, rows, N], any leading dimension >= N) = a (fp16 [.., rows, K]) . w (fp16 [.., N, K])^T on
    the library's algorithm with solution index `algo` (-1: its first choice).  Views are taken as they are (unit inner
    stride), so a column part of a wider y or the K segments of one operand as a batch need no copy.  workspace: a uint8
    device buffer, or None.  Returns True when `algo` was not among the candidates and the first choice ran instead."""
    import ctypes
    lib, ctx, st = _env(a)
    if lt_gemm_version(a.device) is None:
        raise PsgHipError(lt_gemm_error(a.device))
    assert w.is_cuda and y.is_cuda
    fb = ctypes.c_int(0)
    wsp, wsb = (None, 0) if workspace is None else (workspace.data_ptr(), workspace.numel() * workspace.element_size())
    check(lib.psg_lt_gemm(ctx, a.data_ptr(), w.data_ptr(), y.data_ptr(), *_lt_problem(a, w, y), int(algo), wsp, wsb,
                          ctypes.byref(fb), st), "psg_lt_gemm")
    return bool(fb.value)
