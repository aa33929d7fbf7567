"""State-dict schema of the relation head and deterministic weight generators.

Key names are the reference head's own ``state_dict()`` names (prefix ``relation_head.`` inside a
detector checkpoint): timm ``PatchEmbed.proj``, HF ``InstructBlipQFormerModel``,
``relation_query`` / ``rel_cls_query`` (V4:87-90), ``binary_rel_cls_pred`` (V4:92),
``language_projection`` (V4:97-98) and HF ``LlamaForCausalLM`` under ``language_model.``.

Reference checkpoints are partial (part_checkpoint_hook.py:96-116 drops ``language_model.*``), so
loaders must be ``strict=False``; ``llm_keys`` / ``head_keys`` split the schema accordingly.

There are no model files offline, so tests and the benchmark use seeded random weights:
``make_weights_numpy`` (numpy PCG64, sorted-key order, bit-reproducible on any box; used for
parity tests and goldens) and ``make_weights_device`` (torch generator on the GPU; used for the
7B-shaped benchmark where numpy would take minutes).
"""
from __future__ import annotations

import numpy as np
import torch

from .config import REL_CLS_TYPES, PSGConfig


def head_shapes(cfg: PSGConfig) -> dict:
    q = cfg.qformer
    C, P = cfg.feat_channels, cfg.patch_size
    s = {
        "patch_embed.proj.weight": (C, C, P, P),
        "patch_embed.proj.bias": (C,),
        "relation_qformer.embeddings.word_embeddings.weight": (q.vocab, q.hidden),
        "relation_qformer.embeddings.position_embeddings.weight": (q.max_pos, q.hidden),
        "relation_qformer.embeddings.layernorm.weight": (q.hidden,),
        "relation_qformer.embeddings.layernorm.bias": (q.hidden,),
        "relation_query": (1, q.num_query, q.hidden),
        "rel_cls_query": (1, 1, q.hidden),
    }
    if cfg.rel_cls_type not in REL_CLS_TYPES:
        raise ValueError(f"rel_cls_type must be one of {REL_CLS_TYPES}, got {cfg.rel_cls_type!r}")
    if "binary" in cfg.rel_cls_type:                                    # V4:91-92
        s["binary_rel_cls_pred.weight"] = (1, q.hidden)
        s["binary_rel_cls_pred.bias"] = (1,)
    if "multiclass" in cfg.rel_cls_type:                                # V4:93-95
        s["multiclass_rel_cls_pred.weight"] = (cfg.num_relation_classes, q.hidden)
        s["multiclass_rel_cls_pred.bias"] = (cfg.num_relation_classes,)
    s["language_projection.weight"] = (cfg.llm.hidden, q.hidden)
    s["language_projection.bias"] = (cfg.llm.hidden,)
    for l in range(q.layers):
        p = f"relation_qformer.encoder.layer.{l}."
        for att, kin in (("attention", q.hidden), ("crossattention", q.enc_hidden)):
            s[p + f"{att}.attention.query.weight"] = (q.hidden, q.hidden)
            s[p + f"{att}.attention.query.bias"] = (q.hidden,)
            s[p + f"{att}.attention.key.weight"] = (q.hidden, kin)
            s[p + f"{att}.attention.key.bias"] = (q.hidden,)
            s[p + f"{att}.attention.value.weight"] = (q.hidden, kin)
            s[p + f"{att}.attention.value.bias"] = (q.hidden,)
            s[p + f"{att}.output.dense.weight"] = (q.hidden, q.hidden)
            s[p + f"{att}.output.dense.bias"] = (q.hidden,)
            s[p + f"{att}.output.LayerNorm.weight"] = (q.hidden,)
            s[p + f"{att}.output.LayerNorm.bias"] = (q.hidden,)
        for inter, out in (("intermediate", "output"), ("intermediate_query", "output_query")):
            s[p + f"{inter}.dense.weight"] = (q.inter, q.hidden)
            s[p + f"{inter}.dense.bias"] = (q.inter,)
            s[p + f"{out}.dense.weight"] = (q.hidden, q.inter)
            s[p + f"{out}.dense.bias"] = (q.hidden,)
            s[p + f"{out}.LayerNorm.weight"] = (q.hidden,)
            s[p + f"{out}.LayerNorm.bias"] = (q.hidden,)
    return s


def llm_shapes(cfg: PSGConfig) -> dict:
    m = cfg.llm
    s = {
        "language_model.model.embed_tokens.weight": (m.vocab, m.hidden),
        "language_model.model.norm.weight": (m.hidden,),
        "language_model.lm_head.weight": (m.vocab, m.hidden),
    }
    for l in range(m.layers):
        p = f"language_model.model.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):           # k / v: [kv_heads 128, hidden] (grouped-query)
            s[p + f"self_attn.{n}.weight"] = (m.kv_dim if n in ("k_proj", "v_proj") else m.hidden, m.hidden)
        s[p + "mlp.gate_proj.weight"] = (m.inter, m.hidden)
        s[p + "mlp.up_proj.weight"] = (m.inter, m.hidden)
        s[p + "mlp.down_proj.weight"] = (m.hidden, m.inter)
        s[p + "input_layernorm.weight"] = (m.hidden,)
        s[p + "post_attention_layernorm.weight"] = (m.hidden,)
    return s


def all_shapes(cfg: PSGConfig) -> dict:
    s = head_shapes(cfg)
    s.update(llm_shapes(cfg))
    return s


def _std_for(key: str, shape) -> tuple[float, float]:
    """(mean, std) per tensor.  HF's default std=0.02 makes every softmax near-uniform, which would
    hide masking / ordering bugs; q/k get a larger std so attention is peaky."""
    if key.endswith("LayerNorm.weight") or key.endswith("layernorm.weight") or key.endswith("norm.weight"):
        return 1.0, 0.1
    if key.endswith(".bias"):
        return 0.0, 0.05
    if key in ("relation_query", "rel_cls_query"):
        return 0.0, 1.0                       # torch.randn in the reference (V4:87-90)
    if "embeddings.weight" in key or key.endswith("embed_tokens.weight"):
        return 0.0, 1.0
    fan_in = int(np.prod(shape[1:]))
    if key.endswith("patch_embed.proj.weight"):
        return 0.0, 1.0 / np.sqrt(fan_in)     # features ~N(0,1) -> patches ~N(0,1)
    if ".attention.query." in key or ".attention.key." in key:
        return 0.0, 2.2 / np.sqrt(fan_in)
    if "q_proj" in key or "k_proj" in key:
        return 0.0, 2.0 / np.sqrt(fan_in)
    if key.endswith("lm_head.weight"):
        return 0.0, 3.0 / np.sqrt(fan_in)     # logit std ~3 -> argmax margins >> fp32 noise
    if key.startswith("binary_rel_cls_pred"):
        return 0.0, 2.0 / np.sqrt(fan_in)
    if key.startswith("multiclass_rel_cls_pred"):
        return 0.0, 2.0 / np.sqrt(fan_in)
    return 0.0, 1.0 / np.sqrt(fan_in)


def make_weights_numpy(cfg: PSGConfig, seed: int = 0, with_llm: bool = True) -> dict:
    """fp32 CPU tensors, numpy PCG64, filled in sorted-key order (bit-reproducible)."""
    shapes = all_shapes(cfg) if with_llm else head_shapes(cfg)
    rng = np.random.default_rng(seed)
    out = {}
    for key in sorted(shapes):
        mean, std = _std_for(key, shapes[key])
        a = rng.standard_normal(shapes[key], dtype=np.float32) * np.float32(std) + np.float32(mean)
        out[key] = torch.from_numpy(a.astype(np.float32))
    return out


def extend_llm_weights_numpy(w: dict, cfg: PSGConfig, seed_base: int = 1000, threads: int = 8) -> dict:
    """`w` plus every `language_model.*` tensor of `cfg` it lacks (the layers behind a truncated model's), fp32 CPU
    tensors.  ONE numpy PCG64 generator PER TENSOR, seeded `seed_base + i` with i = the tensor's index in the sorted
    schema of `cfg`: bit-reproducible on any box whatever the thread count, and fast enough for the un-truncated
    Llama-2-7B shape (27 GB; `make_weights_numpy`'s single stream would take minutes).  The CPU oracle and the GPU head
    of the 32-layer decode parity check (bench.py `parity...decode_7b_32_layers`, tests/test_gpu_llm7b.py) are both
    fed from this dict, so they hold the same values."""
    from concurrent.futures import ThreadPoolExecutor
    out = dict(w)
    todo = [(i, key, shp) for i, (key, shp) in enumerate(sorted(llm_shapes(cfg).items())) if key not in out]

    def fill(job):                                          # numpy releases the GIL while it draws
        i, key, shp = job
        mean, std = _std_for(key, shp)
        arr = np.random.default_rng(seed_base + i).standard_normal(shp, dtype=np.float32)
        arr *= np.float32(std)
        arr += np.float32(mean)
        return key, torch.from_numpy(arr)
    with ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
        out.update(ex.map(fill, todo))
    return out


def llm_matrices_as_fp16_values(w: dict, in_place=()) -> dict:
    """A dict in which every `language_model.*` matrix is the fp32 image of its fp16 rounding - the values the
    reference's frozen fp16 Llama-2-7b-hf checkpoint has after `from_pretrained` upcast it (V4:99-100,
    configs/psg/baseline_v4_ov.py:61-65).  Norm vectors and the head's own tensors are passed through.  Keys named in
    `in_place` are rounded inside their storage (the 27 GB of an un-truncated model are not held twice); every other
    matrix is a new tensor, so a dict sharing tensors with `w` keeps its values."""
    out, in_place = {}, set(in_place)
    for k, v in w.items():
        if k.startswith("language_model.") and v.dim() >= 2:
            if k in in_place:
                v.copy_(v.half().float())
                out[k] = v
            else:
                out[k] = v.half().float()
        else:
            out[k] = v
    return out


def make_weights_device(cfg: PSGConfig, seed: int, device, head_dtype=torch.float32,
                        llm_dtype=torch.bfloat16, with_llm: bool = True, llm_values=None) -> dict:
    """Random-init weights generated directly in HBM (benchmark use: 7B-shaped LLM).
    llm_values=torch.float16 with an fp32 `llm_dtype`: the LLM's matrices hold fp16 VALUES in fp32 tensors - what
    `from_pretrained` makes of the fp16 Llama-2-7b-hf checkpoint the reference loads and freezes (V4:99-100,
    configs/psg/baseline_v4_ov.py:61-65)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = {}
    shapes = all_shapes(cfg) if with_llm else head_shapes(cfg)
    for key in sorted(shapes):
        mean, std = _std_for(key, shapes[key])
        dt = llm_dtype if key.startswith("language_model.") else head_dtype
        t = torch.empty(shapes[key], device=device, dtype=torch.float32 if len(shapes[key]) < 2 else dt)
        if t.dtype == torch.float32:
            t.normal_(mean, std, generator=g)
        else:
            # fill in fp32 chunks to keep the distribution exact, then cast
            flat = t.view(-1)
            step = 1 << 26
            for o in range(0, flat.numel(), step):
                n = min(step, flat.numel() - o)
                chunk = torch.empty(n, device=device).normal_(mean, std, generator=g)
                if llm_values is not None and key.startswith("language_model."):
                    chunk = chunk.to(llm_values).float()
                flat[o:o + n] = chunk.to(dt)
        if t.dtype == torch.float32 and len(shapes[key]) >= 2 and llm_values is not None and key.startswith("language_model."):
            t = t.to(llm_values).float()
        out[key] = t.to(dt) if len(shapes[key]) >= 2 else t
    return out


# ---- FP8-quantised LLM matrices ---------------------------------------------------------------------------
# ONE definition of the quantised model, used by the head's option, the checkpoint reader, the engine and the tests: a
# matrix is (q, s) = (OCP e4m3fn bytes [N, K], fp32 per-row scales [N]) and its value is W' = float32(q) * s[:, None], one
# fp32 rounding per element.  Per-row scales commute with the row concatenations the engine makes (q|k|v, gate|up).
FP8_MAX = 448.0                                                    # largest finite e4m3fn value
LLM_QUANT_MATRICES = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                      "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")
SCALE_SUFFIX = "_scale"                                            # `<name>.weight` -> `<name>.weight_scale`


def quantize_fp8_rows(W: torch.Tensor):
    """W [N, K] -> (q uint8 [N, K]: e4m3fn bytes, s fp32 [N]).  s[n] = max_k |W[n, k]| / 448 in fp32 (1 for an all-zero
    row), q[n, k] = W[n, k] / s[n] clamped to +-448 and rounded to nearest even on the e4m3fn grid."""
    if W.dim() != 2:
        raise ValueError(f"quantize_fp8_rows takes a matrix, got shape {tuple(W.shape)}")
    W = W.to(torch.float32)
    amax = W.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (W / s[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), s


def dequantize_fp8_rows(q: torch.Tensor, s: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """W' = float32(q) * s[:, None] (one fp32 rounding per element), then `dtype`."""
    q8 = q if q.dtype == torch.float8_e4m3fn else q.view(torch.float8_e4m3fn)
    return (q8.to(torch.float32) * s.to(torch.float32)[:, None]).to(dtype)


def is_quantized(weights: dict, key: str) -> bool:
    return key + SCALE_SUFFIX in weights or key + GSCALE_SUFFIX in weights


def quant_format(weights: dict, key: str):
    """None, 'fp8', 'mxfp4' or 'int4': how the matrix `key` comes in `weights` (an MXFP4 matrix has its block exponents beside
    it, a group-wise INT4 matrix its group scales and zero points)."""
    if key + GSCALE_SUFFIX in weights:
        return "int4"
    if not is_quantized(weights, key):
        return None
    return "mxfp4" if key + BEXP_SUFFIX in weights else "fp8"


# ---- MXFP4-quantised LLM matrices -------------------------------------------------------------------------
# OCP Microscaling FP4: E2M1 elements (+-{0, 0.5, 1, 1.5, 2, 3, 4, 6}), one power-of-two exponent per block of 32
# consecutive k, anchored to the row: a matrix is (q, e, s) = (uint8 [N, K / 2]: two codes per byte, the LOW nibble the
# even k; uint8 [N, K / 32]: 127 + E_b - Emax[n], in 114..127; fp32 [N]: 2^Emax[n]) and its value is
#     W'[n, k] = fp4(q[n, k]) * 2^(e[n, k // 32] - 127) * s[n].
# E_b = floor(log2 max|block|) - 2 (the OCP rule: E2M1's largest binade is 2^2), floored at Emax[n] - 13 with Emax the
# row's largest E_b, so that W' / s is a NORMAL fp16 number or zero and W' is exactly an FP8 model (mxfp4_as_fp8_rows).
BEXP_SUFFIX = "_bexp"                                              # `<name>.weight` -> `<name>.weight_bexp`
MXFP4_BLOCK = 32
MXFP4_EXP_SPAN = 13                                                # a block's exponent lies at most this far below its row's
MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)              # the magnitudes of codes 0..7; bit 3 is the sign


def quantize_mxfp4_rows(W: torch.Tensor):
    """W [N, K], K % 32 == 0 -> (q uint8 [N, K / 2], e uint8 [N, K / 32], s fp32 [N]) as defined above.  An element is the
    nearest grid point to W / 2^E_b, ties to the even code, magnitudes above 6 saturate; a value that rounds to zero takes
    code 0x0, never 0x8 (-0), so that quantising W' again returns the same codes.  An all-zero block takes the floor
    exponent, an all-zero row Emax = 0.  Emax is not taken below -126 (s stays a normal fp32 number)."""
    if W.dim() != 2 or W.shape[1] % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4_rows takes a matrix [N, K] with K % {MXFP4_BLOCK} == 0, got shape {tuple(W.shape)}")
    N, K = W.shape
    Wb = W.to(torch.float32).reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = Wb.abs().amax(dim=2)
    nz = amax > 0
    Eb = torch.frexp(amax)[1].to(torch.int32) - 3                  # amax = m 2^x, m in [0.5, 1): floor(log2) = x - 1
    Eb = torch.where(nz, Eb, torch.full_like(Eb, -1000))
    Emax = Eb.amax(dim=1)
    Emax = torch.where(nz.any(dim=1), Emax, torch.zeros_like(Emax)).clamp_(min=-126)
    Eb = torch.maximum(Eb, (Emax - MXFP4_EXP_SPAN)[:, None])
    a = Wb.abs().to(torch.float64) * torch.exp2(-Eb.to(torch.float64))[:, :, None]      # exact: a power-of-two scale
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
            + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    code = code + (((Wb < 0) & (code > 0)).to(torch.uint8) << 3)
    code = code.reshape(N, K // 2, 2)
    q = code[:, :, 0] | (code[:, :, 1] << 4)
    e = (127 + Eb - Emax[:, None]).to(torch.uint8)
    s = torch.exp2(Emax.to(torch.float32))
    return q.contiguous(), e.contiguous(), s


def _mxfp4_unscaled(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fp4(q) * 2^(e - 127) as fp32 [N, K] (exact)."""
    N, Kh = q.shape
    q = q.view(torch.uint8) if q.dtype != torch.uint8 else q
    code = torch.stack((q & 0xF, q >> 4), dim=2).reshape(N, 2 * Kh).to(torch.int64)
    grid = torch.tensor(MXFP4_GRID + tuple(-g for g in MXFP4_GRID), dtype=torch.float32, device=q.device)
    bs = (e.to(torch.int32) << 23).view(torch.float32)             # 2^(e - 127), as the kernels build it
    return (grid[code].reshape(N, -1, MXFP4_BLOCK) * bs[:, :, None]).reshape(N, 2 * Kh)


def dequantize_mxfp4_rows(q: torch.Tensor, e: torch.Tensor, s: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """W' = (fp4(q) * 2^(e - 127)) * s[:, None] (the bracket is exact, then one fp32 rounding per element), then `dtype`."""
    return (_mxfp4_unscaled(q, e) * s.to(torch.float32)[:, None]).to(dtype)


def mxfp4_as_fp8_rows(q: torch.Tensor, e: torch.Tensor, s: torch.Tensor):
    """The exact FP8 image of an MXFP4 matrix with e in 114..127: (e4m3fn bytes uint8 [N, K] of W' / s * 64, fp32 row scales
    s / 64).  The values lie in 2^-8 .. 384 on e4m3fn's grid, so `dequantize_fp8_rows` of the pair is W' bit for bit."""
    if int(e.min()) < 127 - MXFP4_EXP_SPAN or int(e.max()) > 127:
        raise ValueError(f"mxfp4_as_fp8_rows: block exponents must lie in {127 - MXFP4_EXP_SPAN}..127")
    q8 = (_mxfp4_unscaled(q, e) * 64.0).to(torch.float8_e4m3fn)
    return q8.view(torch.uint8), s.to(torch.float32) / 64.0


def _take_mxfp4(out: dict, path):
    """The MXFP4 matrices of a checkpoint - `*.weight` uint8 [N, K / 2] (low nibble = even k) with a sibling `*.weight_scale`
    uint8 [N, K / 32] (E8M0: the block's scale is 2^(byte - 127)) - row-anchored into the model above: s = 2^(largest
    exponent byte of the row's non-zero blocks - 127) under name + '_scale', the bytes rebased to 127 = the row's largest
    under name + '_bexp', all-zero blocks moved to the floor.  The value of every element is unchanged."""
    from ._lib import PsgHipError
    for ks in [k for k in out if k.endswith(".weight" + SCALE_SUFFIX)]:
        kw = ks[:-len(SCALE_SUFFIX)]
        w, sc = out.get(kw), out[ks]
        if w is None or w.dtype != torch.uint8 or sc.dtype != torch.uint8:
            continue
        if w.dim() != 2 or sc.dim() != 2 or sc.shape[0] != w.shape[0]:
            raise PsgHipError(f"{path}: MXFP4 tensor {kw}: weight {tuple(w.shape)} / weight_scale {tuple(sc.shape)} are not "
                              "[N, K / 2] / [N, K / 32]")
        N, K = w.shape[0], 2 * w.shape[1]
        if K % MXFP4_BLOCK or sc.shape[1] * MXFP4_BLOCK != K:
            raise PsgHipError(f"{path}: MXFP4 tensor {kw}: K = {K} with {sc.shape[1]} block exponents per row (K % "
                              f"{MXFP4_BLOCK} == 0 and one exponent per {MXFP4_BLOCK} elements)")
        lo, hi = w & 0xF, w >> 4
        if bool(((lo == 8) | (hi == 8)).any()):
            raise PsgHipError(f"{path}: MXFP4 tensor {kw} holds the code 0x8 (-0): not part of the model (re-quantising "
                              "would not return it); write +0 (0x0)")
        if bool((sc == 255).any()):
            raise PsgHipError(f"{path}: MXFP4 tensor {kw}: weight_scale holds 0xFF (E8M0 NaN)")
        nzb = (w.reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK // 2) != 0).any(dim=2)          # (no 0x8: a zero block is zero bytes)
        eb = sc.to(torch.int32)
        emax = torch.where(nzb, eb, torch.full_like(eb, -1)).amax(dim=1)
        emax = torch.where(emax >= 0, emax, torch.full_like(emax, 127))                   # an all-zero row: s = 1
        rel = 127 + eb - emax[:, None]
        if bool((nzb & (rel < 127 - MXFP4_EXP_SPAN)).any()):
            n, b = [int(v[0]) for v in torch.nonzero(nzb & (rel < 127 - MXFP4_EXP_SPAN), as_tuple=True)]
            raise PsgHipError(f"{path}: MXFP4 tensor {kw}: block {b} of row {n} lies 2^{int(emax[n] - eb[n, b])} below its "
                              f"row's largest block exponent (at most 2^{MXFP4_EXP_SPAN}: the widened weight must stay a "
                              "normal fp16 number)")
        out[kw + BEXP_SUFFIX] = torch.where(nzb, rel, torch.full_like(rel, 127 - MXFP4_EXP_SPAN)).to(torch.uint8).contiguous()
        out[ks] = torch.exp2((emax - 127).to(torch.float32))
    return out


# ---- group-wise INT4 LLM matrices (GPTQ / AWQ checkpoints) ---------------------------------------------------
# A matrix W [N, K] with group size G is (q, gs, gz) = (uint8 [N, K / 2]: two 4-bit codes per byte, the LOW nibble the even
# k - MXFP4's storage order; fp16 [N, K / G]: finite, non-zero group scales; uint8 [N, K / G]: zero points 0..15) and its
# value is
#     W'[n, k] = float(gs[n, k // G]) * (q[n, k] - gz[n, k // G]):
# the integer difference is exact, the product one fp32 rounding.  G in {32, 64, 128}, K % G == 0; it is K / gs.shape[1].
# Groups lie within a row, so the model commutes with the engine's row concatenations (q|k|v, gate|up).
GSCALE_SUFFIX = "_gscale"                                          # `<name>.weight` -> `<name>.weight_gscale`
GZERO_SUFFIX = "_gzero"                                            # `<name>.weight` -> `<name>.weight_gzero`
INT4_GROUPS = (32, 64, 128)
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)                               # AWQ gemm: nibble i of word m holds column 8 m + AWQ_ORDER[i]


def _nearest_fp16(x: torch.Tensor) -> torch.Tensor:
    """float64 x in [2^-14, 65504] -> the nearest fp16, ties to even, without the double rounding of a cast through fp32."""
    c = x.to(torch.float32).to(torch.float16).view(torch.int16).to(torch.int32)
    cand = torch.stack((c - 1, c, c + 1), dim=-1)                  # (positive: the neighbours are the bit patterns +- 1)
    val = cand.to(torch.int16).view(torch.float16).to(torch.float64)
    err = (val - x.unsqueeze(-1)).abs()
    err = torch.where(torch.isfinite(val), err, torch.full_like(err, float("inf")))
    tie = err == err.amin(dim=-1, keepdim=True)                    # (two candidates equally near: the even bit pattern)
    pick = torch.where(tie & (cand % 2 == 0), 0, torch.where(tie, 1, 2)).argmin(dim=-1, keepdim=True)
    return cand.gather(-1, pick).squeeze(-1).to(torch.int16).view(torch.float16)


def _int4_group(name, K, n_groups):
    if n_groups <= 0 or K % n_groups or K // n_groups not in INT4_GROUPS or K % (K // n_groups):
        raise ValueError(f"{name}: K = {K} with {n_groups} groups per row (a group is one of {INT4_GROUPS} weights, K % G == 0)")
    return K // n_groups


def quantize_int4_groups(W: torch.Tensor, group: int = 128):
    """W [N, K] -> (q uint8 [N, K / 2], gs fp16 [N, K / G], gz uint8 [N, K / G]): round to nearest, asymmetric, per (row,
    group) in float64: lo = min(min w, 0), hi = max(max w, 0); s = (hi - lo) / 15 rounded to the nearest fp16 and clamped to
    [2^-14, 65504]; with that s, z = clamp(rint(-lo / s), 0, 15) and q = clamp(rint(w / s) + z, 0, 15), rint ties to even.
    An all-zero group gets s = 2^-14, z = 0, q = 0."""
    if W.dim() != 2 or group not in INT4_GROUPS or W.shape[1] % group:
        raise ValueError(f"quantize_int4_groups takes a matrix [N, K] with K % group == 0 and group in {INT4_GROUPS}, got shape "
                         f"{tuple(W.shape)}, group {group}")
    N, K = W.shape
    Wg = W.to(torch.float64).reshape(N, K // group, group)
    lo = Wg.amin(dim=2).clamp_max(0.0)
    hi = Wg.amax(dim=2).clamp_min(0.0)
    gs = _nearest_fp16(((hi - lo) / 15.0).clamp(2.0 ** -14, 65504.0))
    s = gs.to(torch.float64)
    z = torch.round(-lo / s).clamp_(0, 15)
    code = (torch.round(Wg / s[:, :, None]) + z[:, :, None]).clamp_(0, 15).to(torch.uint8).reshape(N, K // 2, 2)
    q = code[:, :, 0] | (code[:, :, 1] << 4)
    return q.contiguous(), gs.contiguous(), z.to(torch.uint8).contiguous()


def dequantize_int4_groups(q: torch.Tensor, gs: torch.Tensor, gz: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """W' = float32(gs) * (q - gz) per group (the difference exact, ONE fp32 rounding per element), then `dtype`."""
    N, Kh = q.shape
    K = 2 * Kh
    G = _int4_group("dequantize_int4_groups", K, gs.shape[1])
    if q.dtype != torch.uint8 or gs.dtype != torch.float16 or gz.dtype != torch.uint8 or tuple(gz.shape) != tuple(gs.shape) \
            or gs.shape[0] != N:
        raise ValueError(f"dequantize_int4_groups: q uint8 [N, K / 2], gs fp16 / gz uint8 [N, K / G], got {q.dtype} "
                         f"{tuple(q.shape)}, {gs.dtype} {tuple(gs.shape)}, {gz.dtype} {tuple(gz.shape)}")
    code = torch.stack((q & 15, q >> 4), dim=2).reshape(N, K // G, G).to(torch.float32)
    return ((code - gz.to(torch.float32)[:, :, None]) * gs.to(torch.float32)[:, :, None]).reshape(N, K).to(dtype)


def read_hf_quant_config(path):
    """The weight-quantisation settings of a GPTQ / AWQ checkpoint directory: `quantization_config` of config.json, or the
    sibling quantize_config.json of old AutoGPTQ exports; None when there is neither."""
    import json
    import os
    with open(os.path.join(path, "config.json")) as f:
        qc = json.load(f).get("quantization_config")
    if qc is None and os.path.isfile(os.path.join(path, "quantize_config.json")):
        with open(os.path.join(path, "quantize_config.json")) as f:
            qc = json.load(f)
    return qc


def _unpack_int32_nibbles(t: torch.Tensor, dim: int, order=None) -> torch.Tensor:
    """int32 words -> uint8 nibbles: `dim` grows eightfold, nibble i (bits 4 i .. 4 i + 3) of word m to index 8 m + i - or,
    with `order`, to 8 m + order[i]."""
    t = t.movedim(dim, -1)
    sh = torch.arange(0, 32, 4, dtype=torch.int32)
    nib = ((t.unsqueeze(-1) >> sh) & 15).to(torch.uint8)               # [..., words, 8]
    if order is not None:
        out = torch.empty_like(nib)
        out[..., list(order)] = nib
        nib = out
    return nib.reshape(*t.shape[:-1], t.shape[-1] * 8).movedim(-1, dim)


def _take_int4(out: dict, path):
    """The group-wise INT4 matrices of a GPTQ / AWQ checkpoint - a linear layer X stored as X.qweight, X.qzeros, X.scales
    (+ X.g_idx) - converted WITHOUT changing a value to (q, gs, gz) under X.weight, X.weight_gscale, X.weight_gzero.
    The layouts read (nothing of either tool was available to check them against; INTEGRATION.md repeats this), for K
    inputs, N outputs, g = k // group_size:
      GPTQ (quant_method 'gptq' or absent): qweight int32 [K / 8, N], code (k, n) = bits 4 (k % 8) .. + 3 of qweight[k // 8,
        n]; qzeros int32 [K / G, N / 8], stored (g, n) = bits 4 (n % 8) .. + 3 of qzeros[g, n // 8], z = stored for
        checkpoint_format 'gptq_v2', else (stored + 1) & 15; scales fp16 [K / G, N];
      AWQ (quant_method 'awq', version 'gemm', zero_point true): qweight int32 [K, N / 8], qzeros int32 [K / G, N / 8], nibble
        i of word m holds column 8 m + AWQ_ORDER[i], z = stored; scales fp16 [K / G, N]."""
    from ._lib import PsgHipError
    layers = sorted(k[:-len(".qweight")] for k in out if k.endswith(".qweight"))
    if not layers:
        return out
    qc = read_hf_quant_config(path)
    if qc is None:
        raise PsgHipError(f"{path}: {layers[0]}.qweight is a packed quantised layer, but there is no quantization_config in "
                          "config.json and no quantize_config.json")
    other = sorted(k for k, v in out.items() if k.endswith(".weight" + SCALE_SUFFIX) or
                   v.dtype in (torch.float8_e4m3fn, torch.float8_e4m3fnuz, torch.float8_e5m2, torch.float8_e5m2fnuz))
    if other:
        raise PsgHipError(f"{path}: {layers[0]}.qweight is group-wise INT4 and {other[0]} is FP8 / MXFP4: a checkpoint that mixes "
                          "quantised formats is not built")
    method = str(qc.get("quant_method", "gptq")).lower()
    bits, G = qc.get("bits"), qc.get("group_size")
    for X in layers:
        why = None
        if method not in ("gptq", "awq"):
            why = f"quant_method {method!r} is not built (gptq, awq)"
        elif bits != 4:
            why = f"bits={bits!r}: only 4-bit codes are built"
        elif G not in INT4_GROUPS:
            why = f"group_size={G!r}: a group is one of {INT4_GROUPS} weights (per-channel, -1, is not built)"
        elif qc.get("desc_act"):
            why = "desc_act=true (act-order) is not built"
        elif method == "awq" and str(qc.get("version", "gemm")).lower() != "gemm":
            why = f"AWQ version {qc.get('version')!r} is not built (gemm)"
        elif method == "awq" and not qc.get("zero_point", True):
            why = "AWQ with zero_point=false is not built"
        if why:
            raise PsgHipError(f"{path}: {X}.qweight: {why}")
        qw, qz, sc = out.get(X + ".qweight"), out.get(X + ".qzeros"), out.get(X + ".scales")
        if qz is None or sc is None:
            raise PsgHipError(f"{path}: {X}.qweight has no {X}.qzeros / {X}.scales beside it")
        if qw.dtype != torch.int32 or qz.dtype != torch.int32 or sc.dtype != torch.float16 or qw.dim() != 2:
            raise PsgHipError(f"{path}: {X}: qweight / qzeros must be int32 and scales fp16, got {qw.dtype} / {qz.dtype} / {sc.dtype}")
        K, N = (qw.shape[0] * 8, qw.shape[1]) if method == "gptq" else (qw.shape[0], qw.shape[1] * 8)
        consistent = N % 8 == 0 and sc.dim() == 2 and sc.shape[1] == N and tuple(qz.shape) == (sc.shape[0], N // 8)
        if consistent and K % G:
            raise PsgHipError(f"{path}: {X}.qweight: K = {K} is no multiple of group_size = {G}")
        if not consistent or sc.shape[0] != K // G:
            raise PsgHipError(f"{path}: {X}: qweight {tuple(qw.shape)} as {method} means K = {K}, N = {N}, but scales are "
                              f"{tuple(sc.shape)} (expected {(K // G, N)}) and qzeros {tuple(qz.shape)} (expected "
                              f"{(K // G, N // 8)}): the shapes contradict quant_method {method!r}")
        gi = out.pop(X + ".g_idx", None)
        if gi is not None and not torch.equal(gi.to(torch.int64).reshape(-1), torch.arange(K, dtype=torch.int64) // G):
            raise PsgHipError(f"{path}: {X}.g_idx is not k // group_size: act-order (desc_act) is not built")
        absf = sc.to(torch.float32).abs()
        if not bool(torch.isfinite(absf).all()) or bool((absf < 2.0 ** -14).any()):
            raise PsgHipError(f"{path}: {X}.scales holds a zero, subnormal or non-finite scale")
        b = out.pop(X + ".bias", None)
        if b is not None and bool((b != 0).any()):
            raise PsgHipError(f"{path}: {X}.bias is not zero: bias tensors are not built (Llama / Mistral projections have none)")
        if method == "gptq":
            code = _unpack_int32_nibbles(qw, 0)                        # [K, N]
            z = _unpack_int32_nibbles(qz, 1)                           # [K / G, N]
            if qc.get("checkpoint_format") != "gptq_v2":
                z = (z + 1) & 15                                       # (the exporter stores z - 1)
        else:
            code = _unpack_int32_nibbles(qw, 1, AWQ_ORDER)
            z = _unpack_int32_nibbles(qz, 1, AWQ_ORDER)
        code = code.t().reshape(N, K // 2, 2)
        for k in (".qweight", ".qzeros", ".scales"):
            del out[X + k]
        out[X + ".weight"] = (code[:, :, 0] | (code[:, :, 1] << 4)).contiguous()
        out[X + ".weight" + GSCALE_SUFFIX] = sc.t().contiguous()
        out[X + ".weight" + GZERO_SUFFIX] = z.t().contiguous()
    return out


def llm_quant_keys(n_layers: int, lm_head: bool = False):
    """Names of the matrices llm_weight_quant quantises: q/k/v/o/gate/up/down of the kept layers (+ the lm_head on
    request); never the embedding, the norms or language_projection."""
    keys = [f"language_model.model.layers.{l}.{n}" for l in range(n_layers) for n in LLM_QUANT_MATRICES]
    return keys + (["language_model.lm_head.weight"] if lm_head else [])


def quantize_llm_weights(weights: dict, n_layers: int, lm_head: bool = False, fmt: str = "fp8") -> dict:
    """`weights` with every matrix of `llm_quant_keys` replaced by its (q, s): the byte tensor under the matrix's own name,
    the scales under name + '_scale'; fmt='mxfp4': its (q, e, s), the block exponents under name + '_bexp'; fmt='int4g': its
    (q, gs, gz) in groups of 128, under name, name + '_gscale', name + '_gzero'.  A matrix that already comes quantised - an
    FP8, MXFP4, GPTQ or AWQ checkpoint - is kept as it is."""
    if fmt not in ("fp8", "mxfp4", "int4g"):
        raise ValueError(f"quantize_llm_weights: fmt must be 'fp8', 'mxfp4' or 'int4g', got {fmt!r}")
    out = dict(weights)
    for k in llm_quant_keys(n_layers, lm_head):
        if k in out and not is_quantized(out, k):
            if fmt == "fp8":
                out[k], out[k + SCALE_SUFFIX] = quantize_fp8_rows(out[k])
            elif fmt == "int4g":
                out[k], out[k + GSCALE_SUFFIX], out[k + GZERO_SUFFIX] = quantize_int4_groups(out[k], 128)
            else:
                out[k], out[k + BEXP_SUFFIX], out[k + SCALE_SUFFIX] = quantize_mxfp4_rows(out[k])
    return out


class LazyQuantWeights(dict):
    """The mapping `quantize_llm_weights` would return, without ever holding it: what llm_weight_resident='quantised' hands
    the decode engine.  A matrix of `quant_keys` that is not quantised yet is quantised in row chunks WHERE IT
    LIVES (`quantize_fp8_rows` / `quantize_mxfp4_rows`: rows are independent, so the chunks give the bits of the one-shot call
    on the same device - the model is the one `quantize_llm_weights` makes of the same tensors, which a quantiser run on
    another device need not be: torch divides by a scalar as a multiplication by its reciprocal on the GPU), its parts are
    moved to `device` and handed out under its own name, name + '_scale' and name + '_bexp' - for the ONE matrix asked for
    last; the previous one is dropped.  Everything else comes from
    `weights` as it is; plain dict entries (language_projection.*) are set on the object.  The dense model
    therefore never reaches `device` on the way: host weights are quantised on the host and only bytes are uploaded; weights
    that already live on the device cost one chunk in fp32 plus the quantiser's temporaries."""

    def __init__(self, weights: dict, quant_keys, fmt, device, chunk_elems: int = 1 << 22):
        super().__init__()
        if quant_keys and fmt not in ("fp8", "mxfp4"):
            raise ValueError(f"LazyQuantWeights: fmt must be 'fp8' or 'mxfp4', got {fmt!r}")
        self._src, self._fmt, self._device, self._chunk = weights, fmt, torch.device(device), int(chunk_elems)
        self._quant = {k for k in quant_keys if k in weights and not is_quantized(weights, k)}
        self._last = (None, None)

    def _base(self, key):
        """(matrix name, part) when `key` names a part of a matrix this object quantises, else None."""
        if key in self._quant:
            return key, "q"
        if key.endswith(SCALE_SUFFIX) and key[:-len(SCALE_SUFFIX)] in self._quant:
            return key[:-len(SCALE_SUFFIX)], "s"
        if self._fmt == "mxfp4" and key.endswith(BEXP_SUFFIX) and key[:-len(BEXP_SUFFIX)] in self._quant:
            return key[:-len(BEXP_SUFFIX)], "e"
        return None

    def __contains__(self, key):
        return dict.__contains__(self, key) or self._base(key) is not None or key in self._src

    def __getitem__(self, key):
        if dict.__contains__(self, key):
            return dict.__getitem__(self, key)
        hit = self._base(key)
        if hit is None:
            return self._src[key]
        name, part = hit
        if self._last[0] != name:
            self._last = (None, None)                              # (drop the previous matrix before making this one)
            self._last = (name, self._quantise(self._src[name]))
        return self._last[1][part]

    def _quantise(self, W):
        W = torch.as_tensor(W)
        # (a chunk is at most a quarter of the matrix: the MXFP4 quantiser's float64 temporaries are ~8 x the chunk's fp32
        # bytes, and the load must stay within a few fp32 copies of ONE matrix above the final footprint)
        rows = max(1, min(self._chunk, W.numel() // 4) // max(1, int(W.shape[1])))
        out = []
        for r0 in range(0, W.shape[0], rows):
            Wc = W[r0:r0 + rows]
            out.append(quantize_fp8_rows(Wc) if self._fmt == "fp8" else quantize_mxfp4_rows(Wc))
            del Wc
        parts = [(torch.cat(p, 0) if len(p) > 1 else p[0]).to(self._device) for p in zip(*out)]
        return dict(zip(("q", "s") if self._fmt == "fp8" else ("q", "e", "s"), parts))


def _take_fp8_pairs(out: dict, path):
    """The (weight, weight_scale) pairs of an FP8 checkpoint, as stored: weight stays float8_e4m3fn, the scale becomes
    fp32 [N] (a per-tensor scalar is expanded).  Activation scales (`input_scale`) are dropped: execution is weight-only."""
    from ._lib import PsgHipError
    for k in [k for k in out if k.endswith(".input_scale")]:
        del out[k]
    for ks in [k for k in out if k.endswith(".weight" + SCALE_SUFFIX)]:
        kw = ks[:-len(SCALE_SUFFIX)]
        if kw + BEXP_SUFFIX in out:                                    # an MXFP4 matrix (_take_mxfp4)
            continue
        w, s = out.get(kw), out[ks].to(torch.float32)
        if w is None or w.dtype != torch.float8_e4m3fn or w.dim() != 2:
            raise PsgHipError(f"{path}: {ks} has no float8_e4m3fn matrix {kw} beside it")
        N = w.shape[0]
        if s.numel() == 1:
            s = s.reshape(1).expand(N)
        elif tuple(s.shape) not in ((N,), (N, 1)):
            raise PsgHipError(f"{path}: {ks} has shape {tuple(s.shape)}: block-scaled / group-scaled FP8 is not built (a "
                              f"scalar, [{N}] or [{N}, 1])")
        out[ks] = s.reshape(N).contiguous()
    bare = sorted(k for k, v in out.items() if v.dtype == torch.float8_e4m3fn and k + SCALE_SUFFIX not in out)
    if bare:
        raise PsgHipError(f"{path}: float8_e4m3fn tensors without a weight_scale: {bare[:3]}")
    other = sorted(k for k, v in out.items() if v.dtype in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.float8_e5m2fnuz))
    if other:
        raise PsgHipError(f"{path}: only OCP float8_e4m3fn weights are built, got {out[other[0]].dtype} for {other[:3]}")
    return out


# ---- the LLM of a local HuggingFace checkpoint directory (V4:99-103) --------------------------------------------------
# The reference builds its LLM with `AutoModelForCausalLM.from_pretrained(llm_model_name, low_cpu_mem_usage=True)`
# (V4:99-100): no dtype, so the fp16 tensors on disk are upcast to fp32; `llm_truncate_num` then keeps the first layers
# (V4:101-103).  There is no hub here and no need for the HF module: the head reads the directory itself - config.json,
# then `model.safetensors` / its sharded index / `pytorch_model*.bin` - and hands the tensors, under the names they have
# inside the reference head (`language_model.` + the checkpoint's own names), to the decode engine, which upcasts them on
# the device.  Tensors stay in their STORED dtype on the host: an fp16 checkpoint is then recognised as such by the
# engine's per-tensor round-trip check (llm.py, option llm_w16) exactly as its fp32 upcast would be.
def is_hf_checkpoint_dir(path) -> bool:
    import os
    return isinstance(path, (str, os.PathLike)) and os.path.isfile(os.path.join(path, "config.json"))


def hf_checkpoint_has_weights(path) -> bool:
    """True when the directory holds a model file `read_hf_llama_weights` can read (a tokenizer-only directory does not)."""
    import os
    return any(os.path.isfile(os.path.join(path, f)) for f in
               ("model.safetensors.index.json", "model.safetensors", "pytorch_model.bin.index.json", "pytorch_model.bin"))


def read_hf_llama_config(path, grouped_query=False):
    """LlamaConfig of the checkpoint directory `path` (its config.json).  Raises PsgHipError for an architecture the
    decode kernels are not built for (head_dim != 128, tied embeddings without an lm_head, rope_scaling, an active sliding
    window) or that would load but compute something else (biases, an activation other than SiLU).
    model_type 'llama' and 'mistral' (Mistral's sliding window never applies below the 4096-row rotary table).
    grouped_query=False refuses grouped-query attention (num_key_value_heads < num_attention_heads) as the multi-head
    readers did; the head's constructor passes True: groups of up to 8 query heads per key / value head."""
    import json
    import os
    from .config import LlamaConfig
    from ._lib import PsgHipError
    with open(os.path.join(path, "config.json")) as f:
        c = json.load(f)
    mt = c.get("model_type", "llama")
    if mt not in ("llama", "mistral"):
        raise PsgHipError(f"{path}: model_type {mt!r} is not built (llama, mistral)")
    heads = int(c["num_attention_heads"])
    kv = int(c.get("num_key_value_heads") or heads)
    if kv != heads and not grouped_query:
        raise PsgHipError(f"{path}: num_key_value_heads={kv} != num_attention_heads={heads} (grouped-query attention is "
                          "not built; the reference's LLM is Llama-2-7b, multi-head)")
    hidden = int(c["hidden_size"])
    if hidden % heads or hidden // heads != 128:
        raise PsgHipError(f"{path}: head_dim {hidden / heads:g} unsupported (kernels are built for 128)")
    if c.get("head_dim") is not None and int(c["head_dim"]) != 128:
        raise PsgHipError(f"{path}: head_dim={c['head_dim']} unsupported (kernels are built for 128)")
    if kv <= 0 or heads % kv or heads // kv > 8 or (heads // kv) & (heads // kv - 1):
        raise PsgHipError(f"{path}: num_key_value_heads={kv} with {heads} query heads is not built (grouped-query "
                          "attention takes a power-of-two group of at most 8 query heads per key / value head)")
    if c.get("rope_scaling"):
        raise PsgHipError(f"{path}: rope_scaling={c['rope_scaling']!r} is not built (Llama-2 has none)")
    sw = c.get("sliding_window")
    if sw is not None and int(sw) < 4096:
        raise PsgHipError(f"{path}: sliding_window={sw} is not built (null or >= 4096: a window that never applies)")
    for key in ("attention_bias", "mlp_bias"):
        if c.get(key):
            raise PsgHipError(f"{path}: {key}=true is not built (Llama / Mistral projections have no bias)")
    act = c.get("hidden_act", "silu")
    if act != "silu":
        raise PsgHipError(f"{path}: hidden_act={act!r} is not built (SwiGLU with silu)")

    def tok(name, default):
        v = c.get(name, default)
        return int(v[0] if isinstance(v, (list, tuple)) else default if v is None else v)
    return LlamaConfig(hidden=hidden, heads=heads, layers=int(c["num_hidden_layers"]), inter=int(c["intermediate_size"]),
                       vocab=int(c["vocab_size"]), rms_eps=float(c.get("rms_norm_eps", 1e-6)),
                       rope_theta=float(c.get("rope_theta", 10000.0)), bos=tok("bos_token_id", 1),
                       eos=tok("eos_token_id", 2), pad=0, kv_heads=None if kv == heads else kv)


def read_hf_llama_weights(path, n_layers=None, prefix="language_model."):
    """{prefix + name: tensor (stored dtype, CPU)} of the LlamaForCausalLM checkpoint in directory `path`; layers at or
    past `n_layers` (llm_truncate_num, V4:101-103) are not read.  Formats: model.safetensors, model.safetensors.index.json
    + shards, pytorch_model.bin, pytorch_model.bin.index.json + shards (in that order, as from_pretrained prefers them).
    An FP8 checkpoint (a `*.weight` of dtype float8_e4m3fn with a sibling `*.weight_scale`: per-tensor scalar, [N] or
    [N, 1]) is taken as it is: the matrix stays float8_e4m3fn, its scale becomes fp32 [N] under name + '_scale', nothing
    is re-quantised; `*.input_scale` entries are ignored (weight-only execution).  An MXFP4 checkpoint (`*.weight` uint8
    [N, K / 2] with a sibling `*.weight_scale` uint8 [N, K / 32]) is row-anchored (`_take_mxfp4`): name + '_scale' fp32 [N],
    name + '_bexp' uint8 [N, K / 32].  A GPTQ or AWQ checkpoint (`X.qweight`, `X.qzeros`, `X.scales` in place of `X.weight`)
    is converted value for value to the group-wise INT4 model (`_take_int4`): X.weight uint8 [N, K / 2], X.weight_gscale fp16
    and X.weight_gzero uint8 [N, K / G]."""
    import json
    import os
    from ._lib import PsgHipError

    def wanted(name):
        if name.endswith("rotary_emb.inv_freq"):                       # a buffer old checkpoints carry; recomputed (HF-LL:115-128)
            return False
        if n_layers is not None and n_layers > 0 and name.startswith("model.layers."):
            return int(name.split(".")[2]) < n_layers
        return True

    def shards(index_name, single_name):
        idx = os.path.join(path, index_name)
        if os.path.isfile(idx):
            with open(idx) as f:
                wm = json.load(f)["weight_map"]
            files = {}
            for name, fn in wm.items():
                if wanted(name):
                    files.setdefault(fn, []).append(name)
            return files
        if os.path.isfile(os.path.join(path, single_name)):
            return {single_name: None}
        return None

    out = {}
    files = shards("model.safetensors.index.json", "model.safetensors")
    if files is not None:
        from safetensors import safe_open
        for fn, names in sorted(files.items()):
            with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as f:
                for name in (names if names is not None else f.keys()):
                    if wanted(name):
                        try:
                            out[prefix + name] = f.get_tensor(name)
                        except Exception as e:  # noqa: BLE001  (a safetensors build without float8_e4m3fn)
                            raise PsgHipError(f"{path}: cannot read tensor {name!r} from {fn} ({e}); an FP8 checkpoint needs "
                                              "a safetensors package that delivers float8_e4m3fn") from e
    else:
        files = shards("pytorch_model.bin.index.json", "pytorch_model.bin")
        if files is None:
            raise PsgHipError(f"{path}: no model.safetensors / pytorch_model.bin (or their .index.json) found")
        for fn, names in sorted(files.items()):
            sd = torch.load(os.path.join(path, fn), map_location="cpu", weights_only=True)
            for name in (names if names is not None else list(sd)):
                if wanted(name):
                    out[prefix + name] = sd[name]
            del sd
    if prefix + "lm_head.weight" not in out:
        raise PsgHipError(f"{path}: no lm_head.weight (tied embeddings are not Llama-2's layout)")
    out = _take_int4(out, path)                                        # (drops the all-zero biases of its own layers)
    bias = sorted(k for k in out if k.endswith(".bias"))
    if bias:
        raise PsgHipError(f"{path}: bias tensors are not built (Llama / Mistral projections have none): {bias[:3]}")
    return _take_fp8_pairs(_take_mxfp4(out, path), path)
