"""One record per LLM projection matrix: everything `LlamaDecodeEngine` knows about a (row-concatenated) matrix - its dense
operand, its quantised parts, every image and copy made of it and the stream it has in a decode step - and the functions
that load the records from a weight mapping.  Pure torch apart from the split images: loads on the CPU too.

The formats (W' is the model's weight; it is kept in the engine's dtype unless the matrix is resident as bytes only - every
path not built for a stream computes the same model on the kernels it has):
  * FP8: `name` holds e4m3fn bytes q, `name + '_scale'` the fp32 per-row scales s; W' = float32(q) s.
  * MXFP4: `name` holds two fp4 codes per byte, `name + '_bexp'` the block exponents e, `name + '_scale'` s;
    W' = fp4(q) 2^(e - 127) s.  A shape of W4_STREAM_AS_FP8 (measured slower as nibbles than as bytes) keeps its exact FP8
    image as well and streams through the FP8 kernels: the same W' bit for bit.
  * group-wise INT4 (GPTQ / AWQ): `name` holds two 4-bit codes per byte, `name + '_gscale'` the fp16 group scales
    gs, `name + '_gzero'` the zero points gz; W' = gs (q - gz).  Only the kernel's code and group images are kept, and only
    for groups of 128, K % 256 == 0, N % 16 == 0 and shapes not in INT4_STREAM_OFF.  W' is no fp16 value (gs is an arbitrary
    fp16 number): the fp32s prompt pass runs on it as generic fp32 weights - there is no two-plane image.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import PsgHipError
from .weights import (BEXP_SUFFIX, GSCALE_SUFFIX, GZERO_SUFFIX, SCALE_SUFFIX, dequantize_fp8_rows, dequantize_int4_groups,
                      dequantize_mxfp4_rows, is_quantized, mxfp4_as_fp8_rows, quant_format, _mxfp4_unscaled)

# MXFP4 shapes (N, K) that stream as their exact FP8 image instead of as nibbles (acceptance rule): a shape goes
# here when tools/w4_bench.py measured psg_gemm_w4.hip's range of times NOT wholly below psg_gemm_w8.hip's on the same W'.
# "pair": fp32s engines (psg_split_gemm_w*), "single": 16-bit engines (psg_skinny_gemm_w*).  The image costs a byte per
# weight and is kept for these shapes only
W4_STREAM_AS_FP8 = {"pair": frozenset(), "single": frozenset()}

# Group-wise INT4 shapes (N, K) that do NOT stream as codes (acceptance rule): a shape goes here when
# tools/int4_bench.py measured psg_gemm_int4.hip's range of times not wholly below the range of what the engine runs for
# the shape on W' without the stream (pair: the fp32 decode kernel, single: the 16-bit skinny kernel).  The engine then
# runs it on W'; no image is kept for it
INT4_STREAM_OFF = {"pair": frozenset(), "single": frozenset()}


class LlmMatrix:
    """name, shape [N, K], dtype (of W'), device, fmt (None | 'fp8' | 'mxfp4' | 'int4') and, each None where the matrix has
    none:
      w        the dense operand W' (absent with resident='quantised', DESIGN 15: a dense operand then exists only for the
               length of one product, in the engine's scratch)
      q, s     the FP8 bytes / MXFP4 nibbles and the fp32 row scales; e, e_img: the raw MXFP4 block exponents (kept only
               without W': the expansion reads them) and the decode kernel's exponent image (K % 256 == 0)
      fp8_img  (bytes, row scales): the exact FP8 image of a W4_STREAM_AS_FP8 shape
      int4_img (code image, group image) of an INT4 matrix that streams as codes
      h16      the exact fp16 image of W' / s (of q) for the two-plane prompt pass of an fp32s engine
      w16, wb16  the fp16 / bf16 copy of an unquantised fp32 matrix whose every element is such a value (bf16_value_resident,
               DESIGN 24: `wb16` is then the ONLY thing the record holds - no w, no split, no packed - and the operand of
               every product over it)
      split    ([wh | wl | wh] fp16, the rows' inverse scales): the three-product prompt pass of an fp32s engine
      packed   ([wh | wl], inverse scales) of a generic lm_head under batch_split_gemm
      i2       the interleaved hi / lo image of the row-invariant path, made at first use (`interleaved`)
      stream   (kind, the arguments of ops.split_gemm_<kind> / ops.skinny_gemm_<kind> behind the rows): the stream the matrix
               has in a decode step of <= 32 rows, or None where it runs on W'; decided once, by `decide_stream`."""
    __slots__ = ("name", "shape", "dtype", "device", "fmt", "w", "q", "s", "e", "e_img", "fp8_img", "int4_img", "h16", "w16",
                 "wb16", "split", "packed", "i2", "stream")

    def __init__(self, name, shape, dtype, device, fmt=None, **fields):
        for k in self.__slots__[5:]:
            setattr(self, k, fields.pop(k, None))
        assert not fields, fields
        self.name, self.shape, self.dtype, self.device, self.fmt = name, torch.Size(shape), dtype, torch.device(device), fmt

    def numel(self):
        return self.shape[0] * self.shape[1]

    def quant_tensors(self):
        """The bytes, exponents, scales and stream images of a quantised matrix."""
        return [t for t in (self.q, self.e, self.e_img, self.s, *(self.fp8_img or ()), *(self.int4_img or ())) if t is not None]

    def tensors(self):
        """Every tensor the record owns."""
        own = (self.w, self.h16, self.w16, self.wb16, *(self.split or ()), *(self.packed or ()), *(self.i2 or ()))
        return self.quant_tensors() + [t for t in own if t is not None]

    def two_plane(self):
        """The fp16 operand of the two-plane prompt pass: the image of W' / s, or the fp16 copy of an fp16-valued W'."""
        return self.h16 if self.h16 is not None else self.w16

    def column_scale(self, ones):
        """... and its column scale: s, or `ones(N)` for an fp16-valued matrix (it has no scale of its own)."""
        return self.s if self.s is not None else ones(self.shape[0])

    def interleaved(self):
        if self.i2 is None:                                    # (only the dealt decodes of a pair-sharded job read it:
            self.i2 = ops.split_f16i2(self.w)                  # 4 bytes per weight next to the fp32 tensor)
        return self.i2

    def decide_stream(self):
        """An FP8 image comes before the nibbles (that is what makes a W4_STREAM_AS_FP8 shape stream as bytes); a quantised
        matrix has neither 16-bit copy, an fp16-valued one no bf16 copy."""
        N, K = self.shape
        w8 = self.fp8_img or ((self.q, self.s) if self.fmt == "fp8" else None)
        if w8 is not None and N % 16 == 0 and K % 128 == 0:
            self.stream = ("w8", w8)
        elif self.fmt == "mxfp4" and self.e_img is not None and N % 16 == 0:   # (K % 256 == 0 or there is no exponent image)
            self.stream = ("w4", (self.q, self.e_img, self.s))
        elif self.int4_img is not None:
            self.stream = ("int4", self.int4_img)
        elif self.w16 is not None:
            self.stream = ("w16", (self.w16,))
        else:
            self.stream = ("wb16", (self.wb16,)) if self.wb16 is not None else None
        return self


def dense_matrix(name, w, split=False):
    """The record of an unquantised tensor as it is (`split`: with its three-product split image)."""
    return LlmMatrix(name, w.shape, w.dtype, w.device, w=w, split=ops.split_f16x3(w, weights=True) if split else None)


def quant_parts(weights, keys, device, lean=False):
    """(q, s, e) of the FP8 / MXFP4 matrix of `keys`, row-concatenated and validated: the bytes, the fp32 row scales and the
    block exponents (None for FP8).  A key's parts are read together, one key after the other (the loader quantises a
    matrix when it is asked for and keeps none, head.load_llm_weights)."""
    qs, scs, es = [], [], []
    for k in keys:
        qs.append(weights[k].to(device).view(torch.uint8))
        scs.append(weights[k + SCALE_SUFFIX].to(device=device, dtype=torch.float32).reshape(-1))
        es.append(weights[k + BEXP_SUFFIX].to(device) if k + BEXP_SUFFIX in weights else None)
    if any(e is None for e in es) and not all(e is None for e in es):
        raise PsgHipError(f"{keys}: some parts are FP8-quantised and some MXFP4-quantised")
    # (resident='quantised' keeps a single part as it came: no second copy of the largest matrix during the load)
    cat = lambda ts: (torch.cat(ts, 0) if len(ts) > 1 or not lean else ts[0]).contiguous()   # noqa: E731
    q, sc = cat(qs), cat(scs)
    del qs, scs
    if sc.numel() != q.shape[0]:
        raise PsgHipError(f"{keys}: {sc.numel()} scales for {q.shape[0]} rows (per-row scales only)")
    if es[0] is None:
        return q, sc, None
    e = cat(es)
    N, K = q.shape[0], 2 * q.shape[1]
    if e.dtype != torch.uint8 or tuple(e.shape) != (N, K // 32) or K % 32 or int(e.min()) < 114 or int(e.max()) > 127:
        raise PsgHipError(f"{keys}: block exponents must be uint8 [{N}, {K // 32}] in 114..127 "
                          "(weights.quantize_mxfp4_rows), got " f"{e.dtype} {tuple(e.shape)}")
    return q, sc, e


def _lean_matrix(weights, keys, device, dtype):
    """resident='quantised': the matrix of `keys` as its bytes only."""
    name = keys[0].rsplit(".", 2)[0] + "." + "|".join(k.split(".")[-2] for k in keys)
    q, sc, e = quant_parts(weights, keys, device, lean=True)
    if e is None:
        N, K = q.shape
        if N % 16 or K % 128:
            raise PsgHipError(f"resident='quantised': {name} [{N}, {K}] does not fit the FP8 byte-stream kernels of the "
                              "decode steps (N % 16 == 0, K % 128 == 0), and there is no W' to fall back on: "
                              "resident='all' runs it on W'")
        return LlmMatrix(name, (N, K), dtype, device, "fp8", q=q, s=sc)
    N, K = q.shape[0], 2 * q.shape[1]
    if N % 16 or K % 256:
        raise PsgHipError(f"resident='quantised': {name} [{N}, {K}] does not fit the MXFP4 nibble-stream kernels of the "
                          "decode steps (N % 16 == 0, K % 256 == 0), and there is no W' to fall back on: "
                          "resident='all' runs it on W'")
    # (a W4_STREAM_AS_FP8 shape streams as nibbles here: its FP8 image would be a second resident copy)
    return LlmMatrix(name, (N, K), dtype, device, "mxfp4", q=q, s=sc, e=e, e_img=ops.mxfp4_exp_image(e))


def _int4_matrix(weights, keys, device, dtype):
    q = torch.cat([weights[k].to(device).view(torch.uint8) for k in keys], 0).contiguous()
    gss = [weights[k + GSCALE_SUFFIX].to(device) for k in keys]
    gzs = [weights[k + GZERO_SUFFIX].to(device) for k in keys]
    N, K = q.shape[0], 2 * q.shape[1]
    B = gss[0].shape[-1]
    if (any(t.dtype != torch.float16 or t.dim() != 2 or t.shape[1] != B for t in gss) or B <= 0 or K % B
            or K // B not in (32, 64, 128)
            or any(z.dtype != torch.uint8 or z.shape != t.shape for z, t in zip(gzs, gss))
            or sum(t.shape[0] for t in gss) != N):
        raise PsgHipError(f"{keys}: group scales must be fp16 and zero points uint8 [{N} rows in all, K / G] with G "
                          f"in (32, 64, 128) and K = {K} (weights.quantize_int4_groups), got "
                          f"{[(t.dtype, tuple(t.shape)) for t in gss + gzs]}")
    gs, gz = torch.cat(gss, 0).contiguous(), torch.cat(gzs, 0).contiguous()
    absf = gs.float().abs()
    if not bool(torch.isfinite(absf).all()) or bool((absf < 2.0 ** -14).any()) or int(gz.max()) > 15:
        raise PsgHipError(f"{keys}: group scales must be finite, normal fp16 numbers and zero points 0..15")
    rec = LlmMatrix(keys[0], (N, K), dtype, device, "int4", w=dequantize_int4_groups(q, gs, gz, dtype).contiguous())
    if (K // B == 128 and K % 256 == 0 and N % 16 == 0
            and (N, K) not in INT4_STREAM_OFF["pair" if dtype == torch.float32 else "single"]):
        rec.int4_img = (ops.int4_q_image(q), ops.int4_group_image(gs, gz))
    return rec


def bf16_valued(t, chunk_elems: int = 1 << 22) -> bool:
    """Is every element of `t` a bf16 value (`t.bfloat16().float() == t`, the test `complete` makes)?  Checked where `t`
    lives, in row chunks of at most `chunk_elems` elements: the temporaries are a chunk's, not the tensor's.  A tensor that
    is already torch.bfloat16 passes without a look."""
    if t.dtype == torch.bfloat16:
        return True
    t2 = t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(1, -1)
    rows = max(1, int(chunk_elems) // max(1, int(t2.shape[1])))
    return all(torch.equal((c := t2[r0:r0 + rows]).bfloat16().float(), c.float()) for r0 in range(0, t2.shape[0], rows))


def load_bf16_matrix(weights, keys, device, dtype, chunk_elems: int = 1 << 22):
    """bf16_value_resident: the record of the (row-concatenated) matrix of `keys` as its bf16 copy ONLY - or the
    first key whose tensor is not a bf16 value (a str: the caller decides what that means for the matrix).  The check and
    the conversion run where a tensor lives, chunk by chunk, and every chunk is copied straight into its rows of the one
    device tensor: the fp32 matrix never reaches `device`, and the load's peak above the record is one chunk."""
    parts = [weights[k] for k in keys]
    K = int(parts[0].shape[1])
    if any(t.dim() != 2 or int(t.shape[1]) != K for t in parts):
        raise PsgHipError(f"{keys}: parts must be 2-D with the same K, got {[tuple(p.shape) for p in parts]}")
    out = torch.empty((sum(int(t.shape[0]) for t in parts), K), device=device, dtype=torch.bfloat16)
    rows, r = max(1, int(chunk_elems) // max(1, K)), 0
    for k, t in zip(keys, parts):
        for r0 in range(0, t.shape[0], rows):
            c = t[r0:r0 + rows]
            b = c.bfloat16()                                   # (`bf16_valued`'s test, on the chunk that is copied anyway)
            if c.dtype != torch.bfloat16 and not torch.equal(b.float(), c.float()):
                return k
            out[r + r0:r + r0 + c.shape[0]].copy_(b)
        r += t.shape[0]
    return LlmMatrix(keys[0], out.shape, dtype, device, wb16=out)


def load_matrix(weights, keys, device, dtype, lean=False, prefill_split=False):
    """The record of the (row-concatenated) matrix of `keys`, W' in `dtype`, with its stream parts when every part is
    quantised (per-row scales commute with the concatenation).  lean: resident='quantised'; prefill_split: an fp32s engine
    (a quantised matrix keeps its two-plane image).  The value copies, split images and the stream follow in `complete`."""
    quant = [is_quantized(weights, k) for k in keys]
    if any(quant) and not all(quant):
        raise PsgHipError(f"{keys}: some parts are FP8-quantised and some are not")
    if lean and quant[0]:
        return _lean_matrix(weights, keys, device, dtype)
    if not quant[0]:
        w = torch.cat([weights[k] for k in keys], 0) if len(keys) > 1 else weights[keys[0]]
        return dense_matrix(keys[0], w.to(device=device, dtype=dtype).contiguous())
    fmts = {quant_format(weights, k) for k in keys}
    if len(fmts) > 1 and "int4" in fmts:
        raise PsgHipError(f"{keys}: some parts are INT4-quantised and some FP8- / MXFP4-quantised")
    if len(fmts) > 1:
        raise PsgHipError(f"{keys}: some parts are FP8-quantised and some MXFP4-quantised")
    if fmts == {"int4"}:
        return _int4_matrix(weights, keys, device, dtype)
    q, sc, e = quant_parts(weights, keys, device)
    two_plane = prefill_split and dtype == torch.float32
    if e is None:
        return LlmMatrix(keys[0], q.shape, dtype, device, "fp8", w=dequantize_fp8_rows(q, sc, dtype).contiguous(), q=q, s=sc,
                         h16=q.view(torch.float8_e4m3fn).to(torch.float16) if two_plane else None)
    N, K = q.shape[0], 2 * q.shape[1]
    rec = LlmMatrix(keys[0], (N, K), dtype, device, "mxfp4", w=dequantize_mxfp4_rows(q, e, sc, dtype).contiguous(), q=q, s=sc,
                    e_img=ops.mxfp4_exp_image(e) if K % 256 == 0 else None,
                    h16=_mxfp4_unscaled(q, e).to(torch.float16) if two_plane else None)
    if (N, K) in W4_STREAM_AS_FP8["pair" if dtype == torch.float32 else "single"]:
        rec.fp8_img = mxfp4_as_fp8_rows(q, e, sc)
    return rec


def complete(layer_mats, lm_head, dtype, prefill_split=False, llm_w16=False, bf16_value_stream=False, batch_split_gemm=False):
    """The passes over the loaded records of the decoder layers and the lm_head, then each record's stream.
    llm_w16 (fp32 engines): are the projection weights fp16 VALUES?  The reference's LLM is the frozen Llama-2-7b-hf checkpoint
    (fp16 on disk, configs/psg/baseline_v4_ov.py:61-65) upcast by from_pretrained (V4:99-100): a matrix whose every element
    round-trips through fp16 keeps an fp16 copy, which the decode steps stream - half the HBM bytes - instead of the fp32
    tensor: exact mode 'fp32' on the same f32 matrix instructions (psg_skinny_gemm_w16, bit-identical), mode 'fp32s' as two
    fp16 products of the split activations (psg_split_gemm_w16, 2^-22).  Per tensor: a fine-tuned lm_head keeps its fp32
    stream alone, anything trained in fp32 fails the check.
    bf16_value_stream: the same question for bf16 - Mistral-7B, Llama-3 and most current Llama-family checkpoints are bf16 on
    disk, and a bf16 value below fp16's subnormal grid (0.02 % of an N(0, 0.02) matrix) fails the round trip above: a matrix
    that is neither quantised nor fp16-valued and round-trips through bf16 keeps a bf16 copy (2 bytes per weight beside the
    fp32 tensor and its split image, which the prompt pass still reads).
    prefill_split: [wh | wl | wh] fp16 + the per-row power of two that undoes the row scaling, per decoder projection that
    is not FP8 / MXFP4 (those run the two-plane prompt pass on `h16`): 3 x 2 bytes per weight next to the fp32 copy the
    decode steps stream (40 GB + 27 GB for Llama-2-7B, of 288 GB).
    batch_split_gemm: a generic fp32 lm_head has no split image (the prompt pass reads one row per pair of it, the decode
    steps of <= 32 rows stream the fp32 tensor), and its SGEMM is the longest launch of a 33..160-row step (288-291 us at
    80 / 160 rows against 146 / 187 on the planes): it keeps the packed [wh | wl] image - 4 bytes per weight, 0.52 GB at
    32000 x 4096."""
    mats = list(layer_mats) + [lm_head]
    for rec in mats:
        # (a quantised matrix has its own stream: never a copy; one resident as its bf16 copy only has nothing to test)
        if dtype != torch.float32 or rec.fmt is not None or rec.w is None:
            continue
        if llm_w16 and torch.equal((h := rec.w.half()).float(), rec.w):
            rec.w16 = h
        elif bf16_value_stream and torch.equal((b := rec.w.bfloat16()).float(), rec.w):
            rec.wb16 = b
    if prefill_split:
        for rec in layer_mats:
            if rec.fmt not in ("fp8", "mxfp4") and rec.w is not None:
                rec.split = ops.split_f16x3(rec.w, weights=True)
    lm = lm_head
    if (batch_split_gemm and lm.fmt is None and lm.w is not None and lm.dtype == torch.float32 and lm.w16 is None
            and lm.shape[0] % 16 == 0
            and lm.shape[1] % 64 == 0):
        img, inv = ops.split_f16x3(lm.w, weights=True)
        lm.packed = (img[:, :2 * lm.shape[1]].contiguous(), inv)
    for rec in mats:
        rec.decide_stream()
