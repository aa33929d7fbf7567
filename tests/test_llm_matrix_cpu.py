"""openpsg_amd/llm_matrix.py on the CPU: what a record holds per format with and without W', that W' is `dequantize_*` bit
for bit, the stream each record gets (precedence and shape conditions), the fp16 / bf16 value copies, and every error of
the loading code with its message.  The split images are a kernel (`ops.split_f16x3(weights=True)`): the GPU tests hold
them."""
import pytest
import torch

from openpsg_amd import llm_matrix as LM
from openpsg_amd import ops
from openpsg_amd import weights as W
from openpsg_amd._lib import PsgHipError

A, B = "model.layers.0.mlp.gate_proj.weight", "model.layers.0.mlp.up_proj.weight"
HEAD = "lm_head.weight"
FP32, BF16 = torch.float32, torch.bfloat16


def _dense(N, K, seed=0):
    return torch.randn(N, K, generator=torch.Generator().manual_seed(seed + N + K)) * 0.05


def _quantised(fmt, shapes, group=128):
    """weights dict of the matrices `shapes` = {key: (N, K)} in `fmt` (None: dense), and the quantised parts per key."""
    w, parts = {}, {}
    for i, (k, (N, K)) in enumerate(shapes.items()):
        d = _dense(N, K, i)
        if fmt is None:
            w[k] = d
        elif fmt == "fp8":
            q, s = parts[k] = W.quantize_fp8_rows(d)
            w.update({k: q, k + W.SCALE_SUFFIX: s})
        elif fmt == "mxfp4":
            q, e, s = parts[k] = W.quantize_mxfp4_rows(d)
            w.update({k: q, k + W.BEXP_SUFFIX: e, k + W.SCALE_SUFFIX: s})
        else:
            q, gs, gz = parts[k] = W.quantize_int4_groups(d, group)
            w.update({k: q, k + W.GSCALE_SUFFIX: gs, k + W.GZERO_SUFFIX: gz})
    return w, parts


def _cat(parts, i):
    return torch.cat([p[i] for p in parts.values()], 0)


def _complete(recs, dtype=FP32, **kw):
    """`complete` over `recs` as decoder matrices beside a small dense lm_head; returns the lm_head's record."""
    head = LM.load_matrix({HEAD: _dense(16, 64)}, (HEAD,), "cpu", dtype)
    LM.complete(recs, head, dtype, **kw)
    return head


def _kind(rec):
    return rec.stream[0] if rec.stream is not None else None


def _owned(rec):
    """Every tensor reachable from a field of the record."""
    out = []
    for name in rec.__slots__:
        v = getattr(rec, name)
        out += [v] if torch.is_tensor(v) else [t for t in v if torch.is_tensor(t)] if isinstance(v, tuple) else []
    return out


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("lean", [False, True])
def test_an_fp8_record(lean, K, dtype):
    w, parts = _quantised("fp8", {A: (32, K), B: (32, K)})
    q, s = _cat(parts, 0), _cat(parts, 1)
    rec = LM.load_matrix(w, (A, B), "cpu", dtype, lean=lean, prefill_split=not lean)
    assert rec.fmt == "fp8" and tuple(rec.shape) == (64, K) and rec.dtype == dtype and rec.numel() == 64 * K
    assert torch.equal(rec.q, q) and torch.equal(rec.s, s) and rec.q.dtype == torch.uint8 and rec.s.dtype == FP32
    assert rec.e is None and rec.e_img is None and rec.fp8_img is None and rec.int4_img is None
    if lean:
        assert rec.w is None and rec.h16 is None and rec.name == "model.layers.0.mlp.gate_proj|up_proj"
    else:
        assert rec.w.dtype == dtype and torch.equal(rec.w, W.dequantize_fp8_rows(q, s, dtype))
        # the two-plane image of an fp32s engine: q exactly, in fp16
        assert (rec.h16 is not None) == (dtype == FP32)
        if dtype == FP32:
            assert rec.h16.dtype == torch.float16 and torch.equal(rec.h16.float() * s[:, None], rec.w)
            assert rec.two_plane() is rec.h16 and rec.column_scale(None) is rec.s
    _complete([rec], dtype, llm_w16=True, bf16_value_stream=True)
    assert rec.stream[0] == "w8" and rec.stream[1][0] is rec.q and rec.stream[1][1] is rec.s
    assert rec.w16 is None and rec.wb16 is None and rec.split is None
    assert {id(t) for t in rec.tensors()} == {id(t) for t in _owned(rec)}
    assert {id(t) for t in rec.quant_tensors()} == {id(rec.q), id(rec.s)}


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("lean", [False, True])
def test_an_mxfp4_record(lean, K, dtype):
    w, parts = _quantised("mxfp4", {A: (32, K), B: (32, K)})
    q, e, s = _cat(parts, 0), _cat(parts, 1), _cat(parts, 2)
    rec = LM.load_matrix(w, (A, B), "cpu", dtype, lean=lean, prefill_split=not lean)
    assert rec.fmt == "mxfp4" and tuple(rec.shape) == (64, K) and tuple(rec.q.shape) == (64, K // 2)
    assert torch.equal(rec.q, q) and torch.equal(rec.s, s) and torch.equal(rec.e_img, ops.mxfp4_exp_image(e))
    assert rec.fp8_img is None and rec.int4_img is None
    if lean:                                                   # the expansion reads the raw exponents: kept without W' only
        assert rec.w is None and rec.h16 is None and torch.equal(rec.e, e)
    else:
        assert rec.e is None and torch.equal(rec.w, W.dequantize_mxfp4_rows(q, e, s, dtype))
        assert (rec.h16 is not None) == (dtype == FP32)
        if dtype == FP32:
            assert torch.equal(rec.h16, W._mxfp4_unscaled(q, e).to(torch.float16)) and torch.equal(rec.h16.float() * s[:, None], rec.w)
    _complete([rec], dtype, llm_w16=True, bf16_value_stream=True)
    assert rec.stream[0] == "w4" and all(a is b for a, b in zip(rec.stream[1], (rec.q, rec.e_img, rec.s)))
    assert rec.w16 is None and rec.wb16 is None
    assert {id(t) for t in rec.tensors()} == {id(t) for t in _owned(rec)}


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("K", [256, 512])
def test_an_int4_record(K, dtype):
    w, parts = _quantised("int4", {A: (32, K), B: (32, K)})
    q, gs, gz = _cat(parts, 0), _cat(parts, 1), _cat(parts, 2)
    rec = LM.load_matrix(w, (A, B), "cpu", dtype, prefill_split=True)
    assert rec.fmt == "int4" and tuple(rec.shape) == (64, K)
    assert torch.equal(rec.w, W.dequantize_int4_groups(q, gs, gz, dtype))
    # only the kernel's images are kept, and no two-plane image: W' is no fp16 value
    assert rec.q is None and rec.s is None and rec.h16 is None
    assert torch.equal(rec.int4_img[0], ops.int4_q_image(q)) and torch.equal(rec.int4_img[1], ops.int4_group_image(gs, gz))
    _complete([rec], dtype, llm_w16=True, bf16_value_stream=True)
    assert rec.stream[0] == "int4" and rec.stream[1] is rec.int4_img and rec.w16 is None and rec.wb16 is None
    assert {id(t) for t in rec.quant_tensors()} == {id(t) for t in rec.int4_img}
    assert {id(t) for t in rec.tensors()} == {id(t) for t in _owned(rec)}


def test_a_dense_record():
    w, _ = _quantised(None, {A: (32, 256), B: (16, 256)})
    for dtype in (FP32, BF16):
        rec = LM.load_matrix(w, (A, B), "cpu", dtype)
        assert rec.fmt is None and tuple(rec.shape) == (48, 256) and torch.equal(rec.w, torch.cat([w[A], w[B]], 0).to(dtype))
        assert not rec.quant_tensors() and [id(t) for t in rec.tensors()] == [id(rec.w)]
        _complete([rec], dtype)
        assert rec.stream is None


def test_an_fp8_image_comes_before_the_nibbles(monkeypatch):
    w, parts = _quantised("mxfp4", {A: (32, 256)})
    monkeypatch.setitem(LM.W4_STREAM_AS_FP8, "pair", frozenset({(32, 256)}))
    rec = LM.load_matrix(w, (A,), "cpu", FP32)
    _complete([rec])
    q8, s8 = W.mxfp4_as_fp8_rows(*parts[A])
    assert _kind(rec) == "w8" and torch.equal(rec.stream[1][0], q8) and torch.equal(rec.stream[1][1], s8)
    assert rec.stream[1] is rec.fp8_img and {id(t) for t in rec.fp8_img} <= {id(t) for t in rec.quant_tensors()}
    assert torch.equal(W.dequantize_fp8_rows(q8, s8), rec.w)                      # the same W' bit for bit
    # the table is per form: a 16-bit engine ("single") is not listed, and a matrix held as bytes only keeps no second copy
    single, lean = LM.load_matrix(w, (A,), "cpu", BF16), LM.load_matrix(w, (A,), "cpu", FP32, lean=True)
    _complete([single, lean], BF16)
    assert _kind(single) == "w4" and single.fp8_img is None and _kind(lean) == "w4" and lean.fp8_img is None


def test_shapes_a_stream_kernel_does_not_take_run_on_the_dense_operand(monkeypatch):
    # MXFP4 with K % 256 != 0: no exponent image, no nibble stream
    w, _ = _quantised("mxfp4", {A: (32, 160)})
    rec = LM.load_matrix(w, (A,), "cpu", FP32)
    _complete([rec], llm_w16=True, bf16_value_stream=True)
    assert rec.e_img is None and rec.stream is None and rec.w is not None
    # FP8 with N % 16 != 0 (and K % 128 != 0)
    for shape in ((24, 256), (32, 192)):
        w, _ = _quantised("fp8", {A: shape})
        rec = LM.load_matrix(w, (A,), "cpu", FP32)
        _complete([rec], llm_w16=True, bf16_value_stream=True)
        assert rec.stream is None and rec.q is not None
    # INT4 in groups of 64; N % 16 != 0; a shape listed in INT4_STREAM_OFF (per form)
    w, _ = _quantised("int4", {A: (32, 256)}, group=64)
    rec = LM.load_matrix(w, (A,), "cpu", FP32)
    _complete([rec])
    assert rec.int4_img is None and rec.stream is None and not rec.quant_tensors()
    w, _ = _quantised("int4", {A: (24, 256)})
    assert LM.load_matrix(w, (A,), "cpu", FP32).int4_img is None
    w, _ = _quantised("int4", {A: (32, 256)})
    monkeypatch.setitem(LM.INT4_STREAM_OFF, "pair", frozenset({(32, 256)}))
    off, on = LM.load_matrix(w, (A,), "cpu", FP32), LM.load_matrix(w, (A,), "cpu", BF16)
    _complete([off])
    _complete([on], BF16)
    assert off.int4_img is None and off.stream is None and _kind(on) == "int4"


def _valued(kind):
    t = _dense(32, 256)
    if kind == "fp16":
        return t.half().float()
    if kind == "bf16":
        t = t.bfloat16().float()
        t[0, 0] = 2.0 ** -30                                   # a bf16 value below fp16's subnormal grid
        return t
    t[0, 0] = 1.0 / 3.0
    return t


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("w16", [False, True])
def test_value_copies(w16, bf16):
    recs = {k: LM.load_matrix({A: _valued(k)}, (A,), "cpu", FP32) for k in ("fp16", "bf16", "third")}
    wq, _ = _quantised("fp8", {B: (32, 256)})
    recs["fp8"] = LM.load_matrix(wq, (B,), "cpu", FP32)
    head = _complete(list(recs.values()), llm_w16=w16, bf16_value_stream=bf16)
    f, b, t, q = (recs[k] for k in ("fp16", "bf16", "third", "fp8"))
    # an fp16 value is a bf16 value only by accident: with the fp16 check off, this one (10 mantissa bits) is none
    assert (f.w16 is not None) == w16 and f.wb16 is None and _kind(f) == ("w16" if w16 else None)
    if w16:
        assert f.w16.dtype == torch.float16 and torch.equal(f.w16.float(), f.w) and f.stream[1] == (f.w16,)
        assert f.two_plane() is f.w16 and torch.equal(f.column_scale(torch.ones), torch.ones(32))
    assert b.w16 is None and (b.wb16 is not None) == bf16 and _kind(b) == ("wb16" if bf16 else None)
    if bf16:
        assert b.wb16.dtype == BF16 and torch.equal(b.wb16.float(), b.w) and b.stream[1] == (b.wb16,)
    assert t.w16 is None and t.wb16 is None and t.stream is None
    assert q.w16 is None and q.wb16 is None and _kind(q) == "w8"
    assert head.w16 is None and head.wb16 is None              # (random fp32 values)
    # the copies belong to the fp32 engines only
    r16 = LM.load_matrix({A: _valued("fp16")}, (A,), "cpu", BF16)
    _complete([r16], BF16, llm_w16=True, bf16_value_stream=True)
    assert r16.w16 is None and r16.wb16 is None and r16.stream is None


def test_the_packed_lm_head_image_is_for_generic_fp32_heads_only():
    """batch_split_gemm keeps a packed image of a generic fp32 lm_head: not of an fp16-valued or quantised one, nor of a shape
    psg_batch_gemm_s does not take (the image itself is a kernel: held by tests/test_gpu_llm_batch_split.py)."""
    wq, _ = _quantised("fp8", {HEAD: (32, 256)})
    for head, dtype in ((LM.load_matrix({HEAD: _valued("fp16")}, (HEAD,), "cpu", FP32), FP32),
                        (LM.load_matrix(wq, (HEAD,), "cpu", FP32), FP32),
                        (LM.load_matrix({HEAD: _dense(24, 256)}, (HEAD,), "cpu", FP32), FP32),
                        (LM.load_matrix({HEAD: _dense(32, 256)}, (HEAD,), "cpu", BF16), BF16)):
        LM.complete([], head, dtype, llm_w16=True, batch_split_gemm=True)
        assert head.packed is None and head.split is None


def _raises(msg, w, keys, **kw):
    with pytest.raises(PsgHipError) as e:
        LM.load_matrix(w, keys, "cpu", kw.pop("dtype", FP32), **kw)
    assert msg in str(e.value), str(e.value)


def test_errors_keep_their_messages():
    f8, _ = _quantised("fp8", {A: (32, 256)})
    m4, _ = _quantised("mxfp4", {B: (32, 256)})
    i4, _ = _quantised("int4", {B: (32, 256)})
    dense, _ = _quantised(None, {B: (32, 256)})
    for lean in (False, True):
        _raises(f"{(A, B)}: some parts are FP8-quantised and some MXFP4-quantised", {**f8, **m4}, (A, B), lean=lean)
        _raises(f"{(A, B)}: some parts are FP8-quantised and some are not", {**f8, **dense}, (A, B), lean=lean)
        bad = dict(f8)
        bad[A + W.SCALE_SUFFIX] = f8[A + W.SCALE_SUFFIX][:31]
        _raises(f"{(A,)}: 31 scales for 32 rows (per-row scales only)", bad, (A,), lean=lean)
        for e in (113, 128):
            bad = dict(m4)
            bad[B + W.BEXP_SUFFIX] = m4[B + W.BEXP_SUFFIX].clone()
            bad[B + W.BEXP_SUFFIX][3, 1] = e
            _raises(f"{(B,)}: block exponents must be uint8 [32, 8] in 114..127 (weights.quantize_mxfp4_rows), got "
                    "torch.uint8 (32, 8)", bad, (B,), lean=lean)
    _raises(f"{(A, B)}: some parts are INT4-quantised and some FP8- / MXFP4-quantised", {**f8, **i4}, (A, B))
    for gs in (2.0 ** -15, float("inf"), float("nan")):        # a subnormal, and what no fp16 scale may be
        bad = dict(i4)
        bad[B + W.GSCALE_SUFFIX] = i4[B + W.GSCALE_SUFFIX].clone()
        bad[B + W.GSCALE_SUFFIX][5, 0] = gs
        _raises(f"{(B,)}: group scales must be finite, normal fp16 numbers and zero points 0..15", bad, (B,))
    bad = dict(i4)
    bad[B + W.GZERO_SUFFIX] = i4[B + W.GZERO_SUFFIX].clone()
    bad[B + W.GZERO_SUFFIX][0, 1] = 16
    _raises(f"{(B,)}: group scales must be finite, normal fp16 numbers and zero points 0..15", bad, (B,))
    bad = dict(i4)
    bad[B + W.GSCALE_SUFFIX] = i4[B + W.GSCALE_SUFFIX].float()
    _raises(f"{(B,)}: group scales must be fp16 and zero points uint8 [32 rows in all, K / G] with G in (32, 64, 128) and "
            "K = 256 (weights.quantize_int4_groups), got ", bad, (B,))
    # resident='quantised': a shape the stream kernels do not take has no W' to fall back on
    name = "model.layers.0.mlp.gate_proj"
    for shape in ((24, 256), (32, 192)):
        w, _ = _quantised("fp8", {A: shape})
        _raises(f"resident='quantised': {name} [{shape[0]}, {shape[1]}] does not fit the FP8 byte-stream kernels of the decode "
                "steps (N % 16 == 0, K % 128 == 0), and there is no W' to fall back on: resident='all' runs it on W'", w, (A,),
                lean=True)
    for shape in ((24, 256), (32, 128)):
        w, _ = _quantised("mxfp4", {A: shape})
        _raises(f"resident='quantised': {name} [{shape[0]}, {shape[1]}] does not fit the MXFP4 nibble-stream kernels of the "
                "decode steps (N % 16 == 0, K % 256 == 0), and there is no W' to fall back on: resident='all' runs it on W'",
                w, (A,), lean=True)
