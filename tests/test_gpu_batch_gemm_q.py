"""psg_batch_gemm_w8 / _w4 and psg_batch_split_gemm_w8 / _w4 (psg_batch_gemm_q.hip): the decode projections of
33..160 rows over an FP8- or MXFP4-quantised weight against the float64 product on the SAME weight values.  Bytes, nibbles
and block scales are widened exactly, so what is checked is the arithmetic of the 32-row families, to their bounds: the
pair form to 2e-6 of |x| @ |W'|^T, the single form (against float64 of the rounded x) to 2^-20 of it.  On top of the
32-row families' structure checks - <= 16 slices, two calls bit-equal, rows independent of their neighbours - a row's
slices must not depend on the row count: rows :M of the 160-row call are bit-equal to the M-row call.

Measured on an MI355X, worst |got - ref| / (|x| @ |W'|^T) over every shape, M and plan mode: pair fp8 2.02e-07, pair mxfp4
2.43e-07 (bound 2e-6); bf16 fp8 1.33e-07, bf16 mxfp4 1.72e-07, fp16 fp8 1.75e-07, fp16 mxfp4 1.92e-07 (bound 2^-20 = 9.54e-07)."""
import ctypes

import pytest
import torch

from tests.test_gpu_gemm_w4 import _weight as _weight4
from tests.test_gpu_gemm_w8 import _check
from tests.test_gpu_gemm_w8 import _weight as _weight8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MODES = (0, 1, 2)
# one partial slab and one K granule / a slab tail and an odd granule count / fewer units than workgroups / many slabs
SMALL8 = ((16, 128), (272, 384), (48, 4096), (4096, 256))
SMALL4 = ((16, 256), (272, 768), (48, 4096), (4096, 256))
LLAMA8 = ((12288, 4096), (4096, 11008), (32000, 4096))
LLAMA4 = ((12288, 4096), (4096, 11008), (32000, 4096))       # (11008 = 43 x 256: the down projection streams as nibbles too)
MS_SMALL = (33, 40, 64, 65, 96, 160)                         # one-row tile tails, full tiles, every tile count, the maximum
MS_LLAMA = (40, 160)
CASES = [("fp8", s, MS_SMALL) for s in SMALL8] + [("fp8", s, MS_LLAMA) for s in LLAMA8] + \
        [("mxfp4", s, MS_SMALL) for s in SMALL4] + [("mxfp4", s, MS_LLAMA) for s in LLAMA4]
IDS = [f"{f}-{n}x{k}" for f, (n, k), _ in CASES]


def _weight(fmt, N, K):
    """(the weight arguments of the ops entry, W' float64): the weights of the 32-row families' tests, made once per shape."""
    if fmt == "fp8":
        q, s, wd = _weight8(N, K)
        return (q, s), wd
    q, ei, s, wd = _weight4(N, K)
    return (q, ei, s), wd


def _structure(call, x_of, M, full=None):
    """<= 16 slices; two calls bit-equal; rows :2 do not see rows 2: replaced; rows :M of the 160-row call bit-equal."""
    part = call(x_of(slice(0, M), None))
    assert part.splits <= 16
    assert torch.equal(call(x_of(slice(0, M), None)).t, part.t)
    assert torch.equal(call(x_of(slice(0, M), 2)).t[:, :2], part.t[:, :2])
    if full is not None:
        assert part.splits == full.splits and torch.equal(part.t, full.t[:, :M]), f"M={M}: rows differ from the 160-row call's"
    return part


@pytest.mark.parametrize("fmt,shape,ms", CASES, ids=IDS)
def test_pair_form_is_fp32_grade(fmt, shape, ms):
    """fp32 rows of magnitudes 1e-6 .. 1e3 (every 33 consecutive rows span the range) through psg_split_f16x2."""
    from openpsg_amd import ops
    N, K = shape
    wargs, wd = _weight(fmt, N, K)
    fn = ops.batch_split_gemm_w8 if fmt == "fp8" else ops.batch_split_gemm_w4
    g = torch.Generator(device=DEV).manual_seed(90 + N + K)
    x = torch.randn(160, K, generator=g, device=DEV) * torch.logspace(-6, 3, 33, device=DEV).repeat(5)[:160, None]
    other = torch.randn(160, K, generator=g, device=DEV)

    def x_of(rows, keep):
        v = x[rows].clone()
        if keep is not None:
            v[keep:] = other[rows][keep:]
        return ops.split_f16x2(v.contiguous())

    for mode in MODES:
        call = lambda a, mode=mode: fn(a[0], a[1], *wargs, mode)
        full = _structure(call, x_of, 160)
        assert full.t.shape[1:] == (160, N)
        for M in ms:
            part = full if M == 160 else _structure(call, x_of, M, full)
            _check(f"pair {fmt} M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x[:M].double(), wd, 2e-6)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("fmt,shape,ms", CASES, ids=IDS)
def test_single_form_is_exact_up_to_fp32_accumulation(fmt, shape, ms, dtype):
    """Against float64 of the ROUNDED x every product is exact: the error is fp32 accumulation alone."""
    from openpsg_amd import ops
    N, K = shape
    wargs, wd = _weight(fmt, N, K)
    fn = ops.batch_gemm_w8 if fmt == "fp8" else ops.batch_gemm_w4
    g = torch.Generator(device=DEV).manual_seed(190 + N + K)
    x = torch.randn(160, K, generator=g, device=DEV).to(dtype)
    other = torch.randn(160, K, generator=g, device=DEV).to(dtype)

    def x_of(rows, keep):
        v = x[rows].clone()
        if keep is not None:
            v[keep:] = other[rows][keep:]
        return v.contiguous()

    for mode in MODES:
        call = lambda a, mode=mode: fn(a, *wargs, mode)
        full = _structure(call, x_of, 160)
        assert full.t.shape[1:] == (160, N)
        for M in ms:
            part = full if M == 160 else _structure(call, x_of, M, full)
            _check(f"{dtype} {fmt} M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x[:M].double(), wd, 2.0 ** -20)


def test_unsupported_shapes_are_refused():
    """M in {32, 161}, N = 24, fp8 K in {64, 192}, mxfp4 K in {128, 384}: PSG_ERR_UNSUPPORTED before any launch; an fp32 x in
    the single form: refused by the wrapper."""
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError

    def args(fmt, M, N, K):
        s = torch.ones(N, device=DEV)
        x = torch.zeros((M, K), dtype=torch.float16, device=DEV)
        x2, inv = torch.zeros((2, M, K), dtype=torch.float16, device=DEV), torch.ones(M, device=DEV)
        if fmt == "fp8":
            return x, x2, inv, (torch.zeros((N, K), dtype=torch.uint8, device=DEV), s)
        return x, x2, inv, (torch.zeros((N, K // 2), dtype=torch.uint8, device=DEV),
                            torch.full((max(K // 256, 1), N, 2, 4), 127, dtype=torch.uint8, device=DEV), s)

    for fmt, single, pair, bad in (("fp8", ops.batch_gemm_w8, ops.batch_split_gemm_w8, ((32, 16, 128), (161, 16, 128), (40, 24, 128),
                                                                                      (40, 16, 64), (40, 16, 192))),
                                   ("mxfp4", ops.batch_gemm_w4, ops.batch_split_gemm_w4, ((32, 16, 256), (161, 16, 256), (40, 24, 256),
                                                                                        (40, 16, 128), (40, 16, 384)))):
        for M, N, K in bad:
            x, x2, inv, w = args(fmt, M, N, K)
            with pytest.raises(PsgHipError, match="status"):
                single(x, *w)
            with pytest.raises(PsgHipError, match="status"):
                pair(x2, inv, *w)
        x, x2, inv, w = args(fmt, 40, 16, 256)
        with pytest.raises(PsgHipError, match="bf16 or fp16"):
            single(x.float(), *w)
        assert single(x, *w).t.shape[1:] == (40, 16)         # (the shape itself is fine)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_nothing_is_written_behind_the_slices(fmt):
    """The four entries called through the ABI with `part` one slice larger than the plan's, filled with a NaN pattern: the
    tail keeps its bits, the slices hold no NaN.  A slab tail (N = 272), every tile count, every mode."""
    from openpsg_amd import ops
    N, K = 272, 768
    wargs, _ = _weight(fmt, N, K)
    pat = 0x7FC12345
    for M in (33, 65, 160):
        x = torch.randn(M, K, device=DEV)
        x2, inv = ops.split_f16x2(x)
        x16 = x.to(torch.bfloat16)
        lib, ctx, st = ops._env(x)
        w = [ops._p(t) for t in wargs]
        for mode in MODES:
            for name, pre, dt in ((f"batch_gemm_w{fmt[-1]}", [ops._p(x16)], (ops._dt(x16),)),
                                  (f"batch_split_gemm_w{fmt[-1]}", [ops._p(x2), ops._p(inv)], ())):
                s = ctypes.c_int(0)
                ops.check(getattr(lib, f"psg_{name}_plan")(ctx, M, N, K, *dt, mode, ctypes.byref(s)), name)
                buf = torch.full(((s.value + 1) * M * N,), pat, dtype=torch.int32, device=DEV)
                ops.check(getattr(lib, f"psg_{name}")(ctx, *pre, *w, ops._p(buf), M, N, K, s.value, *dt, mode, st), name)
                assert (buf[s.value * M * N:] == pat).all(), f"{name} M={M} mode={mode}: wrote behind its slices"
                assert torch.isfinite(buf[:s.value * M * N].view(torch.float32)).all()
