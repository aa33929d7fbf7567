"""psg_batch_split_gemm_wb16 (psg_batch_gemm_b3.hip): the fp32s decode projections of 33..160 rows over a weight
held as its bf16 copy only, against the float64 product on the SAME values (x as given, W the bf16 values),
`tests.test_gpu_gemm_w8._check`: worst |got - ref| / (|x| @ |W|^T).  Bound 2e-6, the bar of tests/test_gpu_gemm_wb16.py for
the same arithmetic at <= 32 rows (three exact bf16 products, fp32 accumulation).  On top: slots <= 16 and equal to the
plan's, two calls bit-equal, rows independent of their neighbours, rows :M of the 160-row call bit-equal to the M-row call
(the plan is made for 160 rows), nothing written behind the slices, every refusal.

Measured on an MI355X, worst |got - ref| / (|x| @ |W|^T) over every shape, M and plan mode: 1.18e-7 ((12288, 4096), M = 160)."""
import ctypes

import pytest
import torch

from tests.test_gpu_batch_gemm_q import _structure
from tests.test_gpu_gemm_w8 import _check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MODES = (0, 1, 2)
# one partial slab and one K step / slab tails and an odd step count / fewer units than workgroups / many slabs
SMALL = ((16, 64), (272, 192), (48, 4096), (4096, 256))
LLAMA = ((12288, 4096), (4096, 11008))
MS_SMALL = (33, 40, 64, 65, 96, 97, 160)                      # tile tails of one row, full tiles, every tile count, the maximum
MS_LLAMA = (40, 160)
CASES = [(s, MS_SMALL) for s in SMALL] + [(s, MS_LLAMA) for s in LLAMA]
IDS = [f"{n}x{k}" for (n, k), _ in CASES]
BOUND = 2e-6
_W = {}


def _weight(N, K):
    """bf16 [N, K]: rows of magnitudes 2^-12 .. 2^-2 that are no powers of two.  Made once per shape."""
    if (N, K) not in _W:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        w = torch.randn(N, K, generator=g, device=DEV)
        _W[(N, K)] = (w * (torch.exp2(torch.rand(N, generator=g, device=DEV) * 10 - 12) * 0.977)[:, None]).bfloat16()
    return _W[(N, K)]


def _x(N, K):
    """160 fp32 rows of magnitudes 1e-6 .. 1e3 (every 33 consecutive rows span the range), a second set to swap in, and
    `x_of(rows, keep)` -> (the planes of psg_split_b16x3,)."""
    from openpsg_amd import ops
    g = torch.Generator(device=DEV).manual_seed(90 + N + K)
    x = torch.randn(160, K, generator=g, device=DEV) * torch.logspace(-6, 3, 33, device=DEV).repeat(5)[:160, None]
    other = torch.randn(160, K, generator=g, device=DEV)

    def x_of(rows, keep):
        v = x[rows].clone()
        if keep is not None:
            v[keep:] = other[rows][keep:]
        return (ops.split_b16x3(v.contiguous()),)
    return x, x_of


@pytest.mark.parametrize("shape,ms", CASES, ids=IDS)
def test_three_plane_form_is_fp32_grade(shape, ms):
    from openpsg_amd import ops
    N, K = shape
    w = _weight(N, K)
    x, x_of = _x(N, K)
    x3 = x_of(slice(0, 160), None)[0]
    assert torch.equal(x3.float().sum(0), x)                                # (the planes are the rows, exactly)
    for mode in MODES:
        call = lambda a, mode=mode: ops.batch_split_gemm_wb16(a[0], w, mode)       # noqa: E731
        full = _structure(call, x_of, 160)
        assert full.t.shape[1:] == (160, N)
        for M in ms:
            part = full if M == 160 else _structure(call, x_of, M, full)
            assert part.splits == ops.batch_split_gemm_wb16_plan(M, N, K, DEV, mode) <= 16
            _check(f"wb16 M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x[:M].double(), w.double(), BOUND)


def test_unsupported_shapes_are_refused():
    """M in {32, 161}, N = 24, K = 96, misaligned operands: PSG_ERR_UNSUPPORTED before any launch; wrong operand types: the
    binding's own message."""
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError

    def args(M, N, K):
        return torch.zeros((3, M, K), dtype=torch.bfloat16, device=DEV), torch.zeros((N, K), dtype=torch.bfloat16, device=DEV)
    for M, N, K in ((32, 16, 64), (161, 16, 64), (40, 24, 64), (40, 16, 96)):
        x3, w = args(M, N, K)
        with pytest.raises(PsgHipError, match="status"):
            ops.batch_split_gemm_wb16(x3, w)
        with pytest.raises(PsgHipError, match="status"):
            ops.batch_split_gemm_wb16_plan(M, N, K, DEV)
    x3, w = args(40, 16, 64)
    with pytest.raises(PsgHipError, match="status"):
        ops.batch_split_gemm_wb16(x3, w, mode=3)
    flat = torch.zeros(16 * 64 + 4, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(PsgHipError, match="status"):                         # a weight 8 bytes off
        ops.batch_split_gemm_wb16(x3, flat[4:].view(16, 64))
    flat = torch.zeros(3 * 40 * 64 + 4, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(PsgHipError, match="status"):                         # planes 8 bytes off
        ops.batch_split_gemm_wb16(flat[4:].view(3, 40, 64), w)
    for bad_x, bad_w, msg in ((x3.half(), w, "bf16 planes"), (x3[:2], w, "bf16 planes"), (x3, w.float(), "contiguous bf16"),
                              (x3, torch.zeros((16, 128), dtype=torch.bfloat16, device=DEV), "contiguous bf16"),
                              (x3, w.cpu(), "contiguous bf16")):
        with pytest.raises(PsgHipError, match=msg):
            ops.batch_split_gemm_wb16(bad_x, bad_w)
    assert ops.batch_split_gemm_wb16(x3, w).t.shape[1:] == (40, 16)          # (the shape itself is fine)


def test_nothing_is_written_behind_the_slices():
    """The entry called through the ABI with `part` one slice larger than the plan's, filled with a NaN pattern: the tail
    keeps its bits, the slices hold no NaN; a slot count that is not the plan's is refused.  Slab tails (N = 272), every tile
    count, every mode."""
    from openpsg_amd import ops
    N, K = 272, 192
    w = _weight(N, K)
    pat = 0x7FC12345
    for M in (33, 65, 160):
        x3 = ops.split_b16x3(torch.randn(M, K, device=DEV))
        lib, ctx, st = ops._env(x3)
        for mode in MODES:
            s = ctypes.c_int(0)
            ops.check(lib.psg_batch_split_gemm_wb16_plan(ctx, M, N, K, mode, ctypes.byref(s)), "plan")
            buf = torch.full(((s.value + 1) * M * N,), pat, dtype=torch.int32, device=DEV)
            assert lib.psg_batch_split_gemm_wb16(ctx, ops._p(x3), ops._p(w), ops._p(buf), M, N, K, s.value + 1, mode, st) != 0
            assert (buf == pat).all()
            ops.check(lib.psg_batch_split_gemm_wb16(ctx, ops._p(x3), ops._p(w), ops._p(buf), M, N, K, s.value, mode, st), "launch")
            assert (buf[s.value * M * N:] == pat).all(), f"M={M} mode={mode}: wrote behind its slices"
            assert torch.isfinite(buf[:s.value * M * N].view(torch.float32)).all()
