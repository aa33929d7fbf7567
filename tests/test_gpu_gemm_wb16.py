"""psg_split_gemm_wb16 (`-m gpu`): fp32 rows as three bf16 planes against a weight that is a bf16 value, on the
16-bit matrix cores.  Reference: the float64 product x @ w^T.  Bar: 2e-6 * (|x| @ |w|^T), the project's fp32-grade bar
(tests/test_gpu_w16.py).  The operands are exact and every bf16 x bf16 product is exact in fp32, so what is measured is
the fp32 accumulation alone.

Measured (MI355X, worst |got - ref| / (|x| @ |w|^T) over M, the modes and the shapes below; printed per case): 1.9e-7, at
(4096, 256) and M = 5; (12288, 4096) at M = 20: 1.3e-7 - a tenth of the bar."""
import pytest
import torch

from tests.split_b16_ref import bf16_valued, wide_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-6
SHAPES = ((16, 64), (272, 384), (48, 4096), (4096, 256))
_cache = {}


def _case(N, K, M):
    """(x fp32 [M, K], w fp32 of bf16 values [N, K], float64 reference, float64 |x| @ |w|^T): computed once per shape."""
    key = (N, K, M)
    if key not in _cache:
        g = torch.Generator(device=DEV).manual_seed(N + K + M)
        x = wide_rows(M, K, g, DEV)
        w = bf16_valued((N, K), g, device=DEV)
        assert not torch.equal(w.half().float(), w)             # the fp16 round trip fails
        _cache[key] = (x, w, x.double() @ w.double().t(), x.abs().double() @ w.abs().double().t())
    return _cache[key]


def _check(N, K, M, mode):
    from openpsg_amd import ops
    x, w, ref, bound = _case(N, K, M)
    wb = w.bfloat16()
    assert torch.equal(wb.float(), w)
    x3 = ops.split_b16x3(x)
    try:
        slots = ops.split_gemm_wb16_plan(M, N, K, DEV, mode)
    except Exception as exc:                                    # a forced mode may have no plan; the estimate must
        assert mode != 0, exc
        return None
    part = ops.split_gemm_wb16(x3, wb, mode)
    assert tuple(part.t.shape) == (slots, M, N) and 1 <= slots <= 16
    got = part.t.double().sum(0)
    worst = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"split_gemm_wb16 N={N} K={K} M={M} mode={mode}: slots={slots} worst |got - ref| / (|x| @ |w|^T) = {worst:.3e}")
    assert ((got - ref).abs() <= BAR * bound + 1e-300).all(), f"N={N} K={K} M={M} mode={mode}: worst {worst:.3e}"
    assert torch.equal(ops.split_gemm_wb16(x3, wb, mode).t, part.t), "two calls differ"
    return x, x3, wb, part


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("M", [1, 5, 20, 32])
def test_split_gemm_wb16_is_fp32_grade(M, mode):
    from openpsg_amd import ops
    g = torch.Generator(device=DEV).manual_seed(7)
    for N, K in SHAPES:
        res = _check(N, K, M, mode)
        if res is None or M < 5:
            continue
        x, x3, wb, part = res
        x_ = x.clone()                                          # rows :2 are blind to rows 2:
        x_[2:] = torch.randn(M - 2, K, generator=g, device=DEV)
        assert torch.equal(ops.split_gemm_wb16(ops.split_b16x3(x_), wb, mode).t[:, :2], part.t[:, :2])


def test_llama_qkv_shape_at_20_rows():
    assert _check(12288, 4096, 20, 0) is not None


def test_a_slice_behind_part_is_left_untouched():
    from openpsg_amd import ops
    for (N, K), mode in (((272, 384), 0), ((48, 4096), 2), ((4096, 256), 1)):
        x, w, _, _ = _case(N, K, 20)
        x3, wb = ops.split_b16x3(x), w.bfloat16()
        S = ops.split_gemm_wb16_plan(20, N, K, DEV, mode)
        buf = torch.full((S + 1, 20, N), float("nan"), device=DEV)
        part = ops.split_gemm_wb16(x3, wb, mode, part=buf[:S])
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[S]).all()) and not bool(torch.isnan(buf[:S]).any())
        assert torch.equal(part.t, ops.split_gemm_wb16(x3, wb, mode).t)      # unused slots are zero-filled, not left over


def test_the_gemm_refuses_what_it_does_not_take():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    z = lambda *s: torch.zeros(s, device=DEV, dtype=torch.bfloat16)          # noqa: E731
    with pytest.raises(PsgHipError, match=r"status -2.*M=33"):
        ops.split_gemm_wb16(z(3, 33, 64), z(16, 64))
    with pytest.raises(PsgHipError, match=r"status -2.*N=24"):
        ops.split_gemm_wb16(z(3, 4, 64), z(24, 64))
    with pytest.raises(PsgHipError, match=r"status -2.*K=96"):
        ops.split_gemm_wb16(z(3, 4, 96), z(16, 96))
    flat = z(3 * 4 * 64 + 8)
    with pytest.raises(PsgHipError, match=r"status -2.*16-byte aligned"):
        ops.split_gemm_wb16(flat[4:4 + 3 * 4 * 64].view(3, 4, 64), z(16, 64))
    wflat = z(16 * 64 + 8)
    with pytest.raises(PsgHipError, match=r"status -2.*16-byte aligned"):
        ops.split_gemm_wb16(z(3, 4, 64), wflat[4:4 + 16 * 64].view(16, 64))
    S = ops.split_gemm_wb16_plan(4, 16, 64, DEV)
    with pytest.raises(PsgHipError, match="slots = the plan's"):
        ops.split_gemm_wb16(z(3, 4, 64), z(16, 64), part=torch.zeros((S + 1, 4, 16), device=DEV))
    import ctypes
    from openpsg_amd import _lib
    part = torch.full((S + 1, 4, 16), 7.0, device=DEV)          # the library's own check of the slot count
    x3, w = z(3, 4, 64), z(16, 64)
    rc = _lib.load().psg_split_gemm_wb16(_lib.ctx(0), x3.data_ptr(), w.data_ptr(), part.data_ptr(), 4, 16, 64, S + 1, 0,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and "the plan" in _lib.last_error() and bool((part == 7.0).all())
    with pytest.raises(PsgHipError, match="bf16 planes"):
        ops.split_gemm_wb16(z(3, 4, 64).half(), z(16, 64))
