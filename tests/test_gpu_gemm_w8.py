"""psg_split_gemm_w8 / psg_skinny_gemm_w8 (psg_gemm_w8.hip): decode-step projections over an FP8-quantised weight
W' = float(q) * s[:, None] (q: OCP e4m3fn bytes, s: fp32 per-row scales; weights.quantize_fp8_rows) against the float64
product on the SAME weight values.  The bytes are widened exactly, so what is checked is the arithmetic of the 2-byte
kernels: the pair form to the bound test_split_gemm_w16_is_fp32_grade holds, the single form to fp32 accumulation."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MS = (1, 5, 16, 20, 32)
# K % 128 == 0 is the kernel's constraint (one K step = a 128-byte fp8 row piece): 128 is its minimum, 384 its odd multiple
SHAPES = ((16, 128), (272, 384), (48, 4096), (4096, 256), (12288, 4096), (4096, 11008), (32000, 4096))
MODES = (0, 1, 2)
_W = {}


def _weight(N, K):
    """(q uint8 [N, K], s fp32 [N], W' float64): every e4m3fn byte but the two NaNs - zeros of both signs, subnormals and
    +-448 included - and scales spread over 2^-14 .. 2^3 that are no powers of two.  Made once per shape."""
    if (N, K) not in _W:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        q = torch.randint(0, 256, (N, K), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
        q = torch.where((q & 0x7F) == 0x7F, q - 1, q)                       # 0x7F / 0xFF (NaN) -> +-448
        q.view(-1)[:6] = torch.tensor([0x7E, 0xFE, 0x00, 0x80, 0x01, 0x87], dtype=torch.uint8, device=DEV)
        s = torch.exp2(torch.rand(N, generator=g, device=DEV) * 17 - 14) * 0.977
        wd = q.view(torch.float8_e4m3fn).double() * s.double()[:, None]
        assert torch.isfinite(wd).all() and wd.abs().max() <= 448 * 8
        _W[(N, K)] = (q, s, wd)
    return _W[(N, K)]


def _check(name, got, x64, wd, rel):
    ref = x64 @ wd.t()
    bound = x64.abs() @ wd.abs().t()
    worst = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: worst |got - ref| / (|x| @ |W'|^T) = {worst:.3e} (bound {rel:.3e})")
    assert ((got - ref).abs() <= rel * bound + 1e-300).all(), f"{name}: worst {worst:.3e} > {rel:.3e}"


@pytest.mark.parametrize("N,K", SHAPES)
def test_split_gemm_w8_is_fp32_grade(N, K):
    """PAIR form (fp32s): fp32 rows of very different magnitudes through psg_split_f16x2; <= 2e-6 of |x| @ |W'|^T - the
    bound of the 2-byte kernel for the same arithmetic.  <= 16 slices, rows independent of their neighbours, two calls
    bit-equal, every plan mode."""
    from openpsg_amd import ops
    q, s, wd = _weight(N, K)
    for M in MS:
        g = torch.Generator(device=DEV).manual_seed(90 + M)
        x = torch.randn(M, K, generator=g, device=DEV) * torch.logspace(-6, 3, M, device=DEV)[:, None]
        x2, inv = ops.split_f16x2(x)
        for mode in MODES:
            part = ops.split_gemm_w8(x2, inv, q, s, mode)
            assert part.t.shape[1:] == (M, N) and part.splits <= 16
            _check(f"pair M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x.double(), wd, 2e-6)
            assert torch.equal(ops.split_gemm_w8(x2, inv, q, s, mode).t, part.t)
            if M >= 5:
                x_ = x.clone()
                x_[2:] = torch.randn(M - 2, K, generator=g, device=DEV)
                x2b, invb = ops.split_f16x2(x_)
                assert torch.equal(ops.split_gemm_w8(x2b, invb, q, s, mode).t[:, :2], part.t[:, :2])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_skinny_gemm_w8_is_exact_up_to_fp32_accumulation(N, K, dtype):
    """Single form (bf16 / fp16 / mixed): against float64 of the ROUNDED x every product is exact, so the error is fp32
    accumulation alone: <= 2^-20 of |x| @ |W'|^T."""
    from openpsg_amd import ops
    q, s, wd = _weight(N, K)
    for M in MS:
        g = torch.Generator(device=DEV).manual_seed(190 + M)
        x = torch.randn(M, K, generator=g, device=DEV).to(dtype)
        for mode in MODES:
            part = ops.skinny_gemm_w8(x, q, s, mode)
            assert part.t.shape[1:] == (M, N) and part.splits <= 16
            _check(f"{dtype} M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x.double(), wd, 2.0 ** -20)
            assert torch.equal(ops.skinny_gemm_w8(x, q, s, mode).t, part.t)
            if M >= 5:
                x_ = x.clone()
                x_[2:] = torch.randn(M - 2, K, generator=g, device=DEV).to(dtype)
                assert torch.equal(ops.skinny_gemm_w8(x_, q, s, mode).t[:, :2], part.t[:, :2])


def test_unsupported_shapes_are_refused():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    s = torch.ones(16, device=DEV)
    for M, N, K in ((33, 16, 128), (4, 16, 64), (4, 16, 192), (4, 24, 128)):
        q = torch.zeros((N, K), dtype=torch.uint8, device=DEV)
        with pytest.raises(PsgHipError, match="status"):
            ops.skinny_gemm_w8(torch.zeros((M, K), dtype=torch.float16, device=DEV), q, s[:N].contiguous() if N <= 16 else
                               torch.ones(N, device=DEV))
    # every operand is fetched by 16-byte LDS-DMA: a misaligned byte image is refused, in both forms
    M, N, K = 4, 16, 128
    q = torch.zeros((N, K), dtype=torch.uint8, device=DEV)
    x = torch.zeros((M, K), dtype=torch.float16, device=DEV)
    x2 = torch.zeros((2, M, K), dtype=torch.float16, device=DEV)
    buf = torch.zeros(N * K + 16, dtype=torch.uint8, device=DEV)
    q_off = buf[1:1 + N * K].view(N, K)                                         # a byte image one byte off
    with pytest.raises(PsgHipError, match="status"):
        ops.skinny_gemm_w8(x, q_off, s)
    with pytest.raises(PsgHipError, match="status"):
        ops.split_gemm_w8(x2, torch.ones(M, device=DEV), q_off, s)
    assert ops.skinny_gemm_w8(x, q, s).t.abs().max() == 0
