"""psg_split_gemm_w4 / psg_skinny_gemm_w4 (psg_gemm_w4.hip): decode-step projections over an MXFP4-quantised weight
W' = fp4(q) * 2^(e - 127) * s[:, None] (q: two E2M1 codes per byte, low nibble = even k; e: one exponent byte per 32 k;
s: fp32 per-row scales; weights.quantize_mxfp4_rows) against the float64 product on the SAME weight values.  Nibbles and
block scales are widened exactly, so what is checked is the arithmetic of the 2-byte kernels: the pair form to the bound
test_split_gemm_w16_is_fp32_grade / test_split_gemm_w8_is_fp32_grade hold, the single form to fp32 accumulation.  The
pinned first bytes (+-6, +-0, +-0.5 pairs, each nibble order) also establish which nibble the conversion instruction
returns first: a swapped pair misses either bound by orders of magnitude.

Measured on an MI355X, worst |got - ref| / (|x| @ |W'|^T) over every shape, M and plan mode: pair 2.39e-07 (bound 2e-6),
bf16 1.76e-07 and fp16 2.31e-07 (bound 2^-20 = 9.54e-07)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MS = (1, 5, 16, 20, 32)
# K % 256 == 0 is the kernel's constraint (one K step = a 128-byte fp4 row piece): 256 is its minimum, 768 its odd multiple
SHAPES = ((16, 256), (272, 768), (48, 4096), (4096, 512), (12288, 4096), (4096, 11008), (32000, 4096))
MODES = (0, 1, 2)
_W = {}


def _weight(N, K):
    """(q uint8 [N, K / 2], e_img, s fp32 [N], W' float64): codes uniform over all 16 (0x8 = -0 included: the kernel takes
    any nibble) with the first bytes pinned to the (+6, -6), (+0, -0), (+0.5, -0.5) pairs and their mirror images, block
    exponents uniform in 114..127, scales spread over 2^-14 .. 2^3 that are no powers of two.  Made once per shape."""
    if (N, K) not in _W:
        from openpsg_amd import ops
        from openpsg_amd.weights import dequantize_mxfp4_rows
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        q = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
        q.view(-1)[:6] = torch.tensor([0xF7, 0x80, 0x91, 0x7F, 0x08, 0x19], dtype=torch.uint8, device=DEV)
        e = torch.randint(114, 128, (N, K // 32), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
        s = torch.exp2(torch.rand(N, generator=g, device=DEV) * 17 - 14) * 0.977
        wd = dequantize_mxfp4_rows(q, e, torch.ones_like(s)).double() * s.double()[:, None]
        assert torch.isfinite(wd).all() and wd.abs().max() <= 6 * 8
        assert wd[0, 0] == 6 * 2.0 ** (int(e[0, 0]) - 127) * s[0].double() and wd[0, 1] == -wd[0, 0]    # low nibble = even k
        _W[(N, K)] = (q, ops.mxfp4_exp_image(e), s, wd)
    return _W[(N, K)]


def _check(name, got, x64, wd, rel):
    ref = x64 @ wd.t()
    bound = x64.abs() @ wd.abs().t()
    worst = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: worst |got - ref| / (|x| @ |W'|^T) = {worst:.3e} (bound {rel:.3e})")
    assert ((got - ref).abs() <= rel * bound + 1e-300).all(), f"{name}: worst {worst:.3e} > {rel:.3e}"


@pytest.mark.parametrize("N,K", SHAPES)
def test_split_gemm_w4_is_fp32_grade(N, K):
    """PAIR form (fp32s): fp32 rows of very different magnitudes through psg_split_f16x2; <= 2e-6 of |x| @ |W'|^T - the
    bound of the 2-byte and FP8 kernels for the same arithmetic.  <= 16 slices, rows independent of their neighbours, two
    calls bit-equal, every plan mode."""
    from openpsg_amd import ops
    q, ei, s, wd = _weight(N, K)
    for M in MS:
        g = torch.Generator(device=DEV).manual_seed(90 + M)
        x = torch.randn(M, K, generator=g, device=DEV) * torch.logspace(-6, 3, M, device=DEV)[:, None]
        x2, inv = ops.split_f16x2(x)
        for mode in MODES:
            part = ops.split_gemm_w4(x2, inv, q, ei, s, mode)
            assert part.t.shape[1:] == (M, N) and part.splits <= 16
            _check(f"pair M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x.double(), wd, 2e-6)
            assert torch.equal(ops.split_gemm_w4(x2, inv, q, ei, s, mode).t, part.t)
            if M >= 5:
                x_ = x.clone()
                x_[2:] = torch.randn(M - 2, K, generator=g, device=DEV)
                x2b, invb = ops.split_f16x2(x_)
                assert torch.equal(ops.split_gemm_w4(x2b, invb, q, ei, s, mode).t[:, :2], part.t[:, :2])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_skinny_gemm_w4_is_exact_up_to_fp32_accumulation(N, K, dtype):
    """Single form (bf16 / fp16 / mixed): against float64 of the ROUNDED x every product is exact, so the error is fp32
    accumulation alone: <= 2^-20 of |x| @ |W'|^T."""
    from openpsg_amd import ops
    q, ei, s, wd = _weight(N, K)
    for M in MS:
        g = torch.Generator(device=DEV).manual_seed(190 + M)
        x = torch.randn(M, K, generator=g, device=DEV).to(dtype)
        for mode in MODES:
            part = ops.skinny_gemm_w4(x, q, ei, s, mode)
            assert part.t.shape[1:] == (M, N) and part.splits <= 16
            _check(f"{dtype} M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x.double(), wd, 2.0 ** -20)
            assert torch.equal(ops.skinny_gemm_w4(x, q, ei, s, mode).t, part.t)
            if M >= 5:
                x_ = x.clone()
                x_[2:] = torch.randn(M - 2, K, generator=g, device=DEV).to(dtype)
                assert torch.equal(ops.skinny_gemm_w4(x_, q, ei, s, mode).t[:, :2], part.t[:, :2])


def test_unsupported_shapes_are_refused():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    for M, N, K in ((33, 16, 256), (4, 16, 128), (4, 16, 384), (4, 24, 256)):
        q = torch.zeros((N, K // 2), dtype=torch.uint8, device=DEV)
        ei = torch.full((max(K // 256, 1), N, 2, 4), 127, dtype=torch.uint8, device=DEV)
        s = torch.ones(N, device=DEV)
        with pytest.raises(PsgHipError, match="status"):
            ops.skinny_gemm_w4(torch.zeros((M, K), dtype=torch.float16, device=DEV), q, ei, s)
        x2 = torch.zeros((2, M, K), dtype=torch.float16, device=DEV)
        with pytest.raises(PsgHipError, match="status"):
            ops.split_gemm_w4(x2, torch.ones(M, device=DEV), q, ei, s)
    # every operand is fetched by 16-byte LDS-DMA: a misaligned image is refused, in both forms
    M, N, K = 4, 16, 256
    q = torch.zeros((N, K // 2), dtype=torch.uint8, device=DEV)
    ei = torch.full((1, N, 2, 4), 127, dtype=torch.uint8, device=DEV)
    s = torch.ones(N, device=DEV)
    x = torch.zeros((M, K), dtype=torch.float16, device=DEV)
    x2 = torch.zeros((2, M, K), dtype=torch.float16, device=DEV)
    buf = torch.zeros(N * K // 2 + 16, dtype=torch.uint8, device=DEV)
    q_off = buf[1:1 + N * K // 2].view(N, K // 2)                               # a nibble image one byte off
    buf = torch.full((N * 8 + 16,), 127, dtype=torch.uint8, device=DEV)
    ei_off = buf[8:8 + N * 8].view(1, N, 2, 4)                                  # an exponent image eight bytes off
    for qi, ee in ((q_off, ei), (q, ei_off)):
        with pytest.raises(PsgHipError, match="status"):
            ops.skinny_gemm_w4(x, qi, ee, s)
        with pytest.raises(PsgHipError, match="status"):
            ops.split_gemm_w4(x2, torch.ones(M, device=DEV), qi, ee, s)
    assert ops.skinny_gemm_w4(x, q, ei, s).t.abs().max() == 0
