"""psg_expand_w8 / psg_expand_w4 (psg_expand.hip): the dense operands an engine with resident='quantised'
rebuilds from the bytes.  Both sides of every comparison are ONE exact widening, ONE fp32 multiply and ONE rounding, so the
bar is equality of the bits (`torch.equal` on the integer views), never a tolerance.  The references run on the same device
tensors: q.view(float8_e4m3fn).half(), _mxfp4_unscaled(q, e).half(), dequantize_fp8_rows, dequantize_mxfp4_rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

NS = (1, 16, 48, 257)
K8 = (32, 256, 1280, 11008)
K4 = (32, 256, 1280)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _scales(N, g):
    """(powers of two 2^-14 .. 2^3, cycled over the rows; no powers of two: amax / 448 of random rows)."""
    pow2 = torch.exp2(((torch.arange(N, device=DEV) * 5) % 18 - 14).float())
    odd = (torch.randn(N, 64, generator=g, device=DEV) * torch.logspace(-3, 1, N, device=DEV)[:, None]).abs().amax(1) / 448.0
    assert not torch.equal(torch.frexp(odd)[0], torch.full_like(odd, 0.5))
    return pow2, odd


def _fp8(N, K):
    """Every finite e4m3fn byte (0x7F / 0xFF, the NaNs, excluded as in tests/test_gpu_gemm_w8.py): zeros of both signs,
    subnormals and +-448 included; all 254 appear in every matrix of >= 254 elements, the first row of a smaller one cycles."""
    g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
    q = torch.randint(0, 256, (N, K), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
    q = torch.where((q & 0x7F) == 0x7F, q - 1, q)
    codes = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8, device=DEV)
    n = min(q.numel(), codes.numel())
    q.view(-1)[:n] = codes[:n]
    return q, g


def _fp4(N, K):
    """Every code except 0x8 (-0: not part of the model) in both nibbles, block exponents covering 114..127."""
    g = torch.Generator(device=DEV).manual_seed(2000 * N + K)
    lo = torch.randint(0, 16, (N, K // 2), generator=g, device=DEV, dtype=torch.int32)
    hi = torch.randint(0, 16, (N, K // 2), generator=g, device=DEV, dtype=torch.int32)
    lo, hi = torch.where(lo == 8, lo - 8, lo), torch.where(hi == 8, hi - 8, hi)
    q = (lo | (hi << 4)).to(torch.uint8)
    codes = torch.tensor([c for c in range(16) if c != 8], dtype=torch.int32, device=DEV)
    n = min(q.numel(), 15)
    q.view(-1)[:n] = (codes[:n] | (codes.flip(0)[:n] << 4)).to(torch.uint8)
    e = (114 + (torch.arange(N * (K // 32), device=DEV) * 3) % 14).to(torch.uint8).view(N, K // 32)
    return q, e, g


def _same_bits(name, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{name}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    a, b = got.contiguous().view(_BITS[got.dtype]), ref.contiguous().view(_BITS[ref.dtype])
    bad = int((a != b).sum())
    assert bad == 0 and torch.equal(a, b), f"{name}: {bad} of {a.numel()} elements differ in their bits"


@pytest.mark.parametrize("K", K8)
@pytest.mark.parametrize("N", NS)
def test_expand_w8_is_bit_exact(N, K):
    from openpsg_amd import ops
    from openpsg_amd.weights import dequantize_fp8_rows
    q, g = _fp8(N, K)
    _same_bits("unscaled fp16", ops.expand_w8(q), q.view(torch.float8_e4m3fn).half())
    for kind, s in zip(("2^n", "amax / 448"), _scales(N, g)):
        for dt in DTYPES:
            _same_bits(f"scaled {dt} ({kind})", ops.expand_w8(q, s, dtype=dt), dequantize_fp8_rows(q, s, dt))


@pytest.mark.parametrize("K", K4)
@pytest.mark.parametrize("N", NS)
def test_expand_w4_is_bit_exact(N, K):
    from openpsg_amd import ops
    from openpsg_amd.weights import _mxfp4_unscaled, dequantize_mxfp4_rows
    q, e, g = _fp4(N, K)
    assert K // 32 * N < 14 or (int(e.min()), int(e.max())) == (114, 127)
    _same_bits("unscaled fp16", ops.expand_w4(q, e), _mxfp4_unscaled(q, e).half())
    for kind, s in zip(("2^n", "amax / 448"), _scales(N, g)):
        for dt in DTYPES:
            _same_bits(f"scaled {dt} ({kind})", ops.expand_w4(q, e, s, dtype=dt), dequantize_mxfp4_rows(q, e, s, dt))


def test_refused_shapes_return_unsupported():
    """K = 48 (no multiple of 32) and a row pointer that is not 16-byte aligned: PSG_ERR_UNSUPPORTED (-2), nothing written."""
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    q = torch.zeros((16, 48), device=DEV, dtype=torch.uint8)
    out = torch.full((16 * 48,), 7.0, device=DEV, dtype=torch.float16)
    with pytest.raises(PsgHipError, match=r"status -2"):
        ops.expand_w8(q, out=out)
    buf = torch.zeros(16 * 64 + 16, device=DEV, dtype=torch.uint8)
    with pytest.raises(PsgHipError, match=r"status -2"):
        ops.expand_w8(buf[8:8 + 16 * 64].view(16, 64), out=out.new_empty(16 * 64))
    e = torch.full((16, 2), 127, device=DEV, dtype=torch.uint8)
    with pytest.raises(PsgHipError, match=r"status -2"):
        ops.expand_w4(buf[8:8 + 16 * 32].view(16, 32), e, out=out.new_empty(16 * 64))
    with pytest.raises(PsgHipError):                                         # (K = 48 has no [N, K / 32] exponents at all)
        ops.expand_w4(torch.zeros((16, 24), device=DEV, dtype=torch.uint8), e[:, :1])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_a_smaller_matrix_leaves_the_tail_of_the_buffer_untouched():
    """The engine's scratch is sized for its largest matrix: a second expansion of a smaller one writes its N * K elements
    and nothing behind them."""
    from openpsg_amd import ops
    from openpsg_amd.weights import dequantize_fp8_rows, dequantize_mxfp4_rows
    q, g = _fp8(257, 1280)
    s = _scales(257, g)[1]
    buf = torch.empty(257 * 1280, device=DEV, dtype=torch.bfloat16)
    big = ops.expand_w8(q, s, out=buf)
    assert big.data_ptr() == buf.data_ptr()
    before = buf.clone()
    q2, e2, g2 = _fp4(48, 256)
    s2 = _scales(48, g2)[1]
    small = ops.expand_w4(q2, e2, s2, out=buf)
    _same_bits("small", small, dequantize_mxfp4_rows(q2, e2, s2, torch.bfloat16))
    _same_bits("tail", buf[48 * 256:], before[48 * 256:])
    _same_bits("big", before.view(257, 1280), dequantize_fp8_rows(q, s, torch.bfloat16))
    half = ops.expand_w8(q[:8], out=buf.view(torch.float16))                 # the unscaled fp16 form in the same bytes:
    assert half.numel() <= 48 * 256                                          # 8 x 1280 elements, inside the head written above
    _same_bits("fp16 head", half, q[:8].view(torch.float8_e4m3fn).half())
    _same_bits("tail after fp16", buf[48 * 256:], before[48 * 256:])
