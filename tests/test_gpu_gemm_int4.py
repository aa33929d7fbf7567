"""psg_split_gemm_int4 / psg_skinny_gemm_int4 (psg_gemm_int4.hip): decode-step projections over a group-wise INT4 weight
W'[n, k] = float(gs[n, k // 128]) * (q[n, k] - gz[n, k // 128]) (weights.dequantize_int4_groups) against the float64 product
on the SAME weight values.  The codes are widened to exact integers and each group's sum is scaled in fp32, so what is
checked is the arithmetic of the 2-byte kernels: the pair form to the bound tests/test_gpu_gemm_w4.py holds for it (2e-6 of
|x| @ |W'|^T), the single form to fp32 accumulation (2^-20).  A CPU model of the arithmetic (exact integer weights, fp32 sums
in 16-k steps, one fp32 scale per group) stays below 1e-7, so the reference is well inside both.  The pinned first bytes
(codes 15 and 0 sharing a byte, z = 0 in group 0 and 15 in group 1 of row 0) make a wrong nibble order or a zero point applied
to the wrong group miss either bound by orders of magnitude.

Measured on an MI355X, worst |got - ref| / (|x| @ |W'|^T) over every shape, M and plan mode: pair 8.77e-08 (bound 2e-6),
bf16 4.92e-08 and fp16 5.40e-08 (bound 2^-20 = 9.54e-07); the CPU model 5.03e-08 (pair) and 2.50e-08 (bf16)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MS = (1, 5, 20, 32)
# (16, 256): one unit, N below a wave's 32 rows; (272, 768): odd unit count, ragged last slab; (4096, 11008): 43 units
SHAPES = ((16, 256), (272, 768), (48, 4096), (4096, 512), (4096, 11008))
MODES = (0, 1, 2)
_W = {}


def _weight(N, K, device=DEV):
    """(q_img, g_img, W' float64): codes and zero points uniform over 0..15, scales fp16(2^U(-12, -2) * 0.977) - no powers
    of two - with the first bytes pinned.  Made once per shape."""
    if (N, K, device) not in _W:
        from openpsg_amd import ops
        from openpsg_amd.weights import dequantize_int4_groups
        g = torch.Generator(device=device).manual_seed(1000 * N + K)
        q = torch.randint(0, 256, (N, K // 2), generator=g, device=device, dtype=torch.int32).to(torch.uint8)
        q.view(-1)[:4] = torch.tensor([0x0F, 0xF0, 0x1E, 0xE1], dtype=torch.uint8, device=device)
        gz = torch.randint(0, 16, (N, K // 128), generator=g, device=device, dtype=torch.int32).to(torch.uint8)
        gz[0, 0], gz[0, 1] = 0, 15
        gs = (torch.exp2(torch.rand(N, K // 128, generator=g, device=device) * 10 - 12) * 0.977).to(torch.float16)
        wd = dequantize_int4_groups(q, gs, gz).double()
        assert torch.isfinite(wd).all()
        s0 = gs[0, 0].double()
        assert wd[0, 0] == 15 * s0 and wd[0, 1] == 0 and wd[0, 2] == 0 and wd[0, 3] == 15 * s0     # low nibble = even k
        assert wd[0, 4] == 14 * s0 and wd[0, 5] == s0 and wd[0, 6] == s0 and wd[0, 7] == 14 * s0
        assert wd[0, 128] == (int(q[0, 64]) & 15) * gs[0, 1].double() - 15 * gs[0, 1].double()
        _W[(N, K, device)] = (ops.int4_q_image(q), ops.int4_group_image(gs, gz), wd)
    return _W[(N, K, device)]


def _check(name, got, x64, wd, rel):
    ref = x64 @ wd.t()
    bound = x64.abs() @ wd.abs().t()
    worst = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: worst |got - ref| / (|x| @ |W'|^T) = {worst:.3e} (bound {rel:.3e})")
    assert ((got - ref).abs() <= rel * bound + 1e-300).all(), f"{name}: worst {worst:.3e} > {rel:.3e}"
    return worst


@pytest.mark.parametrize("N,K", SHAPES)
def test_split_gemm_int4_is_fp32_grade(N, K):
    """PAIR form (fp32s): fp32 rows of very different magnitudes through psg_split_f16x2; <= 2e-6 of |x| @ |W'|^T - the
    bound of the 2-byte, FP8 and MXFP4 kernels for the same arithmetic.  <= 16 slices, rows independent of their neighbours,
    two calls bit-equal, every plan mode."""
    from openpsg_amd import ops
    qi, gi, wd = _weight(N, K)
    for M in MS:
        g = torch.Generator(device=DEV).manual_seed(90 + M)
        x = torch.randn(M, K, generator=g, device=DEV) * torch.logspace(-6, 3, M, device=DEV)[:, None]
        x2, inv = ops.split_f16x2(x)
        for mode in MODES:
            part = ops.split_gemm_int4(x2, inv, qi, gi, mode)
            assert part.t.shape[1:] == (M, N) and part.splits <= 16
            _check(f"pair M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x.double(), wd, 2e-6)
            assert torch.equal(ops.split_gemm_int4(x2, inv, qi, gi, mode).t, part.t)
            if M >= 5:
                x_ = x.clone()
                x_[2:] = torch.randn(M - 2, K, generator=g, device=DEV)
                x2b, invb = ops.split_f16x2(x_)
                assert torch.equal(ops.split_gemm_int4(x2b, invb, qi, gi, mode).t[:, :2], part.t[:, :2])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_skinny_gemm_int4_is_exact_up_to_fp32_accumulation(N, K, dtype):
    """Single form (bf16 / fp16 / mixed): against float64 of the ROUNDED x every integer product is exact, so the error is
    fp32 accumulation and the fp32 group scale: <= 2^-20 of |x| @ |W'|^T."""
    from openpsg_amd import ops
    qi, gi, wd = _weight(N, K)
    for M in MS:
        g = torch.Generator(device=DEV).manual_seed(190 + M)
        x = torch.randn(M, K, generator=g, device=DEV).to(dtype)
        for mode in MODES:
            part = ops.skinny_gemm_int4(x, qi, gi, mode)
            assert part.t.shape[1:] == (M, N) and part.splits <= 16
            _check(f"{dtype} M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x.double(), wd, 2.0 ** -20)
            assert torch.equal(ops.skinny_gemm_int4(x, qi, gi, mode).t, part.t)
            if M >= 5:
                x_ = x.clone()
                x_[2:] = torch.randn(M - 2, K, generator=g, device=DEV).to(dtype)
                assert torch.equal(ops.skinny_gemm_int4(x_, qi, gi, mode).t[:, :2], part.t[:, :2])


@pytest.mark.parametrize("N,K", ((16, 256), (272, 768), (48, 4096), (64, 11008)))
def test_cpu_model_of_the_arithmetic_is_far_inside_the_bounds(N, K):
    """The kernel's arithmetic restated on the CPU - fp16 hi / lo planes or bf16 x, exact integers q - z, fp32 sums in 16-k
    steps within a group, acc += float(gs) * group sum in fp32 - stays below 1e-7 of |x| @ |W'|^T: the float64 reference
    on W' is a fair reference for both bounds above."""
    from openpsg_amd.weights import dequantize_int4_groups
    g = torch.Generator().manual_seed(7 * N + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    gz = torch.randint(0, 16, (N, K // 128), generator=g, dtype=torch.int32).to(torch.uint8)
    gs = (torch.exp2(torch.rand(N, K // 128, generator=g) * 10 - 12) * 0.977).to(torch.float16)
    wd = dequantize_int4_groups(q, gs, gz).double()
    ints = (torch.stack((q & 15, q >> 4), dim=2).reshape(N, K).float() - gz.float().repeat_interleave(128, dim=1))
    M = 5

    def model(planes):                                                         # planes: list of [M, K] fp32 holding 16-bit values
        acc = torch.zeros(M, N)
        for grp in range(K // 128):
            for p in planes:
                tmp = torch.zeros(M, N)
                for k0 in range(128 * grp, 128 * grp + 128, 16):
                    tmp = tmp + (p[:, k0:k0 + 16].double() @ ints[:, k0:k0 + 16].double().t()).float()   # exact products
                acc = torch.addcmul(acc.double(), tmp.double(), gs[:, grp].double()[None, :]).float()     # one fused rounding
        return acc
    x = torch.randn(M, K, generator=g) * torch.logspace(-6, 3, M)[:, None]
    amax = x.abs().amax(dim=1, keepdim=True)
    sc = torch.exp2(torch.floor(torch.log2(amax)))                             # a power of two per row: the planes are exact
    xh = (x / sc).half()
    xl = ((x / sc) - xh.float()).half()
    got = model([xh.float(), xl.float()]).double() * sc.double()
    assert _check(f"cpu pair N={N} K={K}", got, x.double(), wd, 1e-7) < 1e-7
    xb = torch.randn(M, K, generator=g).bfloat16()
    assert _check(f"cpu bf16 N={N} K={K}", model([xb.float()]).double(), xb.double(), wd, 1e-7) < 1e-7


def test_unsupported_shapes_and_misaligned_images_are_refused():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError

    def both(M, K, qi, gi, **kw):
        with pytest.raises(PsgHipError, match="status"):
            ops.skinny_gemm_int4(torch.zeros((M, K), dtype=torch.float16, device=DEV), qi, gi, **kw)
        x2 = torch.zeros((2, M, K), dtype=torch.float16, device=DEV)
        with pytest.raises(PsgHipError, match="status"):
            ops.split_gemm_int4(x2, torch.ones(M, device=DEV), qi, gi, **kw)
    for M, N, K in ((33, 16, 256), (4, 16, 128), (4, 16, 384), (4, 24, 256)):
        qi = torch.zeros((N, K // 2), dtype=torch.uint8, device=DEV)
        gi = torch.zeros((max(K // 256, 1), N, 8), dtype=torch.uint8, device=DEV)
        both(M, K, qi, gi)
    N, K = 16, 256
    qi = torch.zeros((N, K // 2), dtype=torch.uint8, device=DEV)
    gi = torch.zeros((1, N, 8), dtype=torch.uint8, device=DEV)
    both(4, K, qi, gi, group=64)                                               # groups of 64 load and run on W', they do not stream
    buf = torch.zeros(N * K // 2 + 16, dtype=torch.uint8, device=DEV)
    both(4, K, buf[1:1 + N * K // 2].view(N, K // 2), gi)                      # a code image one byte off
    buf = torch.zeros(N * 8 + 16, dtype=torch.uint8, device=DEV)
    both(4, K, qi, buf[8:8 + N * 8].view(1, N, 8))                             # a group image eight bytes off
    assert ops.skinny_gemm_int4(torch.zeros((4, K), dtype=torch.float16, device=DEV), qi, gi).t.abs().max() == 0
