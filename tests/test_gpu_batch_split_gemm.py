"""psg_batch_split_gemm_w16 / _w32 (psg_batch_gemm_s.hip): the fp32s decode projections of 33..160 rows over an
unquantised weight held as fp16 planes, against the float64 product on the SAME fp32 values (x as given; W the fp16 values
of the w16 form, the fp32 weight the image was split from in the w32 form), `tests.test_gpu_gemm_w8._check`: worst
|got - ref| / (|x| @ |W|^T).  Bounds: w16 2e-6, the project's pair-form bar; w32 2.5e-6, the same bar + 2 x 2^-22 for the
weight's split residual and the dropped xl.wl term.  On top: <= 16 slices, two calls bit-equal, rows independent of their
neighbours, and rows :M of the 160-row call bit-equal to the M-row call (the plan is made for 160 rows).

Measured on an MI355X, worst |got - ref| / (|x| @ |W|^T) over every shape, M and plan mode: w16 9.12e-08 (bound 2e-6);
w32 1.31e-07 on the [wh | wl | wh] image and on the packed image alike (bound 2.5e-6)."""
import ctypes

import pytest
import torch

from tests.test_gpu_batch_gemm_q import _structure
from tests.test_gpu_gemm_w8 import _check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MODES = (0, 1, 2)
# one partial slab and one K step / a slab tail and an odd step count / fewer units than workgroups / many slabs
SMALL = ((16, 64), (272, 192), (48, 4096), (4096, 256))
LLAMA = ((12288, 4096), (4096, 11008))
MS_SMALL = (33, 40, 64, 65, 96, 97, 160)                      # tile tails of one row, full tiles, every tile count, the maximum
MS_LLAMA = (40, 160)
CASES = [(s, MS_SMALL) for s in SMALL] + [(s, MS_LLAMA) for s in LLAMA]
IDS = [f"{n}x{k}" for (n, k), _ in CASES]
W16_BOUND, W32_BOUND = 2e-6, 2.5e-6
_W = {}


def _weight(N, K):
    """fp32 [N, K]: rows of magnitudes 2^-12 .. 2^-2 that are no powers of two.  Made once per shape."""
    if (N, K) not in _W:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        w = torch.randn(N, K, generator=g, device=DEV)
        _W[(N, K)] = w * (torch.exp2(torch.rand(N, generator=g, device=DEV) * 10 - 12) * 0.977)[:, None]
    return _W[(N, K)]


def _x(N, K):
    """160 fp32 rows of magnitudes 1e-6 .. 1e3 (every 33 consecutive rows span the range), a second set to swap in, and
    `x_of(rows, keep)` -> the planes of psg_split_f16x2."""
    from openpsg_amd import ops
    g = torch.Generator(device=DEV).manual_seed(90 + N + K)
    x = torch.randn(160, K, generator=g, device=DEV) * torch.logspace(-6, 3, 33, device=DEV).repeat(5)[:160, None]
    other = torch.randn(160, K, generator=g, device=DEV)

    def x_of(rows, keep):
        v = x[rows].clone()
        if keep is not None:
            v[keep:] = other[rows][keep:]
        return ops.split_f16x2(v.contiguous())
    return x, x_of


def _run(name, fn, wargs_of, wd, shape, ms, bound):
    N, K = shape
    x, x_of = _x(N, K)
    for mode in MODES:
        call = lambda a, mode=mode: fn(a[0], a[1], *wargs_of(mode))          # noqa: E731
        full = _structure(call, x_of, 160)
        assert full.t.shape[1:] == (160, N)
        for M in ms:
            part = full if M == 160 else _structure(call, x_of, M, full)
            _check(f"{name} M={M} N={N} K={K} mode={mode}", part.t.sum(0).double(), x[:M].double(), wd, bound)


@pytest.mark.parametrize("shape,ms", CASES, ids=IDS)
def test_w16_form_is_fp32_grade(shape, ms):
    """A weight that IS an fp16 value, with a column scale that is no power of two."""
    from openpsg_amd import ops
    N, K = shape
    w16 = _weight(N, K).half()
    cs = torch.rand(N, device=DEV) + 0.5
    wd = w16.double() * cs.double()[:, None]
    _run("w16", ops.batch_split_gemm_w16, lambda mode: (w16, cs, mode), wd, shape, ms, W16_BOUND)


@pytest.mark.parametrize("layout", ["s_image", "packed"])
@pytest.mark.parametrize("shape,ms", CASES, ids=IDS)
def test_w32_form_is_fp32_grade(shape, ms, layout):
    """A generic fp32 weight through psg_split_f16x3: the prompt pass's [wh | wl | wh] image read in place (stride 3 K,
    lo_off K), and a packed [wh | wl] copy of its first two segments (stride 2 K)."""
    from openpsg_amd import ops
    N, K = shape
    w = _weight(N, K)
    img, inv = ops.split_f16x3(w, weights=True)
    if layout == "packed":
        img = img[:, :2 * K].contiguous()
    _run(f"w32 {layout}", ops.batch_split_gemm_w32, lambda mode: (img, inv, K, None, mode), w.double(), shape, ms, W32_BOUND)


def test_w16_rows_of_another_stride_are_read_in_place():
    """w16 as a column view of a wider tensor (row stride 3 K / K + 8): bit-equal to the contiguous copy's slices."""
    from openpsg_amd import ops
    N, K = 272, 192
    x, x_of = _x(N, K)
    x2, inv = x_of(slice(0, 65), None)
    w16 = _weight(N, K).half()
    ref = ops.batch_split_gemm_w16(x2, inv, w16)                             # (col_scale None: ones)
    _check("w16 contiguous", ref.t.sum(0).double(), x[:65].double(), w16.double(), W16_BOUND)
    for stride, at in ((3 * K, K), (K + 8, 8)):
        big = torch.full((N, stride), 7.0, dtype=torch.float16, device=DEV)
        big[:, at:at + K] = w16
        view = big[:, at:at + K]
        assert not view.is_contiguous()
        assert torch.equal(ops.batch_split_gemm_w16(x2, inv, view).t, ref.t)


def test_w32_lo_off_picks_the_low_plane():
    """The low plane anywhere behind the high one: [wh | pad | wl] with lo_off = K + 64 gives the packed image's slices."""
    from openpsg_amd import ops
    N, K = 48, 256
    x, x_of = _x(N, K)
    x2, inv = x_of(slice(0, 40), None)
    img, ws = ops.split_f16x3(_weight(N, K), weights=True)
    ref = ops.batch_split_gemm_w32(x2, inv, img, ws, K)
    wide = torch.full((N, 2 * K + 64), 3.0, dtype=torch.float16, device=DEV)
    wide[:, :K], wide[:, K + 64:] = img[:, :K], img[:, K:2 * K]
    assert torch.equal(ops.batch_split_gemm_w32(x2, inv, wide, ws, K, lo_off=K + 64).t, ref.t)


def test_unsupported_shapes_are_refused():
    """M in {32, 161}, N = 24, K = 96, a misaligned row: PSG_ERR_UNSUPPORTED before any launch."""
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError

    def args(M, N, K):
        return (torch.zeros((2, M, K), dtype=torch.float16, device=DEV), torch.ones(M, device=DEV),
                torch.zeros((N, 3 * K), dtype=torch.float16, device=DEV), torch.ones(N, device=DEV))
    for M, N, K in ((32, 16, 64), (161, 16, 64), (40, 24, 64), (40, 16, 96)):
        x2, inv, img, s = args(M, N, K)
        with pytest.raises(PsgHipError, match="status"):
            ops.batch_split_gemm_w16(x2, inv, img[:, :K], s)
        with pytest.raises(PsgHipError, match="status"):
            ops.batch_split_gemm_w32(x2, inv, img, s, K)
    x2, inv, img, s = args(40, 16, 64)
    wide = torch.zeros((16, 3 * 64 + 12), dtype=torch.float16, device=DEV)
    for bad16, bad32 in ((wide[:, 4:68], (wide[:, 4:], 64)),                 # the first row 8 bytes off
                         (wide[:, :64], (wide, 68))):                       # rows of 408 bytes / a low plane 8 bytes off
        with pytest.raises(PsgHipError, match="status"):
            ops.batch_split_gemm_w16(x2, inv, bad16, s)
        with pytest.raises(PsgHipError, match="status"):
            ops.batch_split_gemm_w32(x2, inv, bad32[0], s, 64, lo_off=bad32[1])
    assert ops.batch_split_gemm_w16(x2, inv, img[:, :64], s).t.shape[1:] == (40, 16)     # (the shape itself is fine)
    assert ops.batch_split_gemm_w32(x2, inv, img, s, 64).t.shape[1:] == (40, 16)


def test_nothing_is_written_behind_the_slices():
    """Both entries called through the ABI with `part` one slice larger than the plan's, filled with a NaN pattern: the tail
    keeps its bits, the slices hold no NaN.  A slab tail (N = 272), every tile count, every mode."""
    from openpsg_amd import ops
    N, K = 272, 192
    img, ws = ops.split_f16x3(_weight(N, K), weights=True)
    pat = 0x7FC12345
    for M in (33, 65, 160):
        x = torch.randn(M, K, device=DEV)
        x2, inv = ops.split_f16x2(x)
        lib, ctx, st = ops._env(x)
        for mode in MODES:
            for name, wargs in (("batch_split_gemm_w16", (img.data_ptr(), 3 * K, ops._p(ws))),
                                ("batch_split_gemm_w32", (img.data_ptr(), 3 * K, K, ops._p(ws)))):
                s = ctypes.c_int(0)
                ops.check(getattr(lib, f"psg_{name}_plan")(ctx, M, N, K, mode, ctypes.byref(s)), name)
                buf = torch.full(((s.value + 1) * M * N,), pat, dtype=torch.int32, device=DEV)
                ops.check(getattr(lib, f"psg_{name}")(ctx, ops._p(x2), ops._p(inv), *wargs, ops._p(buf), M, N, K, s.value, mode, st),
                          name)
                assert (buf[s.value * M * N:] == pat).all(), f"{name} M={M} mode={mode}: wrote behind its slices"
                assert torch.isfinite(buf[:s.value * M * N].view(torch.float32)).all()
