"""The LLM row kernels and the fp32s split chain against references that are not the kernels themselves (`-m gpu`).

A  psg_split_f16x3 (orders 0 / 1 / 2), psg_split_f16x2, psg_scale_rows_cols: every operation is exact or one IEEE rounding,
   so the reference is a plain torch emulation on the CPU and the comparison is on the raw bits (fp16 viewed as int16: the
   sign of a zero counts).
B  psg_rmsnorm: the residual update bit for bit (it is one or two roundings), the normalised output against float64.
C  psg_silu_mul against float64.
D  psg_rope_kvwrite with rope_pos != tok_pos against HF's half-split rotation in float64.

fp32 outputs are held to a multiple of 2^-24 |ref| stated beside each check; 16-bit outputs to units in the last place of
the output type at the reference value, and - for cases of at least 10^4 elements - at most 0.2 % of the elements may
differ from the reference rounded to the output type.  Where an operation takes its output buffer, the buffer has extra
rows filled with a sentinel and the rows past the end must stay untouched (the split kernels allocate their outputs inside
`openpsg_amd.ops`; for them the shapes are checked instead).  Every case prints its worst error / bound ratio.

Worst err / bound measured on an MI355X: B 0.28 (fp32: 4.5 x 2^-24 |ref|), 0.50 (16-bit: a correctly rounded result);
C 0.45 (fp32: 3.6 x 2^-24 |ref|), 0.50 (16-bit: one unit in the last place of the two allowed); D 0.46 (fp32), 0.50
(16-bit).  Worst share of 16-bit elements that differ from the rounded reference: psg_rmsnorm 1.5e-4, psg_silu_mul 1.1e-5.
"""
import pytest
import torch

from tests.rowops_ref_common import _check, _sentinel, _ulp

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TINY = 2.0 ** -126
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
SHARE = 2e-3                                                        # 16-bit elements that may differ from the rounded reference


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _gen(seed, dev=None):
    return torch.Generator(device=dev or "cpu").manual_seed(seed)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]),
                                                                     b.contiguous().view(BITS[b.dtype]))


def _slice_sum(t):
    """fp32 sum of split-K slices in slice order: ((p0 + p1) + p2) + ..."""
    acc = t[0].clone()
    for s in range(1, t.shape[0]):
        acc = acc + t[s]
    return acc


def _share(got, ref, dtype):
    """share of the elements of a 16-bit output that differ from the float64 reference rounded once to the type"""
    return (got != ref.to(dtype)).double().mean().item()


# ---- A. the split kernels, bit for bit -----------------------------------------------------------------------------
ROW_KINDS = 7


def _split_row(kind, K, g):
    """one fp32 row [K] of the kinds the split has to survive"""
    x = torch.randn(K, generator=g)
    if kind == 0:                                                   # all zero: scale 1 (e = 13), every part +0
        return torch.zeros(K)
    if kind == 1:                                                   # the maximum exactly a power of two (|randn| < 32)
        x[K // 3] = -32.0
        return x
    if kind == 2:                                                   # maximum 3.4e38: scale 2^-114, most of hi underflows to +-0
        x[1::5] *= 1e36
        x[K - 1] = 3.4e38
        return x
    if kind == 3:                                                   # the se clamp: scale 2^126, inv_scale 2^-126
        return x * 1e-37
    if kind == 4:                                                   # twelve decades in one row
        return x * torch.logspace(-12, 0, K)
    return x * (1e30 if kind == 5 else 1e-30)


def _split_cases(rows, K, seed):
    """inputs [rows, K] such that every row kind appears in every (rows, K) case: ceil(7 / rows) inputs"""
    g = _gen(seed)
    for call in range((ROW_KINDS + rows - 1) // rows):
        yield torch.stack([_split_row((call * rows + r) % ROW_KINDS, K, g) for r in range(rows)])


def _split_emul(x):
    """hi, lo (fp16 [rows, K]) and inv_scale of fp32 rows x on the CPU: scale = 2^(13 - floor(log2 max|x|)), its
    exponent field clamped to [1, 253]; s = x scale (fp32, exact up to fp32 underflow); hi = fp16(s); lo = fp16(s - hi)"""
    assert x.device.type == "cpu" and x.dtype == torch.float32
    mx = x.abs().amax(1)
    _, ex = torch.frexp(mx)                                         # mx = m 2^ex, m in [0.5, 1)
    e = torch.where(mx > 0, ex - 1, torch.full_like(ex, 13))
    se = (127 + 13 - e).clamp(1, 253).to(torch.int32)
    scale = (se << 23).view(torch.float32)                          # 2^(se - 127)
    inv_scale = ((254 - se) << 23).view(torch.float32)              # 2^(127 - se)
    assert torch.equal(scale.double(), torch.exp2((se - 127).double()))
    s = x * scale[:, None]
    hi = s.half()
    lo = (s - hi.float()).half()
    assert torch.isfinite(hi.float()).all()
    return hi, lo, inv_scale


def _x3_layout(hi, lo, order):
    rows, K = hi.shape
    if order == 0:
        return torch.cat([hi, hi, lo], 1)
    if order == 1:
        return torch.cat([hi, lo, hi], 1)
    return torch.stack([hi.view(rows, K // 32, 32), lo.view(rows, K // 32, 32)], 2).reshape(rows, 2 * K)


def _run_x3(x, order):
    from openpsg_amd import ops
    return ops.split_f16i2(x) if order == 2 else ops.split_f16x3(x, weights=order == 1)


def _expect_split(name, got, got_inv, want, want_inv):
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and got_inv.dtype == torch.float32
    assert _same_bits(got_inv.cpu(), want_inv), (name, "inv_scale", got_inv.cpu().tolist(), want_inv.tolist())
    g, w = got.cpu().view(torch.int16), want.contiguous().view(torch.int16)
    assert g.shape == w.shape, (name, tuple(g.shape), tuple(w.shape))
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{name}: {bad.shape[0]} of {g.numel()} fp16 words differ from the emulation, first at {i}: "
                             f"got {int(g[i]) & 0xffff:#06x}, want {int(w[i]) & 0xffff:#06x}")


# K <= 4096: the 1024-thread register kernel with NCH = 1 (4: one float4 per row; 4096: every thread one);
# 4100, 11008, 12288: NCH = 3 (12288 without a tail); 12292, 14336, 16384: NCH = 4 (16384 without a tail);
# 16388 (K > 16384) and rows = 65 (rows > 64) at every K: the 256-thread two-pass kernel
@pytest.mark.parametrize("K", [4, 4096, 4100, 11008, 12288, 12292, 14336, 16384, 16388])
@pytest.mark.parametrize("rows", [1, 3, 64, 65])
def test_split_f16x2_equals_the_emulation_bit_for_bit(rows, K):
    from openpsg_amd import ops
    dev = _dev()
    for i, x in enumerate(_split_cases(rows, K, rows * 100003 + K)):
        hi, lo, inv = _split_emul(x)
        out, got_inv = ops.split_f16x2(x.to(dev))
        assert out.shape == (2, rows, K) and got_inv.shape == (rows,)
        _expect_split(f"split_f16x2 rows={rows} K={K} input {i}", out, got_inv, torch.stack([hi, lo]), inv)


@pytest.mark.parametrize("order,K", [(o, k) for o in (0, 1) for k in (4, 36, 1024, 1028, 11008)]
                         + [(2, k) for k in (32, 1024, 11008)])
@pytest.mark.parametrize("rows", [1, 5])
def test_split_f16x3_equals_the_emulation_bit_for_bit(rows, order, K):
    dev = _dev()
    for i, x in enumerate(_split_cases(rows, K, rows * 7001 + K * 3 + order)):
        hi, lo, inv = _split_emul(x)
        out, got_inv = _run_x3(x.to(dev), order)
        assert out.shape == (rows, (2 if order == 2 else 3) * K) and got_inv.shape == (rows,)
        _expect_split(f"split_f16x3 order={order} rows={rows} K={K} input {i}", out, got_inv, _x3_layout(hi, lo, order), inv)


# (3, 4100): split_f16x2's register kernel (NCH = 3, tail); (65, 4100): its 256-thread kernel
@pytest.mark.parametrize("kernel,rows,K", [("x2", 3, 4100), ("x2", 65, 4100), ("x3-0", 5, 1028), ("x3-1", 5, 1028),
                                           ("x3-2", 5, 1024)])
def test_split_kernels_read_only_k_columns_of_a_strided_row(kernel, rows, K):
    """x = wide[:, :K] of a [rows, K + 8] tensor (row_stride > K) whose last 8 columns hold 1e30: they are outside the row,
    must not enter its maximum and must not be split."""
    from openpsg_amd import ops
    dev = _dev()
    for i, x in enumerate(_split_cases(rows, K, rows * 31 + K)):
        wide = torch.full((rows, K + 8), 1e30)
        wide[:, :K] = x
        xd = wide.to(dev)[:, :K]
        assert xd.stride(0) == K + 8
        hi, lo, inv = _split_emul(x)
        if kernel == "x2":
            out, got_inv = ops.split_f16x2(xd)
            want = torch.stack([hi, lo])
        else:
            order = int(kernel[-1])
            out, got_inv = _run_x3(xd, order)
            want = _x3_layout(hi, lo, order)
        _expect_split(f"strided {kernel} rows={rows} K={K} input {i}", out, got_inv, want, inv)


def test_split_f16x3_order_2_refuses_k_36():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    with pytest.raises((PsgHipError, AssertionError)):
        ops.split_f16i2(torch.ones(2, 36, device=_dev()))
    torch.cuda.synchronize()


# (1030, 4096): 1 054 720 float4s > 4096 blocks x 256 threads: the grid-stride loop takes a second pass
@pytest.mark.parametrize("rows,N", [(1, 4), (3, 12), (1030, 4096)])
def test_scale_rows_cols_equals_the_fp32_expression_bit_for_bit(rows, N):
    """y * (rs[:, None] * cs[None, :]) in fp32 - the kernel's own order of the two products - with scales that are no
    powers of two, so that both roundings happen."""
    from openpsg_amd import ops
    dev = _dev()
    g = _gen(rows * 17 + N)
    y = torch.randn(rows, N, generator=g) * torch.logspace(-3, 3, N)[None]
    rs = 0.5 + torch.rand(rows, generator=g)
    cs = (0.5 + torch.rand(N, generator=g)) * 1e-3
    want = y * (rs[:, None] * cs[None, :])
    buf, pristine = _sentinel(rows, N, torch.float32, dev)
    buf[:rows] = y.to(dev)
    ops.scale_rows_cols(buf[:rows], rs.to(dev), cs.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(buf[rows:], pristine[rows:]), "rows past the end were written"
    assert _same_bits(buf[:rows].cpu(), want), f"{(buf[:rows].cpu() != want).sum().item()} of {want.numel()} elements differ"


# ---- B. psg_rmsnorm ------------------------------------------------------------------------------------------------
# (activation type T, residual type R): R = T, or fp32 under 16-bit rows (the mixed mode)
RMS_VARIANTS = [("fp32", "fp32"), ("bf16", "bf16"), ("fp16", "fp16"), ("bf16", "fp32"), ("fp16", "fp32")]
RMS_IDS = ["fp32", "bf16", "fp16", "bf16-res32", "fp16-res32"]


def _rms_inputs(rows, hidden, T, R, seed, dev):
    """residual rows as stored (randn * 3; row 1 all zero, row 2 at 1e4, row 3 at 1e-4 where the case has them), the
    weight, a dense delta of type T and 16 fp32 slices; the zero row's deltas are zero, so that it stays zero"""
    g = _gen(seed, dev)
    resid = torch.randn(rows, hidden, generator=g, device=dev) * 3
    if rows > 2:
        resid[2] = (torch.randn(hidden, generator=g, device=dev) * 1e4).clamp(-6e4, 6e4)       # finite in fp16
    if rows > 3:
        resid[3] = torch.randn(hidden, generator=g, device=dev) * 1e-4
    w = 1 + 0.1 * torch.randn(hidden, generator=g, device=dev)
    dense = torch.randn(rows, hidden, generator=g, device=dev)
    parts = torch.randn(16, rows, hidden, generator=g, device=dev)
    if rows > 1:
        resid[1] = 0
        dense[1] = 0
        parts[:, 1] = 0
    return resid.to(R), w, dense.to(T), parts


def _rms_case(name, resid0, delta, w, eps, T, dev):
    """one psg_rmsnorm call on sentinel-extended buffers against the references; -> (err / bound, differing share)"""
    from openpsg_amd import ops
    rows, hidden = resid0.shape
    R = resid0.dtype
    rbuf, rprist = _sentinel(rows, hidden, R, dev)
    rbuf[:rows] = resid0
    obuf, oprist = _sentinel(rows, hidden, T, dev)
    ops.rmsnorm(rbuf[:rows], delta, w, eps, obuf[:rows])
    torch.cuda.synchronize()
    assert torch.equal(rbuf[rows:], rprist[rows:]) and torch.equal(obuf[rows:], oprist[rows:]), \
        f"{name}: rows past the end were written"
    # the residual update: d = the dense delta, or the slice-order fp32 sum rounded to T; resid = rnd_R(resid + d), the
    # sum in fp32; without a delta the stream is not touched
    if delta is None:
        v = resid0
    else:
        d = _slice_sum(delta.t).to(T).float() if isinstance(delta, ops.Partials) else delta.float()
        v = (resid0.float() + d).to(R)
    assert _same_bits(rbuf[:rows], v), f"{name}: {(rbuf[:rows] != v).sum().item()} residual elements differ from rnd(resid + d)"
    v64, w64 = v.double(), w.double()
    ref = w64 * v64 / torch.sqrt((v64 * v64).mean(-1, keepdim=True) + eps)
    # fp32: 16 x 2^-24 |ref| (a plain fp32 torch evaluation measures <= 3.9 x 2^-24 at hidden 4 .. 8192; the kernel's tree
    # - at most 32 serial terms + 6 + 16 - has a worst case near 40 x 2^-24 and a typical error like torch's); 16-bit: one
    # unit in the last place of T on top
    bound = 16 * EPS * ref.abs() + TINY + _ulp(ref, T)
    got = obuf[:rows]
    ratio = _check(name, got, ref, bound)
    if rows > 1:
        assert not got[1].any(), f"{name}: the all-zero row did not stay zero"
    share = 0.0
    if T != torch.float32 and got.numel() >= 10 ** 4:
        share = _share(got, ref, T)
        assert share <= SHARE, f"{name}: {share:.2e} of the elements differ from the reference rounded once"
    return ratio, share


def _rms_deltas(T, dense, parts):
    from openpsg_amd import ops
    return [("none", None), ("dense", dense)] + [(f"S={S}", ops.Partials(parts[:S].contiguous())) for S in (1, 3, 16)]


# threads per row and chunks per thread (NCH) of rmsnorm_kernel: 1024 threads for <= 64 rows of >= 4096 columns, else 256
RMS_BLOCK_SHAPES = [(1, 4),         # 256 threads, NCH 1, one thread with work
                    (3, 100),       # 256, NCH 1, a tail (25 of 256 threads)
                    (5, 1024),      # 256, NCH 1, full
                    (5, 1028),      # 256, NCH 2, one thread in the second chunk
                    (2, 4092),      # 256, NCH 4, tail (hidden < 4096 keeps 256 threads)
                    (64, 4096),     # 1024 threads, NCH 1
                    (65, 4096),     # 256 threads, NCH 4 (fp32; 16-bit without slices: the wave-per-row kernel)
                    (7, 4100),      # 1024, NCH 2, one thread in the second chunk
                    (3, 5120),      # 1024, NCH 2, tail
                    (20, 8192),     # 1024, NCH 2, full
                    (65, 8192),     # 256, NCH 8
                    (2, 8188)]      # 1024, NCH 2, tail of one float4


@pytest.mark.parametrize("rows,hidden", RMS_BLOCK_SHAPES)
@pytest.mark.parametrize("dt,rdt", RMS_VARIANTS, ids=RMS_IDS)
def test_rmsnorm_block_kernel_vs_float64(dt, rdt, rows, hidden):
    """rmsnorm_kernel<T, NCH, R> at every thread count / chunk count / tail it is launched with, without a delta, with a
    dense one and with 1, 3 and 16 split-K slices, eps 1e-5 and 1e-6.  (65, 4096) in 16 bits without slices is the
    wave-per-row kernel's; with option ln_half_wave = 0 it is the block kernel's, so it runs both ways.  Measured: fp32
    outputs reach 0.28 of the bound (4.5 x 2^-24 |ref|), 16-bit outputs 0.50 (half a unit in the last place)."""
    from openpsg_amd import _lib
    dev, T, R = _dev(), DTYPES[dt], DTYPES[rdt]
    resid0, w, dense, parts = _rms_inputs(rows, hidden, T, R, rows * 131 + hidden + len(dt) + len(rdt), dev)
    worst = share = 0.0
    wave_rows = (0, 1) if (rows > 64 and T != torch.float32 and hidden == 4096) else (1,)
    try:
        for hw in wave_rows:
            _lib.set_option(0, "ln_half_wave", hw)
            for eps in (1e-5, 1e-6):
                for dname, delta in _rms_deltas(T, dense, parts):
                    r, s = _rms_case(f"rmsnorm {dt}/{rdt} ({rows}, {hidden}) {dname} eps={eps} hw={hw}", resid0, delta, w, eps,
                                     T, dev)
                    worst, share = max(worst, r), max(share, s)
    finally:
        _lib.set_option(0, "ln_half_wave", 1)
    print(f"B rmsnorm block {dt}/{rdt} ({rows}, {hidden}): max err/bound {worst:.3f}, differing share {share:.2e}")


@pytest.fixture(params=[1, 0], ids=["wave-per-row", "block"])
def rows16_kernel(request):
    """option ln_half_wave = 1 (default): 16-bit prompt-pass rows take rmsnorm_rows16_kernel; 0: the block kernel"""
    from openpsg_amd import _lib
    _lib.set_option(0, "ln_half_wave", request.param)
    yield request.param
    _lib.set_option(0, "ln_half_wave", 1)


# rows 65 and 67 leave the last 4-row workgroup with 1 and 3 rows; hidden 512 / 1024 / 4096: NCH 1 / 2 / 8
@pytest.mark.parametrize("hidden", [512, 1024, 4096])
@pytest.mark.parametrize("rows", [65, 67, 200])
@pytest.mark.parametrize("dt,rdt", RMS_VARIANTS[1:], ids=RMS_IDS[1:])
def test_rmsnorm_wave_per_row_kernel_vs_float64(rows16_kernel, dt, rdt, rows, hidden):
    """rmsnorm_rows16_kernel<E, NCH, R32> (more than 64 16-bit rows of 512 / 1024 / 4096 columns, no slices), residual
    stream 16-bit and fp32, without and with a dense delta; the same cases through the block kernel; and rows = 200 with
    three slices, which the block kernel takes under either option."""
    from openpsg_amd import ops
    dev, T, R = _dev(), DTYPES[dt], DTYPES[rdt]
    resid0, w, dense, parts = _rms_inputs(rows, hidden, T, R, rows * 137 + hidden + len(dt) + len(rdt), dev)
    cases = [("none", None, 1e-5), ("dense", dense, 1e-6)]
    if rows == 200:
        cases.append(("S=3", ops.Partials(parts[:3].contiguous()), 1e-5))
    worst = share = 0.0
    for dname, delta, eps in cases:
        r, s = _rms_case(f"rmsnorm rows16 {dt}/{rdt} ({rows}, {hidden}) {dname} hw={rows16_kernel}", resid0, delta, w, eps, T,
                         dev)
        worst, share = max(worst, r), max(share, s)
    print(f"B rmsnorm rows16 {dt}/{rdt} ({rows}, {hidden}) ln_half_wave={rows16_kernel}: max err/bound {worst:.3f}, "
          f"differing share {share:.2e}")


def test_rmsnorm_refusals_leave_the_buffers_untouched():
    """hidden 6 (no multiple of 4) and 8196 (> 8192): PSG_ERR_UNSUPPORTED (-2); 17 slices (> PSG_MAX_SPLITS): -2; a
    residual type that is neither the activation type nor fp32: refused before the launch."""
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    dev = _dev()

    def refused(resid_dt, out_dt, rows, hidden, S, match):
        rbuf, rprist = _sentinel(rows, hidden, resid_dt, dev)
        obuf, oprist = _sentinel(rows, hidden, out_dt, dev)
        delta = ops.Partials(torch.ones(S, rows, hidden, device=dev)) if S else None
        with pytest.raises(PsgHipError, match=match):
            ops.rmsnorm(rbuf[:rows], delta, torch.ones(hidden, device=dev), 1e-5, obuf[:rows])
        torch.cuda.synchronize()
        assert torch.equal(rbuf, rprist) and torch.equal(obuf, oprist)

    for dt in DTYPES.values():
        refused(dt, dt, 3, 6, 0, r"status -2")
        refused(dt, dt, 3, 8196, 0, r"status -2")
        refused(dt, dt, 3, 8, 17, r"status -2")
    refused(torch.bfloat16, torch.float16, 3, 8, 0, "residual stream must be")
    refused(torch.float16, torch.bfloat16, 3, 8, 0, "residual stream must be")
    refused(torch.bfloat16, torch.float32, 3, 8, 0, "residual stream must be")


# ---- C. psg_silu_mul -----------------------------------------------------------------------------------------------
def _silu_inputs(rows, inter, S, T, seed, dev):
    """gate | up rows [rows, 2 inter]: gates uniform in [-80, 80] with a 0.0 and a -0.0, up = randn * 3; as a tensor of
    type T (S = 0) or as S fp32 slices whose slice-order sum they are.  -> (kernel input, gate and up as the kernel sees
    them, float64)"""
    from openpsg_amd import ops
    g = _gen(seed, dev)
    gu = torch.empty(rows, 2 * inter, device=dev)
    gu[:, :inter] = torch.rand(rows, inter, generator=g, device=dev) * 160 - 80
    gu[:, inter:] = torch.randn(rows, inter, generator=g, device=dev) * 3
    gu[0, 0], gu[0, 1] = 0.0, -0.0
    if S == 0:
        x = gu.to(T)
        seen = x
    else:
        t = torch.randn(S, rows, 2 * inter, generator=g, device=dev) * 10
        t[S - 1] = gu if S == 1 else gu - _slice_sum(t[:S - 1])
        x = ops.Partials(t)
        seen = _slice_sum(t).to(T)                                  # summed in fp32 in slice order, rounded to T
    seen = seen.double()
    return x, seen[:, :inter], seen[:, inter:]


def _silu_case(name, rows, inter, S, T, seed, dev):
    from openpsg_amd import ops
    x, g64, u64 = _silu_inputs(rows, inter, S, T, seed, dev)
    assert g64.abs().max().item() <= 80.5
    obuf, oprist = _sentinel(rows, inter, T, dev)
    ops.silu_mul(x, obuf[:rows])
    torch.cuda.synchronize()
    assert torch.equal(obuf[rows:], oprist[rows:]), f"{name}: rows past the end were written"
    got = obuf[:rows]
    silu = g64 / (1 + torch.exp(-g64))
    if T == torch.float32:
        # 8 x 2^-24 |ref|: expf within an ulp (2 x 2^-24), then an add, a division and a product of half an ulp each;
        # a plain fp32 torch evaluation measures 3.2 x 2^-24
        ref = silu * u64
        return _check(name, got, ref, 8 * EPS * ref.abs() + TINY), 0.0
    # 16-bit, as the kernel documents (HF rounds act_fn(gate) before the product): silu rounded to T, multiplied, rounded
    # again; two units in the last place of slack for the fp32 evaluation of silu under the first rounding
    ref = (silu.to(T).double() * u64).to(T).double()
    ratio = _check(name, got, ref, 2 * _ulp(ref, T))
    share = 0.0
    if got.numel() >= 10 ** 4:
        share = _share(got, ref, T)
        assert share <= SHARE, f"{name}: {share:.2e} of the elements differ from the twice-rounded reference"
    return ratio, share


# every fp32 shape runs silu_mul_kernel<float>; (400, 11008): 1 100 800 float4s > 4096 blocks x 256 threads, so the
# grid-stride loop takes a second pass
@pytest.mark.parametrize("S", [0, 1, 3, 16])
@pytest.mark.parametrize("rows,inter", [(1, 4), (3, 12), (7, 11008), (20, 14336), (400, 11008)])
def test_silu_mul_fp32_vs_float64(rows, inter, S):
    dev = _dev()
    ratio, _ = _silu_case(f"silu_mul fp32 ({rows}, {inter}) S={S}", rows, inter, S, torch.float32, rows * 3 + inter + S, dev)
    print(f"C silu_mul fp32 ({rows}, {inter}) S={S}: max err/bound {ratio:.3f}")


@pytest.mark.parametrize("rows,inter,S", [(7, 688, 0),       # <= 64 rows: silu_mul_kernel<T>, dense 16-bit input
                                          (7, 688, 4),       # silu_mul_kernel<T>, slices rounded to T
                                          (20, 688, 0),      # the two above with >= 10^4 elements, so that the share of
                                          (20, 688, 4),      # differing elements is held on silu_mul_kernel<T> as well
                                          (65, 12, 0),       # inter % 8 != 0 keeps silu_mul_kernel<T> above 64 rows
                                          (65, 172, 0),      # ... with >= 10^4 elements
                                          (65, 8, 0),        # silu_mul_rows_bf16_kernel, one thread per row
                                          (65, 2056, 0),     # ... two column blocks, the second with one thread
                                          (32773, 8, 0)])    # ... gridDim.y = 32768: rows 32768 .. 32772 by the row loop
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_silu_mul_16bit_vs_float64(dt, rows, inter, S):
    dev = _dev()
    ratio, share = _silu_case(f"silu_mul {dt} ({rows}, {inter}) S={S}", rows, inter, S, DTYPES[dt],
                              rows * 5 + inter + S + len(dt), dev)
    print(f"C silu_mul {dt} ({rows}, {inter}) S={S}: max err/bound {ratio:.3f}, differing share {share:.2e}")


# ---- D. psg_rope_kvwrite -------------------------------------------------------------------------------------------
ROPE_PAIRS, ROPE_SEQ, ROPE_CTX, ROPE_TABLE = 5, 9, 40, 64
ROPE_LENGTHS = [9, 4, 9, 1, 6]


def _rope_rows(dev):
    """5 pairs x 9 rows, left-padded as in the training forward: the first 9 - length rows of a pair are padding
    (tok_pos -1), the others fill cache slots 0 .. length - 1 and carry rotary position = their place in the padded row"""
    pair = torch.arange(ROPE_PAIRS, dtype=torch.int32)[:, None].expand(-1, ROPE_SEQ).reshape(-1).contiguous()
    tok_pos = torch.full((ROPE_PAIRS, ROPE_SEQ), -1, dtype=torch.int32)
    rope_pos = torch.zeros(ROPE_PAIRS, ROPE_SEQ, dtype=torch.int32)
    for p, n in enumerate(ROPE_LENGTHS):
        tok_pos[p, ROPE_SEQ - n:] = torch.arange(n, dtype=torch.int32)
        rope_pos[p, ROPE_SEQ - n:] = tok_pos[p, ROPE_SEQ - n:] + (ROPE_SEQ - n)
    return pair.to(dev), tok_pos.reshape(-1).to(dev), rope_pos.reshape(-1).to(dev)


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "S=3"])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_rope_kvwrite_with_rope_pos_vs_float64(dt, heads, sliced):
    """Multi-head psg_rope_kvwrite: q and k rotated by rope_pos (which differs from the cache slot tok_pos for the three
    pairs shorter than 9), k and v written at slot tok_pos of (pair, head); then the same call with rope_pos = None
    (rotary position = slot).  fp32: 4 x 2^-24 (|x1 cos| + |x2 sin|) - a rounded product and one fused multiply-add;
    16-bit: one unit in the last place on top.  v is copied: bit-equal to the input (or its slice-order sum rounded to T)."""
    from openpsg_amd import ops
    dev, T = _dev(), DTYPES[dt]
    hidden, rows = heads * 128, ROPE_PAIRS * ROPE_SEQ
    g = _gen(heads * 10 + len(dt) + int(sliced), dev)
    pair, tok_pos, rope_pos = _rope_rows(dev)
    assert int((rope_pos != tok_pos)[tok_pos >= 0].sum()) > 0
    inv_f = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
    ang = torch.arange(ROPE_TABLE, dtype=torch.float32)[:, None] * inv_f[None, :]
    rope = (ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev))
    if sliced:
        t = torch.randn(3, rows, 3 * hidden, generator=g, device=dev)
        qkv, x = ops.Partials(t), _slice_sum(t).to(T)
    else:
        qkv = x = torch.randn(rows, 3 * hidden, generator=g, device=dev).to(T)
    x64 = x.double().view(rows, 3, heads, 2, 64)                   # [row][q | k | v][head][half][64]
    valid = tok_pos >= 0
    vp, vs = pair[valid].long(), tok_pos[valid].long()
    worst = 0.0
    for rp in (rope_pos, None):
        pos = (tok_pos if rp is None else rp).long().clamp_min(0)
        cs, sn = rope[0][pos].double()[:, None, None, :], rope[1][pos].double()[:, None, None, :]   # [row][1][1][64]
        x1, x2 = x64[:, :2, :, 0], x64[:, :2, :, 1]                 # q and k: [row][2][head][64]
        ref = torch.stack([x1 * cs - x2 * sn, x2 * cs + x1 * sn], 3)                               # [row][2][head][half][64]
        mag = torch.stack([(x1 * cs).abs() + (x2 * sn).abs(), (x2 * cs).abs() + (x1 * sn).abs()], 3)
        bound = 4 * EPS * mag + _ulp(ref, T)
        qbuf, qprist = _sentinel(rows, hidden, T, dev)
        kc = torch.full((ROPE_PAIRS, heads, ROPE_CTX, 128), -1234.5, device=dev, dtype=T)
        vc = kc.clone()
        ops.rope_kvwrite(qkv, pair, tok_pos, rope, heads, 128, ROPE_CTX, qbuf[:rows], kc, vc, rope_pos=rp)
        torch.cuda.synchronize()
        name = f"rope_kvwrite {dt} heads={heads} sliced={sliced} rope_pos={'given' if rp is not None else 'None'}"
        assert torch.equal(qbuf[rows:], qprist[rows:]), f"{name}: rows past the end of q_out were written"
        assert torch.equal(qbuf[:rows][~valid], qprist[:rows][~valid]), f"{name}: padding rows of q_out were written"
        worst = max(worst, _check(name + " q", qbuf[:rows][valid].view(-1, heads, 2, 64), ref[valid, 0], bound[valid, 0]))
        written = torch.zeros(ROPE_PAIRS, heads, ROPE_CTX, dtype=torch.bool, device=dev)
        written[vp, :, vs] = True
        assert int(written.sum()) == heads * sum(ROPE_LENGTHS)
        assert bool((kc[~written] == -1234.5).all()) and bool((vc[~written] == -1234.5).all()), \
            f"{name}: cache rows other than (pair, head, tok_pos) were written"
        worst = max(worst, _check(name + " k", kc[vp, :, vs].view(-1, heads, 2, 64), ref[valid, 1], bound[valid, 1]))
        assert _same_bits(vc[vp, :, vs].reshape(-1, heads, 128), x.view(rows, 3, heads, 128)[valid, 2]), \
            f"{name}: v rows are not the input's bits"
    print(f"D rope_kvwrite {dt} heads={heads} {'S=3' if sliced else 'dense'}: max err/bound {worst:.3f}")
