"""The Q-Former inference row kernels against float64 references (`-m gpu`): add + LayerNorm in its plain / periodic /
indexed forms (fp32 kernel, the 16-bit half-wave-per-row kernel, the wave-per-row 16-bit kernel, the mixed-mode dual-output
kernel), the existence head, the row gathers and the split-K partial reduction.

Until now these were checked by the goldens at six scene sizes and by tests that compare one variant with another; a
mistake shared by a kernel and its variant passed both.  Here the reference is the plain formula in float64, rounded once
to the output dtype.  fp32 outputs are held to an fp32 error bound scaled to the operands (RED * 2^-24 * sum|terms| for a
reduction, RED = the kernel's per-lane serial length + its tree depth); 16-bit outputs to one unit in the last place of the
output dtype at the reference value, plus that fp32 bound (which matters only where cancellation leaves the output near
zero).  Every output buffer is longer than the kernel's rows and sentinel-filled: rows past the end must stay untouched.
"""
import pytest
import torch

from tests.rowops_ref_common import _check, _sentinel, _ulp

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TINY = 2.0 ** -126
H = 768
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ln_ref(v, gamma, beta, eps, va):
    """float64 LayerNorm of the summed rows v, and the fp32 error bound of the kernels computing it from the fp32-summed
    operands (va = sum of the operands' magnitudes, element-wise)"""
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    xh = (v - mu) * rs
    y = xh * gamma + beta
    red = 24 + 6                                                    # 24 features per lane (16-bit kernel), then the tree
    e_v = 2 * EPS * va
    e_mu = red * EPS * v.abs().mean(-1, keepdim=True) + e_v.mean(-1, keepdim=True)
    e_xh = (e_v + e_mu) * rs + xh.abs() * ((red + 6) * EPS)
    bound = 2 * (gamma.abs() * e_xh + EPS * ((xh * gamma).abs() + beta.abs()))
    return y, bound


def _ln_inputs(rows, dtype, seed, dev, table_rows=None):
    g = _gen(seed)
    x = torch.randn(rows, H, generator=g)
    x[3::7] += 100.0                                                # rows with a large common offset
    res = torch.randn(rows if table_rows is None else table_rows, H, generator=g)
    bias = torch.randn(H, generator=g)
    gamma = 1 + 0.5 * torch.randn(H, generator=g)
    beta = torch.randn(H, generator=g)
    return x.to(dev, dtype), res.to(dev, dtype), bias.to(dev), gamma.to(dev), beta.to(dev)


def _ln_expect(x, res_rows, bias, gamma, beta, eps, out_dtype):
    """float64 reference of LayerNorm(x + bias + res_rows) and the bound for an output of out_dtype"""
    v = x.double()
    va = v.abs()
    if bias is not None:
        v, va = v + bias.double(), va + bias.double().abs()
    if res_rows is not None:
        v, va = v + res_rows.double(), va + res_rows.double().abs()
    y, b32 = _ln_ref(v, gamma.double(), beta.double(), eps, va)
    return y, b32 + _ulp(y, out_dtype)


# fp32 rows take the wave-per-row kernel; 16-bit rows the half-wave-per-row kernel (option ln_half_wave = 1, the
# default) or the wave-per-row kernel (0)
VARIANTS = [("fp32", 1), ("bf16", 1), ("bf16", 0), ("fp16", 1), ("fp16", 0)]
VARIANT_IDS = ["fp32", "bf16-halfwave", "bf16-wave", "fp16-halfwave", "fp16-wave"]


@pytest.fixture(params=VARIANTS, ids=VARIANT_IDS)
def variant(request):
    from openpsg_amd import _lib
    dt, hw = request.param
    _lib.set_option(0, "ln_half_wave", hw)
    yield dt, hw
    _lib.set_option(0, "ln_half_wave", 1)


@pytest.mark.parametrize("rows", [1, 2, 3, 33, 34 * 33 + 1, 82500])
def test_add_layernorm_plain_vs_float64(variant, rows):
    """psg_add_layernorm: LayerNorm(x + bias + residual), bias and residual each present or absent.  Odd row counts leave
    the last half-wave of the 16-bit kernel without a row (it is clamped to rows - 1 and must not store)."""
    from openpsg_amd import ops
    dt, half_wave = variant
    dev, dtype, eps = _dev(), DTYPES[dt], 1e-12
    x, res, bias, gamma, beta = _ln_inputs(rows, dtype, rows * 3 + len(dt), dev)
    worst = 0.0
    for use_bias in (True, False):
        for use_res in (True, False):
            b, r = (bias if use_bias else None), (res if use_res else None)
            buf, pristine = _sentinel(rows, H, dtype, dev)
            x_before = x.clone()
            ops.add_layernorm(x, r, b, gamma, beta, eps, out=buf[:rows])
            torch.cuda.synchronize()
            assert torch.equal(buf[rows:], pristine[rows:]), "rows past the end of the output were written"
            assert torch.equal(x, x_before), "the input changed although an output buffer was given"
            want, bound = _ln_expect(x, r, b, gamma, beta, eps, dtype)
            worst = max(worst, _check(f"add_layernorm {dt} bias={use_bias} res={use_res}", buf[:rows], want, bound))
    print(f"add_layernorm {dt} rows={rows} half_wave={half_wave}: max err/bound {worst:.3f}")


@pytest.mark.parametrize("rows", [1, 3, 34, 34 * 33 + 1])
def test_add_layernorm_periodic_vs_float64(variant, rows):
    """psg_add_layernorm_periodic: residual row r % 33 of a 33-row table; rows not a multiple of 33."""
    from openpsg_amd import ops
    dt, half_wave = variant
    dev, dtype, eps = _dev(), DTYPES[dt], 1e-12
    x, tab, bias, gamma, beta = _ln_inputs(rows, dtype, rows * 5 + len(dt), dev, table_rows=33)
    buf, pristine = _sentinel(rows, H, dtype, dev)
    ops.add_layernorm_periodic(x, tab, bias, gamma, beta, eps, out=buf[:rows])
    torch.cuda.synchronize()
    assert torch.equal(buf[rows:], pristine[rows:]), "rows past the end of the output were written"
    want, bound = _ln_expect(x, tab[torch.arange(rows, device=dev) % 33], bias, gamma, beta, eps, dtype)
    print(f"add_layernorm_periodic {dt} rows={rows} half_wave={half_wave}: err/bound {_check('periodic', buf[:rows], want, bound):.3f}")


@pytest.mark.parametrize("rows", [33, 99, 35 * 33, 2501 * 33])
def test_add_layernorm_indexed_vs_float64(variant, rows):
    """psg_add_layernorm_indexed: groups of 33 rows take block block_index[g] of a 7-block table (blocks repeat); odd
    multiples of 33 reach the dead half-wave of the 16-bit kernel."""
    from openpsg_amd import ops
    dt, half_wave = variant
    dev, dtype, eps = _dev(), DTYPES[dt], 1e-5
    x, tab, bias, gamma, beta = _ln_inputs(rows, dtype, rows * 11 + len(dt), dev, table_rows=7 * 33)
    G = rows // 33
    idx = torch.randint(0, 7, (G,), generator=_gen(rows))
    idx[:2] = torch.tensor([6, 6])[:G]
    idx = idx.to(torch.int32).to(dev)
    buf, pristine = _sentinel(rows, H, dtype, dev)
    ops.add_layernorm_indexed(x, tab, idx, 33, bias, gamma, beta, eps, out=buf[:rows])
    torch.cuda.synchronize()
    assert torch.equal(buf[rows:], pristine[rows:]), "rows past the end of the output were written"
    rrow = (idx.long()[:, None] * 33 + torch.arange(33, device=dev)[None]).reshape(-1)
    want, bound = _ln_expect(x, tab[rrow], bias, gamma, beta, eps, dtype)
    print(f"add_layernorm_indexed {dt} rows={rows} half_wave={half_wave}: err/bound {_check('indexed', buf[:rows], want, bound):.3f}")


@pytest.mark.parametrize("mode,rows", [(m, r) for m in ("plain", "periodic", "none") for r in (1, 99, 2501 * 33)]
                         + [("indexed", 33), ("indexed", 99), ("indexed", 2501 * 33)])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_add_layernorm_res32_vs_float64(dt, rows, mode):
    """psg_add_layernorm_res32 (mixed mode): 16-bit x + bias + fp32 residual (plain, 33-periodic, indexed blocks, or none)
    written as out16 only, out32 only, or both.  out32 is the unrounded fp32 result; out16 is exactly its rounding."""
    from openpsg_amd import ops
    dev, dtype, eps = _dev(), DTYPES[dt], 1e-12
    g = _gen(rows + len(mode))
    x, _, bias, gamma, beta = _ln_inputs(rows, dtype, rows * 13 + len(mode), dev)
    period, index = 0, None
    if mode == "plain":
        res = torch.randn(rows, H, generator=g).to(dev)
        res_rows = res
    elif mode == "periodic":
        period, res = 33, torch.randn(33, H, generator=g).to(dev)
        res_rows = res[torch.arange(rows, device=dev) % 33]
    elif mode == "indexed":
        period, res = 33, torch.randn(5 * 33, H, generator=g).to(dev)
        index = torch.randint(0, 5, (rows // 33,), generator=g).to(torch.int32).to(dev)
        res_rows = res[(index.long()[:, None] * 33 + torch.arange(33, device=dev)[None]).reshape(-1)]
    else:
        res = res_rows = None
    want, b32 = _ln_expect(x, res_rows, bias, gamma, beta, eps, torch.float32)
    b16 = b32 + _ulp(want, dtype)
    worst = 0.0
    for want16, want32 in ((True, True), (True, False), (False, True)):
        o16, p16 = _sentinel(rows, H, dtype, dev)
        o32, p32 = _sentinel(rows, H, torch.float32, dev)
        ops.add_layernorm_res32(x, res, bias, gamma, beta, eps, out16=o16[:rows], out32=o32[:rows], period=period,
                                index=index, want16=want16, want32=want32)
        torch.cuda.synchronize()
        assert torch.equal(o16[rows:], p16[rows:]) and torch.equal(o32[rows:], p32[rows:]), "rows past the end written"
        assert want16 or torch.equal(o16, p16), "out16 written although not requested"
        assert want32 or torch.equal(o32, p32), "out32 written although not requested"
        if want32:
            worst = max(worst, _check(f"res32 {mode} out32", o32[:rows], want, b32))
        if want16:
            worst = max(worst, _check(f"res32 {mode} out16", o16[:rows], want, b16))
        if want16 and want32:
            assert torch.equal(o16[:rows], o32[:rows].to(dtype)), "out16 is not the rounding of out32"
    print(f"add_layernorm_res32 {dt} rows={rows} {mode}: max err/bound {worst:.3f}")


def test_add_layernorm_rejects_other_widths():
    """Every add + LayerNorm variant is built for hidden == 768 only: any other width is refused, not computed."""
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    dev = _dev()
    for hidden in (512, 1024, 64):
        for dtype in DTYPES.values():
            x = torch.randn(66, hidden, device=dev).to(dtype)
            before = x.clone()
            w, b = torch.ones(hidden, device=dev), torch.zeros(hidden, device=dev)
            with pytest.raises(PsgHipError):
                ops.add_layernorm(x, None, None, w, b, 1e-12)
            with pytest.raises(PsgHipError):
                ops.add_layernorm_periodic(x, x[:33].contiguous(), None, w, b, 1e-12)
            with pytest.raises(PsgHipError):
                ops.add_layernorm_indexed(x, x[:33].contiguous(), torch.zeros(2, dtype=torch.int32, device=dev), 33, None,
                                          w, b, 1e-12)
            if dtype != torch.float32:
                with pytest.raises(PsgHipError):
                    ops.add_layernorm_res32(x, None, None, w, b, 1e-12)
            torch.cuda.synchronize()
            assert torch.equal(x, before)


# ---- existence head -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("P", [0, 1, 3, 5, 2500])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_exist_head_vs_float64(dt, P, nq):
    """logit[p] = x[p * nq] . w + b, prob = sigmoid(logit): only row 0 of each pair is read (the others are NaN here),
    and prob saturates to 0 / 1 for logits of -+100 without a NaN.  P = 0 (no pairs: empty tensors, whose NULL data
    pointers the C ABI used to refuse) gives empty results."""
    from openpsg_amd import ops
    dev, dtype = _dev(), DTYPES[dt]
    g = _gen(P * 3 + nq + len(dt))
    w = torch.randn(H, generator=g)
    b = torch.randn(1, generator=g)
    x = torch.full((P * nq, H), float("nan"))
    x[::nq] = torch.randn(P, H, generator=g) if P else x[::nq]
    if P >= 3:
        w16 = w.to(dtype).float()
        x[0] = w16 * (100.0 / (w16 * w16).sum())                      # logit ~ +100 + b
        x[nq] = -x[0]                                                 # logit ~ -100 + b
    x, w, b = x.to(dev, dtype), w.to(dev), b.to(dev)
    logit, prob = ops.exist_head(x, w, b, P, nq)
    torch.cuda.synchronize()
    assert logit.shape == (P,) and prob.shape == (P,)
    if P == 0:
        return
    x0 = x[::nq].double()
    ref = x0 @ w.double() + b.double()
    bl = 2 * (12 + 6 + 2) * EPS * ((x0.abs() @ w.double().abs()) + b.double().abs())
    rp = torch.sigmoid(ref)
    bp = rp * (1 - rp) * bl + 4 * EPS * rp + TINY
    assert torch.isfinite(prob).all() and bool(((prob >= 0) & (prob <= 1)).all())
    if P >= 3:
        assert prob[0].item() == 1.0 and prob[1].item() < 1e-40, (prob[0].item(), prob[1].item())
    print(f"exist_head {dt} P={P} nq={nq}: err/bound logit {_check('exist logit', logit, ref, bl):.3f}, "
          f"prob {_check('exist prob', prob, rp, bp):.3f}")


# ---- row gathers --------------------------------------------------------------------------------------------------
PAIRS = [("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "bf16"), ("bf16", "fp32"), ("fp32", "fp16"), ("fp16", "fp16"),
         ("fp16", "fp32")]


@pytest.mark.parametrize("cols", [4, 12, 260, 768])
@pytest.mark.parametrize("src_dt,dst_dt", PAIRS)
def test_gather_rows_vs_indexing(src_dt, dst_dt, cols):
    """dst[r] = src[idx[r]] converted once (idx < 0 -> a zero row), on row-strided source and destination views: the
    bytes between the rows and the rows past the end of the destination stay untouched."""
    from openpsg_amd import ops
    dev = _dev()
    sdt, ddt = DTYPES[src_dt], DTYPES[dst_dt]
    g = _gen(cols + len(src_dt) * 10 + len(dst_dt))
    n_src, n = 50, 37
    big = torch.randn(n_src, cols + 12, generator=g).to(dev, sdt)
    src = big[:, 4:4 + cols]
    idx = torch.randint(0, n_src, (n,), generator=g)
    idx[:4] = torch.tensor([-1, n_src - 1, -7, 0])
    idx = idx.to(torch.int32).to(dev)
    dbig, pristine = _sentinel(n, cols + 8, ddt, dev)
    dst = dbig[:n, :cols]
    ops.gather_rows(src, idx, dst)
    torch.cuda.synchronize()
    want = torch.where((idx >= 0)[:, None], src[idx.long().clamp_min(0)].to(ddt), torch.zeros((), dtype=ddt, device=dev))
    assert torch.equal(dst, want), "gathered rows differ from indexing + one conversion"
    assert torch.equal(dbig[:n, cols:], pristine[:n, cols:]) and torch.equal(dbig[n:], pristine[n:]), \
        "bytes outside the destination rows were written"


def test_gather_rows_rejects_other_conversions():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    dev = _dev()
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    for s, d in (("bf16", "fp16"), ("fp16", "bf16")):
        dst = torch.zeros(2, 8, device=dev, dtype=DTYPES[d])
        with pytest.raises(PsgHipError):
            ops.gather_rows(torch.ones(3, 8, device=dev, dtype=DTYPES[s]), idx, dst)
        torch.cuda.synchronize()
        assert not dst.any()


@pytest.mark.parametrize("want_aux", [True, False])
@pytest.mark.parametrize("T", [0, 7])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_gather_pair_rows_vs_indexing(dt, T, want_aux):
    """psg_gather_pair_rows against Python indexing of the same tables: selected global pair ids inside and outside the
    chunk's window [first, first + count) (outside -> the chunk's first pair, mine = 0), shifted by slot_off, text rows
    through text_index."""
    from openpsg_amd import ops
    dev, dtype = _dev(), DTYPES[dt]
    g = _gen(T * 2 + int(want_aux) + len(dt))
    nq, cols, first, count, slot_off, nblk = 3, 260, 40, 9, 2, 4
    npos = slot_off + count
    xq = torch.randn(npos * nq, cols, generator=g).to(dev, dtype)
    xt = torch.randn(nblk * T, cols, generator=g).to(dev, dtype) if T else None
    text_index = torch.randint(0, nblk, (npos,), generator=g).to(torch.int32).to(dev) if T else None
    text_mask = (torch.rand(npos, T, generator=g) < 0.6).to(torch.uint8).to(dev)
    pair_index = torch.randperm(1000, generator=g)[:npos].to(torch.int32).to(dev)
    sel = torch.tensor([first + 3, first, 12, first + count - 1, first + count, first - 1, first + 3], dtype=torch.int32)
    K = sel.numel()
    out, tm, pi, mine = ops.gather_pair_rows(xq, xt, text_index, text_mask, pair_index, sel.to(dev), first, count,
                                             slot_off, nq, T, want_aux=want_aux)
    torch.cuda.synchronize()
    ids = sel.tolist()
    m = [first <= i < first + count for i in ids]
    pos = [(i - first if mi else 0) + slot_off for i, mi in zip(ids, m)]
    want_q = torch.cat([xq[p * nq:(p + 1) * nq] for p in pos])
    assert torch.equal(out[:K * nq], want_q), "query rows"
    if T:
        ti = text_index.tolist()
        want_t = torch.cat([xt[ti[p] * T:(ti[p] + 1) * T] for p in pos])
        assert torch.equal(out[K * nq:], want_t), "text rows"
    assert out.shape == (K * (nq + T), cols)
    if want_aux:
        assert pi.tolist() == [pair_index[p].item() for p in pos]
        assert mine.tolist() == [int(x) for x in m]
        if T:
            assert torch.equal(tm, text_mask[torch.tensor(pos, device=dev)])


# ---- split-K partial sums -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4), (3, 12), (20, 4096)])
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_partials_reduce_vs_float64(dt, S, shape):
    """Partials.reduce: the fp32 sum of the S slices in split order, converted once: within S 2^-24 sum|slices| (+ one
    ulp of a 16-bit output) of the float64 sum; a single slice converts exactly."""
    from openpsg_amd import ops
    dev, dtype = _dev(), DTYPES[dt]
    g = _gen(S * 100 + shape[1] + len(dt))
    t = (torch.randn(S, *shape, generator=g) * torch.logspace(-3, 3, shape[1])[None, None]).to(dev)
    y = ops.Partials(t).reduce(dtype)
    torch.cuda.synchronize()
    assert y.shape == shape and y.dtype == dtype
    if S == 1:
        assert torch.equal(y, t[0].to(dtype))
    ref = t.double().sum(0)
    bound = S * EPS * t.double().abs().sum(0) + _ulp(ref, dtype) + 1e-300
    print(f"reduce_partials {dt} S={S} {shape}: err/bound {_check('reduce', y, ref, bound):.3f}")
