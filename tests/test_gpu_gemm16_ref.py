"""psg_skinny_gemm in bf16 / fp16 (psg_gemm.hip: the register variant and every LDS-DMA instantiation sg_launch can
dispatch) and psg_dense_gemm (psg_dense_gemm.hip: every tile geometry, the persistent walk over more tiles than
workgroups, the GELU and SwiGLU epilogues) against float64 (`-m gpu`).  These two kernels are what most of the suite is
compared with bit for bit (the fused and wide-slab variants, psg_decode_layer(s), psg_batch_gemm on 32 rows; every
dense tile against 256 x 256): this file is their own anchor.

References, input families and bounds are tests/gemm_ref.py (self-checked on the CPU by test_gemm_ref_cpu.py): the
`exact` family (integers in [-8, 8]: the fp32 result must equal the integer product bit for bit, in any accumulation
order) and the `spread` family (row scales over 16 / 12 binades: per element within 2^-20 |x| @ |w|^T of float64, plus
the output type's spacing for a 16-bit output).  Every test runs both families and both dtypes and prints its worst
err / bound.

Every skinny launch writes into a caller-provided partial buffer cut from the middle of a larger allocation: the
partials start as NaN, the floats before and after them and one extra trailing slice hold the sentinel of
rowops_ref_common; afterwards the sentinels must be untouched and every partial finite (none left unwritten)."""
import contextlib
import functools

import pytest
import torch

from tests import gemm_ref as G
from tests.rowops_ref_common import _sentinel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(f, d) for f in G.FAMILIES for d in G.DTYPES]
IDS = [f"{f}-{G.NAMES[d]}" for f, d in CASES]
OPTION_DEFAULTS = {"skinny_wide": 1, "skinny_dma": 813}     # psg_common.h (restored to if the option cannot be read)
GUARD_ROWS = 2
_WORST = {}


# ---- shared inputs and references (made once per shape, never modified) ----
@functools.lru_cache(maxsize=None)
def _x(family, M, K, dtype):
    return G.make_x(family, M, K, dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _w(family, N, K, dtype):
    return G.make_w(family, N, K, dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(family, M, N, K, dtype):
    ref, A = G.ref64(_x(family, M, K, dtype), _w(family, N, K, dtype))
    if family == "exact":
        G.assert_exact_range(A)
    return ref, A


@pytest.fixture(scope="module", autouse=True)
def _release_shared_tensors():
    yield
    for f in (_x, _w, _ref):
        f.cache_clear()
    for k in sorted(_WORST):
        print(f"worst err / bound, {k}: {_WORST[k]:.3g}")


def _note(kernel, dtype, ratio):
    key = f"{kernel} {G.NAMES[dtype]}"
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    return ratio


@contextlib.contextmanager
def _options(**opts):
    """context options for the duration of a block, restored to the values read before"""
    from openpsg_amd import _lib
    old = {}
    for k in opts:
        try:
            old[k] = _lib.get_option(0, k)
        except Exception:
            if k not in OPTION_DEFAULTS:
                raise
            old[k] = OPTION_DEFAULTS[k]
    try:
        for k, v in opts.items():
            _lib.set_option(0, k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(0, k, v)


# ---- the skinny kernel ----
def _skinny(x, w, splits=None, finite=True):
    """psg_skinny_gemm into a guarded partial buffer; splits=None: the planner's count under the current options"""
    from openpsg_amd import ops
    (M, K), N = x.shape, w.shape[0]
    S = ops.skinny_gemm_plan(M, N, K, x.dtype, DEV) if splits is None else splits
    buf, _ = _sentinel((S + 1) * M + 2 * GUARD_ROWS, N, torch.float32, DEV, extra=0)
    sentinel = float(buf[0, 0])
    flat = buf.view(-1)
    lo = GUARD_ROWS * N
    hi = lo + S * M * N                                      # then: one more slice and the trailing guard rows
    flat[lo:hi] = float("nan")
    part = flat[lo:hi].view(S, M, N)
    got = ops.skinny_gemm(x, w, splits=S, part=part)
    assert got.t.data_ptr() == part.data_ptr() and got.splits == S
    assert bool((flat[:lo] == sentinel).all()), "psg_skinny_gemm wrote in front of its partial buffer"
    assert bool((flat[hi:] == sentinel).all()), "psg_skinny_gemm wrote behind its partial buffer"
    if finite:
        assert bool(torch.isfinite(part).all()), "a partial was left unwritten (or is not finite)"
    return part


def _check_skinny(kernel, tag, family, dtype, M, N, K, part):
    ref, A = _ref(family, M, N, K, dtype)
    got = G.sum_slices(part)
    if family == "exact":
        assert torch.equal(got, ref.float()), f"{tag}: differs from the integer product in " \
                                              f"{int((got != ref.float()).sum())} of {got.numel()} elements"
        return 0.0
    return _note(kernel, dtype, G.check_out(tag, got, ref, G.bound32(A)))


def test_part_buffer_argument_is_checked():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    x, w = _x("exact", 4, 64, torch.float16), _w("exact", 16, 64, torch.float16)
    store = torch.zeros(4 * 16 + 8, device=DEV)
    with pytest.raises(PsgHipError, match="aligned"):
        ops.skinny_gemm(x, w, splits=1, part=store[1:65].view(1, 4, 16))
    with pytest.raises(PsgHipError, match="contiguous"):
        ops.skinny_gemm(x, w, splits=1, part=torch.zeros(1, 4, 32, device=DEV)[:, :, ::2])
    with pytest.raises(PsgHipError, match="part must be"):
        ops.skinny_gemm(x, w, splits=1, part=torch.zeros(2, 4, 16, device=DEV))
    with pytest.raises(PsgHipError, match="float32"):
        ops.skinny_gemm(x, w, splits=1, part=torch.zeros(1, 4, 16, device=DEV, dtype=torch.float64))
    part = store[4:68].view(1, 4, 16)
    assert ops.skinny_gemm(x, w, splits=1, part=part).t.data_ptr() == part.data_ptr()
    assert torch.equal(part, ops.skinny_gemm(x, w, splits=1).t)            # absent: as before


REG_MS = (1, 15, 16, 17, 31, 32)
# N, K, splits (None = planned): one wave's rows, nb == 0 | partial slab, nb == 0 with 3 remainder blocks | second slab
# partial, 5 K blocks: a batch + a remainder block (1 slice), uneven 2 / 3 blocks (2) | 17 K blocks: 4 batches + 1
# remainder, even and odd batch counts in the double-buffered stream
REG_SHAPES = [(16, 64, 1), (48, 192, 1), (80, 320, 1), (80, 320, 2), (1008, 1088, 1), (1008, 1088, 2), (1008, 1088, None)]


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
@pytest.mark.parametrize("N,K,splits", REG_SHAPES)
def test_skinny_register_variant(family, dtype, N, K, splits):
    assert N < 1024 or K < 1024
    worst = 0.0
    for M in REG_MS:
        part = _skinny(_x(family, M, K, dtype), _w(family, N, K, dtype), splits)
        worst = max(worst, _check_skinny("skinny register", f"M={M} N={N} K={K} S={part.shape[0]}", family, dtype, M, N,
                                         K, part))
    print(f"register variant N={N} K={K} splits={splits}: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_skinny_register_variant_several_slabs_per_workgroup(family, dtype):
    """N = 11088, K = 960, 3 slices, one workgroup per CU: 174 slabs of 64 rows (the last one partial) over
    ceil(CUs / 3) column groups - 86 on 256 CUs: workgroups walk 2 and 3 slabs, the pipelined load cursor crosses slab
    ends (5 K blocks per slice: one batch + one remainder block per slab)."""
    N, K = 11088, 960
    worst = 0.0
    with _options(skinny_wg_per_cu=1):
        for M in REG_MS:
            part = _skinny(_x(family, M, K, dtype), _w(family, N, K, dtype), 3)
            worst = max(worst, _check_skinny("skinny register", f"M={M} N={N} K={K} S=3", family, dtype, M, N, K, part))
    print(f"register variant N={N} K={K} splits=3, 1 workgroup per CU: worst err / bound = {worst:.3g}")


DMA_MS = (1, 16, 17, 32)
DMA_CONFIGS = [dict(skinny_dma=d, skinny_nt=nt, skinny_xdma=xd, skinny_wide=0)
               for d in (813, 815, 823, 414, 416, 423, 424) for nt, xd in ((1, 1), (1, 0), (0, 0))]
DMA_CONFIGS.append(dict(skinny_dma=813, skinny_nt=1, skinny_xdma=1, skinny_wide=1))
DMA_CONFIGS.append(dict(skinny_dma=0, skinny_nt=1, skinny_xdma=1, skinny_wide=0))       # the register kernel at these shapes
# minimum shape (416: the 4-batch stream is shorter than the 6-slot ring) | last slab 16 valid rows of 128 (DMA source
# clamp), 17 K blocks in one slice: x staged in 3 DMA chunks per row, the last masked; an odd block count for the UD = 2
# configurations (remainder blocks by direct loads beside pending DMAs)
DMA_SHAPES = [(1024, 1024, None), (1040, 1088, 1), (1040, 1088, None)]


def _cfg_name(cfg):
    return "dma={skinny_dma} nt={skinny_nt} xdma={skinny_xdma} wide={skinny_wide}".format(**cfg)


def _kernel_name(cfg):
    return f"skinny dma {cfg['skinny_dma']}" if cfg["skinny_dma"] else "skinny register"


def _dma_lds(cfg, M, K, S):
    """LDS bytes of the LDS-DMA kernel (psg_gemm.hip): the waves' rings, the partial tile, the x slice"""
    wv, ud, sl = cfg["skinny_dma"] // 100, cfg["skinny_dma"] // 10 % 10, cfg["skinny_dma"] % 10
    return wv * sl * ud * 2048 + 32 * (16 * wv + 4) * 4 + M * (-(-(K // 64) // S) * 128 + 16)


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
@pytest.mark.parametrize("N,K,splits", DMA_SHAPES)
def test_skinny_dma_variants(family, dtype, N, K, splits):
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    assert N >= 1024 and K >= 1024
    worst = 0.0
    for cfg in DMA_CONFIGS:
        with _options(**cfg):
            for M in DMA_MS:
                S = ops.skinny_gemm_plan(M, N, K, dtype, DEV) if splits is None else splits
                if cfg["skinny_dma"] and _dma_lds(cfg, M, K, S) > 160 * 1024:
                    # 32 rows of a 1088-wide slice beside the 5-slot or two-block rings: more than a CU's LDS - refused
                    assert M == 32 and S == 1 and cfg["skinny_dma"] in (815, 823)
                    with pytest.raises(PsgHipError, match="LDS"):
                        _skinny(_x(family, M, K, dtype), _w(family, N, K, dtype), S)
                    continue
                part = _skinny(_x(family, M, K, dtype), _w(family, N, K, dtype), S)
                tag = f"{_cfg_name(cfg)} M={M} N={N} K={K} S={part.shape[0]}"
                worst = max(worst, _check_skinny(_kernel_name(cfg), tag, family, dtype, M, N, K, part))
    print(f"LDS-DMA variants N={N} K={K} splits={splits}: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_skinny_dma_second_slab_per_workgroup(family, dtype):
    """N = 8336, K = 1024, 8 slices, 8-wave slabs: 66 slabs over 64 column groups on 256 CUs (fewer groups for the
    configurations with larger rings, 131 slabs for the 4-wave ones) - some workgroups carry their ring across a slab
    end and reuse the partial tile in LDS.  That a workgroup really walked two slabs is read from the kernel's trace
    buffer (words 6 and 7 of a wave: slabs walked, K blocks of its slice), not inferred."""
    from openpsg_amd import _lib
    N, K, S = 8336, 1024, 8
    trace = torch.zeros(1 << 17, dtype=torch.int64, device=DEV)
    worst = 0.0
    for cfg in DMA_CONFIGS:
        if cfg["skinny_wide"]:
            continue
        with _options(**cfg):
            for M in DMA_MS:
                trace.zero_()
                _lib.set_trace_buffer(0, _lib.PSG_TRACE_SKINNY_GEMM, trace)
                try:
                    part = _skinny(_x(family, M, K, dtype), _w(family, N, K, dtype), S)
                    torch.cuda.synchronize()
                finally:
                    _lib.set_trace_buffer(0, _lib.PSG_TRACE_NONE)
                tag = f"{_cfg_name(cfg)} M={M} N={N} K={K} S={S}"
                worst = max(worst, _check_skinny(_kernel_name(cfg), tag, family, dtype, M, N, K, part))
                if cfg["skinny_dma"]:
                    t = trace.view(-1, 8)
                    t = t[t[:, 0] > 0]
                    rows = 16 * (cfg["skinny_dma"] // 100)
                    assert t.shape[0] > 0, f"{tag}: no wave wrote its trace"
                    assert int(t[:, 6].max()) >= 2, f"{tag}: no workgroup walked a second slab"
                    assert int(t[:, 6].sum()) == S * (-(-N // rows)) * (rows // 16), f"{tag}: slabs walked"
                    assert bool((t[:, 7] == K // 64 // S).all()), f"{tag}: K blocks per slice"
    print(f"LDS-DMA variants N={N} K={K} splits={S}: worst err / bound = {worst:.3g}")


def _round_cost(cus, N, splits, waves):
    """sg_round_cost of psg_gemm.hip: slab rounds of a workgroup x slab height"""
    groups = max(cus // splits, 1)
    slabs = -(-N // (16 * waves))
    return -(-slabs // groups) * waves


def _slab_waves(cus, N, splits):
    """the slab height (in waves) sg_launch picks with skinny_wide on"""
    wv = 8
    for cand in (11, 12):
        if _round_cost(cus, N, splits, cand) < 0.95 * _round_cost(cus, N, splits, wv):
            wv = cand
    return wv


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
@pytest.mark.parametrize("N,waves", [(2800, 11), (2816, 11), (3056, 12), (3072, 12)])
def test_skinny_dma_wide_slabs(family, dtype, N, waves):
    """K = 1024 in 16 slices on 256 CUs: the cost rule picks 11-wave slabs for N = 2800 (last slab partial) and 2816,
    12-wave slabs for 3056 (partial) and 3072.  Same per-row arithmetic: bit-equal to the 8-wave kernel at the same
    slices, and both against the reference."""
    from openpsg_amd import _lib
    cus = _lib.device_info(0)[0]
    if cus != 256:
        pytest.skip(f"the slab heights of this test are what the cost rule picks on 256 CUs; this device has {cus}")
    K, S = 1024, 16
    assert _slab_waves(cus, N, S) == waves
    worst = 0.0
    for M in DMA_MS:
        x, w = _x(family, M, K, dtype), _w(family, N, K, dtype)
        with _options(skinny_dma=813, skinny_nt=1, skinny_xdma=1, skinny_wide=0):
            want = _skinny(x, w, S)
        with _options(skinny_dma=813, skinny_nt=1, skinny_xdma=1, skinny_wide=1):
            got = _skinny(x, w, S)
        assert torch.equal(got, want), f"M={M} N={N}: the {waves}-wave slabs differ from the 8-wave kernel"
        worst = max(worst, _check_skinny(f"skinny dma 813 ({waves}-wave slabs)", f"wide M={M} N={N} K={K} S={S}", family,
                                         dtype, M, N, K, got))
        _check_skinny("skinny dma 813", f"M={M} N={N} K={K} S={S}", family, dtype, M, N, K, want)
    print(f"{waves}-wave slabs N={N}: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_skinny_rows_do_not_leak_into_each_other(family, dtype):
    """N = 1040, K = 1088, every variant: with every x row but one NaN, the clean row's partials keep their bits and every
    other row is NaN."""
    M, N, K, keep = 17, 1040, 1088, 3
    x, w = _x(family, M, K, dtype), _w(family, N, K, dtype)
    xp = torch.full_like(x, float("nan"))
    xp[keep] = x[keep]
    others = [m for m in range(M) if m != keep]
    for cfg in DMA_CONFIGS:
        with _options(**cfg):
            base = _skinny(x, w)
            got = _skinny(xp, w, base.shape[0], finite=False)
        assert torch.equal(got[:, keep], base[:, keep]), f"{_cfg_name(cfg)}: the clean row changed with its neighbours"
        assert bool(torch.isnan(got[:, others]).all()), f"{_cfg_name(cfg)}: a poisoned row came out without NaN"


# ---- the dense kernel ----
TILES16 = ("256x256", "256x192", "256x128", "256x64", "128x128")
TILES32 = ("256x256", "256x128", "256x64", "128x128")                  # built with the fp32 output (and its GELU)
# tile, M, N, K: more padded tiles than the 256 persistent workgroups of a 256-CU device -> a second tile per workgroup
# (the next tile's first K step requested during the last one, LDS buffer parity across the hand-over with 1, 2 and 3 K
# steps, padding tiles of tile_mn skipped), ragged M (1 row) and N (16 columns).  10 (9) row blocks pad to 16, times 18
# (17) column blocks = 288 (272) tiles.  The last row is the other branch of tile_mn (fewer than 8 row blocks: the prompt
# pass): 7 x 33 blocks pad to 7 x 40 = 280 tiles, three workgroups walk a second tile, 31 find only padding
WALK = [("128x128", 1153, 2192, 64), ("128x128", 1153, 2192, 128), ("128x128", 1153, 2192, 192),
        ("256x256", 2305, 4368, 64), ("256x256", 2305, 4368, 128),
        ("256x64", 2049, 1040, 128), ("256x128", 2049, 2064, 128), ("256x192", 2049, 3088, 128),
        ("128x128", 769, 4112, 128)]
SMALL = [(1, 16, 64), (33, 272, 192)]                                  # minimum shape; N smaller than any tile


def _padded_tiles(tile, M, N):
    """ntile of dense_gemm_kernel: the row (or column) blocks padded to a multiple of 8 for the XCD map"""
    bm, bn = (int(v) for v in tile.split("x"))
    mb, nb = -(-M // bm), -(-N // bn)
    return -(-mb // 8) * 8 * nb if mb >= 8 else mb * (-(-nb // 8) * 8)


def _dense(tile, family, dtype, M, N, K, odt, bias=False, scales=False, gelu=False):
    """one psg_dense_gemm launch into a sentinel buffer, checked against float64; returns err / bound (0: bit-equal)"""
    from openpsg_amd import ops
    x, w = _x(family, M, K, dtype), _w(family, N, K, dtype)
    ref, A = _ref(family, M, N, K, dtype)
    b = G.make_bias(family, N).to(DEV) if bias else None
    ones = (torch.ones(M, device=DEV), torch.ones(N, device=DEV)) if scales else (None, None)
    buf, pristine = _sentinel(M, N, odt, DEV)
    ops.dense_gemm(x, w, b, gelu=gelu, out=buf[:M], out_dtype=odt, row_scale=ones[0], col_scale=ones[1], tile=tile)
    assert torch.equal(buf[M:], pristine[M:]), f"tile {tile}: rows past M were written"
    got = buf[:M]
    v, Av = (ref + b.double(), A + b.double().abs()) if bias else (ref, A)
    tag = f"dense {tile} {G.NAMES[dtype]}->{G.NAMES[odt]} M={M} N={N} K={K} bias={bias} scales={scales} gelu={gelu}"
    kernel = f"dense {tile} -> {'fp32' if odt == torch.float32 else '16-bit'}{' gelu' if gelu else ''}"
    if gelu:
        return _note(kernel, dtype, G.check_out(tag, got, G.gelu64(v), G.gelu_bound(v, G.bound32(Av), odt), odt))
    if family == "exact":
        assert torch.equal(got, v.to(odt)), f"{tag}: differs from the (rounded) integer result in " \
                                            f"{int((got != v.to(odt)).sum())} elements"
        return 0.0
    return _note(kernel, dtype, G.check_out(tag, got, v, G.bound_out(v, Av, odt), odt))


def _dense_all_outputs(tile, family, dtype, M, N, K):
    worst = _dense(tile, family, dtype, M, N, K, dtype, bias=True)
    worst = max(worst, _dense(tile, family, dtype, M, N, K, dtype))
    if tile in TILES32:
        worst = max(worst, _dense(tile, family, dtype, M, N, K, torch.float32))
        worst = max(worst, _dense(tile, family, dtype, M, N, K, torch.float32, bias=True, scales=True))
    return worst


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
@pytest.mark.parametrize("tile,M,N,K", WALK)
def test_dense_persistent_walk(family, dtype, tile, M, N, K):
    assert _padded_tiles(tile, M, N) > 256
    worst = _dense_all_outputs(tile, family, dtype, M, N, K)
    print(f"dense {tile} M={M} N={N} K={K}: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
@pytest.mark.parametrize("tile", TILES16)
def test_dense_smallest_shapes(family, dtype, tile):
    worst = max(_dense_all_outputs(tile, family, dtype, M, N, K) for M, N, K in SMALL)
    print(f"dense {tile} at {SMALL}: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_dense_gelu_epilogue(family, dtype):
    """GELU on the 256 x 256 tile with the 16-bit output and on every tile built with the fp32 output, at the shapes of
    the walk (a second tile per workgroup for 128 x 128 and 256 x 256), with a bias."""
    worst = 0.0
    for K in (64, 128):
        worst = max(worst, _dense("256x256", family, dtype, 2305, 4368, K, dtype, bias=True, gelu=True))
        worst = max(worst, _dense("256x256", family, dtype, 2305, 4368, K, torch.float32, bias=True, scales=True, gelu=True))
    for tile in ("256x128", "256x64", "128x128"):
        for K in (64, 128, 192):
            worst = max(worst, _dense(tile, family, dtype, 1153, 2192, K, torch.float32, bias=True, scales=True, gelu=True))
            worst = max(worst, _dense(tile, family, dtype, 1153, 2192, K, torch.float32, gelu=True))
    print(f"dense GELU: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("family,dtype", CASES, ids=IDS)
def test_dense_swiglu_epilogue(family, dtype):
    """SwiGLU on every tile at M = 1153, 2 x 1096 interleaved gate / up rows, K = 128, against the float64 formula with
    the documented roundings (GEMM output, silu(gate), product) and the bound derived in gemm_ref.swiglu64."""
    from openpsg_amd import ops
    M, inter, K = 1153, 1096, 128
    x, w = _x(family, M, K, dtype), _w(family, 2 * inter, K, dtype)
    ref, A = _ref(family, M, 2 * inter, K, dtype)
    want, bound = G.swiglu64(ref[:, :inter], ref[:, inter:], A[:, :inter], A[:, inter:], dtype)
    idx = torch.arange(2 * inter, device=DEV)                             # groups of 16 rows: 8 gate rows, their 8 up rows
    p, r = idx // 16, idx % 16
    wi = w[torch.where(r < 8, 8 * p + r, inter + 8 * p + r - 8)].contiguous()
    worst = 0.0
    for tile in TILES16:
        buf, pristine = _sentinel(M, inter, dtype, DEV)
        ops.dense_gemm(x, wi, swiglu=True, out=buf[:M], tile=tile)
        assert torch.equal(buf[M:], pristine[M:]), f"tile {tile}: rows past M were written"
        r_ = G.check_out(f"SwiGLU {tile} {G.NAMES[dtype]}", buf[:M], want, bound, dtype)
        worst = max(worst, _note(f"dense {tile} swiglu", dtype, r_))
    print(f"dense SwiGLU: worst err / bound = {worst:.3g}")
