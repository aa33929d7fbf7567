"""llm_batch_split_gemm: what can be checked without a GPU - the option's validation (before any GPU work), the
ABI of the four psg_batch_split_gemm_w16 / _w32 entries, the routing table's lookup, and a torch model of the w32 entry's
arithmetic (psg_split.hip's three products over K steps of 64) against float64.

The model, measured: worst |got - ref| / (|x| @ |W|^T) <= 1.2e-7 over the three shapes; with either cross term dropped
>= 1.9e-5.  The bound between them is the GPU test's for the w32 form, 2.5e-6 (tests/test_gpu_batch_split_gemm.py)."""
import inspect
import re

import pytest
import torch

from openpsg_amd import _lib
from openpsg_amd._lib import PsgHipError
from tests.test_abi_symbols import HEADER, _declared

W32_BOUND = 2.5e-6          # the pair-form bar 2e-6 + 2 x 2^-22: the weight's split residual and the dropped xl.wl term


def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    return RelationTransformerHeadV4(device="cpu", tokenizers="word", **kw)


@pytest.mark.parametrize("bad", ("ours", "kernel", None, True))
def test_a_bad_value_raises(bad):
    with pytest.raises(PsgHipError, match="llm_batch_split_gemm must be 'library' or 'own'"):
        _head(llm_batch_split_gemm=bad, dtype="fp32s")


def test_a_head_without_an_llm_stage_has_no_decode_steps():
    with pytest.raises(PsgHipError, match="no LLM stage"):
        _head(llm_batch_split_gemm="own", dtype="fp32s", rel_cls_type="multiclass")


@pytest.mark.parametrize("dtype", ("fp32", "bf16", "fp16", "mixed"))
def test_only_fp32s_takes_the_option(dtype):
    with pytest.raises(PsgHipError, match="psg_batch_gemm"):
        _head(llm_batch_split_gemm="own", dtype=dtype)
    assert _head(llm_batch_split_gemm="library", dtype=dtype).llm_batch_split_gemm == "library"


def test_fp32s_takes_it_and_the_default_is_library():
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.llm import LlamaDecodeEngine
    assert _head(llm_batch_split_gemm="own", dtype="fp32s").llm_batch_split_gemm == "own"
    assert inspect.signature(RelationTransformerHeadV4.__init__).parameters["llm_batch_split_gemm"].default == "library"
    assert inspect.signature(LlamaDecodeEngine.__init__).parameters["batch_split_gemm"].default is False
    assert _head(dtype="fp32s").llm_batch_split_gemm == "library"


def test_the_inference_tool_has_the_flag():
    import os
    src = open(os.path.join(os.path.dirname(HEADER), "..", "tools", "infer.py")).read()
    assert '"--llm-batch-split-gemm", choices=["library", "own"], default="library"' in src
    assert src.count('llm_batch_split_gemm=getattr(a, "llm_batch_split_gemm", "library")') == 2


def test_abi_610_declares_binds_and_exports_the_four_entries():
    m = re.search(r"#define\s+PSG_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert int(m.group(1)) == _lib.PSG_ABI_VERSION == _lib.load().psg_version() >= 610
    decl = _declared()
    for name, nargs in (("psg_batch_split_gemm_w16_plan", 6), ("psg_batch_split_gemm_w16", 13),
                        ("psg_batch_split_gemm_w32_plan", 6), ("psg_batch_split_gemm_w32", 14)):
        assert decl[name] == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)
    from openpsg_amd import ops
    assert list(inspect.signature(ops.batch_split_gemm_w16).parameters) == ["x2", "inv_scale", "w16", "col_scale", "mode"]
    assert list(inspect.signature(ops.batch_split_gemm_w32).parameters) == ["x2", "inv_scale", "w_img", "col_scale", "K", "lo_off",
                                                                           "mode"]


def test_the_wrappers_check_their_arguments_before_the_library():
    """`_x2_args`' checks and the weight's: dtype, rank, row layout, scale shapes, the planes' places - on host tensors,
    so that nothing past the checks is reached."""
    from openpsg_amd import ops
    x2, inv = torch.zeros((2, 40, 64), dtype=torch.float16), torch.ones(40)
    w16, s = torch.zeros((16, 64), dtype=torch.float16), torch.ones(16)
    img = torch.zeros((16, 192), dtype=torch.float16)
    for call, match in (
            (lambda: ops.batch_split_gemm_w16(x2.float(), inv, w16, s), "fp16 planes"),
            (lambda: ops.batch_split_gemm_w16(x2, inv[:39], w16, s), "inv_scale must be fp32"),
            (lambda: ops.batch_split_gemm_w16(x2, inv, w16.float(), s), "w16 must be fp16"),
            (lambda: ops.batch_split_gemm_w16(x2, inv, w16[:, :32], s), r"w16 must be fp16 \[N, 64\]"),
            (lambda: ops.batch_split_gemm_w16(x2, inv, w16.t().contiguous().t(), s), "contiguous rows"),
            (lambda: ops.batch_split_gemm_w16(x2, inv, w16, s[:8]), "col_scale must be fp32"),
            (lambda: ops.batch_split_gemm_w16(x2, inv, w16, s), "HBM"),
            (lambda: ops.batch_split_gemm_w32(x2, inv, img, s, 128), "x2 has K = 64"),
            (lambda: ops.batch_split_gemm_w32(x2, inv, img, s, 64, lo_off=32), "low plane"),
            (lambda: ops.batch_split_gemm_w32(x2, inv, img, s, 64, lo_off=160), "low plane"),
            (lambda: ops.batch_split_gemm_w32(x2, inv, img.float(), s, 64), "w_img must be fp16"),
            (lambda: ops.batch_split_gemm_w32(x2, inv, img, s.double(), 64), "col_scale must be fp32"),
            (lambda: ops.batch_split_gemm_w32(x2, inv, img, s, 64), "HBM")):
        with pytest.raises(PsgHipError, match=match):
            call()


def test_the_routing_lookup_takes_the_kernel_for_what_is_not_listed_and_honours_a_row_range():
    from openpsg_amd import llm
    table = {("w32", 4096, 4096): [(33, 49), (113, 161)], ("w16", 12288, 4096): [(33, 161)]}
    route = lambda *a: llm._batch_split_route(*a, table=table)               # noqa: E731
    assert [route("w32", 4096, 4096, r) for r in (33, 48, 49, 112, 113, 160)] == \
        ["library", "library", "own", "own", "library", "library"]
    assert route("w16", 4096, 4096, 40) == "own"                             # another form
    assert route("w32", 4096, 11008, 40) == "own"                            # another shape
    assert route("w16", 12288, 4096, 160) == "library"
    assert llm._batch_split_route("w32", 17, 19, 40) == "own"                # the module's table: an unlisted shape
    for key, ranges in llm._BATCH_SPLIT_LIBRARY.items():                     # well-formed: form, shape, row ranges
        assert key[0] in ("w16", "w32") and len(key) == 3
        assert all(33 <= lo < hi <= 161 for lo, hi in ranges)


# ---- the w32 arithmetic, modelled in torch ---------------------------------------------------------------------------------
def _split(v):
    """psg_split_f16x3 / psg_split_f16x2 on fp32 rows: (hi, lo) fp16 planes of v 2^t with the row's largest magnitude in
    [2^13, 2^14), and inv_scale = 2^-t."""
    mx = v.abs().amax(dim=1)
    e = torch.floor(torch.log2(mx.double())).to(torch.int32)
    e = torch.where(mx > 0, e, torch.full_like(e, 13))
    se = (127 + 13 - e).clamp(1, 253)
    scale = torch.exp2((se - 127).double()).float()
    inv = torch.exp2((127 - se).double()).float()
    s = v * scale[:, None]                                                   # exact: a power of two
    hi = s.half()                                                            # round to nearest even
    lo = (s - hi.float()).half()                                             # (the difference is exact in fp32)
    return hi, lo, inv


def _model_w32(x, w, terms=("hh", "hl", "lh")):
    """(xh.wh + xh.wl + xl.wh) inv_scale[m] col_scale[n]: every fp16 product exact in fp32, fp32 accumulation over K steps of
    64 in the kernel's order (xh.wh, xh.wl, xl.wh per step).  `terms` drops products (the mutants)."""
    xh, xl, xi = _split(x)
    wh, wl, wi = _split(w)
    acc = torch.zeros((x.shape[0], w.shape[0]), dtype=torch.float32)
    for k0 in range(0, x.shape[1], 64):
        k = slice(k0, k0 + 64)
        if "hh" in terms:
            acc += xh[:, k].float() @ wh[:, k].float().t()
        if "hl" in terms:
            acc += xh[:, k].float() @ wl[:, k].float().t()
        if "lh" in terms:
            acc += xl[:, k].float() @ wh[:, k].float().t()
    return acc * (xi[:, None] * wi[None, :])


@pytest.mark.parametrize("N,K", [(272, 384), (48, 4096), (4096, 256)])
def test_the_three_product_model_is_fp32_grade_and_needs_both_cross_terms(N, K):
    g = torch.Generator().manual_seed(610 + N + K)
    x = torch.randn(160, K, generator=g) * torch.logspace(-6, 3, 33).repeat(5)[:160, None]
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.rand(N, generator=g) * 10 - 12)[:, None] * 0.977
    ref = x.double() @ w.double().t()
    bound = x.double().abs() @ w.double().abs().t()

    def worst(got):
        return ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    clean, no_hl, no_lh = worst(_model_w32(x, w)), worst(_model_w32(x, w, ("hh", "lh"))), worst(_model_w32(x, w, ("hh", "hl")))
    print(f"w32 model N={N} K={K}: worst / (|x| @ |W|^T) = {clean:.3e}; without xh.wl {no_hl:.3e}, without xl.wh {no_lh:.3e} "
          f"(bound {W32_BOUND:.1e})")
    assert clean < W32_BOUND
    assert no_hl > W32_BOUND and no_lh > W32_BOUND
