"""llm_batch_weight_stream: what can be checked without a GPU - the option's validation (before any GPU work),
the ABI of the eight psg_batch_*_w8 / _w4 entries, and the routing table's lookup."""
import inspect
import re

import pytest

from openpsg_amd import _lib
from openpsg_amd._lib import PsgHipError
from tests.test_abi_symbols import HEADER, _declared


def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    return RelationTransformerHeadV4(device="cpu", tokenizers="word", **kw)


@pytest.mark.parametrize("bad", ("quantized", "stream", None, True))
def test_a_bad_value_raises(bad):
    with pytest.raises(PsgHipError, match="llm_batch_weight_stream must be 'dense' or 'quantised'"):
        _head(llm_batch_weight_stream=bad, llm_weight_quant="fp8")


def test_a_head_without_an_llm_stage_has_no_weights_to_stream():
    with pytest.raises(PsgHipError, match="no LLM stage"):
        _head(llm_batch_weight_stream="quantised", rel_cls_type="multiclass")


def test_an_unquantised_llm_has_no_bytes_to_stream():
    with pytest.raises(PsgHipError, match="llm_weight_quant='fp8' / 'mxfp4'"):
        _head(llm_batch_weight_stream="quantised")
    for fmt in ("fp8", "mxfp4"):
        assert _head(llm_batch_weight_stream="quantised", llm_weight_quant=fmt).llm_batch_weight_stream == "quantised"


def test_the_default_is_dense():
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.llm import LlamaDecodeEngine
    assert inspect.signature(RelationTransformerHeadV4.__init__).parameters["llm_batch_weight_stream"].default == "dense"
    assert inspect.signature(LlamaDecodeEngine.__init__).parameters["batch_quant_stream"].default is False
    assert _head().llm_batch_weight_stream == "dense"


def test_abi_608_declares_binds_and_exports_the_eight_entries():
    m = re.search(r"#define\s+PSG_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert int(m.group(1)) == _lib.PSG_ABI_VERSION == _lib.load().psg_version() >= 608
    decl = _declared()
    for name, nargs in (("psg_batch_gemm_w8_plan", 7), ("psg_batch_gemm_w8", 12), ("psg_batch_split_gemm_w8_plan", 6),
                        ("psg_batch_split_gemm_w8", 12), ("psg_batch_gemm_w4_plan", 7), ("psg_batch_gemm_w4", 13),
                        ("psg_batch_split_gemm_w4_plan", 6), ("psg_batch_split_gemm_w4", 13)):
        assert decl[name] == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)


def test_the_routing_lookup_streams_what_is_not_listed_and_honours_a_row_range():
    from openpsg_amd import llm
    table = {("fp8", "single", 4096, 4096): [(33, 49), (113, 161)], ("mxfp4", "pair", 12288, 4096): [(33, 161)]}
    route = lambda *a: llm._batch_quant_route(*a, table=table)               # noqa: E731
    assert [route("fp8", "single", 4096, 4096, r) for r in (33, 48, 49, 112, 113, 160)] == \
        ["dense", "dense", "stream", "stream", "dense", "dense"]
    assert route("fp8", "pair", 4096, 4096, 40) == "stream"                  # another form
    assert route("mxfp4", "single", 4096, 4096, 40) == "stream"              # another format
    assert route("fp8", "single", 4096, 11008, 40) == "stream"               # another shape
    assert route("mxfp4", "pair", 12288, 4096, 160) == "dense"
    assert llm._batch_quant_route("fp8", "single", 17, 19, 40) == "stream"   # the module's table: an unlisted shape
    for key, ranges in llm._BATCH_QUANT_DENSE.items():                       # well-formed: format, form, shape, row ranges
        assert key[0] in ("fp8", "mxfp4") and key[1] in ("single", "pair") and len(key) == 4
        assert all(33 <= lo < hi <= 161 for lo, hi in ranges)
