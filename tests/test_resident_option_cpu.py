"""llm_weight_resident: what can be checked without a GPU - the option's validation (before any GPU work), the
ABI of the two expansion entries, and the mapping that quantises a model matrix by matrix for the lean loader."""
import re

import pytest
import torch

from openpsg_amd import _lib
from openpsg_amd._lib import PsgHipError
from tests.test_abi_symbols import HEADER, _declared


def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    return RelationTransformerHeadV4(device="cpu", tokenizers="word", **kw)


@pytest.mark.parametrize("bad", ("quantized", "bytes", None, True))
def test_a_bad_value_raises(bad):
    with pytest.raises(PsgHipError, match="llm_weight_resident must be 'all' or 'quantised'"):
        _head(llm_weight_resident=bad)


def test_multiclass_only_heads_have_no_llm_to_keep_lean():
    with pytest.raises(PsgHipError, match="no LLM stage"):
        _head(llm_weight_resident="quantised", rel_cls_type="multiclass")
    with pytest.raises(PsgHipError, match="no LLM stage"):                   # as llm_weight_quant does
        _head(llm_weight_quant="fp8", rel_cls_type="multiclass")


def test_the_default_is_all():
    from openpsg_amd.head import RelationTransformerHeadV4
    import inspect
    assert inspect.signature(RelationTransformerHeadV4.__init__).parameters["llm_weight_resident"].default == "all"
    from openpsg_amd.llm import LlamaDecodeEngine
    assert inspect.signature(LlamaDecodeEngine.__init__).parameters["resident"].default == "all"


def test_abi_607_declares_binds_and_exports_the_expansion_entries():
    m = re.search(r"#define\s+PSG_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert int(m.group(1)) == _lib.PSG_ABI_VERSION == _lib.load().psg_version() >= 607
    decl = _declared()
    for name, nargs in (("psg_expand_w8", 8), ("psg_expand_w4", 9)):
        assert decl[name] == nargs == len(_lib.SIGNATURES[name])
        assert hasattr(_lib.load(), name)


@pytest.mark.parametrize("fmt", ("fp8", "mxfp4"))
def test_lazy_quant_weights_is_quantize_llm_weights_one_matrix_at_a_time(fmt):
    """The lean loader's mapping hands out exactly what `quantize_llm_weights` returns - chunked by rows, one matrix held at
    a time - and passes everything else through."""
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.weights import LazyQuantWeights, llm_quant_keys, make_weights_numpy, quantize_llm_weights
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 2, 512, 512), max_object_num=30)
    w = {k: torch.as_tensor(v) for k, v in make_weights_numpy(cfg, seed=3).items() if k.startswith("language_model.")}
    keys = llm_quant_keys(2, lm_head=True)
    ref = quantize_llm_weights(w, 2, True, fmt)
    lazy = LazyQuantWeights(w, keys, fmt, "cpu", chunk_elems=256 * 40)       # 40-row chunks: several per matrix, a ragged last
    lazy["language_projection.bias"] = torch.zeros(3)
    assert "language_projection.bias" in lazy and "nope" not in lazy
    for k in ref:
        assert k in lazy
        assert torch.equal(torch.as_tensor(lazy[k]), torch.as_tensor(ref[k])), k
    assert ("language_model.lm_head.weight_bexp" in lazy) == (fmt == "mxfp4")
    assert lazy._last[0] is not None and len(lazy._last[1]) == (2 if fmt == "fp8" else 3)   # one matrix held, not the model
    again = LazyQuantWeights(ref, keys, fmt, "cpu")                          # an already quantised model is passed through
    assert not again._quant and all(again[k] is ref[k] for k in ref)
