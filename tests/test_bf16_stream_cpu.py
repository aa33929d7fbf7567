"""llm_bf16_value_stream: what can be checked without a GPU - the option's validation (before any GPU work), the
ABI of the five new entries, the exactness of the three-plane bf16 split (tests/split_b16_ref.py, the restatement the GPU
tests compare the kernels with) and the premise of the feature: a bf16-valued matrix fails the fp16 round trip."""
import inspect
import re

import pytest
import torch

from openpsg_amd import _lib
from openpsg_amd._lib import PsgHipError
from tests.split_b16_ref import bf16_valued, split_b16x3, wide_rows
from tests.test_abi_symbols import HEADER, _declared


def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    return RelationTransformerHeadV4(device="cpu", tokenizers="word", **kw)


def test_the_default_is_off():
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.llm import LlamaDecodeEngine
    assert inspect.signature(RelationTransformerHeadV4.__init__).parameters["llm_bf16_value_stream"].default is False
    assert inspect.signature(LlamaDecodeEngine.__init__).parameters["bf16_value_stream"].default is False
    assert _head(dtype="fp32s").llm_bf16_value_stream is False
    assert _head(dtype="fp32s", llm_bf16_value_stream=True).llm_bf16_value_stream is True


@pytest.mark.parametrize("bad", (1, 0, "on", None, "True"))
def test_a_value_that_is_not_a_bool_raises(bad):
    with pytest.raises(PsgHipError, match="llm_bf16_value_stream must be True or False"):
        _head(llm_bf16_value_stream=bad, dtype="fp32s")


def test_a_head_without_an_llm_stage_has_no_decode_steps():
    with pytest.raises(PsgHipError, match="llm_bf16_value_stream=True.*no LLM stage"):
        _head(llm_bf16_value_stream=True, dtype="fp32s", rel_cls_type="multiclass")


@pytest.mark.parametrize("dtype", ("fp32", "bf16", "fp16", "mixed"))
def test_only_fp32s_takes_the_option(dtype):
    with pytest.raises(PsgHipError, match="llm_bf16_value_stream=True.*fp32s"):
        _head(llm_bf16_value_stream=True, dtype=dtype)
    assert _head(llm_bf16_value_stream=False, dtype=dtype).llm_bf16_value_stream is False


@pytest.mark.parametrize("quant", ("fp8", "mxfp4", "int4g"))
def test_a_quantised_llm_does_not_take_the_option(quant):
    with pytest.raises(PsgHipError, match="llm_bf16_value_stream=True.*llm_weight_quant"):
        _head(llm_bf16_value_stream=True, dtype="fp32s", llm_weight_quant=quant)


def test_the_inference_tool_has_the_flag():
    import os
    src = open(os.path.join(os.path.dirname(HEADER), "..", "tools", "infer.py")).read()
    assert '"--llm-bf16-value-stream", action="store_true"' in src
    assert src.count('llm_bf16_value_stream=bool(getattr(a, "llm_bf16_value_stream", False))') == 2


def test_abi_612_declares_binds_and_exports_the_five_entries():
    m = re.search(r"#define\s+PSG_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert int(m.group(1)) == _lib.PSG_ABI_VERSION == _lib.load().psg_version() >= 612
    decl = _declared()
    for name, nargs in (("psg_split_b16x3", 7), ("psg_rmsnorm_split_b16x3", 10), ("psg_silu_mul_split_b16x3", 7),
                        ("psg_split_gemm_wb16_plan", 6), ("psg_split_gemm_wb16", 10)):
        assert decl[name] == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)
    from openpsg_amd import ops
    assert list(inspect.signature(ops.split_b16x3).parameters) == ["x"]
    assert list(inspect.signature(ops.rmsnorm_split_b16x3).parameters) == ["resid", "delta", "w", "eps"]
    assert list(inspect.signature(ops.silu_mul_split_b16x3).parameters) == ["gate_up"]
    assert list(inspect.signature(ops.split_gemm_wb16).parameters) == ["x3", "wb16", "mode", "part"]


def test_the_wrappers_check_their_arguments_before_the_library():
    from openpsg_amd import ops
    x3, w = torch.zeros((3, 20, 64), dtype=torch.bfloat16), torch.zeros((16, 64), dtype=torch.bfloat16)
    for call, match in (
            (lambda: ops.split_b16x3(torch.zeros(4, 64, dtype=torch.float16)), "x must be fp32"),
            (lambda: ops.split_b16x3(torch.zeros(64)), "x must be fp32"),
            (lambda: ops.split_b16x3(torch.zeros(4, 64)), "only on the GPU"),
            (lambda: ops.rmsnorm_split_b16x3(torch.zeros(4, 64).half(), None, torch.ones(64), 1e-5), "x must be fp32"),
            (lambda: ops.silu_mul_split_b16x3(torch.zeros(4, 128).half()), "gate_up must be fp32"),
            (lambda: ops.silu_mul_split_b16x3(torch.zeros(4, 100)), "gate_up must be fp32"),
            (lambda: ops.split_gemm_wb16(x3.half(), w), "bf16 planes"),
            (lambda: ops.split_gemm_wb16(x3[:2], w), "bf16 planes"),
            (lambda: ops.split_gemm_wb16(x3, w.half()), "w must be contiguous bf16"),
            (lambda: ops.split_gemm_wb16(x3, w[:, :32]), r"w must be contiguous bf16 \[N, 64\]"),
            (lambda: ops.split_gemm_wb16(x3, w), "only on the GPU")):
        with pytest.raises(PsgHipError, match=match):
            call()


def test_the_routing_table_is_well_formed():
    from openpsg_amd import llm
    assert isinstance(llm.WB16_STREAM_OFF, frozenset)
    assert all(len(s) == 2 and s[0] % 16 == 0 and s[1] % 64 == 0 for s in llm.WB16_STREAM_OFF)


def _rows():
    g = torch.Generator().manual_seed(3)
    tiny = torch.finfo(torch.float32).tiny
    x = wide_rows(37, 512, g)                                   # magnitudes 1e-6 .. 1e3
    edge = torch.zeros(4, 512)
    edge[0, ::2] = -0.0
    edge[1] = tiny                                              # the smallest normal number, both signs
    edge[1, ::2] = -tiny
    edge[2] = torch.randn(512, generator=g) * tiny * 2.0 ** 17  # full mantissas at the smallest magnitudes that still split
    edge[2] = torch.where(edge[2].abs() >= tiny * 2.0 ** 16, edge[2], torch.full_like(edge[2], tiny * 2.0 ** 16))
    edge[3] = torch.tensor([1.0, -1.0, 3.0e38, -3.0e38] * 128) * (1 + 2.0 ** -23)
    return torch.cat([x, edge])


def test_three_bf16_planes_reproduce_an_fp32_value_exactly():
    x = _rows()
    p = split_b16x3(x)
    assert p.dtype == torch.bfloat16 and tuple(p.shape) == (3,) + tuple(x.shape)
    total = p[0].double() + p[1].double() + p[2].double()
    assert torch.equal(total, x.double())
    # both intermediate differences are exact, and the planes descend by 2^-8 at the least
    r1 = x - p[0].float()
    assert torch.equal(r1.double(), x.double() - p[0].double())
    assert torch.equal((r1 - p[1].float()).double(), r1.double() - p[1].double())
    assert bool((p[1].float().abs() <= p[0].float().abs() * 2.0 ** -8).all())
    assert bool((p[2].float().abs() <= p[1].float().abs() * 2.0 ** -8).all())
    # signed zeros: -0 stays -0 in the leading plane and contributes nothing below
    z = split_b16x3(torch.tensor([0.0, -0.0]))
    assert torch.equal(z.float(), torch.zeros(3, 2)) and bool(torch.signbit(z[0].float())[1])


def test_a_bf16_valued_matrix_fails_the_fp16_round_trip_and_passes_the_bf16_one():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(2048, 2048, generator=g) * 0.02).bfloat16().float()
    assert torch.equal(w.bfloat16().float(), w)
    assert not torch.equal(w.half().float(), w)
    share = (w.half().float() != w).float().mean().item()
    assert 0 < share < 1e-2                                     # a few entries below fp16's subnormal grid are enough
    w2 = bf16_valued((256, 256), g)                              # the GEMM test's weights: magnitudes 2^-30 .. 2^3
    assert torch.equal(w2.bfloat16().float(), w2) and not torch.equal(w2.half().float(), w2)
    f = torch.randn(64, 64, generator=g)                        # a matrix trained in fp32 keeps its own stream
    assert not torch.equal(f.bfloat16().float(), f)
