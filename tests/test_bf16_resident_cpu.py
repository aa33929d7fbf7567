"""llm_bf16_value_resident: what can be checked without a GPU - the option's validation (before any GPU work),
the ABI of the two new entries, the loader (records held as their bf16 copy only, the chunked bf16-value check, the refusal
of a matrix that is no bf16 value), the routing lookup, and a torch model of the stacked three-plane product in the fixed
order (y2 + y1) + y0 against float64."""
import inspect
import os
import re

import pytest
import torch

from openpsg_amd import _lib
from openpsg_amd import llm_matrix as LM
from openpsg_amd._lib import PsgHipError
from tests.split_b16_ref import bf16_valued, split_b16x3, wide_rows
from tests.test_abi_symbols import HEADER, _declared

BAR = 2e-6                                                    # the project's bar for fp32-grade products: x (|x| @ |w|^T)


def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    return RelationTransformerHeadV4(device="cpu", tokenizers="word", **kw)


def test_the_default_is_off():
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.llm import LlamaDecodeEngine
    assert inspect.signature(RelationTransformerHeadV4.__init__).parameters["llm_bf16_value_resident"].default is False
    assert inspect.signature(LlamaDecodeEngine.__init__).parameters["bf16_value_resident"].default is False
    assert _head(dtype="fp32s").llm_bf16_value_resident is False
    assert _head(dtype="fp32s", llm_bf16_value_stream=True).llm_bf16_value_resident is False
    assert _head(dtype="fp32s", llm_bf16_value_stream=True, llm_bf16_value_resident=True).llm_bf16_value_resident is True


@pytest.mark.parametrize("bad", (1, 0, "on", None, "True"))
def test_a_value_that_is_not_a_bool_raises(bad):
    with pytest.raises(PsgHipError, match="llm_bf16_value_resident must be True or False"):
        _head(llm_bf16_value_resident=bad, llm_bf16_value_stream=True, dtype="fp32s")


@pytest.mark.parametrize("kw", (dict(dtype="fp32s"), dict(dtype="fp32s", llm_bf16_value_stream=False), dict(dtype="bf16"),
                                dict(dtype="fp32s", llm_weight_quant="fp8"), dict(dtype="fp32s", rel_cls_type="multiclass")))
def test_the_option_needs_the_bf16_value_stream(kw):
    with pytest.raises(PsgHipError, match="llm_bf16_value_resident=True.*needs llm_bf16_value_stream=True"):
        _head(llm_bf16_value_resident=True, **kw)


@pytest.mark.parametrize("kw,match", (
        (dict(dtype="fp32", llm_bf16_value_stream=True), "llm_bf16_value_stream=True.*fp32s"),
        (dict(dtype="fp32s", llm_bf16_value_stream=True, llm_weight_quant="fp8"), "llm_bf16_value_stream=True.*llm_weight_quant"),
        (dict(dtype="fp32s", llm_bf16_value_stream=True, rel_cls_type="multiclass"), "llm_bf16_value_stream=True.*no LLM stage")))
def test_the_stream_option_keeps_its_own_refusals(kw, match):
    """... which is why `True` with the stream implies fp32s, an LLM stage and no llm_weight_quant."""
    with pytest.raises(PsgHipError, match=match):
        _head(llm_bf16_value_resident=True, **kw)


def test_the_engine_validates_its_keyword_before_it_loads_anything():
    from openpsg_amd.llm import LlamaDecodeEngine
    for kw, match in ((dict(bf16_value_resident=1, bf16_value_stream=True, prefill_split=True), "must be a bool"),
                      (dict(bf16_value_resident=True, prefill_split=True), "needs bf16_value_stream=True"),
                      (dict(bf16_value_resident=True, bf16_value_stream=True), "prefill_split"),
                      (dict(bf16_value_resident=True, bf16_value_stream=True, prefill_split=True, resident="quantised"),
                       "resident='all'")):
        with pytest.raises(PsgHipError, match=match):
            LlamaDecodeEngine({}, None, "cpu", torch.float32, **kw)


def test_the_inference_tool_has_the_flag():
    src = open(os.path.join(os.path.dirname(HEADER), "..", "tools", "infer.py")).read()
    assert '"--llm-bf16-value-resident", action="store_true"' in src
    assert src.count('llm_bf16_value_resident=bool(getattr(a, "llm_bf16_value_resident", False))') == 2


def test_abi_615_declares_binds_and_exports_the_two_entries():
    m = re.search(r"#define\s+PSG_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert int(m.group(1)) == _lib.PSG_ABI_VERSION == _lib.load().psg_version() >= 615
    decl = _declared()
    for name, nargs in (("psg_batch_split_gemm_wb16_plan", 6), ("psg_batch_split_gemm_wb16", 10)):
        assert decl[name] == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)
    from openpsg_amd import ops
    assert list(inspect.signature(ops.batch_split_gemm_wb16).parameters) == ["x3", "w", "mode"]
    assert list(inspect.signature(ops.batch_split_gemm_wb16_plan).parameters) == ["M", "N", "K", "device", "mode"]
    src = open(os.path.join(os.path.dirname(HEADER), "..", "openpsg_amd", "csrc", "build.py")).read()
    assert '"psg_batch_gemm_b3.hip"' in src


def test_the_wrapper_checks_its_arguments_before_the_library():
    from openpsg_amd import ops
    x3, w = torch.zeros((3, 40, 64), dtype=torch.bfloat16), torch.zeros((16, 64), dtype=torch.bfloat16)
    for call, match in ((lambda: ops.batch_split_gemm_wb16(x3.half(), w), "bf16 planes"),
                        (lambda: ops.batch_split_gemm_wb16(x3[:2], w), "bf16 planes"),
                        (lambda: ops.batch_split_gemm_wb16(x3, w.half()), "w must be contiguous bf16"),
                        (lambda: ops.batch_split_gemm_wb16(x3, w[:, :32]), r"w must be contiguous bf16 \[N, 64\]"),
                        (lambda: ops.batch_split_gemm_wb16(x3, w), "HBM")):
        with pytest.raises(PsgHipError, match=match):
            call()


def test_the_routing_lookup():
    from openpsg_amd import llm
    assert isinstance(llm._BATCH_WB16_LIBRARY, dict)
    for (N, K), ranges in llm._BATCH_WB16_LIBRARY.items():
        assert N % 16 == 0 and K % 64 == 0 and all(33 <= lo < hi <= 161 for lo, hi in ranges)
    table = {(4096, 4096): [(33, 65), (97, 161)]}
    route = lambda rows, N=4096, K=4096: llm._batch_wb16_route(N, K, rows, table)      # noqa: E731
    assert [route(r) for r in (33, 64, 65, 96, 97, 160)] == ["library", "library", "own", "own", "library", "library"]
    assert route(40, N=12288) == "own" and route(40, K=11008) == "own"
    assert llm._batch_wb16_route(4096, 4096, 40, {}) == "own"


# ---- the loader ---------------------------------------------------------------------------------------------------------
def _matrix(N, K, seed):
    return bf16_valued((N, K), torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("src", ("fp32 tensors of bf16 values", "torch.bfloat16 tensors", "one of each"))
def test_a_record_holds_the_bf16_copy_only(src):
    q, k, v = _matrix(64, 128, 1), _matrix(32, 128, 2), _matrix(32, 128, 3)
    parts = {"fp32 tensors of bf16 values": (q, k, v), "torch.bfloat16 tensors": (q.bfloat16(), k.bfloat16(), v.bfloat16()),
             "one of each": (q, k.bfloat16(), v)}[src]
    weights = dict(zip("qkv", parts))
    for chunk in (1 << 22, 128 * 5, 1):                                      # one chunk / chunks of 5 rows / of one row
        rec = LM.load_bf16_matrix(weights, ("q", "k", "v"), "cpu", torch.float32, chunk_elems=chunk)
        assert isinstance(rec, LM.LlmMatrix) and rec.w is None and rec.split is None and rec.packed is None and rec.w16 is None
        assert rec.fmt is None and tuple(rec.shape) == (128, 128) and rec.dtype == torch.float32
        assert rec.wb16.dtype == torch.bfloat16 and rec.wb16.is_contiguous()
        assert torch.equal(rec.wb16.view(torch.int16), torch.cat([q, k, v]).bfloat16().view(torch.int16))
        assert rec.tensors() == [rec.wb16] and rec.quant_tensors() == []
        LM.complete([rec], rec, torch.float32, prefill_split=True, llm_w16=True, bf16_value_stream=True, batch_split_gemm=True)
        assert rec.w is None and rec.split is None and rec.packed is None and rec.w16 is None    # (nothing is added)
        assert rec.stream[0] == "wb16" and len(rec.stream[1]) == 1 and rec.stream[1][0] is rec.wb16


def test_a_matrix_that_is_no_bf16_value_is_named_and_nothing_is_kept():
    q, k = _matrix(64, 128, 1), _matrix(32, 128, 2)
    v = k.clone()
    v[17, 5] = 1.0 + 2.0 ** -12                                              # one element, in the middle of a chunk
    for chunk in (1 << 22, 128 * 5):
        assert LM.load_bf16_matrix(dict(q=q, k=k, v=v), ("q", "k", "v"), "cpu", torch.float32, chunk_elems=chunk) == "v"
        assert LM.load_bf16_matrix(dict(q=v, k=k), ("q", "k"), "cpu", torch.float32, chunk_elems=chunk) == "q"
    with pytest.raises(PsgHipError, match="same K"):
        LM.load_bf16_matrix(dict(q=q, k=k[:, :64]), ("q", "k"), "cpu", torch.float32)


def test_the_chunked_check_equals_the_one_shot_check():
    g = torch.Generator().manual_seed(5)
    good = _matrix(67, 96, 4)
    bad_last, bad_first = good.clone(), good.clone()
    bad_last[66, 95] = 3.0 + 2.0 ** -20
    bad_first[0, 0] = 3.0 + 2.0 ** -20
    generic = torch.randn(67, 96, generator=g)
    for t in (good, bad_last, bad_first, generic, good.bfloat16(), good.half().float(), good[:, :1], good[:1]):
        one_shot = bool(torch.equal(t.bfloat16().float(), t.float()))
        for chunk in (1 << 22, 96 * 7, 96, 1):
            assert LM.bf16_valued(t, chunk) == one_shot
    assert LM.bf16_valued(torch.full((4, 4), float("nan")).bfloat16())      # (already bf16: passes without a look)
    assert not LM.bf16_valued(torch.full((4, 4), float("nan")))             # (as `complete`'s test: NaN != NaN)


def _tiny_model(seed=7):
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.weights import make_weights_numpy
    cfg = PSGConfig(qformer=QFormerConfig(vocab=30522), llm=tiny_llm(128, 2, 256, 64), max_object_num=50)
    w = {k: torch.as_tensor(v) for k, v in make_weights_numpy(cfg, seed).items()}
    return cfg, {k: (v.bfloat16().float() if k.startswith("language_model.") and v.dim() >= 2 else v) for k, v in w.items()}


def test_the_engine_refuses_a_decoder_matrix_that_is_no_bf16_value(monkeypatch):
    """The refusal names the option and the first such matrix, says how many there are and what runs them.  (The split image
    of `language_projection` is a kernel: a stand-in lets the constructor reach the decoder layers on the CPU.)"""
    from openpsg_amd import llm, ops
    monkeypatch.setattr(ops, "split_f16x3", lambda x, weights=False: (torch.zeros(x.shape[0], 3 * x.shape[1], dtype=torch.float16),
                                                                     torch.ones(x.shape[0])))
    cfg, w = _tiny_model()
    first, second = "language_model.model.layers.0.mlp.up_proj.weight", "language_model.model.layers.1.self_attn.o_proj.weight"
    for k in (first, second):
        w[k] = w[k] + 2.0 ** -20
    w["language_model.lm_head.weight"] = w["language_model.lm_head.weight"] + 2.0 ** -20       # (the lm_head may be anything)
    with pytest.raises(PsgHipError) as e:
        llm.LlamaDecodeEngine(w, cfg, "cpu", torch.float32, prefill_split=True, bf16_value_stream=True, bf16_value_resident=True)
    msg = str(e.value)
    assert "llm_bf16_value_resident" in msg and first in msg and second not in msg
    assert "2 decoder matrices are not bf16 values" in msg and "llm_bf16_value_resident=False runs them" in msg


def test_an_lm_head_that_is_no_bf16_value_keeps_its_fp32_tensor():
    """... and today's routes: the record `load_matrix` makes, which `complete` leaves without a copy."""
    cfg, w = _tiny_model()
    name = "language_model.lm_head.weight"
    w[name] = w[name] + 2.0 ** -20
    assert LM.load_bf16_matrix(w, (name,), "cpu", torch.float32) == name
    head = LM.load_matrix(w, (name,), "cpu", torch.float32, False, True)
    layer = LM.load_bf16_matrix(w, ("language_model.model.layers.0.self_attn.o_proj.weight",), "cpu", torch.float32)
    LM.complete([layer], head, torch.float32, prefill_split=True, bf16_value_stream=True)
    assert head.w is not None and head.w.dtype == torch.float32 and torch.equal(head.w, w[name])
    assert head.wb16 is None and head.stream is None and layer.stream[0] == "wb16"


def test_a_quantised_matrix_is_refused_before_anything_is_loaded():
    from openpsg_amd import llm
    from openpsg_amd.weights import SCALE_SUFFIX
    cfg, w = _tiny_model()
    name = "language_model.lm_head.weight"
    w[name + SCALE_SUFFIX] = torch.ones(w[name].shape[0])
    with pytest.raises(PsgHipError, match=f"bf16_value_resident: {name} is quantised.*llm_weight_resident='quantised'"):
        llm.LlamaDecodeEngine(w, cfg, "cpu", torch.float32, prefill_split=True, bf16_value_stream=True, bf16_value_resident=True)


def test_a_bf16_only_record_takes_fp32_rows_only():
    from openpsg_amd.llm import LlamaDecodeEngine
    rec = LM.load_bf16_matrix(dict(o=_matrix(64, 128, 1)), ("o",), "cpu", torch.float32)
    for x in (torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(4, 128, dtype=torch.float16), torch.zeros(2, 4, 128)):
        with pytest.raises(PsgHipError, match="o: held as its bf16 copy only.*takes fp32 rows"):
            LlamaDecodeEngine._linear_b3(None, x, rec)
    with pytest.raises(PsgHipError, match="o: held as its bf16 copy only.*no dense operand"):
        LlamaDecodeEngine._dense(None, rec)


def _engine_facts(**over):
    """What `_wb16_blockers` reads of an engine, for a model on which the route is open."""
    from types import SimpleNamespace as NS
    facts = dict(layer_kind="wb16", prefill_split=True, dtype=torch.float32, use_skinny=True, qkv_width=1536,
                 hidden=512, inter=1024, shapes=[(1536, 512), (512, 512), (2048, 512), (512, 1024)])
    facts.update(over)
    eng = NS(cfg=NS(llm=NS(hidden=facts.pop("hidden"), inter=facts.pop("inter"))),
             _layer_mats=lambda shapes=facts.pop("shapes"): [NS(shape=sh) for sh in shapes], **facts)
    return eng


@pytest.mark.parametrize("over,rows,why", (
        (dict(layer_kind=None), 1, "the decoder layers are of kind None, not bf16 copies"),
        (dict(prefill_split=False), 1, "not an fp32s engine"),
        (dict(dtype=torch.bfloat16), 1, "not an fp32s engine"),
        (dict(use_skinny=False), 1, "use_skinny is off"),
        (dict(), 33, "33 rows exceed the 32"),
        (dict(hidden=544), 1, "hidden = 544 is no multiple of 64"),
        (dict(inter=992), 1, "inter = 992 is no multiple of 64"),
        (dict(hidden=8320), 1, "hidden = 8320 exceeds 8192"),
        (dict(qkv_width=1544), 1, "q|k|v width 1544 is no multiple of 16"),
        ("table", 1, r"shape \[\(512, 1024\)\] is listed in WB16_STREAM_OFF")))
def test_every_condition_of_the_wb16_route_is_named_and_refuses_a_resident_engine(over, rows, why, monkeypatch):
    """`_can_wb16` and the constructor's refusal read ONE list: each condition closes the route, and a resident engine raises
    with that condition and the remedy."""
    import re
    from openpsg_amd import llm
    E = llm.LlamaDecodeEngine
    if over == "table":
        monkeypatch.setattr(llm, "WB16_STREAM_OFF", frozenset({(512, 1024)}))
        over = {}
    eng = _engine_facts(**over)
    eng._wb16_blockers = lambda r: E._wb16_blockers(eng, r)
    reasons = eng._wb16_blockers(rows)
    assert len(reasons) == 1 and re.search(why, reasons[0]) and not E._can_wb16(eng, rows)
    if rows == 1:
        with pytest.raises(PsgHipError, match=f"cannot stream the bf16 copies.*{why}.*llm_bf16_value_resident=False"):
            E._check_resident_routes(eng)


def test_an_open_route_refuses_nothing():
    from openpsg_amd.llm import LlamaDecodeEngine as E
    eng = _engine_facts()
    eng._wb16_blockers = lambda r: E._wb16_blockers(eng, r)
    assert E._wb16_blockers(eng, 1) == [] and E._wb16_blockers(eng, 32) == [] and E._can_wb16(eng, 20)
    E._check_resident_routes(eng)


# ---- the arithmetic -----------------------------------------------------------------------------------------------------
def test_the_stacked_three_plane_product_in_the_fixed_order_is_fp32_grade():
    """A torch model of `_stacked_b3` and its readers: the planes stacked [x2; x1; x0], ONE product of 3 x rows rows against
    the bf16 values with fp32 accumulation, the slices added in slot order = (y2 + y1) + y0.  Rows 1e-6 .. 1e3, weights bf16
    values over 2^-30 .. 2^3."""
    g = torch.Generator().manual_seed(11)
    rows, K, N = 37, 512, 96
    x = wide_rows(rows, K, g)
    w = bf16_valued((N, K), g)
    assert torch.equal(w.bfloat16().float(), w)
    p = split_b16x3(x)
    stacked = p.flip(0).reshape(3 * rows, K)
    assert torch.equal(stacked[:rows], p[2]) and torch.equal(stacked[2 * rows:], p[0])
    y = (stacked.float() @ w.t()).view(3, rows, N)                           # exact products, fp32 accumulation
    got = (y[0] + y[1]) + y[2]                                               # slot order: (y2 + y1) + y0
    ref = x.double() @ w.double().t()
    bound = x.double().abs() @ w.double().abs().t()
    worst = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"stacked three-plane product, (y2 + y1) + y0: worst |got - ref| / (|x| @ |w|^T) = {worst:.3e} (bar {BAR:.0e})")
    assert ((got.double() - ref).abs() <= BAR * bound + 1e-300).all()
    # the planes are the rows exactly, so in float64 the three slices sum to the product itself
    y64 = (stacked.double() @ w.double().t()).view(3, rows, N)
    assert torch.allclose(y64.sum(0), ref, rtol=1e-12, atol=0)
