"""The launch trace of an fp32s decode step of <= 32 rows (`-m gpu`): which `ops` entries `LlamaDecodeEngine._steps` calls,
in which order and on which weight, on every weight stream and every stream the lm_head can have beside it.  The bit-level
tests of the routes (tests/test_gpu_w16.py, test_gpu_llm_w8.py / _w4.py / _int4.py, test_gpu_llm_bf16_stream.py) hold the
kernels' results; this one holds the Python that sequences them: same entries, same operands, same order - the same bits.

The expected sequences are written out below (`TWO_PLANE`, `THREE_PLANE`, `TAILS`, `CASES`), not derived from the engine.
Only names of `ops`, `_steps` and the head's keywords are used.

Model: the G1 golden case (2 decoder layers, 20 selected pairs), eager (`use_graph = False`)."""
import gc

import pytest
import torch

from tests import llm_matrix_ref as M
from tests.test_gpu_llm_rank import _head, _inputs

pytestmark = pytest.mark.gpu

ROW_OPS = ("rmsnorm", "rmsnorm_split2", "rmsnorm_split_b16x3", "split_f16x2", "split_b16x3", "silu_mul", "silu_mul_split_b16x3",
           "decode_attn", "greedy_step", "trie_greedy_step")
QKV, O, GU, DOWN, HEAD = "q|k|v", "o", "gate|up", "down", "lm_head"

# One decode step = FIRST NORM, then per decoder layer LAYER followed by the next layer's norm (the same entry as the first),
# then - behind the last layer - the tail: the lm_head's norm and the lm_head, and the greedy step.  "G" is the case's
# decoder-layer GEMM entry.
TWO_PLANE = dict(
    norm="rmsnorm_split2",
    layer=(("G", QKV), "decode_attn", "split_f16x2", ("G", O), "rmsnorm_split2", ("G", GU), "silu_mul", "split_f16x2",
           ("G", DOWN)))
THREE_PLANE = dict(
    norm="rmsnorm_split_b16x3",
    layer=(("G", QKV), "decode_attn", "split_b16x3", ("G", O), "rmsnorm_split_b16x3", ("G", GU), "silu_mul_split_b16x3",
           ("G", DOWN)))
# The norm behind the last layer takes the form of the stream the lm_head runs on
TAILS = {
    "pair": ("rmsnorm_split2", "H"),                       # two planes + the head's own pair-form entry "H"
    "b16x3": ("rmsnorm_split_b16x3", "split_gemm_wb16"),   # three planes: bf16-valued layers AND a bf16-valued head
    "fp32": ("rmsnorm", "skinny_gemm"),                    # the head has no 16-bit or quantised stream: its fp32 tensor
}

F16, BF16, GENERIC = "fp16 values", "bf16 values", "neither"
# id: (the decoder matrices' values, llm_weight_quant, llm_quantize_lm_head, the lm_head's values, llm_bf16_value_stream,
#      the step's form, the decoder-layer GEMM entry, the tail, the lm_head's GEMM entry)
CASES = {
    "w16": (F16, None, False, F16, False, TWO_PLANE, "split_gemm_w16", "pair", "split_gemm_w16"),
    "fp8+head": (GENERIC, "fp8", True, GENERIC, False, TWO_PLANE, "split_gemm_w8", "pair", "split_gemm_w8"),
    "fp8,fp16-head": (GENERIC, "fp8", False, F16, False, TWO_PLANE, "split_gemm_w8", "pair", "split_gemm_w16"),
    "fp8,fp32-head": (GENERIC, "fp8", False, GENERIC, False, TWO_PLANE, "split_gemm_w8", "fp32", "skinny_gemm"),
    "mxfp4+head": (GENERIC, "mxfp4", True, GENERIC, False, TWO_PLANE, "split_gemm_w4", "pair", "split_gemm_w4"),
    "mxfp4,fp16-head": (GENERIC, "mxfp4", False, F16, False, TWO_PLANE, "split_gemm_w4", "pair", "split_gemm_w16"),
    "int4g+head": (GENERIC, "int4g", True, GENERIC, False, TWO_PLANE, "split_gemm_int4", "pair", "split_gemm_int4"),
    "int4g,fp16-head": (GENERIC, "int4g", False, F16, False, TWO_PLANE, "split_gemm_int4", "pair", "split_gemm_w16"),
    "bf16,bf16-head": (BF16, None, False, BF16, True, THREE_PLANE, "split_gemm_wb16", "b16x3", "split_gemm_wb16"),
    "bf16,fp16-head": (BF16, None, False, F16, True, THREE_PLANE, "split_gemm_wb16", "pair", "split_gemm_w16"),
    "bf16,fp32-head": (BF16, None, False, GENERIC, True, THREE_PLANE, "split_gemm_wb16", "fp32", "skinny_gemm"),
}
LM_HEAD = "language_model.lm_head.weight"


def _expected_step(m, form, gemm, tail, head_gemm):
    shapes = {QKV: (m.hidden + 2 * m.kv_dim, m.hidden), O: (m.hidden, m.hidden), GU: (2 * m.inter, m.hidden),
              DOWN: (m.hidden, m.inter), HEAD: (m.vocab, m.hidden)}
    tail_norm, tail_gemm = TAILS[tail]
    step = [form["norm"]]
    for l in range(m.layers):
        step += [e if isinstance(e, str) else (gemm, shapes[e[1]]) for e in form["layer"]]
        step.append(form["norm"] if l + 1 < m.layers else tail_norm)
    return step + [(head_gemm if tail_gemm == "H" else tail_gemm, shapes[HEAD]), "greedy_step"]


def _valued(t, kind):
    """`t` as fp32 holding values of `kind`.  Element [0, 0] makes the kind unambiguous: 2^-30 is a bf16 value and no fp16
    value (below fp16's subnormal grid), 1 / 3 is neither."""
    t = torch.as_tensor(t).float().clone()
    if kind == F16:
        return t.half().float()
    if kind == BF16:
        t = t.bfloat16().float()
        t[0, 0] = 2.0 ** -30
        return t
    t[0, 0] = 1.0 / 3.0
    return t


def _weights(w, layers_kind, head_kind):
    out = dict(w)
    for k, v in w.items():
        if k.startswith("language_model.") and k.endswith("_proj.weight"):
            out[k] = _valued(v, layers_kind)
    out[LM_HEAD] = _valued(w[LM_HEAD], head_kind)
    return out


@pytest.fixture
def trace(monkeypatch):
    """The ordered calls of the spied `ops` entries made while `_steps` runs: a row kernel as its name, a GEMM as (name,
    (N, K) of its weight)."""
    from openpsg_amd import ops
    from openpsg_amd.llm import LlamaDecodeEngine
    gemms = tuple(n for n in dir(ops) if n.startswith(("split_gemm_", "skinny_gemm", "batch_")) and not n.endswith("_plan")
                  and callable(getattr(ops, n)))
    assert {"split_gemm_w16", "split_gemm_wb16", "split_gemm_w8", "split_gemm_w4", "split_gemm_int4", "skinny_gemm",
            "skinny_gemm_w8", "batch_gemm", "batch_split_gemm_w8"} <= set(gemms)
    log, state = [], {"in_steps": False}

    def weight_shape(name, a):
        # (x2, inv_scale, weight, ...) for the two-plane entries, (kind, x_out, weight, ...) for the fused one, else (x, weight, ...)
        third = name.startswith(("split_gemm_", "batch_split_gemm_", "skinny_gemm_fused")) and name != "split_gemm_wb16"
        w = a[2 if third else 1]
        return (int(w.shape[0]), int(a[0].shape[-1]) if torch.is_tensor(a[0]) else int(w.shape[1]))
    for fn in gemms + ROW_OPS:
        def wrapped(*a, _f=getattr(ops, fn), _n=fn, **kw):
            if state["in_steps"]:
                log.append((_n, weight_shape(_n, a)) if _n in gemms else _n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrapped)

    def in_steps(self, *a, _f=LlamaDecodeEngine._steps, **kw):
        state["in_steps"] = True
        try:
            return _f(self, *a, **kw)
        finally:
            state["in_steps"] = False
    monkeypatch.setattr(LlamaDecodeEngine, "_steps", in_steps)
    return log


@pytest.mark.parametrize("case", list(CASES))
def test_every_decode_step_is_the_written_out_sequence(case, trace):
    layers_kind, fmt, quant_head, head_kind, bf16, form, gemm, tail, head_gemm = CASES[case]
    g, cfg, w, scene = M.load(M.G1)
    assert cfg.llm.layers == 2
    kw = dict(llm_weight_quant=fmt, llm_quantize_lm_head=quant_head) if fmt is not None else {}
    head = _head(cfg, _weights(w, layers_kind, head_kind), "fp32s", suppress_eos=True, llm_bf16_value_stream=bf16, **kw)
    head.llm_engine.use_graph = False
    head(_inputs(scene))
    torch.cuda.synchronize()
    assert len(head.last["selected_host"]) == 20
    want = _expected_step(cfg.llm, form, gemm, tail, head_gemm)
    ends = [i + 1 for i, e in enumerate(trace) if e == "greedy_step"]
    steps = [trace[lo:hi] for lo, hi in zip([0] + ends, ends)]
    assert len(steps) == head.cfg.max_new_tokens - 1 and ends[-1] == len(trace), (len(steps), len(trace))
    for i, got in enumerate(steps):
        assert got == want, f"{case}: decode step {i + 1}:\n got  {got}\n want {want}"
    del head
    gc.collect()
    torch.cuda.empty_cache()
