"""The LLM option matrix without a GPU (tests/test_gpu_llm_option_matrix.py is the GPU side).

(1) The precondition of the matrix's comparisons.  They hold tokens to the oracle "up to each pair's first near-tie" and ask
that at least 90 % of the paths are compared whole, which means something only if the reference ALONE stays clear of
near-ties: for every (case, weight variant) the matrix decodes on, the constrained walk of the fp32 oracle on W' over the
oracle's own LLM inputs has at most 10 % of its pairs with a child top-2 margin under NEAR_TIE at any step.
(2) Every option combination the matrix builds is accepted by the constructor, and the combinations refused by design keep
their message."""
import numpy as np
import pytest
import torch

from openpsg_amd._lib import PsgHipError
from tests import llm_matrix_ref as M
from tests.test_gpu_llm_constrained import NEAR_TIE, _oracle_walk

_INPUTS = {}


def _case(case):
    """(g, cfg, w, trie, X, seq_len) of a golden case: loaded and run through the oracle's relation query once."""
    if case not in _INPUTS:
        g, cfg, w, scene = M.load(case)
        _INPUTS[case] = (g, cfg, w, M.relation_trie(cfg)) + M.oracle_llm_inputs(g, cfg, w, scene)
    return _INPUTS[case]


@pytest.mark.parametrize("case,fmt,lm_head", M.VARIANTS)
def test_the_oracle_on_the_dequantised_model_stays_clear_of_near_ties(case, fmt, lm_head):
    g, cfg, w, trie, X, seq_len = _case(case)
    wq = M.dequantised({k: v.clone() for k, v in w.items()}, cfg.llm.layers, fmt, lm_head)
    with torch.no_grad():
        tokens, logp, margin = _oracle_walk(cfg, wq, X, seq_len, trie)
    K = tokens.shape[0]
    near = int((margin < NEAR_TIE).any(1).sum())
    paths = len({tuple(t) for t in tokens.tolist()})
    print(f"{case} {fmt}{' + lm_head' if lm_head else ''}: {near} of {K} pairs with a near-tie, min child margin "
          f"{margin.min():.3e}, {paths} distinct paths")
    assert K == 20 and np.isfinite(logp).all() and (logp < 0).all()
    cands = {tuple(c) for c in trie.candidates}
    assert all(tuple(int(t) for t in row if t >= 0) in cands for row in tokens)   # the reference itself walks the trie
    assert near <= 0.1 * K


def _head(**kw):
    from openpsg_amd.config import tiny_llm
    from openpsg_amd.head import RelationTransformerHeadV4
    kw.setdefault("dtype", "fp32s")
    return RelationTransformerHeadV4(device="cpu", qformer_vocab_size=512, llm_config=tiny_llm(256, 2, 512, 512),
                                     llm_feature_size=256, tokenizers="word", on_parse_error="skip", **kw)


_QUANT = [dict(llm_weight_quant=f, llm_quantize_lm_head=h) for f in M.FORMATS for h in (False, True)]
ACCEPTED = (
    # A: constrained (+ likelihood) on every stream, fp32s and the single-form route of `mixed`
    [dict(q, llm_decode="constrained", llm_rel_scores=s) for q in _QUANT for s in ("constant", "likelihood")]
    + [dict(dtype="mixed", llm_weight_quant=f, llm_decode="constrained", llm_rel_scores=s) for f in M.FORMATS
       for s in ("constant", "likelihood")]
    # B: the likelihood pass, every matrix resident
    + [dict(llm_weight_quant=f, llm_weight_resident="all", llm_rel_scores="likelihood", llm_decode=d) for f in M.FORMATS
       for d in ("greedy", "constrained")]
    # C, D: the persistent decoder layer (fp32) and the fused route (bf16) read context options, not keywords
    + [dict(dtype="fp32", llm_decode="constrained", llm_rel_scores="likelihood"),
       dict(dtype="bf16", llm_decode="constrained", llm_rel_scores="likelihood")]
    # E: above 32 rows
    + [dict(llm_decode="constrained", llm_batch_split_gemm="own"),
       dict(llm_decode="constrained", llm_weight_quant="fp8", llm_batch_weight_stream="quantised"),
       dict(llm_decode="constrained", llm_weight_quant="mxfp4", llm_batch_weight_stream="quantised")]
    # the reference heads: option off
    + [dict(llm_decode="constrained"), dict(llm_rel_scores="likelihood"), dict()])


@pytest.mark.parametrize("kw", ACCEPTED, ids=lambda kw: ",".join(f"{k[4:] if k.startswith('llm_') else k}={v}"
                                                                  for k, v in kw.items()) or "defaults")
def test_every_combination_of_the_matrix_is_accepted(kw):
    h = _head(**kw)
    assert h.llm_decode == kw.get("llm_decode", "greedy") and h.llm_rel_scores == kw.get("llm_rel_scores", "constant")
    assert h.llm_weight_quant == kw.get("llm_weight_quant")
    if h.llm_decode == "constrained":
        assert h.relation_trie().key == M.relation_trie(h.cfg).key      # the trie the CPU precondition walks


REFUSED = [
    (dict(llm_weight_quant="int4g", llm_weight_resident="quantised", llm_decode="constrained"),
     r"llm_weight_resident='quantised' is not built for the INT4 format.*use llm_weight_resident='all'"),
    (dict(llm_weight_quant="int4g", llm_batch_weight_stream="quantised", llm_decode="constrained"),
     r"llm_batch_weight_stream='quantised' is not built for the INT4 format.*use llm_batch_weight_stream='dense'"),
    (dict(llm_batch_weight_stream="quantised", llm_decode="constrained"),
     r"llm_batch_weight_stream='quantised' streams a quantised LLM's bytes: set llm_weight_quant="),
] + [(dict(llm_bf16_value_stream=True, llm_weight_quant=f, llm_decode="constrained"),
      rf"llm_bf16_value_stream=True streams the UNQUANTISED.*llm_weight_quant='{f}'.*set one of the two") for f in M.FORMATS] + [
    (dict(q, llm_decode="constrained", suppress_eos=True),
     r"llm_decode='constrained' cannot run with suppress_eos=True") for q in [dict()] + _QUANT[:1]]


@pytest.mark.parametrize("kw,message", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_combinations_refused_by_design_keep_their_message(kw, message):
    with pytest.raises(PsgHipError, match=message):
        _head(**kw)
