"""llm_weight_quant='mxfp4' through the whole head (`-m gpu`).  An MXFP4-quantised LLM is a model whose matrices
ARE W' = fp4(q) * 2^(e - 127) * s, so - as for FP8 (tests/test_gpu_llm_w8.py, whose helpers and bars these are) - the head
with the option is held to a head WITHOUT the option that was loaded with W' and to the CPU oracle on W', never to the
original weights.  Tokens are compared per (pair, step) up to a pair's first near-tie (top-2 margin under 1e-3 in the
option-off head)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import llm_matrix_ref as M
from tests.test_gpu_llm_w8 import _assert_tokens_agree, _decode, _head, _step_margins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dequantised(w, n_layers, lm_head=False):
    """The dict an option-off head (or the oracle) needs to compute the SAME model: W' in fp32 for every quantised matrix."""
    from openpsg_amd.weights import dequantize_mxfp4_rows, llm_quant_keys, quantize_llm_weights
    wq = quantize_llm_weights(w, n_layers, lm_head, fmt="mxfp4")
    for k in llm_quant_keys(n_layers, lm_head):
        wq[k] = dequantize_mxfp4_rows(wq[k], wq.pop(k + "_bexp"), wq.pop(k + "_scale"))
    return wq


def _spy(monkeypatch):
    from openpsg_amd import ops
    calls = {"split_gemm_w4": 0, "skinny_gemm_w4": 0, "split_gemm_w8": 0, "skinny_gemm_w8": 0}
    for fn in calls:
        def wrapped(*a, _f=getattr(ops, fn), _n=fn, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrapped)
    return calls


def _fp32s_pair(case, loader, monkeypatch, lm_head=False):
    g, cfg, w, scene = loader(case)
    sup = bool(g["suppress_eos"])
    ref = _head(cfg, _dequantised(w, cfg.llm.layers, lm_head), "fp32s", suppress_eos=sup)
    assert set(M.formats(ref.llm_engine)) == {None}
    rq0, dec0 = _decode(ref, g, scene)
    margins = _step_margins(ref, dec0, sup)
    t0, f0 = np.asarray(dec0["tokens_host"]).copy(), dec0["first_logits"].float().cpu()
    e0 = rq0["exist_logit"].clone()
    del ref, rq0, dec0
    torch.cuda.empty_cache()
    calls = _spy(monkeypatch)
    head = _head(cfg, w, "fp32s", suppress_eos=sup, llm_weight_quant="mxfp4", llm_quantize_lm_head=lm_head)
    eng = head.llm_engine
    assert eng.layer_kind == "w4" and M.formats(eng).count("mxfp4") == 4 * len(eng.layers) + int(lm_head) and not eng._w16
    assert all(rec.split is None for rec in eng.matrices())                                    # no 6-byte split copies
    assert not eng.decode_uses_library(20) and not eng._can_persist(20, 0) and not eng._can_fuse(20)
    rq, dec = _decode(head, g, scene)
    assert calls["split_gemm_w4"] > 0 and calls["skinny_gemm_w4"] == 0
    assert calls["split_gemm_w8"] == 0 and calls["skinny_gemm_w8"] == 0     # (llm.W4_STREAM_AS_FP8 names none of these shapes)
    assert torch.equal(rq["exist_logit"], e0)                                # the relation query never sees the option
    d = (dec["first_logits"].float().cpu() - f0).abs().max().item()
    print(f"{case} fp32s: first-step logits, option on vs off on W': {d:.3e}")
    assert d < 1e-4
    _assert_tokens_agree(case, np.asarray(dec["tokens_host"]), t0, margins)
    return g, cfg, w, scene, dec


def test_g6_fp32s_agrees_with_the_option_off_head_and_the_oracle_on_the_same_model(monkeypatch):
    """(a) G6 (Llama-2-7B width, 2 layers, 20 pairs), fp32s: first-step logits within 1e-4 of the option-off head on W',
    tokens equal up to each pair's first near-tie with >= 90 % of the entries compared, graph replay identical, existence
    logits bit-equal, no split copies, split_gemm_w4 called and skinny_gemm_w4 not.  (b) the CPU oracle on W': first-step
    logits within 1e-3.  Both bars are the FP8 test's."""
    from oracle import psg_oracle as O
    g, cfg, w, scene, dec = _fp32s_pair("G6_llm_7b_width_n6", H.load_case, monkeypatch)
    wq = _dequantised(w, cfg.llm.layers)
    sel = g["selected"].tolist()
    qids, qmask = H.qformer_prompts(scene)
    pids, pmask = H.llm_prompts(scene, sel)
    fl = dec["first_logits"].float().cpu()
    worst = 0.0
    with torch.no_grad():
        orq = O.relation_query(wq, cfg, scene["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                               scene["pan_results"], qids, qmask)
        for i, si in enumerate(sel):
            x, mask = O.llm_inputs(wq, orq["pair_feature"][si], pids[i], pmask[i])
            _, lg = O.llm_generate(wq, cfg, x, mask, max_new_tokens=1, suppress_eos=bool(g["suppress_eos"]))
            ref = lg[0]
            keep = torch.isfinite(ref)
            worst = max(worst, (fl[i][keep] - ref[keep]).abs().max().item())
    print(f"G6 fp32s + mxfp4 against the oracle on W': first-step logits {worst:.3e}")
    assert worst < 1e-3


def test_g8_grouped_query_fp32s(monkeypatch):
    """G8 (4 query / 2 key-value heads: k / v projections of kv_heads x 128 rows) in fp32s, the checks of (a); the lm_head
    quantised as well."""
    from tests.test_gpu_gqa_head import load_gqa_case
    _fp32s_pair("G8_gqa_512_n10", load_gqa_case, monkeypatch, lm_head=True)


def test_g1_mixed_is_as_close_to_the_oracle_as_the_option_off_head(monkeypatch):
    """G1 in `mixed` against the CPU oracle on W': existence logits bit-equal to the option-off head, first-step logit
    error within twice what the option-off `mixed` head measures against the same oracle in this test."""
    from oracle import psg_oracle as O
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    sup = bool(g["suppress_eos"])
    wq = _dequantised(w, cfg.llm.layers)
    sel = g["selected"].tolist()
    qids, qmask = H.qformer_prompts(scene)
    pids, pmask = H.llm_prompts(scene, sel)
    refs = []
    with torch.no_grad():
        orq = O.relation_query(wq, cfg, scene["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                               scene["pan_results"], qids, qmask)
        for i, si in enumerate(sel):
            x, mask = O.llm_inputs(wq, orq["pair_feature"][si], pids[i], pmask[i])
            refs.append(O.llm_generate(wq, cfg, x, mask, max_new_tokens=1, suppress_eos=sup)[1][0])
    ref = torch.stack(refs)
    keep = torch.isfinite(ref)
    off = _head(cfg, wq, "mixed", suppress_eos=sup)
    rq0, dec0 = _decode(off, g, scene)
    err_off = (dec0["first_logits"].float().cpu() - ref)[keep].abs().max().item()
    calls = _spy(monkeypatch)
    on = _head(cfg, w, "mixed", suppress_eos=sup, llm_weight_quant="mxfp4")
    rq1, dec1 = _decode(on, g, scene)
    assert calls["skinny_gemm_w4"] > 0 and calls["split_gemm_w4"] == 0 and calls["skinny_gemm_w8"] == 0
    assert torch.equal(rq1["exist_logit"], rq0["exist_logit"])
    err_on = (dec1["first_logits"].float().cpu() - ref)[keep].abs().max().item()
    print(f"G1 mixed against the oracle on W': first-step logits option off {err_off:.3e}, mxfp4 {err_on:.3e}")
    assert err_on <= 2.0 * err_off
    # tokens: the caps of (a), against the option-off head's own near-ties
    margins = _step_margins(off, dec0, sup)
    _assert_tokens_agree("G1 mixed", np.asarray(dec1["tokens_host"]), np.asarray(dec0["tokens_host"]), margins)


def test_forward_batch_of_two_images_runs_on_the_dequantised_model(monkeypatch):
    """Routing: a <= 32-row decode calls the new entries; a forward_batch of 2 images (40 decode rows) does not, returns
    per-image results, and its tokens equal the single-image tokens up to each pair's first near-tie."""
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    sup = bool(g["suppress_eos"])
    head = _head(cfg, w, "mixed", suppress_eos=sup, llm_weight_quant="mxfp4")
    dev = torch.device(DEV)
    inputs = dict(mask_features=scene["mask_features"].to(dev), img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"].to(dev))])
    calls = _spy(monkeypatch)
    single = head(inputs)
    assert calls["skinny_gemm_w4"] > 0 and calls["skinny_gemm_w8"] == 0
    names = H.object_names(scene)
    rq = head.run_relation_query(scene["mask_features"].to(dev), scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                                 names, scene["pan_results"].to(dev))
    dec = head.decode_selected(rq, names)                                    # the single image's tokens, its own selection
    t1 = np.asarray(dec["tokens_host"]).copy()
    margins = _step_margins(head, dec, sup)
    n = dict(calls)
    res = head.forward_batch([inputs, inputs])
    assert calls == n                                                        # 40 rows: W' on the batch kernels / the library
    assert len(res) == 2 and all(set(r) == set(single) for r in res) and len(head.last_batch) == 2
    for i, lb in enumerate(head.last_batch):
        _assert_tokens_agree(f"forward_batch image {i}", np.asarray(lb["tokens_host"]), t1, margins)


def test_mxfp4_checkpoint_directory_through_the_constructor(tmp_path):
    """The MXFP4 checkpoint directory of tests/test_mxfp4_quant_cpu.py read by the head's constructor decodes the tokens of
    a head handed the same (q, e, s) through load_weights."""
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_numpy, read_hf_llama_weights
    from tests.test_mxfp4_quant_cpu import write_mxfp4_checkpoint
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 2, 512, 512), max_object_num=30)
    w = make_weights_numpy(cfg, seed=5)
    d = str(tmp_path / "mxfp4")
    write_mxfp4_checkpoint(d, cfg, w)
    kw = dict(dtype="fp32s", device=DEV, qformer_vocab_size=512, tokenizers="word", max_object_num=30, on_parse_error="skip",
              suppress_eos=True, llm_feature_size=256)
    a = RelationTransformerHeadV4(llm_model_name=d, **kw)                     # no option: the checkpoint IS quantised
    assert a.llm_engine.layer_kind == "w4" and a.llm_engine.lm_head_mat.fmt is None
    own = {k: v for k, v in w.items() if not k.startswith("language_model.")}
    a.load_state_dict(own, strict=False)
    b = RelationTransformerHeadV4(llm_config=cfg.llm, **kw)
    b.load_weights({**own, **read_hf_llama_weights(d)})
    scene = make_scene((512, 512), 6, seed=3, device=DEV)
    inputs = dict(mask_features=scene["mask_features"], img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"])])
    ra, rb = a(inputs), b(inputs)
    assert torch.equal(a.last["tokens"], b.last["tokens"]) and torch.equal(a.last["first_logits"], b.last["first_logits"])
    assert ra["rel_pred"] == rb["rel_pred"]
