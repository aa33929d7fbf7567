"""llm_weight_quant='fp8' through the whole head (`-m gpu`).  An FP8-quantised LLM is a model whose matrices ARE
W' = float32(q) * s, so the head with the option is held to the bars of the fp16-checkpoint mode: it agrees with a head
WITHOUT the option that was loaded with W' (today's generic-weights path on the same model) and with the CPU oracle on
W'.  Tokens are compared per (pair, step) up to a pair's first near-tie (top-2 margin under 1e-3 in the option-off head,
read from its own teacher-forced forward over the tokens it generated)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import llm_matrix_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dequantised(w, n_layers, lm_head=False):
    """The dict an option-off head (or the oracle) needs to compute the SAME model: W' in fp32 for every quantised matrix."""
    from openpsg_amd.weights import dequantize_fp8_rows, llm_quant_keys, quantize_llm_weights
    wq = quantize_llm_weights(w, n_layers, lm_head)
    for k in llm_quant_keys(n_layers, lm_head):
        wq[k] = dequantize_fp8_rows(wq[k], wq.pop(k + "_scale"))
    return wq


def _head(cfg, w, dtype, **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    h = RelationTransformerHeadV4(dtype=dtype, device=DEV, qformer_vocab_size=cfg.qformer.vocab, llm_config=cfg.llm,
                                  llm_feature_size=cfg.llm.hidden, tokenizers="word", max_object_num=cfg.max_object_num,
                                  on_parse_error="skip", **kw)
    h.load_weights(w)
    return h


def _decode(head, g, scene):
    dev = torch.device(DEV)
    names = H.object_names(scene)
    rq = head.run_relation_query(scene["mask_features"].to(dev), scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                                 names, scene["pan_results"].to(dev))
    sel = torch.from_numpy(g["selected"].astype(np.int32)).to(dev)
    dec = head.decode_selected(rq, names, selected=sel)
    dec2 = head.decode_selected(rq, names, selected=sel)                     # graph replay
    assert np.array_equal(dec["tokens_host"], dec2["tokens_host"])
    return rq, dec


def _step_margins(head, dec, suppress):
    """Top-2 logit margin of every (pair, step) of `head`'s own generation: one teacher-forced forward of its engine over
    [prompt, generated tokens] at generate's positions (slot == position).  [K, T] on the host; steps behind an EOS: inf."""
    eng = head.llm_engine
    X, plen = dec["llm_inputs"], dec["prompt_len"].to(torch.int64)
    toks = torch.as_tensor(np.asarray(dec["tokens_host"])).to(DEV).long()
    K, T = toks.shape
    n = plen + head.cfg.qformer.num_query                                    # valid prompt rows per pair
    S = X.shape[1] + T - 1
    Xe = torch.zeros((K, S, X.shape[2]), device=DEV, dtype=X.dtype)
    rows = []
    for k in range(K):
        nk = int(n[k])
        Xe[k, :nk] = X[k, :nk]
        Xe[k, nk:nk + T - 1] = eng.embed[toks[k, :T - 1].clamp(min=0)]
        rows += [k * S + nk - 1 + s for s in range(T)]
    rope = torch.arange(S, device=DEV, dtype=torch.int32).repeat(K)
    lg = eng.teacher_forcing_logits(Xe, (n + T - 1).to(torch.int32), rope, torch.tensor(rows, device=DEV)).float()
    if suppress:
        lg[:, head.cfg.llm.eos] = -float("inf")
    top = lg.topk(2, dim=-1).values
    margin = (top[:, 0] - top[:, 1]).view(K, T)
    return torch.where(toks >= 0, margin, torch.full_like(margin, float("inf"))).cpu().numpy()


def _assert_tokens_agree(name, got, ref, margins, need=0.9):
    """Per pair: every step before the first one whose margin (in the reference head) is under 1e-3 must match."""
    K, T = ref.shape
    compared = 0
    for k in range(K):
        tie = next((s for s in range(T) if margins[k, s] < 1e-3), T)
        compared += tie
        assert np.array_equal(got[k, :tie], ref[k, :tie]), f"{name}: pair {k} differs before its first near-tie (step {tie})"
    print(f"{name}: {compared} of {K * T} (pair, step) entries compared")
    assert compared >= need * K * T, f"{name}: only {compared} of {K * T} entries were comparable"


def _spy(monkeypatch):
    from openpsg_amd import ops
    calls = {"split_gemm_w8": 0, "skinny_gemm_w8": 0}
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
    assert "fp8" not in M.formats(ref.llm_engine)
    rq0, dec0 = _decode(ref, g, scene)
    margins = _step_margins(ref, dec0, sup)
    t0, f0 = np.asarray(dec0["tokens_host"]).copy(), dec0["first_logits"].float().cpu()
    e0 = rq0["exist_logit"].clone()
    del ref, rq0, dec0
    torch.cuda.empty_cache()
    calls = _spy(monkeypatch)
    head = _head(cfg, w, "fp32s", suppress_eos=sup, llm_weight_quant="fp8", llm_quantize_lm_head=lm_head)
    eng = head.llm_engine
    assert eng.layer_kind == "w8" and M.streams(eng).count("w8") == 4 * len(eng.layers) + int(lm_head) and not eng._w16
    assert all(rec.split is None for rec in eng.matrices())                                    # no 6-byte split copies
    assert not eng.decode_uses_library(20) and not eng._can_persist(20, 0) and not eng._can_fuse(20)
    rq, dec = _decode(head, g, scene)
    assert calls["split_gemm_w8"] > 0 and calls["skinny_gemm_w8"] == 0
    assert torch.equal(rq["exist_logit"], e0)                                # the relation query never sees the option
    d = (dec["first_logits"].float().cpu() - f0).abs().max().item()
    print(f"{case} fp32s: first-step logits, option on vs off on W': {d:.3e}")
    assert d < 1e-4
    _assert_tokens_agree(case, np.asarray(dec["tokens_host"]), t0, margins)
    return g, cfg, w, scene, dec


def test_g6_fp32s_agrees_with_the_option_off_head_and_the_oracle_on_the_same_model(monkeypatch):
    """(a) G6 (Llama-2-7B width, 2 layers, 20 pairs), fp32s: first-step logits within 1e-4 of the option-off head on W' (the
    bar of test_engine_streams_fp16_valued_weights_as_fp16), tokens equal up to each pair's first near-tie with >= 90 % of
    the entries compared, graph replay identical.  (b) the CPU oracle on W': first-step logits within 1e-3, the bound
    tests/test_gpu_llm7b.py holds the fp32 family to at this width."""
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
    print(f"G6 fp32s + fp8 against the oracle on W': first-step logits {worst:.3e}")
    assert worst < 1e-3


def test_g8_grouped_query_fp32s(monkeypatch):
    """(d) G8 (4 query / 2 key-value heads: k / v projections of kv_heads x 128 rows) in fp32s, the checks of (a); the
    lm_head quantised as well."""
    from tests.test_gpu_gqa_head import load_gqa_case
    _fp32s_pair("G8_gqa_512_n10", load_gqa_case, monkeypatch, lm_head=True)


def test_g1_mixed_is_as_close_to_the_oracle_as_the_option_off_head(monkeypatch):
    """(c) G1 in `mixed` against the CPU oracle on W': existence logits bit-equal to the option-off head, first-step logit
    error within twice what the option-off `mixed` head (library / 2-byte kernels on W' rounded to fp16) measures against
    the same oracle in this test."""
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
    on = _head(cfg, w, "mixed", suppress_eos=sup, llm_weight_quant="fp8")
    rq1, dec1 = _decode(on, g, scene)
    assert calls["skinny_gemm_w8"] > 0 and calls["split_gemm_w8"] == 0
    assert torch.equal(rq1["exist_logit"], rq0["exist_logit"])
    err_on = (dec1["first_logits"].float().cpu() - ref)[keep].abs().max().item()
    print(f"G1 mixed against the oracle on W': first-step logits option off {err_off:.3e}, fp8 {err_on:.3e}")
    assert err_on <= 2.0 * err_off


def test_forward_batch_of_two_images_runs_on_the_dequantised_model(monkeypatch):
    """(e) Routing: a <= 32-row decode calls the new entries (asserted in the tests above through the same spy); a
    forward_batch of 2 images (40 decode rows) does not, returns per-image results, and its tokens equal the single-image
    tokens up to each pair's first near-tie."""
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    sup = bool(g["suppress_eos"])
    head = _head(cfg, w, "mixed", suppress_eos=sup, llm_weight_quant="fp8")
    dev = torch.device(DEV)
    inputs = dict(mask_features=scene["mask_features"].to(dev), img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"].to(dev))])
    calls = _spy(monkeypatch)
    single = head(inputs)
    assert calls["skinny_gemm_w8"] > 0
    names = H.object_names(scene)
    rq = head.run_relation_query(scene["mask_features"].to(dev), scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                                 names, scene["pan_results"].to(dev))
    dec = head.decode_selected(rq, names)                                    # the single image's tokens, its own selection
    t1 = np.asarray(dec["tokens_host"]).copy()
    margins = _step_margins(head, dec, sup)
    n = calls["skinny_gemm_w8"]
    res = head.forward_batch([inputs, inputs])
    assert calls["skinny_gemm_w8"] == n and calls["split_gemm_w8"] == 0      # 40 rows: W' on the batch kernels / the library
    assert len(res) == 2 and all(set(r) == set(single) for r in res) and len(head.last_batch) == 2
    for i, lb in enumerate(head.last_batch):
        _assert_tokens_agree(f"forward_batch image {i}", np.asarray(lb["tokens_host"]), t1, margins)


def test_fp8_checkpoint_directory_through_the_constructor(tmp_path):
    """(f) The FP8 checkpoint directory of tests/test_fp8_quant_cpu.py read by the head's constructor decodes the tokens
    of a head handed the same (q, s) pairs through load_weights."""
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_numpy, read_hf_llama_weights
    from tests.test_fp8_quant_cpu import write_fp8_checkpoint
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 2, 512, 512), max_object_num=30)
    w = make_weights_numpy(cfg, seed=5)
    d = str(tmp_path / "fp8")
    write_fp8_checkpoint(d, cfg, w)
    kw = dict(dtype="fp32s", device=DEV, qformer_vocab_size=512, tokenizers="word", max_object_num=30, on_parse_error="skip",
              suppress_eos=True, llm_feature_size=256)
    a = RelationTransformerHeadV4(llm_model_name=d, **kw)                     # no option: the checkpoint IS quantised
    assert a.llm_engine.layer_kind == "w8" and a.llm_engine.lm_head_mat.fmt is None and a.llm_engine.lm_head_mat.fp8_img is None
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
