"""Grouped-query attention LLMs through the whole head (`-m gpu`): the reference's goldens G8 (Llama, 4 query / 2 key-value
heads), G9 (Mistral-7B width, 32 / 8) and T4 (T1's training case with G8's LLM, tests/golden/, tools/capture_gqa_golden.py)
in every mode; the same head with its key / value weights expanded to multi-head; submit / forward_batch against forward;
a loopback world of 2 ranks; Llama and Mistral checkpoint directories through the constructor; the training gradients;
one 32-layer Mistral-7B-shaped model."""
import ast
import json
import os

import numpy as np
import pytest
import torch

from tests import gqa_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["G8_gqa_512_n10", "G9_mistral_width_n6"]
_W = {}


def _llm(g):
    from openpsg_amd.config import tiny_llm
    return tiny_llm(int(g["llm_hidden"]), int(g["llm_layers"]), int(g["llm_inter"]), int(g["llm_vocab"]),
                    kv_heads=int(g["llm_kv_heads"]))


def load_gqa_case(name):
    """G1 / G6-style case with the GQA config built from the fixture's `llm_kv_heads` (tests/helpers.py stays multi-head)."""
    from openpsg_amd.config import PSGConfig, QFormerConfig
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_numpy
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=_llm(g), max_object_num=30)
    if name not in _W:
        _W[name] = make_weights_numpy(cfg, seed=int(g["weight_seed"]))
    w = {k: v.clone() for k, v in _W[name].items()}
    scene = make_scene(**ast.literal_eval(str(g["scene_kw"])))
    assert np.array_equal(scene["pan_results"].numpy(), g["pan_results"])
    return g, cfg, w, scene


def expand_to_mha(cfg, w):
    """The multi-head model that computes the same function: each key / value head's rows repeated over its group."""
    import dataclasses
    m = cfg.llm
    wm = {k: (R.expand_kv_rows(v, m.kv_group) if k.endswith(("k_proj.weight", "v_proj.weight")) else v) for k, v in w.items()}
    return dataclasses.replace(cfg, llm=dataclasses.replace(m, kv_heads=None)), wm


def _head(cfg, w, dtype, **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    h = RelationTransformerHeadV4(dtype=dtype, device="cuda:0", qformer_vocab_size=cfg.qformer.vocab,
                                  llm_config=cfg.llm, llm_feature_size=cfg.llm.hidden, tokenizers="word",
                                  max_object_num=cfg.max_object_num, on_parse_error="skip", **kw)
    h.load_weights(w)
    return h


def _inputs(scene):
    return dict(mask_features=scene["mask_features"].cuda(), img_metas=[scene["img_meta"]],
                object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"].cuda())])


def _tokens(toks, i):
    return [int(t) for t in toks[i] if t >= 0]


# ---- goldens ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp32s"])
@pytest.mark.parametrize("case", CASES)
def test_gqa_golden_fp32_modes_vs_reference(case, dtype):
    """tests/test_gpu_parity.py's G6 bounds: existence logits within 1e-3, the reference's selection, identical greedy
    tokens, first-step logits at the reference's top 8 within 1e-3."""
    g, cfg, w, scene = load_gqa_case(case)
    head = _head(cfg, w, dtype, suppress_eos=bool(g["suppress_eos"]))
    assert head.llm_engine.kv == cfg.llm.n_kv_heads < cfg.llm.heads
    head(_inputs(scene))
    torch.cuda.synchronize()
    last = head.last
    err = np.abs(last["exist_logit"].cpu().numpy() - g["exist_logit"]).max()
    assert err < 1e-3, f"existence logits differ by {err:.3e}"
    assert last["selected"].cpu().tolist() == g["selected"].tolist()
    toks = last["tokens_host"]
    fl = last["first_logits"].float().cpu().numpy()
    worst = 0.0
    for i in range(toks.shape[0]):
        want = g["gen_tokens"][i]
        assert _tokens(toks, i) == want[want >= 0].tolist(), f"selected pair #{i}: greedy tokens differ from the reference"
        d = np.abs(fl[i][g["gen_top8_idx"][i]] - g["gen_top8_val"][i]).max()
        worst = max(worst, d)
        assert d < 1e-3, f"pair #{i}: first-step logits differ by {d:.3e}"
    print(f"{case} {dtype}: |exist logit| {err:.2e}, |first logits| {worst:.2e}, {toks.shape[0]} pairs token-exact")


@pytest.mark.parametrize("dtype", ["bf16", "mixed"])
@pytest.mark.parametrize("case", CASES)
def test_gqa_golden_16bit_modes_are_bounded(case, dtype):
    """16-bit GEMM operands: the bounds tests/test_gpu_parity.py applies to a bf16 head (existence logits within 0.25 of
    the reference, top-20 overlap >= 14); on the reference's selection the first-step logits at its top 8 stay within
    tests/test_gpu_bf16_path.py's floor (0.45), and the first greedy token is the reference's wherever the reference's
    top-2 margin exceeds that file's FLIP_MARGIN (1.0; logit std ~3) - later tokens may diverge after a near-tie."""
    g, cfg, w, scene = load_gqa_case(case)
    head = _head(cfg, w, dtype, suppress_eos=bool(g["suppress_eos"]))
    dev = torch.device("cuda:0")
    ids = [int(i) for i in scene["object_id_list"]]
    names = H.object_names(scene)
    rq = head.run_relation_query(scene["mask_features"].to(dev), scene["img_meta"], ids, names, scene["pan_results"].to(dev))
    dec = head.decode_selected(rq, names, selected=torch.from_numpy(g["selected"].astype(np.int32)).to(dev))
    torch.cuda.synchronize()
    err = np.abs(rq["exist_logit"].cpu().numpy() - g["exist_logit"]).max()
    overlap = len(set(rq["selected"].cpu().tolist()) & set(g["selected"].tolist()))
    fl = dec["first_logits"].float().cpu().numpy()
    eos = cfg.llm.eos
    d = max(np.abs(np.delete(fl[i][g["gen_top8_idx"][i]] - g["gen_top8_val"][i],
                             np.where(g["gen_top8_idx"][i] == eos)[0])).max() for i in range(fl.shape[0]))
    toks = dec["tokens_host"]
    exact = sum(_tokens(toks, i) == g["gen_tokens"][i][g["gen_tokens"][i] >= 0].tolist() for i in range(toks.shape[0]))
    print(f"{case} {dtype}: |exist logit| {err:.3f}, overlap {overlap}/20, |first logits| {d:.3f}, "
          f"{exact}/{toks.shape[0]} pairs token-exact")
    assert err < 0.25 and overlap >= 14
    assert d < 0.45
    for i in range(toks.shape[0]):
        margin = g["gen_top8_val"][i][0] - g["gen_top8_val"][i][1]
        if margin > 1.0:
            assert int(toks[i][0]) == int(g["gen_top8_idx"][i][0]), f"pair #{i}: first token flipped at margin {margin:.2f}"


# ---- other modes and entry points ---------------------------------------------------------------------------------
def test_gqa_equals_the_head_with_kv_expanded_to_mha():
    """The same model written as multi-head (each key / value head repeated over its group): identical tokens, fp32
    first-step logits within 1e-5 - the grouped kernels compute the multi-head function."""
    g, cfg, w, scene = load_gqa_case("G8_gqa_512_n10")
    cfg_m, w_m = expand_to_mha(cfg, w)
    a = _head(cfg, w, "fp32", suppress_eos=True)
    b = _head(cfg_m, w_m, "fp32", suppress_eos=True)
    assert a.llm_engine.kv == 2 and b.llm_engine.kv is None
    inp = _inputs(scene)
    a(inp)
    b(inp)
    torch.cuda.synchronize()
    assert torch.equal(a.last["exist_logit"], b.last["exist_logit"])
    assert np.array_equal(a.last["tokens_host"], b.last["tokens_host"])
    fa, fb = a.last["first_logits"].float(), b.last["first_logits"].float()
    rel = ((fa - fb).abs() / (1 + fb.abs())).max().item()
    assert rel <= 1e-5, f"first-step logits differ by {rel:.2e}"


def test_gqa_fp16_valued_weights_on_the_w16_path():
    """fp32s over fp16-valued LLM weights (two-plane prompt pass, psg_split_gemm_w16 decode steps, llm_w16): the GQA head
    equals the same model expanded to multi-head."""
    from openpsg_amd.weights import llm_matrices_as_fp16_values
    g, cfg, w, scene = load_gqa_case("G8_gqa_512_n10")
    w16 = llm_matrices_as_fp16_values(w)
    cfg_m, w_m = expand_to_mha(cfg, w16)
    a = _head(cfg, w16, "fp32s", suppress_eos=True)
    b = _head(cfg_m, w_m, "fp32s", suppress_eos=True)
    assert a.llm_engine._w16_all and b.llm_engine._w16_all and a.llm_engine._can_w16(20)
    inp = _inputs(scene)
    a(inp)
    b(inp)
    torch.cuda.synchronize()
    assert np.array_equal(a.last["tokens_host"], b.last["tokens_host"])
    fa, fb = a.last["first_logits"].float(), b.last["first_logits"].float()
    assert ((fa - fb).abs() / (1 + fb.abs())).max().item() <= 1e-5


@pytest.mark.parametrize("dtype", ["fp32", "fp32s", "bf16", "fp16", "mixed"])
def test_gqa_submit_and_forward_batch_equal_forward(dtype):
    """`submit` runs forward's kernels on a slot stream (tokens equal); `forward_batch` decodes the pairs of three images
    as one batch (60 rows: 33-160-row decode steps) - its tokens equal forward's up to the GEMM rounding of another row
    count, so most pairs are token-exact."""
    from openpsg_amd.synthetic import make_scene
    g, cfg, w, _ = load_gqa_case("G8_gqa_512_n10")
    head = _head(cfg, w, dtype, suppress_eos=True)
    scenes = [make_scene((512, 512), n, seed=70 + n, device="cuda:0", tiny_object=True) for n in (6, 9, 7)]
    ref = []
    for s in scenes:
        head(_inputs(s))
        torch.cuda.synchronize()
        ref.append(head.last["tokens_host"].copy())
    pend = [head.submit(_inputs(s), slot=i % 2) for i, s in enumerate(scenes[:2])]     # two images in flight
    for i, p in enumerate(pend):
        p.result()
        assert np.array_equal(head.last["tokens_host"], ref[i]), f"submit: image {i} decodes other tokens than forward"
    outs = head.forward_batch([_inputs(s) for s in scenes])
    torch.cuda.synchronize()
    assert len(outs) == 3 and len(head.last_batch) == 3
    same = n = 0
    for i in range(3):
        t = head.last_batch[i]["tokens_host"]
        assert t.shape == ref[i].shape
        same += int((t == ref[i]).all(axis=1).sum())
        n += t.shape[0]
    print(f"{dtype}: forward_batch {same}/{n} pairs token-exact with forward")
    assert same >= 0.8 * n, f"forward_batch: {same}/{n} pairs token-exact"


def test_gqa_loopback_world_2_equals_the_single_gpu_head():
    """Pair sharding (dist.py unchanged) over a loopback world of 2: fp32s with row-invariant projections, every
    probability and token bit-exact with the single-GPU head."""
    from openpsg_amd.dist import HipBackend, LoopbackWorld
    from openpsg_amd.synthetic import make_scene
    g, cfg, w, _ = load_gqa_case("G8_gqa_512_n10")
    head = _head(cfg, w, "fp32s", suppress_eos=True)
    head.llm_engine.row_invariant = True
    scene = make_scene((1024, 1024), 40, seed=4, device="cuda:0", tiny_object=True)
    head(_inputs(scene))
    torch.cuda.synchronize()
    prob, sel, toks = head.last["exist_prob"].clone(), head.last["selected"].clone(), head.last["tokens_host"].copy()
    fw = LoopbackWorld(2)
    outs = fw.run([p.step_one_image_gen(scene if r == 0 else None) for r, p in enumerate(fw.pipelines(HipBackend(head)))])
    torch.cuda.synchronize()
    for r in range(2):
        assert torch.equal(outs[r]["exist_prob"], prob)
        assert torch.equal(outs[r]["selected"], sel)
        assert np.array_equal(outs[r]["tokens"].cpu().numpy(), toks)


@pytest.mark.parametrize("model_type", ["llama", "mistral"])
def test_gqa_checkpoint_directory_through_the_constructor(tmp_path, model_type):
    """A grouped-query checkpoint directory (fp16 safetensors) loads through the head's constructor and decodes what a
    head handed the same tensors decodes."""
    from safetensors.torch import save_file
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_scene
    g, cfg, w, _ = load_gqa_case("G8_gqa_512_n10")
    m = cfg.llm
    c = dict(architectures=["MistralForCausalLM" if model_type == "mistral" else "LlamaForCausalLM"], model_type=model_type,
             hidden_size=m.hidden, num_attention_heads=m.heads, num_key_value_heads=m.n_kv_heads, num_hidden_layers=m.layers,
             intermediate_size=m.inter, vocab_size=m.vocab, rms_norm_eps=m.rms_eps, rope_theta=m.rope_theta,
             bos_token_id=m.bos, eos_token_id=m.eos, torch_dtype="float16", tie_word_embeddings=False, hidden_act="silu")
    if model_type == "mistral":
        c["sliding_window"] = 4096
    d = str(tmp_path / model_type)
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(c, f)
    save_file({k[len("language_model."):]: v.half().contiguous() for k, v in w.items() if k.startswith("language_model.")},
              os.path.join(d, "model.safetensors"))
    kw = dict(dtype="fp32s", device="cuda:0", qformer_vocab_size=512, llm_feature_size=m.hidden, tokenizers="word",
              max_object_num=30, on_parse_error="skip", suppress_eos=True)
    a = RelationTransformerHeadV4(llm_model_name=d, **kw)
    assert a.cfg.llm == m and a.llm_engine.kv == m.n_kv_heads and a.llm_engine._w16_all
    a.load_state_dict({k: v for k, v in w.items() if not k.startswith("language_model.")}, strict=False)
    b = RelationTransformerHeadV4(llm_config=m, **kw)
    b.load_weights({k: (v.half().float() if k.startswith("language_model.") else v) for k, v in w.items()})   # fp16 on disk
    scene = make_scene((512, 512), 6, seed=3, device="cuda:0")
    a(_inputs(scene))
    b(_inputs(scene))
    torch.cuda.synchronize()
    assert np.array_equal(a.last["tokens_host"], b.last["tokens_host"])
    assert torch.equal(a.last["first_logits"], b.last["first_logits"])


# ---- training -----------------------------------------------------------------------------------------------------
def _train_case():
    from openpsg_amd.config import PSGConfig, QFormerConfig
    from openpsg_amd.synthetic import make_train_scene
    from openpsg_amd.weights import make_weights_numpy
    g = dict(np.load(os.path.join(GOLDEN, "T4_gqa_train_512_n7.npz"), allow_pickle=False))
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=_llm(g), max_object_num=30)
    w = make_weights_numpy(cfg, seed=int(g["weight_seed"]))
    inputs = make_train_scene(tuple(int(v) for v in g["pad_hw"]), [int(c) for c in g["categories"]],
                              [tuple(int(v) for v in r) for r in g["gt_rels"]], seed=int(g["scene_seed"]))
    return g, cfg, w, inputs


def _to_dev(inputs):
    out = dict(inputs)
    out["mask_features"] = inputs["mask_features"].cuda()
    out["gt_semantic_seg"] = [inputs["gt_semantic_seg"][0].cuda()]
    return out


def _train_head(cfg, w):
    from openpsg_amd.head import RelationTransformerHeadV4
    h = RelationTransformerHeadV4(dtype="fp32", device="cuda:0", qformer_vocab_size=cfg.qformer.vocab, llm_config=cfg.llm,
                                  llm_feature_size=cfg.llm.hidden, tokenizers="word", max_object_num=cfg.max_object_num,
                                  train_dropout=False)
    h.load_weights(w)
    h.train(True)
    return h


def test_gqa_training_losses_vs_reference():
    """T4 (T1's draws, G8's LLM): tests/test_gpu_train.py's bounds on both losses, through forward_train (the engine's
    prompt pass on psg_rope_kvwrite_gqa / psg_llm_attn_gqa)."""
    g, cfg, w, inputs = _train_case()
    head = _train_head(cfg, w)
    out = head.forward_train(_to_dev(inputs), sampled=g["sampled"], selected=g["selected"].tolist())
    torch.cuda.synchronize()
    e_logit = np.abs(head.last["bce_logit"].cpu().numpy() - g["bce_logit"]).max()
    e_bce = abs(float(out["binary_rel_cls_loss"]) - float(g["binary_rel_cls_loss"]))
    e_llm = abs(float(out["rel_llm_loss"]) - float(g["rel_llm_loss"]))
    print(f"T4: |logit| {e_logit:.2e}, |bce| {e_bce:.2e}, |llm| {e_llm:.2e} of {float(g['rel_llm_loss']):.4f}")
    assert e_logit < 1e-3 and e_bce < 5e-3 and e_llm < 1e-3


def test_gqa_training_gradients_vs_autograd_on_the_oracle():
    """forward_train_grad (teacher forcing with the key / value heads expanded by repeat_interleave) against torch.autograd
    through the CPU oracle on the model expanded to multi-head - the same function - with the same draws; the bounds of
    tests/test_gpu_train.py (the oracle is an fp32 restatement)."""
    from openpsg_amd.categories import relation_categories
    from oracle import psg_oracle as O
    g, cfg, w, inputs = _train_case()
    head = _train_head(cfg, w)
    out = head.forward_train_grad(_to_dev(inputs), sampled=g["sampled"], selected=g["selected"].tolist(), dropout=False)
    assert abs(float(out["rel_llm_loss"].detach()) - float(g["rel_llm_loss"])) < 1e-3
    (out["binary_rel_cls_loss"] + out["rel_llm_loss"]).backward()
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg_m, w_m = expand_to_mha(cfg, w)
    trainable = [k for k in w if not k.startswith("language_model.")]
    wr = {k: (v.clone().requires_grad_(True) if k in trainable else v) for k, v in w_m.items()}
    meta = inputs["img_metas"][0]
    ids, tmask, llm_prompt, llm_label = H.train_prompts(inputs)
    gtm = inputs["gt_masks"][0].to_tensor(torch.float32, "cpu")
    o = O.train_forward(wr, cfg_m, inputs["mask_features"], meta["masks_info"], meta["gt_rels"][0], gtm,
                        inputs["gt_semantic_seg"][0], ids, tmask, llm_prompt, llm_label, relation_categories,
                        sampled=g["sampled"], selected=g["selected"].tolist())
    og = torch.autograd.grad(o["binary_rel_cls_loss"] + o["rel_llm_loss"], [wr[k] for k in trainable], allow_unused=True)
    mine = dict(head.named_parameters())
    checked = 0
    for k, ref in zip(trainable, og):
        got = mine[k].grad
        got = torch.zeros_like(mine[k]).cpu() if got is None else got.cpu()
        ref = torch.zeros_like(got) if ref is None else ref
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        checked += scale > 0
        assert err <= 2e-3 * scale + 5e-6, f"{k}: max |grad - autograd| = {err:.3e} at gradient scale {scale:.3e}"
    assert checked >= 60


# ---- full size ----------------------------------------------------------------------------------------------------
def test_mistral_7b_shape_32_layers_fp32s_runs_and_submit_equals_forward():
    """The 32-layer Mistral-7B shape (4096 / 32 query, 8 key-value heads / 14336 / 32000) with random fp16-valued weights
    at BASELINE C3 (50 objects, top-20 selection, 16 tokens) in fp32s: it decodes, and `submit` gives forward's tokens."""
    from openpsg_amd.config import LlamaConfig, PSGConfig, QFormerConfig
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_device
    llm = LlamaConfig(inter=14336, kv_heads=8)
    cfg = PSGConfig(qformer=QFormerConfig(), llm=llm, max_object_num=50)
    w = make_weights_device(cfg, 0, torch.device("cuda:0"), llm_dtype=torch.float32, llm_values=torch.float16)
    head = _head(cfg, w, "fp32s", suppress_eos=True)
    del w
    assert head.llm_engine._w16_all and head.llm_engine.kv == 8
    scene = make_scene((1024, 1024), 50, seed=3, device="cuda:0", tiny_object=True)
    head(_inputs(scene))
    torch.cuda.synchronize()
    toks = head.last["tokens_host"].copy()
    assert toks.shape == (20, 16) and (toks >= 0).all() and (toks < llm.vocab).all()
    p = head.submit(_inputs(scene))
    p.result()
    assert np.array_equal(head.last["tokens_host"], toks)
