"""Grouped-query attention (GQA) on the CPU: the checkpoint reader's GQA opt-in and refusals, the state-dict schema, the
fixtures G8 / G9 / T4 (tools/capture_gqa_golden.py) against the CPU oracle on the same model expanded to multi-head, a
tiny GQA safetensors directory through `read_hf_llama_weights`."""
import ast
import json
import os

import numpy as np
import pytest
import torch

from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
from openpsg_amd.weights import llm_shapes, make_weights_numpy, read_hf_llama_config, read_hf_llama_weights
from tests import gqa_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mistral_config(**over):
    c = dict(architectures=["MistralForCausalLM"], model_type="mistral", hidden_size=4096, num_attention_heads=32,
             num_key_value_heads=8, num_hidden_layers=32, intermediate_size=14336, vocab_size=32000, rms_norm_eps=1e-5,
             rope_theta=10000.0, bos_token_id=1, eos_token_id=2, hidden_act="silu", sliding_window=4096,
             max_position_embeddings=32768, tie_word_embeddings=False, torch_dtype="bfloat16")
    c.update(over)
    return c


def _write(path, c):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(c, f)
    return str(path)


def test_reader_opt_in_returns_kv_heads_and_default_still_refuses(tmp_path):
    d = _write(tmp_path / "m", _mistral_config())
    m = read_hf_llama_config(d, grouped_query=True)
    assert (m.hidden, m.heads, m.kv_heads, m.n_kv_heads, m.kv_group, m.inter, m.vocab) == (4096, 32, 8, 8, 4, 14336, 32000)
    assert m.kv_dim == 1024 and m.rms_eps == 1e-5
    with pytest.raises(Exception, match="grouped-query"):
        read_hf_llama_config(d)
    mha = read_hf_llama_config(_write(tmp_path / "l", _mistral_config(model_type="llama", num_key_value_heads=32)))
    assert mha.kv_heads is None and mha.n_kv_heads == 32


def test_reader_accepts_mistral_and_llama_and_defaults_eps_as_hf(tmp_path):
    for i, over in enumerate([dict(sliding_window=None), dict(sliding_window=4096), dict(model_type="llama"),
                              dict(sliding_window=32768)]):
        c = _mistral_config(**over)
        assert read_hf_llama_config(_write(tmp_path / str(i), c), grouped_query=True).kv_heads == 8
    c = _mistral_config()
    del c["rms_norm_eps"]
    assert read_hf_llama_config(_write(tmp_path / "eps", c), grouped_query=True).rms_eps == 1e-6


@pytest.mark.parametrize("over,match", [
    (dict(sliding_window=2048), "sliding_window"),
    (dict(attention_bias=True), "attention_bias"),
    (dict(mlp_bias=True), "mlp_bias"),
    (dict(hidden_act="gelu"), "hidden_act"),
    (dict(head_dim=64), "head_dim"),
    (dict(model_type="gemma"), "model_type"),
    (dict(num_key_value_heads=2), "num_key_value_heads"),             # 16 query heads per key / value head
    (dict(num_key_value_heads=5), "num_key_value_heads"),             # not a divisor
    (dict(rope_scaling={"type": "linear", "factor": 2.0}), "rope_scaling"),
])
def test_reader_refuses_what_would_compute_something_else(tmp_path, over, match):
    with pytest.raises(Exception, match=match):
        read_hf_llama_config(_write(tmp_path / "m", _mistral_config(**over)), grouped_query=True)


def test_state_dict_shapes_and_mha_draws_unchanged():
    llm = tiny_llm(512, 2, 1024, 512, kv_heads=2)
    s = llm_shapes(PSGConfig(llm=llm))
    p = "language_model.model.layers.1.self_attn."
    assert s[p + "q_proj.weight"] == (512, 512) and s[p + "o_proj.weight"] == (512, 512)
    assert s[p + "k_proj.weight"] == (256, 512) and s[p + "v_proj.weight"] == (256, 512)
    mi = tiny_llm(4096, 1, 14336, 32000, kv_heads=8)
    s = llm_shapes(PSGConfig(llm=mi))
    assert s["language_model.model.layers.0.self_attn.k_proj.weight"] == (1024, 4096)
    # kv_heads = None and kv_heads = heads: the multi-head schema, the same seeded draws
    cfg_a = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 1, 512, 512))
    cfg_b = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 1, 512, 512, kv_heads=2))
    a, b = make_weights_numpy(cfg_a, seed=3), make_weights_numpy(cfg_b, seed=3)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_config_checks_the_group():
    tiny_llm(1024, 1, 512, 512, kv_heads=1).check_kv_heads()          # G = 8
    for kv in (3, 16):
        with pytest.raises(ValueError):
            tiny_llm(1024, 1, 512, 512, kv_heads=kv).check_kv_heads()


def test_tiny_gqa_safetensors_directory_round_trips(tmp_path):
    from safetensors.torch import save_file
    llm = tiny_llm(512, 3, 1024, 512, kv_heads=2)
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=llm)
    w = make_weights_numpy(cfg, seed=9)
    d = _write(tmp_path / "d", _mistral_config(hidden_size=512, num_attention_heads=4, num_key_value_heads=2,
                                               num_hidden_layers=3, intermediate_size=1024, vocab_size=512))
    sd = {k[len("language_model."):]: v.half().contiguous() for k, v in w.items() if k.startswith("language_model.")}
    save_file(sd, os.path.join(d, "model.safetensors"))
    m = read_hf_llama_config(d, grouped_query=True)
    assert m == llm
    got = read_hf_llama_weights(d, n_layers=2)
    want = {k: v for k, v in llm_shapes(cfg).items() if ".layers.2." not in k}
    assert set(got) == set(want)
    for k, shp in want.items():
        assert tuple(got[k].shape) == shp and got[k].dtype == torch.float16
        assert torch.equal(got[k], w[k].half())
    # a bias tensor in the weights is refused
    sd["model.layers.0.self_attn.q_proj.bias"] = torch.zeros(512, dtype=torch.float16)
    save_file(sd, os.path.join(d, "model.safetensors"))
    with pytest.raises(Exception, match="bias"):
        read_hf_llama_weights(d)


# ---- fixtures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,arch,kv,heads", [("G8_gqa_512_n10", "llama", 2, 4), ("G9_mistral_width_n6", "mistral", 8, 32),
                                                ("T4_gqa_train_512_n7", "llama", 2, 4)])
def test_fixture_keys(name, arch, kv, heads):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) < 500 * 1024
    g = np.load(path)
    assert str(g["llm_arch"]) == arch and int(g["llm_kv_heads"]) == kv and int(g["llm_heads"]) == heads
    assert int(g["llm_hidden"]) // 128 == heads
    if name.startswith("G"):
        assert g["gen_top8_idx"].shape == (20, 8) and g["gen_tokens"].shape[0] == 20
        assert g["selected"].shape == (20,)


def _expanded(g):
    import dataclasses
    llm = tiny_llm(int(g["llm_hidden"]), int(g["llm_layers"]), int(g["llm_inter"]), int(g["llm_vocab"]),
                   kv_heads=int(g["llm_kv_heads"]))
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=llm, max_object_num=30)
    w = make_weights_numpy(cfg, seed=int(g["weight_seed"]))
    wm = {k: (R.expand_kv_rows(v, llm.kv_group) if k.endswith(("k_proj.weight", "v_proj.weight")) else v) for k, v in w.items()}
    return dataclasses.replace(cfg, llm=dataclasses.replace(llm, kv_heads=None)), wm


def test_g8_fixture_is_the_oracle_on_the_model_expanded_to_mha():
    """The reference's GQA LLM and the CPU oracle's multi-head LLM with each key / value head repeated over its group
    are the same function: existence logits, selection, and the first pairs' greedy tokens agree."""
    from oracle import psg_oracle as O
    from openpsg_amd.synthetic import make_scene
    from tests import helpers as H
    g = dict(np.load(os.path.join(GOLDEN, "G8_gqa_512_n10.npz")))
    cfg, w = _expanded(g)
    scene = make_scene(**ast.literal_eval(str(g["scene_kw"])))
    qids, qmask = H.qformer_prompts(scene)
    with torch.no_grad():
        rq = O.relation_query(w, cfg, scene["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                              scene["pan_results"], qids, qmask)
        assert np.abs(rq["exist_logit"].numpy() - g["exist_logit"]).max() < 1e-4
        sel = g["selected"].tolist()
        pids, pmask = H.llm_prompts(scene, sel[:4])
        for i, si in enumerate(sel[:4]):
            x, mask = O.llm_inputs(w, rq["pair_feature"][si], pids[i], pmask[i])
            toks, _ = O.llm_generate(w, cfg, x, mask, suppress_eos=bool(g["suppress_eos"]))
            want = g["gen_tokens"][i]
            assert toks == want[want >= 0].tolist()


def test_t4_fixture_losses_are_the_oracle_on_the_model_expanded_to_mha():
    from oracle import psg_oracle as O
    from openpsg_amd.categories import relation_categories
    from openpsg_amd.synthetic import make_train_scene
    from tests import helpers as H
    g = dict(np.load(os.path.join(GOLDEN, "T4_gqa_train_512_n7.npz")))
    cfg, w = _expanded(g)
    inputs = make_train_scene(tuple(int(v) for v in g["pad_hw"]), [int(c) for c in g["categories"]],
                              [tuple(int(v) for v in r) for r in g["gt_rels"]], seed=int(g["scene_seed"]))
    meta = inputs["img_metas"][0]
    ids, tmask, llm_prompt, llm_label = H.train_prompts(inputs)
    gtm = inputs["gt_masks"][0].to_tensor(torch.float32, "cpu")
    with torch.no_grad():
        o = O.train_forward(w, cfg, inputs["mask_features"], meta["masks_info"], meta["gt_rels"][0], gtm,
                            inputs["gt_semantic_seg"][0], ids, tmask, llm_prompt, llm_label, relation_categories,
                            sampled=g["sampled"], selected=g["selected"].tolist())
    assert abs(float(o["binary_rel_cls_loss"]) - float(g["binary_rel_cls_loss"])) < 1e-3
    assert abs(float(o["rel_llm_loss"]) - float(g["rel_llm_loss"])) < 1e-4
