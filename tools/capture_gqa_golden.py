"""Captures the grouped-query attention (GQA) goldens from the reference head (CPU only, run once, by hand):

    python tools/capture_gqa_golden.py [G8] [G9] [T4]

  tests/golden/G8_gqa_512_n10.npz        G1's scene and weight seed, the LLM a LlamaForCausalLM at hidden 512 with 4 query
                                         heads and 2 key / value heads (G = 2), 2 layers, natural EOS
  tests/golden/G9_mistral_width_n6.npz   G6's scene at Mistral-7B width through MistralForCausalLM: hidden 4096, 32 query
                                         heads, 8 key / value heads, intermediate 14336, vocabulary 32000, 2 layers, EOS
                                         suppressed as in the benchmark
  tests/golden/T4_gqa_train_512_n7.npz   T1's training case and draws with G8's LLM: the losses

The reference head comes from oracle/capture_reference.py's helpers, unchanged: they build the head with a multi-head
LlamaForCausalLM, which is replaced here by the GQA model (`language_model`, V4:99-100) holding the weights of
`make_weights_numpy` for the GQA config.  The files have G1 / G6 / T1's keys plus `llm_kv_heads` and `llm_arch`;
generation rows keep the top-8 first-step logits only.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import capture_reference as CR  # noqa: E402
from openpsg_amd.config import tiny_llm  # noqa: E402

G8_LLM = tiny_llm(512, 2, 1024, 512, kv_heads=2)
G9_LLM = tiny_llm(4096, 2, 14336, 32000, kv_heads=8)
T1 = "T1_train_512_n7"


def gqa_language_model(llm, arch):
    """The GQA causal LM the reference would build from a Llama / Mistral checkpoint (eager attention)."""
    from transformers import LlamaConfig, LlamaForCausalLM, MistralConfig, MistralForCausalLM
    kw = dict(hidden_size=llm.hidden, intermediate_size=llm.inter, num_hidden_layers=llm.layers,
              num_attention_heads=llm.heads, num_key_value_heads=llm.n_kv_heads, vocab_size=llm.vocab,
              rms_norm_eps=llm.rms_eps, max_position_embeddings=4096, bos_token_id=llm.bos, eos_token_id=llm.eos,
              pad_token_id=None, tie_word_embeddings=False, rope_theta=llm.rope_theta)
    if arch == "mistral":
        lc = MistralConfig(sliding_window=4096, **kw)
        lc._attn_implementation = "eager"
        return MistralForCausalLM(lc)
    lc = LlamaConfig(**kw)
    lc._attn_implementation = "eager"
    return LlamaForCausalLM(lc)


def gqa_builder(arch):
    """CR.build_reference_head with the LLM swapped for the GQA model: the helper gets the weights with each key / value
    head's rows repeated over its group (the multi-head shapes it builds), the GQA model the weights themselves."""
    real = CR.build_reference_head

    def build(mod, cfg, w):
        m = cfg.llm
        G = m.kv_group
        wm = dict(w)
        for k, v in w.items():
            if k.endswith(("k_proj.weight", "v_proj.weight")):
                wm[k] = v.view(m.n_kv_heads, 1, 128, -1).expand(-1, G, -1, -1).reshape(m.hidden, -1).contiguous()
        h = real(mod, cfg, wm)
        lm = gqa_language_model(m, arch)
        sd = {k[len("language_model."):]: v for k, v in w.items() if k.startswith("language_model.")}
        missing, unexpected = lm.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        assert all("rotary_emb" in k for k in missing), missing
        h.language_model = lm.eval()
        return h
    return build


def add_keys(name, llm, arch):
    path = os.path.join(REPO, "tests", "golden", name + ".npz")
    d = dict(np.load(path))
    d["llm_kv_heads"] = np.int64(llm.n_kv_heads)
    d["llm_heads"] = np.int64(llm.heads)
    d["llm_arch"] = np.array(arch)
    np.savez_compressed(path, **d)
    print(f"{name}: kv_heads={llm.n_kv_heads} arch={arch} -> {os.path.getsize(path) / 1024:.0f} KiB")


def capture_scene(mod, name, scene_kw, llm, arch, weight_seed, keep, suppress_eos):
    real = CR.build_reference_head
    CR.build_reference_head = gqa_builder(arch)
    try:
        CR.capture_scene_case(mod, name, scene_kw, llm, weight_seed=weight_seed, keep_pairs=keep, suppress_eos=suppress_eos)
    finally:
        CR.build_reference_head = real
    add_keys(name, llm, arch)


def capture_train(mod, name, llm, arch):
    real, real_tiny = CR.build_reference_head, CR.tiny_llm
    CR.build_reference_head = gqa_builder(arch)
    CR.tiny_llm = lambda *a, **k: llm                        # capture_train_case's LLM
    CR.TRAIN_CASES[name] = CR.TRAIN_CASES[T1]                # T1's scene, weight seed and draws
    try:
        CR.capture_train_case(mod, name)
    finally:
        CR.build_reference_head, CR.tiny_llm = real, real_tiny
        del CR.TRAIN_CASES[name]
    add_keys(name, llm, arch)


def main(only=()):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = CR.import_reference_head()
    want = lambda n: not only or any(n.startswith(o) for o in only)  # noqa: E731
    if want("G8"):
        capture_scene(mod, "G8_gqa_512_n10",
                      dict(pad_hw=(512, 512), num_objects=10, seed=1, void_id=0, force_id0=True, tiny_object=True),
                      G8_LLM, "llama", 11, [0, 7, 55, 99], False)
    if want("T4"):
        capture_train(mod, "T4_gqa_train_512_n7", G8_LLM, "llama")
    if want("G9"):
        capture_scene(mod, "G9_mistral_width_n6", dict(pad_hw=(512, 512), num_objects=6, seed=6, void_id=133),
                      G9_LLM, "mistral", 16, [0, 21], True)


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
