"""The fp32 oracle's per-edge log-probability table of a relation trie, shared by tests/test_beam_cpu.py and
tests/test_gpu_llm_beam.py: oracle.llama_forward over a pair's compact LLM inputs, then one forward per internal trie node
on a copy of its parent's cache (token node_tok at position seq_len + depth - 1), the lm_head in fp32 and
tests/trie_walk_ref.log_softmax64.  table[k, c] = log-probability of trie edge c for pair k; a class's score is the sum
over its path (tests/trie_beam_ref.path_scores)."""
import dataclasses

import numpy as np
import torch

from tests import helpers as H
from tests import trie_walk_ref as W


def load(case):
    if case.startswith(("G8", "G9")):
        from tests.test_gpu_gqa_head import load_gqa_case      # (builds the case on the host: no GPU call)
        return load_gqa_case(case)
    return H.load_case(case)


def _mha(cfg, w):
    """The multi-head model that computes the same function as a grouped-query one (the oracle is multi-head)."""
    from tests import gqa_ref as R
    m = cfg.llm
    w32 = {k: v.float() for k, v in w.items() if k.startswith("language_model.")}
    if m.n_kv_heads != m.heads:
        w32 = {k: (R.expand_kv_rows(v, m.kv_group) if k.endswith(("k_proj.weight", "v_proj.weight")) else v)
               for k, v in w32.items()}
        cfg = dataclasses.replace(cfg, llm=dataclasses.replace(m, kv_heads=None))
    return cfg, w32


@torch.no_grad()
def edge_table(cfg, w, X, seq_len, trie):
    """X [K, >= seq_len, D] (or a list of [seq_len_k, D]) compact fp32 LLM inputs -> float64 [K, n_edges]."""
    from oracle import psg_oracle as O
    cfg_mha, w32 = _mha(cfg, w)
    m = cfg.llm
    emb, head_w = w32["language_model.model.embed_tokens.weight"], w32["language_model.lm_head.weight"]
    K = len(X)
    out = np.zeros((K, trie.n_edges))

    def fill(k, nd, h):
        ls = W.log_softmax64((h[-1] @ head_w.t()).double().numpy())
        c0, c1 = int(trie.child_off[nd]), int(trie.child_off[nd + 1])
        out[k, c0:c1] = ls[trie.child_tok[c0:c1]]
    for k in range(K):
        n = int(seq_len[k])
        cache = [None] * m.layers
        h = O.llama_forward(w32, cfg_mha, X[k][:n].float(), torch.arange(n), torch.ones(n, dtype=torch.bool), cache)
        fill(k, 0, h)
        caches = {}
        for i in range(trie.n_int):                            # parents come before their children
            par, d = int(trie.node_parent[i]), int(trie.node_depth[i])
            cc = list(cache if par < 0 else caches[par])        # llama_forward replaces the list's entries, not the tensors
            hj = O.llama_forward(w32, cfg_mha, emb[int(trie.node_tok[i])][None], torch.tensor([n + d - 1]),
                                 torch.ones(n + d, dtype=torch.bool), cc)
            caches[i] = cc
            fill(k, 1 + i, hj)
    return out


@torch.no_grad()
def oracle_llm_inputs(g, cfg, w, scene):
    """The oracle's own LLM inputs of a golden case's selected pairs, compact: ([x_k [seq_len_k, D]], seq_len [K])."""
    from oracle import psg_oracle as O
    w32 = {k: v.float() for k, v in w.items()}
    ids, mask = H.qformer_prompts(scene)
    rq = O.relation_query(w32, cfg, scene["mask_features"].float(), scene["img_meta"],
                          [int(i) for i in scene["object_id_list"]], scene["pan_results"], ids, mask)
    sel = [int(s) for s in g["selected"]]
    pids, pmask = H.llm_prompts(scene, sel)
    xs = []
    for i, si in enumerate(sel):
        x, msk = O.llm_inputs(w32, rq["pair_feature"][si], pids[i], pmask[i])
        xs.append(x[msk.bool()])
    return xs, np.asarray([x.shape[0] for x in xs])
