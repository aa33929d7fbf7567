"""llm_rel_scores='likelihood' on the GPU (`-m gpu`): psg_tree_attn and psg_token_logprobs against float64 restatements,
the head's log scores of every (pair, class) against a brute-force oracle on the goldens (G1, G2, G8 GQA,
G6 at Llama-2-7B width, G9 at Mistral width), the trie pass against the engine's own teacher-forced forward,
no change to the default path, submit == forward, a replaced tokenizer under a captured graph, and one 32-layer
Llama-2-7B-shaped run."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openpsg_amd.categories import relation_categories
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- kernels --------------------------------------------------------------------------------------------------------
def _rand_trie(gen, n_int, max_depth):
    parent = [-1]
    for i in range(1, n_int):
        p = int(torch.randint(-1, i, (1,), generator=gen))
        depth_p = 0
        a = p
        while a >= 0:
            depth_p += 1
            a = parent[a]
        parent.append(p if depth_p < max_depth else -1)
    anc = np.full((n_int, max_depth), -1, dtype=np.int32)
    for i in range(n_int):
        chain, a = [], i
        while a >= 0:
            chain.append(a)
            a = parent[a]
        anc[i, :len(chain)] = chain[::-1]
    return anc


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("heads,kv_heads", [(4, 4), (4, 2), (8, 2), (8, 1), (16, 2)])
def test_tree_attn_against_float64(dtype, heads, kv_heads):
    from openpsg_amd import ops
    gen = torch.Generator().manual_seed(heads * 10 + kv_heads)
    K, n_int, max_depth, base = 3, 23, 8, 70
    ctx = base + n_int + 5
    anc = _rand_trie(gen, n_int, max_depth)
    plen = torch.tensor([5, 41, 70], dtype=torch.int32)
    rows = K * n_int
    row_pair = torch.arange(K, dtype=torch.int32).repeat_interleave(n_int)
    row_node = torch.arange(n_int, dtype=torch.int32).repeat(K)
    q = torch.randn(rows, heads * 128, generator=gen, dtype=torch.float64)
    kc = torch.randn(K, kv_heads, ctx, 128, generator=gen, dtype=torch.float64)
    vc = torch.randn(K, kv_heads, ctx, 128, generator=gen, dtype=torch.float64)
    qd, kd, vd = (t.to(dtype) for t in (q, kc, vc))
    out = torch.empty(rows, heads * 128, dtype=dtype, device=DEV)
    ops.tree_attn(qd.to(DEV), kd.to(DEV), vd.to(DEV), row_pair.to(DEV), row_node.to(DEV), plen.to(DEV),
                  torch.from_numpy(anc).to(DEV), base, heads, 128, ctx, out, kv_heads=kv_heads)
    q64, k64, v64 = (t.double() for t in (qd, kd, vd))           # the stored values, in float64
    ref = torch.empty(rows, heads * 128, dtype=torch.float64)
    g = heads // kv_heads
    for r in range(rows):
        p, nd = int(row_pair[r]), int(row_node[r])
        slots = list(range(int(plen[p]))) + [base + int(a) for a in anc[nd] if a >= 0]
        for h in range(heads):
            kk, vv = k64[p, h // g, slots], v64[p, h // g, slots]
            s = kk @ q64[r, h * 128:(h + 1) * 128] / math.sqrt(128)
            ref[r, h * 128:(h + 1) * 128] = torch.softmax(s, 0) @ vv
    got = out.double().cpu()
    if dtype == torch.float32:
        err = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert err < 1e-6, err                                   # 1e-6 relative to the output's scale
    else:
        tol = 1e-2 if dtype == torch.bfloat16 else 2e-3
        assert (got - ref).abs().max().item() < tol * max(1.0, ref.abs().max().item())
    # and elementwise inside the derived bound of tests/llm_attn_ref.py (the kernel keeps its probabilities in fp32)
    from tests import llm_attn_ref as L
    r64, A, gx, n = L.tree64(qd, kd, vd, row_pair, row_node, plen, anc, base, heads)
    assert torch.allclose(r64, ref, rtol=0, atol=1e-12)
    L.check("tree_attn", out.cpu(), r64, L.attn_bound(r64, A, gx, n, dtype))


@pytest.mark.parametrize("vocab", [32000, 1000])
@pytest.mark.parametrize("splits,dtype", [(0, torch.float32), (3, torch.float32), (0, torch.bfloat16)])
def test_token_logprobs_against_log_softmax(vocab, splits, dtype):
    from openpsg_amd import ops
    gen = torch.Generator().manual_seed(vocab + splits)
    rows, n_nodes = 7, 4
    child_off = torch.tensor([0, 3, 5, 5, 9], dtype=torch.int32)
    child_tok = torch.randint(0, vocab, (9,), generator=gen, dtype=torch.int32)
    child_tok[0] = vocab - 1
    row_node = torch.tensor([0, 1, 2, 3, 3, 1, 0], dtype=torch.int32)
    row_out = torch.tensor([0, 3, 5, 9, 13, 17, 19], dtype=torch.int64)
    out_len = 22
    if splits:
        parts = torch.randn(splits, rows, vocab, generator=gen) * 4
        logits = ops.Partials(parts.to(DEV).contiguous())
        full = parts[0].clone()
        for s in range(1, splits):
            full = full + parts[s]                                # the kernel's slice-order fp32 sum
        lg = full.double()
    else:
        x = (torch.randn(rows, vocab, generator=gen) * 4).to(dtype)
        logits = x.to(DEV)
        lg = x.double()
    out = torch.full((out_len,), 123.0, device=DEV)
    ops.token_logprobs(logits, row_node.to(DEV), row_out.to(DEV), child_off.to(DEV), child_tok.to(DEV), out)
    ls = torch.log_softmax(lg, dim=1)
    want = torch.full((out_len,), 123.0, dtype=torch.float64)
    for r in range(rows):
        n = int(row_node[r])
        for c in range(int(child_off[n]), int(child_off[n + 1])):
            want[int(row_out[r]) + c - int(child_off[n])] = ls[r, int(child_tok[c])]
    got = out.double().cpu()
    assert ((got - want).abs() <= 1e-6 * want.abs().clamp(min=1.0)).all(), (got - want).abs().max().item()
    # deterministic
    out2 = torch.full((out_len,), 123.0, device=DEV)
    ops.token_logprobs(logits, row_node.to(DEV), row_out.to(DEV), child_off.to(DEV), child_tok.to(DEV), out2)
    assert torch.equal(out, out2)


def test_token_logprobs_skips_minus_inf():
    """A -inf logit (a masked token, a 16-bit overflow) contributes exp(-inf) = 0, also as a row's first entry."""
    from openpsg_amd import ops
    gen = torch.Generator().manual_seed(5)
    rows, vocab = 3, 1000
    x = torch.randn(rows, vocab, generator=gen) * 4
    x[:, :300] = -float("inf")                                   # every thread's first entries
    x[1, 512:700] = -float("inf")
    child_off = torch.tensor([0, 4], dtype=torch.int32)
    child_tok = torch.tensor([300, 999, 450, 811], dtype=torch.int32)
    out = torch.zeros(rows * 4, device=DEV)
    ops.token_logprobs(x.to(DEV), torch.zeros(rows, dtype=torch.int32, device=DEV),
                       (torch.arange(rows, dtype=torch.int64) * 4).to(DEV), child_off.to(DEV), child_tok.to(DEV), out)
    want = torch.log_softmax(x.double(), 1)[:, child_tok.long()].reshape(-1)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    assert ((got - want).abs() <= 1e-6 * want.abs().clamp(min=1.0)).all()


# ---- head against the float64 oracle ----------------------------------------------------------------------------
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


def _load(case):
    if case.startswith(("G8", "G9")):
        from tests.test_gpu_gqa_head import load_gqa_case
        return load_gqa_case(case)
    return H.load_case(case)


def _oracle_log_scores(cfg, w, X, seq_len, trie, pairs=None):
    """Brute force: oracle.llama_forward (fp32, the reference's precision; its additive mask is built for fp32) over the
    prompt (generate's positions 0..seq_len-1), then the candidates' tokens one at a time (token c_j at position
    seq_len + j - 1; a prefix shared by several candidates is fed once, from a copy of its parent's cache), the lm_head
    (fp32 product) and log_softmax of every step in float64.  pairs: the selection ranks to compute (default all); other
    rows are NaN."""
    from tests import gqa_ref as R
    m = cfg.llm
    w32 = {k: v.float() for k, v in w.items() if k.startswith("language_model.")}
    if m.n_kv_heads != m.heads:                                # the multi-head model that computes the same function
        w32 = {k: (R.expand_kv_rows(v, m.kv_group) if k.endswith(("k_proj.weight", "v_proj.weight")) else v)
               for k, v in w32.items()}
    import dataclasses
    cfg_mha = dataclasses.replace(cfg, llm=dataclasses.replace(m, kv_heads=None)) if m.n_kv_heads != m.heads else cfg
    from oracle import psg_oracle as O
    emb, head_w = w32["language_model.model.embed_tokens.weight"], w32["language_model.lm_head.weight"]
    node_of = {tuple(int(trie.node_tok[a]) for a in trie.anc[i] if a >= 0): i for i in range(trie.n_int)}
    K = X.shape[0]
    out = np.full((K, len(trie.candidates)), np.nan)
    for k in (range(K) if pairs is None else pairs):
        n = int(seq_len[k])
        cache = [None] * m.layers
        h = O.llama_forward(w32, cfg_mha, X[k, :n].float(), torch.arange(n), torch.ones(n, dtype=torch.bool), cache)
        root = torch.log_softmax((h[-1] @ head_w.t()).double(), 0)
        caches, lps = {}, {}
        for i in range(trie.n_int):                            # parents come before their children
            par, d = int(trie.node_parent[i]), int(trie.node_depth[i])
            cc = list(cache if par < 0 else caches[par])        # llama_forward replaces the list's entries, not the tensors
            hj = O.llama_forward(w32, cfg_mha, emb[int(trie.node_tok[i])][None], torch.tensor([n + d - 1]),
                                 torch.ones(n + d, dtype=torch.bool), cc)
            caches[i] = cc
            lps[i] = torch.log_softmax((hj[-1] @ head_w.t()).double(), 0)
        for r, c in enumerate(trie.candidates):
            out[k, r] = float(root[c[0]]) + sum(float(lps[node_of[tuple(c[:j])]][c[j]]) for j in range(1, len(c)))
    return out


def _check_against_oracle(case, dtype, pairs=None):
    g, cfg, w, scene = _load(case)
    head = _head(cfg, w, dtype, suppress_eos=bool(g["suppress_eos"]), llm_rel_scores="likelihood",
                 num_llm_ranked_triples=4096)
    res = head(_inputs(scene))
    last = head.last
    K = last["selected_host"].shape[0]
    R = len(relation_categories)
    ls = last["logscores_host"]
    assert ls.shape == (K, R) and np.isfinite(ls).all()
    seq_len = last["prompt_len"].cpu().numpy() + cfg.qformer.num_query
    X = last["llm_inputs"].float().cpu()
    want = _oracle_log_scores(cfg, w, X, seq_len, head.relation_trie(), pairs)
    ks = list(range(K)) if pairs is None else list(pairs)
    err = np.abs(ls[ks] - want[ks]).max()
    assert err < 2e-4, f"log scores differ from the oracle by {err:.3e}"
    # outputs: generated triples first (scored), then every remaining (pair, class) in the oracle's order
    N = len(scene["object_id_list"])
    gen = head._parse_pairs(last["tokens_host"], last["selected_host"], N)
    assert len(res["rel_pred"]) == K * R
    assert res["rel_pred"][:len(gen)] == [t for _, t in gen]
    assert all(isinstance(s, float) for s in res["rel_score"])
    rank_of = {int(s): k for k, s in enumerate(last["selected_host"])}
    ranked = [(rank_of[s * N + o_], r) for s, o_, r in res["rel_pred"][len(gen):]]
    o = np.array([want[k, r] for k, r in ranked if k in ks])     # the oracle's scores, in the head's order
    suffix_max = np.maximum.accumulate(o[::-1])[::-1]
    assert (suffix_max <= o + 1e-4).all(), "ranked triples out of the oracle's order"
    print(f"{case} {dtype}: {len(ks)} of {K} pairs x {R} classes against the oracle, |log s - oracle| {err:.2e}")


@pytest.mark.parametrize("dtype", ["fp32", "fp32s"])
@pytest.mark.parametrize("case", ["G1_c1_512_n10", "G2_768x1024_n12", "G8_gqa_512_n10"])
def test_head_log_scores_and_ranking_against_oracle(case, dtype):
    _check_against_oracle(case, dtype)


@pytest.mark.parametrize("case", ["G6_llm_7b_width_n6", "G9_mistral_width_n6"])
def test_head_log_scores_against_oracle_at_7b_width(case):
    """G6 (Llama-2-7B width, vocabulary 32 000) and G9 (Mistral width, 32 query / 8 key-value heads) in fp32: every
    (pair, class), as on the small goldens (the CPU oracle walks 77 single-token forwards of a 4096-wide model per pair:
    the slowest test of this file)."""
    _check_against_oracle(case, "fp32")


def _teacher_forced(eng, X, seq_len, trie):
    """log s(p, r) from the engine's own teacher-forced forward over [prompt, c_1..c_{n-1}] with generate's positions."""
    K, R = X.shape[0], len(trie.candidates)
    L = trie.max_len
    out = np.zeros((K, R))
    for k in range(K):
        n = int(seq_len[k])
        S = n + L - 1
        Xb = torch.zeros((R, S, X.shape[2]), device=DEV, dtype=X.dtype)
        Xb[:, :n] = X[k, :n]
        lens = torch.tensor([n + len(c) - 1 for c in trie.candidates], device=DEV, dtype=torch.int32)
        for r, c in enumerate(trie.candidates):
            if len(c) > 1:
                Xb[r, n:n + len(c) - 1] = eng.embed[torch.tensor(c[:-1], device=DEV)].to(X.dtype)
        rows = torch.tensor([r * S + n - 1 + j for r in range(R) for j in range(L)], device=DEV, dtype=torch.int32)
        rope = torch.arange(S, device=DEV, dtype=torch.int32).repeat(R)
        lg = eng.teacher_forcing_logits(Xb, lens, rope, rows).double().view(R, L, -1)
        lp = torch.log_softmax(lg, -1).cpu()
        for r, c in enumerate(trie.candidates):
            out[k, r] = sum(float(lp[r, j, c[j]]) for j in range(len(c)))
    return out


# Absolute bounds on log s, about twice the measured maxima (G6 4.9e-5, G9 5.1e-5, G1 2.1e-5 in fp32; mixed 1.9e-2; bf16
# 0.15).  In fp32 the two sides differ in reduction order only - library GEMMs at other row counts, psg_tree_attn against
# psg_llm_attn - which at 2 layers of 4096 and log s of -15..-40 comes to ~5e-5, not the 1e-5 of a single product.
@pytest.mark.parametrize("case,dtype,tol", [("G6_llm_7b_width_n6", "fp32", 1e-4), ("G1_c1_512_n10", "fp32", 5e-5),
                                            ("G9_mistral_width_n6", "fp32", 1e-4), ("G1_c1_512_n10", "mixed", 4e-2),
                                            ("G1_c1_512_n10", "bf16", 3e-1)])
def test_trie_pass_against_teacher_forcing(case, dtype, tol):
    g, cfg, w, scene = _load(case)
    head = _head(cfg, w, dtype, suppress_eos=bool(g["suppress_eos"]), llm_rel_scores="likelihood")
    head(_inputs(scene))
    last = head.last
    seq_len = last["prompt_len"].cpu().numpy() + cfg.qformer.num_query
    tf = _teacher_forced(head.llm_engine, last["llm_inputs"], seq_len, head.relation_trie())
    d = np.abs(last["logscores_host"] - tf)
    assert d.max() <= tol, f"{case} {dtype}: trie pass vs teacher forcing {d.max():.3e}"
    print(f"{case} {dtype}: trie pass vs teacher forcing max {d.max():.2e}")


# ---- the default path does not change -----------------------------------------------------------------------------
def test_option_off_and_on_keep_tokens_and_submit_equals_forward():
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    base = _head(cfg, w, "fp32s", suppress_eos=bool(g["suppress_eos"]))
    off = _head(cfg, w, "fp32s", suppress_eos=bool(g["suppress_eos"]), llm_rel_scores="constant",
                num_llm_ranked_triples=0)
    on = _head(cfg, w, "fp32s", suppress_eos=bool(g["suppress_eos"]), llm_rel_scores="likelihood",
               num_llm_ranked_triples=50)
    r0 = base(_inputs(scene))
    t0 = base.last["tokens_host"].copy()
    r1 = off(_inputs(scene))
    assert np.array_equal(off.last["tokens_host"], t0) and r1 == r0 and all(s == 1 for s in r1["rel_score"])
    r2 = on(_inputs(scene))
    assert np.array_equal(on.last["tokens_host"], t0), "the likelihood pass changed the generated tokens"
    ngen = len(r0["rel_pred"])
    assert r2["rel_pred"][:ngen] == r0["rel_pred"] and len(r2["rel_pred"]) == ngen + 50
    assert all(0.0 < s <= 1.0 for s in r2["rel_score"])
    for slot in (0, 1):
        assert on.submit(_inputs(scene), slot=slot).result() == r2
    assert on(_inputs(scene)) == r2                             # graph replay == first run


def test_replaced_tokenizer_under_a_captured_graph_keeps_the_scores():
    """A tokenizer replaced by an equal one rebuilds the head's trie; the captured decode graph of the old one (same key:
    same candidates) still reads the old trie's device tables, which its decode state keeps alive."""
    import gc
    from openpsg_amd.tokenizers import WordTokenizer
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    head = _head(cfg, w, "fp32s", suppress_eos=bool(g["suppress_eos"]), llm_rel_scores="likelihood",
                 num_llm_ranked_triples=100)
    r0 = head(_inputs(scene))
    ls0 = head.last["logscores_host"].copy()
    t0 = head.relation_trie()
    n_graphs = len(head.llm_engine._graphs)
    tok = WordTokenizer("llama")
    tok.pad_token = tok.unk_token
    head.llm_tokenizer = tok
    assert head.relation_trie() is not t0 and head.relation_trie().key == t0.key
    del t0
    gc.collect()
    # small blocks of the caching allocator handed out again, filled with values no table holds
    junk = [torch.full((n,), -77777, dtype=torch.int32, device=DEV) for n in (16, 64, 128, 256, 512) for _ in range(16)]
    junk += [torch.full((n,), -77777, dtype=torch.int64, device=DEV) for n in (64, 256) for _ in range(16)]
    torch.cuda.synchronize()
    r1 = head(_inputs(scene))
    assert len(head.llm_engine._graphs) == n_graphs                # the captured graph was replayed
    assert np.array_equal(head.last["logscores_host"], ls0) and r1 == r0
    del junk


def test_submission_keeps_the_likelihood_scores(tmp_path):
    import json
    from openpsg_amd.results import write_submission
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    head = _head(cfg, w, "fp32", suppress_eos=bool(g["suppress_eos"]), llm_rel_scores="likelihood",
                 num_llm_ranked_triples=10)
    out = head(_inputs(scene))
    # the dict OpenSeeDRelationV2.simple_test packs (detector._pack)
    res = dict(pan_results=scene["pan_results"].numpy(),
               rel_results=dict(object_id_list=[int(i) for i in scene["object_id_list"]], relation=out["rel_pred"]),
               rel_scores=out["rel_score"])
    assert len(out["rel_score"]) >= 10 and any(s != 1 for s in out["rel_score"])
    path = write_submission([res], str(tmp_path), keep_scores=True)
    recs = json.load(open(path))
    assert recs[0]["relation_scores"] == out["rel_score"]


# ---- 32 layers at Llama-2-7B shapes ---------------------------------------------------------------------------------
def test_32_layer_trie_pass_is_finite_and_sum_consistent():
    from openpsg_amd.config import LlamaConfig, PSGConfig, QFormerConfig
    from openpsg_amd.llm import LlamaDecodeEngine
    from openpsg_amd.rel_scores import RelationTrie, candidate_ids
    from openpsg_amd.tokenizers import WordTokenizer
    from openpsg_amd.weights import make_weights_device
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=LlamaConfig(layers=32), max_object_num=50)
    w = make_weights_device(cfg, 0, DEV, llm_dtype=torch.bfloat16)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    K, Tp = 20, 16
    X = torch.randn((K, 32 + Tp, 4096), device=DEV, generator=gen)
    plen = torch.randint(9, Tp + 1, (K,), device=DEV, generator=gen, dtype=torch.int32)
    tok = WordTokenizer("llama")
    trie = RelationTrie(list(relation_categories), [candidate_ids(tok, n, cfg.llm.eos) for n in relation_categories],
                        cfg.llm.eos)
    eng = LlamaDecodeEngine(w, cfg, DEV, torch.float32, prefill_split=True)
    t0, _ = eng.generate(X, plen, return_first_logits=True)
    t1, _, ls = eng.generate(X, plen, return_first_logits=True, trie=trie)
    torch.cuda.synchronize()
    assert torch.equal(t0, t1)
    ls = ls.double().cpu()
    assert torch.isfinite(ls).all()
    tot = ls.exp().sum(1)
    assert (tot <= 1 + 1e-5).all(), tot.max().item()
    print(f"32 layers fp32s: {trie.n_int} trie rows per pair, P(any relation) per pair {tot.min():.3f}..{tot.max():.3f}")
