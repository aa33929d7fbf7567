"""llm_decode='constrained' on the GPU (`-m gpu`): the decode over the relation-name trie only.

The engine under a constraint reproduces its own free greedy decode wherever that is valid; tokens and path
log-probabilities agree with a brute-force walk of the fp32 oracle and with the trie pass of llm_rel_scores='likelihood';
the decode is max_depth + 1 trie steps and nothing else; a head whose free decode is junk yields one valid relation per
selected pair; forward / submit / forward_batch / graph replay agree; the default path does not change."""
import dataclasses

import numpy as np
import pytest
import torch

from openpsg_amd._lib import PsgHipError
from openpsg_amd.categories import relation_categories
from openpsg_amd.rel_scores import RelationTrie
from tests import helpers as H
from tests import trie_walk_ref as W
from tests.test_gpu_llm_rank import _head, _inputs, _load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEAR_TIE = 1e-3                                               # the threshold of tests/test_gpu_llm_w8.py / _int4.py


def _decode(head, g, scene):
    names = H.object_names(scene)
    rq = head.run_relation_query(scene["mask_features"].to(DEV), scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                                 names, scene["pan_results"].to(DEV))
    sel = torch.from_numpy(g["selected"].astype(np.int32)).to(DEV)
    return head.decode_selected(rq, names, selected=sel)


# ---- 1. the constraint reproduces greedy where greedy is valid ------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [("G1_c1_512_n10", "fp32s"), ("G1_c1_512_n10", "mixed"), ("G8_gqa_512_n10", "fp32s"),
                                        ("G6_llm_7b_width_n6", "fp32s")])
def test_constraint_over_the_greedy_prefixes_reproduces_greedy(case, dtype):
    g, cfg, w, scene = _load(case)
    head = _head(cfg, w, dtype, suppress_eos=True)            # EOS suppressed: every pair has 16 tokens, none of them EOS
    dec = _decode(head, g, scene)
    eng, eos = head.llm_engine, cfg.llm.eos
    X, plen = dec["llm_inputs"], dec["prompt_len"]
    t0 = torch.as_tensor(np.asarray(dec["tokens_host"]))
    f0 = dec["first_logits"].clone()
    K = t0.shape[0]
    assert (t0 >= 0).all() and (t0 != eos).all()
    for n in (1, 2, 3):
        cands = sorted({tuple(int(t) for t in t0[k, :n]) + (eos,) for k in range(K)})
        trie = RelationTrie([str(c) for c in cands], [list(c) for c in cands], eos)
        assert trie.max_depth == n
        tok, fl, logp = eng.generate(X, plen, return_first_logits=True, constraint=trie, path_logp=True)
        torch.cuda.synchronize()
        tok, logp = tok.cpu(), logp.cpu()
        assert tok.shape == t0.shape
        if dtype == "fp32s":                                  # the same launches see the same rows; the arg-max is a child
            assert torch.equal(tok[:, :n], t0[:, :n].to(tok.dtype)), f"n={n}"
            assert torch.equal(fl, f0)
        else:
            assert all(tuple(int(t) for t in tok[k, :n + 1]) in cands for k in range(K))
        assert (tok[:, n] == eos).all() and (tok[:, n + 1:] == -1).all()
        assert torch.isfinite(logp).all() and (logp < 0).all()
        tok2, _, logp2 = eng.generate(X, plen, return_first_logits=True, constraint=trie, path_logp=True)   # graph replay
        assert torch.equal(tok2.cpu(), tok) and torch.equal(logp2.cpu(), logp)
        tok3 = eng.generate(X, plen, constraint=trie)         # without a score: tokens alone, the same ones
        assert torch.equal(tok3.cpu(), tok)
    with pytest.raises(PsgHipError, match="max_new_tokens=3"):
        eng.generate(X, plen, max_new_tokens=3, constraint=trie)
    with pytest.raises(PsgHipError, match="suppress_eos"):
        eng.generate(X, plen, suppress_eos=True, constraint=trie)


# ---- 2. tokens and scores against the oracle ------------------------------------------------------------------------
def _oracle_walk(cfg, w, X, seq_len, trie):
    """Brute force, as tests/test_gpu_llm_rank.py builds its reference: oracle.llama_forward in fp32 over the prompt, then
    one token at a time; lm_head in fp32, log-softmax in float64; the trie walked on the CPU (tests/trie_walk_ref.py).
    Returns tokens [K, max_depth + 1], path log-probability [K], top-2 margin among the children [K, max_depth + 1]."""
    from oracle import psg_oracle as O
    from tests import gqa_ref as R
    m = cfg.llm
    w32 = {k: v.float() for k, v in w.items() if k.startswith("language_model.")}
    if m.n_kv_heads != m.heads:
        w32 = {k: (R.expand_kv_rows(v, m.kv_group) if k.endswith(("k_proj.weight", "v_proj.weight")) else v)
               for k, v in w32.items()}
    cfg_mha = dataclasses.replace(cfg, llm=dataclasses.replace(m, kv_heads=None)) if m.n_kv_heads != m.heads else cfg
    emb, head_w = w32["language_model.model.embed_tokens.weight"], w32["language_model.lm_head.weight"]
    K, steps = X.shape[0], trie.max_depth + 1
    tokens = np.full((K, steps), -1, dtype=np.int64)
    logp = np.zeros(K)
    margin = np.full((K, steps), np.inf)
    for k in range(K):
        n = int(seq_len[k])
        cache = [None] * m.layers
        h = O.llama_forward(w32, cfg_mha, X[k, :n].float(), torch.arange(n), torch.ones(n, dtype=torch.bool), cache)
        node, done = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        for s in range(steps):
            lg = (h[-1] @ head_w.t())
            kids = [int(trie.child_tok[c]) for c in range(trie.child_off[int(node[0])], trie.child_off[int(node[0]) + 1])]
            top = np.sort(lg[kids].double().numpy())[::-1]
            if len(top) > 1:
                margin[k, s] = top[0] - top[1]
            r = W.walk_step(lg.numpy()[None], trie, node, done, m.eos)
            t = int(r["tok"][0])
            tokens[k, s] = t
            logp[k] += W.log_softmax64(lg.double().numpy())[t]
            node, done = r["node"], r["done"]
            if done[0]:
                break
            h = O.llama_forward(w32, cfg_mha, emb[t][None], torch.tensor([n + s]), torch.ones(n + s + 1, dtype=torch.bool),
                                cache)
    return tokens, logp, margin


_ORACLE = {}


def _oracle_for(case, dtype, cfg, w, last, trie):
    """The oracle's walk over the LLM inputs of the (case, dtype) head: computed once, shared, never written to."""
    if (case, dtype) not in _ORACLE:
        seq_len = last["prompt_len"].cpu().numpy() + cfg.qformer.num_query
        with torch.no_grad():
            _ORACLE[case, dtype] = _oracle_walk(cfg, w, last["llm_inputs"].float().cpu(), seq_len, trie)
    return _ORACLE[case, dtype]


def _agree_up_to_near_ties(name, got, ref, margin):
    """Per pair: every step before the first whose child top-2 margin (in the reference) is under NEAR_TIE must match.
    Returns the pairs whose whole path was compared and is equal."""
    K, T = ref.shape
    whole = []
    for k in range(K):
        tie = next((s for s in range(T) if margin[k, s] < NEAR_TIE), T)
        assert np.array_equal(got[k, :tie], ref[k, :tie]), f"{name}: pair {k} differs before its first near-tie (step {tie})"
        if np.array_equal(got[k, :T], ref[k]):
            whole.append(k)
    return whole


@pytest.mark.parametrize("case,dtype,tol", [("G1_c1_512_n10", "fp32s", 2e-4), ("G1_c1_512_n10", "mixed", 4e-2),
                                            ("G8_gqa_512_n10", "fp32s", 2e-4), ("G6_llm_7b_width_n6", "fp32s", 1e-4)])
def test_tokens_and_scores_against_the_oracle(case, dtype, tol):
    g, cfg, w, scene = _load(case)
    head = _head(cfg, w, dtype, llm_decode="constrained", llm_rel_scores="likelihood")
    res = head(_inputs(scene))
    last = head.last
    trie = head.relation_trie()
    T = trie.max_depth + 1
    got, lp = np.asarray(last["tokens_host"]), np.asarray(last["path_logp_host"], dtype=np.float64)
    K = got.shape[0]
    assert (got[:, T:] == -1).all()
    ref, want, margin = _oracle_for(case, dtype, cfg, w, last, trie)
    whole = _agree_up_to_near_ties(f"{case} {dtype}", got, ref, margin)
    err = np.abs(lp[whole] - want[whole]).max() if whole else 0.0
    print(f"{case} {dtype}: {len(whole)} of {K} paths equal to the oracle's, |logp - oracle| {err:.3e} (bound {tol:g})")
    # a path that left the oracle's at a near-tie has another probability: the score is compared on the equal paths, and
    # a case whose paths mostly differ would check nothing
    assert len(whole) >= 0.9 * K
    assert err <= tol, f"{case} {dtype}: path log-probabilities differ from the oracle by {err:.3e}"
    assert len(res["rel_pred"]) == K
    assert np.allclose(res["rel_score"], np.exp(lp), rtol=1e-12) and all(0.0 < s <= 1.0 for s in res["rel_score"])


# ---- 3. consistency with the trie pass ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["G1_c1_512_n10", "G8_gqa_512_n10", "G6_llm_7b_width_n6"])
def test_path_score_equals_the_trie_pass_score(case):
    g, cfg, w, scene = _load(case)
    con = _head(cfg, w, "fp32s", llm_decode="constrained", llm_rel_scores="likelihood")
    res = con(_inputs(scene))
    lp, sel = np.asarray(con.last["path_logp_host"], dtype=np.float64), con.last["selected_host"]
    K = len(sel)
    lik = _head(cfg, w, "fp32s", llm_rel_scores="likelihood")
    lik(_inputs(scene))
    ls = np.asarray(lik.last["logscores_host"], dtype=np.float64)
    assert np.array_equal(lik.last["selected_host"], sel) and len(res["rel_pred"]) == K
    err = max(abs(lp[k] - ls[k, res["rel_pred"][k][2]]) for k in range(K))
    print(f"{case}: |path logp - trie-pass log s| {err:.3e}")
    assert err <= 1e-4                                        # DESIGN 11's fp32 bound
    assert all(0.0 < s <= 1.0 for s in res["rel_score"])
    # N > 0: the trie pass runs as it does today and the ranked triples follow the emitted ones, which keep exp(logp)
    both = _head(cfg, w, "fp32s", llm_decode="constrained", llm_rel_scores="likelihood", num_llm_ranked_triples=7)
    r2 = both(_inputs(scene))
    assert r2["rel_pred"][:K] == res["rel_pred"] and r2["rel_score"][:K] == res["rel_score"]
    assert len(r2["rel_pred"]) == K + 7 and all(0.0 < s <= 1.0 for s in r2["rel_score"])
    assert all(t not in res["rel_pred"] for t in r2["rel_pred"][K:])
    assert np.abs(np.asarray(both.last["logscores_host"]) - ls).max() <= 1e-4


# ---- 4. shape of the decode -----------------------------------------------------------------------------------------
def _spy(monkeypatch, names):
    from openpsg_amd import ops
    calls = {n: 0 for n in names}
    for fn in calls:
        def wrapped(*a, _f=getattr(ops, fn), _n=fn, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrapped)
    return calls


@pytest.mark.parametrize("scores", ["constant", "likelihood"])
def test_decode_is_max_depth_plus_one_trie_steps(monkeypatch, scores):
    g, cfg, w, scene = _load("G1_c1_512_n10")
    head = _head(cfg, w, "fp32s", llm_decode="constrained", llm_rel_scores=scores)
    head.llm_engine.use_graph = False                         # eager: one call of the binding per launch
    calls = _spy(monkeypatch, ["trie_greedy_step", "greedy_step", "tree_attn", "token_logprobs"])
    res = head(_inputs(scene))
    depth = head.relation_trie().max_depth
    assert calls == dict(trie_greedy_step=depth + 1, greedy_step=0, tree_attn=0, token_logprobs=0)
    tok = np.asarray(head.last["tokens_host"])
    assert ((tok == cfg.llm.eos).sum(1) == 1).all()           # every pair done: the engine checked done.all() itself
    assert (tok[:, depth + 1:] == -1).all()
    # under graphs: the warm-up and the capture call the binding, a replay does not
    head2 = _head(cfg, w, "fp32s", llm_decode="constrained", llm_rel_scores=scores)
    for fn in calls:
        calls[fn] = 0
    assert head2(_inputs(scene)) == res
    assert calls == dict(trie_greedy_step=2 * (depth + 1), greedy_step=0, tree_attn=0, token_logprobs=0)
    assert head2(_inputs(scene)) == res and calls["trie_greedy_step"] == 2 * (depth + 1)
    assert head2.llm_engine.last_replays == 1                 # ONE graph: no chunks, no read-back between them


# ---- 5. a head whose free decode is junk ----------------------------------------------------------------------------
def test_junk_decoder_yields_one_valid_relation_per_selected_pair():
    g, cfg, w, scene = _load("G1_c1_512_n10")
    N = len(scene["object_id_list"])
    off = _head(cfg, w, "fp32s")
    r0 = off(_inputs(scene))
    K = len(off.last["selected_host"])
    assert len(r0["rel_pred"]) < K / 2                        # the seeded LLM does not emit class names
    on = _head(cfg, w, "fp32s", llm_decode="constrained")
    r1 = on(_inputs(scene))
    sel = on.last["selected_host"]
    assert np.array_equal(sel, off.last["selected_host"])
    assert len(r1["rel_pred"]) == K and r1["rel_score"] == [1] * K
    for k, (s, o, r) in enumerate(r1["rel_pred"]):            # one triple per pair, in selection order
        assert (s, o) == (int(sel[k]) // N, int(sel[k]) % N) and 0 <= r < len(relation_categories)
    trie = on.relation_trie()
    for k, row in enumerate(np.asarray(on.last["tokens_host"])):
        assert [int(t) for t in row if t >= 0] == trie.candidates[r1["rel_pred"][k][2]]


# ---- 6. call paths agree --------------------------------------------------------------------------------------------
def test_forward_submit_batch_and_replay_agree():
    g, cfg, w, scene = _load("G1_c1_512_n10")
    head = _head(cfg, w, "fp32s", llm_decode="constrained")
    inp = _inputs(scene)
    r = head(inp)
    t1 = np.asarray(head.last["tokens_host"]).copy()
    last = dict(head.last)
    assert head(inp) == r                                     # graph replay == first run
    assert head.submit(inp).result() == r
    assert head.forward_batch([inp])[0] == r
    p0, p1 = head.submit(inp, slot=0), head.submit(inp, slot=1)      # two slots in flight
    assert p1.result() == r and p0.result() == r
    # two images, 40 rows: the projections see another row count, so tokens agree up to each pair's first near-tie
    rb = head.forward_batch([inp, inp])
    trie = head.relation_trie()
    ref, _, margin = _oracle_for("G1_c1_512_n10", "fp32s", cfg, w, last, trie)
    K, T = t1.shape[0], trie.max_depth + 1
    for i, lb in enumerate(head.last_batch):
        tb = np.asarray(lb["tokens_host"])
        assert tb.shape == t1.shape and (tb[:, T:] == -1).all()
        for k in range(K):
            tie = next((s for s in range(T) if margin[k, s] < NEAR_TIE), T)
            assert np.array_equal(tb[k, :tie], t1[k, :tie]), f"image {i} pair {k}"
        assert len(rb[i]["rel_pred"]) == K
        if np.array_equal(tb, t1):
            assert rb[i] == r
    # scored: forward == submit on both slots == replay
    sc = _head(cfg, w, "fp32s", llm_decode="constrained", llm_rel_scores="likelihood")
    rs = sc(inp)
    assert rs["rel_pred"] == r["rel_pred"] and sc(inp) == rs
    for slot in (0, 1):
        assert sc.submit(inp, slot=slot).result() == rs


# ---- 7. the default is untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32s", "mixed"])
def test_option_off_is_the_head_without_the_keyword(dtype):
    g, cfg, w, scene = _load("G1_c1_512_n10")
    sup = bool(g["suppress_eos"])
    base = _head(cfg, w, dtype, suppress_eos=sup)
    off = _head(cfg, w, dtype, suppress_eos=sup, llm_decode="greedy")
    r0, r1 = base(_inputs(scene)), off(_inputs(scene))
    assert r0 == r1
    assert np.array_equal(base.last["tokens_host"], off.last["tokens_host"])
    assert torch.equal(base.last["first_logits"], off.last["first_logits"])
    assert "path_logp" not in off.last
