"""llm_beam_width on the GPU (`-m gpu`): the beam over the relation-name trie through the engine and the head.

Every returned (pair, class) score against the fp32 oracle's per-edge table (tests/beam_oracle.py) and against the trie
pass of llm_rel_scores='likelihood'; the selection against the numpy beam of tests/trie_beam_ref.py (the precondition - the
oracle's own beam has no near-tie on these goldens - is tests/test_beam_cpu.py's); exactness on a trie no level of which
holds more than B nodes; dead rows; the launches, the graph replay, submit; the projection routes of the 60-row steps; the
head's outputs; and the default, which does not change."""
import numpy as np
import pytest
import torch

from openpsg_amd.rel_scores import RelationTrie
from tests import beam_oracle as BO
from tests import trie_beam_ref as BR
from tests.test_gpu_llm_constrained import NEAR_TIE, _decode
from tests.test_gpu_llm_rank import _head, _inputs, _load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BEAM = dict(llm_decode="constrained", llm_rel_scores="likelihood")
TOL = {"fp32s": 2e-4, "mixed": 4e-2}                          # test_tokens_and_scores_against_the_oracle's own bounds
_TABLE, _LIK = {}, {}


def _table_for(key, cfg, w, last, trie):
    """The oracle's per-edge table over the LLM inputs of the `key` head: computed once, shared, never written to."""
    if key not in _TABLE:
        seq_len = last["prompt_len"].cpu().numpy() + cfg.qformer.num_query
        _TABLE[key] = BO.edge_table(cfg, w, last["llm_inputs"].float().cpu(), seq_len, trie)
    return _TABLE[key]


def _full_scores(trie, table):
    return np.stack([BR.path_scores(trie, t) for t in table])


def _beam_head(case, dtype, B, **kw):
    g, cfg, w, scene = _load(case)
    head = _head(cfg, w, dtype, llm_beam_width=B, **BEAM, **kw)
    res = head(_inputs(scene))
    return g, cfg, w, scene, head, res


def _score_error(last, full):
    cls, lp = np.asarray(last["beam_class_host"]), np.asarray(last["beam_logp_host"], dtype=np.float64)
    ok = cls >= 0
    assert ok.all() and np.isfinite(lp).all()                  # 56 classes: every pair fills its B entries
    k = np.arange(cls.shape[0])[:, None].repeat(cls.shape[1], 1)
    return float(np.abs(lp - full[k, cls]).max())


# ---- 1. scores ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("case,dtype", [("G1_c1_512_n10", "fp32s"), ("G1_c1_512_n10", "mixed"), ("G8_gqa_512_n10", "fp32s")])
def test_scores_against_the_oracle_and_the_trie_pass(case, dtype, B):
    g, cfg, w, scene, head, res = _beam_head(case, dtype, B)
    last, trie = head.last, head.relation_trie()
    K = len(last["selected_host"])
    assert K * B in (60, 160) and last["beam_class_host"].shape == (K, B) == last["beam_logp_host"].shape
    full = _full_scores(trie, _table_for((case, dtype), cfg, w, last, trie))
    err = _score_error(last, full)
    print(f"{case} {dtype} B={B}: |beam logp - oracle path sum| {err:.3e} (bound {TOL[dtype]:g})")
    assert err <= TOL[dtype]
    lp = np.asarray(last["beam_logp_host"])
    assert (np.diff(lp, axis=1) <= 0).all() and (lp < 0).all()  # best first
    assert all(len(set(row.tolist())) == B for row in np.asarray(last["beam_class_host"]))
    if dtype == "fp32s":
        if case not in _LIK:
            lik = _head(cfg, w, "fp32s", llm_rel_scores="likelihood")
            lik(_inputs(scene))
            assert np.array_equal(lik.last["selected_host"], last["selected_host"])
            _LIK[case] = np.asarray(lik.last["logscores_host"], dtype=np.float64)
        err2 = _score_error(last, _LIK[case])
        print(f"{case} {dtype} B={B}: |beam logp - trie-pass log s| {err2:.3e}")
        assert err2 <= 1e-4


# ---- 2. selection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("case", ["G1_c1_512_n10", "G8_gqa_512_n10"])
def test_selection_equals_the_numpy_beam_over_the_oracle_table(case, B):
    """A pair whose numpy beam has no level with a gap under NEAR_TIE is compared whole: its B classes, in order.  A
    pair with such a level cannot be compared behind it from the final lists and is left out; at least 90 % are whole."""
    g, cfg, w, scene, head, res = _beam_head(case, "fp32s", B)
    last, trie = head.last, head.relation_trie()
    table = _table_for((case, "fp32s"), cfg, w, last, trie)
    cls = np.asarray(last["beam_class_host"])
    K, whole = cls.shape[0], 0
    for k in range(K):
        want, _, gaps, _ = BR.search(trie, B, table[k])
        if gaps.min() < NEAR_TIE:
            continue
        whole += 1
        assert cls[k].tolist() == want.tolist(), f"{case} B={B}: pair {k}"
    print(f"{case} B={B}: {whole} of {K} pairs compared whole")
    assert whole >= 0.9 * K


# ---- 3. exactness without pruning -----------------------------------------------------------------------------------
def _greedy_prefix_trie(head, g, scene, n, limit):
    """A trie over the first `n` greedy tokens of the pairs (+ EOS), at most `limit` candidates: no level holds more than
    `limit` nodes.  Returns (trie, X, prompt_len)."""
    dec = _decode(head, g, scene)
    t0, eos = np.asarray(dec["tokens_host"]), head.cfg.llm.eos
    assert (t0[:, :n] >= 0).all() and (t0[:, :n] != eos).all()
    cands = sorted({tuple(int(t) for t in t0[k, :n]) + (eos,) for k in range(t0.shape[0])})[:limit]
    return RelationTrie([str(c) for c in cands], [list(c) for c in cands], eos), dec["llm_inputs"], dec["prompt_len"]


@pytest.mark.parametrize("B", [3, 8])
def test_beam_is_the_top_b_of_the_trie_pass_when_no_level_prunes(B):
    g, cfg, w, scene = _load("G1_c1_512_n10")
    head = _head(cfg, w, "fp32s", suppress_eos=True)
    trie, X, plen = _greedy_prefix_trie(head, g, scene, 2, B)
    R = len(trie.candidates)
    assert 2 <= R <= B and trie.max_depth == 2
    assert all(int((trie.node_depth == d).sum()) <= B for d in (1, 2))
    eng = head.llm_engine
    cls, lp = eng.generate(X, plen, constraint=trie, beam=B)
    _, _, ls = eng.generate(X, plen, return_first_logits=True, trie=trie)
    torch.cuda.synchronize()
    cls, lp, ls = cls.cpu().numpy(), lp.double().cpu().numpy(), ls.double().cpu().numpy()
    K = cls.shape[0]
    assert cls.shape == (K, B) and ls.shape == (K, R)
    worst, compared = 0.0, 0
    for k in range(K):
        assert sorted(cls[k, :R].tolist()) == list(range(R)) and (cls[k, R:] == -1).all()      # nothing was pruned
        assert np.isneginf(lp[k, R:]).all()
        worst = max(worst, float(np.abs(lp[k, :R] - ls[k, cls[k, :R]]).max()))
        order = np.argsort(-ls[k], kind="stable")
        gap = np.abs(np.diff(ls[k, order]))
        for i in range(R):
            if (i > 0 and gap[i - 1] < NEAR_TIE) or (i < R - 1 and gap[i] < NEAR_TIE):
                continue
            compared += 1
            assert cls[k, i] == order[i], f"pair {k} position {i}"
    print(f"B={B}: {R} classes, {compared} of {K * R} positions compared, |beam logp - trie pass| {worst:.3e}")
    assert worst <= 1e-4 and compared >= K                   # (on average a position per pair: the comparison is not empty)


# ---- 4. dead rows ---------------------------------------------------------------------------------------------------
def test_dead_rows_change_nothing():
    """A trie whose root has two children: with B = 3 every level has a dead row per pair.  The results are those of
    B = 2, where no row is dead (the row counts differ, so the scores agree to DESIGN 11's fp32 bound, not bit for bit)."""
    g, cfg, w, scene = _load("G1_c1_512_n10")
    head = _head(cfg, w, "fp32s", suppress_eos=True)
    dec = _decode(head, g, scene)
    t0, eos = np.asarray(dec["tokens_host"]), cfg.llm.eos
    firsts = sorted({int(t) for t in t0[:, 0]})
    assert len(firsts) >= 2
    a, b = firsts[:2]
    a2 = int(t0[[k for k in range(len(t0)) if t0[k, 0] == a][0], 1])
    b2 = int(t0[[k for k in range(len(t0)) if t0[k, 0] == b][0], 1])
    cands = [[a, eos], [a, a2, eos], [b, b2, eos]]
    trie = RelationTrie(["a", "aa", "bb"], cands, eos)
    assert trie.child_off[1] - trie.child_off[0] == 2 and trie.max_depth == 2
    eng, X, plen = head.llm_engine, dec["llm_inputs"], dec["prompt_len"]
    c3, l3 = (t.cpu().numpy() for t in eng.generate(X, plen, constraint=trie, beam=3))
    c2, l2 = (t.cpu().numpy() for t in eng.generate(X, plen, constraint=trie, beam=2))
    K = c3.shape[0]
    assert (np.sort(c3, axis=1) == np.arange(3)).all() and np.isfinite(l3).all()
    for k in range(K):
        for i in range(2):
            j = int(np.where(c3[k] == c2[k, i])[0][0])
            assert abs(float(l3[k, j]) - float(l2[k, i])) <= 1e-4, (k, i)
        if np.abs(np.diff(l3[k].astype(np.float64))).min() >= NEAR_TIE:
            assert c3[k, :2].tolist() == c2[k].tolist(), k
    c3b, l3b = (t.cpu().numpy() for t in eng.generate(X, plen, constraint=trie, beam=3))          # the replay
    assert np.array_equal(c3b, c3) and np.array_equal(l3b, l3)


# ---- 5. launches and replay -----------------------------------------------------------------------------------------
def _spy(monkeypatch, names, rows_of=()):
    from openpsg_amd import ops
    calls = {n: 0 for n in names}
    rows = {n: [] for n in rows_of}
    for fn in calls:
        def wrapped(*a, _f=getattr(ops, fn), _n=fn, **kw):
            calls[_n] += 1
            if _n in rows:
                rows[_n].append(int(a[0].shape[0]))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrapped)
    return calls, rows


STEP_OPS = ["trie_beam_step", "greedy_step", "trie_greedy_step", "token_logprobs", "tree_attn"]


def test_decode_is_max_depth_plus_one_beam_steps_and_one_replay(monkeypatch):
    B = 3
    g, cfg, w, scene = _load("G1_c1_512_n10")
    head = _head(cfg, w, "fp32s", llm_beam_width=B, **BEAM)
    head.llm_engine.use_graph = False                         # eager: one call of the binding per launch
    calls, rows = _spy(monkeypatch, STEP_OPS, rows_of=["tree_attn"])
    res = head(_inputs(scene))
    depth, K, layers = head.relation_trie().max_depth, len(head.last["selected_host"]), cfg.llm.layers
    assert calls == dict(trie_beam_step=depth + 1, greedy_step=0, trie_greedy_step=0, token_logprobs=0,
                         tree_attn=depth * layers)
    assert rows["tree_attn"] == [K * B] * (depth * layers)    # max_depth forwards of K x B rows
    first = (np.asarray(head.last["beam_class_host"]).copy(), np.asarray(head.last["beam_logp_host"]).copy())
    # under graphs: the warm-up and the capture call the binding, a replay does not
    head2 = _head(cfg, w, "fp32s", llm_beam_width=B, **BEAM)
    for fn in calls:
        calls[fn] = 0
    inp = _inputs(scene)
    assert head2(inp) == res
    assert calls["trie_beam_step"] == 2 * (depth + 1) and calls["greedy_step"] == calls["trie_greedy_step"] == 0
    assert np.array_equal(head2.last["beam_class_host"], first[0]) and np.array_equal(head2.last["beam_logp_host"], first[1])
    assert head2(inp) == res and calls["trie_beam_step"] == 2 * (depth + 1)
    assert head2.llm_engine.last_replays == 1                 # ONE graph: no chunks, no read-back
    assert np.array_equal(head2.last["beam_class_host"], first[0]) and np.array_equal(head2.last["beam_logp_host"], first[1])
    assert head2.submit(inp).result() == res
    assert np.array_equal(head2.last["beam_logp_host"], first[1])
    p0, p1 = head2.submit(inp, slot=0), head2.submit(inp, slot=1)      # two slots in flight
    assert p1.result() == res and p0.result() == res


def test_engine_refusals():
    from openpsg_amd._lib import PsgHipError
    g, cfg, w, scene = _load("G1_c1_512_n10")
    head = _head(cfg, w, "fp32s", **BEAM)
    dec = _decode(head, g, scene)
    eng, X, plen, trie = head.llm_engine, dec["llm_inputs"], dec["prompt_len"], head.relation_trie()
    with pytest.raises(PsgHipError, match="beam=3.*constraint="):
        eng.generate(X, plen, beam=3)
    with pytest.raises(PsgHipError, match="beam=9"):
        eng.generate(X, plen, constraint=trie, beam=9)
    with pytest.raises(PsgHipError, match="21 pairs x beam 8 = 168 rows.*160"):
        eng.generate(torch.cat([X, X[:1]]), torch.cat([plen, plen[:1]]), constraint=trie, beam=8)
    with pytest.raises(PsgHipError, match="beam=3.*path_logp"):
        eng.generate(X, plen, constraint=trie, beam=3, path_logp=True)


# ---- 6. projection routes -------------------------------------------------------------------------------------------
def test_fp8_bytes_stream_in_the_beam_levels(monkeypatch):
    from tests.test_gpu_llm_w8 import _dequantised
    B, case, dtype = 3, "G1_c1_512_n10", "mixed"
    calls, _ = _spy(monkeypatch, ["batch_gemm_w8", "batch_split_gemm_w8", "tree_attn"])
    g, cfg, w, scene, head, res = _beam_head(case, dtype, B, llm_weight_quant="fp8", llm_batch_weight_stream="quantised")
    last, trie = head.last, head.relation_trie()
    depth, layers = trie.max_depth, cfg.llm.layers
    # warm-up + capture: each of the four decoder projections of every layer of every level goes through exactly one route,
    # and all of them took the byte stream - none is left for a dense product
    assert calls["tree_attn"] == 2 * depth * layers
    assert calls["batch_gemm_w8"] == 2 * depth * layers * 4 and calls["batch_split_gemm_w8"] == 0
    full = _full_scores(trie, _table_for((case, dtype, "fp8"), cfg, _dequantised(w, layers), last, trie))
    err = _score_error(last, full)
    print(f"{case} {dtype} fp8 B={B}: |beam logp - oracle on W'| {err:.3e} (bound {TOL[dtype]:g})")
    assert err <= TOL[dtype]


def test_fp32s_levels_run_on_the_own_split_gemm(monkeypatch):
    B, case, dtype = 3, "G1_c1_512_n10", "fp32s"
    calls, _ = _spy(monkeypatch, ["batch_split_gemm_w16", "batch_split_gemm_w32", "tree_attn"])
    g, cfg, w, scene, head, res = _beam_head(case, dtype, B, llm_batch_split_gemm="own")
    last, trie = head.last, head.relation_trie()
    depth, layers = trie.max_depth, cfg.llm.layers
    assert calls["tree_attn"] == 2 * depth * layers
    assert calls["batch_split_gemm_w16"] + calls["batch_split_gemm_w32"] >= 2 * depth * layers * 4
    full = _full_scores(trie, _table_for((case, dtype), cfg, w, last, trie))
    err = _score_error(last, full)
    print(f"{case} {dtype} own split GEMM B={B}: |beam logp - oracle| {err:.3e} (bound {TOL[dtype]:g})")
    assert err <= TOL[dtype]
    lib = _head(cfg, w, dtype, llm_beam_width=B, **BEAM)      # the default route: none of the own entries
    n = calls["batch_split_gemm_w16"] + calls["batch_split_gemm_w32"]
    lib(_inputs(scene))
    assert calls["batch_split_gemm_w16"] + calls["batch_split_gemm_w32"] == n


# ---- 7. head outputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 8])
def test_head_outputs(B):
    g, cfg, w, scene, head, res = _beam_head("G1_c1_512_n10", "fp32s", B)
    last = head.last
    cls, lp, sel = np.asarray(last["beam_class_host"]), np.asarray(last["beam_logp_host"]), last["selected_host"]
    K, N = len(sel), len(scene["object_id_list"])
    pred, score = res["rel_pred"], res["rel_score"]
    assert len(pred) == K * B == len(score) and len({tuple(t) for t in pred}) == K * B        # none repeated
    assert all(isinstance(s, float) and 0.0 < s <= 1.0 for s in score)
    for k in range(K):                                        # first each pair's best, in selection order
        assert pred[k] == [int(sel[k]) // N, int(sel[k]) % N, int(cls[k, 0])]
        assert score[k] == float(np.exp(np.float64(lp[k, 0])))
    rank_of = {int(s): k for k, s in enumerate(sel)}
    rest = [(-score[i], rank_of[pred[i][0] * N + pred[i][1]], pred[i][2]) for i in range(K, K * B)]
    assert rest == sorted(rest)                               # then by descending score, selection rank, class
    assert sorted((k, r) for _, k, r in rest) == sorted((k, int(cls[k, b])) for k in range(K) for b in range(1, B))
    # the constrained head's triple of a pair is the beam's best hypothesis wherever the oracle-side gap is clear
    assert (pred, score) == head.parse_beam(cls, lp, sel, N)


# ---- 8. the default is untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32s", "mixed"])
def test_width_one_is_the_head_without_the_keyword(dtype, monkeypatch):
    g, cfg, w, scene = _load("G1_c1_512_n10")
    calls, _ = _spy(monkeypatch, ["trie_beam_step", "trie_greedy_step"])
    base = _head(cfg, w, dtype, **BEAM)
    one = _head(cfg, w, dtype, llm_beam_width=1, **BEAM)
    r0, r1 = base(_inputs(scene)), one(_inputs(scene))
    assert r0 == r1 and calls["trie_beam_step"] == 0 and calls["trie_greedy_step"] > 0
    assert np.array_equal(base.last["tokens_host"], one.last["tokens_host"])
    assert np.array_equal(base.last["path_logp_host"], one.last["path_logp_host"])
    assert torch.equal(base.last["first_logits"], one.last["first_logits"])
    assert "beam_class_host" not in one.last
