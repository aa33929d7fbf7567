"""The LLM stage's options composed (`-m gpu`): llm_decode='constrained' and llm_rel_scores='likelihood' on every weight
stream, decode-step route and row count they can meet.  Every kernel below is anchored to float64 on its own; what is held
here is the glue in `LlamaDecodeEngine._steps` / `generate` - which partials each route hands the trie step, whether the
path log-probability and the trie node survive each route under capture and replay, whether the graph key separates calls
that must not share a graph.

A quantised LLM is the model whose matrices are the dequantised W' (tests/test_gpu_llm_w8.py), so the reference is always
the CPU oracle on W' or the option-off head loaded with W', never the head under test.  The seeded LLMs emit 2-7 distinct
relation paths, so token agreement alone is weak: the path log-probabilities (A) and the 4 x 56 log scores (B) are the
sharp checks.  tests/test_llm_option_matrix_cpu.py holds the precondition: the oracle alone has no near-tie on any variant.

A  constrained on the FP8 / MXFP4 / INT4 streams (pair form in fp32s, single form in `mixed`), G1 and G8
B  the likelihood pass (`_rank_pass`) over the quantised models, and the constrained path score against it
C  constrained x the persistent decoder layer (G6, fp32)      D  constrained x the fused route (G6, bf16)
E  constrained above 32 rows (forward_batch, 40 rows) on psg_batch_gemm_s / psg_batch_gemm_q
F  the 32 -> 33 row boundary and the graph cache, on the engine

Every tolerance is the bar the project already holds the same arithmetic to, named where it is used.

Measured on an MI355X: no pair of any variant has a near-tie on the heads' own inputs, so all 20 paths are compared whole
everywhere.  A: |path logp - oracle| at most 1.6e-5 in fp32s (bound 2e-4) and 1.2e-2 in mixed (4e-2), first-step logits at
most 1.8e-5 from the option-off head on W' (1e-4).  B: |log s - oracle| 2.2e-5 (2e-4), |path logp - trie-pass log s| 9.6e-6
(1e-4).  E: both images of every batch equal to the single image's paths.  F: |path logp - oracle| 9.0e-6 at K = 1, 20, 32,
33; K = 1 and K = 32 bit-equal to K = 20 on the shared rows, K = 33 within 7.7e-6 of it.  Each test's docstring has its own."""
import gc

import numpy as np
import pytest
import torch

from openpsg_amd.categories import relation_categories
from tests import llm_matrix_ref as M
from tests.test_gpu_llm_constrained import NEAR_TIE, _agree_up_to_near_ties, _oracle_walk
from tests.test_gpu_llm_rank import _head, _inputs, _oracle_log_scores

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEP_KERNELS = ("trie_greedy_step", "greedy_step", "tree_attn", "token_logprobs")
STREAM = {  # the decode-step entry of each format: [fp32s pair form, 16-bit single form]
    "fp8": ("split_gemm_w8", "skinny_gemm_w8"), "mxfp4": ("split_gemm_w4", "skinny_gemm_w4"),
    "int4g": ("split_gemm_int4", "skinny_gemm_int4")}
ALL_STREAMS = tuple(n for pair in STREAM.values() for n in pair)
BATCH = ("batch_split_gemm_w16", "batch_split_gemm_w32", "batch_split_gemm_w8", "batch_split_gemm_w4", "batch_gemm_w8",
         "batch_gemm_w4")
_ORACLE = {}
_G6 = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_module_caches():
    yield
    _ORACLE.clear()
    _G6.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _quant_kw(fmt, lm_head):
    return {} if fmt is None else dict(llm_weight_quant=fmt, llm_quantize_lm_head=lm_head)


def _spy(monkeypatch, names):
    """Calls of ops.<name>, all of them and those made while a decode step runs (`LlamaDecodeEngine._steps`: the prompt
    pass, whose last layer and lm_head see <= 32 rows too, is over by then)."""
    from openpsg_amd import ops
    from openpsg_amd.llm import LlamaDecodeEngine
    calls, steps = {n: 0 for n in names}, {n: 0 for n in names}
    state = {"in_steps": False}
    for fn in names:
        def wrapped(*a, _f=getattr(ops, fn), _n=fn, **kw):
            calls[_n] += 1
            steps[_n] += int(state["in_steps"])
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrapped)

    def in_steps(self, *a, _f=LlamaDecodeEngine._steps, **kw):
        state["in_steps"] = True
        try:
            return _f(self, *a, **kw)
        finally:
            state["in_steps"] = False
    monkeypatch.setattr(LlamaDecodeEngine, "_steps", in_steps)
    return calls, steps


def _reset(*counters):
    for c in counters:
        for k in c:
            c[k] = 0


def _oracle(case, dtype, fmt, lm_head, cfg, w, X, seq_len, trie):
    """`_oracle_walk` on W' over the LLM inputs of the (case, dtype) head - the relation query never sees the weight
    options, so they are those of every variant: computed once per (case, dtype, fmt, lm_head), shared, never written to."""
    key = (case, dtype, fmt, bool(lm_head))
    if key not in _ORACLE:
        wq = M.dequantised({k: v.clone() for k, v in w.items()}, cfg.llm.layers, fmt, lm_head)
        with torch.no_grad():
            _ORACLE[key] = _oracle_walk(cfg, wq, X.float().cpu(), np.asarray(seq_len), trie)
    return _ORACLE[key]


def _seq_len(cfg, last):
    return last["prompt_len"].cpu().numpy() + cfg.qformer.num_query


def _assert_one_candidate_per_pair(res, last, trie, N):
    """rel_pred[k] is (sel // N, sel % N, r) of pair k, in selection order, and pair k's tokens are candidate r."""
    sel, tok = last["selected_host"], np.asarray(last["tokens_host"])
    assert len(res["rel_pred"]) == len(sel) == tok.shape[0]
    for k, (s, o, r) in enumerate(res["rel_pred"]):
        assert (s, o) == (int(sel[k]) // N, int(sel[k]) % N) and 0 <= r < len(relation_categories)
        assert [int(t) for t in tok[k] if t >= 0] == trie.candidates[r], f"pair {k}"
    assert (tok[:, trie.max_depth + 1:] == -1).all()


# ---- A. constrained decode on every quantised stream ----------------------------------------------------------------
A_PARAMS = ([(M.G1, "fp32s", f, h) for f in M.FORMATS for h in (False, True)] + [(M.G8, "fp32s", f, True) for f in M.FORMATS]
            + [(M.G1, "mixed", f, False) for f in M.FORMATS])


@pytest.mark.parametrize("case,dtype,fmt,lm_head", A_PARAMS)
def test_a_constrained_decode_on_the_quantised_stream(case, dtype, fmt, lm_head, monkeypatch):
    """Routing (eager, by spies), tokens and path log-probability against the oracle on W' (2e-4 in fp32s, 4e-2 in mixed:
    the bars of test_tokens_and_scores_against_the_oracle), one candidate per pair, first-step logits within 1e-4 of the
    option-off constrained head on W' (fp32s; the bar of `_fp32s_pair`), capture + two replays bit-equal, submit ==
    forward.
    Measured on an MI355X: 0 of 20 pairs with a near-tie and 20 of 20 paths equal to the oracle's on all 12 parameters;
    |logp - oracle| 9.0e-6 .. 1.6e-5 in fp32s (G8 int4g + lm_head the largest), 1.2e-2 / 9.4e-3 / 7.5e-3 in mixed (fp8 /
    mxfp4 / int4g); first-step logits 0 .. 1.8e-5 from the option-off head (G1 fp8 the largest), path logp 1.1e-5 from its."""
    g, cfg, w, scene = M.load(case)
    inp, N = _inputs(scene), len(scene["object_id_list"])
    pair = dtype == "fp32s"
    entry = STREAM[fmt][0 if pair else 1]
    # W4_STREAM_AS_FP8: an MXFP4 shape listed there streams its exact FP8 image through the FP8 entry of the same form
    accepted = (entry, STREAM["fp8"][0 if pair else 1]) if fmt == "mxfp4" else (entry,)
    calls, steps = _spy(monkeypatch, STEP_KERNELS + ALL_STREAMS)
    # 1. routing, eager: one call of the binding per launch
    con = _head(cfg, w, dtype, llm_decode="constrained", **_quant_kw(fmt, lm_head))
    eng = con.llm_engine
    eng.use_graph = False
    trie = con.relation_trie()
    T = trie.max_depth + 1
    if pair:
        assert {"fp8": eng._can_w8, "mxfp4": eng._can_w4, "int4g": eng._can_int4}[fmt](20)
        assert not eng._can_wb16(20) and not eng._can_persist(20, 0) and not eng._can_w16(20) and not eng._can_fuse(20)
    else:
        assert not any(f(20) for f in (eng._can_w8, eng._can_w4, eng._can_int4, eng._can_wb16, eng._can_w16, eng._can_fuse))
    if pair:
        assert not eng.decode_uses_library(20)
    _reset(calls, steps)
    r_con = con(inp)
    assert {n: calls[n] for n in STEP_KERNELS} == dict(trie_greedy_step=T, greedy_step=0, tree_attn=0, token_logprobs=0)
    assert steps["trie_greedy_step"] == T - 1                          # the first one belongs to the prompt pass
    per_step = 4 * cfg.llm.layers + int(pair and lm_head)              # every decoder projection (+ a quantised lm_head)
    assert sum(steps[n] for n in accepted) == (T - 1) * per_step and steps[entry] > 0, steps
    assert all(calls[n] == 0 for n in ALL_STREAMS if n not in accepted), calls
    assert r_con["rel_score"] == [1] * len(r_con["rel_pred"])
    _assert_one_candidate_per_pair(r_con, con.last, trie, N)
    t_con = np.asarray(con.last["tokens_host"]).copy()
    del con, eng
    # 2. scored, under graphs: tokens and path log-probability against the oracle on W'
    sc = _head(cfg, w, dtype, llm_decode="constrained", llm_rel_scores="likelihood", **_quant_kw(fmt, lm_head))
    _reset(calls, steps)
    res = sc(inp)
    assert calls["greedy_step"] == 0 and calls["trie_greedy_step"] == 2 * T     # warm-up + capture
    last = dict(sc.last)
    got, lp = np.asarray(last["tokens_host"]).copy(), np.asarray(last["path_logp_host"], dtype=np.float64)
    K = got.shape[0]
    assert np.array_equal(got, t_con)                                  # the score does not change the walk
    ref, want, margin = _oracle(case, dtype, fmt, lm_head, cfg, w, last["llm_inputs"], _seq_len(cfg, last), trie)
    name = f"{case} {dtype} {fmt}{' + lm_head' if lm_head else ''}"
    near = int((margin < NEAR_TIE).any(1).sum())
    whole = _agree_up_to_near_ties(name, got, ref, margin)
    tol = 2e-4 if pair else 4e-2
    err = np.abs(lp[whole] - want[whole]).max() if whole else 0.0
    print(f"{name}: {near} of {K} pairs with a near-tie in the oracle, {len(whole)} of {K} paths equal to the oracle's, "
          f"|logp - oracle| {err:.3e} (bound {tol:g})")
    assert len(whole) >= 0.9 * K
    assert err <= tol, f"{name}: path log-probabilities differ from the oracle by {err:.3e}"
    assert np.allclose(res["rel_score"], np.exp(lp), rtol=1e-12) and all(0.0 < s <= 1.0 for s in res["rel_score"])
    # 3. one candidate per pair
    _assert_one_candidate_per_pair(res, last, trie, N)
    # 5. the capture's replay and two more: bit-equal
    f0, p0 = last["first_logits"].clone(), last["path_logp"].clone()
    for rep in range(2):
        assert sc(inp) == res
        assert np.array_equal(sc.last["tokens_host"], got), f"replay {rep}"
        assert torch.equal(sc.last["path_logp"], p0) and torch.equal(sc.last["first_logits"], f0), f"replay {rep}"
    assert calls["trie_greedy_step"] == 2 * T and sc.llm_engine.last_replays == 1
    # 6. submit on both slots == forward
    for slot in (0, 1):
        assert sc.submit(inp, slot=slot).result() == res
    pa, pb = sc.submit(inp, slot=0), sc.submit(inp, slot=1)            # both in flight
    assert pb.result() == res and pa.result() == res
    del sc
    # 4. first-step logits against the option-off constrained head on W'
    if pair:
        wq = M.dequantised({k: v.clone() for k, v in w.items()}, cfg.llm.layers, fmt, lm_head)
        off = _head(cfg, wq, dtype, llm_decode="constrained", llm_rel_scores="likelihood")
        oe = off.llm_engine
        assert set(M.formats(oe)) == {None}
        _reset(calls, steps)
        off(inp)
        assert all(calls[n] == 0 for n in ALL_STREAMS)
        d = (off.last["first_logits"].float() - f0.float()).abs().max().item()
        t_off = np.asarray(off.last["tokens_host"])
        _agree_up_to_near_ties(name + " against the option-off head", got, t_off[:, :T], margin)
        same = [k for k in whole if np.array_equal(t_off[k], got[k])]
        assert len(same) >= 0.9 * K
        dl = np.abs(np.asarray(off.last["path_logp_host"], dtype=np.float64)[same] - lp[same]).max()
        print(f"{name}: first-step logits, option on vs off on W': {d:.3e} (bound 1e-4); path logp on vs off {dl:.3e}")
        assert d < 1e-4
        assert dl <= 2 * tol                                           # each is within tol of the same oracle's path score


# ---- B. the likelihood pass on every quantised stream ---------------------------------------------------------------
@pytest.mark.parametrize("case,fmt", [(M.G1, "fp8"), (M.G1, "mxfp4"), (M.G1, "int4g"), (M.G8, "int4g")])
def test_b_likelihood_pass_on_the_quantised_model(case, fmt, monkeypatch):
    """Log scores [K, 56] of a head over the quantised model (every matrix resident, the default) against the brute-force
    oracle on W' for 4 pairs spread over the selection, within 2e-4 (the bound of `_check_against_oracle`); and with
    llm_decode='constrained' added, the path score within 1e-4 of the trie-pass score of the emitted class (the bar of
    test_path_score_equals_the_trie_pass_score).
    Measured on an MI355X: |log s - oracle| 2.1e-5 (G1, the three formats) and 2.2e-5 (G8 int4g); |path logp - trie-pass
    log s| 4.8e-6 .. 9.6e-6."""
    g, cfg, w, scene = M.load(case)
    inp, N = _inputs(scene), len(scene["object_id_list"])
    calls, steps = _spy(monkeypatch, STEP_KERNELS + ALL_STREAMS)
    lik = _head(cfg, w, "fp32s", llm_rel_scores="likelihood", llm_weight_resident="all", **_quant_kw(fmt, False))
    eng = lik.llm_engine
    assert {"fp8": eng._can_w8, "mxfp4": eng._can_w4, "int4g": eng._can_int4}[fmt](20) and eng.resident == "all"
    lik(inp)
    assert calls["tree_attn"] == 2 * cfg.llm.layers and calls["token_logprobs"] == 4     # warm-up + capture, root + nodes
    assert calls["trie_greedy_step"] == 0 and steps[STREAM[fmt][0]] > 0                  # greedy tokens, on the stream
    last = lik.last
    ls = np.asarray(last["logscores_host"], dtype=np.float64)
    sel = last["selected_host"]
    K, R = len(sel), len(relation_categories)
    assert ls.shape == (K, R) == (20, 56) and np.isfinite(ls).all() and (ls < 0).all()
    pairs = [0, 6, 13, K - 1]
    trie = lik.relation_trie()
    wq = M.dequantised({k: v.clone() for k, v in w.items()}, cfg.llm.layers, fmt, False)
    with torch.no_grad():
        want = _oracle_log_scores(cfg, wq, last["llm_inputs"].float().cpu(), _seq_len(cfg, last), trie, pairs=pairs)
    err = np.abs(ls[pairs] - want[pairs]).max()
    print(f"{case} fp32s {fmt}: {len(pairs)} pairs x {R} classes against the oracle on W', |log s - oracle| {err:.3e} "
          f"(bound 2e-4)")
    assert err < 2e-4, f"log scores differ from the oracle by {err:.3e}"
    lik.llm_engine._graphs.clear()
    del lik, eng
    con = _head(cfg, w, "fp32s", llm_decode="constrained", llm_rel_scores="likelihood", **_quant_kw(fmt, False))
    res = con(inp)
    lp = np.asarray(con.last["path_logp_host"], dtype=np.float64)
    assert np.array_equal(con.last["selected_host"], sel)
    _assert_one_candidate_per_pair(res, con.last, trie, N)
    d = max(abs(lp[k] - ls[k, res["rel_pred"][k][2]]) for k in range(K))
    print(f"{case} fp32s {fmt}: |path logp - trie-pass log s| {d:.3e} (bound 1e-4)")
    assert d <= 1e-4


# ---- C, D. constrained x the persistent decoder layer / the fused route (G6, loaded once) ---------------------------
def _g6():
    if not _G6:
        _G6["case"] = M.load(M.G6)
    return _G6["case"]


def _three_runs(head, inp):
    """Capture, then two replays: (tokens, path_logp, first_logits) of the first, asserted bit-equal to the others."""
    runs = []
    for _ in range(3):
        res = head(inp)
        runs.append((np.asarray(head.last["tokens_host"]).copy(), head.last["path_logp"].clone().cpu(),
                     head.last["first_logits"].clone().cpu(), res))
    for t, p, f, r in runs[1:]:
        assert np.array_equal(t, runs[0][0]) and torch.equal(p, runs[0][1]) and torch.equal(f, runs[0][2]) and r == runs[0][3]
    return runs[0]


def _with_option(name, dtype, steps, check):
    """A constrained + likelihood G6 head built under context option `name` = 0 and = 1 (the try / finally idiom of
    tests/test_gpu_decode_layer.py): {flag: (tokens, logp, first logits, result, the spy's in-step counts of that head)}."""
    from openpsg_amd import _lib
    g, cfg, w, scene = _g6()
    inp, N = _inputs(scene), len(scene["object_id_list"])
    outs = {}
    for flag in (0, 1):
        _reset(steps)
        _lib.set_option(0, name, flag)
        try:
            head = _head(cfg, w, dtype, llm_decode="constrained", llm_rel_scores="likelihood")
            check(head.llm_engine, flag)
            outs[flag] = _three_runs(head, inp) + (dict(steps),)
            _assert_one_candidate_per_pair(outs[flag][3], head.last, head.relation_trie(), N)
            torch.cuda.synchronize()
        finally:
            _lib.set_option(0, name, 0)
        head.llm_engine._graphs.clear()
        del head
        gc.collect()
        torch.cuda.empty_cache()
    assert np.array_equal(outs[0][0], outs[1][0]), f"{name}: tokens differ between the option's two settings"
    assert torch.equal(outs[0][1], outs[1][1]), f"{name}: path log-probabilities differ"
    assert torch.equal(outs[0][2], outs[1][2]), f"{name}: first-step logits differ"
    assert torch.isfinite(outs[1][1]).all() and (outs[1][1] < 0).all()
    return outs, M.relation_trie(cfg).max_depth + 1, cfg.llm.layers


def test_c_constrained_on_the_persistent_decoder_layer(monkeypatch):
    """G6 in fp32 with decode_persistent 0 and 1: tokens, path log-probability and first-step logits bit-equal between the
    launch chain and psg_decode_layers, over a capture and two replays; the engine follows the flag and takes the route
    (one launch of the layer stack per step)."""
    from openpsg_amd import ops
    m = _g6()[1].llm
    if not ops.decode_layer_supported(20, m.hidden, m.inter, m.heads, torch.float32, DEV):
        pytest.skip("psg_decode_layer needs a 256-CU device")
    calls, steps = _spy(monkeypatch, ("decode_layers", "trie_greedy_step", "greedy_step"))

    def check(eng, flag):
        assert eng.persistent_layer == bool(flag) and eng._can_persist(20, 0) == bool(flag)
    outs, T, layers = _with_option("decode_persistent", "fp32", steps, check)
    for flag in (0, 1):                                                # warm-up + capture
        assert outs[flag][4] == dict(decode_layers=2 * (T - 1) * flag, trie_greedy_step=2 * (T - 1), greedy_step=0)


def test_d_constrained_on_the_fused_route(monkeypatch):
    """G6 in bf16 with llm_fuse_rmsnorm 0 and 1: tokens and path log-probability (and the prompt pass's first-step logits)
    bit-equal - `_decode_step_fused` documents bit-identity with the separate kernels - over a capture and two replays;
    `_can_fuse` follows the option and every RMSNorm of a step runs inside its projection."""
    calls, steps = _spy(monkeypatch, ("skinny_gemm_fused", "trie_greedy_step", "greedy_step"))

    def check(eng, flag):
        assert eng._can_fuse(20) == bool(flag) and not eng._can_persist(20, 0)
    outs, T, layers = _with_option("llm_fuse_rmsnorm", "bf16", steps, check)
    for flag in (0, 1):
        assert outs[flag][4] == dict(skinny_gemm_fused=2 * (T - 1) * (2 * layers + 1) * flag, trie_greedy_step=2 * (T - 1),
                                     greedy_step=0)
    _G6.clear()                                                        # G6 is used by C and D alone


# ---- E. constrained above 32 rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,opt,entries", [
    (None, dict(llm_batch_split_gemm="own"), ("batch_split_gemm_w16", "batch_split_gemm_w32")),
    ("fp8", dict(llm_batch_weight_stream="quantised"), ("batch_split_gemm_w8",)),
    ("mxfp4", dict(llm_batch_weight_stream="quantised"), ("batch_split_gemm_w4", "batch_split_gemm_w8"))],
    ids=["own-split-gemm", "fp8-byte-stream", "mxfp4-nibble-stream"])
def test_e_constrained_forward_batch_of_40_rows(fmt, opt, entries, monkeypatch):
    """G1 in fp32s, forward_batch([inp, inp]): the 40-row decode steps run on psg_batch_gemm_s / psg_batch_gemm_q, each
    image's tokens agree with the single-image run up to each pair's first near-tie (margins of the oracle on W'), every
    pair yields one valid candidate and the two images are identical."""
    case, dtype = M.G1, "fp32s"
    g, cfg, w, scene = M.load(case)
    inp, N = _inputs(scene), len(scene["object_id_list"])
    calls, steps = _spy(monkeypatch, STEP_KERNELS + ALL_STREAMS + BATCH)
    head = _head(cfg, w, dtype, llm_decode="constrained", **_quant_kw(fmt, False), **opt)
    trie = head.relation_trie()
    T = trie.max_depth + 1
    r1 = head(inp)
    assert all(calls[n] == 0 for n in BATCH)                           # 20 rows: the <= 32-row routes
    last = dict(head.last)
    t1 = np.asarray(last["tokens_host"]).copy()
    K = t1.shape[0]
    _assert_one_candidate_per_pair(r1, last, trie, N)
    ref, _, margin = _oracle(case, dtype, fmt, False, cfg, w, last["llm_inputs"], _seq_len(cfg, last), trie)
    whole = _agree_up_to_near_ties(f"{case} {fmt} single image", t1, ref, margin)
    assert len(whole) >= 0.9 * K
    assert head.llm_engine.decode_uses_library(2 * K) and not head.llm_engine._can_w8(2 * K)
    _reset(calls, steps)
    rb = head.forward_batch([inp, inp])
    assert sum(steps[n] for n in entries) > 0 and (fmt is None or steps[entries[0]] > 0), steps
    assert all(calls[n] == 0 for n in BATCH if n not in entries), calls
    assert all(steps[n] == 0 for n in ALL_STREAMS), steps               # no <= 32-row entry in a 40-row step
    assert calls["trie_greedy_step"] == 2 * T and calls["greedy_step"] == 0
    assert len(rb) == 2 and len(head.last_batch) == 2
    tb = [np.asarray(lb["tokens_host"]).copy() for lb in head.last_batch]
    for i in range(2):
        same = _agree_up_to_near_ties(f"{case} {fmt} image {i} of the batch", tb[i], t1[:, :T], margin)
        print(f"{case} fp32s {fmt}: image {i}: {len(same)} of {K} paths equal to the single image's")
        _assert_one_candidate_per_pair(rb[i], head.last_batch[i], trie, N)
        assert rb[i]["rel_score"] == [1] * K
        if np.array_equal(tb[i], t1):
            assert rb[i] == r1
    assert np.array_equal(tb[0], tb[1]) and rb[0] == rb[1]             # a row sees neither its neighbours nor their number
    n = {k: calls[k] for k in BATCH}
    assert head.forward_batch([inp, inp]) == rb and {k: calls[k] for k in BATCH} == n     # the graph's replay


# ---- F. the row-count boundary and the graph cache, on the engine ---------------------------------------------------
def _fp8_engine():
    g, cfg, w, scene = M.load(M.G1)
    head = _head(cfg, w, "fp32s", llm_weight_quant="fp8")
    head(_inputs(scene))
    last = dict(head.last)
    return cfg, w, head, last["llm_inputs"].clone(), last["prompt_len"].clone()


def test_f_row_count_boundary_of_the_quantised_route(monkeypatch):
    """G1 in fp32s + fp8, `eng.generate(constraint=, path_logp=True)` on the 20 LLM input rows tiled to K = 1, 32 and 33.
    Within one call duplicated rows give bit-equal tokens and path log-probability at every K.  K <= 32 takes
    psg_split_gemm_w8 in every step, K = 33 none of it (`_can_w8` / `decode_uses_library` say so, the spy confirms).
    Every K's tokens equal the oracle's on W' up to each pair's first near-tie and its path log-probability is within 2e-4
    of the oracle's (the bar of part A).
    Across calls: K = 32 equals K = 20 BIT FOR BIT on the shared rows.  The decode steps compute a row from that row alone
    whatever the row count (psg_split_gemm_w8, the row kernels, the trie step); the prompt pass is a library product whose
    kernel may follow the row count (what `row_invariant` exists to rule out), and at this model's reductions of 256 and
    512 its 960-row and 1536-row results are measured equal.  K = 33 leaves the stream for the dense path on W' (another
    summation order), K = 1 has a 48-row prompt pass: both are held to agreement up to near-ties, by design no more, and
    whether they came out bit-equal is printed.
    Measured on an MI355X: |logp - oracle| 9.0e-6 at K = 20, 32, 33 and 2.5e-6 at K = 1; K = 1 and K = 32 bit-equal to
    K = 20, K = 33 not (|logp difference| 7.7e-6)."""
    cfg, w, head, X, plen = _fp8_engine()
    eng, trie = head.llm_engine, M.relation_trie(cfg)
    T = trie.max_depth + 1
    seq_len = plen.cpu().numpy() + cfg.qformer.num_query
    ref, want, margin = _oracle(M.G1, "fp32s", "fp8", False, cfg, w, X, seq_len, trie)
    calls, steps = _spy(monkeypatch, STEP_KERNELS + ALL_STREAMS + BATCH)
    outs = {}
    for K in (20, 1, 32, 33):
        idx = torch.arange(K, device=DEV) % 20
        rows = idx.cpu().numpy()
        stream = K <= 32
        assert eng._can_w8(K) == stream and eng.decode_uses_library(K) == (not stream)
        _reset(calls, steps)
        tok, _, logp = eng.generate(X[idx].contiguous(), plen[idx].contiguous(), constraint=trie, path_logp=True)
        torch.cuda.synchronize()
        per_step = 4 * cfg.llm.layers                                  # warm-up + capture
        assert steps["split_gemm_w8"] == (2 * (T - 1) * per_step if stream else 0), (K, steps)
        assert all(calls[n] == 0 for n in ALL_STREAMS + BATCH if n != "split_gemm_w8") and calls["greedy_step"] == 0
        assert calls["trie_greedy_step"] == 2 * T
        tok, logp = tok.cpu().numpy()[:, :T], logp.double().cpu().numpy()
        for k in range(20, K):                                         # duplicates within the call
            assert np.array_equal(tok[k], tok[k - 20]) and logp[k] == logp[k - 20], f"K={K}: row {k} != row {k - 20}"
        whole = _agree_up_to_near_ties(f"K={K}", tok, ref[rows], margin[rows])
        err = np.abs(logp[whole] - want[rows][whole]).max()
        print(f"G1 fp32s fp8, K={K}: {len(whole)} of {K} paths equal to the oracle's, |logp - oracle| {err:.3e} (bound 2e-4)")
        assert len(whole) >= 0.9 * K and err <= 2e-4
        tok2, _, logp2 = eng.generate(X[idx].contiguous(), plen[idx].contiguous(), constraint=trie, path_logp=True)
        assert np.array_equal(tok2.cpu().numpy()[:, :T], tok) and np.array_equal(logp2.double().cpu().numpy(), logp)
        outs[K] = (tok, logp)
    for K in (1, 32, 33):
        n = min(K, 20)
        _agree_up_to_near_ties(f"K={K} against K=20", outs[K][0][:n], outs[20][0][:n], margin[:n])
        bits = np.array_equal(outs[K][0][:n], outs[20][0][:n]) and np.array_equal(outs[K][1][:n], outs[20][1][:n])
        print(f"G1 fp32s fp8, K={K} against K=20 on the shared rows: bit-equal {bits}, |logp difference| "
              f"{np.abs(outs[K][1][:n] - outs[20][1][:n]).max():.3e}")
        assert bits or K != 32, "K = 32 and K = 20 differ on the shared rows: the <= 32-row route is not row-count invariant"


def test_f_one_engine_serves_every_call_kind_from_its_graph_cache():
    """One engine (G1, fp32s + fp8), one X: greedy, constrained, constrained + path_logp, likelihood and constrained +
    likelihood + path_logp calls interleaved twice over.  Every call returns, bit for bit, what the same call returns on a
    fresh engine without graphs, and the second round equals the first: no two of them share a graph."""
    cfg, w, head, X, plen = _fp8_engine()
    eng, trie = head.llm_engine, M.relation_trie(cfg)
    kinds = [dict(), dict(constraint=trie), dict(constraint=trie, path_logp=True), dict(trie=trie),
             dict(constraint=trie, trie=trie, path_logp=True)]
    g, cfg, w, scene = M.load(M.G1)
    fresh = _head(cfg, w, "fp32s", llm_weight_quant="fp8").llm_engine
    fresh.use_graph = False
    want = []
    for kw in kinds:
        out = fresh.generate(X, plen, return_first_logits=True, **kw)
        torch.cuda.synchronize()
        want.append([o.clone() for o in out])
    assert [len(o) for o in want] == [2, 2, 3, 3, 4]
    assert not torch.equal(want[0][0], want[1][0])                     # the free decode is not a relation: the kinds differ
    assert torch.equal(want[1][0], want[2][0]) and torch.equal(want[2][0], want[4][0])
    assert torch.equal(want[3][0], want[0][0]) and torch.equal(want[3][2], want[4][2])
    assert torch.equal(want[2][2], want[4][3])
    eng._graphs.clear()
    for rnd in range(2):
        for i, kw in enumerate(kinds):
            out = eng.generate(X, plen, return_first_logits=True, **kw)
            torch.cuda.synchronize()
            assert len(out) == len(want[i]), f"round {rnd}, call {i}"
            for j, (a, b) in enumerate(zip(out, want[i])):
                assert a.dtype == b.dtype and torch.equal(a, b), f"round {rnd}, call {i} ({sorted(kw)}), output {j}"
        assert len(eng._graphs) == len(kinds)
    for order in ([4, 0, 2, 3, 1], [1, 1, 0, 0]):                      # another order, and back-to-back repeats
        for i in order:
            out = eng.generate(X, plen, return_first_logits=True, **kinds[i])
            assert all(torch.equal(a, b) for a, b in zip(out, want[i])), f"call {i}"
    assert len(eng._graphs) == len(kinds)
