"""llm_beam_width without a GPU: the option's default and refusals, the ABI of psg_trie_beam_step, the
trie's `edge_class` table, `parse_beam`'s ordering, the numpy restatement of the beam (tests/trie_beam_ref.py), and the
precondition of the GPU comparisons: on the goldens the oracle's own beam has no near-tie, so that a GPU beam can be
compared with it entry by entry."""
import os
import re

import numpy as np
import pytest
import torch

from openpsg_amd import _lib
from openpsg_amd._lib import PsgHipError
from openpsg_amd.config import tiny_llm
from tests import beam_oracle as BO
from tests import trie_beam_ref as BR
from tests import trie_walk_ref as W
from tests.test_gpu_llm_constrained import NEAR_TIE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the (case, beam widths) of tests/test_gpu_llm_beam.py
GPU_CASES = [("G1_c1_512_n10", (3, 8)), ("G8_gqa_512_n10", (3, 8))]
WIDTHS = (2, 3, 4, 5, 8)


def _head(llm=None, **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    llm = tiny_llm(256, 2, 512, 512) if llm is None else llm
    return RelationTransformerHeadV4(dtype="fp32", device="cpu", qformer_vocab_size=512, llm_config=llm,
                                     llm_feature_size=llm.hidden, tokenizers="word", **kw)


BEAM = dict(llm_decode="constrained", llm_rel_scores="likelihood")


# ---- 1. the option --------------------------------------------------------------------------------------------------
def test_default_is_one_and_a_width_is_accepted():
    assert _head().llm_beam_width == 1
    assert _head(llm_beam_width=1, llm_decode="constrained").llm_beam_width == 1     # 1 needs nothing
    for b in (2, 8):
        assert _head(llm_beam_width=b, **BEAM).llm_beam_width == b
    assert _head(llm_beam_width=8, num_selected=20, **BEAM).cfg.num_selected == 20   # 160 rows: the most


@pytest.mark.parametrize("bad", [0, 9, -1, 2.0, "3", True, None])
def test_width_must_be_an_int_in_range(bad):
    with pytest.raises(PsgHipError, match="llm_beam_width must be an int in 1..8"):
        _head(llm_beam_width=bad, **BEAM)


def test_refusals_name_the_option():
    with pytest.raises(PsgHipError, match="llm_beam_width=3.*llm_decode='constrained'"):
        _head(llm_beam_width=3, llm_rel_scores="likelihood")
    with pytest.raises(PsgHipError, match="llm_beam_width=3.*llm_rel_scores='likelihood'"):
        _head(llm_beam_width=3, llm_decode="constrained")
    with pytest.raises(PsgHipError, match="llm_beam_width=3.*num_llm_ranked_triples=5"):
        _head(llm_beam_width=3, num_llm_ranked_triples=5, **BEAM)
    with pytest.raises(PsgHipError, match="llm_beam_width=8.*21 selected pairs x 8.*168 rows.*160"):
        _head(llm_beam_width=8, num_selected=21, **BEAM)
    with pytest.raises(PsgHipError, match="llm_beam_width=5.*33 selected pairs x 5.*165 rows.*160"):
        _head(llm_beam_width=5, pair_selector="threshold", max_selected=33, **BEAM)
    assert _head(llm_beam_width=5, max_selected=33, **BEAM).llm_beam_width == 5      # max_selected counts under 'threshold' only
    with pytest.raises(PsgHipError, match="forward_batch.*llm_beam_width=3"):
        _head(llm_beam_width=3, **BEAM).forward_batch([])


def test_existing_refusals_stay():
    from openpsg_amd.dist import HipBackend
    with pytest.raises(PsgHipError, match="llm_decode must be 'greedy' or 'constrained'"):
        _head(llm_decode="beam")
    with pytest.raises(PsgHipError, match="forward_batch"):
        _head(**BEAM).forward_batch([])
    with pytest.raises(PsgHipError):
        HipBackend(_head(llm_beam_width=3, **BEAM))


def test_infer_tool_has_the_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location("infer_tool", os.path.join(ROOT, "tools", "infer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = open(os.path.join(ROOT, "tools", "infer.py")).read()
    assert "--llm-beam-width" in src
    assert mod._beam_options(type("A", (), dict(llm_beam_width=1))()) == {}
    assert mod._beam_options(type("A", (), dict(llm_beam_width=4))()) == dict(llm_beam_width=4, llm_rel_scores="likelihood")


# ---- 2. ABI and tables ----------------------------------------------------------------------------------------------
def test_abi_614_declares_binds_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "psg_hip.h")).read()
    m = re.search(r"#define PSG_ABI_VERSION (\d+)", hdr)
    lib = _lib.load()
    assert int(m.group(1)) == _lib.PSG_ABI_VERSION == lib.psg_version() >= 614
    decl = re.search(r"\bint psg_trie_beam_step\(psg_ctx\*(.*?)\);", hdr, re.S)
    assert decl
    n_args = 1 + decl.group(1).count(",")
    assert len(_lib.SIGNATURES["psg_trie_beam_step"]) == n_args == 33
    fn = lib.psg_trie_beam_step
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
    from openpsg_amd import ops
    assert callable(ops.trie_beam_step)


def test_trie_device_tables_carry_edge_class():
    for t in (W.hand_trie(512), BR.wide_trie(512), _head(**BEAM).relation_trie()):
        d = t.device("cpu")
        assert d["edge_class"].dtype == torch.int32 and d["edge_class"].numel() == t.n_edges
        assert d["edge_node"].tolist() == t.edge_node.tolist()                       # the other keys stay
        assert {"node_tok", "node_depth", "anc", "child_off", "child_tok", "path"} <= set(d)
        want = np.full(t.n_edges, -1)
        for (src, tok), rs in t._leaf_of.items():
            c = [c for c in range(t.child_off[src], t.child_off[src + 1]) if t.child_tok[c] == tok][0]
            want[c] = rs[0]
        assert d["edge_class"].tolist() == want.tolist()
        assert ((want >= 0) == (t.edge_node < 0)).all()                              # a leaf edge completes exactly one class
        assert sorted(want[want >= 0].tolist()) == list(range(len(t.candidates)))
        assert d["max_children"] == max(t.child_off[n + 1] - t.child_off[n] for n in range(t.n_int + 1))


# ---- 3. parse_beam --------------------------------------------------------------------------------------------------
def test_parse_beam_order_and_scores():
    h = _head(llm_beam_width=3, **BEAM)
    N = 5
    sel = np.array([7, 3, 11])                                # pairs (1, 2), (0, 3), (2, 1)
    cls = np.array([[4, 9, 2], [1, 0, -1], [6, 5, 8]])
    lp = np.array([[-1.0, -2.0, -4.0], [-3.0, -2.0, -np.inf], [-0.5, -2.0, -2.0]], dtype=np.float32)
    pred, score = h.parse_beam(cls, lp, sel, N)
    # each pair's best in selection order; then by score: -2 (pair 0, class 9), -2 (pair 1, class 0), -2 (pair 2, class 5
    # before class 8: lower class), -4
    assert pred == [[1, 2, 4], [0, 3, 1], [2, 1, 6], [1, 2, 9], [0, 3, 0], [2, 1, 5], [2, 1, 8], [1, 2, 2]]
    assert score == [float(np.exp(np.float64(v))) for v in (-1.0, -3.0, -0.5, -2.0, -2.0, -2.0, -2.0, -4.0)]
    assert all(isinstance(s, float) and 0.0 < s <= 1.0 for s in score)
    assert len({tuple(t) for t in pred}) == len(pred) == 8    # the -1 padded entry is no triple
    out = dict(beam_class_host=cls, beam_logp_host=lp, selected_host=sel)
    assert h._parse_out(out, N) == (pred, score)


# ---- the numpy beam -------------------------------------------------------------------------------------------------
def test_level_step_rules():
    t = W.hand_trie(512)
    kids0 = {int(t.child_tok[c]): c for c in range(t.child_off[0], t.child_off[1])}
    n10, n20 = int(t.edge_node[kids0[10]]) + 1, int(t.edge_node[kids0[20]]) + 1
    # root: three non-leaf children; B = 2 keeps the two best, ties to the lower edge
    r = BR.level_step(t, 2, [(0, 0.0)], [], lambda b, c: {10: -1.0, 20: -1.0, 511: -3.0}[int(t.child_tok[c])])
    assert [(n, v) for n, v, _, _ in r["live"]] == [(n10, -1.0), (n20, -1.0)] and r["fin"] == []
    assert r["live_gap"] == 0.0 and r["fin_gap"] == np.inf and r["n_live_pool"] == 3
    # two beams with the same node and score: the lower beam first; EOS edges finish classes 0 / 1; node 20's child 21 lives
    tab = {W.EOS: -0.5, 21: -0.25}
    r = BR.level_step(t, 2, [(n20, -1.0), (n20, -1.0), (-1, 0.0), (n10, -2.0)], [(3, -1.75), (2, -9.0)],
                      lambda b, c: tab[int(t.child_tok[c])])
    assert [(b, v) for _, v, b, _ in r["live"]] == [(0, -1.25), (1, -1.25)]
    assert [v for _, v in r["fin"]] == [-1.5, -1.5] and r["fin"][0][0] == 1      # class 1 twice (the two beams), both above -1.75
    # a dropped edge (NaN, -inf, None) is no candidate
    r = BR.level_step(t, 3, [(0, 0.0)], [], lambda b, c: {10: np.nan, 20: -np.inf, 511: None}[int(t.child_tok[c])])
    assert r["live"] == [] and r["fin"] == [] and r["n_live_pool"] == 0


def test_search_is_the_exact_top_b_when_no_level_prunes():
    rng = np.random.default_rng(3)
    for t in (W.hand_trie(512), BR.wide_trie(512)):
        table = -rng.random(t.n_edges) * 5
        full = BR.path_scores(t, table)
        wide = max(int(np.sum(t.node_depth == d)) for d in range(1, t.max_depth + 1))
        for B in (1, 2, 3, 8):
            cls, sc, gaps, exact = BR.search(t, B, table)
            n = min(B, len(full))
            assert (cls[:n] >= 0).all() and (cls[n:] == -1).all() and len(set(cls[:n].tolist())) == n
            assert np.allclose(sc[:n], full[cls[:n]], atol=1e-12) and (np.diff(sc[:n]) <= 0).all()
            assert exact == (B >= wide) and len(gaps) == t.max_depth + 1
            if exact:                                         # no level held more than B nodes: the top-B classes
                assert cls[:n].tolist() == np.argsort(-full, kind="stable")[:n].tolist()
            else:                                             # pruned: still real classes with their own scores
                assert sc[0] <= full.max() + 1e-12
    cls1, sc1, _, _ = BR.search(W.hand_trie(512), 1, np.zeros(10))
    assert cls1[0] == 0 and sc1[0] == 0.0                     # all equal: the lower edge at every level


# ---- 4. the precondition of the GPU comparisons ---------------------------------------------------------------------
@pytest.mark.parametrize("case,gpu_widths", GPU_CASES)
def test_oracle_beam_has_no_near_tie_on_the_goldens(case, gpu_widths):
    g, cfg, w, scene = BO.load(case)
    trie = _head(cfg.llm, **BEAM).relation_trie()
    xs, seq_len = BO.oracle_llm_inputs(g, cfg, w, scene)
    table = BO.edge_table(cfg, w, xs, seq_len, trie)
    K = len(xs)
    assert K == 20 and np.isfinite(table).all() and (table < 0).all()
    assert set(gpu_widths) <= set(WIDTHS)
    for B in WIDTHS:
        gaps = np.array([BR.search(trie, B, table[k])[2].min() for k in range(K)])
        near = int((gaps < NEAR_TIE).sum())
        print(f"{case} B={B}: {near} of {K} pairs with a gap under {NEAR_TIE:g}, smallest gap {gaps.min():.2e}")
        assert near <= 0.1 * K
