"""llm_decode='constrained' without a GPU: the option's refusals and default, the ABI of psg_trie_greedy_step, the trie's
device tables, and the numpy restatement of the constrained walk (tests/trie_walk_ref.py) that the GPU tests use as their
reference."""
import os
import re

import numpy as np
import pytest
import torch

from openpsg_amd import _lib
from openpsg_amd._lib import PsgHipError
from openpsg_amd.categories import relation_categories
from openpsg_amd.config import tiny_llm
from tests import trie_walk_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    llm = tiny_llm(256, 2, 512, 512)
    return RelationTransformerHeadV4(dtype="fp32", device="cpu", qformer_vocab_size=512, llm_config=llm,
                                     llm_feature_size=256, tokenizers="word", **kw)


def test_default_is_greedy_and_constrained_is_accepted():
    assert _head().llm_decode == "greedy"
    h = _head(llm_decode="constrained")
    assert h.llm_decode == "constrained"
    t = h.relation_trie()                                    # built and checked at construction
    assert len(t.candidates) == len(relation_categories) and t.max_depth + 1 == 4
    assert _head(llm_decode="constrained", llm_rel_scores="likelihood", num_llm_ranked_triples=3).llm_decode == "constrained"
    assert _head(llm_decode="constrained", max_new_tokens=4).cfg.max_new_tokens == 4


def test_option_refusals_name_the_option():
    with pytest.raises(PsgHipError, match="llm_decode must be 'greedy' or 'constrained'"):
        _head(llm_decode="beam")
    with pytest.raises(PsgHipError, match="llm_decode='constrained'.*no LLM stage"):
        _head(rel_cls_type="multiclass", llm_decode="constrained")
    with pytest.raises(PsgHipError, match="llm_decode='constrained'.*implicit_bos=True"):
        _head(llm_decode="constrained", implicit_bos=False, on_parse_error="skip")
    with pytest.raises(PsgHipError, match="llm_decode='constrained'.*suppress_eos=True"):
        _head(llm_decode="constrained", suppress_eos=True)
    with pytest.raises(PsgHipError, match="llm_decode='constrained'.*max_new_tokens=3"):
        _head(llm_decode="constrained", max_new_tokens=3)     # the 56 PSG classes need max_depth + 1 = 4 steps


def test_batch_keeps_refusing_likelihood_and_sharded_refuses_constrained():
    from openpsg_amd.dist import HipBackend
    with pytest.raises(PsgHipError, match="forward_batch"):
        _head(llm_decode="constrained", llm_rel_scores="likelihood").forward_batch([])
    with pytest.raises(PsgHipError, match="llm_decode='constrained'"):
        HipBackend(_head(llm_decode="constrained"))


def test_abi_611_declares_binds_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "psg_hip.h")).read()
    m = re.search(r"#define PSG_ABI_VERSION (\d+)", hdr)
    lib = _lib.load()
    assert int(m.group(1)) == _lib.PSG_ABI_VERSION == lib.psg_version() >= 611
    assert re.search(r"\bint psg_trie_greedy_step\(psg_ctx\*", hdr)
    assert len(_lib.SIGNATURES["psg_trie_greedy_step"]) == 26
    fn = lib.psg_trie_greedy_step                            # exported by the library, bound with its argument list
    assert fn.argtypes is not None and len(fn.argtypes) == 26
    from openpsg_amd import ops
    assert callable(ops.trie_greedy_step)


def test_trie_device_tables_carry_edge_node():
    t = W.hand_trie(512)
    d = t.device("cpu")
    assert d["edge_node"].dtype == torch.int32 and d["edge_node"].numel() == t.n_edges == d["child_tok"].numel()
    assert d["edge_node"].tolist() == t.edge_node.tolist()
    assert d["child_off"].numel() == t.n_int + 2


def test_hand_trie_has_the_shapes_the_kernel_test_needs():
    t = W.hand_trie(512)
    kids = lambda n: {int(t.child_tok[c]): int(t.edge_node[c]) for c in range(t.child_off[n], t.child_off[n + 1])}  # noqa: E731
    assert sorted(kids(0)) == [10, 20, 511]                  # a root with three children
    n10, n20, nhi = kids(0)[10] + 1, kids(0)[20] + 1, kids(0)[511] + 1
    assert kids(n10) == {W.EOS: -1}                          # a node whose only child is EOS
    assert sorted(kids(n20)) == [W.EOS, 21] and kids(n20)[W.EOS] == -1 and kids(n20)[21] >= 0
    assert list(kids(nhi)) == [31] and kids(nhi)[31] >= 0    # a node with a single, non-EOS child
    assert t.max_depth == 3


def test_walk_step_rules():
    t = W.hand_trie(512)
    kids0 = {int(t.child_tok[c]): c for c in range(t.child_off[0], t.child_off[1])}
    n20 = int(t.edge_node[kids0[20]]) + 1
    v = np.zeros((7, 512), dtype=np.float32)
    node = np.array([0, 0, n20, 0, 0, 99, 0])
    done = np.array([0, 0, 0, 0, 1, 0, 0])
    v[0, [10, 20, 511]] = [1.5, 1.5, 1.0]                    # equal logits: the lower token id
    v[0, 7] = 50.0                                           # a non-child holds the global maximum: ignored
    v[1, [10, 20, 511]] = [-np.inf, -2.0, -3.0]              # a child at -inf
    v[2, [W.EOS, 21]] = [0.25, 0.5]                          # EOS child against a non-EOS child
    v[3, :] = np.nan                                         # all NaN: the child with the lowest token id
    v[6, [10, 20, 511]] = -np.inf                            # all children -inf: the lowest token id too
    r = W.walk_step(v, t, node, done)
    assert r["tok"].tolist() == [10, 20, 21, 10, -1, -1, 10]
    assert r["emit"].tolist() == [10, 20, 21, 10, W.EOS, W.EOS, 10]
    assert r["done"].tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert r["node"][4] == 0 and r["node"][5] == 99          # a finished / out-of-range row keeps its state
    assert r["node"][0] == int(t.edge_node[kids0[10]]) + 1
    v[2, W.EOS] = 0.75
    r = W.walk_step(v, t, node, done)
    assert r["tok"][2] == W.EOS and r["done"][2] == 1 and r["node"][2] == n20


def test_walk_emits_one_candidate_per_row_and_its_log_probability():
    t = W.hand_trie(512)
    rng = np.random.default_rng(5)
    K = 9
    logits = rng.standard_normal((t.max_depth + 1, K, 512)).astype(np.float32)
    tokens, logp, done = W.walk(lambda s, _: logits[s], t, K)
    assert done.all()
    cands = {tuple(c) for c in t.candidates}
    for k in range(K):
        seq = [int(x) for x in tokens[k] if x >= 0]
        assert tuple(seq) in cands                           # exactly one candidate, then -1
        assert (tokens[k, len(seq):] == -1).all()
        want = sum(W.log_softmax64(logits[s, k])[tok] for s, tok in enumerate(seq))
        assert logp[k] == pytest.approx(want, abs=1e-12) and logp[k] < 0
        # greedy over the children: no other candidate with the same first token has a better first differing step
        n = 0
        for s, tok in enumerate(seq):
            kids = [int(t.child_tok[c]) for c in range(t.child_off[n], t.child_off[n + 1])]
            assert tok in kids and logits[s, k, tok] == max(logits[s, k, kids])
            c = [c for c in range(t.child_off[n], t.child_off[n + 1]) if int(t.child_tok[c]) == tok][0]
            n = int(t.edge_node[c]) + 1
