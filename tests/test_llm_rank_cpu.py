"""llm_rel_scores='likelihood' without a GPU: the token trie over the relation classes' candidate sequences (WordTokenizer
and tests/helpers.py's ChainTokenizer), the checks that refuse a tokenizer whose candidates collide or do not round-trip
through decode + parse, output assembly from given log scores, and the option errors."""
import numpy as np
import pytest

from openpsg_amd._lib import PsgHipError
from openpsg_amd.categories import relation_categories
from openpsg_amd.config import tiny_llm
from openpsg_amd.rel_scores import RelationTrie, assemble, candidate_ids
from openpsg_amd.tokenizers import WordTokenizer
from tests import helpers as H


def _head(tokenizers="word", **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    llm = tiny_llm(256, 2, 512, 512)
    return RelationTransformerHeadV4(dtype="fp32", device="cpu", qformer_vocab_size=512, llm_config=llm,
                                     llm_feature_size=256, tokenizers=tokenizers, **kw)


def _check_trie(head, tok):
    t = head.relation_trie()
    eos = head.cfg.llm.eos
    R = len(relation_categories)
    assert len(t.candidates) == R
    for r, c in enumerate(t.candidates):
        assert c == candidate_ids(tok, relation_categories[r], eos) and c[-1] == eos and eos not in c[:-1]
        # what generate must emit for parse to return exactly {r}
        pred, _ = head.parse(np.array([c]), np.array([7]), 10)
        assert pred == [[0, 7, r]], relation_categories[r]
    # shared prefixes merged: one node per distinct proper prefix
    prefixes = {tuple(c[:j]) for c in t.candidates for j in range(1, len(c))}
    assert t.n_int == len(prefixes)
    assert t.n_edges == t.n_int + R                     # every node has one incoming edge, every class one leaf
    for i in range(t.n_int):
        d = int(t.node_depth[i])
        chain = [a for a in t.anc[i] if a >= 0]
        assert len(chain) == d and chain[-1] == i
        assert all(int(t.node_depth[a]) == j + 1 for j, a in enumerate(chain))
        assert int(t.node_parent[i]) == (chain[-2] if d > 1 else -1)
        assert list(t.anc[i][d:]) == [-1] * (t.anc.shape[1] - d)
    # every class's path: root -> its prefixes -> its EOS leaf, edges carrying its tokens in order
    for r, c in enumerate(t.candidates):
        edges = [e for e in t.path[r] if e < t.n_edges]
        assert [int(t.child_tok[e]) for e in edges] == c
        assert int(t.edge_node[edges[-1]]) == -1
    seq_len = np.array([40, 45, 33])
    rp = t.rope_pos(seq_len)
    assert rp.shape == (3, t.n_int)
    assert (rp == seq_len[:, None] + t.node_depth[None, :] - 1).all()
    return t


def test_word_tokenizer_trie():
    h = _head(llm_rel_scores="likelihood")
    t = _check_trie(h, h.llm_tokenizer)
    assert t.n_int == 76 and t.max_len == 4                  # the 56 PSG classes: 76 rows per pair, at most 4 tokens
    # 'in front of' and 'in' share the prefix 'in'
    c_in, c_front = t.candidates[relation_categories.index("in")], t.candidates[relation_categories.index("in front of")]
    assert c_in[0] == c_front[0]


def test_chain_tokenizer_trie():
    tok = H.ChainTokenizer()
    h = _head(tokenizers=(WordTokenizer("bert"), tok), llm_rel_scores="likelihood")
    _check_trie(h, tok)


class _Collide(WordTokenizer):
    """'on' and 'over' become the same id."""

    def __init__(self):
        super().__init__("llama")
        self.piece_to_id["over"] = self.piece_to_id["on"]


class _Lossy(WordTokenizer):
    """'walking' decodes to 'running'."""

    def __init__(self):
        super().__init__("llama")

    def decode(self, ids):
        return super().decode(ids).replace("walking", "running")


def test_colliding_candidates_raise_and_name_the_classes():
    with pytest.raises(PsgHipError, match="'on'.*'over'|'over'.*'on'"):
        _head(tokenizers=(WordTokenizer("bert"), _Collide()), llm_rel_scores="likelihood")


def test_non_round_tripping_candidate_raises_and_names_the_class():
    with pytest.raises(PsgHipError, match="'walking on'"):
        _head(tokenizers=(WordTokenizer("bert"), _Lossy()), llm_rel_scores="likelihood")


def test_tokenizer_change_rebuilds_and_checks_the_trie():
    h = _head(llm_rel_scores="likelihood")
    t0 = h.relation_trie()
    assert h.relation_trie() is t0
    h.llm_tokenizer = _Collide()
    with pytest.raises(PsgHipError, match="'over'"):
        h.relation_trie()


def test_duplicate_leaves_are_reported():
    t = RelationTrie(["a", "b", "c"], [[5, 2], [6, 2], [5, 2]], 2)
    assert t.duplicates() == [[0, 2]]


def test_assemble_orders_and_deduplicates():
    K, R, N = 3, 4, 10
    ls = np.log(np.array([[0.10, 0.30, 0.05, 0.20],
                          [0.30, 0.01, 0.30, 0.02],
                          [0.25, 0.25, 0.07, 0.03]]))
    sel = np.array([12, 3, 27])
    gen = [(1, [3 // N, 3 % N, 2]), (0, [1, 2, 1])]
    pred, score = assemble(gen, ls, sel, N, 5)
    # generated first, in parse order, re-scored
    assert pred[:2] == [[0, 3, 2], [1, 2, 1]]
    assert score[:2] == pytest.approx([0.30, 0.30])
    assert all(isinstance(s, float) for s in score)
    # then the 5 best remaining: (k1, r0) 0.30 (its r2 was generated); the 0.25 tie of k2 -> r0 before r1; (k0, r3)
    # 0.20; (k0, r0) 0.10 - (k0, r1) 0.30 was generated
    assert pred[2:] == [[0, 3, 0], [2, 7, 0], [2, 7, 1], [1, 2, 3], [1, 2, 0]]
    assert score[2:] == pytest.approx([0.30, 0.25, 0.25, 0.20, 0.10])


def test_assemble_tie_rule_and_limits():
    ls = np.log(np.full((2, 3), 0.2))
    sel = np.array([4, 1])
    pred, _ = assemble([], ls, sel, 3, 4096)
    assert pred == [[1, 1, 0], [1, 1, 1], [1, 1, 2], [0, 1, 0], [0, 1, 1], [0, 1, 2]]
    pred, score = assemble([(0, [1, 1, 2])], ls, sel, 3, 0)          # N = 0 adds nothing
    assert pred == [[1, 1, 2]] and score == pytest.approx([0.2])
    pred, _ = assemble([], ls, sel, 3, 2)
    assert len(pred) == 2


def test_option_errors():
    with pytest.raises(PsgHipError, match="no LLM stage"):
        _head(rel_cls_type="multiclass", llm_rel_scores="likelihood")
    with pytest.raises(PsgHipError, match="needs llm_rel_scores='likelihood'"):
        _head(num_llm_ranked_triples=5)
    with pytest.raises(PsgHipError, match="0..4096"):
        _head(llm_rel_scores="likelihood", num_llm_ranked_triples=4097)
    with pytest.raises(PsgHipError, match="'constant' or 'likelihood'"):
        _head(llm_rel_scores="softmax")
    with pytest.raises(PsgHipError, match="implicit_bos=True"):
        _head(llm_rel_scores="likelihood", implicit_bos=False, on_parse_error="skip")
    h = _head(llm_rel_scores="likelihood", num_llm_ranked_triples=4096)
    assert h.num_llm_ranked_triples == 4096
    assert _head().llm_rel_scores == "constant"


def test_batch_and_sharded_paths_refuse_likelihood():
    from openpsg_amd.dist import HipBackend
    h = _head(llm_rel_scores="likelihood")
    with pytest.raises(PsgHipError, match="forward_batch"):
        h.forward_batch([])
    with pytest.raises(PsgHipError, match="pair-sharded"):
        HipBackend(h)
