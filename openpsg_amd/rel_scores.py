"""Relation likelihoods of the LLM stage: the host side of `llm_rel_scores='likelihood'`.

For every relation class r that the head's `parse` matches against, the candidate c(r) is the LLM tokenizer's ids of the
name (no special tokens) followed by EOS: the sequence `generate` must emit for `parse` to return exactly {r}.  The
candidates form a token trie that is the same for every selected pair:

  * the root is the prompt's last row (its logits are the decode's first-step logits);
  * every proper prefix c_1..c_j (j >= 1) is an internal node = one input row per pair (token c_j at rotary position
    seq_len + j - 1, cache slot trie_base + node);
  * the EOS edges are the leaves: their probabilities are read from the parent's logits, they need no row.

log s(p, r) is the sum of the log-probabilities of the edges on r's path.  This module builds and checks the trie and
assembles the head's outputs from the [K, R] log scores; the engine pass is `LlamaDecodeEngine._rank_pass`.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import PsgHipError
from .tokenizers import WordTokenizer

MAX_RANKED_TRIPLES = 4096


def candidate_ids(tok, name: str, eos: int):
    """c(r): the tokenizer's ids for `name` without special tokens, then EOS."""
    if isinstance(tok, WordTokenizer):
        ids = list(tok.encode(name))
        if tok.style == "llama" and ids and ids[0] == tok.piece_to_id["<s>"]:
            ids = ids[1:]
    else:                                                    # a HF tokenizer object
        ids = list(tok.encode(name, add_special_tokens=False))
    return [int(t) for t in ids] + [int(eos)]


class RelationTrie:
    """Token trie over the candidates of `classes` (a list of names; class index = list index).

    n_int internal nodes, n_edges edges (root's first), max_depth = deepest internal node.  Host arrays:
      node_tok [n_int]      token a node's row inputs (its prefix's last token)
      node_depth [n_int]    1-based prefix length: rotary position seq_len + depth - 1
      node_parent [n_int]   parent internal node, -1 = root
      anc [n_int, max_depth]  the node's ancestors root-side first, the node itself last, -1 padded
      child_off [n_int + 2] / child_tok [n_edges]: children of node 0 = root and node 1 + i = internal i (CSR)
      edge_node [n_edges]   internal node an edge leads to, -1 for a leaf (EOS edge)
      edge_class [n_edges]  class a leaf edge completes (the lowest, where classes share a candidate), -1 for any other edge
      path [R, max_len]     edge indices on class r's path, padded with n_edges (a zero column)
    """

    def __init__(self, classes, candidates, eos: int):
        self.classes = list(classes)
        self.candidates = [list(c) for c in candidates]
        self.eos = int(eos)
        prefix_index = {}
        tok, depth, parent = [], [], []
        for c in self.candidates:
            for j in range(1, len(c)):
                pre = tuple(c[:j])
                if pre not in prefix_index:
                    prefix_index[pre] = len(tok)
                    tok.append(c[j - 1])
                    depth.append(j)
                    parent.append(prefix_index[pre[:-1]] if j > 1 else -1)
        self.n_int = len(tok)
        self.node_tok = np.asarray(tok, dtype=np.int32)
        self.node_depth = np.asarray(depth, dtype=np.int32)
        self.node_parent = np.asarray(parent, dtype=np.int32)
        self.max_depth = int(self.node_depth.max()) if self.n_int else 0
        self.anc = np.full((self.n_int, max(self.max_depth, 1)), -1, dtype=np.int32)
        for i in range(self.n_int):
            chain, a = [], i
            while a >= 0:
                chain.append(a)
                a = parent[a]
            self.anc[i, :len(chain)] = chain[::-1]
        # children per node (0 = root, 1 + i = internal i) in order of first appearance
        kids = [dict() for _ in range(self.n_int + 1)]
        leaf_of = {}
        for r, c in enumerate(self.candidates):
            for j in range(1, len(c) + 1):
                src = 0 if j == 1 else 1 + prefix_index[tuple(c[:j - 1])]
                if j < len(c):
                    kids[src].setdefault(c[j - 1], ("node", prefix_index[tuple(c[:j])]))
                else:
                    kids[src].setdefault(c[j - 1], ("leaf", r))
                    leaf_of.setdefault((src, c[j - 1]), []).append(r)
        off, ctok, enode, edge_of = [0], [], [], {}
        for n, d in enumerate(kids):
            for t, (kind, tgt) in d.items():
                edge_of[(n, t)] = len(ctok)
                ctok.append(t)
                enode.append(tgt if kind == "node" else -1)
            off.append(len(ctok))
        self.child_off = np.asarray(off, dtype=np.int32)
        self.child_tok = np.asarray(ctok, dtype=np.int32)
        self.edge_node = np.asarray(enode, dtype=np.int32)
        self.n_edges = len(ctok)
        self.edge_class = np.full(len(ctok), -1, dtype=np.int32)
        for (src, t), rs in leaf_of.items():
            if enode[edge_of[(src, t)]] < 0:
                self.edge_class[edge_of[(src, t)]] = min(rs)
        self.max_children = int(np.diff(self.child_off).max()) if len(ctok) else 0
        self.max_len = max(len(c) for c in self.candidates) if self.candidates else 0
        self.path = np.full((len(self.candidates), max(self.max_len, 1)), self.n_edges, dtype=np.int64)
        for r, c in enumerate(self.candidates):
            for j in range(1, len(c) + 1):
                src = 0 if j == 1 else 1 + prefix_index[tuple(c[:j - 1])]
                self.path[r, j - 1] = edge_of[(src, c[j - 1])]
        self._leaf_of = leaf_of
        self._dev = {}
        self.key = (self.n_int, self.n_edges, self.max_depth, hash(tuple(tuple(c) for c in self.candidates)))

    def duplicates(self):
        """Groups of classes that share a candidate (the same leaf)."""
        return [rs for rs in self._leaf_of.values() if len(rs) > 1]

    def rope_pos(self, seq_len):
        """Rotary position of every (pair, node) row [K, n_int] for the pairs' valid prompt lengths seq_len [K]."""
        return np.asarray(seq_len)[:, None] + self.node_depth[None, :] - 1

    def device(self, dev):
        """The trie's tables on `dev` (made once per device; the decode graphs read them by address)."""
        dev = torch.device(dev)
        ent = self._dev.get(dev)
        if ent is None:
            t = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
            ent = self._dev[dev] = dict(node_tok=t(self.node_tok), node_depth=t(self.node_depth), anc=t(self.anc),
                                        child_off=t(self.child_off), child_tok=t(self.child_tok),
                                        edge_node=t(self.edge_node), edge_class=t(self.edge_class),
                                        max_children=self.max_children,
                                        path=t(self.path, torch.int64))
        return ent


def build_relation_trie(tok, classes, eos: int, vocab: int, parse_classes):
    """The trie of `classes` under tokenizer `tok`, checked: every candidate decodes and parses (parse_classes(ids) ->
    set of class indices, the head's parse) to exactly its own class, has no EOS inside and fits the vocabulary, and no
    two classes share a candidate.  Raises PsgHipError naming the classes that fail."""
    cands = [candidate_ids(tok, name, eos) for name in classes]
    bad = []
    for r, c in enumerate(cands):
        why = None
        if any(t == eos for t in c[:-1]):
            why = "its tokens contain EOS"
        elif any(t < 0 or t >= vocab for t in c):
            why = f"a token id outside the LLM vocabulary ({vocab})"
        else:
            got = parse_classes(c)
            if got != {r}:
                why = f"decodes and parses to {sorted(classes[i] for i in got)}"
        if why:
            bad.append(f"{classes[r]!r} ({why})")
    if bad:
        raise PsgHipError("llm_rel_scores='likelihood': relation classes whose candidate token sequence does not round-trip "
                          "through decode + parse: " + ", ".join(bad))
    trie = RelationTrie(classes, cands, eos)
    dup = trie.duplicates()
    if dup:
        raise PsgHipError("llm_rel_scores='likelihood': relation classes with the same candidate token sequence: "
                          + "; ".join(" / ".join(repr(classes[r]) for r in g) for g in dup))
    return trie


def assemble(generated, log_scores, selected_host, object_num, num_ranked):
    """rel_pred / rel_score of the LLM stage from the log scores.
    generated: [(k, triple)] in parse order (k = selection rank of the pair); log_scores [K, R] (float); selected_host [K]
    pair ids.  The generated triples come first, each scored s(k, r); then the `num_ranked` best remaining (k, r) by
    descending s, ties to the lower k, then the lower r."""
    ls = np.asarray(log_scores, dtype=np.float64)
    rel_pred, rel_score, taken = [], [], set()
    for k, t in generated:
        rel_pred.append(list(t))
        rel_score.append(float(np.exp(ls[k, t[2]])))
        taken.add((k, t[2]))
    if num_ranked > 0 and ls.size:
        K, R = ls.shape
        kk, rr = np.meshgrid(np.arange(K), np.arange(R), indexing="ij")
        kk, rr, vv = kk.reshape(-1), rr.reshape(-1), ls.reshape(-1)
        order = np.lexsort((rr, kk, -vv))                  # last key first: descending score, then k, then r
        n = 0
        for f in order:
            if n >= num_ranked:
                break
            k, r = int(kk[f]), int(rr[f])
            if (k, r) in taken:
                continue
            si = int(selected_host[k])
            rel_pred.append([si // object_num, si % object_num, r])
            rel_score.append(float(np.exp(vv[f])))
            n += 1
    return rel_pred, rel_score
