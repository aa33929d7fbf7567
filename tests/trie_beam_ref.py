"""numpy / float64 restatement of the beam over a relation trie (psg_trie_beam_step and `generate(beam=)`).
No GPU, no torch: tests/test_beam_cpu.py checks it, the GPU tests use it as their reference.

State per pair: `live`, at most B (node, score) entries - node is a CSR node (0 = root, 1 + i = internal i) -, and
`fin`, at most B (class, score) entries, both best first.  A level scores every edge c of every live entry b with
v = score_b + t(b, c); edges to an internal node go to the live pool, EOS edges to the finish pool with their class.
New live list: the first B of the live pool by v descending, ties to the lower beam, then the lower edge.  New finished
list: the first B of (old finished list + finish pool) by v descending, ties to the lower class."""
import numpy as np

from openpsg_amd.rel_scores import RelationTrie


def wide_trie(vocab, n_root=40, eos=2):
    """A synthetic trie whose root has `n_root` children (tokens 100, 103, ...): 8 beams on the root give 320 candidates,
    more than a workgroup has threads.  Child i of the root has 1 + i % 3 non-EOS children of its own, every third an EOS
    child too; the nodes below end in EOS."""
    cands = []
    for i in range(n_root):
        a = 100 + 3 * i
        if i % 3 == 0:
            cands.append([a, eos])
        for j in range(1 + i % 3):
            cands.append([a, 300 + 5 * j + i % 2, eos])
    assert max(max(c) for c in cands) < vocab
    return RelationTrie([f"w{i}" for i in range(len(cands))], cands, eos)


def _gap(pool, B):
    """Smallest gap between adjacent kept entries and between the last kept and the first dropped one (inf: none)."""
    v = [e[0] for e in pool[:B + 1]]
    return min([v[i] - v[i + 1] for i in range(len(v) - 1)], default=np.inf)


def level_step(trie, B, live, fin, edge_t):
    """One level.  live [(node, score)] (node < 0: a dead entry, kept in its beam position), fin [(class, score)];
    edge_t(beam, edge) -> t (float) or None / NaN / -inf for an edge that is no candidate.
    Returns dict(live=[(node, score, beam, edge)], fin=[(class, score)], live_gap, fin_gap, n_live_pool)."""
    n_nodes = len(trie.child_off) - 1
    live_pool, fin_pool = [], []
    for b, (nd, sc) in enumerate(live):
        if nd < 0 or nd >= n_nodes:
            continue
        for c in range(int(trie.child_off[nd]), int(trie.child_off[nd + 1])):
            t = edge_t(b, c)
            if t is None or np.isnan(t) or t == -np.inf:
                continue
            v = np.float64(sc) + np.float64(t)
            if np.isnan(v):
                continue
            if trie.edge_node[c] >= 0:
                live_pool.append((v, b, c))
            elif trie.edge_class[c] >= 0:
                fin_pool.append((v, int(trie.edge_class[c])))
    live_pool.sort(key=lambda e: (-e[0], e[1], e[2]))
    fin_all = [(np.float64(s), int(r)) for r, s in fin if r >= 0 and not np.isnan(s)] + fin_pool
    fin_all.sort(key=lambda e: (-e[0], e[1]))
    return dict(live=[(int(trie.edge_node[c]) + 1, v, b, c) for v, b, c in live_pool[:B]],
                fin=[(r, v) for v, r in fin_all[:B]], live_gap=_gap(live_pool, B), fin_gap=_gap(fin_all, B),
                n_live_pool=len(live_pool))


def search(trie, B, table):
    """The whole beam of one pair over a per-edge log-probability table [n_edges] (t of an edge does not depend on the
    beam that holds its node: a node has one path).  Returns (classes [B] (-1 padded), scores [B] (-inf padded),
    gaps [max_depth + 1]: per level the smaller of the live pool's and the finished pool's gap, exact [bool]: no level's
    live pool held more than B entries)."""
    live, fin, gaps, exact = [(0, 0.0)], [], [], True
    for _ in range(trie.max_depth + 1):
        r = level_step(trie, B, live, fin, lambda b, c: table[c])
        live, fin = [(n, v) for n, v, _, _ in r["live"]], r["fin"]
        gaps.append(min(r["live_gap"], r["fin_gap"]))
        exact = exact and r["n_live_pool"] <= B
    assert not live, "below the deepest internal nodes there are only EOS leaves"
    cls = np.full(B, -1, dtype=np.int64)
    sc = np.full(B, -np.inf)
    for i, (r, v) in enumerate(fin):
        cls[i], sc[i] = r, v
    return cls, sc, np.asarray(gaps), exact


def path_scores(trie, table):
    """s(p, r) of every class from the per-edge table [n_edges]: the sum over the class's path."""
    ext = np.append(np.asarray(table, dtype=np.float64), 0.0)
    return ext[trie.path].sum(-1)
