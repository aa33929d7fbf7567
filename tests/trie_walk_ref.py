"""numpy restatement of the constrained greedy walk (psg_trie_greedy_step) and the hand-made trie its tests
share.  No GPU, no torch: tests/test_constrained_cpu.py checks it, the GPU tests use it as their reference."""
import numpy as np

from openpsg_amd.rel_scores import RelationTrie

EOS = 2


def hand_trie(vocab):
    """Four candidates over tokens {10, 20, 21, 31, 32, vocab - 1, EOS}:
      root            three children: 10, 20, vocab - 1
      (10)            its only child is EOS
      (20)            an EOS child and a non-EOS child (21)
      (20, 21)        only EOS
      (vocab-1)       a single, non-EOS child (31) -> (.., 31) -> single child 32 -> (.., 32) -> EOS
    max_depth = 3: a walk takes at most 4 steps."""
    hi = vocab - 1
    cands = [[10, EOS], [20, EOS], [20, 21, EOS], [hi, 31, 32, EOS]]
    return RelationTrie([f"c{i}" for i in range(len(cands))], cands, EOS)


def walk_step(values, trie, node, done, eos=EOS):
    """One constrained greedy step over `values` [K, vocab] (the candidate values as the kernel compares them: summed over
    the slices and rounded to the activation type).  node / done int [K] are the state BEFORE the step.
    Returns dict(tok [K] (-1 for a row that decodes nothing), emit [K] (the token whose embedding row is handed on),
    edge [K] (-1), node, done) - the state after the step."""
    values = np.asarray(values)
    K, vocab = values.shape
    n_nodes = len(trie.child_off) - 1
    tok = np.full(K, -1, dtype=np.int64)
    edge = np.full(K, -1, dtype=np.int64)
    emit = np.full(K, eos if 0 <= eos < vocab else 0, dtype=np.int64)
    node2, done2 = np.array(node, dtype=np.int64), np.array(done, dtype=np.int64)
    for k in range(K):
        n = int(node[k])
        if done[k] or n < 0 or n >= n_nodes:
            continue
        kids = [(int(trie.child_tok[c]), c) for c in range(int(trie.child_off[n]), int(trie.child_off[n + 1]))
                if 0 <= int(trie.child_tok[c]) < vocab]
        if not kids:
            continue
        best, bt, bc = -np.inf, None, None
        for t, c in kids:
            v = values[k, t]
            if v > best or (v == best and bt is not None and t < bt):    # NaN compares false: never taken
                best, bt, bc = v, t, c
        if bt is None:                                           # nothing above -inf: the child with the lowest token id
            bt, bc = min(kids)
        tok[k], edge[k], emit[k] = bt, bc, bt
        nx = int(trie.edge_node[bc])
        if nx < 0:
            done2[k] = 1
        else:
            node2[k] = nx + 1
    return dict(tok=tok, emit=emit, edge=edge, node=node2, done=done2)


def log_softmax64(values):
    """float64 log-softmax of the rows of `values` (the score's reference); -inf entries contribute nothing."""
    v = np.asarray(values, dtype=np.float64)
    m = np.max(np.where(np.isfinite(v), v, -np.inf), axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v - (m + np.log(np.sum(np.exp(v - m), axis=-1, keepdims=True)))


def walk(step_values, trie, K, eos=EOS):
    """The whole walk: step_values(step, emitted so far [K, step]) -> values [K, vocab].  Returns tokens [K, max_depth + 1]
    (-1 behind a pair's EOS), path log-probability [K] (float64), done [K]."""
    steps = trie.max_depth + 1
    node, done = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    tokens = np.full((K, steps), -1, dtype=np.int64)
    logp = np.zeros(K, dtype=np.float64)
    for s in range(steps):
        vals = np.asarray(step_values(s, tokens[:, :s]))
        r = walk_step(vals, trie, node, done, eos)
        ls = log_softmax64(vals)
        for k in range(K):
            if r["tok"][k] >= 0:
                logp[k] += ls[k, r["tok"][k]]
        tokens[:, s] = r["tok"]
        node, done = r["node"], r["done"]
    return tokens, logp, done
