"""psg_trie_greedy_step on the GPU (`-m gpu`): the constrained greedy step against the numpy walk of
tests/trie_walk_ref.py over a hand-made trie - every piece of per-pair state exactly, the score against a float64
log-softmax and bit-equal to psg_token_logprobs - with the planted ties, -inf / NaN rows, finished rows and the refusals."""
import numpy as np
import pytest
import torch

from openpsg_amd._lib import PsgHipError
from tests import trie_walk_ref as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HID = 64
MAX_NEW = 6


def _plant(x, K, trie, vocab):
    """Step-0 logits [K, vocab] (fp32 values) with the planted rows; returns (node, done) before the step."""
    kids0 = {int(trie.child_tok[c]): int(trie.edge_node[c]) + 1 for c in range(trie.child_off[0], trie.child_off[1])}
    n20 = kids0[20]
    node, done = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32)
    x[0, [10, 20, vocab - 1]] = torch.tensor([1.5, 1.5, 0.5])         # equal logits: the lower token id wins
    x[0, 7] = 60.0                                                    # a non-child holds the row's global maximum
    if K > 1:
        node[1] = n20
        x[1, W.EOS] = -float("inf")                                   # a child at -inf
    if K > 2:
        done[2] = 1                                                   # a row already done
    if K > 3:
        x[3, :] = float("nan")                                        # an all-NaN row
    if K > 4:
        node[4] = kids0[vocab - 1]                                    # the node with a single child
    for k in range(5, K):
        node[k] = [0, kids0[10], n20, kids0[vocab - 1]][k % 4]
    return node, done


def _logits(gen, K, vocab, splits, dtype, plant=None):
    """(device logits, the values the kernel compares [K, vocab] - summed in slice order, rounded to dtype -, the values it
    scores).  plant(full) writes the planted rows into the fp32 target; with split-K partials those rows (the first five)
    live in slice 0 alone, next to zeros, so that their sums are the planted values exactly."""
    from openpsg_amd import ops
    full = torch.randn(K, vocab, generator=gen) * 4
    if plant is not None:
        plant(full)
    if not splits:
        x = full.to(dtype)
        return x.to(DEV), x.float(), x.float()
    parts = torch.randn(splits, K, vocab, generator=gen) * 2
    if plant is not None:
        parts[0, :5] = full[:5]
        parts[1:, :5] = 0.0
    summed = parts[0].clone()
    for s in range(1, splits):
        summed = summed + parts[s]                                    # the kernel's slice-order fp32 sum
    return ops.Partials(parts.to(DEV).contiguous()), summed.to(dtype).float(), summed


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("splits", [0, 1, 4])
@pytest.mark.parametrize("vocab", [512, 32000, 32001])
@pytest.mark.parametrize("K", [1, 5, 20, 33])
def test_walk_against_numpy(K, vocab, splits, dtype):
    from openpsg_amd import ops
    gen = torch.Generator().manual_seed(K * 7 + vocab + splits)
    trie = W.hand_trie(vocab)
    T = trie.device(DEV)
    E = trie.n_edges
    x_dtype = torch.float32 if dtype == torch.float16 else dtype      # fp16 table next to an fp32 residual stream
    embed = torch.randn(vocab, HID, generator=gen).to(dtype).to(DEV)
    planted = {}

    def plant(full):
        planted["node"], planted["done"] = _plant(full, K, trie, vocab)
    steps = trie.max_depth + 1
    st = None
    for step in range(steps):
        lg, cmp_v, score_v = _logits(gen, K, vocab, splits, dtype, plant if step == 0 else None)
        if step == 0:
            node_h, done_h = planted["node"].copy(), planted["done"].copy()
            st = dict(node=torch.from_numpy(node_h).to(DEV), done=torch.from_numpy(done_h).to(DEV),
                      tokens=torch.full((K, MAX_NEW), -1, dtype=torch.int32, device=DEV),
                      next_ids=torch.full((K,), -5, dtype=torch.int32, device=DEV),
                      tok_pos=torch.arange(K, dtype=torch.int32, device=DEV) + 40,
                      logp=torch.zeros(K, device=DEV), x=torch.full((K, HID), 9.0, dtype=x_dtype, device=DEV))
            # the same state for the run without a score and for the repeat
            st2 = {k: v.clone() for k, v in st.items()}
            st3 = {k: v.clone() for k, v in st.items()}
        before = {k: v.clone() for k, v in st.items()}
        # psg_token_logprobs on the same rows and nodes: the increment must be these very bits
        tl = torch.full((K, E), 0.0, device=DEV)
        safe_node = st["node"].clamp(0, trie.n_int)
        ops.token_logprobs(lg, safe_node.contiguous(), (torch.arange(K, dtype=torch.int64, device=DEV) * E),
                           T["child_off"], T["child_tok"], tl)

        def run(s):
            ops.trie_greedy_step(lg, step, MAX_NEW, W.EOS, T, s["node"], s["tokens"], s["done"], s["next_ids"],
                                 s["tok_pos"], logp=s.get("logp"), dtype=dtype, embed=embed, x_out=s["x"])
        run(st)
        st2["logp"] = None
        run(st2)
        run(st3)
        torch.cuda.synchronize()
        ref = W.walk_step(cmp_v.numpy(), trie, node_h, done_h)
        assert st["tokens"][:, step].cpu().tolist() == ref["tok"].tolist(), (step, st["tokens"][:, step].cpu(), ref["tok"])
        assert (st["tokens"][:, step + 1:] == -1).all()
        assert st["done"].cpu().tolist() == ref["done"].tolist()
        assert st["node"].cpu().tolist() == ref["node"].tolist()
        assert st["next_ids"].cpu().tolist() == ref["emit"].tolist()
        assert torch.equal(st["tok_pos"], before["tok_pos"] + 1)
        assert torch.equal(st["x"], embed[torch.from_numpy(ref["emit"]).to(DEV)].to(x_dtype))
        # score: float64 log-softmax of the values the kernel scores, then bit equality with psg_token_logprobs
        inc = (st["logp"] - before["logp"]).double().cpu().numpy()
        ls64 = W.log_softmax64(score_v.double().numpy())
        tl_h = tl.cpu()
        want_logp = before["logp"].cpu().clone()                      # a row that decodes nothing keeps its score
        for k in range(K):
            if ref["tok"][k] < 0:
                continue
            c0 = int(trie.child_off[int(node_h[k])])
            want_logp[k] = want_logp[k] + tl_h[k, int(ref["edge"][k]) - c0]
            want = ls64[k, ref["tok"][k]]
            if np.isfinite(want) and step == 0:                       # later steps: the sum's own rounding is not the kernel's
                assert abs(inc[k] - want) <= 1e-6 * max(1.0, abs(want)), (k, inc[k], want)
        torch.testing.assert_close(st["logp"].cpu(), want_logp, rtol=0, atol=0, equal_nan=True)
        # without a score every other output is the same; a second call gives the same bits
        for name in ("tokens", "done", "node", "next_ids", "tok_pos", "x"):
            assert torch.equal(st2[name], st[name]), name
            assert torch.equal(st3[name], st[name]), name
        torch.testing.assert_close(st3["logp"], st["logp"], rtol=0, atol=0, equal_nan=True)
        node_h, done_h = ref["node"].astype(np.int32), ref["done"].astype(np.int32)
    # the walk is over: every row that was live sits behind an EOS leaf
    live = planted["done"] == 0
    assert st["done"].cpu().numpy()[live].all()
    for k in range(K):
        seq = [int(t) for t in st["tokens"][k].cpu() if t >= 0]
        if live[k] and planted["node"][k] == 0:
            assert seq in trie.candidates


def test_score_against_float64_log_softmax_at_every_node():
    """The increment of every step against float64, from a zeroed accumulator per step (an accumulated sum rounds on its
    own): the bar test_token_logprobs_against_log_softmax holds psg_token_logprobs to."""
    from openpsg_amd import ops
    vocab, K = 32000, 8
    gen = torch.Generator().manual_seed(11)
    trie = W.hand_trie(vocab)
    T = trie.device(DEV)
    node = torch.tensor([0, 1, 2, 3, 4, 5, 0, 2], dtype=torch.int32)
    for splits, dtype in ((0, torch.float32), (3, torch.float32), (0, torch.bfloat16)):
        if splits:
            parts = torch.randn(splits, K, vocab, generator=gen) * 4
            lg = ops.Partials(parts.to(DEV).contiguous())
            full = parts[0].clone()
            for s in range(1, splits):
                full = full + parts[s]
        else:
            full = (torch.randn(K, vocab, generator=gen) * 4).to(dtype)
            lg = full.to(DEV)
            full = full.float()
        st = dict(node=node.clone().to(DEV), done=torch.zeros(K, dtype=torch.int32, device=DEV),
                  tokens=torch.full((K, 2), -1, dtype=torch.int32, device=DEV),
                  next_ids=torch.zeros(K, dtype=torch.int32, device=DEV), tok_pos=torch.zeros(K, dtype=torch.int32, device=DEV),
                  logp=torch.zeros(K, device=DEV))
        ops.trie_greedy_step(lg, 0, 2, W.EOS, T, st["node"], st["tokens"], st["done"], st["next_ids"], st["tok_pos"],
                             logp=st["logp"], dtype=dtype)
        ref = W.walk_step(full.to(dtype).float().numpy(), trie, node.numpy(), np.zeros(K, dtype=np.int32))
        assert st["tokens"][:, 0].cpu().tolist() == ref["tok"].tolist()
        ls64 = W.log_softmax64(full.double().numpy())
        got = st["logp"].double().cpu().numpy()
        for k in range(K):
            want = ls64[k, ref["tok"][k]]
            assert abs(got[k] - want) <= 1e-6 * max(1.0, abs(want)), (splits, dtype, k, got[k], want)


def _raw_args(T, K, vocab, **over):
    from openpsg_amd import _lib
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    keep = dict(logits=torch.zeros(K, vocab, device=DEV), node=i32(K), tokens=i32(K * 4, -1), done=i32(K), next_ids=i32(K),
                tok_pos=i32(K))
    a = dict(logits=keep["logits"].data_ptr(), splits=0, K=K, vocab=vocab, step=0, max_new=4, eos=W.EOS,
             child_off=T["child_off"].data_ptr(), child_tok=T["child_tok"].data_ptr(), edge_node=T["edge_node"].data_ptr(),
             n_nodes=T["child_off"].numel() - 1, n_edges=T["child_tok"].numel(), node=keep["node"].data_ptr(), logp=None,
             tokens=keep["tokens"].data_ptr(), done=keep["done"].data_ptr(), next_ids=keep["next_ids"].data_ptr(),
             tok_pos=keep["tok_pos"].data_ptr(), embed=None, embed_dtype=0, hidden=0, x_out=None, x_dtype=0, dtype=0,
             stream=torch.cuda.current_stream(DEV).cuda_stream)
    a.update(over)
    lib = _lib.load()
    rc = lib.psg_trie_greedy_step(_lib.ctx(0), *a.values())
    torch.cuda.synchronize()
    return rc, _lib.last_error(), keep


def test_refusals_before_any_launch():
    from openpsg_amd import _lib, ops
    vocab, K = 512, 3
    trie = W.hand_trie(vocab)
    T = trie.device(DEV)
    rc, _, keep = _raw_args(T, K, vocab)
    assert rc == 0 and (keep["tokens"].view(K, 4)[:, 0] >= 0).all()                   # the arguments are good as they stand
    for name in ("child_off", "child_tok", "edge_node"):
        rc, msg, keep = _raw_args(T, K, vocab, **{name: None})
        assert rc < 0
        assert "psg_trie_greedy_step" in msg and "NULL" in msg
        assert (keep["tokens"] == -1).all() and (keep["tok_pos"] == 0).all()          # nothing was launched
    rc, msg, keep = _raw_args(T, K, vocab, n_nodes=0)
    assert rc < 0 and "n_nodes=0" in msg and (keep["tok_pos"] == 0).all()
    rc, msg, keep = _raw_args(T, K, vocab, node=None)
    assert rc < 0 and "NULL" in msg
    rc, msg, keep = _raw_args(T, K, vocab, step=4)
    assert rc < 0 and "step=4" in msg
    # hidden % 4, through the binding
    embed = torch.zeros(vocab, 6, device=DEV)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    tok_pos = i32(K)
    with pytest.raises(PsgHipError, match="hidden %% 4|hidden % 4"):
        ops.trie_greedy_step(torch.zeros(K, vocab, device=DEV), 0, 4, W.EOS, T, i32(K), i32(K * 4, -1).view(K, 4), i32(K),
                             i32(K), tok_pos, embed=embed, x_out=torch.zeros(K, 6, device=DEV))
    torch.cuda.synchronize()
    assert (tok_pos == 0).all()
    # an unknown dtype code
    rc, msg, _ = _raw_args(T, K, vocab, dtype=7)
    assert rc < 0 and "dtype" in msg


def test_a_state_outside_the_tables_is_treated_as_done():
    """node[k] outside [0, n_nodes) cannot be refused on the host without a read-back: the kernel writes -1, reads no
    table for that row and leaves its state alone."""
    from openpsg_amd import ops
    vocab, K = 512, 4
    trie = W.hand_trie(vocab)
    T = trie.device(DEV)
    n_nodes = trie.n_int + 1
    node = torch.tensor([n_nodes, -1, 2 ** 30, 0], dtype=torch.int32, device=DEV)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    tokens, done, nxt, pos, logp = i32(K * 4, -7).view(K, 4), i32(K), i32(K), i32(K), torch.zeros(K, device=DEV)
    embed = torch.randn(vocab, 8, device=DEV)
    x = torch.zeros(K, 8, device=DEV)
    lg = torch.randn(K, vocab, device=DEV)
    ops.trie_greedy_step(lg, 0, 4, W.EOS, T, node, tokens, done, nxt, pos, logp=logp, embed=embed, x_out=x)
    torch.cuda.synchronize()
    assert tokens[:3, 0].tolist() == [-1, -1, -1] and tokens[3, 0].item() in (10, 20, vocab - 1)
    assert node[:3].tolist() == [n_nodes, -1, 2 ** 30] and done[:3].tolist() == [0, 0, 0]
    assert logp[:3].tolist() == [0.0, 0.0, 0.0] and logp[3].item() < 0
    assert nxt[:3].tolist() == [W.EOS] * 3 and pos.tolist() == [1] * 4
    assert torch.equal(x[:3], embed[W.EOS].expand(3, -1))
