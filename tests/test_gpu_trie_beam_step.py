"""psg_trie_beam_step on the GPU (`-m gpu`): one level of the beam against the numpy level step of
tests/trie_beam_ref.py - selection and every piece of per-row state exactly, the scores against float64 and bit-equal to
psg_token_logprobs - over the hand-made trie of the greedy step's tests and a trie whose root has 40 children (8 beams:
320 candidates, more than a workgroup has threads), with the planted ties, -inf / NaN rows, dead beams, the merge of the
finished list, and the refusals.

The data are built so that the order is decided: a row's children sit on a grid of 1/32 (exact in bf16 / fp16), beam b's
offset score_b - lse_b on a grid of 1/4 plus b / 256 (minus an integer per pair, so that score_b <= 0), an old finished
entry on the same grid plus 1/512.  Two candidates are therefore at least 1/512 apart unless a tie is planted, and a planted tie is exact in fp32 and in float64 alike."""
import numpy as np
import pytest
import torch

from openpsg_amd._lib import PsgHipError
from tests import trie_beam_ref as BR
from tests import trie_walk_ref as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HID = 64
BASE = 40                                                     # first trie slot of the cache
MIN_GAP = 1.0 / 512


def _tries(vocab):
    return dict(hand=W.hand_trie(vocab), wide=BR.wide_trie(vocab))


def _state(gen, trie, K, B, beams_in, vocab, zero_scores=False):
    """Random rows and state of one level (CPU, fp32 values): rows [K * beams_in, vocab], node / offs [K, B], the old
    finished list, seq_len."""
    n_nodes = trie.n_int + 1
    ri = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=gen)  # noqa: E731
    rows = torch.randn(K * beams_in, vocab, generator=gen) * 2
    node = torch.full((K, B), -1, dtype=torch.int32)
    if beams_in == 1:
        node[:, 0] = 0
    else:
        node[:] = ri(0, n_nodes, K * B).view(K, B).to(torch.int32)
        node[ri(0, 4, K * B).view(K, B) == 0] = -1              # a quarter of the beams are dead
        node[0, 0] = 0                                          # (at least the root is there)
    for r in range(K * beams_in):
        nd = int(node[r // beams_in, r % beams_in])
        if nd < 0:
            continue
        toks = trie.child_tok[trie.child_off[nd]:trie.child_off[nd + 1]]
        grid = torch.randperm(255, generator=gen)[:len(toks)] - 127
        rows[r, torch.from_numpy(toks.astype(np.int64))] = grid.float() / 32
    offs = -(ri(0, 24, K * B).float() / 4) + (torch.arange(K * B) % B).float() / 256
    if zero_scores:
        offs = None
    fin_n = ri(0, B + 1, K)                                     # how many old finished entries a pair holds
    fin_class = torch.full((K, B), -1, dtype=torch.int32)
    fin_logp = torch.full((K, B), float("-inf"))
    for k in range(K):
        n = min(int(fin_n[k]), len(trie.candidates))
        vals = -(torch.randperm(64, generator=gen)[:n].sort().values.float() / 4) - 6.0 + 1.0 / 512
        fin_logp[k, :n] = vals                                  # best first
        fin_class[k, :n] = torch.randperm(len(trie.candidates), generator=gen)[:n].to(torch.int32)
    seq_len = (ri(20, 36, K)).to(torch.int32)
    return dict(rows=rows, node=node, offs=offs, fin_class=fin_class, fin_logp=fin_logp, seq_len=seq_len)


def _split(gen, rows, splits, same=()):
    """fp32 partial slices whose slice-order sum is `scored` (returned): slices 1.. hold multiples of 1/32, slice 0 the
    rest, so that an entry on the 1/32 grid (and a -inf / NaN entry) sums to itself exactly."""
    if splits <= 1:
        return rows[None].clone(), rows.clone()
    parts = torch.randint(-64, 65, (splits,) + tuple(rows.shape), generator=gen).float() / 32
    rest = parts[1].clone()
    for s in range(2, splits):
        rest = rest + parts[s]
    parts[0] = rows - rest
    for dst, src in same:                                       # two rows planted equal are equal in every slice
        parts[:, dst] = parts[:, src]
    summed = parts[0].clone()
    for s in range(1, splits):
        summed = summed + parts[s]                              # the kernel's slice-order fp32 sum
    return parts, summed


def _finish_case(gen, trie, st, K, B, beams_in, vocab, splits, dtype):
    """Logits as the kernel reads them, the scores on their grid, and the float64 reference of the level."""
    if splits:
        parts, scored = _split(gen, st["rows"], splits, st.get("same_rows", ()))
        logits = parts
    else:
        logits = st["rows"].to(dtype)
        scored = logits.float()
    ls = W.log_softmax64(scored.double().numpy())
    lse = scored.double().numpy()[:, 0] - ls[:, 0]              # (entry 0 is no child and finite unless the row is NaN)
    logp = torch.zeros(K, B)
    if st["offs"] is not None:
        for r in range(K * beams_in):
            k, b = divmod(r, beams_in)
            if np.isfinite(lse[r]):
                # an integer per pair keeps the scores what scores are - log-probabilities, <= 0 - and the grid intact: a
                # positive score_b near lse_b would cancel against t and leave |v| far below the fp32 terms it came from
                pair = lse[k * beams_in:(k + 1) * beams_in]
                shift = np.ceil(pair[np.isfinite(pair)].max()) + 1.0
                logp[k, b] = float(st["offs"][k * B + b]) + float(lse[r]) - shift
    logp = torch.where(st["node"] < 0, torch.full_like(logp, float("-inf")), logp) if beams_in == B else logp
    n_nodes = trie.n_int + 1
    want = dict(node=np.full((K, B), -1), logp=np.full((K, B), -np.inf), row_node=np.full((K, B), -1),
                tok_pos=np.full((K, B), -1), rope_pos=np.zeros((K, B), dtype=np.int64), emit=np.full((K, B), W.EOS),
                fin_class=np.full((K, B), -1), fin_logp=np.full((K, B), -np.inf), src=np.full((K, B, 2), -1))
    gaps = []
    for k in range(K):
        live = [(int(st["node"][k, b]), float(logp[k, b])) for b in range(beams_in)]
        fin = [(int(st["fin_class"][k, j]), float(st["fin_logp"][k, j])) for j in range(B)]

        def edge_t(b, c, k=k):
            tok = int(trie.child_tok[c])
            return ls[k * beams_in + b, tok] if 0 <= tok < vocab else None
        r = BR.level_step(trie, B, live, fin, edge_t)
        for i, (nd, v, b, c) in enumerate(r["live"]):
            ni = nd - 1
            want["node"][k, i], want["logp"][k, i], want["row_node"][k, i] = nd, v, ni
            want["tok_pos"][k, i] = BASE + ni
            want["rope_pos"][k, i] = int(st["seq_len"][k]) + int(trie.node_depth[ni]) - 1
            want["emit"][k, i] = int(trie.node_tok[ni])
            want["src"][k, i] = (b, c)
        for i, (cl, v) in enumerate(r["fin"]):
            want["fin_class"][k, i], want["fin_logp"][k, i] = cl, v
        gaps += [g for g in (r["live_gap"], r["fin_gap"]) if g > 0]   # (a planted tie is exactly 0 in both arithmetics)
        assert all(0 <= nd < n_nodes or nd == -1 for nd, _ in live)
    return dict(logits=logits, scored=scored, logp=logp, want=want, min_gap=min(gaps, default=np.inf), **st)


def _case(trie, K, B, beams_in, vocab, splits, dtype, seed, zero_scores=False, plant=None):
    gen = torch.Generator().manual_seed(seed)
    st = _state(gen, trie, K, B, beams_in, vocab, zero_scores)
    if plant is not None:
        plant(st)
    return _finish_case(gen, trie, st, K, B, beams_in, vocab, splits, dtype)


def _launch(trie, c, K, B, beams_in, vocab, splits, dtype, gen_seed=0):
    from openpsg_amd import ops
    T = trie.device(DEV)
    gen = torch.Generator().manual_seed(1000 + gen_seed)
    x_dtype = torch.float32 if dtype == torch.float16 else dtype      # fp16 table next to an fp32 residual stream
    embed = torch.randn(vocab, HID, generator=gen).to(dtype).to(DEV)
    lg = ops.Partials(c["logits"].to(DEV).contiguous()) if splits else c["logits"].to(DEV)
    outs = []
    for _ in range(2):                                          # the same call twice: the same bits
        s = dict(node=c["node"].reshape(-1).clone().to(DEV), logp=c["logp"].reshape(-1).clone().to(DEV),
                 fin_class=c["fin_class"].clone().to(DEV), fin_logp=c["fin_logp"].clone().to(DEV),
                 row_node=torch.full((K * B,), -9, dtype=torch.int32, device=DEV),
                 tok_pos=torch.full((K * B,), -9, dtype=torch.int32, device=DEV),
                 rope_pos=torch.full((K * B,), -9, dtype=torch.int32, device=DEV),
                 x=torch.full((K * B, HID), 9.0, dtype=x_dtype, device=DEV))
        ops.trie_beam_step(lg, B, beams_in, W.EOS, T, BASE, c["seq_len"].to(DEV), s["node"], s["logp"], s["fin_class"],
                           s["fin_logp"], s["row_node"], s["tok_pos"], s["rope_pos"], embed=embed, x_out=s["x"])
        outs.append(s)
    torch.cuda.synchronize()
    return outs, embed, lg, T, x_dtype


def _check(trie, c, outs, embed, x_dtype, K, B, what):
    s, s2 = outs
    w = c["want"]
    assert c["min_gap"] >= MIN_GAP * 0.99, (what, c["min_gap"])       # the data decide the order (module docstring)
    for name in ("node", "row_node", "tok_pos", "rope_pos", "fin_class"):
        assert s[name].cpu().view(K, B).tolist() == w[name].tolist(), (what, name)
    assert torch.equal(s["x"], embed[torch.from_numpy(w["emit"].reshape(-1)).to(DEV)].to(x_dtype)), what
    for name in ("logp", "fin_logp"):
        got, want = s[name].double().cpu().view(K, B).numpy(), w[name]
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, name)
        ok = np.isfinite(want)
        assert not np.isnan(got).any() and np.isfinite(got[ok]).all(), (what, name)
        err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
        assert err.max(initial=0.0) <= 1e-6, (what, name, err.max())
    for name in s:
        torch.testing.assert_close(s2[name], s[name], rtol=0, atol=0, equal_nan=True, msg=f"{what}: second call, {name}")


SWEEP = [(K, B, bi) for K in (1, 5, 20) for B in (1, 2, 3, 8) for bi in sorted({1, B})]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("splits", [0, 1, 4])
@pytest.mark.parametrize("vocab", [512, 32001])
@pytest.mark.parametrize("K,B,beams_in", SWEEP)
def test_level_against_numpy(K, B, beams_in, vocab, splits, dtype):
    for name, trie in _tries(vocab).items():
        seed = K * 131 + B * 17 + beams_in + vocab + splits * 3 + len(name)
        c = _case(trie, K, B, beams_in, vocab, splits, dtype, seed)
        outs, embed, _, _, x_dtype = _launch(trie, c, K, B, beams_in, vocab, splits, dtype, seed)
        _check(trie, c, outs, embed, x_dtype, K, B, f"{name} K={K} B={B} beams_in={beams_in}")


def test_eight_beams_on_the_40_child_root_rank_320_candidates():
    vocab, K, B = 512, 3, 8
    trie = BR.wide_trie(vocab)

    def plant(st):
        st["node"][:] = 0                                       # every beam of every pair at the root
        kids = torch.from_numpy(trie.child_tok[trie.child_off[0]:trie.child_off[1]].astype(np.int64))
        g = torch.Generator().manual_seed(5)
        for r in range(K * B):
            st["rows"][r, kids] = (torch.randperm(255, generator=g)[:len(kids)] - 127).float() / 32
    c = _case(trie, K, B, B, vocab, 0, torch.float32, 77, plant=plant)
    assert trie.child_off[1] - trie.child_off[0] == 40
    outs, embed, _, _, xd = _launch(trie, c, K, B, B, vocab, 0, torch.float32)
    _check(trie, c, outs, embed, xd, K, B, "320 candidates")
    assert (c["want"]["node"] > 0).all()                        # 8 live rows out of 320 candidates, from several beams
    assert len({int(b) for b in c["want"]["src"][0, :, 0]}) > 1


@pytest.mark.parametrize("splits", [0, 4])
def test_planted_cases(splits):
    """beams_in = B = 3 on the hand-made trie, one pair per planted case."""
    vocab, K, B = 512, 8, 3
    trie = W.hand_trie(vocab)
    kids0 = {int(trie.child_tok[c]): int(trie.edge_node[c]) + 1 for c in range(trie.child_off[0], trie.child_off[1])}
    n10, n20, nhi = kids0[10], kids0[20], kids0[vocab - 1]
    n2021 = [int(trie.edge_node[c]) + 1 for c in range(trie.child_off[n20], trie.child_off[n20 + 1])
             if trie.child_tok[c] == 21][0]
    hi = vocab - 1

    def plant(st):
        rows, node, offs = st["rows"], st["node"], st["offs"]
        node[:] = -1
        offs[:] = (torch.arange(K * B) % B).float() / 256 - 1.0
        st["fin_class"][:], st["fin_logp"][:] = -1, float("-inf")
        # pair 0: two equal children of one beam - the lower edge wins; a non-child holds the row maximum
        node[0, 0] = 0
        rows[0 * B + 0, [10, 20, hi]] = torch.tensor([1.5, 1.5, 0.5])
        rows[0 * B + 0, 7] = 60.0
        # pair 1: two beams with identical rows and scores - the lower beam wins
        node[1, 0] = node[1, 1] = n20
        rows[1 * B + 1] = rows[1 * B + 0]
        rows[1 * B + 1, [W.EOS, 21]] = rows[1 * B + 0, [W.EOS, 21]] = torch.tensor([0.25, 0.5])
        offs[1 * B + 1] = offs[1 * B + 0]
        st["same_rows"] = [(1 * B + 1, 1 * B + 0)]
        # pair 2: a child at -inf
        node[2, 0] = 0
        rows[2 * B + 0, [10, 20, hi]] = torch.tensor([float("-inf"), -2.0, -3.0])
        # pair 3: a dead beam between two live ones
        node[3, 0], node[3, 2] = n20, 0
        rows[3 * B + 0, [W.EOS, 21]] = torch.tensor([1.0, 2.0])
        rows[3 * B + 2, [10, 20, hi]] = torch.tensor([1.0, 2.0, 3.0])
        # pair 4: an all-NaN row next to a live one
        node[4, 0], node[4, 1] = 0, nhi
        rows[4 * B + 0, :] = float("nan")
        rows[4 * B + 1, 31] = 0.75
        # pair 5: fewer candidates than B - one live row, two dead; and nothing at all
        node[5, 0], node[5, 1] = nhi, n10
        rows[5 * B + 0, 31], rows[5 * B + 1, W.EOS] = 0.5, 0.25
        # pair 6: an old finished entry that survives the merge, and one that is displaced
        node[6, 0], node[6, 2] = n10, n2021
        rows[6 * B + 0, W.EOS], rows[6 * B + 2, W.EOS] = -1.0, 2.0
        st["fin_class"][6, :2] = torch.tensor([3, 1], dtype=torch.int32)
        st["fin_logp"][6, :2] = torch.tensor([-0.001953125, -30.0])
        # pair 7: every beam dead - the finished list stays, every row is dead
        st["fin_class"][7, 0], st["fin_logp"][7, 0] = 1, -2.5
    c = _case(trie, K, B, B, vocab, splits, torch.float32, 9, plant=plant)
    outs, embed, _, _, xd = _launch(trie, c, K, B, B, vocab, splits, torch.float32)
    _check(trie, c, outs, embed, xd, K, B, f"planted splits={splits}")
    w, s = c["want"], outs[0]
    node = s["node"].cpu().view(K, B)
    assert node[0].tolist() == [n10, n20, nhi] and w["logp"][0, 0] == w["logp"][0, 1]        # tie: the lower edge first
    assert w["src"][1, :2, 0].tolist() == [0, 1] and w["logp"][1, 0] == w["logp"][1, 1]      # tie: the lower beam first
    assert node[1].tolist() == [n2021, n2021, -1]
    assert s["fin_class"][1].tolist() == [1, 1, -1]
    assert node[2].tolist() == [n20, nhi, -1]                                               # the -inf child is no candidate
    assert node[3].tolist() == [nhi, n20, n2021] and s["fin_class"][3].tolist() == [1, -1, -1]   # n10 is the fourth: dropped
    assert node[4, 1:].tolist() == [-1, -1] and node[4, 0] > 0 and w["src"][4, 0, 0] == 1    # the NaN row yields nothing
    assert node[5].tolist() == [int(w["node"][5, 0]), -1, -1] and node[5, 0] > 0
    assert s["tok_pos"].view(K, B)[5].tolist()[1:] == [-1, -1] and s["row_node"].view(K, B)[5].tolist()[1:] == [-1, -1]
    assert torch.isneginf(s["logp"].view(K, B)[5, 1:]).all()
    assert torch.equal(s["x"].view(K, B, HID)[5, 1:], embed[W.EOS].expand(2, -1))           # a dead row embeds EOS
    assert s["fin_class"][6].tolist() == [3, 2, 0]              # old class 3 survives ahead of the new ones, old class 1 is displaced
    assert node[7].tolist() == [-1, -1, -1] and s["fin_class"][7].tolist() == [1, -1, -1]
    assert s["fin_logp"][7, 0].item() == -2.5


def test_planted_root_level():
    """beams_in = 1: the tie, the -inf child, the NaN row and a dead root, B = 2."""
    vocab, K, B = 512, 4, 2
    trie = W.hand_trie(vocab)
    hi = vocab - 1

    def plant(st):
        st["rows"][0, [10, 20, hi]] = torch.tensor([1.5, 1.5, 1.75])
        st["rows"][0, 7] = 60.0
        st["rows"][1, [10, 20, hi]] = torch.tensor([float("-inf"), float("-inf"), 0.5])
        st["rows"][2, :] = float("nan")
        st["node"][3, 0] = -1
        st["fin_class"][:], st["fin_logp"][:] = -1, float("-inf")
    c = _case(trie, K, B, 1, vocab, 0, torch.float32, 21, plant=plant)
    outs, embed, _, _, xd = _launch(trie, c, K, B, 1, vocab, 0, torch.float32)
    _check(trie, c, outs, embed, xd, K, B, "planted root")
    node = outs[0]["node"].cpu().view(K, B)
    kids0 = {int(trie.child_tok[c_]): int(trie.edge_node[c_]) + 1 for c_ in range(trie.child_off[0], trie.child_off[1])}
    assert node[0].tolist() == [kids0[hi], kids0[10]]           # 20 ties with 10 and loses: the lower edge
    assert node[1].tolist() == [kids0[hi], -1] and node[2].tolist() == [-1, -1] and node[3].tolist() == [-1, -1]


@pytest.mark.parametrize("splits,dtype", [(0, torch.float32), (3, torch.float32), (0, torch.bfloat16), (0, torch.float16)])
@pytest.mark.parametrize("vocab", [512, 32001])
def test_increment_is_token_logprobs_bit_for_bit(vocab, splits, dtype):
    """From zero scores the new score of a row IS the increment: the very bits psg_token_logprobs writes for the source
    row and child."""
    from openpsg_amd import ops
    K, B = 5, 3
    trie = BR.wide_trie(vocab)
    c = _case(trie, K, B, B, vocab, splits, dtype, 31 + splits, zero_scores=True)
    assert c["min_gap"] >= 1e-4, c["min_gap"]                   # no construction here: the seed's own gaps
    outs, embed, lg, T, xd = _launch(trie, c, K, B, B, vocab, splits, dtype)
    s = outs[0]
    w = c["want"]
    for name in ("node", "fin_class"):
        assert s[name].cpu().view(K, B).tolist() == w[name].tolist(), name
    E = trie.n_edges
    rows = K * B
    tl = torch.zeros(rows, E, device=DEV)
    row_node = c["node"].reshape(-1).clamp(0, trie.n_int).to(DEV)
    row_out = torch.arange(rows, dtype=torch.int64, device=DEV) * E
    ops.token_logprobs(lg, row_node.contiguous(), row_out, T["child_off"], T["child_tok"], tl)
    torch.cuda.synchronize()
    tl, got = tl.cpu(), s["logp"].cpu().view(K, B)
    n = 0
    for k in range(K):
        for i in range(B):
            b, e = (int(v) for v in w["src"][k, i])
            if b < 0:
                continue
            c0 = int(trie.child_off[int(c["node"][k, b])])
            assert torch.equal(got[k, i], tl[k * B + b, e - c0]), (k, i)
            n += 1
    assert n >= K                                               # the comparison saw live rows


def _raw(T, K, width, vocab, **over):
    """The C entry with good arguments for buffers of `width` beams, then `over` (which may name another B)."""
    from openpsg_amd import _lib
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    f32 = lambda n, v=0.0: torch.full((n,), v, dtype=torch.float32, device=DEV)  # noqa: E731
    keep = dict(logits=torch.zeros(K, vocab, device=DEV), seq_len=i32(K, 30), node=i32(K * width), logp=f32(K * width),
                fin_class=i32(K * width, -1), fin_logp=f32(K * width, float("-inf")), row_node=i32(K * width, -9),
                tok_pos=i32(K * width, -9), rope_pos=i32(K * width, -9))
    a = dict(logits=keep["logits"].data_ptr(), splits=0, K=K, B=width, beams_in=1, vocab=vocab, eos=W.EOS,
             child_off=T["child_off"].data_ptr(), child_tok=T["child_tok"].data_ptr(), edge_node=T["edge_node"].data_ptr(),
             edge_class=T["edge_class"].data_ptr(), node_tok=T["node_tok"].data_ptr(), node_depth=T["node_depth"].data_ptr(),
             n_nodes=T["child_off"].numel() - 1, n_edges=T["child_tok"].numel(), max_children=T["max_children"],
             trie_base=BASE, seq_len=keep["seq_len"].data_ptr(), node=keep["node"].data_ptr(), logp=keep["logp"].data_ptr(),
             fin_class=keep["fin_class"].data_ptr(), fin_logp=keep["fin_logp"].data_ptr(),
             row_node=keep["row_node"].data_ptr(), tok_pos=keep["tok_pos"].data_ptr(), rope_pos=keep["rope_pos"].data_ptr(),
             embed=None, embed_dtype=0, hidden=0, x_out=None, x_dtype=0, dtype=0,
             stream=torch.cuda.current_stream(DEV).cuda_stream)
    a.update(over)
    rc = _lib.load().psg_trie_beam_step(_lib.ctx(0), *a.values())
    torch.cuda.synchronize()
    return rc, _lib.last_error(), keep


def test_refusals_before_any_launch():
    from openpsg_amd import ops
    vocab, K, B = 512, 3, 2
    T = W.hand_trie(vocab).device(DEV)
    rc, _, keep = _raw(T, K, B, vocab)
    assert rc == 0 and (keep["tok_pos"] != -9).all()            # the arguments are good as they stand
    untouched = lambda keep: (keep["tok_pos"] == -9).all() and (keep["row_node"] == -9).all()  # noqa: E731
    for bad in (0, 9, -1):
        rc, msg, keep = _raw(T, K, 2, vocab, B=bad)
        assert rc < 0 and "psg_trie_beam_step" in msg and f"B={bad}" in msg and untouched(keep)
    for bad in (0, 3, 8):
        rc, msg, keep = _raw(T, K, B, vocab, beams_in=bad)
        assert rc < 0 and f"beams_in={bad}" in msg and untouched(keep)
    for name in ("child_off", "child_tok", "edge_node", "edge_class", "node_tok", "node_depth"):
        rc, msg, keep = _raw(T, K, B, vocab, **{name: None})
        assert rc < 0 and "NULL trie table" in msg and untouched(keep)
    rc, msg, keep = _raw(T, K, B, vocab, n_nodes=0)
    assert rc < 0 and "n_nodes=0" in msg and untouched(keep)
    rc, msg, keep = _raw(T, K, B, vocab, node=None)
    assert rc < 0 and "NULL" in msg and untouched(keep)
    rc, msg, keep = _raw(T, K, B, vocab, max_children=1025)
    assert rc < 0 and "candidates" in msg and untouched(keep)
    rc, msg, _ = _raw(T, K, B, vocab, dtype=7)
    assert rc < 0 and "dtype" in msg
    # through the binding: the width, beams_in, and hidden % 4
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    f32 = lambda n: torch.zeros(n, device=DEV)  # noqa: E731

    def call(B, beams_in, hid=8, rows=None):
        rows = K * beams_in if rows is None else rows
        tok_pos = i32(K * B, -9)
        ops.trie_beam_step(torch.zeros(rows, vocab, device=DEV), B, beams_in, W.EOS, T, BASE, i32(K, 30), i32(K * B),
                           f32(K * B), i32(K * B, -1).view(K, B), f32(K * B).view(K, B), i32(K * B), tok_pos, i32(K * B),
                           embed=torch.zeros(vocab, hid, device=DEV), x_out=torch.zeros(K * B, hid, device=DEV))
        return tok_pos
    with pytest.raises(PsgHipError, match="B=9"):
        call(9, 1)
    with pytest.raises(PsgHipError, match="beams_in=2"):
        call(3, 2, rows=K * 2)
    with pytest.raises(PsgHipError, match="hidden %% 4|hidden % 4"):
        call(2, 1, hid=6)
    torch.cuda.synchronize()
    assert (call(2, 1) != -9).all()


def test_a_state_outside_the_tables_is_a_dead_beam():
    """node outside [0, n_nodes) cannot be refused on the host without a read-back: the kernel reads no table for it."""
    from openpsg_amd import ops
    vocab, K, B = 512, 2, 3
    trie = W.hand_trie(vocab)
    T = trie.device(DEV)
    node = torch.tensor([trie.n_int + 1, 2 ** 30, -5, 0, -1, trie.n_int + 7], dtype=torch.int32, device=DEV)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    logp, fc, fl = torch.zeros(K * B, device=DEV), i32(K * B, -1).view(K, B), torch.full((K, B), float("-inf"), device=DEV)
    rn, tp, rp = i32(K * B, -9), i32(K * B, -9), i32(K * B, -9)
    ops.trie_beam_step(torch.randn(K * B, vocab, device=DEV), B, B, W.EOS, T, BASE, i32(K, 30), node, logp, fc, fl, rn, tp, rp)
    torch.cuda.synchronize()
    assert node[:3].tolist() == [-1, -1, -1] and tp[:3].tolist() == [-1, -1, -1]
    assert (node[3:] > 0).all() and sorted(tp[3:].tolist()) == sorted(BASE + int(n) - 1 for n in node[3:].tolist())
