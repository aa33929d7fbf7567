"""tests/llm_attn_ref.py checks itself on the CPU: the float64 references against gqa_ref.attend64 and a naive per-row
loop, the exact-rotation inputs, and two CPU models of the kernels' arithmetic against the derived bound on every input
family the GPU tests use - the clean models stay inside, three mutated ones (a truncating probability pack, a dropped
visible key, `alpha` left off the running output) do not."""
import math

import pytest
import torch

from tests import gqa_ref as R
from tests import llm_attn_ref as L

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
NAMES = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


# ---- the references ----
def _naive_row(q, k, v):
    """q [128], k / v [n, 128] float64 -> softmax(q . k / sqrt(128)) v by explicit loops over the keys"""
    s = [float((q * k[j]).sum()) / math.sqrt(128.0) for j in range(k.shape[0])]
    mx = max(s)
    e = [math.exp(x - mx) for x in s]
    out = torch.zeros(128, dtype=torch.float64)
    for j, w in enumerate(e):
        out += w / sum(e) * v[j]
    return out


def test_causal_reference_agrees_with_attend64_and_naive_loop():
    g = torch.Generator().manual_seed(1)
    pairs, S, heads, kvh, ctx = 3, 7, 4, 2, 9
    lens = [7, 4, 0]
    q = torch.randn(pairs * S, heads * 128, generator=g, dtype=torch.float64)
    kc = torch.randn(pairs, kvh, ctx, 128, generator=g, dtype=torch.float64)
    vc = torch.randn(pairs, kvh, ctx, 128, generator=g, dtype=torch.float64)
    for p in range(pairs):
        kc[p, :, lens[p]:] = float("nan")
        vc[p, :, lens[p]:] = float("nan")
    tok_pos = torch.tensor([t if t < lens[p] else -1 for p in range(pairs) for t in range(S)])
    tok_pair = torch.arange(pairs).repeat_interleave(S)
    ref, A, gx, n = L.causal64(q, kc, vc, tok_pos, pairs, S, heads)
    want = R.attend64(q.view(-1, heads, 128), kc, vc, tok_pair, tok_pos + 1)
    assert torch.allclose(ref, want, rtol=0, atol=1e-13)
    assert n.tolist() == (tok_pos + 1).tolist()
    assert bool((ref[tok_pos < 0] == 0).all()) and bool((A[tok_pos < 0] == 0).all())
    r, h = 1 * S + 3, 3                                            # row 3 of pair 1, head 3 -> kv head 1
    nv = _naive_row(q[r, h * 128:(h + 1) * 128], kc[1, 1, :4], vc[1, 1, :4])
    assert torch.allclose(ref[r, h * 128:(h + 1) * 128], nv, rtol=0, atol=1e-13)
    assert bool((A >= ref.abs() - 1e-15).all())
    # prefix64 is the same operation row by row
    ref2, A2, gx2, n2 = L.prefix64(q, kc, vc, tok_pair, tok_pos, heads)
    assert torch.allclose(ref2, ref, rtol=0, atol=1e-13) and torch.allclose(A2, A, rtol=0, atol=1e-13)
    assert torch.allclose(gx2, gx, rtol=0, atol=1e-13) and torch.equal(n2, n)
    kk = kc[1, 1, :4]
    assert math.isclose(float(gx[r, h]), float((q[r, h * 128:(h + 1) * 128].abs() * kk.abs()).sum(-1).max()) / math.sqrt(128))


def test_decode_and_tree_references_agree_with_naive_loop():
    g = torch.Generator().manual_seed(2)
    heads, kvh, ctx = 4, 2, 12
    kc = torch.randn(2, kvh, ctx, 128, generator=g, dtype=torch.float64)
    vc = torch.randn(2, kvh, ctx, 128, generator=g, dtype=torch.float64)
    qr = torch.randn(3, heads, 128, generator=g, dtype=torch.float64)
    kr = torch.randn(3, kvh, 128, generator=g, dtype=torch.float64)
    vn = torch.randn(3, kvh, 128, generator=g, dtype=torch.float64)
    pair, pos = torch.tensor([1, 0, 0]), torch.tensor([5, 0, -1])
    kc[1, :, 5:] = float("nan")                                    # unwritten slots are no part of the operation
    ref, A, gx, n = L.decode64(qr, kr, vn, kc, vc, pair, pos, heads)
    assert n.tolist() == [6, 1, 0] and bool((ref[2] == 0).all())
    want = _naive_row(qr[0, 2], torch.cat([kc[1, 1, :5], kr[0, 1:2]]), torch.cat([vc[1, 1, :5], vn[0, 1:2]]))
    assert torch.allclose(ref[0, 256:384], want, rtol=0, atol=1e-13)
    assert torch.allclose(ref[1, 384:], vn[1, 1], rtol=0, atol=1e-13)            # one key: its value
    # trie: prompt slots [0, 3) and [0, 0) plus ancestors at trie_base 6
    kc, vc = torch.nan_to_num(kc, nan=0.5), vc
    anc = torch.tensor([[0, -1, -1], [0, 1, -1], [0, 1, 2]])
    plen = torch.tensor([3, 0])
    rp, rn = torch.tensor([0, 1, 0]), torch.tensor([2, 0, 1])
    q = qr.reshape(3, -1)
    ref, A, gx, n = L.tree64(q, kc, vc, rp, rn, plen, anc, 6, heads)
    assert n.tolist() == [6, 1, 5]
    sl = [0, 1, 2, 6, 7, 8]
    assert torch.allclose(ref[0, :128], _naive_row(qr[0, 0], kc[0, 0, sl], vc[0, 0, sl]), rtol=0, atol=1e-13)
    assert torch.allclose(ref[1, 128:256], vc[1, 0, 6], rtol=0, atol=1e-13)


# ---- the exact-rotation inputs ----
@pytest.mark.parametrize("dtype", DTYPES, ids=NAMES.get)
def test_exact_rotation_inputs_leave_no_rounding_choice(dtype):
    g = torch.Generator().manual_seed(3)
    cos, sin = L.exact_rope_tables(200, g)
    seen = {(float(c), float(s)) for c, s in zip(cos.flatten(), sin.flatten())}
    assert seen == set(L.EXACT_ROT)
    x = L.grid((200, 3, 128), g)
    pos = torch.arange(200)
    assert torch.equal(x.to(dtype).double(), x)                    # the grid itself is representable
    want = L.rope64(x, pos, cos, sin)                              # float64: exact
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    x32 = x.float()
    x1, x2 = x32[..., :64], x32[..., 64:]
    plain = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)      # fp32, two roundings per term
    fused = torch.cat([torch.addcmul(x1 * c, x2, -s), torch.addcmul(x2 * c, x1, s)], -1)
    assert torch.equal(plain.double(), want) and torch.equal(fused.double(), want)
    assert torch.equal(want.to(dtype).double(), want)              # and the storage type holds it
    # unrotate inverts it on the grid
    r = L.grid((200, 3, 128), g, lim=2.0)
    back = L.unrotate(r, pos, cos, sin)
    assert torch.equal(L.rope64(back, pos, cos, sin), r)
    assert float(back.abs().max()) <= 4.0 and torch.equal(torch.round(back * 16), back * 16)
    # split-K partials: exact in any order
    parts = L.split_exact(x, 3, g)
    assert torch.equal((parts[0] + parts[1] + parts[2]).double(), x) and torch.equal((parts[2] + parts[0] + parts[1]).double(), x)


def test_directed_vectors_hit_their_scores():
    g = torch.Generator().manual_seed(4)
    for fam in L.FAMILIES[1:]:
        for n in (1, 2, 64, 200):
            t = L.family_scores(fam, n, torch.float16, g)
            q, k = L.directed_qk(t, 5, g, same_q=True)
            assert float((q @ k.T / math.sqrt(128) - t[None, :]).abs().max()) <= 2e-4
            assert torch.equal(torch.round(k * 16), k * 16) and torch.equal(torch.round(q * 16), q * 16)
    # last_key_matters: the last key of a causal row holds about half the mass
    t = L.family_scores("last_key_matters", 64, torch.bfloat16, g)
    for i in (1, 31, 32, 63):
        assert 0.49 <= float(torch.softmax(t[:i + 1], 0)[-1]) <= 0.67
    # descending_maximum: every later probability in fp16's subnormal range
    t = L.family_scores("descending_maximum", 64, torch.float16, g)
    pr = torch.exp(t[1:] - t[0])
    assert float(pr.max()) <= 2.0 ** -14 and float(pr.min()) >= 2.0 ** -24


# ---- CPU models of the two arithmetics ----
def _trunc(e, dtype):
    """fp32 -> dtype toward zero (e >= 0)"""
    if dtype == torch.bfloat16:
        return (e.view(torch.int32) & ~0xFFFF).view(torch.float32)
    h = e.to(torch.float16)
    down = (h.view(torch.int16) - 1).view(torch.float16)
    return torch.where(h.float() > e, down, h).float()


def model_matrix_core(q, k, v, vis, dtype, trunc=False):
    """(a) the matrix-core order: fp32 scores, unnormalised probabilities rounded to dtype, fp32 sums (the normaliser
    from the unrounded ones), one output rounding"""
    s = (q.float() @ k.float().T) * torch.tensor(L.RSQRT, dtype=torch.float32)
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros(()), m)
    e = torch.exp(s - m)
    lsum = e.sum(-1, keepdim=True)
    p = _trunc(e, dtype) if trunc else e.to(dtype).float()
    o = (p @ v.float()) * torch.where(lsum > 0, 1.0 / lsum, torch.zeros(()))
    return o.to(dtype)


def model_online(q, k, v, vis, dtype, no_alpha=False):
    """(b) the scalar order: online softmax over 64-key passes, fp32 probabilities, one output rounding"""
    nq, n = vis.shape
    m_run = torch.full((nq, 1), float("-inf"))
    l_run = torch.zeros(nq, 1)
    o = torch.zeros(nq, 128)
    sc = torch.tensor(L.RSQRT, dtype=torch.float32)
    for b0 in range(0, n, 64):
        s = (q.float() @ k[b0:b0 + 64].float().T) * sc
        s = s.masked_fill(~vis[:, b0:b0 + 64], float("-inf"))
        m_new = torch.maximum(m_run, s.amax(-1, keepdim=True))
        safe = torch.where(torch.isinf(m_new), torch.zeros(()), m_new)
        alpha = torch.exp(m_run - safe)
        pj = torch.exp(s - safe)
        l_run = l_run * alpha + pj.sum(-1, keepdim=True)
        if not no_alpha:
            o = o * alpha
        o = o + pj @ v[b0:b0 + 64].float()
        m_run = m_new
    return (o * torch.where(l_run > 0, 1.0 / l_run, torch.zeros(()))).to(dtype)


def _problem(family, n, nq, causal, dtype, seed, kstep=1.0 / 16):
    """q [nq, 128], k / v [n, 128] stored in dtype, vis [nq, n]: causal -> nq == n and row i sees keys <= i"""
    g = torch.Generator().manual_seed(seed)
    if family == "random":
        q, k = L.grid((nq, 128), g), L.grid((n, 128), g, lim=1.0)
    else:
        q, k = L.directed_qk(L.family_scores(family, n, dtype, g), nq, g, same_q=family == "probability_rounding_edge",
                               kstep=kstep)
    v = L.family_v(family, (n, 128), g)
    vis = torch.ones(nq, n, dtype=torch.bool).tril() if causal else torch.ones(nq, n, dtype=torch.bool)
    return q.to(dtype), k.to(dtype), v.to(dtype), vis


def _ratio(out, q, k, v, vis, dtype, p_rounded):
    ref, A, gx, n, sv = L.attend_masked64(q.double()[:, None, :], k.double()[None], v.double()[None], vis)
    bound = L.attn_bound(ref[:, 0], A[:, 0], gx, n, dtype, p_rounded=p_rounded, sum_v=sv[:, 0])
    err = (out.double() - ref[:, 0]).abs()
    return float((err / bound).max())


BLOCKS = (1, 17, 32, 33, 64)                                       # causal prompt blocks (model a, and b)
ROWS = (1, 2, 8, 9, 33, 41, 65, 129, 200)                          # keys of a single decode / trie row (model b)


def test_models_stay_inside_the_bound_on_every_family():
    worst = {}
    for dtype in DTYPES:
        for fam in L.FAMILIES:
            for S in BLOCKS:
                q, k, v, vis = _problem(fam, S, S, True, dtype, S)
                if dtype != torch.float32:
                    r = _ratio(model_matrix_core(q, k, v, vis, dtype), q, k, v, vis, dtype, True)
                    worst[("a", NAMES[dtype], fam)] = max(worst.get(("a", NAMES[dtype], fam), 0.0), r)
                r = _ratio(model_online(q, k, v, vis, dtype), q, k, v, vis, dtype, False)
                worst[("b", NAMES[dtype], fam)] = max(worst.get(("b", NAMES[dtype], fam), 0.0), r)
            for n in ROWS:
                q, k, v, vis = _problem(fam, n, 3, False, dtype, 1000 + n)
                r = _ratio(model_online(q, k, v, vis, dtype), q, k, v, vis, dtype, False)
                worst[("b", NAMES[dtype], fam)] = max(worst.get(("b", NAMES[dtype], fam), 0.0), r)
    for key in sorted(worst):
        print("model (%s) %s %-26s worst err / bound %.3f" % (*key, worst[key]))
    assert max(worst.values()) < 1.0, {k_: v_ for k_, v_ in worst.items() if v_ >= 1.0}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=NAMES.get)
def test_truncating_probability_pack_fails(dtype):
    for S, kstep in ((17, 1 / 16), (33, 1 / 16), (64, 1 / 16)) + (((64, 1 / 256),) if dtype == torch.float16 else ()):
        q, k, v, vis = _problem("probability_rounding_edge", S, S, True, dtype, S, kstep)
        assert torch.equal(k.double().to(dtype), k)
        clean = _ratio(model_matrix_core(q, k, v, vis, dtype), q, k, v, vis, dtype, True)
        mut = _ratio(model_matrix_core(q, k, v, vis, dtype, trunc=True), q, k, v, vis, dtype, True)
        print(f"{NAMES[dtype]} S={S} k step {kstep}: rounding pack {clean:.3f}, truncating pack {mut:.3f}")
        assert clean < 1.0 < mut


@pytest.mark.parametrize("dtype", DTYPES, ids=NAMES.get)
def test_dropped_key_fails(dtype):
    """the last visible key of the last row (a tile / tail edge) dropped, in both models"""
    for S in (1 + 1, 33, 64):
        q, k, v, vis = _problem("last_key_matters", S, S, True, dtype, S)
        cut = vis.clone()
        cut[S - 1, S - 1] = False
        for name, model, pr in (("a", model_matrix_core, True), ("b", model_online, False)):
            if name == "a" and dtype == torch.float32:
                continue
            mut = _ratio(model(q, k, v, cut, dtype), q, k, v, vis, dtype, pr)
            print(f"{NAMES[dtype]} S={S} model ({name}): key {S - 1} dropped for row {S - 1}: {mut:.1f}")
            assert mut > 1.0
    for n in (8, 41, 200):                                         # a single row: the last cached key
        q, k, v, vis = _problem("last_key_matters", n, 1, False, dtype, n)
        cut = vis.clone()
        cut[0, n - 1] = False
        mut = _ratio(model_online(q, k, v, cut, dtype), q, k, v, vis, dtype, False)
        print(f"{NAMES[dtype]} n={n} model (b): last key dropped: {mut:.1f}")
        assert mut > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=NAMES.get)
def test_alpha_left_off_the_running_output_fails(dtype):
    for n in (65, 129, 200):
        q, k, v, vis = _problem("ascending_maximum", n, 3, False, dtype, n)
        clean = _ratio(model_online(q, k, v, vis, dtype), q, k, v, vis, dtype, False)
        mut = _ratio(model_online(q, k, v, vis, dtype, no_alpha=True), q, k, v, vis, dtype, False)
        print(f"{NAMES[dtype]} n={n}: online softmax {clean:.3f}, without alpha on the output {mut:.1f}")
        assert clean < 1.0 < mut
