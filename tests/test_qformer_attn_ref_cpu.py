"""The float64 references of the Q-Former attention kernels (tests/qformer_attn_ref.py) and their bound, checked on the
CPU: the references against direct triple-loop restatements on tiny sizes, the bit-table helper, and the bound against
fp32 emulations of the two rounding orders the kernels use (normalised probabilities rounded to the storage type; online
softmax over 32-key tiles with UNNORMALISED probabilities rounded) - and against a truncating rounding, which it must
reject."""
import math

import pytest
import torch

from tests.qformer_attn_ref import (U, attn_bound, cls_input64, cls_input_bound, pack_bits, pair_masks, selfattn64,
                                    unpack_bits, xattn64)


def _softmax(s):
    m = max(s)
    e = [math.exp(x - m) if x != float("-inf") else 0.0 for x in s]
    t = sum(e)
    return [x / t for x in e]


def test_pack_bits_round_trips_and_leaves_the_tail_zero():
    g = torch.Generator().manual_seed(1)
    for L in (1, 31, 32, 33, 63, 64, 65, 100, 128, 129, 320):
        om = torch.rand(5, L, generator=g) < 0.4
        om[0] = True                                               # every bit below L set: the tail must still be zero
        bits = pack_bits(om)
        assert bits.shape == (5, (L + 63) // 64) and bits.dtype == torch.int64
        back, tail = unpack_bits(bits, L)
        assert torch.equal(back, om) and not tail
        for i in range(5):                                         # bit l of word l // 64, independently of numpy
            for l in range(L):
                assert ((int(bits[i, l >> 6]) >> (l & 63)) & 1) == int(om[i, l])
    om = torch.rand(4, 70, generator=g) < 0.5
    pi = torch.tensor([0, 5, 7, 7, 14, 11])
    pm = pair_masks(om, pi, 4)
    for n, p in enumerate(pi.tolist()):
        assert torch.equal(pm[n], om[p // 4] | om[p % 4])


@pytest.mark.parametrize("policy", ["uniform", "unmasked"])
def test_xattn64_equals_a_triple_loop(policy):
    g = torch.Generator().manual_seed(2)
    heads, nq, L, P = 2, 3, 7, 4
    q = torch.randn(P * nq, heads * 64, generator=g, dtype=torch.float64)
    k = torch.randn(L, heads * 64, generator=g, dtype=torch.float64)
    v = torch.randn(L, heads * 64, generator=g, dtype=torch.float64)
    pm = torch.rand(P, L, generator=g) < 0.5
    pm[1] = False                                                  # an empty union
    pm[2] = True
    ref, A = xattn64(q, k, v, pm, heads, nq, policy, chunk=3)
    for p in range(P):
        for i in range(nq):
            for h in range(heads):
                sl = slice(h * 64, (h + 1) * 64)
                s = [float(q[p * nq + i, sl] @ k[l, sl]) / 8.0 for l in range(L)]
                if pm[p].any():
                    s = [x if pm[p, l] else (float("-inf") if policy == "uniform" else x - 10000.0) for l, x in enumerate(s)]
                elif policy == "uniform":
                    s = [0.0] * L
                pr = _softmax(s)
                o = sum(pr[l] * v[l, sl] for l in range(L))
                a = sum(pr[l] * v[l, sl].abs() for l in range(L))
                assert (ref[p * nq + i, sl] - o).abs().max() < 1e-13 and (A[p * nq + i, sl] - a).abs().max() < 1e-13
    if policy == "uniform":
        assert (ref[nq:2 * nq] - v.mean(0)).abs().max() < 1e-13    # the empty pair: the mean of V


@pytest.mark.parametrize("T", [0, 3])
def test_selfattn64_equals_a_triple_loop(T):
    g = torch.Generator().manual_seed(3 + T)
    heads, nq, B = 2, 3, 3
    H = heads * 64
    qkv = torch.randn(B * (nq + T), 3 * H, generator=g, dtype=torch.float64)
    tm = (torch.rand(B, T, generator=g) < 0.6).to(torch.uint8)
    if T:
        tm[0] = 0
    full, A = selfattn64(qkv, tm, B, T, nq, heads, "all")
    for p in range(B):
        rows = list(range(p * nq, (p + 1) * nq)) + list(range(B * nq + p * T, B * nq + (p + 1) * T))
        for r in rows:
            for h in range(heads):
                sl = slice(h * 64, (h + 1) * 64)
                s = []
                for n, j in enumerate(rows):
                    ok = n < nq or bool(tm[p, n - nq])
                    s.append(float(qkv[r, sl] @ qkv[j, H + h * 64:H + (h + 1) * 64]) / 8.0 if ok else float("-inf"))
                pr = _softmax(s)
                o = sum(pr[n] * qkv[j, 2 * H + h * 64:2 * H + (h + 1) * 64] for n, j in enumerate(rows))
                a = sum(pr[n] * qkv[j, 2 * H + h * 64:2 * H + (h + 1) * 64].abs() for n, j in enumerate(rows))
                assert (full[r, sl] - o).abs().max() < 1e-13 and (A[r, sl] - a).abs().max() < 1e-13
    qr, _ = selfattn64(qkv, tm, B, T, nq, heads, "query")
    assert (qr - full[:B * nq]).abs().max() < 1e-13              # (another matmul shape: last bits)
    cls, _ = selfattn64(qkv, tm, B, T, nq, heads, "cls")
    assert (cls - full[0:B * nq:nq]).abs().max() < 1e-13
    cls2, _ = selfattn64((qkv[0:B * nq:nq, :H].clone(), qkv[:, H:].clone()), tm, B, T, nq, heads, "cls")
    assert (cls2 - cls).abs().max() < 1e-13


@pytest.mark.parametrize("shared", [False, True])
def test_cls_input64_equals_a_triple_loop(shared):
    g = torch.Generator().manual_seed(5)
    heads, nq, B, T, H = 2, 3, 4, 2, 16
    Ub = 2 if shared else B
    xq = torch.randn(B * nq, H, generator=g, dtype=torch.float64)
    xt = torch.randn(Ub * T, H, generator=g, dtype=torch.float64)
    ti = torch.tensor([1, 0, 0, 1]) if shared else None
    gg = torch.randn(heads, B, H, generator=g)
    tm = torch.tensor([[1, 0], [1, 1], [0, 0], [0, 1]], dtype=torch.uint8)[:Ub]
    ref, A, gx = cls_input64(xq, xt, ti, gg, tm, B, T, nq, with_gx=True)
    for p in range(B):
        t = int(ti[p]) if shared else p
        X = [xq[p * nq + j] for j in range(nq)] + [xt[t * T + j] for j in range(T)]
        ok = [True] * nq + [bool(tm[t, j]) for j in range(T)]
        for h in range(heads):
            s = [float(gg[h, p].double() @ x) / 8.0 if o else float("-inf") for x, o in zip(X, ok)]
            pr = _softmax(s)
            assert (ref[h, p] - sum(w * x for w, x in zip(pr, X))).abs().max() < 1e-13
            assert (A[h, p] - sum(w * x.abs() for w, x in zip(pr, X))).abs().max() < 1e-13
            assert abs(float(gx[h, p]) - max(float(gg[h, p].double().abs() @ x.abs()) / 8.0 for x in X)) < 1e-12


# ---- the bound against fp32 emulations of the kernels' rounding orders (one head: q [nq, 64], k / v [L, 64]) ----
def _trunc(x, dt):
    """round toward zero to the storage type (what a pack that drops the low bits does)"""
    drop = 16 if dt == torch.bfloat16 else 13
    return (x.float().view(torch.int32) >> drop << drop).view(torch.float32)


def _rne(x, dt):
    return x.to(dt).float()


def _emu_normalised(q, k, v, m, policy, dt, rnd=_rne):
    """the scalar kernels: fp32 scores, the mask added as they do, softmax in fp32, NORMALISED probabilities rounded"""
    s = q.float() @ k.float().T * 0.125
    s = torch.where(m[None, :], s, torch.full_like(s, -3.4028234663852886e38) if policy == "uniform" else s - 10000.0)
    p = rnd(torch.softmax(s, -1), dt)
    return (p @ v.float()).to(dt).double()


def _emu_online(q, k, v, m, policy, dt, rnd=_rne):
    """the matrix-core kernels' generic row tile: raw fp32 scores, online softmax over 32-key tiles in base 2,
    UNNORMALISED probabilities rounded before P.V, the denominator from the unrounded ones"""
    L, nq = k.shape[0], q.shape[0]
    s = q.float() @ k.float().T
    bias = -3.4028234663852886e38 if policy == "uniform" else -80000.0
    s = torch.where(m[None, :], s, s + bias)
    C = 0.125 * 1.4426950408889634
    mr, l, o = torch.full((nq,), float("-inf")), torch.zeros(nq), torch.zeros(nq, 64)
    for t in range(0, L, 32):
        a = s[:, t:t + 32]
        mn = torch.maximum(mr, a.max(1).values)
        al = torch.exp2((mr - mn) * C)
        pv = torch.exp2((a - mn[:, None]) * C)
        l = l * al + pv.sum(1)
        o = o * al[:, None] + rnd(pv, dt) @ v[t:t + 32].float()
        mr = mn
    return (o / l[:, None]).to(dt).double()


def _case(dt, L, nq, dens, scale, seed, ascending=False):
    g = torch.Generator().manual_seed(seed * 1000 + L * 7 + nq)
    q = (torch.randn(nq, 64, generator=g) * scale).to(dt)
    k = torch.randn(L, 64, generator=g) * scale
    if ascending:                                                  # every 32-key tile's scores grow: the running maximum moves
        k = k * (1.5 ** (torch.arange(L) // 32).float())[:, None]
    k = k.to(dt)
    v = torch.randn(L, 64, generator=g).to(dt)
    m = torch.rand(L, generator=g) < dens
    return q, k, v, m


def _ratio(out, q, k, v, m, policy, dt):
    nq = q.shape[0]
    ref, A = xattn64(q, k, v, m[None, :], 1, nq, policy)
    legacy = torch.full((nq,), policy == "unmasked" and not bool(m.any()))
    return ((out - ref).abs() / attn_bound(ref, A, dt, legacy)).max().item()


@pytest.mark.parametrize("policy", ["uniform", "unmasked"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_both_rounding_orders_stay_under_the_bound(dt, policy):
    worst = {"normalised": 0.0, "online": 0.0}
    for seed in range(3):
        for L in (33, 40, 64, 129, 257, 336):
            for dens in (0.0, 0.03, 0.15, 0.9):
                for scale, asc in ((1.5, False), (3.0, False), (4.0, True)):
                    q, k, v, m = _case(dt, L, 33, dens, scale, seed, asc)
                    worst["normalised"] = max(worst["normalised"],
                                              _ratio(_emu_normalised(q, k, v, m, policy, dt), q, k, v, m, policy, dt))
                    worst["online"] = max(worst["online"], _ratio(_emu_online(q, k, v, m, policy, dt), q, k, v, m, policy, dt))
    print(f"{dt} {policy}: worst err / bound {worst}")
    assert worst["normalised"] <= 1.0 and worst["online"] <= 1.0


def _pack_edge(dt, L):
    """Every key but key 0 gets a score whose unnormalised probability exp(s - max) = (1 + 0.98 * 2 ulp) / 2 sits just below
    a value of the storage type: rounding to nearest moves it by 1 % of an ulp, truncation by 98 %; V > 0 lets nothing
    cancel.  q = (8, 2^-4, 0, ...) makes the score k[0] + k[1] / 128: a head and a correction, both exact products."""
    u = U[dt]
    target = math.log(0.5 * (1 + 0.98 * 2 * u))
    q = torch.zeros(33, 64)
    q[:, 0], q[:, 1] = 8.0, 2.0 ** -4
    k = torch.zeros(L, 64)
    k0 = torch.tensor(target).to(dt).float()
    k[1:, 0] = k0
    k[1:, 1] = ((target - k0.double()) * 128.0).float()
    g = torch.Generator().manual_seed(L)
    v = torch.rand(L, 64, generator=g) + 0.5
    return q.to(dt), k.to(dt), v.to(dt), torch.ones(L, dtype=torch.bool)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_a_truncating_rounding_of_the_probabilities_exceeds_the_bound(dt):
    """The bound can bite: the same emulations with the probabilities TRUNCATED to the storage type fail it - on uniform
    weights 1 / 113 (a value 1.75 u above the one below it, in bf16) for the normalised order, and on the edge case above
    for the online order -, while the rounding versions pass both."""
    q, k, v, m = _pack_edge(dt, 96)
    assert _ratio(_emu_online(q, k, v, m, "uniform", dt), q, k, v, m, "uniform", dt) <= 1.0
    assert _ratio(_emu_online(q, k, v, m, "uniform", dt, _trunc), q, k, v, m, "uniform", dt) > 1.0
    inv = 1.0 / torch.arange(40, 400).float()                      # the L whose 1 / L loses most to truncation (113 in bf16)
    L = 40 + int(((inv - _trunc(inv, dt)) / inv).argmax())
    g = torch.Generator().manual_seed(7)
    q = torch.zeros(33, 64).to(dt)
    k = torch.randn(L, 64, generator=g).to(dt)
    v = (torch.rand(L, 64, generator=g) + 0.5).to(dt)
    m = torch.ones(L, dtype=torch.bool)
    assert _ratio(_emu_normalised(q, k, v, m, "uniform", dt), q, k, v, m, "uniform", dt) <= 1.0
    assert _ratio(_emu_normalised(q, k, v, m, "uniform", dt, _trunc), q, k, v, m, "uniform", dt) > 1.0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_split_g_emulation_stays_under_the_cls_input_bound(dt):
    """the input-space kernel: g as a 16-bit head plus a 16-bit remainder, fp32 scores, normalised probabilities rounded"""
    worst = 0.0
    for gs in (0.05, 0.3):
        for S in (33, 34, 47, 48, 64):
            for seed in range(3):
                g_ = torch.Generator().manual_seed(seed * 100 + S)
                nq, T = 33, S - 33
                X = (torch.randn(S, 768, generator=g_) * 0.7).to(dt)
                G = (torch.randn(12, 1, 768, generator=g_) * gs).float()
                tm = (torch.rand(1, T, generator=g_) < 0.7).to(torch.uint8)
                ref, A, gx = cls_input64(X[:nq], X[nq:], None, G, tm, 1, T, nq, with_gx=True)
                hi = G[:, 0].to(dt)
                lo = (G[:, 0] - hi.float()).to(dt)
                valid = torch.cat([torch.ones(nq, dtype=torch.bool), tm[0].bool()])
                s = ((hi.float() @ X.float().T) + (lo.float() @ X.float().T)) * 0.125
                s = s.masked_fill(~valid[None, :], -3.4028234663852886e38)
                out = (torch.softmax(s, -1).to(dt).float() @ X.float()).double()
                worst = max(worst, ((out - ref[:, 0]).abs() / cls_input_bound(A, gx, dt)[:, 0]).max().item())
    print(f"{dt}: worst err / bound {worst:.3f}")
    assert worst <= 1.0
