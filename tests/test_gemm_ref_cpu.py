"""tests/gemm_ref.py checks itself on the CPU: ref64 against an explicit triple loop, the exact family's 2^24 premise,
the Abramowitz-Stegun error constant, and a pessimistic fp32 model of the kernels' accumulation (gemm_ref.fp32_model)
against both checks of the GPU tests on every (dtype, K, slices) combination they use - the clean model stays at or
below 0.5 of the 2^-20 A bound and reproduces the exact family bit for bit; four mutated models do not pass.

Which check catches which mutant (each is run on both families, both dtypes):
  1. one product dropped                               exact: torch.equal fails (the product is a nonzero integer);
                                                       spread: the median-magnitude product is >= 100x the bound.
  2. two x rows swapped                                exact: fails (independent integer rows); spread: the rows differ
                                                       in scale by 2^(16 / (M - 1)) or more, far beyond the bound.
  3. the 16-byte pieces (8 elements) of one 64-element K block permuted on the w side only
                                                       exact: fails (x_k now meets w_pi(k)); spread: fails, the moved
                                                       products are each of the size of a dropped one.
  4. one weight row of a partial last slab replaced by its clamped neighbour, row N - 1
                                                       exact: fails in that output column; spread: fails there, the
                                                       two rows are independent draws.
None of the four is coincidental on these inputs, so every one must fail BOTH checks."""
import pytest
import torch

from tests import gemm_ref as G

# every K the GPU tests use (skinny: 64 .. 1088; dense: 64, 128, 192), the exact family's limit 2048, and the split
# counts they force or the planner picks on any device (1 .. 16)
KS = (64, 128, 192, 320, 960, 1024, 1088, 2048)
SLICES = (1, 2, 3, 4, 8, 16)
M, N = 5, 16


def test_ref64_against_a_triple_loop():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, generator=g).bfloat16()
    w = torch.randn(4, 5, generator=g).bfloat16()
    ref, A = G.ref64(x, w)
    assert ref.dtype == torch.float64 and ref.shape == (3, 4) and A.shape == (3, 4)
    for m in range(3):
        for n in range(4):
            s = a = 0.0
            for k in range(5):
                p = float(x[m, k]) * float(w[n, k])
                s, a = s + p, a + abs(p)
            assert abs(float(ref[m, n]) - s) <= 1e-15 * a and abs(float(A[m, n]) - a) <= 1e-15 * a
    assert bool((A >= ref.abs()).all())


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_families_are_what_they_claim(dtype):
    x, w = G.make_x("exact", 32, 2048, dtype), G.make_w("exact", 48, 2048, dtype)
    assert torch.equal(x.double(), x.double().round()) and float(x.double().abs().max()) == 8
    assert torch.equal(w.double(), w.double().round()) and float(w.double().abs().max()) == 8
    ref, A = G.ref64(x, w)
    G.assert_exact_range(A)
    assert float(A.max()) <= 64 * 2048
    with pytest.raises(AssertionError):
        G.make_x("exact", 1, 2112, dtype)
    with pytest.raises(AssertionError):
        G.assert_exact_range(torch.tensor([2.0 ** 24]))
    for Mx in (1, 17, 32):
        x, w = G.make_x("spread", Mx, 1088, dtype), G.make_w("spread", 80, 1088, dtype)
        for t in (x, w):                                     # normal in fp16 (hence in bf16), finite, rows all different
            a = t.double().abs()
            assert bool(torch.isfinite(a).all()) and float(a.min()) >= 2.0 ** -14
            assert len({tuple(r.tolist()) for r in t[:, :8].double()}) == t.shape[0]
    # same seed -> same tensors (the GPU tests share them), independent of the other operand's shape
    assert torch.equal(G.make_w("spread", 80, 1088, dtype), w)


def test_as_erf_constant_and_gelu_slope():
    E = G.as_erf_max_error()
    assert 5e-8 < E < 2e-7, E                                # A&S quote 1.5e-7 for 7.1.26
    v = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    slope = ((G.gelu64(v[1:]) - G.gelu64(v[:-1])) / (v[1:] - v[:-1])).abs().max().item()
    assert 1.12 < slope < 1.13


def test_swiglu_reference_and_bound():
    """the rounded reference of an exactly representable case, and the bound covers a flipped rounding of the gate"""
    for dtype in G.DTYPES:
        g = torch.tensor([0.0, 1.0, -2.0, 3.0], dtype=torch.float64)
        u = torch.tensor([5.0, -2.0, 0.5, 1.0], dtype=torch.float64)
        z = torch.zeros_like(g)
        ref, bound = G.swiglu64(g, u, z, z, dtype)
        want = ((g * torch.sigmoid(g)).to(dtype).double() * u).to(dtype).double()
        assert torch.equal(ref, want) and bool((bound > 0).all())
        # a gate on a rounding tie: the kernel's fp32 value may sit on either side of it
        tie = torch.tensor([1.0 + 2.0 ** (-8 if dtype == torch.bfloat16 else -11)], dtype=torch.float64)
        A = torch.tensor([4.0], dtype=torch.float64)
        up = torch.tensor([3.0], dtype=torch.float64)
        ref, bound = G.swiglu64(tie, up, A, A, dtype)
        other, _ = G.swiglu64(tie + 2.0 ** -22 * 4.0, up, A, A, dtype)
        assert float((other - ref).abs()) <= float(bound)


def _ratio(part, ref, A):
    return G.worst(G.sum_slices(part), ref, G.bound32(A))


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_clean_model_passes_both_checks(dtype):
    worst = 0.0
    for K in KS:
        xe, we = G.make_x("exact", M, K, dtype), G.make_w("exact", N, K, dtype)
        xs, ws = G.make_x("spread", M, K, dtype), G.make_w("spread", N, K, dtype)
        re, Ae = G.ref64(xe, we)
        rs, As = G.ref64(xs, ws)
        G.assert_exact_range(Ae)
        for S in SLICES:
            if S > K // 64:
                continue
            assert torch.equal(G.sum_slices(G.fp32_model(xe, we, S)), re.float()), (K, S)
            r = _ratio(G.fp32_model(xs, ws, S), rs, As)
            worst = max(worst, r)
            assert r <= 0.5, f"{G.NAMES[dtype]} K={K} slices={S}: clean model at {r:.3g} of the bound"
    print(f"{G.NAMES[dtype]}: clean sequential fp32 model, worst err / bound = {worst:.3g}")


def _median_product(x, w, m, n):
    """k of the median-magnitude NONZERO product of output (m, n)"""
    p = (x[m].double() * w[n].double()).abs()
    idx = torch.nonzero(p > 0).flatten()
    return int(idx[torch.argsort(p[idx])[idx.numel() // 2]])


def _mutants(x, w, S, Kmut):
    """(name, fp32 partials) of the four mutated models; Kmut: the 64-element K block that mutant 3 permutes"""
    Mx, Nw = x.shape[0], w.shape[0]
    yield "dropped product", G.fp32_model(x, w, S, drop=(2, 7, _median_product(x, w, 2, 7)))
    rows = list(range(Mx))
    rows[1], rows[3] = rows[3], rows[1]
    yield "x rows swapped", G.fp32_model(x[rows], w, S)
    wp = w.clone()
    blk = wp[:, 64 * Kmut:64 * Kmut + 64].reshape(Nw, 8, 8)
    wp[:, 64 * Kmut:64 * Kmut + 64] = blk[:, [1, 0, 3, 2, 5, 4, 7, 6]].reshape(Nw, 64)
    yield "w pieces permuted", G.fp32_model(x, wp, S)
    wc = w.clone()
    wc[Nw - 6] = w[Nw - 1]
    yield "clamped weight row", G.fp32_model(x, wc, S)


@pytest.mark.parametrize("dtype", G.DTYPES)
@pytest.mark.parametrize("K,S", [(320, 2), (1088, 1), (1088, 4), (2048, 8)])
def test_mutated_models_fail_both_checks(dtype, K, S):
    Nw = 80                                                   # second slab of 64 rows partial: rows 64 .. 79
    xe, we = G.make_x("exact", M, K, dtype), G.make_w("exact", Nw, K, dtype)
    xs, ws = G.make_x("spread", M, K, dtype), G.make_w("spread", Nw, K, dtype)
    re, _ = G.ref64(xe, we)
    rs, As = G.ref64(xs, ws)
    for name, part in _mutants(xe, we, S, K // 128):
        assert not torch.equal(G.sum_slices(part), re.float()), f"exact family misses: {name}"
    for name, part in _mutants(xs, ws, S, K // 128):
        r = _ratio(part, rs, As)
        print(f"{G.NAMES[dtype]} K={K} slices={S}: {name} at {r:.3g} of the bound")
        assert r > 1.0, f"spread bound misses: {name} ({r:.3g})"
        with pytest.raises(AssertionError):
            G.check_out(name, G.sum_slices(part), rs, G.bound32(As))


def test_check_out_overflow_rule_and_nan():
    ref = torch.tensor([65500.0, 100.0], dtype=torch.float64)
    bound = torch.tensor([40.0, 0.1], dtype=torch.float64)
    got = torch.tensor([float("inf"), 100.0], dtype=torch.float16)
    assert G.check_out("overflow", got, ref, bound, torch.float16) <= 1.0
    for bad in ([-float("inf"), 100.0], [65500.0, float("inf")], [65500.0, float("nan")]):
        with pytest.raises(AssertionError):
            G.check_out("bad", torch.tensor(bad, dtype=torch.float16), ref, bound, torch.float16)
