"""tests/image_ref.py checks itself on the CPU: every reference against an independent restatement (F.conv2d, the naive
masked mean, oracle.mask_pooling on the captured golden, an explicit loop), the exact families' 2^24 premise at every shape
the GPU file uses, the pessimistic fp32 chain against the 2^-20 A constant at every K the GPU file uses, and five mutants
that must each fail BOTH checks of the GPU tests - the exact family's torch.equal and the spread family's bound.

Which check catches which mutant:
  1. one product (patch embed, scorer) or one pixel (mean pool) dropped
                                  exact: the dropped term is a nonzero integer (chosen so); spread: a median-magnitude
                                  product is A / K, far above 2^-20 A and above the scorer's (C + 2) u A; a pixel of
                                  2049 moves a plain channel's mean by |f - mean| / 2048 against a bound of 2.5e-6.
  2. one dy row pair (32 consecutive k) of one channel skipped in patch embed
                                  the same, 32 products at once in every output.
  3. a pool pixel list with its last element dropped at a count of 2049 (a segment's one-pixel tail)
                                  exact: sum and count both change; spread: as 1.
  4. split-pool chunks cut with the remainder given to the LAST chunks
                                  exact: every chunk between the first and the last starts at another pixel; spread: the
                                  chunk means of randn move by ~1 / sqrt(size), the bound is ~1e-6.
  5. the scorer's c < C guard removed
                                  relation r adds the products of relation r + 1's first columns: nonzero integers /
                                  products of the size of the result."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H
from tests import image_ref as R

def test_patch_embed64_against_conv2d():
    for C, Hf, Wf, Cout in [(3, 48, 64, 8), (2, 40, 52, 5), (1, 16, 16, 3)]:
        feat, w, b = R.make_patch_embed("spread", C, Hf, Wf, Cout)
        ref, A = R.patch_embed64(feat, w, b)
        want = F.conv2d(feat.double(), w.double(), b.double(), stride=16).flatten(2).transpose(1, 2)[0]
        wantA = F.conv2d(feat.double().abs(), w.double().abs(), b.double().abs(), stride=16).flatten(2).transpose(1, 2)[0]
        assert ref.dtype == torch.float64 and ref.shape == ((Hf // 16) * (Wf // 16), Cout)
        assert bool(((ref - want).abs() <= 1e-14 * A).all()) and bool(((A - wantA).abs() <= 1e-14 * A).all())
        assert bool((A >= ref.abs()).all())
        # what lies beyond the last whole patch is never read
        feat[:, :, 16 * (Hf // 16):] = float("nan")
        feat[:, :, :, 16 * (Wf // 16):] = float("nan")
        assert torch.equal(R.patch_embed64(feat, w, b)[0], ref)


def test_resample_masks_is_the_closed_form_index_chain():
    """the interpolate -> pad -> interpolate chain equals the fp32 index formula (oracle.mask_grid_closed_form's, per
    object and with padding as no object) on the first geometries of the GPU test"""
    for pan, ids, img, pad, feat in R.slot_geometries()[:6]:
        m = R.resample_masks(pan, ids, img, pad, feat)
        assert m.shape == (len(ids), feat[0], feat[1]) and set(m.unique().tolist()) <= {0.0, 1.0}
        H0, W0 = pan.shape
        sy2, sx2 = np.float32(pad[0]) / np.float32(feat[0]), np.float32(pad[1]) / np.float32(feat[1])
        sy1, sx1 = np.float32(H0) / np.float32(img[0]), np.float32(W0) / np.float32(img[1])
        r, c = np.arange(feat[0], dtype=np.float32), np.arange(feat[1], dtype=np.float32)
        y1 = np.minimum(np.floor(r * sy2).astype(np.int64), pad[0] - 1)
        x1 = np.minimum(np.floor(c * sx2).astype(np.int64), pad[1] - 1)
        y0 = np.minimum(np.floor(y1.astype(np.float32) * sy1).astype(np.int64), H0 - 1)
        x0 = np.minimum(np.floor(x1.astype(np.float32) * sx1).astype(np.int64), W0 - 1)
        src = pan.numpy()[y0[:, None], x0[None, :]]
        inside = (y1 < img[0])[:, None] & (x1 < img[1])[None, :]
        for n, oid in enumerate(ids):
            assert np.array_equal(m[n].numpy() > 0.5, (src == oid) & inside), (oid, img, pad, feat)


def test_slot_geometries_reach_the_edges():
    geos = R.slot_geometries()
    hw = [f[0] * f[1] for *_, f in geos]
    assert max(hw) < 12000 and sum(h % 1024 != 0 for h in hw) >= 20 and min(hw) < 1024
    assert sum(f != (p[0] // 4, p[1] // 4) for _, _, _, p, f in geos) >= 5
    empty = pad0 = absent = 0
    for pan, ids, img, pad, feat in geos:
        m = R.resample_masks(pan, ids, img, pad, feat)
        empty += int((m.reshape(len(ids), -1).sum(1) == 0).sum())
        absent += sum(int((pan == i).sum()) == 0 for i in ids)
        pad0 += int(0 in ids and pad != img)
    assert empty >= 10 and absent >= 5 and pad0 >= 5, (empty, absent, pad0)


def test_mean_pool64_against_the_naive_formula():
    pan, ids, img, pad, feat_hw = R.slot_geometries()[0]
    for family in R.FAMILIES:
        feat = R.make_pool_feat(family, 8, *feat_hw)
        m = R.resample_masks(pan, ids, img, pad, feat_hw)
        ref, mag, counts = R.mean_pool64(feat, m)
        md = m[:, None].double()
        want = (feat.double() * md).sum(dim=[2, 3]) / (md.sum(dim=[2, 3]) + 1e-8)
        assert torch.equal(counts.double(), m.reshape(len(ids), -1).sum(1).double())
        assert bool(((ref - want).abs() <= 1e-13 * mag).all()) and bool((mag >= ref.abs() * (1 - 1e-8)).all())


def test_split_pool64_against_the_oracle_on_the_captured_golden():
    """oracle.mask_pooling is pinned on `_mask_pooling` itself by F4_pooling_scorer.npz (tests/test_oracle_golden.py)"""
    from oracle import psg_oracle as O
    g = dict(np.load(H.GOLDEN + "/F4_pooling_scorer.npz"))
    feature, masks = torch.from_numpy(g["pool_feature"]), torch.from_numpy(g["pool_masks"])
    for k in (1, 4, 7, 64):
        ref, mag, sizes = R.split_pool64(feature, masks[:, 0], k)
        want = torch.stack([O.mask_pooling(feature.double(), masks[i], k) for i in range(masks.shape[0])])
        assert bool(((ref - want).abs() <= 1e-13 * mag).all()), k
        if f"pool_k{k}" in g:
            np.testing.assert_allclose(ref.numpy(), g[f"pool_k{k}"], atol=1e-6)
    ref1, mag1, _ = R.split_pool64(feature, masks[:, 0], 1)
    refm, magm, _ = R.mean_pool64(feature, masks[:, 0])
    assert bool(((ref1[:, 0] - refm).abs() <= 1e-7 * magm).all())         # k = 1 is the mean but for the 1e-8


def test_bilinear64_against_an_explicit_loop():
    B, N, Rr, C = 2, 3, 2, 5
    sub, obj = R.make_bilinear("spread", B, N, Rr, C)
    ref, A = R.bilinear64(sub, obj, Rr)
    assert ref.shape == (B, Rr, N, N)
    for b in range(B):
        for r in range(Rr):
            for s in range(N):
                for o in range(N):
                    acc = a = 0.0
                    for c in range(C):
                        p = float(sub[b, s, r * C + c]) * float(obj[b, o, r * C + c])
                        acc, a = acc + p, a + abs(p)
                    assert abs(float(ref[b, r, s, o]) - acc) <= 1e-15 * a and abs(float(A[b, r, s, o]) - a) <= 1e-15 * a


def test_exact_families_hold_their_premise():
    for C, Hf, Wf, Cout in R.PE_SHAPES:
        assert 64 * C * 256 + 8 < 2 ** 24
    with pytest.raises(AssertionError):
        R.make_patch_embed("exact", 1024, 16, 16, 1)
    with pytest.raises(AssertionError):
        R.assert_exact_range(torch.tensor([2.0 ** 24]))
    feat, w, b = R.make_patch_embed("exact", 33, 32, 32, 16)
    for t in (feat, w, b):
        assert torch.equal(t, t.round()) and float(t.abs().max()) == 8
    ref, A = R.patch_embed64(feat, w, b)
    R.assert_exact_range(A)
    assert float(A.max()) <= 64 * 33 * 256 + 8 and torch.equal(ref, ref.round())
    assert 8 * R.POOL_HW[0] * R.POOL_HW[1] < 2 ** 24 and 8 * 12000 < 2 ** 24        # a pool sums at most the whole map
    f = R.make_pool_feat("exact", max(R.POOL_C), *R.POOL_HW)
    assert torch.equal(f, f.round()) and float(f.abs().max()) == 8
    for C in R.BIL_C:
        sub, obj = R.make_bilinear("exact", max(R.BIL_B), max(R.BIL_N), max(R.BIL_R), C)
        ref, A = R.bilinear64(sub, obj, max(R.BIL_R))
        R.assert_exact_range(A)
        assert float(A.max()) <= 64 * C and torch.equal(ref, ref.round())


def _pe_block(family, K, Cout=8):
    """a block of 4 patches x Cout outputs of the patch-embed GEMM at reduction length K"""
    feat, w, b = R.make_patch_embed(family, K // 256, 32, 32, Cout, seed=3)
    return R.unfold16(feat), w.reshape(Cout, -1), b


def _ref_A(a, w, b):
    ad, wd, bd = a.double(), w.double(), b.double()
    return ad @ wd.t() + bd, ad.abs() @ wd.abs().t() + bd.abs()


@pytest.mark.parametrize("K", R.PE_KS)
def test_fp32_chain_establishes_the_patch_embed_constant(K):
    """the pessimistic chain stays at or below 0.5 of 2^-20 A on the spread family and reproduces the exact family"""
    a, w, b = _pe_block("spread", K)
    ref, A = _ref_A(a, w, b)
    got = R.fp32_chain(a, w, b)
    ratio = R.worst(got, ref, R.bound32(A))
    print(f"fp32 chain K={K}: max err / (2^-20 A) = {ratio:.4f}; primary bound / (2^-20 A) >= {(256 + 3) / 16:.1f}")
    assert ratio <= 0.5
    assert R.worst(got, ref, R.patch_embed_bound(A, K // 256, 1)) <= 0.5
    a, w, b = _pe_block("exact", K)
    ref, A = _ref_A(a, w, b)
    R.assert_exact_range(A)
    assert torch.equal(R.fp32_chain(a, w, b), ref.float())


@pytest.mark.parametrize("K", R.PE_KS)
def test_patch_embed_mutants_fail_both_checks(K):
    C = K // 256
    for family in R.FAMILIES:
        a, w, b = _pe_block(family, K)
        ad, wd = a.double(), w.double()
        ref, A = _ref_A(a, w, b)
        # the dropped product of output (1, 2): the median-magnitude nonzero one
        p = (ad[1] * wd[2]).abs()
        k = int(torch.argsort(torch.where(p > 0, p, torch.full_like(p, float("inf"))))[int((p > 0).sum()) // 2])
        one = np.zeros((4, 8, K), dtype=bool)
        one[1, 2, k] = True
        rows = np.zeros((1, 1, K), dtype=bool)
        k0 = (C - 1) * 256 + 6 * 16
        rows[..., k0:k0 + 32] = True                                    # dy rows 6, 7 of the last channel
        for name, skip in (("product", one), ("dy rows", rows)):
            got = R.fp32_chain(a, w, b, skip=skip)
            if family == "exact":
                assert not torch.equal(got, ref.float()), (name, K)
            else:
                assert R.worst(got, ref, R.bound32(A)) > 1, (name, K)
                if name == "dy rows":                                   # 32 products: beyond the loose primary bound too
                    assert R.worst(got, ref, R.patch_embed_bound(A, C, min(C, 86))) > 1, (name, K)


def _pool_case(family, count=2049, C=8, hw=(80, 80)):
    """an object of `count` pixels as a row-major run starting at pixel 37, and another one behind it"""
    feat = R.make_pool_feat(family, C, *hw, seed=5)
    m = torch.zeros(2, hw[0] * hw[1])
    m[0, 37:37 + count] = 1
    m[1, 37 + count + 3:37 + count + 3 + 500] = 1
    return feat, m.reshape(2, *hw)


def test_pool_models_pass_and_mutants_fail_both_checks():
    for family in R.FAMILIES:
        feat, m = _pool_case(family)
        ref, mag, counts = R.mean_pool64(feat, m)
        assert counts.tolist() == [2049, 500]
        bound = R.mean_pool_bound(mag, counts)
        lists = R.pixel_lists(m)

        def fails(got):
            return (not torch.equal(got, R.exact_quotient(ref))) if family == "exact" else R.worst(got, ref, bound) > 1

        assert not fails(R.pool_fp32_model(feat, lists)), family
        cut = [lists[0][:-1], lists[1]]                                 # the last pixel of 2049 dropped
        assert fails(R.pool_fp32_model(feat, cut)), family
        assert fails(R.pool_fp32_model(feat, cut, count_as=counts)), family          # ... from the sum only
        mid = [torch.cat([lists[0][:1000], lists[0][1001:]]), lists[1]]   # one pixel in the middle dropped
        assert fails(R.pool_fp32_model(feat, mid)), family
        # and the reference itself moves when its input list does
        cut_ref, _, _ = R.split_pool64(feat, m, 1, lists=cut)
        assert fails(cut_ref[:, 0].float()), family


@pytest.mark.parametrize("k", [4, 7, 64])
def test_split_pool_model_passes_and_the_remainder_mutant_fails_both_checks(k):
    for family in R.FAMILIES:
        feat, m = _pool_case(family, count=k * 64 + 1 if k < 64 else 4289)
        ref, mag, sizes = R.split_pool64(feat, m, k)
        assert sizes[0, 0] == sizes[0, -1] + 1                          # a remainder: the first chunk is the longer one
        bound = R.split_pool_bound(mag, sizes)
        lists = R.pixel_lists(m)

        def fails(got):
            return (not torch.equal(got, R.exact_quotient(ref))) if family == "exact" else R.worst(got, ref, bound) > 1

        assert not fails(R.split_fp32_model(feat, lists, k)), (family, k)
        assert fails(R.split_fp32_model(feat, lists, k, remainder_last=True)), (family, k)
        assert fails(R.split_pool64(feat, m, k, remainder_last=True)[0].float()), (family, k)
        assert fails(R.split_fp32_model(feat, [lists[0][:-1], lists[1]], k)), (family, k)


@pytest.mark.parametrize("C", [1, 2, 31, 33, 100])
def test_bilinear_model_passes_and_mutants_fail_both_checks(C):
    B, N, Rr = 2, 5, 3
    for family in R.FAMILIES:
        sub, obj = R.make_bilinear(family, B, N, Rr, C, seed=2)
        ref, A = R.bilinear64(sub, obj, Rr)
        bound = R.bilinear_bound(A, C)

        def fails(got):
            return (not torch.equal(got, ref.float())) if family == "exact" else R.worst(got, ref, bound) > 1

        assert not fails(R.bilinear_fp32_model(sub, obj, Rr)), (family, C)
        unguarded = R.bilinear_fp32_model(sub, obj, Rr, guard=False)
        assert fails(unguarded), (family, C)
        assert torch.equal(unguarded[:, -1], R.bilinear_fp32_model(sub, obj, Rr)[:, -1])   # the last relation reads zeros
        # one dropped product of relation 1: the median-magnitude nonzero one of the first (s, o) that has any
        prod = (sub[1, :, None, C:2 * C].double() * obj[1, None, :, C:2 * C].double()).abs()
        s, o = [int(i) for i in torch.nonzero(prod.sum(-1) > 0)[0]]
        p = prod[s, o]
        c = int(torch.argsort(torch.where(p > 0, p, torch.full_like(p, float("inf"))))[int((p > 0).sum()) // 2])
        assert fails(R.bilinear_fp32_model(sub, obj, Rr, skip=(1, 1, s, o, c))), (family, C)


def test_pinned_pool_scene_reaches_the_edges():
    """the identity geometry reproduces the painted counts, and over k in POOL_KS they give m = 0, m < k, m = k,
    m = 64 k + remainder and chunks of 64, 65 and 129"""
    pan, ids, counts = R.pinned_pool_scene()
    masks = R.resample_masks(pan, ids, R.POOL_HW, R.POOL_HW, R.POOL_HW)
    assert masks.reshape(len(ids), -1).sum(1).long().tolist() == [counts[i] for i in ids]
    assert set(R.POOL_COUNTS) | {0} <= set(counts.values()) and ids != sorted(ids)
    assert (R.POOL_HW[0] * R.POOL_HW[1]) % 1024 == 996
    assert bool(masks[ids.index(0)].reshape(-1)[-100:].all())           # an object inside the index pass's partial block
    ms = list(counts.values())
    sizes_seen, below, equal, above = set(), False, False, False
    for k in R.POOL_KS:
        _, _, sizes = R.split_pool64(torch.zeros(1, 4, *R.POOL_HW), masks, k)
        sizes_seen |= set(sizes.reshape(-1).tolist())
        below |= any(0 < m < k for m in ms)
        equal |= k in ms
        above |= any(m > 64 * k and m % k for m in ms)
    assert below and equal and above and {0, 1, 64, 65, 129} <= sizes_seen
