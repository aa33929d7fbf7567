"""Float64 references, input families and derived bounds for the image-side fp32 kernels: psg_patch_embed
(psg_patch_embed.hip), psg_masked_mean_pool / psg_masked_split_mean_pool / psg_bilinear_scores (psg_pool.hip) and
psg_qformer_embed (psg_rowops.hip).  tests/test_gpu_image_kernels_ref.py checks the kernels against this file and
tests/test_image_ref_cpu.py checks this file on the CPU.  Pure torch (numpy only in the fp32 models), written from the
formulas of the operations and not from the kernels; the references work on whatever device their tensors live on.

References (each returns float64 and the magnitude sum its bound is scaled to):

  patch_embed64     Conv2d(C, Cout, k = 16, s = 16) + flatten + transpose as unfold + matmul: out[l][o] = b[o] +
                    sum_k a[l][k] w[o][k], k = c 256 + dy 16 + dx, l = py gw + px; A = |a| @ |w|^T + |b|.  Rows and columns
                    of the feature map beyond 16 gh / 16 gw belong to no patch and are never read.
  resample_masks    (pan == id).float() -> F.interpolate(size = img) -> F.pad -> F.interpolate(size = feat), on the CPU:
                    the detectors' own chain (ATen legacy 'nearest' derives its scale in the precision of the tensor).
                    Padding is no object, an id of 0 included.
  mean_pool64       sum over the object's pixels / (count + 1e-8); magnitude sum |f| / count.
  split_pool64      `_mask_pooling`: the object's pixels in row-major order cut into k chunks, the first m mod k one pixel
                    longer; m < k repeats the list (chunk c = pixel c mod m); m = 0 gives zeros; magnitude sum |f| / size.
  bilinear64        reshape [B, N, R, C] -> permute -> einsum('nrsc,nroc->nrso'); A = sum_c |s| |o|.
  qformer_embed     no reference of its own: LayerNorm(word[id] + pos[t]) and LayerNorm(query[r]) are `_ln_expect` of
                    tests/test_gpu_rowops_ref.py with x = word[id], res_rows = pos[t], no bias.

Two input families:

  exact    integers in [-8, 8] (the gemm_ref convention), drawn independently per element.  The premise, asserted by
           `assert_exact_range` on the magnitude sums: every sum of products or pixels IN ANY ORDER is an integer below
           2^24, hence exact in fp32 - patch embed 64 C 256 + 8 (C <= 1023), the pools 8 count, the scorer 64 C.  The fp32
           result of patch embed and of the scorer must then equal the integer result bit for bit (torch.equal): a
           dropped, doubled or misplaced element fails it.  For the pools the sum is exact and one division remains: the
           expected value is the float64 quotient rounded once to fp32 (`exact_quotient`).  The library is built with -O3
           and no fast-math flag, so its fp32 division is correctly rounded, and the two roundings agree: the quotient
           s / m of integers |s| <= 8 m, m < 2^16, is never a rounding tie of fp32 (a tie needs 25 significant bits, a
           dyadic s / m has at most 16) and lies at least 2^-25 / m (relative) from the nearest tie, while the reference's
           1e-8 in the denominator moves it by 1e-8 / m and float64's own rounding by 2^-53.
  spread   patch embed and the scorer: randn rows scaled over 9 decades (logspace(-6, 3) across the patches / the subject
           rows) against weight / object rows of randn * 2^randint(-6, 6) (/ sqrt(K) for patch embed), so an absolute
           tolerance means nothing and a swapped row cannot cancel.  The pools: randn plus a common offset of +1000 on
           every third channel, so a sum that loses low bits to cancellation shows.

Bounds, per element, u = 2^-24:

  scorer       (C + 2) u A: a k-ordered fmaf chain over C padded to a multiple of 32 (the padding adds zeros).
  mean pool    (32 + 6 + nseg + 2) u sum|f| / count: a lane makes at most 2048 / 64 = 32 serial adds per 2048-pixel
               segment, the wave's tree adds 6, nseg = ceil(count / 2048) segment sums are added, one division, one spare.
  split pool   (ceil(size / 64) + 6 + 2) u sum|f| / size: the same with one chunk per wave.
  patch embed  primary: (cps 256 + S + 2) u A with S K-splits of cps = ceil(C / S) channels: one fmaf chain per split, the
               splits summed in order, the bias added.  S is read back from psg_patch_embed_workspace (`pe_splits`), never
               from a CU count.  Always safe, loose at K = 65536; so patch embed is ALSO held to the project's constant
               for this MFMA chain, 2^-20 A (REL32: gemm_ref.py, test_gpu_gemm_w8.py).  That constant is established by
               `fp32_chain` below, not by the kernel: a deliberately pessimistic fp32 model - every product rounded to
               fp32 and added to ONE running fp32 sum, front to back over the whole K, a chain longer than any split's.
               Measured by tests/test_image_ref_cpu.py on the spread family for a block of 4 patches x 8 output channels:
               max err / (2^-20 A) = 0.070, 0.038, 0.046, 0.056, 0.047, 0.152 at K = 256, 512, 768, 1280, 8448, 65792
               (every K the GPU file uses); asserted <= 0.5, the margin of 2 covering that the model's order is not the
               kernel's.  No larger power of two was needed.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
REL32 = 2.0 ** -20
FAMILIES = ("exact", "spread")
PATCH = 16
POOL_SEG = 2048

# the shapes of tests/test_gpu_image_kernels_ref.py (here, so that the CPU self-test covers exactly what the GPU file uses)
PE_SHAPES = [(1, 16, 16, 128),                                         # C = 1, L = 1
             (3, 48, 64, 128),                                         # C = 3, L = 12 < 128, Cout = 128
             (2, 48, 688, 256),                                        # L = 129: one full row tile plus one row
             (2, 50, 692, 256),                                        # the same with Hf % 16 = 2, Wf % 16 = 4
             (5, 40, 52, 384),                                         # Hf % 16 = 8, Wf % 16 = 4 (Wf % 4 = 0), Cout = 384
             (33, 256, 256, 1024),                                     # K splits of unequal channel counts (256 CUs: 17
             (257, 256, 256, 256)]                                     #   splits of 2 / 86 of 3): (C, Hf, Wf, Cout)
PE_UNEVEN = PE_SHAPES[-2:]
PE_KS = sorted({c * 256 for c, _, _, _ in PE_SHAPES})
BIL_N, BIL_C, BIL_R, BIL_B = (1, 31, 32, 33, 65), (1, 2, 31, 32, 33, 100), (1, 3), (1, 2)
POOL_HW = (150, 150)                                                   # HW % 1024 = 996
POOL_C = (4, 68)
POOL_KS = (1, 4, 7, 64)
# pixel counts at the boundaries of pool_partial (the 64-stride tail, the 4 x 64 unrolled loop, the 2048-pixel segment);
# 129 and 449 = 7 * 64 + 1 add the chunk sizes 129 (k = 1) and 65 | 64 (k = 7) of the split pool
POOL_COUNTS = (1, 63, 64, 65, 192, 193, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 4289, 129, 449)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def assert_exact_range(A):
    """the exact family's premise: every partial sum in any order is an integer below 2^24"""
    assert float(A.max()) < 2.0 ** 24, f"exact family: a magnitude sum reaches {float(A.max()):.0f} >= 2^24"


def worst(got, ref, bound):
    """max err / bound (a NaN or infinite result counts as infinitely wrong)"""
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max())


# ---- patch embed ----
def unfold16(feat):
    """[1, C, Hf, Wf] or [C, Hf, Wf] -> the im2col matrix [L, C 256] of the 16 x 16 patches, k = c 256 + dy 16 + dx"""
    f = feat.reshape(feat.shape[-3:])
    C, Hf, Wf = f.shape
    gh, gw = Hf // PATCH, Wf // PATCH
    f = f[:, :PATCH * gh, :PATCH * gw].reshape(C, gh, PATCH, gw, PATCH)
    return f.permute(1, 3, 0, 2, 4).reshape(gh * gw, C * PATCH * PATCH)


def patch_embed64(feat, w, b):
    """(reference [L, Cout], A = |a| @ |w|^T + |b|) in float64"""
    a = unfold16(feat.double())
    wm = w.double().reshape(w.shape[0], -1)
    bd = b.double()
    return a @ wm.t() + bd, a.abs() @ wm.abs().t() + bd.abs()


def make_patch_embed(family, C, Hf, Wf, Cout, seed=0):
    """(feat [1, C, Hf, Wf], weight [Cout, C, 16, 16], bias [Cout]) fp32 on the CPU"""
    g = _gen(1000003 * seed + 7919 * C + 131 * Hf + 17 * Wf + Cout)
    K = C * PATCH * PATCH
    if family == "exact":
        assert C <= 1023, "exact family: C <= 1023 keeps A <= 64 C 256 + 8 below 2^24"
        feat = torch.randint(-8, 9, (1, C, Hf, Wf), generator=g).float()
        w = torch.randint(-8, 9, (Cout, C, PATCH, PATCH), generator=g).float()
        return feat, w, torch.randint(-8, 9, (Cout,), generator=g).float()
    assert family == "spread", family
    gh, gw = Hf // PATCH, Wf // PATCH
    rows = torch.logspace(-6, 3, gh * gw).reshape(gh, gw)                 # one scale per patch = per row of the GEMM
    scale = torch.ones(Hf, Wf)
    scale[:PATCH * gh, :PATCH * gw] = rows.repeat_interleave(PATCH, 0).repeat_interleave(PATCH, 1)
    feat = torch.randn(1, C, Hf, Wf, generator=g) * scale
    wscale = torch.exp2(torch.randint(-6, 6, (Cout, 1, 1, 1), generator=g).float()) / math.sqrt(K)
    w = torch.randn(Cout, C, PATCH, PATCH, generator=g) * wscale
    return feat, w, torch.randn(Cout, generator=g) * wscale.reshape(-1) * math.sqrt(K)


def pe_splits(workspace_bytes, L, Cout):
    """the K-split count S of psg_patch_embed, recovered from its workspace: S partial tiles of [mt 128, Cout] fp32"""
    mt = (L + 127) // 128
    S, rest = divmod(workspace_bytes, 4 * 128 * mt * Cout)
    assert rest == 0 and S >= 1, (workspace_bytes, L, Cout)
    return S


def patch_embed_bound(A, C, S):
    """the primary bound: one fmaf chain of cps 256 per split, S splits summed in order, the bias"""
    cps = -(-C // S)
    return (cps * 256 + S + 2) * U * A


def bound32(A):
    return REL32 * A


def fp32_chain(a, w, b=None, skip=None):
    """fp32 model of a @ w^T (+ b): every product rounded to fp32 and added to ONE running fp32 sum, front to back over the
    whole K (numpy's accumulate is strictly sequential).  skip = boolean [M, N, K] or anything broadcastable to it: the
    products left out (a mutant).  a [M, K], w [N, K] -> fp32 [M, N]."""
    an, wn = a.float().numpy(), w.float().numpy()
    p = an[:, None, :] * wn[None, :, :]
    assert p.dtype == np.float32
    if skip is not None:
        p = np.where(np.asarray(skip), np.float32(0), p)
    out = np.add.accumulate(p, axis=-1, dtype=np.float32)[..., -1]
    if b is not None:
        out = out + b.float().numpy()[None, :]
    assert out.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(out))


# ---- the pools ----
def resample_masks(pan, ids, img_hw, pad_hw, feat_hw):
    """the detectors' chain on the CPU -> float32 masks [N, Hf, Wf] of 0 / 1"""
    pan = pan.cpu()
    masks = torch.stack([(pan == int(i)) for i in ids]).float()[None]
    m = F.interpolate(masks, size=(int(img_hw[0]), int(img_hw[1])))
    m = F.pad(m, (0, int(pad_hw[1]) - int(img_hw[1]), 0, int(pad_hw[0]) - int(img_hw[0])))
    return F.interpolate(m, size=(int(feat_hw[0]), int(feat_hw[1])))[0]


def pixel_lists(masks):
    """the row-major pixel indices of every object: a list of int64 tensors"""
    flat = masks.reshape(masks.shape[0], -1) >= 0.5
    return [torch.nonzero(flat[n]).reshape(-1) for n in range(flat.shape[0])]


def mean_pool64(feat, masks):
    """feat [1, C, Hf, Wf] or [C, Hf, Wf], masks [N, Hf, Wf] -> (sum / (count + 1e-8) [N, C], sum|f| / count [N, C],
    counts [N]) in float64; an object without pixels has 0 in both"""
    f = feat.double().reshape(feat.shape[-3], -1).cpu()
    lists = pixel_lists(masks)
    ref = torch.zeros(len(lists), f.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for n, px in enumerate(lists):
        if px.numel():
            ref[n] = f[:, px].sum(1) / (px.numel() + 1e-8)
            mag[n] = f[:, px].abs().sum(1) / px.numel()
    return ref, mag, torch.tensor([px.numel() for px in lists])


def split_chunks(m, k, remainder_last=False):
    """the chunk of each entry of a pixel list of m >= k entries cut into k chunks: int64 [m], sizes int64 [k].  The first
    m mod k chunks are one longer (remainder_last = True, a mutant: the last ones are)."""
    base, rem = divmod(m, k)
    sizes = torch.full((k,), base, dtype=torch.int64)
    if rem:
        if remainder_last:
            sizes[k - rem:] += 1
        else:
            sizes[:rem] += 1
    return torch.repeat_interleave(torch.arange(k), sizes), sizes


def split_pool64(feat, masks, k, lists=None, remainder_last=False):
    """`_mask_pooling(feature, mask, k)` per object -> (chunk means [N, k, C], sum|f| / size [N, k, C], chunk sizes [N, k])
    in float64.  lists: pixel lists to use instead of the masks' own (a mutant)."""
    f = feat.double().reshape(feat.shape[-3], -1).cpu()
    lists = pixel_lists(masks) if lists is None else lists
    N, C = len(lists), f.shape[0]
    ref = torch.zeros(N, k, C, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    sizes = torch.zeros(N, k, dtype=torch.int64)
    for n, px in enumerate(lists):
        m = px.numel()
        if m == 0:
            continue
        if m < k:                                                       # the list repeated up to k entries
            px = px[torch.arange(k) % m]
            m = k
        chunk, size = split_chunks(m, k, remainder_last)
        vals = f[:, px].t()                                             # [m, C]
        ref[n] = torch.zeros(k, C, dtype=torch.float64).index_add_(0, chunk, vals) / size[:, None]
        mag[n] = torch.zeros(k, C, dtype=torch.float64).index_add_(0, chunk, vals.abs()) / size[:, None]
        sizes[n] = size
    return ref, mag, sizes


def exact_quotient(ref):
    """exact family of the pools: the float64 quotient rounded once to fp32 (see the module docstring).  Observed on an
    MI355X: the kernels' fp32 division agrees with it bit for bit at every pinned count - it is correctly rounded."""
    return ref.float()


def mean_pool_bound(mag, counts):
    nseg = (counts + POOL_SEG - 1) // POOL_SEG
    return (32 + 6 + nseg.double() + 2)[:, None] * U * mag


def split_pool_bound(mag, sizes):
    return (((sizes + 63) // 64).double() + 6 + 2)[:, :, None] * U * mag


def make_pool_feat(family, C, Hf, Wf, seed=0):
    """feature map [1, C, Hf, Wf] fp32 on the CPU"""
    g = _gen(1000003 * seed + 7919 * C + 131 * Hf + Wf)
    if family == "exact":
        assert 8 * Hf * Wf < 2 ** 24, "exact family: an object has at most Hf Wf pixels, its sum stays below 2^24"
        return torch.randint(-8, 9, (1, C, Hf, Wf), generator=g).float()
    assert family == "spread", family
    feat = torch.randn(1, C, Hf, Wf, generator=g)
    feat[:, 1::3] += 1000.0                                             # channels with a large common offset
    return feat


def _geometry(rng, max_hw=12000):
    """a random (pan, ids, img, pad, feat) in the style of test_mask_kernels_bit_exact_on_random_geometries, small enough
    for the feature map to stay below max_hw pixels"""
    while True:
        H0, W0 = int(rng.integers(17, 261)), int(rng.integers(17, 261))
        scale = float(rng.uniform(0.4, 2.2))
        img_h, img_w = max(16, int(round(H0 * scale))), max(16, int(round(W0 * scale)))
        pad_h, pad_w = -(-img_h // 32) * 32, -(-img_w // 32) * 32
        if rng.random() < 0.3:
            pad_h += 32
        if rng.random() < 0.35:                                         # a feature map that is not pad / 4
            Hf, Wf = int(rng.integers(5, 100)), int(rng.integers(5, 100))
        else:
            Hf, Wf = pad_h // 4, pad_w // 4
        if Hf * Wf < max_hw:
            break
    n = int(rng.integers(1, 12))
    ids = [int(rng.integers(0, 133)) + 1000 * int(rng.integers(0, 3)) for _ in range(n)]
    if rng.random() < 0.5:
        ids.append(0)                                                   # id 0 is an object; padding must not count as it
    ids = list(dict.fromkeys(ids))
    pan = np.full((H0, W0), 0 if rng.random() < 0.4 else 133, dtype=np.int32)
    for oid in ids:
        y0, x0 = int(rng.integers(0, H0)), int(rng.integers(0, W0))
        hh, ww = int(rng.integers(1, max(2, H0 // 2))), int(rng.integers(1, max(2, W0 // 2)))
        pan[y0:y0 + hh, x0:x0 + ww] = oid
    ids += [7777, 4242][:int(rng.integers(0, 3))]                       # ids absent from the map
    order = rng.permutation(len(ids))
    return torch.from_numpy(pan), [ids[i] for i in order], (img_h, img_w), (pad_h, pad_w), (Hf, Wf)


def slot_geometries():
    """the 40 seeded geometries of the slot-chain test"""
    rng = np.random.default_rng(4321)
    return [_geometry(rng) for _ in range(40)]


def pinned_pool_scene():
    """(pan int32 [150, 150], ids in unsorted order, {id: pixel count}) for the identity geometry (the id map IS the
    feature-resolution slot map): row-major runs of POOL_COUNTS in a shuffled order with gaps of 1..3 background pixels,
    an object scattered over every third pixel of a region, an object on the last 100 pixels of the map (the index
    pass's partial block of 996) and an id that is absent (count 0)."""
    Hf, Wf = POOL_HW
    HW = Hf * Wf
    rng = np.random.default_rng(77)
    flat = np.full(HW, 9999, dtype=np.int32)
    counts, pos = {}, 5
    for j, i in enumerate(rng.permutation(len(POOL_COUNTS))):
        oid = 100 + 3 * int(i)
        flat[pos:pos + POOL_COUNTS[i]] = oid
        counts[oid] = POOL_COUNTS[i]
        pos += POOL_COUNTS[i] + 1 + j % 3
    assert pos <= 20700
    flat[20700:21300:3] = 7                                             # scattered: 200 pixels
    counts[7] = 200
    flat[HW - 100:] = 0                                                 # id 0 on the last pixels of the map
    counts[0] = 100
    counts[31337] = 0                                                   # absent
    ids = [int(i) for i in rng.permutation(list(counts))]
    assert ids != sorted(ids) and sum(counts.values()) < HW
    return torch.from_numpy(flat.reshape(Hf, Wf)), ids, counts


def pool_fp32_model(feat, lists, count_as=None):
    """fp32 model of the mean pool: the listed pixels added one at a time to a running fp32 sum, divided in fp32 by the
    count (count_as: the counts to divide by instead of the lists' own) -> fp32 [N, C]"""
    f = feat.float().reshape(feat.shape[-3], -1).numpy()
    out = np.zeros((len(lists), f.shape[0]), dtype=np.float32)
    for n, px in enumerate(lists):
        m = px.numel() if count_as is None else int(count_as[n])
        if px.numel():
            s = np.add.accumulate(f[:, px.numpy()], axis=-1, dtype=np.float32)[:, -1]
            out[n] = s / (np.float32(m) + np.float32(1e-8))
    return torch.from_numpy(out)


def split_fp32_model(feat, lists, k, remainder_last=False):
    """fp32 model of the split pool: each chunk's pixels added one at a time in fp32, divided in fp32 by the chunk size"""
    f = feat.float().reshape(feat.shape[-3], -1).numpy()
    out = np.zeros((len(lists), k, f.shape[0]), dtype=np.float32)
    for n, px in enumerate(lists):
        m = px.numel()
        if m == 0:
            continue
        if m < k:
            px, m = px[torch.arange(k) % m], k
        _, size = split_chunks(m, k, remainder_last)
        pos = 0
        for c in range(k):
            sl = px[pos:pos + int(size[c])].numpy()
            out[n, c] = np.add.accumulate(f[:, sl], axis=-1, dtype=np.float32)[:, -1] / np.float32(int(size[c]))
            pos += int(size[c])
    return torch.from_numpy(out)


# ---- the bilinear scorer ----
def bilinear64(sub, obj, R):
    """sub / obj [B, N, R C] -> (pred [B, R, N, N], A = sum_c |s| |o|) in float64, by the heads' own reshape + permute +
    einsum"""
    B, N, RC = sub.shape
    C = RC // R
    s4 = sub.double().reshape(B, N, R, C).permute(0, 2, 1, 3)
    o4 = obj.double().reshape(B, N, R, C).permute(0, 2, 1, 3)
    return torch.einsum('nrsc,nroc->nrso', s4, o4), torch.einsum('nrsc,nroc->nrso', s4.abs(), o4.abs())


def bilinear_bound(A, C):
    return (C + 2) * U * A


def make_bilinear(family, B, N, R, C, seed=0):
    """(sub, obj) [B, N, R C] fp32 on the CPU"""
    g = _gen(1000003 * seed + 7919 * N + 131 * C + 17 * R + B)
    if family == "exact":
        assert 64 * C < 2 ** 24
        return (torch.randint(-8, 9, (B, N, R * C), generator=g).float(),
                torch.randint(-8, 9, (B, N, R * C), generator=g).float())
    assert family == "spread", family
    sub = torch.randn(B, N, R * C, generator=g) * torch.logspace(-6, 3, N)[None, :, None]
    obj = torch.randn(B, N, R * C, generator=g) * torch.exp2(torch.randint(-6, 6, (B, N, 1), generator=g).float())
    return sub, obj


def bilinear_fp32_model(sub, obj, R, guard=True, skip=None):
    """fp32 model of the scorer: per (b, r) the chain of `fp32_chain` over c.  guard = False (a mutant): the chain runs
    over C padded to a multiple of 32 without the c < C test, so relation r reads the first columns of relation r + 1 (the
    last relation reads zeros).  skip: (b, r, s, o, c) of one product left out (a mutant)."""
    B, N, RC = sub.shape
    C = RC // R
    Cp = C if guard else -(-C // 32) * 32
    pad = torch.zeros(B, N, Cp, dtype=sub.dtype)
    sp, op = torch.cat([sub, pad], -1), torch.cat([obj, pad], -1)
    out = torch.zeros(B, R, N, N, dtype=torch.float32)
    for b in range(B):
        for r in range(R):
            mask = None
            if skip is not None and skip[:2] == (b, r):
                mask = np.zeros((N, N, Cp), dtype=bool)
                mask[skip[2], skip[3], skip[4]] = True
            out[b, r] = fp32_chain(sp[b, :, r * C:r * C + Cp], op[b, :, r * C:r * C + Cp], skip=mask)
    return out
