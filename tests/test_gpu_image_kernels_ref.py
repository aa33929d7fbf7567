"""The image-side fp32 kernels against float64 references (`-m gpu`): psg_patch_embed, psg_masked_mean_pool,
psg_masked_split_mean_pool, psg_bilinear_scores and psg_qformer_embed - the anchor of these kernels; the max-norm checks
of tests/test_gpu_parity.py at the workload's shapes stay as they are.

References, the two input families and every bound come from tests/image_ref.py (derived there, checked on the CPU by
tests/test_image_ref_cpu.py); no figure here comes from the kernels' output.  Exact family: integers, so the fp32 result
must equal the integer result bit for bit, whatever the accumulation order.  Spread family: row scales over 9 decades /
a +1000 offset, held per element to the derived bound.  Shapes are the smallest that reach each edge of the kernels: the
index pass's partial block of 1024, pixel counts at the 64 / 256 / 2048 boundaries of the partial pass, the slot chain
on 40 random geometries (read back as ordered pixel lists), K splits of unequal channel counts, Cout / 128 of 1, 3 and 8,
feature maps that are no multiple of the patch, tiles of 32 with one row more or less.  Every output buffer is longer
than the result and sentinel-filled; every refusal the kernels document is tried.

Measured on an MI355X (256 CUs), worst err / bound per kernel; every exact-family case is bit-equal, the pools' division
included (the quotient is correctly rounded, no mismatch of even one ulp):
  patch_embed              0.011 of the primary bound, 0.174 of 2^-20 A (L = 129; the outputs that sit near 1 / 16 of
                           2^-20 A are those of the smallest row scales, where the bias is the result and its one
                           rounding u |ref| = u A is the whole error); splits: C = 33 -> 17 of 2, C = 257 -> 86 of 3
  masked_mean_pool         0.041
  masked_split_mean_pool   0.231 (k = 64)
  bilinear_scores          0.462 (N = 65; C = 1 is a single rounding of (C + 2) u A = 3 u A)
  qformer_embed            fp32 0.398, bf16 0.4999, fp16 0.4997 (a 16-bit output is half a unit in the last place)
  pool slot chain          40 of 40 geometries identical pixel lists: 39 maps with HW % 1024 != 0, 15 below 1024 pixels,
                           106 empty objects, 15 maps where a padded id map would alias id 0
"""
import ctypes

import pytest
import torch

from tests import image_ref as R
from tests.rowops_ref_common import _check, _sentinel

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _env():
    from openpsg_amd import _lib
    return _lib.load(), _lib.ctx(0), torch.cuda.current_stream().cuda_stream


def _tail_intact(buf, pristine, used):
    return torch.equal(buf.reshape(-1)[used:], pristine.reshape(-1)[used:])


# ---- the C ABI with a caller-owned output (the ops wrappers allocate theirs) ----
def _patch_embed_into(feat, w, b, out):
    """-> workspace bytes"""
    from openpsg_amd._lib import check
    lib, ctx, st = _env()
    _, C, Hf, Wf = feat.shape
    Cout = w.shape[0]
    nbytes = ctypes.c_int64(0)
    check(lib.psg_patch_embed_workspace(ctx, C, Hf, Wf, Cout, 16, ctypes.byref(nbytes)), "psg_patch_embed_workspace")
    ws = torch.empty(nbytes.value // 4, device=feat.device, dtype=torch.float32)
    check(lib.psg_patch_embed(ctx, feat.data_ptr(), C, Hf, Wf, w.data_ptr(), b.data_ptr(), Cout, 16, out.data_ptr(),
                              ws.data_ptr(), nbytes.value, st), "psg_patch_embed")
    return nbytes.value


def _pool_into(feat, pan, img, pad, ids, out, output_size=None):
    from openpsg_amd._lib import check
    lib, ctx, st = _env()
    _, C, Hf, Wf = feat.shape
    N = ids.numel()
    nbytes = ctypes.c_int64(0)
    check(lib.psg_masked_mean_pool_workspace(ctx, C, Hf, Wf, N, ctypes.byref(nbytes)), "psg_masked_mean_pool_workspace")
    ws = torch.empty(nbytes.value // 4, device=feat.device, dtype=torch.int32)
    head = (ctx, feat.data_ptr(), C, Hf, Wf, pan.data_ptr(), pan.shape[0], pan.shape[1], int(img[0]), int(img[1]),
            int(pad[0]), int(pad[1]), ids.data_ptr(), N)
    if output_size is None:
        check(lib.psg_masked_mean_pool(*head, out.data_ptr(), ws.data_ptr(), nbytes.value, st), "psg_masked_mean_pool")
    else:
        check(lib.psg_masked_split_mean_pool(*head, int(output_size), out.data_ptr(), ws.data_ptr(), nbytes.value, st),
              "psg_masked_split_mean_pool")


def _bilinear_into(sub, obj, R_, pred):
    from openpsg_amd._lib import check
    lib, ctx, st = _env()
    B, N, RC = sub.shape
    check(lib.psg_bilinear_scores(ctx, sub.data_ptr(), obj.data_ptr(), B, N, R_, RC // R_, pred.data_ptr(), st),
          "psg_bilinear_scores")


def _embed_into(ids, B, T, word, pos, query, nq, gamma, beta, eps, hidden, out):
    from openpsg_amd import ops
    from openpsg_amd._lib import check
    lib, ctx, st = _env()
    check(lib.psg_qformer_embed(ctx, ids.data_ptr() if T else None, B, T, word.data_ptr(), pos.data_ptr(),
                                query.data_ptr(), nq, gamma.data_ptr(), beta.data_ptr(), float(eps), hidden,
                                out.data_ptr(), ops._dt(out), st), "psg_qformer_embed")


# ---- patch embed ----
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", R.PE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_patch_embed_vs_float64(shape, family):
    """psg_patch_embed against unfold + matmul in float64.  Feature rows >= 16 gh and columns >= 16 gw are NaN (they
    belong to no patch), the output buffer is longer than L rows, the split count comes from the workspace size."""
    from openpsg_amd import ops
    dev = _dev()
    C, Hf, Wf, Cout = shape
    gh, gw = Hf // 16, Wf // 16
    L = gh * gw
    feat, w, b = R.make_patch_embed(family, C, Hf, Wf, Cout)
    feat[:, :, 16 * gh:] = float("nan")
    feat[:, :, :, 16 * gw:] = float("nan")
    feat, w, b = feat.to(dev), w.to(dev), b.to(dev)
    buf, pristine = _sentinel(L, Cout, torch.float32, dev)
    S = R.pe_splits(_patch_embed_into(feat, w, b, buf[:L]), L, Cout)
    torch.cuda.synchronize()
    assert _tail_intact(buf, pristine, L * Cout), "rows past the end of the output were written"
    assert 1 <= S <= C
    if shape in R.PE_UNEVEN:
        assert C % -(-C // S) != 0, f"C={C} S={S}: the K splits own equal channel counts on this device"
    got = buf[:L]
    assert bool(torch.isfinite(got).all())
    ref, A = R.patch_embed64(feat, w, b)                               # float64 on the device
    if family == "exact":
        R.assert_exact_range(A)
        assert torch.equal(got, ref.float()), f"{int((got != ref.float()).sum())} of {got.numel()} elements differ"
        line = "bit-exact"
    else:
        r1 = _check(f"patch_embed {shape} primary", got, ref, R.patch_embed_bound(A, C, S))
        r2 = _check(f"patch_embed {shape} 2^-20 A", got, ref, R.bound32(A))
        line = f"err / primary bound {r1:.4f}, err / (2^-20 A) {r2:.4f}"
    again, _ = _sentinel(L, Cout, torch.float32, dev)
    _patch_embed_into(feat, w, b, again[:L])
    assert torch.equal(again[:L], got), "two calls differ"
    assert torch.equal(ops.patch_embed(feat, w, b), got)
    print(f"patch_embed C={C} {Hf}x{Wf} Cout={Cout} L={L} S={S} cps={-(-C // S)} {family}: {line}")


def test_patch_embed_refusals():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    dev = _dev()
    for C, Hf, Wf, Cout, patch in [(2, 32, 32, 128, 8), (2, 32, 32, 192, 16), (2, 32, 18, 128, 16), (2, 8, 32, 128, 16)]:
        feat = torch.randn(1, C, Hf, Wf, device=dev)
        w = torch.randn(Cout, C, patch, patch, device=dev)
        with pytest.raises(PsgHipError):
            ops.patch_embed(feat, w, torch.zeros(Cout, device=dev), patch)


# ---- pools: the slot chain ----
def test_pool_slot_chain_pixel_lists_on_random_geometries():
    """The fp32 nearest -> pad -> nearest index chain of pool_slot and the ordered compaction of pool_index, read back
    as pixel lists through the split pool: C = 4 channels holding (row, col, linear index, 1) and output_size = HW, so
    chunk c of an object of m <= HW pixels is exactly its pixel c mod m.  torch.equal to the reference chain."""
    from oracle import psg_oracle as O
    dev = _dev()
    geos = R.slot_geometries()
    assert len(geos) == 40
    partial = small = empty = alias = 0
    for case, (pan, ids, img, pad, (Hf, Wf)) in enumerate(geos):
        HW = Hf * Wf
        assert HW < 12000
        partial += HW % 1024 != 0
        small += HW < 1024
        lin = torch.arange(HW, dtype=torch.float32)
        feat = torch.stack([(lin // Wf), lin % Wf, lin, torch.ones(HW)]).reshape(1, 4, Hf, Wf)
        masks = R.resample_masks(pan, ids, img, pad, (Hf, Wf))
        want, _, _ = R.split_pool64(feat, masks, HW)
        N = len(ids)
        buf, pristine = _sentinel(N * HW, 4, torch.float32, dev)
        _pool_into(feat.to(dev), pan.to(dev), img, pad, torch.tensor(ids, dtype=torch.int32, device=dev), buf[:N * HW],
                   output_size=HW)
        torch.cuda.synchronize()
        assert _tail_intact(buf, pristine, N * HW * 4), case
        got = buf[:N * HW].reshape(N, HW, 4).cpu()
        assert torch.equal(got, want.float()), (case, tuple(pan.shape), img, pad, (Hf, Wf), ids)
        counts = masks.reshape(N, -1).sum(1)
        empty += int((counts == 0).sum())
        if 0 in ids:                                                    # padding is no object: it never counts as id 0
            n0 = ids.index(0)
            kernel_count = int(got[n0, :, 2].unique().numel()) if got[n0, 0, 3] == 1 else 0
            assert kernel_count == int(counts[n0])
            alias += int((O.mask_grid(pan, img, pad, (Hf, Wf)) == 0).sum()) > int(counts[n0])
    print(f"pool slot chain: {partial} of 40 maps with HW % 1024 != 0, {small} below 1024 pixels, {empty} empty objects, "
          f"{alias} maps where padding would alias id 0")
    assert partial >= 20 and small >= 1 and empty >= 10 and alias >= 3


# ---- pools: the arithmetic at pinned pixel counts ----
_SCENE = {}


def _pinned(dev):
    """the pinned scene, its reference masks and pixel counts - made once, never modified"""
    if not _SCENE:
        pan, ids, counts = R.pinned_pool_scene()
        masks = R.resample_masks(pan, ids, R.POOL_HW, R.POOL_HW, R.POOL_HW)
        assert masks.reshape(len(ids), -1).sum(1).long().tolist() == [counts[i] for i in ids]
        assert set(R.POOL_COUNTS) | {0} <= set(counts.values()) and ids != sorted(ids)
        _SCENE.update(pan=pan.to(dev), ids=ids, ids_t=torch.tensor(ids, dtype=torch.int32, device=dev), masks=masks,
                      counts=torch.tensor([counts[i] for i in ids]))
    return _SCENE


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("C", R.POOL_C)
def test_masked_mean_pool_at_pinned_counts(C, family):
    dev = _dev()
    sc = _pinned(dev)
    N = len(sc["ids"])
    feat = R.make_pool_feat(family, C, *R.POOL_HW)
    ref, mag, counts = R.mean_pool64(feat, sc["masks"])
    assert torch.equal(counts, sc["counts"])
    featd = feat.to(dev)
    buf, pristine = _sentinel(N, C, torch.float32, dev)
    _pool_into(featd, sc["pan"], R.POOL_HW, R.POOL_HW, sc["ids_t"], buf[:N])
    torch.cuda.synchronize()
    assert _tail_intact(buf, pristine, N * C), "rows past the end of the output were written"
    got = buf[:N].cpu()
    if family == "exact":
        R.assert_exact_range(8.0 * counts)
        want = R.exact_quotient(ref)
        assert torch.equal(got, want), f"objects of {counts[(got != want).any(1)].tolist()} pixels differ"
        line = "bit-exact"
    else:
        line = f"err / bound {_check(f'mean pool C={C}', got, ref, R.mean_pool_bound(mag, counts)):.4f}"
    again, _ = _sentinel(N, C, torch.float32, dev)
    _pool_into(featd, sc["pan"], R.POOL_HW, R.POOL_HW, sc["ids_t"], again[:N])
    assert torch.equal(again[:N].cpu(), got), "two calls differ"
    print(f"masked_mean_pool C={C} {family}: {line}")


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("k", R.POOL_KS)
@pytest.mark.parametrize("C", R.POOL_C)
def test_masked_split_mean_pool_at_pinned_counts(C, k, family):
    dev = _dev()
    sc = _pinned(dev)
    N = len(sc["ids"])
    feat = R.make_pool_feat(family, C, *R.POOL_HW)
    ref, mag, sizes = R.split_pool64(feat, sc["masks"], k)
    featd = feat.to(dev)
    buf, pristine = _sentinel(N * k, C, torch.float32, dev)
    _pool_into(featd, sc["pan"], R.POOL_HW, R.POOL_HW, sc["ids_t"], buf[:N * k], output_size=k)
    torch.cuda.synchronize()
    assert _tail_intact(buf, pristine, N * k * C), "rows past the end of the output were written"
    got = buf[:N * k].reshape(N, k, C).cpu()
    if family == "exact":
        want = R.exact_quotient(ref)
        assert torch.equal(got, want), f"objects of {sc['counts'][(got != want).any(2).any(1)].tolist()} pixels differ"
        line = "bit-exact"
    else:
        line = f"err / bound {_check(f'split pool C={C} k={k}', got, ref, R.split_pool_bound(mag, sizes)):.4f}"
    again, _ = _sentinel(N * k, C, torch.float32, dev)
    _pool_into(featd, sc["pan"], R.POOL_HW, R.POOL_HW, sc["ids_t"], again[:N * k], output_size=k)
    assert torch.equal(again[:N * k].reshape(N, k, C).cpu(), got), "two calls differ"
    print(f"masked_split_mean_pool C={C} k={k} {family}: {line}")


def test_pool_refusals():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    dev = _dev()
    sc = _pinned(dev)
    feat6 = torch.zeros(1, 6, *R.POOL_HW, device=dev)
    feat4 = torch.zeros(1, 4, *R.POOL_HW, device=dev)
    with pytest.raises(PsgHipError):
        ops.masked_mean_pool(feat6, sc["pan"], R.POOL_HW, R.POOL_HW, sc["ids_t"])
    with pytest.raises(PsgHipError):
        ops.masked_split_mean_pool(feat6, sc["pan"], R.POOL_HW, R.POOL_HW, sc["ids_t"], 4)
    with pytest.raises(PsgHipError):
        ops.masked_split_mean_pool(feat4, sc["pan"], R.POOL_HW, R.POOL_HW, sc["ids_t"], 0)


# ---- the bilinear scorer ----
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N", R.BIL_N)
def test_bilinear_scores_vs_float64(N, family):
    """psg_bilinear_scores over C in {1, 2, 31, 32, 33, 100} x R in {1, 3} x B in {1, 2}: the 32-wide tiles and the
    32-column chunks with one more and one less.  Relation 1's columns and batch 1's rows are NaN-poisoned in turn:
    every other relation / batch keeps its bits."""
    dev = _dev()
    worst = 0.0
    for C in R.BIL_C:
        for Rr in R.BIL_R:
            for B in R.BIL_B:
                sub, obj = R.make_bilinear(family, B, N, Rr, C)
                ref, A = R.bilinear64(sub, obj, Rr)
                subd, objd = sub.to(dev), obj.to(dev)
                n = B * Rr * N * N
                buf = torch.full((n + 64,), SENTINEL, device=dev)
                _bilinear_into(subd, objd, Rr, buf)
                torch.cuda.synchronize()
                assert bool((buf[n:] == SENTINEL).all()), "pred written past its end"
                got = buf[:n].reshape(B, Rr, N, N).cpu()
                name = f"bilinear B={B} N={N} R={Rr} C={C}"
                if family == "exact":
                    R.assert_exact_range(A)
                    assert torch.equal(got, ref.float()), name
                else:
                    worst = max(worst, _check(name, got, ref, R.bilinear_bound(A, C)))
                poisons = []
                if Rr > 1:
                    poisons.append((slice(None), slice(C, 2 * C), lambda p: torch.cat([p[:, :1], p[:, 2:]], 1)))
                if B > 1:
                    poisons.append((slice(1, 2), slice(None), lambda p: p[:1]))
                for rows, cols, keep in poisons:
                    ps, po = sub.clone(), obj.clone()
                    ps[rows, :, cols] = float("nan")
                    po[rows, :, cols] = float("nan")
                    pbuf = torch.full((n + 64,), SENTINEL, device=dev)
                    _bilinear_into(ps.to(dev), po.to(dev), Rr, pbuf)
                    kept = keep(pbuf[:n].reshape(B, Rr, N, N).cpu())
                    assert bool(torch.isfinite(kept).all()) and torch.equal(kept, keep(got)), name + " poisoned"
    print(f"bilinear_scores N={N} {family}: " + ("bit-exact" if family == "exact" else f"max err / bound {worst:.4f}"))


# ---- the Q-Former embedding ----
@pytest.mark.parametrize("B,T,nq", [(1, 1, 0), (1, 0, 33), (3, 7, 33), (5, 31, 1)])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_qformer_embed_vs_float64(dt, B, T, nq):
    """psg_qformer_embed: LayerNorm(query[r]) for the B nq query rows, then LayerNorm(word[id] + pos[t]) for the B T text
    rows, against `_ln_expect` (x = word[id], res_rows = pos[t], no bias).  Row counts that are no multiple of the 4 rows
    of a workgroup, text only, queries only, the first and the last id of the table, word rows with a +100 offset."""
    from tests.test_gpu_rowops_ref import _ln_expect
    dev, dtype, eps, Hd, V = _dev(), DTYPES[dt], 1e-12, 768, 50
    g = torch.Generator().manual_seed(100 * B + 10 * T + nq)
    word = torch.randn(V, Hd, generator=g)
    word[3::7] += 100.0
    pos = torch.randn(max(T, 1), Hd, generator=g)
    query = torch.randn(max(nq, 1), Hd, generator=g)
    gamma, beta = 1 + 0.5 * torch.randn(Hd, generator=g), torch.randn(Hd, generator=g)
    ids = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    ids.view(-1)[:2] = torch.tensor([V - 1, 0], dtype=torch.int32)[:B * T]
    ids.view(-1)[-1:] = 3                                               # an offset row
    if T == 1:
        ids[0, 0] = V - 1
    word, pos, query, gamma, beta, ids = (t.to(dev) for t in (word, pos, query, gamma, beta, ids))
    rows = B * (nq + T)
    buf, pristine = _sentinel(rows, Hd, dtype, dev)
    _embed_into(ids, B, T, word, pos, query, nq, gamma, beta, eps, Hd, buf[:rows])
    torch.cuda.synchronize()
    assert _tail_intact(buf, pristine, rows * Hd), "rows past the end of the output were written"
    worst = 0.0
    if nq:
        want, bound = _ln_expect(query.repeat(B, 1), None, None, gamma, beta, eps, dtype)
        worst = max(worst, _check(f"embed {dt} query rows", buf[:B * nq], want, bound))
    if T:
        tr = torch.arange(B * T, device=dev)
        want, bound = _ln_expect(word[ids.reshape(-1).long()], pos[tr % T], None, gamma, beta, eps, dtype)
        worst = max(worst, _check(f"embed {dt} text rows", buf[B * nq:rows], want, bound))
    print(f"qformer_embed {dt} B={B} T={T} nq={nq}: max err / bound {worst:.4f}")


def test_qformer_embed_rejects_other_widths():
    from openpsg_amd._lib import PsgHipError
    dev = _dev()
    Hd = 512
    word, pos, query = (torch.randn(8, Hd, device=dev) for _ in range(3))
    gamma, beta = torch.ones(Hd, device=dev), torch.zeros(Hd, device=dev)
    ids = torch.zeros(2, 3, dtype=torch.int32, device=dev)
    buf, pristine = _sentinel(2 * (8 + 3), Hd, torch.float32, dev)
    with pytest.raises(PsgHipError):
        _embed_into(ids, 2, 3, word, pos, query, 8, gamma, beta, 1e-12, Hd, buf)
    torch.cuda.synchronize()
    assert torch.equal(buf, pristine)
