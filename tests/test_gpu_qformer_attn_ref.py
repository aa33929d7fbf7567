"""The 16-bit Q-Former attention kernels against float64 (`-m gpu`): the two matrix-core cross-attention generations
(psg_xattn_mfma.hip, psg_xattn_dma.hip, shared blocks in psg_xattn_tile.h) and the scalar checker, the matrix-core and
scalar self-attention (psg_selfattn_mfma.hip, psg_attn.hip) and the cls-row kernels of the selection phase, each compared
with the restatements of tests/qformer_attn_ref.py under the bound derived there (u |ref| + u A + 2e-5), at the key
counts, row tilings, pair lists, masks and score shapes where such kernels go wrong.  Every output buffer is filled with
a sentinel and has spare rows: what a call must not write is asserted bit-unchanged."""
import math

import pytest
import torch

from tests.qformer_attn_ref import (U, attn_bound, cls_input64, cls_input_bound, pack_bits, pair_masks, selfattn64,
                                    xattn64)
from tests.rowops_ref_common import _check, _sentinel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEADS, HID = 12, 768
DTYPES = [torch.bfloat16, torch.float16]
VARIANTS = ("simple", "mfma_v1", "mfma")
WORST = {}


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _unchanged(buf, pristine, lo, hi=None):
    assert torch.equal(buf[lo:hi].view(torch.int16 if buf.element_size() == 2 else torch.int32),
                       pristine[lo:hi].view(torch.int16 if buf.element_size() == 2 else torch.int32)), \
        f"rows [{lo}, {hi}) of the output buffer were written"


# ---- cross-attention ----
def _objects(L, g):
    """Nine object masks over L keys: 0 nothing (pair (0, 0) is the empty union), 1 every key, 2 only key 0, 3 only key
    L - 1 (the last, partial key tile), 4 / 5 only keys in [32, 64) / [64, 96) (the two halves of a 64-bit table word),
    6 three keys of ONE key tile (the pair-tile path skips the others), 7 / 8 random at 15 % / 3 %."""
    NT = (L + 31) // 32
    om = torch.zeros(9, L, dtype=torch.bool)
    om[1] = True
    om[2, 0] = True
    om[3, L - 1] = True
    om[4, 32:64] = True
    om[5, 64:96] = True
    t6 = max(NT - 2, 0) * 32
    om[6, [min(t6 + 3, L - 1), min(t6 + 17, L - 1), min(t6 + 30, L - 1)]] = True
    om[7] = torch.rand(L, generator=g) < 0.15
    om[8] = torch.rand(L, generator=g) < 0.03
    return om


# (i, j): the empty union, every single-object mask alone, (i, j) with i != j in both orders, one pair twice
PAIRS = [(0, 0), (0, 1), (0, 2), (2, 0), (0, 3), (3, 3), (0, 4), (4, 4), (5, 0), (5, 5), (4, 5), (6, 6), (0, 6), (7, 8),
         (8, 7), (7, 7), (7, 7), (2, 3), (3, 2), (1, 7), (8, 8), (6, 2)]


def _pair_list(P, N, g, pairs=PAIRS):
    """P pair ids: a shuffled subset of N * N that holds `pairs` first (cycled when P is larger)"""
    ids = [i * N + j for i, j in pairs]
    rest = [p for p in torch.randperm(N * N, generator=g).tolist() if p not in ids]
    ids = (ids + rest) if P > len(ids) else ids
    ids = [ids[n % len(ids)] for n in range(P)]
    order = torch.randperm(P, generator=g).tolist()
    return torch.tensor([ids[n] for n in order], dtype=torch.int32)


def _legacy_rows(empty_pairs, nq, name, policy):
    """rows that get the 2^-10 A term: an empty union under "unmasked" where the path adds the legacy constant in fp32 -
    the scalar kernel, and the generic row tiles of the matrix-core kernels (cls rows at nq == 33, every row otherwise)"""
    if policy != "unmasked":
        return None
    rows = empty_pairs.repeat_interleave(nq)
    if name != "simple" and nq == 33:
        rows = rows & (torch.arange(rows.numel()) % 33 == 0)
    return rows


def _run_xattn(tag, q, k, v, om, pair_index, nq, dtype, policies=("uniform", "unmasked"), variants=VARIANTS,
               indexed=None, refuse=(), refs=None):
    """q / k / v: CPU tensors of `dtype`.  Every policy x variant (and the indexed entry, given (q_u, q_index)) against
    one float64 reference per policy (kept in `refs` when the caller runs the same inputs again); variants in `refuse`
    must raise instead."""
    from openpsg_amd import _lib, ops
    code = {"simple": _lib.PSG_XATTN_SIMPLE, "mfma_v1": _lib.PSG_XATTN_MFMA_V1, "mfma": _lib.PSG_XATTN_MFMA}
    N, P, rows = om.shape[0], pair_index.numel(), pair_index.numel() * nq
    pm = pair_masks(om, pair_index, N)
    empty = ~pm.any(-1)
    bits = pack_bits(om).to(DEV)
    qd, kd, vd, pi = q.to(DEV), k.to(DEV), v.to(DEV), pair_index.to(DEV)
    worst, refs = {}, ({} if refs is None else refs)
    for policy in policies:
        pol = _lib.PSG_EMPTY_UNIFORM if policy == "uniform" else _lib.PSG_EMPTY_UNMASKED
        if policy not in refs:
            refs[policy] = xattn64(q, k, v, pm, HEADS, nq, policy)
        ref, A = refs[policy]
        for name in variants + (("indexed",) if indexed is not None else ()):
            buf, pristine = _sentinel(rows, HID, dtype, DEV)
            if name in refuse:
                with pytest.raises(_lib.PsgHipError):
                    ops.qformer_cross_attn(qd, kd, vd, bits, pi, N, nq, HEADS, out=buf[:rows], empty_policy=pol,
                                           variant=code[name])
                torch.cuda.synchronize()
                _unchanged(buf, pristine, 0)
                continue
            if name == "indexed":
                q_u, q_index = indexed
                q_cls = q_u.view(-1, 33, HID)[q_index.long(), 0].contiguous()
                got = ops.qformer_cross_attn_indexed(q_u.to(DEV), q_index.to(DEV), q_cls.to(DEV), kd, vd, bits, pi, N, HEADS,
                                                     out=buf[:rows], empty_policy=pol)
                if k.shape[0] > 320:                               # the LDS-DMA image does not fit: the entry says so
                    assert got is None
                    torch.cuda.synchronize()
                    _unchanged(buf, pristine, 0)
                    continue
                assert got is not None
            else:
                ops.qformer_cross_attn(qd, kd, vd, bits, pi, N, nq, HEADS, out=buf[:rows], empty_policy=pol,
                                       variant=code[name])
            torch.cuda.synchronize()
            _unchanged(buf, pristine, rows)
            # the indexed entry runs the LDS-DMA kernel ("mfma") with other query addresses: same row tiles, same terms
            bound = attn_bound(ref, A, dtype, _legacy_rows(empty, nq, "mfma" if name == "indexed" else name, policy))
            r = _check(f"{tag} {policy} {name}", buf[:rows].cpu(), ref, bound)
            worst[name] = max(worst.get(name, 0.0), r)
            _note(f"xattn_{name}", r)
    print(f"{tag}: P={P} worst err / bound " + " ".join(f"{n} {r:.3f}" for n, r in worst.items()))


def _indexed_q(P, dtype, g, scale=1.5):
    """33 query rows per PROMPT, U = 3 < P prompts, an index that repeats -> (q_u, q_index, expanded q)"""
    q_u = (torch.randn(3 * 33, HID, generator=g) * scale).to(dtype)
    q_index = ((torch.arange(P) * 7 + 1) % 3).to(torch.int32)
    return q_u, q_index, q_u.view(3, 33, HID)[q_index.long()].reshape(P * 33, HID).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("L", [1, 31, 32, 33, 40, 64, 65, 128, 129, 256, 257, 320, 352, 512, 576])
def test_cross_attn_key_count_edges(L, dtype):
    """Every mask and pair-list case of _objects / PAIRS at each key count: whole and partial key tiles, one to four
    128-key chunks, L = 352 (the LDS-DMA image no longer fits: the first generation, three chunks), 512 (four chunks)
    and 576 (scalar kernel only: the matrix-core variants refuse)."""
    g = torch.Generator().manual_seed(1000 + L)
    om = _objects(L, g)
    pair_index = _pair_list(len(PAIRS), 9, g)
    q_u, q_index, q = _indexed_q(len(PAIRS), dtype, g)
    k = (torch.randn(L, HID, generator=g) * 1.5).to(dtype)
    v = torch.randn(L, HID, generator=g).to(dtype)
    _run_xattn(f"L={L}", q, k, v, om, pair_index, 33, dtype, indexed=(q_u, q_index),
               refuse=("mfma_v1", "mfma") if L > 512 else ())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("nq,P", [(33, 1), (33, 32), (33, 33), (33, 65), (1, 45), (16, 5), (32, 3), (34, 3), (40, 3)])
def test_cross_attn_row_tiling(nq, P, dtype):
    """nq == 33: the boundaries of the 32-pair cls tiles; other nq: flat 32-row tiles whose last one is partial and which
    span two pairs (nq = 32 cannot: every P gives whole tiles).  L = 72: two whole key tiles and 8 keys of a third."""
    g = torch.Generator().manual_seed(2000 + nq * 100 + P)
    L = 72
    om = _objects(L, g)
    pair_index = _pair_list(P, 9, g)
    q = (torch.randn(P * nq, HID, generator=g) * 1.5).to(dtype)
    k = (torch.randn(L, HID, generator=g) * 1.5).to(dtype)
    v = torch.randn(L, HID, generator=g).to(dtype)
    _run_xattn(f"nq={nq} P={P}", q, k, v, om, pair_index, nq, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_cross_attn_ascending_maximum(dtype):
    """Input scale 4 (near one-hot rows) with the keys of tile t scaled by 1.5^t: the running maximum of the online
    softmax moves at nearly every key tile, so what was accumulated must be rescaled (alpha)."""
    g = torch.Generator().manual_seed(3000)
    L, P = 160, len(PAIRS)
    om = _objects(L, g)
    pair_index = _pair_list(P, 9, g)
    q_u, q_index, q = _indexed_q(P, dtype, g, scale=4.0)
    k = (torch.randn(L, HID, generator=g) * 4.0 * (1.5 ** (torch.arange(L) // 32).float())[:, None]).to(dtype)
    v = torch.randn(L, HID, generator=g).to(dtype)
    s = torch.einsum("qhd,lhd->qhl", q.double().view(-1, HEADS, 64), k.double().view(L, HEADS, 64)).view(-1, HEADS, 5, 32)
    tmax = s.max(-1).values
    frac = (tmax[..., 1:] > tmax[..., :-1]).all(-1).double().mean().item()
    assert frac > 0.5, frac                                        # the case is what it says: most rows ascend at EVERY tile
    _run_xattn("ascending", q, k, v, om, pair_index, 33, dtype, indexed=(q_u, q_index))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("nq", [33, 16])
def test_cross_attn_adversarial_mask(nq, dtype):
    """The MASKED keys carry the largest raw scores (|q . k| ~ 3000, every third key, key 0 and key L - 1 among them);
    the attended ones score as at scale 1.5.  A mask bit read wrong, or a bias too small to absorb, owns the row."""
    g = torch.Generator().manual_seed(4000 + nq)
    L, N = 160, 5
    hot = torch.arange(L) % 3 == 0
    om = (torch.rand(N, L, generator=g) < 0.3) & ~hot
    om[1] = False
    om[1, 65:96] = ~hot[65:96]                                     # one attended key tile: the hot keys of the others are skipped
    pair_index = _pair_list(N * N, N, g, pairs=[(1, 1), (2, 3), (3, 2)])
    P = N * N
    e = torch.full((64,), 55.0 / 8.0).repeat(HEADS)                # |e_h| = 55 per head
    q = (torch.randn(P * nq, HID, generator=g) * 1.5 + e).to(dtype)
    kc = torch.randn(L, HEADS, 64, generator=g) * 1.5
    kc = (kc - kc.mean(-1, keepdim=True)).reshape(L, HID)          # attended keys: no component along e
    k = torch.where(hot[:, None], kc + e, kc).to(dtype)
    v = torch.randn(L, HID, generator=g).to(dtype)
    raw = (q.double().view(-1, HEADS, 64)[:8, :, None, :] * k.double().view(L, HEADS, 64).permute(1, 0, 2)[None]).sum(-1)
    assert om.any(-1).all() and raw[..., hot].min() > 2000 and raw[..., ~hot].abs().max() < 400
    _run_xattn(f"adversarial nq={nq}", q, k, v, om, pair_index, nq, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_cross_attn_probability_rounding_edge(dtype):
    """Every key but key 0 gets a score whose UNNORMALISED probability exp(s - max) = (1 + 0.98 * 2u) / 2 sits just below
    a value of the storage type: rounded to nearest it moves by 1 % of a spacing, truncated by 98 %; V > 0, so nothing
    cancels (tests/test_qformer_attn_ref_cpu.py shows on the CPU that a truncating pack fails this case).  The score is
    k[0] + k[1] / 128 per head: a 16-bit head and its correction, both exact products."""
    g = torch.Generator().manual_seed(5000)
    L, N = 96, 2
    target = math.log(0.5 * (1 + 0.98 * 2 * U[dtype]))
    q = torch.zeros(4 * 33, HEADS, 64)
    q[..., 0], q[..., 1] = 8.0, 2.0 ** -4
    k = torch.zeros(L, HEADS, 64)
    k0 = torch.tensor(target).to(dtype).float()
    k[1:, :, 0] = k0
    k[1:, :, 1] = ((target - k0.double()) * 128.0).float()
    v = torch.rand(L, HID, generator=g) + 0.5
    om = torch.ones(N, L, dtype=torch.bool)
    _run_xattn("rounding edge", q.view(-1, HID).to(dtype), k.view(L, HID).to(dtype), v.to(dtype), om,
               torch.arange(4, dtype=torch.int32), 33, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_cross_attn_options_vs_fp64(dtype):
    """900 pairs of 33 rows (929 row tiles: enough for the LDS-DMA kernel to deal its tiles dynamically and to choose ten
    waves by itself) under the default options, xattn_waves 0 and 10 and xattn_dynamic 0 - each against float64."""
    from openpsg_amd import _lib
    g = torch.Generator().manual_seed(6000)
    L, N = 64, 30
    om = torch.rand(N, L, generator=g) < 0.1
    om[0] = False
    om[N - 1] = False
    pair_index = torch.randperm(N * N, generator=g).to(torch.int32)
    q = (torch.randn(N * N * 33, HID, generator=g) * 1.5).to(dtype)
    k = (torch.randn(L, HID, generator=g) * 1.5).to(dtype)
    v = torch.randn(L, HID, generator=g).to(dtype)
    saved = {n: _lib.get_option(0, n) for n in ("xattn_waves", "xattn_dynamic")}
    refs = {}
    try:
        for setting in ({}, {"xattn_waves": 0}, {"xattn_waves": 10}, {"xattn_dynamic": 0}):
            for n in saved:
                _lib.set_option(0, n, setting.get(n, saved[n]))
            _run_xattn(f"options {setting}", q, k, v, om, pair_index, 33, dtype,
                       policies=("uniform",) if setting else ("uniform", "unmasked"), variants=("mfma",), refs=refs)
    finally:
        for n in saved:
            _lib.set_option(0, n, saved[n])


# ---- self-attention ----
def _self_inputs(B, T, nq, heads, dtype, g):
    qkv = (torch.randn(B * (nq + T), 3 * heads * 64, generator=g) * 1.2).to(dtype)
    tm = (torch.rand(B, max(T, 1), generator=g) < 0.8).to(torch.uint8)[:, :T]
    if T:
        tm[:, 0] = 1
        tm[0] = 0                                                  # pair 0: the whole prompt is masked
        tm[1] = 0
        tm[1, 0] = 1                                               # pair 1: only token 0 is valid
    return qkv, tm.contiguous()


MFMA_CASES = [(33, 0), (33, 1), (33, 14), (33, 31), (32, 32), (40, 24), (64, 0)]
SCALAR_ONLY = [(1, 14), (16, 14), (31, 14), (31, 0)]               # nq < 32: the scalar kernel by dispatch


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("nq,T", MFMA_CASES + SCALAR_ONLY)
def test_self_attn_vs_fp64(nq, T, dtype):
    """psg_qformer_self_attn, every row (query_rows_only 0) and the query rows only (1: the text rows of `out` keep the
    sentinel), on the matrix-core kernel and, under option selfattn_scalar (or for nq < 32), on the scalar one."""
    from openpsg_amd import _lib, ops
    g = torch.Generator().manual_seed(7000 + nq * 100 + T)
    B = 5
    qkv, tm = _self_inputs(B, T, nq, HEADS, dtype, g)
    R = B * (nq + T)
    ref, A = selfattn64(qkv, tm, B, T, nq, HEADS, "all")
    bound = attn_bound(ref, A, dtype)
    qd, td = qkv.to(DEV), tm.to(DEV)
    saved = _lib.get_option(0, "selfattn_scalar")
    worst = {}
    try:
        for scalar in ((1,) if nq < 32 else (0, 1)):               # nq < 32: one kernel whatever the option says
            _lib.set_option(0, "selfattn_scalar", scalar)
            fam = "selfattn_scalar" if scalar or nq < 32 else "selfattn_mfma"
            for q_only in (0, 1):
                buf, pristine = _sentinel(R, HID, dtype, DEV)
                ops.qformer_self_attn(qd, td, B, T, nq, HEADS, bool(q_only), buf[:R])
                torch.cuda.synchronize()
                n = B * nq if q_only else R
                _unchanged(buf, pristine, n)
                r = _check(f"self_attn nq={nq} T={T} {fam} q_only={q_only}", buf[:n].cpu(), ref[:n], bound[:n])
                worst[fam] = max(worst.get(fam, 0.0), r)
                _note(fam, r)
    finally:
        _lib.set_option(0, "selfattn_scalar", saved)
    print(f"self_attn nq={nq} T={T}: worst err / bound {worst}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("T", [14, 0])
def test_self_attn_shared_vs_fp64(T, dtype):
    """psg_qformer_self_attn_shared: ONE [nq, 3 hidden] block of query rows for every pair, against float64 on the qkv
    matrix that repeats it"""
    from openpsg_amd import ops
    g = torch.Generator().manual_seed(8000 + T)
    B, nq = 5, 33
    qkv, tm = _self_inputs(B, T, nq, HEADS, dtype, g)
    qkv_q, qkv_t = qkv[:nq].contiguous(), qkv[B * nq:].contiguous()
    full = torch.cat([qkv_q.repeat(B, 1), qkv_t])
    R = B * (nq + T)
    ref, A = selfattn64(full, tm, B, T, nq, HEADS, "all")
    buf, pristine = _sentinel(R, HID, dtype, DEV)
    ops.qformer_self_attn_shared(qkv_q.to(DEV), qkv_t.to(DEV), tm.to(DEV), B, T, nq, HEADS, buf[:R])
    torch.cuda.synchronize()
    _unchanged(buf, pristine, R)
    r = _check(f"self_attn_shared T={T}", buf[:R].cpu(), ref, attn_bound(ref, A, dtype))
    _note("selfattn_shared", r)
    print(f"self_attn_shared T={T}: worst err / bound {r:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_self_attn_cls_row_mode_is_compact_for_every_dtype(dtype):
    """query_rows_only == 2 through the ABI: out[p] = the cls row of pair p and NOTHING else is written, in bf16 / fp16 as
    in fp32.  The buffer is full-size, so a kernel that wrote the full layout instead would stay inside it (and fail
    here); other values of the argument are rejected."""
    from openpsg_amd import _lib
    g = torch.Generator().manual_seed(9000)
    B, nq, T = 5, 33, 14
    qkv, tm = _self_inputs(B, T, nq, HEADS, dtype, g)
    R = B * (nq + T)
    ref, A = selfattn64(qkv, tm, B, T, nq, HEADS, "cls")
    lib, ctx = _lib.load(), _lib.ctx(0)
    qd, td = qkv.to(DEV), tm.to(DEV)
    buf, pristine = _sentinel(R, HID, dtype, DEV)
    code = {torch.bfloat16: _lib.PSG_BF16, torch.float16: _lib.PSG_F16}[dtype]
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.psg_qformer_self_attn(ctx, qd.data_ptr(), td.data_ptr(), B, T, nq, HEADS, 2, buf.data_ptr(), code, st),
               "psg_qformer_self_attn")
    torch.cuda.synchronize()
    _unchanged(buf, pristine, B)
    r = _check("self_attn mode 2", buf[:B].cpu(), ref, attn_bound(ref, A, dtype))
    _note("selfattn_mode2", r)
    for bad in (3, -1):
        assert lib.psg_qformer_self_attn(ctx, qd.data_ptr(), td.data_ptr(), B, T, nq, HEADS, bad, buf.data_ptr(), code,
                                         st) == -1                 # PSG_ERR_INVALID
    torch.cuda.synchronize()
    _unchanged(buf, pristine, B)
    print(f"self_attn mode 2: worst err / bound {r:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", [12, 16, 17])
@pytest.mark.parametrize("T", [0, 14, 31])
def test_self_attn_cls_vs_fp64(T, heads, dtype):
    """psg_qformer_self_attn_cls (compact cls rows from q_cls and K | V): the one-wave-per-pair kernel at 12 heads and at
    16 (hidden 1024: every lane owns features), the scalar kernel with q_cls at 17 (hidden > 1024); B = 5 and 6 pairs
    (not a multiple of the four waves of a block), pair 0 fully masked."""
    from openpsg_amd import _lib
    lib, ctx = _lib.load(), _lib.ctx(0)
    nq, H = 33, heads * 64
    code = {torch.bfloat16: _lib.PSG_BF16, torch.float16: _lib.PSG_F16}[dtype]
    for B in (5, 6):
        g = torch.Generator().manual_seed(10000 + T * 100 + heads * 10 + B)
        qkv, tm = _self_inputs(B, T, nq, heads, dtype, g)
        q_cls = qkv[0:B * nq:nq, :H].contiguous()
        kv = qkv[:, H:].contiguous()
        ref, A = selfattn64((q_cls, kv), tm, B, T, nq, heads, "cls")
        buf, pristine = _sentinel(B, H, dtype, DEV)
        qd, kd, td = q_cls.to(DEV), kv.to(DEV), tm.to(DEV)
        _lib.check(lib.psg_qformer_self_attn_cls(ctx, qd.data_ptr(), kd.data_ptr(), td.data_ptr(), B, T, nq, heads,
                                                 buf.data_ptr(), code, torch.cuda.current_stream().cuda_stream),
                   "psg_qformer_self_attn_cls")
        torch.cuda.synchronize()
        _unchanged(buf, pristine, B)
        r = _check(f"self_attn_cls T={T} heads={heads} B={B}", buf[:B].cpu(), ref, attn_bound(ref, A, dtype))
        _note("selfattn_cls" if heads <= 16 else "selfattn_cls_fallback", r)
        print(f"self_attn_cls T={T} heads={heads} B={B}: worst err / bound {r:.3f}")


CLS_IN = ([(dt, T) for dt in DTYPES for T in (0, 14, 15, 31)]
          + [(torch.float32, T) for T in (0, 15, 16, 19)])             # fp32: S = 48, 49 and 52, the last that fits the LDS


@pytest.mark.parametrize("shared", [False, True], ids=["per_pair", "shared_text"])
@pytest.mark.parametrize("dtype,T", CLS_IN, ids=[f"{str(d)[6:]}-T{T}" for d, T in CLS_IN])
def test_cls_attn_input_vs_fp64(dtype, T, shared):
    """psg_qformer_cls_attn_input with per-pair text rows, and with x_text / text_index sharing U = 3 text blocks (and
    their mask rows) among B = 7 pairs."""
    from openpsg_amd import _lib
    lib, ctx = _lib.load(), _lib.ctx(0)
    g = torch.Generator().manual_seed(11000 + T * 10 + shared)
    B, nq, Ub = 7, 33, 3 if shared else 7
    xq = (torch.randn(B * nq, HID, generator=g) * 0.7).to(dtype)
    xt = (torch.randn(Ub * T, HID, generator=g) * 0.7).to(dtype)
    gg = (torch.randn(HEADS, B, HID, generator=g) * 0.3).float()
    tm = (torch.rand(Ub, max(T, 1), generator=g) < 0.7).to(torch.uint8)[:, :T].contiguous()
    if T:
        tm[0] = 0                                                  # a text block that is all padding
        tm[1, 0] = 1
    ti = torch.tensor([2, 0, 1, 1, 2, 0, 2], dtype=torch.int32) if shared else None
    ref, A, gx = cls_input64(xq, xt, ti, gg, tm, B, T, nq, with_gx=True)
    x = xq if shared else torch.cat([xq, xt])
    xd = x.to(DEV)
    xtd = xt.to(DEV) if shared else xd[B * nq:]
    buf, pristine = _sentinel(HEADS * B, HID, torch.float32, DEV)
    code = {torch.bfloat16: _lib.PSG_BF16, torch.float16: _lib.PSG_F16, torch.float32: _lib.PSG_F32}[dtype]
    tid, gd, td = (ti.to(DEV) if shared else None), gg.to(DEV), tm.to(DEV)
    _lib.check(lib.psg_qformer_cls_attn_input(ctx, xd.data_ptr(), xtd.data_ptr() if T else None,
                                              tid.data_ptr() if shared else None, gd.data_ptr(), td.data_ptr() if T else None,
                                              B, T, nq, HEADS, HID, buf.data_ptr(), code,
                                              torch.cuda.current_stream().cuda_stream), "psg_qformer_cls_attn_input")
    torch.cuda.synchronize()
    _unchanged(buf, pristine, HEADS * B)
    r = _check(f"cls_attn_input {dtype} T={T} shared={shared}", buf[:HEADS * B].cpu().view(HEADS, B, HID), ref,
               cls_input_bound(A, gx, dtype))
    _note("cls_attn_input_f32" if dtype == torch.float32 else "cls_attn_input", r)
    print(f"cls_attn_input {dtype} T={T} shared={shared}: worst err / bound {r:.3f}")


def test_cls_attn_input_refuses_rows_beyond_the_lds():
    """fp32 rows of 3072 bytes beside the 3072-byte probability table: 52 rows are the last that fit 160 KiB"""
    from openpsg_amd import _lib, ops
    B, nq, T = 2, 33, 20
    x = torch.zeros(B * (nq + T), HID, device=DEV)
    gg = torch.zeros(HEADS, B, HID, device=DEV)
    tm = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.PsgHipError):
        ops.qformer_cls_attn_input(x, gg, tm, B, T, nq, HEADS)
