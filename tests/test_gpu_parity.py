"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the C ABI,
against (a) the goldens captured from the real reference head and (b) the CPU oracle on the same
seeded inputs.

Tolerances: integer/bit work is exact; fp32 verification mode: existence logits within 1e-3 of the
reference (north-star bar), greedy tokens identical; bf16 mode: deviation is measured and bounded
separately (it cannot meet an fp32 1e-3 bar by construction, SURVEY 7 'hard parts').
"""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = ["G1_c1_512_n10", "G2_768x1024_n12", "G4_llm_wide_n6", "G5_c5geo_1024x1344_n8", "G6_llm_7b_width_n6"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _head(cfg, w, dtype, **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    h = RelationTransformerHeadV4(dtype=dtype, device="cuda:0", qformer_vocab_size=cfg.qformer.vocab,
                                  llm_config=cfg.llm, llm_feature_size=cfg.llm.hidden, tokenizers="word",
                                  max_object_num=cfg.max_object_num, on_parse_error="skip", **kw)
    h.load_weights(w)
    return h


def _inputs(scene):
    dev = _dev()
    return dict(mask_features=scene["mask_features"].to(dev), img_metas=[scene["img_meta"]],
                object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"].to(dev))])


def test_library_loaded_and_device():
    from openpsg_amd import _lib
    ncu, arch = _lib.device_info(0)
    assert "gfx950" in arch, arch
    assert ncu >= 200


def test_mask_kernels_bit_exact_vs_reference_goldens():
    from openpsg_amd import ops
    g = dict(np.load(H.GOLDEN + "/G3_mask_grid.npz"))
    dev = _dev()
    for k in range(int(g["num_cases"])):
        pan = torch.from_numpy(g[f"g{k}_pan"]).to(dev)
        ori, img, pad = g[f"g{k}_shapes"]
        gh, gw = [int(x) for x in g[f"g{k}_grid_hw"]]
        ids = torch.from_numpy(g[f"g{k}_ids"]).to(dev)
        grid = ops.mask_grid(pan, tuple(img), tuple(pad), (gh, gw))
        bits = ops.object_bitmasks(grid, ids).cpu().numpy().view(np.uint64)
        L = gh * gw
        got = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder="little")[:, :L].astype(bool)
        want = H.unpack_bits(g[f"g{k}_obj_masks_bits"], L).numpy()
        assert np.array_equal(got, want), f"geometry {k}"


@pytest.fixture(scope="module", params=CASES)
def fp32_run(request):
    g, cfg, w, scene = H.load_case(request.param)
    head = _head(cfg, w, "fp32", suppress_eos=bool(g["suppress_eos"]))
    out = head(_inputs(scene))
    torch.cuda.synchronize()
    return g, cfg, w, scene, head, out


def test_fp32_relation_query_vs_reference(fp32_run):
    g, cfg, w, scene, head, out = fp32_run
    last = head.last
    logit = last["exist_logit"].cpu().numpy()
    err = np.abs(logit - g["exist_logit"]).max()
    print(f"max |exist_logit - reference| = {err:.3e}")
    assert err < 1e-3                                             # north-star tolerance
    hid = last["hidden"].float().cpu().view(-1, 33, 768)
    kept = g["kept_pairs"]
    np.testing.assert_allclose(hid[kept].numpy(), g["qformer_out_kept"], atol=1e-3)
    assert last["selected"].cpu().tolist() == g["selected"].tolist()


def test_fp32_llm_decode_vs_reference(fp32_run):
    g, cfg, w, scene, head, out = fp32_run
    toks = head.last["tokens_host"]
    fl = head.last["first_logits"].float().cpu().numpy()
    for i in range(toks.shape[0]):
        want = g["gen_tokens"][i]
        want = want[want >= 0].tolist()
        got = [int(t) for t in toks[i] if t >= 0]
        assert got == want, f"selected pair #{i}: greedy tokens differ from the reference"
        np.testing.assert_allclose(fl[i][g["gen_top8_idx"][i]], g["gen_top8_val"][i], atol=1e-3)


def test_fp32_output_contract(fp32_run):
    g, cfg, w, scene, head, out = fp32_run
    assert set(out) == {"rel_pred", "rel_score"}
    assert len(out["rel_pred"]) == len(out["rel_score"])
    for t in out["rel_pred"]:
        assert len(t) == 3


@pytest.mark.parametrize("case", ["G2_768x1024_n12"])
def test_bf16_mode_deviation_is_bounded(case):
    g, cfg, w, scene = H.load_case(case)
    head = _head(cfg, w, "bf16", suppress_eos=True)
    head(_inputs(scene))
    logit = head.last["exist_logit"].cpu().numpy()
    err = np.abs(logit - g["exist_logit"]).max()
    overlap = len(set(head.last["selected"].cpu().tolist()) & set(g["selected"].tolist()))
    print(f"bf16: max |logit diff| = {err:.3e}, top-20 overlap = {overlap}/20")
    assert err < 0.25 and overlap >= 14


def _xattn_reference(q, k, v, pm, heads):
    """fp32 torch restatement on the GPU of masked cross-attention with the 'uniform' policy."""
    P33, Hd = q.shape
    L = k.shape[0]
    qh = q.float().view(-1, 33, heads, 64).permute(0, 2, 1, 3)
    kh = k.float().view(L, heads, 64).permute(1, 0, 2)
    vh = v.float().view(L, heads, 64).permute(1, 0, 2)
    s = torch.einsum("phqd,hld->phql", qh, kh) * 0.125
    s = s + ((~pm)[:, None, None, :].float() * torch.finfo(torch.float32).min)
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("phql,hld->phqd", p, vh)
    return o.permute(0, 2, 1, 3).reshape(P33, Hd)


@pytest.mark.parametrize("L,N,P", [(64, 5, 25), (192, 7, 49), (256, 12, 144), (336, 9, 81), (40, 3, 9)])
def test_cross_attn_mfma_vs_fp32_reference(L, N, P):
    from openpsg_amd import ops, _lib
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(L * 1000 + N)
    heads = 12
    q = (torch.randn(P * 33, 768, generator=g) * 1.5).to(dev).bfloat16()
    k = (torch.randn(L, 768, generator=g) * 1.5).to(dev).bfloat16()
    v = torch.randn(L, 768, generator=g).to(dev).bfloat16()
    om = torch.rand(N, L, generator=g) < 0.15
    om[0] = False                                                  # object 0 vanished -> pair (0,0) is empty
    if N > 2:
        om[1] = False
    words = (L + 63) // 64
    bits_np = np.zeros((N, words * 64), dtype=np.uint8)
    bits_np[:, :L] = om.numpy()
    bits = torch.from_numpy(np.packbits(bits_np, axis=-1, bitorder="little").view(np.int64).reshape(N, words)).to(dev)
    pair_index = torch.arange(P, dtype=torch.int32, device=dev)
    pm = (om[:, None, :] | om[None, :, :]).reshape(N * N, L)[:P].to(dev)
    ref = _xattn_reference(q, k, v, pm, heads)
    out_m = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, variant=_lib.PSG_XATTN_MFMA)
    out_1 = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, variant=_lib.PSG_XATTN_MFMA_V1)
    out_s = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, variant=_lib.PSG_XATTN_SIMPLE)
    torch.cuda.synchronize()
    e_m = (out_m.float() - ref).abs().max().item()
    e_1 = (out_1.float() - ref).abs().max().item()
    e_s = (out_s.float() - ref).abs().max().item()
    print(f"L={L}: LDS-DMA kernel err {e_m:.3e}, first-generation kernel err {e_1:.3e}, simple err {e_s:.3e}")
    assert e_s < 2e-2 and e_m < 3e-2 and e_1 < 3e-2               # bf16 outputs of O(1) values
    # and the derived bound against float64 (tests/qformer_attn_ref.py: u |ref| + u A + 2e-5)
    from tests.qformer_attn_ref import attn_bound, xattn64
    from tests.rowops_ref_common import _check
    ref64, A64 = xattn64(q.cpu(), k.cpu(), v.cpu(), pm.cpu(), heads, 33, "uniform")
    for name, o in (("LDS-DMA", out_m), ("first generation", out_1), ("simple", out_s)):
        _check(f"cross_attn {name} L={L}", o.cpu(), ref64, attn_bound(ref64, A64, torch.bfloat16))
    if L <= 320:                                                  # same per-unit arithmetic, other data movement
        assert torch.equal(out_m, out_1)
    # empty pair (0,0): uniform softmax over the L real keys == mean of V
    mean_v = v.float().mean(0)
    assert (out_m[:33].float() - mean_v[None]).abs().max().item() < 2e-2
    # fp32 storage through the scalar kernel is tight
    out_f = ops.qformer_cross_attn(q.float(), k.float(), v.float(), bits, pair_index, N, 33, heads,
                                   variant=_lib.PSG_XATTN_SIMPLE)
    assert (out_f - ref).abs().max().item() < 2e-5


@pytest.mark.parametrize("L,N,nq,policy", [(256, 50, 33, "uniform"), (256, 50, 33, "unmasked"), (96, 9, 33, "unmasked"),
                                           (128, 6, 16, "uniform"), (336, 7, 40, "unmasked")])
def test_cross_attn_mfma_matches_scalar_kernel(L, N, nq, policy):
    """The matrix-core kernel against the scalar checker kernel on what the goldens do not reach: both
    empty-row policies, row counts other than 33 (generic row tiles), a shuffled subset of the pairs (pair
    sharding hands the kernel arbitrary pair lists) and 2500 pairs (many row tiles per wave)."""
    from openpsg_amd import ops, _lib
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(L + 7 * N + nq)
    heads = 12
    perm = torch.randperm(N * N, generator=g)
    pair_index = perm[: max(1, (N * N * 3) // 4)].to(torch.int32).to(dev)
    P = pair_index.numel()
    q = (torch.randn(P * nq, 768, generator=g) * 1.5).to(dev).bfloat16()
    k = (torch.randn(L, 768, generator=g) * 1.5).to(dev).bfloat16()
    v = torch.randn(L, 768, generator=g).to(dev).bfloat16()
    om = torch.rand(N, L, generator=g) < 0.06
    om[0] = False
    om[N - 1] = False                                              # pairs among {0, N-1} have an empty union
    words = (L + 63) // 64
    bits_np = np.zeros((N, words * 64), dtype=np.uint8)
    bits_np[:, :L] = om.numpy()
    bits = torch.from_numpy(np.packbits(bits_np, axis=-1, bitorder="little").view(np.int64).reshape(N, words)).to(dev)
    pol = _lib.PSG_EMPTY_UNIFORM if policy == "uniform" else _lib.PSG_EMPTY_UNMASKED
    out_s = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, nq, heads, empty_policy=pol,
                                   variant=_lib.PSG_XATTN_SIMPLE)
    b = out_s.float()
    for name, var in (("LDS-DMA / default", _lib.PSG_XATTN_MFMA), ("first generation", _lib.PSG_XATTN_MFMA_V1)):
        out_m = torch.full_like(q, float("nan"))
        ops.qformer_cross_attn(q, k, v, bits, pair_index, N, nq, heads, out=out_m, empty_policy=pol, variant=var)
        torch.cuda.synchronize()
        a = out_m.float()
        err = ((a - b).abs() / (1.0 + b.abs())).max().item()      # both outputs are bf16: one ulp is 2^-8 relative
        print(f"L={L} N={N} nq={nq} {policy} [{name}]: P={P}, max |mfma - scalar| / (1 + |scalar|) = {err:.3e}")
        assert torch.isfinite(a).all() and err < 1.2e-2


def _xattn_case(L, N, P, dtype):
    """Inputs of test_cross_attn_mfma_vs_fp32_reference (objects 0 and 1 vanished: pair (0,0) has an empty union) in
    `dtype`, 33 query rows per pair, 12 heads.  Returns q, k, v, bits, pair_index, pair masks [P, L]."""
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(L * 1000 + N)
    q = (torch.randn(P * 33, 768, generator=g) * 1.5).to(dev).to(dtype)
    k = (torch.randn(L, 768, generator=g) * 1.5).to(dev).to(dtype)
    v = torch.randn(L, 768, generator=g).to(dev).to(dtype)
    om = torch.rand(N, L, generator=g) < 0.15
    om[0] = False
    if N > 2:
        om[1] = False
    words = (L + 63) // 64
    bits_np = np.zeros((N, words * 64), dtype=np.uint8)
    bits_np[:, :L] = om.numpy()
    bits = torch.from_numpy(np.packbits(bits_np, axis=-1, bitorder="little").view(np.int64).reshape(N, words)).to(dev)
    pair_index = torch.arange(P, dtype=torch.int32, device=dev)
    pm = (om[:, None, :] | om[None, :, :]).reshape(N * N, L)[:P].to(dev)
    return q, k, v, bits, pair_index, pm


def _xattn_rel(a, b):
    """The metric of test_cross_attn_mfma_matches_scalar_kernel: max |a - b| / (1 + |b|)."""
    a, b = a.float(), b.float()
    assert torch.isfinite(a).all()
    return ((a - b).abs() / (1.0 + b.abs())).max().item()


@pytest.mark.parametrize("L,N,P", [(288, 5, 25), (320, 3, 9)])
def test_cross_attn_three_key_chunks_on_the_dma_kernel(L, N, P):
    """257 <= L <= 320 (three chunks of 128 keys, eight waves) on the LDS-DMA kernel: bit-equal to the first generation,
    close to the fp32 restatement and to the scalar kernel.  L = 320 is the last geometry whose K/V image leaves room for
    the DMA slots; the indexed entry point, which only the LDS-DMA kernel serves, proves that it ran."""
    from openpsg_amd import ops, _lib
    heads = 12
    q, k, v, bits, pair_index, pm = _xattn_case(L, N, P, torch.bfloat16)
    import ctypes
    lds_bytes = _lib.load().psg_cross_attn_dma_lds_bytes   # int (int N, int words, int L): the dispatcher's own formula
    lds_bytes.argtypes, lds_bytes.restype = [ctypes.c_int] * 3, ctypes.c_int
    lds = lds_bytes(N, bits.shape[1], L)
    print(f"L={L} N={N}: LDS-DMA kernel needs {lds} B of LDS")
    assert lds <= 160 * 1024
    if L == 320:                                                   # one more 32-key tile no longer fits
        assert lds_bytes(N, (352 + 63) // 64, 352) > 160 * 1024
    ref = _xattn_reference(q, k, v, pm, heads)
    for pol in (_lib.PSG_EMPTY_UNIFORM, _lib.PSG_EMPTY_UNMASKED):
        out_m = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, empty_policy=pol, variant=_lib.PSG_XATTN_MFMA)
        out_1 = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, empty_policy=pol,
                                       variant=_lib.PSG_XATTN_MFMA_V1)
        out_s = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, empty_policy=pol,
                                       variant=_lib.PSG_XATTN_SIMPLE)
        out_i = ops.qformer_cross_attn_indexed(q, pair_index, q[::33].contiguous(), k, v, bits, pair_index, N, heads,
                                               empty_policy=pol)
        torch.cuda.synchronize()
        assert out_i is not None, "the LDS-DMA kernel does not take this geometry"
        assert torch.equal(out_m, out_1) and torch.equal(out_i, out_m)
        r_m, r_1 = _xattn_rel(out_m, out_s), _xattn_rel(out_1, out_s)
        print(f"L={L} policy {pol}: LDS-DMA vs scalar {r_m:.3e}, first generation vs scalar {r_1:.3e}")
        assert r_m < 1.2e-2 and r_1 < 1.2e-2
        if pol == _lib.PSG_EMPTY_UNIFORM:
            e_m, e_1 = (out_m.float() - ref).abs().max().item(), (out_1.float() - ref).abs().max().item()
            print(f"L={L}: LDS-DMA kernel err {e_m:.3e}, first-generation kernel err {e_1:.3e}")
            assert e_m < 3e-2 and e_1 < 3e-2


@pytest.mark.parametrize("L,N,P", [(40, 3, 9), (192, 7, 49)])
def test_cross_attn_fp16_both_generations(L, N, P):
    """fp16 storage on both matrix-core kernels (L = 40: padding keys in the only key tile): bit-equal to each other and
    within the bf16 test's bound of the scalar kernel run in fp16."""
    from openpsg_amd import ops, _lib
    heads = 12
    q, k, v, bits, pair_index, _ = _xattn_case(L, N, P, torch.float16)
    for pol in (_lib.PSG_EMPTY_UNIFORM, _lib.PSG_EMPTY_UNMASKED):
        out_m = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, empty_policy=pol, variant=_lib.PSG_XATTN_MFMA)
        out_1 = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, empty_policy=pol,
                                       variant=_lib.PSG_XATTN_MFMA_V1)
        out_s = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, empty_policy=pol,
                                       variant=_lib.PSG_XATTN_SIMPLE)
        torch.cuda.synchronize()
        assert out_m.dtype == torch.float16 and torch.equal(out_m, out_1)
        r_m, r_1 = _xattn_rel(out_m, out_s), _xattn_rel(out_1, out_s)
        print(f"fp16 L={L} policy {pol}: LDS-DMA vs scalar {r_m:.3e}, first generation vs scalar {r_1:.3e}")
        assert r_m < 1.2e-2 and r_1 < 1.2e-2


def test_cross_attn_dma_schedules_compute_the_same_bits():
    """841 pairs at L = 96: 868 row tiles per head, which the default deals dynamically to ten waves per workgroup.  The
    static deal, eight waves, ten waves dealt statically and write-back stores change which wave computes a unit and how
    its rows are stored, never the arithmetic: every output equals the default bit for bit."""
    from openpsg_amd import ops, _lib
    heads, N, L = 12, 29, 96
    q, k, v, bits, pair_index, _ = _xattn_case(L, N, N * N, torch.bfloat16)
    out_s = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, variant=_lib.PSG_XATTN_SIMPLE)
    want = ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, variant=_lib.PSG_XATTN_MFMA)
    torch.cuda.synchronize()
    assert _xattn_rel(want, out_s) < 1.2e-2
    names = ("xattn_dynamic", "xattn_waves", "xattn_wt")
    saved = {n: _lib.get_option(0, n) for n in names}
    try:
        for setting in ({"xattn_dynamic": 0}, {"xattn_waves": 0}, {"xattn_waves": 10, "xattn_dynamic": 0}, {"xattn_wt": 0}):
            for n in names:
                _lib.set_option(0, n, setting.get(n, saved[n]))
            got = torch.full_like(q, float("nan"))
            ops.qformer_cross_attn(q, k, v, bits, pair_index, N, 33, heads, out=got, variant=_lib.PSG_XATTN_MFMA)
            torch.cuda.synchronize()
            assert torch.equal(got, want), setting
            assert _xattn_rel(got, out_s) < 1.2e-2, setting
    finally:
        for n in names:
            _lib.set_option(0, n, saved[n])


@pytest.mark.parametrize("K,S,heads", [(20, 46, 32), (3, 64, 4), (5, 33, 2), (1, 7, 1)])
def test_prefill_attn_mfma_vs_scalar_kernel_and_fp32(K, S, heads):
    """psg_prefill_attn (matrix cores) against psg_llm_attn (scalar) and an fp32 torch causal attention on a
    pair-major prompt batch with ragged lengths (padding rows at the end of every pair)."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(K * 100 + S)
    D, ctx = heads * 128, S + 16
    lens = torch.randint(max(1, S - 12), S + 1, (K,), generator=g)
    lens[0] = S
    q = torch.randn(K * S, D, generator=g).to(dev).bfloat16()
    kc = torch.zeros(K, heads, ctx, 128, device=dev, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    kc[:, :, :S] = torch.randn(K, heads, S, 128, generator=g).to(dev).bfloat16()
    vc[:, :, :S] = torch.randn(K, heads, S, 128, generator=g).to(dev).bfloat16()
    t = torch.arange(S)[None, :].expand(K, -1)
    pos = torch.where(t < lens[:, None], t, torch.full_like(t, -1)).reshape(-1).to(torch.int32).to(dev)
    pair = torch.arange(K, dtype=torch.int32)[:, None].expand(-1, S).reshape(-1).contiguous().to(dev)
    kc_clean, vc_clean = kc.clone(), vc.clone()
    for kk in range(K):                                             # the engine does not zero the cache: rows the
        kc[kk, :, int(lens[kk]):] = float("nan")                    # rotary kernel never wrote must not be read
        vc[kk, :, int(lens[kk]):] = float("nan")
    out_m = torch.full((K * S, D), 7.0, device=dev, dtype=torch.bfloat16)
    out_s = torch.empty_like(out_m)
    ops.prefill_attn(q, kc, vc, pos, K, S, heads, 128, ctx, out_m)
    ops.llm_attn(q, kc, vc, pair, pos, heads, 128, ctx, out_s)
    # fp32 reference
    qh = q.float().view(K, S, heads, 128).permute(0, 2, 1, 3)
    sc = torch.einsum("khqd,khjd->khqj", qh, kc_clean[:, :, :S].float()) / 128 ** 0.5
    causal = torch.ones(S, S, dtype=torch.bool, device=dev).tril()
    keyok = (t < lens[:, None]).to(dev)
    sc = sc.masked_fill(~(causal[None, None] & keyok[:, None, None, :]), float("-inf"))
    ref = torch.einsum("khqj,khjd->khqd", torch.softmax(sc, -1), vc_clean[:, :, :S].float()).permute(0, 2, 1, 3).reshape(K * S, D)
    ok = (pos >= 0)
    e_m = (out_m.float() - ref)[ok].abs().max().item()
    e_s = (out_s.float() - ref)[ok].abs().max().item()
    print(f"K={K} S={S}: mfma err {e_m:.3e}, scalar err {e_s:.3e}")
    assert e_m < 3e-2 and e_s < 3e-2
    assert (out_m[~ok] == 0).all()                                  # padding rows: zeros, like the scalar kernel
    # and both inside the derived bound of tests/llm_attn_ref.py against float64 (the matrix-core kernel rounds its
    # probabilities to bf16: + u A)
    from tests import llm_attn_ref as L
    r64, A, gx, n, sv = L.causal64(q.cpu(), kc.cpu(), vc.cpu(), pos.cpu(), K, S, heads, sum_v=True)
    L.check("prefill_attn", out_m.cpu(), r64, L.attn_bound(r64, A, gx, n, torch.bfloat16, p_rounded=True, sum_v=sv))
    L.check("llm_attn", out_s.cpu(), r64, L.attn_bound(r64, A, gx, n, torch.bfloat16))


@pytest.mark.parametrize("dtype,competitors,seed", [("fp32", 0, 5), ("fp32", 1, 2), ("fp32", 1, 1), ("bf16", 1, 2),
                                                    ("bf16", 2, 0)])
def test_natural_eos_early_exit_matches_eager(dtype, competitors, seed):
    """Natural-EOS decoding replays graphs of 4 steps and stops once every pair has emitted EOS (the
    reference's per-pair generate stops at EOS, V4:305-312).  Tokens must equal the un-chunked eager decode,
    and the replay must really stop early when the pairs finish early."""
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.llm import LlamaDecodeEngine
    from openpsg_amd.weights import make_weights_device
    dev = _dev()
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(512, 2, 1024, 512), max_new_tokens=16)
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    w = make_weights_device(cfg, 11, dev, llm_dtype=tdt)
    # lm_head: every row zero except EOS and `competitors` other rows: the more competitors, the later the
    # slowest of the six pairs emits EOS (or never); the (competitors, seed) cases were picked to cover 1, 3 and 4
    # replayed graphs
    key = [k for k in w if k.endswith("lm_head.weight")][0]
    head_w = torch.zeros_like(w[key])
    for r in (cfg.llm.eos, 40, 41, 42)[:1 + competitors]:
        head_w[r] = w[key][r]
    w[key] = head_w
    eng = LlamaDecodeEngine(w, cfg, dev, tdt)
    g = torch.Generator().manual_seed(seed)
    K, Tp = 6, 9
    X = (torch.randn(K, 32 + Tp, cfg.llm.hidden, generator=g) * 0.5).to(dev).to(tdt)
    plen = torch.tensor([9, 7, 9, 5, 8, 9], dtype=torch.int32, device=dev)
    eng.use_graph = False
    want = eng.generate(X, plen, suppress_eos=False).clone()
    eng.use_graph = True
    for _ in range(2):                                            # capture, then pure replay
        got = eng.generate(X, plen, suppress_eos=False)
        assert torch.equal(got, want)
    is_eos = want == cfg.llm.eos
    first = torch.where(is_eos.any(dim=1), is_eos.int().argmax(dim=1), torch.full((K,), 15, device=dev))
    last_eos = int(first.max().item())                            # step at which the slowest pair ends (15: never)
    expect_replays = min(4, last_eos // 4 + 1)
    print(f"{dtype}/{competitors}: slowest pair emits EOS at step {last_eos}; graphs replayed {eng.last_replays} of 4")
    assert eng.last_replays == expect_replays
    # the worst-case (suppressed EOS) path is still one graph
    eng.generate(X, plen, suppress_eos=True)
    assert eng.last_replays == 1


@pytest.mark.parametrize("K,S,heads", [(20, 46, 32), (3, 64, 4), (4, 21, 2)])
def test_prefill_attn_rope_fused_matches_two_kernels(K, S, heads):
    """psg_prefill_attn_rope == psg_rope_kvwrite followed by psg_prefill_attn: attention output, rotated K rows
    and V rows in the cache (real tokens only; cache rows of padding tokens stay untouched)."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(K * 10 + S)
    D, ctx = heads * 128, S + 16
    lens = torch.randint(max(1, S - 9), S + 1, (K,), generator=g)
    lens[0] = S
    qkv = torch.randn(K * S, 3 * D, generator=g).to(dev).bfloat16()
    t = torch.arange(S)[None, :].expand(K, -1)
    pos = torch.where(t < lens[:, None], t, torch.full_like(t, -1)).reshape(-1).to(torch.int32).to(dev)
    pair = torch.arange(K, dtype=torch.int32)[:, None].expand(-1, S).reshape(-1).contiguous().to(dev)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
    ang = torch.arange(ctx, dtype=torch.float32)[:, None] * inv_freq[None, :]
    rope = (ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev))
    kc1 = torch.zeros(K, heads, ctx, 128, device=dev, dtype=torch.bfloat16)
    vc1, kc2, vc2 = torch.zeros_like(kc1), torch.zeros_like(kc1), torch.zeros_like(kc1)
    q = torch.zeros(K * S, D, device=dev, dtype=torch.bfloat16)
    out1 = torch.empty_like(q)
    out2 = torch.full_like(q, 3.0)
    ops.rope_kvwrite(qkv, pair, pos, rope, heads, 128, ctx, q, kc1, vc1)
    ops.prefill_attn(q, kc1, vc1, pos, K, S, heads, 128, ctx, out1)
    ops.prefill_attn_rope(qkv, pos, rope, K, S, heads, 128, ctx, kc2, vc2, out2)
    torch.cuda.synchronize()
    assert torch.equal(vc1, vc2)
    dk = ((kc1.float() - kc2.float()).abs() / (1 + kc1.float().abs())).max().item()
    do = ((out1.float() - out2.float()).abs() / (1 + out1.float().abs())).max().item()
    print(f"K={K} S={S}: cache K rel diff {dk:.2e}, output rel diff {do:.2e}")
    assert dk < 8e-3 and do < 1.2e-2                                # one bf16 ulp
    for k in range(K):                                              # rows past a pair's length: untouched
        assert (kc2[k, :, int(lens[k]):] == 0).all() and (vc2[k, :, int(lens[k]):] == 0).all()


def test_silu_mul_prompt_pass_kernel_equals_decode_kernel():
    """The 16-byte-load SwiGLU kernel used for dense bf16 batches of more than 64 rows computes exactly what the
    generic kernel computes row by row."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    rows, inter = 333, 2752
    gu = (torch.randn(rows, 2 * inter, generator=g) * 2).to(dev).bfloat16()
    big = torch.empty(rows, inter, device=dev, dtype=torch.bfloat16)
    ops.silu_mul(gu, big)
    small = torch.empty_like(big)
    for r0 in range(0, rows, 64):
        ops.silu_mul(gu[r0:r0 + 64].contiguous(), small[r0:r0 + 64])
    assert torch.equal(big, small)
    want = torch.nn.functional.silu(gu[:, :inter].float()).bfloat16().float() * gu[:, inter:].float()
    assert ((big.float() - want).abs() / (1 + want.abs())).max().item() < 8e-3       # one bf16 ulp


@pytest.mark.parametrize("vocab,splits,dtype", [(32000, 4, "bf16"), (32000, 0, "bf16"), (32003, 0, "fp32"), (515, 3, "bf16"),
                                                 (32000, 0, "fp32")])
def test_greedy_step_argmax_ties_suppress_and_bookkeeping(vocab, splits, dtype):
    """psg_greedy_step against torch.argmax: first maximal index on ties, suppressed token, EOS / done / position
    bookkeeping; vocabulary sizes with and without the 16-byte fast path, dense logits and split-K partials."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(vocab + splits)
    K, max_new, eos = 7, 5, 2
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    base = (torch.randn(K, vocab, generator=g) * 2).to(tdt).float()
    base[0, 100] = base[0, 400] = base[0].max() + 1                # tie: index 100 must win
    base[1, eos] = base[1].max() + 3                               # pair 1 emits EOS
    base[2, 7] = base[2].max() + 3                                 # pair 2's maximum is the suppressed token
    base[3, vocab - 1] = base[3].max() + 2                         # last entry (tail loop when vocab % 4 != 0)
    if splits:
        parts = torch.randn(splits, K, vocab, generator=g)
        parts[-1] = base - parts[:-1].sum(0)
        logits = ops.Partials(parts.to(dev).contiguous())
        summed = parts.to(dev)[0].clone()
        for sidx in range(1, splits):
            summed += parts.to(dev)[sidx]
        ref_logits = summed.to(tdt).float() if tdt == torch.bfloat16 else summed
    else:
        logits = base.to(dev).to(tdt).contiguous()
        ref_logits = logits.float()
    ref = ref_logits.clone()
    ref[:, 7] = float("-inf")
    want = ref.argmax(dim=1).to(torch.int32)
    tokens = torch.full((K, max_new), -1, device=dev, dtype=torch.int32)
    done = torch.zeros(K, device=dev, dtype=torch.int32)
    done[4] = 1                                                    # pair 4 finished earlier
    next_ids = torch.zeros(K, device=dev, dtype=torch.int32)
    pos = torch.arange(K, device=dev, dtype=torch.int32) + 40
    # the chosen token's embedding row goes to the next step's residual rows in the same launch (16-bit or fp32 rows)
    emb_dt = torch.float32 if tdt == torch.float32 else tdt
    embed = torch.randn(vocab, 256, generator=g).to(dev, emb_dt)
    x_out = torch.full((K, 256), float("nan"), device=dev, dtype=torch.float32 if splits else emb_dt)
    ops.greedy_step(logits, 1, max_new, eos, 7, tokens, done, next_ids, pos, dtype=tdt, embed=embed, x_out=x_out)
    torch.cuda.synchronize()
    assert torch.equal(next_ids, want)
    assert torch.equal(x_out.float(), embed[want.long()].float())
    if not splits:
        assert int(want[0]) == 100 and int(want[3]) == vocab - 1
    exp_tok = want.clone()
    exp_tok[4] = -1
    assert torch.equal(tokens[:, 1], exp_tok) and (tokens[:, 0] == -1).all()
    exp_done = (want == eos).to(torch.int32)
    exp_done[4] = 1
    assert torch.equal(done, exp_done)
    assert torch.equal(pos, torch.arange(K, device=dev, dtype=torch.int32) + 41)


def test_bias_gelu_many_rows_bf16_kernel():
    """The 16-byte / Abramowitz-Stegun-erf kernel used for bf16 batches of 256+ rows against the generic erff kernel
    (same inputs in chunks of 255 rows) and against torch's exact GELU in fp32."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    rows, cols = 1000, 3072
    x = (torch.randn(rows, cols, generator=g) * 3).to(dev).bfloat16()
    x[0, :8] = torch.tensor([0.0, -0.0, 8.0, -8.0, 1e-3, -1e-3, 30.0, -30.0]).bfloat16()
    b = torch.randn(cols, generator=g).to(dev)
    big = ops.bias_gelu(x.clone(), b)
    small = torch.empty_like(big)
    for r0 in range(0, rows, 255):
        small[r0:r0 + 255] = ops.bias_gelu(x[r0:r0 + 255].clone(), b)
    want = torch.nn.functional.gelu(x.float() + b)
    assert torch.isfinite(big.float()).all()
    mism = (big != small).float().mean().item()
    # half a bf16 ulp relative, plus 2e-6 absolute for the deep negative tail where 1 + erf cancels in fp32 (the
    # reference formula itself is rounding noise there: |gelu| < 1e-5)
    excess = ((big.float() - want).abs() - 4.5e-3 * want.abs()).max().item()
    print(f"bias_gelu: {mism * 100:.3f} % of bf16 outputs differ from the erff kernel (deep tail); max excess error {excess:.2e}")
    assert mism < 2e-2 and excess < 2e-6


@pytest.mark.parametrize("B,T", [(7, 14), (33, 9), (4, 31)])
def test_self_attn_shared_query_rows_equals_full_kernel(B, T):
    """Layer 0: every pair's 33 query rows carry the same Q/K/V projection.  The shared-block kernel entry must give
    bit-identical output to the full kernel run on a qkv matrix that repeats that block for every pair."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(B * 10 + T)
    nq, heads, H = 33, 12, 768
    qkv_q = torch.randn(nq, 3 * H, generator=g).to(dev).bfloat16()
    qkv_t = torch.randn(B * T, 3 * H, generator=g).to(dev).bfloat16()
    mask = (torch.rand(B, T, generator=g) < 0.8).to(torch.uint8)
    mask[:, 0] = 1
    mask = mask.to(dev)
    full = torch.cat([qkv_q.repeat(B, 1), qkv_t]).contiguous()
    want = torch.empty(B * (nq + T), H, device=dev, dtype=torch.bfloat16)
    ops.qformer_self_attn(full, mask, B, T, nq, heads, False, want)
    got = torch.full_like(want, 5.0)
    ops.qformer_self_attn_shared(qkv_q, qkv_t, mask, B, T, nq, heads, got)
    assert torch.equal(got, want)


def test_embed_split_and_periodic_residual_equal_the_full_kernels():
    """Layer-0 redundancy removal: qformer_embed_split writes the query block once + the text rows;
    add_layernorm_periodic reads the residual from that one block.  Both must be bit-identical to the full kernels
    fed with the per-pair copies.
    psg_qformer_embed itself is anchored to float64 in tests/test_gpu_image_kernels_ref.py."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(17)
    B, T, nq, H = 9, 11, 33, 768
    ids = torch.randint(0, 500, (B, T), generator=g, dtype=torch.int32).to(dev)
    word = torch.randn(500, H, generator=g).to(dev)
    posw = torch.randn(64, H, generator=g).to(dev)
    qrows = torch.randn(nq, H, generator=g).to(dev)
    lw, lb = torch.rand(H, generator=g).to(dev) + 0.5, torch.randn(H, generator=g).to(dev)
    full = torch.empty(B * (nq + T), H, device=dev, dtype=torch.bfloat16)
    ops.qformer_embed(ids, word, posw, qrows, lw, lb, 1e-12, full)
    part = torch.full_like(full, 9.0)
    ops.qformer_embed_split(ids, word, posw, qrows, lw, lb, 1e-12, part[:nq], part[B * nq:])
    assert torch.equal(part[:nq], full[:nq]) and torch.equal(part[B * nq:], full[B * nq:])
    assert torch.equal(full[:B * nq], full[:nq].repeat(B, 1))       # the premise: every pair has the same query rows
    assert (part[nq:B * nq] == 9.0).all()                           # rows in between are not touched
    x = torch.randn(B * nq, H, generator=g).to(dev).bfloat16()
    bias = torch.randn(H, generator=g).to(dev)
    want = ops.add_layernorm(x.clone(), full[:B * nq].contiguous(), bias, lw, lb, 1e-12)
    got = ops.add_layernorm_periodic(x.clone(), full[:nq].contiguous(), bias, lw, lb, 1e-12)
    assert torch.equal(got, want)


def test_mask_kernels_bit_exact_on_random_geometries():
    """psg_mask_grid / psg_object_bitmasks against the torch interpolate -> pad -> interpolate chain of the
    reference (V4:416-433, via the oracle) on 40 seeded random geometries: odd sizes, non-square images,
    down- and up-scaling, padding, id 0 (void aliasing person #0), objects that vanish on the grid."""
    from openpsg_amd import ops
    from oracle import psg_oracle as O
    dev = _dev()
    rng = np.random.default_rng(1234)
    for case in range(40):
        H0, W0 = int(rng.integers(17, 700)), int(rng.integers(17, 900))
        scale = float(rng.uniform(0.4, 2.2))
        img_h, img_w = max(16, int(round(H0 * scale))), max(16, int(round(W0 * scale)))
        pad_h, pad_w = -(-img_h // 64) * 64, -(-img_w // 64) * 64        # feature map = pad / 4, patch 16
        if rng.random() < 0.3:
            pad_h += 64
        gh, gw = pad_h // 64, pad_w // 64
        n = int(rng.integers(1, 14))
        ids = [int(rng.integers(0, 133)) + 1000 * int(rng.integers(0, 3)) for _ in range(n)]
        ids = list(dict.fromkeys(ids))
        pan = np.full((H0, W0), 0 if rng.random() < 0.3 else 133, dtype=np.int32)
        for oid in ids:
            y0, x0 = int(rng.integers(0, H0)), int(rng.integers(0, W0))
            hh, ww = int(rng.integers(1, max(2, H0 // 2))), int(rng.integers(1, max(2, W0 // 2)))
            pan[y0:y0 + hh, x0:x0 + ww] = oid
        pan_t = torch.from_numpy(pan)
        want_grid = O.mask_grid(pan_t, (img_h, img_w), (pad_h, pad_w), (gh, gw))
        want = O.object_masks(want_grid, ids).numpy()
        grid = ops.mask_grid(pan_t.to(dev), (img_h, img_w), (pad_h, pad_w), (gh, gw))
        assert torch.equal(grid.cpu().reshape(gh, gw), want_grid), (case, H0, W0, img_h, img_w, pad_h, pad_w)
        bits = ops.object_bitmasks(grid, torch.tensor(ids, dtype=torch.int32, device=dev)).cpu().numpy().view(np.uint64)
        got = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder="little")[:, :gh * gw].astype(bool)
        assert np.array_equal(got, want), (case, ids)


@pytest.mark.parametrize("n,k", [(1, 1), (2, 4), (15, 20), (17, 5), (100, 20), (1030, 20), (2500, 20), (2500, 64),
                                 (3072, 20), (3073, 20), (10000, 20), (2500, 65)])
def test_topk_rank_kernel_matches_sort(n, k):
    """psg_topk (rank-based kernel up to 3072 elements / k <= 64, round-based beyond): larger score first, ties ->
    lower index, NaN last, -1 padding - against a host sort of the same keys (V4:235-237)."""
    from openpsg_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(n * 131 + k)
    s = torch.rand(n, generator=gen)
    s = (s * 50).floor() / 50 if n > 20 else s                     # many exact ties
    if n > 3:
        s[n // 3] = float("nan")
        s[n // 2] = float("inf")
    key = torch.where(torch.isnan(s), torch.full_like(s, -float("inf")), s)
    order = sorted(range(n), key=lambda i: (-key[i].item(), i))[:k]
    want = order + [-1] * (k - len(order))
    idx, val = ops.topk(s.to(dev), k)
    assert idx.cpu().tolist() == want
    got_v = val.cpu()
    for r, i in enumerate(order):
        assert got_v[r].item() == key[i].item()


def test_topk_ties_and_order():
    from openpsg_amd import ops
    dev = _dev()
    s = torch.tensor([0.5, 0.9, 0.9, 0.1, 0.9, 0.5, 1.0, 0.0], device=dev)
    idx, val = ops.topk(s, 6)
    assert idx.cpu().tolist() == [6, 1, 2, 4, 0, 5]
    idx, _ = ops.topk(torch.tensor([0.3, 0.2], device=dev), 4)
    assert idx.cpu().tolist() == [0, 1, -1, -1]
    g = torch.Generator().manual_seed(3)
    big = torch.rand(10000, generator=g)
    want = torch.sort(big, descending=True, stable=True).indices[:20].tolist()
    assert ops.topk(big.to(dev), 20)[0].cpu().tolist() == want


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("rows", [1, 7, 66, 33 * 9])
def test_add_layernorm_16bit_variants_vs_fp32_torch(dtype, rows):
    """add + LayerNorm on 16-bit rows (HF-IB:519-530, 579-596): the half-wave-per-row kernel (option ln_half_wave) and the
    wave-per-row kernel give the fp32 torch result to one rounding of the output; residual taken from the same-shaped
    tensor, from one shared block (periodic) and from a block table through an index (the pair's prompt)."""
    from openpsg_amd import _lib, ops
    dev = _dev()
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 768, generator=g).to(dev, tdt)
    r = torch.randn(rows, 768, generator=g).to(dev, tdt)
    b = torch.randn(768, generator=g).to(dev)
    gam, bet = (1 + 0.2 * torch.randn(768, generator=g)).to(dev), torch.randn(768, generator=g).to(dev)
    ulp = 2.0 ** (-8 if dtype == "bf16" else -11)

    def close(got, want):
        return ((got.float() - want).abs() / (1 + want.abs())).max().item() < 1.5 * ulp

    outs = {}
    G = rows // 33
    tab = torch.randn(4 * 33, 768, generator=g).to(dev, tdt)
    idx = torch.randint(0, 4, (max(G, 1),), generator=g)[:G].to(dev, torch.int32)
    try:
        for hw in (1, 0):
            _lib.set_option(0, "ln_half_wave", hw)
            want = torch.nn.functional.layer_norm(x.float() + b + r.float(), (768,), gam, bet, 1e-12)
            got = ops.add_layernorm(x.clone(), r, b, gam, bet, 1e-12)
            assert close(got, want)
            outs[hw] = [got]
            if rows % 33 == 0:                                     # groups of 33 rows (the query rows of a pair)
                wantp = torch.nn.functional.layer_norm(x.float() + b + tab[:33].float().repeat(G, 1), (768,), gam, bet, 1e-12)
                gotp = ops.add_layernorm_periodic(x.clone(), tab[:33].contiguous(), b, gam, bet, 1e-12)
                rows_i = (idx.long()[:, None] * 33 + torch.arange(33, device=dev)[None, :]).reshape(-1)
                wanti = torch.nn.functional.layer_norm(x.float() + b + tab[rows_i].float(), (768,), gam, bet, 1e-12)
                goti = ops.add_layernorm_indexed(x.clone(), tab, idx, 33, b, gam, bet, 1e-12)
                assert close(gotp, wantp) and close(goti, wanti)
                outs[hw] += [gotp, goti]
    finally:
        _lib.set_option(0, "ln_half_wave", 1)
    for a_, b_ in zip(outs[0], outs[1]):                           # the two kernels: same rounding class
        assert ((a_.float() - b_.float()).abs() / (1 + b_.float().abs())).max().item() < 2.1 * ulp


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("rows", [1, 66, 33 * 9])
def test_add_layernorm_fp32_residual_dual_output_vs_fp32_torch(dtype, rows):
    """Mixed mode's LayerNorm (psg_add_layernorm_res32): 16-bit projection output + fp32 residual -> fp32 result (exact to
    fp32 rounding: the next residual) and its 16-bit copy (one rounding: the next operand); plain, periodic and indexed
    residual rows."""
    from openpsg_amd import ops
    dev = _dev()
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    g = torch.Generator().manual_seed(rows + 5)
    x = torch.randn(rows, 768, generator=g).to(dev, tdt)
    r = torch.randn(rows, 768, generator=g).to(dev)
    b = torch.randn(768, generator=g).to(dev)
    gam, bet = (1 + 0.2 * torch.randn(768, generator=g)).to(dev), torch.randn(768, generator=g).to(dev)
    ulp = 2.0 ** (-8 if dtype == "bf16" else -11)
    G = rows // 33
    tab = torch.randn(4 * 33, 768, generator=g).to(dev)
    idx = torch.randint(0, 4, (max(G, 1),), generator=g)[:G].to(dev, torch.int32)
    cases = [(dict(), r)]
    if rows % 33 == 0:
        rows_i = (idx.long()[:, None] * 33 + torch.arange(33, device=dev)[None, :]).reshape(-1)
        cases += [(dict(period=33), tab[:33].contiguous()), (dict(period=33, index=idx), tab)]
    for kw, res in cases:
        full = res if not kw else (res.repeat(G, 1) if "index" not in kw else tab[rows_i])
        want = torch.nn.functional.layer_norm(x.float() + b + full, (768,), gam, bet, 1e-12)
        o16, o32 = ops.add_layernorm_res32(x.clone(), res, b, gam, bet, 1e-12, **kw)
        assert o16.dtype == tdt and o32.dtype == torch.float32
        assert (o32 - want).abs().max().item() < 2e-5
        assert ((o16.float() - want).abs() / (1 + want.abs())).max().item() < 1.5 * ulp
        only32 = ops.add_layernorm_res32(x.clone(), res, b, gam, bet, 1e-12, want16=False, **kw)
        assert only32[0] is None and torch.equal(only32[1], o32)


def test_row_kernels_vs_torch():
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 768, generator=g).to(dev)
    r = torch.randn(37, 768, generator=g).to(dev)
    b = torch.randn(768, generator=g).to(dev)
    gam, bet = torch.randn(768, generator=g).to(dev), torch.randn(768, generator=g).to(dev)
    want = torch.nn.functional.layer_norm(x + b + r, (768,), gam, bet, 1e-12)
    got = ops.add_layernorm(x.clone(), r, b, gam, bet, 1e-12)
    assert (got - want).abs().max().item() < 1e-5
    y = torch.randn(11, 3072, generator=g).to(dev)
    b2 = torch.randn(3072, generator=g).to(dev)
    assert (ops.bias_gelu(y.clone(), b2) - torch.nn.functional.gelu(y + b2)).abs().max().item() < 1e-6
    for D in (256, 1024, 4096):
        h = torch.randn(9, D, generator=g).to(dev)
        d = torch.randn(9, D, generator=g).to(dev)
        w = torch.randn(D, generator=g).to(dev)
        res = h.clone()
        out = torch.empty_like(h)
        ops.rmsnorm(res, d, w, 1e-5, out)
        hh = h + d
        want = w * (hh * torch.rsqrt(hh.pow(2).mean(-1, keepdim=True) + 1e-5))
        assert (res - hh).abs().max().item() == 0
        assert (out - want).abs().max().item() < 1e-5
    gu = torch.randn(7, 2 * 512, generator=g).to(dev)
    o = torch.empty(7, 512, device=dev)
    ops.silu_mul(gu, o)
    assert (o - torch.nn.functional.silu(gu[:, :512]) * gu[:, 512:]).abs().max().item() < 1e-6


def test_single_object_and_no_object():
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    head = _head(cfg, w, "fp32")
    inp = _inputs(scene)
    inp["object_info"][0]["object_id_list"] = scene["object_id_list"][:1]
    out = head(inp)
    assert head.last["exist_logit"].numel() == 1 and head.last["tokens_host"].shape[0] == 1
    inp["object_info"][0]["object_id_list"] = []
    assert head(inp) == dict(rel_pred=[], rel_score=[])


def test_no_cpu_fallback():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    with pytest.raises(PsgHipError):
        ops.topk(torch.rand(8), 2)                                 # CPU tensor must be rejected loudly


def _fuzz_skinny_shapes():
    """PSG_FUZZ_GEMM=count (a one-off sweep, profiles/r06_fuzz_gemm.txt): random shapes of the 16-bit streaming kernel - 1..32
    rows, N any multiple of 16 up to 8192, K any multiple of 64 up to 16384."""
    import os
    import random
    n = int(os.environ.get("PSG_FUZZ_GEMM", "0"))
    r = random.Random(515)
    return [(r.randint(1, 32), 16 * r.randint(1, 512), 64 * r.randint(1, 256)) for _ in range(n)]


@pytest.mark.parametrize("M,N,K", [(20, 4096, 4096), (20, 4096, 11008), (1, 512, 256), (32, 768, 2752), (7, 32000, 4096)]
                         + _fuzz_skinny_shapes())
def test_skinny_gemm_vs_fp32_reference(M, N, K):
    """A max-norm check at the workload's shapes; the kernel's anchor - float64, per element, both 16-bit types, every
    variant - is tests/test_gpu_gemm16_ref.py."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g).to(dev).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).bfloat16()
    part = ops.skinny_gemm(x, w)
    y = part.reduce(torch.bfloat16)
    print(f"splits = {part.splits}")
    ref = x.float() @ w.float().t()
    err = (y.float() - ref).abs().max().item()
    lib = (torch.nn.functional.linear(x, w).float() - ref).abs().max().item()
    print(f"M={M} N={N} K={K}: skinny err {err:.3e}, hipBLASLt err {lib:.3e}")
    assert err < 2e-2 and err <= lib * 2 + 1e-3
    # batch invariance: a row's result does not depend on the other rows (needed for pair sharding)
    if M > 1:
        y1 = ops.skinny_gemm(x[:1].contiguous(), w, splits=part.splits).reduce(torch.bfloat16)
        assert torch.equal(y1[0], y[0])
    # consumers that sum the split-K slices themselves agree with the materialised reduction
    if N % 8 == 0:
        out = torch.empty(M, N // 2, device=dev, dtype=torch.bfloat16)
        ops.silu_mul(part, out)
        want = torch.empty_like(out)
        ops.silu_mul(y, want)
        assert torch.equal(out, want)


@pytest.mark.parametrize("hw,C", [((256, 256), 256), ((128, 128), 256), ((192, 256), 256), ((256, 336), 256), ((64, 48), 32)])
def test_patch_embed_vs_conv2d(hw, C):
    """A max-norm check at the workload's shapes; the kernel's anchor - float64, per element, both input families, every
    tile / split edge - is tests/test_gpu_image_kernels_ref.py."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(hw[0] + hw[1])
    feat = torch.randn(1, C, hw[0], hw[1], generator=g).to(dev)
    w = (torch.randn(256, C, 16, 16, generator=g) / (C * 256) ** 0.5).to(dev)
    b = torch.randn(256, generator=g).to(dev)
    got = ops.patch_embed(feat, w, b)
    want = torch.nn.functional.conv2d(feat.double(), w.double(), b.double(), stride=16).flatten(2).transpose(1, 2)[0]
    err = (got.double() - want).abs().max().item()
    print(f"patch_embed {hw} C={C}: max err vs fp64 conv {err:.2e}")
    assert got.shape == want.shape and err < 2e-5


@pytest.mark.parametrize("B,T,q_only", [(7, 14, False), (5, 17, True), (3, 31, False), (4, 9, True)])
def test_self_attn_mfma_vs_fp32_reference(B, T, q_only):
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(B * 100 + T)
    nq, heads, H = 33, 12, 768
    R = B * (nq + T)
    qkv = (torch.randn(R, 3 * H, generator=g) * 1.2).to(dev).bfloat16()
    tmask = (torch.rand(B, T, generator=g) < 0.8).to(torch.uint8)
    tmask[:, 0] = 1
    tmask = tmask.to(dev)
    out = torch.zeros(R, H, device=dev, dtype=torch.bfloat16)
    ops.qformer_self_attn(qkv, tmask, B, T, nq, heads, q_only, out)
    # fp32 torch restatement on the same bf16 inputs
    f = qkv.float()
    worst = 0.0
    for p in range(B):
        rows = list(range(p * nq, (p + 1) * nq)) + list(range(B * nq + p * T, B * nq + (p + 1) * T))
        x = f[rows]
        q_, k_, v_ = [x[:, i * H:(i + 1) * H].view(-1, heads, 64).permute(1, 0, 2) for i in range(3)]
        valid = torch.cat([torch.ones(nq, device=dev), tmask[p].float()])
        s = q_ @ k_.transpose(1, 2) * 0.125 + ((1 - valid) * torch.finfo(torch.float32).min)[None, None, :]
        o = (torch.softmax(s, -1) @ v_).permute(1, 0, 2).reshape(-1, H)
        n = nq if q_only else nq + T
        got = out[rows][:n].float()
        worst = max(worst, (got - o[:n]).abs().max().item())
    print(f"self_attn mfma B={B} T={T} q_only={q_only}: max err {worst:.3e}")
    assert worst < 3e-2
    # and the derived bound against float64 (tests/qformer_attn_ref.py: u |ref| + u A + 2e-5)
    from tests.qformer_attn_ref import attn_bound, selfattn64
    from tests.rowops_ref_common import _check
    ref64, A64 = selfattn64(qkv.cpu(), tmask.cpu(), B, T, nq, heads, "query" if q_only else "all")
    _check(f"self_attn mfma B={B} T={T}", out[:ref64.shape[0]].cpu(), ref64, attn_bound(ref64, A64, torch.bfloat16))


@pytest.mark.parametrize("geo", [((1024, 1024), None, None, 50), ((768, 1024), (720, 960), (750, 1000), 12)])
def test_masked_mean_pool_vs_reference_formula(geo):
    """SURVEY 8f rank 4 (openseed_relation.py:453-468): (feat*m).sum/(m.sum+1e-8) per object.
    A max-norm check at the workload's shapes; the kernel's anchor is tests/test_gpu_image_kernels_ref.py."""
    import torch.nn.functional as F
    from openpsg_amd import ops
    from openpsg_amd.synthetic import make_scene
    pad, ori, img, N = geo
    sc = make_scene(pad, N, seed=9, ori_hw=ori, img_hw=img, void_id=0, force_id0=True, tiny_object=True, device="cuda:0")
    feat, pan, meta = sc["mask_features"], sc["pan_results"], sc["img_meta"]
    ids = torch.tensor([int(i) for i in sc["object_id_list"]], dtype=torch.int32, device="cuda:0")
    got = ops.masked_mean_pool(feat, pan, meta["img_shape"][:2], meta["pad_shape"][:2], ids)
    # the reference's chain on the GPU in fp64: per-object masks -> interpolate(img) -> pad -> interpolate(feat)
    # (float32 masks, as the reference's `.to(dtype)`: ATen derives the nearest-neighbour scale in the tensor's precision)
    masks = torch.stack([(pan == i) for i in ids.tolist()]).float()[None]
    m = F.interpolate(masks, size=meta["img_shape"][:2])
    m = F.pad(m, (0, meta["pad_shape"][1] - meta["img_shape"][1], 0, meta["pad_shape"][0] - meta["img_shape"][0]))
    m = F.interpolate(m, size=feat.shape[-2:])[0][:, None].double()
    want = (feat.double() * m).sum(dim=[2, 3]) / (m.sum(dim=[2, 3]) + 1e-8)
    err = (got.double() - want).abs().max().item()
    print(f"masked_mean_pool {pad} N={N}: max err {err:.2e}; empty objects: {int((m.sum(dim=[2,3]) == 0).sum())}")
    assert err < 1e-4
    again = ops.masked_mean_pool(feat, pan, meta["img_shape"][:2], meta["pad_shape"][:2], ids)
    assert torch.equal(got, again)                                  # deterministic


@pytest.mark.parametrize("output_size", [1, 4, 7])
def test_masked_split_mean_pool_vs_reference_formula(output_size):
    """`_mask_pooling(feature, mask, output_size)` (openseed_relation.py:175-200), restated per object in fp64: pixels in
    row-major order, torch.split into output_size chunks (the first n mod k one longer), chunk means; an object with fewer
    pixels than chunks repeats its pixels; an object without pixels gives zeros.
    A max-norm check at the workload's shapes; the kernel's anchor is tests/test_gpu_image_kernels_ref.py."""
    import numpy as np
    import torch.nn.functional as F
    from openpsg_amd import ops
    from openpsg_amd.synthetic import make_scene
    pad, ori, img, N = (768, 1024), (720, 960), (750, 1000), 12
    sc = make_scene(pad, N, seed=9, ori_hw=ori, img_hw=img, void_id=0, force_id0=True, tiny_object=True, device="cuda:0")
    feat, pan, meta = sc["mask_features"], sc["pan_results"], sc["img_meta"]
    ids = torch.tensor([int(i) for i in sc["object_id_list"]], dtype=torch.int32, device="cuda:0")
    got = ops.masked_split_mean_pool(feat, pan, meta["img_shape"][:2], meta["pad_shape"][:2], ids, output_size)
    masks = torch.stack([(pan == i) for i in ids.tolist()]).float()[None]
    m = F.interpolate(masks, size=meta["img_shape"][:2])
    m = F.pad(m, (0, meta["pad_shape"][1] - meta["img_shape"][1], 0, meta["pad_shape"][0] - meta["img_shape"][0]))
    m = F.interpolate(m, size=feat.shape[-2:])[0]
    f = feat[0].double()
    small = 0
    for n in range(N):
        mask = m[n:n + 1]
        if mask.sum() <= 0:                                       # openseed_relation.py:182-183
            want = f.new_zeros((output_size, f.shape[0]))
        else:
            feats = f[:, (mask >= 0.5)[0]]
            if feats.shape[1] < output_size:
                small += 1
                feats = torch.cat([feats] * int(np.ceil(output_size / feats.shape[1])), dim=1)[:, :output_size]
            split = [feats.shape[1] // output_size] * output_size
            for idx in range(feats.shape[1] - sum(split)):
                split[idx] += 1
            want = torch.cat([x.mean(dim=1)[None] for x in torch.split(feats, split, dim=1)], dim=0)
        err = (got[n].double() - want).abs().max().item()
        assert err < 1e-4, (n, err)
    print(f"split-mean pool, output_size {output_size}: objects with fewer pixels than chunks: {small}")
    if output_size == 1:
        mean = ops.masked_mean_pool(feat, pan, meta["img_shape"][:2], meta["pad_shape"][:2], ids)
        assert (got[:, 0] - mean).abs().max().item() < 1e-5


def test_head_state_dict_matches_reference_and_loads_partial_checkpoint():
    """Drop-in checkpoint contract: same parameter names/shapes as the reference module; a partial
    checkpoint (no language_model.*, part_checkpoint_hook.py:96-116) loads with strict=False."""
    import json
    from openpsg_amd.head import RelationTransformerHeadV4
    ref = json.load(open(H.GOLDEN + "/reference_state_dict_keys.json"))
    head = RelationTransformerHeadV4(device="cuda:0", tokenizers="word")          # reference default sizes
    sd = head.state_dict()
    assert set(sd) == set(ref)
    for k, shape in ref.items():
        assert list(sd[k].shape) == shape, k
    ckpt = {k: torch.full(tuple(shape), 0.5) for k, shape in ref.items() if not k.startswith("language_projection")}
    ckpt["some_other.module.weight"] = torch.zeros(3)                              # unexpected keys are ignored
    res = head.load_state_dict(ckpt, strict=False)
    assert "language_projection.weight" in res.missing_keys
    assert float(head.binary_rel_cls_pred.weight[0, 0]) == 0.5
    with pytest.raises(Exception):
        head.llm_engine                                                            # LLM weights were never provided


def test_context_options_and_caller_provided_trace_buffer():
    """Kernel variants are options of the psg_ctx (no process-global state); per-wave stamps go to a buffer the
    CALLER provides (the library never allocates or synchronises)."""
    from openpsg_amd import _lib, ops
    from openpsg_amd._lib import PsgHipError
    dev = _dev()
    assert _lib.get_option(0, "skinny_xdma") in (0, 1)
    with pytest.raises(PsgHipError):
        _lib.set_option(0, "no_such_option", 1)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(20, 4096, generator=g).to(dev).bfloat16()
    w = (torch.randn(4096, 4096, generator=g) / 64).to(dev).bfloat16()
    outs = {}
    old = _lib.get_option(0, "skinny_xdma")
    try:
        for xd in (0, 1):                                           # x slice by plain loads vs by LDS-DMA: same bits
            _lib.set_option(0, "skinny_xdma", xd)
            outs[xd] = ops.skinny_gemm(x, w).t.clone()
    finally:
        _lib.set_option(0, "skinny_xdma", old)
    assert torch.equal(outs[0], outs[1])
    buf = torch.zeros(1 << 18, dtype=torch.int64, device=dev)
    _lib.set_trace_buffer(0, _lib.PSG_TRACE_SKINNY_GEMM, buf)
    try:
        ops.skinny_gemm(x, w)
        torch.cuda.synchronize()
    finally:
        _lib.set_trace_buffer(0, _lib.PSG_TRACE_NONE)
    t = buf.cpu().view(-1, 8)
    t = t[t[:, 0] > 0]
    assert t.shape[0] >= 256 and (t[:, 5] >= t[:, 0]).all()        # every wave stamped start <= end
    buf.zero_()
    ops.skinny_gemm(x, w)                                           # tracing off again: nothing is written
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0


@pytest.mark.parametrize("B,N,R,C", [(1, 50, 56, 768), (2, 7, 3, 40), (1, 100, 56, 256), (1, 33, 5, 33)])
def test_bilinear_scores_vs_einsum(B, N, R, C):
    """The closed-set heads' scorer (relation_transformer_head_v2.py:204-209) against the reference's own
    reshape + permute + einsum in fp64.
    A max-norm check at the workload's shapes; the kernel's anchor is tests/test_gpu_image_kernels_ref.py."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(B * 1000 + N)
    sub = torch.randn(B, N, R * C, generator=g).to(dev)
    obj = torch.randn(B, N, R * C, generator=g).to(dev)
    got = ops.bilinear_scores(sub, obj, R)
    s4 = sub.double().reshape(B, N, R, C).permute(0, 2, 1, 3)
    o4 = obj.double().reshape(B, N, R, C).permute(0, 2, 1, 3)
    want = torch.einsum('nrsc,nroc->nrso', s4, o4)
    err = (got.double() - want).abs().max().item()
    print(f"bilinear scorer B={B} N={N} R={R} C={C}: max err vs fp64 einsum {err:.2e}")
    assert got.shape == (B, R, N, N) and err < 2e-4 * (C ** 0.5)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K,gelu", [(3000, 3072, 768, True), (777, 768, 768, False), (256, 256, 64, True),
                                        (4099, 2304, 3072, False)])
def test_dense_gemm_fused_epilogue_vs_fp32_reference(dt, M, N, K, gelu):
    """psg_dense_gemm (own MFMA GEMM, bias + exact-erf GELU fused; HF-IB:563-577) against fp32 torch, with a ragged
    last row tile, and against the unfused product path (library GEMM + psg_bias_gelu)."""
    from openpsg_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(dev).to(dt)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).to(dt)
    b = torch.randn(N, generator=g).to(dev)
    out = torch.full((M + 3, N), 7.0, device=dev, dtype=dt)           # rows past M must stay untouched
    ops.dense_gemm(x, w, b, gelu=gelu, out=out[:M])
    ref = torch.nn.functional.linear(x.float(), w.float(), b)
    lib = torch.nn.functional.linear(x, w)
    if gelu:
        ref = torch.nn.functional.gelu(ref)
        ops.bias_gelu(lib, b)
    else:
        lib = (lib.float() + b).to(dt)
    tol = 2e-2 if dt == torch.bfloat16 else 3e-3                     # one 16-bit ulp of values up to ~4
    e_own = ((out[:M].float() - ref).abs() / (1 + ref.abs())).max().item()
    e_lib = ((lib.float() - ref).abs() / (1 + ref.abs())).max().item()
    print(f"dense_gemm {dt} M={M} N={N} K={K} gelu={gelu}: rel err own {e_own:.3e}, library path {e_lib:.3e}")
    assert e_own < tol and e_own <= 1.5 * e_lib + 1e-3
    assert (out[M:] == 7.0).all()
