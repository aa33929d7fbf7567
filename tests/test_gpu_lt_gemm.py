"""psg_lt_gemm: the prompt pass's library product called natively with a pinned algorithm (`-m gpu`, plus one CPU twin).

The product is y = a . w^T with fp16 operands and fp32 accumulation in SOME order (the library's kernel decides which).  The
operands here are exact fp16 values and every fp16 x fp16 product is exact in fp32, so the only error is that of summing K'
terms in fp32: for any order, |y - y64| <= gamma_{K'-1} (|a| . |w|^T) with gamma_n = n u / (1 - n u), u = 2^-24 (Higham,
Accuracy and Stability of Numerical Algorithms, eq. 3.5; fused multiply-adds only lower it), and one more u for the
reference's own rounding to fp64 and the comparison - bounded here by (K' + 1) u (|a| . |w|^T) per element.  Nothing in the
bound is tuned; the CPU twin shows torch's own fp32 matmul of the same operands stays inside it, i.e. it is not vacuous."""
import pytest
import torch

U = 2.0 ** -24
SHAPES = [(48, 384, 768), (20, 256, 1536)]                      # (rows, N, K'): rows off every tile; the last layer's row count
WS_BYTES = 32 << 20


def _operands(rows, N, K, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((rows, K), generator=g).half()
    w = (torch.randn((N, K), generator=g) * 0.05).half()
    return a.to(device), w.to(device)


def _ref_and_bound(a, w):
    a64, w64 = a.double(), w.double()
    return a64 @ w64.t(), (a.shape[-1] + 1) * U * (a64.abs() @ w64.abs().t())


def _assert_within(y, a, w, what=""):
    y64, bound = _ref_and_bound(a, w)
    err = (y.double() - y64).abs()
    worst = (err / bound).max().item()
    print(f"{what}: max |y - y64| / bound = {worst:.4f} (max err {err.max().item():.3e})")
    assert torch.isfinite(y).all() and worst <= 1.0, (what, worst)


@pytest.mark.parametrize("rows,N,K", SHAPES)
def test_cpu_fp32_matmul_stays_inside_the_derived_bound(rows, N, K):
    a, w = _operands(rows, N, K, seed=rows + K)
    y64, bound = _ref_and_bound(a, w)
    err = ((a.float() @ w.float().t()).double() - y64).abs()
    assert (err <= bound).all()
    assert err.max() > 0 and (bound > 0).all()                  # a real rounding error under a real bound


def _gpu():
    from openpsg_amd import ops
    dev = torch.device("cuda:0")
    assert ops.lt_gemm_version(dev) is not None, ops.lt_gemm_error(dev)
    return ops, dev, torch.empty(WS_BYTES, device=dev, dtype=torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,N,K", SHAPES)
def test_first_choice_against_float64(rows, N, K):
    ops, dev, ws = _gpu()
    a, w = _operands(rows, N, K, seed=rows + K, device=dev)
    y = torch.full((rows, N), float("nan"), device=dev)
    assert ops.lt_gemm(a, w, y, -1, ws) is False
    _assert_within(y, a, w, f"first choice {rows}x{N}x{K}")


@pytest.mark.gpu
def test_column_part_of_a_wider_output_leaves_the_rest_untouched():
    ops, dev, ws = _gpu()
    rows, N, K = SHAPES[0]
    a, w = _operands(rows, N, K, seed=rows + K, device=dev)
    wide = torch.full((rows, 2 * N), 7.25, device=dev)
    assert ops.lt_gemm(a, w, wide[:, N:], -1, ws) is False      # ldy = 2 N
    assert (wide[:, :N] == 7.25).all()
    _assert_within(wide[:, N:], a, w, "right half")


@pytest.mark.gpu
def test_every_listed_candidate_is_the_same_product():
    ops, dev, ws = _gpu()
    rows, N, K = SHAPES[0]
    a, w = _operands(rows, N, K, seed=rows + K, device=dev)
    cands = ops.lt_gemm_candidates(a, w, max_ws_bytes=WS_BYTES)
    print(f"{len(cands)} candidates: {cands}")
    assert len(cands) >= 2 and len({i for i, _ in cands}) == len(cands)
    for index, need in cands:
        assert 0 <= need <= WS_BYTES
        y = torch.full((rows, N), float("nan"), device=dev)
        assert ops.lt_gemm(a, w, y, index, ws) is False, index
        _assert_within(y, a, w, f"solution {index}")


@pytest.mark.gpu
def test_batched_k_segments_equal_the_separate_calls():
    ops, dev, ws = _gpu()
    rows, N, K = SHAPES[1]
    P, Ks = 6, K // 6
    a, w = _operands(rows, N, K, seed=rows + K, device=dev)
    ab, wb = a.view(rows, P, Ks).permute(1, 0, 2), w.view(N, P, Ks).permute(1, 0, 2)
    # the same solution for both forms (a pinned index, where the two candidate lists share one; else the first choices)
    single = [i for i, _ in ops.lt_gemm_candidates(ab[0], wb[0], max_ws_bytes=WS_BYTES)]
    index = next((i for i, _ in ops.lt_gemm_candidates(ab, wb, max_ws_bytes=WS_BYTES) if i in single), -1)
    yb = torch.full((P, rows, N), float("nan"), device=dev)
    assert ops.lt_gemm(ab, wb, yb, index, ws) is False
    for p in range(P):
        y = torch.full((rows, N), float("nan"), device=dev)
        assert ops.lt_gemm(ab[p], wb[p], y, index, ws) is False
        assert torch.equal(y, yb[p]), (p, index)
    _assert_within(yb.sum(0), a, w, f"sum of {P} slices (solution {index})")


@pytest.mark.gpu
def test_unknown_index_and_stale_table_line_fall_back_visibly():
    from openpsg_amd import llm
    ops, dev, ws = _gpu()
    rows, N, K = SHAPES[0]
    a, w = _operands(rows, N, K, seed=rows + K, device=dev)
    cands = ops.lt_gemm_candidates(a, w, max_ws_bytes=WS_BYTES)
    bogus = max(i for i, _ in cands) + 100003
    y = torch.full((rows, N), float("nan"), device=dev)
    assert ops.lt_gemm(a, w, y, bogus, ws) is True              # the out-flag
    _assert_within(y, a, w, "fallback")
    first = torch.empty_like(y)
    ops.lt_gemm(a, w, first, -1, ws)
    assert torch.equal(y, first)                                # ... and what ran IS the first choice
    version = ops.lt_gemm_version(dev)
    route = llm._LtRoute(dev, {(N, K, 3, False): [(1, 64, bogus, version, ("whole",), WS_BYTES)]})
    plan = route.plan(rows, N, K, 3, False)
    assert plan is not None and route.pinned == (1, "")
    _assert_within(llm._split_mm(a, w, plan), a, w, "route fallback")
    n, why = route.pinned
    assert n == 1 and str(bogus) in why and "first choice" in why
    stale = llm._LtRoute(dev, {(N, K, 3, False): [(1, 64, cands[0][0], version + 1, ("whole",), 0)]})
    assert stale.plan(rows, N, K, 3, False) is None             # the shape keeps its torch.mm route
    n, why = stale.pinned
    assert n == 0 and str(version + 1) in why and "another library version" in why


@pytest.mark.gpu
def test_capturable_and_replays_bit_equal_to_eager():
    ops, dev, ws = _gpu()
    rows, N, K = SHAPES[0]
    a, w = _operands(rows, N, K, seed=1, device=dev)
    index = ops.lt_gemm_candidates(a, w, max_ws_bytes=WS_BYTES)[1][0]
    sa, sw, sy = a.clone(), w.clone(), torch.zeros((rows, N), device=dev)
    ops.lt_gemm(sa, sw, sy, index, ws)                          # the problem's descriptors are built outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.lt_gemm(sa, sw, sy, index, ws)
    for seed in (2, 3):
        a2, w2 = _operands(rows, N, K, seed=seed, device=dev)
        eager = torch.empty((rows, N), device=dev)
        ops.lt_gemm(a2, w2, eager, index, ws)
        sa.copy_(a2)
        sw.copy_(w2)
        sy.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(sy, eager), seed
        _assert_within(sy, a2, w2, f"replay seed {seed}")


@pytest.mark.gpu
def test_engine_on_a_pinned_non_default_candidate(monkeypatch):
    """A 2-layer, 256-wide fp32s engine, prompt pass of 20 pairs x 48 rows, with the table line of the LAST layer's down
    projection (20 kept rows, N = 256, K' = 3 x 512) forced onto the library's second candidate, against the torch.mm
    route.  That product's operands are bit-identical in both routes, so each route's result is within the bound B of the
    module docstring and the two differ by at most 2 B; the final RMSNorm and the lm_head carry that to the logits, to first
    order: with x = resid + delta, E = 2 B |row scale x column scale|, r = sqrt(mean x^2 + eps),
        |d n_i| <= |g_i| (E_i / r + |x_i| sum_j |x_j| E_j / (D r^3)),   |d logit| <= |W| |d n|,
    plus the two routes' own rounding in those two fp32 kernels on their (different) inputs, 2 (D + 8) u |W| |n| (D
    accumulations per logit, a handful of roundings per element of n)."""
    from openpsg_amd import llm
    from openpsg_amd.config import LlamaConfig, PSGConfig, QFormerConfig
    from openpsg_amd.weights import make_weights_device
    ops, dev, _ = _gpu()
    D, inter, K_pairs, Tp = 256, 512, 20, 16
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=LlamaConfig(hidden=D, heads=2, layers=2, inter=inter, vocab=512),
                    max_object_num=8)
    wts = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32)
    eng = llm.LlamaDecodeEngine(wts, cfg, dev, torch.float32, prefill_split=True)
    eng.use_graph = False                                       # eager: the recorders below see live tensors
    gen = torch.Generator(device=dev).manual_seed(3)
    X = torch.randn((K_pairs, 32 + Tp, D), device=dev, generator=gen)
    plen = torch.randint(9, Tp + 1, (K_pairs,), device=dev, generator=gen, dtype=torch.int32)
    key, shape = (D, 3 * inter, 3, True), (torch.empty((K_pairs, 3 * inter), device=dev, dtype=torch.float16),
                                           torch.empty((D, 3 * inter), device=dev, dtype=torch.float16))
    cands = ops.lt_gemm_candidates(*shape, max_ws_bytes=WS_BYTES)
    assert len(cands) >= 2
    index, need = cands[1]
    table = {key: [(K_pairs, K_pairs + 1, index, ops.lt_gemm_version(dev), ("whole",), need)]}

    rec = {}
    real_mm, real_scale, real_norm = llm._split_mm, ops.scale_rows_cols, ops.rmsnorm

    def mm(a3, w3, plan=None, out_dtype=torch.float32):
        y = real_mm(a3, w3, plan, out_dtype)
        if tuple(a3.shape) == (K_pairs, 3 * inter):
            rec["mm"] = (a3.clone(), w3, plan, y.clone())
        return y

    def scale(y, row_scale, col_scale):
        if tuple(y.shape) == (K_pairs, D):
            rec["scales"] = (row_scale.clone(), col_scale.clone())
        return real_scale(y, row_scale, col_scale)

    def norm(resid, delta, *args, **kw):
        if delta is not None and tuple(resid.shape) == (K_pairs, D) and "norm" not in rec:
            rec["norm"] = (resid.clone(), delta.clone())
        return real_norm(resid, delta, *args, **kw)

    monkeypatch.setattr(llm, "_split_mm", mm)
    monkeypatch.setattr(ops, "scale_rows_cols", scale)
    monkeypatch.setattr(ops, "rmsnorm", norm)
    runs = {}
    for name, tab in (("mm", {}), ("lt", table)):
        eng._lt = llm._LtRoute(dev, tab)
        rec.clear()
        tokens, logits = eng.generate(X, plen, max_new_tokens=1, return_first_logits=True)
        torch.cuda.synchronize()
        runs[name] = (tokens.clone(), logits.clone(), dict(rec), eng.lt_gemm_pinned)
    (tok_m, log_m, rec_m, pin_m), (tok_l, log_l, rec_l, pin_l) = runs["mm"], runs["lt"]
    assert pin_m == (0, "") and pin_l == (1, ""), (pin_m, pin_l)
    assert rec_m["mm"][2][0] != "lt" and rec_l["mm"][2][0] == "lt" and rec_l["mm"][2][1] == index
    a3, w3 = rec_m["mm"][0], rec_m["mm"][1]
    assert torch.equal(a3, rec_l["mm"][0]) and torch.equal(rec_m["norm"][0], rec_l["norm"][0])   # same inputs, bit for bit
    for r in (rec_m, rec_l):
        y = r["mm"][3]
        _assert_within(y if y.dim() == 2 else y.sum(0), a3, w3, "last-layer down")
    _, B = _ref_and_bound(a3, w3)
    row, col = rec_m["scales"]
    E = 2 * B * (row.double().abs()[:, None] * col.double().abs()[None, :])
    x = rec_m["norm"][0].double() + rec_m["norm"][1].double()
    g, W = eng.final_norm.double(), eng.lm_head.double()
    r = (x.pow(2).mean(1, keepdim=True) + cfg.llm.rms_eps).sqrt()
    dn = g.abs() * (E / r + x.abs() * (x.abs() * E).sum(1, keepdim=True) / (D * r ** 3))
    n = g * x / r
    bound = dn @ W.abs().t() + 2 * (D + 8) * U * (n.abs() @ W.abs().t())
    diff = (log_l.double() - log_m.double()).abs()
    print(f"engine: max |logits_lt - logits_mm| = {diff.max().item():.3e}, / bound = {(diff / bound).max().item():.4f}, "
          f"bit-equal: {torch.equal(log_l, log_m)}")
    assert (diff <= bound).all()
    assert torch.equal(tok_l, tok_m)
