"""The grouped-query attention entry points (`-m gpu`) against the float64 restatement of tests/gqa_ref.py and against
their multi-head counterparts on the cache expanded to MHA: psg_decode_attn_gqa (every workgroup split of a group),
psg_rope_kvwrite_gqa, psg_rope_kvwrite_scaled_gqa, psg_llm_attn_gqa, psg_prefill_attn_gqa, psg_prefill_attn_rope_gqa.
Caches are filled with NaN past the written slots: a kernel reading them, or writing anywhere but slot `pos` of its
own key / value head, fails the bitwise checks."""
import pytest
import torch

from tests import gqa_ref as R
from tests import llm_attn_ref as L

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"fp32": 2e-5, "fp16": 4e-3, "bf16": 3e-2}           # |out - float64| over outputs of magnitude <= ~3
CTXS = [1, 15, 16, 63, 64, 65, 130]                         # cached keys before the new token


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _decode_case(dtype, heads, kvh, seed):
    """Rows with the context lengths of CTXS plus one padding row; pair = row (shuffled); NaN past each row's slot."""
    g = torch.Generator().manual_seed(seed)
    dt = DT[dtype]
    rows = len(CTXS) + 1
    ctx = max(CTXS) + 6
    W = (heads + 2 * kvh) * 128
    qkv = (torch.randn(rows, W, generator=g) * 1.5).to(dt)
    pos = torch.tensor(CTXS + [-1], dtype=torch.int32)
    pair = torch.randperm(rows, generator=g).to(torch.int32)
    kc = torch.full((rows, kvh, ctx, 128), float("nan"))
    vc = torch.full((rows, kvh, ctx, 128), float("nan"))
    for r in range(rows):
        n = int(pos[r])
        if n > 0:
            kc[int(pair[r]), :, :n] = torch.randn(kvh, n, 128, generator=g) * 1.5
            vc[int(pair[r]), :, :n] = torch.randn(kvh, n, 128, generator=g)
    return qkv, pos, pair, kc.to(dt), vc.to(dt), ctx


def _decode_ref(qkv, pos, pair, kc, vc, heads, kvh, cos, sin, dt):
    """Float64 decode step; the rotated q / k are rounded to the stored dtype as the kernels do."""
    q, k, v = R.split_qkv(qkv.double(), heads, kvh)
    p = pos.clamp(min=0).long()
    qr = R.rope64(q, p, cos, sin).to(dt).double()
    kr = R.rope64(k, p, cos, sin).to(dt).double()
    kc64, vc64 = kc.double().clone(), vc.double().clone()
    for r in range(qkv.shape[0]):
        if pos[r] >= 0:
            kc64[int(pair[r]), :, int(pos[r])] = kr[r]
            vc64[int(pair[r]), :, int(pos[r])] = v[r]
    return R.attend64(qr, kc64, vc64, pair, pos.long() + 1), kr, v


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("splits", [0, 2, 4])
def test_decode_attn_gqa_vs_float64_and_mha(dtype, G, splits):
    from openpsg_amd import _lib, ops
    heads = 16
    kvh = heads // G
    dt = DT[dtype]
    qkv, pos, pair, kc, vc, ctx = _decode_case(dtype, heads, kvh, seed=100 * G + splits)
    cos, sin = R.rope_tables(ctx)
    want, kr, v = _decode_ref(qkv, pos, pair, kc, vc, heads, kvh, cos, sin, dt)
    if splits:                                              # split-K partials whose fp32 sum is the projection
        g = torch.Generator().manual_seed(splits)
        parts = torch.randn(splits, *qkv.shape, generator=g) * 0.25
        parts[-1] = qkv.float() - parts[:-1].sum(0)
        qin = parts
        want_in = parts.sum(0).to(dt)                       # what the kernel sums (fp32, then rounded to dt)
        want, kr, v = _decode_ref(want_in, pos, pair, kc, vc, heads, kvh, cos, sin, dt)
    dev = "cuda"
    rope = (cos.to(dev), sin.to(dev))
    old = _lib.get_option(0, "decode_gqa_qparts")
    try:
        for qparts in (0, 1, 2, 4, 8):
            if qparts > G:
                continue
            _lib.set_option(0, "decode_gqa_qparts", qparts)
            kd, vd = kc.to(dev), vc.to(dev)
            out = torch.zeros(qkv.shape[0], heads * 128, device=dev, dtype=dt)
            x = ops.Partials(qin.to(dev).contiguous()) if splits else qkv.to(dev)
            ops.decode_attn(x, pair.to(dev), pos.to(dev), rope, heads, 128, ctx, kd, vd, out, kv_heads=kvh)
            torch.cuda.synchronize()
            got = out.cpu()
            valid = pos >= 0
            err = (got[valid].double() - want[valid]).abs().max().item()
            assert err <= TOL[dtype], f"qparts={qparts}: max |out - float64| = {err:.3e}"
            assert bool((got[~valid] == 0).all()), "a padding row's output was written"
            # the new K / V rows land in slot pos of their KV head; every other slot keeps its bits (NaN included)
            kw, vw = kc.clone(), vc.clone()
            for r in range(qkv.shape[0]):
                if pos[r] >= 0:
                    kw[int(pair[r]), :, int(pos[r])] = kd.cpu()[int(pair[r]), :, int(pos[r])]
                    vw[int(pair[r]), :, int(pos[r])] = vd.cpu()[int(pair[r]), :, int(pos[r])]
                    kerr = (kd.cpu()[int(pair[r]), :, int(pos[r])].double() - kr[r]).abs().max().item()
                    assert kerr <= {"fp32": 1e-6, "fp16": 8e-3, "bf16": 6e-2}[dtype], f"appended key differs by {kerr:.3e}"
                    verr = (vd.cpu()[int(pair[r]), :, int(pos[r])].double() - v[r].to(dt).double()).abs().max().item()
                    assert verr <= {"fp32": 1e-6, "fp16": 8e-3, "bf16": 6e-2}[dtype], f"appended value differs by {verr:.3e}"
            assert torch.equal(_bits(kd.cpu()), _bits(kw)) and torch.equal(_bits(vd.cpu()), _bits(vw)), \
                "a cache slot other than pos changed"
            if dtype == "fp32" and qparts == 0:
                # the multi-head kernel on the same step expanded to MHA: same per-head arithmetic
                def to_mha(t):                              # [rows, (heads + 2 kvh) 128] -> [rows, 3 heads 128]
                    a, b, c = R.split_qkv(t, heads, kvh)
                    r_ = t.shape[0]
                    return torch.cat([a.reshape(r_, -1), b.repeat_interleave(G, 1).reshape(r_, -1),
                                      c.repeat_interleave(G, 1).reshape(r_, -1)], 1)
                if splits:
                    xm = ops.Partials(torch.stack([to_mha(p_) for p_ in qin]).to(dev).contiguous())
                else:
                    xm = to_mha(qkv).to(dev)
                km, vm = kc.repeat_interleave(G, 1).to(dev), vc.repeat_interleave(G, 1).to(dev)
                om = torch.zeros_like(out)
                ops.decode_attn(xm, pair.to(dev), pos.to(dev), rope, heads, 128, ctx, km, vm, om)
                torch.cuda.synchronize()
                rel = ((om.cpu() - got).abs() / om.cpu().abs().clamp(min=1e-3))[valid].max().item()
                assert rel <= 1e-6, f"GQA vs MHA kernel on the expanded cache: relative {rel:.3e}"
    finally:
        _lib.set_option(0, "decode_gqa_qparts", old)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_rope_kvwrite_and_llm_attn_gqa(dtype, G):
    """Prompt pass of fp32 / long prompts: psg_rope_kvwrite_gqa (+ split-K input) then psg_llm_attn_gqa."""
    from openpsg_amd import ops
    heads, kvh, dt, dev = 8, 8 // G, DT[dtype], "cuda"
    g = torch.Generator().manual_seed(G)
    pairs, S = 3, 70
    lens = [70, 41, 1]
    rows = pairs * S
    ctx = S + 4
    W = (heads + 2 * kvh) * 128
    qkv = (torch.randn(rows, W, generator=g) * 1.5).to(dt)
    tok_pos = torch.tensor([t if t < lens[p] else -1 for p in range(pairs) for t in range(S)], dtype=torch.int32)
    tok_pair = torch.arange(pairs, dtype=torch.int32).repeat_interleave(S)
    cos, sin = R.rope_tables(ctx)
    rope = (cos.to(dev), sin.to(dev))
    for splits in (0, 3):
        kc = torch.full((pairs, kvh, ctx, 128), float("nan"), dtype=dt, device=dev)
        vc = torch.full_like(kc, float("nan"))
        q = torch.zeros(rows, heads * 128, dtype=dt, device=dev)
        if splits:
            parts = torch.randn(splits, rows, W, generator=g) * 0.25
            parts[-1] = qkv.float() - parts[:-1].sum(0)
            src = parts.sum(0).to(dt)
            x = ops.Partials(parts.to(dev).contiguous())
        else:
            src, x = qkv, qkv.to(dev)
        ops.rope_kvwrite(x, tok_pair.to(dev), tok_pos.to(dev), rope, heads, 128, ctx, q, kc, vc, kv_heads=kvh)
        torch.cuda.synchronize()
        qs, ks, vs = R.split_qkv(src.double(), heads, kvh)
        p = tok_pos.clamp(min=0).long()
        valid = tok_pos >= 0
        tol = 1e-6 if dtype == "fp32" else (8e-3 if dtype == "fp16" else 6e-2)
        qw = R.rope64(qs, p, cos, sin)
        assert (q.cpu().double().view(rows, heads, 128)[valid] - qw[valid]).abs().max().item() <= tol
        kw = R.rope64(ks, p, cos, sin)
        kcc, vcc = kc.cpu(), vc.cpu()
        for r in range(rows):
            pp, t = int(tok_pair[r]), int(tok_pos[r])
            if t >= 0:
                assert (kcc[pp, :, t].double() - kw[r]).abs().max().item() <= tol
                assert torch.equal(vcc[pp, :, t], vs[r].to(dt))
        for pp in range(pairs):                              # slots past a pair's tokens: untouched
            assert bool(torch.isnan(kcc[pp, :, lens[pp]:].float()).all()) and bool(torch.isnan(vcc[pp, :, lens[pp]:].float()).all())
        out = torch.zeros_like(q)
        ops.llm_attn(q, kc, vc, tok_pair.to(dev), tok_pos.to(dev), heads, 128, ctx, out, kv_heads=kvh)
        torch.cuda.synchronize()
        want = R.attend64(q.cpu().double().view(rows, heads, 128), kcc.double(), vcc.double(), tok_pair, tok_pos.long() + 1)
        err = (out.cpu().double()[valid] - want[valid]).abs().max().item()
        assert err <= TOL[dtype], f"llm_attn_gqa splits={splits}: {err:.3e}"
        assert bool((out.cpu()[~valid] == 0).all())
        # and inside the derived bound of tests/llm_attn_ref.py (the scalar kernel keeps its probabilities in fp32)
        r64, A, gx, n = L.prefix64(q.cpu(), kcc, vcc, tok_pair, tok_pos, heads)
        L.check(f"llm_attn_gqa splits={splits}", out.cpu(), r64, L.attn_bound(r64, A, gx, n, dt))


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_prefill_attn_gqa_and_rope_form(dtype, G):
    """Pair-major prompt batch (<= 64 rows per pair): psg_prefill_attn_gqa on the cache psg_rope_kvwrite_gqa wrote, the
    fused psg_prefill_attn_rope_gqa (16-bit) against it, and psg_rope_kvwrite_scaled_gqa (fp32) against the plain form."""
    from openpsg_amd import ops
    heads, kvh, dt, dev = 8, 8 // G, DT[dtype], "cuda"
    g = torch.Generator().manual_seed(10 + G)
    S, lens = 50, [50, 33, 64 - 14, 1]
    pairs = len(lens)
    rows, ctx = pairs * S, S + 16
    W = (heads + 2 * kvh) * 128
    qkv = (torch.randn(rows, W, generator=g) * 1.5).to(dt)
    tok_pos = torch.tensor([t if t < lens[p] else -1 for p in range(pairs) for t in range(S)], dtype=torch.int32)
    tok_pair = torch.arange(pairs, dtype=torch.int32).repeat_interleave(S)
    cos, sin = R.rope_tables(ctx)
    rope = (cos.to(dev), sin.to(dev))
    valid = tok_pos >= 0
    kc = torch.full((pairs, kvh, ctx, 128), float("nan"), dtype=dt, device=dev)
    vc = torch.full_like(kc, float("nan"))
    q = torch.zeros(rows, heads * 128, dtype=dt, device=dev)
    ops.rope_kvwrite(qkv.to(dev), tok_pair.to(dev), tok_pos.to(dev), rope, heads, 128, ctx, q, kc, vc, kv_heads=kvh)
    out = torch.zeros_like(q)
    ops.prefill_attn(q, kc, vc, tok_pos.to(dev), pairs, S, heads, 128, ctx, out, kv_heads=kvh)
    torch.cuda.synchronize()
    want = R.attend64(q.cpu().double().view(rows, heads, 128), kc.cpu().double(), vc.cpu().double(), tok_pair,
                      tok_pos.long() + 1)
    err = (out.cpu().double()[valid] - want[valid]).abs().max().item()
    assert err <= TOL[dtype], f"prefill_attn_gqa: {err:.3e}"
    assert bool((out.cpu()[~valid] == 0).all())
    # and inside the derived bound of tests/llm_attn_ref.py (the 16-bit matrix-core kernel rounds its probabilities: + u A)
    r64, A, gx, n, sv = L.causal64(q.cpu(), kc.cpu(), vc.cpu(), tok_pos, pairs, S, heads, sum_v=True)
    L.check("prefill_attn_gqa", out.cpu(), r64, L.attn_bound(r64, A, gx, n, dt, p_rounded=dtype != "fp32", sum_v=sv))
    if dtype != "fp32":
        kc2 = torch.full_like(kc, float("nan"))
        vc2 = torch.full_like(kc, float("nan"))
        out2 = torch.zeros_like(q)
        ops.prefill_attn_rope(qkv.to(dev), tok_pos.to(dev), rope, pairs, S, heads, 128, ctx, kc2, vc2, out2, kv_heads=kvh)
        torch.cuda.synchronize()
        err2 = (out2.cpu().double()[valid] - want[valid]).abs().max().item()
        assert err2 <= TOL[dtype], f"prefill_attn_rope_gqa: {err2:.3e}"
        assert torch.equal(_bits(vc2.cpu()), _bits(vc.cpu())), "fused form wrote other V rows than the plain form"
        # rotated keys: the fused form rotates in a slightly different operation order; values within 1 ulp
        kk, kk2 = kc.cpu().float(), kc2.cpu().float()
        same_nan = torch.equal(torch.isnan(kk), torch.isnan(kk2))
        fin = ~torch.isnan(kk)
        assert same_nan and (kk[fin] - kk2[fin]).abs().max().item() <= 2 * TOL[dtype]
    else:
        # the fp32s prompt pass: a raw product with its power-of-two scales, read by psg_rope_kvwrite_scaled_gqa
        rs = torch.exp2(torch.randint(-3, 4, (rows,), generator=g).float())
        cs = torch.exp2(torch.randint(-3, 4, (W,), generator=g).float())
        y = (qkv / (rs[:, None] * cs[None, :])).contiguous()
        kc3 = torch.full_like(kc, float("nan"))
        vc3 = torch.full_like(kc, float("nan"))
        q3 = torch.zeros_like(q)
        ops.rope_kvwrite_scaled(ops.Scaled(y.to(dev), rs.to(dev), cs.to(dev)), tok_pair.to(dev), tok_pos.to(dev), rope,
                                heads, 128, ctx, q3, kc3, vc3, kv_heads=kvh)
        torch.cuda.synchronize()
        assert torch.equal(_bits(kc3.cpu()), _bits(kc.cpu())) and torch.equal(_bits(vc3.cpu()), _bits(vc.cpu()))
        assert torch.equal(q3.cpu()[valid], q.cpu()[valid])


def test_gqa_entry_points_refuse_bad_groups():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    dev = "cuda"
    cos, sin = R.rope_tables(8)
    x = torch.zeros(2, (6 + 2 * 2) * 128, device=dev)
    kc = torch.zeros(2, 2, 8, 128, device=dev)
    with pytest.raises(PsgHipError, match="kv_heads"):            # 6 / 2 = 3: not a power of two
        ops.decode_attn(x, torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
                        (cos.to(dev), sin.to(dev)), 6, 128, 8, kc, kc.clone(), torch.zeros(2, 768, device=dev), kv_heads=2)
