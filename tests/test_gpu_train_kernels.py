"""The training kernels of csrc/psg_train_bwd.hip, one at a time, against float64 references (`-m gpu`).

tests/test_gpu_train.py checks them only end to end (70 parameter gradients of a whole training step at 2e-3 relative):
a wrong term whose share of a parameter gradient is small - the dropout scale on dv, the dk / dv sums over sequences that
share keys - passes there.  Here every `train_graph` Function is driven through `torch.autograd.grad` with a random
upstream gradient, and its forward output and every input gradient are compared with float64 autograd of the plain
formula, at the shapes the kernels were written around (64-key lane chunks, the 1024-key limit, D between 64 and 128,
rows that leave waves of a block empty, masked and fully dropped rows, ignore_index rows, narrow vocabularies).

Tolerances are fp32 error bounds scaled to the operands, never a number fitted to one run: a reduction of n terms in the
kernel's association (a lane's serial sum, then a 64-lane butterfly) is allowed RED(n) * 2^-24 * sum|terms|, where
RED(n) = ceil(n / lanes) + log2(lanes) levels; sums whose order is unknown (atomics) are allowed n * 2^-24 * sum|terms|.
`_check` reports err / bound, so a passing run shows how much headroom each bound has.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                       # unit round-off of fp32
TINY = 2.0 ** -126                     # smallest normal fp32: the size of what an underflowing term can lose
F32MIN = torch.finfo(torch.float32).min


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _red(n, lanes=64):
    """error-bound length of a kernel reduction over n terms: ceil(n / lanes) serial adds per lane, then the tree"""
    return math.ceil(n / lanes) + int(math.log2(lanes))


def _check(name, got, ref, bound):
    """|got - ref| <= bound element-wise (got: the kernel's fp32, ref / bound: float64)"""
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    assert ratio <= 1.0, (f"{name}: max err / bound = {ratio:.3g} (max err {err.max().item():.3g}, "
                          f"at {tuple(int(i) for i in torch.nonzero(err > bound)[0])})")
    return ratio


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------
def _ln_case(x, eps, seed, dev):
    """LayerNormFn forward + backward against float64 autograd; bounds from the kernel's two-pass arithmetic."""
    from openpsg_amd import train_graph as G
    g = _gen(seed)
    rows, n = x.shape
    gamma = (1 + 0.5 * torch.randn(n, generator=g)).to(dev)
    beta = torch.randn(n, generator=g).to(dev)
    dy = torch.randn(rows, n, generator=g).to(dev)
    xg, gg, bg = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = G.LayerNormFn.apply(xg, gg, bg, eps)
    dx, dgam, dbet = torch.autograd.grad(y, (xg, gg, bg), dy)

    x64, g64, b64, dy64 = (t.double().requires_grad_(True) for t in (x, gamma, beta, dy))
    y64 = F.layer_norm(x64, (n,), g64, b64, eps)
    rdx, rdg, rdb = torch.autograd.grad(y64, (x64, g64, b64), dy64)
    with torch.no_grad():
        xd, gd, bd, dyd = x64.detach(), g64.detach(), b64.detach(), dy64.detach()
        mu = xd.mean(-1, keepdim=True)
        var = ((xd - mu) ** 2).mean(-1, keepdim=True)
        rs = 1.0 / torch.sqrt(var + eps)
        xh = (xd - mu) * rs
        r = _red(n)
        e_mu = r * EPS * xd.abs().mean(-1, keepdim=True)                  # the mean: one reduction of |x|
        e_rs = (r + 6) * EPS                                                # relative: variance sum, divide, sqrt, rcp
        e_xh = e_mu * rs + xh.abs() * (e_rs + 2 * EPS)
        by = 2 * (gd.abs() * e_xh + EPS * ((xh * gd).abs() + bd.abs()))
        gy = dyd * gd
        a, b = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
        e_a = r * EPS * gy.abs().mean(-1, keepdim=True)
        e_b = r * EPS * (gy * xh).abs().mean(-1, keepdim=True) + (gy.abs() * e_xh).mean(-1, keepdim=True)
        bdx = 2 * (rs * (e_a + e_xh * b.abs() + xh.abs() * e_b + 3 * EPS * (gy.abs() + a.abs() + (xh * b).abs()))
                   + e_rs * rdx.abs())
        bdg = 2 * ((dyd.abs() * e_xh).sum(0) + rows * EPS * (dyd * xh).abs().sum(0))
        bdb = 2 * rows * EPS * dyd.abs().sum(0)
    return [_check("layernorm y", y, y64.detach(), by), _check("layernorm dx", dx, rdx, bdx),
            _check("layernorm dgamma", dgam, rdg, bdg), _check("layernorm dbeta", dbet, rdb, bdb)]


@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("rows", [1, 3, 5, 257, 33 * 32])
@pytest.mark.parametrize("hidden", [1, 63, 65, 100, 768, 4096])
def test_layernorm_fwd_bwd_vs_float64(hidden, rows, eps):
    """rows 1 / 3 / 5 / 257 leave waves of the last 4-wave block idle; 33 x 32 rows make dgamma / dbeta sums of 1056
    atomics; hidden 1 (a zero variance), 63 / 65 / 100 (partial 64-lane chunks), 768, 4096."""
    dev = _dev()
    x = torch.randn(rows, hidden, generator=_gen(hidden * 7919 + rows)).to(dev)
    print(f"layernorm hidden={hidden} rows={rows} eps={eps}: err/bound",
          ["%.3f" % r for r in _ln_case(x, eps, hidden + rows, dev)])


@pytest.mark.parametrize("hidden", [768, 4096])
def test_layernorm_large_common_offset(hidden):
    """Rows of mean 1e3 and standard deviation 1e-2: a one-pass variance (E[x^2] - mean^2) loses every digit here, the
    kernel's two-pass one does not.  The bound is still the fp32 one; it is wide because the mean itself carries
    ~2^-24 * 1e3 of error, which is 1e5 x larger in units of the row's deviation."""
    dev = _dev()
    g = _gen(hidden)
    x = (1e3 + 1e-2 * torch.randn(37, hidden, generator=g)).to(dev)
    ratios = _ln_case(x, 1e-12, hidden + 1, dev)
    print(f"layernorm offset 1e3 +- 1e-2, hidden={hidden}: err/bound", ["%.3f" % r for r in ratios])
    # and the bound is far below what a lost variance would cost: y is O(1)
    from openpsg_amd import train_graph as G
    y = G.LayerNormFn.apply(x, torch.ones(hidden, device=dev), torch.zeros(hidden, device=dev), 1e-12)
    ref = F.layer_norm(x.double(), (hidden,), eps=1e-12)
    assert (y.double() - ref).abs().max().item() < 0.05


# ---- RMSNorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 31, 64, 65])
@pytest.mark.parametrize("hidden", [100, 4096])
def test_rmsnorm_fwd_bwd_vs_float64(hidden, rows):
    """HF-LL:53-67 with the FROZEN weight of the training branch: dx against float64 autograd, and no weight gradient."""
    from openpsg_amd import train_graph as G
    dev = _dev()
    g = _gen(hidden * 131 + rows)
    eps = 1e-6
    x = torch.randn(rows, hidden, generator=g).to(dev)
    w = (1 + 0.5 * torch.randn(hidden, generator=g)).to(dev)
    dy = torch.randn(rows, hidden, generator=g).to(dev)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = G.RMSNormFn.apply(xg, wg, eps)
    dx, dw = torch.autograd.grad(y, (xg, wg), dy, allow_unused=True)
    assert dw is None or not dw.abs().any(), "the frozen RMSNorm weight received a gradient"

    x64 = x.double().requires_grad_(True)
    w64, dy64 = w.double(), dy.double()
    y64 = w64 * (x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + eps))
    rdx, = torch.autograd.grad(y64, x64, dy64)
    with torch.no_grad():
        xd = x64.detach()
        r = _red(hidden)
        rs = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps)
        e_rs = (r + 6) * EPS
        by = 2 * (e_rs + 3 * EPS) * y64.abs()
        gy = dy64 * w64
        a = (gy * xd).mean(-1, keepdim=True)
        e_a = r * EPS * (gy * xd).abs().mean(-1, keepdim=True)
        bdx = 2 * (rs * (3 * EPS * gy.abs() + xd.abs() * rs * rs * (e_a + (3 * e_rs + 3 * EPS) * a.abs())) + e_rs * rdx.abs())
    print(f"rmsnorm hidden={hidden} rows={rows}: err/bound y {_check('rmsnorm y', y, y64.detach(), by):.3f}, "
          f"dx {_check('rmsnorm dx', dx, rdx, bdx):.3f}")


# ---- attention ----------------------------------------------------------------------------------------------------
def _attn_inputs(B, Bk, Mq, H, Sq, Sk, D, seed, mask="random", drop=False):
    """fp32 q / k / v / dout and the uint8 keep (and dropout) masks of one case, on the GPU."""
    dev = _dev()
    g = _gen(seed)
    hid = H * D
    q = torch.randn(B, Sq, hid, generator=g).to(dev)
    k = torch.randn(Bk, Sk, hid, generator=g).to(dev)
    v = torch.randn(Bk, Sk, hid, generator=g).to(dev)
    dout = torch.randn(B, Sq, hid, generator=g).to(dev)
    keep = torch.rand(B, Mq, Sk, generator=g) < 0.7
    if mask == "one_key":                  # the same key masked for every query row
        keep = torch.ones(B, Mq, Sk, dtype=torch.bool)
        keep[:, :, Sk // 2] = False
    elif mask == "rows":                   # random keep, plus whole rows masked (uniform softmax)
        keep[0, -1] = False
        keep[B - 1, 0] = False
    elif mask == "none":
        keep = torch.ones(B, Mq, Sk, dtype=torch.bool)
    keep = keep.to(torch.uint8).to(dev)
    dmask = None
    if drop:
        dmask = torch.rand(B, H, Sq, Sk, generator=g) >= 0.1
        dmask[0, H - 1, Sq - 1] = False     # dropout removes every key of this row
        dmask = dmask.to(torch.uint8).to(dev)
    return q, k, v, dout, keep, dmask


def _attn_ref(q, k, v, dout, keep, dmask, dscale, H, scale):
    """float64 reference: softmax(q.k * scale + finfo(fp32).min on masked keys) [x dropout x 1/(1-p)] @ v, its autograd
    gradients, and fp32 error bounds of the forward output, the saved probabilities and dq / dk / dv."""
    B, Sq, hid = q.shape
    Bk, Sk, _ = k.shape
    D = hid // H
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    qh = q64.view(B, Sq, H, D).transpose(1, 2)                                   # [B, H, Sq, D]
    kh = k64.view(Bk, Sk, H, D).transpose(1, 2).expand(B, H, Sk, D)
    vh = v64.view(Bk, Sk, H, D).transpose(1, 2).expand(B, H, Sk, D)
    masked = (keep == 0)[:, None].expand(B, H, Sq, Sk)                           # Mq == 1 broadcasts over the rows
    s = (qh @ kh.transpose(-1, -2)) * scale + masked.double() * F32MIN
    p = torch.softmax(s, -1)
    df = torch.ones_like(p) if dmask is None else dmask.double() * dscale
    o = (p * df) @ vh
    out = o.transpose(1, 2).reshape(B, Sq, hid)
    do64 = dout.double()
    rdq, rdk, rdv = torch.autograd.grad(out, (q64, k64, v64), do64)
    with torch.no_grad():
        p, o = p.detach(), o.detach()
        qa, ka, va = qh.detach().abs(), kh.detach().abs(), vh.detach().abs()
        doh = do64.view(B, Sq, H, D).transpose(1, 2)
        es = D * EPS * scale * (qa @ ka.transpose(-1, -2))                       # error of one fp32 score
        es = es.masked_fill(masked, 0.0)                                         # masked scores: exactly finfo.min in both
        E = es.amax(-1, keepdim=True)
        bp = p * (2 * E + es + (_red(Sk) + 4) * EPS) + TINY                      # the saved p: softmax of perturbed scores
        pd = p * df
        bo = (bp * df) @ va + (Sk + 2) * EPS * (pd @ va)
        dP = (doh @ vh.detach().transpose(-1, -2)) * df
        e_dP = D * EPS * (doh.abs() @ va.transpose(-1, -2)) * df
        c = (p * dP).sum(-1, keepdim=True)
        e_c = (bp * dP.abs() + p * e_dP).sum(-1, keepdim=True) + _red(Sk) * EPS * (p * dP.abs()).sum(-1, keepdim=True)
        dS = p * (dP - c) * scale
        e_dS = scale * (bp * (dP - c).abs() + p * (e_dP + e_c) + 3 * EPS * p * (dP - c).abs())
        bdq = e_dS @ ka + (Sk + 2) * EPS * (dS.abs() @ ka)
        nsum = Sq * (B if Bk == 1 else 1)                                        # atomics into one key row
        bdk = e_dS.transpose(-1, -2) @ qa + (nsum + 2) * EPS * (dS.abs().transpose(-1, -2) @ qa)
        bdv = (bp * df).transpose(-1, -2) @ doh.abs() + (nsum + 2) * EPS * (pd.transpose(-1, -2) @ doh.abs())
        if Bk == 1:
            bdk, bdv = bdk.sum(0, keepdim=True), bdv.sum(0, keepdim=True)

        def flat(t, n):
            return t.transpose(1, 2).reshape(n, -1, hid)
        bounds = dict(out=2 * flat(bo, B), p=2 * bp, dq=2 * flat(bdq, B), dk=2 * flat(bdk, Bk), dv=2 * flat(bdv, Bk))
    return dict(out=out.detach(), p=p, dq=rdq, dk=rdk, dv=rdv), bounds


def _attn_fn_case(B, Bk, Mq, H, Sq, Sk, D, seed, mask="random", drop=False):
    from openpsg_amd import train_graph as G
    q, k, v, dout, keep, dmask = _attn_inputs(B, Bk, Mq, H, Sq, Sk, D, seed, mask, drop)
    scale = D ** -0.5
    dscale = 1.0 / (1.0 - 0.1)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = G.AttnFn.apply(qg, kg, vg, keep, H, scale, None if dmask is None else (dmask, dscale))
    p = out.grad_fn.saved_tensors[3]
    dq, dk, dv = torch.autograd.grad(out, (qg, kg, vg), dout)
    ref, bnd = _attn_ref(q, k, v, dout, keep, dmask, dscale, H, scale)
    got = dict(out=out, p=p, dq=dq, dk=dk, dv=dv)
    return {n: _check(f"attention {n}", got[n], ref[n], bnd[n]) for n in ("out", "p", "dq", "dk", "dv")}


# B, Bk, Mq, H, Sq, Sk, D: one dimension at a time around a small base, then the shapes the training branch runs
ATTN = [
    (3, 3, 5, 2, 5, 65, 64), (1, 1, 5, 2, 5, 65, 64), (32, 32, 1, 2, 3, 65, 64),
    (3, 3, 5, 1, 5, 65, 64), (3, 3, 5, 12, 5, 65, 64),
    (3, 3, 5, 2, 5, 1, 64), (3, 3, 5, 2, 5, 63, 64), (3, 3, 5, 2, 5, 64, 64), (3, 3, 5, 2, 5, 200, 64),
    (3, 3, 5, 2, 5, 1023, 64), (3, 3, 5, 2, 5, 1024, 64), (3, 3, 1, 2, 5, 1024, 128),
    (3, 3, 5, 2, 5, 65, 8), (3, 3, 5, 2, 5, 65, 72), (3, 3, 5, 2, 5, 65, 128), (3, 3, 1, 2, 5, 200, 72),
    (4, 4, 80, 32, 80, 80, 128),                                  # Llama causal shape (keep set by the test)
    (32, 32, 45, 12, 45, 45, 64),                                 # Q-Former self-attention, 33 query + 12 text rows
]


@pytest.mark.parametrize("B,Bk,Mq,H,Sq,Sk,D", ATTN)
def test_attention_fwd_bwd_vs_float64(B, Bk, Mq, H, Sq, Sk, D):
    """AttnFn (Bk == B, or Bk == 1 with B == 1): out, the saved p, dq / dk / dv against float64 autograd, random keep masks.
    Shared keys with B > 1 are covered by test_attention_shared_keys_* below."""
    assert Bk == B or B == 1
    if (Sq, Sk, H) == (80, 80, 32):
        from openpsg_amd import train_graph as G
        q, k, v, dout, _, _ = _attn_inputs(B, Bk, Mq, H, Sq, Sk, D, 80)
        lens = torch.tensor([80, 57, 1, 33])
        valid = torch.arange(Sk)[None] < lens[:, None]
        keep = (torch.tril(torch.ones(Sq, Sk, dtype=torch.bool))[None] & valid[:, None, :]) | (
            (~valid)[:, :, None] & torch.eye(Sq, dtype=torch.bool)[None])
        keep = keep.to(torch.uint8).to(q.device)
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = G.AttnFn.apply(qg, kg, vg, keep, H, D ** -0.5)
        got = dict(out=out, p=out.grad_fn.saved_tensors[3])
        got["dq"], got["dk"], got["dv"] = torch.autograd.grad(out, (qg, kg, vg), dout)
        ref, bnd = _attn_ref(q, k, v, dout, keep, None, 1.0, H, D ** -0.5)
        r = {n: _check(f"attention {n}", got[n], ref[n], bnd[n]) for n in got}
    else:
        r = _attn_fn_case(B, Bk, Mq, H, Sq, Sk, D, seed=B * 1000 + Sk * 7 + D + H + Mq)
    print(f"attention B={B} Bk={Bk} Mq={Mq} H={H} Sq={Sq} Sk={Sk} D={D}: err/bound",
          {n: round(x, 3) for n, x in r.items()})


@pytest.mark.parametrize("mask", ["one_key", "rows", "none"])
@pytest.mark.parametrize("Mq", [1, 5])
def test_attention_masks_and_dropout_vs_float64(mask, Mq):
    """Keep masks (one key masked for all rows, whole rows masked = uniform softmax in both, none) with attention
    dropout p = 0.1 (out = (softmax x keep x 1/(1-p)) @ v) and one row whose dropout removes every key."""
    for drop in (False, True):
        r = _attn_fn_case(3, 3, Mq, 2, 5, 130, 72, seed=17 + Mq, mask=mask, drop=drop)
        print(f"attention mask={mask} Mq={Mq} dropout={drop}: err/bound", {n: round(x, 3) for n, x in r.items()})


def _attn_raw_shared(B, H, Sq, Sk, D, Mq, seed, drop):
    """psg_train_attn_fwd / _bwd with keys and values shared by all B sequences (Bk = 1), called through the C ABI on
    buffers sized for B blocks: block 0 holds k / v (dk / dv start at zero), blocks 1.. are NaN / sentinel-filled, so a
    kernel that read or wrote another sequence's key block fails here instead of touching memory it does not own."""
    from openpsg_amd import ops
    from openpsg_amd._lib import check
    q, k, v, dout, keep, dmask = _attn_inputs(B, 1, Mq, H, Sq, Sk, D, seed, "rows", drop)
    dev, hid = q.device, H * D
    scale, dscale = D ** -0.5, 1.0 / (1.0 - 0.1)
    kb = torch.full((B, Sk, hid), float("nan"), device=dev)
    vb = torch.full((B, Sk, hid), float("nan"), device=dev)
    kb[0], vb[0] = k[0], v[0]
    dkb = torch.full((B, Sk, hid), 7.0, device=dev)
    dvb = torch.full((B, Sk, hid), 7.0, device=dev)
    dkb[0], dvb[0] = 0.0, 0.0
    p = torch.empty((B, H, Sq, Sk), device=dev)
    out = torch.empty_like(q)
    dq = torch.empty_like(q)
    dmp = None if dmask is None else dmask.data_ptr()
    lib, c, st = ops._env(q)
    check(lib.psg_train_attn_fwd(c, q.data_ptr(), kb.data_ptr(), vb.data_ptr(), keep.data_ptr(), B, 1, H, Sq, Sk, D, Mq,
                                 scale, dmp, dscale, p.data_ptr(), out.data_ptr(), st), "psg_train_attn_fwd")
    check(lib.psg_train_attn_bwd(c, q.data_ptr(), kb.data_ptr(), vb.data_ptr(), p.data_ptr(), dout.data_ptr(), B, 1, H,
                                 Sq, Sk, D, scale, dmp, dscale, dq.data_ptr(), dkb.data_ptr(), dvb.data_ptr(), st),
          "psg_train_attn_bwd")
    torch.cuda.synchronize()
    assert bool((dkb[1:] == 7.0).all()) and bool((dvb[1:] == 7.0).all()), "dk / dv written outside the shared key block"
    ref, bnd = _attn_ref(q, k, v, dout, keep, dmask, dscale, H, scale)
    got = dict(out=out, p=p, dq=dq, dk=dkb[:1], dv=dvb[:1])
    return {n: _check(f"attention (shared keys) {n}", got[n], ref[n], bnd[n]) for n in got}


@pytest.mark.parametrize("B,H,Sq,Sk,D,Mq", [(3, 2, 5, 65, 64, 1), (32, 12, 33, 336, 64, 1), (32, 2, 3, 1024, 72, 3),
                                          (3, 1, 4, 1, 8, 4), (5, 2, 3, 64, 128, 1)])
@pytest.mark.parametrize("drop", [False, True])
def test_attention_shared_keys_vs_float64(B, H, Sq, Sk, D, Mq, drop):
    """Bk == 1 (the Q-Former cross-attention: one patch table for every pair; B=32, Sq=33, Mq=1, Sk=336, H=12, D=64 is its
    shape): dk / dv are the sums over all B sequences' queries, which the end-to-end test sees only diluted."""
    r = _attn_raw_shared(B, H, Sq, Sk, D, Mq, seed=B * 31 + Sk + D + int(drop), drop=drop)
    print(f"attention shared keys B={B} H={H} Sq={Sq} Sk={Sk} D={D} Mq={Mq} dropout={drop}: err/bound",
          {n: round(x, 3) for n, x in r.items()})


def test_attention_limits_are_rejected():
    """Sk > 1024 (16 keys per lane), D > 128 and Bk not in (B, 1) are refused by the C ABI (PsgHipError), not computed."""
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError, check
    dev = _dev()
    lib, c, st = ops._env(torch.empty(1, device=dev))
    buf = torch.zeros(1 << 16, device=dev)                      # never touched: every call is refused before a launch
    keep = torch.ones(1 << 16, dtype=torch.uint8, device=dev)
    P = buf.data_ptr()
    for B, Bk, Sk, D in [(1, 1, 1025, 8), (1, 1, 4, 130), (3, 2, 4, 8)]:
        with pytest.raises(PsgHipError):
            check(lib.psg_train_attn_fwd(c, P, P, P, keep.data_ptr(), B, Bk, 1, 1, Sk, D, 1, 1.0, None, 1.0, P, P, st),
                  "psg_train_attn_fwd")
        with pytest.raises(PsgHipError):
            check(lib.psg_train_attn_bwd(c, P, P, P, P, P, B, Bk, 1, 1, Sk, D, 1.0, None, 1.0, P, P, P, st),
                  "psg_train_attn_bwd")
    torch.cuda.synchronize()
    assert not buf.any()


# ---- element-wise: GELU, SwiGLU gate, rotary ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_gelu_fwd_bwd_vs_float64(n):
    """exact-erf GELU x Phi(x) on [-40, 40] with 0 and +-1e-20: value and gradient against float64."""
    from openpsg_amd import train_graph as G
    dev = _dev()
    g = _gen(n)
    x = torch.rand(n, generator=g) * 80 - 40
    x[:6] = torch.tensor([0.0, 1e-20, -1e-20, 40.0, -40.0, -5.0])[:n]
    x, dy = x.to(dev), torch.randn(n, generator=g).to(dev)
    xg = x.clone().requires_grad_(True)
    y = G.GeluFn.apply(xg)
    dx, = torch.autograd.grad(y, xg, dy)
    x64 = x.double().requires_grad_(True)
    y64 = x64 * 0.5 * (1 + torch.erf(x64 / math.sqrt(2)))
    rdx, = torch.autograd.grad(y64, x64, dy.double())
    with torch.no_grad():
        xd = x64.detach()
        phi = torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
        by = 4 * EPS * (xd.abs() + y64.abs()) + TINY
        bdx = 4 * EPS * dy.double().abs() * (1 + xd.abs() * phi * (2 + xd * xd)) + TINY
    print(f"gelu n={n}: err/bound y {_check('gelu y', y, y64.detach(), by):.3f}, dx {_check('gelu dx', dx, rdx, bdx):.3f}")


@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("inter", [1, 11, 688, 11008])
def test_silu_mul_fwd_bwd_vs_float64(inter, rows):
    """silu(gate) * up with gate on [-100, 100] (expf(-gate) overflows below -88.7: the sigmoid underflows to 0, which
    loses at most 2^-126 x |gate up|)."""
    from openpsg_amd import train_graph as G
    dev = _dev()
    g = _gen(inter * 3 + rows)
    gate = torch.rand(rows, inter, generator=g) * 200 - 100
    gate.view(-1)[:4] = torch.tensor([-100.0, 100.0, 0.0, -88.5])[:gate.numel()]
    gu = torch.cat([gate, torch.randn(rows, inter, generator=g)], 1).to(dev)
    dy = torch.randn(rows, inter, generator=g).to(dev)
    gug = gu.clone().requires_grad_(True)
    y = G.SiluMulFn.apply(gug)
    dgu, = torch.autograd.grad(y, gug, dy)
    gu64 = gu.double().requires_grad_(True)
    g64, u64 = gu64[:, :inter], gu64[:, inter:]
    y64 = g64 * torch.sigmoid(g64) * u64
    rdgu, = torch.autograd.grad(y64, gu64, dy.double())
    with torch.no_grad():
        gd, ud, dd = g64.detach(), u64.detach(), dy.double()
        sg = torch.sigmoid(gd)
        by = 8 * EPS * y64.abs() + TINY * (gd * ud).abs()
        bdg = 8 * EPS * (dd * ud).abs() * sg * (1 + gd.abs()) + TINY * (dd * ud).abs() * (1 + gd.abs())
        bdu = 8 * EPS * (dd * gd).abs() * sg + TINY * (dd * gd).abs()
    r = [_check("silu_mul y", y, y64.detach(), by), _check("silu_mul dgate", dgu[:, :inter], rdgu[:, :inter], bdg),
         _check("silu_mul dup", dgu[:, inter:], rdgu[:, inter:], bdu)]
    print(f"silu_mul inter={inter} rows={rows}: err/bound", ["%.3f" % x for x in r])


def _rope_tables(table_rows, hd, dev):
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(table_rows, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev)


@pytest.mark.parametrize("heads", [1, 32])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_rope_fwd_bwd_vs_float64(head_dim, heads):
    """Half-split rotary against HF's x cos + rotate_half(x) sin in float64 (the same fp32 tables), its gradient against
    float64 autograd, and the adjoint identity <rope(x), y> = <x, rope^-1(y)> on the kernel's own outputs; positions 0
    and table_rows - 1 included; a position outside the table is refused."""
    from openpsg_amd import train_graph as G
    from openpsg_amd._lib import PsgHipError
    dev = _dev()
    table_rows, rows = 100, 37
    g = _gen(head_dim + heads)
    cos, sin = _rope_tables(table_rows, head_dim, dev)
    pos = torch.randint(0, table_rows, (rows,), generator=g)
    pos[0], pos[1] = 0, table_rows - 1
    pos = pos.to(torch.int32).to(dev)
    x = torch.randn(rows, heads * head_dim, generator=g).to(dev)
    dy = torch.randn(rows, heads * head_dim, generator=g).to(dev)
    xg = x.clone().requires_grad_(True)
    y = G.RopeFn.apply(xg, pos, cos, sin, heads)
    dx, = torch.autograd.grad(y, xg, dy)

    def rope64(t):
        c = torch.cat([cos, cos], -1).double()[pos.long()][:, None]
        s = torch.cat([sin, sin], -1).double()[pos.long()][:, None]
        th = t.view(rows, heads, head_dim)
        rot = torch.cat([-th[..., head_dim // 2:], th[..., :head_dim // 2]], -1)
        return (th * c + rot * s).reshape(rows, -1), (th.abs() * c.abs() + rot.abs() * s.abs()).reshape(rows, -1)

    x64 = x.double().requires_grad_(True)
    y64, ya = rope64(x64)
    rdx, = torch.autograd.grad(y64, x64, dy.double())
    with torch.no_grad():
        by = 3 * EPS * ya.detach()
        _, dya = rope64(dy.double())
        bdx = 3 * EPS * dya
        r = [_check("rope y", y, y64.detach(), by), _check("rope dx", dx, rdx, bdx)]
        lhs = (y.double() * dy.double()).sum()
        rhs = (x.double() * dx.double()).sum()
        badj = (by * dy.double().abs()).sum() + (x.double().abs() * bdx).sum()
        assert (lhs - rhs).abs() <= badj, (lhs.item(), rhs.item(), badj.item())
    print(f"rope head_dim={head_dim} heads={heads}: err/bound", ["%.3f" % v for v in r])
    for bad in (-1, table_rows):
        p2 = pos.clone()
        p2[5] = bad
        with pytest.raises(PsgHipError):
            G.RopeFn.apply(x, p2, cos, sin, heads)


# ---- losses -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [1, 100, 257, 515, 32000, 32003])
def test_cross_entropy_fwd_bwd_vs_float64(vocab):
    """Per-row -log softmax(logits)[label] and its gradient dloss[row] (softmax - onehot), against float64, with labels 0
    and vocab - 1, ignore_index (-100) rows, rows of logits up to +-1e4 and a dloss that varies by row (a probability
    below 2^-126 may underflow to 0 in fp32).

    Pinned contract: a label >= vocab is ignored exactly like a negative one - loss 0 and a zero gradient row - in both
    the forward and the backward.  torch's cross_entropy would raise for such a label instead."""
    from openpsg_amd import train_graph as G
    dev = _dev()
    g = _gen(vocab)
    rows = 9
    logits = torch.randn(rows, vocab, generator=g) * 3
    logits[2] = (torch.randn(vocab, generator=g) * 1e4).clamp(-1e4, 1e4)
    logits[3] = torch.where(torch.rand(vocab, generator=g) < 0.5, -1e4, 1e4)
    labels = torch.randint(0, vocab, (rows,), generator=g)
    labels[0], labels[1], labels[4], labels[5] = 0, vocab - 1, -100, vocab
    labels[6] = vocab + 1000
    labels = labels.to(torch.int32)
    dloss = torch.randn(rows, generator=g)
    logits, labels_d, dloss = logits.to(dev), labels.to(dev), dloss.to(dev)
    lg = logits.clone().requires_grad_(True)
    loss = G.CrossEntropyRowsFn.apply(lg, labels_d)
    d, = torch.autograd.grad(loss, lg, dloss)

    ign = (labels < 0) | (labels >= vocab)
    safe = labels.clamp(0, vocab - 1).long().to(dev)
    ign_d = ign.to(dev)
    x64 = logits.double().requires_grad_(True)
    ref = (torch.logsumexp(x64, -1) - x64.gather(1, safe[:, None])[:, 0]).masked_fill(ign_d, 0.0)
    rd, = torch.autograd.grad(ref, x64, dloss.double())
    with torch.no_grad():
        xd = x64.detach()
        m = xd.amax(-1, keepdim=True)
        p = torch.softmax(xd, -1)
        r = vocab / 256 + 12
        spread = (p * (xd - m).abs()).sum(-1, keepdim=True)
        lse = torch.logsumexp(xd, -1)
        bl = 4 * EPS * (r + spread[:, 0] + (lse - m[:, 0]).abs() + m[:, 0].abs() + xd.gather(1, safe[:, None])[:, 0].abs())
        bl = bl.masked_fill(ign_d, 0.0)
        onehot = F.one_hot(safe, vocab).double()
        bd = dloss.double().abs()[:, None] * (4 * EPS * (p * (r + 4 + (xd - m).abs() + spread) + onehot) + TINY)
        bd = bd.masked_fill(ign_d[:, None], 0.0)
    assert bool((loss[ign_d] == 0).all()) and bool((d[ign_d] == 0).all()), "an ignored row has a loss or a gradient"
    print(f"cross entropy vocab={vocab}: err/bound loss {_check('ce loss', loss, ref.detach(), bl):.3f}, "
          f"dlogits {_check('ce dlogits', d, rd, bd):.3f}")


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("n", [1, 37, 257, 4096])
def test_bce_fwd_bwd_vs_float64(n, soft):
    """mean BCE-with-logits x 50 (the existence loss) with logits on [-30, 30] and hard or soft labels."""
    from openpsg_amd import train_graph as G
    dev = _dev()
    g = _gen(n * 2 + int(soft))
    x = torch.rand(n, generator=g) * 60 - 30
    x[:2] = torch.tensor([30.0, -30.0])[:n]
    lab = torch.rand(n, generator=g) if soft else (torch.rand(n, generator=g) < 0.3).float()
    x, lab = x.to(dev), lab.to(dev)
    weight, dloss = 50.0, 0.37
    xg = x.clone().requires_grad_(True)
    loss = G.BceFn.apply(xg, lab, weight)
    dx, = torch.autograd.grad(loss, xg, torch.tensor(dloss, device=dev))
    x64 = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(x64, lab.double()) * weight
    rdx, = torch.autograd.grad(ref, x64, torch.tensor(dloss, dtype=torch.float64, device=dev))
    with torch.no_grad():
        xd, yd = x64.detach(), lab.double()
        terms = xd.clamp_min(0) + (xd * yd).abs() + torch.log1p(torch.exp(-xd.abs()))
        bl = 2 * (_red(n, 256) + 6) * EPS * terms.sum() * weight / n
        sg = torch.sigmoid(xd)
        bdx = 4 * EPS * dloss * weight / n * (sg + yd + (sg - yd).abs())
    print(f"bce n={n} soft={soft}: err/bound loss {_check('bce loss', loss.reshape(1), ref.detach().reshape(1), bl.reshape(1)):.3f}, "
          f"dlogit {_check('bce dlogit', dx, rdx, bdx):.3f}")


# ---- patch embedding (weight gradient) ----------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", [128, 96])
def test_patch_embed_fn_grads_vs_float64(Cout):
    """PatchEmbedFn: Cout = 128 runs the fp32 matrix-core kernel forward, Cout = 96 the conv2d branch; dw / db against
    float64 autograd of conv2d (the features are frozen: no gradient)."""
    from openpsg_amd import train_graph as G
    dev = _dev()
    g = _gen(Cout)
    C, Hf, Wf, patch = 16, 48, 64, 16
    feat = torch.randn(1, C, Hf, Wf, generator=g).to(dev)
    w = (torch.randn(Cout, C, patch, patch, generator=g) / (C * patch * patch) ** 0.5).to(dev)
    b = torch.randn(Cout, generator=g).to(dev)
    L = (Hf // patch) * (Wf // patch)
    dp = torch.randn(L, Cout, generator=g).to(dev)
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = G.PatchEmbedFn.apply(feat, wg, bg, patch)
    dw, db = torch.autograd.grad(out, (wg, bg), dp)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv2d(feat.double(), w64, b64, stride=patch).flatten(2).transpose(1, 2)[0]
    rdw, rdb = torch.autograd.grad(ref, (w64, b64), dp.double())
    with torch.no_grad():
        K = C * patch * patch
        cols = F.unfold(feat.double(), patch, stride=patch)[0]                # [K, L]
        bo = 2 * (K + 2) * EPS * (cols.abs().t() @ w.double().abs().reshape(Cout, K).t() + b.double().abs())
        bdw = (2 * (L + 2) * EPS * (dp.double().abs().t() @ cols.abs().t())).view_as(rdw)
        bdb = 2 * (L + 2) * EPS * dp.double().abs().sum(0)
    r = [_check("patch_embed out", out, ref.detach(), bo), _check("patch_embed dw", dw, rdw, bdw),
         _check("patch_embed db", db, rdb, bdb)]
    print(f"patch_embed Cout={Cout}: err/bound", ["%.3f" % x for x in r])
