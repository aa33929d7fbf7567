"""Kernels of csrc/psg_train_bf16.hip (`-m gpu`), each against a float64 computation on the same bf16-rounded inputs.

The bound is derived, not tuned: |err| <= 2^-8 |exact| + 2^-18 sum|terms|.  The first part is one bf16 rounding of the
output (2^-9 relative) with a factor 2 of slack; the second is fp32 arithmetic (2^-24 per operation) over at most a few
thousand terms, and for the attention the hi + lo bf16 split of P and dS (|p - hi - lo| <= 2^-18 |p|).  `terms` are the
elementary products that are summed into the output element, down to the inputs where a factor is itself a sum that
cancels (the statistics of the norms; dS = p (dP - sum p dP), whose dP are dot products): every test says which.  Each
test prints the worst |err| / bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PSG_ERR_UNSUPPORTED = -2
FMIN = float(torch.finfo(torch.float32).min)


def _env():
    from openpsg_amd import ops
    return ops._env(torch.empty(1, device="cuda:0"))


def _bound(name, got, exact, terms, worst=None):
    err = (got.double().cpu() - exact.cpu()).abs()
    bound = 2.0 ** -8 * exact.cpu().abs() + 2.0 ** -18 * terms.cpu()
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    if worst is None:
        print(f"{name}: worst |err| / bound = {ratio:.3f}")
    else:
        worst[name] = max(worst.get(name, 0.0), ratio)
    assert bool((err <= bound).all()), f"{name}: |err| / bound = {ratio:.3f}"
    return ratio


def _rand(shape, gen, scale=1.0, dtype=BF):
    return (torch.randn(shape, generator=gen) * scale).to(dtype).cuda()


def test_unsupported_code_matches_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "psg_hip.h")).read()
    m = re.search(r"PSG_ERR_UNSUPPORTED\s*=\s*(-?\d+)", hdr)
    assert m and int(m.group(1)) == PSG_ERR_UNSUPPORTED


# ---- LayerNorm / RMSNorm ---------------------------------------------------------------------------------------------
NORM_SHAPES = [(r, h) for r in (1, 5, 67) for h in (768, 256, 4096)]


@pytest.mark.parametrize("rows,hidden", NORM_SHAPES)
def test_layernorm_fwd_bwd(rows, hidden):
    """terms: forward |xhat gamma| + |beta| + |gamma| rstd mean|x| (the mean is a sum of the x); backward
    rstd (|g| + mean|g| + |xhat| mean|g xhat|), g = dy gamma; dgamma sum_rows |dy| (|xhat| + rstd mean|x|) (xhat carries the
    mean's summation error, as in the forward), dbeta sum_rows |dy|."""
    lib, c, st = _env()
    gen = torch.Generator().manual_seed(rows * 10000 + hidden)
    eps = 1e-12
    x = _rand((rows, hidden), gen, 2.0, torch.float32) + 0.5
    if rows > 1:
        x[rows - 1] = 1.0                                        # a row of equal values: variance 0, y = beta
    gamma, beta = _rand((hidden,), gen, 1.0, torch.float32) + 1.0, _rand((hidden,), gen, 0.5, torch.float32)
    dy = _rand((rows, hidden), gen)
    y = torch.empty((rows, hidden), device="cuda", dtype=BF)
    mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    assert lib.psg_train_bf16_layernorm_fwd(c, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, rows, hidden,
                                            y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), st) == 0
    dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
    assert lib.psg_train_bf16_layernorm_bwd(c, x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                            rstd.data_ptr(), rows, hidden, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                            st) == 0
    torch.cuda.synchronize()
    X, G, Bt, DY = x.double().cpu(), gamma.double().cpu(), beta.double().cpu(), dy.double().cpu()
    mu = X.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((X - mu) ** 2).mean(1, keepdim=True) + eps)
    live = torch.ones(rows, dtype=torch.bool)
    if rows > 1:
        live[rows - 1] = False                                   # the variance-0 row: rstd = 1e6, only its forward is defined
    xh = (X - mu) * rs
    _bound("layernorm fwd", y, xh * G + Bt, (xh * G).abs() + Bt.abs() + G.abs() * rs * X.abs().mean(1, keepdim=True))
    if rows > 1:
        assert torch.equal(y[rows - 1].float().cpu(), beta.to(BF).float().cpu())
    g = DY * G
    want = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    terms = rs * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
    _bound("layernorm bwd dx", dx[live.cuda()], want[live], terms[live])
    x2, dy2 = x.clone(), dy.clone()                          # dgamma / dbeta over the live rows only
    n = int(live.sum())
    assert lib.psg_train_bf16_layernorm_bwd(c, x2.data_ptr(), dy2.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                            rstd.data_ptr(), n, hidden, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                            st) == 0
    torch.cuda.synchronize()
    _bound("layernorm dgamma", dg, (DY * xh)[live].sum(0),
           (DY.abs() * (xh.abs() + rs * X.abs().mean(1, keepdim=True)))[live].sum(0))
    _bound("layernorm dbeta", db, DY[live].sum(0), DY[live].abs().sum(0))


@pytest.mark.parametrize("rows,hidden", NORM_SHAPES)
def test_rmsnorm_fwd_bwd(rows, hidden):
    """terms: forward |w x r|; backward r (|g| + |x| r^2 mean|g x|), g = dy w."""
    lib, c, st = _env()
    gen = torch.Generator().manual_seed(rows * 20000 + hidden)
    eps = 1e-5
    x = _rand((rows, hidden), gen, 2.0, torch.float32)
    x[rows - 1] = 1.0
    w = _rand((hidden,), gen, 0.3, torch.float32) + 1.0
    dy = _rand((rows, hidden), gen)
    y = torch.empty((rows, hidden), device="cuda", dtype=BF)
    rstd, dx = torch.empty(rows, device="cuda"), torch.empty_like(x)
    assert lib.psg_train_bf16_rmsnorm_fwd(c, x.data_ptr(), w.data_ptr(), eps, rows, hidden, y.data_ptr(), rstd.data_ptr(),
                                          st) == 0
    assert lib.psg_train_bf16_rmsnorm_bwd(c, x.data_ptr(), dy.data_ptr(), w.data_ptr(), rstd.data_ptr(), rows, hidden,
                                          dx.data_ptr(), st) == 0
    torch.cuda.synchronize()
    X, W, DY = x.double().cpu(), w.double().cpu(), dy.double().cpu()
    r = 1.0 / torch.sqrt((X * X).mean(1, keepdim=True) + eps)
    _bound("rmsnorm fwd", y, W * X * r, (W * X * r).abs())
    g = DY * W
    _bound("rmsnorm bwd", dx, r * (g - X * r * r * (g * X).mean(1, keepdim=True)),
           r * (g.abs() + X.abs() * r * r * (g * X).abs().mean(1, keepdim=True)))


def test_norms_refuse_a_hidden_size_that_is_no_multiple_of_8():
    lib, c, st = _env()
    rows, hidden = 3, 100
    x = torch.randn(rows, hidden, device="cuda")
    g = torch.ones(hidden, device="cuda")
    y = torch.empty((rows, hidden), device="cuda", dtype=BF)
    a, b = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    assert lib.psg_train_bf16_layernorm_fwd(c, x.data_ptr(), g.data_ptr(), g.data_ptr(), 1e-12, rows, hidden, y.data_ptr(),
                                            a.data_ptr(), b.data_ptr(), st) == PSG_ERR_UNSUPPORTED
    assert lib.psg_train_bf16_rmsnorm_fwd(c, x.data_ptr(), g.data_ptr(), 1e-5, rows, hidden, y.data_ptr(), a.data_ptr(),
                                          st) == PSG_ERR_UNSUPPORTED
    assert lib.psg_train_bf16_layernorm_bwd(c, x.data_ptr(), y.data_ptr(), g.data_ptr(), a.data_ptr(), b.data_ptr(), rows,
                                            hidden, x.data_ptr(), None, None, st) == PSG_ERR_UNSUPPORTED
    assert lib.psg_train_bf16_rmsnorm_bwd(c, x.data_ptr(), y.data_ptr(), g.data_ptr(), a.data_ptr(), rows, hidden,
                                          x.data_ptr(), st) == PSG_ERR_UNSUPPORTED


# ---- pointwise ---------------------------------------------------------------------------------------------------------
def test_gelu_silu_rope():
    """terms: the products the kernel adds for one element (GELU: Phi = 0.5 + 0.5 erf is itself a sum that cancels for
    x < 0, so forward |x| (0.5 + 0.5 |erf|), backward |dy| (0.5 + 0.5 |erf| + |x phi|); SwiGLU backward:
    |d u s| + |d u s g (1 - s)|; rotary: |a cos| + |b sin|); a single product is bounded by the rounding part alone."""
    lib, c, st = _env()
    gen = torch.Generator().manual_seed(7)
    n = 67 * 3072
    x, dy = _rand((n,), gen, 2.0), _rand((n,), gen)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    assert lib.psg_train_bf16_gelu_fwd(c, x.data_ptr(), n, y.data_ptr(), st) == 0
    assert lib.psg_train_bf16_gelu_bwd(c, x.data_ptr(), dy.data_ptr(), n, dx.data_ptr(), st) == 0
    X, DY = x.double().cpu(), dy.double().cpu()
    erf = torch.erf(X / 2 ** 0.5)
    cdf, acdf = 0.5 * (1 + erf), 0.5 * (1 + erf.abs())
    phi = torch.exp(-0.5 * X * X) / (2 * torch.pi) ** 0.5
    _bound("gelu fwd", y, X * cdf, X.abs() * acdf)
    _bound("gelu bwd", dx, DY * (cdf + X * phi), DY.abs() * (acdf + (X * phi).abs()))
    rows, inter = 37, 1368
    gu, d = _rand((rows, 2 * inter), gen, 2.0), _rand((rows, inter), gen)
    o, dgu = torch.empty((rows, inter), device="cuda", dtype=BF), torch.empty_like(gu)
    assert lib.psg_train_bf16_silu_mul_fwd(c, gu.data_ptr(), rows, inter, o.data_ptr(), st) == 0
    assert lib.psg_train_bf16_silu_mul_bwd(c, gu.data_ptr(), d.data_ptr(), rows, inter, dgu.data_ptr(), st) == 0
    G, U, Dd = gu[:, :inter].double().cpu(), gu[:, inter:].double().cpu(), d.double().cpu()
    s = torch.sigmoid(G)
    _bound("silu_mul fwd", o, G * s * U, (G * s * U).abs())
    _bound("silu_mul bwd gate", dgu[:, :inter], Dd * U * s * (1 + G * (1 - s)), (Dd * U * s).abs() * (1 + (G * (1 - s)).abs()))
    _bound("silu_mul bwd up", dgu[:, inter:], Dd * G * s, (Dd * G * s).abs())
    for heads, hd in ((3, 128), (2, 64)):
        rows, table = 41, 50
        xr = _rand((rows, heads * hd), gen)
        pos = torch.randint(0, table, (rows,), generator=gen).to(torch.int32).cuda()
        ang = torch.rand(table, hd // 2, generator=gen) * 6.0
        cs, sn = ang.cos().cuda().contiguous(), ang.sin().cuda().contiguous()
        for sign in (1.0, -1.0):
            yr = torch.empty_like(xr)
            assert lib.psg_train_bf16_rope(c, xr.data_ptr(), pos.data_ptr(), cs.data_ptr(), sn.data_ptr(), table, rows, heads,
                                           hd, sign, yr.data_ptr(), st) == 0
            Xr = xr.double().cpu().view(rows, heads, hd)
            C_, S_ = cs.double().cpu()[pos.cpu().long()][:, None], sn.double().cpu()[pos.cpu().long()][:, None] * sign
            a, b = Xr[..., :hd // 2], Xr[..., hd // 2:]
            want = torch.cat([a * C_ - b * S_, b * C_ + a * S_], -1).view(rows, -1)
            terms = torch.cat([(a * C_).abs() + (b * S_).abs(), (b * C_).abs() + (a * S_).abs()], -1).view(rows, -1)
            _bound(f"rope sign {sign:+.0f} head_dim {hd}", yr, want, terms)
    assert lib.psg_train_bf16_gelu_fwd(c, x.data_ptr(), 12, y.data_ptr(), st) == PSG_ERR_UNSUPPORTED


def test_pointwise_bf16_nodes_are_the_fp32_nodes_rounded_once():
    """Both precisions instantiate one kernel template (csrc/psg_train_rows.h), so on bf16-representable inputs a bf16
    pointwise node gives the bits of the fp32 node's result rounded once to bf16: GELU and the SwiGLU gate forward and
    backward, rotary at both signs (sign -1 is the node's backward)."""
    from openpsg_amd import train_graph as G
    gen = torch.Generator().manual_seed(11)

    def both(node, x, *args):
        outs = []
        for xx, precision in ((x, "bf16"), (x.float(), None)):
            xx = xx.clone().requires_grad_(True)
            y = node.apply(xx, *args, precision)
            dy = _rand(tuple(y.shape), torch.Generator().manual_seed(13)).to(y.dtype)
            dx, = torch.autograd.grad(y, xx, dy)
            outs.append((y.to(BF), dx.to(BF)))
        (y16, dx16), (y32, dx32) = outs
        assert y16.dtype == BF and torch.equal(y16, y32), node.__name__ + " forward"
        assert torch.equal(dx16, dx32), node.__name__ + " backward"

    for n in (8, 2056):
        both(G.GeluFn, _rand((n,), gen, 2.0))
    both(G.SiluMulFn, _rand((3, 2 * 88), gen, 2.0))
    for hd in (64, 128):
        rows, heads, table = 5, 2, 9
        pos = torch.randint(0, table, (rows,), generator=gen).to(torch.int32).cuda()
        ang = torch.rand(table, hd // 2, generator=gen) * 6.0
        both(G.RopeFn, _rand((rows, heads * hd), gen), pos, ang.cos().cuda().contiguous(), ang.sin().cuda().contiguous(), heads)


# ---- attention -----------------------------------------------------------------------------------------------------------
def _keep_mask(B, Mq, Sq, Sk, gen):
    """One fully masked row, one row with a single kept key, and (Mq == Sq == Sk) a causal keep-matrix."""
    if Mq == Sq and Sq == Sk and Sq > 1:
        keep = torch.tril(torch.ones(Sq, Sk, dtype=torch.uint8))[None].repeat(B, 1, 1)
        keep[1, :, Sk - 3:] = 0                                  # a shorter sequence: its last keys are padding
    else:
        keep = (torch.rand(B, Mq, Sk, generator=gen) > 0.3).to(torch.uint8)
    keep[0, Mq - 1, :] = 0                                       # all masked: uniform softmax
    keep[B - 1, 0, :] = 0
    keep[B - 1, 0, Sk // 2] = 1                                  # a single kept key
    return keep


def _attn_reference(q, k, v, keep, dout, H, scale, drop, dscale):
    """float64 autograd with the additive-min mask; returns out, dq, dk, dv and the |terms| of each."""
    B, Sq, hid = q.shape
    Bk, Sk, _ = k.shape
    D = hid // H
    Q = q.double().cpu().view(B, Sq, H, D).transpose(1, 2).requires_grad_(True)                   # [B, H, Sq, D]
    K = k.double().cpu().view(Bk, Sk, H, D).transpose(1, 2).requires_grad_(True)
    V = v.double().cpu().view(Bk, Sk, H, D).transpose(1, 2).requires_grad_(True)
    dO = dout.double().cpu().view(B, Sq, H, D).transpose(1, 2)
    add = (1.0 - keep.double().cpu())[:, None] * FMIN                                             # [B, 1, Mq, Sk]
    s = Q @ K.transpose(-1, -2) * scale + add
    p = torch.softmax(s, -1)
    dm = torch.ones_like(p) if drop is None else drop.double().cpu() * dscale
    out = (p * dm) @ V
    dq, dk, dv = torch.autograd.grad(out, (Q, K, V), dO)
    with torch.no_grad():
        pd = p * dm
        Va, Ka, Qa, dOa = V.abs().expand(B, -1, -1, -1), K.abs().expand(B, -1, -1, -1), Q.abs(), dO.abs()
        t_out = pd @ Va
        t_dv = pd.transpose(-1, -2) @ dOa                                                         # [B, H, Sk, D]
        A = dm * (dOa @ Va.transpose(-1, -2))                    # sum_d |dO v| behind every dP
        T = p * (A + (p * A).sum(-1, keepdim=True))              # |terms| of dS = p (dP - sum p dP)
        t_dq = scale * (T @ Ka)
        t_dk = scale * (T.transpose(-1, -2) @ Qa)
        if Bk == 1:
            t_dv, t_dk = t_dv.sum(0, keepdim=True), t_dk.sum(0, keepdim=True)
    back = lambda t, b_, s_: t.detach().transpose(1, 2).reshape(b_, s_, hid)                      # noqa: E731
    return (back(out, B, Sq), back(dq, B, Sq), back(dk, Bk, Sk), back(dv, Bk, Sk),
            back(t_out, B, Sq), back(t_dq, B, Sq), back(t_dk, Bk, Sk), back(t_dv, Bk, Sk), p.detach())


def _attn_run(q, k, v, keep, dout, H, scale, drop, dscale):
    lib, c, st = _env()
    B, Sq, hid = q.shape
    Bk, Sk, _ = k.shape
    out, lse = torch.empty_like(q), torch.empty((B, H, Sq), device="cuda")
    dp = None if drop is None else drop.data_ptr()
    rc = lib.psg_train_bf16_attn_fwd(c, q.data_ptr(), k.data_ptr(), v.data_ptr(), keep.data_ptr(), B, Bk, H, Sq, Sk, hid // H,
                                     keep.shape[1], scale, dp, dscale, out.data_ptr(), lse.data_ptr(), st)
    assert rc == 0, rc
    res = []
    for _ in range(2):
        dq, dk, dv, delta = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(lse)
        rc = lib.psg_train_bf16_attn_bwd(c, q.data_ptr(), k.data_ptr(), v.data_ptr(), keep.data_ptr(), dout.data_ptr(),
                                         lse.data_ptr(), B, Bk, H, Sq, Sk, hid // H, keep.shape[1], scale, dp, dscale,
                                         dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), st)
        assert rc == 0, rc
        res.append((dq, dk, dv))
    torch.cuda.synchronize()
    return out, lse, res


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(33, 33), (33, 70), (40, 40), (1, 5), (33, 1100)])
def test_attention_fwd_bwd(D, Sq, Sk):
    """H = 2, B = 3; keys per sequence and shared (Bk in {3, 1}); one keep-row and a keep-matrix per sequence (Mq in
    {1, Sq}); dropout mask off and on.  terms: out sum_j |p_j drop_j v_j|; dV sum_i |p drop dO|; dQ / dK the products
    behind dS = p (dP - sum p dP) down to the |dO v| of every dP, times |k| / |q|."""
    H, B = 2, 3
    scale = D ** -0.5
    worst = {}
    for Bk in (3, 1):
        for Mq in sorted({1, Sq}):
            for use_drop in (False, True):
                gen = torch.Generator().manual_seed(D * 131 + Sq * 17 + Sk + Bk * 3 + Mq + use_drop)
                q, dout = _rand((B, Sq, H * D), gen), _rand((B, Sq, H * D), gen)
                k, v = _rand((Bk, Sk, H * D), gen), _rand((Bk, Sk, H * D), gen)
                keep = _keep_mask(B, Mq, Sq, Sk, gen).cuda().contiguous()
                drop = (torch.rand(B, H, Sq, Sk, generator=gen) >= 0.1).to(torch.uint8).cuda() if use_drop else None
                dscale = 1.0 / 0.9 if use_drop else 1.0
                out, lse, res = _attn_run(q, k, v, keep, dout, H, scale, drop, dscale)
                w_out, w_dq, w_dk, w_dv, t_out, t_dq, t_dk, t_dv, p = _attn_reference(q, k, v, keep, dout, H, scale, drop,
                                                                                     dscale)
                tag = f"Bk={Bk} Mq={Mq} drop={int(use_drop)}"
                _bound("out " + tag, out, w_out, t_out, worst)
                _bound("dq " + tag, res[0][0], w_dq, t_dq, worst)
                _bound("dk " + tag, res[0][1], w_dk, t_dk, worst)
                _bound("dv " + tag, res[0][2], w_dv, t_dv, worst)
                for a, b_ in zip(res[0], res[1]):                # determinism: a second backward gives the same bits
                    assert torch.equal(a, b_)
                if not use_drop:                                 # the all-masked row is the mean of V's rows
                    V, i = v.double().cpu()[0], (Sq - 1 if Mq == Sq else 0)          # sequence 0, the row _keep_mask emptied
                    _bound("all-masked row " + tag, out[0, i], V.mean(0), V.abs().mean(0), worst)
                    assert float(lse[0, 0, i]) == FMIN
    print(f"attention D={D} Sq={Sq} Sk={Sk}: worst |err| / bound " + ", ".join(f"{k_} {v_:.3f}" for k_, v_ in worst.items()))
