"""Gradient path of the training branch: the reference back-propagates `binary_rel_cls_loss` and
`rel_llm_loss` (relation_transformer_head_v4.py:327-351, 463-482) into patch_embed, the relation Q-Former, the two
query parameters, the existence head and `language_projection`; the LLM is frozen (configs/psg/baseline_v4_ov.py:65), so
its weights get no gradient but the loss reaches the trainable parameters THROUGH its layers.

The graph is torch.autograd's; its nodes are
  * the dense projections (`F.linear`, library GEMM; their weight gradients too), and
  * `torch.autograd.Function`s whose forward and backward are the fp32 kernels of csrc/psg_train_bwd.hip: LayerNorm,
    RMSNorm, the three attentions (Q-Former self / cross with the pair masks, Llama causal), GELU, the SwiGLU gate,
    rotary, cross entropy and BCE-with-logits.  The norms, GELU, the gate and rotary are the kernel templates of
    csrc/psg_train_rows.h, which both precisions instantiate.
Training batches are tiny (<= 32 sampled pairs, <= 4 LLM pairs, V4:29-30, 38), so this path is written for exactness
against autograd on the CPU oracle (tests/test_gpu_train.py), not for speed.  No CPU path.

precision='bf16' (the head's train_precision) runs the same graph in the model torch.autocast(bfloat16) gives
the reference (bf16 activations, fp32 residual streams and statistics).  `LayerNormFn`, `RMSNormFn`, `GeluFn`, `SiluMulFn`
and `RopeFn` take the precision as their last argument and call the same templates through the psg_train_bf16_* entry
points of csrc/psg_train_bf16.hip (`_Family`); `AttnBf16Fn` is that file's attention on the matrix cores, `LinearBf16Fn`
a bf16 library GEMM whose weight gradient leaves its fp32 accumulator as fp32 onto the fp32 master.  `PatchEmbedFn`, the
losses and the sampler are shared.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from ._lib import PsgHipError, check


def _env(t):
    return ops._env(t)


BF16 = torch.bfloat16


def _f32(t, name="tensor"):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise PsgHipError(f"{name}: the gradient path runs in fp32 on the GPU (got {t.dtype} on {t.device})")
    return t.contiguous()


def _b16(t, name="tensor"):
    if t.dtype != BF16 or not t.is_cuda:
        raise PsgHipError(f"{name}: the bf16 gradient path takes bf16 activations on the GPU (got {t.dtype} on {t.device})")
    return t.contiguous()


class _Family:
    """What a row / pointwise node needs to know of its precision: the entry points' prefix (csrc/psg_train_bwd.hip |
    csrc/psg_train_bf16.hip, both instantiating csrc/psg_train_rows.h), the activations' dtype with its check, and how
    LayerNorm's dgamma / dbeta arrive: accumulated by atomics into zeros (fp32) or written (bf16: no memset).  The
    residual streams the norms read are fp32 in both."""

    def __init__(self, prefix, dtype, act, dgb):
        self.prefix, self.dtype, self.act, self.dgb = prefix, dtype, act, dgb

    def call(self, op, t, *args):
        lib, c, st = _env(t)
        check(getattr(lib, self.prefix + op)(c, *args, st), self.prefix + op)


_FAMILIES = {None: _Family("psg_train_", torch.float32, _f32, torch.zeros_like),
             "bf16": _Family("psg_train_bf16_", BF16, _b16, torch.empty_like)}


def _family(precision):
    if precision not in (None, "bf16"):
        raise PsgHipError(f"precision must be None or 'bf16', got {precision!r}")
    return _FAMILIES[precision]


class LayerNormFn(torch.autograd.Function):
    """x fp32 (the residual stream under 'bf16') -> y in the precision's activation dtype; gamma / beta fp32 (masters);
    dx, dgamma, dbeta fp32."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, precision=None):
        f = _family(precision)
        x, gamma, beta = _f32(x, "layernorm x"), _f32(gamma), _f32(beta)
        hidden = x.shape[-1]
        rows = x.numel() // hidden
        y = torch.empty(x.shape, device=x.device, dtype=f.dtype)
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        f.call("layernorm_fwd", x, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), rows, hidden, y.data_ptr(),
               mean.data_ptr(), rstd.data_ptr())
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.family = f
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        f = ctx.family
        dy = f.act(dy)
        hidden = x.shape[-1]
        dx = torch.empty_like(x)
        dg, db = f.dgb(gamma), f.dgb(gamma)
        f.call("layernorm_bwd", x, x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
               x.numel() // hidden, hidden, dx.data_ptr(), dg.data_ptr(), db.data_ptr())
        return dx, dg, db, None, None


class RMSNormFn(torch.autograd.Function):
    """HF-LL:53-67 with a FROZEN fp32 weight (no weight gradient); x fp32 (the Llama residual stream under 'bf16') -> y in
    the precision's activation dtype; dx fp32."""

    @staticmethod
    def forward(ctx, x, w, eps, precision=None):
        f = _family(precision)
        x, w = _f32(x, "rmsnorm x"), _f32(w)
        hidden = x.shape[-1]
        rows = x.numel() // hidden
        y = torch.empty(x.shape, device=x.device, dtype=f.dtype)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
        f.call("rmsnorm_fwd", x, x.data_ptr(), w.data_ptr(), float(eps), rows, hidden, y.data_ptr(), rstd.data_ptr())
        ctx.save_for_backward(x, w, rstd)
        ctx.family = f
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        dy = ctx.family.act(dy)
        hidden = x.shape[-1]
        dx = torch.empty_like(x)
        ctx.family.call("rmsnorm_bwd", x, x.data_ptr(), dy.data_ptr(), w.data_ptr(), rstd.data_ptr(), x.numel() // hidden,
                        hidden, dx.data_ptr())
        return dx, None, None, None


class AttnFn(torch.autograd.Function):
    """softmax(q.k * scale + additive mask) v.  q [B, Sq, H*D]; k, v [Bk, Sk, H*D] with Bk == B or 1 (shared by all
    sequences); keep uint8 [B, Mq, Sk], Mq == Sq or 1.  An all-masked row gives a uniform softmax (additive finfo.min).
    drop: None, or (uint8 keep mask [B, heads, Sq, Sk], 1 / (1 - p)) - dropout on the attention probabilities."""

    @staticmethod
    def forward(ctx, q, k, v, keep, heads, scale, drop=None):
        q, k, v = _f32(q, "attention q"), _f32(k), _f32(v)
        keep = keep.to(torch.uint8).contiguous()
        B, Sq, hid = q.shape
        Bk, Sk, _ = k.shape
        D = hid // heads
        Mq = keep.shape[1]
        assert keep.shape == (B, Mq, Sk) and v.shape == k.shape and Bk in (B, 1)
        dmask, dscale = (None, 1.0) if drop is None else (drop[0].to(torch.uint8).contiguous(), float(drop[1]))
        assert dmask is None or dmask.shape == (B, heads, Sq, Sk)
        p = torch.empty((B, heads, Sq, Sk), device=q.device, dtype=torch.float32)
        out = torch.empty_like(q)
        lib, c, st = _env(q)
        check(lib.psg_train_attn_fwd(c, q.data_ptr(), k.data_ptr(), v.data_ptr(), keep.data_ptr(), B, Bk, heads, Sq, Sk, D,
                                     Mq, float(scale), None if dmask is None else dmask.data_ptr(), dscale, p.data_ptr(),
                                     out.data_ptr(), st), "psg_train_attn_fwd")
        ctx.save_for_backward(q, k, v, p)
        ctx.heads, ctx.scale, ctx.dmask, ctx.dscale = heads, float(scale), dmask, dscale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, p = ctx.saved_tensors
        dout = _f32(dout)
        B, Sq, hid = q.shape
        Bk, Sk, _ = k.shape
        dq = torch.empty_like(q)
        dk, dv = torch.zeros_like(k), torch.zeros_like(v)
        lib, c, st = _env(q)
        check(lib.psg_train_attn_bwd(c, q.data_ptr(), k.data_ptr(), v.data_ptr(), p.data_ptr(), dout.data_ptr(), B, Bk,
                                     ctx.heads, Sq, Sk, hid // ctx.heads, ctx.scale,
                                     None if ctx.dmask is None else ctx.dmask.data_ptr(), ctx.dscale, dq.data_ptr(),
                                     dk.data_ptr(), dv.data_ptr(), st), "psg_train_attn_bwd")
        return dq, dk, dv, None, None, None, None


class GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, precision=None):
        f = _family(precision)
        x = f.act(x, "gelu x")
        y = torch.empty_like(x)
        f.call("gelu_fwd", x, x.data_ptr(), x.numel(), y.data_ptr())
        ctx.save_for_backward(x)
        ctx.family = f
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dy = ctx.family.act(dy)
        dx = torch.empty_like(x)
        ctx.family.call("gelu_bwd", x, x.data_ptr(), dy.data_ptr(), x.numel(), dx.data_ptr())
        return dx, None


class SiluMulFn(torch.autograd.Function):
    """gate_up [rows, 2*inter] -> silu(gate) * up [rows, inter] (HF-LL:163-177)."""

    @staticmethod
    def forward(ctx, gu, precision=None):
        f = _family(precision)
        gu = f.act(gu, "gate_up")
        rows, two = gu.shape
        y = torch.empty((rows, two // 2), device=gu.device, dtype=f.dtype)
        f.call("silu_mul_fwd", gu, gu.data_ptr(), rows, two // 2, y.data_ptr())
        ctx.save_for_backward(gu)
        ctx.family = f
        return y

    @staticmethod
    def backward(ctx, dy):
        gu, = ctx.saved_tensors
        dy = ctx.family.act(dy)
        d = torch.empty_like(gu)
        ctx.family.call("silu_mul_bwd", gu, gu.data_ptr(), dy.data_ptr(), gu.shape[0], gu.shape[1] // 2, d.data_ptr())
        return d, None


class RopeFn(torch.autograd.Function):
    """Half-split rotary (HF-LL:130-160) on x [rows, heads*head_dim] at table rows `pos` (int32 [rows])."""

    @staticmethod
    def forward(ctx, x, pos, cos, sin, heads, precision=None):
        f = _family(precision)
        x = f.act(x, "rope x")
        if pos.numel() and (int(pos.max()) >= cos.shape[0] or int(pos.min()) < 0):      # training only: one read-back
            raise PsgHipError(f"rope: position {int(pos.max())} outside the {cos.shape[0]}-row rotary table")
        ctx.save_for_backward(pos, cos, sin)
        ctx.heads, ctx.family = heads, f
        return RopeFn._run(f, x, pos, cos, sin, heads, 1.0)

    @staticmethod
    def _run(f, x, pos, cos, sin, heads, sign):
        rows, hid = x.shape
        y = torch.empty_like(x)
        f.call("rope", x, x.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), cos.shape[0], rows, heads, hid // heads,
               float(sign), y.data_ptr())
        return y

    @staticmethod
    def backward(ctx, dy):
        pos, cos, sin = ctx.saved_tensors
        f = ctx.family
        return RopeFn._run(f, f.act(dy), pos, cos, sin, ctx.heads, -1.0), None, None, None, None, None


class CrossEntropyRowsFn(torch.autograd.Function):
    """Per-row -log softmax(logits)[label]; label < 0 = ignored (loss 0, zero gradient).  V4:337-341."""

    @staticmethod
    def forward(ctx, logits, labels):
        logits = _f32(logits, "logits")
        loss = ops.cross_entropy_rows(logits, labels)
        ctx.save_for_backward(logits, labels)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, labels = ctx.saved_tensors
        dloss = _f32(dloss)
        d = torch.empty_like(logits)
        lib, c, st = _env(logits)
        check(lib.psg_train_ce_bwd(c, logits.data_ptr(), logits.shape[0], logits.shape[1], labels.data_ptr(),
                                   dloss.data_ptr(), d.data_ptr(), st), "psg_train_ce_bwd")
        return d, None


class BceFn(torch.autograd.Function):
    """mean BCE-with-logits x weight (V4:463-482, binary case)."""

    @staticmethod
    def forward(ctx, logit, label, weight):
        logit, label = _f32(logit, "logit"), _f32(label)
        ctx.save_for_backward(logit, label)
        ctx.weight = float(weight)
        return ops.bce_with_logits(logit, label, weight)

    @staticmethod
    def backward(ctx, dloss):
        logit, label = ctx.saved_tensors
        dloss = _f32(dloss).reshape(1)
        d = torch.empty_like(logit)
        lib, c, st = _env(logit)
        check(lib.psg_train_bce_bwd(c, logit.data_ptr(), label.data_ptr(), logit.numel(), ctx.weight, dloss.data_ptr(),
                                    d.data_ptr(), st), "psg_train_bce_bwd")
        return d, None, None


class MlcceRowsFn(torch.autograd.Function):
    """Per-row multilabel categorical cross entropy (V4:484-495) of the multiclass head: forward / backward are
    psg_train_mlcce_fwd / _bwd.  The labels take no gradient."""

    @staticmethod
    def forward(ctx, logits, labels):
        logits, labels = _f32(logits, "logits"), _f32(labels, "labels")
        ctx.save_for_backward(logits, labels)
        return ops.mlcce_rows(logits, labels)

    @staticmethod
    def backward(ctx, dloss):
        logits, labels = ctx.saved_tensors
        return ops.mlcce_rows_bwd(logits, labels, _f32(dloss)), None


def multiclass_loss(logits, labels, weight):
    """V4:473-477: the row losses weighted by themselves - w = loss / loss.max(), NOT detached, so autograd takes the
    gradient through max() (split evenly among tied rows) as in the reference - then mean x rel_cls_loss_weight."""
    loss = MlcceRowsFn.apply(logits, labels)
    w = loss / loss.max()
    return torch.mean(loss * w) * weight


class PatchEmbedFn(torch.autograd.Function):
    """timm PatchEmbed (V4:410): forward = the exact-fp32 matrix-core kernel of the inference path; backward = the weight
    gradient as one GEMM over the unfolded feature map (the features themselves come from the frozen segmenter)."""

    @staticmethod
    def forward(ctx, feat, weight, bias, patch):
        feat = _f32(feat, "mask_features")
        ctx.save_for_backward(feat)
        ctx.patch, ctx.wshape = patch, weight.shape
        if patch == 16 and feat.shape[-1] % 4 == 0 and weight.shape[0] % 128 == 0:
            return ops.patch_embed(feat, _f32(weight), _f32(bias), 16)
        return F.conv2d(feat, weight, bias, stride=patch).flatten(2).transpose(1, 2)[0].contiguous()

    @staticmethod
    def backward(ctx, dp):
        feat, = ctx.saved_tensors
        cols = F.unfold(feat, ctx.patch, stride=ctx.patch)[0]               # [C * patch * patch, L]
        dp = _f32(dp)                                                        # [L, Cout]
        dw = (dp.t() @ cols.t()).view(ctx.wshape)
        return None, dw, dp.sum(0), None


# ---- precision='bf16'  -----------------------------------------------------------------------------------------
class LinearBf16Fn(torch.autograd.Function):
    """x bf16 . W^T (+ b) with W, b the fp32 MASTERS: both operands bf16, fp32 accumulation, bf16 output; backward:
    dx bf16, dW = dy^T x written from the fp32 accumulator as fp32, db summed in fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _b16(x, "linear x")
        wb = weight.to(BF16)
        ctx.save_for_backward(x, wb)
        ctx.has_bias = bias is not None
        return F.linear(x, wb, None if bias is None else bias.to(BF16))

    @staticmethod
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        dy2 = _b16(dy).reshape(-1, dy.shape[-1])
        dx = (dy2 @ wb).view(x.shape) if ctx.needs_input_grad[0] else None
        dw = torch.mm(dy2.t(), x.reshape(-1, x.shape[-1]), out_dtype=torch.float32) if ctx.needs_input_grad[1] else None
        db = dy2.sum(0, dtype=torch.float32) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db


class AttnBf16Fn(torch.autograd.Function):
    """AttnFn's arguments and masking rule on bf16 q / k / v, on the matrix cores; saves the row log-sum-exp, not the
    probabilities; dq / dk / dv bf16, each element written once (no atomics)."""

    @staticmethod
    def forward(ctx, q, k, v, keep, heads, scale, drop=None):
        q, k, v = _b16(q, "attention q"), _b16(k), _b16(v)
        keep = keep.to(torch.uint8).contiguous()
        B, Sq, hid = q.shape
        Bk, Sk, _ = k.shape
        Mq = keep.shape[1]
        assert keep.shape == (B, Mq, Sk) and v.shape == k.shape and Bk in (B, 1)
        dmask, dscale = (None, 1.0) if drop is None else (drop[0].to(torch.uint8).contiguous(), float(drop[1]))
        assert dmask is None or dmask.shape == (B, heads, Sq, Sk)
        lse = torch.empty((B, heads, Sq), device=q.device, dtype=torch.float32)
        out = torch.empty_like(q)
        lib, c, st = _env(q)
        check(lib.psg_train_bf16_attn_fwd(c, q.data_ptr(), k.data_ptr(), v.data_ptr(), keep.data_ptr(), B, Bk, heads, Sq, Sk,
                                          hid // heads, Mq, float(scale), None if dmask is None else dmask.data_ptr(), dscale,
                                          out.data_ptr(), lse.data_ptr(), st), "psg_train_bf16_attn_fwd")
        ctx.save_for_backward(q, k, v, keep, lse)
        ctx.heads, ctx.scale, ctx.dmask, ctx.dscale = heads, float(scale), dmask, dscale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, keep, lse = ctx.saved_tensors
        dout = _b16(dout)
        B, Sq, hid = q.shape
        Bk, Sk, _ = k.shape
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse)
        lib, c, st = _env(q)
        check(lib.psg_train_bf16_attn_bwd(c, q.data_ptr(), k.data_ptr(), v.data_ptr(), keep.data_ptr(), dout.data_ptr(),
                                          lse.data_ptr(), B, Bk, ctx.heads, Sq, Sk, hid // ctx.heads, keep.shape[1], ctx.scale,
                                          None if ctx.dmask is None else ctx.dmask.data_ptr(), ctx.dscale, dq.data_ptr(),
                                          dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), st), "psg_train_bf16_attn_bwd")
        return dq, dk, dv, None, None, None, None


class _Nodes:
    """The graph's nodes for one precision: `qformer_pairs` / `llama_teacher_forcing` are written once over them.
    resid(a, b): the sum a LayerNorm / the Llama stream takes - fp32 in both precisions."""

    def __init__(self, precision):
        b = _family(precision).dtype == BF16
        self.bf16 = b
        bind = lambda fn: (lambda *a: fn.apply(*a, precision))                                   # noqa: E731
        self.ln, self.rms, self.gelu, self.silu, self.rope = map(bind, (LayerNormFn, RMSNormFn, GeluFn, SiluMulFn, RopeFn))
        self.attn = (AttnBf16Fn if b else AttnFn).apply
        self.linear = LinearBf16Fn.apply if b else F.linear
        self.act = (lambda t: t.to(BF16)) if b else (lambda t: t)
        self.resid = (lambda a, r: a.float() + r.float()) if b else (lambda a, r: a + r)


def linear(x, weight, bias=None, precision=None):
    return _Nodes(precision).linear(x, weight, bias)


def layer_norm(x, gamma, beta, eps):
    return LayerNormFn.apply(x, gamma, beta, eps)


class Dropout:
    """The Q-Former's dropouts as the reference trains it: V4:78-84 builds InstructBlipQFormerConfig with its defaults
    (hidden_dropout_prob = attention_probs_dropout_prob = 0.1) and tools/train.py puts the model in train() mode, so HF
    applies dropout after the embedding LayerNorm (HF-IB:728-757), on the attention probabilities (HF-IB:176-196) and on
    every dense output before its residual LayerNorm (HF-IB:519-530, 579-596).  Masks are drawn with torch's generator
    of `device` (or the given one; a CPU generator + upload lets a test replay the same masks in the CPU oracle), in the
    order the layers run."""

    def __init__(self, p_hidden=0.1, p_attn=0.1, generator=None):
        self.p_hidden, self.p_attn, self.generator = float(p_hidden), float(p_attn), generator

    def _keep(self, shape, p, device):
        gdev = device if self.generator is None else self.generator.device
        return (torch.rand(shape, device=gdev, generator=self.generator) >= p).to(device)

    def hidden(self, x):
        if self.p_hidden <= 0:
            return x
        keep = self._keep(x.shape, self.p_hidden, x.device).to(torch.float32) / (1.0 - self.p_hidden)
        return x * keep if x.dtype == torch.float32 else (x.float() * keep).to(x.dtype)   # 16-bit x: one rounding

    def attn(self, B, heads, Sq, Sk, device):
        if self.p_attn <= 0:
            return None
        return self._keep((B, heads, Sq, Sk), self.p_attn, device).to(torch.uint8), 1.0 / (1.0 - self.p_attn)


def qformer_pairs(P, cfg, patches, ids, text_mask, pair_keep, dropout: Dropout | None = None, precision=None):
    """The relation Q-Former (HF-IB:446-757 as driven by V4:179-185) over B pairs, all rows of all layers (training
    keeps the text rows of the last layer out of the loss, V4:185, but computes them like the reference).
    P: parameters by reference name; patches [L, C]; ids int64 [B, T]; text_mask [B, T]; pair_keep uint8 [B, L].
    dropout: None = off (the oracle comparison), or a `Dropout` plan.  precision: None = fp32 | 'bf16' (patches may come
    in fp32; the hidden states are then bf16).  Returns the last hidden state [B, 33 + T, 768]."""
    n = _Nodes(precision)
    layer_norm, patches = n.ln, n.act(patches)
    q = cfg.qformer
    nq, H, heads = q.q_rows, q.hidden, q.heads
    B, T = ids.shape
    pre = "relation_qformer.embeddings."
    query = torch.cat([P["rel_cls_query"][0], P["relation_query"][0]], dim=0)                      # V4:155-157
    emb = P[pre + "word_embeddings.weight"][ids] + P[pre + "position_embeddings.weight"][:T][None]
    h = layer_norm(torch.cat([query[None].expand(B, -1, -1), emb], dim=1), P[pre + "layernorm.weight"],
                   P[pre + "layernorm.bias"], q.ln_eps)
    dev = h.device
    dh = (lambda x: x) if dropout is None else dropout.hidden                                    # noqa: E731
    da = (lambda *a: None) if dropout is None else dropout.attn                                  # noqa: E731
    S, L = nq + T, patches.shape[0]
    h = dh(h)
    self_keep = torch.cat([torch.ones((B, nq), dtype=torch.uint8, device=dev), text_mask.to(torch.uint8)], dim=1)[:, None, :]
    cross_keep = pair_keep.to(torch.uint8)[:, None, :]
    scale = (H // heads) ** -0.5
    lin = lambda pfx, x: n.linear(x, P[pfx + ".weight"], P[pfx + ".bias"])  # noqa: E731
    attn, gelu, add = n.attn, n.gelu, n.resid
    for l in range(q.layers):
        p = f"relation_qformer.encoder.layer.{l}."
        a = attn(lin(p + "attention.attention.query", h), lin(p + "attention.attention.key", h),
                         lin(p + "attention.attention.value", h), self_keep, heads, scale, da(B, heads, S, S, dev))
        a = layer_norm(add(dh(lin(p + "attention.output.dense", a)), h), P[p + "attention.output.LayerNorm.weight"],
                       P[p + "attention.output.LayerNorm.bias"], q.ln_eps)
        q33 = a[:, :nq]
        kx = lin(p + "crossattention.attention.key", patches)[None]                           # shared by every pair
        vx = lin(p + "crossattention.attention.value", patches)[None]
        c = attn(lin(p + "crossattention.attention.query", q33), kx, vx, cross_keep, heads, scale,
                         da(B, heads, nq, L, dev))
        c = layer_norm(add(dh(lin(p + "crossattention.output.dense", c)), q33), P[p + "crossattention.output.LayerNorm.weight"],
                       P[p + "crossattention.output.LayerNorm.bias"], q.ln_eps)
        hq = layer_norm(add(dh(lin(p + "output_query.dense", gelu(lin(p + "intermediate_query.dense", c)))), c),
                        P[p + "output_query.LayerNorm.weight"], P[p + "output_query.LayerNorm.bias"], q.ln_eps)
        at = a[:, nq:]
        ht = layer_norm(add(dh(lin(p + "output.dense", gelu(lin(p + "intermediate.dense", at)))), at),
                        P[p + "output.LayerNorm.weight"], P[p + "output.LayerNorm.bias"], q.ln_eps)
        h = torch.cat([hq, ht], dim=1)
    return h


def llama_teacher_forcing(engine, cfg, X, seq_len, rope_pos, rows, precision=None):
    """Plain `language_model(inputs_embeds, attention_mask)` forward (V4:327-336) through the FROZEN Llama, on compact
    sequences X [K, S, D] (valid tokens first), rope_pos int32 [K, S] = each token's position in the reference's padded
    sequence (-1 behind a sequence's end), rows int64: flat row indices whose logits are wanted.  Returns fp32 logits.
    precision='bf16': `engine` holds bf16 matrices (the head's `_train_llm`), X may be bf16; the stream x is fp32."""
    n = _Nodes(precision)
    rms, rope, attn, silu = n.rms, n.rope, n.attn, n.silu
    m = cfg.llm
    K, S, D = X.shape
    dev = X.device
    valid = torch.arange(S, device=dev)[None, :] < seq_len[:, None]                            # [K, S]
    causal = torch.tril(torch.ones((S, S), dtype=torch.bool, device=dev))
    keep = (causal[None] & valid[:, None, :])
    keep = keep | (~valid)[:, :, None] & torch.eye(S, dtype=torch.bool, device=dev)[None]     # pad rows attend to themselves
    keep = keep.to(torch.uint8).contiguous()
    pos = rope_pos.clamp(min=0).reshape(-1).to(torch.int32).contiguous()
    cos, sin = engine.rope
    x = X.float() if n.bf16 else X                                            # the residual stream: fp32
    scale = m.head_dim ** -0.5
    for L in engine.layers:
        n1 = rms(x, L["ln1"], m.rms_eps)
        qkv = F.linear(n1, L["wqkv"])
        qh = rope(qkv[..., :D].reshape(K * S, D), pos, cos, sin, m.heads).view(K, S, D)
        if m.n_kv_heads == m.heads:
            kh = rope(qkv[..., D:2 * D].reshape(K * S, D), pos, cos, sin, m.heads).view(K, S, D)
            vh = qkv[..., 2 * D:].contiguous()
        else:
            # grouped-query attention: rotate the kv_heads key heads, then give every query head its group's key / value
            # head (repeat_interleave; autograd sums dK / dV over each group)
            Dk, G = m.kv_dim, m.kv_group
            kg = rope(qkv[..., D:D + Dk].reshape(K * S, Dk), pos, cos, sin, m.n_kv_heads)
            kh = kg.view(K, S, m.n_kv_heads, 1, m.head_dim).expand(-1, -1, -1, G, -1).reshape(K, S, D)
            vh = qkv[..., D + Dk:].reshape(K, S, m.n_kv_heads, 1, m.head_dim).expand(-1, -1, -1, G, -1).reshape(K, S, D)
        att = attn(qh, kh, vh, keep, m.heads, scale)
        x = n.resid(x, F.linear(att, L["wo"]))
        n2 = rms(x, L["ln2"], m.rms_eps)
        act = silu(F.linear(n2, L["wgu"]).view(K * S, -1)).view(K, S, -1)
        x = n.resid(x, F.linear(act, L["wdown"]))
    hfin = rms(x, engine.final_norm, m.rms_eps).reshape(K * S, D)
    return F.linear(hfin.index_select(0, rows), engine.lm_head).float()    # the loss takes fp32 logits
