"""The multiclass relation head on the GPU (`-m gpu`): K8b psg_multiclass_head and the row losses of
psg_train_mlcce_fwd / _bwd against float64, K9b psg_topk_large against a stable sort, the eval branch against the
reference's logits (tests/golden/G7_*.npz), the training branch against the reference's losses (tests/golden/T3_*.npz)
with its gradients against autograd through the oracle, and the three inference entry points against each other."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


# ---- K8b ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("nq", [1, 33])
def test_multiclass_head_kernel_vs_float64(dtype, nq):
    from openpsg_amd import ops
    g = torch.Generator().manual_seed(7 + nq)
    for P, R in ((0, 56), (1, 1), (97, 56), (130, 128), (64, 17)):
        N = max(1, int(np.sqrt(max(P, 1))) + 1)
        x = torch.randn(P * nq, 768, generator=g).to(DT[dtype])
        w = torch.randn(R, 768, generator=g) / 768 ** 0.5 * 2
        b = torch.randn(R, generator=g) * 0.05
        pidx = torch.randperm(N * N, generator=g)[:P].to(torch.int32) if P <= N * N else torch.arange(P, dtype=torch.int32)
        lg, pr = ops.multiclass_head(x.cuda(), w.cuda(), b.cuda(), P, nq, pidx.cuda(), N)
        torch.cuda.synchronize()
        assert lg.shape == (P, R) and pr.shape == (P, R)
        if P == 0:
            continue
        xs = x.double().view(P, nq, 768)[:, 0]                            # the stored (rounded) values, exactly
        want = xs @ w.double().T + b.double()
        # fp32 accumulation over 768 products: bound by the magnitude sum (test_gpu_train_kernels.py-style)
        bound = 2e-5 * (xs.abs() @ w.double().abs().T + b.double().abs()) + 1e-6
        err = (lg.cpu().double() - want).abs()
        assert bool((err <= bound).all()), f"P={P} R={R}: max err {float(err.max()):.3e}"
        p = torch.sigmoid(want)
        diag = (pidx // N == pidx % N).to(torch.bool)
        p[diag] = 0
        assert float((pr.cpu().double() - p).abs().max()) < 1e-5
        assert bool((pr.cpu()[diag] == 0).all())


def test_multiclass_head_refuses_more_than_128_classes():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    x = torch.zeros(4, 768, device="cuda")
    with pytest.raises(PsgHipError, match="R=129"):
        ops.multiclass_head(x, torch.zeros(129, 768, device="cuda"), torch.zeros(129, device="cuda"), 4, 1)


# ---- K9b ----------------------------------------------------------------------------------------------------------
def _ref_topk(s, k):
    v = np.where(np.isnan(s), -np.inf, s).astype(np.float64)
    v = np.where(v == 0, 0.0, v)                                          # -0 == +0
    order = np.lexsort((np.arange(v.size), -v))[:k]
    idx = np.full(k, -1, np.int64)
    val = np.full(k, -np.inf, np.float32)
    idx[:order.size] = order
    val[:order.size] = np.where(np.isnan(s[order]), -np.inf, s[order])
    return idx, val


def _scores(n, kind, rng):
    if kind == "random":
        return rng.random(n, dtype=np.float32)
    if kind == "ties":                                                    # few distinct values, +-0, NaN, -inf
        s = rng.integers(0, 5, n).astype(np.float32) / 4
        s[rng.random(n) < 0.1] = -0.0
        s[rng.random(n) < 0.05] = np.nan
        s[rng.random(n) < 0.02] = -np.inf
        return s
    if kind == "equal":
        return np.full(n, 0.5, np.float32)
    return (1 / (1 + np.exp(-rng.standard_normal(n) * 3))).astype(np.float32)   # sigmoid scores of one image


@pytest.mark.parametrize("n", [1, 55, 101, 3072, 4097, 140_000, 560_001])
def test_topk_large_equals_a_stable_sort(n):
    from openpsg_amd import ops
    rng = np.random.default_rng(n)
    for kind in ("random", "ties", "equal", "sigmoid"):
        s = _scores(n, kind, rng)
        sd = torch.from_numpy(s).cuda()
        for k in (1, 20, 100, 256):
            idx, val = ops.topk_large(sd, k)
            want_i, want_v = _ref_topk(s, k)
            got_i, got_v = idx.cpu().numpy(), val.cpu().numpy()
            assert np.array_equal(got_i, want_i), f"n={n} {kind} k={k}"
            assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), f"n={n} {kind} k={k}"
            if n <= 3072 and k <= 64:                                      # the same as psg_topk where both run
                ti, tv = ops.topk(sd, k)
                assert np.array_equal(ti.cpu().numpy(), got_i)


# ---- K3 row losses -------------------------------------------------------------------------------------------------
def _mlcce64(y, x):
    z = (1 - 2 * y) * x
    zero = torch.zeros_like(z[..., :1])
    neg = torch.cat([z - y * 9999, zero], -1)
    pos = torch.cat([z - (1 - y) * 9999, zero], -1)
    return torch.logsumexp(neg, -1) + torch.logsumexp(pos, -1)


def test_mlcce_kernels_vs_float64():
    from openpsg_amd import ops
    g = torch.Generator().manual_seed(3)
    for S, R in ((1, 1), (16, 56), (33, 128), (5, 200)):
        x = (torch.rand(S, R, generator=g) * 2 - 1) * 50                  # |logit| up to 50
        y = (torch.rand(S, R, generator=g) < 0.1).float()
        y[0] = 0                                                          # a row of all zeros ...
        if S > 1:
            y[1] = 1                                                      # ... and one of all ones
        dl = torch.rand(S, generator=g)
        loss = ops.mlcce_rows(x.cuda(), y.cuda())
        d = ops.mlcce_rows_bwd(x.cuda(), y.cuda(), dl.cuda())
        x64 = x.double().requires_grad_(True)
        want = _mlcce64(y.double(), x64)
        (gw,) = torch.autograd.grad((want * dl.double()).sum(), [x64])
        assert float(((loss.cpu().double() - want.detach()).abs() / (want.detach().abs() + 1)).max()) < 2e-6
        assert float((d.cpu().double() - gw).abs().max()) < 2e-6


# ---- G7: the eval branch ---------------------------------------------------------------------------------------------
def _g7():
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_numpy
    g = dict(np.load(os.path.join(GOLDEN, "G7_multiclass_512_n10.npz")))
    llm = tiny_llm(int(g["llm_hidden"]), int(g["llm_layers"]), int(g["llm_inter"]), int(g["llm_vocab"]))
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=llm, max_object_num=30, rel_cls_type=str(g["rel_cls_type"]))
    w = make_weights_numpy(cfg, seed=int(g["weight_seed"]))
    scene = make_scene(**ast.literal_eval(str(g["scene_kw"])))
    return g, cfg, w, scene


def _head(cfg, w, dtype, rel_cls_type, **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    h = RelationTransformerHeadV4(dtype=dtype, device="cuda:0", qformer_vocab_size=cfg.qformer.vocab, llm_config=cfg.llm,
                                  llm_feature_size=cfg.llm.hidden, tokenizers="word", suppress_eos=True,
                                  rel_cls_type=rel_cls_type, max_object_num=cfg.max_object_num, **kw)
    own = set(dict(h.named_parameters()))
    h.load_weights({k: v for k, v in w.items() if k in own or k.startswith("language_model.")})
    return h


def _inputs(scene):
    return dict(mask_features=scene["mask_features"].cuda(), img_metas=[scene["img_meta"]],
                object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"].cuda())])


def _ranking(logit64, N, k=100):
    s = torch.sigmoid(logit64)
    s[torch.arange(N) * N + torch.arange(N)] = 0
    flat = s.reshape(-1).numpy()
    return np.lexsort((np.arange(flat.size), -flat))[:k], flat


@pytest.mark.parametrize("dtype", ["fp32", "fp32s", "bf16"])
def test_g7_multiclass_eval_vs_reference(dtype):
    g, cfg, w, scene = _g7()
    N, R = len(g["object_ids"]), g["mc_logit"].shape[1]
    head = _head(cfg, w, dtype, "binary+multiclass")
    out = head(_inputs(scene))
    torch.cuda.synchronize()
    mc_logit = head.last["mc_logit"].cpu().double()
    err = float((mc_logit - torch.from_numpy(g["mc_logit"]).double()).abs().max())
    order, flat = _ranking(torch.from_numpy(g["mc_logit"]).double(), N)
    L = len(out["rel_pred"]) - 100
    mc_trip = [tuple(t) for t in out["rel_pred"][L:]]
    want = [(f // R // N, f // R % N, f % R) for f in order.tolist()]
    assert all(isinstance(v, float) for v in out["rel_score"][L:]) and out["rel_score"][:L] == [1] * L
    print(f"{dtype}: |mc logit - reference| {err:.2e}, {L} LLM triples")
    if dtype == "bf16":
        assert err < 0.25
        assert len(set(mc_trip) & set(want)) >= 70
    else:
        assert err < 1e-4
        # equal to the float64 ranking of the reference's logits up to order swaps inside a 1e-5 score band
        assert set(mc_trip) == set(want) or all(abs(flat[a] - flat[b]) < 1e-5 for a, b in zip(
            [(i * N + j) * R + r for i, j, r in mc_trip], order.tolist()))
        sc = np.array(out["rel_score"][L:])
        assert np.abs(sc - flat[[(i * N + j) * R + r for i, j, r in mc_trip]]).max() < 1e-5
        assert np.all(np.diff(sc) <= 0)
        # the binary part is untouched: a 'binary' head on the same weights gives the same bits
        hb = _head(cfg, w, dtype, "binary")
        ob = hb(_inputs(scene))
        torch.cuda.synchronize()
        assert torch.equal(hb.last["exist_logit"], head.last["exist_logit"])
        assert torch.equal(hb.last["selected"], head.last["selected"])
        assert np.array_equal(hb.last["tokens_host"], head.last["tokens_host"])
        assert ob["rel_pred"] == out["rel_pred"][:L] and ob["rel_score"] == out["rel_score"][:L]
        e_ex = float(np.abs(head.last["exist_logit"].cpu().numpy() - g["exist_logit"]).max())
        assert e_ex < 1e-3


def test_entry_points_agree_and_multiclass_alone_runs_no_decode():
    g, cfg, w, scene = _g7()
    head = _head(cfg, w, "fp32", "binary+multiclass")
    a = head(_inputs(scene))
    b = head.submit(_inputs(scene)).result()
    c = head.forward_batch([_inputs(scene), _inputs(scene)])
    assert a == b
    # (forward_batch's LLM part may round differently: its decode GEMMs see both images' rows at once)
    for r in c:
        assert r["rel_pred"][-100:] == a["rel_pred"][-100:] and r["rel_score"][-100:] == a["rel_score"][-100:]
    mono = _head(cfg, w, "fp32", "multiclass")
    assert "binary_rel_cls_pred.weight" not in dict(mono.named_parameters())

    def no_decode(*a_, **k_):
        raise AssertionError("'multiclass' alone launched the LLM decode")
    mono.llm_engine.generate = no_decode
    m1 = mono(_inputs(scene))
    m2 = mono.submit(_inputs(scene)).result()
    m3 = mono.forward_batch([_inputs(scene)])[0]
    assert m1 == m2 == m3 and len(m1["rel_pred"]) == 100
    assert m1["rel_pred"] == a["rel_pred"][-100:] and m1["rel_score"] == a["rel_score"][-100:]
    assert mono.last["exist_logit"] is None and mono.last["selected"] is None
    assert mono(_inputs(scene), is_generation=False) == m1


def test_c4_geometry_hundred_objects_in_head():
    """BASELINE C4's object count: 10 000 pairs x 56 classes = 560 000 scores through psg_topk_large inside the head."""
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_numpy
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 1, 512, 512), max_object_num=100,
                    rel_cls_type="binary+multiclass")
    w = make_weights_numpy(cfg, seed=4)
    scene = make_scene(pad_hw=(1024, 1024), num_objects=100, seed=9, void_id=133)
    head = _head(cfg, w, "bf16", "binary+multiclass")
    out = head(_inputs(scene), is_generation=False)
    torch.cuda.synchronize()
    prob = head.last["mc_prob"]
    assert prob.shape == (10_000, 56)
    order = torch.sort(-prob.reshape(-1).double(), stable=True).indices[:100].cpu().numpy()
    got = [(i * 100 + j) * 56 + r for i, j, r in out["rel_pred"]]
    assert got == order.tolist() and len(out["rel_pred"]) == 100
    assert float(prob[torch.arange(100, device="cuda") * 101].abs().max()) == 0.0


# ---- T3: the training branch ---------------------------------------------------------------------------------------
def _t3():
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.synthetic import make_train_scene
    from openpsg_amd.weights import make_weights_numpy
    g = dict(np.load(os.path.join(GOLDEN, "T3_multiclass_train_512_n7.npz")))
    llm = tiny_llm(int(g["llm_hidden"]), int(g["llm_layers"]), int(g["llm_inter"]), int(g["llm_vocab"]))
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=llm, max_object_num=30, rel_cls_type=str(g["rel_cls_type"]))
    w = make_weights_numpy(cfg, seed=int(g["weight_seed"]))
    assert np.array_equal(w["multiclass_rel_cls_pred.weight"].numpy(), g["mc_weight"])
    inputs = make_train_scene(tuple(int(v) for v in g["pad_hw"]), [int(c) for c in g["categories"]],
                              [tuple(int(v) for v in r) for r in g["gt_rels"]], seed=int(g["scene_seed"]))
    return g, cfg, w, inputs


def _train_dev(inputs):
    out = dict(inputs)
    out["mask_features"] = inputs["mask_features"].cuda()
    out["gt_semantic_seg"] = [inputs["gt_semantic_seg"][0].cuda()]
    return out


KEYS = ("binary_rel_cls_loss", "multiclass_rel_cls_loss", "rel_llm_loss")


def test_t3_training_losses_and_gradients_vs_reference():
    from openpsg_amd.categories import relation_categories
    from oracle import psg_oracle as O
    g, cfg, w, inputs = _t3()
    head = _head(cfg, w, "fp32", "binary+multiclass", train_dropout=False)
    head.train(True)
    sel = g["selected"].tolist()
    lv = head.forward_train(_train_dev(inputs), sampled=g["sampled"], selected=sel)
    out = head.forward_train_grad(_train_dev(inputs), sampled=g["sampled"], selected=sel, dropout=False)
    assert tuple(lv) == KEYS and tuple(out) == KEYS
    for k in KEYS:
        for v in (lv[k], out[k].detach()):
            assert abs(float(v) - float(g[k])) <= 1e-3 * abs(float(g[k])), (k, float(v), float(g[k]))
    assert float(np.abs(head.last["mc_logit"].cpu().numpy() - g["mc_logit"]).max()) < 1e-3
    # gradients: autograd through the oracle composition (patch_embed -> qformer_forward -> heads -> restated loss)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    trainable = [k for k in w if not k.startswith("language_model.")]
    mine = dict(head.named_parameters())
    cap = {}
    real_qf = O.qformer_forward

    def qf(*a, **k):
        cap["out_s"] = real_qf(*a, **k)
        return cap["out_s"]
    ids, tmask, llm_prompt, llm_label = H.train_prompts(inputs)
    meta = inputs["img_metas"][0]
    gtm = inputs["gt_masks"][0].to_tensor(torch.float32, "cpu")
    for which in ("multiclass", "sum"):
        for p in mine.values():
            p.grad = None
        out = head.forward_train_grad(_train_dev(inputs), sampled=g["sampled"], selected=sel, dropout=False)
        (out["multiclass_rel_cls_loss"] if which == "multiclass" else sum(out.values())).backward()
        torch.cuda.synchronize()
        wr = {k: (v.clone().requires_grad_(True) if k in trainable else v) for k, v in w.items()}
        O.qformer_forward = qf
        try:
            o = O.train_forward(wr, cfg, inputs["mask_features"], meta["masks_info"], meta["gt_rels"][0], gtm,
                                inputs["gt_semantic_seg"][0], ids, tmask, llm_prompt, llm_label, relation_categories,
                                sampled=g["sampled"], selected=sel)
        finally:
            O.qformer_forward = real_qf
        n = len(meta["masks_info"])
        target = torch.zeros((n, n, 56))
        for i, j, r in meta["gt_rels"][0]:
            target[i, j, r] = 1
        y = target.reshape(-1, 56)[torch.as_tensor(g["sampled"])]
        ml = F.linear(cap["out_s"][:, 0], wr["multiclass_rel_cls_pred.weight"], wr["multiclass_rel_cls_pred.bias"])
        rows = _mlcce64(y, ml)
        mloss = torch.mean(rows * (rows / rows.max())) * 50.0
        total = mloss if which == "multiclass" else mloss + o["binary_rel_cls_loss"] + o["rel_llm_loss"]
        og = torch.autograd.grad(total, [wr[k] for k in trainable], allow_unused=True)
        checked = 0
        for k, ref in zip(trainable, og):
            got = mine[k].grad
            got = torch.zeros_like(mine[k]).cpu() if got is None else got.cpu()
            ref = torch.zeros_like(got) if ref is None else ref
            scale, err = float(ref.abs().max()), float((got - ref).abs().max())
            checked += scale > 0
            floor = 3e-5 if k.endswith("attention.key.bias") else 5e-6
            assert err <= 2e-3 * scale + floor, f"{which} {k}: {err:.3e} at scale {scale:.3e}"
        assert checked >= 30
        assert float(mine["multiclass_rel_cls_pred.weight"].grad.abs().max()) > 0
