"""train_precision='bf16' through the head (`-m gpu`): the gradient path in the bf16 model of DESIGN 13 against the fp32
CPU oracle, bounded by the deviation torch.autocast(bfloat16) itself shows on the oracle
(tests/golden/T_bf16_autocast_baseline.json, tests/test_train_bf16_cpu.py)."""
import random

import pytest
import torch

from tests import helpers as H
from tests import train_bf16_common as C

pytestmark = pytest.mark.gpu

T1, T2, T4 = C.CASES
GROUPS = ("patch_embed.proj.weight", "relation_query", "rel_cls_query", "binary_rel_cls_pred.weight",
          "language_projection.weight", "relation_qformer.embeddings.word_embeddings.weight",
          "relation_qformer.encoder.layer.0.crossattention.attention.key.weight")


def _step(head, g, inputs, dropout=False):
    head.zero_grad(set_to_none=True)
    out = head.forward_train_grad(C.to_dev(inputs), sampled=g["sampled"], selected=g["selected"].tolist(), dropout=dropout)
    (out["binary_rel_cls_loss"] + out["rel_llm_loss"]).backward()
    torch.cuda.synchronize()
    return out


def test_bf16_head_raises_without_the_option_and_trains_with_it():
    g, cfg, w, inputs, _, _ = C.load(T1)
    plain = C.make_head(cfg, w, "bf16", train_precision=None)
    assert not any(p.requires_grad for p in plain.parameters())
    plain.train(True)
    with pytest.raises(NotImplementedError):
        plain(C.to_dev(inputs))
    head = C.make_head(cfg, w, "bf16")
    assert not head.training and all(p.requires_grad and p.dtype == torch.float32 for p in head.parameters())
    head.train(True)
    torch.manual_seed(5)
    random.seed(5)
    out = head(C.to_dev(inputs))
    assert set(out) == {"binary_rel_cls_loss", "rel_llm_loss"}
    assert all(v.requires_grad and v.dtype == torch.float32 for v in out.values())
    with pytest.raises(NotImplementedError):
        head.forward_batch([C.to_dev(inputs)])


def _check_gradients(case, dtype):
    g, cfg, w, inputs, _, _ = C.load(case)
    head = C.make_head(cfg, w, dtype)
    head.train(True)
    out = _step(head, g, inputs)
    for k in ("binary_rel_cls_loss", "rel_llm_loss"):
        r = abs(float(out[k].detach()) / float(g[k]) - 1)
        print(f"{case} {dtype}: {k} deviates {r:.3e} from the golden")
        assert r < 0.05
    _, ref = C.oracle(case, False)
    rec = C.baseline()[case]["tensors"]
    mine = dict(head.named_parameters())
    worst, checked = (0.0, None), 0
    for k, r in ref.items():
        if float(r.abs().max()) <= C.SCALE_FLOOR:
            continue
        assert mine[k].grad is not None and mine[k].grad.dtype == torch.float32, k
        d_head, _ = C.deviation(mine[k].grad.cpu(), r)
        d_ref = rec[k]["d_ref"]
        checked += 1
        if d_head / d_ref > worst[0]:
            worst = (d_head / d_ref, k)
        assert d_head <= 2 * d_ref + 2.0 ** -8, f"{k}: d_head {d_head:.4f} against d_ref {d_ref:.4f}"
    print(f"{case} {dtype}: {checked} tensors, worst d_head / d_ref = {worst[0]:.3f} ({worst[1]})")
    assert checked >= 60
    for k in GROUPS:
        assert float(mine[k].grad.abs().max()) > 0, k
    return head


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [T1, T2])
def test_bf16_gradients_within_twice_the_autocast_deviation(case, dtype):
    _check_gradients(case, dtype)


def test_bf16_gradients_gqa():
    head = _check_gradients(T4, "bf16")
    assert head.llm_engine.kv is not None                       # the grouped-query branch of llama_teacher_forcing ran


def test_bf16_dropout_is_finite_nonzero_and_reproducible():
    from openpsg_amd import train_graph as G
    g, cfg, w, inputs, _, _ = C.load(T1)
    head = C.make_head(cfg, w, "bf16", train_dropout=True)
    head.train(True)
    runs = []
    for _ in range(2):
        plan = G.Dropout(cfg.qformer.hidden_dropout, cfg.qformer.attn_dropout, generator=torch.Generator().manual_seed(11))
        out = _step(head, g, inputs, dropout=plan)
        runs.append(({k: v.detach().clone() for k, v in out.items()},
                     {k: p.grad.clone() for k, p in head.named_parameters()}))
    losses, grads = runs[0]
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    for k in GROUPS:
        assert bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0, k
    plain = head.forward_train_grad(C.to_dev(inputs), sampled=g["sampled"], selected=g["selected"].tolist(), dropout=False)
    assert abs(float(plain["binary_rel_cls_loss"].detach()) - float(losses["binary_rel_cls_loss"])) > 1e-3
    for k, v in losses.items():
        assert torch.equal(v, runs[1][0][k]), k
    for k, v in grads.items():
        assert torch.equal(v, runs[1][1][k]), k


def test_bf16_training_steps_through_forward_reduce_the_loss():
    g, cfg, w, inputs, _, _ = C.load(T1)
    head = C.make_head(cfg, w, "bf16")
    head.train(True)
    opt = torch.optim.AdamW([p for p in head.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.0)
    dev_in = C.to_dev(inputs)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        torch.manual_seed(5)                                     # forward() draws the sampler itself: the same draws each step
        random.seed(5)
        out = head(dev_in)
        total = out["binary_rel_cls_loss"] + out["rel_llm_loss"]
        total.backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in head.parameters() if p.grad is not None)
        opt.step()
        losses.append(float(total.detach()))
    print("bf16 summed loss over 4 AdamW steps:", [round(x, 4) for x in losses])
    assert losses[-1] < losses[0]
    eng = head.llm_engine
    assert all(t.grad is None and not t.requires_grad for t in (eng.lm_head, eng.embed, *eng.layers[0].values()))


def test_inference_is_unchanged_by_the_option():
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    inputs = dict(mask_features=scene["mask_features"].cuda(), img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"].cuda())])

    def infer(h):
        with torch.no_grad():
            h(inputs)
        return h.last["exist_logit"].clone(), h.last["tokens_host"].copy()
    base = infer(C.make_head(cfg, w, "bf16", train_precision=None, suppress_eos=True))
    head = C.make_head(cfg, w, "bf16", suppress_eos=True)
    for _ in range(2):
        logit, toks = infer(head)
        assert torch.equal(logit, base[0]) and (toks == base[1]).all()
        # a training step (T1's scene: the same architecture), then the masters restored: the same bits again
        gt, _, _, tin, _, _ = C.load(T1)
        saved = {k: p.detach().clone() for k, p in head.named_parameters()}
        head.train(True)
        opt = torch.optim.SGD(head.parameters(), lr=1e-3)
        _step(head, gt, tin)
        opt.step()
        head.train(False)
        assert head._train_llm_copy is None
        with torch.no_grad():
            for k, p in head.named_parameters():
                p.copy_(saved[k])
        head.train(False)                                        # drops the packed copies built from the stepped masters
