"""Shared by the train_precision='bf16' tests: the CPU oracle's losses and gradients of a training golden, in fp32 and
inside torch.autocast('cpu', bfloat16) with fp32 leaves, computed once per process and never modified; and the recorded
autocast-vs-fp32 deviations (tests/golden/T_bf16_autocast_baseline.json) that serve as the yardstick `d_ref`."""
import functools
import json
import os

import torch

from tests import helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BASELINE = os.path.join(GOLDEN, "T_bf16_autocast_baseline.json")
CASES = ["T1_train_512_n7", "T2_train_768x1024_n9", "T4_gqa_train_512_n7"]      # T4: T1's draws behind a GQA LLM
SCALE_FLOOR = 1e-4                                                              # max |g_fp32| below it: rounding noise only


@functools.lru_cache(maxsize=None)
def load(case):
    """(golden, cfg, weights, inputs, oracle cfg, oracle weights): the oracle is multi-head, so a GQA case hands it the
    model with every key / value head repeated over its group - the same function (tests/test_gpu_gqa_head.py)."""
    if case.startswith("T4"):
        from tests import test_gpu_gqa_head as Q
        g, cfg, w, inputs = Q._train_case()
        cfg_o, w_o = Q.expand_to_mha(cfg, w)
    else:
        g, cfg, w, inputs = H.load_train_case(case)
        cfg_o, w_o = cfg, w
    return g, cfg, w, inputs, cfg_o, w_o


def trainable(w):
    return [k for k in w if not k.startswith("language_model.")]


@functools.lru_cache(maxsize=None)
def oracle(case, autocast=False):
    """({loss name: float}, {tensor name: fp32 gradient of the summed loss}) of oracle.psg_oracle.train_forward on the
    golden's draws, dropout off - as `_oracle_grads` of tests/test_gpu_train.py."""
    from openpsg_amd.categories import relation_categories
    from oracle import psg_oracle as O
    torch.set_num_threads(min(16, torch.get_num_threads()))
    g, cfg, w, inputs, cfg_o, w_o = load(case)
    names = trainable(w)
    wr = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in w_o.items()}
    meta = inputs["img_metas"][0]
    ids, tmask, llm_prompt, llm_label = H.train_prompts(inputs)
    gtm = inputs["gt_masks"][0].to_tensor(torch.float32, "cpu")
    # oneDNN picks its bf16 kernels (and their summation order) by the host's instruction set: a one-element gradient's
    # d_ref moved by 38 % between two hosts.  torch's own bf16 products are the same code everywhere.
    with torch.backends.mkldnn.flags(enabled=False), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        o = O.train_forward(wr, cfg_o, inputs["mask_features"], meta["masks_info"], meta["gt_rels"][0], gtm,
                            inputs["gt_semantic_seg"][0], ids, tmask, llm_prompt, llm_label, relation_categories,
                            sampled=g["sampled"], selected=g["selected"].tolist())
        total = o["binary_rel_cls_loss"].float() + o["rel_llm_loss"].float()
    og = torch.autograd.grad(total, [wr[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(wr[k]) if r is None else r.detach().float()) for k, r in zip(names, og)}
    losses = {k: float(o[k].detach()) for k in ("binary_rel_cls_loss", "rel_llm_loss")}
    return losses, grads


def deviation(got, ref):
    """(||got - ref||_2 / ||ref||_2, cosine) of two gradients, in float64."""
    a, b = got.double().flatten(), ref.double().flatten()
    nb = float(b.norm())
    return float((a - b).norm()) / nb, float(a @ b) / (float(a.norm()) * nb + 1e-300)


def compute_baseline(case):
    """What the baseline file records for one case: per trainable tensor above the scale floor d_ref and the cosine of
    the autocast gradient against the fp32 one, and the relative deviation of both losses."""
    (l32, g32), (l16, g16) = oracle(case, False), oracle(case, True)
    tensors = {}
    for k, ref in g32.items():
        if float(ref.abs().max()) > SCALE_FLOOR:
            d, c = deviation(g16[k], ref)
            tensors[k] = dict(d_ref=d, cos=c)
    return dict(losses={k: abs(l16[k] / l32[k] - 1) for k in l32}, tensors=tensors)


def baseline():
    with open(BASELINE) as f:
        return json.load(f)


def to_dev(inputs):
    out = dict(inputs)
    out["mask_features"] = inputs["mask_features"].cuda()
    out["gt_semantic_seg"] = [inputs["gt_semantic_seg"][0].cuda()]
    return out


def make_head(cfg, w, dtype, train_precision="bf16", **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    kw.setdefault("train_dropout", False)
    h = RelationTransformerHeadV4(dtype=dtype, device="cuda:0", qformer_vocab_size=cfg.qformer.vocab, llm_config=cfg.llm,
                                  llm_feature_size=cfg.llm.hidden, tokenizers="word", max_object_num=cfg.max_object_num,
                                  train_precision=train_precision, **kw)
    h.load_weights({k: v.clone() for k, v in w.items()})
    return h

