"""Captures the multiclass goldens from the reference head (CPU only, run once, by hand):

    python tools/capture_multiclass_golden.py

  tests/golden/T3_multiclass_train_512_n7.npz  the TRAINING branch with rel_cls_type='binary+multiclass' on T1's scene
                                               and draws: sampled / selected pairs, the multiclass head's logits (forward
                                               hook), the three losses (V4:196-204, 345-351, 463-495)
  tests/golden/G7_multiclass_512_n10.npz       the EVAL branch on G1's scene: the [N^2, R] multiclass logits and the
                                               existence logits (hooks), and the error the reference raises at V4:241
                                               (`multiclass_rel_cls_pred[:, i, i, :] = 0` on a 2-D tensor)

The reference is imported with oracle/capture_reference.py's helpers (unchanged); `multiclass_rel_cls_pred` is attached to
the head they build (which has the binary head only) and filled from `make_weights_numpy` of the multiclass config, so a
test can rebuild every weight from the seed.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import capture_reference as CR  # noqa: E402
from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm  # noqa: E402
from openpsg_amd.synthetic import make_scene, make_train_scene  # noqa: E402
from openpsg_amd.weights import make_weights_numpy  # noqa: E402

TYPE = "binary+multiclass"
G7_SCENE = dict(pad_hw=(512, 512), num_objects=10, seed=1, void_id=0, force_id0=True, tiny_object=True)   # G1's
G7_WEIGHT_SEED = 11


def mc_config(llm) -> PSGConfig:
    return PSGConfig(qformer=QFormerConfig(vocab=512), llm=llm, max_object_num=30, rel_cls_type=TYPE)


def build_multiclass_reference(mod, cfg, w):
    """The reference head of CR.build_reference_head with rel_cls_type = TYPE and its multiclass Linear (V4:93-95)."""
    mc = {k: w[k] for k in w if k.startswith("multiclass_rel_cls_pred.")}
    h = CR.build_reference_head(mod, cfg, {k: v for k, v in w.items() if k not in mc})
    h.rel_cls_type = TYPE
    lin = nn.Linear(cfg.qformer.hidden, len(mod.relation_categories))
    with torch.no_grad():
        lin.weight.copy_(mc["multiclass_rel_cls_pred.weight"])
        lin.bias.copy_(mc["multiclass_rel_cls_pred.bias"])
    h.multiclass_rel_cls_pred = lin.eval()
    return h


def capture_train(mod):
    name = "T1_train_512_n7"
    pad_hw, cats, gt_rels, scene_seed, weight_seed, draw_seed = CR.TRAIN_CASES[name]
    llm = tiny_llm(256, 2, 512, 512)
    cfg = mc_config(llm)
    w = make_weights_numpy(cfg, seed=weight_seed)
    h = build_multiclass_reference(mod, cfg, w)
    h.sampled_qformer_batch_size, h.qformer_neg_over_pos, h.rel_cls_loss_weight = 32, 3, 50.0   # V4:29-32
    h.training = True
    torch.Tensor.cuda = lambda self, *a, **k: self
    inputs = make_train_scene(pad_hw, cats, gt_rels, seed=scene_seed)
    cap = {}
    real_sampler = h.qformer_sampler
    h.qformer_sampler = lambda t: cap.setdefault("sampled", real_sampler(t).clone())
    h.binary_rel_cls_pred.register_forward_hook(lambda m_, i, o: cap.__setitem__("bce_logit", o.detach().clone()))
    h.multiclass_rel_cls_pred.register_forward_hook(lambda m_, i, o: cap.__setitem__("mc_logit", o.detach().clone()))
    real_sample = random.sample

    def sample(pop, k):
        r = real_sample(pop, k)
        cap.setdefault("selected", list(r))
        return r
    mod.random.sample = sample
    torch.manual_seed(draw_seed)
    random.seed(draw_seed)
    try:
        with torch.no_grad():
            out = h(inputs)
    finally:
        mod.random.sample = real_sample
    assert set(out) == {"binary_rel_cls_loss", "multiclass_rel_cls_loss", "rel_llm_loss"}, sorted(out)
    res = dict(
        rel_cls_type=np.array(TYPE), base_case=np.array(name),
        pad_hw=np.array(pad_hw), categories=np.array(cats, dtype=np.int64), gt_rels=np.array(gt_rels, dtype=np.int64),
        scene_seed=np.int64(scene_seed), weight_seed=np.int64(weight_seed),
        llm_hidden=np.int64(llm.hidden), llm_layers=np.int64(llm.layers), llm_inter=np.int64(llm.inter),
        llm_vocab=np.int64(llm.vocab),
        mc_weight=w["multiclass_rel_cls_pred.weight"].numpy(), mc_bias=w["multiclass_rel_cls_pred.bias"].numpy(),
        sampled=cap["sampled"].numpy().astype(np.int64), selected=np.array(cap["selected"], dtype=np.int64),
        bce_logit=cap["bce_logit"].reshape(-1).numpy(), mc_logit=cap["mc_logit"].numpy(),
        binary_rel_cls_loss=np.float32(out["binary_rel_cls_loss"]),
        multiclass_rel_cls_loss=np.float32(out["multiclass_rel_cls_loss"]),
        rel_llm_loss=np.float32(out["rel_llm_loss"]),
    )
    path = os.path.join(REPO, "tests", "golden", "T3_multiclass_train_512_n7.npz")
    np.savez_compressed(path, **res)
    print(f"T3: sampled={len(res['sampled'])} selected={res['selected'].tolist()} "
          f"bce={float(res['binary_rel_cls_loss']):.6f} mc={float(res['multiclass_rel_cls_loss']):.6f} "
          f"llm={float(res['rel_llm_loss']):.6f} -> {os.path.getsize(path) / 1024:.0f} KiB")


def capture_eval(mod):
    llm = tiny_llm(256, 2, 512, 512)
    cfg = mc_config(llm)
    w = make_weights_numpy(cfg, seed=G7_WEIGHT_SEED)
    h = build_multiclass_reference(mod, cfg, w)
    scene = make_scene(**G7_SCENE)
    cap = {}
    h.binary_rel_cls_pred.register_forward_hook(lambda m_, i, o: cap.__setitem__("exist_logit", o.detach().clone()))
    h.multiclass_rel_cls_pred.register_forward_hook(lambda m_, i, o: cap.__setitem__("mc_logit", o.detach().clone()))
    torch.Tensor.cuda = lambda self, *a, **k: self
    inputs = dict(mask_features=scene["mask_features"], img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"])])
    err = None
    with torch.no_grad():
        try:
            h(inputs)
        except IndexError as e:                                   # V4:241, the 2-D tensor indexed with four indices
            err = "IndexError: " + str(e)
    assert err is not None and "too many indices" in err, err
    n = len(scene["object_id_list"])
    assert cap["mc_logit"].shape == (n * n, len(mod.relation_categories)), cap["mc_logit"].shape
    res = dict(
        rel_cls_type=np.array(TYPE), scene_kw=np.array(repr(G7_SCENE)), weight_seed=np.int64(G7_WEIGHT_SEED),
        llm_hidden=np.int64(llm.hidden), llm_layers=np.int64(llm.layers), llm_inter=np.int64(llm.inter),
        llm_vocab=np.int64(llm.vocab),
        object_ids=np.array([int(i) for i in scene["object_id_list"]], dtype=np.int32),
        mc_logit=cap["mc_logit"].numpy(), exist_logit=cap["exist_logit"][:, 0].numpy(),
        reference_error=np.array(err),
    )
    path = os.path.join(REPO, "tests", "golden", "G7_multiclass_512_n10.npz")
    np.savez_compressed(path, **res)
    print(f"G7: N={n} mc_logit={tuple(res['mc_logit'].shape)} err={err!r} -> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = CR.import_reference_head()
    capture_train(mod)
    capture_eval(mod)


if __name__ == "__main__":
    main()
