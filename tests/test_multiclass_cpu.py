"""rel_cls_type='binary+multiclass' / 'multiclass' without a GPU: constructor and parameter schema, the multiclass loss
restated in float64 against the reference's training branch (tests/golden/T3_*.npz), the corrected top-100 decode of the
reference's eval-branch logits (tests/golden/G7_*.npz), and the refusal of pair-sharded multiclass pipelines."""
import json
import os

import numpy as np
import pytest
import torch

from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
from openpsg_amd.weights import head_shapes, make_weights_numpy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_KEYS = {"multiclass_rel_cls_pred.weight", "multiclass_rel_cls_pred.bias"}
BIN_KEYS = {"binary_rel_cls_pred.weight", "binary_rel_cls_pred.bias"}


def _cpu_head(rel_cls_type):
    from openpsg_amd.head import RelationTransformerHeadV4
    return RelationTransformerHeadV4(rel_cls_type=rel_cls_type, device="cpu", qformer_vocab_size=512,
                                     llm_config=tiny_llm(256, 1, 512, 512), llm_feature_size=256, tokenizers="word")


@pytest.mark.parametrize("rel_cls_type", ["binary+multiclass", "multiclass"])
def test_constructor_accepts_the_multiclass_types(rel_cls_type):
    head = _cpu_head(rel_cls_type)
    sd = head.state_dict()
    assert tuple(sd["multiclass_rel_cls_pred.weight"].shape) == (56, 768)
    assert tuple(sd["multiclass_rel_cls_pred.bias"].shape) == (56,)
    assert ("binary_rel_cls_pred.weight" in sd) == (rel_cls_type == "binary+multiclass")
    assert head.has_multiclass and head.has_binary == (rel_cls_type == "binary+multiclass")


def test_unknown_type_raises():
    with pytest.raises(ValueError):
        _cpu_head("ternary")
    with pytest.raises(ValueError):
        head_shapes(PSGConfig(rel_cls_type="multi"))


def test_key_sets_are_the_reference_keys_plus_or_minus_the_two_heads():
    ref = json.load(open(os.path.join(GOLDEN, "reference_state_dict_keys.json")))
    shapes = {t: head_shapes(PSGConfig(rel_cls_type=t)) for t in ("binary", "binary+multiclass", "multiclass")}
    assert set(shapes["binary"]) == set(ref)
    assert set(shapes["binary+multiclass"]) == set(ref) | MC_KEYS
    assert set(shapes["multiclass"]) == (set(ref) - BIN_KEYS) | MC_KEYS
    assert list(shapes["multiclass"]["multiclass_rel_cls_pred.weight"]) == [56, 768]
    # 'binary': the same draws as before the multiclass option existed (the existing goldens depend on them)
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 1, 512, 512))
    w = make_weights_numpy(cfg, seed=3, with_llm=False)
    assert not (set(w) & MC_KEYS) and set(w) >= BIN_KEYS


def _mlcce64(y_true, y_pred):
    """V4:484-495 in float64: the +-9999 masks and the concatenated zero as written."""
    y_pred = (1 - 2 * y_true) * y_pred
    neg = torch.cat([y_pred - y_true * 9999, torch.zeros_like(y_pred[..., :1])], dim=-1)
    pos = torch.cat([y_pred - (1 - y_true) * 9999, torch.zeros_like(y_pred[..., :1])], dim=-1)
    return torch.logsumexp(neg, dim=-1) + torch.logsumexp(pos, dim=-1)


def test_float64_restatement_reproduces_the_reference_multiclass_loss():
    g = np.load(os.path.join(GOLDEN, "T3_multiclass_train_512_n7.npz"))
    n = len(g["categories"])
    target = torch.zeros((n, n, 56), dtype=torch.float64)
    for i, j, r in g["gt_rels"].tolist():
        target[i, j, r] = 1
    y = target.reshape(-1, 56)[torch.as_tensor(g["sampled"])]
    loss = _mlcce64(y, torch.as_tensor(g["mc_logit"], dtype=torch.float64))
    got = float(torch.mean(loss * (loss / loss.max())) * 50.0)
    want = float(g["multiclass_rel_cls_loss"])
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert str(g["rel_cls_type"]) == "binary+multiclass" and y.sum() > 0


def test_corrected_top100_decode_of_the_reference_logits_is_well_defined():
    g = np.load(os.path.join(GOLDEN, "G7_multiclass_512_n10.npz"))
    assert "too many indices" in str(g["reference_error"])                 # V4:241 as committed
    logit = torch.as_tensor(g["mc_logit"], dtype=torch.float64)
    N, R = len(g["object_ids"]), logit.shape[1]
    assert logit.shape == (N * N, R)
    s = torch.sigmoid(logit)
    diag = torch.arange(N) * N + torch.arange(N)
    s[diag] = 0                                                             # the intent of V4:239-241
    flat = s.reshape(-1).numpy()
    order = np.lexsort((np.arange(flat.size), -flat))[:min(100, flat.size)]   # score desc, ties -> lower index
    trip = [(f // R // N, f // R % N, f % R) for f in order.tolist()]       # f = p R + r
    assert len(set(trip)) == len(trip) == 100
    assert all(0 <= a < N and 0 <= b < N and 0 <= r < R for a, b, r in trip)
    assert all(a != b for a, b, _ in trip)                                  # a zeroed diagonal never reaches the top 100
    assert float(s[diag].abs().max()) == 0.0
    assert np.all(np.diff(flat[order]) <= 0)


def test_pair_sharded_pipeline_refuses_a_multiclass_head():
    from openpsg_amd._lib import PsgHipError
    from openpsg_amd.dist import HipBackend
    with pytest.raises(PsgHipError, match="binary"):
        HipBackend(_cpu_head("binary+multiclass"))
