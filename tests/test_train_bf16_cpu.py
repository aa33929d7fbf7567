"""train_precision='bf16' without a GPU: the yardstick of the bf16 gradient path, measured on the reference side only,
and the option's validation.

The yardstick: oracle.psg_oracle.train_forward on the training goldens (their draws, dropout off), once in fp32 and once
inside torch.autocast('cpu', dtype=torch.bfloat16) with fp32 leaves.  Per trainable tensor d_ref = ||g_autocast -
g_fp32||_2 / ||g_fp32||_2 and the cosine of the two gradients, plus the relative deviation of both losses, are recorded
in tests/golden/T_bf16_autocast_baseline.json (results of the oracle only); tests/test_gpu_train_bf16.py bounds the
head's own deviation from the fp32 oracle by 2 d_ref + 2^-8.  T4 (T1's draws behind a grouped-query LLM, the oracle on
the model expanded to multi-head) is recorded for the GQA check.

CPU autocast reaches every product of the oracle: the Q-Former and Llama projections and attention products, the two
heads, language_projection, and the patch embedding's `F.conv2d` as well.  The head does NOT round there: it shares its
exact-fp32 `PatchEmbedFn` with the fp32 path, so it is more exact than the yardstick on that product.  The embedding
gathers and the `index_put` table are copies in either precision.  The comparison is made for every tensor regardless.
"""
import inspect
import json

import pytest

from tests import train_bf16_common as C


@pytest.mark.parametrize("case", C.CASES)
def test_recorded_autocast_baseline_matches_a_fresh_computation(case):
    """The file matches a fresh computation within 20 % (CPU bf16 kernels may change their summation order between torch
    builds); deviations at the fp32 noise floor (< 1e-6) are compared absolutely."""
    fresh, rec = C.compute_baseline(case), C.baseline()[case]
    print(json.dumps(fresh, indent=1))
    assert set(fresh["tensors"]) == set(rec["tensors"]) and len(fresh["tensors"]) >= 60
    for k, f in fresh["tensors"].items():
        r = rec["tensors"][k]
        assert abs(f["d_ref"] - r["d_ref"]) <= 0.2 * r["d_ref"] + 1e-6, (k, f, r)
        assert abs((1 - f["cos"]) - (1 - r["cos"])) <= 0.2 * (1 - r["cos"]) + 1e-6, (k, f, r)
    for k, f in fresh["losses"].items():
        assert abs(f - rec["losses"][k]) <= 0.2 * rec["losses"][k] + 1e-6, (k, f, rec["losses"][k])


def test_train_precision_option_validation():
    from openpsg_amd._lib import PsgHipError
    from openpsg_amd.head import RelationTransformerHeadV4
    assert inspect.signature(RelationTransformerHeadV4.__init__).parameters["train_precision"].default is None
    for bad in ("fp16", "bf16 ", "fp32", True):
        with pytest.raises(PsgHipError, match="train_precision"):
            RelationTransformerHeadV4(train_precision=bad, device="cpu", tokenizers="word")


def test_graph_precision_argument_validation():
    from openpsg_amd import train_graph as G
    from openpsg_amd._lib import PsgHipError
    with pytest.raises(PsgHipError, match="precision"):
        G.linear(None, None, None, precision="fp16")
    for fn in (G.qformer_pairs, G.llama_teacher_forcing):
        assert inspect.signature(fn).parameters["precision"].default is None
    # the five nodes both precisions share: an operand of the other precision's dtype (on the CPU: no library call can
    # have been made) raises an error naming the precision the operand has to have.  The norms read the fp32 residual
    # stream in both precisions; the pointwise nodes read activations of the precision's own dtype.
    import torch
    pos, tab = torch.zeros(2, dtype=torch.int32), torch.zeros(4, 8)
    for precision, other, own in ((None, torch.bfloat16, "fp32"), ("bf16", torch.float32, "bf16")):
        t = torch.zeros(2, 16, dtype=other)
        for node, args in ((G.GeluFn, (t,)), (G.SiluMulFn, (t,)), (G.RopeFn, (t, pos, tab, tab, 1))):
            with pytest.raises(PsgHipError, match=own):
                node.apply(*args, precision)
    g = torch.ones(16)
    for precision in (None, "bf16"):
        x = torch.zeros(2, 16, dtype=torch.bfloat16)
        for node, args in ((G.LayerNormFn, (x, g, g, 1e-12)), (G.RMSNormFn, (x, g, 1e-5))):
            with pytest.raises(PsgHipError, match="fp32"):
                node.apply(*args, precision)
    for node, args in ((G.LayerNormFn, (g, g, g, 1e-12)), (G.RMSNormFn, (g, g, 1e-5)), (G.GeluFn, (g,)), (G.SiluMulFn, (g,)),
                       (G.RopeFn, (g, pos, tab, tab, 1))):
        with pytest.raises(PsgHipError, match="precision"):
            node.apply(*args, "fp16")
