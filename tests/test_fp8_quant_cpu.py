"""The FP8-quantised LLM model on the CPU: `quantize_fp8_rows` - the ONE definition of (q, s) and of
W' = float32(q) * s - the reader of FP8 checkpoint directories, and what the head's option llm_weight_quant='fp8' hands
the decode engine."""
import json
import os

import pytest
import torch

from openpsg_amd._lib import PsgHipError
from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
from openpsg_amd.weights import (LLM_QUANT_MATRICES, dequantize_fp8_rows, llm_quant_keys, llm_shapes, make_weights_numpy,
                                 quantize_fp8_rows, quantize_llm_weights, read_hf_llama_weights)

F8 = torch.float8_e4m3fn


def _f8(q):
    return q.view(F8).to(torch.float32)


def _half_ulp(qv):
    """Half the spacing of the e4m3fn grid around a grid value qv (3 mantissa bits, smallest normal 2^-6, subnormal
    spacing 2^-9): a value between two grid points is at most this far from the nearer one.  For |qv| in [2^e, 2^(e+1))
    the spacing is 2^(e-3), so half of it is 2^(e-4) <= |qv| 2^-4; below 2^-6 it is 2^-10 = 2^-6 2^-4.  Rounding to
    nearest therefore gives |W/s - q| <= 2^-4 max(|q|, 2^-6) (the bound is taken at q, the RESULT: a value rounded up
    to a power of two sits in the finer binade below it, where the bound at q is the coarser, still valid, one)."""
    return 2.0 ** -4 * qv.abs().clamp_min(2.0 ** -6)


def test_round_trip_is_within_half_an_ulp_of_the_e4m3_grid():
    g = torch.Generator().manual_seed(0)
    W = torch.randn(96, 320, generator=g) * torch.logspace(-6, 3, 96)[:, None]
    W[:, 7] *= 1e-3                                                        # values that land on e4m3 subnormals
    W[5] = 0.0                                                             # a zero row
    W[9, 11] = -3.0 * W[9].abs().max()                                     # a row whose maximum is negative
    q, s = quantize_fp8_rows(W)
    assert q.dtype == torch.uint8 and q.shape == W.shape and s.dtype == torch.float32 and s.shape == (96,)
    qv = _f8(q)
    assert torch.isfinite(qv).all() and qv.abs().max() == 448
    assert torch.equal(s[5], torch.tensor(1.0)) and (q[5] == 0).all()
    rows = [i for i in range(96) if i != 5]
    assert torch.equal(s[rows], W[rows].abs().amax(1) / 448)
    assert qv[9, 11] == -448 and qv[9].abs().max() == 448
    assert ((qv.abs() > 0) & (qv.abs() < 2.0 ** -6)).any(), "no subnormal was drawn"
    Wd = dequantize_fp8_rows(q, s)
    assert torch.equal(Wd, qv * s[:, None])                                # the model: one fp32 rounding per element
    # |W' - W| <= s 2^-4 max(|q|, 2^-6), evaluated in float64 (+ the fp32 roundings of W / s and of q s: 2^-23 |W|)
    err = (Wd.double() - W.double()).abs()
    bound = s.double()[:, None] * _half_ulp(qv).double() + 2.0 ** -22 * W.double().abs()
    assert (err <= bound).all(), (err / bound).max()


def test_requantising_the_model_changes_nothing():
    g = torch.Generator().manual_seed(1)
    W = torch.randn(64, 256, generator=g) * torch.logspace(-4, 2, 64)[:, None]
    q, s = quantize_fp8_rows(W)
    q2, s2 = quantize_fp8_rows(dequantize_fp8_rows(q, s))
    assert torch.equal(q2, q) and torch.equal(s2, s)


def test_row_scales_commute_with_the_engines_concatenations():
    g = torch.Generator().manual_seed(2)
    parts = [torch.randn(n, 128, generator=g) * sc for n, sc in ((32, 1.0), (16, 0.01), (16, 30.0))]
    q, s = quantize_fp8_rows(torch.cat(parts, 0))
    qs = [quantize_fp8_rows(p) for p in parts]
    assert torch.equal(q, torch.cat([a for a, _ in qs], 0)) and torch.equal(s, torch.cat([b for _, b in qs], 0))


# ---- the reader ---------------------------------------------------------------------------------------------------------
def _tiny():
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 2, 512, 512), max_object_num=30)
    return cfg, make_weights_numpy(cfg, seed=5)


def write_fp8_checkpoint(path, cfg, w, scale_shapes=None):
    """An FP8 checkpoint directory as the common exporters leave it: `weight` (float8_e4m3fn) + `weight_scale` for the
    decoder layers' matrices - per channel [N, 1] or [N], ONE tensor per-tensor scaled (a scalar) - an ignored
    `input_scale`, the lm_head / embedding / norms in fp16.  Returns {stored name: tensor} as written."""
    from safetensors.torch import save_file
    m = cfg.llm
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(architectures=["LlamaForCausalLM"], hidden_size=m.hidden, num_attention_heads=m.heads,
                       num_key_value_heads=m.n_kv_heads, num_hidden_layers=m.layers, intermediate_size=m.inter,
                       vocab_size=m.vocab, rms_norm_eps=m.rms_eps, rope_theta=m.rope_theta, bos_token_id=m.bos,
                       eos_token_id=m.eos, torch_dtype="float16", tie_word_embeddings=False), f)
    sd = {}
    quant = set(llm_quant_keys(m.layers))
    per_tensor = "language_model.model.layers.1.mlp.down_proj.weight"
    for k, v in w.items():
        if not k.startswith("language_model."):
            continue
        name = k[len("language_model."):]
        if k not in quant:
            sd[name] = v.half().contiguous()
        elif k == per_tensor:                                              # one scale for the whole matrix
            sc = v.abs().max() / 448
            sd[name] = (v / sc).clamp(-448, 448).to(F8)
            sd[name + "_scale"] = sc.reshape(())
        else:
            q, s = quantize_fp8_rows(v)
            sd[name] = q.view(F8)
            sd[name + "_scale"] = s.reshape((scale_shapes or {}).get(k, (-1, 1) if "q_proj" in k else (-1,))).contiguous()
    sd["model.layers.0.self_attn.q_proj.input_scale"] = torch.tensor(0.5)
    save_file(sd, os.path.join(path, "model.safetensors"))
    return sd


def test_reader_takes_an_fp8_checkpoint_as_it_is(tmp_path):
    cfg, w = _tiny()
    d = str(tmp_path / "fp8")
    sd = write_fp8_checkpoint(d, cfg, w)
    got = read_hf_llama_weights(d)
    quant = set(llm_quant_keys(cfg.llm.layers))
    assert set(got) == set(llm_shapes(cfg)) | {k + "_scale" for k in quant}          # no input_scale
    for k in llm_shapes(cfg):
        name = k[len("language_model."):]
        if k in quant:
            assert got[k].dtype == F8 and torch.equal(got[k].view(torch.uint8), sd[name].view(torch.uint8))
            s = got[k + "_scale"]
            assert s.dtype == torch.float32 and s.shape == (got[k].shape[0],)
            assert torch.equal(s, sd[name + "_scale"].reshape(-1).expand(got[k].shape[0]))
        else:
            assert got[k].dtype == torch.float16 and torch.equal(got[k], sd[name])
    # ... and the head's option leaves such pairs alone (never re-quantised)
    again = quantize_llm_weights(got, cfg.llm.layers)
    assert all(again[k] is got[k] for k in got)


def test_reader_refuses_block_scaled_and_unscaled_fp8(tmp_path):
    cfg, w = _tiny()
    k = "language_model.model.layers.0.mlp.up_proj.weight"
    d = str(tmp_path / "block")
    write_fp8_checkpoint(d, cfg, w, scale_shapes={k: (4, -1)})              # [N / 128, K / 128]-style block scales
    with pytest.raises(PsgHipError, match="block-scaled"):
        read_hf_llama_weights(d)
    from safetensors.torch import load_file, save_file
    d2 = str(tmp_path / "bare")
    write_fp8_checkpoint(d2, cfg, w)
    sd = load_file(os.path.join(d2, "model.safetensors"))
    del sd[k[len("language_model."):] + "_scale"]
    save_file(sd, os.path.join(d2, "model.safetensors"))
    with pytest.raises(PsgHipError, match="without a weight_scale"):
        read_hf_llama_weights(d2)


# ---- the head's option --------------------------------------------------------------------------------------------------
def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    cfg, _ = _tiny()
    return RelationTransformerHeadV4(dtype="fp32s", device="cpu", qformer_vocab_size=512, tokenizers="word", max_object_num=30,
                                     llm_config=cfg.llm, llm_feature_size=256, **kw)


def test_head_option_quantises_exactly_the_projection_matrices():
    cfg, w = _tiny()
    llm = {k: v for k, v in w.items() if k.startswith("language_model.")}
    assert _head().quantize_llm_weights(llm).keys() == llm.keys()          # default: nothing new
    for lm_head in (False, True):
        out = _head(llm_weight_quant="fp8", llm_quantize_lm_head=lm_head).quantize_llm_weights(llm)
        quant = set(llm_quant_keys(cfg.llm.layers, lm_head))
        assert len(quant) == len(LLM_QUANT_MATRICES) * cfg.llm.layers + int(lm_head)
        assert set(out) == set(llm) | {k + "_scale" for k in quant}
        for k in llm:
            if k in quant:
                q, s = quantize_fp8_rows(llm[k])
                assert out[k].dtype == torch.uint8 and torch.equal(out[k], q) and torch.equal(out[k + "_scale"], s)
            else:
                assert out[k] is llm[k]                                     # embedding, norms (+ lm_head): untouched


def test_head_option_refusals():
    with pytest.raises(PsgHipError, match="llm_weight_quant"):
        _head(llm_weight_quant="int4")
    with pytest.raises(PsgHipError, match="no LLM stage"):
        _head(llm_weight_quant="fp8", rel_cls_type="multiclass")
    with pytest.raises(PsgHipError, match="llm_quantize_lm_head"):
        _head(llm_quantize_lm_head=True)
