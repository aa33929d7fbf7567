"""The MXFP4-quantised LLM model on the CPU: `quantize_mxfp4_rows` - the ONE definition of (q, e, s) and of
W' = fp4(q) * 2^(e - 127) * s - against a brute-force float64 restatement, the exact FP8 image, the reader of MXFP4
checkpoint directories, and what the head's option llm_weight_quant='mxfp4' hands the decode engine."""
import json
import math
import os

import pytest
import torch

from openpsg_amd._lib import PsgHipError
from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
from openpsg_amd.weights import (LLM_QUANT_MATRICES, dequantize_fp8_rows, dequantize_mxfp4_rows, llm_quant_keys, llm_shapes,
                                 make_weights_numpy, mxfp4_as_fp8_rows, quant_format, quantize_llm_weights,
                                 quantize_mxfp4_rows, read_hf_llama_weights)

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)                            # magnitudes of codes 0..7; bit 3 = sign


def _rows():
    """Gaussian rows whose magnitudes span ten decades, + an all-zero row (5), an all-zero block (row 6, block 1), a block
    2^-23 below its row (row 7, block 2), exact ties (row 8), a block held at the floor (row 9, block 0) and a block
    maximum in (6, 8) x 2^E_b, which saturates (row 10: -7.9 becomes -6, not -8)."""
    g = torch.Generator().manual_seed(0)
    W = torch.randn(40, 160, generator=g) * torch.logspace(-5, 5, 40)[:, None]
    W[5] = 0.0
    W[6, 32:64] = 0.0
    W[7, 64:96] *= 2.0 ** -23
    W[8, :32] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0] * 4) * torch.tensor([1.0, -1.0] * 16)
    W[8, 32:] *= 0.1                                                       # block 0 sets the row's exponent: E = 0
    W[9, :32] *= 2.0 ** -20
    W[10, :32] = 0.0
    W[10, 3] = -7.9
    return W


def _unpack(q):
    return torch.stack((q & 0xF, q >> 4), dim=2).reshape(q.shape[0], -1)


def test_every_element_is_the_nearest_grid_point_in_float64():
    W = _rows()
    N, K = W.shape
    q, e, s = quantize_mxfp4_rows(W)
    assert q.dtype == torch.uint8 and q.shape == (N, K // 2) and e.dtype == torch.uint8 and e.shape == (N, K // 32)
    assert s.dtype == torch.float32 and s.shape == (N,)
    assert int(e.min()) >= 114 and int(e.max()) <= 127
    code = _unpack(q)
    assert not (code == 8).any(), "code 0x8 (-0) appeared"
    # the exponents, restated with math.frexp
    for n in range(N):
        Eb = []
        for b in range(K // 32):
            a = float(W[n, 32 * b:32 * b + 32].abs().max())
            Eb.append(None if a == 0 else math.frexp(a)[1] - 1 - 2)
        Emax = max([x for x in Eb if x is not None], default=0)
        assert float(s[n]) == 2.0 ** Emax
        for b in range(K // 32):
            want = Emax - 13 if Eb[b] is None else max(Eb[b], Emax - 13)
            assert int(e[n, b]) == 127 + want - Emax, (n, b)
    # the elements: brute force over the block's 15-value grid in float64
    Wp = dequantize_mxfp4_rows(q, e, s).double()
    scale = (torch.exp2(e.double() - 127) * s.double()[:, None]).repeat_interleave(32, dim=1)
    grid = torch.tensor(GRID, dtype=torch.float64)
    a = W.double().abs() / scale                                           # exact: a power-of-two scale
    dist = (a[:, :, None] - grid[None, None, :]).abs()
    best = dist.min(dim=2).values
    mag = code & 7
    assert torch.equal(Wp.abs(), grid[mag.long()] * scale)                 # the model's value IS grid x scale
    assert torch.equal((a - grid[mag.long()]).abs(), best), "an element is not a nearest grid point"
    tie = (dist == best[:, :, None]).sum(2) > 1
    assert tie.any() and (mag[tie] % 2 == 0).all(), "a tie did not go to the even code"
    assert ((a > 6) & (mag == 7)).any(), "no value saturated"
    assert (((W < 0) & (mag > 0)) == (code >= 8)).all()                    # sign, and no sign on a zero
    assert (q[5] == 0).all() and float(s[5]) == 1.0 and (e[5] == 114).all()
    assert (q[6, 16:32] == 0).all() and int(e[6, 1]) == 114
    assert int(e[7, 2]) == 114 and int(e[9, 0]) == 114
    assert float(Wp[10, 3]) == -6.0 * 2.0 ** (int(e[10, 0]) - 127) * float(s[10])


def test_requantising_the_model_changes_nothing():
    q, e, s = quantize_mxfp4_rows(_rows())
    q2, e2, s2 = quantize_mxfp4_rows(dequantize_mxfp4_rows(q, e, s))
    assert torch.equal(q2, q) and torch.equal(e2, e) and torch.equal(s2, s)


def test_the_model_over_s_is_a_normal_fp16_number_or_zero():
    q, e, s = quantize_mxfp4_rows(_rows())
    r = dequantize_mxfp4_rows(q, e, s) / s[:, None]                       # exact: s is a power of two
    h = r.to(torch.float16)
    assert torch.equal(h.to(torch.float32), r)
    assert ((h == 0) | (h.abs() >= 2.0 ** -14)).all()
    assert (h.abs() == 2.0 ** -14).any(), "the smallest value 0.5 x 2^-13 was not drawn"


def test_the_fp8_image_is_the_model_bit_for_bit():
    q, e, s = quantize_mxfp4_rows(_rows())
    q8, s8 = mxfp4_as_fp8_rows(q, e, s)
    assert q8.dtype == torch.uint8 and q8.shape == (q.shape[0], 2 * q.shape[1]) and s8.dtype == torch.float32
    assert torch.equal(dequantize_fp8_rows(q8, s8), dequantize_mxfp4_rows(q, e, s))
    s3 = s * 0.977                                                         # ... and for scales that are no powers of two
    q8, s8 = mxfp4_as_fp8_rows(q, e, s3)
    assert torch.equal(dequantize_fp8_rows(q8, s8), dequantize_mxfp4_rows(q, e, s3))


def test_the_low_nibble_is_the_even_k():
    W = torch.zeros(1, 32)
    W[0, 0], W[0, 1], W[0, 2], W[0, 3] = 6.0, -0.5, 0.0, 1.5
    q, e, s = quantize_mxfp4_rows(W)
    assert int(q[0, 0]) == 0x97 and int(q[0, 1]) == 0x30 and int(e[0, 0]) == 127 and float(s[0]) == 1.0
    Wd = dequantize_mxfp4_rows(torch.tensor([[0x97, 0x30] + [0] * 14], dtype=torch.uint8), e, s)
    assert Wd[0, :4].tolist() == [6.0, -0.5, 0.0, 1.5]


def test_row_scales_and_block_exponents_commute_with_the_engines_concatenations():
    g = torch.Generator().manual_seed(2)
    parts = [torch.randn(n, 128, generator=g) * sc for n, sc in ((32, 1.0), (16, 0.01), (16, 30.0))]
    whole = quantize_mxfp4_rows(torch.cat(parts, 0))
    each = [quantize_mxfp4_rows(p) for p in parts]
    for i in range(3):
        assert torch.equal(whole[i], torch.cat([t[i] for t in each], 0))
    with pytest.raises(ValueError, match="K % 32"):
        quantize_mxfp4_rows(torch.zeros(4, 48))


# ---- the reader ---------------------------------------------------------------------------------------------------------
def _tiny():
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 2, 512, 512), max_object_num=30)
    return cfg, make_weights_numpy(cfg, seed=5)


def write_mxfp4_checkpoint(path, cfg, w, edit=None):
    """An MXFP4 checkpoint directory in the layout INTEGRATION documents: `weight` uint8 [N, K / 2] (low nibble = even k) +
    `weight_scale` uint8 [N, K / 32] (E8M0: block scale 2^(byte - 127), ABSOLUTE, not row-anchored) for the decoder layers'
    matrices, the lm_head / embedding / norms in fp16.  `edit(sd)` may damage the tensors before they are written.
    Returns {stored name: tensor} as written."""
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
    for k, v in w.items():
        if not k.startswith("language_model."):
            continue
        name = k[len("language_model."):]
        if k not in quant:
            sd[name] = v.half().contiguous()
        else:
            v = v.clone()
            if "layers.0.mlp.up_proj" in k:
                v[3, 32:64] = 0.0                                          # an all-zero block, stored with a stray exponent
                v[4] = 0.0                                                 # an all-zero row
            q, e, s = quantize_mxfp4_rows(v)
            Emax = torch.log2(s).to(torch.int32)
            absolute = e.to(torch.int32) + Emax[:, None]                   # 127 + E_b
            if "layers.0.mlp.up_proj" in k:
                absolute[3, 1] = 3
                absolute[4] = 200
            sd[name] = q
            sd[name + "_scale"] = absolute.to(torch.uint8)
    if edit is not None:
        edit(sd)
    save_file(sd, os.path.join(path, "model.safetensors"))
    return sd


def _direct(q, sc):
    """Dequantisation of the stored pair as OCP defines it: fp4(q) * 2^(scale byte - 127), float64."""
    code = _unpack(q).long()
    grid = torch.tensor(GRID + tuple(-g for g in GRID), dtype=torch.float64)
    return grid[code] * torch.exp2(sc.double() - 127).repeat_interleave(32, dim=1)


def test_reader_row_anchors_an_mxfp4_checkpoint(tmp_path):
    cfg, w = _tiny()
    d = str(tmp_path / "mxfp4")
    sd = write_mxfp4_checkpoint(d, cfg, w)
    got = read_hf_llama_weights(d)
    quant = set(llm_quant_keys(cfg.llm.layers))
    assert set(got) == set(llm_shapes(cfg)) | {k + "_scale" for k in quant} | {k + "_bexp" for k in quant}
    for k in llm_shapes(cfg):
        name = k[len("language_model."):]
        if k in quant:
            assert quant_format(got, k) == "mxfp4"
            q, e, s = got[k], got[k + "_bexp"], got[k + "_scale"]
            N, K = llm_shapes(cfg)[k]
            assert q.dtype == torch.uint8 and q.shape == (N, K // 2) and torch.equal(q, sd[name])
            assert e.dtype == torch.uint8 and e.shape == (N, K // 32) and int(e.min()) >= 114 and int(e.max()) <= 127
            assert s.dtype == torch.float32 and s.shape == (N,)
            assert torch.equal(dequantize_mxfp4_rows(q, e, s).double(), _direct(sd[name], sd[name + "_scale"]))
        else:
            assert got[k].dtype == torch.float16 and torch.equal(got[k], sd[name])
    k = "language_model.model.layers.0.mlp.up_proj.weight"
    assert int(got[k + "_bexp"][3, 1]) == 114 and float(got[k + "_scale"][4]) == 1.0 and (got[k + "_bexp"][4] == 114).all()
    # ... and the head's option leaves such triples alone (never re-quantised)
    again = quantize_llm_weights(got, cfg.llm.layers, fmt="mxfp4")
    assert all(again[k] is got[k] for k in got)


def test_reader_refusals_name_the_tensor(tmp_path):
    cfg, w = _tiny()
    name = "model.layers.1.self_attn.o_proj.weight"

    def far(sd):                                                           # a non-zero block 14 below its row's largest
        sc = sd[name + "_scale"]
        sd[name][2, 16:32] = 0x22
        sc[2, 1] = sc[2].max() - 14

    def minus_zero(sd):
        sd[name][0, 5] = 0x38

    def ragged(sd):                                                        # K = 272: not a multiple of 32
        sd[name] = torch.cat([sd[name], torch.zeros(sd[name].shape[0], 8, dtype=torch.uint8)], 1)

    for i, (edit, what) in enumerate(((far, "below its"), (minus_zero, "0x8"), (ragged, "K % 32"))):
        d = str(tmp_path / f"bad{i}")
        write_mxfp4_checkpoint(d, cfg, w, edit=edit)
        with pytest.raises(PsgHipError, match=what) as ei:
            read_hf_llama_weights(d)
        assert "o_proj" in str(ei.value) and "layers.1" in str(ei.value)


# ---- the head's option --------------------------------------------------------------------------------------------------
def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    cfg, _ = _tiny()
    return RelationTransformerHeadV4(dtype="fp32s", device="cpu", qformer_vocab_size=512, tokenizers="word", max_object_num=30,
                                     llm_config=cfg.llm, llm_feature_size=256, **kw)


def test_head_option_quantises_exactly_the_projection_matrices():
    cfg, w = _tiny()
    llm = {k: v for k, v in w.items() if k.startswith("language_model.")}
    for lm_head in (False, True):
        out = _head(llm_weight_quant="mxfp4", llm_quantize_lm_head=lm_head).quantize_llm_weights(llm)
        quant = set(llm_quant_keys(cfg.llm.layers, lm_head))
        assert len(quant) == len(LLM_QUANT_MATRICES) * cfg.llm.layers + int(lm_head)
        assert set(out) == set(llm) | {k + "_scale" for k in quant} | {k + "_bexp" for k in quant}
        for k in llm:
            if k in quant:
                q, e, s = quantize_mxfp4_rows(llm[k])
                assert torch.equal(out[k], q) and torch.equal(out[k + "_bexp"], e) and torch.equal(out[k + "_scale"], s)
            else:
                assert out[k] is llm[k]                                     # embedding, norms (+ lm_head): untouched


def test_head_option_validation():
    assert _head(llm_weight_quant="mxfp4").llm_weight_quant == "mxfp4"
    with pytest.raises(PsgHipError, match="llm_weight_quant"):
        _head(llm_weight_quant="int4")
    with pytest.raises(PsgHipError, match="llm_weight_quant"):
        _head(llm_weight_quant="nvfp4")
    with pytest.raises(PsgHipError, match="no LLM stage"):
        _head(llm_weight_quant="mxfp4", rel_cls_type="multiclass")
    with pytest.raises(ValueError, match="fmt"):
        quantize_llm_weights({}, 1, fmt="int4")
