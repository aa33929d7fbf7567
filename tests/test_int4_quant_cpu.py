"""The group-wise INT4 LLM model on the CPU: `quantize_int4_groups` / `dequantize_int4_groups` - the ONE definition
of (q, gs, gz) and of W' = float(gs) * (q - gz) - against a brute-force float64 restatement; the reader of GPTQ (v1, v2) and
AWQ checkpoint directories against directories packed HERE from the layouts' formulas (INTEGRATION), independently of the
reader; and the head's option llm_weight_quant='int4g'."""
import json
import os

import numpy as np
import pytest
import torch

from openpsg_amd._lib import PsgHipError
from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
from openpsg_amd.weights import (LLM_QUANT_MATRICES, dequantize_int4_groups, is_quantized, llm_quant_keys, llm_shapes,
                                 make_weights_numpy, quant_format, quantize_int4_groups, quantize_llm_weights,
                                 read_hf_llama_weights)

AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


def _unpack(q):
    return torch.stack((q & 0xF, q >> 4), dim=2).reshape(q.shape[0], -1)


def _planted():
    """24 x 512 Gaussian rows + an all-zero group (row 1, k 0..127), an all-positive one (row 2), an all-negative one (row 3),
    one outlier of 1e3 (row 4) and values of 1e-7 (row 5, whole row: scales at the 2^-14 floor)."""
    g = torch.Generator().manual_seed(0)
    W = torch.randn(24, 512, generator=g) * 0.05
    W[1, :128] = 0.0
    W[2, :128] = W[2, :128].abs() + 0.01
    W[3, :128] = -W[3, :128].abs() - 0.01
    W[4, 200] = 1e3
    W[5] = torch.randn(512, generator=g) * 1e-7
    return W


@pytest.mark.parametrize("G", [32, 64, 128])
def test_every_code_is_the_nearest_of_the_sixteen_in_float64(G):
    W = _planted()
    N, K = W.shape
    q, gs, gz = quantize_int4_groups(W, G)
    assert q.dtype == torch.uint8 and q.shape == (N, K // 2)
    assert gs.dtype == torch.float16 and gs.shape == (N, K // G) and gz.dtype == torch.uint8 and gz.shape == (N, K // G)
    assert int(gz.max()) <= 15
    s64 = gs.double()
    assert torch.isfinite(s64).all() and (s64 >= 2.0 ** -14).all(), "a scale is zero, subnormal or not finite"
    code = _unpack(q).long()
    assert int(code.max()) <= 15
    s_k, z_k = s64.repeat_interleave(G, dim=1), gz.long().repeat_interleave(G, dim=1)
    # the scale and zero point, restated per (row, group)
    Wg = W.double().reshape(N, K // G, G)
    lo, hi = Wg.amin(2).clamp_max(0), Wg.amax(2).clamp_min(0)
    want_s = ((hi - lo) / 15).clamp(2.0 ** -14, 65504.0)
    assert ((s64 - want_s).abs() <= want_s * 2.0 ** -11).all()                 # nearest fp16: half an ulp at most
    assert torch.equal(gz.double(), torch.round(-lo / s64).clamp(0, 15))
    # brute force: the nearest of the 16 codes given the stored (gs, gz); a tie goes to the even q - z (rint(w / s))
    cand = torch.arange(16, dtype=torch.float64)
    val = s_k[:, :, None] * (cand[None, None, :] - z_k[:, :, None].double())   # exact: 11 x 5 bits
    err = (W.double()[:, :, None] - val).abs()
    best = err.amin(dim=2, keepdim=True)
    tie = err == best
    odd = ((cand[None, None, :].long() - z_k[:, :, None]) % 2) != 0
    rank = torch.where(tie & ~odd, 0, torch.where(tie, 1, 2))
    assert torch.equal(code, rank.argmin(dim=2))
    # the model: one definition, float64 rounded once to fp32
    Wq = dequantize_int4_groups(q, gs, gz)
    assert Wq.dtype == torch.float32
    assert torch.equal(Wq, (s_k * (code - z_k).double()).to(torch.float32))
    inner = (code > 0) & (code < 15)
    assert ((W.double() - Wq.double()).abs()[inner] <= (s_k / 2)[inner] * (1 + 1e-12)).all()
    assert (Wq[1, :128] == 0).all() and float(gs[1, 0]) == 2.0 ** -14 and int(gz[1, 0]) == 0 and (code[1, :128] == 0).all()
    assert int(gz[2, 0]) == 0 and int(gz[3, 0]) == 15


def test_groups_commute_with_row_concatenation_and_bad_shapes_raise():
    g = torch.Generator().manual_seed(3)
    parts = [torch.randn(n, 256, generator=g) for n in (8, 4, 4)]
    whole = quantize_int4_groups(torch.cat(parts, 0))
    each = [quantize_int4_groups(p) for p in parts]
    for i in range(3):
        assert torch.equal(whole[i], torch.cat([t[i] for t in each], 0))
    with pytest.raises(ValueError, match="group"):
        quantize_int4_groups(torch.zeros(4, 192), 128)
    with pytest.raises(ValueError, match="group"):
        quantize_int4_groups(torch.zeros(4, 256), 16)


# ---- checkpoint directories, packed from the layouts' formulas -------------------------------------------------------------
def _tiny():
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 2, 512, 512), max_object_num=30)
    return cfg, make_weights_numpy(cfg, seed=5)


def int4_model(cfg, group=128, seed=11):
    """{matrix name: (q, gs, gz)} for the decoder layers' matrices: codes uniform over 0..15, scales 0.002 .. 0.03 that are
    no powers of two, zero points that take all 16 values in every matrix (0 and 15 first)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in llm_quant_keys(cfg.llm.layers):
        N, K = llm_shapes(cfg)[k]
        q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
        gs = (torch.exp2(torch.rand(N, K // group, generator=g) * 4 - 9) * 0.977).to(torch.float16)
        gz = torch.randint(0, 16, (N, K // group), generator=g, dtype=torch.int32).to(torch.uint8)
        gz.view(-1)[:16] = torch.tensor([0, 15] + list(range(1, 15)), dtype=torch.uint8)
        out[k] = (q, gs, gz)
    return out


def _words(nib, axis):
    """uint8 nibbles -> int32 words along `axis`: nibble i of word m = nib[8 m + i], bits 4 i .. 4 i + 3."""
    nib = np.moveaxis(np.asarray(nib, dtype=np.uint32), axis, 0)
    w = np.zeros((nib.shape[0] // 8,) + nib.shape[1:], dtype=np.uint32)
    for i in range(8):
        w |= nib[i::8] << np.uint32(4 * i)
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(w, 0, axis)).view(np.int32))


def pack_layer(q, gs, gz, method, v2=False):
    """(q, gs, gz) of a layer with K inputs, N outputs -> its (qweight, qzeros, scales) as the layout `method` stores it."""
    code = _unpack(q).numpy().T                                                # [K, N]
    z = gz.numpy().T.astype(np.int64)                                          # [K / G, N]
    scales = gs.t().contiguous()                                               # fp16 [K / G, N]
    if method == "gptq":
        stored = z if v2 else (z - 1) & 15                                     # the v1 exporter subtracts one: z = 0 is stored as 15
        return _words(code, 0), _words(stored, 1), scales
    # AWQ gemm: nibble i of word m holds column 8 m + AWQ_ORDER[i]
    perm = np.array([8 * m + AWQ_ORDER[i] for m in range(code.shape[1] // 8) for i in range(8)])
    return _words(code[:, perm], 1), _words(z[:, perm], 1), scales


def write_int4_checkpoint(path, cfg, w, model, method, v2=False, group=128, qc=None, edit=None, legacy=False):
    """A GPTQ / AWQ checkpoint directory: the decoder layers' matrices packed by `pack_layer`, the lm_head / embedding / norms
    in fp16.  `qc` overrides entries of the quantisation settings, `edit(sd)` may damage the tensors; `legacy`: the settings
    go into a sibling quantize_config.json without quant_method, as old AutoGPTQ exports have them."""
    from safetensors.torch import save_file
    m = cfg.llm
    os.makedirs(path, exist_ok=True)
    if method == "gptq":
        settings = dict(quant_method="gptq", bits=4, group_size=group, desc_act=False, sym=False)
        if v2:
            settings["checkpoint_format"] = "gptq_v2"
    else:
        settings = dict(quant_method="awq", bits=4, group_size=group, zero_point=True, version="GEMM")
    settings.update(qc or {})
    conf = dict(architectures=["LlamaForCausalLM"], hidden_size=m.hidden, num_attention_heads=m.heads,
                num_key_value_heads=m.n_kv_heads, num_hidden_layers=m.layers, intermediate_size=m.inter, vocab_size=m.vocab,
                rms_norm_eps=m.rms_eps, rope_theta=m.rope_theta, bos_token_id=m.bos, eos_token_id=m.eos,
                torch_dtype="float16", tie_word_embeddings=False)
    if legacy:
        settings.pop("quant_method")
        with open(os.path.join(path, "quantize_config.json"), "w") as f:
            json.dump(settings, f)
    else:
        conf["quantization_config"] = settings
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(conf, f)
    sd = {}
    for k, v in w.items():
        if not k.startswith("language_model."):
            continue
        name = k[len("language_model."):]
        if k not in model:
            sd[name] = v.half().contiguous()
            continue
        X = name[:-len(".weight")]
        sd[X + ".qweight"], sd[X + ".qzeros"], sd[X + ".scales"] = pack_layer(*model[k], method, v2)
    if edit is not None:
        edit(sd)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    return sd


def test_gptq_v1_v2_and_awq_directories_load_to_the_same_model(tmp_path):
    cfg, w = _tiny()
    model = int4_model(cfg)
    K_o = llm_shapes(cfg)["language_model.model.layers.1.self_attn.o_proj.weight"][1]

    def old_export(sd):                                                        # what old exports carry: both are dropped
        sd["model.layers.1.self_attn.o_proj.g_idx"] = (torch.arange(K_o) // 128).to(torch.int32)
        sd["model.layers.1.self_attn.o_proj.bias"] = torch.zeros(cfg.llm.hidden, dtype=torch.float16)
    # GPTQ v1 wraps: a zero point of 0 is stored as 15
    qz = pack_layer(*model["language_model.model.layers.0.self_attn.q_proj.weight"], "gptq")[1]
    assert int(qz[0, 0]) & 15 == 15 and (int(qz[0, 0]) >> 4) & 15 == 0         # z = 0 (row 0) and z = 1 (row 1) of group 0
    got = {}
    for tag, kw in (("v1", dict(method="gptq", edit=old_export, legacy=True)), ("v2", dict(method="gptq", v2=True)),
                    ("awq", dict(method="awq"))):
        d = str(tmp_path / tag)
        write_int4_checkpoint(d, cfg, w, model, **kw)
        got[tag] = read_hf_llama_weights(d)
    quant = set(model)
    for tag, r in got.items():
        assert set(r) == set(llm_shapes(cfg)) | {k + "_gscale" for k in quant} | {k + "_gzero" for k in quant}, tag
        for k in llm_shapes(cfg):
            if k in quant:
                q, gs, gz = model[k]
                assert quant_format(r, k) == "int4" and is_quantized(r, k)
                assert r[k].dtype == torch.uint8 and torch.equal(r[k], q), (tag, k)
                assert r[k + "_gscale"].dtype == torch.float16 and torch.equal(r[k + "_gscale"], gs), (tag, k)
                assert r[k + "_gzero"].dtype == torch.uint8 and torch.equal(r[k + "_gzero"], gz), (tag, k)
            else:
                assert r[k].dtype == torch.float16 and quant_format(r, k) is None                # lm_head, embedding, norms
    # ... and the head's option leaves such triples alone (never re-quantised)
    again = quantize_llm_weights(got["awq"], cfg.llm.layers, fmt="int4g")
    assert all(again[k] is got["awq"][k] for k in got["awq"])


def test_reader_refusals_name_the_tensor(tmp_path):
    cfg, w = _tiny()
    model = int4_model(cfg)
    X = "model.layers.1.self_attn.o_proj"

    def scale(v):
        def edit(sd):
            sd[X + ".scales"][1, 7] = v
        return edit

    def act_order(sd):
        gi = torch.arange(256, dtype=torch.int32) // 128
        gi[3], gi[200] = 1, 0
        sd[X + ".g_idx"] = gi

    def ragged(sd):                                                            # K = 264: no multiple of the group
        sd[X + ".qweight"] = torch.cat([sd[X + ".qweight"], torch.zeros(1, 256, dtype=torch.int32)], 0)

    def bias(sd):
        sd[X + ".bias"] = torch.full((256,), 0.5, dtype=torch.float16)

    def fp8_layer(sd):
        Y = "model.layers.0.mlp.up_proj"
        for s in (".qweight", ".qzeros", ".scales"):
            del sd[Y + s]
        sd[Y + ".weight"] = torch.zeros(512, 256).to(torch.float8_e4m3fn)
        sd[Y + ".weight_scale"] = torch.ones(512)

    def mxfp4_layer(sd):
        Y = "model.layers.0.mlp.up_proj"
        for s in (".qweight", ".qzeros", ".scales"):
            del sd[Y + s]
        sd[Y + ".weight"] = torch.zeros(512, 128, dtype=torch.uint8)
        sd[Y + ".weight_scale"] = torch.full((512, 8), 127, dtype=torch.uint8)

    cases = (
        ("gptq", dict(qc=dict(bits=8)), "bits", None),
        ("gptq", dict(qc=dict(bits=3)), "bits", None),
        ("gptq", dict(qc=dict(group_size=-1)), "group_size", None),
        ("gptq", dict(qc=dict(group_size=256)), "group_size", None),
        ("gptq", dict(edit=ragged), "multiple of group_size", X),
        ("gptq", dict(qc=dict(desc_act=True)), "desc_act", None),
        ("gptq", dict(edit=act_order), "g_idx", X),
        ("awq", dict(qc=dict(version="gemv")), "version", None),
        ("awq", dict(qc=dict(quant_method="gptq")), "contradict", None),       # AWQ tensors declared as GPTQ
        ("gptq", dict(qc=dict(quant_method="awq")), "contradict", None),       # ... and the reverse
        ("gptq", dict(edit=scale(0.0)), "zero, subnormal or non-finite", X),
        ("awq", dict(edit=scale(2.0 ** -20)), "zero, subnormal or non-finite", X),
        ("awq", dict(edit=scale(float("inf"))), "zero, subnormal or non-finite", X),
        ("gptq", dict(edit=bias), "bias", X),
        ("gptq", dict(edit=fp8_layer), "mixes", None),
        ("awq", dict(edit=mxfp4_layer), "mixes", None),
    )
    for i, (method, kw, what, name) in enumerate(cases):
        d = str(tmp_path / f"bad{i}")
        write_int4_checkpoint(d, cfg, w, model, method, **kw)
        with pytest.raises(PsgHipError, match=what) as ei:
            read_hf_llama_weights(d)
        msg = str(ei.value)
        assert "model.layers." in msg and "_proj" in msg, msg                  # a tensor is named
        if name is not None:
            assert name in msg, msg
    # packed layers without any quantisation settings
    d = str(tmp_path / "nosettings")
    write_int4_checkpoint(d, cfg, w, model, "gptq")
    with open(os.path.join(d, "config.json")) as f:
        conf = json.load(f)
    del conf["quantization_config"]
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(conf, f)
    with pytest.raises(PsgHipError, match="quantization_config"):
        read_hf_llama_weights(d)


# ---- the head's option ----------------------------------------------------------------------------------------------------
def _head(**kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    cfg, _ = _tiny()
    return RelationTransformerHeadV4(dtype="fp32s", device="cpu", qformer_vocab_size=512, tokenizers="word", max_object_num=30,
                                     llm_config=cfg.llm, llm_feature_size=256, **kw)


def test_head_option_quantises_exactly_the_projection_matrices():
    cfg, w = _tiny()
    llm = {k: v for k, v in w.items() if k.startswith("language_model.")}
    for lm_head in (False, True):
        out = _head(llm_weight_quant="int4g", llm_quantize_lm_head=lm_head).quantize_llm_weights(llm)
        quant = set(llm_quant_keys(cfg.llm.layers, lm_head))
        assert len(quant) == len(LLM_QUANT_MATRICES) * cfg.llm.layers + int(lm_head)
        assert set(out) == set(llm) | {k + "_gscale" for k in quant} | {k + "_gzero" for k in quant}
        for k in llm:
            if k in quant:
                q, gs, gz = quantize_int4_groups(llm[k], 128)
                assert quant_format(out, k) == "int4"
                assert torch.equal(out[k], q) and torch.equal(out[k + "_gscale"], gs) and torch.equal(out[k + "_gzero"], gz)
            else:
                assert out[k] is llm[k] and quant_format(out, k) is None        # embedding, norms (+ lm_head): untouched


def test_head_option_validation():
    assert _head(llm_weight_quant="int4g").llm_weight_quant == "int4g"
    with pytest.raises(PsgHipError, match="llm_weight_quant"):
        _head(llm_weight_quant="int3")
    with pytest.raises(PsgHipError, match="llm_weight_quant.*'int4g'"):      # the bare 'int4' stays refused, and says where to go
        _head(llm_weight_quant="int4")
    with pytest.raises(PsgHipError, match="no LLM stage"):
        _head(llm_weight_quant="int4g", rel_cls_type="multiclass")
    with pytest.raises(PsgHipError, match="llm_weight_resident='quantised' is not built for the INT4 format"):
        _head(llm_weight_quant="int4g", llm_weight_resident="quantised")
    with pytest.raises(PsgHipError, match="llm_batch_weight_stream='quantised' is not built for the INT4 format"):
        _head(llm_weight_quant="int4g", llm_batch_weight_stream="quantised")
    with pytest.raises(ValueError, match="fmt"):
        quantize_llm_weights({}, 1, fmt="int3")
    fp8 = quantize_llm_weights({"language_model.model.layers.0.mlp.up_proj.weight": torch.randn(8, 256)}, 1, fmt="fp8")
    assert quant_format(fp8, "language_model.model.layers.0.mlp.up_proj.weight") == "fp8"
