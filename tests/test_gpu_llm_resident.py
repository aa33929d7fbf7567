"""llm_weight_resident='quantised' through the whole head (`-m gpu`).  The dense operands a lean engine rebuilds
are bit-identical to the ones the 'all' engine stores (tests/test_gpu_expand.py) and go into the same products, so a lean
head is held to the 'all' head on the SAME quantised weights by equality: `torch.equal` on first-step logits, `array_equal`
on tokens, graph replay included - never a tolerance."""
import gc

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_llm_w8 import _head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MATS = ("wqkv", "wo", "wgu", "wdown")


def _quantised(w, cfg, fmt, lm_head=False):
    """The model both heads are loaded with: quantised ONCE, so that 'all' and 'quantised' hold the same (q, [e,] s)."""
    from openpsg_amd.weights import quantize_llm_weights
    return quantize_llm_weights({k: torch.as_tensor(v) for k, v in w.items()}, cfg.llm.layers, lm_head, fmt)


def _inputs(scene, drop=0):
    dev = torch.device(DEV)
    ids = list(scene["object_id_list"])
    return dict(mask_features=scene["mask_features"].to(dev), img_metas=[scene["img_meta"]],
                object_info=[dict(object_id_list=ids[:len(ids) - drop], pan_results=scene["pan_results"].to(dev))])


def _decode(head, g, scene):
    """(existence logits, tokens, first-step logits) of the golden's selection, and the same again from the graph replay."""
    dev = torch.device(DEV)
    names = H.object_names(scene)
    rq = head.run_relation_query(scene["mask_features"].to(dev), scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                                 names, scene["pan_results"].to(dev))
    sel = torch.from_numpy(g["selected"].astype(np.int32)).to(dev)
    out = []
    for _ in range(2):
        dec = head.decode_selected(rq, names, selected=sel)
        out.append((np.asarray(dec["tokens_host"]).copy(), dec["first_logits"].clone()))
    return rq["exist_logit"].clone(), out


def _matrix_shapes(m, lm_head):
    per_layer = [(m.hidden + 2 * m.kv_dim, m.hidden), (m.hidden, m.hidden), (2 * m.inter, m.hidden), (m.hidden, m.inter)]
    return per_layer * m.layers + ([(m.vocab, m.hidden)] if lm_head else [])


def _quantised_bytes(m, fmt, lm_head):
    """numel * element_size of the quantised parts, from the config's shapes.  fp8: q [N, K] + s fp32 [N].  mxfp4: q
    [N, K / 2] + the raw block exponents [N, K / 32] (read by the expansion) + the decode kernels' exponent image (the same
    bytes re-laid-out) + s fp32 [N]."""
    if fmt == "fp8":
        return sum(N * K + 4 * N for N, K in _matrix_shapes(m, lm_head))
    return sum(N * K // 2 + 2 * (N * K // 32) + 4 * N for N, K in _matrix_shapes(m, lm_head))


def _tensors(o, skip=()):
    """Every tensor reachable from an engine attribute / layer table (matrix records opened)."""
    from openpsg_amd.llm_matrix import LlmMatrix
    if isinstance(o, torch.Tensor):
        yield o
    elif isinstance(o, LlmMatrix):
        yield from o.tensors()
    elif isinstance(o, dict):
        for v in o.values():
            yield from _tensors(v)
    elif isinstance(o, (list, tuple)):
        for v in o:
            yield from _tensors(v)


def _assert_holds_bytes_only(eng, m, fmt, lm_head):
    assert eng.resident == "quantised"
    # the layer tables and `lm_head` hold the record itself in place of W': there is none
    assert all(L[k] is M[k] and M[k].w is None for L, M in zip(eng.layers, eng.mats) for k in MATS)
    assert (eng.lm_head is eng.lm_head_mat and eng.lm_head_mat.w is None) == bool(lm_head)
    assert all(rec.h16 is None and rec.i2 is None for rec in eng.matrices() + [eng.proj_mat])
    # (`_w16`: fp16 images of fp16-VALUED matrices that are not quantised - at most the dense lm_head of an fp16 checkpoint)
    assert set(eng._w16) <= (set() if lm_head else {eng.lm_head.data_ptr()})
    assert all(rec.split is None for rec in eng.matrices())
    rb = eng.resident_bytes()
    assert rb["quantised"] == _quantised_bytes(m, fmt, lm_head)
    assert rb["scratch"] == sum(t.numel() * t.element_size() for t in eng._scratch.values()) > 0
    assert rb["total"] == rb["quantised"] + rb["scratch"] + rb["other"]
    # no tensor with a decoder matrix's element count in a floating type outside the scratch.  Not walked: the graphs (KV
    # caches, activations).  Known by identity and allowed: the scratch and the matrices that are NOT quantised (embedding,
    # a dense lm_head, language_projection and its split image, rotary tables), whatever table refers to them
    counts = {N * K for N, K in _matrix_shapes(m, lm_head)}
    allowed = {t.data_ptr() for n in ("_scratch", "embed", "proj_mat", "proj_b", "rope") for t in _tensors(getattr(eng, n))}
    if not lm_head:
        allowed.add(eng.lm_head.data_ptr())
        allowed |= {t.data_ptr() for t in eng._w16.values()}                 # (its fp16 image, asserted above to be the only entry)
    for name, val in vars(eng).items():
        if name in ("_graphs", "_dl_ws"):
            continue
        for t in _tensors(val):
            assert t.data_ptr() in allowed or not (t.is_floating_point() and t.element_size() >= 2 and t.numel() in counts), \
                f"engine.{name} holds a dense {t.dtype} tensor of {t.numel()} elements"


def _pair(case, loader, dtype, fmt, lm_head=False):
    g, cfg, w, scene = loader(case)
    sup = bool(g["suppress_eos"])
    wq = _quantised(w, cfg, fmt, lm_head)
    kw = dict(suppress_eos=sup, llm_weight_quant=fmt, llm_quantize_lm_head=lm_head)
    ref = _head(cfg, wq, dtype, **kw)
    assert ref.llm_engine.resident == "all" and not ref.llm_engine._scratch
    e0, runs0 = _decode(ref, g, scene)
    del ref
    gc.collect()
    torch.cuda.empty_cache()
    lean = _head(cfg, wq, dtype, llm_weight_resident="quantised", **kw)
    eng = lean.llm_engine
    _assert_holds_bytes_only(eng, cfg.llm, fmt, lm_head)
    assert not eng.decode_uses_library(20)                                   # decode steps stay on the byte streams
    e1, runs1 = _decode(lean, g, scene)
    assert torch.equal(e1, e0)                                               # the relation query never sees the option
    for i, ((t0, f0), (t1, f1)) in enumerate(zip(runs0, runs1)):
        d = (f1.float() - f0.float()).abs().max().item()
        print(f"{case} {dtype} {fmt} run {i}: first-step logits lean vs all: max |diff| {d:.3e}, tokens equal "
              f"{np.array_equal(t1, t0)}")
        assert torch.equal(f1.view(torch.int32 if f1.dtype == torch.float32 else torch.int16),
                           f0.view(torch.int32 if f0.dtype == torch.float32 else torch.int16)), f"run {i}: first logits differ"
        assert np.array_equal(t1, t0), f"run {i}: tokens differ"
    _assert_holds_bytes_only(eng, cfg.llm, fmt, lm_head)                     # ... and nothing dense was cached by running
    return lean


def test_g6_fp32s_fp8():
    _pair("G6_llm_7b_width_n6", H.load_case, "fp32s", "fp8")


def test_g8_grouped_query_fp32s_mxfp4_with_the_lm_head():
    from tests.test_gpu_gqa_head import load_gqa_case
    _pair("G8_gqa_512_n10", load_gqa_case, "fp32s", "mxfp4", lm_head=True)


def test_g1_mixed_fp8():
    _pair("G1_c1_512_n10", H.load_case, "mixed", "fp8")


def test_g1_bf16_mxfp4():
    _pair("G1_c1_512_n10", H.load_case, "bf16", "mxfp4")


def test_two_images_in_flight_on_two_slots_have_a_scratch_each():
    """Image A on slot 0, image B on slot 1 before A's result is taken: each returns what `head(inputs)` returns."""
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    head = _head(cfg, _quantised(w, cfg, "fp8"), "fp32s", suppress_eos=bool(g["suppress_eos"]), llm_weight_quant="fp8",
                 llm_weight_resident="quantised")
    a, b = _inputs(scene), _inputs(scene, drop=2)
    ra, ta = head(a), head.last["tokens_host"].copy()                        # (seeded weights emit no parsable relation: the
    rb, tb = head(b), head.last["tokens_host"].copy()                        # tokens are what tells two images apart)
    assert not np.array_equal(ta, tb)
    for _ in range(2):                                                       # capture, then replay
        pa = head.submit(a, slot=0)
        pb = head.submit(b, slot=1)
        assert pa.result() == ra and np.array_equal(head.last["tokens_host"], ta)
        assert pb.result() == rb and np.array_equal(head.last["tokens_host"], tb)
    # engine slot 0 is `forward`'s (the caller's stream), submit slot k decodes on engine slot k + 1: three streams, three buffers
    sc = head.llm_engine._scratch
    assert set(sc) == {0, 1, 2} and len({t.data_ptr() for t in sc.values()}) == 3
    assert head.llm_engine.resident_bytes()["scratch"] == 3 * sc[0].numel() * sc[0].element_size()


def test_forward_batch_expands_above_32_rows():
    """forward_batch([inputs, inputs]) on G1 `mixed` fp8 (40 decode rows: one expansion per matrix per step): tokens and
    per-image results equal the 'all' head's forward_batch."""
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    wq = _quantised(w, cfg, "fp8")
    kw = dict(suppress_eos=bool(g["suppress_eos"]), llm_weight_quant="fp8")
    ref = _head(cfg, wq, "mixed", **kw)
    r0 = ref.forward_batch([_inputs(scene), _inputs(scene)])
    t0 = [np.asarray(lb["tokens_host"]).copy() for lb in ref.last_batch]
    del ref
    gc.collect()
    torch.cuda.empty_cache()
    lean = _head(cfg, wq, "mixed", llm_weight_resident="quantised", **kw)
    r1 = lean.forward_batch([_inputs(scene), _inputs(scene)])
    assert len(r1) == 2 and r1 == r0
    for a, lb in zip(t0, lean.last_batch):
        assert np.array_equal(np.asarray(lb["tokens_host"]), a)


def test_likelihood_scores_equal_the_all_heads():
    """llm_rel_scores='likelihood' on G1 fp32s fp8: the trie pass (more than 32 rows: every projection expands first) gives
    the 'all' head's log scores bit for bit."""
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    wq = _quantised(w, cfg, "fp8")
    kw = dict(suppress_eos=bool(g["suppress_eos"]), llm_weight_quant="fp8", llm_rel_scores="likelihood",
              num_llm_ranked_triples=50)
    ref = _head(cfg, wq, "fp32s", **kw)
    r0 = ref(_inputs(scene))
    ls0, t0 = ref.last["logscores_host"].copy(), np.asarray(ref.last["tokens_host"]).copy()
    del ref
    gc.collect()
    torch.cuda.empty_cache()
    lean = _head(cfg, wq, "fp32s", llm_weight_resident="quantised", **kw)
    r1 = lean(_inputs(scene))
    assert np.array_equal(np.asarray(lean.last["tokens_host"]), t0)
    assert np.array_equal(lean.last["logscores_host"].view(np.int32), ls0.view(np.int32))
    assert r1 == r0 and lean(_inputs(scene)) == r0                           # graph replay


def _tiny(hidden=256, layers=1, inter=512):
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.weights import make_weights_numpy
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(hidden, layers, inter, 512), max_object_num=30)
    return cfg, make_weights_numpy(cfg, seed=5)


def test_refusals_name_the_remedy():
    from openpsg_amd._lib import PsgHipError
    cfg, w = _tiny()
    with pytest.raises(PsgHipError, match=r"llm_weight_quant='fp8' / 'mxfp4'.*resident='all'"):     # an unquantised model
        _head(cfg, w, "fp32s", llm_weight_resident="quantised")
    with pytest.raises(PsgHipError, match=r"dtype='fp32'.*resident='all'"):                        # the exact fp32 mode
        _head(cfg, w, "fp32", llm_weight_quant="fp8", llm_weight_resident="quantised")
    head = _head(cfg, w, "fp32s", llm_weight_quant="fp8", llm_weight_resident="quantised")
    with pytest.raises(PsgHipError, match=r"row-invariant.*resident='all'"):
        head.llm_engine.row_invariant = True
    head.llm_engine.row_invariant = False                                    # (switching it OFF is no request for dense images)
    assert head.llm_engine.row_invariant is False
    g, _, _, inputs = H.load_train_case("T1_train_512_n7")
    head.train(True)                                                         # mmdet toggles the flag freely: no error here
    head.train(False)
    head.train(True)
    for call in (head.forward_train, head.forward_train_grad):
        with pytest.raises(PsgHipError, match=r"llm_weight_resident='all' to train"):
            call(inputs)
    head.train(False)
    with pytest.raises(PsgHipError, match=r"resident='all'"):
        head.llm_engine.teacher_forcing_logits(torch.zeros((1, 4, 256), device=DEV), torch.tensor([4], device=DEV),
                                               torch.arange(4, device=DEV, dtype=torch.int32), torch.tensor([3], device=DEV))
    cfg, w = _tiny(inter=160)                                                # the down projection has K = 160
    with pytest.raises(PsgHipError, match=r"layers\.0\.mlp\.down_proj \[256, 160\].*K % 128 == 0.*resident='all' runs it on W'"):
        _head(cfg, w, "mixed", llm_weight_quant="fp8", llm_weight_resident="quantised")
    cfg, w = _tiny(inter=384)                                                # ... K = 384
    with pytest.raises(PsgHipError, match=r"layers\.0\.mlp\.down_proj \[256, 384\].*K % 256 == 0.*resident='all' runs it on W'"):
        _head(cfg, w, "mixed", llm_weight_quant="mxfp4", llm_weight_resident="quantised")


def _load_growth(cfg, w, **kw):
    """(memory_allocated growth across construction + load_weights, peak above the final value during it, the head)."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    head = _head(cfg, w, "fp32s", llm_weight_quant="fp8", **kw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    gc.collect()
    torch.cuda.empty_cache()
    final = torch.cuda.memory_allocated()
    return final - base, peak - final, head


def test_memory_of_a_lean_head_and_of_its_load():
    """tiny_llm(512, 8, 1024, 512), fp32s, fp8, host weights.  W = the decoder's weight count.  The 'all' head holds 4 + 1 + 2
    bytes per weight, the lean one 1 plus its scratch: the growth differs by at least 0.9 x 6 W.  The lean load never has
    the dense model on the device: its peak stays within the final value + 3 x 4 bytes x the largest matrix + 16 MB."""
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.weights import make_weights_numpy, quantize_fp8_rows
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(512, 8, 1024, 512), max_object_num=30)
    w = {k: torch.as_tensor(v) for k, v in make_weights_numpy(cfg, seed=9).items()}
    shapes = _matrix_shapes(cfg.llm, False)
    W, largest = sum(N * K for N, K in shapes), max(N * K for N, K in shapes)
    g_all, _, head = _load_growth(cfg, w)
    del head
    g_lean, over, head = _load_growth(cfg, w, llm_weight_resident="quantised")
    print(f"W = {W}: growth 'all' {g_all} B, 'quantised' {g_lean} B, difference {(g_all - g_lean) / W:.2f} B per weight; "
          f"lean load peak above final {over} B (allowed {12 * largest + (16 << 20)})")
    assert g_all - g_lean >= 0.9 * 6 * W
    assert over <= 3 * 4 * largest + (16 << 20)
    rb = head.llm_engine.resident_bytes()
    assert rb["quantised"] == _quantised_bytes(cfg.llm, "fp8", False) and rb["scratch"] == 4 * largest
    # the loader quantised in row chunks where the weights live: the bytes and scales of the one-shot quantisation 'all' runs
    L0 = head.llm_engine.layers[0]["wdown"]
    q, s = quantize_fp8_rows(w["language_model.model.layers.0.mlp.down_proj.weight"])
    assert torch.equal(L0.q.cpu(), q) and torch.equal(L0.s.cpu(), s)


def test_fp8_checkpoint_directory_read_lean(tmp_path):
    """The FP8 checkpoint directory of tests/test_fp8_quant_cpu.py read by the constructor with
    llm_weight_resident='quantised' (no llm_weight_quant: the checkpoint IS quantised) decodes the tokens of the same
    directory read with 'all'."""
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_scene
    from tests.test_fp8_quant_cpu import write_fp8_checkpoint
    cfg, w = _tiny(layers=2)
    d = str(tmp_path / "fp8")
    write_fp8_checkpoint(d, cfg, w)
    kw = dict(dtype="fp32s", device=DEV, qformer_vocab_size=512, tokenizers="word", max_object_num=30, on_parse_error="skip",
              suppress_eos=True, llm_feature_size=256, llm_model_name=d)
    own = {k: v for k, v in w.items() if not k.startswith("language_model.")}
    scene = make_scene((512, 512), 6, seed=3, device=DEV)
    inputs = dict(mask_features=scene["mask_features"], img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"])])
    a = RelationTransformerHeadV4(**kw)
    a.load_state_dict(own, strict=False)
    ra = a(inputs)
    b = RelationTransformerHeadV4(llm_weight_resident="quantised", **kw)
    b.load_state_dict(own, strict=False)
    assert b.llm_engine.resident == "quantised" and b.llm_engine.layer_kind == "w8"
    _assert_holds_bytes_only(b.llm_engine, cfg.llm, "fp8", False)
    rb = b(inputs)
    assert torch.equal(a.last["tokens"], b.last["tokens"]) and torch.equal(a.last["first_logits"], b.last["first_logits"])
    assert ra["rel_pred"] == rb["rel_pred"]
