"""llm_bf16_value_resident through the whole head (`-m gpu`): an fp32s head whose LLM matrices are bf16 VALUES
holds their bf16 copies only - no fp32 tensor, no split image - and runs every product on three bf16 planes of its fp32 rows.
The yardstick is the `llm_bf16_value_stream=True` head on the same weights and inputs, next to it in the same test: the
decode steps of <= 32 rows are the same kernel on the same operand (bit-equal from one state), the prompt pass is another
reduction order of the same exact products (first-step logits within twice that head's own distance from the CPU oracle,
DESIGN 16's rule, and within the project's fp32s bar of 1e-3), tokens equal up to each pair's first near-tie.

Cases: G6 (Llama-2-7B width, 2 layers, 20 pairs), G8 (grouped-query) and the small LLM of tests/test_gpu_w16.py
(512 / 1024 / 512), the LLM's matrices rounded through bf16 and held on the host.

Measured on an MI355X (first-step logits against the CPU oracle, stream head / resident head): G6 1.352e-4 / 1.335e-4,
small 1.139e-4 / 1.050e-4; tokens equal on all 320 (pair, step) entries of every case; constrained path and beam scores
1.06e-5 / 9.8e-6 from the oracle's table, the likelihood pass 1.9e-5 from the resident-off head's."""
import gc

import numpy as np
import pytest
import torch

from openpsg_amd._lib import PsgHipError
from tests import helpers as H
from tests.test_gpu_llm_batch_quant import _batch, _free
from tests.test_gpu_llm_batch_split import FP32S_ORACLE_BAR, _oracle_distance, _oracle_first_logits
from tests.test_gpu_llm_bf16_stream import _case, _decode, _names, _Spy, _valued
from tests.test_gpu_llm_resident import _inputs, _matrix_shapes, _tensors
from tests.test_gpu_llm_w8 import _assert_tokens_agree, _step_margins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("G6_llm_7b_width_n6", "G8_gqa_512_n10", "small")
ON = dict(llm_bf16_value_stream=True, llm_bf16_value_resident=True)
MATS = ("wqkv", "wo", "wgu", "wdown")


@pytest.fixture
def spy():
    s = _Spy()
    try:
        yield s
    finally:
        s.close()


def _host(w):
    return {k: torch.as_tensor(v).cpu() for k, v in w.items()}


def _bf16_case(name):
    cfg, w, scene, sup, sel = _case(name)
    return cfg, _host(_valued(w, torch.bfloat16)), scene, sup, sel


def _new(cfg, **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    return RelationTransformerHeadV4(dtype="fp32s", device=DEV, qformer_vocab_size=cfg.qformer.vocab, llm_config=cfg.llm,
                                     llm_feature_size=cfg.llm.hidden, tokenizers="word", max_object_num=cfg.max_object_num,
                                     on_parse_error="skip", **kw)


def _head(cfg, w, **kw):
    return _new(cfg, **kw).load_weights(w)


def _other_bytes(cfg):
    """`resident_bytes()['other']` of a resident engine, from the shapes: 2 bytes per weight of the decoder matrices and the
    lm_head; fp32 embedding, norms, rotary tables; language_projection as before (fp32, its split image and row scales)."""
    m, nq = cfg.llm, 768
    mats = 2 * sum(N * K for N, K in _matrix_shapes(m, True))
    proj = m.hidden * nq * 4 + m.hidden * 3 * nq * 2 + m.hidden * 4 + m.hidden * 4            # W, [wh | wl | wh], scales, bias
    return mats + 4 * m.vocab * m.hidden + 4 * m.hidden * (1 + 2 * m.layers) + 2 * 4 * 4096 * (m.head_dim // 2) + proj


def _assert_holds_bf16_only(eng, cfg):
    m = cfg.llm
    assert eng.bf16_value_resident and eng.bf16_stream_active and eng.layer_kind == "wb16"
    assert all(L[k] is M[k] for L, M in zip(eng.layers, eng.mats) for k in MATS) and eng.lm_head is eng.lm_head_mat
    for rec in eng.matrices():
        assert rec.w is None and rec.split is None and rec.packed is None and rec.w16 is None and rec.h16 is None
        assert rec.wb16.dtype == torch.bfloat16 and rec.stream[0] == "wb16" and rec.stream[1][0] is rec.wb16
    # no 4-byte tensor of a decoder matrix's element count anywhere in the engine (known by identity and allowed: the
    # embedding and language_projection, which are held as before, and the rotary tables - 4096 x 64 is the element count
    # of a 512 x 512 output projection).  Not walked: the graphs (KV caches, activations)
    counts = {N * K for N, K in _matrix_shapes(m, False)}
    allowed = {eng.embed.data_ptr()} | {t.data_ptr() for t in eng.proj_mat.tensors()} | {t.data_ptr() for t in eng.rope}
    for name, v in vars(eng).items():
        if name == "_graphs":
            continue
        for t in _tensors(v):
            assert not (t.numel() in counts and t.element_size() == 4 and t.data_ptr() not in allowed), (name, tuple(t.shape))
    rb = eng.resident_bytes()
    assert rb["quantised"] == 0 and rb["scratch"] == 0 and not eng._scratch
    assert rb["other"] == rb["total"] == _other_bytes(cfg)


def _step_slices(eng, st):
    """The lm_head slices of one 'wb16' decode step from the state `st`, which is left as it was."""
    x0 = st["x"].clone()
    out = eng._decode_step_split(st, "wb16").t.clone()
    st["x"].copy_(x0)
    return out


@pytest.mark.parametrize("case", CASES)
def test_no_fp32_copy_same_decode_steps_and_the_prompt_pass_within_the_oracle_rule(case, spy):
    cfg, wb, scene, sup, sel = _bf16_case(case)
    ref = _head(cfg, wb, suppress_eos=sup, llm_bf16_value_stream=True)
    d_ref = _decode(ref, scene, sel)
    t_ref, f_ref = np.asarray(d_ref["tokens_host"]).copy(), d_ref["first_logits"].float().cpu()
    margins = _step_margins(ref, d_ref, sup)
    log_ref = spy.take()
    rb_ref = ref.llm_engine.resident_bytes()

    # the load: only bf16 reaches the device, matrix by matrix
    own, llm = ({k: v for k, v in wb.items() if k.startswith("language_model.") == f} for f in (False, True))
    on = _new(cfg, suppress_eos=sup, **ON).load_weights(own)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    on.load_llm_weights(llm)
    torch.cuda.synchronize()
    peak, final = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
    eng = on.llm_engine
    _assert_holds_bf16_only(eng, cfg)
    rb = eng.resident_bytes()
    largest = 2 * max(N * K for N, K in _matrix_shapes(cfg.llm, True))
    print(f"{case}: resident_bytes {rb_ref['total']} -> {rb['total']} B; load growth {final} B, peak {peak} B "
          f"(allowed: {rb['total']} + {largest} + 2 MB)")
    assert final <= rb["total"] + (2 << 20)                                  # (allocator granules of ~100 small tensors)
    assert peak <= rb["total"] + largest + (2 << 20)
    for k in MATS:                                                           # the copies are the source's values, bit for bit
        assert torch.equal(eng.mats[0][k].wb16, ref.llm_engine.mats[0][k].wb16)

    d_on = _decode(on, scene, sel)
    t_on, f_on = np.asarray(d_on["tokens_host"]).copy(), d_on["first_logits"].float().cpu()
    log_on = spy.take()
    # a decode step's op sequence is exactly DESIGN 20's - the stream head's own
    strip = lambda log: [e if isinstance(e, str) else e[:2] for e in log]    # noqa: E731  (addresses differ between heads)
    per_step = ["rmsnorm_split_b16x3"]
    for _ in eng.layers:
        per_step += ["split_gemm_wb16", "decode_attn", "split_b16x3", "split_gemm_wb16", "rmsnorm_split_b16x3",
                     "split_gemm_wb16", "silu_mul_split_b16x3", "split_gemm_wb16", "rmsnorm_split_b16x3"]
    per_step += ["split_gemm_wb16", "greedy_step"]
    n = len(per_step)
    assert len(log_on) % n == 0 and all(_names(log_on[i:i + n]) == per_step for i in range(0, len(log_on), n))
    assert strip(log_on)[:n] == strip(log_ref)[:n]
    # one step from ONE post-prefill state (the stream head's) on both engines: the same kernel on the same operand
    st = ref.llm_engine._prefill(d_ref["llm_inputs"], d_ref["prompt_len"], cfg.max_new_tokens, sup, False)
    assert torch.equal(_step_slices(eng, st), _step_slices(ref.llm_engine, st))
    spy.take()
    # first-step logits (the prompt pass) against the CPU oracle on the same weights
    sel_list = [int(i) for i in d_ref["selected_host"]]
    assert sel_list == [int(i) for i in d_on["selected_host"]]
    on_host = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in scene.items()}    # (the oracle runs on the CPU)
    oracle = _oracle_first_logits((case, "bf16-valued"), wb, cfg, on_host, sel_list, sup)
    K = t_ref.shape[0]
    dist_ref, dist_on = _oracle_distance(f_ref, oracle, K, 1), _oracle_distance(f_on, oracle, K, 1)
    print(f"{case}: first-step logits against the CPU oracle: stream head {dist_ref:.3e}, resident head {dist_on:.3e} "
          f"(bars {FP32S_ORACLE_BAR:.0e} and twice the stream head's)")
    assert dist_on < FP32S_ORACLE_BAR and dist_on <= 2 * dist_ref
    _assert_tokens_agree(f"{case} resident against the stream head", t_on, t_ref, margins)
    _free(ref, on, d_ref, d_on)


def _batch_spy(monkeypatch):
    """While a decode step runs: the weight shapes of ops.batch_split_gemm_wb16 / _w32 calls, of F.linear calls and of
    torch.mm calls whose operands are fp32 (a bf16 torch.mm is the stacked-plane product, listed apart)."""
    from openpsg_amd import llm, ops
    calls = dict(wb16=[], w32=[], linear=[], mm_f32=[], mm_b16=[])
    state = {"in_steps": False}

    def wb16(x3, w, *a, _f=ops.batch_split_gemm_wb16, **kw):
        calls["wb16"].append((tuple(w.shape), int(x3.shape[1])))
        return _f(x3, w, *a, **kw)

    def w32(*a, _f=ops.batch_split_gemm_w32, **kw):
        calls["w32"].append(1)
        return _f(*a, **kw)

    def linear(x, w, *a, _f=llm.F.linear, **kw):
        if state["in_steps"]:
            calls["linear"].append(tuple(w.shape))
        return _f(x, w, *a, **kw)

    def mm(a, b, *r, _f=torch.mm, **kw):
        if state["in_steps"]:
            calls["mm_f32" if a.dtype == torch.float32 or b.dtype == torch.float32 else "mm_b16"].append((b.shape[1], b.shape[0]))
        return _f(a, b, *r, **kw)

    def steps(self, *a, _f=llm.LlamaDecodeEngine._steps, **kw):
        state["in_steps"] = True
        try:
            return _f(self, *a, **kw)
        finally:
            state["in_steps"] = False
    monkeypatch.setattr(ops, "batch_split_gemm_wb16", wb16)
    monkeypatch.setattr(ops, "batch_split_gemm_w32", w32)
    monkeypatch.setattr(llm.F, "linear", linear)
    monkeypatch.setattr(torch, "mm", mm)
    monkeypatch.setattr(llm.LlamaDecodeEngine, "_steps", steps)
    return calls


def test_forward_batch_runs_the_kernel_and_images_do_not_see_each_other(monkeypatch):
    """forward_batch([A, A]) at 40 rows: every decoder projection (and the lm_head) the routing table does not list goes
    through ops.batch_split_gemm_wb16, none through F.linear, an fp32 torch.mm or batch_split_gemm_w32; each image's tokens
    agree with the stream head's single-image decode.  [A, A, A] at 60 rows: three identical arrays, and the replay's."""
    from openpsg_amd.llm import _batch_wb16_route
    cfg, wb, scene, sup, _ = _bf16_case("G6_llm_7b_width_n6")
    inputs, names = _inputs(scene), H.object_names(scene)
    ref = _head(cfg, wb, suppress_eos=sup, llm_bf16_value_stream=True)
    rq = ref.run_relation_query(inputs["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]], names,
                                inputs["object_info"][0]["pan_results"])
    dec = ref.decode_selected(rq, names)
    t1 = np.asarray(dec["tokens_host"]).copy()
    margins = _step_margins(ref, dec, sup)
    K = t1.shape[0]
    assert 2 * K == 40
    _free(ref, rq, dec)
    on = _head(cfg, wb, suppress_eos=sup, **ON)
    assert on.llm_engine.decode_uses_library(2 * K)                          # (keeps its meaning: two such decodes never overlap)
    calls = _batch_spy(monkeypatch)
    _, toks, _ = _batch(on, inputs)
    shapes = set(_matrix_shapes(cfg.llm, True))
    own = {sh for sh in shapes if _batch_wb16_route(sh[0], sh[1], 2 * K) == "own"}
    assert own and {c[0] for c in calls["wb16"]} == own and {c[1] for c in calls["wb16"]} == {2 * K}
    assert set(calls["mm_b16"]) == shapes - own                              # (listed shapes: the stacked-plane product)
    assert not calls["linear"] and not calls["mm_f32"] and not calls["w32"]
    for i, t in enumerate(toks):
        _assert_tokens_agree(f"G6 resident batch of 2, image {i}", t, t1, margins)
    res3, toks3, _ = _batch(on, inputs, n=3)
    assert {c[1] for c in calls["wb16"]} == {2 * K, 3 * K}
    assert np.array_equal(toks3[0], toks3[1]) and np.array_equal(toks3[0], toks3[2]) and res3[0] == res3[1] == res3[2]
    res3b, toks3b, _ = _batch(on, inputs, n=3)
    assert res3b == res3 and all(np.array_equal(a, b) for a, b in zip(toks3, toks3b))


def test_constrained_decode_and_a_beam_against_the_oracle_table(monkeypatch):
    """G8, bf16-valued: a constrained run returns one valid triple per selected pair whose path log-probability is within
    DESIGN 22's 2e-4 of the oracle's per-edge table (tests/beam_oracle.py); a beam of width 3 (60 rows: the levels' projections
    on psg_batch_split_gemm_wb16) returns valid classes with scores within the same bound."""
    from tests.test_gpu_llm_beam import _full_scores, _score_error, _table_for
    cfg, wb, scene, sup, _ = _bf16_case("G8_gqa_512_n10")
    inp = _inputs(scene)
    con = _head(cfg, wb, llm_decode="constrained", llm_rel_scores="likelihood", **ON)
    rc = con(inp)
    last, trie = con.last, con.relation_trie()
    sel, N = last["selected_host"], len(scene["object_id_list"])
    K = len(sel)
    assert len(rc["rel_pred"]) == K
    full = _full_scores(trie, _table_for(("G8 bf16-valued resident", "fp32s"), cfg, wb, last, trie))
    lp = np.asarray(last["path_logp_host"], dtype=np.float64)
    cls = []
    for k, (s, o, rel) in enumerate(rc["rel_pred"]):
        assert (s, o) == (int(sel[k]) // N, int(sel[k]) % N)
        assert [int(t) for t in np.asarray(last["tokens_host"])[k] if t >= 0] == trie.candidates[rel]
        cls.append(rel)
    err = float(np.abs(lp - full[np.arange(K), cls]).max())
    print(f"G8 resident, constrained: |path logp - oracle path sum| {err:.3e} (bound 2e-4)")
    assert err <= 2e-4 and con(inp) == rc
    _free(con)
    beam = _head(cfg, wb, llm_decode="constrained", llm_rel_scores="likelihood", llm_beam_width=3, **ON)
    calls = _batch_spy(monkeypatch)
    rb = beam(inp)
    assert beam.last["beam_class_host"].shape == (K, 3) and 3 * K == 60
    assert calls["wb16"] and {c[1] for c in calls["wb16"]} == {60} and not calls["linear"] and not calls["mm_f32"]
    assert np.array_equal(beam.last["selected_host"], sel)
    err = _score_error(beam.last, full)
    print(f"G8 resident, beam of 3: |beam logp - oracle path sum| {err:.3e} (bound 2e-4)")
    assert err <= 2e-4 and beam(inp) == rb
    trip = {(s, o) for s, o, _ in rb["rel_pred"]}
    assert trip <= {(int(x) // N, int(x) % N) for x in sel} and all(0 <= r < len(trie.candidates) for _, _, r in rb["rel_pred"])


def test_submit_with_two_slots_in_flight_and_the_likelihood_pass():
    cfg, wb, scene, sup, _ = _bf16_case("G8_gqa_512_n10")
    inp = _inputs(scene)
    head = _head(cfg, wb, suppress_eos=sup, **ON)
    r = head(inp)
    assert head(inp) == r and head.submit(inp).result() == r
    p0, p1 = head.submit(inp, slot=0), head.submit(inp, slot=1)
    assert p1.result() == r and p0.result() == r
    _free(head)
    # the relation-likelihood pass (the trie pass: stacked-plane library products) against the resident-off head's
    off = _head(cfg, wb, llm_rel_scores="likelihood", llm_bf16_value_stream=True)
    off(inp)
    ls_off, sel = np.asarray(off.last["logscores_host"], dtype=np.float64), off.last["selected_host"].copy()
    _free(off)
    on = _head(cfg, wb, llm_rel_scores="likelihood", **ON)
    on(inp)
    assert np.array_equal(on.last["selected_host"], sel)
    err = float(np.abs(np.asarray(on.last["logscores_host"], dtype=np.float64) - ls_off).max())
    print(f"G8 resident, likelihood pass: |log s - the resident-off head's| {err:.3e} (bound 2e-4)")
    assert err <= 2e-4


def test_every_refusal():
    cfg, wb, scene, sup, _ = _bf16_case("small")
    name = "language_model.model.layers.1.mlp.down_proj.weight"
    bad = dict(wb)
    bad[name] = wb[name] + 2.0 ** -20
    with pytest.raises(PsgHipError, match=f"llm_bf16_value_resident.*1 decoder matrices are not bf16 values.*{name}.*"
                                          "llm_bf16_value_resident=False runs them"):
        _head(cfg, bad, **ON)
    # an lm_head fine-tuned in fp32 keeps its fp32 tensor and today's routes
    mixed = dict(wb)
    mixed["language_model.lm_head.weight"] = wb["language_model.lm_head.weight"] + 2.0 ** -20
    head = _head(cfg, mixed, suppress_eos=sup, **ON)
    eng = head.llm_engine
    assert eng.lm_head_mat.w is not None and eng.lm_head_mat.w.dtype == torch.float32 and eng.lm_head_mat.wb16 is None
    assert all(rec.w is None for rec in eng._layer_mats())
    ref = _head(cfg, mixed, suppress_eos=sup, llm_bf16_value_stream=True)
    _, _, _, _, sel = _case("small")
    d_ref, d_on = _decode(ref, scene, sel), _decode(head, scene, sel)
    _assert_tokens_agree("small, fp32 lm_head", np.asarray(d_on["tokens_host"]), np.asarray(d_ref["tokens_host"]),
                         _step_margins(ref, d_ref, sup))
    _free(ref, d_ref, d_on)
    with pytest.raises(PsgHipError, match="use_skinny=False.*llm_bf16_value_resident=False"):
        eng.use_skinny = False
    with pytest.raises(PsgHipError, match="row-invariant.*llm_bf16_value_resident=False"):
        eng.row_invariant = True
    assert eng.use_skinny and not eng.row_invariant
    with pytest.raises(PsgHipError, match="bf16_value_resident.*training forward"):
        eng.teacher_forcing_logits(torch.zeros((1, 4, cfg.llm.hidden), device=DEV), torch.tensor([4], device=DEV),
                                   torch.arange(4, device=DEV, dtype=torch.int32), torch.tensor([3], device=DEV))
    with pytest.raises(PsgHipError, match="no dense operand"):
        eng._dense(eng.mats[0]["wo"])
    head.train(True)
    train_inputs = dict(_inputs(scene))
    for fn in (head.forward_train, head.forward_train_grad):
        with pytest.raises(PsgHipError, match="llm_bf16_value_resident=True is an inference mode"):
            fn(train_inputs)
    head.train(False)


def test_a_model_the_decode_steps_cannot_stream_is_refused_at_construction(monkeypatch):
    """There is no dense fallback: a model that fails a condition of the 'wb16' decode route raises when the engine is built,
    naming the condition and the remedy - an MLP width that is no multiple of 64, and a decoder shape listed in
    `llm.WB16_STREAM_OFF`.  The same models load with the option off (and then do not take the stream)."""
    from openpsg_amd import llm
    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.weights import make_weights_device
    cfg = PSGConfig(qformer=QFormerConfig(vocab=30522), llm=tiny_llm(512, 2, 992, 512), max_object_num=50)
    wb = _host(_valued(make_weights_device(cfg, 7, torch.device(DEV), llm_dtype=torch.float32), torch.bfloat16))
    with pytest.raises(PsgHipError, match="cannot stream the bf16 copies.*inter = 992 is no multiple of 64.*"
                                          "llm_bf16_value_resident=False"):
        _head(cfg, wb, **ON)
    off = _head(cfg, wb, llm_bf16_value_stream=True)
    assert not off.llm_engine.bf16_stream_active and all(rec.w is not None for rec in off.llm_engine.matrices())
    _free(off)
    cfg, wb, _, _, _ = _bf16_case("small")
    monkeypatch.setattr(llm, "WB16_STREAM_OFF", frozenset({(cfg.llm.hidden, cfg.llm.inter)}))
    with pytest.raises(PsgHipError, match=r"cannot stream the bf16 copies.*\(512, 1024\)\] is listed in WB16_STREAM_OFF.*"
                                          "llm_bf16_value_resident=False"):
        _head(cfg, wb, **ON)
    monkeypatch.setattr(llm, "WB16_STREAM_OFF", frozenset())
    assert _head(cfg, wb, **ON).llm_engine.bf16_stream_active


def test_a_bf16_checkpoint_directory_loads_through_the_constructor(tmp_path):
    """A checkpoint directory saved in bf16 (torch.bfloat16 tensors on disk) read by the constructor: the records are the
    stored values bit for bit, and the head decodes the tokens of the stream head on the same directory."""
    import json
    import os
    from safetensors.torch import save_file
    from openpsg_amd.head import RelationTransformerHeadV4
    cfg, wb, scene, sup, sel = _bf16_case("small")
    m = cfg.llm
    d = str(tmp_path / "bf16")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(architectures=["LlamaForCausalLM"], hidden_size=m.hidden, num_attention_heads=m.heads,
                       num_key_value_heads=m.n_kv_heads, num_hidden_layers=m.layers, intermediate_size=m.inter,
                       vocab_size=m.vocab, rms_norm_eps=m.rms_eps, rope_theta=m.rope_theta, bos_token_id=m.bos,
                       eos_token_id=m.eos, torch_dtype="bfloat16", tie_word_embeddings=False), f)
    save_file({k[len("language_model."):]: v.bfloat16().contiguous() for k, v in wb.items() if k.startswith("language_model.")},
              os.path.join(d, "model.safetensors"))
    kw = dict(dtype="fp32s", device=DEV, qformer_vocab_size=cfg.qformer.vocab, tokenizers="word",
              max_object_num=cfg.max_object_num, on_parse_error="skip", suppress_eos=sup, llm_feature_size=m.hidden,
              llm_model_name=d)
    own = {k: v for k, v in wb.items() if not k.startswith("language_model.")}
    a = RelationTransformerHeadV4(llm_bf16_value_stream=True, **kw)
    a.load_state_dict(own, strict=False)
    b = RelationTransformerHeadV4(**ON, **kw)
    b.load_state_dict(own, strict=False)
    _assert_holds_bf16_only(b.llm_engine, cfg)
    key = "language_model.model.layers.0.mlp.down_proj.weight"
    assert torch.equal(b.llm_engine.mats[0]["wdown"].wb16.cpu().view(torch.int16), wb[key].bfloat16().view(torch.int16))
    d_a, d_b = _decode(a, scene, sel), _decode(b, scene, sel)
    _assert_tokens_agree("small, bf16 directory", np.asarray(d_b["tokens_host"]), np.asarray(d_a["tokens_host"]),
                         _step_margins(a, d_a, sup))


def test_the_option_off_is_the_head_without_the_keyword(spy):
    cfg, wb, scene, sup, sel = _bf16_case("small")
    out = {}
    for name, kw in (("plain", {}), ("off", dict(llm_bf16_value_resident=False))):
        h = _head(cfg, wb, suppress_eos=sup, llm_bf16_value_stream=True, **kw)
        assert not h.llm_engine.bf16_value_resident and all(rec.w is not None for rec in h.llm_engine.matrices())
        d = _decode(h, scene, sel)
        out[name] = (np.asarray(d["tokens_host"]).copy(), d["first_logits"].clone(), h.llm_engine.resident_bytes(),
                     [e if isinstance(e, str) else e[:2] for e in spy.take()])
        _free(h, d)
    assert np.array_equal(out["plain"][0], out["off"][0]) and torch.equal(out["plain"][1], out["off"][1])
    assert out["plain"][2] == out["off"][2] and out["plain"][3] == out["off"][3]
