"""llm_batch_split_gemm='own' through the whole head (`-m gpu`): forward_batch's decode steps of 33..160 rows of
an fp32s head over its UNQUANTISED matrices on psg_batch_gemm_s.hip.  The option changes which kernel computes a projection
of the same weights, so a head with it is held to what the option-off forward_batch is held to, in the same test, on the
same inputs, next to the option-off head: each image's tokens agree with that image's single-image decode up to each
pair's first near-tie, and the first-step logits of every image stay within the fp32s bar (1e-3, tests/test_gpu_llm_w8.py)
of the CPU oracle on the same weights."""
import numpy as np
import pytest
import torch

from openpsg_amd.llm import _batch_split_route
from tests import helpers as H
from tests.test_gpu_llm_batch_quant import _batch, _free, _load
from tests.test_gpu_llm_resident import _inputs, _matrix_shapes, _quantised
from tests.test_gpu_llm_w8 import _assert_tokens_agree, _head, _step_margins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ("batch_split_gemm_w16", "batch_split_gemm_w32")
FP32S_ORACLE_BAR = 1e-3                                       # tests/test_gpu_llm_w8.py, tests/test_gpu_llm7b.py at this width


def _spy(monkeypatch):
    """Calls of the two new entries by weight shape (N, K), and the library products (F.linear / torch.mm) of more than 32
    rows issued while a decode step runs (`LlamaDecodeEngine._steps`: the prompt pass is over by then), by weight shape.
    A product whose weight is one of `calls["head_ptrs"]` (the lm_head and its fp16 copy, `_watch_head`) is listed under
    "<name>_head" instead: G8's lm_head has the shape of its output projection."""
    from openpsg_amd import llm, ops
    calls = {n + t: [] for n in ENTRIES + ("library",) for t in ("", "_head")}
    calls["head_ptrs"] = set()
    state = {"in_steps": False}

    def note(name, w, shape):
        calls[name + ("_head" if w.data_ptr() in calls["head_ptrs"] else "")].append(shape)

    def w16(*a, _f=ops.batch_split_gemm_w16, **kw):
        note("batch_split_gemm_w16", a[2], (int(a[2].shape[0]), int(a[2].shape[1])))
        return _f(*a, **kw)

    def w32(*a, _f=ops.batch_split_gemm_w32, **kw):
        note("batch_split_gemm_w32", a[2], (int(a[2].shape[0]), int(a[4])))
        return _f(*a, **kw)
    monkeypatch.setattr(ops, "batch_split_gemm_w16", w16)
    monkeypatch.setattr(ops, "batch_split_gemm_w32", w32)

    def linear(x, w, *a, _f=llm.F.linear, **kw):
        if state["in_steps"] and x.dim() == 2 and x.shape[0] > 32:
            note("library", w, (int(w.shape[0]), int(w.shape[1])))
        return _f(x, w, *a, **kw)

    def mm(a, b, *r, _f=torch.mm, **kw):
        if state["in_steps"] and a.shape[0] > 32:
            note("library", b, (int(b.shape[1]), int(b.shape[0])))
        return _f(a, b, *r, **kw)
    monkeypatch.setattr(llm.F, "linear", linear)
    monkeypatch.setattr(torch, "mm", mm)

    def steps(self, *a, _f=llm.LlamaDecodeEngine._steps, **kw):
        state["in_steps"] = True
        try:
            return _f(self, *a, **kw)
        finally:
            state["in_steps"] = False
    monkeypatch.setattr(llm.LlamaDecodeEngine, "_steps", steps)
    return calls


def _watch_head(calls, head):
    eng = head.llm_engine
    rec = eng.lm_head_mat
    copies = [rec.w16, rec.packed[0] if rec.packed is not None else None]
    calls["head_ptrs"] = {eng.lm_head.data_ptr()} | {c.data_ptr() for c in copies if c is not None}
    for n in list(calls):
        if n != "head_ptrs":
            calls[n].clear()


def _fp16_valued(w):
    """Every LLM matrix rounded to an fp16 value: what from_pretrained yields from a checkpoint that is fp16 on disk."""
    return {k: (torch.as_tensor(v).half().float() if k.startswith("language_model.") and torch.as_tensor(v).dim() >= 2 else v)
            for k, v in w.items()}


_ORACLE = {}


def _oracle_first_logits(key, w, cfg, scene, sel, suppress):
    """First-step logits [K, vocab] of the CPU oracle for the pairs `sel` on the weights `w`; made once per (case, weights)."""
    if key not in _ORACLE:
        from oracle import psg_oracle as O
        if getattr(cfg.llm, "kv_heads", None):                               # the oracle is multi-head: the same function with
            from tests.test_gpu_gqa_head import expand_to_mha               # each key / value head repeated over its group
            cfg, w = expand_to_mha(cfg, w)
        qids, qmask = H.qformer_prompts(scene)
        pids, pmask = H.llm_prompts(scene, sel)
        out = []
        with torch.no_grad():
            orq = O.relation_query(w, cfg, scene["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                                   scene["pan_results"], qids, qmask)
            for i, si in enumerate(sel):
                x, mask = O.llm_inputs(w, orq["pair_feature"][si], pids[i], pmask[i])
                _, lg = O.llm_generate(w, cfg, x, mask, max_new_tokens=1, suppress_eos=suppress)
                out.append(lg[0].float())
        _ORACLE[key] = torch.stack(out)
    return _ORACLE[key]


def _oracle_distance(fl, ref, K, n):
    keep = torch.isfinite(ref)
    return max((fl[i * K:(i + 1) * K][keep] - ref[keep]).abs().max().item() for i in range(n))


@pytest.mark.parametrize("case,valued,entry", [
    ("G6_llm_7b_width_n6", False, "batch_split_gemm_w32"),
    ("G6_llm_7b_width_n6", True, "batch_split_gemm_w16"),
    ("G8_gqa_512_n10", False, "batch_split_gemm_w32"),
], ids=["G6-generic", "G6-fp16-valued", "G8-gqa-generic"])
def test_two_images_run_the_kernel_and_agree_with_the_single_image_decode_and_the_oracle(case, valued, entry, monkeypatch):
    """Option off: neither new entry is called.  Option on: every decoder projection of the 2 K-row steps that the routing
    table does not list goes through `entry`, none of them through F.linear / torch.mm.  Both batches agree with the
    single-image tokens up to each pair's first near-tie (>= 90 % of each image's entries compared), and both batches'
    first-step logits are within 1e-3 of the CPU oracle's for every image."""
    g, cfg, w, scene = _load(case)
    if valued:
        w = _fp16_valued(w)
    sup = bool(g["suppress_eos"])
    inputs, names = _inputs(scene), H.object_names(scene)
    calls = _spy(monkeypatch)
    off = _head(cfg, w, "fp32s", suppress_eos=sup)
    assert off.llm_batch_split_gemm == "library" and not off.llm_engine.batch_split_gemm
    assert bool(off.llm_engine._w16_all) == valued
    rb_off = off.llm_engine.resident_bytes()
    rq = off.run_relation_query(inputs["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]], names,
                                inputs["object_info"][0]["pan_results"])
    dec = off.decode_selected(rq, names)                                     # the single image's tokens, its own selection
    t1, sel = np.asarray(dec["tokens_host"]).copy(), [int(i) for i in dec["selected_host"]]
    K = t1.shape[0]
    assert 32 < 2 * K <= 160
    margins = _step_margins(off, dec, sup)
    _watch_head(calls, off)
    r_off, t_off, f_off = _batch(off, inputs)
    layer_shapes = set(_matrix_shapes(cfg.llm, False)[:4])
    assert not any(calls[n] or calls[n + "_head"] for n in ENTRIES), "the default must keep today's launches"
    assert layer_shapes <= set(calls["library"]) and calls["library_head"]
    for i, t in enumerate(t_off):
        _assert_tokens_agree(f"{case} valued={valued} option off, image {i}", t, t1, margins)
    ref = _oracle_first_logits((case, valued), w, cfg, scene, sel, sup)
    err_off = _oracle_distance(f_off, ref, K, 2)
    _free(off)

    on = _head(cfg, w, "fp32s", suppress_eos=sup, llm_batch_split_gemm="own")
    _watch_head(calls, on)
    assert on.llm_engine.batch_split_gemm and on.llm_engine.decode_uses_library(2 * K)        # (keeps its meaning)
    extra = 0 if valued else 4 * cfg.llm.vocab * cfg.llm.hidden + 4 * cfg.llm.vocab    # the lm_head's [wh | wl] image + scales
    rb_on = on.llm_engine.resident_bytes()
    assert rb_on["other"] - rb_off["other"] == extra and rb_on["quantised"] == rb_off["quantised"] == 0
    r_on, t_on, f_on = _batch(on, inputs)
    form = "w16" if valued else "w32"
    own = {sh for sh in layer_shapes if _batch_split_route(form, sh[0], sh[1], 2 * K) == "own"}
    assert len(own) >= 2 and all(not calls[n] and not calls[n + "_head"] for n in ENTRIES if n != entry)
    assert set(calls[entry]) & layer_shapes == own
    assert not own & set(calls["library"])
    # the lm_head follows the table like every other matrix: an fp16 value on its fp16 copy, a generic one on the packed
    # [wh | wl] image the option makes the engine keep (4 bytes per weight, under `other`)
    head_own = _batch_split_route(form, cfg.llm.vocab, cfg.llm.hidden, 2 * K) == "own"
    assert bool(calls[entry + "_head"]) == head_own and bool(calls["library_head"]) == (not head_own)
    assert (on.llm_engine.lm_head_mat.packed is None) == valued
    if not valued:
        assert tuple(on.llm_engine.lm_head_mat.packed[0].shape) == (cfg.llm.vocab, 2 * cfg.llm.hidden)
    err_on = _oracle_distance(f_on, ref, K, 2)
    print(f"{case} valued={valued}: first-step logits of a batch of 2 against the CPU oracle: option off {err_off:.3e}, "
          f"on {err_on:.3e} (bar {FP32S_ORACLE_BAR:.0e})")
    assert err_off < FP32S_ORACLE_BAR and err_on < FP32S_ORACLE_BAR
    for i, t in enumerate(t_on):
        _assert_tokens_agree(f"{case} valued={valued} option on, image {i}", t, t1, margins)
    assert [set(r) for r in r_on] == [set(r) for r in r_off]


def test_three_images_do_not_see_each_other(monkeypatch):
    """forward_batch([A, A, A]) at 60 rows: three identical token arrays (a row's slices depend on neither its neighbours
    nor their number), and the graph replay repeats them."""
    g, cfg, w, scene = H.load_case("G6_llm_7b_width_n6")
    head = _head(cfg, w, "fp32s", suppress_eos=bool(g["suppress_eos"]), llm_batch_split_gemm="own")
    calls = _spy(monkeypatch)
    res, toks, _ = _batch(head, _inputs(scene), n=3)
    assert calls["batch_split_gemm_w32"] and 3 * toks[0].shape[0] == 60
    assert np.array_equal(toks[0], toks[1]) and np.array_equal(toks[0], toks[2]) and res[0] == res[1] == res[2]
    res2, toks2, _ = _batch(head, _inputs(scene), n=3)
    assert res2 == res and all(np.array_equal(a, b) for a, b in zip(toks, toks2))


def test_a_quantised_matrix_follows_llm_batch_weight_stream_alone(monkeypatch):
    """An FP8-quantised fp32s head (the lm_head too) with llm_batch_weight_stream='quantised': with this option on as
    well, no matrix reaches the new entries, no image is made for the lm_head, and results, tokens and first-step logits are
    those of the head without it, bit for bit."""
    g, cfg, w, scene = _load("G8_gqa_512_n10")
    wq = _quantised(w, cfg, "fp8", True)
    kw = dict(suppress_eos=bool(g["suppress_eos"]), llm_weight_quant="fp8", llm_quantize_lm_head=True,
              llm_batch_weight_stream="quantised")
    inputs = _inputs(scene)
    ref = _head(cfg, wq, "fp32s", **kw)
    r0, t0, f0 = _batch(ref, inputs)
    _free(ref)
    calls = _spy(monkeypatch)
    head = _head(cfg, wq, "fp32s", llm_batch_split_gemm="own", **kw)
    _watch_head(calls, head)
    r1, t1, f1 = _batch(head, inputs)
    assert not any(calls[n] or calls[n + "_head"] for n in ENTRIES) and head.llm_engine.lm_head_mat.packed is None
    assert r1 == r0 and all(np.array_equal(a, b) for a, b in zip(t0, t1))
    assert torch.equal(f1.view(torch.int32), f0.view(torch.int32))
