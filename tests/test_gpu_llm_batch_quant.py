"""llm_batch_weight_stream='quantised' through the whole head (`-m gpu`): forward_batch's decode steps of 33..160
rows on the byte / nibble streams of psg_batch_gemm_q.hip.  The option changes which kernel computes a projection of the
SAME model W', so a head with it is held to what the option-off forward_batch is held to - each image's tokens agree with
that image's single-image decode up to each pair's first near-tie - in the same test, on the same inputs, next to the
option-off head; and to equality where equality is due: between the images of one batch, between a batch and its graph
replay, and between llm_weight_resident='quantised' and 'all' (which now run the same launches on the same bytes)."""
import gc

import numpy as np
import pytest
import torch

from openpsg_amd.llm import _batch_quant_route
from tests import helpers as H
from tests.test_gpu_llm_resident import _inputs, _matrix_shapes, _quantised
from tests.test_gpu_llm_w8 import _assert_tokens_agree, _head, _step_margins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ("batch_gemm_w8", "batch_split_gemm_w8", "batch_gemm_w4", "batch_split_gemm_w4")


def _load(case):
    if case.startswith("G8"):
        from tests.test_gpu_gqa_head import load_gqa_case
        return load_gqa_case(case)
    return H.load_case(case)


def _spy(monkeypatch):
    """Calls of the four new entries and of ops.batch_gemm by weight shape (N, K); expansions counted while a decode step
    runs (`LlamaDecodeEngine._steps`: the prompt pass is over by then)."""
    from openpsg_amd import ops
    from openpsg_amd.llm import LlamaDecodeEngine
    calls = {n: [] for n in ENTRIES + ("batch_gemm",)}
    calls["expand_in_steps"] = 0
    state = {"in_steps": False}

    def shape_of(name, a):
        w = a[2] if "split" in name else a[1]
        return (int(w.shape[0]), int(w.shape[1]) * (2 if name.endswith("w4") else 1))
    for fn in ENTRIES + ("batch_gemm",):
        def wrapped(*a, _f=getattr(ops, fn), _n=fn, **kw):
            calls[_n].append(shape_of(_n, a))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrapped)
    for fn in ("expand_w8", "expand_w4"):
        def wrapped(*a, _f=getattr(ops, fn), **kw):
            calls["expand_in_steps"] += int(state["in_steps"])
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn, wrapped)

    def steps(self, *a, _f=LlamaDecodeEngine._steps, **kw):
        state["in_steps"] = True
        try:
            return _f(self, *a, **kw)
        finally:
            state["in_steps"] = False
    monkeypatch.setattr(LlamaDecodeEngine, "_steps", steps)
    return calls


def _step_margins_f32(head, dec, suppress):
    """`tests.test_gpu_llm_w8._step_margins` for a 16-bit head, over the logits its greedy step compares: the same
    teacher-forced forward of its engine over [prompt, generated tokens], the lm_head product with an fp32 result
    (`_lm_head_f32`) instead of one rounded to the activation dtype.  [K, T] on the host; steps behind an EOS: inf."""
    from openpsg_amd import ops
    eng = head.llm_engine
    m = head.cfg.llm
    X, plen = dec["llm_inputs"], dec["prompt_len"].to(torch.int64)
    toks = torch.as_tensor(np.asarray(dec["tokens_host"])).to(DEV).long()
    K, T = toks.shape
    n = plen + head.cfg.qformer.num_query
    S = X.shape[1] + T - 1
    Xe = torch.zeros((K, S, X.shape[2]), device=DEV, dtype=X.dtype)
    rows = []
    for k in range(K):
        nk = int(n[k])
        Xe[k, :nk] = X[k, :nk]
        Xe[k, nk:nk + T - 1] = eng.embed[toks[k, :T - 1].clamp(min=0)]
        rows += [k * S + nk - 1 + s for s in range(T)]
    seq_len = (n + T - 1).to(torch.int32)
    t = torch.arange(S, device=DEV, dtype=torch.int32)[None, :].expand(K, -1)
    tok_pos = torch.where(t < seq_len[:, None], t, torch.full_like(t, -1)).reshape(-1).contiguous()
    tok_pair = torch.arange(K, device=DEV, dtype=torch.int32)[:, None].expand(-1, S).reshape(-1).contiguous()
    kc = [torch.empty((K, m.n_kv_heads, S, m.head_dim), device=DEV, dtype=eng.dtype) for _ in eng.layers]
    vc = [torch.empty((K, m.n_kv_heads, S, m.head_dim), device=DEV, dtype=eng.dtype) for _ in eng.layers]
    with torch.no_grad():
        h = eng._forward(Xe.reshape(K * S, -1).to(eng.resid_dtype, copy=True), tok_pair, tok_pos, kc, vc, S,
                         rope_pos=torch.arange(S, device=DEV, dtype=torch.int32).repeat(K).contiguous())
        h_rows = torch.empty((len(rows), h.shape[1]), device=DEV, dtype=eng.dtype)
        ops.gather_rows(h, torch.tensor(rows, device=DEV, dtype=torch.int32), h_rows)
        lg = eng._lm_head_f32(h_rows)
    assert lg.dtype == torch.float32
    if suppress:
        lg[:, m.eos] = -float("inf")
    top = lg.topk(2, dim=-1).values
    margin = (top[:, 0] - top[:, 1]).view(K, T)
    return torch.where(toks >= 0, margin, torch.full_like(margin, float("inf"))).cpu().numpy()


def _batch(head, inputs, n=2):
    """forward_batch of n copies of `inputs`: (results, per-image tokens, first-step logits [n K, vocab] on the host)."""
    eng, got = head.llm_engine, []
    orig = eng.generate

    def generate(*a, **kw):
        kw["return_first_logits"] = True
        toks, fl = orig(*a, **kw)
        got.append(fl.float().cpu())
        return toks
    eng.generate = generate
    try:
        res = head.forward_batch([inputs] * n)
    finally:
        del eng.generate
    assert len(res) == n and len(head.last_batch) == n
    return res, [np.asarray(lb["tokens_host"]).copy() for lb in head.last_batch], got[0]


def _free(*heads):
    del heads
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case,dtype,fmt,lm_head,entry", [
    ("G1_c1_512_n10", "mixed", "fp8", False, "batch_gemm_w8"),
    ("G6_llm_7b_width_n6", "fp32s", "fp8", False, "batch_split_gemm_w8"),
    ("G8_gqa_512_n10", "fp32s", "mxfp4", True, "batch_split_gemm_w4"),
    ("G1_c1_512_n10", "bf16", "mxfp4", False, "batch_gemm_w4"),
])
def test_two_images_stream_the_bytes_and_agree_with_the_single_image_decode(case, dtype, fmt, lm_head, entry, monkeypatch):
    """Option off: no new entry is called.  Option on: every decoder projection of the 40-row steps that the routing table
    does not list goes through `entry` and none of them through ops.batch_gemm.  Both batches agree with the single-image tokens up to each pair's first near-tie (>= 90 %
    of the entries compared; bf16: margins of the fp32 logits its argmax sees, `_step_margins_f32`), and the option-on
    batch's first-step logits are within twice the option-off batch's distance from the single-image decode's."""
    g, cfg, w, scene = _load(case)
    sup = bool(g["suppress_eos"])
    wq = _quantised(w, cfg, fmt, lm_head)
    kw = dict(suppress_eos=sup, llm_weight_quant=fmt, llm_quantize_lm_head=lm_head)
    inputs, names = _inputs(scene), H.object_names(scene)
    calls = _spy(monkeypatch)
    off = _head(cfg, wq, dtype, **kw)
    assert off.llm_batch_weight_stream == "dense" and not off.llm_engine.batch_quant_stream
    rq = off.run_relation_query(inputs["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]], names,
                                inputs["object_info"][0]["pan_results"])
    dec = off.decode_selected(rq, names)                                     # the single image's tokens, its own selection
    t1, f1 = np.asarray(dec["tokens_host"]).copy(), dec["first_logits"].float().cpu()
    K = t1.shape[0]
    # a 16-bit head's greedy step takes the argmax of the fp32 lm_head sums (`exact_argmax`), so the margins that decide its
    # tokens are fp32 ones; `_step_margins` reads the teacher-forced logits ROUNDED to the head's dtype, which in bf16
    # (spacing 2^-4 at |x| in 8..16) turns a quarter of them into exact ties
    margins = _step_margins(off, dec, sup) if dtype != "bf16" else _step_margins_f32(off, dec, sup)
    r_off, t_off, f_off = _batch(off, inputs)
    assert not any(calls[n] for n in ENTRIES), "the default must keep today's launches"
    err_off = max((f_off[i * K:(i + 1) * K] - f1).abs().max().item() for i in range(2))
    for i, t in enumerate(t_off):
        _assert_tokens_agree(f"{case} {dtype} {fmt} option off, image {i}", t, t1, margins)
    _free(off)
    calls["batch_gemm"].clear()
    on = _head(cfg, wq, dtype, llm_batch_weight_stream="quantised", **kw)
    assert on.llm_engine.batch_quant_stream and on.llm_engine.decode_uses_library(2 * K)      # (keeps its meaning)
    r_on, t_on, f_on = _batch(on, inputs)
    # what streams is what the fixed routing table leaves (G6 has Llama-2-7B's width: `o` in the fp8 pair form at 40 rows is a
    # listed loser and must NOT stream; the small models' shapes are not listed), through `entry` and nothing else
    form = "pair" if dtype == "fp32s" else "single"
    layer_shapes = set(_matrix_shapes(cfg.llm, False)[:4])
    streams = {sh for sh in layer_shapes if _batch_quant_route(fmt, form, sh[0], sh[1], 2 * K) == "stream"}
    assert len(streams) >= 3 and all(not calls[n] for n in ENTRIES if n != entry)
    assert set(calls[entry]) & layer_shapes == streams
    assert not streams & set(calls["batch_gemm"])
    assert ((cfg.llm.vocab, cfg.llm.hidden) in calls[entry]) == bool(lm_head)        # the lm_head follows its tensor's stream
    err_on = max((f_on[i * K:(i + 1) * K] - f1).abs().max().item() for i in range(2))
    print(f"{case} {dtype} {fmt}: first-step logits, batch of 2 vs single image: option off {err_off:.3e}, on {err_on:.3e}")
    assert err_on <= 2.0 * err_off
    for i, t in enumerate(t_on):
        _assert_tokens_agree(f"{case} {dtype} {fmt} option on, image {i}", t, t1, margins)
    assert [set(r) for r in r_on] == [set(r) for r in r_off]


def test_three_images_do_not_see_each_other(monkeypatch):
    """forward_batch([A, A, A]) at 60 rows: three identical token arrays (a row's slices depend on neither its neighbours
    nor their number), and the graph replay repeats them."""
    g, cfg, w, scene = H.load_case("G1_c1_512_n10")
    head = _head(cfg, _quantised(w, cfg, "fp8"), "mixed", suppress_eos=bool(g["suppress_eos"]), llm_weight_quant="fp8",
                 llm_batch_weight_stream="quantised")
    calls = _spy(monkeypatch)
    res, toks, _ = _batch(head, _inputs(scene), n=3)
    assert calls["batch_gemm_w8"] and 32 < 3 * toks[0].shape[0] <= 160
    assert np.array_equal(toks[0], toks[1]) and np.array_equal(toks[0], toks[2]) and res[0] == res[1] == res[2]
    res2, toks2, _ = _batch(head, _inputs(scene), n=3)
    assert res2 == res and all(np.array_equal(a, b) for a, b in zip(toks, toks2))


@pytest.mark.parametrize("case,dtype,fmt,lm_head", [("G1_c1_512_n10", "mixed", "fp8", False),
                                                    ("G8_gqa_512_n10", "fp32s", "mxfp4", True)])
def test_bytes_only_residency_equals_all_and_never_expands_in_a_decode_step(case, dtype, fmt, lm_head, monkeypatch):
    """With the option on, llm_weight_resident='quantised' and 'all' run the same launches on the same bytes in every decode
    step: results, tokens and first-step logits equal bit for bit, no expansion after the prompt pass, and the footprint
    `resident_bytes()` reports is the option-off lean head's."""
    g, cfg, w, scene = _load(case)
    wq = _quantised(w, cfg, fmt, lm_head)
    kw = dict(suppress_eos=bool(g["suppress_eos"]), llm_weight_quant=fmt, llm_quantize_lm_head=lm_head)
    inputs = _inputs(scene)
    ref = _head(cfg, wq, dtype, llm_batch_weight_stream="quantised", **kw)
    r0, t0, f0 = _batch(ref, inputs)
    _free(ref)
    lean_off = _head(cfg, wq, dtype, llm_weight_resident="quantised", **kw)
    rb_off = lean_off.llm_engine.resident_bytes()
    _free(lean_off)
    calls = _spy(monkeypatch)
    lean = _head(cfg, wq, dtype, llm_weight_resident="quantised", llm_batch_weight_stream="quantised", **kw)
    assert lean.llm_engine.resident_bytes() == rb_off
    for run in range(2):                                                     # capture, then replay
        r1, t1, f1 = _batch(lean, inputs)
        assert r1 == r0 and all(np.array_equal(a, b) for a, b in zip(t0, t1)), f"run {run}: tokens differ"
        assert torch.equal(f1.view(torch.int32), f0.view(torch.int32)), f"run {run}: first-step logits differ"
    assert calls["expand_in_steps"] == 0 and any(calls[n] for n in ENTRIES)
    assert lean.llm_engine.resident_bytes() == rb_off


def test_a_matrix_the_kernels_refuse_keeps_the_dense_path(monkeypatch):
    """A down projection with K = 160 (no multiple of 128) under fp8: `engine.linear` returns what the option-off engine
    returns for it instead of raising, while the matrices that fit stream; forward_batch of two images runs."""
    from openpsg_amd import ops
    from openpsg_amd.synthetic import make_scene
    from tests.test_gpu_llm_resident import _tiny
    cfg, w = _tiny(inter=160)
    head = _head(cfg, w, "mixed", suppress_eos=True, llm_weight_quant="fp8", llm_batch_weight_stream="quantised")
    eng = head.llm_engine
    L = eng.mats[0]
    calls = _spy(monkeypatch)
    xd = torch.randn(40, 160, device=DEV).to(eng.dtype)
    y_on = eng.linear(xd, L["wdown"], decode=True)
    assert not calls["batch_gemm_w8"]
    xq = torch.randn(40, 256, device=DEV).to(eng.dtype)
    q_on = eng.linear(xq, L["wqkv"], decode=True)
    assert calls["batch_gemm_w8"] == [(768, 256)]
    eng.batch_quant_stream = False
    y_off = eng.linear(xd, L["wdown"], decode=True)
    eng.batch_quant_stream = True
    raw = lambda y: y.t if isinstance(y, ops.Partials) else y                # noqa: E731
    assert type(y_on) is type(y_off) and torch.equal(raw(y_on), raw(y_off))
    q, s = L["wqkv"].q, L["wqkv"].s
    wd = q.view(torch.float8_e4m3fn).double() * s.double()[:, None]
    assert ((q_on.t.sum(0).double() - xq.double() @ wd.t()).abs() <= 2.0 ** -20 * (xq.double().abs() @ wd.abs().t())).all()
    scene = make_scene((512, 512), 6, seed=3, device=DEV)
    inputs = dict(mask_features=scene["mask_features"], img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"])])
    res = head.forward_batch([inputs, inputs])
    assert len(res) == 2 and (256, 160) not in calls["batch_gemm_w8"] and (320, 256) in calls["batch_gemm_w8"]
