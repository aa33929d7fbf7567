"""llm_bf16_value_stream through the whole head (`-m gpu`): an fp32s head whose LLM matrices are bf16 VALUES
streams bf16 copies in the decode steps (psg_split_gemm_wb16).  The option changes which kernel computes a projection of
the same weights from the same fp32 rows - exactly split - so the head with it is held to the option-off head on the
same inputs: step logits within 1e-4 from one and the same post-prefill state (the bar tests/test_gpu_w16.py sets for the
fp16 stream on G6), and tokens EQUAL (no near-tie fall-back: none of the three cases needed one).

Cases: G6 (Llama-2-7B width, 2 layers, 20 pairs), G8 (grouped-query) and the small LLM of tests/test_gpu_w16.py
(512 / 1024 / 512), the LLM's matrices rounded through bf16.

Measured on an MI355X (step-logit distance; tokens): G6 1.05e-5, G8 6.7e-6, small 5.2e-6; equal in all three."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import llm_matrix_ref as M
from tests.test_gpu_llm_batch_quant import _free, _load
from tests.test_gpu_llm_resident import _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_BAR = 1e-4
NEW_OPS = ("split_gemm_wb16", "split_b16x3", "rmsnorm_split_b16x3", "silu_mul_split_b16x3")
OLD_OPS = ("skinny_gemm", "skinny_gemm_w16", "split_gemm_w16", "split_f16x2", "rmsnorm_split2", "rmsnorm", "silu_mul",
           "decode_attn", "decode_layers", "greedy_step", "trie_greedy_step")
CASES = ("G6_llm_7b_width_n6", "G8_gqa_512_n10", "small")


def _valued(w, dtype):
    """Every LLM matrix rounded to a value of `dtype`: what from_pretrained yields from a checkpoint stored in it."""
    return {k: (torch.as_tensor(v).to(dtype).float() if k.startswith("language_model.") and torch.as_tensor(v).dim() >= 2 else v)
            for k, v in w.items()}


def _case(name):
    """(cfg, generic fp32 weights, scene, suppress_eos, the golden's selection or None)"""
    if name == "small":
        from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
        from openpsg_amd.synthetic import make_scene
        from openpsg_amd.weights import make_weights_device
        cfg = PSGConfig(qformer=QFormerConfig(vocab=30522), llm=tiny_llm(512, 2, 1024, 512), max_object_num=50)
        return cfg, make_weights_device(cfg, 7, torch.device(DEV), llm_dtype=torch.float32), \
            make_scene((512, 768), 12, seed=4, device=DEV), True, None
    g, cfg, w, scene = _load(name)
    return cfg, w, scene, bool(g["suppress_eos"]), g["selected"].astype(np.int32)


def _head(cfg, w, **kw):
    from openpsg_amd.head import RelationTransformerHeadV4
    h = RelationTransformerHeadV4(dtype="fp32s", device=DEV, qformer_vocab_size=cfg.qformer.vocab, llm_config=cfg.llm,
                                  llm_feature_size=cfg.llm.hidden, tokenizers="word", max_object_num=cfg.max_object_num,
                                  on_parse_error="skip", **kw)
    h.load_weights(w)
    return h


def _decode(head, scene, sel):
    dev = torch.device(DEV)
    names = H.object_names(scene)
    rq = head.run_relation_query(scene["mask_features"].to(dev), scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                                 names, scene["pan_results"].to(dev))
    selected = None if sel is None else torch.from_numpy(sel).to(dev)
    dec = head.decode_selected(rq, names, selected=selected)
    dec2 = head.decode_selected(rq, names, selected=selected)                # graph replay == first run
    assert np.array_equal(dec["tokens_host"], dec2["tokens_host"])
    return dec


class _Spy:
    """The ops a decode step (`LlamaDecodeEngine._steps`: the prompt pass is over by then) calls, in order; a projection
    entry as (name, its weight's shape, its weight's address)."""

    def __init__(self):
        from openpsg_amd import llm, ops
        self.ops, self.llm, self.saved, self.log, self.depth = ops, llm, {}, [], 0
        for name in NEW_OPS + OLD_OPS:
            self.saved[name] = getattr(ops, name)
            setattr(ops, name, self._wrap(name, self.saved[name]))
        self.steps = llm.LlamaDecodeEngine._steps
        spy = self

        def steps(eng, *a, **kw):
            spy.depth += 1
            try:
                return spy.steps(eng, *a, **kw)
            finally:
                spy.depth -= 1
        llm.LlamaDecodeEngine._steps = steps

    def _wrap(self, name, f):
        def wrapped(*a, **kw):
            if self.depth:
                w = a[1] if name in ("split_gemm_wb16", "skinny_gemm", "skinny_gemm_w16") else a[2] if name == "split_gemm_w16" else None
                self.log.append(name if w is None else (name, tuple(w.shape), w.data_ptr()))
            return f(*a, **kw)
        return wrapped

    def take(self):
        out, self.log = self.log, []
        return out

    def close(self):
        for name, f in self.saved.items():
            setattr(self.ops, name, f)
        self.llm.LlamaDecodeEngine._steps = self.steps


@pytest.fixture
def spy():
    s = _Spy()
    try:
        yield s
    finally:
        s.close()


def _names(log):
    return [e if isinstance(e, str) else e[0] for e in log]


def _step_logits(eng, dec, sup):
    """One decode step from ONE post-prefill state on both routes: (`_decode_step_split` on 'wb16', the option-off chain) fp32 logits."""
    st = eng._prefill(dec["llm_inputs"], dec["prompt_len"], eng.cfg.max_new_tokens, sup, False)
    x0 = st["x"].clone()                                                     # (a step adds its deltas to the residual rows)
    a = eng._decode_step_split(st, "wb16").reduce(torch.float32)
    st["x"].copy_(x0)
    h = eng._forward(st["x"], st["dec_pair"], st["dec_pos"], st["kc"], st["vc"], st["ctx_len"], decode=True)
    b = eng.logits(h)
    b = b.reduce(torch.float32) if hasattr(b, "reduce") else b.float()
    torch.cuda.synchronize()
    return a, b


@pytest.mark.parametrize("case", CASES)
def test_the_option_routes_the_decode_steps_and_keeps_the_tokens(case, spy):
    cfg, w, scene, sup, sel = _case(case)
    wb = _valued(w, torch.bfloat16)
    shapes = {(cfg.llm.hidden + 2 * cfg.llm.kv_dim, cfg.llm.hidden), (cfg.llm.hidden, cfg.llm.hidden),
              (2 * cfg.llm.inter, cfg.llm.hidden), (cfg.llm.hidden, cfg.llm.inter)}
    # a head built without the keyword, and one with the option spelled off: the same launches, the same bits
    plain = _head(cfg, wb, suppress_eos=sup)
    assert not plain.llm_engine._w16_all, "a bf16-valued model must fail the fp16 round trip"
    d_plain = _decode(plain, scene, sel)
    t_plain, f_plain = np.asarray(d_plain["tokens_host"]).copy(), d_plain["first_logits"].clone()
    log_plain = spy.take()
    rb_plain = plain.llm_engine.resident_bytes()
    _free(plain, d_plain)
    off = _head(cfg, wb, suppress_eos=sup, llm_bf16_value_stream=False)
    assert not off.llm_engine.bf16_stream_active and "wb16" not in M.streams(off.llm_engine)
    d_off = _decode(off, scene, sel)
    t_off = np.asarray(d_off["tokens_host"]).copy()
    assert np.array_equal(t_off, t_plain) and torch.equal(d_off["first_logits"], f_plain)
    log_off = spy.take()
    strip = lambda log: [e if isinstance(e, str) else e[:2] for e in log]    # noqa: E731  (addresses differ between heads)
    assert strip(log_off) == strip(log_plain) and not set(_names(log_off)) & set(NEW_OPS), "option off: no new op may be called"
    assert off.llm_engine.resident_bytes() == rb_plain
    _free(off)

    on = _head(cfg, wb, suppress_eos=sup, llm_bf16_value_stream=True)
    eng = on.llm_engine
    assert eng.bf16_stream_active and M.streams(eng).count("wb16") == 4 * len(eng.layers) + 1 and not eng.decode_uses_library(20)
    copies = sum(rec.wb16.numel() for rec in eng.matrices())
    rb_on = eng.resident_bytes()
    assert rb_on["other"] - rb_plain["other"] == 2 * copies and rb_on["quantised"] == 0      # 2 bytes per weight
    d_on = _decode(on, scene, sel)
    t_on = np.asarray(d_on["tokens_host"]).copy()
    log_on = spy.take()
    # every decoder projection (and this model's lm_head) of a decode step through psg_split_gemm_wb16: none through the
    # fp32 skinny kernel, the persistent layer or the fp16 stream
    assert {e[1] for e in log_on if e[0] == "split_gemm_wb16"} == shapes | {(cfg.llm.vocab, cfg.llm.hidden)}
    assert not {"skinny_gemm", "skinny_gemm_w16", "split_gemm_w16", "decode_layers", "split_f16x2", "rmsnorm_split2",
                "rmsnorm", "silu_mul"} & set(_names(log_on))
    per_step = ["rmsnorm_split_b16x3"]
    for _ in eng.layers:
        per_step += ["split_gemm_wb16", "decode_attn", "split_b16x3", "split_gemm_wb16", "rmsnorm_split_b16x3",
                     "split_gemm_wb16", "silu_mul_split_b16x3", "split_gemm_wb16", "rmsnorm_split_b16x3"]
    per_step += ["split_gemm_wb16", "greedy_step"]
    n = len(per_step)
    assert len(log_on) % n == 0 and all(_names(log_on[i:i + n]) == per_step for i in range(0, len(log_on), n))
    assert torch.equal(d_on["first_logits"], f_plain), "the prompt pass must not change"
    # one step on both routes from one and the same post-prefill state
    a, b = _step_logits(eng, d_on, sup)
    dist = (a - b).abs().max().item()
    equal = np.array_equal(t_on, t_off)
    print(f"{case}: step logits, bf16 stream against the option-off chain: {dist:.3e} (bar {STEP_BAR:.0e}); tokens "
          f"{'equal' if equal else 'differ'}")
    assert dist < STEP_BAR
    assert equal, f"{case}: tokens differ between the bf16 stream and the option-off head"


def test_forward_submit_replay_and_the_constrained_decode_agree(spy):
    cfg, w, scene, sup, _ = _case("G8_gqa_512_n10")
    wb = _valued(w, torch.bfloat16)
    inp = _inputs(scene)
    head = _head(cfg, wb, suppress_eos=sup, llm_bf16_value_stream=True)
    assert head.llm_engine.bf16_stream_active
    r = head(inp)
    assert head(inp) == r                                         # graph replay == first run
    assert head.submit(inp).result() == r
    p0, p1 = head.submit(inp, slot=0), head.submit(inp, slot=1)
    assert p1.result() == r and p0.result() == r
    _free(head)
    con = _head(cfg, wb, llm_decode="constrained", llm_bf16_value_stream=True)
    assert con.llm_engine.bf16_stream_active
    spy.take()
    rc = con(inp)
    names = _names(spy.take())                                    # trie_greedy_step stays the LAST launch of a step
    ends = [i for i, n in enumerate(names) if n == "trie_greedy_step"]
    assert ends and "greedy_step" not in names and names[-1] == "trie_greedy_step"
    assert all(names[i - 1] == "split_gemm_wb16" for i in ends)
    assert all(names[i + 1] == "rmsnorm_split_b16x3" for i in ends[:-1])
    sel, N = con.last["selected_host"], len(scene["object_id_list"])
    K = len(sel)
    assert len(rc["rel_pred"]) == K                               # one valid triple per selected pair, in selection order
    trie = con.relation_trie()
    for k, (s, o, rel) in enumerate(rc["rel_pred"]):
        assert (s, o) == (int(sel[k]) // N, int(sel[k]) % N)
        assert [int(t) for t in np.asarray(con.last["tokens_host"])[k] if t >= 0] == trie.candidates[rel]
    assert con(inp) == rc


def test_mixed_generic_and_fp16_valued_weights(spy):
    cfg, w, scene, sup, sel = _case("small")
    wb = _valued(w, torch.bfloat16)
    # an fp32 fine-tuned lm_head keeps its fp32 stream while the decoder layers take the route; the tokens are those of the
    # option-off head on the same weights
    wm = dict(wb)
    wm["language_model.lm_head.weight"] = torch.as_tensor(w["language_model.lm_head.weight"]).clone()
    off = _head(cfg, wm, suppress_eos=sup)
    t_off = np.asarray(_decode(off, scene, sel)["tokens_host"]).copy()
    spy.take()
    _free(off)
    on = _head(cfg, wm, suppress_eos=sup, llm_bf16_value_stream=True)
    eng = on.llm_engine
    assert eng.bf16_stream_active and M.streams(eng).count("wb16") == 4 * len(eng.layers) and eng.lm_head_mat.wb16 is None
    t_on = np.asarray(_decode(on, scene, sel)["tokens_host"]).copy()
    log = spy.take()
    head_ptr = eng.lm_head.data_ptr()                             # (this model's lm_head has the output projection's shape)
    assert {e[0] for e in log if not isinstance(e, str) and e[2] == head_ptr} == {"skinny_gemm"}
    assert {e[0] for e in log if not isinstance(e, str) and e[2] != head_ptr} == {"split_gemm_wb16"}
    assert np.array_equal(t_on, t_off)
    _free(on)
    # generic fp32 weights: nothing to narrow - the option-off head's launches
    logs = {}
    for flag in (False, True):
        h = _head(cfg, w, suppress_eos=sup, llm_bf16_value_stream=flag)
        assert not h.llm_engine.bf16_stream_active and "wb16" not in M.streams(h.llm_engine)
        logs[flag] = (np.asarray(_decode(h, scene, sel)["tokens_host"]).copy(), spy.take())
        _free(h)
    strip = lambda log: [e if isinstance(e, str) else e[:2] for e in log]    # noqa: E731  (addresses differ between heads)
    assert strip(logs[True][1]) == strip(logs[False][1]) and np.array_equal(logs[True][0], logs[False][0])
    assert not set(_names(logs[True][1])) & set(NEW_OPS)
    # fp16-valued weights still take the fp16 stream
    h = _head(cfg, _valued(w, torch.float16), suppress_eos=sup, llm_bf16_value_stream=True)
    assert h.llm_engine._w16_all and "wb16" not in M.streams(h.llm_engine) and not h.llm_engine.bf16_stream_active
    _decode(h, scene, sel)
    names = set(_names(spy.take()))
    assert "split_gemm_w16" in names and not names & set(NEW_OPS)
