"""Route digests of the LLM decode engine on one MI355X: for every engine configuration below, ONE whole head call on the
G1 golden case (2 decoder layers, 20 selected pairs; eager, `use_graph = False`) is recorded as
  * its launch trace - the ordered calls into `ops` and into torch.mm / torch.bmm / F.linear, a GEMM with the shape and
    dtype of its weight operand;
  * the SHA-256 of the generated tokens and of the first step's logits (the bytes the first greedy step reads);
  * the three totals of `resident_bytes()`.
A change of which kernel runs on which image of which matrix, of the bits it computes or of what the engine keeps in HBM
shows here.  Two trees that must route and compute alike are compared by running this file on both (it spies on `ops` and
calls the head by keyword only) and diffing the outputs:

    python tools/llm_route_digest.py [--out profiles/llm_route_digest.json] [--only NAME ...]
    python tools/llm_route_digest.py --compare A.json B.json
"""
from __future__ import annotations

import argparse
import gc
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASE = "G1_c1_512_n10"
LM_HEAD = "language_model.lm_head.weight"
F16, BF16, GENERIC = "fp16 values", "bf16 values", "neither"
QUERIES = ("_plan", "_supported", "_counters", "_workspace", "_workspace_bytes", "_version", "_error", "_candidates")


def _quant(fmt, lm_head=False, **kw):
    return dict(values=GENERIC, head=dict(llm_weight_quant=fmt, llm_quantize_lm_head=lm_head, **kw))


# name -> dtype, values of the LLM matrices, head keywords, images per call, engine switches, a set_projection + second call
CONFIGS = {
    "fp32s fp16-valued": dict(dtype="fp32s", values=F16),
    "fp32s generic": dict(dtype="fp32s", values=GENERIC),
    "fp32s bf16-valued stream": dict(dtype="fp32s", values=BF16, head=dict(llm_bf16_value_stream=True)),
    **{f"fp32s {fmt}{'+head' if h else ''}": dict(dtype="fp32s", **_quant(fmt, h))
       for fmt in ("fp8", "mxfp4", "int4g") for h in (False, True)},
    **{f"fp32s {fmt} resident": dict(dtype="fp32s", **_quant(fmt, llm_weight_resident="quantised")) for fmt in ("fp8", "mxfp4")},
    "fp32s generic row-invariant i2": dict(dtype="fp32s", values=GENERIC, options=dict(split_i2=1), row_invariant=True,
                                           set_projection=True),
    "fp32 fp16-valued": dict(dtype="fp32", values=F16),
    "fp32 generic": dict(dtype="fp32", values=GENERIC),
    "bf16": dict(dtype="bf16", values=GENERIC),
    **{f"bf16 {fmt}": dict(dtype="bf16", **_quant(fmt)) for fmt in ("fp8", "mxfp4", "int4g")},
    "bf16 fp8 resident": dict(dtype="bf16", **_quant("fp8", llm_weight_resident="quantised")),
    "mixed": dict(dtype="mixed", values=GENERIC),
    "batch bf16 fp8 stream": dict(dtype="bf16", images=2, **_quant("fp8", llm_batch_weight_stream="quantised")),
    "batch fp32s mxfp4 stream": dict(dtype="fp32s", images=2, **_quant("mxfp4", llm_batch_weight_stream="quantised")),
    "batch fp32s fp16-valued own": dict(dtype="fp32s", values=F16, images=2, head=dict(llm_batch_split_gemm="own")),
    "batch fp32s generic own": dict(dtype="fp32s", values=GENERIC, images=2, head=dict(llm_batch_split_gemm="own")),
}


def _valued(t, kind):
    """`t` as fp32 holding values of `kind`.  Element [0, 0] makes the kind unambiguous: 2^-30 is a bf16 value and no fp16
    value, 1 / 3 is neither."""
    t = torch.as_tensor(t).float().clone()
    if kind == F16:
        return t.half().float()
    if kind == BF16:
        t = t.bfloat16().float()
        t[0, 0] = 2.0 ** -30
        return t
    t[0, 0] = 1.0 / 3.0
    return t


def _weights(w, kind):
    out = dict(w)
    for k, v in w.items():
        if k.startswith("language_model.") and k.endswith("_proj.weight") or k == LM_HEAD:
            out[k] = _valued(v, kind)
    return out


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


class Spy:
    """Wraps every public function of `ops` that is not a host-side query, and torch.mm / torch.bmm / F.linear; while
    `on`, logs each call and keeps what the greedy steps read and write."""

    def __init__(self):
        import torch.nn.functional as F
        from openpsg_amd import ops
        self.ops, self.on, self.log, self.first_logits, self.tokens = ops, False, [], None, None
        self.saved = []
        names = [n for n, f in vars(ops).items() if not n.startswith("_") and callable(f) and not isinstance(f, type)
                 and getattr(f, "__module__", None) == ops.__name__ and not n.endswith(QUERIES)]
        for mod, name in [(ops, n) for n in names] + [(torch, "mm"), (torch, "bmm"), (F, "linear")]:
            self.saved.append((mod, name, getattr(mod, name)))
            setattr(mod, name, self._wrap(mod is ops, name, getattr(mod, name)))

    def restore(self):
        for mod, name, f in self.saved:
            setattr(mod, name, f)

    @staticmethod
    def _weight(own, name, a):
        """The weight operand of a GEMM call, else None."""
        if not own:
            return a[1]
        if "gemm" not in name:
            return None
        # (x2, inv_scale, weight, ...) for the two-plane entries, (kind, x_out, weight, ...) for the fused one, else (x, weight, ...)
        third = name.startswith(("split_gemm_", "batch_split_gemm_", "skinny_gemm_fused")) and name != "split_gemm_wb16"
        return a[2 if third else 1]

    def _wrap(self, own, name, f):
        def wrapped(*a, **kw):
            if self.on:
                w = self._weight(own, name, a)
                entry = name if own else "torch." + name
                if torch.is_tensor(w):
                    entry += f" {'x'.join(str(int(d)) for d in w.shape)} {str(w.dtype).replace('torch.', '')}"
                self.log.append(entry)
                if own and name in ("greedy_step", "trie_greedy_step"):
                    if self.first_logits is None:
                        lg = a[0].t if isinstance(a[0], self.ops.Partials) else a[0]
                        self.first_logits = _sha(lg)
                    self.tokens = a[6] if name == "trie_greedy_step" else a[5]
            return f(*a, **kw)
        return wrapped

    def record(self, call):
        self.log, self.first_logits, self.tokens, self.on = [], None, None, True
        try:
            call()
            torch.cuda.synchronize()
        finally:
            self.on = False
        entries = sorted(set(self.log))
        index = {e: i for i, e in enumerate(entries)}
        return dict(entries=entries, sequence=" ".join(str(index[e]) for e in self.log), calls=len(self.log),
                    trace_sha256=hashlib.sha256("\n".join(self.log).encode()).hexdigest(),
                    tokens_sha256=_sha(self.tokens), first_logits_sha256=self.first_logits)


def _run(name, c, spy, case):
    from openpsg_amd import _lib
    from openpsg_amd.head import RelationTransformerHeadV4
    g, cfg, w, scene = case
    old = {k: _lib.get_option(0, k) for k in c.get("options", {})}
    for k, v in c.get("options", {}).items():
        _lib.set_option(0, k, v)
    try:
        head = RelationTransformerHeadV4(dtype=c["dtype"], device="cuda:0", qformer_vocab_size=cfg.qformer.vocab,
                                         llm_config=cfg.llm, llm_feature_size=cfg.llm.hidden, tokenizers="word",
                                         max_object_num=cfg.max_object_num, on_parse_error="skip", suppress_eos=True,
                                         **c.get("head", {}))
        head.load_weights(_weights(w, c["values"]))
        eng = head.llm_engine
        eng.use_graph = False
        if c.get("row_invariant"):
            eng.row_invariant = True
        inputs = dict(mask_features=scene["mask_features"].cuda(), img_metas=[scene["img_meta"]],
                      object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"].cuda())])
        images = c.get("images", 1)
        call = (lambda: head(inputs)) if images == 1 else (lambda: head.forward_batch([inputs] * images))
        out = dict(call=spy.record(call))
        if c.get("set_projection"):
            # a projection of other values behind the first call: every image derived from the old one must go with it
            pw, pb = head.language_projection.weight.data, head.language_projection.bias.data
            eng.set_projection(pw.roll(1, 0) * 0.5, pb.roll(1, 0))
            out["call_after_set_projection"] = spy.record(call)
        out["resident_bytes"] = {k: int(v) for k, v in eng.resident_bytes().items() if k != "total"}
        return out
    finally:
        for k, v in old.items():
            _lib.set_option(0, k, v)


def digests(only=None):
    from tests import helpers as H
    case = H.load_case(CASE)
    assert case[1].llm.layers == 2
    spy, out = Spy(), {}
    try:
        for name, c in CONFIGS.items():
            if only and name not in only:
                continue
            out[name] = _run(name, c, spy, case)
            print(f"{name}: {out[name]['call']['calls']} calls", flush=True)
            gc.collect()
            torch.cuda.empty_cache()
    finally:
        spy.restore()
    return out


def compare(a, b):
    ca, cb = json.load(open(a))["cases"], json.load(open(b))["cases"]
    bad = sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))
    for k in bad:
        print("DIFFERENT", k)
    print(f"{len(ca)} / {len(cb)} cases, {len(bad)} different")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "llm_route_digest.json"))
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    res = dict(case=CASE, cases=digests(a.only))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print(f"wrote {a.out}: {len(res['cases'])} cases")


if __name__ == "__main__":
    main()
