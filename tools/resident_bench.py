"""What llm_weight_resident='quantised' costs and saves on one MI355X: BASELINE C3 (1024x1024, 50 objects,
top-20, 16 tokens, EOS suppressed) through head(inputs) with a 32-layer Llama-2-7B-shaped LLM, `fp32s` and `mixed`, FP8 and
MXFP4, 'all' against 'quantised' - the same seeded weights, one head at a time in the same process.

    python tools/resident_bench.py [--out profiles/resident_bench.json] [--steps 9] [--llm-layers 32] [--modes fp32s,mixed]
                                   [--quants fp8,mxfp4]

Per configuration: ms per image (median, min-max over --steps timed images after 3 warm-up images); for 'quantised' the
expansion launches of ONE prompt pass, each timed with events in the order and on the matrices the pass runs them (eager,
every matrix read cold from HBM as in the pass: 32 layers of bytes do not fit the Infinity Cache), their sum, the sum as a
share of the prompt pass (the eager prompt pass of the same image, event-timed) and against the model of DESIGN 8.1
(6 us + bytes / 6.4 TB/s per launch); `resident_bytes()`; the allocator's figures after the load and at the peak.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _events_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def _expansions(eng, reps):
    """Summed time of the expansion launches of one prompt pass (ms: median, min, max over reps), the bytes they move and
    the model's time for them.  The pass expands q|k|v, o, gate|up, down of every layer (+ nothing for the lm_head: 20 rows)."""
    unscaled = eng.prefill_split                                       # fp32s: the exact fp16 image; 16-bit engines: W'
    mats = [L[k] for L in eng.layers for k in ("wqkv", "wo", "wgu", "wdown")]
    out_bytes = 2
    moved = sum(w.q.numel() + (w.e.numel() if w.e is not None else 0) + w.numel() * out_bytes for w in mats)
    model_ms = sum(6e-3 + (w.q.numel() + w.numel() * out_bytes) / 6.4e9 for w in mats)

    def one_pass():
        for w in mats:
            eng._dense(w, unscaled=unscaled)
    one_pass()
    ts = _events_ms(one_pass, reps)
    return dict(launches=len(mats), bytes_moved=moved, model_ms=round(model_ms, 3), ms_median=round(statistics.median(ts), 3),
                ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))


def _prompt_pass_ms(head, inputs, reps):
    """The eager prompt pass (+ first token) of the image's selected pairs, event-timed."""
    feat, meta, info, obj_ids, names = head._unpack(inputs)
    rq = head.run_relation_query(feat, meta, obj_ids, names, info["pan_results"])
    X, plen = head.llm_inputs(rq, names)
    eng = head.llm_engine

    def run():
        with torch.no_grad():
            eng._prefill(X, plen, 1, True, False)
    run()
    ts = _events_ms(run, reps)
    return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))


def bench(mode, quant, resident, steps, layers):
    from openpsg_amd.config import LlamaConfig, PSGConfig, QFormerConfig
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_device
    dev = torch.device("cuda", 0)
    scene = make_scene((1024, 1024), 50, seed=0, device=str(dev))
    inputs = dict(mask_features=scene["mask_features"], img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"])])
    llm = LlamaConfig(layers=layers)
    cfg = PSGConfig(qformer=QFormerConfig(), llm=llm, max_object_num=50)
    gc.collect()
    torch.cuda.empty_cache()
    # (the seeded weights are drawn on the device, in fp16, and freed after the load: they are the caller's, not the head's)
    w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float16)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    h = RelationTransformerHeadV4(dtype=mode, device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                  on_parse_error="skip", suppress_eos=True, llm_weight_quant=quant,
                                  llm_weight_resident=resident)
    h.load_weights(w)
    torch.cuda.synchronize()
    load_peak = torch.cuda.max_memory_allocated() - base
    del w
    gc.collect()
    torch.cuda.empty_cache()
    after_load = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(3):                                                 # warm-up: graphs, prompt tables, library plans
        h(inputs)
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h(inputs)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    eng = h.llm_engine
    r = dict(mode=mode, llm_weight_quant=quant, llm_weight_resident=resident, layers=layers,
             ms_per_image_median=round(statistics.median(times), 2), ms_per_image_min=round(min(times), 2),
             ms_per_image_max=round(max(times), 2), ms_per_image_all=[round(t, 2) for t in times],
             resident_bytes=eng.resident_bytes(),
             allocator=dict(allocated_after_load=after_load, load_peak_above_start=load_peak,
                            max_allocated_running=torch.cuda.max_memory_allocated(), reserved=torch.cuda.memory_reserved()))
    r["prompt_pass"] = _prompt_pass_ms(h, inputs, 5)
    if resident == "quantised":
        r["expansions"] = _expansions(eng, 7)
        r["expansions"]["share_of_prompt_pass"] = round(r["expansions"]["ms_median"] / r["prompt_pass"]["ms_median"], 4)
        r["expansions"]["over_model"] = round(r["expansions"]["ms_median"] / r["expansions"]["model_ms"], 3)
    print("image", json.dumps(r), flush=True)
    del h, eng
    gc.collect()
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resident_bench.json"))
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--modes", default="fp32s,mixed")
    ap.add_argument("--quants", default="fp8,mxfp4")
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), workload="BASELINE C3, EOS suppressed", image_c3=[])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for mode in a.modes.split(","):
        for quant in a.quants.split(","):
            for resident in ("all", "quantised"):
                res["image_c3"].append(bench(mode, quant, resident, a.steps, a.llm_layers))
                json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
