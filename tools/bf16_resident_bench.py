"""Timings and memory of llm_bf16_value_resident on one MI355X:

  per launch    40 / 80 / 160 rows at the Llama-2-7B shapes (q|k|v, o, gate|up, down, lm_head) over bf16-valued weights:
                  own        psg_split_b16x3 + psg_batch_split_gemm_wb16 on the bf16 copy
                  yardstick  what the mode runs otherwise on the same copy: psg_split_b16x3 + the stacked-plane library
                             product (planes flipped to [x2; x1; x0], one torch.mm of 3 x rows bf16 rows, fp32 result)
                  for information, the parent's routes for the same step on the same values: psg_split_f16x2 +
                  psg_batch_split_gemm_w32 on the [wh | wl | wh] image, and F.linear on fp32 W (the library SGEMM).
                Every side hands its consumer fp32 slices or a dense result as the engine does; the acceptance rule of
                DESIGN 12 / 16 / 18 decides `llm._BATCH_WB16_LIBRARY`: a (shape, rows) whose range of times does not lie wholly
                below the yardstick's goes into the table.
  whole image   BASELINE C3 (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed), 32-layer Llama-2-7B-shaped LLM,
                seeded bf16-valued weights: llm_bf16_value_stream=True with resident off against on, two heads in one
                process, 2 warm-up images and `--image-steps` timed per variant, alternating image by image; the prompt
                pass alone (a generation of one token) and the decode (the difference); forward_batch of `--images`
                images and beams of `--beams` widths by the same method; resident_bytes() and memory_allocated.

    python tools/bf16_resident_bench.py [--out profiles/bf16_resident_bench.json] [--rounds 7] [--no-launches]
                                        [--image-steps 7] [--llm-layers 32] [--images 2,4,8] [--beams 3,5,8]

Kernel times: tools/batch_split_bench.py's method - CUDA-event-timed replays of a graph of 64 captured launches that cycle
over distinct weight matrices of the shape (COLD: the rotation puts the streamed bytes above 300 MB), median and min-max over
the rounds."""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.w8_bench import SHAPES, _graph_us                              # noqa: E402

ROWS = (40, 80, 160)
SPAN = {40: (33, 65), 80: (65, 97), 160: (97, 161)}                       # the row ranges of the tile counts 2 / 3 / 5


def bench_launches(rounds=7, parent=True):
    from openpsg_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, K in SHAPES:
        per = N * K * 2                                                   # bytes the kernel streams per launch
        mats = max(8, -(-int(300e6) // per))
        reps = max(64, 2 * mats)
        ws = [(torch.randn(N, K, device=dev, generator=gen) / K ** 0.5).bfloat16() for _ in range(mats)]
        for rows in ROWS:
            x = torch.randn(rows, K, device=dev, generator=gen)

            def own(w):
                return ops.batch_split_gemm_wb16(ops.split_b16x3(x), w)

            def yard(w):
                y = torch.mm(ops.split_b16x3(x).flip(0).view(3 * rows, K), w.t(), out_dtype=torch.float32)
                return ops.Partials(y.view(3, rows, N))
            r = dict(shape=name, N=N, K=K, rows=rows, slices=own(ws[0]).splits, stream_bytes=per, rotation=mats,
                     model_us=round(6 + per / 6.4e6, 1))
            for tag, fn in (("own", own), ("yardstick", yard)):
                med, lo, hi = _graph_us([lambda w=w, fn=fn: fn(w) for w in ws], reps=reps, rounds=rounds)
                r[tag] = dict(us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2))
            r["own_wins"] = r["own"]["us_max"] < r["yardstick"]["us_min"]
            res.append(r)
            print("launch", json.dumps(r), flush=True)
        if parent:                                                        # the parent's routes, on the same VALUES
            few = ws[:max(8, -(-int(300e6) // (2 * per)))]
            w32 = [w.float() for w in few]
            imgs = [ops.split_f16x3(w, weights=True) for w in w32]
            for rows in ROWS:
                x = torch.randn(rows, K, device=dev, generator=gen)
                r = next(q for q in res if q["N"] == N and q["K"] == K and q["rows"] == rows)
                med, lo, hi = _graph_us([lambda a=a: ops.batch_split_gemm_w32(*ops.split_f16x2(x), a[0], a[1], K) for a in imgs],
                                        reps=reps, rounds=rounds)
                r["parent_w32"] = dict(us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2))
                med, lo, hi = _graph_us([lambda w=w: F.linear(x, w) for w in w32], reps=reps, rounds=rounds)
                r["parent_sgemm"] = dict(us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2))
                print("parent", json.dumps(dict(shape=name, rows=rows, w32=r["parent_w32"], sgemm=r["parent_sgemm"])), flush=True)
            del w32, imgs
        del ws
        gc.collect()
        torch.cuda.empty_cache()
    return res


def routing_table(launches):
    """The rows that do not win against the yardstick, as `llm._BATCH_WB16_LIBRARY` lists them."""
    table = {}
    for r in launches:
        if not r["own_wins"]:
            table.setdefault(f"{r['N']},{r['K']}", []).append(list(SPAN[r["rows"]]))
    return table


def _stat(ts):
    return dict(ms_median=round(statistics.median(ts), 2), ms_min=round(min(ts), 2), ms_max=round(max(ts), 2))


def _alternate(fns, steps):
    """{tag: ms per call}: 2 warm-up calls and `steps` timed per variant, alternating call by call."""
    times = {tag: [] for tag in fns}
    for i in range(2 + steps):
        for tag, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= 2:
                times[tag].append((time.perf_counter() - t0) * 1e3)
    return {tag: _stat(ts) for tag, ts in times.items()}


def bench_images(steps, layers, images, beams):
    import numpy as np
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
    w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32, llm_values=torch.bfloat16)
    heads, mem = {}, {}
    for tag, on in (("off", False), ("on", True)):
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        h = RelationTransformerHeadV4(dtype="fp32s", device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                      on_parse_error="skip", suppress_eos=True, llm_bf16_value_stream=True,
                                      llm_bf16_value_resident=on)
        h.load_weights(w)
        gc.collect()
        torch.cuda.empty_cache()
        assert h.llm_engine.bf16_stream_active and h.llm_engine.bf16_value_resident == on
        heads[tag] = h
        mem[tag] = dict(resident_bytes=h.llm_engine.resident_bytes(), memory_allocated_growth=torch.cuda.memory_allocated() - m0)
        print("memory", tag, json.dumps(mem[tag]), flush=True)
    del w
    gc.collect()
    torch.cuda.empty_cache()
    out = {}
    res = dict(layers=layers, memory=mem)
    res["image"] = _alternate({tag: (lambda h=h, tag=tag: out.__setitem__(tag, h(inputs))) for tag, h in heads.items()}, steps)
    res["tokens_equal"] = bool(np.array_equal(np.asarray(heads["off"].last["tokens_host"]), np.asarray(heads["on"].last["tokens_host"])))
    res["results_equal"] = out["off"] == out["on"]
    print("image", json.dumps(res["image"]), "tokens equal:", res["tokens_equal"], flush=True)
    # the LLM stage alone on the image's own inputs: all 16 tokens, and the prompt pass + first token; decode = the difference
    gen = {}
    for tag, h in heads.items():
        X, plen = h.last["llm_inputs"], h.last["prompt_len"]
        gen[tag + " generate"] = lambda h=h, X=X, plen=plen: h.llm_engine.generate(X, plen, suppress_eos=True)
        gen[tag + " prompt"] = lambda h=h, X=X, plen=plen: h.llm_engine.generate(X, plen, max_new_tokens=1, suppress_eos=True)
    res["llm_stage"] = _alternate(gen, steps)
    for tag in heads:
        res["llm_stage"][tag + " decode (difference of medians)"] = round(
            res["llm_stage"][tag + " generate"]["ms_median"] - res["llm_stage"][tag + " prompt"]["ms_median"], 2)
    print("llm stage", json.dumps(res["llm_stage"]), flush=True)
    res["forward_batch"] = {}
    for n in images:
        res["forward_batch"][str(n)] = _alternate({tag: (lambda h=h, n=n: h.forward_batch([inputs] * n)) for tag, h in heads.items()},
                                                  steps)
        print("forward_batch", n, json.dumps(res["forward_batch"][str(n)]), flush=True)
    res["beam"] = {}
    trie = heads["off"].relation_trie()
    for B in beams:
        fns = {}
        for tag, h in heads.items():
            X, plen = h.last["llm_inputs"], h.last["prompt_len"]
            if X.shape[0] * B > 160:
                continue
            fns[tag] = lambda h=h, X=X, plen=plen, B=B: h.llm_engine.generate(X, plen, constraint=trie, beam=B)
        if fns:
            res["beam"][str(B)] = _alternate(fns, steps)
            print("beam", B, json.dumps(res["beam"][str(B)]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bf16_resident_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--image-steps", type=int, default=7)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--images", default="2,4,8")
    ap.add_argument("--beams", default="3,5,8")
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = json.load(open(a.out)) if a.no_launches and os.path.exists(a.out) else {}
    res["device"] = _lib.device_info(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not a.no_launches:
        res["launches"] = bench_launches(rounds=max(7, a.rounds), parent=not a.no_parent)
        res["routing_table_library"] = routing_table(res["launches"])
        json.dump(res, open(a.out, "w"), indent=1)
        print("llm._BATCH_WB16_LIBRARY:", json.dumps(res["routing_table_library"]), flush=True)
    if a.image_steps > 0:
        ints = lambda s: [int(i) for i in s.split(",") if i]                                  # noqa: E731
        res["image_c3"] = bench_images(a.image_steps, a.llm_layers, ints(a.images), ints(a.beams))
        json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
