"""Timings of the FP8-quantised LLM weight stream (llm_weight_quant='fp8') on one MI355X:

  per launch    20 rows at the Llama-2-7B shapes (q|k|v, o, gate|up, down, lm_head): psg_split_gemm_w8 next to
                psg_split_gemm_w16 (fp32s: two-plane fp32 rows) and psg_skinny_gemm_w8 next to the 16-bit psg_skinny_gemm
                (fp16 rows), in the same process
  whole image   BASELINE C3 (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed) through head(inputs) with a
                32-layer Llama-2-7B-shaped LLM: fp32s on fp16-valued weights and mixed, each with and without the option

    python tools/w8_bench.py [--out profiles/w8_bench.json] [--image-steps 5] [--llm-layers 32] [--rounds 7]

Kernel times: CUDA-event-timed replays of a graph of 64 captured launches that cycle over 8 distinct weight matrices of the
shape (8 layers' worth: 0.27-2.1 GB, beyond the 256 MB Infinity Cache), each replay divided out; median and min-max over
the rounds.  TB/s = the WEIGHT bytes of the launch over its time.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = (("q|k|v", 12288, 4096), ("o", 4096, 4096), ("gate|up", 22016, 4096), ("down", 4096, 11008), ("lm_head", 32000, 4096))


def _graph_us(fns, reps=64, rounds=7):
    """us per launch of `fns[i % len(fns)]()`, i < reps, replayed as one captured graph: (median, min, max) over rounds."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            for i in range(reps):
                fns[i % len(fns)]()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out = sorted(out[1:])                                              # (the first replay uploads the graph)
    return out[len(out) // 2], out[0], out[-1]


def bench_launches(rows=20, mats=8, rounds=7):
    from openpsg_amd import ops
    from openpsg_amd.weights import quantize_fp8_rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, K in SHAPES:
        w16 = [(torch.randn(N, K, device=dev, generator=gen) / K ** 0.5).half() for _ in range(mats)]
        w8 = [quantize_fp8_rows(w.float()) for w in w16]
        x = torch.randn(rows, K, device=dev, generator=gen)
        x2, inv = ops.split_f16x2(x)
        xh = x.half()
        kernels = (("psg_split_gemm_w16", 2, [(lambda w=w: ops.split_gemm_w16(x2, inv, w)) for w in w16]),
                   ("psg_split_gemm_w8", 1, [(lambda q=q, s=s: ops.split_gemm_w8(x2, inv, q, s)) for q, s in w8]),
                   ("psg_skinny_gemm fp16", 2, [(lambda w=w: ops.skinny_gemm(xh, w)) for w in w16]),
                   ("psg_skinny_gemm_w8 fp16", 1, [(lambda q=q, s=s: ops.skinny_gemm_w8(xh, q, s)) for q, s in w8]))
        for kname, nbytes, fns in kernels:
            med, lo, hi = _graph_us(fns, rounds=rounds)
            r = dict(shape=name, N=N, K=K, rows=rows, kernel=kname, slices=fns[0]().splits, weight_bytes=N * K * nbytes,
                     us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2),
                     tbps=round(N * K * nbytes / med / 1e6, 3))
            res.append(r)
            print("launch", r, flush=True)
        del w16, w8
        torch.cuda.empty_cache()
    return res


def bench_images(steps, layers):
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
    res = []
    for mode, quant in (("fp32s", None), ("fp32s", "fp8"), ("mixed", None), ("mixed", "fp8")):
        w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32 if mode == "fp32s" else torch.float16,
                                llm_values=torch.float16 if mode == "fp32s" else None)
        h = RelationTransformerHeadV4(dtype=mode, device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                      on_parse_error="skip", suppress_eos=True, llm_weight_quant=quant)
        h.load_weights(w)
        del w
        torch.cuda.empty_cache()
        for _ in range(2):                                            # warm-up: graphs, prompt tables, library plans
            h(inputs)
        times = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h(inputs)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        eng = h.llm_engine
        r = dict(mode=mode, llm_weight_quant=quant, layers=layers, w16_stream=bool(eng._w16_all), w8_stream=eng.layer_kind == "w8",
                 ms_per_image_median=round(sorted(times)[len(times) // 2], 2), ms_per_image_all=[round(t, 2) for t in times])
        res.append(r)
        print("image", r, flush=True)
        del h, eng
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "w8_bench.json"))
    ap.add_argument("--image-steps", type=int, default=5)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), launches=bench_launches(rounds=a.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    if a.image_steps > 0:
        res["image_c3"] = bench_images(a.image_steps, a.llm_layers)
        json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
