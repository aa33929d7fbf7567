"""Timings of the MXFP4-quantised LLM weight stream (llm_weight_quant='mxfp4') on one MI355X, against the FP8
stream of the SAME model:

  per launch    20 rows at the Llama-2-7B shapes (q|k|v, o, gate|up, down, lm_head): psg_split_gemm_w4 next to
                psg_split_gemm_w8 (fp32s: two-plane fp32 rows) and psg_skinny_gemm_w4 next to psg_skinny_gemm_w8 (fp16
                rows), in the same process, both over the same W': the FP8 operand is weights.mxfp4_as_fp8_rows of the
                MXFP4 one.  A shape whose MXFP4 range (min-max) does not lie wholly below its FP8 range belongs in
                llm.W4_STREAM_AS_FP8 (`as_fp8` in the output)
  whole image   BASELINE C3 (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed) through head(inputs) with a
                32-layer Llama-2-7B-shaped LLM: fp32s and mixed, each with 'mxfp4', 'fp8' and without the option

    python tools/w4_bench.py [--out profiles/w4_bench.json] [--image-steps 5] [--llm-layers 32] [--rounds 7]

Kernel times as tools/w8_bench.py's: CUDA-event-timed replays of a graph of 64 captured launches that cycle over distinct
weight matrices of the shape, each replay divided out; median and min-max over the rounds.  Cold weights: as many
matrices as make their nibble images 512 MB together (8 to 64; the FP8 images of the same matrices are twice that), beyond
the 256 MB Infinity Cache in either format.  TB/s = the WEIGHT bytes of the launch (block exponents included) over its time.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.w8_bench import SHAPES, _graph_us  # noqa: E402


def bench_launches(rows=20, rounds=7, cold_bytes=512e6):
    from openpsg_amd import ops
    from openpsg_amd.weights import mxfp4_as_fp8_rows, quantize_mxfp4_rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, K in SHAPES:
        w4, w8 = [], []
        b4, b8 = N * K // 2 + N * K // 32, N * K
        for _ in range(min(64, max(8, -(-int(cold_bytes) // b4)))):
            q, e, s = quantize_mxfp4_rows(torch.randn(N, K, device=dev, generator=gen) / K ** 0.5)
            w8.append(mxfp4_as_fp8_rows(q, e, s))
            w4.append((q, ops.mxfp4_exp_image(e), s))
        x = torch.randn(rows, K, device=dev, generator=gen)
        x2, inv = ops.split_f16x2(x)
        xh = x.half()
        kernels = (("psg_split_gemm_w8", b8, [(lambda q=q, s=s: ops.split_gemm_w8(x2, inv, q, s)) for q, s in w8]),
                   ("psg_split_gemm_w4", b4, [(lambda q=q, e=e, s=s: ops.split_gemm_w4(x2, inv, q, e, s)) for q, e, s in w4]),
                   ("psg_skinny_gemm_w8 fp16", b8, [(lambda q=q, s=s: ops.skinny_gemm_w8(xh, q, s)) for q, s in w8]),
                   ("psg_skinny_gemm_w4 fp16", b4, [(lambda q=q, e=e, s=s: ops.skinny_gemm_w4(xh, q, e, s)) for q, e, s in w4]))
        rs = []
        for kname, nbytes, fns in kernels:
            med, lo, hi = _graph_us(fns, rounds=rounds)
            rs.append(dict(shape=name, N=N, K=K, rows=rows, kernel=kname, matrices=len(fns), slices=fns[0]().splits, weight_bytes=nbytes,
                           us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2), tbps=round(nbytes / med / 1e6, 3)))
        for r8, r4 in ((rs[0], rs[1]), (rs[2], rs[3])):                # the acceptance rule: MXFP4's range wholly below FP8's
            r4["as_fp8"] = not r4["us_max"] < r8["us_min"]
        for r in rs:
            print("launch", r, flush=True)
        res += rs
        del w4, w8
        torch.cuda.empty_cache()
    return res


def bench_images(steps, layers):
    import time
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
    for mode in ("fp32s", "mixed"):
        for quant in (None, "fp8", "mxfp4"):
            w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32 if mode == "fp32s" else torch.float16,
                                    llm_values=torch.float16 if mode == "fp32s" else None)
            h = RelationTransformerHeadV4(dtype=mode, device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                          on_parse_error="skip", suppress_eos=True, llm_weight_quant=quant)
            h.load_weights(w)
            del w
            torch.cuda.empty_cache()
            for _ in range(2):                                        # warm-up: graphs, prompt tables, library plans
                h(inputs)
            times = []
            for _ in range(steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h(inputs)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            eng = h.llm_engine
            r = dict(mode=mode, llm_weight_quant=quant, layers=layers, w16_stream=bool(eng._w16_all),
                     w8_stream=eng.layer_kind == "w8", w4_stream=eng.layer_kind == "w4",
                     ms_per_image_median=round(sorted(times)[len(times) // 2], 2), ms_per_image_all=[round(t, 2) for t in times])
            res.append(r)
            print("image", r, flush=True)
            del h, eng
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "w4_bench.json"))
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
