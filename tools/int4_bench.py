"""Timings of the group-wise INT4 LLM weight stream (llm_weight_quant='int4g') on one MI355X, against what the
engine runs for the same shape on W' WITHOUT the stream:

  per launch    20 rows at the Llama-2-7B shapes (q|k|v, o, gate|up, down, lm_head), cold weights, in one process:
                  psg_split_gemm_int4 (fp32s: two-plane fp32 rows)  next to its YARDSTICK, the fp32 decode kernel on W' in fp32
                                                                    (psg_skinny_gemm: 4 bytes per weight),
                  psg_skinny_gemm_int4 (fp16 rows)                  next to its YARDSTICK, the 16-bit skinny kernel on W' in
                                                                    fp16 (2 bytes per weight),
                and, for information, psg_split_gemm_w4 / psg_skinny_gemm_w4 on an MXFP4 matrix of the shape: the same bytes
                per weight, so parity is the expectation (a model, not a measurement).
                THE ACCEPTANCE RULE: a shape and form whose INT4 range (min-max) does not lie wholly below its yardstick's
                range belongs in llm.INT4_STREAM_OFF (`stream_off` in the output; the entries are printed at the end)
  whole image   BASELINE C3 (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed) through head(inputs) with a
                32-layer Llama-2-7B-shaped LLM: fp32s and mixed, each with 'int4g' and without the option

    python tools/int4_bench.py [--out profiles/int4_bench.json] [--image-steps 5] [--llm-layers 32] [--rounds 7]

Kernel times as tools/w8_bench.py's: CUDA-event-timed replays of a graph of 64 captured launches that cycle over distinct
weight matrices of the shape, each replay divided out; median and min-max over the rounds.  Cold weights: as many matrices
as make their code images 512 MB together (8 to 64), beyond the 256 MB Infinity Cache in every format.  TB/s = the WEIGHT
bytes of the launch (group image included) over its time.
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
    from openpsg_amd.weights import dequantize_int4_groups
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, K in SHAPES:
        i4, w4, w32, w16 = [], [], [], []
        b4 = N * K // 2 + N * K // 32
        for _ in range(min(64, max(8, -(-int(cold_bytes) // b4)))):
            q = torch.randint(0, 256, (N, K // 2), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            gs = (torch.exp2(torch.rand(N, K // 128, device=dev, generator=gen) * 2 - 8) * 0.977).to(torch.float16)
            gz = torch.randint(0, 16, (N, K // 128), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            w = dequantize_int4_groups(q, gs, gz)
            w32.append(w)
            w16.append(w.half())
            i4.append((ops.int4_q_image(q), ops.int4_group_image(gs, gz)))
            e = torch.randint(114, 128, (N, K // 32), device=dev, generator=gen, dtype=torch.int32).to(torch.uint8)
            w4.append((q, ops.mxfp4_exp_image(e), torch.ones(N, device=dev)))    # (the same bytes read as MXFP4: any nibble is a code)
        x = torch.randn(rows, K, device=dev, generator=gen)
        x2, inv = ops.split_f16x2(x)
        xh = x.half()
        kernels = (("psg_skinny_gemm fp32 on W' (yardstick)", 4 * N * K, [(lambda w=w: ops.skinny_gemm(x, w)) for w in w32]),
                   ("psg_split_gemm_int4", b4, [(lambda a=a, b=b: ops.split_gemm_int4(x2, inv, a, b)) for a, b in i4]),
                   ("psg_split_gemm_w4", b4, [(lambda q=q, e=e, s=s: ops.split_gemm_w4(x2, inv, q, e, s)) for q, e, s in w4]),
                   ("psg_skinny_gemm fp16 on W' (yardstick)", 2 * N * K, [(lambda w=w: ops.skinny_gemm(xh, w)) for w in w16]),
                   ("psg_skinny_gemm_int4 fp16", b4, [(lambda a=a, b=b: ops.skinny_gemm_int4(xh, a, b)) for a, b in i4]),
                   ("psg_skinny_gemm_w4 fp16", b4, [(lambda q=q, e=e, s=s: ops.skinny_gemm_w4(xh, q, e, s)) for q, e, s in w4]))
        rs = []
        for kname, nbytes, fns in kernels:
            med, lo, hi = _graph_us(fns, rounds=rounds)
            rs.append(dict(shape=name, N=N, K=K, rows=rows, kernel=kname, matrices=len(fns), slices=fns[0]().splits, weight_bytes=nbytes,
                           us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2), tbps=round(nbytes / med / 1e6, 3)))
        for form, ry, ri in (("pair", rs[0], rs[1]), ("single", rs[3], rs[4])):   # the acceptance rule
            ri["form"], ri["stream_off"] = form, not ri["us_max"] < ry["us_min"]
        for r in rs:
            print("launch", r, flush=True)
        res += rs
        del i4, w4, w32, w16
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
        for quant in (None, "int4g"):
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
                     int4_stream=eng.layer_kind == "int4",
                     ms_per_image_median=round(sorted(times)[len(times) // 2], 2), ms_per_image_all=[round(t, 2) for t in times])
            res.append(r)
            print("image", r, flush=True)
            del h, eng
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "int4_bench.json"))
    ap.add_argument("--image-steps", type=int, default=5)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), launches=bench_launches(rounds=a.rounds))
    off = {form: sorted((r["N"], r["K"]) for r in res["launches"] if r.get("form") == form and r["stream_off"])
           for form in ("pair", "single")}
    res["int4_stream_off"] = off
    print("llm.INT4_STREAM_OFF =", {f: f"frozenset({v})" for f, v in off.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    if a.image_steps > 0:
        res["image_c3"] = bench_images(a.image_steps, a.llm_layers)
        json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
