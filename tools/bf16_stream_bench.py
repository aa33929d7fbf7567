"""Timings of the bf16 value stream (llm_bf16_value_stream) on one MI355X, against what the engine runs for the
same shape on the same values WITHOUT the option:

  per launch    20 rows at the Llama-2-7B shapes (q|k|v, o, gate|up, down, lm_head), cold weights, in one process:
                  psg_split_gemm_wb16 (three bf16 planes of the fp32 rows, 2 bytes per weight)  next to its YARDSTICK, the
                  fp32 decode kernel on the fp32 tensor (psg_skinny_gemm: 4 bytes per weight), and, for information,
                  psg_split_gemm_w16 on an fp16 copy of the shape (two planes, the same bytes per weight).
                THE ACCEPTANCE RULE: a shape whose range (min-max) does not lie wholly below its yardstick's range belongs
                in llm.WB16_STREAM_OFF (`stream_off` in the output; the entries are printed at the end)
  row kernels   the row launches of one decoder layer of a decode step at 20 rows on the three routes (the bf16 route has ONE
                stand-alone split per layer where the fp16 route has two), us per launch and per layer
  whole image   BASELINE C3 (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed) through head(inputs) with a 32-layer
                Llama-2-7B-shaped LLM of seeded bf16-valued weights: option off against on in ONE process, 2 warm-up images
                and `--image-steps` timed ones per variant, alternating image by image

    python tools/bf16_stream_bench.py [--out profiles/bf16_stream_bench.json] [--image-steps 7] [--llm-layers 32] [--rounds 7]

Kernel times as tools/w8_bench.py's: CUDA-event-timed replays of a graph of 64 captured launches that cycle over distinct
weight matrices of the shape, each replay divided out; median and min-max over the rounds.  Cold weights: as many matrices as
make the bf16 copies 320 MB together (at least 4), beyond the 256 MB Infinity Cache.  TB/s = the weight bytes of the launch
over its time.
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


def _row(r):
    return dict(us_median=round(r[0], 2), us_min=round(r[1], 2), us_max=round(r[2], 2))


def bench_launches(rows=20, rounds=7, cold_bytes=320e6):
    from openpsg_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, K in SHAPES:
        n = min(64, max(4, -(-int(cold_bytes) // (2 * N * K))))
        wb = [(torch.randn(N, K, device=dev, generator=gen) * 0.02).bfloat16() for _ in range(n)]
        w32 = [w.float() for w in wb]                                   # the same values: what from_pretrained upcasts
        w16 = [w.half() for w in w32]
        x = torch.randn(rows, K, device=dev, generator=gen)
        x3 = ops.split_b16x3(x)
        x2, inv = ops.split_f16x2(x)
        kernels = (("psg_skinny_gemm fp32 (yardstick)", 4 * N * K, [(lambda w=w: ops.skinny_gemm(x, w)) for w in w32]),
                   ("psg_split_gemm_wb16", 2 * N * K, [(lambda w=w: ops.split_gemm_wb16(x3, w)) for w in wb]),
                   ("psg_split_gemm_w16 on an fp16 copy (information)", 2 * N * K,
                    [(lambda w=w: ops.split_gemm_w16(x2, inv, w)) for w in w16]))
        rs = []
        for kname, nbytes, fns in kernels:
            t = _graph_us(fns, rounds=rounds)
            rs.append(dict(shape=name, N=N, K=K, rows=rows, kernel=kname, matrices=len(fns), slices=fns[0]().splits,
                           weight_bytes=nbytes, streamed_bytes=nbytes * len(fns), tbps=round(nbytes / t[0] / 1e6, 3), **_row(t)))
        rs[1]["stream_off"] = not rs[1]["us_max"] < rs[0]["us_min"]     # the acceptance rule
        for r in rs:
            print("launch", r, flush=True)
        res += rs
        del wb, w32, w16
        torch.cuda.empty_cache()
    return res


def bench_row_kernels(rows=20, hidden=4096, inter=11008, rounds=7):
    """The row launches of one decoder layer of a decode step: (route, kernel, launches per layer, us)."""
    from openpsg_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    resid = torch.randn(rows, hidden, device=dev, generator=gen)
    delta = ops.Partials(torch.randn(8, rows, hidden, device=dev, generator=gen) * 0.01)
    gu = ops.Partials(torch.randn(2, rows, 2 * inter, device=dev, generator=gen))
    g = torch.ones(hidden, device=dev)
    att, act, n = torch.randn(rows, hidden, device=dev, generator=gen), torch.empty(rows, inter, device=dev), torch.empty_like(resid)
    table = (("bf16 stream", "psg_rmsnorm_split_b16x3", 2, lambda: ops.rmsnorm_split_b16x3(resid, delta, g, 1e-5)),
             ("bf16 stream", "psg_split_b16x3 (attention output)", 1, lambda: ops.split_b16x3(att)),
             ("bf16 stream", "psg_silu_mul_split_b16x3", 1, lambda: ops.silu_mul_split_b16x3(gu)),
             ("fp16 stream", "psg_rmsnorm_split2", 2, lambda: ops.rmsnorm_split2(resid, delta, g, 1e-5)),
             ("fp16 stream", "psg_split_f16x2 (attention output)", 1, lambda: ops.split_f16x2(att)),
             ("fp16 stream", "psg_silu_mul", 1, lambda: ops.silu_mul(gu, act)),
             ("fp16 stream", "psg_split_f16x2 (SwiGLU output)", 1, lambda: ops.split_f16x2(act)),
             ("fp32 stream", "psg_rmsnorm", 2, lambda: ops.rmsnorm(resid, delta, g, 1e-5, n)),
             ("fp32 stream", "psg_silu_mul", 1, lambda: ops.silu_mul(gu, act)))
    res = []
    for route, kname, per_layer, fn in table:
        r = dict(route=route, kernel=kname, rows=rows, launches_per_layer=per_layer, **_row(_graph_us([fn], rounds=rounds)))
        print("row", r, flush=True)
        res.append(r)
    per = {}
    for r in res:
        per[r["route"]] = round(per.get(r["route"], 0.0) + r["launches_per_layer"] * r["us_median"], 2)
    print("row kernels, us per layer and step:", per, flush=True)
    return dict(kernels=res, us_per_layer_step=per)


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
    w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32, llm_values=torch.bfloat16)
    heads = {}
    for on in (False, True):
        h = RelationTransformerHeadV4(dtype="fp32s", device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                      on_parse_error="skip", suppress_eos=True, llm_bf16_value_stream=on)
        h.load_weights(w)
        assert not h.llm_engine._w16_all and not (h.llm_engine.bf16_stream_active and not on)
        heads[on] = h
    del w
    torch.cuda.empty_cache()
    times, out = {False: [], True: []}, {}
    for i in range(2 + steps):                                        # 2 warm-up images per variant, then alternating
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[on] = heads[on](inputs)
            torch.cuda.synchronize()
            if i >= 2:
                times[on].append((time.perf_counter() - t0) * 1e3)
    res = []
    for on in (False, True):
        t = sorted(times[on])
        r = dict(llm_bf16_value_stream=on, layers=layers, stream_active=bool(heads[on].llm_engine.bf16_stream_active),
                 ms_per_image_median=round(t[len(t) // 2], 2), ms_per_image_min=round(t[0], 2), ms_per_image_max=round(t[-1], 2),
                 ms_per_image_all=[round(v, 2) for v in times[on]], resident_bytes=heads[on].llm_engine.resident_bytes())
        res.append(r)
        print("image", r, flush=True)
    same = np_equal(heads[False].last["tokens_host"], heads[True].last["tokens_host"])
    print("tokens of the two variants equal:", same, flush=True)
    return dict(variants=res, tokens_equal=same, results_equal=out[False] == out[True])


def np_equal(a, b):
    import numpy as np
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bf16_stream_bench.json"))
    ap.add_argument("--image-steps", type=int, default=7)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), launches=bench_launches(rounds=a.rounds))
    off = sorted((r["N"], r["K"]) for r in res["launches"] if r.get("stream_off"))
    res["wb16_stream_off"] = off
    print(f"llm.WB16_STREAM_OFF = frozenset({off})")
    res["row_kernels"] = bench_row_kernels(rounds=a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    if a.image_steps > 0:
        res["image_c3"] = bench_images(a.image_steps, a.llm_layers)
        json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
