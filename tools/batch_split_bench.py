"""Timings of the fp32s batched decode of UNQUANTISED weights on psg_batch_gemm_s.hip (llm_batch_split_gemm='own')
on one MI355X:

  per launch    40 / 80 / 160 rows at the Llama-2-7B shapes (q|k|v, o, gate|up, down, lm_head), both forms, psg_split_f16x2
                included, next to exactly what the option-off engine runs for the same product:
                  w32 (generic fp32 weights)  F.linear on fp32 W (the library SGEMM), against psg_batch_split_gemm_w32 on the
                                              prompt pass's [wh | wl | wh] image read in place;
                  w16 (fp16-valued weights)   psg_split_f16x2 + torch.mm of the stacked planes [xh; xl] + Scaled.dense(),
                                              against psg_batch_split_gemm_w16 on the fp16 copy.
                The baselines hand their consumer a dense result, so the new entry is charged a psg_reduce_partials pass.
                The acceptance rule of DESIGN 12 / 16 decides the routing table: a (form, shape, rows) whose range of times
                does not lie wholly below the baseline's goes back to the library.
  whole step    forward_batch of 2 / 4 / 8 BASELINE C3 images (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed),
                32-layer Llama-2-7B-shaped LLM, seeded weights, generic and fp16-valued: option off against option on, on
                the SAME head (the engine's switch is flipped and its graphs dropped), 2 warm-up batches, then `--steps` timed

    python tools/batch_split_bench.py [--out profiles/batch_split_bench.json] [--rounds 7] [--no-launches] [--steps 5]
                                      [--llm-layers 32] [--weights generic,fp16] [--images 2,4,8]

Kernel times: CUDA-event-timed replays of a graph of 64 captured launches that cycle over distinct weight matrices of the
shape, each replay divided out; median and min-max over the rounds.  COLD weights on every side: the rotation holds as
many matrices as put the bytes the NEW kernel streams above 300 MB, beyond the 256 MB Infinity Cache (8 at least), and the
graph walks the rotation at least twice.  `model_us` = 6 us + streamed weight bytes / 6.4 TB/s, for orientation.
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
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.w8_bench import SHAPES, _graph_us                              # noqa: E402

ROWS = (40, 80, 160)


def bench_launches(rounds=7):
    from openpsg_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, K in SHAPES:
        for form in ("w32", "w16"):
            per = N * K * (4 if form == "w32" else 2)                    # bytes the new kernel streams per launch
            mats = max(8, -(-int(300e6) // per))
            reps = max(64, 2 * mats)
            ones = torch.ones(N, device=dev)
            ws = []
            for _ in range(mats):
                w = torch.randn(N, K, device=dev, generator=gen) / K ** 0.5
                if form == "w32":
                    ws.append((w, ops.split_f16x3(w, weights=True)))     # fp32 W (baseline) / ([wh | wl | wh], inverse scales)
                else:
                    ws.append((None, w.half()))                          # an fp16 value: both sides read the fp16 copy
                    del w
            for rows in ROWS:
                x = torch.randn(rows, K, device=dev, generator=gen)
                if form == "w32":
                    new = lambda a: ops.batch_split_gemm_w32(*ops.split_f16x2(x), a[0], a[1], K)      # noqa: E731
                    base = lambda w, a: F.linear(x, w)                                                # noqa: E731
                    baseline = "F.linear fp32"
                else:
                    new = lambda a: ops.batch_split_gemm_w16(*ops.split_f16x2(x), a, ones)            # noqa: E731

                    def base(w, a):
                        a2, inv = ops.split_f16x2(x)
                        y2 = torch.mm(a2.view(2 * rows, K), a.t(), out_dtype=torch.float32)
                        return ops.Scaled(y2.view(2, rows, N), inv, ones).dense()
                    baseline = "split_f16x2 + torch.mm [xh; xl] + Scaled.dense"
                runs = (("own", [lambda a=a: new(a).reduce(torch.float32) for _, a in ws]),
                        ("library", [lambda w=w, a=a: base(w, a) for w, a in ws]))
                r = dict(shape=name, N=N, K=K, form=form, rows=rows, baseline=baseline, slices=new(ws[0][1]).splits,
                         stream_bytes=per, rotation=mats, model_us=round(6 + per / 6.4e6, 1))
                for tag, fns in runs:
                    med, lo, hi = _graph_us(fns, reps=reps, rounds=rounds)
                    r[tag] = dict(us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2))
                r["own_wins"] = r["own"]["us_max"] < r["library"]["us_min"]
                res.append(r)
                print("launch", json.dumps(r), flush=True)
            del ws
            gc.collect()
            torch.cuda.empty_cache()
    return res


def routing_table(launches):
    """The rows that lose against the library, as `llm._BATCH_SPLIT_LIBRARY` lists them (row ranges of the measured counts'
    x tile counts: 40 -> 33..64 (2 tiles), 80 -> 65..96 (3), 160 -> 97..160 (5))."""
    span = {40: (33, 65), 80: (65, 97), 160: (97, 161)}
    table = {}
    for r in launches:
        if not r["own_wins"]:
            table.setdefault(f"{r['form']},{r['N']},{r['K']}", []).append(list(span[r["rows"]]))
    return table


def bench_step(weights, images, steps, layers):
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
    w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32, llm_values=torch.float16 if weights == "fp16" else None)
    h = RelationTransformerHeadV4(dtype="fp32s", device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                  on_parse_error="skip", suppress_eos=True, llm_batch_split_gemm="own")
    h.load_weights(w)
    del w
    gc.collect()
    torch.cuda.empty_cache()
    eng = h.llm_engine
    assert bool(eng._w16_all) == (weights == "fp16")
    out = []
    for n in images:
        r = dict(mode="fp32s", weights=weights, layers=layers, images=n)
        for tag, on in (("library", False), ("own", True)):
            torch.cuda.synchronize()
            eng._graphs.clear()                                        # the switch is no part of a graph's key
            eng.batch_split_gemm = on
            for _ in range(2):                                         # warm-up: graphs, prompt tables, library plans
                h.forward_batch([inputs] * n)
            times = []
            for _ in range(steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h.forward_batch([inputs] * n)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            r[tag] = dict(ms_median=round(statistics.median(times), 2), ms_min=round(min(times), 2), ms_max=round(max(times), 2))
        out.append(r)
        print("step", json.dumps(r), flush=True)
    del h, eng
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_split_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--weights", default="generic,fp16")
    ap.add_argument("--images", default="2,4,8")
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = json.load(open(a.out)) if a.no_launches and os.path.exists(a.out) else {}
    res["device"] = _lib.device_info(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not a.no_launches:
        res["launches"] = bench_launches(rounds=max(7, a.rounds))
        res["routing_table_library"] = routing_table(res["launches"])
        json.dump(res, open(a.out, "w"), indent=1)
        print("routing table (library):", json.dumps(res["routing_table_library"]), flush=True)
    if a.steps > 0:
        res["forward_batch_c3"] = []
        for weights in a.weights.split(","):
            res["forward_batch_c3"] += bench_step(weights, [int(i) for i in a.images.split(",")], a.steps, a.llm_layers)
            json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
