"""Timings of the quantised weight streams in the batched decode (llm_batch_weight_stream='quantised') on one
MI355X:

  per launch    40 / 80 / 160 rows at the Llama-2-7B shapes (q|k|v, o, gate|up, down, lm_head), FP8 and MXFP4, the single
                form (fp16 rows: `mixed`) and the pair form (fp32 rows: `fp32s`, its psg_split_f16x2 included), next to what
                the option-off engine runs for the same product on W': `_plan_batch_mm`'s choice in the 16-bit modes, the
                library SGEMM on fp32 W' in fp32s - and, for llm_weight_resident='quantised', the expansion plus that
                product.  Where the baseline hands its consumer a dense result, the stream is charged a
                psg_reduce_partials pass.  The acceptance rule of DESIGN 12 decides the routing table: a (format, form,
                shape, rows) whose range of times does not lie wholly below the baseline's goes back to the dense path.
  whole step    forward_batch of 2 / 4 / 8 BASELINE C3 images (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed),
                32-layer Llama-2-7B-shaped LLM, seeded weights: option off against option on, on the SAME head (the engine's
                switch is flipped and its graphs dropped), per mode x format x residency

    python tools/batch_quant_bench.py [--out profiles/batch_quant_bench.json] [--rounds 7] [--no-launches]
                                      [--steps 5] [--llm-layers 32] [--modes mixed,fp32s] [--quants fp8,mxfp4]
                                      [--residents all,quantised] [--images 2,4,8]

Kernel times: CUDA-event-timed replays of a graph of captured launches that cycle over distinct weight matrices of the
shape, each replay divided out; median and min-max over the rounds.  COLD weights on every side: the rotation holds as many
matrices as put the streamed bytes of the format alone above 300 MB, beyond the 256 MB Infinity Cache (8 at least: 18 for
o in fp8, 34 in mxfp4), and the graph walks the rotation at least twice.
`model_us` = 6 us + streamed weight bytes / 6.4 TB/s, for orientation.
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


def _weights(fmt, N, K, mats, dev, gen):
    """`mats` quantised matrices of random codes: a list of the kernel's weight arguments and of (q, e, s) for the expansion."""
    from openpsg_amd import ops
    out = []
    for _ in range(mats):
        s = torch.exp2(torch.rand(N, generator=gen, device=dev) * 4 - 8)
        if fmt == "fp8":
            q = torch.randint(0, 256, (N, K), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
            q = torch.where((q & 0x7F) == 0x7F, q - 1, q)
            out.append(((q, s), (q, None, s)))
        else:
            q = torch.randint(0, 256, (N, K // 2), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
            e = torch.randint(114, 128, (N, K // 32), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
            out.append(((q, ops.mxfp4_exp_image(e), s), (q, e, s)))
    return out


def _expand(raw, dtype, out=None):
    from openpsg_amd import ops
    q, e, s = raw
    return ops.expand_w8(q, s, out=out, dtype=dtype) if e is None else ops.expand_w4(q, e, s, out=out, dtype=dtype)


def _rotation(fmt, N, K, floor=8, cold_bytes=300e6):
    """Matrices in the rotation: enough that the streamed bytes of `fmt` alone do not fit the Infinity Cache."""
    per = N * K + 4 * N if fmt == "fp8" else N * K // 2 + N * K // 32 + 4 * N
    return max(floor, -(-int(cold_bytes) // per))


def bench_launches(rounds=7):
    from openpsg_amd import ops
    from openpsg_amd.llm import _plan_batch_mm
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, K in SHAPES:
        for fmt in ("fp8", "mxfp4"):
            if K % (128 if fmt == "fp8" else 256):
                res.append(dict(shape=name, N=N, K=K, format=fmt, unsupported=f"K % {128 if fmt == 'fp8' else 256} != 0"))
                print("launch", res[-1], flush=True)
                continue
            mats = _rotation(fmt, N, K)
            reps = max(64, 2 * mats)
            ws = _weights(fmt, N, K, mats, dev, gen)
            wbytes = sum(t.numel() * t.element_size() for t in ws[0][0])
            for form, xdt in (("single", torch.float16), ("pair", torch.float32)):
                dense = [_expand(raw, xdt) for _, raw in ws]             # W' in the engine's dtype: what 'all' keeps
                scratch = torch.empty_like(dense[0])
                for rows in ROWS:
                    x = torch.randn(rows, K, device=dev, generator=gen).to(xdt)
                    if form == "single":
                        plan = _plan_batch_mm(x, dense)
                        stream = (ops.batch_gemm_w8 if fmt == "fp8" else ops.batch_gemm_w4)
                        new = lambda a: stream(x, *a)                    # noqa: E731
                    else:
                        plan = ("lib",)
                        stream = (ops.batch_split_gemm_w8 if fmt == "fp8" else ops.batch_split_gemm_w4)
                        new = lambda a: stream(*ops.split_f16x2(x), *a)  # noqa: E731
                    if plan[0] == "own":                                 # slices on both sides: nothing to charge
                        base = lambda w: ops.batch_gemm(x, w, plan[1], plan[2])   # noqa: E731
                        new_c = new
                    else:
                        base = lambda w: F.linear(x, w)                  # noqa: E731
                        new_c = lambda a: new(a).reduce(xdt)             # noqa: E731
                    runs = (("stream", [lambda a=a: new_c(a) for a, _ in ws]),
                            ("dense", [lambda w=w: base(w) for w in dense]),
                            ("expand+dense", [lambda r=r: base(_expand(r, xdt, out=scratch)) for _, r in ws]))
                    r = dict(shape=name, N=N, K=K, format=fmt, form=form, rows=rows, baseline="/".join(map(str, plan)),
                             slices=new(ws[0][0]).splits, stream_bytes=wbytes, rotation=mats,
                             model_us=round(6 + wbytes / 6.4e6, 1), model_dense_us=round(6 + dense[0].numel() * dense[0].element_size() / 6.4e6, 1))
                    for tag, fns in runs:
                        med, lo, hi = _graph_us(fns, reps=reps, rounds=rounds)
                        r[tag] = dict(us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2))
                    r["streams_vs_all"] = r["stream"]["us_max"] < r["dense"]["us_min"]
                    r["streams_vs_quantised"] = r["stream"]["us_max"] < r["expand+dense"]["us_min"]
                    res.append(r)
                    print("launch", json.dumps(r), flush=True)
                del dense, scratch
                torch.cuda.empty_cache()
            del ws
            torch.cuda.empty_cache()
    return res


def routing_table(launches):
    """The rows that lose against the 'all' baseline, as `llm._BATCH_QUANT_DENSE` lists them (row ranges of the measured
    counts' x tile counts: 40 -> 33..64 (2 tiles), 80 -> 65..96 (3), 160 -> 97..160 (5))."""
    span = {40: (33, 65), 80: (65, 97), 160: (97, 161)}
    table = {}
    for r in launches:
        if "rows" in r and not r["streams_vs_all"]:
            table.setdefault(f"{r['format']},{r['form']},{r['N']},{r['K']}", []).append(list(span[r["rows"]]))
    return table


def bench_step(mode, quant, resident, images, steps, layers):
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
    w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float16)
    h = RelationTransformerHeadV4(dtype=mode, device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                  on_parse_error="skip", suppress_eos=True, llm_weight_quant=quant,
                                  llm_weight_resident=resident, llm_batch_weight_stream="quantised")
    h.load_weights(w)
    del w
    gc.collect()
    torch.cuda.empty_cache()
    eng = h.llm_engine
    out = []
    for n in images:
        r = dict(mode=mode, llm_weight_quant=quant, llm_weight_resident=resident, layers=layers, images=n)
        for tag, on in (("dense", False), ("quantised", True)):
            torch.cuda.synchronize()
            eng._graphs.clear()                                        # the switch is no part of a graph's key
            eng.batch_quant_stream = on
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_quant_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--modes", default="mixed,fp32s")
    ap.add_argument("--quants", default="fp8,mxfp4")
    ap.add_argument("--residents", default="all,quantised")
    ap.add_argument("--images", default="2,4,8")
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = json.load(open(a.out)) if a.no_launches and os.path.exists(a.out) else {}
    res["device"] = _lib.device_info(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not a.no_launches:
        res["launches"] = bench_launches(rounds=max(7, a.rounds))
        res["routing_table_dense"] = routing_table(res["launches"])
        json.dump(res, open(a.out, "w"), indent=1)
        print("routing table (dense):", json.dumps(res["routing_table_dense"]), flush=True)
    if a.steps > 0:
        res.setdefault("forward_batch_c3", [])
        for mode in a.modes.split(","):
            for quant in a.quants.split(","):
                for resident in a.residents.split(","):
                    res["forward_batch_c3"] += bench_step(mode, quant, resident, [int(i) for i in a.images.split(",")],
                                                          a.steps, a.llm_layers)
                    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
