"""Timings of the multiclass relation head (one MI355X):

  K8b psg_multiclass_head   2 500 / 10 000 pairs x nq in {1, 33} x fp32 / bf16 inputs, R = 56: us and GB/s (cls rows
                            once + W) against the 8 TB/s HBM floor
  K9b psg_topk_large        n = 140 000 / 560 000, k = 100, next to torch.topk(sorted=True) and psg_topk on the same tensor
  whole image               BASELINE C3 (1024x1024, 50 objects, Llama-2-7B shape, fp32s) through head(inputs) with
                            rel_cls_type 'binary' and 'binary+multiclass' on the same weights, alternated in one process

    python tools/multiclass_bench.py [--out profiles/multiclass_bench.json] [--image-steps 10] [--llm-layers 32]

Kernel times: `us` = median of CUDA-event-timed graph replays of 50 captured launches (each launch divided out: the
kernels alone); `host_us` = the same loop issued from Python (what an eager caller pays per call, ctypes included).
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


def _loop_us(fn, reps=50, rounds=7, graph=True):
    fn()
    torch.cuda.synchronize()
    run = None
    if graph:
        g = torch.cuda.CUDAGraph()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            fn()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                for _ in range(reps):
                    fn()
        torch.cuda.synchronize()
        run = g.replay
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if run is not None:
            run()
        else:
            for _ in range(reps):
                fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out.sort()
    return out[len(out) // 2]


def bench_head_kernel():
    from openpsg_amd import ops
    rows = []
    R, H = 56, 768
    w = torch.randn(R, H, device="cuda") * 0.07
    b = torch.randn(R, device="cuda") * 0.05
    for P in (2500, 10000):
        N = int(round(P ** 0.5))
        pidx = torch.arange(P, device="cuda", dtype=torch.int32)
        lg = torch.empty((P, R), device="cuda")
        pr = torch.empty((P, R), device="cuda")
        for nq in (1, 33):
            for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                x = torch.randn(P * nq, H, device="cuda").to(dt)
                fn = lambda: ops.multiclass_head(x, w, b, P, nq, pidx, N, logit=lg, prob=pr)  # noqa: E731
                us, host = _loop_us(fn), _loop_us(fn, graph=False)
                nbytes = P * H * x.element_size() + R * H * 4 + 2 * P * R * 4
                rows.append(dict(pairs=P, nq=nq, dtype=name, us=round(us, 2), host_us=round(host, 2), bytes=nbytes,
                                 gbps=round(nbytes / us / 1e3, 1), floor_us_8tbs=round(nbytes / 8e12 * 1e6, 2)))
                print("K8b", rows[-1], flush=True)
                del x
    return rows


def bench_topk():
    from openpsg_amd import ops
    rows = []
    for n in (140_000, 560_000):
        s = torch.sigmoid(torch.randn(n, device="cuda") * 3)
        k = 100
        ws = torch.empty(ops.topk_large_workspace_bytes(s.device, n, k), device="cuda", dtype=torch.uint8)
        idx = torch.empty(k, device="cuda", dtype=torch.int32)
        val = torch.empty(k, device="cuda", dtype=torch.float32)
        fl = lambda: ops.topk_large(s, k, ws, idx=idx, val=val)  # noqa: E731
        ft = lambda: torch.topk(s, k, sorted=True)  # noqa: E731
        t_large, t_torch = _loop_us(fl), _loop_us(ft)
        h_large, h_torch = _loop_us(fl, graph=False), _loop_us(ft, graph=False)
        t_psg = _loop_us(lambda: ops.topk(s, k), reps=5, rounds=3)
        ref = torch.topk(s, k, sorted=True)
        same_vals = bool(torch.equal(ref.values, val))
        rows.append(dict(n=n, k=k, psg_topk_large_us=round(t_large, 2), torch_topk_us=round(t_torch, 2),
                         psg_topk_us=round(t_psg, 2), psg_topk_large_host_us=round(h_large, 2),
                         torch_topk_host_us=round(h_torch, 2), same_values_as_torch=same_vals))
        print("K9b", rows[-1], flush=True)
    return rows


def bench_image(steps, llm_layers):
    from openpsg_amd.config import LlamaConfig, PSGConfig, QFormerConfig
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_device
    dev = torch.device("cuda", 0)
    cfg = PSGConfig(qformer=QFormerConfig(), llm=LlamaConfig(layers=llm_layers), max_object_num=50,
                    rel_cls_type="binary+multiclass")
    w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32)
    heads = {}
    for t in ("binary", "binary+multiclass"):
        h = RelationTransformerHeadV4(dtype="fp32s", device=str(dev), tokenizers="word", max_object_num=50,
                                      llm_config=cfg.llm, on_parse_error="skip", suppress_eos=True, rel_cls_type=t)
        h.load_weights(w)
        heads[t] = h
    del w
    torch.cuda.empty_cache()
    scene = make_scene((1024, 1024), 50, seed=0, device=str(dev))
    inputs = dict(mask_features=scene["mask_features"], img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"])])
    for h in heads.values():                                        # warm-up: graphs, prompt tables, library plans
        for _ in range(2):
            h(inputs)
    times = {t: [] for t in heads}
    for _ in range(steps):
        for t, h in heads.items():                                  # alternated: drifts hit both alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = h(inputs)
            torch.cuda.synchronize()
            times[t].append((time.perf_counter() - t0) * 1e3)
    med = {t: sorted(v)[len(v) // 2] for t, v in times.items()}
    res = dict(config="C3 1024x1024, 50 objects, fp32s, Llama-2-7B shape", llm_layers=llm_layers, steps=steps,
               ms_per_image_median={t: round(v, 3) for t, v in med.items()},
               ms_per_image_all={t: [round(x, 3) for x in v] for t, v in times.items()},
               extra_ms=round(med["binary+multiclass"] - med["binary"], 3),
               triples_of_the_multiclass_head_output=len(out["rel_pred"]))
    print("image", {k: v for k, v in res.items() if k != "ms_per_image_all"}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multiclass_bench.json"))
    ap.add_argument("--image-steps", type=int, default=10)
    ap.add_argument("--llm-layers", type=int, default=32)
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), head_kernel=bench_head_kernel(), topk=bench_topk())
    if a.image_steps > 0:
        res["image"] = bench_image(a.image_steps, a.llm_layers)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
