"""Timings of grouped-query attention (GQA) on one MI355X:

  decode attention   psg_decode_attn_gqa at 20 rows, 32 query / 8 key-value heads, positions 48..80, fp32 and bf16, for
                     every split of a group over workgroups (option decode_gqa_qparts; 0 = the library's rule), next to
                     psg_decode_attn (decode_attn4_kernel) on a 32-head multi-head cache at the same positions
  whole image        BASELINE C3 (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed) through head(inputs) with a
                     32-layer Mistral-7B-shaped LLM (4096 / 32 q, 8 kv heads / 14336 / 32000) in fp32s (generic fp32
                     weights and fp16-valued weights) and mixed, and the Llama-2-7B shape in fp32s next to them

    python tools/gqa_bench.py [--out profiles/gqa_bench.json] [--image-steps 5] [--llm-layers 32]

Kernel times: median over 7 rounds of CUDA-event-timed graph replays of 64 captured launches, each divided out.  The
launches cycle over 8 cache sets (the layers of a decode step), so the caches are not all resident in the Infinity Cache.
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


def _graph_us(fns, reps=64, rounds=7):
    """Median us per launch of `fns[i % len(fns)]()`, i < reps, replayed as one captured graph."""
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
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    out.sort()
    return out[len(out) // 2]


def bench_decode_attn(rows=20, heads=32, kv=8, layers=8):
    from openpsg_amd import _lib, ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    pos = torch.randint(48, 81, (rows,), device=dev, generator=gen, dtype=torch.int32)
    pair = torch.arange(rows, device=dev, dtype=torch.int32)
    ctx = 96
    hd = 128
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(4096, dtype=torch.float32)[:, None] * inv_freq[None, :]
    rope = (ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev))
    res = []
    old = _lib.get_option(0, "decode_gqa_qparts")
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for kind, nkv in (("mha", heads), ("gqa", kv)):
            qkv = torch.randn(rows, (heads + 2 * nkv) * hd, device=dev, generator=gen).to(dt)
            kc = [torch.randn(rows, nkv, ctx, hd, device=dev, generator=gen).to(dt) for _ in range(layers)]
            vc = [torch.randn(rows, nkv, ctx, hd, device=dev, generator=gen).to(dt) for _ in range(layers)]
            out = torch.empty(rows, heads * hd, device=dev, dtype=dt)
            # bytes a launch must move: the cache rows [0, pos) it reads + q|k|v in + the output
            nbytes = int(pos.sum()) * nkv * hd * 2 * kc[0].element_size() + qkv.numel() * qkv.element_size() \
                + out.numel() * out.element_size()
            kvh = None if kind == "mha" else nkv

            def mk(l):
                return lambda: ops.decode_attn(qkv, pair, pos, rope, heads, hd, ctx, kc[l], vc[l], out, kv_heads=kvh)
            fns = [mk(l) for l in range(layers)]
            for qp in ((0,) if kind == "mha" else (0, 1, 2, 4)):
                _lib.set_option(0, "decode_gqa_qparts", qp)
                us = _graph_us(fns)
                r = dict(dtype=name, kind=kind, heads=heads, kv_heads=nkv, rows=rows, positions="48..80",
                         qparts=qp if kind == "gqa" else None, us=round(us, 2), bytes=nbytes,
                         gbps=round(nbytes / us / 1e3, 1))
                res.append(r)
                print("decode_attn", r, flush=True)
            del kc, vc
    _lib.set_option(0, "decode_gqa_qparts", old)
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
    mistral = LlamaConfig(layers=layers, inter=14336, kv_heads=8)
    llama = LlamaConfig(layers=layers)
    runs = [("mistral-7b", mistral, "fp32s", None), ("mistral-7b", mistral, "fp32s", torch.float16),
            ("mistral-7b", mistral, "mixed", None), ("llama-2-7b", llama, "fp32s", None)]
    res = []
    for model, llm, mode, values in runs:
        cfg = PSGConfig(qformer=QFormerConfig(), llm=llm, max_object_num=50)
        w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32, llm_values=values)
        h = RelationTransformerHeadV4(dtype=mode, device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                      on_parse_error="skip", suppress_eos=True)
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
        r = dict(model=model, mode=mode, weights="fp16-valued" if values is not None else "generic fp32", layers=layers,
                 kv_heads=llm.n_kv_heads, inter=llm.inter, w16_stream=bool(h.llm_engine._w16_all),
                 ms_per_image_median=round(sorted(times)[len(times) // 2], 2), ms_per_image_all=[round(t, 2) for t in times])
        res.append(r)
        print("image", r, flush=True)
        del h
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gqa_bench.json"))
    ap.add_argument("--image-steps", type=int, default=5)
    ap.add_argument("--llm-layers", type=int, default=32)
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), decode_attn=bench_decode_attn())
    if a.image_steps > 0:
        res["image_c3"] = bench_images(a.image_steps, a.llm_layers)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
