"""Cost of llm_rel_scores='likelihood'  on one MI355X:

  whole image   BASELINE C3 (1024x1024, 50 objects, top-20, 16 tokens, EOS suppressed) through head(inputs) with a 32-layer
                Llama-2-7B-shaped LLM, in fp32s and mixed: ms per image with the option off ('constant') and on
                ('likelihood', num_llm_ranked_triples=100), the same head object toggled between the two
  the pass      trie rows (K x internal nodes) and the device time of one image's kernels split into GEMM (library and
                own projections), attention (psg_tree_attn), log-prob (psg_token_logprobs) and the rest, as the difference
                between a profiled 'likelihood' image and a profiled 'constant' image (torch.profiler, eager launches:
                use_graph off for the profiled pair only)

    python tools/llm_rank_bench.py [--out profiles/llm_rank_bench.json] [--image-steps 5] [--llm-layers 32]
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


def _kernel_split(h, inputs):
    """Device us per category of one eager image (profiler), {category: us}."""
    from torch.profiler import ProfilerActivity, profile
    h.llm_engine.use_graph = False
    h(inputs)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        h(inputs)
        torch.cuda.synchronize()
    h.llm_engine.use_graph = True
    cats = dict(gemm=0.0, tree_attn=0.0, token_logprobs=0.0, other=0.0)
    for e in prof.key_averages():
        name = e.key.lower()
        t = float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)))
        if "tree_attn" in name:
            cats["tree_attn"] += t
        elif "token_logprobs" in name:
            cats["token_logprobs"] += t
        elif any(s in name for s in ("gemm", "cijk", "gemv", "mfma", "matmul", "split_mm", "batch_gemm")):
            cats["gemm"] += t
        else:
            cats["other"] += t
    return cats


def bench(steps, layers, modes):
    from openpsg_amd.config import LlamaConfig, PSGConfig, QFormerConfig
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_scene
    from openpsg_amd.weights import make_weights_device
    dev = torch.device("cuda", 0)
    scene = make_scene((1024, 1024), 50, seed=0, device=str(dev))
    inputs = dict(mask_features=scene["mask_features"], img_metas=[scene["img_meta"]],
                  object_info=[dict(object_id_list=scene["object_id_list"], pan_results=scene["pan_results"])])
    llm = LlamaConfig(layers=layers)
    res = []
    for mode in modes:
        cfg = PSGConfig(qformer=QFormerConfig(), llm=llm, max_object_num=50)
        w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32)
        h = RelationTransformerHeadV4(dtype=mode, device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                      on_parse_error="skip", suppress_eos=True)
        h.load_weights(w)
        del w
        torch.cuda.empty_cache()
        trie = None
        r = dict(model="llama-2-7b", mode=mode, layers=layers)
        for opt in ("constant", "likelihood"):
            h.llm_rel_scores = opt
            h.num_llm_ranked_triples = 100 if opt == "likelihood" else 0
            if opt == "likelihood":
                trie = h.relation_trie()
            for _ in range(2):                                        # warm-up: graphs, prompt tables, library plans
                out = h(inputs)
            times = []
            for _ in range(steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = h(inputs)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            r[opt] = dict(ms_per_image_median=round(sorted(times)[len(times) // 2], 2),
                          ms_per_image_all=[round(t, 2) for t in times], triples=len(out["rel_pred"]))
        K = int(h.last["selected_host"].shape[0])
        r["trie_rows_per_pair"] = trie.n_int
        r["trie_rows"] = K * trie.n_int
        r["added_ms_per_image"] = round(r["likelihood"]["ms_per_image_median"] - r["constant"]["ms_per_image_median"], 2)
        try:
            split = {}
            for opt in ("constant", "likelihood"):
                h.llm_rel_scores = opt
                h.num_llm_ranked_triples = 100 if opt == "likelihood" else 0
                split[opt] = _kernel_split(h, inputs)
            r["pass_device_us"] = {k: round(split["likelihood"][k] - split["constant"][k], 1) for k in split["constant"]}
        except Exception as e:  # noqa: BLE001  (the profiler is a diagnostic, not the measurement)
            r["pass_device_us"] = f"profiler unavailable: {e}"
        res.append(r)
        print("image", json.dumps(r), flush=True)
        del h
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "llm_rank_bench.json"))
    ap.add_argument("--image-steps", type=int, default=5)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--modes", default="fp32s,mixed")
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), image_c3=bench(a.image_steps, a.llm_layers, a.modes.split(",")))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
