"""Cost of the LLM stage with and without llm_decode='constrained'  on one MI355X.

BASELINE C3 (1024x1024, 50 objects, top-20 pairs, 16 new tokens) through head(inputs) with a 32-layer Llama-2-7B-shaped
LLM of seeded weights, in fp32s and mixed.  ONE head object per mode is toggled between the variants, and the variants
alternate image by image inside the timed window, so that every variant sees the same weights, the same process and the
same neighbours on the machine:

  greedy_suppressed      option off, EOS suppressed: 15 decode steps behind the prompt pass (the yardstick)
  greedy_natural         option off, natural EOS: early-exit chunks with a read-back each
  constrained_constant   'constrained', llm_rel_scores='constant'
  constrained_likelihood 'constrained', llm_rel_scores='likelihood', num_llm_ranked_triples=0 (no trie pass)
  greedy_likelihood      option off (EOS suppressed), llm_rel_scores='likelihood', N = 0: the trie pass scores the triples

ms per image = host clock around head(inputs) ending in a device synchronise; median (min - max) over --image-steps.

    python tools/constrained_bench.py [--out profiles/constrained_bench.json] [--image-steps 7] [--llm-layers 32]
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

VARIANTS = {
    "greedy_suppressed": dict(llm_decode="greedy", suppress_eos=True, llm_rel_scores="constant"),
    "greedy_natural": dict(llm_decode="greedy", suppress_eos=False, llm_rel_scores="constant"),
    "constrained_constant": dict(llm_decode="constrained", suppress_eos=False, llm_rel_scores="constant"),
    "constrained_likelihood": dict(llm_decode="constrained", suppress_eos=False, llm_rel_scores="likelihood"),
    "greedy_likelihood": dict(llm_decode="greedy", suppress_eos=True, llm_rel_scores="likelihood"),
}


def _set(h, opts):
    for k, v in opts.items():
        setattr(h, k, v)
    h.num_llm_ranked_triples = 0


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
                                      on_parse_error="skip")
        h.load_weights(w)
        del w
        torch.cuda.empty_cache()
        trie = h.relation_trie()
        r = dict(model="llama-2-7b", mode=mode, layers=layers, max_new_tokens=cfg.max_new_tokens,
                 trie_steps=trie.max_depth + 1, decode_forwards=dict(greedy_suppressed=cfg.max_new_tokens - 1,
                                                                     constrained=trie.max_depth))
        times, triples = {v: [] for v in VARIANTS}, {}
        for v, opts in VARIANTS.items():                              # warm-up: graphs, prompt tables, library plans
            _set(h, opts)
            for _ in range(2):
                h(inputs)
        for _ in range(steps):
            for v, opts in VARIANTS.items():                          # alternate: one image of each variant per round
                _set(h, opts)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = h(inputs)
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) * 1e3)
                triples[v] = len(out["rel_pred"])
        for v, ts in times.items():
            s = sorted(ts)
            r[v] = dict(ms_per_image_median=round(s[len(s) // 2], 2), ms_per_image_min=round(s[0], 2),
                        ms_per_image_max=round(s[-1], 2), ms_per_image_all=[round(t, 2) for t in ts], triples=triples[v])
        y, c, cl, gl = (r[v] for v in ("greedy_suppressed", "constrained_constant", "constrained_likelihood",
                                       "greedy_likelihood"))
        r["accept_constrained_below_yardstick"] = bool(c["ms_per_image_median"] < y["ms_per_image_median"]
                                                       and c["ms_per_image_max"] < y["ms_per_image_min"])
        r["accept_scored_below_trie_pass"] = bool(cl["ms_per_image_median"] < gl["ms_per_image_median"])
        res.append(r)
        print("image", json.dumps(r), flush=True)
        del h
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "constrained_bench.json"))
    ap.add_argument("--image-steps", type=int, default=7)
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
