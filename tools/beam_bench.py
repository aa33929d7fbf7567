"""Cost of llm_beam_width against the trie pass that yields the same number of scored triples, on one MI355X.

BASELINE C3 (1024x1024, 50 objects, top-20 pairs) through head(inputs) with a 32-layer Llama-2-7B-shaped LLM of seeded
weights.  ONE head object per mode is toggled between the variants, and the variants alternate image by image inside the
timed window (tools/constrained_bench.py's method), so that every variant sees the same weights, the same process and the
same neighbours on the machine.  All variants run llm_decode='constrained' + llm_rel_scores='likelihood':

  floor          llm_beam_width=1, num_llm_ranked_triples=0: one scored triple per pair (20)
  beam_B         llm_beam_width=B in {3, 5, 8}: B scored triples per pair, max_depth forwards of 20 x B rows
  trie_pass_B    the yardstick: llm_beam_width=1, num_llm_ranked_triples=20 (B - 1) - the same number of scored triples the
                 way the head produced them before the option, one forward over 20 x n_int rows on the library

Modes: fp32s with llm_batch_split_gemm 'library' and 'own', mixed, mixed + llm_weight_quant='fp8' +
llm_batch_weight_stream='quantised'.

ms per image = host clock around head(inputs) ending in a device synchronise; median (min - max) over --image-steps.

    python tools/beam_bench.py [--out profiles/beam_bench.json] [--image-steps 7] [--llm-layers 32] [--modes ...]
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

WIDTHS = (3, 5, 8)
MODES = {
    "fp32s_library": dict(dtype="fp32s", llm_batch_split_gemm="library"),
    "fp32s_own": dict(dtype="fp32s", llm_batch_split_gemm="own"),
    "mixed": dict(dtype="mixed"),
    "mixed_fp8_quantised": dict(dtype="mixed", llm_weight_quant="fp8", llm_batch_weight_stream="quantised"),
}


def _variants(K):
    v = {"floor": (1, 0)}
    for B in WIDTHS:
        v[f"beam_{B}"] = (B, 0)
        v[f"trie_pass_{B}"] = (1, K * (B - 1))
    return v


def _set(h, width, ranked):
    h.llm_beam_width, h.num_llm_ranked_triples = width, ranked


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
        opts = dict(MODES[mode])
        cfg = PSGConfig(qformer=QFormerConfig(), llm=llm, max_object_num=50)
        w = make_weights_device(cfg, 0, dev, llm_dtype=torch.float32)
        h = RelationTransformerHeadV4(device=str(dev), tokenizers="word", max_object_num=50, llm_config=llm,
                                      on_parse_error="skip", llm_decode="constrained", llm_rel_scores="likelihood", **opts)
        h.load_weights(w)
        del w
        torch.cuda.empty_cache()
        trie = h.relation_trie()
        K = cfg.num_selected
        variants = _variants(K)
        r = dict(model="llama-2-7b", mode=mode, options=opts, layers=layers, pairs=K, trie_nodes=trie.n_int,
                 trie_depth=trie.max_depth, beam_rows={B: K * B for B in WIDTHS}, trie_pass_rows=K * trie.n_int)
        times, triples = {v: [] for v in variants}, {}
        for v, (width, ranked) in variants.items():                   # warm-up: graphs, prompt tables, library plans
            _set(h, width, ranked)
            for _ in range(2):
                h(inputs)
        for _ in range(steps):
            for v, (width, ranked) in variants.items():               # alternate: one image of each variant per round
                _set(h, width, ranked)
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
        for B in WIDTHS:                                              # the beam's range wholly below its yardstick's?
            b, y = r[f"beam_{B}"], r[f"trie_pass_{B}"]
            r[f"beam_{B}_wholly_below_trie_pass"] = bool(b["ms_per_image_max"] < y["ms_per_image_min"])
            r[f"beam_{B}_same_triples_as_trie_pass"] = bool(b["triples"] == y["triples"])
        res.append(r)
        print("image", json.dumps(r), flush=True)
        del h
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "beam_bench.json"))
    ap.add_argument("--image-steps", type=int, default=7)
    ap.add_argument("--llm-layers", type=int, default=32)
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), image_c3=bench(a.image_steps, a.llm_layers, a.modes.split(",")))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
