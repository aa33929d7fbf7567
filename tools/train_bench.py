"""Times one training step (forward + backward of the summed loss) of the head behind a Llama-2-7B-width LLM, in the
two precisions of the gradient path:

    python tools/train_bench.py [--layers 32] [--steps 10] [--warmup 3] [--out profiles/train_bf16_bench.json]

  fp32   dtype='fp32', train_precision=None   the fp32 kernels of csrc/psg_train_bwd.hip, fp32 library GEMMs
  bf16   dtype='bf16', train_precision='bf16' csrc/psg_train_bf16.hip, bf16 library GEMMs, fp32 masters
(the row and pointwise kernels of both are the templates of csrc/psg_train_rows.h)

Shapes: the training golden T2's geometry (768 x 1024, 9 segments, its relations), synthetic weights, the LLM at
hidden 4096 / 32 heads / inter 11008 / vocab 32000.  Each precision runs in a process of its own (peak memory is per
process); per step the time is taken with device events around forward + backward after `--warmup` untimed steps, and
the median with min - max of `--steps` is reported, with torch's peak allocated memory."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_one(mode, layers, steps, warmup):
    import random

    import numpy as np
    import torch

    from openpsg_amd.config import PSGConfig, QFormerConfig, tiny_llm
    from openpsg_amd.head import RelationTransformerHeadV4
    from openpsg_amd.synthetic import make_train_scene
    from openpsg_amd.weights import make_weights_numpy
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "T2_train_768x1024_n9.npz"), allow_pickle=False))
    inputs = make_train_scene(tuple(int(v) for v in g["pad_hw"]), [int(c) for c in g["categories"]],
                              [tuple(int(v) for v in r) for r in g["gt_rels"]], seed=int(g["scene_seed"]))
    inputs["mask_features"] = inputs["mask_features"].cuda()
    inputs["gt_semantic_seg"] = [inputs["gt_semantic_seg"][0].cuda()]
    hidden, inter, vocab = 4096, 11008, 32000
    cfg = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(hidden, layers, inter, vocab), max_object_num=30)
    small = PSGConfig(qformer=QFormerConfig(vocab=512), llm=tiny_llm(256, 1, 512, 512), max_object_num=30)
    w = {k: v for k, v in make_weights_numpy(small, seed=3).items()                 # the head's own tensors (LLM-independent)
         if not k.startswith("language_model.") and not k.startswith("language_projection.")}
    dt = torch.float32 if mode == "fp32" else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s, sc=0.02: (torch.randn(*s, device="cuda", generator=gen) * sc).to(dt)   # noqa: E731
    llm = {"language_model.model.embed_tokens.weight": r(vocab, hidden), "language_model.lm_head.weight": r(vocab, hidden),
           "language_model.model.norm.weight": torch.ones(hidden, device="cuda")}
    for l in range(layers):
        p = f"language_model.model.layers.{l}."
        for n in "qkvo":
            llm[p + f"self_attn.{n}_proj.weight"] = r(hidden, hidden)
        llm[p + "mlp.gate_proj.weight"], llm[p + "mlp.up_proj.weight"] = r(inter, hidden), r(inter, hidden)
        llm[p + "mlp.down_proj.weight"] = r(hidden, inter)
        llm[p + "input_layernorm.weight"] = torch.ones(hidden, device="cuda")
        llm[p + "post_attention_layernorm.weight"] = torch.ones(hidden, device="cuda")
    head = RelationTransformerHeadV4(dtype=mode, device="cuda:0", qformer_vocab_size=512, llm_config=cfg.llm,
                                     llm_feature_size=hidden, tokenizers="word", max_object_num=30, train_dropout=True,
                                     train_precision=None if mode == "fp32" else "bf16")
    head.load_weights(w)
    with torch.no_grad():
        head.language_projection.weight.copy_(torch.randn(hidden, 768, generator=torch.Generator().manual_seed(2)) * 0.02)
    head.load_llm_weights(llm)
    del llm
    head.train(True)
    torch.cuda.reset_peak_memory_stats()
    times = []
    for it in range(warmup + steps):
        torch.manual_seed(5)
        random.seed(5)
        head.zero_grad(set_to_none=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = head(inputs)
        (out["binary_rel_cls_loss"] + out["rel_llm_loss"]).backward()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(a.elapsed_time(b))
    return dict(mode=mode, layers=layers, steps=steps, warmup=warmup, ms_median=statistics.median(times), ms_min=min(times),
                ms_max=max(times), peak_allocated_gb=torch.cuda.max_memory_allocated() / 2 ** 30,
                loss=float(out["binary_rel_cls_loss"].detach() + out["rel_llm_loss"].detach()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_bf16_bench.json"))
    ap.add_argument("--one", choices=["fp32", "bf16"], help="(internal) run one precision and print its JSON line")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(run_one(a.one, a.layers, a.steps, a.warmup)), flush=True)
        return
    results = []
    for mode in ("fp32", "bf16"):                               # a fresh process each: peak memory is per process
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, "--layers", str(a.layers), "--steps",
                            str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=900)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"train_bench: the {mode} run failed (exit {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]))
    with open(a.out, "w") as f:
        json.dump(dict(shapes="T2 geometry, Llama-2-7B width", results=results,
                       speedup=results[0]["ms_median"] / results[1]["ms_median"]), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
