"""Headline A/B of this tree against another checkout (the parent commit, built, in its own directory) on ONE box:
plain `bench.py` runs interleaved parent, this, parent, this, ... - each a fresh process, one at a time, under its own
time limit - so both trees see the same box, clock state and neighbours.

    python tools/bench_ab.py --parent DIR [--runs 7] [--out profiles/x.json] [-- extra bench.py arguments]

The gain criterion of DESIGN 21: every run of this tree below every run of the parent AND the difference of the medians at
least three times the parent's own min-max range in the session.  Stops at the first run that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(tree, extra, limit):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"] + extra, cwd=tree,
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit(f"bench.py in {tree} ended with {r.returncode}:\n{r.stderr[-1500:]}")
    return float(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--limit", type=int, default=420, help="seconds per bench.py run")
    ap.add_argument("--out", default=None)
    ap.add_argument("extra", nargs="*")
    a = ap.parse_args()
    import torch
    from openpsg_amd import ops
    box = f"{os.uname().nodename}: {torch.cuda.get_device_name(0)}"
    version = ops.lt_gemm_version("cuda:0")
    parent, pr = [], []
    for i in range(a.runs):
        parent.append(one(os.path.abspath(a.parent), a.extra, a.limit))
        pr.append(one(REPO, a.extra, a.limit))
        print(f"run {i}: parent {parent[-1]:.3f}  this {pr[-1]:.3f} ms per image", flush=True)
    rng = max(parent) - min(parent)
    diff = statistics.median(parent) - statistics.median(pr)
    res = {"bench": "bench.py --gpus 1 --steps 20 --warmup 5 " + " ".join(a.extra), "box": box, "gemm_library_version": version,
           "order": "parent, this, parent, this, ...", "parent_ms": parent, "this_ms": pr,
           "parent_median": statistics.median(parent), "this_median": statistics.median(pr),
           "parent_range_ms": round(rng, 3), "median_gain_ms": round(diff, 3),
           "every_run_below_every_parent_run": max(pr) < min(parent),
           "gain_at_least_3x_parent_range": diff >= 3 * rng}
    res["counts_as_a_gain"] = res["every_run_below_every_parent_run"] and res["gain_at_least_3x_parent_range"]
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    main()
