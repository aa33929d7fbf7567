"""Which library kernel should run each split-fp16 product of the fp32s prompt pass.

For the eight prompt-pass shapes at BASELINE C3 - generic fp32 weights: 960 rows, (N, K') = (12288, 12288) q|k|v,
(4096, 12288) o, (22016, 12288) gate|up, (4096, 33024) down; fp16-valued weights: the two-plane operand, 1920 rows, K = 4096 /
11008 - list the library's candidates (ops.lt_gemm_candidates, up to 64 per problem) in every layout the engine can route
(whole; two column halves written in place; 2 / 3 / 6 K segments as one batched product where the reader sums slices) and time
each against the INCUMBENT, what the shape runs today (`llm._plan_split_mm` through torch.mm / torch.bmm):

  * random-normal operands split the way the engine splits them (ops.split_f16x3 / split_f16x2) - zeros flatter the clock;
    the weights of a shape rotate over copies that together exceed the 256 MB Infinity Cache, for both sides alike;
  * 3 warm-up + 20 timed launches per candidate, each timed by its own pair of HIP events, the incumbent launched in the SAME
    loop right behind it so both see the same clock state; median / min / max in us.  K-segment layouts are charged the
    reader's extra slice reads at 4 TB/s (as PSG_PLAN=measure does), the incumbent too;
  * a candidate whose result is not bit-identical over 10 repeats is rejected (atomics: tests/test_gpu_plans.py demands
    identical digests from two fresh processes);
  * ACCEPT (a `_LT_ALGO_TABLE` line is printed) only when the candidate's whole range lies below the incumbent's whole range.

One invocation, on the GPU, under a timeout of the caller's.  Every step's status is checked (a failed call raises) and the
script stops at the first failure: a library kernel that faults is a finding, not something to retry.

    python tools/lt_gemm_tune.py [--shapes generic,w16] [--timed 20] > profiles/lt_gemm_tune.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openpsg_amd import llm, ops  # noqa: E402

WS_BYTES = 128 << 20
MALL_BYTES = 256 << 20
#        name, rows, N, K (of the fp32 operand), planes, the reader sums slices
SHAPES = [("qkv", 960, 12288, 4096, 3, False), ("o", 960, 4096, 4096, 3, True), ("gate_up", 960, 22016, 4096, 3, False),
          ("down", 960, 4096, 11008, 3, True),
          ("qkv_w16", 1920, 12288, 4096, 2, False), ("o_w16", 1920, 4096, 4096, 2, True),
          ("gate_up_w16", 1920, 22016, 4096, 2, False), ("down_w16", 1920, 4096, 11008, 2, True)]


def operands(rows, N, K, planes, dev, gen):
    """(a3 fp16 [rows, K'], [w3 fp16 [N, K'], ...]) as the engine makes them from fp32 activations and weights."""
    if planes == 3:
        a3 = ops.split_f16x3(torch.randn((rows, K), device=dev, generator=gen))[0]
        mk = lambda: ops.split_f16x3(torch.randn((N, K), device=dev, generator=gen) / K ** 0.5, weights=True)[0]   # noqa: E731
    else:                                                      # [xh; xl] (2 x rows/2 rows) against an fp16-valued weight
        a3 = ops.split_f16x2(torch.randn((rows // 2, K), device=dev, generator=gen))[0].view(rows, K)
        mk = lambda: (torch.randn((N, K), device=dev, generator=gen) / K ** 0.5).half()                             # noqa: E731
    w0 = mk()
    copies = max(2, -(-MALL_BYTES // (w0.numel() * 2)) + 1)
    return a3, [w0] + [mk() for _ in range(copies - 1)]


def lt_launch(a3, w3, layout, index, ws, y):
    rows, N = a3.shape[0], w3.shape[0]
    if layout[0] == "kseg":
        P = layout[1]
        K = a3.shape[1] // P
        return ops.lt_gemm(a3.view(rows, P, K).permute(1, 0, 2), w3.view(N, P, K).permute(1, 0, 2), y, index, ws)
    parts = layout[1] if layout[0] == "cols" else 1
    h = N // parts
    fb = False
    for p in range(parts):
        fb |= ops.lt_gemm(a3, w3[p * h:(p + 1) * h], y[:, p * h:(p + 1) * h], index, ws)
    return fb


def lt_candidates(a3, w3, layout):
    rows, N = a3.shape[0], w3.shape[0]
    if layout[0] == "kseg":
        P = layout[1]
        K = a3.shape[1] // P
        return ops.lt_gemm_candidates(a3.view(rows, P, K).permute(1, 0, 2), w3.view(N, P, K).permute(1, 0, 2), None, WS_BYTES)
    if layout[0] == "cols":
        h = N // layout[1]
        y = torch.empty((rows, N), device=a3.device, dtype=torch.float32)
        return ops.lt_gemm_candidates(a3, w3[:h], y[:, :h], WS_BYTES)
    return ops.lt_gemm_candidates(a3, w3, None, WS_BYTES)


def charge_us(layout, rows, N):
    """The reader's extra slice reads of a K-segment layout at 4 TB/s."""
    return (layout[1] - 1) * rows * N * 4 / 4e6 if layout[0] == "kseg" else 0.0


def stats(ts, extra):
    ts = [t * 1e3 + extra for t in ts]
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="generic,w16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    version = ops.lt_gemm_version(dev)
    if version is None:
        sys.exit("lt_gemm_tune: " + ops.lt_gemm_error(dev))
    print(f"# {torch.cuda.get_device_name(0)}; GEMM library version {version}; torch {torch.__version__}; "
          f"{args.warmup} warm-up + {args.timed} timed launches, candidate and incumbent interleaved; us: median min max")
    print("# kernel names: the C entry points do not expose them; the kernel trace of bench.py names what a pinned line runs")
    ws = torch.empty(WS_BYTES, device=dev, dtype=torch.uint8)
    gen = torch.Generator(device=dev).manual_seed(0)
    want = args.shapes.split(",")
    ev = lambda: torch.cuda.Event(enable_timing=True)          # noqa: E731
    for name, rows, N, K, planes, k3 in SHAPES:
        if ("w16" if planes == 2 else "generic") not in want:
            continue
        a3, pool = operands(rows, N, K, planes, dev, gen)
        Kp = a3.shape[1]
        inc_plan = llm._plan_split_mm(rows, pool[0], k3=k3)
        inc_extra = charge_us(inc_plan, rows, N)
        layouts = [("whole",)]
        if N % 512 == 0 and N // 2 >= 2048:
            layouts.append(("cols", 2))
        if k3:
            layouts += [("kseg", p) for p in (2, 3, 6) if Kp % (64 * p) == 0]
        print(f"## {name}: rows={rows} N={N} K'={Kp} planes={planes} reader-sums-slices={k3}; incumbent {inc_plan} via torch; "
              f"{len(pool)} weight copies in rotation", flush=True)
        accepted = []
        for layout in layouts:
            cands = lt_candidates(a3, pool[0], layout)
            extra = charge_us(layout, rows, N)
            y = torch.empty((layout[1], rows, N) if layout[0] == "kseg" else (rows, N), device=dev, dtype=torch.float32)
            for rank, (index, need) in enumerate(cands):
                # bit-reproducibility first: 10 repeats against the first result
                if lt_launch(a3, pool[0], layout, index, ws, y):
                    sys.exit(f"lt_gemm_tune: listed solution {index} was not found again for {name} {layout}")
                first = y.clone()
                same = True
                for _ in range(args.repeats - 1):
                    y.fill_(float("nan"))
                    lt_launch(a3, pool[0], layout, index, ws, y)
                    same = same and torch.equal(y, first)
                torch.cuda.synchronize()
                tc, ti = [], []
                evs = []
                for i in range(args.warmup + args.timed):
                    w3 = pool[i % len(pool)]
                    e = [ev(), ev(), ev(), ev()]
                    e[0].record()
                    lt_launch(a3, w3, layout, index, ws, y)
                    e[1].record()
                    e[2].record()
                    llm._split_mm(a3, w3, inc_plan)
                    e[3].record()
                    evs.append(e)
                torch.cuda.synchronize()                       # (a fault surfaces here and ends the script)
                for e in evs[args.warmup:]:
                    tc.append(e[0].elapsed_time(e[1]))
                    ti.append(e[2].elapsed_time(e[3]))
                c, inc = stats(tc, extra), stats(ti, inc_extra)
                verdict = "REJECT not bit-reproducible" if not same else ("ACCEPT" if c[2] < inc[1] else "-")
                print(f"{name:12s} {str(layout):12s} #{rank:<2d} solution {index:<7d} ws {need:>10d} v{version}  "
                      f"{c[0]:7.1f} {c[1]:7.1f} {c[2]:7.1f}   incumbent {inc[0]:7.1f} {inc[1]:7.1f} {inc[2]:7.1f}   {verdict}",
                      flush=True)
                if verdict == "ACCEPT":
                    accepted.append((c[0], layout, index, need, c, inc))
            del y
        if accepted:
            # one summed result first, then fewer slices for the reader, then the median
            accepted.sort(key=lambda t: (t[1][1] if t[1][0] == "kseg" else 1, t[0]))
            _, layout, index, need, c, inc = accepted[0]
            lo, hi = rows, rows + 1                            # a line holds for the row count it was tuned at
            print(f"TABLE ({N}, {Kp}, {planes}, {k3}): [({lo}, {hi}, {index}, {version}, {layout}, {need})],   "
                  f"# {name}: {c[1]:.0f}-{c[2]:.0f} us against {inc[1]:.0f}-{inc[2]:.0f} ({inc_plan})", flush=True)
        else:
            print(f"TABLE none for {name}: no candidate's range lies wholly below the incumbent's", flush=True)
        del a3, pool
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
