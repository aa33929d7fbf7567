"""Per-image kernel table from ONE rocprofv3 kernel trace (rocpd sqlite) of `bench.py --steps K --warmup W`.

    rocprofv3 --kernel-trace -d DIR -- python bench.py --gpus 1 --steps 20 --warmup 5
    python tools/lt_gemm_trace_summary.py DIR/*/*_results.db 20 [out.csv]

An image's prompt pass is the only place the library's `Cijk_*` kernels run in the fp32s head, one dense burst per image with
the relation query and ~90 ms of decode steps between two bursts.  So the trace is cut where two consecutive `Cijk_*`
launches lie more than 3 ms apart; the last K windows [burst i, burst i + 1) are the K timed images (warm-up, capture and
setup come before them), and every kernel launched inside them is summed by name: calls and microseconds per image.
Prints the two figures DESIGN 21 tracks: the summed `Cijk_*` time and the `rmsnorm_split` time per image."""
import sqlite3
import sys


def main(db, steps, out=None):
    cur = sqlite3.connect(db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    start, end = ("start", "end") if "start" in cols else ("start_timestamp", "end_timestamp")
    rows = list(cur.execute(f"select name, {start}, {end} from kernels order by {start}"))
    cuts, last = [], None
    for name, s, _ in rows:
        if name.startswith("Cijk_"):
            if last is None or s - last > 3e6:
                cuts.append(s)
            last = s
    if len(cuts) < steps:
        sys.exit(f"only {len(cuts)} prompt-pass bursts in the trace, {steps} timed steps asked for")
    t0 = cuts[-steps]
    table = {}
    for name, s, e in rows:
        if s >= t0:
            c = table.setdefault(name, [0, 0.0])
            c[0] += 1
            c[1] += (e - s) / 1e3
    per = sorted(((n, c / steps, us / steps) for n, (c, us) in table.items()), key=lambda r: -r[2])
    tot = sum(r[2] for r in per)
    lines = ["kernel,calls_per_image,us_per_image,avg_us,pct"]
    for n, c, us in per:
        lines.append(f"{n.replace(',', ';')[:110]},{c:.2f},{us:.1f},{us / c:.2f},{100 * us / tot:.2f}")
    lines.append(f"TOTAL,{sum(r[1] for r in per):.1f},{tot:.1f},,100")
    if out:
        open(out, "w").write("\n".join(lines) + "\n")
    cijk = [r for r in per if r[0].startswith("Cijk_")]
    norm = [r for r in per if "rmsnorm_split" in r[0]]
    print(f"images {steps}  Cijk_us_per_image {sum(r[2] for r in cijk):.1f}  Cijk_calls_per_image {sum(r[1] for r in cijk):.1f}  "
          f"rmsnorm_split_us_per_image {sum(r[2] for r in norm):.1f}  all_kernels_us_per_image {tot:.1f}")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)
