"""LMM relation decode engine: batched greedy Llama decode for the K selected pairs.

Replaces the serial loop at relation_transformer_head_v4.py:293-312 (one HF `generate` per pair,
batch 1, fp32 weights re-streamed ~17 times per pair) with ONE batched prefill + (max_new-1)
batched decode steps, so the LLM weights stream from HBM once per step for all K pairs.

Layout decisions (all per-pair results are independent of K and of the other pairs):
  * the reference left-pads prompts, which puts pad tokens in the MIDDLE of the sequence (after the
    32 visual rows, V4:296-301) and relies on HF's additive mask + cumsum positions.  Here every
    pair's sequence is COMPACTED: slots [0, 32+n_k) hold its tokens, position == slot
    (== cumsum(mask)-1, probe-verified in SURVEY Appendix B), so the only mask is causal;
  * prefill runs on a fixed [K, 32+T_p] token grid (rows beyond a pair's length carry pos = -1 and
    are skipped by the kernels), decode on [K] rows: static shapes, no host sync, graph-capturable;
  * KV cache [layers][K, kv_heads, ctx, 128] in the activation dtype (kv_heads = heads unless grouped-query);
  * the greedy step (argmax, EOS bookkeeping, next ids, positions) is a device kernel.

Dense projections go through torch (`F.linear` -> hipBLASLt) or, for the decode steps, through the
hand-written weight-streaming kernel in libpsg_hip.so; RMSNorm, rotary+KV write, attention, SwiGLU
gate and the greedy step are HIP kernels.
"""
from __future__ import annotations

import collections
import os
import sys

import torch
import torch.nn.functional as F

from . import _lib, ops
from ._lib import PsgHipError
from .config import PSGConfig
from .llm_matrix import INT4_STREAM_OFF, W4_STREAM_AS_FP8, complete, dense_matrix, load_bf16_matrix, load_matrix  # noqa: F401  (the tables: also llm.<name>)


# How the library runs one split-fp16 product [rows, K'] x [N, K']^T -> fp32: whole, or cut into column / row parts written
# in place, or as a batched product over K segments.  hipBLASLt's pick for a shape is a heuristic, and at K' = 3K it is erratic
# (Llama-2-7B gate|up at 960 rows: 694 us whole, 480 us as two column halves; tools/split_gemm_bench.py), so a cut pays.
# The forms are NOT numerically equivalent (K segments change the fp32 summation order, parts can make the library pick
# another kernel), so the choice must not depend on anything a process measures: it comes from the FIXED table below - the
# measured winners for the Llama-2-7B shapes on gfx950 (gpurun_out/plans_run*.txt of round 6: two runs of the old per-process
# timing disagreed on 3 of 12 shapes at near-ties, which is exactly what the table retires).  Every rank, every box and every
# process then runs the same arithmetic on the same input (tests/test_gpu_plans.py: two fresh processes, identical logits
# and tokens).  `PSG_PLAN=measure` brings the timing back as a TOOL: it times the candidates and prints table lines.
#   key: (N, K', result is fp32, the reader sums [P, rows, N] slices)  ->  [(rows from, rows below, plan), ...]; else whole
_SPLIT_PLAN_TABLE = {
    # fp32s prompt pass, generic fp32 weights: [xh | xh | xl] . [wh | wl | wh]^T over K' = 3K (960 rows at BASELINE C3)
    (22016, 12288, True, False): [(512, 2048, ("cols", 2))],      # gate|up: 702-709 us whole, 466-494 as two column halves
    (4096, 33024, True, True): [(512, 2048, ("kseg", 6))],        # down: 335-347 us whole, 283-293 as six K segments
    # fp32s prompt pass, fp16-valued weights: the two-plane operand [xh; xl] (2 x rows) against the fp16 weight over K
    (22016, 4096, True, False): [(1024, 6144, ("cols", 2))],      # gate|up: 375 us whole, 326-332 in halves (1920 rows)
    # 16-bit prompt pass of several images (forward_batch: 1920 / 3840 rows; 7680: whole)
    (22016, 4096, False, False): [(1024, 6144, ("cols", 2))],     # 598-604 us whole, 534-539 in halves (3840 rows)
}
_SPLIT_PLANS: dict = {}                                            # PSG_PLAN=measure only: what this process measured


def _plan_measuring() -> bool:
    return os.environ.get("PSG_PLAN", "") == "measure"


def _split_mm(a3, w3, plan=None, out_dtype=torch.float32):
    """a3 [rows, K'] . w3 [N, K']^T -> [rows, N] through the library, whole or in the parts `plan` names.
    out_dtype fp32: the split-fp16 products of the fp32s mode; None: the operands' 16-bit type (the 16-bit prompt pass)."""
    kw = {} if out_dtype is None else {"out_dtype": out_dtype}
    if plan is None or plan[0] == "whole":
        return torch.mm(a3, w3.t(), **kw)
    if plan[0] == "lt":                                        # the library called natively, algorithm pinned (`_LtRoute`)
        return plan[3].mm(a3, w3, plan)
    if plan[0] == "kseg":                                      # P segments of K' as ONE batched product: [P, rows, N] slices
        rows, N, P = a3.shape[0], w3.shape[0], plan[1]
        K = a3.shape[1] // P
        return torch.bmm(a3.view(rows, P, K).permute(1, 0, 2), w3.view(N, P, K).permute(1, 2, 0), **kw)
    rows, N = a3.shape[0], w3.shape[0]
    y = torch.empty((rows, N), device=a3.device, dtype=out_dtype or a3.dtype)
    kind, parts = plan
    if kind == "cols":                                         # ldc = N: the parts land where the whole product puts them
        h = N // parts
        for p_ in range(parts):
            torch.mm(a3, w3[p_ * h:(p_ + 1) * h].t(), out=y[:, p_ * h:(p_ + 1) * h], **kw)
    else:
        h = -(-rows // (16 * parts)) * 16
        for r0 in range(0, rows, h):
            torch.mm(a3[r0:r0 + h], w3.t(), out=y[r0:r0 + h], **kw)
    return y


# WHICH library kernel runs a split-fp16 product of the prompt pass.  torch.mm / torch.bmm take the library's first
# heuristic choice for a shape, and the table above steers that heuristic by re-cutting the product; psg_lt_gemm calls the
# library natively with the algorithm PINNED by its solution index instead (ops.lt_gemm).  A line is a measured
# winner of tools/lt_gemm_tune.py: it enters only when the candidate's range of times lies wholly below the range of what
# the shape runs today (the acceptance rule of DESIGN 14 / 17) and its result was bit-identical over 10 repeats.  A solution
# index means something only within one library version: a line whose version is not the running library's is ignored (the
# shape keeps its `_SPLIT_PLAN_TABLE` route) and `lt_gemm_pinned` says so.  Like the table above, a pure function of the
# shape: no process measures anything.
#   key: (N, K', planes of the operand, the reader sums [P, rows, N] slices)
#        ->  [(rows from, rows below, solution index, library version, layout, workspace bytes), ...]  (a line holds for
#        the row count it was tuned at: which solutions the library lists, and how they rank, changes with the rows)
#   layout: ("whole",) one [rows, N] result (a split-K algorithm sums through the workspace); ("cols", P) P column parts
#   written in place (ldy = N); ("kseg", P) P segments of K' as one batched product, [P, rows, N] slices for the reader
# profiles/lt_gemm_tune.txt (library version 100000; eight shapes, up to 64 candidates per layout, two runs - a line is kept
# only when BOTH accepted it): q|k|v and down keep their `_SPLIT_PLAN_TABLE` route (the first choice is the fastest whole
# q|k|v, nothing beats down's six segments), and so does every two-plane shape (fp16-valued weights, 1920 rows)
_LT_ALGO_TABLE: dict = {
    # fp32s prompt pass, generic fp32 weights, 960 rows at BASELINE C3 (us: range of the candidate against the incumbent's)
    (22016, 12288, 3, False): [(960, 961, 625805, 100000, ("cols", 2), 0)],      # gate|up: 435-470 against 474-514 (two halves)
    (4096, 12288, 3, True): [(960, 961, 625813, 100000, ("kseg", 2), 0)],        # o: 96-105 against 105-113 (whole)
}


class _LtRoute:
    """The lines of `_LT_ALGO_TABLE` that hold for the library this process runs, and the one workspace their algorithms
    share (allocated here, once, outside any graph: captured launches replay against its address)."""

    def __init__(self, device, table=None):
        self.device = torch.device(device)
        self.lines, self.stale, self.fell_back = {}, [], []
        table = _LT_ALGO_TABLE if table is None else table
        self.version = ops.lt_gemm_version(self.device) if table and self.device.type == "cuda" else None
        self.error = None if self.version is not None or not table else (ops.lt_gemm_error(self.device) or "no GPU")
        ws = 0
        for key, rules in table.items():
            for lo, hi, index, version, layout, ws_bytes in rules:
                if self.version is None:
                    continue
                if version != self.version:
                    self.stale.append((key, version))
                    continue
                self.lines.setdefault(key, []).append((lo, hi, int(index), tuple(layout)))
                ws = max(ws, int(ws_bytes))
        self.workspace = torch.empty(ws, device=self.device, dtype=torch.uint8) if ws else None

    def plan(self, rows, N, K, planes, k3):
        """("lt", solution index, layout, self) - a plan of `_split_mm` - for a shape the table pins, else None."""
        for lo, hi, index, layout in self.lines.get((int(N), int(K), int(planes), bool(k3)), ()):
            if lo <= rows < hi:
                return ("lt", index, layout, self)
        return None

    def mm(self, a3, w3, plan):
        """a3 [rows, K'] . w3 [N, K']^T -> fp32 [rows, N] (or [P, rows, N] slices) on the pinned algorithm."""
        _, index, layout, _ = plan
        rows, N = a3.shape[0], w3.shape[0]
        if layout[0] == "kseg":
            P = layout[1]
            K = a3.shape[1] // P
            y = torch.empty((P, rows, N), device=a3.device, dtype=torch.float32)
            fb = ops.lt_gemm(a3.view(rows, P, K).permute(1, 0, 2), w3.view(N, P, K).permute(1, 0, 2), y, index, self.workspace)
        else:
            y = torch.empty((rows, N), device=a3.device, dtype=torch.float32)
            parts = layout[1] if layout[0] == "cols" else 1
            h = N // parts
            fb = False
            for p_ in range(parts):
                fb |= ops.lt_gemm(a3, w3[p_ * h:(p_ + 1) * h], y[:, p_ * h:(p_ + 1) * h], index, self.workspace)
        if fb and (N, a3.shape[1], index) not in self.fell_back:
            self.fell_back.append((N, a3.shape[1], index))
        return y

    @property
    def pinned(self):
        """(table lines in force, why the others are not - '' when every line is)."""
        why = []
        if self.error:
            why.append(f"library not usable: {self.error}")
        if self.stale:
            why.append(f"{len(self.stale)} line(s) tuned for another library version than {self.version}: "
                       + ", ".join(f"{k} @ {v}" for k, v in self.stale))
        if self.fell_back:
            why.append("solution not among the library's candidates, its first choice ran: "
                       + ", ".join(f"(N={n}, K'={k}) #{i}" for n, k, i in self.fell_back))
        return sum(len(v) for v in self.lines.values()), "; ".join(why)


def _plan_split_mm(rows, w3, out_dtype=torch.float32, k3=False, pool=None):
    """The form the library product of this shape runs in: a pure function of the shape (`_SPLIT_PLAN_TABLE`; 'whole' for
    every shape the table does not name), unless PSG_PLAN=measure."""
    if _plan_measuring():
        return _measure_split_plan(rows, w3, out_dtype, k3, pool)
    N, K3 = w3.shape
    for lo, hi, plan in _SPLIT_PLAN_TABLE.get((int(N), int(K3), out_dtype == torch.float32, bool(k3)), ()):
        if lo <= rows < hi:
            return plan
    return ("whole",)


def _measure_split_plan(rows, w3, out_dtype=torch.float32, k3=False, pool=None):
    """PSG_PLAN=measure (a tool, not the product path: its result depends on timing noise).
    The fastest of {whole, 2 / 3 column parts, 2 / 3 / 4 row parts} for this shape, timed on the device (7 runs each,
    minimum); a cut must win by 5 % to be taken.  Cached per process; prints the line `_SPLIT_PLAN_TABLE` would carry.
    k3: the caller's reader can sum slices (psg_rmsnorm_split) - 3 / 6 / 12 segments of K' as ONE batched product with a
    [P, rows, N] result are candidates too (P x the tiles: down at 960 rows 331 us whole, 303 as 3, 247 as 6 slices; o
    105 -> 98); the reader's extra slice reads are charged at 4 TB/s.
    pool: the other weights of this shape (the layers'): timed in rotation, so that a weight small enough for the
    Infinity Cache is as cold as it is in the pass itself."""
    N, K3 = w3.shape
    key = (int(rows), int(N), int(K3), w3.device.index or 0, str(out_dtype), bool(k3), str(w3.dtype))
    plan = _SPLIT_PLANS.get(key)
    if plan is not None:
        return plan
    if rows < 128 or torch.cuda.is_current_stream_capturing():
        return ("whole",)                                      # (not cached while capturing: planned at the next eager use)
    cands = [("whole",)]
    cands += [("cols", p_) for p_ in (2, 3) if N % (256 * p_) == 0 and N // p_ >= 2048]
    cands += [("rows", p_) for p_ in (2, 3, 4) if rows >= 128 * p_]
    if k3 and out_dtype == torch.float32:
        cands += [("kseg", p_) for p_ in (3, 6, 12) if K3 % (64 * p_) == 0]
    # (drain the device first: the timing loop is EAGER library work, and an eager library GEMM beside one inside another
    # slot's replaying graph is the combination that hung the GPU in round 4, tools/inflight_stress.py)
    torch.cuda.synchronize(w3.device)
    a3 = torch.randn((rows, K3), device=w3.device, generator=torch.Generator(device=w3.device).manual_seed(0)).to(w3.dtype)
    best, best_t, whole_t = cands[0], None, None
    pool = [w_ for w_ in (pool or [w3]) if w_.shape == w3.shape and w_.dtype == w3.dtype] or [w3]
    for c in cands:
        ts = []
        for i in range(9):
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()
            _split_mm(a3, pool[i % len(pool)], c, out_dtype)
            e_.record()
            e_.synchronize()
            if i >= 2:
                ts.append(s_.elapsed_time(e_))
        t = min(ts)
        if c[0] == "kseg":
            t += (c[1] - 1) * rows * N * 4 / 4e9               # ms: the reader sums c[1] slices instead of reading one
        if c[0] == "whole":
            whole_t = best_t = t
        elif t < best_t and t < 0.95 * whole_t:
            best, best_t = c, t
    _SPLIT_PLANS[key] = best
    print(f"[psg plan] ({N}, {K3}, {out_dtype == torch.float32}, {bool(k3)}): rows={rows} -> {best}  # {best_t * 1e3:.0f} us "
          f"(whole {whole_t * 1e3:.0f} us)", file=sys.stderr, flush=True)
    return best


# Decode steps with 33..160 rows (several images' pairs decoded together, head.forward_batch): the library GEMM against the
# variants of psg_batch_gemm (slab height x range mode) per (rows, N, K).  'own' hands fp32 slices to the consumer where 'lib'
# hands a 16-bit-rounded result, so - like the split products above - the choice is a FIXED table of the measured winners at
# the Llama-2-7B shapes (COLD weights, the consumer's slice sums charged to the variants; profiles/r05_batch_gemm_ab.txt,
# gpurun_out/plans_run*.txt of round 6), never a per-process measurement.  At 160 rows the library streams o / down at
# 1.0-1.3 TB/s and wins on gate|up; at 40 rows psg_batch_gemm wins everywhere but the lm_head.
#   key: (N, K) -> [(rows from, rows below, plan), ...]; anything else: the library
_BATCH_PLAN_TABLE = {
    (12288, 4096): [(33, 49, ("own", 128, 2))],                                        # q|k|v: 80 / 160 rows library (32 / 40 us)
    (4096, 4096): [(33, 49, ("own", 128, 1)), (113, 161, ("own", 128, 1))],            # o: 80 rows library 22 us; 160: 29 vs 31
    (22016, 4096): [(33, 49, ("own", 128, 2))],                                        # gate|up
    (4096, 11008): [(33, 113, ("own", 128, 1)), (113, 161, ("own", 256, 1))],          # down: 160 rows 42 us vs library 72
}
_BATCH_PLANS: dict = {}                                            # PSG_PLAN=measure only


def _plan_batch_mm(x, pool):
    if _plan_measuring():
        return _measure_batch_plan(x, pool)
    w, rows = pool[0], int(x.shape[0])
    for lo, hi, plan in _BATCH_PLAN_TABLE.get((int(w.shape[0]), int(w.shape[1])), ()):
        if lo <= rows < hi:
            return plan
    return ("lib",)


def _measure_batch_plan(x, pool):
    """PSG_PLAN=measure (a tool): library vs the psg_batch_gemm variants, timed once per process on COLD weights (the layers'
    own weights of that shape in rotation) with a psg_reduce_partials pass charged to the variants."""
    w = pool[0]
    key = (int(x.shape[0]), int(w.shape[0]), int(w.shape[1]), str(x.dtype), str(w.dtype), w.device.index or 0)
    plan = _BATCH_PLANS.get(key)
    if plan is not None:
        return plan
    if torch.cuda.is_current_stream_capturing():
        return ("lib",)
    torch.cuda.synchronize(w.device)                           # (as in _measure_split_plan: no eager library work beside a replaying graph)
    cands = [("lib",)] + [("own", bn, mode) for bn in (256, 128) for mode in (1, 2)]
    best, best_t = cands[0], None
    for c in cands:
        if c[0] == "own":
            try:
                ops.batch_gemm(x, w, c[1], c[2])
            except PsgHipError:
                continue
        ts = []
        for i in range(8):                                     # a sample = 4 launches back to back on 4 different weights
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()
            for j in range(4):
                wi = pool[(4 * i + j) % len(pool)]
                if c[0] == "lib":
                    F.linear(x, wi)
                else:
                    ops.batch_gemm(x, wi, c[1], c[2]).reduce(x.dtype)
            e_.record()
            e_.synchronize()
            if i >= 2:
                ts.append(s_.elapsed_time(e_) / 4)
        t = sorted(ts)[len(ts) // 2]
        if best_t is None or t < best_t * (0.97 if best[0] == "lib" else 1.0):
            best, best_t = c, t
    _BATCH_PLANS[key] = best
    print(f"[psg plan] decode projection ({key[1]}, {key[2]}): rows={key[0]} -> {best}  # {best_t * 1e3:.0f} us", file=sys.stderr,
          flush=True)
    return best


# Decode steps with 33..160 rows over a QUANTISED matrix, engine option batch_quant_stream: psg_batch_gemm_q.hip
# streams the bytes / nibbles where the steps above run on the dense W'.  Like _BATCH_PLAN_TABLE a FIXED table, never a
# per-process measurement: a listed row range sends a measured loser (tools/batch_quant_bench.py: the stream's range of
# times not wholly below the dense path's) back to the dense path; a shape that is not listed streams.
#   key: (format 'fp8' / 'mxfp4', form 'single' / 'pair', N, K) -> [(rows from, rows below), ...]
# resident='quantised' never consults it: there the alternative is the expansion plus the dense product.
# Measured at the Llama-2-7B shapes and 40 / 80 / 160 rows = 2 / 3 / 5 x tiles (profiles/batch_quant_bench.json; the row
# ranges are those of the tile counts: 33..64, 65..96, 97..160).  The pair form (fp32s, against the library SGEMM on fp32
# W') wins by 1.08-3.9 x everywhere but o in fp8 at 40 rows (level).  The single form meets 2-byte paths that stream at
# 2-3 TB/s and is matrix-core bound from 80 rows on: it keeps q|k|v (and mxfp4 gate|up) up to 64 rows, down from 97 rows
# (mxfp4: up to 64 as well) and the lm_head up to 96 rows (fp8: 65..96).
_BATCH_QUANT_DENSE: dict = {
    ("fp8", "single", 12288, 4096): [(65, 161)],               # q|k|v: 31.2 / 42.0 us against the library's 29.1 / 37.3
    ("fp8", "single", 4096, 4096): [(33, 161)],                # o: 11.3 / 25.2 / 20.8 against 10.0 / 16.6 / 19.1
    ("fp8", "pair", 4096, 4096): [(33, 65)],                   # o, 40 rows: 24.9 (24.3-25.1) against 24.9 (24.0-26.4): overlap
    ("fp8", "single", 22016, 4096): [(33, 161)],               # gate|up, 40 rows: 37.2 (36.3-40.7) against 39.6 (38.9-42.2): overlap
    # down, 40 rows: 19.8 (19.4-20.5) against 20.8 (20.5-21.0): overlap.  65..96 rows (both formats): 2.6 us ahead per launch,
    # but a `mixed` step of 4 images in which down was the only matrix that streamed ran 0.4-1.2 ms per batch BEHIND the
    # option-off step (mxfp4: disjoint ranges; DESIGN 16, whole step)
    ("fp8", "single", 4096, 11008): [(33, 97)],
    ("fp8", "single", 32000, 4096): [(33, 65), (97, 161)],     # lm_head: 49.5 (48.2-52.6) against 51.7: overlap; 160 rows: 75.3 against 62.2
    ("mxfp4", "single", 12288, 4096): [(65, 161)],
    ("mxfp4", "single", 4096, 4096): [(33, 161)],
    ("mxfp4", "single", 22016, 4096): [(65, 161)],
    ("mxfp4", "single", 4096, 11008): [(65, 97)],
    ("mxfp4", "single", 32000, 4096): [(97, 161)],
}


def _batch_quant_route(fmt, form, N, K, rows, table=None):
    """'stream' or 'dense' for a decode projection of `rows` rows over a quantised [N, K] matrix."""
    for lo, hi in (_BATCH_QUANT_DENSE if table is None else table).get((fmt, form, int(N), int(K)), ()):
        if lo <= rows < hi:
            return "dense"
    return "stream"


# Decode steps with 33..160 rows of an fp32s engine over an UNQUANTISED matrix, engine option batch_split_gemm:
# psg_batch_gemm_s.hip runs the split products where the steps above run the library SGEMM (generic fp32 weights) or the
# stacked-plane fp16 product (fp16-valued weights).  A FIXED table like _BATCH_QUANT_DENSE: a listed row range sends a
# measured loser (tools/batch_split_bench.py: the kernel's range of times not wholly below the library path's) back to
# the library; a shape that is not listed takes the kernel.
#   key: (form 'w16' / 'w32', N, K) -> [(rows from, rows below), ...]
# Measured at the Llama-2-7B shapes and 40 / 80 / 160 rows = 2 / 3 / 5 x tiles (profiles/batch_split_bench.json; the row
# ranges are those of the tile counts: 33..64, 65..96, 97..160; us per launch, median (min-max), own against library).  The
# w32 form (against the SGEMM on fp32 W) wins by 1.05-2.0 x everywhere but q|k|v and o at 40 rows.  The w16 form meets a
# library product that streams 2 bytes per weight as well: it keeps q|k|v and down at every row count, o at 80 rows and
# the lm_head at 40.
_BATCH_SPLIT_LIBRARY: dict = {
    ("w32", 12288, 4096): [(33, 65)],                          # q|k|v, 40 rows: 49.8 (46.7-57.3) against 58.9 (55.6-69.1): overlap
    ("w32", 4096, 4096): [(33, 65)],                           # o, 40 rows: 25.8 (25.2-26.3) against 25.3 (24.4-26.1)
    ("w16", 4096, 4096): [(33, 65), (97, 161)],                # o: 26.6 against 25.6; 160 rows: 41.0 against 39.1
    ("w16", 22016, 4096): [(33, 161)],                         # gate|up: 56.6 (55.0-62.3) / 74.4 / 97.1 against 56.7 / 70.3 / 92.2
    ("w16", 32000, 4096): [(65, 161)],                         # lm_head: 88.2 / 118.3 against 84.6 / 117.5
}


def _batch_split_route(form, N, K, rows, table=None):
    """'own' or 'library' for a decode projection of `rows` fp32s rows over an unquantised [N, K] matrix."""
    for lo, hi in (_BATCH_SPLIT_LIBRARY if table is None else table).get((form, int(N), int(K)), ()):
        if lo <= rows < hi:
            return "library"
    return "own"


# fp32s decode steps of <= 32 rows over bf16-VALUED matrices, engine option bf16_value_stream: psg_split_gemm_wb16
# streams the bf16 copy (2 bytes per weight, three bf16 products) where the steps above stream the fp32 tensor on
# psg_skinny_gemm (4 bytes per weight).  A FIXED table like INT4_STREAM_OFF: a listed (N, K) is a measured loser
# (tools/bf16_stream_bench.py at 20 rows: the kernel's range of times not wholly below the fp32 kernel's) and switches the
# route off for a model that has a decoder matrix of that shape; a shape that is not listed takes the route.
# Measured (profiles/bf16_stream_bench.json; us per launch, median (min-max), bf16 stream against the fp32 kernel): q|k|v 24.7
# (23.7-28.3) against 39.1 (37.7-44.2), o 11.0 (10.6-11.6) against 15.0 (14.9-15.1), gate|up 38.0 (37.2-39.3) against 65.0
# (63.8-71.4), down 21.0 (20.8-21.3) against 35.3 (35.0-36.4), lm_head 64.1 (62.9-64.3) against 99.4 (97.0-100.0): every
# Llama-2-7B shape lies wholly below its yardstick, nothing is listed.
WB16_STREAM_OFF: frozenset = frozenset()

# Decode steps with 33..160 rows of an fp32s engine whose matrices are resident as their bf16 copies only, engine option
# bf16_value_resident: psg_batch_gemm_b3.hip runs the three bf16-plane products.  A FIXED table like
# _BATCH_SPLIT_LIBRARY: a listed row range sends a measured loser (tools/bf16_resident_bench.py, tools/batch_split_bench.py's
# method: the kernel's range of times not wholly below the yardstick's) to the yardstick - what this mode runs otherwise on
# the same bf16 copy: split_b16x3 + the stacked-plane library product (`_stacked_b3`); a shape that is not listed takes the
# kernel.
#   key: (N, K) -> [(rows from, rows below), ...]
# Measured at the Llama-2-7B shapes and 40 / 80 / 160 rows = 2 / 3 / 5 x tiles (profiles/bf16_resident_bench.json; the row
# ranges are those of the tile counts; us per launch, median (min-max), own against yardstick).  The kernel wins the shapes
# whose slabs are cut into many slices - o 15.9 / 22.6 / 30.5 against 23.2 / 29.9 / 38.1, down 31.9 / 45.9 / 65.6 against
# 48.6 / 62.7 / 86.6 - and loses the wide ones, where a workgroup walks all of K for 128 weight rows and the matrix
# instructions of three planes are not hidden behind 16 KB of weights per step:
_BATCH_WB16_LIBRARY: dict = {
    (12288, 4096): [(33, 161)],                                # q|k|v: 38.7 (36.2-43.5) against 38.8 (38.5-40.7): overlap; 55.0 / 76.8 against 47.8 / 64.9
    (22016, 4096): [(33, 161)],                                # gate|up: 56.1 (54.6-62.9) against 55.2 (53.0-55.8); 84.5 / 120.0 against 71.2 / 93.5
    (32000, 4096): [(33, 161)],                                # lm_head: 77.1 / 114.7 / 161.8 against 68.6 / 87.7 / 120.9
}


def _batch_wb16_route(N, K, rows, table=None):
    """'own' or 'library' for a decode projection of `rows` fp32s rows over the bf16 copy of an [N, K] matrix."""
    for lo, hi in (_BATCH_WB16_LIBRARY if table is None else table).get((int(N), int(K)), ()):
        if lo <= rows < hi:
            return "library"
    return "own"

_LAYER_MATRICES = ("wqkv", "wo", "wgu", "wdown")                  # a decoder layer's projections, by their key in `layers`
# The streams a matrix can have in a decode step of <= 32 rows (`LlmMatrix.stream`), each also the name of the step
# route on which every decoder matrix has it (`_decode_route`) and the suffix of its pair-form entry ops.split_gemm_<kind>:
# kind -> the planes of the fp32 rows that entry reads (two fp16 planes + a row scale, or three bf16 planes)
_STREAM_PLANES = {"w16": 2, "w8": 2, "w4": 2, "int4": 2, "wb16": 3}
_QUANT_STREAMS = {"w8": "fp8", "w4": "mxfp4", "int4": "int4"}      # ... of a quantised matrix -> the format it streams


class LlamaDecodeEngine:
    def __init__(self, weights: dict, cfg: PSGConfig, device, dtype=torch.bfloat16, n_layers=None, resid_dtype=None,
                 prefill_split=False, resident="all", batch_quant_stream=False, batch_split_gemm=False,
                 bf16_value_stream=False, bf16_value_resident=False):
        """prefill_split (fp32 engines): the prompt pass's projections as split-fp16 products on the 16-bit matrix cores,
        `linear_split` below; the decode steps stay exact fp32 (psg_gemm_f32.hip).
        resid_dtype: storage type of the residual stream; None = `dtype` (what HF keeps for a model cast to 16
        bits), torch.float32 with a 16-bit `dtype` = mixed mode (16-bit GEMM operands, the residual stream - the sum
        of 2 x layers updates - never rounded to 16 bits; costs 160 KB more traffic per decode row kernel).
        batch_quant_stream: decode steps of 33..160 rows stream a quantised matrix's bytes (`_batch_quant`)
        instead of reading W'.
        batch_split_gemm (fp32s engines): decode steps of 33..160 rows run an unquantised matrix on psg_batch_gemm_s.hip
        (`_batch_split`) instead of the library GEMM.
        bf16_value_stream (fp32s engines): decoder matrices and an lm_head that are bf16 VALUES (a bf16 checkpoint upcast on
        load; verified per tensor) keep a bf16 copy, and the decode steps of <= 32 rows stream it on psg_split_gemm_wb16
        (`_decode_step_split` on the 'wb16' route) instead of the fp32 tensor.
        bf16_value_resident (with bf16_value_stream): every decoder matrix must be a bf16 value and is held as its
        bf16 copy ONLY (so is a bf16-valued lm_head) - no fp32 W', no split image; every product of the engine runs on the
        three bf16 planes of its fp32 rows against that copy (`_linear_b3`, `_forward_split_b3`).  Inference only."""
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise PsgHipError(f"activation dtype must be float32, bfloat16 or float16, got {dtype}")
        if resident not in ("all", "quantised"):
            raise PsgHipError(f"resident must be 'all' or 'quantised', got {resident!r}")
        # resident='quantised' (DESIGN 15): a quantised matrix is held as its bytes only - no W', no fp16 image - and every
        # product that reads a dense operand (more than 32 rows) has it expanded into a scratch buffer first (`_dense`)
        self.resident = resident
        lean = resident == "quantised"
        if not isinstance(bf16_value_resident, bool):
            raise PsgHipError(f"bf16_value_resident must be a bool, got {bf16_value_resident!r}")
        if bf16_value_resident and not (bf16_value_stream is True and dtype == torch.float32 and prefill_split and not lean):
            raise PsgHipError("bf16_value_resident keeps the bf16 copies that bf16_value_stream streams as the ONLY copy of an "
                              "fp32s engine's matrices: it needs bf16_value_stream=True, dtype float32 with prefill_split and "
                              "resident='all'")
        self.bf16_value_resident = bf16_value_resident
        if lean and dtype == torch.float32 and not prefill_split:
            raise PsgHipError("resident='quantised': the exact fp32 mode (dtype='fp32') reads W' in every decode step, there is "
                              "nothing to drop - use dtype='fp32s' / 'mixed' / 'bf16' / 'fp16', or resident='all'")
        self.resid_dtype = dtype if resid_dtype is None else resid_dtype
        if self.resid_dtype not in (dtype, torch.float32):
            raise PsgHipError(f"residual dtype must be {dtype} or float32, got {self.resid_dtype}")
        m = cfg.llm
        if m.head_dim != 128:
            raise PsgHipError(f"LLM head_dim {m.head_dim} unsupported (kernels are built for 128)")
        try:
            m.check_kv_heads()
        except ValueError as e:
            raise PsgHipError(f"LLM: {e}") from None
        # grouped-query attention (kv_heads < heads): the q|k|v rows are (heads + 2 kv_heads) 128 wide, the KV caches hold
        # kv_heads heads, and the attention launches are the *_gqa entry points; None keeps every multi-head launch as it was
        self.kv = m.n_kv_heads if m.n_kv_heads != m.heads else None
        self.qkv_width = m.hidden + 2 * m.kv_dim
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        self.n_layers = m.layers if n_layers is None else n_layers        # llm_truncate_num (V4:101-103)
        self.prefill_split = bool(prefill_split) and dtype == torch.float32
        dev_i = self.device.index or 0
        f32 = lambda k: weights[k].to(device=self.device, dtype=torch.float32).contiguous()   # noqa: E731
        from .weights import BEXP_SUFFIX, GSCALE_SUFFIX, SCALE_SUFFIX, is_quantized, llm_quant_keys
        if any(str(k).endswith(GSCALE_SUFFIX) for k in weights.keys()) and (lean or batch_quant_stream):
            opt = "resident='quantised'" if lean else "batch_quant_stream"
            raise PsgHipError(f"{opt} is not built for the INT4 format: there is no expand kernel and no 33..160-row kernel "
                              "for it")
        if lean:
            dense = [k for k in llm_quant_keys(self.n_layers) if k + SCALE_SUFFIX not in weights]
            if dense:
                raise PsgHipError(f"resident='quantised' needs every decoder-layer matrix quantised; {len(dense)} are not (e.g. "
                                  f"{dense[0]}): set llm_weight_quant='fp8' / 'mxfp4' or load an FP8 / MXFP4 checkpoint, or use "
                                  "resident='all'")
        # one `LlmMatrix` record per (row-concatenated) projection matrix (llm_matrix.py): `mats[l][key]`,
        # `lm_head_mat`, `proj_mat`.  `layers[l][key]` and `lm_head` are what the records hold as the dense operand W' - or the
        # record itself where a matrix is resident as bytes only - for readers outside the engine (and the layer norms)
        def load(*keys, may_be_fp32=False):
            """The record of the matrix of `keys`.  bf16_value_resident: its bf16 copy only - or, for a matrix that is no bf16
            value, the name of its first such part (may_be_fp32, the lm_head: the fp32 record it has without the option)."""
            if not self.bf16_value_resident:
                return load_matrix(weights, keys, self.device, dtype, lean, self.prefill_split)
            if any(is_quantized(weights, k) for k in keys):
                raise PsgHipError(f"bf16_value_resident: {keys[0]} is quantised - the option holds UNQUANTISED bf16 values "
                                  "(llm_weight_resident='quantised' is the lean mode of a quantised model)")
            rec = load_bf16_matrix(weights, keys, self.device, dtype)
            if isinstance(rec, str) and may_be_fp32:
                return load_matrix(weights, keys, self.device, dtype, False, self.prefill_split)
            return rec
        held = lambda rec: rec if rec.w is None else rec.w                                             # noqa: E731
        self.embed = weights["language_model.model.embed_tokens.weight"].to(device=self.device, dtype=dtype).contiguous()
        # (an lm_head fine-tuned in fp32 keeps its fp32 tensor and today's routes, as DESIGN 20 keeps its stream)
        self.lm_head_mat = load("language_model.lm_head.weight", may_be_fp32=True)
        self.lm_head = held(self.lm_head_mat)
        self.final_norm = f32("language_model.model.norm.weight")
        self.set_projection(weights["language_projection.weight"], weights["language_projection.bias"])
        self.mats, self.layers = [], []
        not_bf16 = []                                          # bf16_value_resident: decoder matrices that are no bf16 values
        for l in range(self.n_layers):
            p = f"language_model.model.layers.{l}."
            for n, rows_ in (("q", m.hidden), ("k", m.kv_dim), ("v", m.kv_dim)):
                shp = tuple(weights[p + f"self_attn.{n}_proj.weight"].shape)
                if (p + f"self_attn.{n}_proj.weight" + BEXP_SUFFIX in weights
                        or p + f"self_attn.{n}_proj.weight" + GSCALE_SUFFIX in weights):   # (MXFP4 / INT4: two codes per byte)
                    shp = (shp[0], 2 * shp[1])
                if shp != (rows_, m.hidden):
                    raise PsgHipError(f"{p}self_attn.{n}_proj.weight has shape {shp}, expected {(rows_, m.hidden)} "
                                      f"({m.heads} query / {m.n_kv_heads} key-value heads of 128)")
            recs = dict(
                wqkv=load(*[p + f"self_attn.{n}_proj.weight" for n in "qkv"]),
                wo=load(p + "self_attn.o_proj.weight"),
                wgu=load(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"),
                wdown=load(p + "mlp.down_proj.weight"))
            not_bf16 += [rec for rec in recs.values() if isinstance(rec, str)]
            if not_bf16:                                       # (looked at to the last layer: the refusal counts them)
                continue
            self.mats.append(recs)
            self.layers.append(dict({k: held(rec) for k, rec in self.mats[-1].items()},
                                    ln1=f32(p + "input_layernorm.weight"), ln2=f32(p + "post_attention_layernorm.weight")))
        if not_bf16:
            raise PsgHipError(f"bf16_value_resident=True (llm_bf16_value_resident) holds every decoder matrix as its bf16 copy "
                              f"only, and {len(not_bf16)} decoder matrices are not bf16 values (the first: {not_bf16[0]}): "
                              "llm_bf16_value_resident=False runs them on their fp32 tensors")
        layer_m = self._layer_mats()
        n_q, n_q4, n_qi = (sum(rec.fmt == f for rec in layer_m) for f in ("fp8", "mxfp4", "int4"))
        bytes_fmt = any(rec.fmt in ("fp8", "mxfp4") for rec in self.matrices())
        if n_qi and (n_qi < len(layer_m) or bytes_fmt):
            raise PsgHipError(f"{n_qi} of the {len(layer_m)} decoder-layer matrices are INT4-quantised: all or none, and one format")
        if n_q and n_q4:
            raise PsgHipError(f"{n_q} decoder-layer matrices are FP8-quantised and {n_q4} MXFP4-quantised: one format")
        if 0 < n_q < len(layer_m):
            raise PsgHipError(f"{n_q} of the {len(layer_m)} decoder-layer matrices are FP8-quantised: all or none")
        if 0 < n_q4 < len(layer_m):
            raise PsgHipError(f"{n_q4} of the {len(layer_m)} decoder-layer matrices are MXFP4-quantised: all or none")
        self._any_quant = n_q + n_q4 + n_qi > 0 or self.lm_head_mat.fmt is not None
        self._use_skinny = True
        self.batch_quant_stream = bool(batch_quant_stream)
        if self.batch_quant_stream and not bytes_fmt:
            raise PsgHipError("batch_quant_stream streams a quantised LLM's bytes in the batched decode, and no matrix of this "
                              "model is quantised: set llm_weight_quant='fp8' / 'mxfp4' or load an FP8 / MXFP4 checkpoint")
        self.batch_split_gemm = bool(batch_split_gemm)
        if self.batch_split_gemm and not self.prefill_split:
            raise PsgHipError("batch_split_gemm runs the batched decode of an fp32s engine (dtype float32 with prefill_split) on "
                              "split-fp16 products: the 16-bit engines run psg_batch_gemm there, the exact fp32 engine its SGEMM")
        if not isinstance(bf16_value_stream, bool):
            raise PsgHipError(f"bf16_value_stream must be a bool, got {bf16_value_stream!r}")
        self.bf16_value_stream = bf16_value_stream
        complete(layer_m, self.lm_head_mat, dtype, prefill_split=self.prefill_split, llm_w16=bool(_lib.get_option(dev_i, "llm_w16")),
                 bf16_value_stream=bf16_value_stream, batch_split_gemm=self.batch_split_gemm)
        # What every decoder-layer matrix is, as the step route it opens (a key of `_STREAM_PLANES`), or None: FP8 / MXFP4
        # bytes ('w8' / 'w4': all or none, above; an MXFP4 shape may stream its FP8 image), INT4 with every code stream
        # ('int4'), fp16 values - the lm_head too - ('w16': the fused decode step / two-plane prompt pass need all of them),
        # bf16 copies ('wb16')
        every = lambda f: bool(layer_m) and all(f(rec) for rec in layer_m)                             # noqa: E731
        self.layer_kind = ("w8" if n_q else "w4" if n_q4 else "int4" if every(lambda r: r.int4_img is not None)
                           else "w16" if all(r.w16 is not None for r in self.matrices())
                           else "wb16" if every(lambda r: r.wb16 is not None) else None)
        self._skinny_ok = {}
        self._ones_cache = {}
        if self.bf16_value_resident:
            self._check_resident_routes()
        # row_invariant (fp32s engines): the prompt pass's projections and the language projection on psg_dense_gemm - one
        # k-ordered accumulation per output element whatever the row count of the call - instead of the library GEMM, whose
        # kernel choice follows the row count: a pair decoded in a batch of 3 (decodes DEALT over the ranks of a pair-sharded
        # job) then gives the bits it gives in the batch of 20.  ~1.3x the prompt pass's GEMM time: the sharded
        # pipeline switches it on, a single GPU does not need it
        self._row_invariant = False
        self.split_i2 = bool(_lib.get_option(dev_i, "split_i2"))
        # greedy argmax over the fp32 split-K sums of the lm_head, NOT over their 16-bit rounding: HF computes the logits of
        # a model cast to 16 bits in 16 bits, but the reference runs the LLM in fp32 (V4:99-100), and a 16-bit logit has
        # an ulp of 0.008-0.016 (fp16) / 0.06 (bf16) at |x| ~ 8-16 - wider than many top-2 margins of a 32000-way
        # argmax, so rounding first turns near-ties into ties that the lower index wins
        self.exact_argmax = True
        self._mm_out_dtype = None        # torch.mm(..., out_dtype=fp32) available? (probed at first use)
        # row operations that run as the PROLOGUE of the projection that consumes them (one launch instead of two;
        # psg_skinny_gemm_fused).  Built for "rmsnorm", bit-identical, and OFF by default: measured 26.6 vs 25.6 us
        # per (RMSNorm + q/k/v projection), 75.2 vs 74.0 ms per image - the in-launch hand-off (write-through
        # publish, counter, poll, x staged after it) costs what the separate launch costs
        self.fuse_rowops = frozenset({"rmsnorm"}) if _lib.get_option(dev_i, "llm_fuse_rmsnorm") else frozenset()
        self.prefill_attn_scalar = bool(_lib.get_option(dev_i, "prefill_attn_scalar"))
        # decode steps as ONE persistent launch per layer (psg_decode_layer; fp32 engines at Llama-2-7B width on a 256-CU
        # device, 13..24 rows): bit-identical to the launch chain, so every other shape - and the in-flight slots, since
        # only one persistent launch may run on a device at a time - simply keeps the chain
        self.persistent_layer = bool(_lib.get_option(dev_i, "decode_persistent"))
        # fp32s prompt pass: the split of a projection's operand and the un-scaling of its result inside the row kernels
        # next to it (psg_rmsnorm_split / psg_rope_kvwrite_scaled / psg_silu_mul_split; bit-identical, 7 launches per layer less)
        self.fuse_split = bool(_lib.get_option(dev_i, "llm_fuse_split"))
        # fp32s prompt pass: run each library product whole or in the column / row parts measured fastest (_plan_split_mm)
        self.plan_split = True
        # ... and on the library algorithm `_LT_ALGO_TABLE` pins for the shape (psg_lt_gemm), where a line of it holds
        self._lt = _LtRoute(self.device)
        # decode steps of 33..160 rows: psg_batch_gemm where it beats the library (option decode_batch_gemm)
        self.batch_gemm = bool(_lib.get_option(dev_i, "decode_batch_gemm"))
        self._w_pools = {}
        for rec in self.matrices():
            if rec.w is not None:                              # (pools time dense tensors in rotation, PSG_PLAN=measure)
                self._w_pools.setdefault(tuple(rec.shape), []).append(rec.w)
        # resident='quantised': one scratch buffer per slot (`head.submit` runs two streams), as large as the largest
        # quantised matrix in the engine's dtype - the widest form `_dense` makes (the unscaled fp16 operand of the fp32s
        # prompt pass uses its head).  Allocated once, outside any graph: captured graphs replay against its address
        self._slot = 0
        self._scratch = {}
        self._scratch_elems = max([rec.numel() for rec in self.matrices() if rec.w is None], default=0)
        if lean:
            self._scratch_for(0)
        self._dl_ws = {}
        self._dl_host_buf = None
        self.use_graph = True            # capture the batched decode in a HIP graph (per input shape)
        self.early_exit_chunk = 4        # natural-EOS decode: steps per graph between "all pairs done?" checks
        self.last_replays = 0
        self._graphs = collections.OrderedDict()   # input shape -> captured decode graphs (LRU, at most max_graphs)
        self.max_graphs = 8              # a graph owns its KV caches (~0.7 GB at K = 20 for Llama-2-7B); `forward` + two submit slots
        hd = m.head_dim
        # rotary tables as HF builds them (HF-LL:115-128): inv_freq and the outer product in fp32 on the
        # host, cos/sin per position; the kernels index them by position
        inv_freq = 1.0 / (m.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
        ang = torch.arange(4096, dtype=torch.float32)[:, None] * inv_freq[None, :]
        self.rope = (ang.cos().contiguous().to(self.device), ang.sin().contiguous().to(self.device))

    def _check_resident_routes(self):
        """bf16_value_resident has no dense fallback: the decode steps of <= 32 rows run on the 'wb16' route of
        `_decode_step_split` or not at all.  Raises, naming the first condition of `_can_wb16` the model fails."""
        why = self._wb16_blockers(1)
        if why:
            raise PsgHipError(f"bf16_value_resident: the decode steps cannot stream the bf16 copies ({why[0]}), and there is no "
                              "fp32 tensor to fall back on - use llm_bf16_value_resident=False")

    @property
    def use_skinny(self):
        return self._use_skinny

    @use_skinny.setter
    def use_skinny(self, on):
        if not on and getattr(self, "bf16_value_resident", False):
            raise PsgHipError("bf16_value_resident: use_skinny=False sends the decode steps to library products on dense fp32 "
                              "tensors, which this engine does not hold - build it with llm_bf16_value_resident=False")
        self._use_skinny = bool(on)

    @property
    def row_invariant(self):
        return self._row_invariant

    @row_invariant.setter
    def row_invariant(self, on):
        if on and self.bf16_value_resident:
            raise PsgHipError("bf16_value_resident: the row-invariant prompt pass (pair-sharded pipelines) reads dense "
                              "interleaved images of every weight - build the engine with llm_bf16_value_resident=False")
        if on and self.resident == "quantised":
            raise PsgHipError("resident='quantised': the row-invariant prompt pass (pair-sharded pipelines) reads dense "
                              "interleaved images of every weight - build the engine with resident='all'")
        self._row_invariant = bool(on)

    def _layer_mats(self):
        """The record of every decoder-layer projection matrix, layer after layer."""
        return [M[k] for M in self.mats for k in _LAYER_MATRICES]

    def matrices(self):
        """... and the lm_head's."""
        return self._layer_mats() + [self.lm_head_mat]

    @property
    def _w16(self):
        """For the benchmark only: address of a dense tensor of `layers` / `lm_head` -> its fp16 copy."""
        return {rec.w.data_ptr(): rec.w16 for rec in self.matrices() if rec.w16 is not None}

    @property
    def _w16_all(self):
        """... and: is every decoder-layer matrix and the lm_head an fp16 value?"""
        return self.layer_kind == "w16"

    def _scratch_for(self, slot):
        buf = self._scratch.get(slot)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise PsgHipError(f"resident='quantised': slot {slot}'s scratch must exist before a graph is captured")
            buf = self._scratch[slot] = torch.empty(self._scratch_elems, device=self.device, dtype=self.dtype)
        return buf

    def _dense(self, w, unscaled=False):
        """THE accessor for the dense operand of a product over the record `w`: W' in the engine's dtype or, `unscaled`, the
        fp16 operand of the fp32s two-plane prompt pass - the exact image of W' / s (s is applied as the column scale) or the
        copy of an fp16-valued W'.  A matrix resident as bytes only is expanded on the current stream into the current slot's
        scratch (psg_expand_w8 / _w4: weights.dequantize_*_rows bit for bit) and a view of that is returned, valid until
        the slot's next expansion: expand per matrix, immediately before its product."""
        if w.w is not None:
            return w.two_plane() if unscaled else w.w
        if w.fmt is None:                                      # bf16_value_resident: `_linear_b3` is THE route of such a record
            raise PsgHipError(f"{w.name}: held as its bf16 copy only (bf16_value_resident), there is no dense operand")
        buf = self._scratch_for(self._slot)
        if unscaled:
            buf = buf.view(torch.float16)
        s = None if unscaled else w.s
        if w.fmt == "fp8":
            return ops.expand_w8(w.q, s, out=buf)
        return ops.expand_w4(w.q, w.e, s, out=buf)

    def resident_bytes(self):
        """What the engine holds in HBM, in bytes (numel * element_size): `quantised` - the byte streams, block exponents,
        row scales and stream images of its quantised matrices; `scratch` - every slot's expansion scratch; `other` - every
        other tensor (embedding, norms, rotary tables, and what the records own beside: the dense W', their 16-bit copies and
        split images); `total`.  KV caches and graph pools belong to a generation, not to the engine, and are not counted."""
        mats = self.matrices() + [self.proj_mat]
        norms = [L[k] for L in self.layers for k in ("ln1", "ln2")]
        seen = set()

        def count(tensors):                                    # (a tensor two records share is counted once)
            fresh = [t for t in tensors if t.data_ptr() not in seen and not seen.add(t.data_ptr())]
            return sum(t.numel() * t.element_size() for t in fresh)
        quant = count(t for rec in mats for t in rec.quant_tensors())
        scratch = count(self._scratch.values())
        other = count([self.embed, self.final_norm, self.proj_b, *self.rope, *norms, *self._ones_cache.values()]
                      + [t for rec in mats for t in rec.tensors()])
        return dict(quantised=quant, scratch=scratch, other=other, total=quant + scratch + other)

    def _dense_split(self, w):
        """Does `linear_split` run the split image of the record `w` on psg_dense_gemm (the row-invariant path)?"""
        return self.row_invariant and w.split is not None and w.shape[0] % 256 == 0 and (3 * w.shape[1]) % 64 == 0

    def linear_split(self, x, w, bias=None):
        """x [rows, K] fp32 @ w.T (+ bias) as ONE fp16 matrix-core GEMM over 3K: [xh | xh | xl] . [wh | wl | wh]^T with fp32
        accumulation, rows and columns rescaled by their powers of two afterwards (exact).  Products of fp16 values
        are exact in fp32, so what is lost against an fp32 GEMM is the xl.wl term and the split residuals: ~7e-7
        relative per product (fp32 rounds each product to 6e-8), at 3/16 of the fp32 matrix time."""
        w3, inv_c = w.split
        if self._dense_split(w):
            if self.split_i2 and w.shape[1] % 32 == 0:
                # round 6: interleaved hi / lo images, the three products from one staging (psg_dense_gemm_split)
                w2, inv_c = w.interleaved()
                a2, inv_r = ops.split_f16i2(x)
                return ops.dense_gemm_split(a2, w2, bias, inv_r, inv_c, tile="256x256")
            a3, inv_r = ops.split_f16x3(x)
            return ops.dense_gemm(a3, w3, bias, out_dtype=torch.float32, row_scale=inv_r, col_scale=inv_c)
        a3, inv_r = ops.split_f16x3(x)
        y = _split_mm(a3, w3, _plan_split_mm(a3.shape[0], w3) if self.plan_split else None)
        y = ops.scale_rows_cols(y, inv_r, inv_c)
        return y if bias is None else y + bias

    def set_projection(self, weight, bias):
        """Replaces the packed copy of `language_projection` (a checkpoint loaded after the engine was built, an optimizer
        step in training mode): a new record, so everything derived from the old tensor - the fp32s split image, the
        interleaved image of the row-invariant path - goes with it."""
        self.proj_mat = dense_matrix("language_projection", weight.to(device=self.device, dtype=self.dtype).contiguous(),
                                     split=self.prefill_split)
        self.proj_b = bias.to(device=self.device, dtype=self.dtype).contiguous()

    def _streams(self, rows, w, dtype):
        """Can the weight-streaming kernel run `rows` rows of `dtype` against w?  It keeps the rows' K slice in LDS beside its
        weight rings: the fp32 kernel takes 32 rows up to K = 11776 and 20 rows up to K = 20480 (every Llama-2-7B / 13B shape
        at the reference's 20 selected pairs).  A wider model falls through to the library GEMM for that projection (exact
        fp32, not batch-invariant) instead of failing."""
        if not (w.shape[0] % 16 == 0 and w.shape[1] % 64 == 0 and w.shape[1] >= 256):
            return False
        key = (rows, tuple(w.shape), dtype)
        ok = self._skinny_ok.get(key)
        if ok is None:
            try:
                ops.skinny_gemm_plan(rows, w.shape[0], w.shape[1], dtype, self.device)
                ok = True
            except PsgHipError:
                ok = False
            self._skinny_ok[key] = ok
        return ok

    def _ones(self, n):
        """fp32 ones [n]: the column scale of a product against an fp16-valued weight (it has no scale of its own)."""
        t = self._ones_cache.get(n)
        if t is None:
            t = self._ones_cache[n] = torch.ones(n, device=self.device, dtype=torch.float32)
        return t

    def linear(self, x, rec, decode=False, batch_stream=True):
        """Bias-free projection of x over the matrix of the record `rec`.  Decode-step shapes (<= 32 rows) use the hand-written weight-streaming kernel - in
        the 16-bit modes and in the fp32 mode (the reference's own precision, V4:99-100) alike; the prompt pass goes
        through hipBLASLt; decode steps of 33..160 rows (several images' pairs, 16-bit modes) through whichever of
        psg_batch_gemm's variants and the library was measured fastest for the shape (_plan_batch_mm) - or, with
        batch_quant_stream, over a quantised matrix's bytes (`_batch_quant`; batch_stream=False: the caller keeps W')."""
        if rec.w is None and rec.fmt is None:                  # bf16_value_resident: the bf16 copy is the operand of every product
            return self._linear_b3(x, rec, decode, batch_stream)
        kind, args = rec.stream or (None, None)
        if (kind in _QUANT_STREAMS and self.use_skinny and x.shape[0] <= 32 and x.dtype == rec.dtype
                and (self.prefill_split or x.dtype != torch.float32)):
            # quantised matrix, <= 32 rows: one byte (FP8, psg_gemm_w8.hip) or 4.25 bits (MXFP4, psg_gemm_w4.hip; group-wise INT4,
            # psg_gemm_int4.hip) per weight.  The exact fp32 mode, shapes without a stream and more rows run the paths
            # below on W'
            if x.dtype == torch.float32:
                x2, inv = ops.split_f16x2(x)
                return getattr(ops, "split_gemm_" + kind)(x2, inv, *args)
            return getattr(ops, "skinny_gemm_" + kind)(x, *args)
        if (self.batch_quant_stream and batch_stream and decode and self.use_skinny and 32 < x.shape[0] <= 160 and x.dtype == rec.dtype
                and kind in ("w8", "w4") and (self.prefill_split or x.dtype != torch.float32)):   # (no such kernel for INT4)
            out = self._batch_quant(x, rec)
            if out is not None:
                return out
        w = self._dense(rec)                                  # (resident='quantised': W' expanded into the slot's scratch)
        if self.use_skinny and x.shape[0] <= 32 and x.dtype == w.dtype and self._streams(x.shape[0], w, x.dtype):
            wh = rec.w16 if x.dtype == torch.float32 else None
            if wh is not None and self.prefill_split:         # fp32s: two fp16 products of the split rows, 2 bytes per weight
                x2, inv = ops.split_f16x2(x)
                return ops.split_gemm_w16(x2, inv, wh)
            if wh is not None:                                # exact fp32: the same f32 instructions on the widened weight
                return ops.skinny_gemm_w16(x, wh)
            return ops.skinny_gemm(x, w)          # fp32 split-K partials, reduced by the consumer kernel
        if (decode and self.batch_gemm and self.use_skinny and 32 < x.shape[0] <= 160 and x.dtype == w.dtype
                and x.dtype in (torch.bfloat16, torch.float16) and w.shape[0] % 16 == 0 and w.shape[1] % 64 == 0):
            plan = _plan_batch_mm(x, self._w_pools.get(tuple(w.shape), [w]))
            if plan[0] == "own":
                return ops.batch_gemm(x, w, plan[1], plan[2])
        if (self.plan_split and x.shape[0] >= 1024 and x.dtype == w.dtype and x.dtype in (torch.bfloat16, torch.float16)
                and x.dim() == 2 and x.is_contiguous()):
            # the 16-bit prompt pass of several images (forward_batch: 2 / 4 / 8 x 960 rows): the library's pick for the
            # whole product against its column / row parts (_plan_split_mm; 7-14 % per layer at 1920-7680 rows, nothing at 960)
            return _split_mm(x, w, _plan_split_mm(x.shape[0], w, None, pool=self._w_pools.get(tuple(w.shape))), None)
        if (self.batch_split_gemm and batch_stream and decode and self.use_skinny and self.prefill_split and rec.fmt is None
                and 32 < x.shape[0] <= 160 and x.dtype == torch.float32):
            out = self._batch_split(x, rec)
            if out is not None:
                return out
        if decode and x.dtype == torch.float32 and x.shape[0] > 32:
            # fp32 engines, decode steps of 33..160 rows (several images' pairs, head.forward_batch - BASELINE C5's batch of 8
            # at the reference's precision): the weight leaves HBM ONCE per step for all rows.  fp16-valued weights of an
            # fp32s engine: the two planes of the split rows [xh; xl] against the fp16 copy in ONE library product with an
            # fp32 result (2 bytes per weight, 2^-22 per product - the arithmetic of psg_split_gemm_w16); generic fp32
            # weights: the library SGEMM, exact (4 bytes per weight) - NOT the three-segment split product of the prompt
            # pass, which would stream 6 bytes per weight for flops a 160-row step does not need to save
            wh = rec.w16 if self.prefill_split else None
            if wh is not None and w.shape[1] % 8 == 0:
                a2, inv = ops.split_f16x2(x)
                y2 = torch.mm(a2.view(2 * x.shape[0], x.shape[1]), wh.t(), out_dtype=torch.float32)
                return ops.Scaled(y2.view(2, x.shape[0], w.shape[0]), inv, self._ones(w.shape[0])).dense()
            return F.linear(x, w)
        if rec.split is not None and x.dtype == torch.float32:
            return self.linear_split(x, rec)
        return F.linear(x, w)

    def _stacked_b3(self, x3, rec, plan=None):
        """The stacked-plane library product of bf16_value_resident: x3 bf16 [3, rows, K], the planes
        [x0; x1; x2] of `split_b16x3`, against the bf16 copy of `rec` in ONE library product of 3 x rows rows with an fp32
        result.  The planes are stacked [x2; x1; x0], so the result's slices are [y2, y1, y0] and a reader that adds slices
        in slot order - every consumer of `ops.Partials` - computes (y2 + y1) + y0: THE order of the three plane sums, small
        planes first, as psg_split_gemm_wb16's flush.  Every product is exact; only fp32 accumulation is left."""
        _, rows, K = x3.shape
        y = _split_mm(x3.flip(0).view(3 * rows, K), rec.wb16, plan)
        return ops.Partials(y.view(3, rows, rec.shape[0]))

    def _linear_b3(self, x, rec, decode=False, batch_stream=True):
        """`linear` over a record held as its bf16 copy only: fp32 rows, three bf16 planes (exact), fp32 slices.  <= 32 rows:
        psg_split_gemm_wb16 (the decode step's kernel); decode steps of 33..160 rows (`forward_batch`, beam levels):
        psg_batch_split_gemm_wb16 unless `_BATCH_WB16_LIBRARY` lists the shape; everything else - more rows, the trie pass
        (batch_stream=False), shapes the kernels do not take - `split_b16x3` + the stacked-plane library product."""
        if x.dtype != torch.float32 or x.dim() != 2:
            raise PsgHipError(f"{rec.name}: held as its bf16 copy only (bf16_value_resident), it takes fp32 rows, got {x.dtype} "
                              f"{tuple(x.shape)}")
        rows, (N, K) = int(x.shape[0]), rec.shape
        x3 = ops.split_b16x3(x if x.is_contiguous() else x.contiguous())
        fits = N % 16 == 0 and K % 64 == 0
        if fits and rows <= 32:
            return ops.split_gemm_wb16(x3, rec.wb16)
        if fits and decode and batch_stream and 32 < rows <= 160 and _batch_wb16_route(N, K, rows) == "own":
            return ops.batch_split_gemm_wb16(x3, rec.wb16)
        return self._stacked_b3(x3, rec)

    def _batch_quant(self, x, rec):
        """Decode projection of 33..160 rows over a quantised matrix on its byte / nibble stream (psg_batch_gemm_q.hip,
        DESIGN 16): fp32 slices for the consumers of `ops.batch_gemm`, or None where the shape does not fit the kernels or
        the routing table sends it to the dense path.  fp32s rows go through `split_f16x2` and the pair form, 16-bit rows
        take the single form.  The stream is the one the matrix has below 33 rows (`rec.stream`: a matrix with an FP8 image -
        FP8 itself, or a W4_STREAM_AS_FP8 shape - streams that)."""
        rows, (N, K) = int(x.shape[0]), rec.shape
        kind, args = rec.stream
        pair = x.dtype == torch.float32
        if (self.resident != "quantised"
                and _batch_quant_route(_QUANT_STREAMS[kind], "pair" if pair else "single", N, K, rows) == "dense"):
            return None
        if pair:
            x2, inv = ops.split_f16x2(x)
            return getattr(ops, "batch_split_gemm_" + kind)(x2, inv, *args)
        return getattr(ops, "batch_gemm_" + kind)(x, *args)

    def _batch_split(self, x, rec):
        """Decode projection of 33..160 fp32s rows over an unquantised matrix on psg_batch_gemm_s.hip: fp32
        slices for the consumers of `ops.batch_gemm`, or None where the shape does not fit the kernel, the matrix has no
        16-bit operand or the routing table sends it to the library.  An fp16-valued matrix streams its fp16 copy (2 bytes
        per weight, two products); a generic one the [wh | wl] planes of the prompt pass's split image in place - the
        lm_head: of its packed image - (4 bytes per weight, three products)."""
        rows, (N, K) = int(x.shape[0]), rec.shape
        if N % 16 or K % 64:
            return None
        ws = rec.split or rec.packed
        if rec.w16 is None and ws is None or _batch_split_route("w32" if rec.w16 is None else "w16", N, K, rows) == "library":
            return None
        x2, inv = ops.split_f16x2(x)
        if rec.w16 is not None:
            return ops.batch_split_gemm_w16(x2, inv, rec.w16, self._ones(N))
        return ops.batch_split_gemm_w32(x2, inv, ws[0], ws[1], K)

    def decode_uses_library(self, rows) -> bool:
        """Does a decode step of `rows` rows run a library GEMM?  Above 32 rows, without the weight-streaming kernel, or
        when a projection's K slice does not fit it at this row count (`_streams`: fp32 at K = 14336, Mistral-7B's
        down projection, above 20 rows).  Two library decodes must not run side by side on two streams (`head.submit`)."""
        rows = int(rows)
        if not self.use_skinny or rows > 32:
            return True
        # (the persistent layer and the fused step run the chain's own weight-streaming kernels: answered as the chain)
        route = self._decode_route(rows, per_call=False)
        if route == "wb16":                                    # psg_split_gemm_wb16 for every decoder projection; the lm_head
            head = self.lm_head_mat                            # follows the stream its tensor has
            return not (head.wb16 is not None or head.w16 is not None or self._streams(rows, head, self.dtype))
        if route is not None:                                  # psg_split_gemm_w16 / _w8 / _w4 / _int4 for every projection
            return False
        ws = (list(self.mats[0].values()) if self.mats else []) + [self.lm_head_mat]
        return not all(self._streams(rows, w, self.dtype) for w in ws)

    def logits(self, h, batch_stream=True):
        """lm_head.  <= 32 rows: the weight-streaming kernel (fp32 split-K partials, summed inside the greedy step);
        more rows (several images' pairs decoded together): the library GEMM with an fp32 result, so that the greedy
        argmax sees unrounded logits on this path too (exact_argmax) - or, with batch_quant_stream and a quantised
        lm_head, the fp32 slices of its byte stream (batch_stream=False, the trie pass: never)."""
        out = self.linear(h, self.lm_head_mat, decode=True, batch_stream=batch_stream)
        if isinstance(out, ops.Partials) or not self.exact_argmax or h.dtype == torch.float32:
            return out
        return self._lm_head_f32(h, out)

    def _lm_head_f32(self, h, rounded=None):
        """lm_head of 16-bit rows with an fp32 result (the values `logits` hands the greedy step above 32 rows).
        rounded: the 16-bit product, where the caller has it: without `out_dtype` it is widened instead of computed again."""
        if self._mm_out_dtype is None:
            try:
                probe = self.embed if self.lm_head_mat.w is None else self.lm_head_mat.w
                torch.mm(h[:1], probe[:16].t(), out_dtype=torch.float32)
                self._mm_out_dtype = True
            except (TypeError, RuntimeError):
                self._mm_out_dtype = False
        if self._mm_out_dtype:
            return torch.mm(h, self._dense(self.lm_head_mat).t(), out_dtype=torch.float32)
        return (F.linear(h, self._dense(self.lm_head_mat)) if rounded is None else rounded).float()

    # ---- one pass over `rows` token rows -------------------------------------------------------
    def _forward(self, resid, tok_pair, tok_pos, kc, vc, ctx_len, decode=False, prefill_shape=None, rope_pos=None,
                 keep_rows=None, tree=None):
        """resid [rows, D] is updated in place (residual stream); returns final-norm hidden [rows, D].
        decode=True: every row is the newest token of its pair -> fused rotary + KV append + attention.
        prefill_shape=(pairs, rows_per_pair): the rows are a pair-major prompt batch -> matrix-core attention
        (bf16, <= 64 rows per pair); otherwise the scalar cache-attention kernel.
        rope_pos int32 [rows]: rotary positions when they differ from the cache slots `tok_pos` (training).
        keep_rows int32 [k]: the caller reads only these rows of the result (prompt pass: the last token of every
        pair).  The last layer then writes K/V for every row (the cache needs them) and runs everything behind the
        attention - output projection, norms, MLP - on those k rows only; returns [k, D].
        tree (the relation-likelihood pass, `_rank_pass`): dict(row_node, prefix_len, anc, base, rope_bound) - the rows are
        token-trie nodes whose attention is psg_tree_attn over their pair's prompt slots and their trie ancestors.  With
        decode=True (the levels of a beam, `_steps`) the projections take the decode-step routes of `linear`, and a row whose
        tok_pos / row_node is -1 (a dead hypothesis) writes no cache slot and attends to nothing."""
        m = self.cfg.llm
        rows, D = resid.shape
        if (self.prefill_split and self.fuse_split and not self.row_invariant and not decode and prefill_shape is not None
                and rope_pos is None
                and rows > 32 and m.head_dim == 128 and prefill_shape[1] <= 64 and not self.prefill_attn_scalar
                and m.inter <= 16384 and D <= 8192):
            return self._forward_split(resid, tok_pair, tok_pos, kc, vc, ctx_len, prefill_shape, keep_rows)
        n = torch.empty((rows, D), device=self.device, dtype=self.dtype)
        ops.rmsnorm(resid, None, self.layers[0]["ln1"], m.rms_eps, n)
        q = torch.empty_like(n)
        # (a dead beam row's attention output is written by nobody: zeros, so that the row stays finite and reproducible)
        att = torch.zeros_like(n) if decode and tree is not None else torch.empty_like(n)
        act = torch.empty((rows, m.inter), device=self.device, dtype=self.dtype)
        mfma_prefill = (prefill_shape is not None and m.head_dim == 128 and prefill_shape[1] <= 64
                        and not self.prefill_attn_scalar)
        fused_rope = mfma_prefill and self.dtype in (torch.bfloat16, torch.float16)       # rotary + cache write in the launch
        for l, (L, M) in enumerate(zip(self.layers, self.mats)):
            qkv = self.linear(n, M["wqkv"], decode=decode)
            if decode and tree is None:
                ops.decode_attn(qkv, tok_pair, tok_pos, self.rope, m.heads, m.head_dim, ctx_len, kc[l], vc[l], att,
                                kv_heads=self.kv)
            elif fused_rope and isinstance(qkv, torch.Tensor) and rope_pos is None:
                ops.prefill_attn_rope(qkv, tok_pos, self.rope, prefill_shape[0], prefill_shape[1], m.heads, m.head_dim,
                                      ctx_len, kc[l], vc[l], att, kv_heads=self.kv)
            elif tree is not None:
                ops.rope_kvwrite(qkv, tok_pair, tok_pos, self.rope, m.heads, m.head_dim, ctx_len, q, kc[l], vc[l],
                                 rope_pos=rope_pos, kv_heads=self.kv, rope_pos_bound=tree["rope_bound"])
                ops.tree_attn(q, kc[l], vc[l], tok_pair, tree["row_node"], tree["prefix_len"], tree["anc"], tree["base"],
                              m.heads, m.head_dim, ctx_len, att, kv_heads=self.kv)
            else:
                ops.rope_kvwrite(qkv, tok_pair, tok_pos, self.rope, m.heads, m.head_dim, ctx_len, q, kc[l], vc[l],
                                 rope_pos=rope_pos, kv_heads=self.kv)
                if mfma_prefill:
                    ops.prefill_attn(q, kc[l], vc[l], tok_pos, prefill_shape[0], prefill_shape[1], m.heads, m.head_dim,
                                     ctx_len, att, kv_heads=self.kv)
                else:
                    ops.llm_attn(q, kc[l], vc[l], tok_pair, tok_pos, m.heads, m.head_dim, ctx_len, att, kv_heads=self.kv)
            if keep_rows is not None and l == len(self.layers) - 1:
                att, resid = self._gather_kept(att, resid, keep_rows)
                n = torch.empty_like(att)
                act = torch.empty((keep_rows.numel(), m.inter), device=self.device, dtype=self.dtype)
            o = self.linear(att, M["wo"], decode=decode)
            ops.rmsnorm(resid, o, L["ln2"], m.rms_eps, n)                      # resid += o ; n = norm(resid)
            gu = self.linear(n, M["wgu"], decode=decode)
            ops.silu_mul(gu, act)
            d = self.linear(act, M["wdown"], decode=decode)
            nxt = self.layers[l + 1]["ln1"] if l + 1 < len(self.layers) else self.final_norm
            ops.rmsnorm(resid, d, nxt, m.rms_eps, n)                           # resid += d ; n = norm(resid)
        return n

    def _gather_kept(self, att, resid, keep_rows):
        """Last layer of a pass whose caller reads only `keep_rows`: the attention output and the residual stream of those
        rows - everything behind the attention then runs on them alone."""
        k, D = keep_rows.numel(), att.shape[1]
        att_k = torch.empty((k, D), device=self.device, dtype=att.dtype)
        resid_k = torch.empty((k, D), device=self.device, dtype=resid.dtype)
        ops.gather_rows(att, keep_rows, att_k)
        ops.gather_rows(resid, keep_rows, resid_k)
        return att_k, resid_k

    def _forward_split(self, resid, tok_pair, tok_pos, kc, vc, ctx_len, prefill_shape, keep_rows):
        """`_forward` for the prompt pass of the fp32s mode with the operand splits and result scalings fused into the row
        kernels: RMSNorm and SwiGLU write the split fp16 operand, every projection result stays raw (`ops.Scaled`) until
        its reader applies the scales while loading.  Same arithmetic as `_forward` + linear_split, bit for bit.
        Three planes (generic fp32 weights): [hi | hi | lo] K segments against the split weight [wh | wl | wh] and its
        column scale.  Two planes (every matrix an fp16 value or FP8 / MXFP4 bytes): a weight has no low part, so a product is ONE
        library GEMM of the operand [xh; xl] (2 x rows rows) against the fp16 weight over K - two thirds of the flops, and
        no split copy of the weights at all; its [2, rows, N] result is summed by the reader (`slices`), the only scale
        left is the row's."""
        if self.bf16_value_resident:
            return self._forward_split_b3(resid, tok_pair, tok_pos, kc, vc, ctx_len, prefill_shape, keep_rows)
        m = self.cfg.llm
        rows, D = resid.shape
        planes = 2 if self.layer_kind in ("w16", "w8", "w4") else 3

        def plan(r, w, k3=False):                              # a pinned library algorithm, else the shape's table form
            if not self.plan_split:
                return None
            lt = None if _plan_measuring() else self._lt.plan(r, w.shape[0], w.shape[1], planes, k3)
            return lt or _plan_split_mm(r, w, k3=k3)
        if planes == 3:
            weight = lambda rec: rec.split                                                  # noqa: E731
            mm = lambda a3, w3, k3: _split_mm(a3, w3, plan(a3.shape[0], w3, k3=k3))         # noqa: E731
            split = ops.split_f16x3
        else:                                                  # W' = (the exact fp16 image) s, or an fp16 value: s = 1
            # (resident='quantised': the same operand, expanded right before its product)
            weight = lambda rec: (self._dense(rec, unscaled=True), rec.column_scale(self._ones))   # noqa: E731
            split = ops.split_f16x2

            def mm(a2, w16, k3):                               # a2 [2, r, K] -> raw product slices [S, r, N]
                r = a2.shape[1]
                y = _split_mm(a2.view(2 * r, a2.shape[2]), w16, plan(2 * r, w16, k3=k3))
                return y.view(-1, r, w16.shape[0])

        def proj(a, inv, rec, k3=False):                       # k3: the reader (rmsnorm_split) can sum K slices
            w, col = weight(rec)
            return ops.Scaled(mm(a, w, k3), inv, col)

        a, inv_r = ops.rmsnorm_split(resid, None, self.layers[0]["ln1"], m.rms_eps, planes=planes)
        q = torch.empty((rows, D), device=self.device, dtype=torch.float32)
        att = torch.empty_like(q)
        n = None
        for l, (L, M) in enumerate(zip(self.layers, self.mats)):
            qkv = proj(a, inv_r, M["wqkv"])
            ops.rope_kvwrite_scaled(qkv, tok_pair, tok_pos, self.rope, m.heads, m.head_dim, ctx_len, q, kc[l], vc[l],
                                    kv_heads=self.kv)
            ops.prefill_attn(q, kc[l], vc[l], tok_pos, prefill_shape[0], prefill_shape[1], m.heads, m.head_dim, ctx_len, att,
                             kv_heads=self.kv)
            last = l == len(self.layers) - 1
            if keep_rows is not None and last:
                att, resid = self._gather_kept(att, resid, keep_rows)
            ao, inv_o = split(att)                              # a row's maximum spans all heads: stays a kernel of its own
            o = proj(ao, inv_o, M["wo"], k3=True)
            a, inv_r = ops.rmsnorm_split(resid, o, L["ln2"], m.rms_eps, planes=planes)
            gu = proj(a, inv_r, M["wgu"])
            aa, inv_a = ops.silu_mul_split(gu, m.inter, planes=planes)
            d = proj(aa, inv_a, M["wdown"], k3=True)
            if last:                                            # the lm_head reads fp32 rows
                n = torch.empty_like(resid)
                ops.rmsnorm(resid, d.dense(), self.final_norm, m.rms_eps, n)
            else:
                a, inv_r = ops.rmsnorm_split(resid, d, self.layers[l + 1]["ln1"], m.rms_eps, planes=planes)
        return n

    def _forward_split_b3(self, resid, tok_pair, tok_pos, kc, vc, ctx_len, prefill_shape, keep_rows):
        """`_forward_split`'s third plane mode, bf16_value_resident: three bf16 planes of the fp32 rows against
        the bf16 copies.  RMSNorm and SwiGLU write the planes [3][rows][K] directly (no row maximum, no scale), a
        projection is ONE library product of the stacked planes (`_stacked_b3`: the flop count of the 3K product), and its
        three fp32 slices go to the reader as `ops.Partials`, summed (y2 + y1) + y0 while loading."""
        m = self.cfg.llm
        rows, D = resid.shape

        proj = self._stacked_b3                                # (whole: `_SPLIT_PLAN_TABLE` holds no measured bf16 shape)
        a = ops.rmsnorm_split_b16x3(resid, None, self.layers[0]["ln1"], m.rms_eps)
        q = torch.empty((rows, D), device=self.device, dtype=torch.float32)
        att = torch.empty_like(q)
        n = None
        for l, (L, M) in enumerate(zip(self.layers, self.mats)):
            ops.rope_kvwrite(proj(a, M["wqkv"]), tok_pair, tok_pos, self.rope, m.heads, m.head_dim, ctx_len, q, kc[l], vc[l],
                             kv_heads=self.kv)
            ops.prefill_attn(q, kc[l], vc[l], tok_pos, prefill_shape[0], prefill_shape[1], m.heads, m.head_dim, ctx_len, att,
                             kv_heads=self.kv)
            last = l == len(self.layers) - 1
            if keep_rows is not None and last:
                att, resid = self._gather_kept(att, resid, keep_rows)
            o = proj(ops.split_b16x3(att), M["wo"])
            gu = proj(ops.rmsnorm_split_b16x3(resid, o, L["ln2"], m.rms_eps), M["wgu"])
            d = proj(ops.silu_mul_split_b16x3(gu), M["wdown"])
            if last:                                            # the lm_head reads fp32 rows
                n = torch.empty_like(resid)
                ops.rmsnorm(resid, d, self.final_norm, m.rms_eps, n)
            else:
                a = ops.rmsnorm_split_b16x3(resid, d, self.layers[l + 1]["ln1"], m.rms_eps)
        return n

    @property
    def lt_gemm_pinned(self):
        """(lines of `_LT_ALGO_TABLE` in force for this engine, the reason the others are not): a table tuned for another
        library version, or a solution the library no longer offers, is visible here instead of silently falling back."""
        return self._lt.pinned

    def _can_persist(self, rows, slot):
        m = self.cfg.llm
        return (self.persistent_layer and self.use_skinny and slot == 0 and self.dtype == torch.float32
                and not self._any_quant and self.kv is None                           # the persistent decoder layer is multi-head only
                and ops.decode_layer_supported(rows, m.hidden, m.inter, m.heads, self.dtype, self.device))

    def _decode_step_persistent(self, st, counters):
        """One decode step on psg_decode_layers: ONE launch for the whole stack of decoder layers (chained inside the
        launch), then the final RMSNorm and the lm_head as in the chain.
        counters: int32 [layers * ops.decode_layer_counters()], zeroed."""
        m = self.cfg.llm
        x = st["x"]
        K = x.shape[0]
        ent = self._dl_ws.get(K)
        if ent is None:
            ws, _ = ops.decode_layer_workspace(K, m.hidden, m.inter, self.device)
            ent = self._dl_ws[K] = (ws, torch.empty((2, 16, K, m.hidden), device=self.device, dtype=torch.float32))
        ws, dparts = ent
        if "dl_table" not in st:                               # per decode state: the table holds its KV-cache pointers
            # (pinned staging + an async copy: capturable as a memcpy node, replayed with the graph)
            rows = ops.decode_layer_table(self.layers, st["kc"], st["vc"], device="cpu")
            host = self._dl_host_buf if self._dl_host_buf is not None else torch.empty_like(rows).pin_memory()
            self._dl_host_buf = None                           # (allocated by generate() BEFORE the capture began)
            host.copy_(rows)
            st["dl_table_host"] = host
            st["dl_table"] = torch.empty(host.shape, dtype=torch.int64, device=self.device)
            st["dl_table"].copy_(host, non_blocking=True)
        delta = ops.decode_layers(x, None, st["dl_table"], len(self.layers), st["dec_pair"], st["dec_pos"], self.rope, m.heads,
                                  st["ctx_len"], m.rms_eps, m.inter, ws, counters, dparts)
        n = torch.empty_like(x)
        ops.rmsnorm(x, delta, self.final_norm, m.rms_eps, n)
        return self.logits(n)

    def _can_pair(self, rows, kind, k_multiple):
        """fp32s decode steps of <= 32 rows with every projection on the two-plane entry of ONE stream (the decoder layers
        are of `kind`, `layer_kind`), the row kernels writing that operand directly (`_decode_step_split`).  k_multiple: the
        K step of the stream's kernel."""
        m = self.cfg.llm
        return (self.layer_kind == kind and self.prefill_split and self.use_skinny and self.fuse_split and rows <= 32
                and self.dtype == torch.float32 and m.hidden % k_multiple == 0 and m.inter % k_multiple == 0 and m.inter <= 16384
                and m.hidden <= 8192 and m.vocab % 16 == 0)

    def _can_w16(self, rows):
        """`_can_pair` over fp16-valued weights: psg_split_gemm_w16, 2 bytes per weight from HBM, two fp16 products per
        projection (high and low part of the fp32 rows) on the 16-bit matrix cores."""
        return self._can_pair(rows, "w16", 64)

    def _can_w8(self, rows):
        """`_can_pair` over FP8-quantised decoder layers: psg_split_gemm_w8, 1 byte per weight, the same two fp16 products on the exactly
        widened bytes, the per-row weight scale applied in fp32 where a slice is stored."""
        return self._can_pair(rows, "w8", 128)

    def _can_w4(self, rows):
        """`_can_pair` over MXFP4-quantised decoder layers: psg_split_gemm_w4 - or, for a shape of W4_STREAM_AS_FP8, psg_split_gemm_w8 on
        its exact FP8 image - 4.25 bits per weight, nibbles and block scale widened exactly to fp16 in registers."""
        return self._can_pair(rows, "w4", 256)

    def _can_int4(self, rows):
        """`_can_pair` over group-wise INT4 decoder layers, every one of which has its code stream (groups of 128, K % 256 == 0, none in
        INT4_STREAM_OFF): psg_split_gemm_int4, 4.25 bits per weight, the codes widened to the exact integers q - z in fp16,
        each group's sum scaled in fp32."""
        return self._can_pair(rows, "int4", 256)

    @property
    def bf16_stream_active(self):
        """Does a decode step of this engine stream bf16 copies (`bf16_value_stream` set AND the model qualifies)?"""
        return self._can_wb16(1)

    def _can_wb16(self, rows):
        """fp32s decode steps over bf16-valued decoder layers (option bf16_value_stream): every projection as
        psg_split_gemm_wb16 - 2 bytes per weight, three bf16 products (the exact three-plane form of the fp32 rows) - the row
        kernels writing its three-plane operand directly (`_decode_step_split`)."""
        return not self._wb16_blockers(rows)

    def _wb16_blockers(self, rows):
        """THE conditions of the 'wb16' decode route, as the reasons that hold against it (none: the route is open)."""
        m = self.cfg.llm
        off = [tuple(w.shape) for w in self._layer_mats() if tuple(w.shape) in WB16_STREAM_OFF]
        conditions = (
            (self.layer_kind == "wb16", f"the decoder layers are of kind {self.layer_kind!r}, not bf16 copies"),
            (self.prefill_split and self.dtype == torch.float32, "the engine is not an fp32s engine"),
            (self.use_skinny, "use_skinny is off"),
            (rows <= 32, f"{rows} rows exceed the 32 of the decode-step kernel"),
            (m.hidden % 64 == 0, f"hidden = {m.hidden} is no multiple of 64"),
            (m.inter % 64 == 0, f"inter = {m.inter} is no multiple of 64"),
            (m.hidden <= 8192, f"hidden = {m.hidden} exceeds 8192"),
            (self.qkv_width % 16 == 0, f"the q|k|v width {self.qkv_width} is no multiple of 16"),
            (not off, f"a decoder matrix of shape {off[:1]} is listed in WB16_STREAM_OFF"))
        return [why for ok, why in conditions if not ok]

    def _decode_route(self, rows, slot=0, per_call=True):
        """THE route of a decode step of `rows` rows: a key of `_STREAM_PLANES` (`_decode_step_split`), 'persist'
        (`_decode_step_persistent`), 'fused' (`_decode_step_fused`) or None - the launch chain of `_forward`.  The first
        that is possible, in this order.  per_call=False leaves out the two routes that need state made per `_steps` call
        (their counter blocks), which a call of no steps does not make."""
        if self._can_wb16(rows):                               # option bf16_value_stream: the user asked for the stream
            return "wb16"
        if per_call and self._can_persist(rows, slot):
            return "persist"
        for kind, can in (("w16", self._can_w16), ("w8", self._can_w8), ("w4", self._can_w4), ("int4", self._can_int4)):
            if can(rows):
                return kind
        return "fused" if per_call and self._can_fuse(rows) else None

    def _operand_form(self, planes, rows):
        """The row kernels that write the operand of the ops.split_gemm_* entries of `planes` planes directly:
        (norm(x, delta, ln), split(att), swiglu(gate|up)).  Each returns the operand as the tuple of arguments the entry
        takes before its weight.
        Two planes: (fp16 planes, row scale).  A row's maximum spans all heads / all `inter` columns, so attention and SwiGLU
        have a split launch of their own behind them; folding it into the producers needs a rendezvous of the row's 32 / 11
        workgroups - built and measured in round 6 (profiles/r06_split2_rendezvous_ab.txt): inside a graph the launch costs
        2.6 / 3.5 us, the rendezvous 9.3 / 3.4.
        Three planes: (bf16 planes,).  Element-wise, no row maximum: RMSNorm and SwiGLU write the planes themselves."""
        m = self.cfg.llm
        if planes == 3:
            return (lambda x, delta, ln: (ops.rmsnorm_split_b16x3(x, delta, ln, m.rms_eps),),
                    lambda att: (ops.split_b16x3(att),),
                    lambda gu: (ops.silu_mul_split_b16x3(gu),))

        def swiglu(gu):
            act = torch.empty((rows, m.inter), device=self.device, dtype=torch.float32)
            ops.silu_mul(gu, act)
            return ops.split_f16x2(act)
        return (lambda x, delta, ln: ops.rmsnorm_split2(x, delta, ln, m.rms_eps)), ops.split_f16x2, swiglu

    def _split_gemm(self, planes, operand, w):
        """The projection of a split operand of `planes` planes over `w` on the stream it has: ops.split_gemm_<kind>, looked
        up when it is called."""
        if w.stream is None or _STREAM_PLANES[w.stream[0]] != planes:
            raise PsgHipError(f"decode step: the matrix {tuple(w.shape)} has no stream that reads a {planes}-plane operand")
        return getattr(ops, "split_gemm_" + w.stream[0])(*operand, *w.stream[1])

    def _decode_step_split(self, st, kind):
        """One fp32s decode step of <= 32 rows on the route `kind` (a key of `_STREAM_PLANES`): every decoder projection as
        ops.split_gemm_<the stream its matrix has>, the row kernels writing that entry's split operand directly."""
        m = self.cfg.llm
        x = st["x"]
        rows, D = x.shape
        planes = _STREAM_PLANES[kind]
        norm, split, swiglu = self._operand_form(planes, rows)
        att = torch.empty((rows, D), device=self.device, dtype=torch.float32)
        a = norm(x, None, self.layers[0]["ln1"])
        for l, (L, M) in enumerate(zip(self.layers, self.mats)):
            qkv = self._split_gemm(planes, a, M["wqkv"])
            ops.decode_attn(qkv, st["dec_pair"], st["dec_pos"], self.rope, m.heads, m.head_dim, st["ctx_len"], st["kc"][l],
                            st["vc"][l], att, kv_heads=self.kv)
            o = self._split_gemm(planes, split(att), M["wo"])
            gu = self._split_gemm(planes, norm(x, o, L["ln2"]), M["wgu"])
            d = self._split_gemm(planes, swiglu(gu), M["wdown"])
            if l + 1 < len(self.layers):
                a = norm(x, d, self.layers[l + 1]["ln1"])
        return self._lm_head_tail(x, d, planes)

    def _lm_head_tail(self, x, delta, planes):
        """The final norm and the lm_head behind the last layer of `_decode_step_split`.  The lm_head runs on the stream ITS
        tensor has, the norm writing that stream's operand - where the stream takes the operand form of the step's route
        (`planes`), or is the fp16 copy.  Every other head runs as in the launch chain (fp32 rows, `logits`): one without a
        stream on its fp32 tensor, a quantised lm_head under bf16-valued layers on its own stream behind a split launch, and
        the bf16 copy of an lm_head under quantised layers is not streamed."""
        m = self.cfg.llm
        stream = self.lm_head_mat.stream
        if stream is not None and m.vocab % 16 == 0 and (_STREAM_PLANES[stream[0]] == planes or stream[0] == "w16"):
            planes = _STREAM_PLANES[stream[0]]
            norm = self._operand_form(planes, x.shape[0])[0]
            return self._split_gemm(planes, norm(x, delta, self.final_norm), self.lm_head_mat)
        n = torch.empty_like(x)
        ops.rmsnorm(x, delta, self.final_norm, m.rms_eps, n)
        return self.logits(n)

    def _can_fuse(self, rows):
        m = self.cfg.llm
        D = m.hidden
        return (bool(self.fuse_rowops) and not self._any_quant and self.use_skinny and self.dtype in (torch.bfloat16, torch.float16)
                and self.resid_dtype == self.dtype and rows <= 32 and D in (1024, 4096) and m.inter >= 1024 and m.inter % 64 == 0
                and m.vocab >= 1024 and m.vocab % 16 == 0)

    def _decode_step_fused(self, st, sync):
        """One decode step with the row operations named in `fuse_rowops` folded into the projection that consumes
        them (same arithmetic, same order: bit-identical to the separate kernels).  Returns the lm_head partials.
        sync: int32 [>= 2 * (4 * layers + 1)], zeroed."""
        m = self.cfg.llm
        x = st["x"]                                            # residual stream [K, D], embedding of the new tokens
        K = x.shape[0]
        n = torch.empty_like(x)
        att = torch.empty_like(x)
        act = torch.empty((K, m.inter), device=self.device, dtype=self.dtype)
        f = self.fuse_rowops
        slot = [0]

        def words():
            w = sync[2 * slot[0]:2 * slot[0] + 2]
            slot[0] += 1
            return w

        def norm_proj(delta, ln, w):                           # x += delta ; n = norm(x) ; n @ w.T
            if "rmsnorm" in f:
                return ops.skinny_gemm_fused(ops.PSG_PRO_RMSNORM, n, w, words(), inp=delta, resid=x, norm_w=ln,
                                             eps=m.rms_eps)
            ops.rmsnorm(x, delta, ln, m.rms_eps, n)
            return ops.skinny_gemm(n, w)

        delta = None
        for l, L in enumerate(self.layers):
            qkv = norm_proj(delta, L["ln1"], L["wqkv"])
            ops.decode_attn(qkv, st["dec_pair"], st["dec_pos"], self.rope, m.heads, m.head_dim, st["ctx_len"],
                            st["kc"][l], st["vc"][l], att, kv_heads=self.kv)
            o = ops.skinny_gemm(att, L["wo"])
            gu = norm_proj(o, L["ln2"], L["wgu"])
            ops.silu_mul(gu, act)
            delta = ops.skinny_gemm(act, L["wdown"])
        return norm_proj(delta, self.final_norm, self.lm_head)

    def build_inputs(self, pair_feature_rows, prompt_ids, prompt_len):
        """V4:294-301 for all K pairs.  pair_feature_rows [K*32, 768] (activation dtype),
        prompt_ids int32 [K, Tp] COMPACT (valid ids first, -1 after), prompt_len int32 [K].
        Returns X [K, 32+Tp, D]."""
        m = self.cfg.llm
        K, Tp = prompt_ids.shape
        nv = self.cfg.qformer.num_query
        X = torch.empty((K, nv + Tp, m.hidden), device=self.device, dtype=self.dtype)
        if self._dense_split(self.proj_mat):
            vis = self.linear_split(pair_feature_rows.contiguous(), self.proj_mat, bias=self.proj_b)
        else:                                                  # the exact library product: `linear_split`'s fallback is not
            vis = F.linear(pair_feature_rows, self.proj_mat.w, self.proj_b)
        X[:, :nv] = vis.view(K, nv, m.hidden)
        tok = torch.empty((K * Tp, m.hidden), device=self.device, dtype=self.dtype)
        ops.gather_rows(self.embed, prompt_ids.reshape(-1).contiguous(), tok)
        X[:, nv:] = tok.view(K, Tp, m.hidden)
        return X

    @torch.no_grad()
    def teacher_forcing_logits(self, X, seq_len, rope_pos, rows):
        """Training forward (V4:327-336: a plain `language_model(inputs_embeds, attention_mask)` call).
        X [K, S, D] COMPACT sequences (pads removed), seq_len int32 [K], rope_pos int32 [K*S] = each row's position
        in the reference's PADDED sequence (HF numbers positions 0..T-1 over pads in a plain forward), rows int32:
        flat row indices whose logits are wanted.  Returns logits [len(rows), vocab] in the activation dtype."""
        if self.resident == "quantised":
            raise PsgHipError("resident='quantised': the training forward would keep views of a scratch buffer that the next "
                              "product overwrites - train on an engine built with resident='all'")
        if self.bf16_value_resident:
            raise PsgHipError("bf16_value_resident: an inference mode - the training forward reads the fp32 tensors this engine "
                              "does not hold; train on an engine built with llm_bf16_value_resident=False")
        m = self.cfg.llm
        K, S, D = X.shape
        dev = self.device
        t = torch.arange(S, device=dev, dtype=torch.int32)[None, :].expand(K, -1)
        tok_pos = torch.where(t < seq_len[:, None].to(torch.int32), t, torch.full_like(t, -1)).reshape(-1).contiguous()
        tok_pair = torch.arange(K, device=dev, dtype=torch.int32)[:, None].expand(-1, S).reshape(-1).contiguous()
        kc = [torch.empty((K, m.n_kv_heads, S, m.head_dim), device=dev, dtype=self.dtype) for _ in self.layers]
        vc = [torch.empty((K, m.n_kv_heads, S, m.head_dim), device=dev, dtype=self.dtype) for _ in self.layers]
        resid = X.reshape(K * S, D).to(self.resid_dtype, copy=True)
        h = self._forward(resid, tok_pair, tok_pos, kc, vc, S, rope_pos=rope_pos.contiguous())
        h_rows = torch.empty((rows.numel(), D), device=dev, dtype=self.dtype)
        ops.gather_rows(h, rows.to(torch.int32).contiguous(), h_rows)
        return F.linear(h_rows, self.lm_head)

    @torch.no_grad()
    def generate(self, X, prompt_len, max_new_tokens=None, suppress_eos=False, return_first_logits=False, slot=0,
                 gate=None, defer=False, trie=None, constraint=None, path_logp=False, beam=None):
        """Batched greedy decode.  X [K, 32+Tp, D]; prompt_len int32 [K] (# of prompt tokens).
        Returns tokens int32 [K, max_new] (device; -1 after a pair's EOS) and optionally the
        first-step logits [K, vocab].

        The decode is captured in HIP graphs per input shape and replayed: nothing in it depends on
        the host (selection, argmax, EOS flags and positions all live on the device).
          * suppress_eos (benchmark worst case): ONE graph = prefill + max_new-1 steps (~5000 launches);
          * natural EOS: the reference's per-pair `generate` stops at EOS (V4:305-312), and a relation string
            is a handful of tokens, so the steps are cut into graphs of `early_exit_chunk` steps and the
            replay stops as soon as every pair has emitted EOS (one 4-byte read-back per chunk).
        slot: graphs (with their KV caches and static buffers) are kept per slot, so that two generations - of two
        images on two HIP streams, `head.submit` - can be in flight at once; a slot is used by one stream at a time.
        gate: callable run between the prompt pass (+ first token) and the decode steps, which are then separate graphs -
        the caller makes the stream wait there for the previous image's decode (the prompt pass of image k+1 is
        matrix-core work that fits beside image k's HBM-bound decode steps; two decodes side by side only share the HBM).
        defer (natural EOS only): enqueue the prompt pass and the first chunk of steps WITHOUT a host wait and return a
        callable instead of the results; calling it replays the remaining chunks (with their "all done?" read-backs) and
        returns what the direct call returns.  `head.submit` hands it to the pending result, so that `result()` stays
        the only host wait of an image in flight.
        trie (`rel_scores.RelationTrie`): the relation-likelihood pass runs inside the prompt-pass graph (`_rank_pass`)
        and the result gains a third entry, the log scores [K, R] (fp32) - returned as (tokens, first_logits, scores).
        constraint (`rel_scores.RelationTrie`): decode over the trie only - every step's arg-max runs over the
        children of the pair's trie node (`ops.trie_greedy_step`), so every pair emits exactly one candidate (a class name
        + EOS) in constraint.max_depth + 1 greedy steps: ONE graph, no early-exit chunks and no read-back.  path_logp: the
        log-probability of each pair's emitted sequence, fp32 [K], is appended to the result (behind the scores of
        `trie`, if any).
        beam (2..8, with constraint=): a beam of that width over the constraint's trie instead of the greedy
        walk - level 0 on the prompt's last rows, then constraint.max_depth levels of ONE forward over K x beam rows each
        (`_forward(decode=True, tree=...)`: the decode-step projections, psg_tree_attn over the trie slots behind the
        decode region) and one `ops.trie_beam_step`; ONE graph, no read-back.  Returns (beam_class int32 [K, beam] (-1
        padded), beam_logp fp32 [K, beam] (-inf padded)), best first, and nothing else."""
        max_new = self.cfg.max_new_tokens if max_new_tokens is None else max_new_tokens
        beam = None if beam is None or int(beam) == 1 else int(beam)
        if beam is not None:
            if constraint is None:
                raise PsgHipError(f"beam={beam} is a beam over a relation trie: it needs constraint=")
            if not 2 <= beam <= ops.BEAM_MAX_WIDTH:
                raise PsgHipError(f"beam={beam}: the beam width must be in 1..{ops.BEAM_MAX_WIDTH}")
            if trie is not None or path_logp or return_first_logits:
                raise PsgHipError(f"beam={beam} returns the beam's classes and scores only: trie=, path_logp and "
                                  "return_first_logits belong to the greedy decodes")
            if X.shape[0] * beam > 160:
                raise PsgHipError(f"beam decode: {X.shape[0]} pairs x beam {beam} = {X.shape[0] * beam} rows exceed the 160 rows "
                                  "of the decode-step kernels")
        n_steps = max_new
        if constraint is not None:
            n_steps = constraint.max_depth + 1
            if max_new < n_steps:
                raise PsgHipError(f"constrained decode: max_new_tokens={max_new} is below the trie's depth + 1 = {n_steps}: "
                                  "the longest candidate could not finish, and a truncated one parses to nothing")
            if suppress_eos:
                raise PsgHipError("constrained decode: a constrained sequence ends in EOS by definition (suppress_eos=True)")
        elif path_logp:
            raise PsgHipError("path_logp is the log-probability of a constrained decode's path: it needs constraint=")
        if not self.use_graph:
            outs = self._generate_eager(X, prompt_len, max_new, suppress_eos, return_first_logits, slot=slot, trie=trie,
                                        constraint=constraint, path_logp=path_logp, beam=beam)
            outs = outs if beam is not None else self._finish(outs, return_first_logits)
            return (lambda: outs) if defer else outs
        chunk = 0 if suppress_eos or constraint is not None else int(self.early_exit_chunk)
        split = gate is not None and n_steps > 1 and beam is None       # a beam is ONE graph: the gate is not called
        key = (tuple(X.shape), max_new, bool(suppress_eos), bool(return_first_logits), chunk, int(slot), split,
               bool(self.row_invariant))
        if trie is not None:
            key = key + (trie.key,)
        if constraint is not None:
            key = key + ("constraint", constraint.key, bool(path_logp))
        if beam is not None:
            key = key + (("beam", beam),)
        if self.bf16_value_stream:
            key = key + ("bf16_value_stream",)
        if self.bf16_value_resident:
            key = key + ("bf16_value_resident",)
        ent = self._graphs.get(key)
        if ent is not None:
            self._graphs.move_to_end(key)
        if ent is None:
            while len(self._graphs) >= self.max_graphs:        # least recently used shape: frees its graph pool
                # the evicted graph (or its KV pool) may still be replaying on another slot's stream
                torch.cuda.synchronize(self.device)
                self._graphs.popitem(last=False)
            Xs, ps = X.clone(), prompt_len.to(torch.int32).clone()
            if self.persistent_layer:                          # pinned staging of the layer table: not allocatable while capturing
                self._dl_host_buf = None
                pinned = torch.empty((len(self.layers), 8), dtype=torch.int64).pin_memory()
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):                      # warm-up: lazy library init must not be captured
                self._generate_eager(Xs, ps, max_new, suppress_eos, return_first_logits, slot=slot, trie=trie,
                                     constraint=constraint, path_logp=path_logp, beam=beam)
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            if self.persistent_layer:
                self._dl_host_buf = pinned
            bounds = [n_steps] if chunk <= 0 else list(range(chunk, max_new, chunk)) + [max_new]
            if split:                                          # the gate sits right behind the prompt pass + first token
                bounds = [1] + bounds
            bounds = sorted(set(bounds))
            graphs, st, lo = [], None, 0
            for hi in bounds:                                  # graph i runs steps [lo, hi); step 0 includes the prefill
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=graphs[0][0].pool() if graphs else None):
                    if st is None:
                        st = self._prefill(Xs, ps, max_new, suppress_eos, return_first_logits, slot=slot, trie=trie,
                                           constraint=constraint, path_logp=path_logp, beam=beam)
                        self._steps(st, 1, hi)
                    else:
                        self._steps(st, lo, hi)
                    all_done = st["done"].min() if (chunk > 0 and hi >= chunk) else None
                graphs.append((g, hi, all_done))
                lo = hi
            ent = self._graphs[key] = (graphs, Xs, ps, st)
        graphs, Xs, ps, st = ent
        Xs.copy_(X)
        ps.copy_(prompt_len)
        self.last_replays = 0
        cursor = [0]

        def advance(budget):
            """Replays graphs from the cursor on; budget = how many graphs may be enqueued without a read-back (None: run
            to the end, reading the all-done flag after every chunk)."""
            while cursor[0] < len(graphs):
                g, hi, all_done = graphs[cursor[0]]
                if budget is not None and cursor[0] >= budget:
                    return
                if cursor[0] == 1 and gate is not None:
                    gate()
                g.replay()
                cursor[0] += 1
                self.last_replays += 1
                if budget is None and hi < max_new and all_done is not None and int(all_done.item()) != 0:
                    break                                       # every pair has emitted EOS: the rest would be -1
            cursor[0] = len(graphs)

        def finish():
            advance(None)
            self._check_persistent(st)
            # the graph's static buffers are overwritten by the next replay: hand out copies
            if st.get("beam"):
                return st["fin_class"].clone(), st["fin_logp"].clone()
            fl = st["first_logits"]
            outs = (st["tokens"].clone(), None if fl is None else fl.clone())
            if st.get("rank") is not None:
                outs = outs + (st["rank"].clone(),)
            if st.get("logp") is not None:
                outs = outs + (st["logp"].clone(),)
            return self._finish(outs, return_first_logits)
        if defer and chunk > 0:
            advance(2 if split else 1)                          # prompt pass (+ gate) + the first chunk of steps: no host wait
            return finish
        outs = finish()
        return (lambda: outs) if defer else outs

    @staticmethod
    def _finish(outs, want_first):
        return outs if want_first or len(outs) > 2 else outs[0]

    def _check_persistent(self, st):
        """psg_decode_layer bounds every hand-off poll and reports a producer that never arrived through word
        PSG_DL_TIMEOUT of the launch's counter block (`ops.DL_TIMEOUT_WORD`).  Raises if any launch of this
        generation set it - its tokens are not to be trusted; the caller can switch `persistent_layer` off (the launch
        chain computes the same bits)."""
        for sync in st.get("dl_counters", ()):
            ncnt = ops.decode_layer_counters(self.device)
            if bool((sync.view(-1, ncnt)[:, ops.DL_TIMEOUT_WORD] != 0).any().item()):
                raise PsgHipError("psg_decode_layer: a hand-off poll timed out (cnt[PSG_DL_TIMEOUT] set); the tokens of this "
                                  "generation are invalid - disable option decode_persistent")

    def _generate_eager(self, X, prompt_len, max_new, suppress_eos, return_first_logits, slot=0, trie=None,
                        constraint=None, path_logp=False, beam=None):
        st = self._prefill(X, prompt_len, max_new, suppress_eos, return_first_logits, slot=slot, trie=trie,
                           constraint=constraint, path_logp=path_logp, beam=beam)
        self._steps(st, 1, max_new if constraint is None else constraint.max_depth + 1)
        if beam is not None:
            # below the deepest internal nodes there are only EOS leaves: the live pool is empty after the last level.
            # Checked once, never inside a capture
            if not torch.cuda.is_current_stream_capturing() and bool((st["node"] >= 0).any().item()):
                raise PsgHipError("beam decode: a hypothesis is still alive after max_depth + 1 levels (trie tables and beam "
                                  "state disagree)")
            return st["fin_class"], st["fin_logp"]
        if not torch.cuda.is_current_stream_capturing():
            self._check_persistent(st)
            # every path of the trie ends in an EOS leaf within max_depth + 1 edges: checked once, never inside a capture
            if constraint is not None and not bool(st["done"].all().item()):
                raise PsgHipError("constrained decode: a pair did not reach an EOS leaf of the trie in max_depth + 1 steps "
                                  "(trie tables and decode state disagree)")
        outs = (st["tokens"], st["first_logits"])
        if trie is not None:
            outs = outs + (st["rank"],)
        if st["logp"] is not None:
            outs = outs + (st["logp"],)
        return outs

    def _prefill(self, X, prompt_len, max_new, suppress_eos, return_first_logits, slot=0, trie=None, constraint=None,
                 path_logp=False, beam=None):
        """Prompt pass + first greedy token (+ the relation-likelihood pass over `trie`, whose rows own the cache slots
        behind the decode region).  Returns the decode state (KV caches, token / flag buffers)."""
        m = self.cfg.llm
        self._slot = int(slot)
        K, maxlen, D = X.shape
        nv = self.cfg.qformer.num_query
        # (a beam's rows own the trie slots behind the decode region, as the rows of the relation-likelihood pass do)
        slots = trie if trie is not None else (constraint if beam is not None else None)
        ctx_len = maxlen + max_new + (slots.n_int if slots is not None else 0)
        dev = self.device
        seq_len = (prompt_len.to(torch.int32) + nv)                                   # valid tokens per pair
        t = torch.arange(maxlen, device=dev, dtype=torch.int32)[None, :].expand(K, -1)
        tok_pos = torch.where(t < seq_len[:, None], t, torch.full_like(t, -1)).reshape(-1).contiguous()
        tok_pair = torch.arange(K, device=dev, dtype=torch.int32)[:, None].expand(-1, maxlen).reshape(-1).contiguous()
        # no zero fill (650 MB of stores per image for Llama-2-7B): every kernel reads only cache rows that were written
        kc = [torch.empty((K, m.n_kv_heads, ctx_len, m.head_dim), device=dev, dtype=self.dtype) for _ in self.layers]
        vc = [torch.empty((K, m.n_kv_heads, ctx_len, m.head_dim), device=dev, dtype=self.dtype) for _ in self.layers]
        resid = X.reshape(K * maxlen, D).to(self.resid_dtype, copy=True)
        last_rows = (torch.arange(K, device=dev, dtype=torch.int32) * maxlen + seq_len - 1).contiguous()
        h_last = self._forward(resid, tok_pair, tok_pos, kc, vc, ctx_len, prefill_shape=(K, maxlen), keep_rows=last_rows)
        logits = self.logits(h_last)
        first_logits = None
        if return_first_logits:
            first_logits = logits.reduce(self.dtype) if isinstance(logits, ops.Partials) else logits.to(self.dtype)
        rank = None
        if trie is not None:
            rank = self._rank_pass(logits, seq_len, kc, vc, ctx_len, maxlen, maxlen + max_new, trie)
        if beam is not None:
            return self._beam_root(logits, seq_len, kc, vc, ctx_len, maxlen, maxlen + max_new, constraint, beam, slot)
        tokens = torch.full((K, max_new), -1, device=dev, dtype=torch.int32)
        done = torch.zeros(K, device=dev, dtype=torch.int32)
        next_ids = torch.zeros(K, device=dev, dtype=torch.int32)
        dec_pos = (seq_len - 1).contiguous()                                           # greedy_step does += 1
        dec_pair = torch.arange(K, device=dev, dtype=torch.int32)
        sup = m.eos if suppress_eos else -1
        x = torch.empty((K, D), device=dev, dtype=self.resid_dtype)   # residual stream of the decode rows
        # the greedy step also writes the chosen token's embedding row into x: the next step's input, no gather launch
        node = logp = ctab = None
        if constraint is not None:                              # the same launch slot, the arg-max over the root's children
            ctab = constraint.device(dev)
            node = torch.zeros(K, device=dev, dtype=torch.int32)
            logp = torch.zeros(K, device=dev, dtype=torch.float32) if path_logp else None
            ops.trie_greedy_step(logits, 0, max_new, m.eos, ctab, node, tokens, done, next_ids, dec_pos, logp=logp,
                                 dtype=torch.float32 if self.exact_argmax else self.dtype, embed=self.embed, x_out=x)
        else:
            ops.greedy_step(logits, 0, max_new, m.eos, sup, tokens, done, next_ids, dec_pos,
                            dtype=torch.float32 if self.exact_argmax else self.dtype, embed=self.embed, x_out=x)
        return dict(node=node, logp=logp, con_trie=constraint, con_tables=ctab,     # kept alive with the graph, as rank_trie
                    kc=kc, vc=vc, ctx_len=ctx_len, tokens=tokens, done=done, next_ids=next_ids, dec_pos=dec_pos,
                    dec_pair=dec_pair, sup=sup, x=x, max_new=max_new, first_logits=first_logits, slot=int(slot), rank=rank,
                    # a captured graph reads the trie's device tables by address: the decode state (which the graph entry
                    # holds) keeps the trie and its tables alive as long as the graph, whatever becomes of the head's trie
                    rank_trie=trie, rank_tables=None if trie is None else trie.device(dev))

    def _beam_root(self, root_logits, seq_len, kc, vc, ctx_len, maxlen, base, trie, B, slot):
        """Level 0 of a beam of width B over `trie` on the prompt's last rows, and the state of its levels: row
        k * B + b is hypothesis b of pair k; a live row sits at an internal trie node, whose cache slot is base + node and
        whose rotary position is seq_len + depth - 1 (the slots and positions of `_rank_pass`)."""
        m = self.cfg.llm
        dev = self.device
        K = seq_len.numel()
        T = trie.device(dev)
        if base + trie.n_int > ctx_len:
            raise PsgHipError(f"beam decode: trie slots [{base}, {base + trie.n_int}) exceed the {ctx_len}-slot cache")
        i32 = dict(device=dev, dtype=torch.int32)
        node = torch.full((K, B), -1, **i32)
        node[:, 0] = 0                                            # one live hypothesis per pair: the root, score 0
        st = dict(beam=int(B), beam_tables=T, beam_trie=trie,     # kept alive with the graph (DESIGN 11's lifetime rule)
                  node=node.view(-1), logp=torch.zeros(K * B, device=dev, dtype=torch.float32),
                  fin_class=torch.full((K, B), -1, **i32),
                  fin_logp=torch.full((K, B), float("-inf"), device=dev, dtype=torch.float32),
                  row_node=torch.empty(K * B, **i32), tok_pos=torch.empty(K * B, **i32), rope_pos=torch.empty(K * B, **i32),
                  row_pair=torch.arange(K, **i32).repeat_interleave(B).contiguous(),
                  x=torch.empty((K * B, m.hidden), device=dev, dtype=self.resid_dtype), seq_len=seq_len.contiguous(),
                  kc=kc, vc=vc, ctx_len=ctx_len, base=int(base), slot=int(slot))
        st["tree"] = dict(row_node=st["row_node"], prefix_len=st["seq_len"], anc=T["anc"], base=int(base),
                          rope_bound=int(maxlen + trie.max_depth))
        self._beam_step(st, root_logits, 1)
        return st

    def _beam_step(self, st, logits, beams_in):
        ops.trie_beam_step(logits, st["beam"], beams_in, self.cfg.llm.eos, st["beam_tables"], st["base"], st["seq_len"],
                           st["node"], st["logp"], st["fin_class"], st["fin_logp"], st["row_node"], st["tok_pos"],
                           st["rope_pos"], embed=self.embed, x_out=st["x"])

    def _rank_pass(self, root_logits, seq_len, kc, vc, ctx_len, maxlen, base, trie):
        """The relation-likelihood pass: log s(p, r) for every selected pair p and every class r of `trie`.
        Every internal trie node is one row per pair - its token's embedding at rotary position seq_len + depth - 1, cache
        slot base + node - and ONE forward over all K x n_int rows runs every layer on them (projections through
        `linear`, as the prompt pass; attention over the pair's prompt slots and the node's trie ancestors,
        psg_tree_attn).  psg_token_logprobs turns the lm_head rows (and the prompt's last rows, `root_logits`) into the
        log-probabilities of the trie edges; a class's score is the sum over its path.  Static shapes, no host wait:
        captured with the prompt pass.  Returns fp32 [K, R]."""
        m = self.cfg.llm
        dev = self.device
        K = seq_len.numel()
        T = trie.device(dev)
        n, E = trie.n_int, trie.n_edges
        if base + n > ctx_len:
            raise PsgHipError(f"relation-likelihood pass: trie slots [{base}, {base + n}) exceed the {ctx_len}-slot cache")
        lp = torch.zeros((K, E + 1), device=dev, dtype=torch.float32)       # column E: the zero that pads the paths
        pair_ids = torch.arange(K, device=dev, dtype=torch.int32)
        ops.token_logprobs(root_logits, torch.zeros(K, device=dev, dtype=torch.int32),
                           pair_ids.to(torch.int64) * (E + 1), T["child_off"], T["child_tok"], lp)
        row_pair = pair_ids[:, None].expand(K, n).reshape(-1).contiguous()
        row_node = torch.arange(n, device=dev, dtype=torch.int32).repeat(K)
        tok_pos = (row_node + base).contiguous()
        rope_pos = (seq_len.to(torch.int32)[row_pair.long()] + T["node_depth"][row_node.long()] - 1).contiguous()
        ids = T["node_tok"][row_node.long()].contiguous()
        emb = torch.empty((K * n, m.hidden), device=dev, dtype=self.dtype)
        ops.gather_rows(self.embed, ids, emb)
        resid = emb.to(self.resid_dtype, copy=True)
        tree = dict(row_node=row_node, prefix_len=seq_len.to(torch.int32).contiguous(), anc=T["anc"], base=int(base),
                    rope_bound=int(maxlen + trie.max_depth))
        h = self._forward(resid, row_pair, tok_pos, kc, vc, ctx_len, rope_pos=rope_pos, tree=tree)
        if h.dtype == torch.float32:
            logits = self.logits(h, batch_stream=False)
        else:                                                  # fp32 logits of the 16-bit modes, ONE product (`logits` would
            logits = self._lm_head_f32(h)                      # run the 16-bit product first and discard it)
        row_out = (row_pair.to(torch.int64) * (E + 1) + T["child_off"][(row_node + 1).long()].to(torch.int64)).contiguous()
        ops.token_logprobs(logits, (row_node + 1).contiguous(), row_out, T["child_off"], T["child_tok"], lp)
        return lp[:, T["path"]].sum(-1)

    def _steps(self, st, lo, hi):
        """Decode steps lo .. hi-1 (step s writes tokens[:, s])."""
        m = self.cfg.llm
        self._slot = int(st.get("slot", 0))
        if st.get("beam"):                                     # level `step` of a beam: K x B rows at their trie nodes
            for step in range(lo, hi):
                h = self._forward(st["x"], st["row_pair"], st["tok_pos"], st["kc"], st["vc"], st["ctx_len"], decode=True,
                                  rope_pos=st["rope_pos"], tree=st["tree"])
                self._beam_step(st, self.logits(h), st["beam"])
            return
        route = self._decode_route(st["x"].shape[0], st.get("slot", 0), hi > lo)
        if route == "persist":                                 # one counter block per layer launch, zeroed once per call
            per_step = ops.decode_layer_counters(self.device) * len(self.layers)
            sync = torch.zeros((hi - lo) * per_step, device=self.device, dtype=torch.int32)
            # kept in the decode state: a hand-off poll that gave up reports through the block's time-out word, which
            # `generate` reads back with the tokens (`_check_persistent`) - a dead producer must not yield silent garbage
            st.setdefault("dl_counters", []).append(sync)
        if route == "fused":                                   # two counter words per fused launch, zeroed once per call
            per_step = 2 * (4 * len(self.layers) + 1)
            sync = torch.zeros((hi - lo) * per_step, device=self.device, dtype=torch.int32)
        for step in range(lo, hi):
            if route in _STREAM_PLANES:
                logits = self._decode_step_split(st, route)
            elif route == "persist":
                logits = self._decode_step_persistent(st, sync[(step - lo) * per_step:(step - lo + 1) * per_step])
            elif route == "fused":
                logits = self._decode_step_fused(st, sync[(step - lo) * per_step:(step - lo + 1) * per_step])
            else:
                h = self._forward(st["x"], st["dec_pair"], st["dec_pos"], st["kc"], st["vc"], st["ctx_len"], decode=True)
                logits = self.logits(h)
            if st.get("con_tables") is not None:
                ops.trie_greedy_step(logits, step, st["max_new"], m.eos, st["con_tables"], st["node"], st["tokens"],
                                     st["done"], st["next_ids"], st["dec_pos"], logp=st["logp"],
                                     dtype=torch.float32 if self.exact_argmax else self.dtype, embed=self.embed,
                                     x_out=st["x"])
                continue
            ops.greedy_step(logits, step, st["max_new"], m.eos, st["sup"], st["tokens"], st["done"], st["next_ids"],
                            st["dec_pos"], dtype=torch.float32 if self.exact_argmax else self.dtype, embed=self.embed,
                            x_out=st["x"])
