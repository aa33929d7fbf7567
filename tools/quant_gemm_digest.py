"""Bit digests of the weight-streaming GEMM families (psg_gemm_w8 / _w4 / _int4, psg_batch_gemm_q, psg_batch_gemm) on one
MI355X: every entry point x plan mode x a few shapes and row counts is called ONCE and `splits` plus the SHA-256 of the
bytes of its fp32 slices - all slots, the zero-filled ones included - are recorded.  A changed grid, range, slot rank,
summation order or scale order shows here even where the tolerance tests would pass, so two trees that must compute the
same bits are compared by running this file on both (it uses the `ops` API only) and diffing the outputs:

    python tools/quant_gemm_digest.py [--out profiles/quant_gemm_digest.json]
    python tools/quant_gemm_digest.py --compare A.json B.json

Every input comes from a seeded CPU generator, so the inputs do not depend on the tree.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MODES = (0, 1, 2)
ROWS32, ROWS_BATCH = (1, 20, 32), (33, 80, 160)
BATCH_SHAPES = ((272, 768), (4096, 11008))


def _shapes32(bk):
    """N, K of the 32-row families, bk = the family's K granule: one unit with N below a wave's 32 rows, an odd unit count
    with a ragged last slab, a long K walk of one slab, a Llama-2-7B down projection."""
    return ((16, bk), (272, 3 * bk), (48, 4096), (4096, 11008))


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % 2 ** 31)


def _bytes(shape, g, lo=0, hi=256):
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(torch.uint8)


def _x(M, K, dev):
    """fp32 rows of very different magnitudes; (planes, inv_scale), bf16 rows, fp16 rows"""
    from openpsg_amd import ops
    x = torch.randn(M, K, generator=_gen(7, M, K)) * torch.logspace(-3, 2, M)[:, None]
    xd = x.to(dev)
    return ops.split_f16x2(xd), xd.bfloat16(), xd.half()


def _weights(N, K, dev):
    """the operands of every family for one shape (those whose K granule divides K), from CPU generators"""
    from openpsg_amd import ops
    w = {}
    g = _gen(1, N, K)
    s = (torch.exp2(torch.rand(N, generator=g) * 17 - 14) * 0.977).to(dev)
    w16 = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    w["w16"] = (w16.to(dev), w16.bfloat16().to(dev))
    if K % 128 == 0:
        q = _bytes((N, K), g)
        q = torch.where((q & 0x7F) == 0x7F, q - 1, q)                           # 0x7F / 0xFF (NaN) -> +-448
        w["w8"] = (q.to(dev), s)
    if K % 256 == 0:
        w["w4"] = (_bytes((N, K // 2), g).to(dev), ops.mxfp4_exp_image(_bytes((N, K // 32), g, 114, 128).to(dev)), s)
        gs = (torch.randn(N, K // 128, generator=g) * 0.01).half()
        gs = torch.where(gs.abs() < 2.0 ** -14, torch.full_like(gs, 2.0 ** -10), gs)
        gz = _bytes((N, K // 128), g, 0, 16)
        w["int4"] = (ops.int4_q_image(_bytes((N, K // 2), g).to(dev)), ops.int4_group_image(gs.to(dev), gz.to(dev)))
    return w


def _record(out, name, part):
    torch.cuda.synchronize()
    out[name] = dict(splits=int(part.splits), sha256=hashlib.sha256(part.t.contiguous().cpu().numpy().tobytes()).hexdigest())


def digests():
    from openpsg_amd import ops
    dev = torch.device("cuda", 0)
    out = {}
    shapes = sorted(set(_shapes32(64) + _shapes32(128) + _shapes32(256)))
    for N, K in shapes:
        w = _weights(N, K, dev)
        for M in ROWS32:
            (x2, inv), xb, xh = _x(M, K, dev)
            for mode in MODES:
                tag = f"M={M} N={N} K={K} mode={mode}"
                if (N, K) in _shapes32(64):
                    _record(out, f"split_gemm_w16 {tag}", ops.split_gemm_w16(x2, inv, w["w16"][0], mode))
                if (N, K) in _shapes32(128):
                    _record(out, f"split_gemm_w8 {tag}", ops.split_gemm_w8(x2, inv, *w["w8"], mode))
                    _record(out, f"skinny_gemm_w8 bf16 {tag}", ops.skinny_gemm_w8(xb, *w["w8"], mode))
                    _record(out, f"skinny_gemm_w8 fp16 {tag}", ops.skinny_gemm_w8(xh, *w["w8"], mode))
                if (N, K) in _shapes32(256):
                    _record(out, f"split_gemm_w4 {tag}", ops.split_gemm_w4(x2, inv, *w["w4"], mode))
                    _record(out, f"skinny_gemm_w4 bf16 {tag}", ops.skinny_gemm_w4(xb, *w["w4"], mode))
                    _record(out, f"skinny_gemm_w4 fp16 {tag}", ops.skinny_gemm_w4(xh, *w["w4"], mode))
                    _record(out, f"split_gemm_int4 {tag}", ops.split_gemm_int4(x2, inv, *w["int4"], mode))
                    _record(out, f"skinny_gemm_int4 bf16 {tag}", ops.skinny_gemm_int4(xb, *w["int4"], mode))
                    _record(out, f"skinny_gemm_int4 fp16 {tag}", ops.skinny_gemm_int4(xh, *w["int4"], mode))
        del w
        torch.cuda.empty_cache()
    for N, K in BATCH_SHAPES:
        w = _weights(N, K, dev)
        for M in ROWS_BATCH:
            (x2, inv), xb, xh = _x(M, K, dev)
            for mode in MODES:
                tag = f"M={M} N={N} K={K} mode={mode}"
                _record(out, f"batch_split_gemm_w8 {tag}", ops.batch_split_gemm_w8(x2, inv, *w["w8"], mode))
                _record(out, f"batch_split_gemm_w4 {tag}", ops.batch_split_gemm_w4(x2, inv, *w["w4"], mode))
                for dt, x, w16 in (("bf16", xb, w["w16"][1]), ("fp16", xh, w["w16"][0])):
                    _record(out, f"batch_gemm_w8 {dt} {tag}", ops.batch_gemm_w8(x, *w["w8"], mode))
                    _record(out, f"batch_gemm_w4 {dt} {tag}", ops.batch_gemm_w4(x, *w["w4"], mode))
                    for slab in (128, 256):
                        _record(out, f"batch_gemm {dt} slab={slab} {tag}", ops.batch_gemm(x, w16, slab, mode))
        del w
        torch.cuda.empty_cache()
    return out


def compare(a, b):
    ca, cb = json.load(open(a))["cases"], json.load(open(b))["cases"]
    bad = sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))
    for k in bad:
        print("DIFFERENT", k, ca.get(k), cb.get(k))
    print(f"{len(ca)} / {len(cb)} cases, {len(bad)} different")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quant_gemm_digest.json"))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    from openpsg_amd import _lib
    res = dict(device=_lib.device_info(0), cases=digests())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print(f"wrote {a.out}: {len(res['cases'])} cases")


if __name__ == "__main__":
    main()
