"""Float64 references, input families and derived bounds for the 16-bit GEMMs (psg_skinny_gemm in bf16 / fp16 and
psg_dense_gemm): what test_gpu_gemm16_ref.py checks the kernels against and test_gemm_ref_cpu.py checks on the CPU.
Pure torch, nothing here touches the GPU, and nothing here is written from the kernels (the helpers work on whatever
device their tensors live on).  The operands are the STORED 16-bit tensors converted to float64.

Two input families (make_x, make_w):

  exact    x and w hold integers in [-8, 8], drawn independently per element; bf16 and fp16 represent them exactly.  With
           K <= 2048 the magnitude sum A = |x| @ |w|^T is at most 64 K <= 2^17 < 2^24, so every product and every partial
           sum IN ANY ORDER is an integer below 2^24: exact in fp32.  The fp32 result - the split-K slices summed in fp32
           included - must therefore equal the integer product bit for bit (torch.equal), with no tolerance, for any
           accumulation order: a dropped, doubled or K-permuted element fails it.
  spread   x rows are randn * 2^linspace(-8, 8, M), w rows randn / sqrt(K) * 2^randint(-6, 6): 16 binades of row scales
           on one side, 12 on the other, every row of x and of w different (a swapped row cannot cancel).  Magnitudes
           below fp16's smallest normal 2^-14 are raised to it (sign kept) for BOTH types, so no operand is subnormal (or
           infinite) after the cast: the matrix cores see normal numbers only.

Bounds, per element, against float64 of the rounded operands (A = |x| @ |w|^T, plus |bias| where there is one):

  fp32 partials and fp32 outputs   2^-20 A.  The products of two 16-bit numbers are exact in fp32, so the error is the
           fp32 accumulation alone.  The constant is the one tests/test_gpu_gemm_w8.py holds the same MFMA chain to at K up
           to 11008.  `fp32_model` below is a deliberately pessimistic model of that chain (every product added to the
           running sum one at a time, front to back over the slice, the slices then summed): on the spread family it stays
           below 0.15 of the bound at every K from 64 to 2048 for 1 to 16 slices, while one dropped median-magnitude
           product lands 300 to 1700 times above it (test_gemm_ref_cpu.py asserts <= 0.5 and > 1).
  16-bit outputs   the spacing of the type at the reference (`_ulp` of rowops_ref_common: that file's convention) plus the
           fp32 bound.  Where |ref| + bound reaches past the type's largest finite number the kernel may round to
           infinity: check_out accepts the infinity of the reference's sign there.
  GELU     reference 0.5 v (1 + erf(v / sqrt 2)) in float64; bound 1.13 d + |v| (E + 16 * 2^-24) + (ulp for a 16-bit
           output): d the fp32 bound of the pre-activation v, 1.13 an upper limit of |gelu'| (its maximum is 1.129 at
           v = sqrt 2), E the maximum absolute error of the Abramowitz-Stegun 7.1.26 erf that dg_gelu evaluates
           (as_erf_max_error computes it against torch.special.erf on a dense grid; the self-test asserts E < 2e-7), and
           16 * 2^-24 |v| for the fp32 evaluation of that form (reciprocal, four fused steps, exp2, the final products).
  SwiGLU   out = rn(rn(silu(rn(g))) * rn(u)), rn = rounding to the 16-bit type (GEMM output, act_fn(gate), product: the
           documented roundings).  swiglu64 applies them to the float64 products; the kernel's fp32 g and u are within
           dg, du = 2^-20 A of the float64 ones, so its ROUNDED g and u are within dg + ulp, du + ulp (a rounding can
           flip); |silu'| <= 1.1, the fp32 silu adds 8 * 2^-24 |silu| and its rounding one more ulp; the product carries
           |u| dsg + |sg| du + dsg du and the last rounding one ulp at the reference's magnitude plus that slack.
"""
import math

import torch

from tests.rowops_ref_common import _ulp

DTYPES = (torch.bfloat16, torch.float16)
FAMILIES = ("exact", "spread")
NAMES = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
REL32 = 2.0 ** -20
FP16_MIN_NORMAL = 2.0 ** -14


# ---- reference ----
def ref64(x, w):
    """(x @ w^T, |x| @ |w|^T) in float64: the reference and its magnitude sum A"""
    xd, wd = x.double(), w.double()
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


# ---- inputs ----
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _no_subnormal(v):
    """magnitudes below fp16's smallest normal are raised to it, the sign kept (+ for zero)"""
    sign = torch.where(v < 0, -1.0, 1.0)
    return sign * v.abs().clamp_min(FP16_MIN_NORMAL)


def _assert_normal(t, dtype):
    a = t.double().abs()
    assert bool(torch.isfinite(a).all()), "an operand is infinite after the cast"
    assert bool((a >= FP16_MIN_NORMAL).all()), "an operand is zero or subnormal in fp16 after the cast"
    assert t.dtype == dtype


def make_x(family, M, K, dtype, seed=0):
    """activations [M, K] of `dtype` (on the CPU)"""
    g = _gen(1000003 * seed + 7919 * M + K)
    if family == "exact":
        assert K <= 2048, "exact family: K <= 2048 keeps A = |x| @ |w|^T <= 64 K below 2^24"
        return torch.randint(-8, 9, (M, K), generator=g).to(dtype)
    assert family == "spread", family
    scale = torch.exp2(torch.linspace(-8, 8, M, dtype=torch.float64))[:, None]
    x = _no_subnormal(torch.randn(M, K, generator=g, dtype=torch.float64) * scale).to(dtype)
    _assert_normal(x, dtype)
    return x


def make_w(family, N, K, dtype, seed=0):
    """weights [N, K] of `dtype` (on the CPU)"""
    g = _gen(1000003 * seed + 104729 * N + K + 1)
    if family == "exact":
        assert K <= 2048, "exact family: K <= 2048 keeps A = |x| @ |w|^T <= 64 K below 2^24"
        return torch.randint(-8, 9, (N, K), generator=g).to(dtype)
    assert family == "spread", family
    scale = torch.exp2(torch.randint(-6, 6, (N, 1), generator=g).double()) / math.sqrt(K)
    w = _no_subnormal(torch.randn(N, K, generator=g, dtype=torch.float64) * scale).to(dtype)
    _assert_normal(w, dtype)
    return w


def make_bias(family, N, seed=0):
    """fp32 bias [N]: integers in [-8, 8] (exact family: the sum stays an integer below 2^24) or randn"""
    g = _gen(1000003 * seed + 31 * N + 2)
    if family == "exact":
        return torch.randint(-8, 9, (N,), generator=g).float()
    return torch.randn(N, generator=g)


def assert_exact_range(A):
    """the exact family's premise: every partial sum in any order is an integer below 2^24"""
    assert float(A.max()) < 2.0 ** 24, f"exact family: A reaches {float(A.max()):.0f} >= 2^24"


# ---- bounds ----
def bound32(A):
    return REL32 * A


def bound_out(ref, A, dtype):
    """per-element bound of an output of `dtype` (fp32: the accumulation bound alone)"""
    return _ulp(ref, dtype) + bound32(A)


def worst(got, ref, bound):
    """max err / bound (a NaN or infinite result counts as infinitely wrong)"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bound.clamp_min(1e-300)).max())


def check_out(name, got, ref, bound, dtype=torch.float32):
    """assert |got - ref| <= bound per element; returns the worst ratio.  A 16-bit result may be the infinity of the
    reference's sign where |ref| + bound reaches past the type's largest finite number."""
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    g = got.double()
    if dtype != torch.float32:
        fmax = torch.finfo(dtype).max
        ref = ref.clamp(-fmax, fmax)                         # a reference that itself rounded to infinity
        over = (ref.abs() + bound >= fmax) & torch.isinf(g) & (torch.sign(g) == torch.sign(ref))
        g = torch.where(over, ref, g)
    ratio = worst(g, ref, bound)
    assert ratio <= 1.0, f"{name}: max err / bound = {ratio:.3g}"
    return ratio


# ---- GELU ----
def gelu64(v):
    return 0.5 * v * (1.0 + torch.special.erf(v / math.sqrt(2.0)))


def as_erf(x):
    """Abramowitz-Stegun 7.1.26 in float64: 1 - (a1 t + ... + a5 t^5) exp(-x^2), t = 1 / (1 + p |x|), odd in x"""
    ax = x.abs()
    t = 1.0 / (1.0 + 0.3275911 * ax)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    return torch.sign(x) * (1.0 - poly * torch.exp(-ax * ax))


_E = []


def as_erf_max_error():
    """E: max |as_erf - erf| on a dense grid over [-6, 6] (beyond it both are 1 to 1e-16)"""
    if not _E:
        x = torch.linspace(-6.0, 6.0, 1200001, dtype=torch.float64)
        _E.append(float((as_erf(x) - torch.special.erf(x)).abs().max()))
    return _E[0]


def gelu_bound(v, d, dtype):
    """bound of gelu computed in fp32 by the 7.1.26 form from a pre-activation within d of v (float64)"""
    ref = gelu64(v)
    return 1.13 * d + v.abs() * (as_erf_max_error() + 16 * 2.0 ** -24) + _ulp(ref, dtype)


# ---- SwiGLU ----
def _rn(v, dtype):
    return v.to(dtype).double()


def swiglu64(g, u, Ag, Au, dtype):
    """(reference with the documented roundings, bound) from the float64 gate / up products and their magnitude sums"""
    dg, du = bound32(Ag) + _ulp(g, dtype), bound32(Au) + _ulp(u, dtype)
    gr, ur = _rn(g, dtype), _rn(u, dtype)
    sg = gr * torch.sigmoid(gr)
    dsg = 1.1 * dg + 8 * 2.0 ** -24 * sg.abs()
    dsg = dsg + _ulp(sg.abs() + dsg, dtype)
    sgr = _rn(sg, dtype)
    slack = ur.abs() * dsg + sgr.abs() * du + dsg * du
    prod = sgr * ur
    ref = _rn(prod, dtype)                                   # +-inf where the product overflows the type: see check_out
    return ref, slack + _ulp((prod.abs() + slack).clamp_max(torch.finfo(dtype).max), dtype)


# ---- a pessimistic fp32 model of the accumulation ----
def k_slices(K, slices):
    """the K ranges of the split-K slices: blocks of 64, slice s owns blocks [KB s / S, KB (s + 1) / S)"""
    KB = K // 64
    assert K % 64 == 0 and 1 <= slices <= KB
    return [(64 * (KB * s // slices), 64 * (KB * (s + 1) // slices)) for s in range(slices)]


def fp32_model(x, w, slices=1, drop=None):
    """fp32 partials [slices, M, N] of x @ w^T with every product (exact in fp32) added to the running fp32 sum one at a
    time, front to back over the slice - longer rounding chains than any MFMA order.  drop = (m, n, k): that one product
    is left out (a mutant)."""
    xf, wf = x.float(), w.float()
    M, K = xf.shape
    out = torch.zeros(slices, M, w.shape[0], dtype=torch.float32)
    for s, (k0, k1) in enumerate(k_slices(K, slices)):
        acc = out[s]
        for k in range(k0, k1):
            p = xf[:, k, None] * wf[None, :, k]
            if drop is not None and drop[2] == k:
                p[drop[0], drop[1]] = 0.0
            acc += p
    return out


def sum_slices(part):
    """the consumers' reduction: the slices added in split order in fp32"""
    acc = part[0].clone()
    for s in range(1, part.shape[0]):
        acc += part[s]
    return acc
