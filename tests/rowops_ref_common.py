"""What the float64-reference tests of the row kernels share (test_gpu_rowops_ref.py: the Q-Former side,
test_gpu_llm_rowops_ref.py: the LLM side): the spacing of a 16-bit format at a reference value, the error / bound check
and the sentinel-filled output buffer."""
import torch


def _ulp(ref, dtype):
    """spacing of `dtype` at |ref| (float64 in, float64 out); fp32 -> 0 (fp32 outputs carry their own bound)"""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    a = ref.abs().to(dtype).double()
    _, e = torch.frexp(a)                                           # a = m 2^e, m in [0.5, 1)
    e = torch.where(a > 0, e - 1, torch.full_like(e, emin)).clamp_min(emin)
    return torch.exp2((e - mant).double())


def _check(name, got, ref, bound):
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    assert ratio <= 1.0, (f"{name}: max err / bound = {ratio:.3g} (max err {err.max().item():.3g}, "
                          f"at {tuple(int(i) for i in torch.nonzero(~(err <= bound))[0])})")
    return ratio


def _sentinel(rows, cols, dtype, dev, extra=5):
    """an output buffer of rows + extra rows, filled with a value no kernel writes; returns (buffer, pristine copy)"""
    buf = torch.full((rows + extra, cols), -1234.5, device=dev, dtype=dtype)
    return buf, buf.clone()
