"""Torch restatement of psg_split_b16x3 (openpsg_amd/csrc/psg_split_b16.h): an fp32 value as three bf16 values,

    x0 = bf16(x)    x1 = bf16(x - x0)    x2 = bf16(x - x0 - x1)        (round to nearest even)

Both differences are exact in fp32 (x - x0 has <= 16 significant bits, x - x0 - x1 <= 8), so x0 + x1 + x2 == x exactly as
long as x's lowest set bit is >= 2^-133, bf16's smallest subnormal - every |x| >= 2^-110, and every bf16-representable x
below that.  `.bfloat16()` rounds to nearest even on the CPU and the GPU alike."""
import torch


def split_b16x3(x: torch.Tensor) -> torch.Tensor:
    """fp32 [..., K] -> bf16 [3, ..., K]"""
    assert x.dtype == torch.float32
    x0 = x.bfloat16()
    r1 = x - x0.float()
    x1 = r1.bfloat16()
    r2 = r1 - x1.float()
    return torch.stack([x0, x1, r2.bfloat16()])


def bf16_valued(shape, gen, lo=-30, hi=3, device="cpu"):
    """fp32 tensor of bf16 VALUES with magnitudes spread over 2^lo .. 2^hi: such a tensor fails the fp16 round trip (values
    below fp16's subnormal grid 2^-24 lose bits or vanish)."""
    m = torch.randn(shape, generator=gen, device=device)
    e = torch.randint(lo, hi + 1, shape, generator=gen, device=device).float()
    return (m * torch.exp2(e)).bfloat16().float()


def wide_rows(rows, K, gen, device="cpu"):
    """fp32 rows whose magnitudes span 1e-6 .. 1e3 from the first to the last row."""
    scale = torch.logspace(-6, 3, rows, device=device) if rows > 1 else torch.ones(1, device=device)
    return torch.randn(rows, K, generator=gen, device=device) * scale[:, None]
