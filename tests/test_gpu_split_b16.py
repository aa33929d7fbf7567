"""The row kernels of the bf16 value stream (`-m gpu`): psg_split_b16x3 against its torch restatement
(tests/split_b16_ref.py) bit for bit, and the two fused producers - psg_rmsnorm_split_b16x3, psg_silu_mul_split_b16x3 -
against the unfused pair (row kernel into fp32 rows, then psg_split_b16x3) bit for bit."""
import pytest
import torch

from tests.split_b16_ref import split_b16x3, wide_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("K", [64, 4096, 11008])
@pytest.mark.parametrize("rows", [1, 5, 20, 32])
def test_split_b16x3_equals_the_restatement_bit_for_bit(rows, K):
    from openpsg_amd import ops
    g = torch.Generator(device=DEV).manual_seed(rows * 13 + K)
    x = wide_rows(rows, K, g, DEV)
    x[0, :4] = torch.tensor([0.0, -0.0, torch.finfo(torch.float32).tiny, -torch.finfo(torch.float32).tiny], device=DEV)
    got = ops.split_b16x3(x)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (3, rows, K)
    assert torch.equal(got.view(torch.int16), split_b16x3(x).view(torch.int16))
    assert torch.equal(got.double().sum(0), x.double())
    if (rows, K) == (5, 4096):                                  # a row stride above K: the columns of a wider buffer
        wide = torch.full((rows, K + 192), float("nan"), device=DEV)
        wide[:, 64:64 + K] = x
        assert torch.equal(ops.split_b16x3(wide[:, 64:64 + K]).view(torch.int16), got.view(torch.int16))


@pytest.mark.parametrize("hidden", [512, 4096])
def test_fused_rmsnorm_equals_the_row_kernel_followed_by_the_split_bit_for_bit(hidden):
    from openpsg_amd import ops
    g = torch.Generator(device=DEV).manual_seed(hidden)
    w = 1.0 + 0.1 * torch.randn(hidden, generator=g, device=DEV)
    for rows in (1, 20, 32):
        for S in (0, 1, 4, 16):
            resid = torch.randn(rows, hidden, generator=g, device=DEV) * 3
            delta = ops.Partials(torch.randn(S, rows, hidden, generator=g, device=DEV).contiguous()) if S else None
            ra, rb = resid.clone(), resid.clone()
            n = torch.empty_like(ra)
            ops.rmsnorm(ra, delta, w, 1e-5, n)
            a3 = ops.split_b16x3(n)
            b3 = ops.rmsnorm_split_b16x3(rb, delta, w, 1e-5)
            assert torch.equal(ra, rb), (rows, hidden, S)
            assert torch.equal(a3.view(torch.int16), b3.view(torch.int16)), (rows, hidden, S)
            assert torch.equal(b3.double().sum(0), n.double())


@pytest.mark.parametrize("inter", [1024, 11008])
def test_fused_swiglu_equals_the_row_kernel_followed_by_the_split_bit_for_bit(inter):
    from openpsg_amd import ops
    g = torch.Generator(device=DEV).manual_seed(inter)
    for rows in (1, 20, 32):
        for S in (1, 4, 16):
            gu = ops.Partials((torch.randn(S, rows, 2 * inter, generator=g, device=DEV) * 2).contiguous())
            act = torch.empty((rows, inter), device=DEV)
            ops.silu_mul(gu, act)
            a3 = ops.split_b16x3(act)
            b3 = ops.silu_mul_split_b16x3(gu)
            assert torch.equal(a3.view(torch.int16), b3.view(torch.int16)), (rows, inter, S)
            assert torch.equal(b3.double().sum(0), act.double())
    dense = torch.randn(20, 2 * inter, generator=g, device=DEV)  # a dense fp32 gate|up (no slices)
    act = torch.empty((20, inter), device=DEV)
    ops.silu_mul(dense, act)
    assert torch.equal(ops.split_b16x3(act).view(torch.int16), ops.silu_mul_split_b16x3(dense).view(torch.int16))


def test_the_row_kernels_refuse_what_they_do_not_take():
    from openpsg_amd import ops
    from openpsg_amd._lib import PsgHipError
    x = torch.randn(4, 128, device=DEV)
    for call, match in (
            (lambda: ops.split_b16x3(x.half()), "x must be fp32"),
            (lambda: ops.split_b16x3(x.t()), "contiguous rows"),
            (lambda: ops.split_b16x3(x[:, :66]), "multiples of 4"),
            (lambda: ops.split_b16x3(x[:, 2:66]), "16-byte aligned"),
            (lambda: ops.rmsnorm_split_b16x3(x.half(), None, torch.ones(128, device=DEV), 1e-5), "x must be fp32"),
            (lambda: ops.rmsnorm_split_b16x3(x, x, torch.ones(128, device=DEV), 1e-5), "Partials"),
            (lambda: ops.rmsnorm_split_b16x3(x, ops.Partials(torch.zeros(2, 4, 64, device=DEV)), torch.ones(128, device=DEV),
                                             1e-5), "do not match"),
            (lambda: ops.rmsnorm_split_b16x3(x, None, torch.ones(64, device=DEV), 1e-5), "hidden is 128"),
            (lambda: ops.silu_mul_split_b16x3(x.half()), "gate_up must be fp32"),
            (lambda: ops.silu_mul_split_b16x3(x[:, :100].contiguous()), "gate_up must be fp32")):
        with pytest.raises(PsgHipError, match=match):
            call()
    resid = torch.full((3, 8196), -1234.5, device=DEV)          # above the row kernel's 8192 columns: refused, untouched
    with pytest.raises(PsgHipError, match="status -2"):
        ops.rmsnorm_split_b16x3(resid, None, torch.ones(8196, device=DEV), 1e-5)
    torch.cuda.synchronize()
    assert bool((resid == -1234.5).all())
