"""The oracle in float64: what tests/test_hip_workload_parity.py uses as its high-precision reference.  The FFT-sequence forms
keep the input's precision end to end (out_ft takes the spectrum's dtype) and so.to_float64() casts the complex weights, which
nn.Module.double() leaves in single precision.  Checked against the dense float64 closed forms, which involve no FFT library."""
import numpy as np
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import spectral_oracle as so


def test_float64_block_2d_matches_the_dense_form():
    torch.manual_seed(3)
    blk32 = so.OracleOperatorBlock2d(3, 5, 12, 10, 4, 3)
    blk = so.to_float64(blk32)
    assert all(p.dtype in (torch.float64, torch.complex128) for p in blk.parameters())
    assert all(p.dtype in (torch.float32, torch.complex64) for p in blk32.parameters())         # a copy: the source is untouched
    for (k, p), (_, q) in zip(blk.named_parameters(), blk32.named_parameters()):
        assert torch.equal(p.detach(), q.detach().to(p.dtype)), k                                # the float32 values, cast up
    x = torch.randn(2, 3, 16, 14, dtype=torch.float64, requires_grad=True)
    y = blk(x, 12, 10)
    assert y.dtype == torch.float64
    ys = blk.conv(x, 12, 10)
    assert ys.dtype == torch.float64
    dense, _ = so.spectral_conv2d_dense(x.detach().numpy(), blk.conv.weights1.detach().numpy(), blk.conv.weights2.detach().numpy(), 12, 10)
    assert rel_err(ys.detach().numpy(), dense) < 1e-12
    pw = so.pointwise2d(x.detach(), blk.w.conv.weight, blk.w.conv.bias, 12, 10)
    assert rel_err(y.detach().numpy(), F.gelu(torch.from_numpy(dense) + pw).detach().numpy()) < 1e-12
    y.sum().backward()
    assert x.grad.dtype == torch.float64 and blk.conv.weights1.grad.dtype == torch.complex128
    # float32 input: unchanged behaviour (cfloat spectrum, float32 result)
    assert blk32(x.detach().float(), 12, 10).dtype == torch.float32


def test_float64_block_3d_matches_the_dense_form():
    torch.manual_seed(4)
    blk = so.to_float64(so.OracleOperatorBlock3d(2, 3, 8, 8, 6, 3, 2, 2, Normalize=True))
    x = torch.randn(2, 2, 10, 8, 8, dtype=torch.float64, requires_grad=True)
    y = blk(x, 8, 8, 6)
    assert y.dtype == torch.float64
    ys = blk.conv(x, 8, 8, 6)
    ws = [getattr(blk.conv, f"weights{k}").detach().numpy() for k in range(1, 5)]
    assert ws[0].dtype == np.complex128
    dense, _ = so.spectral_conv3d_dense(x.detach().numpy(), ws, 8, 8, 6)
    assert ys.dtype == torch.float64 and rel_err(ys.detach().numpy(), dense) < 1e-12
    pw = so.pointwise3d(x.detach(), blk.w.conv.weight, blk.w.conv.bias, 8, 8, 6)
    ref = F.gelu(blk.normalize_layer(torch.from_numpy(dense) + pw))
    assert rel_err(y.detach().numpy(), ref.detach().numpy()) < 1e-12
    y.sum().backward()
    assert x.grad.dtype == torch.float64 and blk.conv.weights4.grad.dtype == torch.complex128
