"""CPU side of the two-source GELU projection (K11's TWO form; reference navier_stokes_uno2d.py:121-125, 320-324): the stock-op form that
`gelu_project2` takes for CPU tensors against the float64 formula, forward and all five gradients, and the host-side argument checks of
the three C entry points (no device is touched: the library loads here as tests/test_capi_symbols.py loads it)."""
import ctypes
import math

import pytest
import torch

from conftest import rel_err


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def _formula(pre, s, w, b, act2):
    """out[b][p] = bias + sum_c w[c] gelu(pre[b][c][p]) + sum_d w[C1 + d] f(s[b][d][p]) in float64, written out"""
    C1 = pre.shape[1]
    out = torch.einsum("c,bc...->b...", w[0, :C1], _gelu64(pre)) + torch.einsum("d,bd...->b...", w[0, C1:], _gelu64(s) if act2 else s)
    return (out + b[0]).unsqueeze(1)


@pytest.mark.parametrize("act2", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 3, (3, 7)), (1, 1, 1, (1,)), (2, 12, 16, (9, 5, 2))])
def test_cpu_fallback_equals_the_float64_formula(shape, act2):
    from uno_amd.integral_operators import gelu_project2
    B, C1, C2, grid = shape
    g = torch.Generator().manual_seed(7)
    pre, s = torch.randn(B, C1, *grid, generator=g), torch.randn(B, C2, *grid, generator=g)
    w, b = torch.randn(1, C1 + C2, generator=g), torch.randn(1, generator=g)
    gout = torch.randn(B, 1, *grid, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (pre, s, w, b)]
    out = gelu_project2(*leaves, act2=act2)
    assert out.shape == (B, 1, *grid) and out.dtype == torch.float32
    grads = torch.autograd.grad(out, leaves, gout)
    leaves64 = [t.double().requires_grad_(True) for t in (pre, s, w, b)]
    ref = _formula(*leaves64, act2)
    refs = torch.autograd.grad(ref, leaves64, gout.double())
    # float32 stock ops against float64: sums of at most C1 + C2 = 28 terms (out) or B * pixels = 180 terms (gw, gb)
    assert rel_err(out.detach().numpy(), ref.detach().numpy()) < 2e-6
    for name, a, r in zip(("gpre", "gs", "gw", "gb"), grads, refs):
        assert a.shape == r.shape
        assert rel_err(a.numpy(), r.numpy()) < 2e-6, name
    # without bias, and with a second source that needs no gradient
    out = gelu_project2(leaves[0], s, leaves[2], None, act2=act2)
    assert rel_err(out.detach().numpy(), (ref - leaves64[3][0]).detach().numpy()) < 2e-6


def test_other_dtypes_and_wider_outputs_take_the_stock_form():
    from uno_amd.integral_operators import gelu_project2
    g = torch.Generator().manual_seed(8)
    pre, s = torch.randn(2, 4, 6, dtype=torch.float64, generator=g), torch.randn(2, 3, 6, dtype=torch.float64, generator=g)
    w, b = torch.randn(2, 7, dtype=torch.float64, generator=g), torch.randn(2, dtype=torch.float64, generator=g)
    out = gelu_project2(pre, s, w, b, act2=True)
    ref = torch.einsum("oc,bcp->bop", w, torch.cat([_gelu64(pre), _gelu64(s)], 1)) + b.view(1, 2, 1)
    assert out.shape == (2, 2, 6) and rel_err(out.numpy(), ref.numpy()) < 1e-14


@pytest.fixture(scope="module")
def lib():
    from uno_amd import build, _native
    build.build()
    return _native.lib()


def test_entry_points_are_bound_and_the_abi_version_stays(lib):
    from uno_amd import _native
    for name in ("uno_gelu_project2_forward", "uno_gelu_project2_bwd_ws_bytes", "uno_gelu_project2_backward"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.uno_abi_version() == 14


def test_argument_errors_are_reported_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    fwd, bwd, wsb = lib.uno_gelu_project2_forward, lib.uno_gelu_project2_backward, lib.uno_gelu_project2_bwd_ws_bytes

    def err(rc, needle):
        assert rc < 0 and needle in lib.uno_last_error(), (rc, lib.uno_last_error())

    err(fwd(p, p, p, nul, p, 1, 0, 3, 5, 0, None), b"bad sizes")                    # C1 < 1
    err(fwd(p, p, p, nul, p, 1, 3, 0, 5, 0, None), b"bad sizes")                    # C2 < 1
    err(fwd(p, p, p, nul, p, -1, 3, 2, 5, 0, None), b"bad sizes")
    err(fwd(p, p, p, nul, p, 1, 3, 2, -5, 0, None), b"bad sizes")
    err(fwd(p, p, p, nul, p, 1, 1000, 25, 5, 0, None), b"at most 1024")             # the channel limit (GP_MAXC)
    err(fwd(p, p, p, nul, p, 1, 3, 2, 5, 2, None), b"act2")
    err(fwd(nul, p, p, nul, p, 1, 3, 2, 5, 0, None), b"null")
    err(fwd(p, nul, p, nul, p, 1, 3, 2, 5, 1, None), b"null")                       # the second source
    err(fwd(p, p, nul, nul, p, 1, 3, 2, 5, 0, None), b"null")
    err(fwd(p, p, p, nul, nul, 1, 3, 2, 5, 0, None), b"null")
    err(fwd(p, p, p, nul, p, 70000, 3, 2, 5, 0, None), b"batch")                    # K11's own limits
    err(fwd(p, p, p, nul, p, 1, 3, 2, 1 << 31, 0, None), b"pixels")
    err(bwd(p, p, p, p, p, p, p, p, p, 1, 0, 3, 5, 0, None), b"bad sizes")
    err(bwd(p, p, p, p, p, p, p, p, p, 1, 600, 600, 5, 0, None), b"at most 1024")
    err(bwd(p, p, p, p, p, p, p, p, p, 1, 3, 2, 5, -1, None), b"act2")
    err(bwd(p, p, p, p, p, p, nul, p, p, 1, 3, 2, 5, 0, None), b"null")             # gw is required
    err(bwd(p, nul, p, p, p, p, p, p, p, 1, 3, 2, 5, 0, None), b"null")
    err(bwd(p, p, p, p, nul, p, p, p, p, 1, 3, 2, 5, 0, None), b"null")             # gpre is required (gs and gb are not)
    err(bwd(p, p, p, p, p, p, p, p, nul, 1, 3, 2, 5, 0, None), b"null")             # the workspace
    err(bwd(p, p, p, p, p, p, p, p, p, 70000, 3, 2, 5, 0, None), b"batch")
    # zero-sized problems succeed without touching the device
    assert fwd(nul, nul, nul, nul, nul, 0, 3, 2, 5, 0, None) == 0
    assert fwd(nul, nul, nul, nul, nul, 2, 3, 2, 0, 1, None) == 0
    # the workspace of the two-source call is that of a one-source call over C1 + C2 channels
    assert wsb(2, 40, 24, 5000) == lib.uno_gelu_project_bwd_ws_bytes(2, 64, 5000) > 0
    assert wsb(32, 12, 4, 4096) == lib.uno_gelu_project_bwd_ws_bytes(32, 16, 4096) > 0
    assert wsb(2, 0, 3, 10) == 0 and wsb(2, 1000, 25, 10) == 0


def test_binding_refuses_host_tensors_and_mismatched_sources():
    from uno_amd import _native
    pre, s, w = torch.zeros(1, 2, 4), torch.zeros(1, 3, 4), torch.zeros(5)
    with pytest.raises(RuntimeError, match="HIP device"):
        _native.gelu_project2_forward(pre, s, w)
    with pytest.raises(RuntimeError, match="HIP device"):
        _native.gelu_project2_backward(pre, s, w, torch.zeros(1, 4))
