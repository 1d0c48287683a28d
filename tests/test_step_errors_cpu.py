"""The per-time-step error metric of the NS-3D loop (reference ns_train_3d.py:55-62, 84-98) without a GPU: the stock path of
harness.step_errors against the reference's own numbers (stored with the model goldens, tools/gen_golden_ns3d_models.py), the
`with_step_error` form of ns3d_loss, and the argument checks of uno_rel_l2_steps (no launch: as tests/test_capi_symbols.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Case, load_cases
from oracle import spectral_oracle as so
from uno_amd.harness import StepErrors, Uno3D_T10, ns3d_loss, ns3d_step_error, step_errors

Z10, _ = load_cases("harness_ns3d_t10.npz")
Z9, _ = load_cases("harness_ns3d_t9.npz")
CASES = {"t10": Z10, "t10both": Z10, "t9": Z9}
TOL = 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_stock_path_reproduces_the_reference_metric(name):
    c = Case(CASES[name], name)
    pred, yy = torch.from_numpy(c.pred), torch.from_numpy(c.yy)
    r = step_errors(pred, yy)
    assert isinstance(r, StepErrors)
    B, T = pred.shape[0], pred.shape[-1]
    assert r.sums.shape == (B, T, 2) and r.per_step.shape == (B, T) and r.full.shape == (B,) and r.step_sum.dim() == 0 and r.full_sum.dim() == 0
    e_step = abs(float(r.step_sum) - float(c.step_err64)) / float(c.step_err64)
    e_full = abs(float(r.full_sum) - float(c.full_err64)) / float(c.full_err64)
    e_each = float(np.max(np.abs(r.per_step.numpy() - c.per_step64) / c.per_step64))
    print(f"[{name}] step {e_step:.2e}, full {e_full:.2e}, per step {e_each:.2e}")
    assert e_step <= TOL and e_full <= TOL and e_each <= TOL
    # the float32 numbers the reference's loop itself computes are as close
    assert abs(float(r.step_sum) - float(c.step_err)) <= TOL * float(c.step_err)
    assert abs(float(r.full_sum) - float(c.full_err)) <= TOL * float(c.full_err)
    # sums are what per_step and full are made of
    p64, y64 = pred.double(), yy.double()
    num = ((p64 - y64) ** 2).reshape(B, -1, T).sum(1)
    den = (y64 ** 2).reshape(B, -1, T).sum(1)
    assert torch.allclose(r.sums[..., 0].double(), num, rtol=TOL, atol=0) and torch.allclose(r.sums[..., 1].double(), den, rtol=TOL, atol=0)
    assert torch.allclose(r.full.double(), num.sum(1).sqrt() / den.sum(1).sqrt(), rtol=TOL, atol=0)
    assert float(ns3d_step_error(pred, yy)) == float(r.step_sum)


def test_stock_path_takes_other_dtypes_and_long_time_axes():
    g = torch.Generator().manual_seed(2)
    pred, y = torch.randn(2, 5, 3, 257, generator=g), torch.randn(2, 5, 3, 257, generator=g)
    r = step_errors(pred, y)
    r64 = step_errors(pred.double(), y.double())
    assert r64.per_step.dtype == torch.float64 and r.per_step.shape == (2, 257)
    assert torch.allclose(r.per_step.double(), r64.per_step, rtol=TOL, atol=0)
    assert abs(float(r.step_sum) - float(r64.step_sum)) <= TOL * float(r64.step_sum)
    with pytest.raises(RuntimeError):
        step_errors(pred, y[..., :256])


def test_ns3d_loss_with_step_error_keeps_the_loss_and_adds_the_metric():
    c = Case(Z10, "t10")
    torch.manual_seed(int(c.seed))
    model = Uno3D_T10(6, 2, pad=3, block_cls=so.OracleOperatorBlock3d)
    xx, yy = torch.from_numpy(c.xx), torch.from_numpy(c.yy)
    plain = ns3d_loss(model, xx, yy)
    loss, err = ns3d_loss(model, xx, yy, with_step_error=True)
    assert torch.equal(plain.detach(), loss.detach()) and loss.requires_grad
    assert err.dim() == 0 and not err.requires_grad
    assert abs(float(err) - float(c.step_err64)) <= TOL * float(c.step_err64)


def test_ns3d_evaluate_sums_the_batches_and_restores_the_mode():
    from uno_amd.harness import ns3d_evaluate
    c = Case(Z10, "t10")
    torch.manual_seed(int(c.seed))
    model = Uno3D_T10(6, 2, pad=3, block_cls=so.OracleOperatorBlock3d)
    xx, yy = torch.from_numpy(c.xx), torch.from_numpy(c.yy)
    model.train()
    total = ns3d_evaluate(model, [(xx[:1], yy[:1]), (xx[1:], yy[1:])])
    assert model.training and not total.requires_grad
    assert abs(float(total) - float(c.step_err64)) <= TOL * float(c.step_err64)
    model.eval()
    ns3d_evaluate(model, [(xx[:1], yy[:1])])
    assert not model.training


@pytest.fixture(scope="module")
def lib():
    from uno_amd import build, _native
    build.build()
    return _native.lib()


def test_argument_errors_are_reported_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    for k in range(6):                      # each pointer in turn
        ptrs = [nul if i == k else p for i in range(6)]
        assert lib.uno_rel_l2_steps(*ptrs, 1, 4, 3, None) < 0 and b"null" in lib.uno_last_error()
    assert lib.uno_rel_l2_steps(p, p, p, p, p, p, 1, 4, 0, None) < 0 and b"bad sizes" in lib.uno_last_error()
    assert lib.uno_rel_l2_steps(p, p, p, p, p, p, 1, 4, 257, None) < 0 and b"at most 256" in lib.uno_last_error()
    assert lib.uno_rel_l2_steps(p, p, p, p, p, p, 1, 0, 3, None) < 0 and b"bad sizes" in lib.uno_last_error()
    assert lib.uno_rel_l2_steps(p, p, p, p, p, p, -1, 4, 3, None) < 0 and b"bad sizes" in lib.uno_last_error()
    # an empty batch is a no-op that succeeds without touching the device
    assert lib.uno_rel_l2_steps(nul, nul, nul, nul, nul, nul, 0, 4, 3, None) == 0


def test_workspace_size_is_positive_and_never_shrinks_with_the_pixel_count(lib):
    for T in (1, 9, 13, 40, 255, 256):
        last = 0
        for P in (1, 2, 49, 300, 4096, 4097, 20011, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 24, 1 << 31):
            ws = lib.uno_rel_l2_steps_ws_bytes(2, P, T)
            assert ws > 0 and ws % 8 == 0 and ws >= last, (T, P, ws, last)
            last = ws
        assert lib.uno_rel_l2_steps_ws_bytes(4, 4096, T) == 2 * lib.uno_rel_l2_steps_ws_bytes(2, 4096, T)
    assert lib.uno_rel_l2_steps_ws_bytes(2, 100, 0) == 0 and lib.uno_rel_l2_steps_ws_bytes(2, 100, 257) == 0


def test_binding_refuses_host_tensors_and_unequal_shapes():
    from uno_amd import _native
    with pytest.raises(RuntimeError):
        _native.rel_l2_steps(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
