"""The any-grid FFT crop / resample of pointwise_op_3D (uno_fft_resample3d_any: K1a / K5a / K3a, uno_amd/csrc/resample3d_any.hip) and the
model it exists for, the harness Uno3D_T40.  pytest -m gpu

Every comparison is against the reference's op sequence evaluated at run time (float64 on the host); nothing is read from golden
files.  Bounds: the operator and the module are held to 2e-5, the bound of the same quantities on the pruned-DFT kernels
(test_hip_spectral3d.py: TOL) and of the stock-path module test; blocks and the whole model follow tests/test_hip_workload_parity.py:
rel_err(P, R64) <= max(5e-5 for a block / 1e-4 for a model, 4 x rel_err(R32, R64))."""
import pytest
import torch

from conftest import rel_err
from oracle import spectral_oracle as so
from test_hip_redzone import redzone  # noqa: F401  (fixture: guarded device allocations)
from test_hip_spectral3d import RESAMPLE3D, TOL
from test_hip_workload_parity import MODEL_TOL, _block_case, _r, _rel, compare_to_reference, forward_backward

pytestmark = pytest.mark.gpu

T40_GRIDS = [((32, 32, 31), (48, 48, 41)), ((48, 48, 41), (64, 64, 52)), ((32, 32, 28), (48, 48, 38)), ((48, 48, 38), (64, 64, 48))]
OPERATOR_CASES = (
    [(1, 2, din, dout) for din, dout in T40_GRIDS]                                                      # Uno3D_T40 conv7 / conv8, pad 3 and pad 2
    + [(2, 3, (15, 15, 9), (7, 7, 6)), (1, 2, (8, 64, 40), (8, 48, 30)), (2, 3, (9, 9, 7), (12, 12, 9))]  # refused by the pruned-DFT plan
    + [(2, 2, (7, 9, 11), (13, 15, 17))]                                                                # all odd, up-sampling
    + [(1, 1, (128, 128, 64), (96, 96, 64))]                                                            # the largest planes
)
SHARED_CASES = [RESAMPLE3D[1], RESAMPLE3D[4], RESAMPLE3D[7]]       # also in range for the pruned-DFT kernels


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _reference_sequence(x, gy, dout):
    """the reference's rfftn / four corner copies / irfftn(s=size) in float64 on the host -> (y, grad_x)"""
    xr = x.double().requires_grad_(True)
    spec = torch.fft.rfftn(xr, dim=[-3, -2, -1])
    kept = torch.zeros_like(spec)
    h1, h2, h3 = dout[0] // 2, dout[1] // 2, dout[2] // 2
    for rows in (slice(None, h1), slice(-h1, None)):
        for cols in (slice(None, h2), slice(-h2, None)):
            kept[:, :, rows, cols, :h3] = spec[:, :, rows, cols, :h3]
    yr = torch.fft.irfftn(kept, s=dout)
    yr.backward(gy.double())
    return yr.detach(), xr.grad


def _run_any(x, gy, dout):
    from uno_amd.spectral3d import _FftResample3dAnyFn, _resample3d_plan_any
    plan = _resample3d_plan_any(tuple(x.shape[-3:]), dout, dev())
    assert plan is not None
    xd = x.to(dev()).requires_grad_(True)
    y = _FftResample3dAnyFn.apply(xd, dout, plan)
    y.backward(gy.to(dev()))
    return y.detach(), xd.grad


def _case_tensors(B, C, din, dout):
    g = torch.Generator().manual_seed(sum(din) * 7 + sum(dout))
    return torch.randn(B, C, *din, generator=g), torch.randn(B, C, *dout, generator=g)


# ------------------------------------------------------------------------------------------------ 1. operator
@pytest.mark.parametrize("cfg", OPERATOR_CASES, ids=lambda c: "x".join(map(str, c[2])) + "-" + "x".join(map(str, c[3])))
def test_any_grid_resample_matches_the_reference_op_sequence(cfg):
    """Forward and input gradient on grids the pruned-DFT plan refuses (and the sizes where the reference misplaces the negative
    frequencies), against the reference's op sequence in float64."""
    from uno_amd.spectral3d import _resample3d_plan
    B, C, din, dout = cfg
    assert _resample3d_plan(din, dout, dev()) is None
    x, gy = _case_tensors(B, C, din, dout)
    yr, gxr = _reference_sequence(x, gy, dout)
    y, gx = _run_any(x, gy, dout)
    assert y.shape == yr.shape and gx.shape == gxr.shape
    ey, eg = rel_err(y.cpu().numpy(), yr.numpy()), rel_err(gx.cpu().numpy(), gxr.numpy())
    print(f"[any-grid {din} -> {dout}] y {ey:.2e}, grad_x {eg:.2e} (bound {TOL:.0e})")
    assert ey < TOL
    assert eg < TOL


@pytest.mark.parametrize("cfg", SHARED_CASES, ids=lambda c: "x".join(map(str, c[2])) + "-" + "x".join(map(str, c[3])))
def test_any_grid_resample_agrees_with_the_pruned_dft_kernels_where_both_apply(cfg):
    from uno_amd.spectral3d import _FftResample3dFn, _resample3d_plan
    B, C, din, dout = cfg
    x, gy = _case_tensors(B, C, din, dout)
    yr, gxr = _reference_sequence(x, gy, dout)
    y, gx = _run_any(x, gy, dout)
    plan = _resample3d_plan(din, dout, dev())
    assert plan is not None
    xd = x.to(dev()).requires_grad_(True)
    y_old = _FftResample3dFn.apply(xd, dout, plan)
    y_old.backward(gy.to(dev()))
    assert rel_err(y.cpu().numpy(), yr.numpy()) < TOL and rel_err(gx.cpu().numpy(), gxr.numpy()) < TOL
    assert rel_err(y.cpu().numpy(), y_old.detach().cpu().numpy()) < TOL
    assert rel_err(gx.cpu().numpy(), xd.grad.cpu().numpy()) < TOL


# ------------------------------------------------------------------------------------------------ 2. module
@pytest.mark.parametrize("cfg", [((15, 15, 9), (7, 7, 6)), ((9, 9, 7), (12, 12, 9)), ((32, 32, 31), (48, 48, 41))])
def test_pointwise_op_3d_opt_in_matches_the_oracle(cfg):
    """pointwise_op_3D with `native_any_grid` set against the oracle module with the same state_dict: y, grad_x and both parameter
    gradients; a module WITHOUT the attribute still raises while NATIVE_RESAMPLE3D_ANY is False, and runs once the switch is on."""
    import uno_amd.integral_operators as io
    from uno_amd.spectral3d import _resample3d_plan
    din, dout = cfg
    assert _resample3d_plan(din, dout, dev()) is None
    torch.manual_seed(0)
    ref = so.OraclePointwise3d(4, 3, *dout)
    mod = io.pointwise_op_3D(4, 3, *dout)
    mod.load_state_dict(ref.state_dict(), strict=True)
    mod = mod.to(dev())
    mod.native_any_grid = True
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, *din, generator=g)
    gy = torch.randn(2, 3, *dout, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr, *dout)
    yr.backward(gy)
    xd = x.to(dev()).requires_grad_(True)
    y = mod(xd, *dout)
    y.backward(gy.to(dev()))
    errs = {"y": rel_err(y.detach().cpu().numpy(), yr.detach().numpy()), "gx": rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()),
            "gw": rel_err(mod.conv.weight.grad.cpu().numpy(), ref.conv.weight.grad.numpy()),
            "gb": rel_err(mod.conv.bias.grad.cpu().numpy(), ref.conv.bias.grad.numpy())}
    print(f"[pointwise_op_3D {din} -> {dout}] {errs}")
    for k, e in errs.items():
        assert e < 2e-5, (k, e)

    plain = io.pointwise_op_3D(4, 3, *dout)
    plain.load_state_dict(ref.state_dict(), strict=True)
    plain = plain.to(dev())
    assert io.NATIVE_RESAMPLE3D_ANY is False
    with pytest.raises(RuntimeError, match="outside the range of the") as info:
        plain(xd.detach(), *dout)
    assert "STOCK_FFT_RESAMPLE3D" in str(info.value) and "NATIVE_RESAMPLE3D_ANY" in str(info.value)
    io.NATIVE_RESAMPLE3D_ANY = True
    try:
        with torch.no_grad():
            y2 = plain(xd.detach(), *dout)
    finally:
        io.NATIVE_RESAMPLE3D_ANY = False
    assert torch.equal(y2, y.detach())


# ------------------------------------------------------------------------------------------------ 3. blocks
@pytest.mark.parametrize("layer", ["conv7", "conv8"])
def test_t40_blocks_match_the_float64_oracle(layer):
    """OperatorBlock_3D at the geometry of Uno3D_T40(6, 8, pad=3)'s conv7 (InstanceNorm3d) and conv8 on (2, 64, 64, 10): output, input
    gradient and every parameter gradient under the block rule of test_hip_workload_parity.py (max(5e-5, 4 x floor))."""
    from uno_amd.integral_operators import OperatorBlock_3D, enable_native_resample3d_any
    w = 8
    Ci, Co, din, dout, modes, norm = {"conv7": (8 * w, 2 * w, (32, 32, 31), (48, 48, 41), (14, 14, 10), True),
                                      "conv8": (4 * w, 2 * w, (48, 48, 41), (64, 64, 52), (20, 20, 14), False)}[layer]
    torch.manual_seed(700 + len(layer) + Ci)
    ob = so.OracleOperatorBlock3d(Ci, Co, *dout, *modes, Normalize=norm)
    blk = enable_native_resample3d_any(OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=norm))
    g = torch.Generator().manual_seed(710 + Ci)
    xs = [torch.randn(2, Ci, *din, generator=g)]
    gy = torch.randn(2, Co, *dout, generator=g)
    f = lambda b, x: b(x[0], *dout)
    _block_case(f"t40 w{w} {layer}", ob, blk, xs, gy, f, f)


# ------------------------------------------------------------------------------------------------ 4. + 6. whole model, kernel names
def test_uno3d_t40_matches_the_float64_oracle_and_runs_the_any_grid_kernels():
    """Uno3D_T40(6, 8, pad=3) on (2, 64, 64, 10, 1): prediction, ns3d_loss and every parameter gradient against the same model on the
    oracle's blocks in float64 with the same weights (model rule: max(1e-4, 4 x floor)), with STOCK_FFT_RESAMPLE3D off.  The profiled
    kernel names of the pass hold the three any-grid kernels; the point-wise branches of the four out-of-range layers (conv7 / conv8 at
    pad 3 and pad 2), run on their own, launch no plane-batched pruned-DFT kernel."""
    import uno_amd.integral_operators as io
    from uno_amd import _native
    from uno_amd.harness import Uno3D_T40
    wl = "c4_t40"            # (the c4 family of test_hip_workload_parity.py: ns3d_loss, prediction through a forward hook)
    assert io.STOCK_FFT_RESAMPLE3D is False and io.NATIVE_RESAMPLE3D_ANY is False
    g = torch.Generator().manual_seed(1234)
    inp = (torch.randn(2, 64, 64, 10, 1, generator=g), torch.randn(2, 64, 64, 40, generator=g))
    torch.manual_seed(0)
    m32 = Uno3D_T40(6, 8, pad=3, block_cls=so.OracleOperatorBlock3d)
    state = {k: v.clone() for k, v in m32.state_dict().items()}
    m64 = so.to_float64(m32)
    pred32, loss32 = forward_backward(wl, m32, inp)
    pred64, loss64 = forward_backward(wl, m64, tuple(t.double() for t in inp))
    assert pred64.dtype == torch.float64 and tuple(pred64.shape) == (2, 64, 64, 40, 1)
    ref = {"pred": pred64, "loss": float(loss64), "grads": {}, "floor": {}, "norm32": {}}
    ref["floor"]["pred"] = _rel(pred32, pred64)
    ref["floor"]["loss"] = abs(float(loss32) - float(loss64)) / abs(float(loss64))
    p32 = dict(m32.named_parameters())
    norm = lambda t: float(torch.linalg.vector_norm(_r(t)))
    for k, p in m64.named_parameters():
        ref["grads"][k] = p.grad
        ref["floor"][k] = _rel(p32[k].grad, p.grad)
        ref["norm32"][k] = norm(p32[k].grad)
    norms = {k: norm(v) for k, v in ref["grads"].items()}
    ref["gmax"] = max(norms.values())
    ref["zero"] = sorted(k for k, n in norms.items() if n <= 1e-12 * ref["gmax"])
    assert ref["zero"] == ["conv0.w.conv.bias", "conv3.w.conv.bias", "conv7.w.conv.bias"]      # the 1x1x1 bias in front of an InstanceNorm3d

    torch.manual_seed(0)
    prod = Uno3D_T40(6, 8, pad=3)
    prod.load_state_dict(state, strict=True)
    prod = prod.to(dev())
    dinp = tuple(t.to(dev()) for t in inp)
    _native.profile_begin(100000)
    try:
        pred, loss = forward_backward(wl, prod, dinp)
        torch.cuda.synchronize()
    finally:
        names = {n for n, _, _ in _native.profile_end()}
    bad = compare_to_reference("Uno3D_T40(6, 8, pad=3)", ref, pred, loss, {k: p.grad for k, p in prod.named_parameters()}, tol=MODEL_TOL)
    assert not bad, bad
    for k in ("uno::resample3d_any_fwd_plane_kernel", "uno::resample3d_any_axis_kernel", "uno::resample3d_any_inv_plane_kernel"):
        assert k in names, (k, sorted(names))

    # the out-of-range layers' point-wise branches on their own: the any-grid kernels, none of the plane-batched pruned-DFT forms
    for blk, (din, dout) in zip((prod.conv7, prod.conv8, prod.conv7, prod.conv8), T40_GRIDS):
        x = torch.randn(2, blk.conv.in_channels, *din, device=dev(), requires_grad=True)
        _native.profile_begin(1000)
        try:
            blk.w(x, *dout).sum().backward()
            torch.cuda.synchronize()
        finally:
            layer_names = [n for n, _, _ in _native.profile_end()]
        assert sum("resample3d_any" in n for n in layer_names) == 6, layer_names
        assert not any("dft2d_" in n and "plane" in n for n in layer_names), layer_names

    # and the model trains: one optimiser step moves every parameter
    from uno_amd.harness import ComplexAdam
    opt = ComplexAdam(prod.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.step()
    moved = sum(not torch.equal(p.detach().cpu(), state[k]) for k, p in prod.named_parameters())
    assert moved == len(state)


# ------------------------------------------------------------------------------------------------ 5. properties
@pytest.mark.parametrize("cfg", [((15, 15, 9), (7, 7, 6)), ((9, 11, 7), (12, 14, 10)), ((32, 32, 31), (48, 48, 41))])
def test_adjoint_identity(cfg):
    """<A x, g> == <x, A^T g> to 1e-4 relative"""
    din, dout = cfg
    x, gy = _case_tensors(2, 2, din, dout)
    y, gx = _run_any(x, gy, dout)
    lhs = float((y.double().cpu() * gy.double()).sum())
    rhs = float((x.double() * gx.double().cpu()).sum())
    scale = float(torch.linalg.vector_norm(y.double())) * float(torch.linalg.vector_norm(gy.double()))
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), 1e-3 * scale), (lhs, rhs)


def test_two_runs_are_bit_identical():
    for din, dout in (((48, 48, 41), (64, 64, 52)), ((15, 15, 9), (7, 7, 6))):
        x, gy = _case_tensors(2, 3, din, dout)
        y1, g1 = _run_any(x, gy, dout)
        y2, g2 = _run_any(x, gy, dout)
        assert torch.equal(y1, y2) and torch.equal(g1, g2)


@pytest.mark.parametrize("cfg", [((15, 15, 9), (7, 7, 6)), ((9, 9, 7), (12, 12, 9)), ((32, 32, 31), (48, 48, 41)), ((5, 127, 3), (4, 5, 128))])
def test_guard_bands_stay_intact(redzone, cfg):  # noqa: F811
    """output, workspace and input gradient are allocated with 64 KiB guard bands on both sides: nothing is written outside them"""
    din, dout = cfg
    x, gy = _case_tensors(2, 3, din, dout)
    _run_any(x, gy, dout)
    assert redzone.check(f"fft_resample3d_any {din} -> {dout}") >= 4        # y + workspace, forward and adjoint


def test_reads_stay_inside_the_input():
    """the input wrapped in NaN on both sides: the result does not change"""
    from test_hip_redzone import nan_wrapped
    from uno_amd.spectral3d import _FftResample3dAnyFn, _resample3d_plan_any
    for din, dout in (((15, 15, 9), (7, 7, 6)), ((9, 9, 7), (12, 12, 9))):
        x, _ = _case_tensors(2, 3, din, dout)
        plan = _resample3d_plan_any(din, dout, dev())
        with torch.no_grad():
            a = _FftResample3dAnyFn.apply(x.to(dev()), dout, plan)
            b = _FftResample3dAnyFn.apply(nan_wrapped(x.to(dev())), dout, plan)
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_first_seen_any_grid_inside_a_capture():
    """a grid no other test uses first appears inside a hipGraph capture: tables are uploaded without ending it, replay == eager"""
    from test_hip_capture import _capture_then_compare
    from uno_amd.integral_operators import enable_native_resample3d_any, pointwise_op_3D
    torch.manual_seed(0)
    layer = enable_native_resample3d_any(pointwise_op_3D(3, 4, 23, 19, 21)).cuda()       # 17 x 29 x 15 -> 23 x 19 x 21
    x = torch.randn(2, 3, 17, 29, 15).cuda()
    _capture_then_compare(layer, x, lambda m, v: m(v, 23, 19, 21))
