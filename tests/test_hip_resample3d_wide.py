"""The wide-axis FFT crop / resample of pointwise_op_3D (uno_fft_resample3d_wide / _acc: K1w / K5w / K3w, uno_amd/csrc/resample3d_wide.hip):
the grids of Uno3D_T20_256 / Uno3D_T10_256 at S = 256 and the edges of the kernels' range.  pytest -m gpu

Every comparison is against the reference's op sequence evaluated at run time (float64 on the host).  Bounds: the operator, the module
and the spectral branch are held to TOL = 2e-5 of test_hip_spectral3d.py (the reference's own float32 evaluation of these grids is at
1.6e-7 ... 2.7e-7 of float64); the accumulate form to bit equality with (old y) + (the plain call), its activation to the device-GELU
figure of test_hip_block3d_any.py; blocks to the rule of test_hip_resample3d_any.py, max(5e-5, 4 x rel_err(R32, R64))."""
import pytest
import torch

from conftest import rel_err
from oracle import spectral_oracle as so
from test_hip_block3d_any import _check_gelu, _graph_nodes
from test_hip_redzone import redzone  # noqa: F401  (fixture: guarded device allocations)
from test_hip_resample3d_any import _case_tensors, _reference_sequence, _run_any
from test_hip_spectral3d import TOL
from test_hip_uninit import _three_runs
from test_hip_workload_parity import _block_case

pytestmark = pytest.mark.gpu

MODEL_GRIDS = [(1, 2, (256, 256, 12), (64, 64, 12)), (1, 2, (64, 64, 24), (256, 256, 24)), (1, 2, (64, 64, 10), (256, 256, 10)),
               (1, 1, (256, 256, 16), (64, 64, 16)), (1, 1, (64, 64, 32), (256, 256, 32))]
OPERATOR_CASES = MODEL_GRIDS + [
    (2, 3, (256, 8, 6), (64, 8, 6)), (2, 3, (8, 256, 6), (8, 64, 6)), (2, 3, (64, 8, 6), (256, 8, 8)), (2, 3, (8, 64, 6), (8, 256, 8)),      # one long axis at a time
    (2, 2, (129, 5, 7), (255, 7, 9)),           # odd lengths
    (1, 2, (200, 130, 5), (50, 33, 4)),         # odd kept-row counts
    (1, 2, (6, 255, 64), (5, 131, 63)),         # the longest last axis
    (2, 3, (9, 9, 7), (12, 12, 9)),             # the smallest tiles, below every MFMA tile size
]
SHARED_WITH_ANY = [(1, 2, (32, 32, 31), (48, 48, 41)), (2, 3, (15, 15, 9), (7, 7, 6))]
ACC_CASES = [OPERATOR_CASES[0], OPERATOR_CASES[2], OPERATOR_CASES[9], OPERATOR_CASES[10], OPERATOR_CASES[12]]
_ids = lambda c: f"{c[0]}x{c[1]}-" + "x".join(map(str, c[2])) + "-" + "x".join(map(str, c[3]))
_REFERENCE = {}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _reference(cfg):
    """(x, gy, y64, grad_x64) of a case: computed once, shared, never written to"""
    if cfg not in _REFERENCE:
        B, C, din, dout = cfg
        x, gy = _case_tensors(B, C, din, dout)
        _REFERENCE[cfg] = (x, gy, *_reference_sequence(x, gy, dout))
    return _REFERENCE[cfg]


def _run_wide(x, gy, dout):
    from uno_amd.spectral3d import _FftResample3dWideFn, _resample3d_plan_wide
    plan = _resample3d_plan_wide(tuple(x.shape[-3:]), dout, dev())
    assert plan is not None
    xd = x.to(dev()).requires_grad_(True)
    y = _FftResample3dWideFn.apply(xd, dout, plan)
    y.backward(gy.to(dev()))
    return y.detach(), xd.grad


# ------------------------------------------------------------------------------------------------ 1. operator
@pytest.mark.parametrize("cfg", OPERATOR_CASES, ids=_ids)
def test_wide_resample_matches_the_reference_op_sequence(cfg):
    """forward and input gradient against the reference's op sequence in float64"""
    B, C, din, dout = cfg
    x, gy, yr, gxr = _reference(cfg)
    y, gx = _run_wide(x, gy, dout)
    assert y.shape == yr.shape and gx.shape == gxr.shape
    ey, eg = rel_err(y.cpu().numpy(), yr.numpy()), rel_err(gx.cpu().numpy(), gxr.numpy())
    print(f"[wide {din} -> {dout}] y {ey:.2e}, grad_x {eg:.2e} (bound {TOL:.0e})")
    assert ey < TOL
    assert eg < TOL


@pytest.mark.parametrize("cfg", SHARED_WITH_ANY, ids=_ids)
def test_wide_resample_agrees_with_the_any_grid_kernels_where_both_apply(cfg):
    B, C, din, dout = cfg
    x, gy, yr, gxr = _reference(cfg)
    y, gx = _run_wide(x, gy, dout)
    ya, gxa = _run_any(x, gy, dout)
    assert rel_err(y.cpu().numpy(), yr.numpy()) < TOL and rel_err(gx.cpu().numpy(), gxr.numpy()) < TOL
    assert rel_err(ya.cpu().numpy(), yr.numpy()) < TOL and rel_err(gxa.cpu().numpy(), gxr.numpy()) < TOL
    assert rel_err(y.cpu().numpy(), ya.cpu().numpy()) < TOL and rel_err(gx.cpu().numpy(), gxa.cpu().numpy()) < TOL


# ------------------------------------------------------------------------------------------------ 2. accumulate / activation forms
def _operands(cfg, adjoint):
    """-> (x, s, size, plan arguments): the operator din -> dout, or its adjoint dout -> din with the same tables"""
    from uno_amd.spectral3d import _resample3d_plan_wide
    B, C, din, dout = cfg
    t1, t2, m3 = _resample3d_plan_wide(din, dout, dev())
    a, b = _case_tensors(B, C, din, dout)
    x, size = (b, din) if adjoint else (a, dout)
    s = torch.randn(B, C, *size, generator=torch.Generator().manual_seed(91 + sum(size))) * 1.5
    return x.to(dev()), s.to(dev()), size, ((t1, t1), (t2, t2), m3, 1.0 / (dout[0] * dout[1] * dout[2]))


@pytest.mark.parametrize("adjoint", [False, True], ids=["operator", "adjoint"])
@pytest.mark.parametrize("cfg", ACC_CASES, ids=_ids)
def test_accumulate_and_activation_forms(redzone, cfg, adjoint):  # noqa: F811
    """y ends as (old y) + (the plain call's result) - one float32 addition of the same operands, so bit for bit - y_act = gelu(y), and
    nothing outside y / y_act / the workspace is written (64 KiB guard bands around every allocation of the calls)"""
    from uno_amd import _native
    x, s, size, args = _operands(cfg, adjoint)
    plain = _native.fft_resample3d_wide(x, size, *args, adjoint=adjoint)
    buf = s.clone()
    got = _native.fft_resample3d_wide(x, size, *args, adjoint=adjoint, out=buf)
    assert got is buf and torch.equal(got, s + plain)
    buf2 = s.clone()
    out, ya = _native.fft_resample3d_wide(x, size, *args, adjoint=adjoint, out=buf2, act=True)
    assert out is buf2 and ya.shape == out.shape and ya.data_ptr() != out.data_ptr()
    assert torch.equal(out, s + plain)
    _check_gelu(ya, out, f"wide {cfg[2]} -> {cfg[3]} adjoint={adjoint}")
    assert redzone.check(f"fft_resample3d_wide {cfg[2]} -> {cfg[3]}") >= 5          # y + workspace, workspace, workspace + y_act


# ------------------------------------------------------------------------------------------------ 3. properties
def test_two_runs_are_bit_identical():
    for cfg in (OPERATOR_CASES[1], OPERATOR_CASES[9], OPERATOR_CASES[10]):
        x, gy = _case_tensors(*cfg)
        y1, g1 = _run_wide(x, gy, cfg[3])
        y2, g2 = _run_wide(x, gy, cfg[3])
        assert torch.equal(y1, y2) and torch.equal(g1, g2)


def test_results_do_not_depend_on_what_empty_memory_held(monkeypatch):
    """output, workspace and y_act come from torch.empty: poisoned with 0xFF / 0x7F the results are finite and bit-equal"""
    from uno_amd import _native
    cfgs = (OPERATOR_CASES[5], OPERATOR_CASES[9], OPERATOR_CASES[12])

    def workload():
        res = []
        for cfg in cfgs:
            x, gy = _case_tensors(*cfg)
            res += list(_run_wide(x, gy, cfg[3]))
            xd, s, size, args = _operands(cfg, False)
            res += list(_native.fft_resample3d_wide(xd, size, *args, adjoint=False, out=s, act=True))
        return res
    _three_runs(monkeypatch, workload, 6 * len(cfgs), "fft_resample3d_wide")       # per case: y + workspace, grad_x + workspace, workspace + y_act


def test_reads_stay_inside_the_input():
    """the input wrapped in NaN on both sides: the result does not change"""
    from test_hip_redzone import nan_wrapped
    from uno_amd.spectral3d import _FftResample3dWideFn, _resample3d_plan_wide
    for cfg in (OPERATOR_CASES[5], OPERATOR_CASES[9], OPERATOR_CASES[12]):
        _, _, din, dout = cfg
        x, _ = _case_tensors(*cfg)
        plan = _resample3d_plan_wide(din, dout, dev())
        with torch.no_grad():
            a = _FftResample3dWideFn.apply(x.to(dev()), dout, plan)
            b = _FftResample3dWideFn.apply(nan_wrapped(x.to(dev())), dout, plan)
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 4. module
# (256,16,12) <-> (64,4,12) have planes of at most 192 elements and 64 kept rows: the pruned-DFT kernels take them (no limit on the
# leading axis there), and a grid an older family takes keeps it - so the opted-in module is checked on them as it is, and on
# (256,160,12) <-> (64,40,12), planes of 1920 elements, which only the wide-axis kernels take
@pytest.mark.parametrize("cfg", [((256, 16, 12), (64, 4, 12)), ((64, 4, 12), (256, 16, 12)), ((256, 160, 12), (64, 40, 12)), ((64, 40, 12), (256, 160, 12))],
                         ids=lambda c: "x".join(map(str, c)))
def test_pointwise_op_3d_opt_in_matches_the_oracle(cfg):
    """pointwise_op_3D with `native_wide_grid` set against the oracle module with the same state_dict: y, grad_x and both parameter
    gradients; on a grid only the wide-axis kernels take, a module WITHOUT the attribute still raises, naming the new switch"""
    import uno_amd.integral_operators as io
    from uno_amd import _native
    from uno_amd.spectral3d import _resample3d_pruned_applies
    din, dout = cfg
    family = "pruned" if _resample3d_pruned_applies(din, dout) else "wide"
    assert family == ("wide" if 160 in din + dout else "pruned")
    torch.manual_seed(0)
    ref = so.OraclePointwise3d(4, 3, *dout)
    mod = io.pointwise_op_3D(4, 3, *dout)
    mod.load_state_dict(ref.state_dict(), strict=True)
    mod = mod.to(dev())
    mod.native_wide_grid = True
    assert io._resample3d_kernels(mod, din, dout, dev())[1] == family
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, *din, generator=g)
    gy = torch.randn(2, 3, *dout, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr, *dout)
    yr.backward(gy)
    xd = x.to(dev()).requires_grad_(True)
    _native.profile_begin(1000)
    try:
        y = mod(xd, *dout)
        y.backward(gy.to(dev()))
        torch.cuda.synchronize()
    finally:
        names = [n for n, _, _ in _native.profile_end()]
    assert sum("resample3d_wide" in n for n in names) == (6 if family == "wide" else 0), names
    errs = {"y": rel_err(y.detach().cpu().numpy(), yr.detach().numpy()), "gx": rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()),
            "gw": rel_err(mod.conv.weight.grad.cpu().numpy(), ref.conv.weight.grad.numpy()),
            "gb": rel_err(mod.conv.bias.grad.cpu().numpy(), ref.conv.bias.grad.numpy())}
    print(f"[pointwise_op_3D {din} -> {dout}] {errs}")
    for k, e in errs.items():
        assert e < TOL, (k, e)

    if family != "wide":
        return
    plain = io.pointwise_op_3D(4, 3, *dout)
    plain.load_state_dict(ref.state_dict(), strict=True)
    plain = plain.to(dev())
    assert io.NATIVE_RESAMPLE3D_WIDE is False and io.NATIVE_RESAMPLE3D_ANY is False and io.STOCK_FFT_RESAMPLE3D is False
    with pytest.raises(RuntimeError, match="outside the range of the") as info:
        plain(xd.detach(), *dout)
    assert "NATIVE_RESAMPLE3D_WIDE" in str(info.value) and "NATIVE_RESAMPLE3D_ANY" in str(info.value)
    plain.native_any_grid = True            # the older opt-in alone does not reach a 256 axis
    with pytest.raises(RuntimeError, match="outside the range of the"):
        plain(xd.detach(), *dout)


# ------------------------------------------------------------------------------------------------ 5. block
# ((64,16,12) -> (256,64,12) is inside the pruned-DFT range as well - see above; (64,38,12) -> (256,152,12), planes of 1824 elements, is not)
@pytest.mark.parametrize("grids", [(2, (64, 16, 12), (256, 64, 12)), (1, (64, 38, 12), (256, 152, 12))], ids=["256x64", "256x152"])
@pytest.mark.parametrize("norm", [False, True], ids=["gelu", "instnorm"])
def test_one_buffer_block_matches_the_float64_oracle(norm, grids):
    """OperatorBlock_3D(4, 8) in one buffer with the wide opt-in: output, input gradient and every parameter gradient under the block
    rule max(5e-5, 4 x floor); the graph holds the one-buffer node and no stock add / GELU; on the second grid the accumulate form of
    the wide-axis kernels ran"""
    from uno_amd import _native
    from uno_amd.integral_operators import OperatorBlock_3D, enable_native_resample3d_wide
    from uno_amd.spectral3d import _resample3d_pruned_applies
    B, din, dout = grids
    modes = (8, 8, 5)
    torch.manual_seed(800 + norm)
    ob = so.OracleOperatorBlock3d(4, 8, *dout, *modes, Normalize=norm)
    blk = OperatorBlock_3D(4, 8, *dout, *modes, Normalize=norm)
    blk.one_buffer_any_grid = True
    enable_native_resample3d_wide(blk)
    assert not hasattr(blk.w, "native_any_grid")
    g = torch.Generator().manual_seed(810)
    xs = [torch.randn(B, 4, *din, generator=g)]
    gy = torch.randn(B, 8, *dout, generator=g)
    seen = {}

    def run(b, x):
        y = b(x[0], *dout)
        seen["nodes"] = _graph_nodes(y)
        return y
    _block_case(f"wide block norm={norm}", ob, blk, xs, gy, run, lambda b, x: b(x[0], *dout))
    assert "_OperatorBlock3dFnBackward" in seen["nodes"], seen["nodes"]
    assert not seen["nodes"] & {"AddBackward0", "GeluBackward0", "_FftResample3dWideFnBackward", "_SpectralConv3dFnBackward"}, seen["nodes"]
    wide = not _resample3d_pruned_applies(din, dout)
    assert wide == (dout[1] == 152)
    _native.profile_begin(1000)         # the launch records of one forward pass of THIS block (moved to the device by _block_case)
    try:
        with torch.no_grad():
            blk(xs[0].to(dev()), *dout)
        torch.cuda.synchronize()
    finally:
        kernels = [n for n, _, _ in _native.profile_end()]
    assert ("uno::resample3d_wide_inv_plane_acc_kernel" in kernels) == wide, kernels
    assert any("resample3d_wide" in n for n in kernels) == wide, kernels


# ------------------------------------------------------------------------------------------------ 6. the spectral branch at these grids
@pytest.mark.parametrize("cfg", [((256, 256, 12), (64, 64, 12), (32, 32, 5)), ((64, 64, 24), (256, 256, 24), (32, 32, 8))],
                         ids=["conv0", "conv8"])
def test_spectral_conv3d_at_the_256_grids(cfg):
    """SpectralConv3d_Uno alone at conv0's and conv8's grids (the plane-by-plane 2-D kernels plus uno_cdft_axis: accepted before, never
    run at 256 rows): forward and all gradients against the oracle layer in float64"""
    from uno_amd.integral_operators import SpectralConv3d_Uno
    din, dout, modes = cfg
    torch.manual_seed(5)
    ref = so.OracleSpectralConv3d(2, 2, *dout, *modes)
    mod = SpectralConv3d_Uno(2, 2, *dout, *modes)
    mod.load_state_dict(ref.state_dict(), strict=True)
    mod = mod.to(dev())
    ref = so.to_float64(ref)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 2, *din, generator=g)
    gy = torch.randn(1, 2, *dout, generator=g)
    xr = x.double().requires_grad_(True)
    yr = ref(xr, *dout)
    yr.backward(gy.double())
    yr = yr.detach()
    xd = x.to(dev()).requires_grad_(True)
    y = mod(xd, *dout)
    y.backward(gy.to(dev()))
    errs = {"y": rel_err(y.detach().cpu().numpy(), yr.numpy()), "gx": rel_err(xd.grad.cpu().numpy(), xr.grad.numpy())}
    for k, p in mod.named_parameters():
        errs[k] = rel_err(torch.view_as_real(p.grad).cpu().numpy(), torch.view_as_real(dict(ref.named_parameters())[k].grad).numpy())
    print(f"[SpectralConv3d_Uno {din} -> {dout}] {errs}")
    for k, e in errs.items():
        assert e < TOL, (k, e)
