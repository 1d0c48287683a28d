"""OperatorBlock_3D in one buffer on the any-grid kernels: the accumulate / activation forms of K3a (uno_fft_resample3d_any_acc,
uno_amd/csrc/resample3d_any.hip), the opt-in of the block (`one_buffer_any_grid`, enable_one_buffer_any_grid) and
Uno3D_T40(one_buffer_any=True).  pytest -m gpu

The accumulate form is held to BIT equality with (old value) + (the plain call): both are one IEEE float32 addition of the same two
operands, so any difference means the accumulate instantiation changed the transform.  The activation is compared with float64 at the
device-GELU figure of tests/test_hip_pointwise_fused.py (test_device_gelu_and_its_derivative_against_float64: 2.4e-7 max(1, |x|)).
Blocks and the whole model follow tests/test_hip_workload_parity.py: rel_err(P, R64) <= max(5e-5 for a block / 1e-4 for a model,
4 x rel_err(R32, R64)) against the float64 oracle evaluated at run time."""
import pytest
import torch

from conftest import rel_err
from oracle import spectral_oracle as so
from test_hip_redzone import redzone  # noqa: F401  (fixture: guarded device allocations)
from test_hip_resample3d_any import OPERATOR_CASES, SHARED_CASES, T40_GRIDS, _case_tensors
from test_hip_spectral3d import TOL
from test_hip_workload_parity import MODEL_TOL, _block_case, _r, _rel, compare_to_reference, forward_backward

pytestmark = pytest.mark.gpu

GELU_TOL = 2.4e-7        # x max(1, |x|): tests/test_hip_pointwise_fused.py, the device GELU against float64
ACC_NAME, INV_NAME = "uno::resample3d_any_inv_plane_acc_kernel", "uno::resample3d_any_inv_plane_kernel"
CASES = OPERATOR_CASES + [(2, 2, din, dout) for din, dout in T40_GRIDS if (2, 2, din, dout) not in OPERATOR_CASES]
_ids = lambda c: f"{c[0]}x{c[1]}-" + "x".join(map(str, c[2])) + "-" + "x".join(map(str, c[3]))


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _operands(cfg, adjoint, seed=0):
    """-> (x, s, size, plan arguments): the operator din -> dout, or its adjoint dout -> din with the same tables"""
    from uno_amd.spectral3d import _resample3d_plan_any
    B, C, din, dout = cfg
    plan = _resample3d_plan_any(din, dout, dev())
    assert plan is not None
    a, b = _case_tensors(B, C, din, dout)
    x, size = (b, din) if adjoint else (a, dout)
    g = torch.Generator().manual_seed(91 + seed + sum(size))
    s = torch.randn(B, C, *size, generator=g) * 1.5
    t1, t2, m3 = plan
    return x.to(dev()), s.to(dev()), size, ((t1, t1), (t2, t2), m3, 1.0 / (dout[0] * dout[1] * dout[2]))


def _gelu64(t):
    t = t.double()
    return 0.5 * t * (1 + torch.erf(t / 2 ** 0.5))


def _check_gelu(ya, out, tag):
    err = float(((ya.double() - _gelu64(out)).abs() / out.double().abs().clamp(min=1)).max())
    print(f"[{tag}] gelu against float64: {err:.3e} max(1, |x|) (bound {GELU_TOL:.1e})")
    assert err <= GELU_TOL, (tag, err)


# ------------------------------------------------------------------------------------------------ 1. operator, exact
@pytest.mark.parametrize("adjoint", [False, True], ids=["operator", "adjoint"])
@pytest.mark.parametrize("cfg", CASES, ids=_ids)
def test_accumulate_form_is_one_float32_addition_on_top_of_the_plain_call(cfg, adjoint):
    from uno_amd import _native
    x, s, size, args = _operands(cfg, adjoint)
    plain = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint)
    buf = s.clone()
    got = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=buf)
    assert got is buf and got.data_ptr() == buf.data_ptr()
    assert torch.equal(got, s + plain)
    assert torch.equal(_native.fft_resample3d_any(x, size, *args, adjoint=adjoint), plain)        # and the plain form is what it was


# ------------------------------------------------------------------------------------------------ 2. activation
@pytest.mark.parametrize("adjoint", [False, True], ids=["operator", "adjoint"])
@pytest.mark.parametrize("cfg", CASES, ids=_ids)
def test_activation_form(cfg, adjoint):
    from uno_amd import _native
    x, s, size, args = _operands(cfg, adjoint)
    plain = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint)
    buf = s.clone()
    res = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=buf, act=True)
    assert isinstance(res, tuple) and len(res) == 2
    out, ya = res
    assert out is buf and ya.shape == out.shape and ya.dtype == torch.float32 and ya.data_ptr() != out.data_ptr()
    assert torch.equal(out, s + plain)
    _check_gelu(ya, out, f"{cfg[2]} -> {cfg[3]} adjoint={adjoint}")


# ------------------------------------------------------------------------------------------------ 3. agreement with the pruned-DFT kernels
@pytest.mark.parametrize("adjoint", [False, True], ids=["operator", "adjoint"])
@pytest.mark.parametrize("cfg", SHARED_CASES, ids=_ids)
def test_agrees_with_the_pruned_dft_accumulate_form_where_both_apply(cfg, adjoint):
    from uno_amd import _native
    from uno_amd.spectral3d import _resample3d_plan
    B, C, din, dout = cfg
    old_plan = _resample3d_plan(din, dout, dev())
    assert old_plan is not None
    x, s, size, args = _operands(cfg, adjoint)
    o1, o2, om3 = old_plan
    want, want_act = _native.fft_resample3d(x, size, (o1, o1), (o2, o2), om3, args[3], adjoint=adjoint, out=s.clone(), act=True)
    got, got_act = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=s.clone(), act=True)
    e, ea = rel_err(got.cpu().numpy(), want.cpu().numpy()), rel_err(got_act.cpu().numpy(), want_act.cpu().numpy())
    print(f"[shared {din} -> {dout} adjoint={adjoint}] out {e:.2e}, act {ea:.2e} (bound {TOL:.0e})")
    assert e < TOL and ea < TOL


# ------------------------------------------------------------------------------------------------ 4. blocks
def _t40_block(layer, grid, w=8):
    Ci, Co, modes, norm = {"conv7": (8 * w, 2 * w, (14, 14, 10), True), "conv8": (4 * w, 2 * w, (20, 20, 14), False)}[layer]
    din, dout = grid
    return Ci, Co, din, dout, modes, norm


def _graph_nodes(y):
    seen, todo = set(), [y.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        todo += [f for f, _ in n.next_functions]
    return {type(n).__name__ for n in seen}


@pytest.mark.parametrize("case", list(zip(("conv7", "conv8", "conv7", "conv8"), T40_GRIDS)),
                         ids=["conv7-pad3", "conv8-pad3", "conv7-pad2", "conv8-pad2"])
def test_opted_in_t40_blocks_match_the_float64_oracle(case):
    """The four out-of-range blocks of Uno3D_T40(6, 8) (conv7 with its InstanceNorm3d, conv8; pad 3 and pad 2) at batch 2, opted into the
    one-buffer form: output, input gradient and every parameter gradient under the block rule max(5e-5, 4 x floor); the output comes out
    of _OperatorBlock3dFn's node with no stock add / GELU in the graph; conv7's output is bit-equal to the two-branch form's."""
    from uno_amd.integral_operators import OperatorBlock_3D, enable_native_resample3d_any, enable_one_buffer_any_grid
    from uno_amd.spectral3d import _resample3d_plan
    layer, grid = case
    Ci, Co, din, dout, modes, norm = _t40_block(layer, grid)
    assert _resample3d_plan(din, dout, dev()) is None
    torch.manual_seed(700 + len(layer) + Ci + din[2])
    ob = so.OracleOperatorBlock3d(Ci, Co, *dout, *modes, Normalize=norm)
    state = {k: v.clone() for k, v in ob.state_dict().items()}
    blk = enable_one_buffer_any_grid(OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=norm))
    g = torch.Generator().manual_seed(710 + Ci + din[2])
    xs = [torch.randn(2, Ci, *din, generator=g)]
    gy = torch.randn(2, Co, *dout, generator=g)
    ref_run = lambda b, x: b(x[0], *dout)
    seen = {}

    def run(b, x):
        y = b(x[0], *dout)
        seen["y"], seen["head"], seen["nodes"] = y.detach(), type(y.grad_fn).__name__, _graph_nodes(y)
        return y
    _block_case(f"t40 w8 {layer} {din} one-buffer", ob, blk, xs, gy, run, ref_run)
    assert "_OperatorBlock3dFnBackward" in seen["nodes"], seen["nodes"]
    assert not seen["nodes"] & {"AddBackward0", "GeluBackward0", "_FftResample3dAnyFnBackward", "_SpectralConv3dFnBackward"}, seen["nodes"]
    if not norm:
        assert seen["head"] == "_OperatorBlock3dFnBackward"
    else:       # sum -> InstanceNorm: the pre-norm sums are bit-equal (one float32 addition either way), so the outputs are
        two = enable_native_resample3d_any(OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=norm))
        two.load_state_dict(state, strict=True)
        two = two.to(dev())
        assert not getattr(two, "one_buffer_any_grid", False)
        with torch.no_grad():
            y2 = two(xs[0].to(dev()), *dout)
        assert torch.equal(seen["y"], y2)


# ------------------------------------------------------------------------------------------------ 5. launch record
def _record(fn):
    from uno_amd import _native
    _native.profile_begin(100000)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        names = [n for n, _, _ in _native.profile_end()]
    return names


def test_launch_record():
    import uno_amd.integral_operators as io
    from uno_amd.harness import Uno3D_T40, ns3d_loss
    assert io.ONE_BUFFER_3D is True and io.ONE_BUFFER_3D_ANY is False and io.NATIVE_RESAMPLE3D_ANY is False
    Ci, Co, din, dout, modes, norm = _t40_block("conv8", T40_GRIDS[1])
    torch.manual_seed(3)
    x = torch.randn(2, Ci, *din, device=dev())

    def fwd_bwd(blk):
        xd = x.clone().requires_grad_(True)
        blk(xd, *dout).sum().backward()

    opted = io.enable_one_buffer_any_grid(io.OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=norm)).to(dev())
    names = _record(lambda: fwd_bwd(opted))
    assert names.count(ACC_NAME) == 1 and names.count(INV_NAME) == 1, names          # the accumulating forward; the adjoint is plain
    assert sum("resample3d_any" in n for n in names) == 6, names
    plain = io.enable_native_resample3d_any(io.OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=norm)).to(dev())
    names = _record(lambda: fwd_bwd(plain))
    assert names.count(ACC_NAME) == 0 and names.count(INV_NAME) == 2, names
    # cleared again: back to the two branches
    io.enable_one_buffer_any_grid(opted, enabled=False)
    names = _record(lambda: fwd_bwd(opted))
    assert names.count(ACC_NAME) == 0 and names.count(INV_NAME) == 2, names
    # the module switches: both are needed for a block that carries no attribute
    bare = io.OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=norm).to(dev())
    with pytest.raises(RuntimeError, match="outside the range of the"):
        bare(x, *dout)
    io.ONE_BUFFER_3D_ANY = True
    try:
        with pytest.raises(RuntimeError, match="outside the range of the"):        # the block switch alone opts no point-wise layer in
            bare(x, *dout)
        io.NATIVE_RESAMPLE3D_ANY = True
        names = _record(lambda: fwd_bwd(bare))
    finally:
        io.ONE_BUFFER_3D_ANY = io.NATIVE_RESAMPLE3D_ANY = False
    assert names.count(ACC_NAME) == 1 and names.count(INV_NAME) == 1, names

    # nothing changed by default: a default model never launches the accumulate form
    torch.manual_seed(0)
    model = Uno3D_T40(6, 8, pad=3).to(dev())
    g = torch.Generator().manual_seed(5)
    inp = torch.randn(2, 64, 64, 10, 1, generator=g).to(dev()), torch.randn(2, 64, 64, 40, generator=g).to(dev())
    names = _record(lambda: ns3d_loss(model, *inp).backward())
    assert names.count(ACC_NAME) == 0 and names.count(INV_NAME) == 4, names       # conv7 and conv8, forward and adjoint


# ------------------------------------------------------------------------------------------------ 6. whole model
def test_uno3d_t40_one_buffer_any_matches_the_float64_oracle():
    """Uno3D_T40(6, 8, pad=3, one_buffer_any=True) on (2, 64, 64, 10, 1): prediction, ns3d_loss and every parameter gradient against the
    oracle model in float64 with the same weights (procedure and MODEL_TOL rule of
    test_hip_resample3d_any.py::test_uno3d_t40_matches_the_float64_oracle_and_runs_the_any_grid_kernels); the record holds the
    accumulate kernel (conv7 and conv8: twice); one ComplexAdam step moves every parameter."""
    import uno_amd.integral_operators as io
    from uno_amd import _native
    from uno_amd.harness import ComplexAdam, Uno3D_T40
    wl = "c4_t40"
    assert io.STOCK_FFT_RESAMPLE3D is False and io.NATIVE_RESAMPLE3D_ANY is False and io.ONE_BUFFER_3D_ANY is False
    g = torch.Generator().manual_seed(1234)
    inp = (torch.randn(2, 64, 64, 10, 1, generator=g), torch.randn(2, 64, 64, 40, generator=g))
    torch.manual_seed(0)
    m32 = Uno3D_T40(6, 8, pad=3, one_buffer_any=True, block_cls=so.OracleOperatorBlock3d)
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
    prod = Uno3D_T40(6, 8, pad=3, one_buffer_any=True)
    prod.load_state_dict(state, strict=True)
    prod = prod.to(dev())
    dinp = tuple(t.to(dev()) for t in inp)
    _native.profile_begin(100000)
    try:
        pred, loss = forward_backward(wl, prod, dinp)
        torch.cuda.synchronize()
    finally:
        names = [n for n, _, _ in _native.profile_end()]
    bad = compare_to_reference("Uno3D_T40(6, 8, pad=3, one_buffer_any=True)", ref, pred, loss, {k: p.grad for k, p in prod.named_parameters()},
                               tol=MODEL_TOL)
    assert not bad, bad
    assert names.count(ACC_NAME) == 2 and names.count(INV_NAME) == 2, sorted(set(names))
    for k in ("uno::resample3d_any_fwd_plane_kernel", "uno::resample3d_any_axis_kernel"):
        assert names.count(k) == 4, (k, names.count(k))

    opt = ComplexAdam(prod.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.step()
    moved = sum(not torch.equal(p.detach().cpu(), state[k]) for k, p in prod.named_parameters())
    assert moved == len(state)


# ------------------------------------------------------------------------------------------------ 7. properties
PROPERTY_CASES = [(2, 3, (15, 15, 9), (7, 7, 6)), (2, 3, (9, 9, 7), (12, 12, 9)), (1, 2, (32, 32, 31), (48, 48, 41)), (2, 3, (5, 127, 3), (4, 5, 128))]


@pytest.mark.parametrize("cfg", PROPERTY_CASES, ids=_ids)
def test_guard_bands_stay_intact(redzone, cfg):  # noqa: F811
    """y (accumulated into), y_act and the workspace sit between 64 KiB guard bands, operator and adjoint: nothing is written outside"""
    from uno_amd import _native
    for adjoint in (False, True):
        x, s, size, args = _operands(cfg, adjoint)
        buf = torch.empty(s.shape, dtype=torch.float32, device=dev())          # guarded
        buf.copy_(s)
        out, ya = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=buf, act=True)     # + guarded workspace and y_act
        assert torch.isfinite(out).all() and torch.isfinite(ya).all()
        buf2 = torch.empty(s.shape, dtype=torch.float32, device=dev())
        buf2.copy_(s)
        _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=buf2)
        assert torch.equal(buf2, out)
    assert redzone.check(f"fft_resample3d_any(out=, act=) {cfg[2]} -> {cfg[3]}") >= 10       # (y, ws, y_act | y, ws) x 2


@pytest.mark.parametrize("cfg", PROPERTY_CASES[:3], ids=_ids)
def test_reads_stay_inside_x_and_the_accumulated_buffer(cfg):
    """x and the buffer accumulated into are each wrapped in NaN on both sides: finite results, bit-equal to the run on ordinary tensors"""
    from test_hip_redzone import nan_wrapped
    from uno_amd import _native
    for adjoint in (False, True):
        x, s, size, args = _operands(cfg, adjoint)
        a, a_act = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=s.clone(), act=True)
        b, b_act = _native.fft_resample3d_any(nan_wrapped(x), size, *args, adjoint=adjoint, out=nan_wrapped(s), act=True)
        assert torch.isfinite(a).all() and torch.isfinite(a_act).all()
        assert torch.equal(a, b) and torch.equal(a_act, b_act)
        c = _native.fft_resample3d_any(nan_wrapped(x), size, *args, adjoint=adjoint, out=nan_wrapped(s))
        assert torch.equal(a, c)


def test_two_runs_are_bit_identical():
    from uno_amd import _native
    for cfg in ((2, 3, (48, 48, 41), (64, 64, 52)), (2, 3, (15, 15, 9), (7, 7, 6))):
        for adjoint in (False, True):
            x, s, size, args = _operands(cfg, adjoint)
            a, a_act = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=s.clone(), act=True)
            b, b_act = _native.fft_resample3d_any(x, size, *args, adjoint=adjoint, out=s.clone(), act=True)
            assert torch.equal(a, b) and torch.equal(a_act, b_act)


def test_first_seen_any_grid_block_inside_a_capture():
    """a block shape no other test uses first appears inside a hipGraph capture: tables are uploaded without ending it, replay == eager"""
    from test_hip_capture import _capture_then_compare
    from uno_amd.integral_operators import OperatorBlock_3D, enable_one_buffer_any_grid
    from uno_amd.spectral3d import _resample3d_plan
    assert _resample3d_plan((19, 27, 13), (25, 21, 17), dev()) is None
    torch.manual_seed(0)
    blk = enable_one_buffer_any_grid(OperatorBlock_3D(3, 4, 25, 21, 17, 4, 4, 3)).cuda()       # 19 x 27 x 13 -> 25 x 21 x 17
    x = torch.randn(2, 3, 19, 27, 13).cuda()
    _capture_then_compare(blk, x, lambda m, v: m(v, 25, 21, 17))


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_launch_nothing():
    from uno_amd import _native
    from uno_amd.spectral3d import _resample3d_plan_any
    lib = _native.lib()
    din, dout = (9, 9, 7), (12, 12, 9)
    t1, t2, m3 = _resample3d_plan_any(din, dout, dev())
    f = ((t1, t1), (t2, t2), m3, 1.0)
    x = torch.randn(2, 3, *din, device=dev())
    s = torch.randn(2, 3, *dout, device=dev())
    keep = s.clone()
    ws = torch.empty(lib.uno_fft_resample3d_any_ws_bytes(6, 9, 12, 9, 9, m3), dtype=torch.uint8, device=dev())
    sq = torch.randn(2, 3, 9, 9, 9, device=dev())        # a cube: x and y of one shape, so that they can alias
    tq = _resample3d_plan_any((9, 9, 9), (9, 9, 9), dev())
    ptr = lambda t: t.data_ptr()

    def raw(xp, yp, yap, d_in, d_out, tabs):
        a, b, m = tabs
        return lib.uno_fft_resample3d_any_acc(xp, yp, yap, ptr(ws), 6, *d_in, *d_out, a.numel(), ptr(a), ptr(a), b.numel(), ptr(b), ptr(b), m,
                                              1.0, 0, 1, None)

    def refused(call, *words):
        names = _record(lambda: _expect_error(call, words))
        assert names == [], names

    def _expect_error(call, words):
        with pytest.raises(RuntimeError) as info:
            call()
        for w in words:
            assert w in str(info.value), (w, str(info.value))

    def checked(rc):
        _native._check(rc, "uno_fft_resample3d_any_acc")

    refused(lambda: checked(raw(ptr(x), ptr(s), ptr(s), din, dout, (t1, t2, m3))), "uno_fft_resample3d_any_acc", "y_act must not alias y")
    refused(lambda: checked(raw(ptr(sq), ptr(sq), None, (9, 9, 9), (9, 9, 9), tq)), "uno_fft_resample3d_any_acc", "x must not alias y")
    refused(lambda: checked(raw(ptr(sq), ptr(s), ptr(sq), (9, 9, 9), (9, 9, 9), tq)), "x must not alias y_act")
    # an axis of 129
    big = torch.zeros(1, 1, 129, 4, 4, device=dev())
    t4 = _native.table_to_device(torch.arange(4, dtype=torch.int32), dev())
    refused(lambda: _native.fft_resample3d_any(big, (8, 4, 4), (t4, t4), (t4, t4), 2, 1.0, adjoint=False,
                                               out=torch.zeros(1, 1, 8, 4, 4, device=dev())), "uno_fft_resample3d_any_acc", "2 ... 128")
    refused(lambda: _native.fft_resample3d_any(torch.zeros(1, 1, 8, 4, 4, device=dev()), (129, 4, 4), (t4, t4), (t4, t4), 2, 1.0, adjoint=False,
                                               out=torch.zeros(1, 1, 129, 4, 4, device=dev()), act=True), "2 ... 128")
    # `out` of the wrong shape / non-contiguous / wrong dtype: the binding's checks, those of fft_resample3d
    refused(lambda: _native.fft_resample3d_any(x, dout, *f, adjoint=False, out=torch.zeros(2, 3, 12, 12, 8, device=dev())), "out must be a contiguous")
    refused(lambda: _native.fft_resample3d_any(x, dout, *f, adjoint=False, out=torch.zeros(2, 3, 12, 9, 12, device=dev()).transpose(-1, -2)),
            "contiguous")
    refused(lambda: _native.fft_resample3d_any(x, dout, *f, adjoint=False, out=s.double()))
    torch.cuda.synchronize()
    assert torch.equal(s, keep)
