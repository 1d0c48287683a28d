"""K25 (uno_amd/csrc/sobolev_loss.hip) on the MI355X against the float64 definition (tests/sobolev_reference.py): forward, gradient,
layouts, determinism, harness.losses' dispatch, and a training step of the 2-D and 3-D models with HsLoss.

Tolerances.  TOL = 2e-5 is the relative L2 bound the project holds its dense-DFT transforms to (tests/test_hip_dft2d_instances.py).  On
white noise every mode carries comparable energy, so the derivation of tests/test_hip_shell_spectrum.py carries over with the weights
inside the sums: |X_g - X| <= TOL |X| in the w2-weighted L2 norm gives |num_g - num| <= 2 TOL num to first order, likewise den, and the
ratio sqrt(num / den) is held to the same 2 TOL = 4e-5.  The gradient chains two transforms (TOL each) and the coefficient 1 / sqrt(num den)
(2 TOL): relative L2 per sample <= 4 TOL = 8e-5.

Steep spectra (amplitude ~ (1 + |k|^2)^(-3/2), what the workloads' fields look like): a float32 transform - dense or FFT - spreads its
rounding over all modes while the weights grow as |k|^4, so no bound is fixed in advance; the kernel is held to STEEP_FACTOR times the
error of the float32 torch.fft path on the same inputs, computed in the same test.  See test_steep_spectra_against_the_float32_fft."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import sobolev_reference as ref

pytestmark = pytest.mark.gpu
TOL = 2e-5
FWD_TOL = 2 * TOL
GRAD_TOL = 4 * TOL
STEEP_FACTOR = 8
GUARD = 64

# (B, T, H, W): K24's cases - one, two and three bands, a short last band, odd sizes, T not a multiple of 4, and the table (421) and LDS
# (512) limits
CASES = [(1, 1, 8, 8), (3, 3, 9, 9), (1, 10, 21, 21), (3, 20, 32, 32), (3, 10, 64, 32), (1, 20, 85, 85), (3, 1, 8, 9), (1, 3, 21, 16),
         (1, 1, 421, 421), (1, 2, 512, 512)]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(B, T, H, W):
    """white-noise frames x, y (B, T, H, W) on the device and their float64 copies (of the float32-rounded values); made once"""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + T)
    x, y = torch.randn(B, T, H, W, generator=g), torch.randn(B, T, H, W, generator=g)
    return x.to(dev()), y.to(dev()), x.double().numpy(), y.double().numpy()


def table(H, W, k, a=None):
    from uno_amd.harness import spectra
    return spectra.sobolev_table(H, W, k, a, dev(), torch.float32)


def relmax(got, want):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else got
    return float((np.abs(got - want) / np.abs(want)).max())


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("B,T,H,W", CASES)
def test_forward_against_float64(B, T, H, W, k):
    from uno_amd import _native
    x, y, xd, yd = case(B, T, H, W)
    num, den = ref.sums_f64(xd, yd, k)
    errs = []
    for per_frame in (False, True):
        record, z = _native.sobolev_forward(x, y, table(H, W, k), per_frame)
        assert z is None
        sums, ratio, total = _native.sobolev_views(record, B, T, per_frame)
        want = ref.ratio_f64(xd, yd, k, per_frame=per_frame)
        assert ratio.shape == want.shape
        errs += [relmax(sums[..., 0], num), relmax(sums[..., 1], den), relmax(ratio, want), relmax(total, want.sum())]
    print(f"[K25 {B} x {T} x {H} x {W} k={k}] relative error (num, den, ratio, total) per sample {errs[:4]}, per frame {errs[4:]}")
    assert max(errs) <= FWD_TOL


@pytest.mark.parametrize("B,T,H,W", CASES)
def test_order_zero_is_the_relative_l2_of_k20(B, T, H, W):
    from uno_amd.harness import losses
    x, y, xd, yd = case(B, T, H, W)
    got = losses.sobolev_rel(x, y, "bthw", k=0, native=True)
    k20 = losses.rel_l2(x, y)
    want = np.sqrt(((xd - yd) ** 2).sum(axis=(1, 2, 3)) / (yd ** 2).sum(axis=(1, 2, 3)))
    assert relmax(got, want) <= FWD_TOL and relmax(got, k20.double().cpu().numpy()) <= FWD_TOL


def sample_l2(got, want):
    """worst over the samples of ||got_b - want_b|| / ||want_b||"""
    got = got.double().cpu().numpy()
    B = want.shape[0]
    return float((np.linalg.norm((got - want).reshape(B, -1), axis=1) / np.linalg.norm(want.reshape(B, -1), axis=1)).max())


@pytest.mark.parametrize("B,T,H,W", CASES)
def test_gradient_against_the_closed_form(B, T, H, W):
    from uno_amd.harness import losses
    x, y, xd, yd = case(B, T, H, W)
    errs = []
    for per_frame in (False, True):
        rows = (B, T) if per_frame else (B,)
        g = torch.rand(*rows, generator=torch.Generator().manual_seed(3)) + 0.5
        for gv in (g, torch.ones(rows)):                                      # one value per row; the expanded gradient of .sum()
            xg = x.clone().requires_grad_(True)
            r = losses.sobolev_rel(xg, y, "bthw", k=1, per_frame=per_frame, native=True)
            ((r * gv.to(dev())).sum() if gv is g else r.sum()).backward()
            errs.append(sample_l2(xg.grad, ref.grad_f64(xd, yd, gv.double().numpy(), 1, per_frame=per_frame)))
    print(f"[K25 {B} x {T} x {H} x {W}] gradient, relative L2 per sample: {errs}")
    assert max(errs) <= GRAD_TOL


def test_order_two_coefficients_and_the_loss_object():
    from uno_amd.harness import HsLoss
    B, T, H, W = 3, 1, 21, 16
    x, y, xd, yd = case(1, 3, 21, 16)
    x, y, xd, yd = x[0], y[0], xd[0][:, None], yd[0][:, None]                 # three (H, W) samples: layout "bhw"
    a = (0.5, 0.25)
    want = ref.ratio_f64(xd, yd, 2, a)
    for size_average, scale in ((True, 1.0 / B), (False, 1.0)):
        xg = x.clone().requires_grad_(True)
        loss = HsLoss(k=2, a=a, size_average=size_average, native=True)(xg, y)
        assert loss.dim() == 0 and abs(float(loss.detach()) - want.sum() * scale) <= FWD_TOL * want.sum() * scale
        loss.backward()
        assert sample_l2(xg.grad[:, None], ref.grad_f64(xd, yd, np.full(B, scale), 2, a)) <= GRAD_TOL
    each = HsLoss(k=2, a=a, reduction=False, native=True)(x, y)
    assert each.shape == (B,) and relmax(each, want) <= FWD_TOL


def test_layouts_and_views_give_the_bits_of_a_contiguous_copy():
    from uno_amd.harness import losses
    g = torch.Generator().manual_seed(5)
    B, T, H, W = 2, 3, 21, 18
    big_x, y = torch.randn(B, 2 * H, 2 * W, T, generator=g).to(dev()), torch.randn(B, T, H, W, generator=g).to(dev())
    xc = big_x[:, ::2, ::2].permute(0, 3, 1, 2).contiguous()                  # (B, T, H, W)
    gv = (torch.rand(B, T, generator=g) + 0.5).to(dev())

    def run(x_leaf, view, yv, layout, g_rows=gv):
        x_leaf = x_leaf.clone().requires_grad_(True)
        r = losses.sobolev_rel(view(x_leaf), yv, layout, k=1, per_frame=True, native=True)
        (r * g_rows).sum().backward()
        return r.detach(), x_leaf.grad
    r0, g0 = run(xc, lambda t: t, y, "bthw")
    r1, g1 = run(big_x, lambda t: t[:, ::2, ::2], y.permute(0, 2, 3, 1), "bhwt")           # sub-sampled x, y seen through a permutation
    assert bits(r1, r0) and bits(g1[:, ::2, ::2].permute(0, 3, 1, 2), g0)
    assert float(g1[:, 1::2].abs().max()) == 0.0 and float(g1[:, :, 1::2].abs().max()) == 0.0
    r2, g2 = run(xc.permute(0, 2, 3, 1).contiguous(), lambda t: t, y.permute(0, 2, 3, 1).contiguous(), "bhwt")
    assert bits(r2, r0) and bits(g2.permute(0, 3, 1, 2), g0) and g2.is_contiguous()
    r3, g3 = run(xc[:, 1], lambda t: t, y[:, 1], "bhw", gv[:, 1])
    assert bits(r3, r0[:, 1]) and bits(g3, g0[:, 1])


@pytest.mark.parametrize("B,T,H,W", CASES)
def test_steep_spectra_against_the_float32_fft(B, T, H, W):
    """num and den of frames whose amplitude falls as (1 + |k|^2)^(-3/2), k = 1 and 2: the kernel's relative error against float64 is held
    to STEEP_FACTOR times that of the float32 torch.fft path on the same inputs (floored at the float32 unit round-off, which the FFT
    path reaches at the smallest grids).  Measured on the MI355X (profiles/sobolev_loss_accuracy.txt): the ratio kernel / FFT was at most
    2.64 (1 x 2 x 512 x 512, k = 2: 1.53e-5 against 5.8e-6 - at 512 points a side the |k|^4 weights lift the transform's rounding floor
    of the highest shells to 1e-5 of the sum in either form; 2.60 at 1 x 20 x 85 x 85, k = 1: 5.1e-7 against 2.0e-7; 0.05 ... 1.65 at the
    other eighteen), and 8 is the smallest power of two that leaves a factor of 2 over that - BIN_FACTOR's rule
    (tests/test_hip_shell_spectrum.py)."""
    from uno_amd import _native
    from uno_amd.harness import losses
    xd, yd = ref.steep_frames(B, T, H, W, 7 * H + W), ref.steep_frames(B, T, H, W, 7 * H + W + 1)
    x, y = torch.from_numpy(xd).float(), torch.from_numpy(yd).float()
    xd, yd = x.double().numpy(), y.double().numpy()
    x, y = x.to(dev()), y.to(dev())
    for k in (1, 2):
        num, den = ref.sums_f64(xd, yd, k)
        record, _ = _native.sobolev_forward(x, y, table(H, W, k), True)
        sums = _native.sobolev_views(record, B, T, True)[0]
        wt = losses._half_weights(H, W, k, None, x.device, x.dtype)
        D, Y = torch.fft.rfft2(x - y), torch.fft.rfft2(y)
        s_num, s_den = (wt * (D.real ** 2 + D.imag ** 2)).sum(dim=(-2, -1)), (wt * (Y.real ** 2 + Y.imag ** 2)).sum(dim=(-2, -1))
        e_kern = max(relmax(sums[..., 0], num), relmax(sums[..., 1], den))
        e_fft = max(relmax(s_num, num), relmax(s_den, den), 2.0 ** -24)
        print(f"[K25 steep {B} x {T} x {H} x {W} k={k}] worst relative error of num, den: kernel {e_kern:.3e}, float32 torch.fft {e_fft:.3e}, "
              f"ratio {e_kern / e_fft:.2f}")
        assert e_kern <= STEEP_FACTOR * e_fft


def guarded(n, fill):
    """(buffer with GUARD words of NaN before and after n floats of `fill`, the view of the n floats)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev())
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def raw_call(x, y, w2, gv, per_frame, fill):
    """forward + backward through the C ABI on guarded buffers filled with `fill` -> (sums, ratio, total, z, gx) and the buffers"""
    from uno_amd import _native
    L = _native.lib()
    B, T, H, W = x.shape
    rows = B * T if per_frame else B
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sizes = (2 * B * T, rows, 1, B * T * H * (W // 2 + 1) * 2, _native.sobolev_ws_floats(B, T, H, W), B * T * H * W)
    bufs, (sums, ratio, total, z, ws, gx) = zip(*(guarded(n, fill) for n in sizes))
    assert ws.data_ptr() % 8 == 0 and z.data_ptr() % 8 == 0
    assert L.uno_sobolev_forward(p(x), *x.stride(), p(y), *y.stride(), p(w2), p(sums), p(ratio), p(total), p(z), p(ws), B, T, H, W,
                                 int(per_frame), stream) == 0
    gxv = gx.view(B, T, H, W)
    assert L.uno_sobolev_backward(p(z), p(sums), p(gv), 1, 1.0, int(per_frame), p(gxv), *gxv.stride(), B, T, H, W, stream) == 0
    return (sums, ratio, total, z, gxv), bufs, ws


def test_determinism_and_what_the_buffers_held_before():
    """two calls, a sample alone and inside its batch, a call with 16 CUs reserved, NaN- and 7.0-filled outputs, spectrum and workspace:
    the same bits; the guard words around every buffer stay as they were"""
    from uno_amd import _native
    for (B, T, H, W), per_frame in (((3, 3, 9, 9), False), ((3, 10, 64, 32), True), ((3, 20, 32, 32), False)):
        x, y, _, _ = case(B, T, H, W)
        w2 = table(H, W, 1)
        rows = B * T if per_frame else B
        gv = (torch.rand(rows, generator=torch.Generator().manual_seed(9)) + 0.5).to(dev())
        first, _, _ = raw_call(x, y, w2, gv, per_frame, float("nan"))
        for fill in (float("nan"), 7.0):
            again, bufs, ws = raw_call(x, y, w2, gv, per_frame, fill)
            assert all(bits(a, b) for a, b in zip(again, first))
            for buf in bufs:
                assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()
            assert not any(torch.isnan(t).any() for t in again) and not torch.isnan(ws).any()
        before = _native.reserve_cus(16)
        try:
            reserved, _, _ = raw_call(x, y, w2, gv, per_frame, 7.0)
        finally:
            _native.reserve_cus(before)
        assert all(bits(a, b) for a, b in zip(reserved, first))
        per = T if per_frame else 1
        for b in range(B):
            alone, _, _ = raw_call(x[b:b + 1], y[b:b + 1], w2, gv[b * per:(b + 1) * per].clone(), per_frame, 7.0)
            assert bits(alone[0], first[0][2 * T * b:2 * T * (b + 1)]) and bits(alone[1], first[1][b * per:(b + 1) * per])
            assert bits(alone[3], first[3].view(B, -1)[b]) and bits(alone[4], first[4][b:b + 1])


def test_forward_and_backward_replayed_from_a_graph():
    """captured once on one stream (a shape the process has not seen: the tables are uploaded inside the capture), replayed on new data"""
    from uno_amd.harness import losses
    B, T, H, W = 2, 3, 23, 20
    g = torch.Generator().manual_seed(21)
    data = [(torch.randn(B, H, W, T, generator=g).to(dev()), torch.randn(B, H, W, T, generator=g).to(dev())) for _ in range(2)]
    xs, ys = torch.zeros(B, H, W, T, device=dev(), requires_grad=True), torch.zeros(B, H, W, T, device=dev())
    with torch.no_grad():
        xs.copy_(data[0][0]); ys.copy_(data[0][1])
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            loss = losses.HsLoss(k=2, layout="bhwt", size_average=False, native=True)(xs, ys)
            gx, = torch.autograd.grad(loss, xs)
    torch.cuda.current_stream().wait_stream(s)
    for xv, yv in reversed(data):
        with torch.no_grad():
            xs.copy_(xv); ys.copy_(yv)
        graph.replay()
        torch.cuda.synchronize()
        xe = xv.clone().requires_grad_(True)
        want = losses.HsLoss(k=2, layout="bhwt", size_average=False, native=True)(xe, yv)
        want.backward()
        assert bits(loss.detach(), want.detach()) and bits(gx, xe.grad)


def test_dispatch():
    from uno_amd import _native
    from uno_amd.harness import losses
    B, T, H, W = 3, 10, 64, 32
    x, y, xd, yd = case(B, T, H, W)
    want = ref.ratio_f64(xd, yd, 1)
    record, _ = _native.sobolev_forward(x, y, table(H, W, 1), False)
    kern = _native.sobolev_views(record, B, T, False)[1]
    assert bits(losses.sobolev_rel(x, y, "bthw", native=True), kern)
    if losses.sobolev_native_default(B, T, H, W):
        assert bits(losses.sobolev_rel(x, y, "bthw"), kern)                   # native=None: the kernel
    stock = losses.sobolev_rel(x, y, "bthw", native=False)
    assert not bits(stock, kern) and relmax(stock, want) <= FWD_TOL
    r64 = losses.sobolev_rel(x.double(), y.double(), "bthw")
    assert r64.dtype == torch.float64 and relmax(r64, want) <= 1e-12
    with pytest.raises(RuntimeError, match="takes float32"):
        losses.sobolev_rel(x.double(), y.double(), "bthw", native=True)
    yg = y.clone().requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    losses.sobolev_rel(xg, yg, "bthw").sum().backward()                       # stock ops: autograd reaches the target
    assert yg.grad is not None and float(yg.grad.abs().max()) > 0 and relmax(losses.sobolev_rel(xg, yg, "bthw"), want) <= FWD_TOL
    with pytest.raises(RuntimeError, match="target requires grad"):
        losses.sobolev_rel(xg, yg, "bthw", native=True)
    with pytest.raises(RuntimeError, match="on cpu"):
        losses.sobolev_rel(x.cpu(), y.cpu(), "bthw", native=True)
    for shape in ((1, 2, 6, 6), (1, 1, 520, 16)):
        gen = torch.Generator().manual_seed(1)
        sx, sy = torch.randn(*shape, generator=gen).to(dev()), torch.randn(*shape, generator=gen).to(dev())
        got = losses.sobolev_rel(sx, sy, "bthw")
        assert relmax(got, ref.ratio_f64(sx.double().cpu().numpy(), sy.double().cpu().numpy(), 1)) <= FWD_TOL
        with pytest.raises(RuntimeError, match="points per axis"):
            losses.sobolev_rel(sx, sy, "bthw", native=True)
    with pytest.raises(RuntimeError, match="points per axis"):
        _native.sobolev_forward(torch.zeros(1, 1, 6, 6, device=dev()), torch.zeros(1, 1, 6, 6, device=dev()), torch.ones(4, 4, device=dev()))
    e = torch.zeros(0, 8, 8, 2, device=dev(), requires_grad=True)
    empty = losses.sobolev_rel(e, torch.zeros(0, 8, 8, 2, device=dev()), "bhwt", per_frame=True, native=True)
    assert empty.shape == (0, 2)
    empty.sum().backward()
    assert e.grad.shape == e.shape
    L = _native.lib()
    nul = ctypes.c_void_p(0)
    assert L.uno_sobolev_forward(nul, 0, 0, 0, 0, nul, 0, 0, 0, 0, nul, nul, nul, nul, nul, nul, 0, 1, 8, 8, 0, None) == 0
    assert L.uno_sobolev_backward(nul, nul, nul, 0, 1.0, 0, nul, 0, 0, 0, 0, 0, 1, 8, 8, None) == 0


# ------------------------------------------------------------------------------------------------------------------------ model level
def _assert_grads(native, stock, tol):
    """tests/test_hip_headline_parity.py's bound: ||g - g_ref|| <= tol ||g_ref|| + 1e-6 max ||g_ref|| for every parameter"""
    gmax = max(float(torch.linalg.vector_norm(g)) for g in stock.values())
    for name, gr in stock.items():
        n, err = float(torch.linalg.vector_norm(gr)), float(torch.linalg.vector_norm(native[name] - gr))
        assert err <= tol * n + 1e-6 * gmax, (name, err / max(n, 1e-30))


def _step(model, inp, target, loss_fn):
    for p in model.parameters():
        p.grad = None
    loss = loss_fn(model(inp), target)
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def test_darcy_model_step_native_against_stock_loss():
    from uno_amd.harness import HsLoss, UNO_9
    torch.manual_seed(31)
    model = UNO_9(3, 8, pad=5).to(dev())
    g = torch.Generator().manual_seed(32)
    a, u = torch.rand(3, 85, 85, 1, generator=g).to(dev()), torch.rand(3, 85, 85, generator=g).to(dev())
    run = lambda native: _step(model, a, u, lambda out, t: HsLoss(k=1, size_average=False, native=native)(out.reshape(3, 85, 85), t))
    (l_nat, g_nat), (l_ref, g_ref) = run(True), run(False)
    assert abs(l_nat - l_ref) < 1e-4 * abs(l_ref)
    _assert_grads(g_nat, g_ref, 1e-4)


def test_ns3d_model_step_native_against_stock_loss():
    from uno_amd.harness import HsLoss, load_model, models
    torch.manual_seed(33)
    # (load_model opts the model into the resample family its grids need, as tests/test_hip_shell_spectrum.py builds it)
    model = load_model(models.Uno3D_T10(6, 2).state_dict(), model="Uno3D_T10", in_width=6, width=2, device=dev()).train()
    g = torch.Generator().manual_seed(34)
    x, y = torch.randn(3, 30, 30, 10, 1, generator=g).to(dev()), torch.randn(3, 30, 30, 10, generator=g).to(dev())
    run = lambda native: _step(model, x, y, lambda out, t: HsLoss(k=1, layout="bhwt", size_average=False, native=native)(out.reshape(3, 30, 30, 10), t))
    (l_nat, g_nat), (l_ref, g_ref) = run(True), run(False)
    assert abs(l_nat - l_ref) < 1e-4 * abs(l_ref)
    _assert_grads(g_nat, g_ref, 1e-4)


def test_command_line_trains_darcy_on_h1(tmp_path):
    """two epochs of `fit darcy --loss h1` on a tiny file: the objective is recorded, the figures stay relative L2"""
    scipy_io = pytest.importorskip("scipy.io")
    from uno_amd.harness import fit
    g = torch.Generator().manual_seed(35)
    data, out = str(tmp_path / "darcy.mat"), str(tmp_path / "darcy.pt")
    scipy_io.savemat(data, {"coeff": torch.rand(7, 85, 85, generator=g).numpy(), "sol": torch.rand(7, 85, 85, generator=g).numpy()})
    rec = fit.main(["darcy", "--data", data, "--width", "8", "--pad", "5", "--ntrain", "4", "--nval", "2", "--ntest", "1", "--batch-size", "2",
                    "--epochs", "2", "--seed", "7", "--loss", "h1", "--out", out])
    with open(out + ".json") as f:
        record = json.load(f)
    assert record["loss"] == "h1" and record["test"] == list(rec.test)
    assert len(rec.epochs) == 2 and all(np.isfinite([e.train, e.val]).all() for e in rec.epochs) and 0 < rec.test[0] < 10
