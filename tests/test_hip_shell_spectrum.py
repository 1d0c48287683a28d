"""K24 (uno_amd/csrc/shell_spectrum.hip) on the MI355X against the float64 definition (tests/spectra_reference.py), its layouts and its
determinism, harness.spectra's dispatch, and the Predictor's spectra=True.

Tolerance.  TOL = 2e-5 is the relative L2 bound the project holds its dense-DFT transforms to (tests/test_hip_dft2d_instances.py).
|U_g - U| <= TOL |U| in L2 gives sum_k |E_g(k) - E(k)| <= sum |U_g - U| (|U_g| + |U|) <= 2 TOL sum_k E(k) to first order, so the l1 bin
error relative to the total energy is held to L1_TOL = 4e-5, per frame and per spectrum (the difference spectrum against ITS total).
Measured on the MI355X (profiles/shell_spectrum_accuracy.txt): at most 1.5e-7.

Per bin, on white noise (every shell holds comparable energy per mode): the kernel's worst relative bin error against float64 is held
to BIN_FACTOR times the same figure of the float32 torch.fft path on the same inputs, computed in the same test.  See
test_per_bin_error_against_the_float32_fft for factor and measurement."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from spectra_reference import spectrum_f64

pytestmark = pytest.mark.gpu
TOL = 2e-5
L1_TOL = 2 * TOL
RTOL_ERRORS = 2e-4          # RTOL_PRINTED of tests/dropin_loops.py: what tests/test_hip_predict.py holds predict's errors to
BIN_FACTOR = 8
GUARD = 64

# (B, T, H, W): every H = W of 8, 9, 21, 32, 64, 85, the non-square grids, T of 1, 3, 10, 20 and B of 1, 3 spread over them (T neither a
# multiple of 4 nor of the 16-wide MFMA tile everywhere; 8 ... 9: one band, 21 ... 32: two, 64: three, 85: three with a last band of 11
# columns), and one frame set each at the table (421: odd, 14 bands) and LDS (512: eight row tiles per wave) limits
CASES = [(1, 1, 8, 8), (3, 3, 9, 9), (1, 10, 21, 21), (3, 20, 32, 32), (1, 3, 64, 64), (3, 10, 64, 64), (1, 20, 85, 85), (3, 1, 8, 9), (1, 3, 21, 16),
         (3, 10, 64, 32), (1, 1, 421, 421), (1, 2, 512, 512)]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(B, T, H, W):
    """white-noise frames x, y (B, T, H, W) on the device and the float64 spectra (B, T, 3, K) of x, y and x - y; computed once"""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + T)
    x, y = torch.randn(B, T, H, W, generator=g), torch.randn(B, T, H, W, generator=g)
    xd, yd = x.double().numpy(), y.double().numpy()
    want = np.stack((spectrum_f64(xd), spectrum_f64(yd), spectrum_f64(xd - yd)), axis=2)
    return x.to(dev()), y.to(dev()), want


def l1(got, want):
    """worst over the leading axes of sum_k |got - want| / sum_k want"""
    got = got.double().cpu().numpy()
    return float((np.abs(got - want).sum(-1) / want.sum(-1)).max())


@pytest.mark.parametrize("B,T,H,W", CASES)
def test_spectra_against_float64(B, T, H, W):
    from uno_amd import _native
    x, y, want = case(B, T, H, W)
    three, one = _native.shell_spectrum(x, y), _native.shell_spectrum(x)
    K = want.shape[-1]
    assert three.shape == (B, T, 3, K) and one.shape == (B, T, 1, K)
    errs = [l1(three[:, :, i], want[:, :, i]) for i in range(3)] + [l1(one[:, :, 0], want[:, :, 0])]
    print(f"[K24 {B} x {T} x {H} x {W}] l1 bin error / total energy: x {errs[0]:.2e}, y {errs[1]:.2e}, x - y {errs[2]:.2e}, x alone {errs[3]:.2e}")
    assert max(errs) <= L1_TOL
    # Parseval and the relative-L2 identity, in the kernel's own numbers
    xs, ys = x.double(), y.double()
    assert torch.allclose(three[:, :, 0].double().sum(-1), (xs * xs).mean(dim=(2, 3)), rtol=L1_TOL)
    rel2 = ((xs - ys) ** 2).sum(dim=(2, 3)) / (ys * ys).sum(dim=(2, 3))
    assert torch.allclose(three[:, :, 2].double().sum(-1) / three[:, :, 1].double().sum(-1), rel2, rtol=2 * L1_TOL)


@pytest.mark.parametrize("B,T,H,W", CASES)
def test_per_bin_error_against_the_float32_fft(B, T, H, W):
    """The worst relative error of any bin, max_k |E_g(k) - E(k)| / E(k), of the kernel against that of harness.spectra's float32
    torch.fft path on the same white-noise frames.  A dense length-S float32 sum accumulates more rounding than an FFT's log2 S
    stages, so the kernel gets BIN_FACTOR = 8 over the FFT path: measured on the MI355X (profiles/shell_spectrum_accuracy.txt) the
    ratio kernel / FFT was at most 3.30 (3 x 3 x 9 x 9: 1.75e-6 against 5.3e-7; 2.92 at 3 x 10 x 64 x 64, 0.16 ... 1.97 at the other
    ten shapes - the worst bin is a shell of few modes that happens to hold little energy, in either form), and 8 is the smallest
    power of two that leaves a factor of 2 over that."""
    from uno_amd import _native
    from uno_amd.harness import spectra
    x, _, want = case(B, T, H, W)
    want = want[:, :, 0]
    kern = _native.shell_spectrum(x)[:, :, 0].double().cpu().numpy()
    fft = spectra._torch_spectra(x).double().cpu().numpy()
    e_kern, e_fft = float((np.abs(kern - want) / want).max()), float((np.abs(fft - want) / want).max())
    print(f"[K24 {B} x {T} x {H} x {W}] worst relative bin error: kernel {e_kern:.3e}, float32 torch.fft {e_fft:.3e}, ratio {e_kern / e_fft:.2f}")
    assert e_kern <= BIN_FACTOR * e_fft


def single_mode(H, W, a, b, amp=1.0):
    r, c = torch.arange(H, dtype=torch.float64).reshape(H, 1), torch.arange(W, dtype=torch.float64).reshape(1, W)
    return (amp * torch.cos(2 * np.pi * (a * r / H + b * c / W))).float()


# (H, W, a, b, shell, energy): a generic mode, the two sides of the rounding boundary, the constant, the Nyquist column and row (energy
# 1, not 1/2: they are their own mirror images), and for odd sizes the corner mode, which lands in the last shell
MODES = [(32, 32, 3, 4, 5, 0.5), (32, 32, 1, 1, 1, 0.5), (32, 32, 2, 2, 3, 0.5), (32, 32, 0, 0, 0, 1.0), (32, 32, 0, 16, 16, 1.0),
         (32, 32, 16, 0, 16, 1.0), (64, 32, 3, 4, 5, 0.5), (64, 32, 0, 16, 16, 1.0), (64, 32, 32, 0, 32, 1.0), (64, 32, 32, 16, 36, 1.0),
         (21, 21, 3, 4, 5, 0.5), (21, 21, 2, 2, 3, 0.5), (21, 21, 10, 10, 14, 0.5), (85, 85, 42, 42, 59, 0.5), (85, 85, 1, 1, 1, 0.5),
         (21, 16, 10, 8, 13, 0.5), (21, 16, 10, 7, 12, 0.5)]


def test_single_modes_land_in_their_shell():
    from uno_amd import _native
    from uno_amd.harness import spectra
    for H, W, a, b, shell, energy in MODES:
        amp = 1.5 if (a, b) == (0, 0) else 1.0
        u = single_mode(H, W, a, b, amp).to(dev()).reshape(1, 1, H, W)
        e = _native.shell_spectrum(u)[0, 0, 0].double().cpu()
        total = energy * amp * amp
        assert e.shape == (spectra.n_shells(H, W),) and shell == round(float(np.hypot(a, b)))
        if H % 2 and W % 2 and (a, b) == (H // 2, W // 2):
            assert shell == e.numel() - 1
        rest = e.clone()
        rest[shell] = 0
        assert abs(float(e[shell]) - total) <= L1_TOL * total and float(rest.abs().sum()) <= L1_TOL * total, (H, W, a, b, e)


def test_layouts_and_views_give_the_bits_of_a_contiguous_copy():
    from uno_amd import _native
    from uno_amd.harness import spectra
    g = torch.Generator().manual_seed(5)
    B, T, H, W = 2, 3, 21, 18
    big_x, big_y = torch.randn(B, 2 * H, 2 * W, T, generator=g).to(dev()), torch.randn(B, T, 2 * H, 2 * W, generator=g).to(dev())
    x, y = big_x[:, ::2, ::2], big_y[:, :, ::2, ::2]                          # (B, H, W, T) and (B, T, H, W) views
    xc, yc = x.permute(0, 3, 1, 2).contiguous(), y.contiguous()              # time-major copies
    want = _native.shell_spectrum(xc, yc)
    assert bits(_native.shell_spectrum(x.permute(0, 3, 1, 2), y), want)       # sub-sampled, and x and y in different layouts
    assert bits(_native.shell_spectrum(xc.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), yc), want)       # (B, S, S, T) dense
    r = spectra.spectral_errors(x, y.permute(0, 2, 3, 1), "bhwt", native=True)
    assert bits(r.pred, want[:, :, 0]) and bits(r.target, want[:, :, 1]) and bits(r.error, want[:, :, 2])
    assert bits(spectra.energy_spectrum(y, "bthw", native=True), want[:, :, 1])
    assert bits(spectra.energy_spectrum(x[..., 1], "bhw", native=True), want[:, 1, 0])
    assert bits(spectra.energy_spectrum(xc[:, 2], "bhw"), want[:, 2, 0])
    assert torch.equal(r.k, torch.arange(want.shape[-1], device=dev()))


def guarded(n, fill):
    """(buffer with GUARD words of NaN before and after n floats of `fill`, the view of the n floats)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev())
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def test_determinism_and_what_the_buffers_held_before():
    """two calls, a sample alone and inside its batch, a call with 16 CUs reserved, NaN-filled spec and ws: the same bits; the guard words
    around spec and ws stay as they were"""
    from uno_amd import _native
    for B, T, H, W in ((3, 3, 64, 64), (3, 10, 21, 16)):
        x, y, _ = case(*((3, 3, 64, 64) if H == 64 else (3, 10, 21, 21)))
        x, y = x[..., :W], y[..., :W]                                         # (a view where W < 21)
        first = _native.shell_spectrum(x, y)
        assert bits(_native.shell_spectrum(x, y), first)
        for b in range(B):
            assert bits(_native.shell_spectrum(x[b:b + 1], y[b:b + 1]), first[b:b + 1])
        before = _native.reserve_cus(16)
        try:
            assert bits(_native.shell_spectrum(x, y), first)
        finally:
            _native.reserve_cus(before)
        K = first.shape[-1]
        n_ws = _native.shell_spectrum_ws_floats(B, T, H, W, True)
        for fill in (float("nan"), 7.0):
            sbuf, spec = guarded(B * T * 3 * K, fill)
            wbuf, ws = guarded(n_ws, fill)
            got = _native.shell_spectrum(x, y, out=spec.view(B, T, 3, K), ws=ws)
            assert bits(got, first)
            for buf in (sbuf, wbuf):
                assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()
            assert not torch.isnan(ws).any()                                  # every word of the workspace the call asks for is written
        one = _native.shell_spectrum(x)
        assert bits(one[:, :, 0], first[:, :, 0])


def test_dispatch_of_energy_spectrum():
    from uno_amd import _native
    from uno_amd.harness import spectra
    x, _, want = case(3, 10, 64, 32)
    assert bits(spectra.energy_spectrum(x, "bthw", native=True), _native.shell_spectrum(x)[:, :, 0])
    assert bits(spectra.energy_spectrum(x, "bthw"), _native.shell_spectrum(x)[:, :, 0])                 # native=None: the kernel
    stock = spectra.energy_spectrum(x, "bthw", native=False)
    assert not bits(stock, _native.shell_spectrum(x)[:, :, 0]) and l1(stock, want[:, :, 0]) <= L1_TOL
    xd = x.double()
    e64 = spectra.energy_spectrum(xd, "bthw")
    assert e64.dtype == torch.float64 and np.allclose(e64.cpu().numpy(), want[:, :, 0], rtol=1e-12, atol=1e-12 * want.max())
    with pytest.raises(RuntimeError, match="takes float32"):
        spectra.energy_spectrum(xd, "bthw", native=True)
    for shape in ((1, 2, 6, 6), (1, 1, 520, 16)):
        small = torch.randn(*shape, generator=torch.Generator().manual_seed(1)).to(dev())
        e = spectra.energy_spectrum(small, "bthw")
        assert l1(e, spectrum_f64(small.double().cpu().numpy())) <= L1_TOL
        with pytest.raises(RuntimeError, match="points per axis"):
            spectra.energy_spectrum(small, "bthw", native=True)
    with pytest.raises(RuntimeError, match="points per axis"):
        _native.shell_spectrum(torch.zeros(1, 1, 6, 6, device=dev()))
    empty = spectra.energy_spectrum(torch.zeros(0, 8, 8, 2, device=dev()))
    assert empty.shape == (0, 2, spectra.n_shells(8, 8))
    L = _native.lib()
    nul = ctypes.c_void_p(0)
    assert L.uno_shell_spectrum(nul, 0, 0, 0, 0, nul, 0, 0, 0, 0, nul, nul, 0, 1, 8, 8, None) == 0


# ------------------------------------------------------------------------------------------------------------------- the Predictor
def check_prediction(r, plain, target_of, layout_frames):
    """spectra=True changed nothing else; the spectra are spectral_errors of the returned frames; their sums give err_step^2"""
    from uno_amd.harness import spectra
    assert bits(r.pred, plain.pred) and bits(r.err_step, plain.err_step) and bits(r.err_full, plain.err_full)
    assert plain.spec_pred is None and plain.spec_true is None and plain.spec_err is None
    T = r.err_step.shape[1]
    want = spectra.spectral_errors(r.pred[..., :T].to(dev()), target_of[..., :T].to(dev()))
    whole = spectra.energy_spectrum(r.pred.to(dev()))
    assert r.spec_pred.shape == (r.pred.shape[0], layout_frames, whole.shape[-1]) and r.spec_true.shape == r.spec_err.shape == want.error.shape
    for got, ref in ((r.spec_pred, whole), (r.spec_true, want.target), (r.spec_err, want.error)):
        ref = ref.double().cpu()
        assert float(((got.double() - ref).abs().sum(-1) / ref.sum(-1)).max()) <= L1_TOL
    ratio = r.spec_err.double().sum(-1) / r.spec_true.double().sum(-1)
    assert torch.allclose(ratio, r.err_step.double() ** 2, rtol=2 * TOL + RTOL_ERRORS, atol=0)


def test_predictor_ns2d_with_spectra_eager_and_from_a_graph():
    """width-8 UNO, T_in = 4, horizon = 6, T = 4, at 56^2 - the smallest grid check_resolution accepts for UNO (its 22 modes need 42
    points on the 3/4-size grid of its first block; 32^2 is refused before any launch); batches of 2, 2 and 1"""
    from uno_amd.harness import Predictor, models, spectra
    torch.manual_seed(11)
    model = models.UNO(8, 8).to(dev()).eval()
    g = torch.Generator().manual_seed(12)
    xx, yy = torch.randn(5, 56, 56, 4, generator=g).to(dev()), torch.randn(5, 56, 56, 4, generator=g).to(dev())
    p = Predictor(model, batch_size=2)
    plain, r = p.ns2d(xx, 6, yy), p.ns2d(xx, 6, yy, spectra=True)
    check_prediction(r, plain, yy.cpu(), 6)
    free = p.ns2d(xx, 6, spectra=True)
    assert bits(free.spec_pred, r.spec_pred) and free.spec_true is None and free.spec_err is None and bits(free.pred, r.pred)
    pg = Predictor(model, batch_size=2, graph=True)
    graphed = pg.ns2d(xx, 6, yy, spectra=True)
    for key in ("pred", "err_step", "err_full", "spec_pred", "spec_true", "spec_err"):
        assert bits(getattr(graphed, key), getattr(r, key)), key
    assert len(pg._replays) == 1
    assert bits(pg.ns2d(xx, 6, yy).pred, r.pred) and len(pg._replays) == 2     # spectra=False is a graph of its own, as before


def test_predictor_ns3d_and_darcy_with_spectra():
    """Uno3D_T10 at 30^2 x 10, the smallest grid check_resolution accepts for it; UNO_9 at 85^2"""
    from uno_amd.harness import Predictor, check_resolution, load_model, models, spectra
    torch.manual_seed(13)
    model = load_model(models.Uno3D_T10(6, 2).state_dict(), model="Uno3D_T10", in_width=6, width=2, device=dev())
    with pytest.raises(ValueError):
        check_resolution(model, 29, 10)
    g = torch.Generator().manual_seed(14)
    x, y = torch.randn(3, 30, 30, 10, 1, generator=g).to(dev()), torch.randn(3, 30, 30, 10, generator=g).to(dev())
    p = Predictor(model, batch_size=2)
    plain, r = p.ns3d(x, y=y), p.ns3d(x, y=y, spectra=True)
    check_prediction(r, plain, y.cpu(), 10)
    graphed = Predictor(model, batch_size=2, graph=True).ns3d(x, y=y, spectra=True)
    for key in ("pred", "err_step", "err_full", "spec_pred", "spec_true", "spec_err"):
        assert bits(getattr(graphed, key), getattr(r, key)), key
    short = p.ns3d(x, y=y[..., :4], spectra=True)                             # 4 measured frames of 10
    assert short.spec_pred.shape == r.spec_pred.shape and short.spec_true.shape == (3, 4, r.spec_pred.shape[-1])
    assert bits(short.spec_true, r.spec_true[:, :4]) and bits(short.spec_err, r.spec_err[:, :4])

    torch.manual_seed(15)
    darcy = models.UNO_9(3, 8, pad=5).to(dev()).eval()
    a, sol = torch.rand(3, 85, 85, 1, generator=g).to(dev()), torch.rand(3, 85, 85, generator=g).to(dev())
    pd = Predictor(darcy, batch_size=2)
    plain, d = pd.darcy(a, sol), pd.darcy(a, sol, spectra=True)
    assert bits(d.pred, plain.pred) and bits(d.err, plain.err) and plain.spec_pred is None
    want = spectra.spectral_errors(d.pred.to(dev()), sol, "bhw")
    for got, ref in ((d.spec_pred, want.pred), (d.spec_true, want.target), (d.spec_err, want.error)):
        ref = ref[:, 0].double().cpu()
        assert got.shape == ref.shape and float(((got.double() - ref).abs().sum(-1) / ref.sum(-1)).max()) <= L1_TOL
    assert torch.allclose(d.spec_err.double().sum(-1) / d.spec_true.double().sum(-1), d.err.double() ** 2, rtol=2 * TOL + RTOL_ERRORS, atol=0)
    assert pd.darcy(a, spectra=True).spec_true is None


def test_command_line_writes_the_spectra(tmp_path, capsys):
    scipy_io = pytest.importorskip("scipy.io")
    from uno_amd.harness import MatReader, models, predict, spectra
    torch.manual_seed(16)
    weights, data, out = str(tmp_path / "uno.pt"), str(tmp_path / "ns.mat"), str(tmp_path / "pred.mat")
    torch.save(models.UNO(8, 8).state_dict(), weights)
    scipy_io.savemat(data, {"u0": torch.randn(2, 56, 56, 10, generator=torch.Generator().manual_seed(17)).numpy()})
    args = ["ns2d", "--weights", weights, "--model", "UNO", "--in-width", "8", "--width", "8", "--data", data, "--split", "all", "--samples", "2",
            "--gen-batch", "2", "--size", "56", "--t-in", "4", "--horizon", "6", "--spectra", "--out", out]
    summary = predict.main(args + ["--no-pred"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    K = spectra.n_shells(56, 56)
    assert line["spectra"] == K and line["frames"] == 6
    reader = MatReader(out)
    assert "pred" not in reader.data
    assert reader.read_field("spec_pred").shape == (2, 6, K) and reader.read_field("spec_true").shape == (2, 6, K)
    assert bits(reader.read_field("spec_err"), summary["result"].spec_err) and reader.read_field("k").reshape(-1).tolist() == list(range(K))
    predict.main(args)
    capsys.readouterr()
    assert MatReader(out).read_field("pred").shape == (2, 56, 56, 6) and "spec_pred" in MatReader(out).data
    predict.main(args[:args.index("--spectra")] + ["--out", out])
    assert "spectra" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1]) and "spec_pred" not in MatReader(out).data
