"""K22 on the GPU (uno_amd/csrc/ns2d_solver.hip through _native.ns2d_* and harness.datagen.navier_stokes_2d) against the float64
restatement tests/ns2d_reference.py.  pytest -m gpu

THE tolerance: the native result's error against float64 is at most 8 x the error of the float32 torch.fft restatement against float64
on the same input (the yardstick, computed here on the CPU).  8 = sqrt(256 / log2 256) = 5.7 - a dense 256-term f32 sum against a radix
FFT - rounded up to a power of two.  Snapshots are compared in relative L2.  Where a comparison is per entry, the entry's error is taken
relative to the plane's largest magnitude and bounded by 8 x the yardstick's relative L2 error of that plane: rounding errors and white-
noise values are both near-Gaussian over a plane's thousands of entries, so the largest error stands to the rms error as the largest
value to the rms value, and (max error) / (max value) = (rms error) / (rms value) carries the L2 bound over.

Inputs are white noise unless a case says otherwise: the random field's spectrum decays like k^-2.5 and would hide the Nyquist rule.
Every ratio is printed before it is asserted (pytest -s shows them; DESIGN.md section 8 records them)."""
import functools
import math

import pytest
import torch

import ns2d_reference as ref

pytestmark = pytest.mark.gpu
FACTOR = 8.0
VISC, DT = 1e-3, 1e-3
EPS = 2.0 ** -23


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def half(z):
    return z[..., :z.shape[-1] // 2 + 1]


def per_entry(got, want):
    """largest |got - want| per plane, relative to the plane's largest |want|; complex or real (B, N, M) -> (B,)"""
    return ((got - want).abs().amax(dim=(-2, -1)) / want.abs().amax(dim=(-2, -1)))


def plane_l2(got, want):
    d = (got - want).abs() ** 2
    return (d.sum(dim=(-2, -1)) / (want.abs() ** 2).sum(dim=(-2, -1))).sqrt()


@functools.lru_cache(maxsize=None)
def noise(B, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, N, generator=g), 0.1 * torch.randn(N, N, generator=g), 0.1 * torch.randn(B, N, N, generator=g)


@functools.lru_cache(maxsize=None)
def transforms(B, N):
    """(w, rfft2 f64, rfft2 f32, z with imaginary parts in columns 0 and N/2, irfft2 f64, irfft2 f32)"""
    w = noise(B, N, seed=3)[0]
    g = torch.Generator().manual_seed(4)
    z = torch.complex(torch.randn(B, N, N // 2 + 1, generator=g), torch.randn(B, N, N // 2 + 1, generator=g)) * N
    assert float(z[..., 0].imag.abs().min()) > 0 and float(z[..., N // 2].imag.abs().min()) > 0
    return (w, torch.fft.rfft2(w.double()), torch.fft.rfft2(w), z, torch.fft.irfft2(z.to(torch.complex128), s=(N, N)),
            torch.fft.irfft2(z, s=(N, N)))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [32, 64, 128, 256])
def test_forward_and_inverse_against_rfft2_and_irfft2(N, B):
    from uno_amd import _native
    w, W64, W32, z, x64, x32 = transforms(B, N)
    got = _native.ns2d_forward(w.to(dev())).cpu().to(torch.complex128)
    yard, err, rel = plane_l2(W32.to(torch.complex128), W64), per_entry(got, W64), plane_l2(got, W64)
    print(f"forward N={N} B={B}: per-entry / yardstick {float((err / yard).max()):.2f}, L2 / yardstick {float((rel / yard).max()):.2f}, "
          f"yardstick {float(yard.max()):.2e}")
    assert bool((err <= FACTOR * yard).all()) and bool((rel <= FACTOR * yard).all()), (err / yard, rel / yard)
    got = _native.ns2d_inverse(z.to(dev())).cpu().double()
    yard, err, rel = plane_l2(x32.double(), x64), per_entry(got, x64), plane_l2(got, x64)
    print(f"inverse N={N} B={B}: per-entry / yardstick {float((err / yard).max()):.2f}, L2 / yardstick {float((rel / yard).max()):.2f}, "
          f"yardstick {float(yard.max()):.2e}")
    assert bool((err <= FACTOR * yard).all()) and bool((rel <= FACTOR * yard).all()), (err / yard, rel / yard)
    # the contract ignores the imaginary parts of columns 0 and N/2 after the inverse along axis 0 - and nothing else
    z2 = z.clone()
    z2[..., 1] = z2[..., 1].conj()
    assert l2(torch.fft.irfft2(z2.to(torch.complex128), s=(N, N)), x64) > 1e-2


@pytest.mark.parametrize("N", [32, 64, 128, 256])
def test_one_step_spectrum_per_entry(N):
    from uno_amd import _native
    B = 2
    w0, _, fb = noise(B, N, seed=1)          # a per-sample white-noise forcing: it is visible in every mode, outside the mask too
    want = half(ref.spectrum_after(w0, fb, VISC, DT, 1))
    yard = plane_l2(half(ref.spectrum_after(w0, fb, VISC, DT, 1, dtype=torch.float32)).to(torch.complex128), want)
    w_h = _native.ns2d_forward(w0.to(dev()))
    f_h = _native.ns2d_forward(fb.to(dev()))
    before = w_h.cpu()
    _native.ns2d_steps(w_h, f_h, 1, VISC, DT)
    got = w_h.cpu().to(torch.complex128)
    err, rel = per_entry(got, want), plane_l2(got, want)
    print(f"one step N={N}: per-entry / yardstick {float((err / yard).max()):.2f}, L2 / yardstick {float((rel / yard).max()):.2f}, "
          f"yardstick {float(yard.max()):.2e}")
    assert bool((err <= FACTOR * yard).all()) and bool((rel <= FACTOR * yard).all()), (err / yard, rel / yard)
    # the named entries one by one, each relative to the plane's maximum: DC, the Nyquist row / column / corner, the dealias edge
    km, edge = N // 2, (2 * (N // 2)) // 3
    scale = want.abs().amax(dim=(-2, -1))
    for name, (r, c) in {"dc": (0, 0), "nyquist column": (3, km), "nyquist row": (km, 3), "nyquist corner": (km, km), "inside edge": (edge, edge),
                         "inside edge (negative kx)": (N - edge, edge), "outside edge": (edge + 1, 1), "outside edge column": (1, edge + 1)}.items():
        e = (got[:, r, c] - want[:, r, c]).abs() / scale
        assert bool((e <= FACTOR * yard).all()), (name, e / yard)
    # outside the mask the step is linear: w <- (dt f + (1 - c) w) / (1 + c), c = dt visc lap / 2, on the kernel's own input.  Seven f32
    # roundings (4 pi^2, lap, c, the products, the sum, the quotient), each at most eps / 2 of a term no larger than |w| + dt |f|, and a
    # factor (1 - c) / (1 + c) whose sensitivity to c is below 2: 8 eps
    lap = half(ref.neg_laplacian(N, torch.float64))
    out = half(ref.dealias_mask(N, torch.float64)) == 0
    assert 0.5 < float(out.double().mean()) < 0.6           # (1 - (2/3)^2 of the plane, on the half spectrum too)
    cn = 0.5 * DT * VISC * lap
    fh = f_h.cpu().to(torch.complex128)
    lin = (DT * fh + (1.0 - cn) * before.to(torch.complex128)) / (1.0 + cn)
    bound = 8 * EPS * (before.abs().double() + DT * fh.abs())
    assert bool(((got - lin).abs() <= bound)[:, out].all())
    assert not bool(((got - lin).abs() <= bound)[:, ~out].all())        # ... and inside it the non-linear term is there


CASES = [(32, 3, 64, 4), (64, 2, 64, 4), (256, 2, 8, 4)]


def horizon(steps):
    T = steps * DT
    assert math.ceil(T / DT) == steps
    return T


@functools.lru_cache(maxsize=None)
def solved(N, B, steps, records, forcing):
    """(w0, f, sol f64, per-record yardstick): forcing 'shared' | 'batched' on white noise, 'field' = the generator's own input"""
    w0, fs, fb = noise(B, N, seed=2)
    f = fb if forcing == "batched" else fs
    if forcing == "field":
        coeff = torch.randn(B, N, N, 2, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
        w0 = ref.grf_from_draw(coeff, N, 2.5, 7.0).float()
        t = torch.linspace(0, 1, N + 1)[:-1]
        f = 0.1 * (torch.sin(2 * math.pi * (t[:, None] + t[None, :])) + torch.cos(2 * math.pi * (t[:, None] + t[None, :])))
    T = horizon(steps)
    sol64, t64 = ref.solve(w0, f, VISC, T, DT, records)
    sol32, _ = ref.solve(w0, f, VISC, T, DT, records, dtype=torch.float32)
    return w0, f, sol64, t64, [l2(sol32[..., c], sol64[..., c]) for c in range(records)]


def check_records(tag, sol, sol64, yard):
    ratios = [l2(sol[..., c].cpu(), sol64[..., c]) / yard[c] for c in range(len(yard))]
    print(f"{tag}: native / yardstick per record {[f'{r:.2f}' for r in ratios]}, yardstick {[f'{y:.1e}' for y in yard]}")
    assert all(r <= FACTOR for r in ratios), (tag, ratios)


def native_records(w0, f, steps, records):
    """the records through the three entry points: one ns2d_steps call per recorded interval"""
    from uno_amd import _native
    w_h = _native.ns2d_forward(w0.to(dev()))
    f_h = _native.ns2d_forward((f if f.dim() == 3 else f[None]).to(dev()))
    f_h = f_h if f.dim() == 3 else f_h[0]
    out = []
    for _ in range(records):
        _native.ns2d_steps(w_h, f_h, steps // records, VISC, DT)
        out.append(_native.ns2d_inverse(w_h))
    return torch.stack(out, -1)


@pytest.mark.parametrize("forcing", ["shared", "batched"])
@pytest.mark.parametrize("N,B,steps,records", CASES)
def test_multi_step_records(N, B, steps, records, forcing):
    w0, f, sol64, _, yard = solved(N, B, steps, records, forcing)
    if forcing == "batched":
        assert l2(f[0], f[1]) > 1.0         # the samples' forcings differ
    check_records(f"records N={N} B={B} steps={steps} {forcing}", native_records(w0, f, steps, records), sol64, yard)


def test_multi_step_records_on_a_random_field():
    w0, f, sol64, _, yard = solved(64, 2, 64, 4, "field")
    check_records("records N=64 B=2 steps=64 random field", native_records(w0, f, 64, 4), sol64, yard)


def test_two_runs_and_a_split_run_give_the_same_bits():
    from uno_amd import _native
    w0, fs, _ = noise(2, 64, seed=2)
    start = _native.ns2d_forward(w0.to(dev()))
    f_h = _native.ns2d_forward(fs[None].to(dev()))[0]
    assert torch.equal(start, _native.ns2d_forward(w0.to(dev())))
    a = _native.ns2d_steps(start.clone(), f_h, 8, VISC, DT)
    b = _native.ns2d_steps(start.clone(), f_h, 8, VISC, DT)
    c = _native.ns2d_steps(_native.ns2d_steps(start.clone(), f_h, 5, VISC, DT), f_h, 3, VISC, DT)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)) and torch.equal(torch.view_as_real(a), torch.view_as_real(c))
    assert not torch.equal(torch.view_as_real(a), torch.view_as_real(start))
    assert torch.equal(_native.ns2d_inverse(a), _native.ns2d_inverse(b))


def test_every_sample_of_a_batch_equals_its_own_run():
    from uno_amd import _native
    N, B = 32, 21
    w0, fs, fb = noise(B, N, seed=5)
    w0d, fbd = w0.to(dev()), fb.to(dev())
    f_shared = _native.ns2d_forward(fs[None].to(dev()))[0]
    start, f_batched = _native.ns2d_forward(w0d), _native.ns2d_forward(fbd)
    shared = _native.ns2d_steps(start.clone(), f_shared, 3, VISC, DT)
    batched = _native.ns2d_steps(start.clone(), f_batched, 3, VISC, DT)
    back = _native.ns2d_inverse(batched)
    for s in range(B):
        one = _native.ns2d_forward(w0d[s:s + 1].contiguous())
        assert torch.equal(torch.view_as_real(one[0]), torch.view_as_real(start[s])), s
        f_one = _native.ns2d_forward(fbd[s:s + 1].contiguous())
        assert torch.equal(torch.view_as_real(f_one[0]), torch.view_as_real(f_batched[s])), s
        got = _native.ns2d_steps(one.clone(), f_shared, 3, VISC, DT)
        assert torch.equal(torch.view_as_real(got[0]), torch.view_as_real(shared[s])), s
        got = _native.ns2d_steps(one.clone(), f_one, 3, VISC, DT)
        assert torch.equal(torch.view_as_real(got[0]), torch.view_as_real(batched[s])), s
        assert torch.equal(_native.ns2d_inverse(got)[0], back[s]), s
    assert not torch.equal(torch.view_as_real(shared), torch.view_as_real(batched))


@pytest.mark.parametrize("N,B", [(32, 3), (64, 1), (256, 2)])
def test_guards_stay_and_the_workspace_need_not_be_initialised(N, B):
    from uno_amd import _native
    d, h, G = dev(), N // 2 + 1, 4096
    w0, fs, _ = noise(B, N, seed=7)
    w0d, fsd = w0.to(d), fs[None].to(d)

    def guarded(n_floats):
        raw = torch.full((G + n_floats + G,), -7.25, device=d)
        return raw, raw[G:G + n_floats]

    def intact(raw, n_floats):
        return bool((raw[:G] == -7.25).all()) and bool((raw[G + n_floats:] == -7.25).all())

    n_ws = int(_native.lib().uno_ns2d_ws_bytes(B, N)) // 4
    ws_raw, ws = guarded(n_ws)
    ws.fill_(float("nan"))
    st_raw, st = guarded(2 * B * N * h)
    w_h = torch.view_as_complex(st.view(B, N, h, 2))
    out_raw, out = guarded(B * N * N)
    out = out.view(B, N, N)
    plain_h = _native.ns2d_forward(w0d)
    f_h = _native.ns2d_forward(fsd)[0]
    _native.ns2d_forward(w0d, out=w_h, ws=ws.view(torch.uint8))
    assert torch.equal(torch.view_as_real(w_h), torch.view_as_real(plain_h))
    plain = _native.ns2d_steps(plain_h, f_h, 2, VISC, DT)
    ws.fill_(float("nan"))
    _native.ns2d_steps(w_h, f_h, 2, VISC, DT, ws=ws.view(torch.uint8))
    assert torch.equal(torch.view_as_real(w_h), torch.view_as_real(plain)) and bool(torch.isfinite(torch.view_as_real(w_h)).all())
    ws.fill_(float("nan"))
    _native.ns2d_inverse(w_h, out=out, ws=ws.view(torch.uint8))
    assert torch.equal(out, _native.ns2d_inverse(plain)) and bool(torch.isfinite(out).all())
    assert intact(ws_raw, n_ws) and intact(st_raw, 2 * B * N * h) and intact(out_raw, B * N * N)


def test_public_api_on_the_device():
    from uno_amd import _native
    from uno_amd.harness import navier_stokes_2d
    N, B, steps, records = 64, 2, 64, 4
    for forcing in ("shared", "batched"):
        w0, f, sol64, t64, yard = solved(N, B, steps, records, forcing)
        sol, sol_t = navier_stokes_2d(w0.to(dev()), f.to(dev()), VISC, horizon(steps), DT, records)
        assert tuple(sol.shape) == (B, N, N, records) and sol.is_cuda and sol.dtype == torch.float32
        assert torch.equal(sol_t.cpu(), t64)
        assert torch.equal(sol, native_records(w0, f, steps, records))          # what the multi-step case computes, bit for bit
        check_records(f"navier_stokes_2d N={N} {forcing}", sol, sol64, yard)
        assert torch.equal(sol, navier_stokes_2d(w0.to(dev()), f.to(dev()), VISC, horizon(steps), DT, records, native=True)[0])


def test_public_api_limits_and_fallback():
    from uno_amd.harness import navier_stokes_2d
    g = torch.Generator().manual_seed(8)
    w48, f48 = torch.randn(2, 48, 48, generator=g), 0.1 * torch.randn(48, 48, generator=g)
    w64, f64 = noise(2, 64, seed=2)[:2]
    T = horizon(4)
    with pytest.raises(RuntimeError, match="32 ... 256"):
        navier_stokes_2d(w48.to(dev()), f48.to(dev()), VISC, T, DT, 2, native=True)
    with pytest.raises(RuntimeError, match="float32"):
        navier_stokes_2d(w64.double().to(dev()), f64.double().to(dev()), VISC, T, DT, 2, native=True)
    # native=None falls back to torch.fft on the device and matches the restatement: float32 arithmetic at N = 48 (within 8 x the
    # yardstick, as everywhere), float64 at N = 64 (summation order only)
    want, _ = ref.solve(w48, f48, VISC, T, DT, 2)
    want32, _ = ref.solve(w48, f48, VISC, T, DT, 2, dtype=torch.float32)
    sol, _ = navier_stokes_2d(w48.to(dev()), f48.to(dev()), VISC, T, DT, 2)
    assert sol.dtype == torch.float32 and all(l2(sol[..., c].cpu(), want[..., c]) <= FACTOR * l2(want32[..., c], want[..., c]) for c in range(2))
    want, _ = ref.solve(w64, f64, VISC, T, DT, 2)
    sol, _ = navier_stokes_2d(w64.double().to(dev()), f64.double().to(dev()), VISC, T, DT, 2)
    assert sol.dtype == torch.float64 and l2(sol.cpu(), want) < 1e-12


def test_zero_steps_and_an_empty_batch_launch_nothing():
    from uno_amd import _native
    from uno_amd.harness import navier_stokes_2d
    w0, fs, _ = noise(2, 64, seed=2)
    w_h = _native.ns2d_forward(w0.to(dev()))
    f_h = _native.ns2d_forward(fs[None].to(dev()))[0]
    keep = w_h.clone()
    empty_h = torch.empty((0, 64, 33), dtype=torch.complex64, device=dev())
    empty_w = torch.empty((0, 64, 64), device=dev())
    torch.cuda.synchronize()
    _native.profile_begin(64)
    _native.ns2d_steps(w_h, f_h, 0, VISC, DT)
    _native.ns2d_steps(empty_h, f_h, 5, VISC, DT)
    assert tuple(_native.ns2d_forward(empty_w).shape) == (0, 64, 33) and tuple(_native.ns2d_inverse(empty_h).shape) == (0, 64, 64)
    sol, sol_t = navier_stokes_2d(empty_w, fs.to(dev()), VISC, horizon(4), DT, 2)
    assert _native.profile_end() == []
    assert tuple(sol.shape) == (0, 64, 64, 2) and tuple(sol_t.shape) == (2,)
    assert torch.equal(torch.view_as_real(w_h), torch.view_as_real(keep))
    _native.profile_begin(64)
    _native.ns2d_steps(w_h, f_h, 2, VISC, DT)
    names = [n for n, _, _ in _native.profile_end()]
    assert len(names) == 6 and sum("ns2d_axis1" in n for n in names) == 2, names        # three launches per step
