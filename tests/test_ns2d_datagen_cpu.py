"""The Navier-Stokes data generator without a GPU (uno_amd/harness/datagen.py, dropin/random_fields.py, the uno_ns2d_* entry points): the
torch.fft path against the restatement tests/ns2d_reference.py in float64, the record schedule, the random field against its formula on
the same draw, the .mat file through dropin's MatReader, and the host-side argument checks of the C entry points."""
import ctypes
import math
import os
import sys

import pytest
import torch

from conftest import ROOT
import ns2d_reference as ref


def _inputs(B, N, seed=0, per_sample_f=False):
    g = torch.Generator().manual_seed(seed)
    w0 = torch.randn(B, N, N, generator=g, dtype=torch.float64)
    f = 0.1 * torch.randn(*((B, N, N) if per_sample_f else (N, N)), generator=g, dtype=torch.float64)
    return w0, f


@pytest.mark.parametrize("per_sample_f", [False, True])
def test_stock_path_equals_the_restatement_in_float64(per_sample_f):
    from uno_amd.harness.datagen import navier_stokes_2d
    w0, f = _inputs(2, 32, per_sample_f=per_sample_f)
    T, dt, records = 0.012, 1e-3, 4
    assert math.ceil(T / dt) == 12
    sol, sol_t = navier_stokes_2d(w0, f, 1e-3, T, dt, records)
    want, want_t = ref.solve(w0, f, 1e-3, T, dt, records)
    assert sol.dtype == torch.float64 and tuple(sol.shape) == (2, 32, 32, records)
    for c in range(records):        # same formulas, another order of the element-wise products: a few ulp per step
        err = float((sol[..., c] - want[..., c]).norm() / want[..., c].norm())
        assert err < 1e-13, (c, err)
    assert torch.equal(sol_t, want_t)
    assert float((want[..., -1] - want[..., 0]).norm() / want[..., 0].norm()) > 1e-3       # the records differ: the solver moved


def test_shapes_record_rule_and_times():
    from uno_amd.harness.datagen import navier_stokes_2d
    w0, f = _inputs(1, 32, seed=1)
    # 11 steps, 4 records: record_time = floor(11 / 4) = 2, records after 2, 4, 6, 8 steps; what the last three steps do is not seen
    T, dt = 0.0105, 1e-3
    assert math.ceil(T / dt) == 11
    sol, sol_t = navier_stokes_2d(w0, f, 1e-3, T, dt, record_steps=4)
    assert tuple(sol.shape) == (1, 32, 32, 4) and tuple(sol_t.shape) == (4,) and sol_t.dtype == torch.float32
    assert ref.record_plan(T, dt, 4) == (2, [2, 4, 6, 8])
    t, times = 0.0, []
    for j in range(8):
        t += dt
        if (j + 1) % 2 == 0:
            times.append(t)
    assert torch.equal(sol_t, torch.tensor(times, dtype=torch.float32))
    f_h = torch.fft.fft2(f)
    for c, n_steps in enumerate((2, 4, 6, 8)):
        want = ref.to_real(ref.spectrum_after(w0, f, 1e-3, dt, n_steps), 32)
        assert float((sol[..., c] - want).norm() / want.norm()) < 1e-13
    assert f_h.shape == (32, 32)
    # one record: the state after all floor(steps / 1) steps
    sol1, t1 = navier_stokes_2d(w0, f, 1e-3, T, dt)
    want = ref.to_real(ref.spectrum_after(w0, f, 1e-3, dt, 11), 32)
    assert tuple(sol1.shape) == (1, 32, 32, 1) and float((sol1[..., 0] - want).norm() / want.norm()) < 1e-13
    assert abs(float(t1[0]) - 0.011) < 1e-8
    with pytest.raises(ValueError, match="records"):
        navier_stokes_2d(w0, f, 1e-3, 0.002, dt, record_steps=4)          # 2 steps cannot hold 4 records


def test_float32_and_odd_sizes_take_the_stock_path_on_the_cpu():
    from uno_amd.harness.datagen import native_takes, navier_stokes_2d
    g = torch.Generator().manual_seed(2)
    w0, f = torch.randn(2, 48, 48, generator=g), 0.1 * torch.randn(48, 48, generator=g)
    assert not native_takes(w0, f)
    sol, _ = navier_stokes_2d(w0, f, 1e-3, 0.004, 1e-3, 2)
    want, _ = ref.solve(w0, f, 1e-3, 0.004, 1e-3, 2, dtype=torch.float32)
    assert sol.dtype == torch.float32 and float((sol - want).norm() / want.norm()) < 1e-5
    with pytest.raises(RuntimeError, match="32 ... 256"):
        navier_stokes_2d(w0, f, 1e-3, 0.004, 1e-3, 2, native=True)
    with pytest.raises(RuntimeError, match="float32"):
        navier_stokes_2d(w0.double(), f.double(), 1e-3, 0.004, 1e-3, 2, native=True)


def test_gaussian_rf_equals_its_formula_on_the_same_draw():
    from uno_amd.harness import GaussianRF
    s, alpha, tau = 32, 2.5, 7
    grf = GaussianRF(2, s, alpha=alpha, tau=tau)
    assert grf.sqrt_eig[0, 0] == 0 and tuple(grf.sqrt_eig.shape) == (s, s)
    assert grf.sigma == tau ** (0.5 * (2 * alpha - 2))          # the default: tau^(alpha - dim / 2)
    assert GaussianRF(2, s).sigma == 3 ** (0.5 * (2 * 2 - 2))
    e64 = ref.sqrt_eig(s, alpha, tau)
    assert float((grf.sqrt_eig.double() - e64).abs().max() / e64.abs().max()) < 1e-6
    got = grf.sample(3, generator=torch.Generator().manual_seed(5))
    coeff = torch.randn(3, s, s, 2, generator=torch.Generator().manual_seed(5))
    want = ref.grf_from_draw(coeff.double(), s, alpha, tau)
    assert tuple(got.shape) == (3, s, s) and got.dtype == torch.float32
    assert float((got.double() - want).norm() / want.norm()) < 1e-5
    # a generator given at construction is the default of sample()
    again = GaussianRF(2, s, alpha=alpha, tau=tau, generator=torch.Generator().manual_seed(5)).sample(3)
    assert torch.equal(again, got)
    assert float(got.mean(dim=(1, 2)).abs().max()) < 1e-5       # sqrt_eig[0,0] = 0: every sample has zero mean
    for dim in (1, 3):
        with pytest.raises(NotImplementedError, match="dim = 2"):
            GaussianRF(dim, s)


def test_dropin_module_reexports_the_sampler():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        import random_fields
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    from uno_amd.harness.datagen import GaussianRF
    assert random_fields.GaussianRF is GaussianRF


def test_mat_file_round_trip(tmp_path):
    from uno_amd.harness import generate_ns_dataset
    from uno_amd.harness.datagen import GaussianRF, navier_stokes_2d, ns_forcing
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from utilities3 import MatReader
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    path = str(tmp_path / "ns.mat")
    kw = dict(s=32, record_steps=3, bsize=2, visc=1e-3, T=0.006, delta_t=1e-3, alpha=2.5, tau=7)
    assert generate_ns_dataset(path, n_samples=4, seed=11, device="cpu", **kw) == 2
    reader = MatReader(path)
    gen = torch.Generator().manual_seed(11)
    grf = GaussianRF(2, 32, alpha=2.5, tau=7, generator=gen)
    f = ns_forcing(32)
    t = torch.linspace(0, 1, 33)[:-1]
    assert torch.allclose(f, 0.1 * (torch.sin(2 * math.pi * (t[:, None] + t[None, :])) + torch.cos(2 * math.pi * (t[:, None] + t[None, :]))))
    for j in range(2):
        w0 = grf.sample(2)
        sol, sol_t = navier_stokes_2d(w0, f, 1e-3, 0.006, 1e-3, 3)
        a, u, tt = reader.read_field(f"a{j}"), reader.read_field(f"u{j}"), reader.read_field(f"t{j}")
        assert tuple(a.shape) == (2, 32, 32) and tuple(u.shape) == (2, 32, 32, 3)
        assert torch.equal(a, w0) and torch.equal(u, sol) and torch.equal(tt.reshape(-1), sol_t)
    assert not torch.equal(reader.read_field("a0"), reader.read_field("a1"))


@pytest.fixture(scope="module")
def lib():
    from uno_amd import build, _native
    build.build()
    return _native.lib()


def test_entry_points_are_declared_and_bound(lib):
    from uno_amd import _native
    for name in ("uno_ns2d_ws_bytes", "uno_ns2d_forward", "uno_ns2d_inverse", "uno_ns2d_steps"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.uno_abi_version() == _native.ABI_VERSION


def test_argument_errors_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    for fn, name in ((lib.uno_ns2d_forward, b"uno_ns2d_forward"), (lib.uno_ns2d_inverse, b"uno_ns2d_inverse")):
        assert fn(nul, p, p, 1, 64, None) < 0 and b"null" in lib.uno_last_error() and name in lib.uno_last_error()
        assert fn(p, nul, p, 1, 64, None) < 0 and b"null" in lib.uno_last_error()
        assert fn(p, p, nul, 1, 64, None) < 0 and b"null" in lib.uno_last_error()
        for N in (48, 16, 512, 0, -64):
            assert fn(p, p, p, 1, N, None) < 0 and b"32 ... 256" in lib.uno_last_error(), N
        assert fn(p, p, p, -1, 64, None) < 0 and b"batch" in lib.uno_last_error()
        assert fn(nul, nul, nul, 0, 64, None) == 0          # an empty batch: nothing to do, nothing touched
    steps = lib.uno_ns2d_steps
    assert steps(nul, p, 0, p, 1, 64, 1, 1e-3, 1e-4, None) < 0 and b"null" in lib.uno_last_error()
    assert steps(p, nul, 0, p, 1, 64, 1, 1e-3, 1e-4, None) < 0 and b"null" in lib.uno_last_error()
    assert steps(p, p, 0, nul, 1, 64, 1, 1e-3, 1e-4, None) < 0 and b"null" in lib.uno_last_error()
    for N in (48, 16, 512):
        assert steps(p, p, 0, p, 1, N, 1, 1e-3, 1e-4, None) < 0 and b"32 ... 256" in lib.uno_last_error()
    assert steps(p, p, 0, p, -2, 64, 1, 1e-3, 1e-4, None) < 0 and b"batch" in lib.uno_last_error()
    assert steps(p, p, 0, p, 1, 64, -1, 1e-3, 1e-4, None) < 0 and b"step count" in lib.uno_last_error()
    for dt in (0.0, -1e-4, float("nan"), float("inf")):
        assert steps(p, p, 0, p, 1, 64, 1, 1e-3, dt, None) < 0 and b"delta_t" in lib.uno_last_error(), dt
    for visc in (-1e-3, float("nan")):
        assert steps(p, p, 0, p, 1, 64, 1, visc, 1e-4, None) < 0 and b"visc" in lib.uno_last_error(), visc
    assert steps(nul, nul, 0, nul, 0, 64, 5, 1e-3, 1e-4, None) == 0       # B == 0
    assert steps(nul, nul, 0, nul, 3, 64, 0, 1e-3, 1e-4, None) == 0       # n_steps == 0


def test_workspace_size_is_positive_and_monotone(lib):
    sizes = (32, 64, 128, 256)
    for N in sizes:
        prev = 0
        for B in (1, 2, 3, 20, 21):
            b = lib.uno_ns2d_ws_bytes(B, N)
            assert b == 5 * 8 * B * N * (N // 2 + 1) and b > prev
            prev = b
    for B in (1, 20):
        assert [lib.uno_ns2d_ws_bytes(B, N) for N in sizes] == sorted(lib.uno_ns2d_ws_bytes(B, N) for N in sizes)
        assert lib.uno_ns2d_ws_bytes(B, 32) < lib.uno_ns2d_ws_bytes(B, 64) < lib.uno_ns2d_ws_bytes(B, 128) < lib.uno_ns2d_ws_bytes(B, 256)
    assert lib.uno_ns2d_ws_bytes(1 << 22, 256) == 5 * 8 * (1 << 22) * 256 * 129       # 64-bit
    assert lib.uno_ns2d_ws_bytes(1, 48) == 0 and lib.uno_ns2d_ws_bytes(-1, 64) == 0


def test_bindings_refuse_cpu_tensors_and_name_the_sizes():
    from uno_amd import _native
    with pytest.raises(RuntimeError, match="HIP device"):
        _native.ns2d_forward(torch.zeros(1, 32, 32))
    assert _native.ns2d_supported(64) and not _native.ns2d_supported(48) and not _native.ns2d_supported(512)
