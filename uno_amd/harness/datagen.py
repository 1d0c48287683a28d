"""The reference's Navier-Stokes data generator (Data Generation/Navier Stocks/ns_datagen.py and random_fields-2.py) as importable
functions on current PyTorch.  The reference's two files call torch.rfft / torch.irfft / torch.ifft, which no PyTorch since 1.8 has, and
do all their work at import; here the same algorithm is a module:

    GaussianRF(2, s, alpha, tau).sample(B)              the random initial vorticity (random_fields-2.py:8-99)
    navier_stokes_2d(w0, f, visc, T, delta_t, records)   the pseudo-spectral solver (ns_datagen.py:15-140)
    generate_ns_dataset(path, ...)                       the driver loop and its .mat file (ns_datagen.py:143-223)
    python -m uno_amd.harness.datagen --out FILE [--samples 1200 --size 256 --T 50 ...]

The solver's time loop is the hot path: on a HIP device, float32, with N a power of two in 32 ... 256 it runs on the K22 kernels
(_native.ns2d_steps: three launches per time step from one C loop, no step loop in Python).  Every other input - CPU tensors, float64,
other sizes - takes the torch.fft path below, which states the same algorithm with the documented meaning of the removed calls:
rfft(x, 2, onesided=False) is fft2 of a real field, and irfft(z, 2, onesided=False, signal_sizes=(N, N)) is irfft2 of the first N/2 + 1
columns of z.  The sampler is not a hot path and uses torch.fft everywhere."""
from __future__ import annotations

import argparse
import io
import math

import torch

from .. import _native

__all__ = ["GaussianRF", "navier_stokes_2d", "generate_ns_dataset", "ns_forcing", "native_takes"]

# Where measurement says the native path loses to the torch.fft path at a size, `native=None` takes the stock path there (DESIGN.md
# section 8, "NS-2D data generator"); native=True still runs K22.
NATIVE_DEFAULT_SIZES = _native.NS2D_SIZES


def _wavenumbers(n: int, device, dtype=None):
    k_max = n // 2
    k = torch.cat((torch.arange(0, k_max, device=device), torch.arange(-k_max, 0, device=device)), 0)
    return k if dtype is None else k.to(dtype)


class GaussianRF(object):
    """random_fields-2.py:8-99, dim = 2: samples of a periodic Gaussian random field with covariance sigma^2 (-Laplacian + tau^2)^(-alpha)."""

    def __init__(self, dim, size, alpha=2, tau=3, sigma=None, boundary="periodic", device=None, generator=None):
        if dim != 2:
            raise NotImplementedError(f"GaussianRF: dim={dim}: only the 2-D field the Navier-Stokes generator uses is implemented (dim = 2)")
        self.dim, self.device, self.generator = dim, device, generator
        if sigma is None:
            sigma = tau ** (0.5 * (2 * alpha - self.dim))
        self.sigma = sigma
        k_y = _wavenumbers(size, device).repeat(size, 1)
        k_x = k_y.transpose(0, 1)
        self.sqrt_eig = (size ** 2) * math.sqrt(2.0) * sigma * ((4 * (math.pi ** 2) * (k_x ** 2 + k_y ** 2) + tau ** 2) ** (-alpha / 2.0))
        self.sqrt_eig[0, 0] = 0.0
        self.size = (size,) * dim

    def sample(self, N, generator=None):
        """(N, size, size): Re ifft2(sqrt_eig (a + i b)), (a, b) = randn(N, size, size, 2)"""
        gen = generator if generator is not None else self.generator
        coeff = torch.randn(N, *self.size, 2, device=self.device, generator=gen)
        return torch.fft.ifft2(torch.complex(self.sqrt_eig * coeff[..., 0], self.sqrt_eig * coeff[..., 1])).real


def native_takes(w0, f) -> bool:
    """True when K22 runs this input: HIP tensors, float32, (B, N, N) with N a power of two in 32 ... 256"""
    return (w0.is_cuda and f.is_cuda and w0.dtype == torch.float32 and f.dtype == torch.float32 and w0.dim() == 3
            and w0.shape[-1] == w0.shape[-2] and _native.ns2d_supported(int(w0.shape[-1])))


def _schedule(T, delta_t, record_steps):
    """(steps between records, [t of record 0, 1, ...]) by ns_datagen.py:23, 36, 121-134.  Where steps is no multiple of record_steps
    the reference would hit (j + 1) % record_time == 0 more than record_steps times and fail on sol[..., record_steps]; the first
    record_steps hits are kept and the steps after the last of them, which no output depends on, are not run."""
    steps = math.ceil(T / delta_t)
    if record_steps < 1 or steps < record_steps:
        raise ValueError(f"navier_stokes_2d: {steps} steps cannot hold {record_steps} records")
    record_time = math.floor(steps / record_steps)
    t, times = 0.0, []
    for j in range(record_time * record_steps):
        t += delta_t
        if (j + 1) % record_time == 0:
            times.append(t)
    return record_time, times


def _stock_steps(w_h, f_h, n_steps, visc, delta_t, tables):
    """n_steps of ns_datagen.py:67-118 on the full spectrum w_h (B, N, N) with torch.fft"""
    k_x, k_y, lap, dealias = tables
    N = w_h.shape[-1]
    h = N // 2 + 1
    two_pi_i = 2j * math.pi

    def inv(z):
        return torch.fft.irfft2(z[..., :h], s=(N, N))

    for _ in range(n_steps):
        psi_h = w_h / lap
        q = inv(two_pi_i * k_y * psi_h)
        v = inv(-two_pi_i * k_x * psi_h)
        w_x = inv(two_pi_i * k_x * w_h)
        w_y = inv(two_pi_i * k_y * w_h)
        F_h = torch.fft.fft2(q * w_x + v * w_y) * dealias
        w_h = (-delta_t * F_h + delta_t * f_h + (1.0 - 0.5 * delta_t * visc * lap) * w_h) / (1.0 + 0.5 * delta_t * visc * lap)
    return w_h


def navier_stokes_2d(w0, f, visc, T, delta_t=1e-4, record_steps=1, native=None):
    """ns_datagen.py:15-140 -> (sol (B, N, N, record_steps), sol_t (record_steps,)).  w0: (B, N, N) initial vorticity; f: (N, N) forcing
    shared by the batch or (B, N, N).  native: None - K22 where it applies (native_takes and N in NATIVE_DEFAULT_SIZES), torch.fft
    otherwise; True - K22 or an error that names its limits; False - torch.fft."""
    N = int(w0.shape[-1])
    if native is None:
        native = native_takes(w0, f) and N in NATIVE_DEFAULT_SIZES
    elif native and not native_takes(w0, f):
        raise RuntimeError("navier_stokes_2d(native=True): the native solver takes float32 tensors on a HIP device, w0 of shape (B, N, N) "
                           f"with N a power of two in 32 ... 256 (got {w0.dtype} {tuple(w0.shape)} on {w0.device})")
    record_time, times = _schedule(T, delta_t, record_steps)
    sol = torch.zeros(*w0.shape, record_steps, device=w0.device, dtype=w0.dtype)
    sol_t = torch.tensor(times, device=w0.device, dtype=torch.float32)
    if native:
        B = int(w0.shape[0])
        if B == 0:
            return sol, sol_t
        if f.dim() == 3 and int(f.shape[0]) != B:
            raise RuntimeError(f"navier_stokes_2d: a per-sample forcing needs {B} samples (got {tuple(f.shape)})")
        ws = _native.ns2d_workspace(B, N, w0.device)
        w_h = _native.ns2d_forward(w0.contiguous(), ws=ws)
        f_h = _native.ns2d_forward(f.contiguous() if f.dim() == 3 else f.contiguous()[None], ws=ws)
        f_h = f_h if f.dim() == 3 else f_h[0]
        w = torch.empty((B, N, N), dtype=torch.float32, device=w0.device)
        for c in range(record_steps):
            _native.ns2d_steps(w_h, f_h, record_time, visc, delta_t, ws=ws)
            _native.ns2d_inverse(w_h, out=w, ws=ws)
            sol[..., c].copy_(w)
        return sol, sol_t
    w_h, f_h = torch.fft.fft2(w0), torch.fft.fft2(f)
    k_y = _wavenumbers(N, w0.device, w0.dtype).repeat(N, 1)
    k_x = k_y.transpose(0, 1)
    lap = 4 * (math.pi ** 2) * (k_x ** 2 + k_y ** 2)
    lap[0, 0] = 1.0
    k_max = math.floor(N / 2.0)
    dealias = torch.logical_and(torch.abs(k_y) <= (2.0 / 3.0) * k_max, torch.abs(k_x) <= (2.0 / 3.0) * k_max).to(w0.dtype)
    for c in range(record_steps):
        w_h = _stock_steps(w_h, f_h, record_time, visc, delta_t, (k_x, k_y, lap, dealias))
        sol[..., c] = torch.fft.irfft2(w_h[..., :N // 2 + 1], s=(N, N))
    return sol, sol_t


def ns_forcing(s, device=None):
    """0.1 (sin(2 pi (x + y)) + cos(2 pi (x + y))) on the s x s periodic grid (ns_datagen.py:164-169)"""
    t = torch.linspace(0, 1, s + 1, device=device)[0:-1]
    X, Y = torch.meshgrid(t, t, indexing="ij")
    return 0.1 * (torch.sin(2 * math.pi * (X + Y)) + torch.cos(2 * math.pi * (X + Y)))


def generate_ns_dataset(path, n_samples=1200, s=256, record_steps=50, bsize=20, visc=1e-3, T=50.0, delta_t=1e-4, alpha=2.5, tau=7, seed=None,
                        device=None, native=None, verbose=False):
    """The driver of ns_datagen.py:143-223: n_samples // bsize batches of GaussianRF(2, s, alpha, tau) initial conditions solved to T
    under the forcing of ns_forcing, written batch by batch to ONE MATLAB v5 file as fields a{j} (bsize, s, s), u{j} (bsize, s, s,
    record_steps) and t{j} (record_steps) - the file dropin/utilities3.MatReader.read_field reads.  (The reference appends whole
    savemat outputs, header included, which leaves a file only its first batch can be read from; here the later batches are appended as
    data elements of the same file.)  Returns the number of batches written."""
    import scipy.io

    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    gen = None
    if seed is not None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
    grf = GaussianRF(2, s, alpha=alpha, tau=tau, device=device, generator=gen)
    f = ns_forcing(s, device)
    n_batches = n_samples // bsize
    for j in range(n_batches):
        w0 = grf.sample(bsize)
        sol, sol_t = navier_stokes_2d(w0, f, visc, T, delta_t, record_steps, native=native)
        fields = {f"a{j}": w0.cpu().numpy(), f"u{j}": sol.cpu().numpy(), f"t{j}": sol_t.cpu().numpy()}
        if j == 0:
            scipy.io.savemat(path, mdict=fields, do_compression=True)
        else:       # a v5 file is a 128-byte header followed by data elements: append this batch's elements without a second header
            buf = io.BytesIO()
            scipy.io.savemat(buf, mdict=fields, do_compression=True)
            with open(path, "ab") as fh:
                fh.write(buf.getvalue()[128:])
        if verbose:
            print(f"batch {j + 1} / {n_batches}: {(j + 1) * bsize} samples", flush=True)
    return n_batches


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m uno_amd.harness.datagen", description="Generate a 2-D Navier-Stokes dataset (.mat)")
    ap.add_argument("--out", required=True, help="the .mat file to write")
    ap.add_argument("--samples", type=int, default=1200)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--records", type=int, default=50)
    ap.add_argument("--bsize", type=int, default=20)
    ap.add_argument("--visc", type=float, default=1e-3)
    ap.add_argument("--T", type=float, default=50.0)
    ap.add_argument("--delta-t", type=float, default=1e-4)
    ap.add_argument("--alpha", type=float, default=2.5)
    ap.add_argument("--tau", type=float, default=7.0)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    n = generate_ns_dataset(a.out, a.samples, a.size, a.records, a.bsize, a.visc, a.T, a.delta_t, a.alpha, a.tau, a.seed, a.device, verbose=True)
    print(f"wrote {n} batches to {a.out}")


if __name__ == "__main__":
    main()
