"""The reference's Darcy-flow data generator (the MATLAB files Data Generation/darcy Flow/GRF.m, demo.m and solve_gwf.m) as importable
functions:

    darcy_grf(alpha, tau, s, n)              the Gaussian random field with Neumann covariance (GRF.m:7-23)
    threshold(u, hi, lo)                     the piecewise-constant coefficient (demo.m:25-27); exp(u) is the lognormal one (demo.m:22)
    solve_gwf(coef, F)                       -div(coef grad p) = F on the unit square, p = 0 on the border (solve_gwf.m:4-37)
    generate_darcy_dataset(path, ...)        samples of (coefficient, solution) in the .mat file the Darcy loaders read
    python -m uno_amd.harness.darcy_datagen --out FILE [--samples 1024 --size 421 --lo 3 ...]

What solve_gwf computes.  The coefficient and the right-hand side live on the s cell centres (2 i - 1) / (2 s) a side; the equation is
discretised on the K = s nodes i / (K - 1).  Both are moved to the nodes by a separable not-a-knot cubic spline (the nodes 0 and K - 1 lie
half a cell outside the centres: the end polynomials extrapolate), a 5-point system with the face coefficients (c_i + c_j) / 2 is solved
on the (K - 2)^2 interior nodes, and the nodal solution with its zero border is splined back to the centres.  Both grids are uniform, so
each transfer is one fixed K x K matrix applied from both sides, S V S^T.  The spline of a thresholded coefficient overshoots: nodal and
face coefficients below zero are ordinary inputs here and nothing about their sign is assumed or checked.

Where MATLAB solves the system directly, this module iterates: conjugate gradients in float64, preconditioned by the 5-point Laplacian
with unit coefficient applied as a fast Poisson solve (DST-I from both sides, a divide by the eigenvalue sums, DST-I again), with the
flexible beta = z_new^T (r_new - r_old) / (z_old^T r_old), to a relative residual rtol.  On a HIP device with s in 8 ... 512 the work
runs on the K23 kernels (_native.darcy_transform / darcy_solve: the preconditioner in float32 on the MFMA, everything else float64, the
iteration loop in C).  Every other input - CPU tensors, other sizes, native=False - takes the stock path below: the same algorithm in
plain float64 torch operations."""
from __future__ import annotations

import argparse
import functools
import math

import torch

from .. import _native

__all__ = ["darcy_grf", "threshold", "spline_matrix", "dct_matrix", "solve_gwf", "generate_darcy_dataset", "native_takes"]

# Where measurement says the native path loses to the stock path at a size, `native=None` takes the stock path there (DESIGN.md section
# 8, "Darcy data generator"); native=True still runs K23.
NATIVE_DEFAULT_SIZES = range(_native.DARCY_SIZES[0], _native.DARCY_SIZES[1] + 1)


def native_takes(t) -> bool:
    """True when K23 runs this input: a HIP tensor (B, s, s) with s in 8 ... 512"""
    return t.is_cuda and t.dim() == 3 and t.shape[-1] == t.shape[-2] and _native.darcy_supported(int(t.shape[-1]))


# ------------------------------------------------------------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=8)
def dct_matrix(s: int) -> torch.Tensor:
    """D (s, s) float64 with idct2(L) = D L D^T: the orthonormal inverse DCT-II, D[x, k] = w_k cos(pi (2 x + 1) k / (2 s)), w_0 =
    sqrt(1 / s), w_k = sqrt(2 / s)"""
    # (the phase is reduced in integers: (2 x + 1) k mod 4 s)
    phase = torch.remainder((2 * torch.arange(s)[:, None] + 1) * torch.arange(s)[None, :], 4 * s).to(torch.float64)
    D = torch.cos(math.pi * phase / (2 * s)) * math.sqrt(2.0 / s)
    D[:, 0] = math.sqrt(1.0 / s)
    return D


def spline_matrix(x_from, x_to) -> torch.Tensor:
    """S (len(x_to), len(x_from)) float64 with S y = the not-a-knot cubic spline through (x_from, y) evaluated at x_to; points outside
    x_from are extrapolated by the end polynomial (interp2(..., 'spline'), solve_gwf.m:11-12 and 35, along one axis).  Built on the host
    from the spline's second derivatives m: the continuity equations of the interior knots, third-derivative continuity at the second
    and the last-but-one knot, solved for all unit vectors y at once."""
    xf = torch.as_tensor(x_from, dtype=torch.float64).cpu()
    xt = torch.as_tensor(x_to, dtype=torch.float64).cpu()
    m = xf.numel()
    if m < 4:
        raise ValueError("spline_matrix: a not-a-knot spline needs at least 4 points")
    h = xf[1:] - xf[:-1]
    T = torch.zeros(m, m, dtype=torch.float64)
    R = torch.zeros(m, m, dtype=torch.float64)
    for i in range(1, m - 1):
        T[i, i - 1], T[i, i], T[i, i + 1] = h[i - 1], 2 * (h[i - 1] + h[i]), h[i]
        R[i, i - 1], R[i, i], R[i, i + 1] = 6 / h[i - 1], -6 / h[i - 1] - 6 / h[i], 6 / h[i]
    T[0, 0], T[0, 1], T[0, 2] = h[1], -(h[0] + h[1]), h[0]
    T[m - 1, m - 3], T[m - 1, m - 2], T[m - 1, m - 1] = h[m - 2], -(h[m - 3] + h[m - 2]), h[m - 3]
    M2 = torch.linalg.solve(T, R)                      # second derivatives at the knots per unit vector y
    i = torch.clamp(torch.searchsorted(xf, xt, right=True) - 1, 0, m - 2)
    hi = h[i]
    a, b = xf[i + 1] - xt, xt - xf[i]                   # (negative outside: the end cubic goes on)
    S = (a ** 3 / (6 * hi) - hi * a / 6)[:, None] * M2[i] + (b ** 3 / (6 * hi) - hi * b / 6)[:, None] * M2[i + 1]
    rows = torch.arange(xt.numel())
    S[rows, i] += a / hi
    S[rows, i + 1] += b / hi
    return S


@functools.lru_cache(maxsize=8)
def _grid_tables(K: int):
    """(centres -> nodes, nodes -> centres, DST-I, 1 / (lambda_i + lambda_j)) of the K-grid, float64 on the host"""
    centres = (2 * torch.arange(1, K + 1, dtype=torch.float64) - 1) / (2 * K)
    nodes = torch.arange(K, dtype=torch.float64) / (K - 1)
    n = K - 2
    idx = torch.arange(1, n + 1)
    phase = torch.remainder(idx[:, None] * idx[None, :], 2 * (n + 1)).to(torch.float64)
    dst = math.sqrt(2.0 / (n + 1)) * torch.sin(math.pi * phase / (n + 1))
    lam = (K - 1) ** 2 * 4.0 * torch.sin(math.pi * idx.to(torch.float64) / (2 * (n + 1))) ** 2
    return spline_matrix(centres, nodes), spline_matrix(nodes, centres), dst, 1.0 / (lam[:, None] + lam[None, :])


_DEVICE_TABLES = {}


def _device_table(kind: str, K: int, device):
    """the padded float64 table `kind` (cn | nc | dct) of size K as K23-T reads it, cached per device"""
    key = (kind, K, str(device))
    if key not in _DEVICE_TABLES:
        M = dct_matrix(K) if kind == "dct" else _grid_tables(K)[0 if kind == "cn" else 1]
        _DEVICE_TABLES[key] = _native.darcy_table(M, device)
    return _DEVICE_TABLES[key]


def _two_sided(kind: str, v, native: bool):
    """M v M^T for the table `kind` of v's size, float64"""
    K = int(v.shape[-1])
    if native:
        return _native.darcy_transform(_device_table(kind, K, v.device), v.contiguous())
    M = (dct_matrix(K) if kind == "dct" else _grid_tables(K)[0 if kind == "cn" else 1]).to(v.device)
    return M @ v @ M.T


# ------------------------------------------------------------------------------------------------------------------------ the field
def darcy_grf(alpha, tau, s, n=1, device=None, generator=None, xi=None, native=None):
    """GRF.m:7-23 -> (n, s, s) float64: idct2(s coef xi) with coef = tau^(alpha - 1) (pi^2 (k1^2 + k2^2) + tau^2)^(-alpha / 2) on k = 0 ...
    s - 1, the (0, 0) entry zeroed (the field's mean is 0), xi = randn(n, s, s) unless given.  MATLAB's random stream is not reproduced."""
    if xi is None:
        device = torch.device("cpu" if device is None else device)
        xi = torch.randn(n, s, s, dtype=torch.float64, device=device, generator=generator)
    else:
        xi = xi.to(torch.float64)
        if xi.dim() == 2:
            xi = xi[None]
        if tuple(xi.shape[-2:]) != (s, s):
            raise ValueError(f"darcy_grf: xi must be (n, {s}, {s}) (got {tuple(xi.shape)})")
    k = torch.arange(s, dtype=torch.float64, device=xi.device)
    coef = tau ** (alpha - 1.0) * (math.pi ** 2 * (k[:, None] ** 2 + k[None, :] ** 2) + tau ** 2) ** (-alpha / 2.0)
    L = s * coef * xi
    L[:, 0, 0] = 0.0
    if native is None:
        native = native_takes(L) and s in NATIVE_DEFAULT_SIZES
    elif native and not native_takes(L):
        raise RuntimeError(f"darcy_grf(native=True): the native transform takes HIP tensors with s in 8 ... 512 (got s={s} on {L.device})")
    return _two_sided("dct", L, native)


def threshold(u, hi=12.0, lo=4.0):
    """demo.m:25-27: hi where u >= 0, lo elsewhere, in u's dtype"""
    return torch.where(u >= 0, torch.full_like(u, hi), torch.full_like(u, lo))


# ------------------------------------------------------------------------------------------------------------------------ the solve
def _stock_apply(c, p):
    """A p on the interior (B, n, n) for the nodal coefficient c (B, K, K): solve_gwf.m:16-32 without the matrix"""
    K = c.shape[-1]
    pp = torch.nn.functional.pad(p, (1, 1, 1, 1))
    c0, pc = c[:, 1:-1, 1:-1], p
    acc = 0.5 * (c0 + c[:, :-2, 1:-1]) * (pc - pp[:, :-2, 1:-1])
    acc = acc + 0.5 * (c0 + c[:, 2:, 1:-1]) * (pc - pp[:, 2:, 1:-1])
    acc = acc + 0.5 * (c0 + c[:, 1:-1, :-2]) * (pc - pp[:, 1:-1, :-2])
    acc = acc + 0.5 * (c0 + c[:, 1:-1, 2:]) * (pc - pp[:, 1:-1, 2:])
    return float((K - 1) ** 2) * acc


def _stock_solve(c, F, rtol, max_iter):
    """the K23 iteration in float64 torch operations -> (nodal P (B, K, K), iterations, relative residual, status)"""
    B, K = int(c.shape[0]), int(c.shape[-1])
    _, _, dst, inv = _grid_tables(K)
    dst, inv = dst.to(c.device), inv.to(c.device)

    def precondition(r):
        return dst @ ((dst @ r @ dst) * inv) @ dst

    def dot(a, b):
        return (a * b).sum(dim=(1, 2))

    b = F[:, 1:-1, 1:-1].contiguous()
    x, r = torch.zeros_like(b), b.clone()
    bb = dot(b, b)
    status = torch.where(bb == 0, 1, torch.where(torch.isfinite(bb), 0, 2)).to(torch.int32)
    iters = torch.zeros(B, dtype=torch.int32, device=c.device)
    relres = torch.where(bb == 0, torch.zeros_like(bb), torch.ones_like(bb))
    z = precondition(r)
    rho, p = dot(z, r), z
    status = torch.where((status == 0) & ((rho == 0) | ~torch.isfinite(rho)), 2, status).to(torch.int32)
    for _ in range(max_iter):
        active = status == 0
        if not bool(active.any()):
            break
        ap = _stock_apply(c, p)
        pap = dot(p, ap)
        bad = active & ((pap == 0) | ~torch.isfinite(pap))
        status = torch.where(bad, 2, status).to(torch.int32)
        active = status == 0
        am = active[:, None, None]
        alpha = torch.where(active, rho / pap, torch.zeros_like(rho))[:, None, None]
        x = torch.where(am, x + alpha * p, x)
        r_new = torch.where(am, r - alpha * ap, r)
        d = r_new - r
        r = r_new
        rr = dot(r, r)
        iters = iters + active.to(torch.int32)
        relres = torch.where(active, torch.sqrt(rr / bb), relres)
        done = active & (torch.sqrt(rr) <= rtol * torch.sqrt(bb))
        status = torch.where(active & ~torch.isfinite(rr), 2, torch.where(done, 1, status)).to(torch.int32)
        active = status == 0
        z = precondition(r)
        rho_new, beta = dot(z, r), dot(z, d) / rho
        bad = active & ((rho_new == 0) | ~torch.isfinite(rho_new) | ~torch.isfinite(beta))
        status = torch.where(bad, 2, status).to(torch.int32)
        active = status == 0
        p = torch.where(active[:, None, None], z + beta[:, None, None] * p, p)
        rho = torch.where(active, rho_new, rho)
    return torch.nn.functional.pad(x, (1, 1, 1, 1)), iters, relres, status


def solve_gwf(coef, F=None, rtol=1e-10, max_iter=500, native=None, return_info=False, check_every=8):
    """solve_gwf.m:4-37: the solution of -div(coef grad p) = F, p = 0 on the border, on the s x s cell centres, for coef (B, s, s) or
    (s, s) and F of the same shape (default: ones, demo.m:30), in coef's dtype and shape; float64 inside, cast once at the end.  The
    result is NOT transposed against the input (the reference's column-major A \\ F(:), row-major vec2mat and trailing ' cancel).
    native: None - K23 for HIP tensors with s in 8 ... 512 (and in NATIVE_DEFAULT_SIZES), the stock path otherwise; True - K23 or an
    error that names its limits; False - the stock path.  A sample that misses rtol within max_iter raises RuntimeError naming it and its
    residual; with return_info=True the call returns (p, info) instead, info = dict(iterations, residual, converged, status) of (B,)
    tensors (status: 1 converged, 0 max_iter reached, 2 breakdown: a zero or non-finite p^T A p, rho or norm)."""
    single = coef.dim() == 2
    c = (coef[None] if single else coef)
    if c.dim() != 3 or c.shape[-1] != c.shape[-2]:
        raise ValueError(f"solve_gwf: coef must be (B, s, s) or (s, s) (got {tuple(coef.shape)})")
    s = int(c.shape[-1])
    if s < 4:
        raise ValueError("solve_gwf: the spline transfer needs s >= 4")
    if native is None:
        native = native_takes(c) and s in NATIVE_DEFAULT_SIZES
    elif native and not native_takes(c):
        raise RuntimeError(f"solve_gwf(native=True): the native solver takes HIP tensors (B, s, s) with s in 8 ... 512 "
                           f"(got {tuple(coef.shape)} on {coef.device})")
    c64 = c.to(torch.float64)
    f64 = torch.ones_like(c64) if F is None else (F[None] if F.dim() == 2 else F).to(torch.float64).expand_as(c64)
    if int(c64.shape[0]) == 0:
        out = torch.empty_like(coef)
        empty = dict(iterations=torch.zeros(0, dtype=torch.int32, device=coef.device), residual=torch.zeros(0, dtype=torch.float64, device=coef.device),
                     converged=torch.zeros(0, dtype=torch.bool, device=coef.device), status=torch.zeros(0, dtype=torch.int32, device=coef.device))
        return (out, empty) if return_info else out
    c_nodes = _two_sided("cn", c64, native)
    f_nodes = _two_sided("cn", f64.contiguous(), native)
    if native:
        P, iters, relres, status = _native.darcy_solve(c_nodes, f_nodes, rtol=rtol, max_iter=max_iter, check_every=check_every)
    else:
        P, iters, relres, status = _stock_solve(c_nodes, f_nodes, rtol, max_iter)
    info = dict(iterations=iters, residual=relres, converged=status == 1, status=status)
    if not return_info:
        bad = torch.nonzero(status != 1).flatten().tolist()
        if bad:
            res = relres.cpu()
            raise RuntimeError(f"solve_gwf: sample {bad[0]} did not reach rtol={rtol:g} within {max_iter} iterations (relative residual "
                               f"{float(res[bad[0]]):.3e}, status {int(status[bad[0]])}; {len(bad)} of {len(res)} samples failed)")
    p = _two_sided("nc", P, native).to(coef.dtype)
    p = p[0] if single else p
    return (p, info) if return_info else p


# ------------------------------------------------------------------------------------------------------------------------ the dataset
def generate_darcy_dataset(path, n_samples=1024, s=421, alpha=2, tau=3, hi=12, lo=4, kind="thresh", bsize=16, seed=None, device=None,
                           native=None, verbose=False):
    """n_samples of demo.m:13-34 in batches of bsize (the last may be smaller): u = darcy_grf(alpha, tau, s), coeff = threshold(u, hi, lo)
    (kind="thresh") or exp(u) (kind="lognorm"), sol = solve_gwf(coeff, 1), written with scipy.io.savemat as `coeff` and `sol`, both
    (n_samples, s, s) float32 - the fields data_load_darcy.py reads through MatReader.  Returns (coeff, sol) as numpy arrays."""
    import numpy as np
    import scipy.io

    if kind not in ("thresh", "lognorm"):
        raise ValueError(f"generate_darcy_dataset: kind must be 'thresh' or 'lognorm' (got {kind!r})")
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    gen = None
    if seed is not None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
    coeff = np.empty((n_samples, s, s), dtype=np.float32)
    sol = np.empty((n_samples, s, s), dtype=np.float32)
    done = 0
    while done < n_samples:
        nb = min(bsize, n_samples - done)
        u = darcy_grf(alpha, tau, s, nb, device=device, generator=gen, native=native)
        a = threshold(u, float(hi), float(lo)) if kind == "thresh" else torch.exp(u)
        p = solve_gwf(a, native=native)
        coeff[done:done + nb] = a.to(torch.float32).cpu().numpy()
        sol[done:done + nb] = p.to(torch.float32).cpu().numpy()
        done += nb
        if verbose:
            print(f"{done} / {n_samples} samples", flush=True)
    scipy.io.savemat(path, mdict={"coeff": coeff, "sol": sol}, do_compression=True)
    return coeff, sol


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m uno_amd.harness.darcy_datagen", description="Generate a Darcy-flow dataset (.mat)")
    ap.add_argument("--out", required=True, help="the .mat file to write")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--size", type=int, default=421)
    ap.add_argument("--alpha", type=float, default=2.0)
    ap.add_argument("--tau", type=float, default=3.0)
    ap.add_argument("--hi", type=float, default=12.0)
    ap.add_argument("--lo", type=float, default=4.0, help="the low value of the thresholded coefficient (the public FNO files used 3)")
    ap.add_argument("--kind", choices=("thresh", "lognorm"), default="thresh")
    ap.add_argument("--bsize", type=int, default=16)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    generate_darcy_dataset(a.out, a.samples, a.size, a.alpha, a.tau, a.hi, a.lo, a.kind, a.bsize, a.seed, a.device, verbose=True)
    print(f"wrote {a.samples} samples to {a.out}")


if __name__ == "__main__":
    main()
