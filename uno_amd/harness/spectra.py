"""Shell-binned energy spectra of predictions: at which wavenumber a roll-out loses the truth, whether a prediction at a finer grid
carries energy above the trained modes, whether a free-running roll-out is still physical where no target is left.

For a real frame u of H x W samples on the unit periodic box

    U = fft2(u) / (H W),   integer wavenumbers ky, kx in fftfreq order,
    shell s(ky, kx) = round(hypot(ky, kx)), decided in integers: s = k iff (2k - 1)^2 <= 4 (ky^2 + kx^2) < (2k + 1)^2,
    K = n_shells(H, W) = round(hypot(H // 2, W // 2)) + 1,   E(k) = sum over both Hermitian halves of |U|^2 on shell k,

so that sum_k E(k) = mean(u^2), and for a prediction u and a target v: sum_k E_{u-v}(k) / sum_k E_v(k) = (relative L2 error)^2 - the
figure rel_l2 / step_errors report, resolved by wavenumber.

float32 device tensors of 8 ... 512 points per axis whose frames are four non-negative strides apart take the native kernel (K24,
_native.shell_spectrum: one pass, the complex spectrum never written to memory, fixed summation order); everything else the same
definition on torch.fft.rfft2 and index_add_ in the input's dtype.  Forward only."""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

LAYOUTS = ("bhwt", "bthw", "bhw")


def n_shells(H: int, W: int) -> int:
    """K: every mode of an H x W frame falls in one of the shells 0 ... K - 1"""
    return _shell(int(H) // 2, int(W) // 2) + 1


def _shell(ky: int, kx: int) -> int:
    m = math.isqrt(4 * (ky * ky + kx * kx))
    return (m + 1) // 2


_TABLES = {}


def shell_index(H: int, W: int, device=None) -> torch.Tensor:
    """(H, W // 2 + 1) int64: the shell of every mode of the half spectrum rfft2 returns, by the integer rule"""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"shell_index: a {H} x {W} frame")
    device = torch.device("cpu") if device is None else torch.device(device)
    key = (H, W, str(device))
    if key not in _TABLES:
        ky = torch.fft.fftfreq(H, d=1.0 / H).round().to(torch.int64).reshape(H, 1)
        kx = torch.arange(W // 2 + 1, dtype=torch.int64).reshape(1, -1)
        n = 4 * (ky * ky + kx * kx)
        m = n.to(torch.float64).sqrt().floor().to(torch.int64)          # floor(sqrt(n)), corrected in integers below
        m = m - (m * m > n).to(torch.int64)
        m = m + ((m + 1) * (m + 1) <= n).to(torch.int64)
        from .. import _native
        _TABLES[key] = _native.table_to_device((m + 1) // 2, device)
    return _TABLES[key]


def _sobolev_a(k, a):
    """the k coefficients a_1 ... a_k as a tuple of floats (a: None - all 1 -, one number for every order, or k numbers)"""
    k = int(k)
    if k < 0:
        raise ValueError(f"sobolev_weights: order k = {k}")
    if a is None:
        return (1.0,) * k
    a = (float(a),) * k if isinstance(a, (int, float)) else tuple(float(v) for v in a)
    if len(a) != k:
        raise ValueError(f"sobolev_weights: {len(a)} coefficients for order k = {k}")
    return a


def sobolev_weights(H: int, W: int, k: int = 1, a=None) -> torch.Tensor:
    """(H // 2 + 1, W // 2 + 1) float64 on the CPU: w2[|ky|][|kx|] = 1 + sum_{j = 1 .. k} a_j^2 (ky^2 + kx^2)^j - the weight every mode
    (ky, kx) of the full spectrum takes in the Sobolev loss (losses.sobolev_rel); for k <= 2 the weight of FNO's HsLoss, squared.
    a_j defaults to 1; k = 0 gives all ones (plain relative L2, by Parseval)."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"sobolev_weights: a {H} x {W} frame")
    a = _sobolev_a(k, a)
    ky = torch.arange(H // 2 + 1, dtype=torch.float64).reshape(-1, 1)
    kx = torch.arange(W // 2 + 1, dtype=torch.float64).reshape(1, -1)
    k2 = ky * ky + kx * kx
    w2 = torch.ones_like(k2)
    for j, aj in enumerate(a, start=1):
        w2 = w2 + (aj * aj) * k2 ** j
    return w2


_SOBOLEV_TABLES = {}


def sobolev_table(H: int, W: int, k: int = 1, a=None, device=None, dtype=torch.float32) -> torch.Tensor:
    """sobolev_weights on `device` in `dtype`, cached per (H, W, k, a, device, dtype) as shell_index is"""
    device = torch.device("cpu") if device is None else torch.device(device)
    key = (int(H), int(W), int(k), _sobolev_a(k, a), str(device), dtype)
    if key not in _SOBOLEV_TABLES:
        from .. import _native
        _SOBOLEV_TABLES[key] = _native.table_to_device(sobolev_weights(H, W, k, a).to(dtype), device)
    return _SOBOLEV_TABLES[key]


def _frames(u, layout, name):
    """-> the (B, T, H, W) view of u"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {', '.join(LAYOUTS)}")
    if u.dim() != len(layout):
        raise ValueError(f"{name} {tuple(u.shape)} is not a {layout!r} tensor of {len(layout)} axes")
    if not u.is_floating_point():
        raise ValueError(f"{name} must be a real floating-point tensor (got {u.dtype})")
    if u.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"energy spectra are not differentiable: {name} requires grad (detach it, or call under torch.no_grad())")
    if layout == "bhwt":
        return u.permute(0, 3, 1, 2)
    return u if layout == "bthw" else u.unsqueeze(1)


def _native_refusal(x, y):
    """None where K24 takes these (B, T, H, W) views, or why it does not"""
    from .. import _native
    lo, hi = _native.SHELL_SPECTRUM_MIN, _native.SHELL_SPECTRUM_MAX
    for name, t in (("the input", x), ("the target", y)):
        if t is None:
            continue
        if not t.is_cuda:
            return f"{name} is on {t.device}, the kernel runs on the GPU"
        if t.dtype != torch.float32:
            return f"{name} is {t.dtype}, the kernel takes float32"
        if min(t.stride()) < 0:
            return f"{name} has a negative stride {t.stride()}"
    H, W = x.shape[2:]
    if not (lo <= H <= hi and lo <= W <= hi):
        return f"frames of {H} x {W}: the kernel takes {lo} ... {hi} points per axis"
    if x.shape[1] < 1:
        return "no frame per sample"
    if y is not None and y.device != x.device:
        return f"input on {x.device}, target on {y.device}"
    return None


def _torch_spectra(x):
    """(B, T, H, W) of any float dtype and device -> (B, T, K) by the definition, on rfft2 and index_add_"""
    B, T, H, W = x.shape
    K = n_shells(H, W)
    if B * T == 0:
        return x.new_zeros((B, T, K))
    U = torch.fft.rfft2(x, dim=(-2, -1))
    p = U.real * U.real + U.imag * U.imag
    w = torch.full((W // 2 + 1,), 2.0, dtype=p.dtype, device=p.device)
    w[0] = 1.0
    if W % 2 == 0:
        w[W // 2] = 1.0
    p = p * (w / (float(H) * W) ** 2)
    out = p.new_zeros((B * T, K))
    out.index_add_(1, shell_index(H, W, x.device).reshape(-1), p.reshape(B * T, -1))
    return out.view(B, T, K)


def _spectra(x, y, native, who):
    """(B, T, H, W) views -> (B, T, 1 or 3, K)"""
    if y is not None and y.shape != x.shape:
        raise ValueError(f"{who}: prediction {tuple(x.shape)} and target {tuple(y.shape)} differ")
    why = _native_refusal(x, y)
    if native and why is not None:
        raise RuntimeError(f"{who}(native=True): {why}")
    if native is None and why is None:
        native = True
    if native and x.shape[0] > 0:
        from .. import _native
        return _native.shell_spectrum(x, y)
    if y is None:
        return _torch_spectra(x).unsqueeze(2)
    if y.dtype != x.dtype or y.device != x.device:
        raise ValueError(f"{who}: prediction ({x.dtype}, {x.device}) and target ({y.dtype}, {y.device}) differ")
    return torch.stack((_torch_spectra(x), _torch_spectra(y), _torch_spectra(x - y)), dim=2)


def energy_spectrum(u, layout="bhwt", native=None):
    """E(k) of every frame of u: (B, H, W, T) -> (B, T, K) for layout "bhwt", (B, T, H, W) -> (B, T, K) for "bthw", (B, H, W) -> (B, K)
    for "bhw"; views (time slices, [::r, ::r] sub-sampling) are read where they lie.  native: None - the kernel where it applies, else
    torch; True - the kernel, a RuntimeError saying why where it does not apply; False - torch."""
    x = _frames(u, layout, "u")
    with torch.no_grad():
        e = _spectra(x, None, native, "energy_spectrum")[:, :, 0]
    return e[:, 0] if layout == "bhw" else e


class SpectralErrors(NamedTuple):
    """spectra of a prediction, of its target and of their difference, (B, T, K) each, and k = arange(K)"""
    pred: torch.Tensor
    target: torch.Tensor
    error: torch.Tensor
    k: torch.Tensor


def spectral_errors(pred, target, layout="bhwt", native=None):
    """-> SpectralErrors(E_pred, E_target, E_{pred - target}, k), (B, T, K) each (T = 1 for layout "bhw"); the two tensors may lie in
    memory differently as long as `layout` describes both.  sum_k error / sum_k target = (relative L2 error)^2 per frame."""
    x, y = _frames(pred, layout, "pred"), _frames(target, layout, "target")
    with torch.no_grad():
        e = _spectra(x, y, native, "spectral_errors")
    return SpectralErrors(e[:, :, 0], e[:, :, 1], e[:, :, 2], torch.arange(e.shape[-1], device=e.device))
