"""The float64 yardstick of the Sobolev loss tests: the definition of uno_amd.harness.losses.sobolev_rel over the FULL np.fft.fft2 spectrum
with a brute-force weight - no half spectrum, no Hermitian weights, no table."""
import numpy as np


def weight_full(H, W, k=1, a=None):
    """(H, W) float64: 1 + sum_{j = 1 .. k} a_j^2 (ky^2 + kx^2)^j at the integer wavenumbers of np.fft.fft2"""
    ky = np.fft.fftfreq(H, d=1.0 / H).round().reshape(H, 1)
    kx = np.fft.fftfreq(W, d=1.0 / W).round().reshape(1, W)
    k2 = ky * ky + kx * kx
    a = [1.0] * k if a is None else ([float(a)] * k if np.isscalar(a) else [float(v) for v in a])
    assert len(a) == k
    w = np.ones((H, W))
    for j in range(1, k + 1):
        w = w + a[j - 1] ** 2 * k2 ** j
    return w


def sums_f64(x, y, k=1, a=None):
    """x, y (..., H, W) -> num, den (...): sum_k w |X - Y|^2 and sum_k w |Y|^2 with X = fft2(x) / (H W)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    H, W = x.shape[-2:]
    w = weight_full(H, W, k, a)
    D, Y = np.fft.fft2(x - y) / (H * W), np.fft.fft2(y) / (H * W)
    return (w * np.abs(D) ** 2).sum(axis=(-2, -1)), (w * np.abs(Y) ** 2).sum(axis=(-2, -1))


def ratio_f64(x, y, k=1, a=None, per_frame=False):
    """x, y (B, T, H, W) -> (B, T) per frame, else (B,) from the sums over a sample's frames"""
    num, den = sums_f64(x, y, k, a)
    if not per_frame:
        num, den = num.sum(axis=1), den.sum(axis=1)
    return np.sqrt(num) / np.sqrt(den)


def grad_f64(x, y, g, k=1, a=None, per_frame=False):
    """the closed-form gradient of sum(g * ratio) at x, (B, T, H, W): g f / (H W sqrt(num den)), f = ifft2(w fft2(x - y)); g: (B, T) or (B,)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    H, W = x.shape[-2:]
    f = np.fft.ifft2(weight_full(H, W, k, a) * np.fft.fft2(x - y))
    assert np.abs(f.imag).max() <= 1e-9 * max(np.abs(f.real).max(), 1e-300)
    num, den = sums_f64(x, y, k, a)
    g = np.asarray(g, dtype=np.float64)
    if not per_frame:
        num, den, g = num.sum(axis=1)[:, None], den.sum(axis=1)[:, None], g.reshape(-1, 1)
    coef = g / (H * W * np.sqrt(num * den))
    return (coef * np.ones(x.shape[:2]))[:, :, None, None] * f.real


def steep_frames(B, T, H, W, seed):
    """(B, T, H, W) float64 frames whose spectral amplitude falls as (1 + |k|^2)^(-3/2): white noise filtered in float64"""
    rng = np.random.default_rng(seed)
    ky = np.fft.fftfreq(H, d=1.0 / H).reshape(H, 1)
    kx = np.fft.fftfreq(W, d=1.0 / W).reshape(1, W)
    u = np.fft.ifft2(np.fft.fft2(rng.standard_normal((B, T, H, W))) * (1.0 + ky * ky + kx * kx) ** -1.5).real
    return u / np.sqrt((u * u).mean())
