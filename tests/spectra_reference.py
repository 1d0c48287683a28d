"""The float64 yardstick of the shell-binned energy spectrum, shared by tests/test_spectra_cpu.py and tests/test_hip_shell_spectrum.py:
the definition restated on np.fft.fft2 over the FULL spectrum with a brute-force round(hypot) - no half-spectrum weights, no integer rule."""
import numpy as np


def full_shells(H, W):
    """round(hypot(ky, kx)) of every mode of the full fftfreq grid"""
    ky, kx = np.fft.fftfreq(H, 1.0 / H)[:, None], np.fft.fftfreq(W, 1.0 / W)[None, :]
    return np.rint(np.hypot(ky, kx)).astype(np.int64)


def spectrum_f64(u):
    """(..., H, W) -> (..., K) float64: every mode of fft2(u) / (H W) binned by its shell"""
    u = np.asarray(u, dtype=np.float64)
    H, W = u.shape[-2:]
    sh = full_shells(H, W).ravel()
    p = (np.abs(np.fft.fft2(u) / (H * W)) ** 2).reshape(-1, H * W)
    K = int(sh.max()) + 1
    out = np.stack([np.bincount(sh, weights=row, minlength=K) for row in p]) if p.shape[0] else np.zeros((0, K))
    return out.reshape(u.shape[:-2] + (K,))
