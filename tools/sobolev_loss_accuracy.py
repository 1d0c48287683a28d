"""Accuracy of the Sobolev loss kernel (uno_sobolev_forward, K25) and of the float32 torch.fft path of harness.losses against the float64
definition (np.fft.fft2 over the full spectrum, brute-force weight) at the shapes of tests/test_hip_sobolev_loss.py, on white noise and
on frames with a steep spectrum (amplitude ~ (1 + |k|^2)^(-3/2)), k = 1 and 2: per shape the worst relative error of a frame's num and
den for both forms, and the ratio kernel / FFT that the test's STEEP_FACTOR is set from (developer tool).
usage: python tools/sobolev_loss_accuracy.py        (profiles/sobolev_loss_accuracy.txt; needs an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import sobolev_reference as ref
from uno_amd import _native
from uno_amd.harness import losses, spectra

if not torch.cuda.is_available():
    sys.exit("sobolev_loss_accuracy.py: no HIP device")
dev = torch.device("cuda:0")
CASES = [(1, 1, 8, 8), (3, 3, 9, 9), (1, 10, 21, 21), (3, 20, 32, 32), (3, 10, 64, 32), (1, 20, 85, 85), (3, 1, 8, 9), (1, 3, 21, 16),
         (1, 1, 421, 421), (1, 2, 512, 512)]


def worst(got, want):
    return float((np.abs(got.double().cpu().numpy() - want) / want).max())


def measure(x, y, k):
    """-> (kernel, fft): the worst relative error of num and den over the frames"""
    B, T, H, W = x.shape
    num, den = ref.sums_f64(x.double().numpy(), y.double().numpy(), k)
    x, y = x.to(dev), y.to(dev)
    record, _ = _native.sobolev_forward(x, y, spectra.sobolev_table(H, W, k, None, dev, torch.float32), True)
    sums = _native.sobolev_views(record, B, T, True)[0]
    wt = losses._half_weights(H, W, k, None, dev, torch.float32)
    D, Y = torch.fft.rfft2(x - y), torch.fft.rfft2(y)
    s_num, s_den = (wt * (D.real ** 2 + D.imag ** 2)).sum(dim=(-2, -1)), (wt * (Y.real ** 2 + Y.imag ** 2)).sum(dim=(-2, -1))
    return max(worst(sums[..., 0], num), worst(sums[..., 1], den)), max(worst(s_num, num), worst(s_den, den))


print(f"# frames (B, T, H, W), float32, against float64; one MI355X ({torch.cuda.get_device_name(0)})")
print("# worst over the frames of |num - num64| / num64 and |den - den64| / den64; the test floors the FFT figure at 2^-24 = 5.96e-08")
for B, T, H, W in CASES:
    g = torch.Generator().manual_seed(1000 * H + 10 * W + T)              # the test's white-noise frames
    white = torch.randn(B, T, H, W, generator=g), torch.randn(B, T, H, W, generator=g)
    steep = tuple(torch.from_numpy(ref.steep_frames(B, T, H, W, 7 * H + W + i)).float() for i in range(2))       # the test's steep frames
    for k in (1, 2):
        (wk, wf), (sk, sf) = measure(*white, k), measure(*steep, k)
        print(f"({B}, {T}, {H}, {W}) k={k}  white: kernel {wk:.3e}  fft {wf:.3e}   steep: kernel {sk:.3e}  fft {sf:.3e}  "
              f"ratio {sk / max(sf, 2.0 ** -24):.2f}")
