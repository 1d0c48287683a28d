"""Accuracy of the shell-binned energy spectrum kernel (uno_shell_spectrum, K24) and of the float32 torch.fft path of harness.spectra
against the float64 definition (np.fft.fft2 over the full spectrum, brute-force round(hypot)) on white-noise frames, at the shapes of
tests/test_hip_shell_spectrum.py: per shape the worst l1 bin error relative to the total energy and the worst relative error of a single
bin, for both forms, and the ratio kernel / FFT that the test's BIN_FACTOR is set from (developer tool).
usage: python tools/shell_spectrum_accuracy.py        (profiles/shell_spectrum_accuracy.txt; needs an MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spectra_reference import spectrum_f64
from uno_amd import _native
from uno_amd.harness import spectra

if not torch.cuda.is_available():
    sys.exit("shell_spectrum_accuracy.py: no HIP device")
dev = torch.device("cuda:0")
CASES = [(1, 1, 8, 8), (3, 3, 9, 9), (1, 10, 21, 21), (3, 20, 32, 32), (1, 3, 64, 64), (3, 10, 64, 64), (1, 20, 85, 85), (3, 1, 8, 9), (1, 3, 21, 16),
         (3, 10, 64, 32), (1, 1, 421, 421), (1, 2, 512, 512)]

print(f"# white-noise frames (B, T, H, W), float32, against float64; one MI355X ({torch.cuda.get_device_name(0)})")
print("# l1: max over frames of sum_k |E - E64| / sum_k E64;  bin: max over frames and shells of |E - E64| / E64")
for B, T, H, W in CASES:
    g = torch.Generator().manual_seed(1000 * H + 10 * W + T)              # the test's frames
    x = torch.randn(B, T, H, W, generator=g)
    want = spectrum_f64(x.double().numpy())
    x = x.to(dev)
    kern = _native.shell_spectrum(x)[:, :, 0].double().cpu().numpy()
    fft = spectra._torch_spectra(x).double().cpu().numpy()
    l1 = [float((np.abs(v - want).sum(-1) / want.sum(-1)).max()) for v in (kern, fft)]
    bn = [float((np.abs(v - want) / want).max()) for v in (kern, fft)]
    print(f"({B}, {T}, {H}, {W})  l1: kernel {l1[0]:.2e}  fft {l1[1]:.2e}   bin: kernel {bn[0]:.3e}  fft {bn[1]:.3e}  ratio {bn[0] / bn[1]:.2f}")
