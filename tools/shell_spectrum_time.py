"""Time of the shell-binned energy spectra of a prediction, its target and their difference (harness.spectral_errors / energy_spectrum) in
their two forms: the native one-pass call (uno_shell_spectrum, K24: two launches) and the stock path (torch.fft.rfft2, abs^2, Hermitian
weight, index_add_ per spectrum) at the shapes the predict stage hands it: the NS-2D roll-out's time-major (20, 40, 64, 64) with target,
the NS-3D output (8, 64, 64, 20) and (4, 256, 256, 20) time-innermost with target, and Darcy (16, 421, 421) without (developer tool;
bench.py is the contract).
usage: python tools/shell_spectrum_time.py [calls]

One process, the two forms alternated call by call; every shape warmed up first; median and min .. max of `calls` (at least 50) timed
calls, device events around each call with one synchronisation at its end - the time covers the host's enqueueing where that is the
longer of the two.  harness.spectra dispatches to the kernel by default (native=None) wherever it applies: a shape at which the kernel's
median exceeded the stock path's would have to be taken out of that dispatch.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uno_amd.harness import energy_spectrum, spectral_errors

if not torch.cuda.is_available():
    sys.exit("shell_spectrum_time.py: no HIP device")
calls = max(50, int(sys.argv[1])) if sys.argv[1:] else 60
dev = torch.device("cuda:0")
# (what, shape, layout, with target)
SHAPES = [("NS-2D roll-out, time-major", (20, 40, 64, 64), "bthw", True), ("NS-3D output", (8, 64, 64, 20), "bhwt", True),
          ("NS-3D output at 256^2", (4, 256, 256, 20), "bhwt", True), ("Darcy", (16, 421, 421), "bhw", False)]


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def ab(forms, n, warm=5):
    """-> {name: (median, min, max)} in ms; the forms alternate call by call"""
    for _ in range(warm):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(n):
        for k, fn in forms.items():
            t[k].append(one(fn))
    return {k: stats(v) for k, v in t.items()}


def fmt(s):
    return f"{s[0]:8.3f} ms ({s[1]:.3f} .. {s[2]:.3f})"


print(f"# shell-binned energy spectra, float32, one MI355X ({torch.cuda.get_device_name(0)}); {calls} alternated calls each, median (min .. max)")
for what, shape, layout, with_target in SHAPES:
    g = torch.Generator().manual_seed(1)
    y = torch.randn(*shape, generator=g).to(dev)
    x = y + 0.1 * torch.randn(*shape, generator=g).to(dev)
    if with_target:
        forms = {"native": lambda: spectral_errors(x, y, layout, native=True), "stock": lambda: spectral_errors(x, y, layout, native=False)}
        a, b = forms["native"]().error, forms["stock"]().error
    else:
        forms = {"native": lambda: energy_spectrum(x, layout, native=True), "stock": lambda: energy_spectrum(x, layout, native=False)}
        a, b = forms["native"](), forms["stock"]()
    dist = float((a.double() - b.double()).abs().sum() / b.double().sum())
    r = ab(forms, calls)
    moved = 4.0 * x.numel() * (2 if with_target else 1) / 1e6
    verdict = "kernel" if r["native"][0] <= r["stock"][0] else "STOCK PATH (the kernel is slower here)"
    print(f"{what} {shape} {'with' if with_target else 'without'} target   native {fmt(r['native'])}   stock {fmt(r['stock'])}   "
          f"ratio {r['native'][0] / r['stock'][0]:.3f}   {moved:.1f} MB of frames   l1 distance of the two forms {dist:.1e}   native=None: {verdict}")
