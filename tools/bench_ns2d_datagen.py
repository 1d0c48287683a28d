"""Time of the Navier-Stokes data generator's solver, harness.datagen.navier_stokes_2d (reference ns_datagen.py:15-140), in its two forms
on one GPU: the native one (K22: uno_ns2d_steps, three launches per time step from one C loop) and the torch.fft path of the same
function (native=False: five 2-D FFTs and the element-wise operations between them per step), at (N, B) = (256, 20) - the reference's
own configuration - (128, 20) and (64, 20), on the generator's own input (GaussianRF(2, N, alpha=2.5, tau=7), the forcing of
ns_datagen.py:164-169, visc = 1e-3, delta_t = 1e-4) (developer tool; bench.py is the contract).
usage: python tools/bench_ns2d_datagen.py [blocks] [steps per block]

One process; both forms warmed up at every size, then `blocks` (default 7, at least 5) timed calls of `steps` (default 200) time steps
each, the forms alternated block by block, a host clock around a call that ends in a device synchronise; median and min .. max of the
blocks.  A call is navier_stokes_2d with one record, so it carries one forward and one inverse transform besides its steps (under 1 %).
Printed per size: microseconds per time step of both forms, their device launches per step (the library's own launch records for the
native form, torch.profiler for the stock one), the distance of the two results, the time both forms would need for the reference's
batch of 500 000 steps, and the median time of each of the three kernels over 100 more steps (the library's launch records: HIP events
around every launch, which add a few microseconds to a step).  Needs an MI355X: there is no CPU path."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from uno_amd import _native
from uno_amd.harness.datagen import GaussianRF, navier_stokes_2d, ns_forcing

if not torch.cuda.is_available():
    sys.exit("bench_ns2d_datagen.py: no HIP device")
blocks = max(5, int(sys.argv[1])) if sys.argv[1:] else 7
steps = max(1, int(sys.argv[2])) if sys.argv[2:] else 200
dev = torch.device("cuda:0")
VISC, DT, REFERENCE_STEPS = 1e-3, 1e-4, 500_000


def horizon(n):
    """a T that navier_stokes_2d turns into exactly n steps"""
    return (n - 0.5) * DT


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def stock_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA)


print(f"# navier_stokes_2d, float32, one MI355X ({torch.cuda.get_device_name(0)}); {blocks} alternated blocks of {steps} time steps per form, "
      f"median (min .. max) in microseconds per step")
for N, B in ((256, 20), (128, 20), (64, 20)):
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    w0 = GaussianRF(2, N, alpha=2.5, tau=7, device=dev, generator=gen).sample(B)
    f = ns_forcing(N, dev)
    forms = {"native": lambda n=steps: navier_stokes_2d(w0, f, VISC, horizon(n), DT, 1, native=True)[0],
             "stock": lambda n=steps: navier_stokes_2d(w0, f, VISC, horizon(n), DT, 1, native=False)[0]}
    out = {k: fn() for k, fn in forms.items()}          # warm-up: every shape both forms use
    dist = float((out["native"] - out["stock"]).norm() / out["stock"].norm())
    t = {k: [] for k in forms}
    for _ in range(blocks):
        for k, fn in forms.items():
            t[k].append(timed(fn) / steps * 1e6)
    r = {k: stats(v) for k, v in t.items()}
    _native.profile_begin(64)
    forms["native"](3)
    n3 = len(_native.profile_end())
    _native.profile_begin(64)
    forms["native"](1)
    native_per_step = (n3 - len(_native.profile_end())) / 2
    try:
        stock_per_step = (stock_launches(lambda: forms["stock"](3)) - stock_launches(lambda: forms["stock"](1))) / 2
    except Exception as e:          # the profiler is a convenience here: the timings do not depend on it
        stock_per_step = float("nan")
        print(f"    stock launch count unavailable: {type(e).__name__}: {e}")
    print(f"N={N:3d} B={B}  native {r['native'][0]:8.1f} us/step ({r['native'][1]:.1f} .. {r['native'][2]:.1f}), {native_per_step:g} launches/step"
          f"   stock {r['stock'][0]:8.1f} us/step ({r['stock'][1]:.1f} .. {r['stock'][2]:.1f}), {stock_per_step:g} launches/step"
          f"   native / stock {r['native'][0] / r['stock'][0]:.3f}   result distance after {steps} steps {dist:.1e}")
    print(f"           a batch of {REFERENCE_STEPS} steps: native {r['native'][0] * REFERENCE_STEPS / 1e6 / 60:.1f} min, "
          f"stock {r['stock'][0] * REFERENCE_STEPS / 1e6 / 60:.1f} min (projected from the medians)")
    w_h = _native.ns2d_forward(w0.contiguous())          # (sample() returns the real part of a complex tensor: a strided view)
    f_h = _native.ns2d_forward(f[None])[0]
    _native.profile_begin(512)
    _native.ns2d_steps(w_h, f_h, 100, VISC, DT)
    per_kernel = {}
    for name, ms, nbytes in _native.profile_end():
        per_kernel.setdefault(name, []).append((ms * 1e3, nbytes))
    print("           " + "   ".join(f"{name.split('::')[-1]} {stats([u for u, _ in v])[0]:.1f} us ({v[0][1] / 1e6:.1f} MB algorithmic)"
                                     for name, v in per_kernel.items()))
