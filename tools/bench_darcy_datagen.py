"""Time of the Darcy-flow data generator's solve, harness.darcy_datagen.solve_gwf (reference solve_gwf.m:4-37), in its two forms on one
GPU: the native one (K23: the spline transfers on uno_darcy_transform, the preconditioned CG loop of uno_darcy_solve, 9 launches per
iteration from one C loop) and the stock path of the same function (native=False: the same iteration in float64 torch operations), at
421^2 - the size of the reference's dataset - for batches of 1 and 16, on the generator's own input (thresholded 12 | 4 fields of
darcy_grf(2, 3, 421), f = 1, rtol = 1e-10) (developer tool; bench.py is the contract; there is no pass / fail threshold).
usage: python tools/bench_darcy_datagen.py [blocks] [size]

One process; both forms warmed up, then `blocks` (default 7, at least 5) timed calls each, the forms alternated call by call, a host clock
around a call that ends in a device synchronise; median and min .. max of the blocks.  Printed per batch size: milliseconds per sample of
both forms, the iteration counts of both, the native form's launches per iteration (the library's own launch records) and the median
time of each kernel over one more solve (HIP events around every launch, which add a few microseconds each).  Needs an MI355X: the
comparison has no CPU form."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from uno_amd import _native
from uno_amd.harness.darcy_datagen import darcy_grf, solve_gwf, threshold

if not torch.cuda.is_available():
    sys.exit("bench_darcy_datagen.py: no HIP device")
blocks = max(5, int(sys.argv[1])) if sys.argv[1:] else 7
S = int(sys.argv[2]) if sys.argv[2:] else 421
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


print(f"# solve_gwf, {S}^2, thresholded GRF(2, 3), f = 1, rtol = 1e-10, one MI355X ({torch.cuda.get_device_name(0)}); {blocks} alternated calls "
      f"per form, median (min .. max) in milliseconds per sample")
for B in (1, 16):
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    coef = threshold(darcy_grf(2, 3, S, B, device=dev, generator=gen))
    forms = {"native": lambda: solve_gwf(coef, native=True, return_info=True), "stock": lambda: solve_gwf(coef, native=False, return_info=True)}
    out = {k: fn() for k, fn in forms.items()}          # warm-up: tables, allocator
    dist = float((out["native"][0] - out["stock"][0]).norm() / out["stock"][0].norm())
    its = {k: v[1]["iterations"].tolist() for k, v in out.items()}
    assert all(bool(v[1]["converged"].all()) for v in out.values())
    t = {k: [] for k in forms}
    for _ in range(blocks):
        for k, fn in forms.items():
            t[k].append(timed(fn) / B * 1e3)
    r = {k: stats(v) for k, v in t.items()}
    torch.cuda.synchronize()
    _native.profile_begin(4096)
    forms["native"]()
    records = _native.profile_end()
    solve_launches = sum(1 for name, _, _ in records if "darcy" in name) - 6          # (the three spline transfers: 2 launches each)
    max_it = max(its["native"])
    enq = -(-max_it // 8) * 8           # the loop runs to the next look at the status words
    per_kernel = {}
    for name, ms, _ in records:
        per_kernel.setdefault(name, []).append(ms * 1e3)
    print(f"B={B:2d}  native {r['native'][0]:8.3f} ms/sample ({r['native'][1]:.3f} .. {r['native'][2]:.3f})   stock {r['stock'][0]:8.3f} ms/sample "
          f"({r['stock'][1]:.3f} .. {r['stock'][2]:.3f})   native / stock {r['native'][0] / r['stock'][0]:.3f}   distance of the results {dist:.1e}")
    print(f"      iterations native {min(its['native'])} .. {max_it}, stock {min(its['stock'])} .. {max(its['stock'])}; "
          f"{solve_launches} launches in the solve = 8 + 9 x {(solve_launches - 8) / 9:g} enqueued iterations (expected {enq})")
    print("      " + "   ".join(f"{name.split('::')[-1]} x{len(v)} {stats(v)[0]:.1f} us" for name, v in per_kernel.items()))
