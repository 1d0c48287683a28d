"""Time of the relative Sobolev loss (harness.HsLoss, k = 1, summed over the batch) in its two forms - the native one (uno_sobolev_forward /
uno_sobolev_backward, K25: two launches forward, one backward) and the stock path (torch.fft.rfft2, weight, abs^2, sums; autograd's irfft2
chain backward) - forward alone and forward + backward, and beside them K20's relative L2 (harness.LpLoss), the floor a training step
paid before, at the shapes the three loops hand a loss: Darcy (16, 421, 421) and (32, 64, 64) as "bhw", NS-3D (8, 64, 64, 20) and
(4, 256, 256, 20) time-innermost as "bhwt", and a scan of shapes between them (developer tool; bench.py is the contract).
usage: python tools/sobolev_loss_time.py [calls]        (profiles/sobolev_loss_time.txt)

One process, the forms alternated call by call; every shape warmed up first; median and min .. max of `calls` (at least 50) timed calls,
device events around each call with one synchronisation at its end - the time covers the host's enqueueing where that is the longer of
the two.  losses.sobolev_native_default keeps the kernel under native=None only where its median forward + backward time was below the
stock path's (a bound on the grid side and on the dense work per call, set from this table); every shape's line says what the rule takes.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uno_amd.harness import HsLoss, LpLoss
from uno_amd.harness.losses import sobolev_native_default

if not torch.cuda.is_available():
    sys.exit("sobolev_loss_time.py: no HIP device")
calls = max(50, int(sys.argv[1])) if sys.argv[1:] else 60
dev = torch.device("cuda:0")
# (what, shape, layout)
SHAPES = [("Darcy", (16, 421, 421), "bhw"), ("Darcy at 64^2", (32, 64, 64), "bhw"), ("NS-3D output", (8, 64, 64, 20), "bhwt"),
          ("NS-3D output at 256^2", (4, 256, 256, 20), "bhwt"),
          # between the workloads' shapes: where the dense transforms stop paying (losses.sobolev_native_default)
          ("scan", (16, 128, 128), "bhw"), ("scan", (8, 128, 128, 20), "bhwt"), ("scan", (16, 256, 256), "bhw"), ("scan", (2, 256, 256, 20), "bhwt"),
          ("scan", (8, 85, 85, 20), "bhwt"), ("scan", (4, 421, 421), "bhw"), ("scan", (32, 421, 421), "bhw"), ("scan", (4, 512, 512), "bhw")]


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
    return f"{s[0]:7.3f} ms ({s[1]:.3f} .. {s[2]:.3f})"


print(f"# relative Sobolev loss H^1 against K20's relative L2, float32, one MI355X ({torch.cuda.get_device_name(0)}); {calls} alternated calls "
      "each, median (min .. max)")
for what, shape, layout in SHAPES:
    g = torch.Generator().manual_seed(1)
    y = torch.randn(*shape, generator=g).to(dev)
    x = (y + 0.1 * torch.randn(*shape, generator=g).to(dev)).requires_grad_(True)
    hs = {name: HsLoss(k=1, layout=layout, size_average=False, native=native) for name, native in (("native", True), ("stock", False))}
    l2 = LpLoss(size_average=False)

    def both(loss):
        x.grad = None
        loss(x, y).backward()

    def alone(loss):
        with torch.no_grad():
            loss(x, y)
    fwd = ab({"native": lambda: alone(hs["native"]), "stock": lambda: alone(hs["stock"]), "l2": lambda: alone(l2)}, calls)
    fb = ab({"native": lambda: both(hs["native"]), "stock": lambda: both(hs["stock"]), "l2": lambda: both(l2)}, calls)
    both(hs["native"])
    ga = x.grad.clone()
    both(hs["stock"])
    dist = float((ga - x.grad).norm() / x.grad.norm())
    frames, (H, W) = (shape[0] * (shape[3] if layout == "bhwt" else 1)), shape[1:3]
    verdict = ("the kernel is faster" if fb["native"][0] <= fb["stock"][0] else "THE KERNEL IS SLOWER") + "; native=None takes " + \
        ("the kernel" if sobolev_native_default(frames, 1, H, W) else "stock ops")
    print(f"{what} {shape} {layout!r}   {4.0 * x.numel() / 1e6:.1f} MB per tensor   dense work {frames * H * W * (W + 2 * H) / 1e9:.2f} G   gradient distance of the two forms {dist:.1e}   forward + backward: {verdict}")
    for name, r in (("forward", fwd), ("forward + backward", fb)):
        print(f"    {name:18s} native {fmt(r['native'])}   stock {fmt(r['stock'])}   ratio {r['native'][0] / r['stock'][0]:.3f}   "
              f"relative L2 (K20) {fmt(r['l2'])}")
