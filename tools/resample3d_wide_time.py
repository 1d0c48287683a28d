"""Forward + backward time of pointwise_op_3D on the first and last layer of Uno3D_T20_256 at S = 256, pad 2 - conv0
(256,256,12) -> (64,64,12) and conv8 (64,64,24) -> (256,256,24), width 8, batch 4 - through the wide-axis HIP kernels
(uno_fft_resample3d_wide) and through STOCK_FFT_RESAMPLE3D = True (torch.fft / rocFFT: the only way to run these grids before), and one
Uno3D_T20_256(6, 8, pad=2) training step at batch 4 both ways ("layers"); OperatorBlock_3D forward + backward on the same two layers on
the wide-axis kernels in one buffer (uno_fft_resample3d_wide_acc) against the two branches ("blocks"); and the three kernels of both
layers, operator and adjoint, from the library's event records with their algorithmic bytes ("kernels").  Developer tool; bench.py is
the contract.
usage: python tools/resample3d_wide_time.py [iters] [reps] [all | layers | blocks | kernels]

One process, the two paths alternated group by group; every shape warmed up first; median and min .. max of `reps` timed groups of
`iters` passes, device events around each group, one synchronisation at each end.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import uno_amd.integral_operators as io
from uno_amd.harness import ComplexAdam, ns3d_loss
from uno_amd.harness.models import Uno3D_T20_256

if not torch.cuda.is_available():
    sys.exit("resample3d_wide_time.py: no HIP device")
section = "all"
if sys.argv[1:] and sys.argv[-1] in ("all", "layers", "blocks", "kernels"):
    section = sys.argv.pop()
args = [int(a) for a in sys.argv[1:]]
iters, reps = (args + [10, 7])[:2] if len(args) < 2 else args[:2]
dev = torch.device("cuda:0")
W, B = 8, 4
# (Ci / w, Co / w, din, dout, modes, InstanceNorm3d) at S = 256, pad 2
LAYERS = {"conv0": (1, 2, (256, 256, 12), (64, 64, 12), (32, 32, 5), True), "conv8": (4, 2, (64, 64, 24), (256, 256, 24), (32, 32, 8), False)}


def group(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def ab(first, second, n=iters):
    """-> ((median, min, max) of `first`, the same of `second`) in ms; groups alternate"""
    for _ in range(3):
        first()
        second()
    t = ([], [])
    for _ in range(reps):
        t[0].append(group(first, n))
        t[1].append(group(second, n))
    return tuple((sorted(v)[len(v) // 2], min(v), max(v)) for v in t)


def switched(fn, **switches):
    """fn under the given module switches of integral_operators, which are back at their defaults afterwards"""
    def run():
        for k, v in switches.items():
            setattr(io, k, v)
        try:
            fn()
        finally:
            for k in switches:
                setattr(io, k, False)
    return run


def report(what, r, names):
    (mn, lo, hi), (ms, slo, shi) = r
    print(f"{what:<46} {names[0]} {mn:8.3f} ms ({lo:.3f} .. {hi:.3f})   {names[1]} {ms:8.3f} ms ({slo:.3f} .. {shi:.3f})   "
          f"ratio {mn / ms:5.2f}", flush=True)


print(f"{torch.cuda.get_device_name(0)}; {iters} passes per group, {reps} groups per path, median (min .. max)")
NATIVE = dict(NATIVE_RESAMPLE3D_WIDE=True, NATIVE_RESAMPLE3D_ANY=True)
for name, (ci, co, din, dout, modes, norm) in LAYERS.items() if section in ("all", "layers") else ():
    torch.manual_seed(0)
    layer = io.pointwise_op_3D(ci * W, co * W, *dout).to(dev)
    x = torch.randn(B, ci * W, *din, device=dev, requires_grad=True)
    gy = torch.randn(B, co * W, *dout, device=dev)

    def fb():
        x.grad = None
        layer.zero_grad(set_to_none=True)
        layer(x, *dout).backward(gy)
    report(f"pointwise_op_3D {name} w{W} B{B} fwd+bwd", ab(switched(fb, **NATIVE), switched(fb, STOCK_FFT_RESAMPLE3D=True)), ("wide-axis kernels", "torch.fft"))
    del layer, x, gy

for name, (ci, co, din, dout, modes, norm) in LAYERS.items() if section in ("all", "blocks") else ():
    torch.manual_seed(0)
    blk = io.OperatorBlock_3D(ci * W, co * W, *dout, *modes, Normalize=norm).to(dev)
    x = torch.randn(B, ci * W, *din, device=dev, requires_grad=True)
    gy = torch.randn(B, co * W, *dout, device=dev)

    def fb():
        x.grad = None
        blk.zero_grad(set_to_none=True)
        blk(x, *dout).backward(gy)
    report(f"OperatorBlock_3D {name} w{W} B{B} fwd+bwd", ab(switched(fb, ONE_BUFFER_3D_ANY=True, **NATIVE), switched(fb, **NATIVE)), ("one buffer", "two branches"))
    del blk, x, gy

if section in ("all", "layers", "blocks"):
    torch.manual_seed(0)
    model = Uno3D_T20_256(6, W, pad=2).to(dev)
    for m in model.modules():                       # the module switches decide the path here, not the class's own opt-ins
        if isinstance(m, io.pointwise_op_3D):
            m.native_any_grid = m.native_wide_grid = False
    opt = ComplexAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(1)
    xb, yb = torch.randn(B, 256, 256, 10, 1, generator=g).to(dev), torch.randn(B, 256, 256, 20, generator=g).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        ns3d_loss(model, xb, yb).backward()
        opt.step()
    n = max(2, iters // 2)
    if section != "blocks":
        report(f"Uno3D_T20_256(6, {W}, pad=2) B{B} training step", ab(switched(step, **NATIVE), switched(step, STOCK_FFT_RESAMPLE3D=True), n), ("wide-axis kernels", "torch.fft"))
    if section != "layers":
        report(f"Uno3D_T20_256(6, {W}, pad=2) B{B} training step", ab(switched(step, ONE_BUFFER_3D_ANY=True, **NATIVE), switched(step, **NATIVE), n), ("one buffer", "two branches"))
    del model, opt, xb, yb

# ---- kernels: K1w / K5w / K3w of both layers, operator and adjoint, from the library's own event records
if section in ("all", "kernels"):
    from uno_amd import _native
    from uno_amd.spectral3d import _resample3d_plan_wide
    for name, (_, co, din, dout, _modes, _norm) in LAYERS.items():
        t1, t2, m3 = _resample3d_plan_wide(din, dout, dev)
        a = ((t1, t1), (t2, t2), m3, 1.0 / (dout[0] * dout[1] * dout[2]))
        for adjoint, (src, size) in ((False, (din, dout)), (True, (dout, din))):
            x = torch.randn(B, co * W, *src, device=dev)
            for _ in range(3):
                _native.fft_resample3d_wide(x, size, *a, adjoint=adjoint)
            torch.cuda.synchronize()
            _native.profile_begin(8 * iters)
            for _ in range(iters):
                _native.fft_resample3d_wide(x, size, *a, adjoint=adjoint)
            torch.cuda.synchronize()
            recs = _native.profile_end()
            for i, kernel in enumerate(("K1w fwd_plane", "K5w axis", "K3w inv_plane")):
                ms = sorted(r[1] for r in recs[i::3])
                med, nbytes = ms[len(ms) // 2], recs[i][2]
                print(f"{kernel:<14} {name} {'adjoint ' if adjoint else 'operator'} {src} -> {size} x {B * co * W} volumes "
                      f"{med * 1e3:8.1f} us ({ms[0] * 1e3:.1f} .. {ms[-1] * 1e3:.1f})   {nbytes / 1e6:7.1f} MB algorithmic = {nbytes / med / 1e6:5.0f} GB/s",
                      flush=True)
            del x
