"""Forward + backward time of pointwise_op_3D on the two Uno3D_T40 layers outside the pruned-DFT kernels' range, through the any-grid
HIP kernels (uno_fft_resample3d_any) and through STOCK_FFT_RESAMPLE3D = True (torch.fft: what a user of these layers ran before),
and one Uno3D_T40(6, 8, pad=3) training step both ways; then ("blocks") OperatorBlock_3D forward + backward on the same two layers
with the any-grid kernels in both forms - one buffer (`one_buffer_any_grid`: uno_fft_resample3d_any_acc, no stock add / GELU / gradient
sum) against the two branches - and the training step both ways; and ("kernels") K1a, K5a and K3a in its plain, accumulate and accumulate +
GELU forms from the library's event records, which is also the program to put behind `rocprofv3 --kernel-trace --stats --`
(developer tool; bench.py is the contract).
usage: python tools/resample3d_any_time.py [iters] [reps] [all | layers | blocks | kernels]

One process, the two paths alternated group by group; every shape warmed up first; median and min .. max of `reps` timed groups of
`iters` passes, device events around each group, one synchronisation at each end.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import uno_amd.integral_operators as io
from uno_amd.harness import ComplexAdam, Uno3D_T40, ns3d_loss

if not torch.cuda.is_available():
    sys.exit("resample3d_any_time.py: no HIP device")
section = "all"
if sys.argv[1:] and sys.argv[-1] in ("all", "layers", "blocks", "kernels"):
    section = sys.argv.pop()
args = [int(a) for a in sys.argv[1:]]
iters, reps = (args + [10, 7])[:2] if len(args) < 2 else args[:2]
dev = torch.device("cuda:0")
LAYERS = {"conv7": (8, 2, (32, 32, 31), (48, 48, 41)), "conv8": (4, 2, (48, 48, 41), (64, 64, 52))}     # (Ci / w, Co / w, din, dout), pad 3


def group(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def ab(native, stock, n=iters):
    """-> {path: (median, min, max)} in ms; groups alternate native / stock"""
    for _ in range(3):
        native()
        stock()
    t = {"native": [], "stock": []}
    for _ in range(reps):
        t["native"].append(group(native, n))
        t["stock"].append(group(stock, n))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def with_switch(native, fn):
    def run():
        io.NATIVE_RESAMPLE3D_ANY, io.STOCK_FFT_RESAMPLE3D = native, not native
        try:
            fn()
        finally:
            io.NATIVE_RESAMPLE3D_ANY, io.STOCK_FFT_RESAMPLE3D = False, False
    return run


def report(what, r):
    (mn, lo, hi), (ms, slo, shi) = r["native"], r["stock"]
    print(f"{what:<44} any-grid kernels {mn:8.3f} ms ({lo:.3f} .. {hi:.3f})   torch.fft {ms:8.3f} ms ({slo:.3f} .. {shi:.3f})   "
          f"native / stock {mn / ms:5.2f}", flush=True)


print(f"{torch.cuda.get_device_name(0)}; {iters} passes per group, {reps} groups per path, median (min .. max)")
B = 8
for w in (8, 32) if section in ("all", "layers") else ():
    for name, (ci, co, din, dout) in LAYERS.items():
        torch.manual_seed(0)
        layer = io.pointwise_op_3D(ci * w, co * w, *dout).to(dev)
        x = torch.randn(B, ci * w, *din, device=dev, requires_grad=True)
        gy = torch.randn(B, co * w, *dout, device=dev)

        def fb():
            x.grad = None
            layer.zero_grad(set_to_none=True)
            layer(x, *dout).backward(gy)
        report(f"pointwise_op_3D {name} w{w} B{B} fwd+bwd", ab(with_switch(True, fb), with_switch(False, fb)))
        del layer, x, gy

torch.manual_seed(0)
model = Uno3D_T40(6, 8, pad=3).to(dev)
opt = ComplexAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
g = torch.Generator().manual_seed(1)
xb, yb = torch.randn(B, 64, 64, 10, 1, generator=g).to(dev), torch.randn(B, 64, 64, 40, generator=g).to(dev)


def step():
    opt.zero_grad(set_to_none=True)
    ns3d_loss(model, xb, yb).backward()
    opt.step()


if section in ("all", "layers"):
    for m in model.modules():                      # the module switches decide the path here, not the per-module opt-in
        if isinstance(m, io.pointwise_op_3D):
            m.native_any_grid = False
    report(f"Uno3D_T40(6, 8, pad=3) B{B} training step", ab(with_switch(True, step), with_switch(False, step), n=max(2, iters // 2)))


# ---- blocks: one buffer against two branches, both on the any-grid kernels (the module switch decides, group by group)
def with_one_buffer(on, fn):
    def run():
        io.NATIVE_RESAMPLE3D_ANY, io.ONE_BUFFER_3D_ANY = True, on
        try:
            fn()
        finally:
            io.NATIVE_RESAMPLE3D_ANY, io.ONE_BUFFER_3D_ANY = False, False
    return run


def report_blocks(what, r):
    (mn, lo, hi), (ms, slo, shi) = r["native"], r["stock"]
    print(f"{what:<44} one buffer {mn:8.3f} ms ({lo:.3f} .. {hi:.3f})   two branches {ms:8.3f} ms ({slo:.3f} .. {shi:.3f})   "
          f"one / two {mn / ms:5.2f}", flush=True)


BLOCKS = {"conv7": ((14, 14, 10), True), "conv8": ((20, 20, 14), False)}       # modes, InstanceNorm3d
for w in (8, 32) if section in ("all", "blocks") else ():
    for name, (ci, co, din, dout) in LAYERS.items():
        modes, norm = BLOCKS[name]
        torch.manual_seed(0)
        blk = io.OperatorBlock_3D(ci * w, co * w, *dout, *modes, Normalize=norm).to(dev)
        x = torch.randn(B, ci * w, *din, device=dev, requires_grad=True)
        gy = torch.randn(B, co * w, *dout, device=dev)

        def fb():
            x.grad = None
            blk.zero_grad(set_to_none=True)
            blk(x, *dout).backward(gy)
        report_blocks(f"OperatorBlock_3D {name} w{w} B{B} fwd+bwd", ab(with_one_buffer(True, fb), with_one_buffer(False, fb)))
        del blk, x, gy

if section in ("all", "blocks"):
    for m in model.modules():
        if isinstance(m, io.pointwise_op_3D):
            m.native_any_grid = False
    report_blocks(f"Uno3D_T40(6, 8, pad=3) B{B} training step", ab(with_one_buffer(True, step), with_one_buffer(False, step), n=max(2, iters // 2)))


# ---- kernels: K3a plain / accumulate / accumulate + GELU, one launch of each per round, the library's own event records
if section in ("all", "kernels"):
    from uno_amd import _native
    from uno_amd.spectral3d import _resample3d_plan_any
    FORMS = ("plain", "acc", "acc+gelu")
    for w in (8, 32):
        for name, (_, co, din, dout) in LAYERS.items():
            t1, t2, m3 = _resample3d_plan_any(din, dout, dev)
            x = torch.randn(B, co * w, *din, device=dev)
            s = torch.zeros(B, co * w, *dout, device=dev)
            a = ((t1, t1), (t2, t2), m3, 1.0 / (dout[0] * dout[1] * dout[2]))

            def round_():
                _native.fft_resample3d_any(x, dout, *a, adjoint=False)
                _native.fft_resample3d_any(x, dout, *a, adjoint=False, out=s)
                _native.fft_resample3d_any(x, dout, *a, adjoint=False, out=s, act=True)
            for _ in range(3):
                round_()
            torch.cuda.synchronize()
            _native.profile_begin(16 * iters)
            for _ in range(iters):
                round_()
            torch.cuda.synchronize()
            every = _native.profile_end()
            for kernel, part in (("K1a", "fwd_plane"), ("K5a", "axis")):        # the same launch in all three calls of a round
                ms = sorted(r[1] for r in every if part in r[0])
                med, nbytes = ms[len(ms) // 2], next(r[2] for r in every if part in r[0])
                print(f"{kernel} {name} grid w{w} B{B} {part:<9} {med * 1e3:8.1f} us ({ms[0] * 1e3:.1f} .. {ms[-1] * 1e3:.1f})   "
                      f"{nbytes / 1e6:7.1f} MB algorithmic = {nbytes / med / 1e6:5.0f} GB/s", flush=True)
            recs = [r for r in every if "inv_plane" in r[0]]
            for i, form in enumerate(FORMS):
                ms = sorted(r[1] for r in recs[i::3])
                med, nbytes = ms[len(ms) // 2], recs[i][2]
                print(f"K3a {name} grid w{w} B{B} {form:<9} {med * 1e3:8.1f} us ({ms[0] * 1e3:.1f} .. {ms[-1] * 1e3:.1f})   "
                      f"{nbytes / 1e6:7.1f} MB algorithmic = {nbytes / med / 1e6:5.0f} GB/s", flush=True)
            del x, s
