"""Time of the NS-3D loop's per-time-step error metric (reference ns_train_3d.py:55-62) in its two forms: the native one-pass call
(harness.step_errors -> uno_rel_l2_steps, K17: two launches) and the stock loop the reference runs - T slices, each `sub`, two `norm`s,
`div`, `sum`, `add` - at (B, S, S, T_f) = (8, 64, 64, 40), (8, 64, 64, 20) and (16, 64, 64, 10), the output shapes of Uno3D_T40 / T20 / T10
at their benchmark batch sizes; then, for Uno3D_T40 and Uno3D_T20 at widths 8 and 32 (batch 8, 64^2), the eager training step
(forward + loss + backward + Adam) without the metric, with the native one and with the stock loop, and the share of the plain step each
form adds (developer tool; bench.py is the contract).
usage: python tools/step_error_time.py [calls] [all | kernel | models]

One process, the two forms alternated call by call; every shape warmed up first; median and min .. max of `calls` (at least 50) timed
calls, device events around each call with one synchronisation at its end - the time covers the host's enqueueing where that is the
longer of the two, as it is for the stock loop's ~6 T launches.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uno_amd.harness import ComplexAdam, Uno3D_T20, Uno3D_T40, lp_loss_rel_sum, step_errors

if not torch.cuda.is_available():
    sys.exit("step_error_time.py: no HIP device")
section = "all"
if sys.argv[1:] and sys.argv[-1] in ("all", "kernel", "models"):
    section = sys.argv.pop()
calls = max(50, int(sys.argv[1])) if sys.argv[1:] else 60
dev = torch.device("cuda:0")
SHAPES = [(8, 64, 64, 40), (8, 64, 64, 20), (16, 64, 64, 10)]


def stock_loop(out, y):
    """the reference's loop with LpLoss(size_average=False).rel written out (utilities3.py:86-100)"""
    B = out.shape[0]
    total = 0
    for t in range(out.shape[-1]):
        k, l = out[..., t].reshape(B, -1), y[..., t].reshape(B, -1)
        diff = torch.norm(k - l, 2, 1)
        norm = torch.norm(l, 2, 1)
        total = total + torch.sum(diff / norm)
    return total


def native(out, y):
    return step_errors(out, y).step_sum


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


def kernel_section():
    print(f"# per-time-step relative L2 error of (B, S, S, T_f) float32 under no_grad; {calls} alternated calls each, median (min .. max)")
    for shape in SHAPES:
        g = torch.Generator().manual_seed(1)
        y = torch.randn(*shape, generator=g).to(dev)
        out = y + 0.1 * torch.randn(*shape, generator=g).to(dev)
        with torch.no_grad():
            a, b = float(native(out, y)), float(stock_loop(out, y))
            r = ab({"native": lambda: native(out, y), "stock": lambda: stock_loop(out, y)}, calls)
        moved = 8.0 * y.numel() / 1e6
        print(f"{shape}  native {fmt(r['native'])}   stock loop {fmt(r['stock'])}   ratio {r['native'][0] / r['stock'][0]:.3f}"
              f"   {moved:.1f} MB read once = {moved / r['native'][0] / 1e3:.2f} TB/s   native / stock value distance {abs(a - b) / abs(b):.1e}")


def model_section():
    print(f"# eager training step (forward + loss + backward + Adam), batch 8, 64^2, float32, synthetic data, one MI355X "
          f"({torch.cuda.get_device_name(0)}); {calls} alternated steps each, median (min .. max)")
    for cls, T_f in ((Uno3D_T40, 40), (Uno3D_T20, 20)):
        for width in (8, 32):
            torch.manual_seed(0)
            m = cls(6, width, pad=3).to(dev)
            opt = ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4)
            x, y = torch.randn(8, 64, 64, 10, 1, device=dev), torch.randn(8, 64, 64, T_f, device=dev)

            def step(metric):
                opt.zero_grad(set_to_none=True)
                out = m(x).view(8, 64, 64, T_f)
                if metric is not None:
                    with torch.no_grad():
                        metric(out.detach(), y)
                lp_loss_rel_sum(out.reshape(8, -1), y.reshape(8, -1)).backward()
                opt.step()
            r = ab({"plain": lambda: step(None), "native": lambda: step(native), "stock": lambda: step(stock_loop)}, calls, warm=3)
            p = r["plain"][0]
            print(f"{cls.__name__}(6, {width}, pad=3)  without the metric {fmt(r['plain'])}   with native {fmt(r['native'])} = {100 * (r['native'][0] - p) / p:+.1f} %"
                  f"   with the stock loop {fmt(r['stock'])} = {100 * (r['stock'][0] - p) / p:+.1f} %")
            del m, opt
            torch.cuda.empty_cache()


if section in ("all", "kernel"):
    kernel_section()
if section in ("all", "models"):
    model_section()
