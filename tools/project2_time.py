"""Forward + backward time of the two-source GELU projection (K11's TWO form, `gelu_project2`: the end of UNO_P / UNO_S256) against the
stock composition it replaces - `channel_mix(torch.cat([F.gelu(pre), F.gelu(s)], 1), weight, bias)` under autograd, which is what
`gelu_project2` itself falls back to and what these models would run without the kernel - at (B, C1, C2, pixels) = (16, 96, 16, 256^2)
and (32, 96, 16, 64^2); then one training-step time each of UNO_P(14, 32) at 64^2, batch 16, T_f = 40 (replayed from one HIP graph),
of UNO(14, 32) in the same setting for scale, and of UNO_S256(14, 32) at 256^2, batch 16, single step (eager and replayed)
(developer tool; bench.py is the contract).
usage: python tools/project2_time.py [iters] [reps] [all | kernel | models]

One process, the two paths alternated group by group; every shape warmed up first; median and min .. max of `reps` timed groups of
`iters` passes, device events around each group, one synchronisation at each end.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from uno_amd.harness import UNO, UNO_P, UNO_S256, ComplexAdam, GraphedStep, ns2d_rollout_loss
from uno_amd.integral_operators import channel_mix, gelu_project2

if not torch.cuda.is_available():
    sys.exit("project2_time.py: no HIP device")
section = "all"
if sys.argv[1:] and sys.argv[-1] in ("all", "kernel", "models"):
    section = sys.argv.pop()
args = [int(a) for a in sys.argv[1:]]
iters, reps = (args + [10, 7][len(args):])[:2]
dev = torch.device("cuda:0")
SHAPES = [(16, 96, 16, (256, 256)), (32, 96, 16, (64, 64))]


def group(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def ab(native, stock, n):
    """-> {path: (median, min, max)} in ms; groups alternate native / stock"""
    for _ in range(3):
        native()
        stock()
    t = {"native": [], "stock": []}
    for _ in range(reps):
        t["native"].append(group(native, n))
        t["stock"].append(group(stock, n))
    return {k: stats(v) for k, v in t.items()}


def fmt(s):
    return f"{s[0]:8.3f} ms ({s[1]:.3f} .. {s[2]:.3f})"


def kernel_section():
    print(f"# gelu_project2 forward + backward, act2 = 1, every operand with gradient; {reps} groups of {iters} passes, median (min .. max)")
    for B, C1, C2, grid in SHAPES:
        g = torch.Generator().manual_seed(1)
        pre = torch.randn(B, C1, *grid, generator=g).to(dev).requires_grad_(True)
        s = torch.randn(B, C2, *grid, generator=g).to(dev).requires_grad_(True)
        w = torch.randn(1, C1 + C2, generator=g).to(dev).requires_grad_(True)
        b = torch.randn(1, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(B, 1, *grid, generator=g).to(dev)
        leaves = (pre, s, w, b)

        def native():
            return torch.autograd.grad(gelu_project2(pre, s, w, b, act2=True), leaves, gy)

        def stock():
            return torch.autograd.grad(channel_mix(torch.cat([F.gelu(pre), F.gelu(s)], 1), w, b), leaves, gy)
        worst = max(float((a - r).norm() / r.norm()) for a, r in zip(native(), stock()))
        r = ab(native, stock, iters)
        P = grid[0] * grid[1]
        moved = 4.0 * B * P * (2 * (C1 + C2) + (C1 + C2) + 2) / 1e6          # forward reads both sources; backward reads and writes them
        print(f"({B}, {C1}, {C2}, {grid[0]}x{grid[1]})  native {fmt(r['native'])}   stock {fmt(r['stock'])}   ratio {r['native'][0] / r['stock'][0]:.3f}"
              f"   native bytes {moved:.0f} MB = {moved / r['native'][0] / 1e3:.2f} TB/s   worst gradient distance native / stock {worst:.1e}")
        del pre, s, gy
        torch.cuda.empty_cache()


def graphed(model_cls, B, S, T_in, T_f, label):
    torch.manual_seed(0)
    m = model_cls(T_in + 4, 32).to(dev)
    xx, yy = torch.randn(B, S, S, T_in, device=dev), torch.randn(B, S, S, T_f, device=dev)
    opt = ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    gs = GraphedStep(m, opt, lambda a, b: ns2d_rollout_loss(m, a, b, T_f=T_f, step=1), (xx, yy))
    for _ in range(2):
        gs.step(xx, yy)
    t = [group(lambda: gs.step(xx, yy), max(1, iters // 4)) for _ in range(reps)]
    print(f"{label}: forward + loss + backward + Adam replayed from one HIP graph   {fmt(stats(t))}")
    del gs, m, opt
    torch.cuda.empty_cache()


def eager(model_cls, B, S, T_in, label):
    torch.manual_seed(0)
    m = model_cls(T_in + 4, 32).to(dev)
    xx, yy = torch.randn(B, S, S, T_in, device=dev), torch.randn(B, S, S, 1, device=dev)
    opt = ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        ns2d_rollout_loss(m, xx, yy, T_f=1, step=1).backward()
        opt.step()
    for _ in range(3):
        step()
    t = [group(step, iters) for _ in range(reps)]
    print(f"{label}: eager forward + loss + backward + Adam   {fmt(stats(t))}")
    del m, opt
    torch.cuda.empty_cache()


def models_section():
    print(f"# training steps, width 32, float32, synthetic data, one MI355X ({torch.cuda.get_device_name(0)}); {reps} groups, median (min .. max)")
    graphed(UNO_P, 16, 64, 10, 40, "UNO_P(14, 32), 64^2, batch 16, T 10 -> 40 roll-out")
    graphed(UNO, 16, 64, 10, 40, "UNO(14, 32), 64^2, batch 16, T 10 -> 40 roll-out (for scale)")
    eager(UNO_S256, 16, 256, 10, "UNO_S256(14, 32), 256^2, batch 16, single step")
    graphed(UNO_S256, 16, 256, 10, 1, "UNO_S256(14, 32), 256^2, batch 16, single step")


if section in ("all", "kernel"):
    kernel_section()
if section in ("all", "models"):
    models_section()
