"""What gradient-norm clipping costs, A/B in one process (developer tool; bench.py is the contract):

  (a) the optimiser step without clipping: ComplexAdam.step() - K10, the path every earlier commit takes;
  (b) the step with native clipping: ComplexAdam(max_grad_norm=...).step() - K26 (two launches per 24 tensors + one) and the guarded K10;
  (c) torch.nn.utils.clip_grad_norm_(foreach=True) followed by (a) - the stock remedy, without its host-side isfinite check;

on the parameter sets of UNO_9(3, 64, pad=5) (the headline Darcy model) and of the NS-2D UNO(14, 32), with random gradients that are
never clipped (max_grad_norm far above the norm: (c) skips no work, its multiply by 1 included); then the whole eager Darcy step
(forward, loss, backward, update at 421^2, batch 16) with and without max_grad_norm.
usage: python tools/bench_grad_clip.py [rounds] [all | optim | step]

The forms alternate inside every round; a figure is the median over the rounds of the mean time of `inner` back-to-back steps, timed
with device events (no host synchronisation inside a window).  (a) is timed twice per round: the distance of its two medians is the
run-to-run spread to read (b) - (a) and (c) - (a) against.  Needs an MI355X: there is no CPU path."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from uno_amd.harness import UNO, UNO_9, ComplexAdam, LpLoss

if not torch.cuda.is_available():
    sys.exit("bench_grad_clip.py: no HIP device")
section = "all"
if sys.argv[1:] and sys.argv[-1] in ("all", "optim", "step"):
    section = sys.argv.pop()
rounds = max(5, int(sys.argv[1])) if sys.argv[1:] else 15
dev = torch.device("cuda:0")


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def report(name, forms, inner):
    """forms: {label: callable}; every round times each once, in the given order"""
    for fn in forms.values():            # warm-up: code objects, plans, moments
        timed(fn, 3)
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(timed(fn, inner))
    med = {k: median(v) for k, v in times.items()}
    print(f"--- {name} ({rounds} rounds of {inner} steps; ms per step: median (min .. max))")
    for k, v in times.items():
        print(f"  {k:34s} {med[k]:8.4f} ({min(v):.4f} .. {max(v):.4f})")
    return med


def optimiser_forms(model):
    """three optimisers on three copies of the parameter set, each with its own random gradients"""
    def copy():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
        g = torch.Generator(device=dev).manual_seed(1)
        for p in ps:
            p.grad = torch.randn(p.shape, dtype=p.dtype, device=dev, generator=g) * 1e-3
        return ps
    pa, pb, pc = copy(), copy(), copy()
    oa, ob, oc = ComplexAdam(pa, lr=1e-3, weight_decay=1e-3), ComplexAdam(pb, lr=1e-3, weight_decay=1e-3, max_grad_norm=1e6), \
        ComplexAdam(pc, lr=1e-3, weight_decay=1e-3)

    def stock():
        torch.nn.utils.clip_grad_norm_(pc, 1e6, foreach=True)
        oc.step()
    floats = sum(p.numel() * (2 if p.is_complex() else 1) for p in pa)
    return floats, len(pa), {"(a) step, no clipping": oa.step, "(b) step, native clipping": ob.step, "(c) clip_grad_norm_ + (a)": stock,
                             "(a) again": oa.step}


def optim_section():
    for name, model in (("UNO_9(3, 64, pad=5)", UNO_9(3, 64, pad=5)), ("NS-2D UNO(14, 32)", UNO(14, 32))):
        floats, n, forms = optimiser_forms(model.to(dev))
        med = report(f"{name}: {n} tensors, {floats / 1e6:.2f} M floats", forms, 50)
        a = med["(a) step, no clipping"]
        print(f"  (b) - (a) = {med['(b) step, native clipping'] - a:+.4f} ms   (c) - (a) = {med['(c) clip_grad_norm_ + (a)'] - a:+.4f} ms   "
              f"spread of (a) = {abs(med['(a) again'] - a):.4f} ms")
        del forms
        torch.cuda.empty_cache()


def step_section():
    g = torch.Generator().manual_seed(1)
    x, y = torch.rand(16, 421, 421, 1, generator=g).to(dev), torch.rand(16, 421, 421, generator=g).to(dev)
    loss = LpLoss(size_average=False)

    def make(**guard):
        torch.manual_seed(0)
        model = UNO_9(3, 64, pad=5).to(dev)
        opt = ComplexAdam(model.parameters(), lr=1e-3, weight_decay=1e-3, **guard)

        def step():
            opt.zero_grad(set_to_none=True)
            loss(model(x).reshape(16, -1), y.reshape(16, -1)).backward()
            opt.step()
        return step
    plain, clipped = make(), make(max_grad_norm=1e6)
    med = report("Darcy step, UNO_9(3, 64, pad=5), 421^2, batch 16 (forward + loss + backward + update, eager)",
                 {"no clipping": plain, "max_grad_norm": clipped, "no clipping again": plain}, 10)
    print(f"  with - without = {med['max_grad_norm'] - med['no clipping']:+.4f} ms   spread = {abs(med['no clipping again'] - med['no clipping']):.4f} ms")


if section in ("all", "optim"):
    optim_section()
if section in ("all", "step"):
    step_section()
