"""Time and peak memory of one NS-3D training step (forward + ns3d_loss + backward + Adam, harness.DarcyTrainer.step_with as the c4 workload
of bench.py runs it) with the model's inner skip connections in their two forms: the default (torch.cat of a block's output and the
resized skip tensor in front of the next block: reference navier_stokes_uno3d.py `torch.cat([x_c, skip], dim=1)`) and cat-free
(harness.models.enable_cat_free_skips_3d -> OperatorBlock_3D.forward_cat: the next block reads its two sources where they lie), on ONE
model whose `cat_free_skips` attribute is flipped step by step - same weights, same batch, same process (developer tool; bench.py is
the contract).
usage: python tools/ns3d_skips_time.py [steps] [all | w8 | w32 | 256 | w32ends]

Configurations: Uno3D_T20(6, 8, pad=3) and Uno3D_T20(6, 32, pad=3) at 64^2, batch 8; Uno3D_T20_256(6, 8, pad=2) at 256^2, batch 4; and
the width-32 64^2 model with enable_native_ends_3d on in BOTH forms (then the cat-free form has no torch.cat of activations left).
Both forms are warmed up; median and min .. max of `steps` (at least 20) timed steps each, the forms alternating, device events around
every step with one synchronisation at its end.  Peak memory: torch.cuda.max_memory_allocated over one step of each form, reset in
front of it (what the step allocates on top of the model, optimiser state and batch, plus those).  The library's own launch records of
one step of each form give the launches per step.  Needs an MI355X: there is no CPU path."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from uno_amd import _native
from uno_amd.harness import DarcyTrainer, Uno3D_T20, ns3d_loss
from uno_amd.harness.models import Uno3D_T20_256, enable_cat_free_skips_3d, enable_native_ends_3d

if not torch.cuda.is_available():
    sys.exit("ns3d_skips_time.py: no HIP device")
args = sys.argv[1:]
section = args.pop() if args and args[-1] in ("all", "w8", "w32", "256", "w32ends") else "all"
steps = max(20, int(args[0])) if args else 20
dev = torch.device("cuda:0")
# class, width, pad, S, batch, native ends
CONFIGS = {"w8": (Uno3D_T20, 8, 3, 64, 8, False), "w32": (Uno3D_T20, 32, 3, 64, 8, False), "256": (Uno3D_T20_256, 8, 2, 256, 4, False),
           "w32ends": (Uno3D_T20, 32, 3, 64, 8, True)}


def build(key):
    cls, width, pad, S, B, ends = CONFIGS[key]
    torch.manual_seed(0)
    model = cls(6, width, pad=pad).to(dev)
    enable_native_ends_3d(model, ends)
    trainer = DarcyTrainer(model, lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(1234)
    x, y = torch.randn(B, S, S, 10, 1, generator=g).to(dev), torch.randn(B, S, S, 20, generator=g).to(dev)

    def step(cat_free):
        enable_cat_free_skips_3d(model, cat_free)
        return trainer.step_with(lambda: ns3d_loss(model, x, y))
    return f"{cls.__name__}(6, {width}, pad={pad}), {S}^2, batch {B}" + (", native ends" if ends else ""), step


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def fmt(s):
    return f"{s[0]:8.3f} ms ({s[1]:.3f} .. {s[2]:.3f})"


def launches(step, cat_free):
    _native.profile_begin(100000)
    try:
        step(cat_free)
        torch.cuda.synchronize()
    finally:
        rec = _native.profile_end()
    return len(rec)


def peak(step, cat_free):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    step(cat_free)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev)


def run(key):
    what, step = build(key)
    for _ in range(3):
        step(False)
        step(True)
    torch.cuda.synchronize()
    t = {False: [], True: []}
    for _ in range(steps):
        for cat_free in (False, True):
            t[cat_free].append(one(lambda: step(cat_free)))
    d, n = stats(t[False]), stats(t[True])
    if n[1] > d[2]:
        verdict = "SLOWER: the two min .. max ranges do not overlap"
    elif n[2] < d[1]:
        verdict = "faster: the two min .. max ranges do not overlap"
    else:
        verdict = ("faster" if n[0] < d[0] else "slower") + " by the medians, the min .. max ranges overlap"
    print(f"{what}: default {fmt(d)}   cat-free skips {fmt(n)}   ratio {n[0] / d[0]:.3f}   ({verdict})")
    md, mn = peak(step, False), peak(step, True)
    print(f"    peak allocated memory: default {md / 2**20:9.1f} MiB, cat-free skips {mn / 2**20:9.1f} MiB ({(mn - md) / 2**20:+.1f} MiB: "
          f"{'fell' if mn < md else 'did not fall'})")
    print(f"    library launches per step: default {launches(step, False)}, cat-free skips {launches(step, True)}")


print(f"# NS-3D training step, the inner skip connections in both forms, one MI355X ({torch.cuda.get_device_name(0)}); {steps} alternated steps "
      "each, median (min .. max)")
for key in CONFIGS:
    if section in ("all", key):
        run(key)
