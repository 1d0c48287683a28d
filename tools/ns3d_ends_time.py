"""Time of one NS-3D training step (forward + ns3d_loss + backward + Adam, harness.DarcyTrainer.step_with as the c4 workload of bench.py
runs it) with the model's two ends in their two forms: the default (F.gelu + F.pad after the lift, torch.cat + crop + .contiguous() in
front of fc1: reference navier_stokes_uno3d.py:304-318, 358-382) and opted into the short-row window kernels
(harness.models.enable_native_ends_3d -> csrc/channel_mix_rows.hip), on ONE model whose `native_ends` attribute is flipped step by
step - same weights, same batch, same process (developer tool; bench.py is the contract).
usage: python tools/ns3d_ends_time.py [steps] [all | w8 | w32 | 256 | one256]

Configurations: Uno3D_T20(6, 8, pad=3) and Uno3D_T20(6, 32, pad=3) at 64^2, batch 8; Uno3D_T20_256(6, 8, pad=2) at 256^2, batch 4.
Both forms are warmed up; median and min .. max of `steps` (at least 20) timed steps each, the forms alternating, device events around
every step with one synchronisation at its end.  The library's own launch records of one step of each form follow (kernel, launches,
total ms, algorithmic GB/s of the new kernels).  `one256 default|native` runs a few steps of the 256^2 configuration in ONE form, for
a kernel trace of its own.  Needs an MI355X: there is no CPU path."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from uno_amd import _native
from uno_amd.harness import DarcyTrainer, Uno3D_T20, ns3d_loss
from uno_amd.harness.models import Uno3D_T20_256, enable_native_ends_3d

if not torch.cuda.is_available():
    sys.exit("ns3d_ends_time.py: no HIP device")
args = sys.argv[1:]
form = args.pop() if args and args[-1] in ("default", "native") else None
section = args.pop() if args and args[-1] in ("all", "w8", "w32", "256", "one256") else "all"
steps = max(20, int(args[0])) if args else 20
dev = torch.device("cuda:0")
CONFIGS = {"w8": (Uno3D_T20, 8, 3, 64, 8), "w32": (Uno3D_T20, 32, 3, 64, 8), "256": (Uno3D_T20_256, 8, 2, 256, 4)}
NEW = ("uno::rows_mix_kernel", "uno::rows_grad_kernel", "uno::rows_wgrad_kernel", "uno::rows_act_padded_kernel", "uno::rows_dgelu_kernel")


def build(key):
    cls, width, pad, S, B = CONFIGS[key]
    torch.manual_seed(0)
    model = cls(6, width, pad=pad).to(dev)
    trainer = DarcyTrainer(model, lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(1234)
    x, y = torch.randn(B, S, S, 10, 1, generator=g).to(dev), torch.randn(B, S, S, 20, generator=g).to(dev)

    def step(native):
        enable_native_ends_3d(model, native)
        return trainer.step_with(lambda: ns3d_loss(model, x, y))
    return f"{cls.__name__}(6, {width}, pad={pad}), {S}^2, batch {B}", step


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


def records(step, native):
    _native.profile_begin(100000)
    try:
        step(native)
        torch.cuda.synchronize()
    finally:
        rec = _native.profile_end()
    out = {}
    for name, ms, by in rec:
        n, t, b = out.get(name, (0, 0.0, 0.0))
        out[name] = (n + 1, t + ms, b + by)
    return out


def run(key):
    what, step = build(key)
    for _ in range(3):
        step(False)
        step(True)
    torch.cuda.synchronize()
    t = {False: [], True: []}
    for _ in range(steps):
        for native in (False, True):
            t[native].append(one(lambda: step(native)))
    d, n = stats(t[False]), stats(t[True])
    if n[1] > d[2]:
        verdict = "SLOWER: the two min .. max ranges do not overlap"
    elif n[2] < d[1]:
        verdict = "faster: the two min .. max ranges do not overlap"
    else:
        verdict = ("faster" if n[0] < d[0] else "slower") + " by the medians, the min .. max ranges overlap"
    print(f"{what}: default {fmt(d)}   native ends {fmt(n)}   ratio {n[0] / d[0]:.3f}   ({verdict})")
    rd, rn = records(step, False), records(step, True)
    assert not any(k.startswith(NEW) for k in rd)
    print(f"    library launches per step: default {sum(v[0] for v in rd.values())}, native ends {sum(v[0] for v in rn.values())}")
    for k in NEW:
        if k in rn:
            c, ms, by = rn[k]
            print(f"    {k:32s} x{c}  {ms:8.3f} ms  {by / 1e6:9.1f} MB algorithmic = {by / ms / 1e9 if ms > 0 else 0.0:6.2f} TB/s")


print(f"# NS-3D training step, the models' two ends in both forms, one MI355X ({torch.cuda.get_device_name(0)}); {steps} alternated steps each, "
      "median (min .. max)")
if section == "one256":
    _, step = build("256")
    for _ in range(5):
        step(form == "native")
    torch.cuda.synchronize()
    print(f"five steps of the 256^2 configuration, {form or 'default'} form")
else:
    for key in CONFIGS:
        if section in ("all", key):
            run(key)
