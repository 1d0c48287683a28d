"""Time and launch count of the NS-2D TRAINING step (reference ns_train_2d.py:46-68: roll-out loss, one backward, Adam update) at
configuration C3 - UNO(14, 32), 64^2, batch 32 - for T_f = 40 and T_f = 10, stock against native on the same initial weights and inputs:
  stock          harness.ns2d_rollout_loss (the default: one `cat` per step for the window, LpLoss per step), eager
  native         ns2d_rollout_loss(native=True): the window-free roll-out (K19 / K19-B, uno_amd/csrc/rollout_train.hip), eager
  stock graph    the stock step replayed from one HIP graph (harness.GraphedStep, ComplexAdam(capturable=True))
  native graph   the native step replayed from one HIP graph
(developer tool; bench.py is the contract).
usage: python tools/rollout_train_time.py [calls]

One process, the forms alternated call by call; every form warmed up first; median and min .. max of `calls` (at least 20) timed steps,
device events around each step with one synchronisation at its end - the time covers the host's enqueueing where that is the longer of
the two.  `stock graph again` times the stock replay a second time: the distance between the two is the run-to-run spread the
native / stock difference is read against.
Launches: the library's own launches of one eager step through uno_profile_begin / uno_profile_end (count, summed device time and
algorithmic bytes; the roll-out kernels listed by name), and all device kernels of one eager step,
torch's included, from torch.profiler where that is available.  Needs an MI355X: there is no CPU path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from uno_amd import _native
from uno_amd.harness import UNO, ComplexAdam, GraphedStep, ns2d_rollout_loss

if not torch.cuda.is_available():
    sys.exit("rollout_train_time.py: no HIP device")
calls = max(20, int(sys.argv[1])) if sys.argv[1:] else 20
dev = torch.device("cuda:0")
B, S, T_IN, WIDTH = 32, 64, 10, 32


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def ab(forms, n, warm=3):
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


def make(capturable):
    torch.manual_seed(0)
    m = UNO(T_IN + 4, WIDTH).to(dev)
    return m, ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=capturable)


def eager_step(model, opt, xx, yy, T_f, native):
    opt.zero_grad(set_to_none=True)
    loss = ns2d_rollout_loss(model, xx, yy, T_f, native=native)
    loss.backward()
    opt.step()
    return loss.detach()


def library_launches(fn):
    """-> (count, ms, MB, {kernel: (count, ms)}) of the library's launches of one call"""
    _native.profile_begin(200000)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        rows = _native.profile_end()
    by = {}
    for name, ms, nbytes in rows:
        c, t = by.get(name, (0, 0.0))
        by[name] = (c + 1, t + ms)
    return len(rows), sum(r[1] for r in rows), sum(r[2] for r in rows) / 1e6, by


def device_kernels(fn):
    """all device kernels of one call, torch's included (None where the profiler gives no device events)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and not any(s in e.name for s in ("Memcpy", "Memset")))
        return n or None
    except Exception as exc:            # (a profiler that does not come up is no reason to lose the timings)
        print(f"  (torch.profiler unavailable: {type(exc).__name__})")
        return None


ROLLOUT_KERNELS = ("rollout_lift_kernel", "rollout_lift_bwd_kernel", "rollout_loss_seed_kernel", "rollout_advance_kernel",
                   "rel_l2_steps_finish_kernel")

print(f"# NS-2D training step, UNO({T_IN + 4}, {WIDTH}), {S}^2, batch {B}, float32, synthetic data, one MI355X "
      f"({torch.cuda.get_device_name(0)}); {calls} alternated steps each, median (min .. max)")
counts = []
for T_f in (40, 10):
    g = torch.Generator().manual_seed(T_f)
    xx, yy = torch.randn(B, S, S, T_IN, generator=g).to(dev), torch.randn(B, S, S, T_f, generator=g).to(dev)
    ms, os_ = make(False)
    mn, on = make(False)
    l_stock = float(ns2d_rollout_loss(ms, xx, yy, T_f).detach())
    l_native = float(ns2d_rollout_loss(mn, xx, yy, T_f, native=True).detach())
    mgs, ogs = make(True)
    mgn, ogn = make(True)
    gs = GraphedStep(mgs, ogs, lambda a, b: ns2d_rollout_loss(mgs, a, b, T_f), (xx, yy))
    gn = GraphedStep(mgn, ogn, lambda a, b: ns2d_rollout_loss(mgn, a, b, T_f, native=True), (xx, yy))
    forms = {"stock": lambda: eager_step(ms, os_, xx, yy, T_f, False), "native": lambda: eager_step(mn, on, xx, yy, T_f, True),
             "stock graph": lambda: gs.step(xx, yy), "native graph": lambda: gn.step(xx, yy), "stock graph again": lambda: gs.step(xx, yy)}
    res = ab(forms, calls)
    print(f"T_f = {T_f}   (loss of the first step: stock {l_stock:.6f}, native {l_native:.6f}, distance {abs(l_native - l_stock) / abs(l_stock):.1e})")
    for k, v in res.items():
        base = res["stock graph"] if "graph" in k else res["stock"]
        print(f"  {k:18s} {fmt(v)}   {v[0] / base[0]:.3f} of {'stock graph' if 'graph' in k else 'stock'}")
    print(f"  spread between the two stock-graph columns {abs(res['stock graph'][0] - res['stock graph again'][0]) / res['stock graph'][0]:.2%} of the median")
    for name, model, opt, native in (("stock", ms, os_, False), ("native", mn, on, True)):
        n, t, mb, by = library_launches(lambda: eager_step(model, opt, xx, yy, T_f, native))
        print(f"  {name:7s} library launches per step {n:6d}, {t:8.3f} ms summed, {mb:9.1f} MB algorithmic")
        for kname, (c, kt) in sorted(by.items()):
            short = kname.replace("uno::", "")
            if any(short.startswith(r) for r in ROLLOUT_KERNELS):
                print(f"      {short:40s} {c:5d} x, {kt * 1e3 / c:7.1f} us each")
        counts.append((T_f, name, model, opt, native))
    del gs, gn
    torch.cuda.empty_cache()

print("all device kernels of one eager step, torch's included (torch.profiler):")
for T_f, name, model, opt, native in counts:
    g = torch.Generator().manual_seed(T_f)
    xx, yy = torch.randn(B, S, S, T_IN, generator=g).to(dev), torch.randn(B, S, S, T_f, generator=g).to(dev)
    n = device_kernels(lambda: eager_step(model, opt, xx, yy, T_f, native))
    print(f"  T_f = {T_f:2d} {name:7s} {n if n is not None else 'n/a'}")
    if n is None:
        break
