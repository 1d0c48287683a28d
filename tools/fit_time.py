"""Time of an epoch (training batches + validation pass) in two forms, per workload, in one process on the same device-resident batches:

  (a) the reference's loop as tests/dropin_loops.py writes it out, on the drop-in modules (dropin/: the harness models, ComplexAdam,
      LpLoss on K20) - `loss.item()` per batch, T_f loss calls per NS-3D batch for the step metric, a new optimiser per call;
  (b) the epoch runner (harness.fit_darcy / fit_ns2d / fit_ns3d), eager and with graph=True.

Workloads: Darcy at the headline shape (UNO_9(3, 64, pad=5), 421^2, batch 16); NS-3D at configuration C4's shape (Uno3D_T20(6, w, pad=3),
64 x 64 x 20, batch 8) at widths 8 and 32; NS-2D at C3's (UNO(14, 32), 64^2, batch 32, T_f = 40).  A few batches per epoch.
Then the NS-3D loss alone (forward + backward at the model's output, step metric included) and the NS-3D training step, stock against
ns3d_loss(native=True) (developer tool; bench.py is the contract).
usage: python tools/fit_time.py [epochs] [all | darcy | ns3d | ns2d | loss]

(a) runs `epochs` (at least 5) epochs after one warm-up epoch, then (b) eager and (b) graph run one call of the runner each and give the
time of every epoch that validates (both Navier-Stokes loops validate on even epochs only; the first, which holds warm-up and
capture, is dropped), then (a) runs again: the distance of its two medians is the run-to-run spread to read the others against.
Wall time per epoch, synchronised at its end.  Needs an MI355X: there is no CPU path."""
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[0:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

import dropin_loops
from uno_amd.harness import (ComplexAdam, Uno3D_T20, fit_darcy, fit_ns2d, fit_ns3d, lp_loss_rel_sum, ns3d_loss, step_errors, step_losses)

if not torch.cuda.is_available():
    sys.exit("fit_time.py: no HIP device")
section = "all"
if sys.argv[1:] and sys.argv[-1] in ("all", "darcy", "ns3d", "ns2d", "loss"):
    section = sys.argv.pop()
epochs = max(5, int(sys.argv[1])) if sys.argv[1:] else 5
dev = torch.device("cuda:0")


def dropin():
    mods = {}
    for name in ("darcy_flow_uno2d", "navier_stokes_uno2d", "navier_stokes_uno3d", "Adam", "utilities3"):
        spec = importlib.util.spec_from_file_location("_dropin_" + name, os.path.join(ROOT, "dropin", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods


MODS = dropin()
WORKLOADS = {
    "darcy": dict(loop="darcy", module="darcy_flow_uno2d", cls="UNO_9", ctor=[3, 64], ctor_kw={"pad": 5}, x_shape=[16, 421, 421, 1],
                  y_shape=[16, 421, 421], T_f=1, train_batches=6, val_batches=1),
    "ns3d w8": dict(loop="ns3d", module="navier_stokes_uno3d", cls="Uno3D_T20", ctor=[6, 8], ctor_kw={"pad": 3}, x_shape=[8, 64, 64, 10, 1],
                    y_shape=[8, 64, 64, 20], T_f=20, train_batches=6, val_batches=1),
    "ns3d w32": dict(loop="ns3d", module="navier_stokes_uno3d", cls="Uno3D_T20", ctor=[6, 32], ctor_kw={"pad": 3}, x_shape=[8, 64, 64, 10, 1],
                     y_shape=[8, 64, 64, 20], T_f=20, train_batches=6, val_batches=1),
    "ns2d": dict(loop="ns2d", module="navier_stokes_uno2d", cls="UNO", ctor=[14, 32], ctor_kw={}, x_shape=[32, 64, 64, 10],
                 y_shape=[32, 64, 64, 40], T_f=40, train_batches=2, val_batches=1),
}
for w in WORKLOADS.values():
    w.update(data_seed=1, model_seed=0, lr=1e-3, weight_decay=1e-3, test_batches=1)
FIT = {"darcy": fit_darcy, "ns2d": fit_ns2d, "ns3d": fit_ns3d}


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def fmt(s, unit="s", scale=1.0):
    return f"{s[0] * scale:9.4f} {unit} ({s[1] * scale:.4f} .. {s[2] * scale:.4f})"


def reference_epochs(cfg, batches, n):
    """(a): n timed calls of the written-out loop (training + validation; the test list is empty) after one warm-up call"""
    model = dropin_loops.build_model(cfg, MODS[cfg["module"]]).to(dev)
    loop = dropin_loops.LOOP_FNS[cfg["loop"]]
    held = {"train": batches["train"], "val": batches["val"], "test": []}
    times = []
    for i in range(n + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop(model, MODS["Adam"].Adam, MODS["utilities3"].LpLoss, held, cfg, dev)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times[1:]


def runner_epochs(cfg, batches, n, graph):
    """(b): one call of the runner; the seconds of every validating epoch but the first"""
    model = dropin_loops.build_model(cfg, MODS[cfg["module"]]).to(dev)
    every = 1 if cfg["loop"] == "darcy" else 2
    kw = {} if cfg["loop"] == "darcy" else {"T_f": cfg["T_f"]}
    rec = FIT[cfg["loop"]](model, batches["train"], batches["val"], batches["val"], epochs=every * n + 1, lr=cfg["lr"],
                           weight_decay=cfg["weight_decay"], graph=graph, log=lambda *a: None, **kw)
    return [e.seconds for e in rec.epochs if e.val is not None][1:]


def epoch_section(name):
    cfg = WORKLOADS[name]
    batches = {k: [(x.to(dev), y.to(dev)) for x, y in v] for k, v in dropin_loops.make_batches(cfg).items()}
    a1 = stats(reference_epochs(cfg, batches, epochs))
    eager = stats(runner_epochs(cfg, batches, epochs, False))
    graph = stats(runner_epochs(cfg, batches, epochs, True))
    a2 = stats(reference_epochs(cfg, batches, epochs))
    spread = abs(a1[0] - a2[0])
    print(f"{name}: {cfg['cls']}({', '.join(map(str, cfg['ctor']))}), x {tuple(cfg['x_shape'])}, {cfg['train_batches']} training + "
          f"{cfg['val_batches']} validation batches per epoch, {epochs} epochs each, median (min .. max)")
    print(f"  (a) reference loop, first run  {fmt(a1)}")
    print(f"  (a) reference loop, second run {fmt(a2)}   run-to-run spread of the median {spread:.4f} s")
    for label, s in (("(b) runner, eager", eager), ("(b) runner, graph=True", graph)):
        print(f"  {label:<30} {fmt(s)}   = {s[0] / min(a1[0], a2[0]):.3f} of (a)")
    model = dropin_loops.build_model(cfg, MODS[cfg["module"]]).to(dev)
    alloc = []
    for _ in range(epochs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MODS["Adam"].Adam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"]).init_state()
        torch.cuda.synchronize()
        alloc.append(time.perf_counter() - t0)
    del model
    print(f"  (a) builds its optimiser inside every timed call, as tests/dropin_loops.py writes the loop: each of its epochs allocates and "
          f"zero-fills the Adam moments, (b) does so in its dropped first epoch only.  That alone takes {fmt(stats(alloc[1:]))}: "
          f"subtract it from (a) before reading the ratios")
    sys.stdout.flush()
    del batches
    torch.cuda.empty_cache()


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def ab(forms, n, warm=3):
    for _ in range(warm):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(n):
        for k, fn in forms.items():
            t[k].append(one(fn))
    return {k: stats(v) for k, v in t.items()}


def loss_section():
    calls = max(50, 10 * epochs)
    B, S, T_f = 8, 64, 20
    g = torch.Generator().manual_seed(1)
    y = torch.randn(B, S, S, T_f, generator=g).to(dev)
    out = (y + 0.1 * torch.randn(B, S, S, T_f, generator=g).to(dev)).requires_grad_(True)

    def stock():
        out.grad = None
        loss = lp_loss_rel_sum(out.reshape(B, -1), y.reshape(B, -1))
        with torch.no_grad():
            step_errors(out.detach(), y).step_sum
        loss.backward()

    def native():
        out.grad = None
        step_losses(out, y).full_sum.backward()

    r = ab({"stock": stock, "native": native}, calls)
    print(f"NS-3D loss + step metric alone at the output ({B}, {S}, {S}, {T_f}), forward + backward, {calls} alternated calls, median (min .. max)")
    print(f"  stock loss + K17 metric        {fmt(r['stock'], 'ms', 1e3)}")
    print(f"  step_losses (K17 / K17-B)      {fmt(r['native'], 'ms', 1e3)}   = {r['native'][0] / r['stock'][0]:.3f} of stock")
    for width in (8, 32):
        torch.manual_seed(0)
        m = Uno3D_T20(6, width, pad=3).to(dev)
        opt = ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-3)
        x = torch.randn(B, S, S, 10, 1, device=dev)

        def step(flag):
            opt.zero_grad(set_to_none=True)
            loss, _ = ns3d_loss(m, x, y, with_step_error=True, native=flag)
            loss.backward()
            opt.step()
        r = ab({"stock": lambda: step(False), "native": lambda: step(True)}, max(20, 4 * epochs))
        print(f"  Uno3D_T20(6, {width}, pad=3) eager training step with step error: default {fmt(r['stock'], 'ms', 1e3)}   native=True "
              f"{fmt(r['native'], 'ms', 1e3)}   = {r['native'][0] / r['stock'][0]:.3f}")
        del m, opt
        torch.cuda.empty_cache()
    sys.stdout.flush()


print(f"# {torch.cuda.get_device_name(0)}, float32, seeded synthetic data resident on the device")
for name in WORKLOADS:
    if section in ("all", name.split()[0]):
        epoch_section(name)
if section in ("all", "loss"):
    loss_section()
