"""Golden record for the drop-in modules (dropin/) from the genuine reference, on the CPU.

Development machine only (it imports the reference checkout, which never enters this repository and never travels to the GPU box):

    python tools/gen_golden_dropin.py --ref <reference checkout> [--out tests/golden]

Writes data only:
  tests/golden/dropin.json
    signatures   {"<module>.<class>": [[parameter name, default or "<required>"], ...]} of the constructors of the reference's model
                 classes, Adam and LpLoss (tuples as lists)
    loops        the configuration of the three recorded runs: class, constructor arguments, seeds, data shapes, batch counts,
                 learning rate and weight decay - what tests/dropin_loops.py rebuilds the run from
  tests/golden/dropin.npz, per run `<run>.<field>`:
    data_ck      float64 [sum, sum of squares] of the seeded data (tests/dropin_loops.py: make_batches)
    loss0        the genuine LpLoss(size_average=False) of the first training batch before any update
    printed      what the genuine training function prints for its one epoch, times left out: train_darcy.train_model [train_l2, val_l2,
                 test_l2]; ns_train_2d.train_model [train_loss, val_loss, test step loss, test trajectory loss];
                 ns_train_3d.train_model_3d [train_loss, val_loss, test trajectory loss, test step loss]
    after.norm.<param>   float64 l2 norm of every parameter in the weights the run saved after its two optimiser steps
    after.full.<param>   those weights themselves where a parameter has at most 4096 entries
The model configurations are the small ones of the harness goldens (oracle/gen_golden.py: uno9_case, ns2d_case, ns3d_case); initial
weights are not stored, they come from torch.manual_seed(seed) + the constructor's registration order.  train_darcy and ns_train_3d
move their batches with `.cuda()`: Tensor.cuda is the identity while this tool runs them.
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import sys
import tempfile

import numpy as np
import torch

from _reference import import_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dropin_loops  # noqa: E402  (the data recipe lives with the tests that replay it)

LOOPS = {
    "darcy": dict(loop="darcy", module="darcy_flow_uno2d", cls="UNO_9", ctor=[3, 4], ctor_kw={"pad": 5}, model_seed=5, data_seed=105,
                  x_shape=[2, 72, 72, 1], y_shape=[2, 72, 72], train_batches=2, val_batches=1, test_batches=1, T_f=1, lr=1e-3,
                  weight_decay=1e-3),
    "ns2d": dict(loop="ns2d", module="navier_stokes_uno2d", cls="UNO", ctor=[14, 4], ctor_kw={}, model_seed=21, data_seed=121,
                 x_shape=[1, 64, 64, 10], y_shape=[1, 64, 64, 2], train_batches=2, val_batches=1, test_batches=1, T_f=2, lr=1e-3,
                 weight_decay=1e-3),
    "ns3d": dict(loop="ns3d", module="navier_stokes_uno3d", cls="Uno3D_T20", ctor=[6, 2], ctor_kw={"pad": 3}, model_seed=31, data_seed=131,
                 x_shape=[1, 32, 32, 10, 1], y_shape=[1, 32, 32, 20], train_batches=2, val_batches=1, test_batches=1, T_f=20, lr=1e-3,
                 weight_decay=1e-3),
}
SIGNATURES = {"darcy_flow_uno2d": ["UNO_9", "UNO_11"], "navier_stokes_uno2d": ["UNO", "UNO_P", "UNO_S256"],
              "navier_stokes_uno3d": ["Uno3D_T40", "Uno3D_T20", "Uno3D_T10", "Uno3D_T9"], "Adam": ["Adam"], "utilities3": ["LpLoss"]}


def signature_record(cls):
    out = []
    for name, p in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        d = "<required>" if p.default is inspect.Parameter.empty else p.default
        out.append([name, list(d) if isinstance(d, tuple) else d])
    return out


class Recorder:
    """stands in for `print` inside a reference training module: keeps every call's arguments"""

    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kw):
        self.calls.append(args)

    def line(self, first):
        hits = [c for c in self.calls if c and c[0] == first]
        assert len(hits) == 1, (first, self.calls)
        return hits[0]


def printed_values(name, rec):
    if name == "darcy":
        epoch = [c for c in rec.calls if len(c) == 4 and not isinstance(c[2], str)]
        test = [c for c in rec.calls if len(c) == 4 and c[2] == "Test Error"]
        assert len(epoch) == 1 and len(test) == 1, rec.calls
        return [epoch[0][2], epoch[0][3], test[0][3]]
    epoch = rec.line("epochs")
    if name == "ns2d":
        test = rec.line("Test set Evaluation ")
        return [epoch[5], epoch[7], test[2], test[3]]
    test = rec.line("*** Test error: ")
    return [epoch[5], epoch[7], test[1], test[2]]


def run(name, cfg, mods, tmp):
    module, trainer, utilities3 = mods[cfg["module"]], mods["trainer_" + name], mods["utilities3"]
    batches = dropin_loops.make_batches(cfg)
    out = {f"{name}.data_ck": dropin_loops.data_checksum(batches)}
    model = dropin_loops.build_model(cfg, module)
    out[f"{name}.loss0"] = np.array(dropin_loops.first_loss(model, utilities3.LpLoss, batches, cfg, "cpu"))
    rec = Recorder()
    trainer.print = rec
    path = os.path.join(tmp, name + ".pt")
    n = cfg["x_shape"][0]
    counts = [n * cfg["train_batches"], n * cfg["val_batches"], n * cfg["test_batches"]]
    common = dict(T_f=cfg["T_f"], epochs=1, learning_rate=cfg["lr"], weight_decay=cfg["weight_decay"])
    if name == "darcy":
        trainer.train_model(model, batches["train"], batches["val"], batches["test"], *counts, cfg["x_shape"][1], path, **common)
    elif name == "ns2d":
        trainer.train_model(model, batches["train"], batches["val"], batches["test"], *counts, path, device="cpu", **common)
    else:
        trainer.train_model_3d(model, batches["train"], batches["val"], batches["test"], *counts, path, **common)
    out[f"{name}.printed"] = np.array([float(v) for v in printed_values(name, rec)], dtype=np.float64)
    saved = torch.load(path)
    for k, _ in model.named_parameters():
        p = saved[k]
        q = p.to(torch.complex128 if p.is_complex() else torch.float64)
        out[f"{name}.after.norm.{k}"] = np.array(float(torch.linalg.vector_norm(q)))
        if p.numel() <= 4096:
            out[f"{name}.after.full.{k}"] = p.numpy().copy()
    print(name, "loss0", float(out[f"{name}.loss0"]), "printed", out[f"{name}.printed"].tolist())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (development machine only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    names = list(SIGNATURES) + ["train_darcy", "ns_train_2d", "ns_train_3d"]
    mods = dict(zip(names, import_reference(args.ref, *names)))
    for name, key in (("darcy", "train_darcy"), ("ns2d", "ns_train_2d"), ("ns3d", "ns_train_3d")):
        mods["trainer_" + name] = mods[key]
    for m in list(mods.values()) + [sys.modules["integral_operators"]]:
        assert os.path.dirname(os.path.abspath(m.__file__)) == os.path.abspath(args.ref), f"{m.__name__} is not the reference's module"
    sigs = {f"{m}.{c}": signature_record(getattr(mods[m], c)) for m, classes in SIGNATURES.items() for c in classes}
    torch.Tensor.cuda = lambda self, *a, **k: self          # train_darcy / ns_train_3d: `x, y = x.cuda(), y.cuda()`
    z = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, cfg in LOOPS.items():
            z.update(run(name, cfg, mods, tmp))
    with open(os.path.join(args.out, "dropin.json"), "w") as f:
        json.dump({"signatures": sigs, "loops": LOOPS}, f, indent=1, sort_keys=True)
        f.write("\n")
    path = os.path.join(args.out, "dropin.npz")
    np.savez_compressed(path, **z)
    print("dropin.npz", os.path.getsize(path), "dropin.json", os.path.getsize(os.path.join(args.out, "dropin.json")))


if __name__ == "__main__":
    main()
