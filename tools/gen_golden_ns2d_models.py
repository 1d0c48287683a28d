"""Golden values for the harness models UNO_P and UNO_S256 from the genuine reference (navier_stokes_uno2d.py:24-138, 246-337).

Development machine only (it imports the reference checkout, which never enters this repository and never travels to the GPU box):

    python tools/gen_golden_ns2d_models.py --ref <reference checkout> [--out tests/golden]

Writes tests/golden/harness_ns2d_p.npz and tests/golden/harness_ns2d_s256.npz in the format of harness_ns.npz
(oracle/gen_golden.py, ns2d_case): per case `<case>.<field>` with
    ck64.<param>      [sum |p|, ||p||_2] in float64 of every seeded parameter - the weights themselves are NOT stored, they come from
                      torch.manual_seed(seed) + the constructor's registration order
    seed, ctor        the seed and the constructor arguments (in_width, width, pad)
    sd_keys, sd_shapes  the ordered state_dict keys and their shapes (rows padded with -1 to four dimensions)
    xx, yy            input window (B, S, S, T_in) and targets (B, S, S, steps)
    pred, loss        the roll-out's predictions (B, S, S, steps) and its summed relative-L2 loss (ns_train_2d.py:46-62)
    gradnorm.<param>  l2 norm of every parameter gradient
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from _reference import import_reference

# (file, case, class, (in_width, width, pad), model seed, data seed, S, T_in, steps)
CASES = [
    ("harness_ns2d_p.npz", "p64", "UNO_P", (14, 4, 0), 41, 42, 64, 10, 2),
    ("harness_ns2d_p.npz", "p56pad", "UNO_P", (14, 4, 4), 43, 44, 56, 10, 1),
    ("harness_ns2d_s256.npz", "s256", "UNO_S256", (5, 4, 0), 45, 46, 256, 1, 1),
]


def _np(t):
    return t.detach().cpu().numpy().copy()


def case(n2, LpLoss, name, cls, ctor, seed, data_seed, S, T_in, steps):
    torch.manual_seed(seed)
    model = getattr(n2, cls)(ctor[0], ctor[1], pad=ctor[2])
    out = {f"{name}.seed": np.array(seed), f"{name}.ctor": np.array(ctor)}
    for k, p in model.named_parameters():
        q = p.detach().to(torch.complex128 if p.is_complex() else torch.float64)
        out[f"{name}.ck64.{k}"] = np.array([float(q.abs().sum()), float(torch.linalg.vector_norm(q))])
    sd = model.state_dict()
    out[f"{name}.sd_keys"] = np.array(list(sd.keys()))
    out[f"{name}.sd_shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    g = torch.Generator().manual_seed(data_seed)
    xx = torch.randn(1, S, S, T_in, generator=g)
    yy = torch.randn(1, S, S, steps, generator=g)
    out[f"{name}.xx"], out[f"{name}.yy"] = _np(xx), _np(yy)
    myloss = LpLoss(size_average=False)
    loss, x, preds = 0, xx, []
    for t in range(steps):
        im = model(x)
        preds.append(im)
        loss = loss + myloss(im.reshape(1, -1), yy[..., t:t + 1].reshape(1, -1))
        x = torch.cat((x[..., 1:], im), dim=-1)
    loss.backward()
    out[f"{name}.loss"] = np.array(float(loss.detach()))
    out[f"{name}.pred"] = _np(torch.cat(preds, -1))
    for k, p in model.named_parameters():
        out[f"{name}.gradnorm.{k}"] = np.array(float(torch.linalg.vector_norm(p.grad)))
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (development machine only)")
    ap.add_argument("--out", default=os.path.join(root, "tests", "golden"))
    args = ap.parse_args()
    n2, utilities3 = import_reference(args.ref, "navier_stokes_uno2d", "utilities3")
    files = {}
    for fname, *row in CASES:
        files.setdefault(fname, {}).update(case(n2, utilities3.LpLoss, *row))
    for fname, z in files.items():
        path = os.path.join(args.out, fname)
        np.savez_compressed(path, **z)
        print(fname, os.path.getsize(path))


if __name__ == "__main__":
    main()
