"""Golden values for the harness models Uno3D_T10 and Uno3D_T9 from the genuine reference (navier_stokes_uno3d.py:412-602, 605-797),
for Uno3D_T20_256 and Uno3D_T10_256 at S = 256 (:993-1181, :1184-1372) and for the NS-3D loop's per-time-step error metric
(ns_train_3d.py:55-62).

Development machine only (it imports the reference checkout, which never enters this repository and never travels to the GPU box):

    python tools/gen_golden_ns3d_models.py --ref <reference checkout> [--out tests/golden]

Writes tests/golden/harness_ns3d_t10.npz and tests/golden/harness_ns3d_t9.npz in the format of tools/gen_golden_ns2d_models.py: per case
`<case>.<field>` with
    ck64.<param>      [sum |p|, ||p||_2] in float64 of every seeded parameter - the weights themselves are NOT stored, they come from
                      torch.manual_seed(seed) + the constructor's registration order
    seed, ctor        the seed and the constructor arguments (in_width, width, pad, pad_both)
    sd_keys, sd_shapes  the ordered state_dict keys and their shapes (rows padded with -1 to five dimensions)
    xx, yy            input (B, S, S, T_in, 1) and target (B, S, S, T_f)
    pred, loss        the prediction (B, S, S, T_f) and the training loss LpLoss(size_average=False) of the whole trajectory (:64)
    gradnorm.<param>  l2 norm of every parameter gradient
    step_err, full_err      the loop's temp_step_loss = sum_t LpLoss(size_average=False)(pred[..., t], yy[..., t]) (:55-62) and the
                            whole-trajectory LpLoss of (pred, yy), in float32 as the reference computes them
    step_err64, full_err64  the same from float64 copies of (pred, yy)
    per_step64        (B, T_f): the float64 per-sample, per-step ratios
and tests/golden/harness_ns3d_256.npz, whose tensors at S = 256 are too large to store: in its cases
    data              (data seed, B, S, T_in, T_f): xx and yy are torch.randn of a CPU torch.Generator().manual_seed(data seed), xx first
    xx_ck64, yy_ck64  [sum |v|, ||v||_2] in float64 of those tensors (the tests verify them before anything else, as they do ck64)
    pred              pred[:, ::8, ::8, :] only;  pred_ck64: [sum |v|, ||v||_2] in float64 of the whole prediction
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from _reference import import_reference

# (file, case, class, (in_width, width, pad, pad_both), model seed, data seed, S, batch, T_in, T_f)
# Uno3D_T9's conv1 keeps 18 modes on the half grid: the reference raises below S = 36, hence S = 48
CASES = [
    ("harness_ns3d_t10.npz", "t10", "Uno3D_T10", (6, 2, 3, 0), 51, 52, 32, 2, 10, 10),
    ("harness_ns3d_t10.npz", "t10both", "Uno3D_T10", (6, 2, 3, 1), 53, 54, 32, 1, 10, 10),
    ("harness_ns3d_t9.npz", "t9", "Uno3D_T9", (6, 2, 3, 0), 55, 56, 48, 2, 6, 9),
    ("harness_ns3d_256.npz", "t20_256", "Uno3D_T20_256", (6, 2, 2, 0), 61, 62, 256, 1, 10, 20),
    ("harness_ns3d_256.npz", "t20_256both", "Uno3D_T20_256", (6, 2, 3, 1), 63, 64, 256, 1, 10, 20),
    ("harness_ns3d_256.npz", "t10_256", "Uno3D_T10_256", (6, 2, 2, 0), 65, 66, 256, 1, 10, 10),
]
SAMPLED_FROM = 256      # cases of at least this size store checksums of xx / yy and a sample of pred
SAMPLE_STRIDE = 8


def _np(t):
    return t.detach().cpu().numpy().copy()


def _ck64(t):
    q = t.detach().double()
    return np.array([float(q.abs().sum()), float(torch.linalg.vector_norm(q))])


def _step_loss(myloss, out, y):
    """ns_train_3d.py:55-62"""
    B, T_f = out.shape[0], out.shape[-1]
    total = 0
    for time in range(T_f):
        k, l = out[..., time], y[..., time]
        total += myloss(k.reshape(B, -1), l.reshape(B, -1))
    return total


def case(n3, LpLoss, name, cls, ctor, seed, data_seed, S, B, T_in, T_f):
    torch.manual_seed(seed)
    model = getattr(n3, cls)(ctor[0], ctor[1], pad=ctor[2], pad_both=bool(ctor[3]))
    out = {f"{name}.seed": np.array(seed), f"{name}.ctor": np.array(ctor)}
    for k, p in model.named_parameters():
        q = p.detach().to(torch.complex128 if p.is_complex() else torch.float64)
        out[f"{name}.ck64.{k}"] = np.array([float(q.abs().sum()), float(torch.linalg.vector_norm(q))])
    sd = model.state_dict()
    out[f"{name}.sd_keys"] = np.array(list(sd.keys()))
    out[f"{name}.sd_shapes"] = np.array([list(v.shape) + [-1] * (5 - v.dim()) for v in sd.values()], dtype=np.int64)
    g = torch.Generator().manual_seed(data_seed)
    xx = torch.randn(B, S, S, T_in, 1, generator=g)
    yy = torch.randn(B, S, S, T_f, generator=g)
    if S >= SAMPLED_FROM:
        out[f"{name}.data"] = np.array([data_seed, B, S, T_in, T_f])
        out[f"{name}.xx_ck64"], out[f"{name}.yy_ck64"] = _ck64(xx), _ck64(yy)
    else:
        out[f"{name}.xx"], out[f"{name}.yy"] = _np(xx), _np(yy)
    myloss = LpLoss(size_average=False)
    pred = model(xx).view(B, S, S, T_f)
    with torch.no_grad():
        step = _step_loss(myloss, pred, yy)
    loss = myloss(pred.view(B, -1), yy.view(B, -1))
    loss.backward()
    out[f"{name}.loss"] = np.array(float(loss.detach()))
    if S >= SAMPLED_FROM:
        out[f"{name}.pred"], out[f"{name}.pred_ck64"] = _np(pred[:, ::SAMPLE_STRIDE, ::SAMPLE_STRIDE, :]), _ck64(pred)
    else:
        out[f"{name}.pred"] = _np(pred)
    for k, p in model.named_parameters():
        out[f"{name}.gradnorm.{k}"] = np.array(float(torch.linalg.vector_norm(p.grad)))
    out[f"{name}.step_err"] = np.array(float(step), dtype=np.float32)
    out[f"{name}.full_err"] = np.array(float(loss.detach()), dtype=np.float32)
    p64, y64 = pred.detach().double(), yy.double()
    out[f"{name}.step_err64"] = np.array(float(_step_loss(myloss, p64, y64)))
    out[f"{name}.full_err64"] = np.array(float(myloss(p64.reshape(B, -1), y64.reshape(B, -1))))
    d = (p64 - y64).reshape(B, -1, T_f)
    out[f"{name}.per_step64"] = _np(torch.linalg.vector_norm(d, dim=1) / torch.linalg.vector_norm(y64.reshape(B, -1, T_f), dim=1))
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (development machine only)")
    ap.add_argument("--out", default=os.path.join(root, "tests", "golden"))
    ap.add_argument("--only", default=None, help="write this file only (the others keep their bytes)")
    args = ap.parse_args()
    n3, utilities3 = import_reference(args.ref, "navier_stokes_uno3d", "utilities3")
    files = {}
    for fname, *row in CASES:
        if args.only and fname != args.only:
            continue
        files.setdefault(fname, {}).update(case(n3, utilities3.LpLoss, *row))
    for fname, z in files.items():
        path = os.path.join(args.out, fname)
        np.savez_compressed(path, **z)
        print(fname, os.path.getsize(path))


if __name__ == "__main__":
    main()
