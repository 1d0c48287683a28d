"""The layer plan of the nine Navier-Stokes U-NO models, recorded from the genuine reference (navier_stokes_uno2d.py,
navier_stokes_uno3d.py): which operator blocks each constructor builds and on which grids each forward pass calls them.

Development machine only (it imports the reference checkout, which never enters this repository and never travels to the GPU box):

    python tools/gen_golden_model_census.py --ref <reference checkout> [--out tests/golden]

The reference modules take their blocks from `from integral_operators import *`, so replacing the module globals `OperatorBlock_2D` /
`OperatorBlock_3D` with a recording stand-in before a model is constructed is enough: no reference block is built or run.

Writes tests/golden/model_census.json and, for the two 3-D models for 256 x 256 simulations (classes of uno_amd.harness.models),
tests/golden/model_census_256.json (data only): {"<class>-S<S>-pad<pad>[-both]": case} with
    cls, args, kwargs, input   what tests/test_model_census_cpu.py / tests/test_model_census_256_cpu.py need to build our class and its zeros input
    ctor     per block in construction order: the positional arguments (in, out, default grid, modes), then Normalize, Non_Lin
    calls    per block call in order: [the input's shape[1:] (channels first, so the skip concatenations are pinned), the output grid]
    out      the output's shape
    raises   instead of calls / out: the class name of the exception the reference raised
Whole numbers are stored as integers (2 * factor * width arrives as 6.0 with factor = 3/4)."""
from __future__ import annotations

import argparse
import json
import os

import torch
import torch.nn as nn

from _reference import import_reference

S3D, PADS3D = (32, 48, 50, 64), (0, 2, 3)
S2D, PADS2D = (56, 64, 100, 256), (0, 4)
# class -> (in_width, width, input steps)
MODELS3D = {"Uno3D_T20": (6, 2, 10), "Uno3D_T10": (6, 2, 10), "Uno3D_T9": (6, 2, 6), "Uno3D_T40": (6, 2, 10)}
MODELS2D = {"UNO": (14, 4, 10), "UNO_P": (14, 4, 10), "UNO_S256": (5, 4, 1)}
# the 3-D models for 256 x 256 simulations (their grids are D/4 ... D/32: the sizes they are for, and half of that)
S3D_256 = (256, 128)
MODELS3D_256 = {"Uno3D_T20_256": (6, 2, 10), "Uno3D_T10_256": (6, 2, 10)}


class Recorder(nn.Module):
    """Stands in for OperatorBlock_2D / OperatorBlock_3D: records every constructor call and every forward call, returns zeros."""
    ctor, calls = [], []

    def __init__(self, *args, Normalize=False, Non_Lin=True):
        super().__init__()
        self.out_codim = int(args[1])
        self.ctor.append([*args, Normalize, Non_Lin])

    def forward(self, x, *dims):
        self.calls.append([list(x.shape[1:]), list(dims)])
        return x.new_zeros(x.shape[0], self.out_codim, *dims)


def plain(v):
    if isinstance(v, (list, tuple)):
        return [plain(e) for e in v]
    return int(v) if isinstance(v, float) and v == int(v) else v


def record(cls, args, kwargs, input_shape):
    Recorder.ctor.clear()
    Recorder.calls.clear()
    case = {"cls": cls.__name__, "args": list(args), "kwargs": kwargs, "input": list(input_shape)}
    try:
        model = cls(*args, **kwargs)
        with torch.no_grad():
            out = model(torch.zeros(*input_shape))
        case.update(ctor=plain(Recorder.ctor), calls=plain(Recorder.calls), out=list(out.shape))
    except Exception as e:
        case.update(ctor=plain(Recorder.ctor), raises=type(e).__name__)
    return case


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (development machine only)")
    ap.add_argument("--out", default=os.path.join(root, "tests", "golden"))
    args = ap.parse_args()
    n2, n3 = import_reference(args.ref, "navier_stokes_uno2d", "navier_stokes_uno3d")
    n2.OperatorBlock_2D = n3.OperatorBlock_3D = Recorder
    cases = {}
    for name, (in_width, width, T_in) in MODELS3D.items():
        for S in S3D:
            for pad in PADS3D:
                for both in (False, True):
                    key = f"{name}-S{S}-pad{pad}" + ("-both" if both else "")
                    cases[key] = record(getattr(n3, name), (in_width, width), {"pad": pad, "pad_both": both}, (1, S, S, T_in, 1))
    for name, (in_width, width, T_in) in MODELS2D.items():
        for S in S2D:
            for pad in PADS2D:
                cases[f"{name}-S{S}-pad{pad}"] = record(getattr(n2, name), (in_width, width), {"pad": pad}, (1, S, S, T_in))
    cases_256 = {}
    for name, (in_width, width, T_in) in MODELS3D_256.items():
        for S in S3D_256:
            for pad in PADS3D:
                for both in (False, True):
                    key = f"{name}-S{S}-pad{pad}" + ("-both" if both else "")
                    cases_256[key] = record(getattr(n3, name), (in_width, width), {"pad": pad, "pad_both": both}, (1, S, S, T_in, 1))
    for fname, group in (("model_census.json", cases), ("model_census_256.json", cases_256)):
        path = os.path.join(args.out, fname)
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in group.items()) + "\n}\n")
        print(path, len(group), "cases,", sum("raises" in c for c in group.values()), "raise,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
