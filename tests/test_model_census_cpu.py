"""The layer plan of the seven Navier-Stokes harness models as a whole - which operator blocks each constructor builds (channels,
default grid, modes, Normalize / Non_Lin) and on which input shapes and output grids each forward pass calls them - against the plan
recorded from the genuine reference (tests/golden/model_census.json; tools/gen_golden_model_census.py): 3-D at S = 32, 48, 50, 64,
pad 0 / 2 / 3, padded on one side and on both; 2-D at S = 56, 64, 100, 256, pad 0 / 4.  The grid arithmetic is full of float
expressions whose rounding matters (int(3 * d1 / 4), int(d3 * 1.2), int(8 * d3 / 6)): every one of them is pinned here."""
import json
import os

import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
import uno_amd.harness as harness

with open(os.path.join(GOLDEN, "model_census.json")) as f:
    CENSUS = json.load(f)
# the Darcy model (the headline path) has parity tests of its own
EXEMPT = {"UNO_9"}


class RecordingBlock(nn.Module):
    """Stands in for OperatorBlock_2D / OperatorBlock_3D: records the constructor's positional arguments + (Normalize, Non_Lin) and,
    per call, [the input's shape[1:], the output grid]; returns zeros of the output shape."""
    ctor, calls = [], []

    def __init__(self, *args, Normalize=False, Non_Lin=True):
        super().__init__()
        self.out_codim = int(args[1])
        self.ctor.append([*args, Normalize, Non_Lin])

    def forward(self, x, *dims):
        self.calls.append([list(x.shape[1:]), list(dims)])
        return x.new_zeros(x.shape[0], self.out_codim, *dims)


def record(cls, *args, **kwargs):
    """cls(*args, **kwargs, block_cls=RecordingBlock): the model, with RecordingBlock.ctor holding its rows and .calls emptied"""
    RecordingBlock.ctor.clear()
    RecordingBlock.calls.clear()
    return cls(*args, **kwargs, block_cls=RecordingBlock)


@pytest.mark.parametrize("key", list(CENSUS))
def test_layer_plan_equals_the_reference(key):
    c = CENSUS[key]
    model = record(getattr(harness, c["cls"]), *c["args"], **c["kwargs"])
    assert RecordingBlock.ctor == c["ctor"]                 # (6.0 == 6: the channel counts are floats where the factor is one)
    x = torch.zeros(*c["input"])
    if "raises" in c:
        with pytest.raises(Exception) as e:
            model(x)
        assert type(e.value).__name__ == c["raises"]
        return
    with torch.no_grad():
        out = model(x)
    assert RecordingBlock.calls == c["calls"]
    assert list(out.shape) == c["out"]


def test_every_exported_ns_model_has_census_cases():
    models = {n for n in dir(harness) if n.startswith(("UNO", "Uno3D_")) and isinstance(getattr(harness, n), type)} - EXEMPT
    assert models and models == {c["cls"] for c in CENSUS.values()}
