"""The three training loops of the reference's scripts, written out in tests/dropin_loops.py, on the MI355X with the drop-in classes
(dropin/: the harness models on the native layers, ComplexAdam on K10, LpLoss on K20), two optimiser steps each, against the recorded
genuine CPU runs (tests/golden/dropin.json, dropin.npz) at the bounds of the CPU test (tests/dropin_loops.py).  Reads tests/golden/ only.

The drop-in files are loaded by path under private names: a module called `Adam` or `integral_operators` left in sys.modules would be
what every later test of this process imports under that name.

Measured on the MI355X (printed per loop): the first batch's loss is 1e-7 (darcy), 7.0e-7 (ns2d), 1e-7 (ns3d) from the
recorded one, relative, at the eight digits printed; the printed figures differ by at most 1.0e-7 / 2.4e-7 / 2.3e-7 relative; the stored parameters after two steps by at most
1.1e-7 / 1.3e-8 / 4.9e-6 (conftest.rel_err)."""
import importlib.util
import os

import pytest
import torch

import dropin_loops
from conftest import ROOT

pytestmark = pytest.mark.gpu
NAMES = ("darcy_flow_uno2d", "navier_stokes_uno2d", "navier_stokes_uno3d", "Adam", "utilities3")


@pytest.fixture(scope="module")
def dropin():
    mods = {}
    for name in NAMES:
        spec = importlib.util.spec_from_file_location("_dropin_" + name, os.path.join(ROOT, "dropin", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods


@pytest.mark.parametrize("name", dropin_loops.LOOPS)
def test_written_out_loop_on_the_device_matches_the_recorded_reference_run(dropin, name, monkeypatch):
    from uno_amd import _native
    calls = {"forward": 0, "backward": 0}
    for key in calls:
        real = getattr(_native, "rel_l2_" + key)
        monkeypatch.setattr(_native, "rel_l2_" + key, lambda *a, _real=real, _key=key: (calls.__setitem__(_key, calls[_key] + 1), _real(*a))[1])
    assert torch.cuda.is_available()
    dropin_loops.run_and_compare(name, dropin, torch.device("cuda:0"))
    # the loss ran on K20: first_loss + every training, validation and test evaluation forward, one backward per training step
    cfg = dropin_loops.record()["loops"][name]
    # (two training batches, one validation batch, one test batch; the NS loops evaluate one loss per time step, ns_train_2d's test pass
    # and ns_train_3d's training and test passes the whole-trajectory loss as well)
    T_f = cfg["T_f"]
    assert calls["forward"] == 1 + {"darcy": 4, "ns2d": 4 * T_f + 1, "ns3d": 2 * (T_f + 1) + T_f + (T_f + 1)}[name], calls
    assert calls["backward"] == 2 * {"darcy": 1, "ns2d": T_f, "ns3d": 1}[name], calls
