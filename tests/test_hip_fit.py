"""The epoch runners (uno_amd/harness/fit.py) on the MI355X, on the recorded tiny configurations of tests/golden/dropin.json: the
native loss paths against the recorded genuine CPU runs (tests/golden/dropin.npz) at the bounds of tests/test_hip_dropin_loops.py
(tests/dropin_loops.py: RTOL_PRINTED, TOL_PARAM_NORM, TOL_PARAM), graph replay against eager, the read-backs of an epoch, and the command
line end to end.  Reads tests/golden/ only.

Measured on the MI355X (printed per loop): the runners' figures differ from the recorded ones by at most 1.0e-7 (darcy), 2.4e-7 (ns2d),
2.3e-7 (ns3d), relative."""
import math

import numpy as np
import pytest
import torch

import dropin_loops
from conftest import Case, load_cases, rel_err
from dropin_loops import RTOL_PRINTED, TOL_PARAM, TOL_PARAM_NORM

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def build(name, on_device=True):
    from uno_amd.harness import models
    cfg = dropin_loops.record()["loops"][name]
    model = dropin_loops.build_model(cfg, models).to(dev())
    batches = dropin_loops.make_batches(cfg)
    if on_device:
        batches = {k: [(x.to(dev()), y.to(dev())) for x, y in v] for k, v in batches.items()}
    return cfg, model, batches


def fit(name, model, batches, cfg, **kw):
    from uno_amd.harness import fit_darcy, fit_ns2d, fit_ns3d
    if name != "darcy":
        kw["T_f"] = int(cfg["T_f"])
    kw.setdefault("log", lambda *a: None)
    return {"darcy": fit_darcy, "ns2d": fit_ns2d, "ns3d": fit_ns3d}[name](
        model, batches["train"], batches["val"], batches["test"], lr=cfg["lr"], weight_decay=cfg["weight_decay"], **kw)


@pytest.mark.parametrize("name", dropin_loops.LOOPS)
def test_one_epoch_on_the_native_paths_matches_the_recorded_reference_run(name):
    cfg, model, batches = build(name, on_device=False)         # host batches: the runner moves them, as the reference's loop does
    c = Case(load_cases("dropin.npz")[0], name)
    rec = fit(name, model, batches, cfg, epochs=1, native=True)
    got = [rec.epochs[0].train, rec.epochs[0].val, *rec.test]
    print(f"[fit {name} on the device] {got} (recorded {c.printed.tolist()})")
    assert np.allclose(got, c.printed, rtol=RTOL_PRINTED), (got, c.printed.tolist())
    params = dict(model.named_parameters())
    norms = c.sub("after.norm")
    assert sorted(norms) == sorted(params)
    for k, ref in norms.items():
        n = float(torch.linalg.vector_norm(params[k].detach().to(torch.complex128 if params[k].is_complex() else torch.float64)))
        assert abs(n - float(ref)) <= TOL_PARAM_NORM * float(ref) + 1e-9, (k, n, float(ref))
    for k, v in c.sub("after.full").items():
        assert rel_err(params[k].detach().cpu().numpy(), v) < TOL_PARAM, k


@pytest.mark.parametrize("name", ["ns2d", "ns3d"])
def test_one_epoch_of_the_navier_stokes_runners_from_a_graph_matches_the_recorded_run(name):
    """graph=True: the training step replayed with its optimiser update (NS-3D: the step error read from the graph's own tensor), NS-2D's
    validation and test roll-outs replayed from a GraphedRollout - the recorded figures and parameters at the bounds of the eager test"""
    c = Case(load_cases("dropin.npz")[0], name)
    cfg, model, batches = build(name)
    rec = fit(name, model, batches, cfg, epochs=1, graph=True)
    got = [rec.epochs[0].train, rec.epochs[0].val, *rec.test]
    print(f"[fit {name} graph=True] {got} (recorded {c.printed.tolist()})")
    assert np.allclose(got, c.printed, rtol=RTOL_PRINTED), (got, c.printed.tolist())
    params = dict(model.named_parameters())
    for k, ref in c.sub("after.norm").items():
        n = float(torch.linalg.vector_norm(params[k].detach().to(torch.complex128 if params[k].is_complex() else torch.float64)))
        assert abs(n - float(ref)) <= TOL_PARAM_NORM * float(ref) + 1e-9, (k, n, float(ref))
    for k, v in c.sub("after.full").items():
        assert rel_err(params[k].detach().cpu().numpy(), v) < TOL_PARAM, k


def test_two_epochs_of_fit_darcy_from_a_graph_equal_eager_bit_for_bit():
    cfg, eager_model, batches = build("darcy")
    eager = fit("darcy", eager_model, batches, cfg, epochs=2, scheduler_step=1)
    cfg, graph_model, batches = build("darcy")
    graphed = fit("darcy", graph_model, batches, cfg, epochs=2, scheduler_step=1, graph=True)
    assert [(e.train, e.val, e.lr) for e in graphed.epochs] == [(e.train, e.val, e.lr) for e in eager.epochs]
    assert graphed.test == eager.test and graphed.best_epoch == eager.best_epoch
    for (k, a), (_, b) in zip(eager_model.state_dict().items(), graph_model.state_dict().items()):
        assert torch.equal(a, b), k


def test_a_short_last_batch_runs_eagerly_beside_the_graph():
    """three training batches of 2, 2 and 1 samples: the graph replays the first two, the third runs eagerly; the figures equal the
    eager runner's bit for bit"""
    def run(graph):
        cfg, model, batches = build("darcy")
        x, y = batches["val"][0]
        batches["train"].append((x[:1].clone(), y[:1].clone()))
        return fit("darcy", model, batches, cfg, epochs=2, graph=graph), model
    (eager, me), (graphed, mg) = run(False), run(True)
    assert [(e.train, e.val) for e in graphed.epochs] == [(e.train, e.val) for e in eager.epochs] and graphed.test == eager.test
    for (k, a), (_, b) in zip(me.state_dict().items(), mg.state_dict().items()):
        assert torch.equal(a, b), k


class Watched:
    """a list of batches that checks, whenever the runner comes back for the next batch, that no device value was read since the
    pass over it began"""

    def __init__(self, batches, reads):
        self.batches, self.reads, self.passes = batches, reads, 0

    def __iter__(self):
        start = len(self.reads)
        for b in self.batches:
            yield b
            assert len(self.reads) == start, f"device values were read inside the batch loop: {self.reads[start:]}"
        self.passes += 1


@pytest.mark.parametrize("name", dropin_loops.LOOPS)
def test_no_device_value_is_read_inside_a_batch_loop(name, monkeypatch):
    """Tensor.item / tolist / cpu are counted: none between the first and the last batch of a pass, and at most one per phase and epoch
    (two epochs: training twice, validation twice - NS validates in epoch 0 only - and one test pass)"""
    cfg, model, batches = build(name)
    reads = []
    for attr in ("item", "tolist", "cpu"):
        real = getattr(torch.Tensor, attr)
        monkeypatch.setattr(torch.Tensor, attr, lambda self, *a, _real=real, _attr=attr, **kw: (reads.append(_attr), _real(self, *a, **kw))[1])
    x, y = batches["train"][0]
    batches["train"].append((x.clone(), y.clone()))             # three batches per pass
    watched = {k: Watched(v, reads) for k, v in batches.items()}
    rec = fit(name, model, watched, cfg, epochs=2)
    phases = {"darcy": 2 + 2 + 1, "ns2d": 2 + 1 + 1, "ns3d": 2 + 1 + 1}[name]
    assert watched["train"].passes == 2 and watched["test"].passes == 1 and watched["val"].passes == (2 if name == "darcy" else 1)
    assert 1 <= len(reads) <= phases, reads
    assert all(math.isfinite(e.train) for e in rec.epochs)


def test_command_line_end_to_end(tmp_path, capsys):
    pytest.importorskip("scipy.io")
    from uno_amd.harness import LpLoss, UNO_9, generate_darcy_dataset, load_darcy
    from uno_amd.harness import fit as fit_module
    cfg = dropin_loops.record()["loops"]["darcy"]
    s = int(cfg["x_shape"][1])
    data, out = str(tmp_path / "darcy.mat"), str(tmp_path / "best.pt")
    generate_darcy_dataset(data, n_samples=7, s=s, bsize=4, seed=11)
    rec = fit_module.main(["darcy", "--data", data, "--ntrain", "4", "--nval", "2", "--ntest", "1", "--width", str(cfg["ctor"][1]),
                           "--pad", str(cfg["ctor_kw"]["pad"]), "--batch-size", "2", "--epochs", "1", "--out", out, "--seed", "5"])
    printed = capsys.readouterr().out
    assert len(rec.epochs) == 1 and all(math.isfinite(v) for v in (rec.epochs[0].train, rec.epochs[0].val, *rec.test))
    assert "Test Error" in printed and repr(rec.test[0]) in printed
    model = UNO_9(*cfg["ctor"], **cfg["ctor_kw"]).to(dev())
    model.load_state_dict(torch.load(out, map_location=dev()), strict=True)
    model.eval()
    x, y, _, _ = load_darcy(data, 1, 7, 1)
    (_, _), (_, _), (xt, yt) = fit_module._split(x, y, 4, 2, 1, 5)
    with torch.no_grad():
        again = float(LpLoss(size_average=False)(model(xt.to(dev())).reshape(1, -1), yt.to(dev()).reshape(1, -1))) / 1
    # the same kernels on the same sample and weights: float32 rounding of one ratio at the most
    assert abs(again - rec.test[0]) <= 1e-6 * abs(rec.test[0]), (again, rec.test[0])
