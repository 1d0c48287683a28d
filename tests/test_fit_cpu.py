"""The epoch runners (uno_amd/harness/fit.py), the loaders and the device dataset (uno_amd/harness/data.py) on the CPU.

One epoch of each runner on the seeded batches of the recorded drop-in runs (tests/dropin_loops.py, tests/golden/dropin.json /
dropin.npz: the genuine reference loops on the genuine modules) must give the recorded printed figures and parameter norms at that
file's bounds - RTOL_PRINTED, TOL_PARAM_NORM, TOL_PARAM; no new tolerance.  The spectral layers have no CPU path in the product, so the
models get the oracle's operator blocks through `block_cls`, as tests/test_dropin_cpu.py builds them; the runners themselves import
nothing from oracle/.  Schedules, the even-epoch validation, the best-epoch weights, the loaders and the dataset are checked on the
same tiny configurations."""
import numpy as np
import pytest
import torch

import dropin_loops
from conftest import Case, load_cases, rel_err
from dropin_loops import RTOL_PRINTED, TOL_PARAM, TOL_PARAM_NORM

from uno_amd.harness import DeviceDataset, fit_darcy, fit_ns2d, fit_ns3d, load_darcy, load_ns
from uno_amd.harness import models as harness_models

FIT = {"darcy": fit_darcy, "ns2d": fit_ns2d, "ns3d": fit_ns3d}
DEFAULT_STEP = {"darcy": 50, "ns2d": 100, "ns3d": 50}


def build(name):
    from oracle import spectral_oracle as so
    cfg = dropin_loops.record()["loops"][name]
    block = so.OracleOperatorBlock3d if name == "ns3d" else so.OracleOperatorBlock2d
    return cfg, dropin_loops.build_model(cfg, harness_models, block), dropin_loops.make_batches(cfg)


def run(name, model, batches, cfg, lines=None, **kw):
    if name != "darcy":
        kw["T_f"] = int(cfg["T_f"])
    kw.setdefault("scheduler_step", DEFAULT_STEP[name])
    log = (lambda *a: lines.append(a)) if lines is not None else (lambda *a: None)
    return FIT[name](model, batches["train"], batches["val"], batches["test"], lr=cfg["lr"], weight_decay=cfg["weight_decay"], log=log, **kw)


def printed(name, rec):
    """the runner's figures in the order tests/dropin_loops.py returns the loop's"""
    e = rec.epochs[0]
    return [e.train, e.val, *rec.test]


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("name", dropin_loops.LOOPS)
def test_one_epoch_matches_the_recorded_reference_run(name, native):
    cfg, model, batches = build(name)
    c = Case(load_cases("dropin.npz")[0], name)
    assert np.allclose(dropin_loops.data_checksum(batches), c.data_ck, rtol=1e-12)
    rec = run(name, model, batches, cfg, epochs=1, native=native)
    got = printed(name, rec)
    print(f"[fit {name} native={native}] {got} (recorded {c.printed.tolist()})")
    assert np.allclose(got, c.printed, rtol=RTOL_PRINTED), (got, c.printed.tolist())
    assert rec.best_epoch == 0 and rec.best_val == rec.epochs[0].val
    params = dict(model.named_parameters())
    norms = c.sub("after.norm")
    assert sorted(norms) == sorted(params)
    for k, ref in norms.items():
        got_n = float(torch.linalg.vector_norm(params[k].detach().to(torch.complex128 if params[k].is_complex() else torch.float64)))
        assert abs(got_n - float(ref)) <= TOL_PARAM_NORM * float(ref) + 1e-9, (k, got_n, float(ref))
    for k, v in c.sub("after.full").items():
        assert rel_err(params[k].detach().numpy(), v) < TOL_PARAM, k


@pytest.mark.parametrize("name", dropin_loops.LOOPS)
def test_three_epochs_schedule_validation_and_best_weights(name, tmp_path):
    """scheduler_step = 2, gamma 0.5, three epochs: Darcy and NS-3D step the scheduler after every epoch's training batches (lr, lr,
    lr / 2); NS-2D after a validation pass, which only even epochs have, so its second step comes after epoch 2 (lr, lr, lr).  Both
    Navier-Stokes loops validate on even epochs only.  The weights kept are those the model had after the best validation epoch, in
    memory and in the file alike, and the test figures are theirs."""
    cfg, model, batches = build(name)
    snapshots, lines = {}, []

    def log(*a):
        lines.append(a)
        if a and a[0] in ("..Saving Model..", "model saved"):
            snapshots[len(snapshots)] = {k: v.detach().clone() for k, v in model.state_dict().items()}

    kw = {} if name == "darcy" else {"T_f": int(cfg["T_f"])}
    rec = FIT[name](model, batches["train"], batches["val"], batches["test"], epochs=3, lr=cfg["lr"], weight_decay=cfg["weight_decay"],
                    scheduler_step=2, log=log, **kw)
    lr = cfg["lr"]
    assert [e.lr for e in rec.epochs] == ([lr, lr, lr] if name == "ns2d" else [lr, lr, lr / 2])
    assert [e.val is not None for e in rec.epochs] == ([True, True, True] if name == "darcy" else [True, False, True])
    vals = [(e.val, e.epoch) for e in rec.epochs if e.val is not None]
    assert (rec.best_val, rec.best_epoch) == min(vals)
    assert len(snapshots) >= 1
    best = snapshots[len(snapshots) - 1]               # the last save is the best epoch's
    assert list(best) == list(rec.state_dict) == list(model.state_dict())
    for k, v in best.items():
        assert torch.equal(v, rec.state_dict[k]) and torch.equal(v, model.state_dict()[k]), k
    # the same run saving to a path: the file holds the same weights, and the test figures are equal
    cfg, model2, batches = build(name)
    path = str(tmp_path / "best.pt")
    rec2 = FIT[name](model2, batches["train"], batches["val"], batches["test"], epochs=3, lr=cfg["lr"], weight_decay=cfg["weight_decay"],
                     scheduler_step=2, weight_path=path, log=lambda *a: None, **kw)
    assert rec2.state_dict is None and rec2.test == rec.test and rec2.best_epoch == rec.best_epoch
    saved = torch.load(path)
    for k, v in best.items():
        assert torch.equal(v, saved[k]), k


def test_darcy_loader_round_trip(tmp_path):
    pytest.importorskip("scipy.io")
    from uno_amd.harness import generate_darcy_dataset
    path = str(tmp_path / "darcy.mat")
    coeff, sol = generate_darcy_dataset(path, n_samples=5, s=17, bsize=2, seed=3, device="cpu")
    for r, s in ((1, 17), (2, 9), (3, 6), (5, 4)):
        x_train, y_train, x_test, y_test = load_darcy(path, r, 3, 2)
        assert tuple(x_train.shape) == (3, s, s, 1) and tuple(y_train.shape) == (3, s, s)
        assert tuple(x_test.shape) == (2, s, s, 1) and tuple(y_test.shape) == (2, s, s)
        assert x_train.dtype == y_test.dtype == torch.float32
        assert torch.equal(x_train[..., 0], torch.from_numpy(coeff[:3, ::r, ::r])) and torch.equal(y_train, torch.from_numpy(sol[:3, ::r, ::r]))
        assert torch.equal(x_test[..., 0], torch.from_numpy(coeff[-2:, ::r, ::r])) and torch.equal(y_test, torch.from_numpy(sol[-2:, ::r, ::r]))
    with pytest.raises(ValueError, match="within the 5 samples"):
        load_darcy(path, 1, 6, 1)


def test_ns_loader_round_trip(tmp_path):
    pytest.importorskip("scipy.io")
    from uno_amd.harness import MatReader, generate_ns_dataset
    path = str(tmp_path / "ns.mat")
    assert generate_ns_dataset(path, n_samples=6, s=16, record_steps=5, bsize=2, T=0.05, delta_t=1e-2, seed=4, device="cpu") == 3
    reader = MatReader(path)
    u = [reader.read_field(f"u{j}") for j in range(3)]
    assert tuple(u[0].shape) == (2, 16, 16, 5)
    # the split is by whole generation batches: 4 <= train -> two batches train, the third test; the resize is the identity at size 16
    ta, tu, sa, su = load_ns(path, 4, 2, sample_num=6, batch=2, T_in=3, T=2, size=16)
    assert torch.equal(ta, torch.cat((u[0][..., :3], u[1][..., :3]))) and torch.equal(tu, torch.cat((u[0][..., 3:5], u[1][..., 3:5])))
    assert torch.equal(sa, u[2][..., :3]) and torch.equal(su, u[2][..., 3:5])
    # train = 3 holds one whole batch only (the second would make 4 > 3)
    ta, tu, sa, su = load_ns(path, 3, 3, sample_num=6, batch=2, T_in=3, T=2, size=16)
    assert ta.shape[0] == 2 and sa.shape[0] == 4 and torch.equal(sa[:2], u[1][..., :3])
    # a smaller grid: bilinear with align_corners=True keeps the four corners
    ta, tu, _, _ = load_ns(path, 6, 0, sample_num=6, batch=2, T_in=3, T=2, size=8)
    assert tuple(ta.shape) == (6, 8, 8, 3) and tuple(tu.shape) == (6, 8, 8, 2)
    full = torch.cat(u)
    for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert torch.allclose(ta[:, i, j], full[:, i, j, :3], rtol=0, atol=1e-6)


def test_device_dataset_batches():
    x = torch.arange(11, dtype=torch.float32).reshape(11, 1).repeat(1, 3)
    y = torch.arange(11, dtype=torch.float32) * 10
    ds = DeviceDataset(x, y, "cpu")
    assert len(ds) == 11
    g = torch.Generator().manual_seed(0)
    orders = []
    for _ in range(2):
        got = list(ds.batches(4, generator=g))
        assert [b[0].shape[0] for b in got] == [4, 4, 3]                # the short last batch is kept
        xs, ys = torch.cat([b[0] for b in got]), torch.cat([b[1] for b in got])
        assert torch.equal(ys, xs[:, 0] * 10)                           # x and y stay paired
        assert sorted(xs[:, 0].tolist()) == list(range(11))             # every sample once
        orders.append(xs[:, 0].tolist())
    assert orders[0] != orders[1] and orders[0] != sorted(orders[0])    # a new permutation per pass
    plain = list(ds.batches(4, shuffle=False))
    assert torch.equal(torch.cat([b[0] for b in plain]), x) and torch.equal(torch.cat([b[1] for b in plain]), y)
    with pytest.raises(ValueError):
        DeviceDataset(x, y[:5])


def test_runner_takes_a_device_dataset():
    """the same one epoch from DeviceDatasets in file order (shuffle off through batch order: a pre-batched list and a dataset cut into
    the same batches give the same figures bit for bit)"""
    cfg, model, batches = build("darcy")
    rec_list = run("darcy", model, batches, cfg, epochs=1)
    cfg, model, batches = build("darcy")
    n = cfg["x_shape"][0]
    val = DeviceDataset(torch.cat([b[0] for b in batches["val"]]), torch.cat([b[1] for b in batches["val"]]))
    test = DeviceDataset(torch.cat([b[0] for b in batches["test"]]), torch.cat([b[1] for b in batches["test"]]))
    rec_ds = fit_darcy(model, batches["train"], val, test, batch_size=n, epochs=1, lr=cfg["lr"], weight_decay=cfg["weight_decay"],
                       log=lambda *a: None)
    assert printed("darcy", rec_ds) == printed("darcy", rec_list)
    with pytest.raises(ValueError, match="batch_size"):
        fit_darcy(model, batches["train"], val, test, epochs=1, log=lambda *a: None)
