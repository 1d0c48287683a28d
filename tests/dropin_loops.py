"""What the drop-in tests share (tests/test_dropin_cpu.py, tests/test_hip_dropin_loops.py) and tools/gen_golden_dropin.py reads: the
seeded data of the three recorded training runs, the three loops written out as the reference's scripts write them (train_darcy.py,
ns_train_2d.py, ns_train_3d.py: one epoch - every training batch, then validation, then the test pass), and the comparison with the
golden record (tests/golden/dropin.json for configurations and signatures, tests/golden/dropin.npz for numbers).

Bounds - none is new:
    loss0        the loss of the first batch before any update: 1e-5 relative, the bound of a loss value in every harness golden
                 test (test_harness_cpu.py::test_uno9_forward_loss_grads_match_reference, TOL_PRED of test_harness_ns*.py)
    printed      the values the script prints (training, validation and test figures): every one of them contains passes made AFTER
                 an optimiser step, so they take the bound test_harness_cpu.py::test_three_training_steps_match_reference_adam sets
                 for losses along reference-Adam steps, np.allclose(rtol=2e-4)
    parameters   after the two optimiser steps, as that test bounds them after three: | ||p|| - ||p_ref|| | <= 1e-4 ||p_ref|| + 1e-9 for
                 every parameter, and rel_err < 1e-3 for those stored in full (at most 4096 entries)"""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN, Case, load_cases, rel_err

TOL_LOSS0, RTOL_PRINTED, TOL_PARAM_NORM, TOL_PARAM = 1e-5, 2e-4, 1e-4, 1e-3
LOOPS = ("darcy", "ns2d", "ns3d")


def record():
    with open(os.path.join(GOLDEN, "dropin.json")) as f:
        return json.load(f)


def make_batches(cfg):
    """{"train": [(x, y), ...], "val": [...], "test": [...]} on the host from cfg["data_seed"]: uniform fields for Darcy (the
    coefficient is positive there), normal ones for the two Navier-Stokes runs"""
    g = torch.Generator().manual_seed(int(cfg["data_seed"]))
    draw = torch.rand if cfg["loop"] == "darcy" else torch.randn
    out = {}
    for part in ("train", "val", "test"):
        out[part] = [(draw(*cfg["x_shape"], generator=g), draw(*cfg["y_shape"], generator=g)) for _ in range(int(cfg[part + "_batches"]))]
    return out


def data_checksum(batches):
    """float64 [sum, sum of squares] over every tensor: the test's generator reproduced the recorded run's data"""
    s = q = 0.0
    for part in ("train", "val", "test"):
        for pair in batches[part]:
            for t in pair:
                s += float(t.double().sum())
                q += float((t.double() ** 2).sum())
    return np.array([s, q])


def build_model(cfg, module, block_cls=None):
    """cfg's model from `module` (a drop-in module, or the reference's) under cfg's seed"""
    torch.manual_seed(int(cfg["model_seed"]))
    kw = dict(cfg["ctor_kw"])
    if block_cls is not None:
        kw["block_cls"] = block_cls
    return getattr(module, cfg["cls"])(*cfg["ctor"], **kw)


def _counts(cfg):
    n = int(cfg["x_shape"][0])
    return n * int(cfg["train_batches"]), n * int(cfg["val_batches"]), n * int(cfg["test_batches"])


def _setup(model, Adam, LpLoss, cfg, scheduler_step):
    optimizer = Adam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"], amsgrad=False)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=scheduler_step, gamma=0.5)
    return optimizer, scheduler, LpLoss(size_average=False)


def darcy_loop(model, Adam, LpLoss, batches, cfg, device):
    """train_darcy.py:35-97, one epoch -> [train_l2, val_l2, test_l2]"""
    ntrain, nval, ntest = _counts(cfg)
    s = int(cfg["x_shape"][1])
    optimizer, scheduler, myloss = _setup(model, Adam, LpLoss, cfg, 50)
    model.train()
    train_l2 = 0
    for x, y in batches["train"]:
        x, y = x.to(device), y.to(device)
        batch_size = x.shape[0]
        optimizer.zero_grad()
        out = model(x).reshape(batch_size, s, s)
        loss = myloss(out.view(batch_size, -1), y.view(batch_size, -1))
        loss.backward()
        optimizer.step()
        train_l2 += loss.item()
    scheduler.step()
    model.eval()
    held = []
    with torch.no_grad():
        for part in ("val", "test"):
            l2 = 0.0
            for x, y in batches[part]:
                x, y = x.to(device), y.to(device)
                batch_size = x.shape[0]
                out = model(x).reshape(batch_size, s, s)
                l2 += myloss(out.view(batch_size, -1), y.view(batch_size, -1)).item()
            held.append(l2)
    return [train_l2 / ntrain, held[0] / nval, held[1] / ntest]


def ns2d_loop(model, Adam, LpLoss, batches, cfg, device):
    """ns_train_2d.py:34-168, one epoch -> [train_loss, val_loss, test step loss, test trajectory loss]"""
    ntrain, nval, ntest = _counts(cfg)
    T_f, step = int(cfg["T_f"]), 1
    optimizer, scheduler, myloss = _setup(model, Adam, LpLoss, cfg, 100)

    def rollout(xx, yy):
        loss = 0
        batch_size = yy.shape[0]
        for t in range(0, T_f, step):
            y = yy[..., t:t + step]
            im = model(xx)
            loss += myloss(im.reshape(batch_size, -1), y.reshape(batch_size, -1))
            pred = im if t == 0 else torch.cat((pred, im), -1)
            xx = torch.cat((xx[..., step:], im), dim=-1)
        return loss, pred

    model.train()
    train_l2_step = 0
    for xx, yy in batches["train"]:
        xx, yy = xx.to(device), yy.to(device)
        loss, _ = rollout(xx, yy)
        train_l2_step += loss.item()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
    model.eval()
    val_l2_step = test_l2_step = test_l2 = 0
    with torch.no_grad():
        for xx, yy in batches["val"]:
            val_l2_step += rollout(xx.to(device), yy.to(device))[0].item()
        scheduler.step()
        for xx, yy in batches["test"]:
            xx, yy = xx.to(device), yy.to(device)
            loss, pred = rollout(xx, yy)
            test_l2_step += loss.item()
            test_l2 += myloss(pred.reshape(yy.shape[0], -1), yy.reshape(yy.shape[0], -1)).item()
    per = T_f / step
    return [train_l2_step / ntrain / per, val_l2_step / nval / per, test_l2_step / ntest / per, test_l2 / ntest]


def ns3d_loop(model, Adam, LpLoss, batches, cfg, device):
    """ns_train_3d.py:34-147, one epoch -> [train_loss, val_loss, test trajectory loss, test step loss]"""
    ntrain, nval, ntest = _counts(cfg)
    T_f = int(cfg["T_f"])
    optimizer, scheduler, myloss = _setup(model, Adam, LpLoss, cfg, 50)

    def step_loss(out, y, batch_size):
        total = 0
        for time in range(T_f):
            k, l = out[..., time], y[..., time]
            total += myloss(k.view(batch_size, -1), l.view(batch_size, -1))
        return total

    model.train()
    train_l2_step = 0
    for x, y in batches["train"]:
        x, y = x.to(device), y.to(device)
        batch_size, S = x.shape[0], x.shape[1]
        optimizer.zero_grad()
        out = model(x).view(batch_size, S, S, T_f)
        with torch.no_grad():
            train_l2_step += step_loss(out, y, batch_size).item()
        l2 = myloss(out.view(batch_size, -1), y.view(batch_size, -1))
        l2.backward()
        optimizer.step()
    scheduler.step()
    model.eval()
    val_l2_step = test_l2_step = test_l2 = 0.0
    with torch.no_grad():
        for x, y in batches["val"]:
            x, y = x.to(device), y.to(device)
            batch_size, S = x.shape[0], x.shape[1]
            out = model(x).view(batch_size, S, S, T_f)
            val_l2_step += step_loss(out, y, batch_size).item()
        for x, y in batches["test"]:
            x, y = x.to(device), y.to(device)
            batch_size, S = x.shape[0], x.shape[1]
            out = model(x).view(batch_size, S, S, T_f)
            test_l2 += myloss(out.view(batch_size, -1), y.view(batch_size, -1)).item()
            test_l2_step += step_loss(out, y, batch_size).item()
    return [train_l2_step / (ntrain * T_f), val_l2_step / (nval * T_f), test_l2 / ntest, test_l2_step / (ntest * T_f)]


LOOP_FNS = {"darcy": darcy_loop, "ns2d": ns2d_loop, "ns3d": ns3d_loop}


def first_loss(model, LpLoss, batches, cfg, device):
    """the training loss of the first batch before any update (no gradient is taken)"""
    x, y = (t.to(device) for t in batches["train"][0])
    myloss = LpLoss(size_average=False)
    n = x.shape[0]
    with torch.no_grad():
        if cfg["loop"] == "ns2d":
            return float(myloss(model(x).reshape(n, -1), y[..., 0:1].reshape(n, -1)))
        return float(myloss(model(x).reshape(n, -1), y.reshape(n, -1)))


def run_and_compare(name, modules, device, block_cls=None):
    """Build cfg's model from the drop-in `modules` = {module name: module}, run its loop on `device`, compare with the record."""
    cfg = record()["loops"][name]
    z, _ = load_cases("dropin.npz")
    c = Case(z, name)
    batches = make_batches(cfg)
    assert np.allclose(data_checksum(batches), c.data_ck, rtol=1e-12), "the seeded data differ from the recorded run's"
    model = build_model(cfg, modules[cfg["module"]], block_cls).to(device)
    Adam, LpLoss = modules["Adam"].Adam, modules["utilities3"].LpLoss
    loss0 = first_loss(model, LpLoss, batches, cfg, device)
    printed = LOOP_FNS[name](model, Adam, LpLoss, batches, cfg, device)
    print(f"[dropin {name} on {device}] loss0 {loss0:.8g} (recorded {float(c.loss0):.8g}), printed {printed} (recorded {c.printed.tolist()})")
    assert abs(loss0 - float(c.loss0)) < TOL_LOSS0 * abs(float(c.loss0))
    assert np.allclose(printed, c.printed, rtol=RTOL_PRINTED), (printed, c.printed.tolist())
    params = dict(model.named_parameters())
    norms = c.sub("after.norm")
    assert sorted(norms) == sorted(params)
    worst = 0.0
    for k, ref in norms.items():
        got = float(torch.linalg.vector_norm(params[k].detach().to(torch.complex128 if params[k].is_complex() else torch.float64)))
        assert abs(got - float(ref)) <= TOL_PARAM_NORM * float(ref) + 1e-9, (k, got, float(ref))
    for k, v in c.sub("after.full").items():
        e = rel_err(params[k].detach().cpu().numpy(), v)
        worst = max(worst, float(e))
        assert e < TOL_PARAM, (k, e)
    print(f"[dropin {name} on {device}] largest relative error of a stored parameter after two steps {worst:.2e}")
