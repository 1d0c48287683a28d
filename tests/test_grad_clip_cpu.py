"""ComplexAdam(max_grad_norm=, skip_nonfinite=) on host parameters (uno_amd/harness/optim.py: the stock-op twin of K26 and the guarded
K10) and the resumable epoch runners (uno_amd/harness/fit.py: checkpoint=, resume=, --clip-norm, --save-every, --resume), on the CPU.

Bounds: float64 parameters against torch.nn.utils.clip_grad_norm_ + a plain step at rtol 1e-12 (both sides evaluate the same formula
in double; they differ in the order of the norm's sum); float32 at rel_err < 1e-6, the tolerance of tests/test_hip_adam.py.  Skips and
resumed runs are compared bit for bit.  The spectral layers have no CPU path in the product, so the models get the oracle's operator
blocks through `block_cls`, as tests/test_fit_cpu.py builds them."""
import dataclasses
import json
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from uno_amd.harness import DeviceDataset, fit_darcy, fit_ns2d, fit_ns3d
from uno_amd.harness import models as harness_models
from uno_amd.harness.optim import ComplexAdam


def params(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    return [torch.nn.Parameter(torch.randn(7, 5, dtype=dtype, generator=g)), torch.nn.Parameter(torch.randn(6, 3, dtype=cd, generator=g))]


def grads(ps, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(p.shape, dtype=p.dtype, generator=g) for p in ps]


def real(t):
    t = t.detach()
    return (torch.view_as_real(t) if t.is_complex() else t).numpy()


def state_of(opt, ps):
    return [(int(opt.state[p]["step"]), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_host_path_equals_clip_grad_norm_then_step(dtype):
    """4 steps; the gradient scale alternates so that steps 1 and 3 clip and steps 2 and 4 do not"""
    pa, pb = params(dtype), params(dtype)
    oa = ComplexAdam(pa, lr=3e-3, weight_decay=1e-2, max_grad_norm=2.0)
    ob = ComplexAdam(pb, lr=3e-3, weight_decay=1e-2)
    norms = []
    for t in range(4):
        gs = grads(pa, 10 + t, scale=(3.0, 0.05)[t % 2])
        for p, q, g in zip(pa, pb, gs):
            p.grad, q.grad = g.clone(), g.clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(pb, 2.0)))
        ob.step()
        oa.step()
        assert oa.last_grad_norm.dtype == torch.float64
        assert math.isclose(float(oa.last_grad_norm), norms[-1], rel_tol=1e-12 if dtype == torch.float64 else 1e-6)
    assert [n > 2.0 for n in norms] == [True, False, True, False]
    for p, q in zip(pa, pb):
        if dtype == torch.float64:
            np.testing.assert_allclose(real(p), real(q), rtol=1e-12, atol=0)
            np.testing.assert_allclose(oa.state[p]["exp_avg_sq"].numpy(), ob.state[q]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        else:
            assert rel_err(real(p), real(q)) < 1e-6
            assert rel_err(oa.state[p]["exp_avg_sq"].numpy(), ob.state[q]["exp_avg_sq"].numpy()) < 1e-6
    stats = oa.clip_stats()
    assert (stats["steps"], stats["clipped"], stats["skipped"], stats["nonfinite"]) == (4, 2, 0, 0)
    assert math.isclose(stats["grad_norm"], sum(norms) / 4, rel_tol=1e-6) and math.isclose(stats["grad_norm_max"], max(norms), rel_tol=1e-6)
    assert oa.clip_stats()["steps"] == 0            # read and reset


def test_a_norm_below_the_threshold_changes_nothing():
    pa, pb = params(torch.float32), params(torch.float32)
    oa = ComplexAdam(pa, lr=3e-3, weight_decay=1e-2, max_grad_norm=1e3)
    ob = ComplexAdam(pb, lr=3e-3, weight_decay=1e-2)
    for t in range(4):
        for p, q, g in zip(pa, pb, grads(pa, 20 + t)):
            p.grad, q.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
        for p, q in zip(pa, pb):
            assert torch.equal(p.detach(), q.detach())
            assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])
    assert oa.clip_stats()["clipped"] == 0


def test_plain_optimiser_is_untouched_by_the_new_keywords():
    opt = ComplexAdam(params(torch.float32), lr=1e-3)
    assert not opt.guarded and "max_grad_norm" not in opt.param_groups[0] and opt.last_grad_norm is None
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        opt.clip_stats()
    assert ComplexAdam(params(torch.float32), max_grad_norm=1.0).skip_nonfinite
    assert not ComplexAdam(params(torch.float32), max_grad_norm=1.0, skip_nonfinite=False).skip_nonfinite
    assert ComplexAdam(params(torch.float32), skip_nonfinite=True).guarded
    with pytest.raises(ValueError, match="max_grad_norm"):
        ComplexAdam(params(torch.float32), max_grad_norm=0.0)


@pytest.mark.parametrize("bad", ["inf", "nan_imag"])
def test_a_nonfinite_step_is_skipped_bit_for_bit(bad):
    pa, pb = params(torch.float32), params(torch.float32)           # pb: the twin that never sees the bad step
    oa = ComplexAdam(pa, lr=3e-3, weight_decay=1e-2, max_grad_norm=2.0)
    ob = ComplexAdam(pb, lr=3e-3, weight_decay=1e-2, max_grad_norm=2.0)
    for p, q, g in zip(pa, pb, grads(pa, 30, 3.0)):
        p.grad, q.grad = g.clone(), g.clone()
    oa.step()
    ob.step()
    before = [p.detach().clone() for p in pa], state_of(oa, pa)
    gs = grads(pa, 31)
    if bad == "inf":
        gs[0].view(-1)[-1] = math.inf
    else:
        gs[1].view(-1)[4] = complex(1.0, math.nan)
    for p, g in zip(pa, gs):
        p.grad = g
    oa.step()
    after = [p.detach().clone() for p in pa], state_of(oa, pa)
    for x, y in zip(before[0], after[0]):
        assert torch.equal(x, y)
    for (s0, m0, v0), (s1, m1, v1) in zip(before[1], after[1]):
        assert s0 == s1 == 1 and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert not math.isfinite(float(oa.last_grad_norm))
    stats = oa.clip_stats()
    assert (stats["steps"], stats["skipped"], stats["nonfinite"], stats["clipped"]) == (2, 1, 1, 1)
    for p, q, g in zip(pa, pb, grads(pa, 32)):
        p.grad, q.grad = g.clone(), g.clone()
    oa.step()
    ob.step()
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"]) and oa.state[p]["step"] == ob.state[q]["step"] == 2


def test_skipping_off_takes_the_step():
    pa = params(torch.float32)
    oa = ComplexAdam(pa, lr=3e-3, max_grad_norm=2.0, skip_nonfinite=False)
    gs = grads(pa, 40)
    gs[0].view(-1)[0] = math.inf
    for p, g in zip(pa, gs):
        p.grad = g
    oa.step()
    stats = oa.clip_stats()
    assert (stats["steps"], stats["skipped"], stats["nonfinite"]) == (1, 0, 1) and oa.state[pa[0]]["step"] == 1


def test_inputs_the_norm_cannot_take_raise_and_name_the_parameter():
    ps = params(torch.float32)
    ps.append(torch.nn.Parameter(torch.randn(4).half()))          # (the mixed-precision trainer's half-precision tensors fall here)
    opt = ComplexAdam(ps, max_grad_norm=1.0)
    for p in ps:
        p.grad = torch.zeros_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match=r"parameter 2 of group 0 \(shape \(4,\), torch.float16, cpu\) with a torch.float16 gradient"):
        opt.step()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, ps)) and opt.clip_stats()["steps"] == 0


def test_mixed_host_and_device_parameters_raise(monkeypatch):
    """no GPU needed: the check reads Tensor.is_cuda only, so one host parameter reports itself as a device one"""
    ps = params(torch.float32)
    opt = ComplexAdam(ps, max_grad_norm=1.0)
    for p in ps:
        p.grad = torch.zeros_like(p)
    odd = ps[1]
    real_is_cuda = torch.Tensor.is_cuda.__get__
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True if self is odd else real_is_cuda(self)))
    with pytest.raises(RuntimeError, match=r"host and device parameters in one optimiser - parameter 1 of group 0 \(shape \(6, 3\), torch.complex64"):
        opt.step()


# ------------------------------------------------------------------------------------------------------------------------------ resume
# The grids are those of the recorded tiny runs (tests/golden/dropin.json: 72, 64, 32), not 16 x 16: the model classes keep the
# reference's fixed mode counts (UNO_9 asks for 18 modes of its first level), which a 16 x 16 grid does not have.
GRID = {"darcy": 72, "ns2d": 64, "ns3d": 32}
CLIP = {"darcy": 8.5, "ns2d": 2.0, "ns3d": 0.1}         # between the smallest and the largest gradient norm of each 4-epoch run
RUNNERS = {"darcy": fit_darcy, "ns2d": fit_ns2d, "ns3d": fit_ns3d}


def tiny(name, seed=7):
    """a width-4 model on the oracle's blocks, and 8 / 4 / 4 samples"""
    S = GRID[name]
    from oracle import spectral_oracle as so
    g = torch.Generator().manual_seed(100 + seed)
    torch.manual_seed(seed)
    if name == "darcy":
        model = harness_models.UNO_9(3, 4, pad=5, block_cls=so.OracleOperatorBlock2d)
        shapes, kw, draw = ((S, S, 1), (S, S)), {}, torch.rand
    elif name == "ns2d":
        model = harness_models.UNO(14, 4, block_cls=so.OracleOperatorBlock2d)
        shapes, kw, draw = ((S, S, 10), (S, S, 2)), {"T_f": 2}, torch.randn
    else:
        model = harness_models.Uno3D_T10(6, 4, pad=2, block_cls=so.OracleOperatorBlock3d)
        shapes, kw, draw = ((S, S, 10, 1), (S, S, 10)), {"T_f": 10}, torch.randn
    parts = [DeviceDataset(draw(n, *shapes[0], generator=g), draw(n, *shapes[1], generator=g), "cpu") for n in (8, 4, 4)]
    return model, parts, kw


def go(name, epochs, **kw):
    model, parts, extra = tiny(name)
    rec = RUNNERS[name](model, *parts, batch_size=4, epochs=epochs, lr=1e-2, weight_decay=1e-3, scheduler_step=1, max_grad_norm=CLIP[name],
                        generator=torch.Generator().manual_seed(3), log=lambda *a: None, **extra, **kw)
    return model, rec


def same_records(a, b):
    strip = lambda r: [dataclasses.replace(e, seconds=0.0) for e in r.epochs]
    assert strip(a) == strip(b)
    assert (a.best_epoch, a.best_val, a.test) == (b.best_epoch, b.best_val, b.test)
    assert list(a.state_dict) == list(b.state_dict)
    for k in a.state_dict:
        assert torch.equal(a.state_dict[k], b.state_dict[k]), k


def same_optimiser_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert list(a["state"]) == list(b["state"])
    for k in a["state"]:
        for field in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][k][field], b["state"][k][field]), (k, field)
        assert int(a["state"][k]["step"]) == int(b["state"][k]["step"])


@pytest.mark.parametrize("name", list(RUNNERS))
def test_two_plus_two_epochs_equal_four(name, tmp_path):
    path = str(tmp_path / "run.ckpt")
    straight_model, straight = go(name, 4, checkpoint=(str(tmp_path / "straight.ckpt"), 4))
    go(name, 2, checkpoint=(path, 2))
    resumed_model, resumed = go(name, 4, checkpoint=(path, 2), resume=path)
    assert [e.epoch for e in resumed.epochs] == [0, 1, 2, 3]
    assert all(e.grad_norm is not None and e.grad_norm_max >= e.grad_norm > 0 for e in resumed.epochs)
    assert 0 < sum(e.clipped for e in resumed.epochs) < 8       # 8 steps: some clipped, some not
    same_records(straight, resumed)
    for (k, a), (_, b) in zip(straight_model.state_dict().items(), resumed_model.state_dict().items()):
        assert torch.equal(a, b), k
    # the optimiser state after epoch 4, as both runs' last checkpoints hold it
    a, b = torch.load(str(tmp_path / "straight.ckpt")), torch.load(path)
    assert a["epoch"] == b["epoch"] == 4
    same_optimiser_state(a["optimizer"], b["optimizer"])
    assert a["scheduler"] == b["scheduler"]
    with pytest.raises(ValueError, match="resume: setting lr is 0.02 here and 0.01 in"):
        model, parts, extra = tiny(name)
        RUNNERS[name](model, *parts, batch_size=4, epochs=4, lr=2e-2, weight_decay=1e-3, scheduler_step=1, max_grad_norm=CLIP[name],
                      generator=torch.Generator().manual_seed(3), log=lambda *a: None, resume=path, **extra)


def test_epoch_record_keeps_its_old_constructions():
    from uno_amd.harness.fit import EpochRecord
    e = EpochRecord(0, 1e-3, 0.5, 0.1, None)
    assert (e.grad_norm, e.grad_norm_max, e.clipped, e.skipped) == (None, None, 0, 0)


def test_command_line_record_and_resume(tmp_path, monkeypatch, capsys):
    """--clip-norm / --save-every / --resume through main() on the CPU (the model on the oracle's blocks): the record carries the new
    keys, harness.predict.load_model reads it, 1 + 1 epochs give the 2-epoch run's weights, and a changed --lr is refused"""
    pytest.importorskip("scipy.io")
    from oracle import spectral_oracle as so
    from uno_amd.harness import fit as fit_module
    from uno_amd.harness import generate_darcy_dataset
    from uno_amd.harness.predict import load_model
    monkeypatch.setattr(fit_module, "_model", lambda a, cls: getattr(harness_models, a.model or cls)(a.in_width, a.width, pad=a.pad,
                                                                                                     block_cls=so.OracleOperatorBlock2d))
    data = str(tmp_path / "darcy.mat")
    generate_darcy_dataset(data, n_samples=7, s=GRID["darcy"], bsize=4, seed=11, device="cpu")

    def argv(out, epochs, *more):
        return ["darcy", "--data", data, "--ntrain", "4", "--nval", "2", "--ntest", "1", "--width", "4", "--pad", "5", "--batch-size", "2",
                "--epochs", str(epochs), "--out", out, "--seed", "5", "--device", "cpu", "--clip-norm", "0.5", *more]

    straight, split = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    rec2 = fit_module.main(argv(straight, 2))
    fit_module.main(argv(split, 1, "--save-every", "1"))
    rec11 = fit_module.main(argv(split, 2, "--save-every", "1", "--resume"))
    capsys.readouterr()
    assert [(e.train, e.val, e.grad_norm, e.clipped) for e in rec11.epochs] == [(e.train, e.val, e.grad_norm, e.clipped) for e in rec2.epochs]
    assert rec11.test == rec2.test
    wa, wb = torch.load(straight), torch.load(split)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k
    with open(split + ".json") as f:
        record = json.load(f)
    assert record["clip_norm"] == 0.5 and record["skip_nonfinite"] is True and record["skipped_steps"] == 0
    model = load_model(split, block_cls=so.OracleOperatorBlock2d)
    for k, v in model.state_dict().items():
        assert torch.equal(v, wb[k]), k
    old = {k: v for k, v in record.items() if k not in ("clip_norm", "skip_nonfinite", "skipped_steps")}
    assert load_model(split, record=old, block_cls=so.OracleOperatorBlock2d) is not None          # a record from before the keys
    with pytest.raises(SystemExit, match="--resume: setting lr is 0.002 here and 0.001 in"):
        fit_module.main(argv(split, 3, "--resume", "--lr", "2e-3"))
    with pytest.raises(SystemExit):
        fit_module.main(argv(str(tmp_path / "none.pt"), 1, "--resume"))


def test_argument_errors_of_the_new_entry_points_without_a_gpu():
    """uno_grad_norm_ws_bytes / uno_grad_norm / uno_adam_step_multi_guarded validate on the host before any launch"""
    import ctypes as C
    from uno_amd import _native
    lib = _native.lib()
    n = (C.c_longlong * 3)(1, 1024, 513)
    cplx = (C.c_int * 3)(0, 0, 1)
    assert lib.uno_grad_norm_ws_bytes(3, n, cplx) == 8 * (1 + 1 + 2)          # one double per 1024 floats; 513 complex = 1026 floats
    assert lib.uno_grad_norm_ws_bytes(0, None, None) == 0
    bad = (C.c_longlong * 1)(-1)
    assert lib.uno_grad_norm_ws_bytes(1, bad, cplx) < 0 and b"tensor 0" in lib.uno_last_error()
    buf = C.create_string_buffer(128)
    p = C.cast(buf, C.c_void_p)
    g = (C.c_void_p * 3)(p, p, p)
    assert lib.uno_grad_norm(3, g, n, cplx, None, 1, p, 32, p, None) < 0 and b"null" in lib.uno_last_error()
    assert lib.uno_grad_norm(3, g, n, cplx, p, 1, p, 24, p, None) < 0 and b"workspace of 24 bytes, 32 needed" in lib.uno_last_error()
    g[1] = None
    assert lib.uno_grad_norm(3, g, n, cplx, p, 1, p, 32, p, None) < 0 and b"tensor 1" in lib.uno_last_error()
    g[1] = p
    dbl = [C.c_double(v) for v in (1e-3, 0.9, 0.999, 1e-8, 0.0)]
    assert lib.uno_adam_step_multi_guarded(3, g, g, g, g, n, cplx, *dbl, p, p, None, None, 1, None) < 0 and b"bad arguments" in lib.uno_last_error()
    dbl[1] = C.c_double(1.0)
    assert lib.uno_adam_step_multi_guarded(3, g, g, g, g, n, cplx, *dbl, p, p, None, p, 1, None) < 0 and b"bad betas" in lib.uno_last_error()
