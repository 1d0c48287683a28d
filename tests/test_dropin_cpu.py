"""The drop-in modules (dropin/) on the CPU: with that directory first on the path, the names the reference's training scripts import -
the model classes, `Adam`, `LpLoss`, `MatReader` - resolve to this project's classes, take the reference's constructor arguments and
train as the reference does.  The reference's side of every comparison is recorded data (tests/golden/dropin.json, dropin.npz,
written by tools/gen_golden_dropin.py from the genuine modules); bounds and loops are those of tests/dropin_loops.py - no new tolerance.

Every check runs in a fresh interpreter (this file, run as a script, is that child): a module named `Adam` or `utilities3` imported
into the test process would stay in sys.modules for every later test.  The spectral layers have no CPU path in the product, so the
models get the oracle's operator blocks through `block_cls`, as tests/test_harness_cpu.py does.

One test needs the reference checkout itself and is skipped without it (set UNO_REFERENCE to its directory): the genuine
ns_train_2d.train_model runs once on the reference's own modules and once with dropin/ ahead of them."""
import importlib
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
DROPIN = os.path.join(ROOT, "dropin")
DROPIN_MODULES = ("darcy_flow_uno2d", "navier_stokes_uno2d", "navier_stokes_uno3d", "integral_operators", "Adam", "utilities3")


def child(check, *args, path=(DROPIN, ROOT, TESTS)):
    """run `check` of this file in a fresh interpreter whose sys.path starts with `path`; -> its output"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), os.pathsep.join(path), check, *args], capture_output=True, text=True,
                       cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"{check} failed:\n{r.stdout[-4000:]}\n{r.stderr[-6000:]}"
    return r.stdout


# ------------------------------------------------------------------------------------------------------------------ the child's checks
def _dropin():
    mods = {n: importlib.import_module(n) for n in DROPIN_MODULES}
    for n, m in mods.items():
        assert os.path.dirname(os.path.abspath(m.__file__)) == DROPIN, f"{n} resolved to {m.__file__}, not to dropin/"
    return mods


def check_signatures():
    """every recorded reference signature is a prefix of the drop-in class's, with equal defaults"""
    import dropin_loops
    mods = _dropin()
    sigs = dropin_loops.record()["signatures"]
    assert len(sigs) == 11
    for key, recorded in sigs.items():
        module, cls = key.split(".")
        own = list(inspect.signature(getattr(mods[module], cls).__init__).parameters.values())[1:]
        assert len(own) >= len(recorded), key
        for p, (name, default) in zip(own, recorded):
            assert p.name == name, (key, p.name, name)
            got = "<required>" if p.default is inspect.Parameter.empty else p.default
            got = list(got) if isinstance(got, tuple) else got
            assert got == default and type(got) is type(default), (key, name, got, default)
    # the harness classes themselves, not copies
    from uno_amd import harness
    assert mods["darcy_flow_uno2d"].UNO_9 is harness.UNO_9 and mods["navier_stokes_uno2d"].UNO_P is harness.UNO_P
    assert mods["navier_stokes_uno3d"].Uno3D_T40 is harness.Uno3D_T40 and mods["utilities3"].LpLoss is harness.LpLoss
    assert issubclass(mods["Adam"].Adam, harness.ComplexAdam)
    import uno_amd.integral_operators as native
    assert mods["integral_operators"].OperatorBlock_2D is native.OperatorBlock_2D
    ns = {}
    exec("from utilities3 import *\nfrom Adam import Adam", ns)               # the scripts' own import lines
    assert ns["LpLoss"] is harness.LpLoss and "MatReader" in ns


def check_constructors():
    """Adam(..., amsgrad=False) constructs; amsgrad=True and UNO_11(...) raise and say why"""
    import torch
    mods = _dropin()
    p = torch.nn.Parameter(torch.zeros(3))
    opt = mods["Adam"].Adam([p], lr=1e-3, weight_decay=1e-3, amsgrad=False)
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 1e-3
    torch.optim.lr_scheduler.StepLR(opt, step_size=50, gamma=0.5)
    with pytest.raises(ValueError, match="torch.maximum"):
        mods["Adam"].Adam([p], lr=1e-3, amsgrad=True)
    with pytest.raises(TypeError, match="residual"):
        mods["darcy_flow_uno2d"].UNO_11(3, 8, pad=5)


def check_lploss():
    """LpLoss against the float64 formula: the four flag combinations, p = 1, and the strided out[..., t].view(B, -1) call"""
    import torch
    LpLoss = _dropin()["utilities3"].LpLoss
    g = torch.Generator().manual_seed(7)
    B, S, T = 3, 6, 5
    y = torch.randn(B, S, S, T, generator=g)
    x = (y + 0.1 * torch.randn(B, S, S, T, generator=g)).requires_grad_(True)

    def want(a, b, p):
        a, b = a.detach().double().reshape(B, -1), b.double().reshape(B, -1)
        return torch.linalg.vector_norm(a - b, ord=p, dim=1) / torch.linalg.vector_norm(b, ord=p, dim=1)

    def close(got, ref):
        got, ref = got.detach().double(), ref
        assert got.shape == ref.shape
        assert bool(((got - ref).abs() <= 1e-5 * ref.abs()).all()), (got, ref)

    assert LpLoss().d == 2 and LpLoss().p == 2 and LpLoss().size_average and LpLoss().reduction
    for size_average in (True, False):
        for reduction in (True, False):
            loss = LpLoss(size_average=size_average, reduction=reduction)
            r = want(x, y, 2)
            ref = r if not reduction else (r.mean() if size_average else r.sum())
            close(loss(x, y), ref)
            close(loss.rel(x.view(B, -1), y.view(B, -1)), ref)
    close(LpLoss(p=1, size_average=False)(x, y), want(x, y, 1).sum())
    for t in (0, T - 1):                                      # ns_train_3d.py:58-61
        k, l = x[..., t], y[..., t]
        close(LpLoss(size_average=False)(k.view(B, -1), l.view(B, -1)), want(k, l, 2).sum())
    # differentiable: d/dx sum_b ratio_b = (x - y) / (||x - y|| ||y||) per row
    LpLoss(size_average=False)(x.view(B, -1), y.view(B, -1)).backward()
    d = (x.detach() - y).double().reshape(B, -1)
    ref = d / (d.norm(dim=1, keepdim=True) * y.double().reshape(B, -1).norm(dim=1, keepdim=True))
    assert float((x.grad.double().reshape(B, -1) - ref).norm() / ref.norm()) < 1e-5


def check_matreader(folder):
    """a file written with scipy.io.savemat comes back through MatReader's methods"""
    import scipy.io
    import torch
    MatReader = _dropin()["utilities3"].MatReader
    rng = np.random.default_rng(0)
    coeff, sol = rng.standard_normal((4, 5, 6)), rng.standard_normal((4, 5))
    path = os.path.join(folder, "fields.mat")
    scipy.io.savemat(path, {"coeff": coeff, "sol": sol})
    reader = MatReader(path)
    got = reader.read_field("coeff")
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == (4, 5, 6)
    assert np.array_equal(got.numpy(), coeff.astype(np.float32))
    reader.set_torch(False)
    reader.set_float(False)
    raw = reader.read_field("sol")
    assert isinstance(raw, np.ndarray) and raw.dtype == np.float64 and np.array_equal(raw, sol)
    reader.set_torch(True)
    reader.set_cuda(False)
    reader.load_file(path)
    assert reader.read_field("sol").dtype == torch.float64


def check_loop(name):
    """the written-out loop of tests/dropin_loops.py on the drop-in classes against the recorded genuine run"""
    import dropin_loops
    from oracle import spectral_oracle as so
    block = so.OracleOperatorBlock3d if name == "ns3d" else so.OracleOperatorBlock2d
    dropin_loops.run_and_compare(name, _dropin(), "cpu", block_cls=block)


def check_genuine(which, reference, out):
    """the genuine ns_train_2d.train_model(device="cpu"), one epoch of the recorded ns2d run; the saved weights go to `out`"""
    import torch
    import dropin_loops
    import ns_train_2d
    import navier_stokes_uno2d
    import integral_operators
    import Adam
    import utilities3
    assert os.path.dirname(os.path.abspath(ns_train_2d.__file__)) == os.path.abspath(reference)
    home = DROPIN if which == "dropin" else os.path.abspath(reference)
    for m in (navier_stokes_uno2d, integral_operators, Adam, utilities3):
        assert os.path.dirname(os.path.abspath(m.__file__)) == home, (which, m.__file__)
    assert ns_train_2d.Adam is Adam.Adam and ns_train_2d.LpLoss is utilities3.LpLoss
    cfg = dropin_loops.record()["loops"]["ns2d"]
    batches = dropin_loops.make_batches(cfg)
    block = None
    if which == "dropin":
        from oracle import spectral_oracle as so
        block = so.OracleOperatorBlock2d
    model = dropin_loops.build_model(cfg, navier_stokes_uno2d, block)
    n = cfg["x_shape"][0]
    ns_train_2d.train_model(model, batches["train"], batches["val"], batches["test"], n * cfg["train_batches"], n * cfg["val_batches"],
                            n * cfg["test_batches"], out, T_f=cfg["T_f"], epochs=1, learning_rate=cfg["lr"], device="cpu",
                            weight_decay=cfg["weight_decay"])
    assert os.path.exists(out) and list(torch.load(out)) == list(model.state_dict())


CHECKS = {"signatures": check_signatures, "constructors": check_constructors, "lploss": check_lploss, "matreader": check_matreader,
          "loop": check_loop, "genuine": check_genuine}


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def static_checks():
    return child("static")


@pytest.mark.parametrize("name", ["signatures", "constructors", "lploss"])
def test_names_signatures_and_loss(static_checks, name):
    """signatures: every recorded reference signature is a prefix of the drop-in class's, with equal defaults; constructors:
    Adam(amsgrad=False) constructs, amsgrad=True and UNO_11 raise; lploss: the four flag combinations, p = 1 and the strided call
    against float64"""
    assert f"ok {name}\n" in static_checks


def test_matreader_round_trip(tmp_path):
    pytest.importorskip("scipy.io")
    assert "ok matreader\n" in child("matreader", str(tmp_path))


@pytest.mark.parametrize("name", ["darcy", "ns2d", "ns3d"])
def test_written_out_loop_matches_the_recorded_reference_run(name):
    assert "ok loop\n" in child("loop", name)


def test_genuine_ns_train_2d_runs_unchanged_on_the_dropin_modules(tmp_path):
    """the reference's own ns_train_2d.py, imported from its checkout: once on the reference's modules, once with dropin/ ahead of them
    (route A' of INTEGRATION.md) - the saved weights agree to the parameter bounds of tests/dropin_loops.py"""
    import torch
    from conftest import rel_err
    from dropin_loops import TOL_PARAM, TOL_PARAM_NORM
    reference = os.environ.get("UNO_REFERENCE", "")
    if not (reference and os.path.isfile(os.path.join(reference, "ns_train_2d.py"))):
        pytest.skip("needs the reference checkout (UNO_REFERENCE=<directory>)")
    ref_out, own_out = str(tmp_path / "reference.pt"), str(tmp_path / "dropin.pt")
    child("genuine", "reference", reference, ref_out, path=(reference, TESTS, ROOT))
    child("genuine", "dropin", reference, own_out, path=(DROPIN, ROOT, reference, TESTS))
    ref, own = torch.load(ref_out), torch.load(own_out)
    assert list(ref) == list(own)
    worst = 0.0
    for k, v in ref.items():
        n = float(torch.linalg.vector_norm(v))
        assert abs(float(torch.linalg.vector_norm(own[k])) - n) <= TOL_PARAM_NORM * n + 1e-9, k
        e = float(rel_err(torch.view_as_real(own[k]).numpy() if own[k].is_complex() else own[k].numpy(),
                          torch.view_as_real(v).numpy() if v.is_complex() else v.numpy()))
        worst = max(worst, e)
        assert e < TOL_PARAM, (k, e)
    print(f"[dropin genuine ns_train_2d] largest relative difference of a saved parameter {worst:.2e}")


if __name__ == "__main__":
    sys.path[0:0] = sys.argv[1].split(os.pathsep)
    check, args = sys.argv[2], sys.argv[3:]
    for name in (("signatures", "constructors", "lploss") if check == "static" else (check,)):
        CHECKS[name](*args)
        print(f"ok {name}", flush=True)
