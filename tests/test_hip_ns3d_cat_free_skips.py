"""The NS-3D models with their inner skip connections consumed without torch.cat (harness.models.CAT_FREE_SKIPS_3D /
enable_cat_free_skips_3d: OperatorBlock_3D.forward_cat on the block after each inner skip): against the reference-generated goldens the
default path is held to, against the default path itself - alone and together with enable_native_ends_3d, after which no torch.cat of
activations is left in the model body - and under graph capture.  pytest -m gpu

This file mirrors tests/test_hip_ns3d_native_ends.py: its six CONFIGS, its bounds (1e-4 / 2e-4 against the goldens; opted-in against
default 2e-6 for the prediction and 2e-5 relative L2 for EVERY parameter gradient, element-wise) and its residue rule for the 1x1x1 biases
in front of an InstanceNorm3d, whose gradient is exactly zero in exact arithmetic.  All of these are that file's own, where they are
explained.  The two paths differ in the order of the 1x1x1 convolutions' float32 sums only: the two-source spectral layer runs the
transform kernels the concatenation would run and is bit-equal to it (tests/test_hip_dft3d_grouped.py)."""
import inspect

import pytest
import torch

from harness_checks import assert_graphed_step_equals_eager
from test_hip_ns3d_native_ends import CONFIGS, TOL_GRAD, TOL_PRED, TOL_SAME_GRAD, TOL_SAME_PRED, _float64_gradients, _pass
from uno_amd.harness import Uno3D_T10, Uno3D_T20, Uno3D_T40, models, ns3d_loss

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def opted(monkeypatch):
    monkeypatch.setattr(models, "CAT_FREE_SKIPS_3D", True)


@pytest.mark.parametrize("name", ["t10", "t10both", "t9"])
def test_t10_t9_goldens_with_cat_free_skips(name, opted):
    from test_harness_ns3d_models import parity
    model, _ = parity(name, None, dev(), TOL_PRED, TOL_GRAD)
    assert model._cat_free_skips(torch.zeros(1, device=dev()))


def test_t20_golden_with_cat_free_skips(opted):
    from test_harness_ns import _ns3d
    _ns3d(None, dev(), TOL_PRED, TOL_GRAD)


def _compare(key, tag, model, g64, p0, g0, p1, g1):
    """prediction and every parameter gradient of an opted-in pass against the default pass's: the criteria of
    tests/test_hip_ns3d_native_ends.py::test_opted_in_equals_default_and_runs_the_new_kernels"""
    ep = float((p1.double() - p0.double()).norm() / p0.double().norm())
    n64 = {k: float(v.norm()) for k, v in g64.items()}
    zero = sorted(k for k, n in n64.items() if n <= 1e-12 * max(n64.values()))
    assert zero == sorted(f"{name}.w.conv.bias" for name in model._NORMALIZED), zero        # exactly zero in exact arithmetic: nothing else
    nmax = max(float(torch.linalg.vector_norm(v)) for v in g0.values())
    worst = ("", 0.0)
    bad = []
    for k, a in g0.items():
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, g1[k]))
        if k in zero:                           # a residue on both paths
            na, nb = float(torch.linalg.vector_norm(a)), float(torch.linalg.vector_norm(b))
            if not nb <= 4 * max(na, 1e-6 * nmax):
                bad.append((k, "residue", nb / nmax))
            continue
        e = float((a.double() - b.double()).norm() / a.double().norm())
        if e > worst[1]:
            worst = (k, e)
        if not e < TOL_SAME_GRAD:
            bad.append((k, e))
    print(f"[{key}] {tag} against default: prediction {ep:.2e}, worst gradient {worst[1]:.2e} ({worst[0]})")
    assert ep < TOL_SAME_PRED
    assert not bad, bad


@pytest.mark.parametrize("key", list(CONFIGS))
def test_opted_in_equals_default_alone_and_with_native_ends(key):
    """prediction within 2e-6 and EVERY parameter gradient within 2e-5 (relative L2) of the default path's, with the inner skips cat-free
    and with the native ends as well; switching both off again gives the default path back bit for bit.

    Measured on one MI355X (prediction; worst parameter gradient), cat-free skips | with native ends as well:
    t10-pad3 6.5e-8; 8.8e-7 | 3.5e-7; 7.5e-6 - t10-pad2-both 7.1e-8; 6.0e-7 | 4.2e-7; 8.3e-6 - t9-pad3 1.3e-7; 1.8e-6 | 8.9e-7; 8.5e-6 -
    t20-pad3-both 1.6e-7; 1.0e-6 | 1.2e-6; 9.3e-6 - t40-pad3 0; 0 | 5.0e-7; 3.9e-6 - t20-pad0 1.6e-7; 1.7e-6 | 1.8e-6; 1.1e-5.
    (t40 is bit-equal: its conv7 / conv8 resample on the any-grid kernels and take the two branches, where forward_cat is the stock
    composition; the seven-block models at S <= 64 run both inner skips on the two-source Function.)"""
    cls, kw, S, T_in, T_out, B = CONFIGS[key]
    torch.manual_seed(17)
    width = 4 if cls is Uno3D_T40 else 2
    model = cls(6, width, **kw).to(dev())
    g = torch.Generator().manual_seed(18)
    xx, yy = torch.randn(B, S, S, T_in, 1, generator=g).to(dev()), torch.randn(B, S, S, T_out, generator=g).to(dev())
    assert models.CAT_FREE_SKIPS_3D is False and not model.cat_free_skips and not model.native_ends
    p0, g0, _ = _pass(model, xx, yy)
    g64 = _float64_gradients(cls, width, kw, model, xx, yy)
    assert models.enable_cat_free_skips_3d(model) is model and model.cat_free_skips and model._cat_free_skips(xx)
    p1, g1, _ = _pass(model, xx, yy)
    assert p1.shape == p0.shape == (B, S, S, T_out, 1)
    _compare(key, "cat-free skips", model, g64, p0, g0, p1, g1)
    models.enable_native_ends_3d(model)
    p2, g2, _ = _pass(model, xx, yy)
    _compare(key, "cat-free skips + native ends", model, g64, p0, g0, p2, g2)
    models.enable_native_ends_3d(model, False)
    models.enable_cat_free_skips_3d(model, False)
    p3, g3, _ = _pass(model, xx, yy)
    assert torch.equal(p3, p0) and all(torch.equal(g3[k], g0[k]) for k in g0)


def test_no_activation_cat_is_left_in_the_model_body(monkeypatch):
    """torch.cat calls on 5-D tensors along dim 1 in one training pass of Uno3D_T20: 3 by default (two inner skips and the last one), 1
    with the cat-free skips, 0 with the native ends as well"""
    cls, kw, S, T_in, T_out, B = CONFIGS["t20-pad3-both"]
    torch.manual_seed(3)
    model = cls(6, 2, **kw).to(dev())
    xx, yy = torch.randn(B, S, S, T_in, 1, device=dev()), torch.randn(B, S, S, T_out, device=dev())
    calls = []
    cat = torch.cat

    def counting(tensors, *args, **kwargs):
        tensors = list(tensors)
        dim = kwargs.get("dim", args[0] if args else 0)
        if dim == 1 and all(t.dim() == 5 for t in tensors):
            calls.append(tuple(t.shape[1] for t in tensors))
        return cat(tensors, *args, **kwargs)
    monkeypatch.setattr(torch, "cat", counting)

    def count():
        calls.clear()
        _pass(model, xx, yy)
        return len(calls)
    assert count() == 3
    models.enable_cat_free_skips_3d(model)
    assert count() == 1
    models.enable_native_ends_3d(model)
    assert count() == 0
    models.enable_cat_free_skips_3d(model, False)
    assert count() == 2


def test_graphed_step_equals_eager_step_uno3d_t10_with_cat_free_skips(opted):
    """harness.GraphedStep on an opted-in Uno3D_T10(6, 2, pad=3), S = 32, batch 2, two batches: the replay is bit-equal to the eager step
    (the pattern of test_graphed_step_equals_eager_step_uno3d_t10, tests/test_hip_ns3d_models.py)"""
    from uno_amd.harness import ComplexAdam

    def make(cap):
        torch.manual_seed(5)
        m = Uno3D_T10(6, 2, pad=3).to(dev())
        return m, ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(2, 32, 32, 10, 1, generator=g).to(dev()), torch.randn(2, 32, 32, 10, generator=g).to(dev())) for _ in range(2)]
    assert_graphed_step_equals_eager(make, ns3d_loss, batches)


def test_the_switch_is_off_by_default_and_the_bench_workloads_do_not_opt_in():
    from uno_amd.harness import workloads
    assert models.CAT_FREE_SKIPS_3D is False and Uno3D_T20.cat_free_skips is False
    assert "cat_free_skips" not in inspect.getsource(workloads) and "CAT_FREE_SKIPS_3D" not in inspect.getsource(workloads)
