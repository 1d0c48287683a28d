"""`Uno3D_T20_256` / `Uno3D_T10_256` on the product blocks on the MI355X at S = 256, width 2, batch 1: against the reference-generated
goldens of tests/test_harness_ns3d_256_cpu.py (whose helpers these tests share), and element by element against the same model on the
oracle's blocks in float64 with the same weights.  pytest -m gpu

Bounds: 1e-4 for prediction and loss, 2e-4 for the gradient norms against the fixture - those of tests/test_hip_ns3d_models.py; the
model rule of tests/test_hip_resample3d_any.py against the oracle, rel_err <= max(1e-4, 4 x rel_err(R32, R64))."""
import importlib.util
import os

import pytest
import torch

from conftest import ROOT
from oracle import spectral_oracle as so
from test_harness_ns3d_256_cpu import CASES, parity
from test_hip_workload_parity import MODEL_TOL, _r, _rel, compare_to_reference, forward_backward
from uno_amd.harness.models import Uno3D_T10_256, Uno3D_T20_256

pytestmark = pytest.mark.gpu
TOL_PRED, TOL_GRAD = 1e-4, 2e-4
# every transform of torch.fft (the stock path of integral_operators uses rfftn / irfftn, its 1-D layers rfft / irfft)
FFT_FUNCTIONS = [n for n in dir(torch.fft) if n.lstrip("ihr").startswith("fft") and not n.endswith(("freq", "shift")) and callable(getattr(torch.fft, n))]
WIDE = ("uno::resample3d_wide_fwd_plane_kernel", "uno::resample3d_wide_axis_kernel", "uno::resample3d_wide_inv_plane_kernel")


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_product(name):
    parity(name, None, dev(), TOL_PRED, TOL_GRAD)


@pytest.mark.parametrize("cls,T_f,pad,both", [(Uno3D_T20_256, 20, 3, True), (Uno3D_T10_256, 10, 2, False)], ids=["t20_256-pad3-both", "t10_256-pad2"])
def test_matches_the_float64_oracle_and_runs_the_wide_kernels(cls, T_f, pad, both, monkeypatch):
    """prediction, ns3d_loss and every parameter gradient against the same model on the oracle's blocks in float64 with the same weights,
    every switch of integral_operators at its default.  The library's launch records of the pass hold the wide-axis kernels - three
    launches forward and three backward for conv0 and for conv8, twelve in all.  The library's records hold its own kernels only, so
    "no rocFFT kernel ran" is shown from the other side: every transform function of torch.fft raises during the product pass;
    conv0's and conv8's point-wise branches on their own launch the wide-axis kernels and no other resample family."""
    import uno_amd.integral_operators as io
    from uno_amd import _native
    wl = "c4_256"           # (the c4 family of test_hip_workload_parity.py: ns3d_loss, prediction through a forward hook)
    assert (io.STOCK_FFT_RESAMPLE3D, io.NATIVE_RESAMPLE3D_ANY, io.NATIVE_RESAMPLE3D_WIDE, io.ONE_BUFFER_3D_ANY) == (False,) * 4
    g = torch.Generator().manual_seed(4321 + T_f)
    inp = (torch.randn(1, 256, 256, 10, 1, generator=g), torch.randn(1, 256, 256, T_f, generator=g))
    torch.manual_seed(0)
    m32 = cls(6, 2, pad=pad, pad_both=both, block_cls=so.OracleOperatorBlock3d)
    state = {k: v.clone() for k, v in m32.state_dict().items()}
    m64 = so.to_float64(m32)
    pred32, loss32 = forward_backward(wl, m32, inp)
    pred64, loss64 = forward_backward(wl, m64, tuple(t.double() for t in inp))
    assert pred64.dtype == torch.float64 and tuple(pred64.shape) == (1, 256, 256, T_f, 1)
    ref = {"pred": pred64, "loss": float(loss64), "grads": {}, "floor": {}, "norm32": {}}
    ref["floor"]["pred"] = _rel(pred32, pred64)
    ref["floor"]["loss"] = abs(float(loss32) - float(loss64)) / abs(float(loss64))
    p32 = dict(m32.named_parameters())
    norm = lambda t: float(torch.linalg.vector_norm(_r(t)))
    for k, p in m64.named_parameters():
        ref["grads"][k] = p.grad
        ref["floor"][k] = _rel(p32[k].grad, p.grad)
        ref["norm32"][k] = norm(p32[k].grad)
    norms = {k: norm(v) for k, v in ref["grads"].items()}
    ref["gmax"] = max(norms.values())
    ref["zero"] = sorted(k for k, n in norms.items() if n <= 1e-12 * ref["gmax"])
    assert ref["zero"] == [f"conv{i}.w.conv.bias" for i in (0, 3, 5, 7)]         # the 1x1x1 bias in front of an InstanceNorm3d

    torch.manual_seed(0)
    prod = cls(6, 2, pad=pad, pad_both=both)
    prod.load_state_dict(state, strict=True)
    prod = prod.to(dev())
    dinp = tuple(t.to(dev()) for t in inp)
    assert {"rfftn", "irfftn", "fftn", "ifftn", "rfft", "irfft", "fft", "ifft", "rfft2", "irfft2", "hfft", "ihfft"} <= set(FFT_FUNCTIONS)

    def no_fft(*a, **k):
        raise AssertionError("torch.fft was entered on the product path")
    with monkeypatch.context() as patch:
        for name in FFT_FUNCTIONS:
            patch.setattr(torch.fft, name, no_fft)
        _native.profile_begin(100000)
        try:
            pred, loss = forward_backward(wl, prod, dinp)
            torch.cuda.synchronize()
        finally:
            names = [n for n, _, _ in _native.profile_end()]
    bad = compare_to_reference(f"{cls.__name__}(6, 2, pad={pad})", ref, pred, loss, {k: p.grad for k, p in prod.named_parameters()}, tol=MODEL_TOL)
    assert not bad, bad
    for k in WIDE:
        assert names.count(k) == 4, (k, names.count(k))        # conv0 and conv8, forward and backward
    assert sum("resample3d_any" in n for n in names) == (6 if cls is Uno3D_T20_256 and pad == 3 and both else 0)

    d3 = 10 + (2 if both else 1) * int(pad * 0.1 * 10)
    grids, _ = prod._plan(256, 256, d3, 0)
    for blk, din, dout in ((prod.conv0, (256, 256, d3), grids[0]), (prod.conv8, grids[7], grids[8])):
        assert max(din[0], dout[0]) == 256 and min(din[0], dout[0]) == 64
        x = torch.randn(1, blk.conv.in_channels, *din, device=dev(), requires_grad=True)
        _native.profile_begin(1000)
        try:
            blk.w(x, *dout).sum().backward()
            torch.cuda.synchronize()
        finally:
            layer = [n for n, _, _ in _native.profile_end()]
        assert sum("resample3d_wide" in n for n in layer) == 6, layer
        assert not any("resample3d_any" in n or ("dft2d_" in n and "plane" in n) for n in layer), layer


def test_one_training_step_through_the_drop_in_names():
    """dropin/navier_stokes_uno3d.py exports the harness classes under the reference's names; a model built through it takes one
    optimiser step at S = 256 that moves every parameter"""
    from uno_amd.harness import ComplexAdam, ns3d_loss
    spec = importlib.util.spec_from_file_location("_dropin_navier_stokes_uno3d_256", os.path.join(ROOT, "dropin", "navier_stokes_uno3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.Uno3D_T20_256 is Uno3D_T20_256 and mod.Uno3D_T10_256 is Uno3D_T10_256
    assert not hasattr(mod, "Uno3D_T40_256") and not hasattr(mod, "Uno3D_T9_256")
    torch.manual_seed(2)
    model = mod.Uno3D_T10_256(6, 2, pad=2).to(dev())
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = ComplexAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(3)
    xx, yy = torch.randn(1, 256, 256, 10, 1, generator=g).to(dev()), torch.randn(1, 256, 256, 10, generator=g).to(dev())
    loss = ns3d_loss(model, xx, yy)
    loss.backward()
    opt.step()
    assert torch.isfinite(loss.detach())
    assert all(not torch.equal(p.detach(), before[k]) for k, p in model.named_parameters())
