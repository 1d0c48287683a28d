"""NS-3D harness models `Uno3D_T10` and `Uno3D_T9` (reference navier_stokes_uno3d.py:412-602, 605-797) against reference-generated golden
values (tests/golden/harness_ns3d_t10.npz, harness_ns3d_t9.npz; tools/gen_golden_ns3d_models.py).  As in tests/test_harness_ns.py the
golden weights are seeded, not stored: every test first verifies the per-parameter float64 checksums, i.e. that the constructor
reproduced the reference's initialisation bit for bit, and the ordered state_dict keys and shapes.  The oracle blocks are the test
doubles here; tests/test_hip_ns3d_models.py runs the product path.

Bounds: 1e-5 for prediction and loss, 5e-4 for the gradient norms - those of test_ns3d_cpu_oracle_blocks (tests/test_harness_ns.py) for
`Uno3D_T20`, which has the same layer kinds."""
import pytest
import torch

from conftest import Case, load_cases, rel_err
from harness_checks import check_grads, check_init, check_strict_load
from oracle import spectral_oracle as so
from test_model_census_cpu import RecordingBlock, record
from uno_amd.harness import Uno3D_T9, Uno3D_T10, Uno3D_T20, ns3d_loss

Z10, _ = load_cases("harness_ns3d_t10.npz")
Z9, _ = load_cases("harness_ns3d_t9.npz")
# case -> (fixture file, class, output steps)
CASES = {"t10": (Z10, Uno3D_T10, 10), "t10both": (Z10, Uno3D_T10, 10), "t9": (Z9, Uno3D_T9, 9)}
TOL_PRED, TOL_GRAD = 1e-5, 5e-4


def build(name, block_cls):
    z, cls, T_f = CASES[name]
    c = Case(z, name)
    in_width, width, pad, both = (int(v) for v in c.ctor)
    torch.manual_seed(int(c.seed))
    kw = {"block_cls": block_cls} if block_cls else {}
    return c, cls(in_width, width, pad=pad, pad_both=bool(both), **kw), T_f


def parity(name, block_cls, dev, tol_pred, tol_grad):
    c, model, T_f = build(name, block_cls)
    check_init(model, c)
    check_strict_load(model, c, lambda: type(model)(model.in_width, model.width, pad=model.pad, pad_both=model.pad_both, block_cls=type(model.conv0)))
    model = model.to(dev)
    xx, yy = torch.from_numpy(c.xx).to(dev), torch.from_numpy(c.yy).to(dev)
    B, S = xx.shape[0], xx.shape[1]
    with torch.no_grad():
        out = model(xx)
    assert out.shape == (B, S, S, T_f, 1)
    e = rel_err(out.view(B, S, S, T_f).cpu().numpy(), c.pred)
    loss = ns3d_loss(model, xx, yy)
    loss.backward()
    print(f"[{name} {dev}] prediction {e:.2e}, loss {abs(float(loss.detach()) - float(c.loss)) / abs(float(c.loss)):.2e}")
    assert e < tol_pred
    assert abs(float(loss.detach()) - float(c.loss)) < tol_pred * abs(float(c.loss))
    check_grads(model, c, tol_grad)
    return model, c


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_oracle_blocks(name):
    parity(name, so.OracleOperatorBlock3d, "cpu", TOL_PRED, TOL_GRAD)


def test_both_are_uno3d_t20_with_the_same_constructor_arguments():
    for cls in (Uno3D_T10, Uno3D_T9):
        m = cls(6, 2, pad=2, factor=1, pad_both=False, block_cls=so.OracleOperatorBlock3d)
        assert isinstance(m, Uno3D_T20) and m.fc.weight.shape == (12, 6) and m.fc2.weight.shape == (1, 8)
        assert m.get_grid.__func__ is Uno3D_T20.get_grid and m._resize is Uno3D_T20._resize


# (Uno3D_T9's conv1 keeps 18 modes on the half grid: S >= 36)
@pytest.mark.parametrize("cls,T_in,T_out,S", [(Uno3D_T10, 10, 10, 64), (Uno3D_T10, 10, 10, 48), (Uno3D_T10, 10, 10, 32), (Uno3D_T9, 6, 9, 64), (Uno3D_T9, 6, 9, 48)])
@pytest.mark.parametrize("pad", [0, 2, 3])
@pytest.mark.parametrize("both", [False, True])
def test_census_every_layer_is_inside_the_pruned_dft_range(cls, T_in, T_out, S, pad, both):
    """Every pointwise_op_3D grid pair of both models at S = 64 (and at the fixtures' 48 and 32) is inside the pruned-DFT resampling kernels' range (neither model needs
    the any-grid opt-in that Uno3D_T40 takes), and every SpectralConv3d_Uno call keeps no more modes than its grids hold."""
    from uno_amd.spectral3d import _resample3d_pruned_applies
    model = record(cls, 6, 2, pad=pad, pad_both=both)
    with torch.no_grad():
        out = model(torch.zeros(1, S, S, T_in, 1))
    if not both:            # (padded on both sides Uno3D_T9 returns 10 steps as the reference does: 6 + 1 + 1 -> int(9 * 8 / 6) = 12, less 1 + 1)
        assert out.shape == (1, S, S, T_out, 1)
    assert len(RecordingBlock.calls) == 7
    for (*_, m1, m2, m3, _norm, _non_lin), ((_c, *din), dout) in zip(RecordingBlock.ctor, RecordingBlock.calls):      # (the blocks are called in construction order)
        assert _resample3d_pruned_applies(tuple(din), tuple(dout)), (din, dout)
        so.check_modes_3d(*din, *dout, m1, m2, m3)
