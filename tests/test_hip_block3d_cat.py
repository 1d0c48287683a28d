"""OperatorBlock_3D.forward_cat: a skip connection consumed from its two tensors where they lie (_OperatorBlock3dCatFn: the two-source
spectral layer, the two-source channel-mix calls, the one-source block's resample and epilogue) against the same block on torch.cat.
pytest -m gpu

Criteria: those of the 2-D test test_forward_cat_equals_block_of_concatenation (tests/test_hip_blocks.py) - output
max|d| / max|ref| < 2e-6, every gradient max|d| <= 2e-5 max|ref| + 2e-6 gmax.  The channel counts are chosen so that each source and the
concatenation are on the same side of the 48-volume threshold between the one-workgroup-per-volume kernels and the plane path at B = 3
(16 + 16 and 64 + 64: 48 volumes or more each; 5 + 7: fewer each) - and the two-source layer calls choose their transform kernels for
the concatenation's count in any case - so the spectral branch is bit-equal and what differs is the order of the 1x1x1 convolution's
float32 sums:
    16 + 16   one two-source mix launch forward (sources split at a multiple of 16), two accumulating launches for the input gradients
    64 + 64   split destinations from one launch and the two-source weight-gradient kernel as well
    5 + 7     every fallback: two one-source launches forward, backward and for the weight gradient
Grids (at most 16 x 16 x 12): down-sampling, same-size and up-sampling inside the pruned-DFT resample kernels' range, and one any-grid
geometry under enable_one_buffer_any_grid.

Measured on one MI355X: 16 + 16 and 64 + 64 (and the any-grid case) bit-equal in output and every gradient on all three grids; 5 + 7
output 1.0e-7 ... 4.1e-7, worst gradient at 0.009 ... 0.51 of its bound."""
import pytest
import torch

from test_hip_uninit import _grads, _three_runs
from uno_amd.integral_operators import OperatorBlock_3D, enable_one_buffer_any_grid
from uno_amd.spectral3d import _resample3d_plan

pytestmark = pytest.mark.gpu
B = 3
GRIDS = {"down": ((16, 16, 12), (8, 8, 8)), "same": ((12, 12, 10), (12, 12, 10)), "up": ((8, 8, 8), (16, 16, 12))}
MODES = (4, 4, 3)
SPLITS = {"16+16": (16, 16, 32), "64+64": (64, 64, 24), "5+7": (5, 7, 9)}      # C1, C2, Co
CAT_NODE, ONE_NODE = "_OperatorBlock3dCatFnBackward", "_OperatorBlock3dFnBackward"


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nodes(y):
    seen, todo = set(), [y.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        todo += [f for f, _ in n.next_functions]
    return {type(n).__name__ for n in seen}


def _compare(blk, a, b, dout, what):
    params = list(blk.parameters())
    y = blk.forward_cat([a, b], *dout)
    assert CAT_NODE in _nodes(y) and "CatBackward0" not in _nodes(y), _nodes(y)
    gy = torch.randn_like(y)
    got = torch.autograd.grad(y, [a, b] + params, gy)
    y2 = blk(torch.cat([a, b], dim=1), *dout)
    assert ONE_NODE in _nodes(y2)
    ref = torch.autograd.grad(y2, [a, b] + params, gy)
    ey = ((y - y2).abs().max() / y2.abs().max()).item()
    gmax = max(float(r.abs().max()) for r in ref)
    eg = max(float((g - r).abs().max()) / (2e-5 * float(r.abs().max()) + 2e-6 * gmax) for g, r in zip(got, ref))
    print(f"[{what}] output {ey:.2e} (bound 2e-6), worst gradient at {eg:.3f} of its bound")
    assert y.shape == y2.shape and ey < 2e-6
    for g, r in zip(got, ref):
        assert g.shape == r.shape
        assert float((g - r).abs().max()) <= 2e-5 * float(r.abs().max()) + 2e-6 * gmax


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_forward_cat_equals_block_of_concatenation(grid, normalize, split):
    din, dout = GRIDS[grid]
    C1, C2, Co = SPLITS[split]
    assert _resample3d_plan(din, dout, dev()) is not None
    assert (B * C1 >= 48) == (B * C2 >= 48) == (B * (C1 + C2) >= 48)            # one transform path for the sources and the concatenation
    torch.manual_seed(5)
    blk = OperatorBlock_3D(C1 + C2, Co, *dout, *MODES, Normalize=normalize).to(dev())
    a = torch.randn(B, C1, *din, device=dev(), requires_grad=True)
    b = torch.randn(B, C2, *din, device=dev(), requires_grad=True)
    _compare(blk, a, b, dout, f"{grid} {split} normalize={normalize}")


def test_forward_cat_on_an_any_grid_geometry():
    din, dout = (15, 15, 9), (7, 7, 6)
    assert _resample3d_plan(din, dout, dev()) is None
    torch.manual_seed(6)
    blk = enable_one_buffer_any_grid(OperatorBlock_3D(16 + 16, 8, *dout, 3, 3, 3)).to(dev())
    a = torch.randn(B, 16, *din, device=dev(), requires_grad=True)
    b = torch.randn(B, 16, *din, device=dev(), requires_grad=True)
    _compare(blk, a, b, dout, "any grid 16+16")


def test_fallbacks_return_what_forward_of_the_concatenation_returns():
    din, dout = GRIDS["down"]
    torch.manual_seed(7)
    blk = OperatorBlock_3D(5 + 7, 4, *dout, *MODES)
    a, b = torch.randn(2, 5, *din), torch.randn(2, 7, *din)
    # CPU tensors: the spectral layer has no host path and raises, as forward() does on the concatenation
    with pytest.raises(RuntimeError, match="HIP device") as e1:
        blk.forward_cat([a, b])
    with pytest.raises(RuntimeError, match="HIP device") as e2:
        blk(torch.cat([a, b], dim=1))
    assert str(e1.value) == str(e2.value)
    blk = blk.to(dev())
    a, b = a.to(dev()), b.to(dev())
    # the two sources on different grids: torch.cat's refusal
    with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
        blk.forward_cat([a, b[..., :-1].contiguous()])
    # the spectral layer's default grid differs from the point-wise layer's: no one-buffer form, the two branches on the concatenation
    blk.w.dim1 = dout[0] + 2
    with pytest.raises(RuntimeError) as e1:
        blk.forward_cat([a, b])
    with pytest.raises(RuntimeError) as e2:
        blk(torch.cat([a, b], dim=1))
    assert str(e1.value) == str(e2.value)
    blk.w.dim1 = dout[0]
    # three sources, and channels that do not sum to in_channels with the default grids: forward() on the concatenation, bit for bit
    c = torch.randn(2, 3, *din, device=dev())
    three = blk.forward_cat([a, b[:, :4].contiguous(), c])
    assert ONE_NODE in _nodes(three) and torch.equal(three, blk(torch.cat([a, b[:, :4], c], dim=1)))
    with pytest.raises(RuntimeError, match="input channels"):
        blk.forward_cat([a, c])


def test_call_time_grid_override_persists_on_the_spectral_layer():
    din, dout = GRIDS["down"]
    torch.manual_seed(8)
    blk = OperatorBlock_3D(16 + 16, 4, *dout, *MODES).to(dev())
    a, b = torch.randn(B, 16, *din, device=dev()), torch.randn(B, 16, *din, device=dev())
    y = blk.forward_cat([a, b], 8, 8, 6)
    assert CAT_NODE in _nodes(y) and y.shape[-3:] == (8, 8, 6)
    assert (blk.conv.dim1, blk.conv.dim2, blk.conv.dim3) == (8, 8, 6) and (blk.w.dim1, blk.w.dim2, blk.w.dim3) == dout


def test_forward_cat_on_poisoned_memory(monkeypatch):
    """plain, 0xFF and 0x7F allocations (the fixture of tests/test_hip_uninit.py): output and gradients finite and bit-equal across the
    three.  At least 11 poisoned allocations per block (22 per run): y, xtrunc and the workspace of the forward layer call, the 1x1x1 convolution's
    output; gx1, gx2, the four weight gradients and the workspace of the backward layer call - the resample calls' come on top."""
    din, dout = GRIDS["down"]

    def workload():
        torch.manual_seed(9)
        out = []
        for C1, C2 in ((64, 64), (5, 7)):
            blk = OperatorBlock_3D(C1 + C2, 6, *dout, *MODES).to(dev())
            a = torch.randn(B, C1, *din, device=dev(), requires_grad=True)
            b = torch.randn(B, C2, *din, device=dev(), requires_grad=True)
            y = blk.forward_cat([a, b])
            assert type(y.grad_fn).__name__ == CAT_NODE
            y.square().sum().backward()
            out += [y.detach(), a.grad, b.grad] + _grads(blk)
        return out
    _three_runs(monkeypatch, workload, 22, "OperatorBlock_3D.forward_cat")
