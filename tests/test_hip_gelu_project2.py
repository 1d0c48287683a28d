"""K11's two-source form (csrc/pointwise_fused.hip, `gelu_project2`: the end of UNO_P / UNO_S256, reference navier_stokes_uno2d.py:121-125,
320-324) against the float64 stock sequence on the device, as tests/test_hip_pointwise_fused.py holds the one-source form: 2e-6 for
out, gpre and gs, 2e-5 for gw and gb (the same operation class, the bounds of that file).  pytest -m gpu

Which form a shape reaches (gelu_project_threads / gelu_project_splits): one-wave workgroups while batch x ceil(pixels / 1024) < 1024,
and with them, from C1 + C2 = 16 channels on, the SPLIT forward (four waves share a tile) and the four channel splits of the backward."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [  # B, C1, C2, grid
    (1, 1, 1, (1,)),                 # smallest
    (2, 5, 3, (3, 7)),               # ragged quads
    (3, 96, 16, (45, 41)),           # UNO_P width 32 (SPLIT, channel splits of 28: the second source starts inside the last one)
    (2, 12, 16, (4099,)),            # UNO_S256 width 4, tail after whole tiles (SPLIT; the sources meet inside a split)
    (32, 12, 2, (64, 64)),           # small tensor just below the 16 channels of the SPLIT / channel-split forms: one wave walks all 14
    (2, 1000, 24, (130,)),           # C1 + C2 at the limit (GP_MAXC = 1024)
    (32, 12, 4, (64, 64)),           # the same small tensor AT 16 channels: SPLIT forward, 4 channel splits of 4 (the last is the second source)
    (16, 3, 2, (256, 257)),          # batch x ceil(pixels / 1024) = 1040: the 256-thread workgroups, ragged last tile
]


def rel(a, b):
    d = (a.double() - b).norm().item()
    n = b.norm().item()
    return d / n if n > 0 else d


def _reference(pre, s, w, b, gy, act2, s_grad):
    """float64 stock sequence: channel_mix(cat([gelu(pre), f(s)], 1), w, b) and its gradients"""
    pre2, s2, w2 = (t.detach().double().requires_grad_(True) for t in (pre, s, w))
    b2 = b.detach().double().requires_grad_(True) if b is not None else None
    y2 = torch.einsum("oc,bc...->bo...", w2, torch.cat([F.gelu(pre2), F.gelu(s2) if act2 else s2], 1))
    if b is not None:
        y2 = y2 + b2.view(1, 1, *([1] * (pre.dim() - 2)))
    leaves = [pre2] + ([s2] if s_grad else []) + [w2] + ([b2] if b is not None else [])
    return y2.detach(), torch.autograd.grad(y2, leaves, gy.double())


@pytest.mark.parametrize("s_grad", [True, False])
@pytest.mark.parametrize("act2", [False, True])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,C1,C2,grid", SHAPES)
def test_gelu_project2(B, C1, C2, grid, with_bias, act2, s_grad):
    from uno_amd.integral_operators import gelu_project2
    g = torch.Generator().manual_seed(B + C1 + 7 * C2)
    pre = (2.0 * torch.randn(B, C1, *grid, generator=g)).cuda().requires_grad_(True)
    s = (2.0 * torch.randn(B, C2, *grid, generator=g)).cuda().requires_grad_(s_grad)
    w = torch.randn(1, C1 + C2, generator=g).cuda().requires_grad_(True)
    b = torch.randn(1, generator=g).cuda().requires_grad_(True) if with_bias else None
    y = gelu_project2(pre, s, w, b, act2=act2)
    assert y.shape == (B, 1, *grid)
    assert type(y.grad_fn.next_functions[0][0]).__name__ == "_GeluProject2FnBackward"     # (under the final view) the native form, not the stock composition
    gy = torch.randn_like(y)
    leaves = [pre] + ([s] if s_grad else []) + [w] + ([b] if with_bias else [])
    got = torch.autograd.grad(y, leaves, gy)
    y2, ref = _reference(pre, s, w, b, gy, act2, s_grad)
    names = ["gpre"] + (["gs"] if s_grad else []) + ["gw"] + (["gb"] if with_bias else [])
    errs = {"out": rel(y, y2)}
    for n, a, r in zip(names, got, ref):
        assert a.shape == r.shape, n
        errs[n] = rel(a, r)
    print(" ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for n, e in errs.items():
        assert e < (2e-5 if n in ("gw", "gb") else 2e-6), (n, e)


def test_backward_is_reproducible():
    """two backward calls on (4, 96, 16, 9000) are bit-equal: per-workgroup partial sums, reduced in a fixed order"""
    from uno_amd import _native
    g = torch.Generator().manual_seed(11)
    pre, s = torch.randn(4, 96, 9000, generator=g).cuda(), torch.randn(4, 16, 9000, generator=g).cuda()
    w, gout = torch.randn(112, generator=g).cuda(), torch.randn(4, 9000, generator=g).cuda()
    first = _native.gelu_project2_backward(pre, s, w, gout, act2=True)
    second = _native.gelu_project2_backward(pre, s, w, gout, act2=True)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.equal(_native.gelu_project2_forward(pre, s, w, None, True), _native.gelu_project2_forward(pre, s, w, None, True))


def test_second_source_without_gradient_is_not_written():
    """need_gs=False passes gs = NULL: the other results are those of the full call, bit for bit"""
    from uno_amd import _native
    g = torch.Generator().manual_seed(12)
    pre, s = torch.randn(3, 20, 777, generator=g).cuda(), torch.randn(3, 6, 777, generator=g).cuda()
    w, gout = torch.randn(26, generator=g).cuda(), torch.randn(3, 777, generator=g).cuda()
    gpre, gs, gw, gb = _native.gelu_project2_backward(pre, s, w, gout, act2=False)
    gpre2, gs2, gw2, gb2 = _native.gelu_project2_backward(pre, s, w, gout, act2=False, need_gs=False, need_bias=False)
    assert gs2 is None and gb2 is None and gs is not None
    assert torch.equal(gpre, gpre2) and torch.equal(gw, gw2)
    assert torch.equal(gs, w[20:].view(1, 6, 1) * gout.view(3, 1, 777))            # identity second source: gs = w gout exactly
