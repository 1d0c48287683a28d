"""K11's two-source backward under the two process-wide launch switches (tests/test_hip_launch_state.py): it takes its sweep direction at
the one `next_sweep_reversed(SWEEP_PROJ)` call site that the one-source form uses, so it runs here pinned forward and pinned reversed -
both meet the float64 reference at the bounds of tests/test_hip_gelu_project2.py and all outputs are bit-equal between the two - and once
each with 0, 16 and 248 reserved CUs, every output and the workspace between guard bands that stay untouched.  pytest -m gpu"""
import pytest
import torch
import torch.nn.functional as F

from test_hip_launch_state import _check, _g, _rn, state  # noqa: F401  (fixture: sets and restores direction / reserved CUs)
from test_hip_redzone import redzone  # noqa: F401  (fixture: guarded device allocations)

pytestmark = pytest.mark.gpu

# B, C1, C2, P: one-wave workgroups with four channel splits (3 pixel tiles + a ragged tail, the sources meet inside the third split),
# and 256-thread workgroups (batch x ceil(P / 1024) = 1025) without a channel split
SHAPES = [(3, 20, 9, 777), (41, 3, 2, 24601)]


def _proj2_bwd(B, C1, C2, P, act2, need_gs=True):
    from uno_amd import _native
    g = _g(19)
    pre, s, gout, w = _rn(g, B, C1, P, scale=2.0), _rn(g, B, C2, P, scale=2.0), _rn(g, B, P), _rn(g, C1 + C2)
    gpre, gs, gw, gb = _native.gelu_project2_backward(pre, s, w, gout, act2=act2, need_gs=need_gs)
    p2, s2, w2 = pre.double().requires_grad_(True), s.double().requires_grad_(True), w.double().requires_grad_(True)
    out = torch.einsum("c,bcp->bp", w2, torch.cat([F.gelu(p2), F.gelu(s2) if act2 else s2], 1))
    rp, rs, rw = torch.autograd.grad(out, (p2, s2, w2), gout.double())
    res = [("gpre", gpre, rp, 2e-6), ("gw", gw, rw, 2e-5), ("gb", gb, gout.double().sum().view(1), 2e-5)]
    return res + ([("gs", gs, rs, 2e-6)] if need_gs else [])


@pytest.mark.parametrize("act2", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_both_directions_meet_the_reference_and_are_bit_equal(state, shape, act2):  # noqa: F811
    state("forward")
    fwd = _proj2_bwd(*shape, act2)
    _check(fwd, f"proj2 backward {shape} forward")
    state("reversed")
    rev = _proj2_bwd(*shape, act2)
    _check(rev, f"proj2 backward {shape} reversed")
    for (n, a, _, _), (_, b, _, _) in zip(fwd, rev):
        assert torch.equal(a, b), f"{n} depends on the sweep direction"


@pytest.mark.parametrize("reserve", [0, 16, 248])
def test_reserved_cus_between_guard_bands(state, redzone, reserve):  # noqa: F811
    from uno_amd import _native
    state("reversed" if reserve == 16 else "forward", reserve=reserve)
    for shape in SHAPES:
        _check(_proj2_bwd(*shape, True), f"proj2 backward {shape} reserve {reserve}")
        _check(_proj2_bwd(*shape, False, need_gs=False), f"proj2 backward {shape} reserve {reserve}, no gs")
    g = _g(23)
    pre, s, w, b = _rn(g, 3, 20, 777, scale=2.0), _rn(g, 3, 9, 777, scale=2.0), _rn(g, 29), _rn(g, 1)
    out = _native.gelu_project2_forward(pre, s, w, b, True)
    ref = torch.einsum("c,bcp->bp", w.double(), torch.cat([F.gelu(pre.double()), F.gelu(s.double())], 1)) + b.double()
    _check([("out", out, ref, 2e-6)], f"proj2 forward reserve {reserve}")
    # per backward call: gpre, gw, gb, the workspace (and gs); the forward's out
    assert redzone.check(f"proj2 reserve {reserve}") >= 2 * (5 + 4) + 1
