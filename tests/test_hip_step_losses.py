"""uno_rel_l2_steps_backward (K17-B, uno_amd/csrc/rel_l2_steps.hip) through harness.step_losses on the MI355X: the gradient of the
whole-trajectory loss (full_sum) and of the per-step sum (step_sum) at pred from ONE forward pass, and ns3d_loss(native=True) on it.

Reference: float64 autograd through harness.losses._step_errors_stock (the slice-by-slice stock formula) on the CPU, computed once per
shape.  Bound: conftest.rel_err <= 1e-5, the gradient bound of tests/test_hip_lp_loss.py; the forward fields must equal step_errors'
bit for bit (the same two launches).

Shapes (B, P, T): (2, 33, 3) the 4-byte path with ragged everything; (3, 1024, 20) the 16-byte path; (1, 5000, 1) T = 1;
(2, P*, 256) T at its limit with P* = 17, the smallest P at which K17 cuts T = 256 into more than one chunk (found below from the
kernel's own workspace rule: 16 pixels per chunk there); views whose base is 4-byte but not 16-byte aligned at T = 5 (T % 4 != 0) and
at T = 8 (the 16-byte path's T, refused by the alignment); (4, 65536, 12) and (4, 70000, 5), 3.1 M and 1.4 M elements per tensor: more work than
the launch has workgroups for on either path, so threads walk the grid-stride loop more than once and a reservation changes the grid.

Measured on the MI355X (printed per case): gradient relative error 4.1e-8 ... 1.9e-7 over all shapes and weightings; ns3d_loss on
Uno3D_T20(6, 2, pad=3), 32^2, batch 2: default 2.073801 / 41.476429, native 2.0738008 / 41.476429 (loss / step error)."""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL_GRAD = 1e-5
COMBOS = [(1.0, 0.0), (0.0, 1.0), (0.7, -1.3)]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def chunks(B, P, T):
    from uno_amd import _native
    return _native.lib().uno_rel_l2_steps_ws_bytes(B, P, T) // (8 * B * T)


@functools.lru_cache(maxsize=None)
def p_star():
    P = 1
    while chunks(2, P, 256) < 2:
        P += 1
    return P


def shapes():
    return [(2, 33, 3), (3, 1024, 20), (1, 5000, 1), (2, p_star(), 256)]


SHAPE_IDS = ["2x33x3", "3x1024x20", "1x5000x1", "2xPstarx256"]


@functools.lru_cache(maxsize=None)
def problem(shape, equal_slice=None):
    """(pred, target) on the host, and the float64 gradients of full_sum and of step_sum at pred (never modified)"""
    from uno_amd.harness.losses import _step_errors_stock
    B, P, T = shape
    g = torch.Generator().manual_seed(B * 7 + P * 3 + T)
    target = torch.randn(B, P, T, generator=g)
    pred = target + 0.1 * torch.randn(B, P, T, generator=g)
    if equal_slice is not None:
        pred[equal_slice[0], :, equal_slice[1]] = target[equal_slice[0], :, equal_slice[1]]
    p64 = pred.double().requires_grad_(True)
    r = _step_errors_stock(p64, target.double())
    g_full, = torch.autograd.grad(r.full_sum, p64, retain_graph=True)
    g_step, = torch.autograd.grad(r.step_sum, p64)
    return pred, target, g_full, g_step


def step_losses(pred, target):
    from uno_amd.harness import step_losses as fn
    return fn(pred, target)


def same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def grad_of(p, y, a, b):
    p = p.detach().requires_grad_(True)
    r = step_losses(p, y)
    (a * r.full_sum + b * r.step_sum).backward()
    return p.grad


def unaligned(t):
    """a dense device copy of t whose base is 4-byte but not 16-byte aligned"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev())
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_p_star_is_the_first_p_with_two_chunks_at_t_256():
    assert p_star() == 17 and chunks(2, p_star() - 1, 256) == 1 and chunks(2, p_star(), 256) == 2


def test_the_symbol_and_the_binding_exist():
    from uno_amd import _native
    assert hasattr(_native.lib(), "uno_rel_l2_steps_backward") and callable(_native.rel_l2_steps_backward)


@pytest.mark.parametrize("shape", range(4), ids=SHAPE_IDS)
def test_forward_fields_equal_step_errors_bit_for_bit(shape):
    from uno_amd.harness import step_errors
    pred, target, _, _ = problem(shapes()[shape])
    p, y = pred.to(dev()), target.to(dev())
    r = step_losses(p.requires_grad_(True), y)
    assert same_bits(r, step_errors(p.detach(), y))
    assert r.full_sum.requires_grad and r.step_sum.requires_grad
    assert not r.sums.requires_grad and not r.per_step.requires_grad and not r.full.requires_grad


@pytest.mark.parametrize("ab", COMBOS, ids=lambda c: f"{c[0]}_{c[1]}")
@pytest.mark.parametrize("shape", range(4), ids=SHAPE_IDS)
def test_gradient_against_float64_autograd(shape, ab):
    shape = shapes()[shape]
    pred, target, g_full, g_step = problem(shape)
    a, b = ab
    got = grad_of(pred.to(dev()), target.to(dev()), a, b)
    e = rel_err(got.double().cpu().numpy(), (a * g_full + b * g_step).numpy())
    print(f"[step_losses {shape} a={a} b={b}] gradient relative error {e:.2e}")
    assert got.shape == pred.shape and e <= TOL_GRAD


@pytest.mark.parametrize("ab", COMBOS, ids=lambda c: f"{c[0]}_{c[1]}")
@pytest.mark.parametrize("shape", [(2, 100, 5), (2, 100, 8)], ids=["2x100x5", "2x100x8"])
def test_gradient_of_views_with_a_base_that_is_not_16_byte_aligned(shape, ab):
    pred, target, g_full, g_step = problem(shape)
    a, b = ab
    p, y = unaligned(pred), unaligned(target)
    got = grad_of(p, y, a, b)
    e = rel_err(got.double().cpu().numpy(), (a * g_full + b * g_step).numpy())
    print(f"[step_losses unaligned {shape} a={a} b={b}] gradient relative error {e:.2e}")
    assert e <= TOL_GRAD
    assert torch.equal(got, grad_of(pred.to(dev()), target.to(dev()), a, b))      # every element is one product: the path does not matter


def test_a_slice_with_pred_equal_to_target_has_a_finite_gradient_and_no_step_term():
    shape = (2, 33, 3)
    pred, target, g_full, g_step = problem(shape, equal_slice=(0, 1))
    p, y = pred.to(dev()), target.to(dev())
    gs = grad_of(p, y, 0.0, 1.0)
    assert torch.isfinite(gs).all() and float(gs[0, :, 1].abs().max()) == 0.0
    gb = grad_of(p, y, 0.7, -1.3)
    assert torch.isfinite(gb).all()
    assert rel_err(gs.double().cpu().numpy(), g_step.numpy()) <= TOL_GRAD
    assert rel_err(gb.double().cpu().numpy(), (0.7 * g_full - 1.3 * g_step).numpy()) <= TOL_GRAD
    # all of a batch entry equal: both terms vanish there, nothing is NaN
    q = p.clone()
    q[1] = y[1]
    gz = grad_of(q, y, 0.7, -1.3)
    assert torch.isfinite(gz).all() and float(gz[1].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [1, 3], ids=["3x1024x20", "2xPstarx256"])
def test_two_calls_reserved_cus_and_a_graph_replay_give_the_same_bits(shape):
    from uno_amd import _native
    shape = shapes()[shape]
    pred, target, _, _ = problem(shape)
    p, y = pred.to(dev()), target.to(dev())
    first = grad_of(p, y, 0.7, -1.3)
    assert torch.equal(first, grad_of(p, y, 0.7, -1.3))
    prev = _native.reserve_cus(200)
    try:
        under = grad_of(p, y, 0.7, -1.3)
    finally:
        _native.reserve_cus(prev)
    assert torch.equal(first, under)
    # capture forward + backward on other values, replay on these
    sp, sy = (p * 0.5).requires_grad_(True), (y * 2.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = step_losses(sp, sy)
        (0.7 * r.full_sum - 1.3 * r.step_sum).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    sp.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = step_losses(sp, sy)
        (0.7 * r.full_sum - 1.3 * r.step_sum).backward()
    with torch.no_grad():
        sp.copy_(p)
        sy.copy_(y)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, sp.grad)


@pytest.mark.parametrize("shape", [(4, 65536, 12), (4, 70000, 5)], ids=["4x65536x12", "4x70000x5"])
def test_the_grid_stride_loop_and_a_launch_of_another_size(shape):
    """Shapes with more work than the launch has workgroups for: the kernel takes ceil(8 * usable CUs / B) workgroups per batch entry,
    at most ceil(P * T / (256 * lane width)) - 512 against 768 (16-byte lanes) / 1368 (4-byte lanes) on the 256 CUs of an MI355X, so
    the lower threads walk twice and `t` advances by (stride mod T) with its wrap; with 200 CUs reserved the launch has 112
    workgroups per entry and every thread walks 6 to 13 times.  Both against float64 and against each other bit for bit."""
    from uno_amd import _native
    B, P, T = shape
    lanes = 4 if T % 4 == 0 else 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert B * -(-P * T // (256 * lanes)) > 8 * cus, "the shape no longer exceeds the launch: the loop would run once"
    pred, target, g_full, g_step = problem(shape)
    p, y = pred.to(dev()), target.to(dev())
    want = (0.7 * g_full - 1.3 * g_step).numpy()
    plain = grad_of(p, y, 0.7, -1.3)
    e = rel_err(plain.double().cpu().numpy(), want)
    print(f"[step_losses {shape}] gradient relative error {e:.2e}")
    assert e <= TOL_GRAD
    prev = _native.reserve_cus(200)
    try:
        under = grad_of(p, y, 0.7, -1.3)
    finally:
        _native.reserve_cus(prev)
    assert torch.equal(plain, under)
    assert rel_err(under.double().cpu().numpy(), want) <= TOL_GRAD


@pytest.mark.parametrize("shape", range(4), ids=SHAPE_IDS)
def test_gx_is_written_completely_and_nothing_beside_it(shape, monkeypatch):
    """gx sits between two poisoned guard bands (tests/test_hip_redzone.py) and starts out as NaN: afterwards every element is finite
    and the bands are untouched"""
    from test_hip_redzone import RedZone
    shape = shapes()[shape]
    pred, target, g_full, g_step = problem(shape)
    p, y = pred.to(dev()).requires_grad_(True), target.to(dev())
    r = step_losses(p, y)
    zone = RedZone(monkeypatch)
    guarded = torch.empty_like
    filled = []

    def empty_like_nan(t, **kw):
        out = guarded(t, **kw)
        if out.is_floating_point():
            out.fill_(float("nan"))
            filled.append(out)
        return out

    monkeypatch.setattr(torch, "empty_like", empty_like_nan)
    gx, = torch.autograd.grad(0.7 * r.full_sum - 1.3 * r.step_sum, p)
    assert zone.check(f"step_losses backward {shape}") >= 1
    assert any(f.data_ptr() == gx.data_ptr() for f in filled), "gx did not come from the guarded, NaN-filled allocation"
    assert torch.isfinite(gx).all()
    assert rel_err(gx.double().cpu().numpy(), (0.7 * g_full - 1.3 * g_step).numpy()) <= TOL_GRAD


def test_binding_refuses_what_the_kernel_does_not_take():
    from uno_amd import _native
    x = torch.zeros(2, 10, 4, device=dev())
    sums = torch.ones(2, 4, 2, device=dev())
    one = torch.ones(1, device=dev())
    for bad in (x.double(), x[:, ::2], x[..., :3], x.cpu()):
        with pytest.raises(RuntimeError):
            _native.rel_l2_steps_backward(x, bad, sums, one, one)
    with pytest.raises(RuntimeError):
        _native.rel_l2_steps_backward(x, x, sums[:, :3], one, one)
    with pytest.raises(RuntimeError):
        _native.rel_l2_steps_backward(x, x, sums, torch.ones(2, device=dev()), one)
    assert float(_native.rel_l2_steps_backward(x + 1, x, sums, None, None).abs().max()) == 0.0        # NULL, NULL: a zero gradient


@functools.lru_cache(maxsize=None)
def small_model():
    from uno_amd.harness import Uno3D_T20
    torch.manual_seed(31)
    model = Uno3D_T20(6, 2, pad=3).to(dev())
    g = torch.Generator().manual_seed(131)
    x, y = torch.randn(2, 32, 32, 10, 1, generator=g).to(dev()), torch.randn(2, 32, 32, 20, generator=g).to(dev())
    return model, x, y


def test_ns3d_loss_native_equals_the_default_path():
    from uno_amd.harness import ns3d_loss
    model, x, y = small_model()
    loss_d, step_d = ns3d_loss(model, x, y, with_step_error=True)
    loss_n, step_n = ns3d_loss(model, x, y, with_step_error=True, native=True)
    assert loss_n.requires_grad and not step_n.requires_grad
    loss_d, loss_n = loss_d.detach(), loss_n.detach()
    print(f"[ns3d_loss] default {float(loss_d):.8g} / {float(step_d):.8g}, native {float(loss_n):.8g} / {float(step_n):.8g}")
    assert abs(float(loss_n) - float(loss_d)) <= 1e-5 * abs(float(loss_d))
    assert abs(float(step_n) - float(step_d)) <= 1e-5 * abs(float(step_d))
    assert float(ns3d_loss(model, x, y, native=True).detach()) == float(loss_n)


def test_ns3d_loss_native_costs_three_library_launches():
    """forward and backward of the model are the same launches on both paths; the native loss adds exactly K17's two and K17-B's one
    (the default path's loss is stock ops: no library launch)"""
    from uno_amd import _native
    from uno_amd.harness import ns3d_loss
    model, x, y = small_model()

    def launches(native):
        model.zero_grad(set_to_none=True)
        ns3d_loss(model, x, y, native=native).backward()         # (a first pass outside the profile: one-time set-up launches)
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        _native.profile_begin()
        try:
            ns3d_loss(model, x, y, native=native).backward()
            torch.cuda.synchronize()
        finally:
            names = [n for n, _, _ in _native.profile_end()]
        model.zero_grad(set_to_none=True)
        return names

    default, native = launches(False), launches(True)
    loss = [n for n in native if "rel_l2" in n]
    assert sorted(loss) == sorted(["uno::rel_l2_steps_partial_kernel", "uno::rel_l2_steps_finish_kernel", "uno::rel_l2_steps_backward_kernel"]), loss
    assert not [n for n in default if "rel_l2" in n]
    assert len(native) == len(default) + 3
