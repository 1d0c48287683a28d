"""harness.ns2d_rollout_loss(native=True) on the host: the three autograd Functions of the window-free training roll-out run on their
stock-op restatements (no device), so what is tested here is the STRUCTURE - which frames a window reads, where each predicted
frame's gradient is accumulated, the reverse step order the accumulation relies on, the one weight-gradient finish, the loss term of
every frame - against the stock loop (`native=False`, the reference's ns_train_2d.py:46-62 written out).

Bound 1e-9 relative in float64: the two paths differ only in the summation order of <= 1e5 float64 terms (about 1e-11); a structural
mistake is O(1).  The golden case keeps the bounds of tests/test_harness_ns.py::_ns2d (loss 1e-5, gradient norms 5e-4)."""
import pytest
import torch
import torch.nn as nn

from conftest import Case, load_cases
from harness_checks import check_grads, check_init
from oracle import spectral_oracle as so
from uno_amd.harness import UNO, UNO_P, ns2d_rollout_loss
from uno_amd.integral_operators import channel_mix

TOL = 1e-9


class Toy(nn.Module):
    """fc + the prototype's body im = (tanh(h) . a).sum(1); features: F seeded planes, the same for every batch entry"""

    def __init__(self, T_in, F, Cm):
        super().__init__()
        self.fc = nn.Linear(T_in + F, Cm)
        self.a = nn.Parameter(torch.randn(Cm))
        self.F = F

    def get_grid(self, shape, device):
        g = torch.Generator().manual_seed(77)
        return torch.randn(1, shape[1], shape[2], self.F, generator=g, dtype=torch.float64).expand(shape[0], -1, -1, -1).to(device)

    def body_cf(self, h):
        return (torch.tanh(h) * self.a.view(1, -1, 1, 1)).sum(1, keepdim=True)

    def forward_cf(self, x):
        return self.body_cf(channel_mix(x, self.fc.weight, self.fc.bias))


def rel(a, b):
    return float((a - b).norm() / b.norm())


def both_paths(model, xx, yy, T_f, scale=1.0):
    """-> [(loss, {name: grad})] of the stock loop and of the native path"""
    out = []
    for native in (False, True):
        model.zero_grad(set_to_none=True)
        loss = ns2d_rollout_loss(model, xx, yy, T_f, step=1, native=native)
        (scale * loss).backward()
        out.append((loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    return out


def assert_same(stock, native, tol=TOL):
    (l0, g0), (l1, g1) = stock, native
    assert abs(float(l1) - float(l0)) <= tol * abs(float(l0))
    assert sorted(g0) == sorted(g1)
    worst = max(rel(g1[k], g0[k]) for k in g0)
    print(f"loss {abs(float(l1) - float(l0)) / abs(float(l0)):.2e}, worst gradient {worst:.2e}")
    for k in g0:
        assert rel(g1[k], g0[k]) <= tol, k


@pytest.mark.parametrize("B,T_in,F,Cm,P,T_f,scale", [(2, 3, 2, 5, 37, 8, 1.0), (2, 3, 2, 5, 37, 8, 3.0), (2, 1, 0, 4, 11, 5, 1.0), (1, 4, 1, 3, 6, 1, 1.0),
                                                      (2, 3, 2, 5, 12, 3, 1.0)])
def test_toy_body_native_equals_stock_loop(B, T_in, F, Cm, P, T_f, scale):
    """T_f > T_in (windows that are all given, straddling and all predicted), the loss scaled before backward (gL != 1), T_in = 1 with
    no features, one step, and T_f = T_in"""
    torch.manual_seed(3)
    model = Toy(T_in, F, Cm).double()
    xx, yy = torch.randn(B, P, 1, T_in, dtype=torch.float64), torch.randn(B, P, 1, T_f + 1, dtype=torch.float64)
    assert_same(*both_paths(model, xx, yy, T_f, scale))


@pytest.mark.parametrize("cls", [UNO, UNO_P])
def test_uno_models_native_equals_default_float64(cls):
    """UNO(14, 4) and UNO_P(14, 4) (whose h also feeds the two-source projection: autograd sums two gh) on oracle blocks in float64,
    batch 1, T_f = 3.  At 64^2: the models keep 22 / 14 modes per corner on their first level's grid, which 32^2 and 48^2 do not hold
    (the stock loop raises there too); one pass of both paths takes 0.3 s."""
    torch.manual_seed(11)
    model = so.to_float64(cls(14, 4, block_cls=so.OracleOperatorBlock2d))
    g = torch.Generator().manual_seed(12)
    xx, yy = torch.randn(1, 64, 64, 10, generator=g, dtype=torch.float64), torch.randn(1, 64, 64, 3, generator=g, dtype=torch.float64)
    assert_same(*both_paths(model, xx, yy, 3))


def test_golden_case_native():
    """_ns2d of tests/test_harness_ns.py with native=True: the reference's recorded loss and gradient norms, that test's bounds"""
    Z, _ = load_cases("harness_ns.npz")
    c = Case(Z, "ns2d")
    torch.manual_seed(21)
    model = UNO(14, 4, block_cls=so.OracleOperatorBlock2d)
    check_init(model, c)
    xx, yy = torch.from_numpy(c.xx), torch.from_numpy(c.yy)
    loss = ns2d_rollout_loss(model, xx, yy, T_f=2, step=1, native=True)
    loss.backward()
    assert abs(float(loss.detach()) - float(c.loss)) < 1e-5 * abs(float(c.loss))
    check_grads(model, c, 5e-4)


def test_second_pass_on_fresh_state_gives_the_same_bits():
    torch.manual_seed(3)
    model = Toy(3, 2, 5).double()
    xx, yy = torch.randn(2, 37, 1, 3, dtype=torch.float64), torch.randn(2, 37, 1, 8, dtype=torch.float64)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        loss = ns2d_rollout_loss(model, xx, yy, 8, native=True)
        loss.backward()
        runs.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_native_refuses_what_it_does_not_cover():
    torch.manual_seed(3)
    model = Toy(3, 2, 5).double()
    xx = torch.randn(2, 6, 1, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="step == 1"):
        ns2d_rollout_loss(model, xx, torch.randn(2, 6, 1, 4, dtype=torch.float64), 4, step=2, native=True)
    with pytest.raises(RuntimeError, match="T_f <= 256"):
        ns2d_rollout_loss(model, xx, torch.randn(2, 6, 1, 257, dtype=torch.float64), 257, native=True)

    class NoBody(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(3, 2)

        def forward(self, x):
            return self.fc(x).sum(-1, keepdim=True)

    with pytest.raises(RuntimeError, match="body_cf"):
        ns2d_rollout_loss(NoBody().double(), xx, torch.randn(2, 6, 1, 4, dtype=torch.float64), 2, native=True)
    # more input channels than the lift kernel keeps in registers
    wide = Toy(30, 3, 5).double()
    with pytest.raises(RuntimeError, match="<= 32"):
        ns2d_rollout_loss(wide, torch.randn(1, 6, 1, 30, dtype=torch.float64), torch.randn(1, 6, 1, 2, dtype=torch.float64), 2, native=True)


@pytest.mark.parametrize("cls", [UNO, UNO_P])
def test_forward_cf_is_body_cf_of_the_lift_bit_for_bit(cls):
    torch.manual_seed(4)
    model = cls(14, 4, block_cls=so.OracleOperatorBlock2d)
    x = torch.randn(2, 14, 64, 64)                      # (the smallest grid that holds the models' modes)
    with torch.no_grad():
        assert torch.equal(model.forward_cf(x), model.body_cf(channel_mix(x, model.fc.weight, model.fc.bias)))


def test_zero_difference_slice_gives_a_zero_loss_gradient():
    """pred == target at one (b, t): ||d|| = 0 there; the loss term of that frame is 0 (torch.linalg.vector_norm's backward), not NaN"""
    from uno_amd.harness.train import _RolloutTrain
    torch.manual_seed(3)
    model = Toy(2, 1, 3).double()
    xx, yy = torch.randn(2, 5, 1, 2, dtype=torch.float64), torch.randn(2, 5, 1, 3, dtype=torch.float64)
    st = _RolloutTrain(model, xx, yy, 3)
    for t in range(3):
        st.record_frame(torch.randn(2, 1, 5, 1, dtype=torch.float64), t)
    st.pred[1, 2] = st.target[1, 2]                     # the last frame of batch entry 1
    st.pred[0, 1] = st.target[0, 1]
    loss = st.finish()
    assert torch.isfinite(loss)
    g_last = st.seed(torch.ones((), dtype=torch.float64))
    assert torch.isfinite(g_last).all() and float(g_last[1].abs().max()) == 0.0 and float(g_last[0].abs().max()) > 0.0
    gh = torch.zeros(2, 3, 5, 1, dtype=torch.float64)   # no gradient through the lift: what is left is the loss term of frame 1
    g1 = st.lift_backward(gh, model.fc.weight.detach(), 2)
    assert torch.isfinite(g1).all() and float(g1[0].abs().max()) == 0.0 and float(g1[1].abs().max()) > 0.0
    # and the whole path agrees with the stock loop's gradient where a slice matches exactly: a model whose output is the target
    want = torch.autograd.functional.jacobian(lambda p: torch.linalg.vector_norm(p - yy[1, :, :, 2].reshape(-1)), yy[1, :, :, 2].reshape(-1).clone())
    assert float(want.abs().max()) == 0.0
