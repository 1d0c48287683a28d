"""`Uno3D_T10` / `Uno3D_T9` on the product blocks and the NS-3D loop's error metric on the MI355X, against the reference-generated goldens
of tests/test_harness_ns3d_models.py (whose helpers these tests share).  pytest -m gpu

Bounds: 1e-4 for prediction and loss, 2e-4 for the gradient norms - those of test_ns3d_gpu_product (tests/test_harness_ns.py, where
they are derived); 1e-4 for the metric, a sum of ratios of norms of that prediction."""
import pytest
import torch

from harness_checks import assert_graphed_step_equals_eager
from test_harness_ns3d_models import CASES, build, parity
from uno_amd.harness import Uno3D_T10, ns3d_evaluate, ns3d_loss, ns3d_step_error

pytestmark = pytest.mark.gpu
TOL_PRED, TOL_GRAD = 1e-4, 2e-4


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_product(name):
    parity(name, None, dev(), TOL_PRED, TOL_GRAD)


@pytest.mark.parametrize("name", list(CASES))
def test_loss_with_step_error_against_the_reference_metric(name):
    c, model, T_f = build(name, None)
    model = model.to(dev())
    xx, yy = torch.from_numpy(c.xx).to(dev()), torch.from_numpy(c.yy).to(dev())
    plain = ns3d_loss(model, xx, yy)
    loss, err = ns3d_loss(model, xx, yy, with_step_error=True)
    assert torch.equal(plain.detach(), loss.detach()) and loss.requires_grad
    assert err.is_cuda and err.dim() == 0 and not err.requires_grad
    e = abs(float(err) - float(c.step_err64)) / float(c.step_err64)
    print(f"[{name}] step error {float(err):.6f}, reference {float(c.step_err64):.6f}: {e:.2e}")
    assert e <= TOL_PRED
    loss.backward()                                 # the metric left the training graph alone
    assert all(p.grad is not None for p in model.parameters())


def test_evaluate_is_the_sum_of_the_per_batch_metrics():
    c, model, T_f = build("t10", None)
    model = model.to(dev()).train()
    xx, yy = torch.from_numpy(c.xx).to(dev()), torch.from_numpy(c.yy).to(dev())
    batches = [(xx[:1].contiguous(), yy[:1].contiguous()), (xx[1:].contiguous(), yy[1:].contiguous())]
    total = ns3d_evaluate(model, batches)
    assert model.training and total.is_cuda and not total.requires_grad
    model.eval()
    with torch.no_grad():
        each = [ns3d_step_error(model(x).view(1, 32, 32, T_f), y) for x, y in batches]
    assert torch.equal(total, each[0] + each[1])
    assert abs(float(total) - float(c.step_err64)) <= TOL_PRED * float(c.step_err64)


def test_graphed_step_equals_eager_step_uno3d_t10():
    """harness.GraphedStep on Uno3D_T10(6, 2, pad=3), S = 32, batch 2, two batches: loss, gradients and updated parameters of the replay
    are bit-equal to the eager step's (the pattern of test_graphed_step_equals_eager_step_uno_p, tests/test_harness_ns2d_models.py)."""
    from uno_amd.harness import ComplexAdam

    def make(cap):
        torch.manual_seed(5)
        m = Uno3D_T10(6, 2, pad=3).to(dev())
        return m, ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(2, 32, 32, 10, 1, generator=g).to(dev()), torch.randn(2, 32, 32, 10, generator=g).to(dev())) for _ in range(2)]
    assert_graphed_step_equals_eager(make, ns3d_loss, batches)
