"""Parity of the HEADLINE workload at the geometry bench.py times it: UNO_9(3, 64, pad=5) on 421 x 421 Darcy fields, batch 16 (BASELINE.json
configs[1]; reference darcy_flow_uno2d.py:94-133, train_darcy.py:47-56, Adam.py:27-52).  pytest -m gpu

About 75 % of the timed step runs in the point-wise kernels (K7 resampling, K8 / K9 channel mixing, K11-K13 element-wise ends); the
shape-class tests elsewhere compare them with float64 references at small shapes.  "A variant can be wrong only at the geometry a
benchmark dispatches it with" (tests/test_hip_bench_shapes.py) holds for them too, so here
  * the whole model runs forward + loss + backward at S = 421, batch 16, width 64 on the product kernels and on the oracle's blocks
    (the reference's op sequence on the host, pinned by the goldens) with the same weights: prediction, loss and EVERY parameter
    gradient at 1e-4 - every kernel of the step at its bench geometry inside one oracle comparison;
  * each operator block of the model (conv0, conv1, conv2, conv4; conv5 is in test_hip_bench_shapes.py) and the model's lift / projection
    ends are compared on their own at batch 16, so that a failure names the layer;
  * the optimiser runs over the model's 65 M parameters against the oracle's restatement of the reference Adam;
  * the last test reads the committed bench line and fails if its per-kernel table of the training step (roofline.step_kernels) names a
    kernel that none of these comparisons launched.
Tolerances: blocks 5e-5 (as in test_hip_bench_shapes.py), whole model 1e-4 (five blocks, two InstanceNorms, measured ~3e-6)."""
import glob
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_err
from oracle import spectral_oracle as so

pytestmark = pytest.mark.gpu
S, B, WIDTH, D = 421, 16, 64, 446
RAN = set()              # every library kernel INSTANTIATION (template arguments kept) launched inside an oracle-compared call of this module


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _profiled(fn, record=True):
    """record=True: the kernels fn launches count as oracle-checked (RAN), fn's result is returned; record=False: their names are returned"""
    from uno_amd import _native
    _native.profile_begin(8192)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        names = [n for n, _, _ in _native.profile_end()]
    if not record:
        return names
    RAN.update(n.replace("uno::", "") for n in names)
    return out


def _assert_grads(prod, ref, tol, skip=()):
    pr = dict(ref.named_parameters())
    gmax = max(float(torch.linalg.vector_norm(q.grad)) for q in pr.values() if q.grad is not None)
    worst = ("", 0.0)
    for k, p in prod.named_parameters():
        if k in skip:
            continue
        g, gr = p.grad.cpu(), pr[k].grad
        n = float(torch.linalg.vector_norm(gr))
        err = float(torch.linalg.vector_norm(g - gr))
        if err / max(n, 1e-30) > worst[1]:
            worst = (k, err / max(n, 1e-30))
        assert err <= tol * n + 1e-6 * gmax, (k, err / max(n, 1e-30))
    return worst


def test_headline_model_full_size_matches_oracle():
    from uno_amd.harness import UNO_9, lp_loss_rel_sum, synthetic_darcy_batch
    torch.manual_seed(0)
    ref = UNO_9(3, WIDTH, pad=5, block_cls=so.OracleOperatorBlock2d)
    prod = UNO_9(3, WIDTH, pad=5)
    prod.load_state_dict(ref.state_dict(), strict=True)
    prod = prod.to(dev())
    a, u = synthetic_darcy_batch(B, S, 1234, "cpu")              # bench.py's batch
    out_ref = ref(a)
    loss_ref = lp_loss_rel_sum(out_ref.reshape(B, -1), u.reshape(B, -1))
    loss_ref.backward()

    def run():
        out = prod(a.to(dev()))
        loss = lp_loss_rel_sum(out.reshape(B, -1), u.to(dev()).reshape(B, -1))
        loss.backward()
        return out, loss
    out, loss = _profiled(run)
    assert rel_err(out.detach().cpu().numpy(), out_ref.detach().numpy()) < 1e-4
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * abs(float(loss_ref))
    # (the 1x1-convolution biases in front of an InstanceNorm have a true gradient of exactly zero: both sides hold rounding residue)
    worst = _assert_grads(prod, ref, 1e-4, skip=("conv1.w.conv.bias", "conv4.w.conv.bias"))
    print("worst parameter gradient:", worst)
    # second pass from the same weights (gradients cleared: in-place gradient targets and cached plans are what runs now), then one
    # step driven as the workload drives it (DarcyTrainer: flat gradient buffer, bucket hooks, optimiser) - the optimiser runs
    # AFTER that backward pass, so the gradients left in .grad still belong to the weights the oracle was evaluated at
    from uno_amd.harness import DarcyTrainer
    for prm in prod.parameters():
        prm.grad = None
    out, loss = _profiled(run)
    assert rel_err(out.detach().cpu().numpy(), out_ref.detach().numpy()) < 1e-4
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * abs(float(loss_ref))
    print("second pass:", _assert_grads(prod, ref, 1e-4, skip=("conv1.w.conv.bias", "conv4.w.conv.bias")))
    tr = DarcyTrainer(prod, lr=1e-3, weight_decay=1e-3)
    ad, ud = a.to(dev()), u.to(dev())
    loss = _profiled(lambda: tr.step(ad, ud))
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * abs(float(loss_ref))
    print("trainer-driven step:", _assert_grads(prod, ref, 1e-4, skip=("conv1.w.conv.bias", "conv4.w.conv.bias")))


BLOCKS = {      # name: (Ci, Co, H -> Ho, modes, Normalize) of darcy_flow_uno2d.py:108-116 at width 64, padded grid 446
    "conv0": (64, 128, D, D // 2, 18, False), "conv1": (128, 256, D // 2, D // 4, 8, True),
    "conv2": (256, 256, D // 4, D // 4, 8, False), "conv4": (256, 128, D // 4, D // 2, 8, True),
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_headline_blocks_full_size(name):
    """OperatorBlock_2D forward (spectral + point-wise branch, [InstanceNorm], GELU) and every gradient at batch 16, against the oracle block"""
    from uno_amd.integral_operators import OperatorBlock_2D
    Ci, Co, H, Ho, m, norm = BLOCKS[name]
    torch.manual_seed(len(name) + Ci)
    ob = so.OracleOperatorBlock2d(Ci, Co, Ho, Ho, m, m, Normalize=norm)
    blk = OperatorBlock_2D(Ci, Co, Ho, Ho, m, m, Normalize=norm)
    blk.load_state_dict(ob.state_dict(), strict=True)
    blk = blk.to(dev())
    g = torch.Generator().manual_seed(Ci + Ho)
    x = torch.randn(B, Ci, H, H, generator=g)
    gy = torch.randn(B, Co, Ho, Ho, generator=g)
    xr = x.clone().requires_grad_(True)
    y_ref = ob(xr, Ho, Ho)
    y_ref.backward(gy)
    xd = x.to(dev()).requires_grad_(True)

    def run():
        y = blk(xd, Ho, Ho)
        y.backward(gy.to(dev()))
        return y
    y = _profiled(run)
    assert rel_err(y.detach().cpu().numpy(), y_ref.detach().numpy()) < 5e-5
    assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) < 5e-5
    _assert_grads(blk, ob, 5e-5, skip=("w.conv.bias",) if norm else ())


def test_headline_lift_and_projection_ends_full_size():
    """fc0(gelu(fc_n1(x))) -> gelu -> domain padding, and fc2(gelu(fc1(cat([gelu(pre), lifted])))) (reference darcy_flow_uno2d.py:94-107,
    122-131) at batch 16 on the 421 / 446 grids, against the stock ops on the host in FLOAT64 (the weight gradients are sums over 2.8 M
    pixels: a float32 reference would carry more summation error than the kernels do)"""
    from uno_amd.integral_operators import channel_mix, channel_mix_cat_project, gelu_channel_mix, gelu_pad2d
    torch.manual_seed(7)
    fc_n1, fc0 = torch.nn.Linear(3, WIDTH // 2).double(), torch.nn.Linear(WIDTH // 2, WIDTH).double()
    fc1, fc2 = torch.nn.Linear(2 * WIDTH, WIDTH).double(), torch.nn.Linear(WIDTH, 1).double()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, S, S, 3, generator=g)
    # ---- lift (channels-last reference, channels-first product)
    xr = x.double().requires_grad_(True)
    lifted_ref = F.pad(F.gelu(fc0(F.gelu(fc_n1(xr)))).permute(0, 3, 1, 2), [0, D - S, 0, D - S])
    gl = torch.randn(B, WIDTH, D, D, generator=g)
    lifted_ref.backward(gl.double())
    mods = [m_.to(dev()) for m_ in (torch.nn.Linear(3, WIDTH // 2), torch.nn.Linear(WIDTH // 2, WIDTH))]
    for dst, src in zip(mods, (fc_n1, fc0)):
        dst.load_state_dict({k: v.float() for k, v in src.state_dict().items()})
    xd = x.permute(0, 3, 1, 2).contiguous().to(dev()).requires_grad_(True)

    def run_lift():
        lifted = gelu_pad2d(gelu_channel_mix(channel_mix(xd, mods[0].weight, mods[0].bias), mods[1].weight, mods[1].bias), D - S, D - S)
        lifted.backward(gl.to(dev()))
        return lifted
    lifted = _profiled(run_lift)
    assert rel_err(lifted.detach().cpu().numpy(), lifted_ref.detach().numpy()) < 2e-5
    assert rel_err(xd.grad.permute(0, 2, 3, 1).cpu().numpy(), xr.grad.numpy()) < 2e-5
    for dst, src in zip(mods, (fc_n1, fc0)):
        assert rel_err(dst.weight.grad.cpu().numpy(), src.weight.grad.numpy()) < 2e-5
        assert rel_err(dst.bias.grad.cpu().numpy(), src.bias.grad.numpy()) < 2e-5
    # ---- projection end: pre-activation block output + skip tensor -> fc1 -> gelu -> fc2 (one output channel)
    pre = torch.randn(B, WIDTH, D, D, generator=g)
    skip = torch.randn(B, WIDTH, D, D, generator=g)
    gout = torch.randn(B, 1, D, D, generator=g)
    pr, sr = pre.double().requires_grad_(True), skip.double().requires_grad_(True)
    cat = torch.cat([F.gelu(pr), sr], dim=1).permute(0, 2, 3, 1)
    out_ref = fc2(F.gelu(fc1(cat))).permute(0, 3, 1, 2)
    out_ref.backward(gout.double())
    tail = [m_.to(dev()) for m_ in (torch.nn.Linear(2 * WIDTH, WIDTH), torch.nn.Linear(WIDTH, 1))]
    for dst, src in zip(tail, (fc1, fc2)):
        dst.load_state_dict({k: v.float() for k, v in src.state_dict().items()})
    pd, sd = pre.to(dev()).requires_grad_(True), skip.to(dev()).requires_grad_(True)

    def run_tail():
        out = channel_mix_cat_project([pd, sd], tail[0].weight, tail[0].bias, tail[1].weight, tail[1].bias, gelu_first=True)
        out.backward(gout.to(dev()))
        return out
    out = _profiled(run_tail)
    assert rel_err(out.detach().cpu().numpy(), out_ref.detach().numpy()) < 2e-5
    assert rel_err(pd.grad.cpu().numpy(), pr.grad.numpy()) < 2e-5 and rel_err(sd.grad.cpu().numpy(), sr.grad.numpy()) < 2e-5
    for dst, src in zip(tail, (fc1, fc2)):
        assert rel_err(dst.weight.grad.cpu().numpy(), src.weight.grad.numpy()) < 2e-5
        assert rel_err(dst.bias.grad.cpu().numpy(), src.bias.grad.numpy()) < 2e-5


def test_headline_optimiser_full_size():
    """ComplexAdam over the parameter set of UNO_9(3, 64) (65 M real-equivalent values, complex-modulus second moment, coupled L2): two
    steps against the oracle's restatement of reference Adam.py:27-52"""
    from uno_amd.harness import ComplexAdam, UNO_9
    torch.manual_seed(1)
    model = UNO_9(3, WIDTH, pad=5)
    g = torch.Generator().manual_seed(2)
    params = [p.detach().clone() for p in model.parameters()]
    grads = [[torch.randn(p.shape, dtype=p.dtype, generator=g) * 0.1 for p in params] for _ in range(2)]
    ref_p = [p.clone() for p in params]
    m_ = [torch.zeros_like(p) for p in params]
    v_ = [torch.zeros_like(p) for p in params]
    for step in (1, 2):
        so.reference_adam_step(ref_p, grads[step - 1], m_, v_, step, 1e-3, 0.9, 0.999, 1e-8, 1e-3)
    dp = [torch.nn.Parameter(p.clone().to(dev())) for p in params]
    opt = ComplexAdam(dp, lr=1e-3, weight_decay=1e-3)

    def run():
        for step in (0, 1):
            for p, gr in zip(dp, grads[step]):
                p.grad = gr.to(dev())
            opt.step()
    _profiled(run)
    for p, r in zip(dp, ref_p):
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (p.detach().cpu(), r))
        assert float((a - b).norm()) <= 1e-6 * float(b.norm()) + 1e-9


def test_headline_gradients_are_bit_reproducible_launch_to_launch():
    """forward + loss + backward of the headline model at batch 16, eight times from the same weights and batch: every parameter gradient
    bit for bit (fixed-order reductions everywhere; round 6 found one packed accumulation that lost terms in one launch of four - a
    failure mode an oracle comparison at 1e-4 can miss)"""
    from uno_amd.harness import UNO_9, lp_loss_rel_sum, synthetic_darcy_batch
    torch.manual_seed(0)
    model = UNO_9(3, WIDTH, pad=5).to(dev())
    a, u = synthetic_darcy_batch(B, S, 99, dev())
    ref = None
    for it in range(8):
        for prm in model.parameters():
            prm.grad = None
        out = model(a)
        lp_loss_rel_sum(out.reshape(B, -1), u.reshape(B, -1)).backward()
        grads = [prm.grad.clone() for prm in model.parameters()]
        if ref is None:
            ref = grads
        else:
            for k, (g0, g1) in enumerate(zip(ref, grads)):
                assert torch.equal(torch.view_as_real(g0) if g0.is_complex() else g0, torch.view_as_real(g1) if g1.is_complex() else g1), (it, k)


def test_zz_every_kernel_of_the_timed_step_was_oracle_checked_at_bench_geometry():
    """The kernel instantiations of the headline step (full names: an accumulating or second-step form does not pass as covered by a
    sibling instantiation) - taken from the library's launch records of two steps of the workload run HERE, at the bench geometry
    (not from a committed profile) - all ran inside a full-size oracle comparison of this module."""
    if len(RAN) < 10:
        pytest.skip("the full-size parity tests of this module did not run in this session")
    from uno_amd.harness import workloads
    w = workloads.build("c2", dev())
    w.step()
    names = _profiled(lambda: (w.step(), w.step()), record=False)
    named = {k.replace("uno::", "") for k in names}
    missing = sorted(named - RAN)
    assert not missing, f"the timed step launches kernels no full-size oracle comparison launched: {missing}"
