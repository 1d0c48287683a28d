"""The checks that the harness-model tests share (tests/test_harness_ns.py, test_harness_ns2d_models.py, test_harness_ns3d_models.py,
test_hip_ns3d_models.py), each said once.  `c` is a conftest.Case of a reference-generated golden file."""
import numpy as np
import torch


def check_init(model, c):
    """The constructor reproduced the reference's seeded initialisation bit for bit (per-parameter float64 checksums) and, where the
    case carries them, the reference's ordered state_dict keys and shapes."""
    # float64 sums on both sides: a float32 sum over the large 3-D weights depends on the host's thread count
    for k, p in model.named_parameters():
        ck = getattr(c, f"ck64.{k}")
        q = p.detach().to(torch.complex128 if p.is_complex() else torch.float64)
        got = np.array([float(q.abs().sum()), float(torch.linalg.vector_norm(q))])
        assert np.allclose(got, ck, rtol=1e-12), f"seeded init of {k} differs from the reference's"
    if hasattr(c, "sd_keys"):
        sd = model.state_dict()
        assert list(sd.keys()) == [str(k) for k in c.sd_keys]
        for v, row in zip(sd.values(), c.sd_shapes):
            assert list(v.shape) == [int(d) for d in row if d >= 0]


def check_strict_load(model, c, rebuild):
    """a state dict built from the reference's key / shape list loads with strict=True into `rebuild()`, a second instance of the
    model, and is what that instance then holds"""
    g = torch.Generator().manual_seed(3)
    ref = model.state_dict()
    sd = {str(k): torch.randn(*[int(d) for d in row if d >= 0], generator=g).to(ref[str(k)].dtype) for k, row in zip(c.sd_keys, c.sd_shapes)}
    twin = rebuild()
    res = twin.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in twin.state_dict().items():
        assert torch.equal(v, sd[k]), k


def check_grads(model, c, rtol):
    gmax = max(float(getattr(c, f"gradnorm.{k}")) for k, _ in model.named_parameters())
    for k, p in model.named_parameters():
        ref = float(getattr(c, f"gradnorm.{k}"))
        got = float(torch.linalg.vector_norm(p.grad))
        assert abs(got - ref) <= rtol * ref + 1e-5 * gmax, (k, got, ref)


def assert_graphed_step_equals_eager(make, loss_fn, batches, capturable=False):
    """harness.GraphedStep: forward + loss + backward (+ the optimiser update where `capturable`) replayed from a HIP graph give the
    eager step's loss, gradients and updated parameters bit for bit (every kernel is deterministic), for every batch through one
    capture.  make(capturable) -> (model, optimiser) from a fixed seed; loss_fn(model, x, y) -> loss.  Returns the GraphedStep and
    the graphed model's optimiser."""
    from uno_amd.harness import GraphedStep
    me, oe = make(False)
    mg, og = make(capturable)
    gs = GraphedStep(mg, og, lambda a, b: loss_fn(mg, a, b), batches[0])
    # the eager model's first backward pass is set-up too: it runs the spectral weight gradients use by use and only the later ones
    # batch them over the roll-out (_param_grads.TIME_BATCHED_WGRAD) - the capture's warm-up passes have put the graphed model in
    # that mode
    loss_fn(me, *batches[0]).backward()
    for xx, yy in batches:
        oe.zero_grad(set_to_none=True)
        le = loss_fn(me, xx, yy)
        le.backward()
        ge = {k: p.grad.clone() for k, p in me.named_parameters()}
        oe.step()
        lg = gs.step(xx, yy)
        assert float(lg) == float(le)
        for (k, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
            assert torch.equal(ge[k], pg.grad), k
            assert torch.equal(pe, pg), k
    return gs, og
