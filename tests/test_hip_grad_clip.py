"""K26 (csrc/adam.hip: the global gradient norm on the device), the guarded K10 and ComplexAdam(max_grad_norm=, skip_nonfinite=) on the
MI355X; fit_darcy's resume on the device, eager and from a graph.

Bounds.  The norm against the float64 norm of the same float32 gradients at rtol 1e-12: every term is positive and a float's square
is exact in double, so the relative error of the sum is at most (adds along a path) * 2^-53 - 4 in a thread, 6 + 2 across a
workgroup, at most a few across the partials of these sizes and 6 + 4 in stage 2: under 40 roundings, 4e-15 - and the square root
halves it.  Clipped updates against the host path at rel_err < 1e-6, the tolerance of tests/test_hip_adam.py.  Everything else - an
update that never clips, a skipped step, two calls on the same data, replay against eager, a resumed run - bit for bit.

Measured on the MI355X (printed per case): the norm differs from the float64 one by 0 in 16 of the 18 cases and by 1.7e-16, relative,
in the two with 25 tensors."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from uno_amd.harness.optim import ComplexAdam

pytestmark = pytest.mark.gpu


def draw(shapes, cplx, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(*s, dtype=torch.complex64 if c else torch.float32, generator=g) for s, c in zip(shapes, cplx)]


def mixed_60():
    """the 60 shapes of test_adam_multi_tensor_launches_many_mixed_tensors: real and complex, 1 to 70000 entries"""
    rng = np.random.default_rng(12)
    shapes = [tuple(int(v) for v in rng.integers(1, [70000, 300, 40][nd - 1] + 1, size=nd)) for nd in rng.integers(1, 4, size=60)]
    return shapes, [bool(v) for v in rng.integers(0, 2, size=60)]


def at_offset(t):
    """a device copy of t that is a view at float offset 3 (real) or 2 (complex) of a flat buffer: 4-byte alignment only"""
    nflt, off = t.numel() * (2 if t.is_complex() else 1), 2 if t.is_complex() else 3
    seg = torch.zeros(nflt + off + 5, device="cuda")[off:off + nflt]
    view = torch.view_as_complex(seg.view(*t.shape, 2)) if t.is_complex() else seg.view(t.shape)
    view.copy_(t.cuda())
    return view


def norm64(grads):
    return math.sqrt(sum(float((torch.view_as_real(g) if g.is_complex() else g).double().square().sum()) for g in grads))


def device_norm(grads, max_norm=1.0, poison=False, record=None):
    """one uno_grad_norm call -> the record as a list of Python floats"""
    from uno_amd import _native
    plan = _native.GradNormPlan(grads)
    scratch = torch.full((plan.partials + 3,), math.nan if poison else 0.0, dtype=torch.float64, device="cuda")
    state = torch.zeros(_native.GRAD_NORM_RECORD, dtype=torch.float64, device="cuda") if record is None else record
    plan.run(torch.tensor([max_norm], dtype=torch.float64, device="cuda"), True, scratch, state)
    assert plan.partials == sum(-(-g.numel() * (2 if g.is_complex() else 1) // 1024) for g in grads)
    return dict(zip(_native.GRAD_NORM_FIELDS, state.tolist()))


CASES = {
    "1": ([(1,)], [False]), "1023": ([(1023,)], [False]), "1024": ([(1024,)], [False]), "1025": ([(1025,)], [False]),
    "c511": ([(511,)], [True]), "c512": ([(512,)], [True]), "c513": ([(513,)], [True]),
    "25 tensors": ([(1 + 97 * i,) for i in range(25)], [i % 3 == 0 for i in range(25)]),
    "60 mixed": mixed_60(),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("offset", [False, True])
def test_norm_against_float64(name, offset):
    shapes, cplx = CASES[name]
    host = draw(shapes, cplx, 7)
    grads = [at_offset(t) if offset else t.cuda() for t in host]
    ref = norm64(host)
    got = device_norm(grads, max_norm=0.5 * ref)
    print(f"[K26 {name} offset={offset}] norm {got['norm']!r} float64 {ref!r} rel {abs(got['norm'] - ref) / ref:.2e}")
    assert abs(got["norm"] - ref) <= 1e-12 * ref
    assert got["coef"] == float(np.float32(0.5 * ref / (got["norm"] + 1e-6))) and got["finite"] == 1.0
    assert (got["steps"], got["clipped"], got["skipped"], got["nonfinite"]) == (1, 1, 0, 0) and got["sum"] == got["max"] == got["norm"]
    # the same data again, into a scratch full of NaN: the same bits (no atomics; every partial read was written by this call)
    again = device_norm(grads, max_norm=0.5 * ref, poison=True)
    assert again["norm"] == got["norm"] and again["coef"] == got["coef"]


def test_an_all_zero_gradient_and_one_too_large_for_float():
    zero = device_norm([torch.zeros(1025, device="cuda"), torch.zeros(513, dtype=torch.complex64, device="cuda")], max_norm=1.0)
    assert zero["norm"] == 0.0 and zero["coef"] == 1.0 and zero["finite"] == 1.0 and zero["clipped"] == 0
    assert not any(math.isnan(v) for v in zero.values())
    # 1e25 in every entry: a float sum of squares overflows; the double one does not - clipped, not skipped
    p = torch.nn.Parameter(torch.ones(1025, device="cuda"))
    opt = ComplexAdam([p], lr=1e-2, max_grad_norm=1.0)
    p.grad = torch.full((1025,), 1e25, device="cuda")
    opt.step()
    ref = float(np.float32(1e25)) * math.sqrt(1025)
    assert abs(float(opt.last_grad_norm) - ref) <= 1e-12 * ref
    stats = opt.clip_stats()
    assert (stats["steps"], stats["clipped"], stats["skipped"], stats["nonfinite"]) == (1, 1, 0, 0)
    assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), torch.ones_like(p)) and int(opt.state[p]["step"]) == 1


SHAPES = [(1,), (7,), (1001,), (33, 5, 3), (64, 9), (1025,)]
CPLX = [False, True, False, True, True, False]


def twins(seed, kw_a, kw_b, device_b="cuda", shapes=SHAPES, cplx=CPLX):
    p0 = draw(shapes, cplx, seed)
    pa = [torch.nn.Parameter(t.clone().cuda()) for t in p0]
    pb = [torch.nn.Parameter(t.clone().to(device_b)) for t in p0]
    return pa, pb, ComplexAdam(pa, lr=3e-3, weight_decay=1e-2, **kw_a), ComplexAdam(pb, lr=3e-3, weight_decay=1e-2, **kw_b)


def give(ps, host_grads):
    for p, g in zip(ps, host_grads):
        p.grad = g.clone().to(p.device)


def flat(t):
    t = t.detach().cpu()
    return (torch.view_as_real(t) if t.is_complex() else t).numpy()


def test_clipped_update_against_the_host_path():
    """4 steps, the gradient scale alternating: steps 1 and 3 clip, steps 2 and 4 do not"""
    pd, pc, od, oc = twins(1, {"max_grad_norm": 20.0}, {"max_grad_norm": 20.0}, device_b="cpu")
    for t in range(4):
        gs = draw(SHAPES, CPLX, 50 + t, scale=(3.0, 0.05)[t % 2])
        give(pd, gs)
        give(pc, gs)
        od.step()
        oc.step()
        assert (norm64(gs) > 20.0) == (t % 2 == 0)
        assert abs(float(od.last_grad_norm) - float(oc.last_grad_norm)) <= 1e-12 * float(oc.last_grad_norm)
    for a, b in zip(pd, pc):
        assert rel_err(flat(a), flat(b)) < 1e-6, tuple(a.shape)
        assert rel_err(od.state[a]["exp_avg_sq"].cpu().numpy(), oc.state[b]["exp_avg_sq"].numpy()) < 1e-6, tuple(a.shape)
    sd, sc = od.clip_stats(), oc.clip_stats()
    assert (sd["steps"], sd["clipped"], sd["skipped"]) == (sc["steps"], sc["clipped"], sc["skipped"]) == (4, 2, 0)
    assert math.isclose(sd["grad_norm"], sc["grad_norm"], rel_tol=1e-12) and math.isclose(sd["grad_norm_max"], sc["grad_norm_max"], rel_tol=1e-12)


def test_an_update_that_never_clips_equals_the_plain_optimiser():
    pa, pb, oa, ob = twins(2, {"max_grad_norm": 1e4}, {})
    for t in range(4):
        gs = draw(SHAPES, CPLX, 60 + t)
        give(pa, gs)
        give(pb, gs)
        oa.step()
        ob.step()
        for a, b in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach()), (t, tuple(a.shape))
            assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
    assert oa.clip_stats()["clipped"] == 0 and int(oa.state[pa[0]]["step"]) == 4


def snapshot(opt, ps):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), int(opt.state[p]["step"])) for p in ps]


@pytest.mark.parametrize("bad", ["inf", "nan_imag"])
def test_a_nonfinite_step_changes_nothing(bad):
    """25 tensors (two launches): inf in the last element of the last one, or NaN in one imaginary part"""
    shapes, cplx = [(1 + 97 * i,) for i in range(25)], [i % 3 == 0 for i in range(25)]
    pa, pb, oa, ob = twins(3, {"max_grad_norm": 5.0}, {"max_grad_norm": 5.0}, shapes=shapes, cplx=cplx)         # pb: never sees the bad step
    gs = draw(shapes, cplx, 70)
    give(pa, gs)
    give(pb, gs)
    oa.step()
    ob.step()
    before = snapshot(oa, pa)
    gs = draw(shapes, cplx, 71)
    if bad == "inf":
        gs[-1].view(-1)[-1] = math.inf
    else:
        gs[3].view(-1)[5] = complex(0.5, math.nan)
    give(pa, gs)
    oa.step()
    assert not math.isfinite(float(oa.last_grad_norm))
    for (p0, m0, v0, s0), (p1, m1, v1, s1) in zip(before, snapshot(oa, pa)):
        assert torch.equal(torch.view_as_real(p0) if p0.is_complex() else p0, torch.view_as_real(p1) if p1.is_complex() else p1)
        assert torch.equal(m0, m1) and torch.equal(v0, v1) and s0 == s1 == 1
    stats = oa.clip_stats()
    assert (stats["steps"], stats["skipped"], stats["nonfinite"]) == (2, 1, 1)
    gs = draw(shapes, cplx, 72)
    give(pa, gs)
    give(pb, gs)
    oa.step()
    ob.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach()), tuple(a.shape)
        assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
    assert int(oa.state[pa[0]]["step"]) == int(ob.state[pb[0]]["step"]) == 2


def test_unsupported_device_inputs_raise():
    p, q = torch.nn.Parameter(torch.randn(5, device="cuda")), torch.nn.Parameter(torch.randn(4, 6, device="cuda").half())
    opt = ComplexAdam([p, q], max_grad_norm=1.0)
    p.grad, q.grad = torch.zeros_like(p), torch.zeros_like(q)
    with pytest.raises(RuntimeError, match=r"parameter 1 of group 0 \(shape \(4, 6\), torch.float16, cuda:0\)"):
        opt.step()
    r = torch.nn.Parameter(torch.randn(4, 6, device="cuda"))
    opt = ComplexAdam([p, r], max_grad_norm=1.0)
    r.grad = torch.zeros(6, 4, device="cuda").t()
    with pytest.raises(RuntimeError, match=r"parameter 1 of group 0 .* not contiguous"):
        opt.step()
    h = torch.nn.Parameter(torch.randn(3))
    opt = ComplexAdam([p, h], max_grad_norm=1.0)
    h.grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match=r"host and device parameters in one optimiser - parameter 1 of group 0 \(shape \(3,\), torch.float32, cpu\)"):
        opt.step()


def test_captured_step_equals_the_eager_guarded_optimiser():
    """opt.step() alone in a graph; 5 replays, a non-finite gradient on replay 3, max_grad_norm and lr halved before replay 4"""
    shapes, cplx = [(9, 5), (33,), (1025,)], [True, False, False]
    pe, pg, oe, og = twins(4, {"max_grad_norm": 30.0}, {"max_grad_norm": 30.0, "capturable": True}, shapes=shapes, cplx=cplx)
    for p in pg:
        p.grad = torch.zeros_like(p)
    og.init_state()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        og.step()
    norms = []
    for t in range(5):
        if t == 3:
            for o in (oe, og):
                o.param_groups[0]["lr"] *= 0.5
                o.param_groups[0]["max_grad_norm"] *= 0.5
        gs = draw(shapes, cplx, 80 + t)
        if t == 2:
            gs[2][-1] = math.nan
        norms.append(norm64(gs))
        give(pe, gs)
        for q, g in zip(pg, gs):
            q.grad.copy_(g.cuda())
        oe.step()
        og.sync_hyper()
        graph.replay()
        torch.cuda.synchronize()
        for p, q in zip(pe, pg):
            assert torch.equal(torch.view_as_real(p.detach()) if p.is_complex() else p.detach(),
                               torch.view_as_real(q.detach()) if q.is_complex() else q.detach()), t
            assert torch.equal(oe.state[p]["exp_avg_sq"], og.state[q]["exp_avg_sq"]), t
        assert float(oe.last_grad_norm) == float(og.last_grad_norm) or t == 2
    # (norms of about 34: steps 1, 2 at the threshold 30 and steps 4, 5 at 15 all clip; the halved threshold must have reached the replay)
    se, sg = oe.clip_stats(), og.clip_stats()
    assert se == sg and (sg["steps"], sg["skipped"]) == (5, 1)
    assert sg["clipped"] == sum(1 for t, n in enumerate(norms) if math.isfinite(n) and n > (30.0 if t < 3 else 15.0))
    assert int(og.state[pg[0]]["step"]) == int(oe.state[pe[0]]["step"]) == 4


# ------------------------------------------------------------------------------------------------------------------------------ resume
def darcy_run(epochs, graph, **kw):
    """UNO_9(3, 4, pad=5) on 8 / 4 / 4 samples of the 72 x 72 grid of the recorded tiny run (tests/golden/dropin.json: the class keeps
    the reference's fixed mode counts, which a 16 x 16 grid does not have)"""
    from uno_amd.harness import DeviceDataset, fit_darcy
    from uno_amd.harness import models
    g = torch.Generator().manual_seed(107)
    torch.manual_seed(7)
    model = models.UNO_9(3, 4, pad=5).cuda()
    parts = [DeviceDataset(torch.rand(n, 72, 72, 1, generator=g), torch.rand(n, 72, 72, generator=g), "cuda") for n in (8, 4, 4)]
    rec = fit_darcy(model, *parts, batch_size=4, epochs=epochs, lr=1e-2, weight_decay=1e-3, scheduler_step=1, max_grad_norm=8.5, graph=graph,
                    generator=torch.Generator(device="cuda").manual_seed(3), log=lambda *a: None, **kw)
    return model, rec


def assert_same_run(a, b):
    (ma, ra), (mb, rb) = a, b
    strip = lambda r: [dataclasses.replace(e, seconds=0.0) for e in r.epochs]
    assert strip(ra) == strip(rb) and (ra.best_epoch, ra.best_val, ra.test) == (rb.best_epoch, rb.best_val, rb.test)
    for (k, x), (_, y) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(x, y), k
    for k in ra.state_dict:
        assert torch.equal(ra.state_dict[k], rb.state_dict[k]), k


@pytest.mark.parametrize("graph", [False, True])
def test_fit_darcy_resumed_equals_straight(graph, tmp_path):
    path = str(tmp_path / "run.ckpt")
    first = darcy_run(4, graph, checkpoint=(str(tmp_path / "first.ckpt"), 4))
    second = darcy_run(4, graph)
    assert_same_run(first, second)                  # the control: the determinism the comparison below rests on
    darcy_run(2, graph, checkpoint=(path, 2))
    resumed = darcy_run(4, graph, checkpoint=(path, 4), resume=path)
    assert_same_run(first, resumed)
    assert all(e.grad_norm is not None and e.grad_norm > 0 for e in resumed[1].epochs) and sum(e.skipped for e in resumed[1].epochs) == 0
    a, b = torch.load(str(tmp_path / "first.ckpt")), torch.load(path)
    assert a["epoch"] == b["epoch"] == 4 and a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]
    for k in a["optimizer"]["state"]:
        sa, sb = a["optimizer"]["state"][k], b["optimizer"]["state"][k]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and int(sa["step"]) == int(sb["step"]) == 8
