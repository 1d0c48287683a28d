"""uno_rel_l2_steps (K17, uno_amd/csrc/rel_l2_steps.hip) through harness.step_errors on the MI355X: the per-time-step and whole-trajectory
relative L2 errors of the NS-3D loop (reference ns_train_3d.py:55-62) in one pass, against float64 on the host from the same inputs.

Bound: relative error <= 1e-5 for every entry of `sums`, `per_step`, `full` and for `step_sum`, `full_sum` - the project's bound for a
loss value (TOL_PRED of the harness tests).  A ceiling, not a target: the stock float32 slice-by-slice path is 1.0e-7 from float64 at
(2, 64 * 64, 40) on the host.  Measured on the MI355X (the maximum over the five quantities, printed per case): 2.4e-8 at (1, 1, 1),
2.7e-7 at (3, 49, 9), 1.2e-7 at (2, 4096, 40), 8.8e-8 at (2, 20011, 13), 1.4e-7 at (1, 300, 256), 1.6e-7 at (2, 100, 255) and 2.7e-7 on the
stock path at (2, 64, 257).

The shapes (B, P, T) are the smallest at which this kernel can go wrong; what each exercises is written beside it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-5

SHAPES = [
    (1, 1, 1),              # the smallest problem
    (3, 49, 9),             # odd P * T: batch entries 1 and 2 start misaligned
    (2, 4096, 40),          # 256 % 40 != 0: idle threads; the Uno3D_T40 output shape
    (2, 20011, 13),         # prime P: 62 chunks of 323 pixels, a ragged last one
    (1, 300, 256),          # the largest T
    (2, 100, 255),          # one active row per pass
    (2, 64, 257),           # beyond the kernel: the stock path of step_errors, still right
]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def problem(shape, seed=0, zero=None):
    """(pred, target) on the host and the float64 results from them (computed once per shape, never modified)"""
    B, P, T = shape
    g = torch.Generator().manual_seed(1000 * seed + B * 7 + P * 3 + T)
    target = torch.randn(B, P, T, generator=g)
    pred = target + 0.1 * torch.randn(B, P, T, generator=g)
    if zero is not None:
        target[zero[0], :, zero[1]] = 0
    p64, y64 = pred.double(), target.double()
    num, den = ((p64 - y64) ** 2).sum(1), (y64 ** 2).sum(1)
    per_step = num.sqrt() / den.sqrt()
    full = num.sum(1).sqrt() / den.sum(1).sqrt()
    return pred, target, {"sums": torch.stack((num, den), -1), "per_step": per_step, "full": full, "step_sum": per_step.sum(),
                          "full_sum": full.sum()}


def worst(r, want, skip=None):
    """largest relative error over the five quantities; skip: a boolean (B, T) mask of entries that are checked elsewhere"""
    out = 0.0
    for k, w in want.items():
        got = getattr(r, k).double().cpu()
        assert got.shape == w.shape, k
        e = (got - w).abs() / w.abs()
        if skip is not None:
            if k in ("sums", "per_step"):
                e = e[~skip]
            elif k == "step_sum":
                continue
        assert not torch.isnan(e).any(), k
        out = max(out, float(e.max()))
    return out


def step_errors(pred, target):
    from uno_amd.harness import step_errors as fn
    return fn(pred, target)


def chunks(shape):
    """how many chunks the partial launch takes per batch entry (from the workspace size: exact while below the cap of 64)"""
    from uno_amd import _native
    B, P, T = shape
    return _native.lib().uno_rel_l2_steps_ws_bytes(B, P, T) // (8 * B * T)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64(shape):
    """Measured on the MI355X: 2.4e-8 ... 2.7e-7 over the seven shapes (the figures are in the module docstring)."""
    pred, target, want = problem(shape)
    r = step_errors(pred.to(dev()), target.to(dev()))
    B, P, T = shape
    assert r.sums.shape == (B, T, 2) and r.per_step.shape == (B, T) and r.full.shape == (B,) and r.step_sum.dim() == 0 and r.full_sum.dim() == 0
    assert all(t.is_cuda and t.dtype == torch.float32 for t in r)
    e = worst(r, want)
    print(f"[step_errors {shape}] chunks {chunks(shape) if T <= 256 else '-'}, max relative error {e:.2e}")
    assert e <= TOL


def test_the_prime_shape_has_several_chunks_and_a_ragged_last_one():
    assert chunks((2, 20011, 13)) >= 3 and chunks((2, 4096, 40)) >= 3 and chunks((3, 49, 9)) == 1


def test_space_axes_may_be_separate_and_the_views_alias_one_record():
    pred, target, want = problem((2, 4096, 40))
    r = step_errors(pred.view(2, 64, 64, 40).to(dev()), target.view(2, 64, 64, 40).to(dev()))
    assert worst(r, want) <= TOL
    assert r.per_step.data_ptr() + 4 * 40 == r.full.data_ptr()          # rel (B, T + 1): per_step and full are views of it


def same_bits(a, b):
    # (inf == inf and the comparison is of bits, not values: view as integers)
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", [(3, 49, 9), (2, 20011, 13)], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_give_the_same_bits(shape):
    pred, target, _ = problem(shape)
    p, y = pred.to(dev()), target.to(dev())
    assert same_bits(step_errors(p, y), step_errors(p, y))


def test_reserved_cus_do_not_change_the_bits():
    from uno_amd import _native
    pred, target, _ = problem((2, 20011, 13))
    p, y = pred.to(dev()), target.to(dev())
    before = step_errors(p, y)
    prev = _native.reserve_cus(16)
    try:
        under = step_errors(p, y)
    finally:
        _native.reserve_cus(prev)
    assert same_bits(before, under)


def test_graph_replay_gives_the_eager_bits_on_fresh_inputs():
    shape = (2, 4096, 40)
    pred, target, _ = problem(shape)
    fresh_p, fresh_y, want = problem(shape, seed=1)
    sp, sy = pred.to(dev()), target.to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # eager warm-up off the default stream, as capture requires
        step_errors(sp, sy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step_errors(sp, sy)
    sp.copy_(fresh_p.to(dev()))
    sy.copy_(fresh_y.to(dev()))
    graph.replay()
    torch.cuda.synchronize()
    eager = step_errors(fresh_p.to(dev()), fresh_y.to(dev()))
    assert same_bits(captured, eager)
    assert worst(captured, want) <= TOL


def test_a_zero_target_slice_gives_inf_as_stock_and_leaves_the_rest_alone():
    shape = (2, 500, 7)
    pred, target, want = problem(shape, zero=(0, 2))
    r = step_errors(pred.to(dev()), target.to(dev()))
    assert float(r.sums[0, 2, 1]) == 0.0
    assert float(r.per_step[0, 2]) == float("inf")
    assert float(r.step_sum) == float("inf")
    skip = torch.zeros(2, 7, dtype=torch.bool)
    skip[0, 2] = True
    assert abs(float(r.sums[0, 2, 0]) - float(want["sums"][0, 2, 0])) <= TOL * float(want["sums"][0, 2, 0])
    assert worst(r, want, skip=skip) <= TOL         # every other entry, `full` and `full_sum` included
    # 0 / 0 is NaN, as torch.norm(.) / torch.norm(.) gives
    z = torch.zeros(1, 10, 3, device=dev())
    assert torch.isnan(step_errors(z, z).per_step).all()


def test_a_permuted_view_gives_the_result_of_its_contiguous_copy():
    pred, target, want = problem((3, 49, 9))
    base = pred.permute(0, 2, 1).contiguous().to(dev())         # (B, T, P) in memory
    view = base.permute(0, 2, 1)                                # (B, P, T), not dense
    assert not view.is_contiguous()
    y = target.to(dev())
    assert same_bits(step_errors(view, y), step_errors(view.contiguous(), y))
    assert worst(step_errors(view, y), want) <= TOL


@pytest.mark.parametrize("shape", [(3, 49, 9), (2, 20011, 13), (1, 300, 256)], ids=lambda s: "x".join(map(str, s)))
def test_outputs_and_workspace_stay_inside_their_allocations(shape, monkeypatch):
    """sums, rel, totals and the workspace each sit between two poisoned 64 KiB guard bands (tests/test_hip_redzone.py): the bands
    are untouched after the call."""
    from test_hip_redzone import RedZone
    pred, target, want = problem(shape)
    p, y = pred.to(dev()), target.to(dev())
    zone = RedZone(monkeypatch)
    r = step_errors(p, y)
    assert zone.check(f"step_errors {shape}") == 4
    assert worst(r, want) <= TOL


def test_binding_refuses_what_the_kernel_does_not_take():
    from uno_amd import _native
    x = torch.zeros(2, 10, 4, device=dev())
    for bad in (x.double(), x[:, ::2], x[..., :3], x.cpu()):           # dtype, density, shape, device
        with pytest.raises(RuntimeError):
            _native.rel_l2_steps(x, bad)
    with pytest.raises(RuntimeError):
        _native.rel_l2_steps(torch.zeros(2, 3, 257, device=dev()), torch.zeros(2, 3, 257, device=dev()))
