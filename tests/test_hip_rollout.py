"""uno_rollout_advance / uno_rollout_finish (K18, uno_amd/csrc/rollout.hip) and the NS-2D evaluation roll-out built on them
(harness.ns2d_rollout_errors, ns2d_evaluate, GraphedRollout) on the MI355X.

Kernel level, synthetic tensors (seeded randn, frame_t = target_t + 0.1 noise), all T steps of a roll-out: after every step the window
equals the reference's concatenation bit for bit, `shift = 0` leaves it alone, `pred` holds the frames bit for bit, and the five error
quantities are within 1e-5 relative of float64 on the host from the same inputs - the project's bound for a loss value (TOL of
tests/test_hip_step_errors.py); a ceiling: K17 measured <= 2.7e-7.  Measured on the MI355X (the maximum over the five quantities,
printed per case): 2.9e-8 at (1, 1, 1, 1, 1), 1.1e-7 at (3, 7, 3, 49, 4), 6.4e-8 at (2, 14, 10, 4096, 3), 1.0e-7 at (2, 6, 2, 20011, 2) and
6.8e-8 at (1, 5, 5, 1028, 2).

Model level (UNO / UNO_P at 64^2, batch 2, T_f = 3, product blocks): the native roll-out's prediction equals the reference-style stock
loop's bit for bit, its errors are within 1e-5 of float64 from that prediction (measured: 8.4e-8 for UNO, 1.1e-7 for UNO_P; the golden
case's step_sum is 1.2e-7 from the recorded loss), a graph replay equals the eager call bit for bit.

The shapes (B, C, T_in, P, T) are the smallest at which this kernel can go wrong; what each exercises is written beside it."""
import functools

import pytest
import torch

from conftest import Case, load_cases

pytestmark = pytest.mark.gpu
TOL = 1e-5

SHAPES = [
    (1, 1, 1, 1, 1),            # the smallest problem; T_in = C = 1: the shift only replaces
    (3, 7, 3, 49, 4),           # odd P: the 4-byte path, batch entries misaligned, one chunk
    (2, 14, 10, 4096, 3),       # the UNO(14, .) window at 64^2: 4 chunks, two full groups of four frames in the shift
    (2, 6, 2, 20011, 2),        # prime P: 20 chunks and a ragged last one
    (1, 5, 5, 1028, 2),         # no feature channels; P % 4 == 0 but not a chunk multiple: a last chunk of one 16-byte lane
]
ids = lambda s: "x".join(map(str, s))


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def problem(shape, seed=0, zero=None):
    """(window, frames (B, T, P), target (B, T, P)) on the host, the window after every step, and the float64 results (computed once per
    shape, never modified)"""
    B, C, T_in, P, T = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 5 * C + 3 * T_in + P + T)
    window = torch.randn(B, C, P, generator=g)
    target = torch.randn(B, T, P, generator=g)
    if zero is not None:
        target[zero[0], zero[1]] = 0
    frames = target + 0.1 * torch.randn(B, T, P, generator=g)
    windows, z = [], window
    for t in range(T):
        z = torch.cat((z[:, 1:T_in], frames[:, t, None], z[:, T_in:]), 1)         # the reference's window update, channels-first
        windows.append(z)
    f64, y64 = frames.double(), target.double()
    num, den = ((f64 - y64) ** 2).sum(2), (y64 ** 2).sum(2)
    per_step = num.sqrt() / den.sqrt()
    full = num.sum(1).sqrt() / den.sum(1).sqrt()
    want = {"sums": torch.stack((num, den), -1), "per_step": per_step, "full": full, "step_sum": per_step.sum(), "full_sum": full.sum()}
    return window, frames, target, windows, want


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


def bits(a, b):
    # (inf == inf and the comparison is of bits, not values: view as integers)
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_bits(a, b):
    return all(bits(x, y) for x, y in zip(a, b))


def chunks(P):
    """how many chunks a launch takes per batch entry (from the workspace size: exact while below the cap of 64)"""
    from uno_amd import _native
    return _native.lib().uno_rollout_ws_bytes(1, P, 1) // 8


def roll(shape, window, frames, target, with_pred=True, check=None):
    """all T steps on device copies -> (StepErrors, final window, pred); check(t, window) is called after every step.  The window and
    pred come from torch.empty, as the workspace and the record of the results do: the red-zone fixture guards all four."""
    from uno_amd import _native
    from uno_amd.harness import StepErrors
    B, C, T_in, P, T = shape
    z = torch.empty((B, C, P), dtype=torch.float32, device=dev())
    z.copy_(window)
    f, y = frames.to(dev()), target.to(dev())
    pred = torch.empty((B, T, P), dtype=torch.float32, device=dev()).fill_(float("nan")) if with_pred else None
    ws = _native.rollout_ws(B, P, T, dev())
    for t in range(T):
        _native.rollout_advance(z, f[:, t].contiguous(), y, pred, ws, T_in, t, True)
        if check is not None:
            check(t, z)
    sums, rel, totals = _native.rollout_finish(ws, B, P, T)
    return StepErrors(sums, rel[:, :T], rel[:, T], totals[0], totals[1]), z, pred


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_all_steps_against_the_reference_update_and_float64(shape):
    """Measured on the MI355X: the figures are in the module docstring."""
    from uno_amd import _native
    B, C, T_in, P, T = shape
    window, frames, target, windows, want = problem(shape)

    def check(t, z):
        assert bits(z, windows[t].to(dev())), f"window after step {t}"
        before = z.clone()                                   # shift = 0: sums and pred only, the window stays
        _native.rollout_advance(z, frames[:, t].to(dev()).contiguous(), target.to(dev()), None, _native.rollout_ws(B, P, T, dev()), T_in, t, False)
        assert bits(z, before), f"shift = 0 at step {t}"

    r, z, pred = roll(shape, window, frames, target, check=check)
    assert r.sums.shape == (B, T, 2) and r.per_step.shape == (B, T) and r.full.shape == (B,) and r.step_sum.dim() == 0 and r.full_sum.dim() == 0
    assert bits(pred, frames.to(dev()))
    e = worst(r, want)
    print(f"[rollout {shape}] chunks {chunks(P)}, max relative error {e:.2e}")
    assert e <= TOL
    # without pred: the same sums, the same window
    r2, z2, none = roll(shape, window, frames, target, with_pred=False)
    assert none is None and same_bits(r, r2) and bits(z, z2)


def test_chunk_counts():
    assert chunks(20011) == 20 and chunks(4096) == 4 and chunks(49) == 1 and chunks(1028) == 2 and chunks(1) == 1
    assert chunks(20011) >= 3


@pytest.mark.parametrize("shape", [(3, 7, 3, 49, 4), (2, 6, 2, 20011, 2)], ids=ids)
def test_two_runs_give_the_same_bits(shape):
    window, frames, target, _, _ = problem(shape)
    a, b = roll(shape, window, frames, target), roll(shape, window, frames, target)
    assert same_bits(a[0], b[0]) and bits(a[1], b[1]) and bits(a[2], b[2])


def test_reserved_cus_do_not_change_the_bits():
    from uno_amd import _native
    shape = (2, 6, 2, 20011, 2)
    window, frames, target, _, _ = problem(shape)
    before = roll(shape, window, frames, target)
    prev = _native.reserve_cus(16)
    try:
        under = roll(shape, window, frames, target)
    finally:
        _native.reserve_cus(prev)
    assert same_bits(before[0], under[0]) and bits(before[1], under[1]) and bits(before[2], under[2])


def test_graph_replay_gives_the_eager_bits_on_fresh_inputs():
    from uno_amd import _native
    shape = (2, 14, 10, 4096, 3)
    B, C, T_in, P, T = shape
    window, frames, target, _, _ = problem(shape)
    fresh_w, fresh_f, fresh_y, _, want = problem(shape, seed=1)
    sz, sf, sy = window.to(dev()), frames.to(dev()), target.to(dev())
    spred = torch.empty_like(sy)

    def run():
        ws = _native.rollout_ws(B, P, T, dev())
        for t in range(T):
            _native.rollout_advance(sz, sf[:, t].contiguous(), sy, spred, ws, T_in, t, t + 1 < T)
        return _native.rollout_finish(ws, B, P, T)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # eager warm-up off the default stream, as capture requires
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    sz.copy_(fresh_w)
    sf.copy_(fresh_f)
    sy.copy_(fresh_y)
    graph.replay()
    torch.cuda.synchronize()
    ez, ef, ey = fresh_w.to(dev()), fresh_f.to(dev()), fresh_y.to(dev())
    epred = torch.empty_like(ey)
    ws = _native.rollout_ws(B, P, T, dev())
    for t in range(T):
        _native.rollout_advance(ez, ef[:, t].contiguous(), ey, epred, ws, T_in, t, t + 1 < T)
    eager = _native.rollout_finish(ws, B, P, T)
    assert same_bits(captured, eager) and bits(sz, ez) and bits(spred, epred)
    from uno_amd.harness import StepErrors
    sums, rel, totals = captured
    assert worst(StepErrors(sums, rel[:, :T], rel[:, T], totals[0], totals[1]), want) <= TOL


def test_a_zero_target_slice_gives_inf_and_leaves_the_rest_alone():
    shape = (2, 4, 2, 500, 3)
    window, frames, target, _, want = problem(shape, zero=(0, 1))
    r, _, _ = roll(shape, window, frames, target)
    assert float(r.sums[0, 1, 1]) == 0.0
    assert float(r.per_step[0, 1]) == float("inf")
    assert float(r.step_sum) == float("inf")
    skip = torch.zeros(2, 3, dtype=torch.bool)
    skip[0, 1] = True
    assert abs(float(r.sums[0, 1, 0]) - float(want["sums"][0, 1, 0])) <= TOL * float(want["sums"][0, 1, 0])
    assert worst(r, want, skip=skip) <= TOL         # every other entry, `full` and `full_sum` included
    # 0 / 0 is NaN, as torch.norm(.) / torch.norm(.) gives
    z = torch.zeros(1, 2, 10)
    rz, _, _ = roll((1, 3, 2, 10, 2), torch.zeros(1, 3, 10), z, z)
    assert torch.isnan(rz.per_step).all() and torch.isnan(rz.full).all()


@pytest.mark.parametrize("shape", [(3, 7, 3, 49, 4), (2, 6, 2, 20011, 2), (1, 5, 5, 1028, 2)], ids=ids)
def test_outputs_workspace_window_and_pred_stay_inside_their_allocations(shape, monkeypatch):
    """the window, pred, ws and the record of sums, rel and totals each sit between two poisoned 64 KiB guard bands
    (tests/test_hip_redzone.py): the bands are untouched after the roll-out."""
    from test_hip_redzone import RedZone
    window, frames, target, windows, want = problem(shape)
    zone = RedZone(monkeypatch)
    r, z, pred = roll(shape, window, frames, target)
    assert zone.check(f"rollout {shape}") == 4
    assert worst(r, want) <= TOL and bits(z, windows[-1].to(dev())) and bits(pred, frames.to(dev()))


def test_binding_refuses_what_the_kernel_does_not_take():
    from uno_amd import _native
    B, C, T_in, P, T = 2, 5, 3, 12, 4
    w, f, y = torch.zeros(B, C, P, device=dev()), torch.zeros(B, P, device=dev()), torch.zeros(B, T, P, device=dev())
    ws = _native.rollout_ws(B, P, T, dev())
    _native.rollout_advance(w, f, y, None, ws, T_in, 0, True)                    # the good call
    wide = torch.zeros(B, 2 * P, device=dev())
    bad_frames = (f.double(), wide[:, ::2], torch.zeros(B, P + 1, device=dev()), f.cpu())      # dtype, density, shape, device
    for bad in bad_frames:
        with pytest.raises(RuntimeError):
            _native.rollout_advance(w, bad, y, None, ws, T_in, 0, True)
    with pytest.raises(RuntimeError):
        _native.rollout_advance(w, f, y[:, :, :P - 1].contiguous(), None, ws, T_in, 0, True)
    with pytest.raises(RuntimeError):
        _native.rollout_advance(w, f, y, torch.zeros(B, T + 1, P, device=dev()), ws, T_in, 0, True)
    with pytest.raises(RuntimeError):
        _native.rollout_advance(w, f, y, None, ws[:8], T_in, 0, True)             # a workspace too small
    with pytest.raises(RuntimeError, match="at most 256"):
        _native.rollout_advance(w, f, torch.zeros(B, 257, P, device=dev()), None, ws, T_in, 0, True)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _native.rollout_advance(w, f, y, None, ws, T_in, T, True)                 # t = T
    with pytest.raises(RuntimeError, match="bad sizes"):
        _native.rollout_advance(w, f, y, None, ws, C + 1, 0, True)                # T_in > C
    with pytest.raises(RuntimeError, match="at most 256"):
        _native.rollout_finish(ws, B, P, 257)


# ------------------------------------------------------------------------------------------------------------------ model level
def stock_loop(model, xx, yy, T_f):
    """the reference's loop (ns_train_2d.py:141-157) on the same model -> the concatenated prediction (B, S, S, T_f)"""
    with torch.no_grad():
        for t in range(T_f):
            im = model(xx)
            pred = im if t == 0 else torch.cat((pred, im), -1)
            xx = torch.cat((xx[..., 1:], im), dim=-1)
    return pred


def float64_errors(pred, yy):
    B, T = pred.shape[0], pred.shape[-1]
    p64, y64 = pred.double().cpu().reshape(B, -1, T), yy.double().cpu().reshape(B, -1, T)
    num, den = ((p64 - y64) ** 2).sum(1), (y64 ** 2).sum(1)
    per_step = num.sqrt() / den.sqrt()
    full = num.sum(1).sqrt() / den.sum(1).sqrt()
    return {"sums": torch.stack((num, den), -1), "per_step": per_step, "full": full, "step_sum": per_step.sum(), "full_sum": full.sum()}


@functools.lru_cache(maxsize=None)
def model_problem(name):
    """(model, three batches (xx, yy)) on the device, T_f = 3"""
    from uno_amd import harness
    torch.manual_seed(5)
    model = getattr(harness, name)(14, 4).to(dev())
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(2, 64, 64, 10, generator=g).to(dev()), torch.randn(2, 64, 64, 3, generator=g).to(dev())) for _ in range(3)]
    return model, batches


@pytest.mark.parametrize("name", ["UNO", "UNO_P"])
def test_native_rollout_equals_the_stock_loop(name):
    from uno_amd.harness import ns2d_rollout_errors
    model, batches = model_problem(name)
    xx, yy = batches[0]
    r = ns2d_rollout_errors(model, xx, yy, 3, return_pred=True)
    want_pred = stock_loop(model, xx, yy, 3)
    assert r.pred.shape == want_pred.shape == (2, 64, 64, 3)
    assert bits(r.pred, want_pred)
    e = worst(r.errors, float64_errors(want_pred, yy))
    print(f"[{name} roll-out] max relative error of the five quantities against float64 {e:.2e}")
    assert e <= TOL
    assert all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in r.errors)
    plain = ns2d_rollout_errors(model, xx, yy, 3)
    assert plain.pred is None and same_bits(plain.errors, r.errors)


def test_native_rollout_on_the_golden_case():
    from uno_amd.harness import UNO, ns2d_rollout_errors
    c = Case(load_cases("harness_ns.npz")[0], "ns2d")
    torch.manual_seed(21)
    model = UNO(14, 4).to(dev())
    xx, yy = torch.from_numpy(c.xx).to(dev()), torch.from_numpy(c.yy).to(dev())
    e = ns2d_rollout_errors(model, xx, yy, T_f=2).errors
    d = abs(float(e.step_sum) - float(c.loss)) / abs(float(c.loss))
    print(f"[ns2d golden, native] step_sum against the recorded loss {d:.2e}")
    assert d < 1e-5


@pytest.mark.parametrize("name", ["UNO", "UNO_P"])
def test_graphed_rollout_equals_eager_and_sees_parameter_updates(name):
    from uno_amd.harness import GraphedRollout, ns2d_rollout_errors
    model, batches = model_problem(name)
    gr = GraphedRollout(model, 3, batches[0], return_pred=True)
    for xx, yy in batches[1:]:
        got = gr.errors(xx, yy)
        want = ns2d_rollout_errors(model, xx, yy, 3, return_pred=True)
        assert same_bits(got.errors, want.errors) and bits(got.pred, want.pred)
    first = gr.errors(*batches[1])
    second = gr.errors(*batches[2])                      # clones: an earlier result survives the next replay
    assert same_bits(first.errors, ns2d_rollout_errors(model, *batches[1], 3).errors) and not same_bits(first.errors, second.errors)
    with torch.no_grad():
        model.fc2.bias.add_(0.5)
    try:
        got = gr.errors(*batches[1])
        want = ns2d_rollout_errors(model, *batches[1], 3, return_pred=True)
        assert same_bits(got.errors, want.errors) and bits(got.pred, want.pred)
        assert not same_bits(got.errors, first.errors)
    finally:
        with torch.no_grad():
            model.fc2.bias.sub_(0.5)
    with pytest.raises(RuntimeError):
        gr.errors(batches[0][0][:1], batches[0][1][:1])
    step_total, full_total = gr.evaluate(batches)
    want = [ns2d_rollout_errors(model, xx, yy, 3).errors for xx, yy in batches]
    assert abs(float(step_total) - sum(float(e.step_sum) for e in want)) <= TOL * float(step_total)
    assert abs(float(full_total) - sum(float(e.full_sum) for e in want)) <= TOL * float(full_total)


def test_graphed_rollout_refuses_where_the_native_path_does_not_apply():
    from uno_amd.harness import GraphedRollout
    model, batches = model_problem("UNO")
    xx, yy = batches[0]
    with pytest.raises(RuntimeError):
        GraphedRollout(model, 3, (xx.double(), yy.double()))
    with pytest.raises(RuntimeError):
        GraphedRollout(model, 257, (xx, yy))


def test_ns2d_evaluate_sums_the_batches_and_restores_the_mode():
    from uno_amd.harness import ns2d_evaluate, ns2d_rollout_errors
    model, batches = model_problem("UNO")
    model.train()
    step_total, full_total = ns2d_evaluate(model, batches, 3)
    assert model.training and step_total.is_cuda and step_total.dim() == 0 and full_total.dim() == 0
    model.eval()
    want = [ns2d_rollout_errors(model, xx, yy, 3).errors for xx, yy in batches]
    total = want[0].step_sum + want[1].step_sum + want[2].step_sum
    full = want[0].full_sum + want[1].full_sum + want[2].full_sum
    assert bits(step_total, total) and bits(full_total, full)
    ns2d_evaluate(model, batches[:1], 3)
    assert not model.training
    model.train()
