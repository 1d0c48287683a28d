"""uno_rollout_lift / uno_rollout_lift_backward / uno_rollout_loss_seed (K19, K19-B, uno_amd/csrc/rollout_train.hip) and the window-free
NS-2D training roll-out built on them (harness.ns2d_rollout_loss(native=True)) on the MI355X.

Kernel level, synthetic tensors (seeded randn; the recorded frames are target + 0.1 noise, gh of every window randn, gL = 1.7), every
window t = 0 ... T - 1 of a roll-out forwards, then backwards in descending t as a backward pass walks them, against float64 on the host
from the same inputs, l2-relative:
    h 2e-6;  gframe, gpred, gw, gb 2e-5  (the project's bounds for channel sums and for weight / bias gradients,
    tests/test_hip_channel_mix.py);  loss 1e-5  (TOL of tests/test_hip_rollout.py).
Measured on the MI355X (printed per case), the maximum over the windows of a case:
    shape                       h        gframe   gpred    gw       gb       loss
    (1, 1, 0, 1, 1, 2)          4.0e-8   8.8e-8   0        5.7e-8   0        5.1e-8
    (3, 3, 4, 5, 49, 5)         6.6e-8   6.8e-8   5.3e-8   1.2e-7   9.0e-8   1.1e-8
    (2, 10, 4, 16, 4096, 12)    8.6e-8   1.0e-7   9.0e-8   3.1e-7   4.8e-7   2.0e-8
    (2, 2, 1, 64, 20011, 3)     4.0e-8   1.5e-7   1.4e-7   2.7e-7   3.3e-7   2.4e-8
    (1, 28, 4, 3, 1028, 2)      1.3e-7   1.2e-7   0        2.8e-7   2.9e-7   9.8e-8
(gpred is exactly zero where no frame is ever an older predicted frame of a window: T = 2.)

Model level (product blocks, 64^2): the golden case of tests/test_harness_ns.py with native=True inside that test's bounds; UNO(14, 4)
and UNO_P(14, 4), batch 2, T_f = 12 > T_in, default and native path each against a float64 oracle-block run of the same model on the
host - the native error may be at most twice the default path's (both run the same body kernels and differ only in the lift's and the
loss's summation order); GraphedStep on the native loss equals the eager step bit for bit.  Measured on the MI355X against float64,
(gradient, loss): UNO default (3.3e-8, 2.9e-8), native (4.3e-8, 2.9e-8); UNO_P default (6.3e-8, 4.5e-9), native (6.4e-8, 4.5e-9); the
golden case's native loss is 1.2e-7 from the recorded one.

The shapes (B, T_in, F, Cm, P, T) are the smallest at which these kernels can go wrong; what each exercises is written beside it."""
import functools

import pytest
import torch

from conftest import Case, load_cases
from harness_checks import assert_graphed_step_equals_eager, check_grads, check_init

pytestmark = pytest.mark.gpu
TOL_H, TOL_G, TOL_LOSS = 2e-6, 2e-5, 1e-5

SHAPES = [
    (1, 1, 0, 1, 1, 2),             # the smallest problem: one pixel, one frame, no features, one lifted channel
    (3, 3, 4, 5, 49, 5),            # odd P: the 4-byte path, misaligned batch entries; windows all given, straddling, all predicted
    (2, 10, 4, 16, 4096, 12),       # the UNO(14, 32) lift at 64^2 with T > T_in: 4 chunks, 256-pixel tiles
    (2, 2, 1, 64, 20011, 3),        # prime P: 20 chunks with a ragged last one, at the Cm limit: 128-pixel tiles
    (1, 28, 4, 3, 1028, 2),         # C = 32, the limit; a last chunk of one 16-byte lane
]
ids = lambda s: "x".join(map(str, s))
GL = 1.7


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def l2(got, want):
    got, want = got.double().cpu().reshape(-1), want.reshape(-1)
    n = float(want.norm())
    return float((got - want).norm()) / n if n > 0 else float((got - want).norm())


def bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def problem(shape, seed=0):
    """float32 inputs on the host and the float64 results from them (computed once per shape, never modified)"""
    B, T_in, F, Cm, P, T = shape
    C = T_in + F
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 5 * T_in + 3 * F + 11 * Cm + P + T)
    inp = {"given": torch.randn(B, T_in, P, generator=g), "feat": torch.randn(F, P, generator=g) if F else None,
           "w": torch.randn(Cm, C, generator=g) / C ** 0.5, "bias": torch.randn(Cm, generator=g), "target": torch.randn(B, T, P, generator=g),
           "gh": torch.randn(T, B, Cm, P, generator=g)}
    inp["frames"] = inp["target"] + 0.1 * torch.randn(B, T, P, generator=g)
    d = {k: (v.double() if v is not None else None) for k, v in inp.items()}
    seq = torch.cat((d["given"], d["frames"]), 1)                                       # the sequence of frames (B, T_in + T, P)
    feat = d["feat"].unsqueeze(0).expand(B, -1, -1) if F else seq[:, :0]
    want = {"h": [], "gframe": [None] * T}
    num, den = ((d["frames"] - d["target"]) ** 2).sum(2), (d["target"] ** 2).sum(2)     # (B, T)
    want["loss"] = (num.sqrt() / den.sqrt()).sum()
    lterm = GL * (d["frames"] - d["target"]) / (num.sqrt() * den.sqrt()).unsqueeze(-1)  # (B, T, P)
    gseq = torch.zeros_like(seq)                                                        # the gradient of every frame through the lifts
    gw, gb = torch.zeros(Cm, C, dtype=torch.float64), torch.zeros(Cm, dtype=torch.float64)
    for t in range(T):
        x = torch.cat((seq[:, t:t + T_in], feat), 1)                                    # (B, C, P)
        want["h"].append(torch.einsum("mc,bcp->bmp", d["w"], x) + d["bias"].view(1, -1, 1))
        gw += torch.einsum("bmp,bcp->mc", d["gh"][t], x)
        gb += d["gh"][t].sum((0, 2))
        gseq[:, t:t + T_in] += torch.einsum("mk,bmp->bkp", d["w"][:, :T_in], d["gh"][t])
    gfull = gseq[:, T_in:] + lterm                                                      # the complete gradient of every predicted frame
    want["gseed"] = lterm[:, T - 1]
    for t in range(1, T):
        want["gframe"][t] = gfull[:, t - 1]
    # gpred after the whole walk: the shares of the windows in which the frame is NOT the newest (window q + 1 adds the rest into gframe)
    gp = torch.zeros(B, T, P, dtype=torch.float64)
    for t in range(T):
        gx = torch.einsum("mk,bmp->bkp", d["w"][:, :T_in], d["gh"][t])
        for k in range(max(0, T_in - t), T_in - 1):
            gp[:, t + k - T_in] += gx[:, k]
    want.update(gpred=gp, gw=gw, gb=gb)
    return inp, want


def run(shape, inp, checks=True):
    """the whole roll-out on device copies -> dict of everything the kernels wrote (h per window, pred, loss, gseed, gframe per window,
    gpred, gw, gb).  Outputs and workspaces come from torch.empty / zeros: the red-zone fixture guards them."""
    from uno_amd import _native
    B, T_in, F, Cm, P, T = shape
    D = dev()
    given, target, frames, w, bias = (inp[k].to(D) for k in ("given", "target", "frames", "w", "bias"))
    feat = inp["feat"].to(D) if F else None
    gh = inp["gh"].to(D)
    pred = torch.empty((B, T, P), dtype=torch.float32, device=D).fill_(float("nan"))
    ws = _native.rollout_ws(B, P, T, D)
    out = {"h": [], "gframe": [None] * T}
    for t in range(T):
        out["h"].append(_native.rollout_lift(given, pred, feat, w, bias, t))
        _native.rollout_advance(given, frames[:, t].contiguous(), target, pred, ws, T_in, t, False)
    sums, _, totals = _native.rollout_finish(ws, B, P, T)
    out["pred"], out["loss"] = pred, totals[0]
    gL = torch.full((1,), GL, dtype=torch.float32, device=D)
    gpred = torch.zeros((B, T, P), dtype=torch.float32, device=D)
    parts = _native.rollout_lift_bwd_ws(B, T_in, F, Cm, P, T, D)
    out["gseed"] = torch.empty((B, P), dtype=torch.float32, device=D)
    _native.rollout_loss_seed(pred, target, sums, gL, out["gseed"])
    for t in range(T - 1, -1, -1):
        gframe = torch.empty((B, P), dtype=torch.float32, device=D).fill_(float("nan"))
        _native.rollout_lift_backward(gh[t], given, pred, target, feat, w, sums, gL, gpred, gframe, parts, t)
        if t >= 1:
            out["gframe"][t] = gframe
        elif checks:
            assert torch.isnan(gframe).all(), "window 0 has no newest predicted frame: gframe must stay untouched"
    out["gpred"] = gpred
    out["gw"], out["gb"] = _native.channel_wgrad_finish(parts, T_in + F, Cm, True)
    return out


def flat(out):
    return [*out["h"], out["pred"], out["loss"], out["gseed"], *[g for g in out["gframe"] if g is not None], out["gpred"], out["gw"], out["gb"]]


def same_bits(a, b):
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(bits(x, y) for x, y in zip(fa, fb))


def errors(shape, out, want):
    T = shape[-1]
    e = {"h": max(l2(out["h"][t], want["h"][t]) for t in range(T)),
         "gframe": max([l2(out["gseed"], want["gseed"])] + [l2(out["gframe"][t], want["gframe"][t]) for t in range(1, T)]),
         "gpred": l2(out["gpred"], want["gpred"]), "gw": l2(out["gw"], want["gw"]), "gb": l2(out["gb"], want["gb"]),
         "loss": abs(float(out["loss"]) - float(want["loss"])) / abs(float(want["loss"]))}
    return e


def within(e):
    return e["h"] <= TOL_H and all(e[k] <= TOL_G for k in ("gframe", "gpred", "gw", "gb")) and e["loss"] <= TOL_LOSS


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_all_windows_against_float64(shape):
    """Measured on the MI355X: the figures are in the module docstring."""
    inp, want = problem(shape)
    out = run(shape, inp)
    assert bits(out["pred"], inp["frames"].to(dev()))
    e = errors(shape, out, want)
    print(f"[rollout_train {shape}] " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["h"] <= TOL_H
    for k in ("gframe", "gpred", "gw", "gb"):
        assert e[k] <= TOL_G, k
    assert e["loss"] <= TOL_LOSS
    assert out["h"][0].shape == (shape[0], shape[3], shape[4]) and out["gw"].shape == (shape[3], shape[1] + shape[2]) and out["gb"].shape == (shape[3],)


@pytest.mark.parametrize("shape", [(3, 3, 4, 5, 49, 5), (2, 2, 1, 64, 20011, 3)], ids=ids)
def test_two_runs_give_the_same_bits(shape):
    inp, _ = problem(shape)
    assert same_bits(run(shape, inp), run(shape, inp))


def test_reserved_cus_do_not_change_the_bits():
    from uno_amd import _native
    shape = (2, 2, 1, 64, 20011, 3)
    inp, _ = problem(shape)
    before = run(shape, inp)
    prev = _native.reserve_cus(16)
    try:
        under = run(shape, inp)
    finally:
        _native.reserve_cus(prev)
    assert same_bits(before, under)


def test_graph_replay_gives_the_eager_bits_on_fresh_inputs():
    from uno_amd import _native
    shape = (2, 10, 4, 16, 4096, 12)
    B, T_in, F, Cm, P, T = shape
    inp, _ = problem(shape)
    fresh, want = problem(shape, seed=1)
    D = dev()
    keys = ("given", "feat", "w", "bias", "target", "frames", "gh")
    static = {k: inp[k].to(D) for k in keys}
    gL = torch.full((1,), GL, dtype=torch.float32, device=D)

    def walk(s):
        pred = torch.empty((B, T, P), dtype=torch.float32, device=D)
        ws = _native.rollout_ws(B, P, T, D)
        hs = []
        for t in range(T):
            hs.append(_native.rollout_lift(s["given"], pred, s["feat"], s["w"], s["bias"], t))
            _native.rollout_advance(s["given"], s["frames"][:, t].contiguous(), s["target"], pred, ws, T_in, t, False)
        sums, _, totals = _native.rollout_finish(ws, B, P, T)
        gpred = torch.zeros((B, T, P), dtype=torch.float32, device=D)
        parts = _native.rollout_lift_bwd_ws(B, T_in, F, Cm, P, T, D)
        gseed = torch.empty((B, P), dtype=torch.float32, device=D)
        _native.rollout_loss_seed(pred, s["target"], sums, gL, gseed)
        gframes = []
        for t in range(T - 1, -1, -1):
            gframes.append(torch.empty((B, P), dtype=torch.float32, device=D))
            _native.rollout_lift_backward(s["gh"][t], s["given"], pred, s["target"], s["feat"], s["w"], sums, gL, gpred, gframes[-1], parts, t)
        gw, gb = _native.channel_wgrad_finish(parts, T_in + F, Cm, True)
        return [*hs, pred, totals[0], gseed, *gframes[:-1], gpred, gw, gb]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # eager warm-up off the default stream, as capture requires
        walk(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = walk(static)
    for k in keys:
        static[k].copy_(fresh[k])
    graph.replay()
    torch.cuda.synchronize()
    eager = walk({k: fresh[k].to(D) for k in keys})
    assert len(captured) == len(eager) and all(bits(a, b) for a, b in zip(captured, eager))
    assert abs(float(captured[T + 1]) - float(want["loss"])) <= TOL_LOSS * float(want["loss"])
    assert l2(captured[-2], want["gw"]) <= TOL_G


@pytest.mark.parametrize("shape", [(3, 3, 4, 5, 49, 5), (2, 2, 1, 64, 20011, 3), (1, 28, 4, 3, 1028, 2)], ids=ids)
def test_outputs_and_workspaces_stay_inside_their_allocations(shape, monkeypatch):
    """h, pred, gpred, gframe, the chunk-sum and the weight-sum workspace, gw and gb each sit between two poisoned 64 KiB guard bands
    (tests/test_hip_redzone.py): the bands are untouched after the roll-out."""
    from test_hip_redzone import RedZone
    inp, want = problem(shape)
    T = shape[-1]
    zone = RedZone(monkeypatch)
    out = run(shape, inp)
    # at least: T x h, pred, the chunk-sum workspace, the record, gpred, the weight-sum workspace, gseed, T x gframe
    assert zone.check(f"rollout_train {shape}") >= 2 * T + 6
    assert within(errors(shape, out, want))


def test_a_zero_difference_slice_gives_a_zero_loss_term_and_a_zero_target_slice_inf():
    from uno_amd import _native
    shape = (2, 2, 1, 3, 500, 3)
    B, T_in, F, Cm, P, T = shape
    inp, _ = problem(shape)
    inp = dict(inp)
    inp["frames"] = inp["frames"].clone()
    inp["frames"][1, 2] = inp["target"][1, 2]            # ||d|| = 0 at the last frame of batch entry 1 ...
    inp["frames"][0, 0] = inp["target"][0, 0]            # ... and at frame 0 of batch entry 0
    inp["gh"] = torch.zeros_like(inp["gh"])              # nothing through the lifts: gframe is the loss term alone
    out = run(shape, inp)
    assert torch.isfinite(out["gseed"]).all() and float(out["gseed"][1].abs().max()) == 0.0 and float(out["gseed"][0].abs().max()) > 0.0
    g0 = out["gframe"][1]
    assert torch.isfinite(g0).all() and float(g0[0].abs().max()) == 0.0 and float(g0[1].abs().max()) > 0.0
    inp["target"] = inp["target"].clone()
    inp["target"][0, 2] = 0                              # a zero target slice: inf, as torch gives
    out = run(shape, inp)
    assert torch.isinf(out["gseed"][0]).any() and torch.isfinite(out["gseed"][1]).all()


def test_binding_refuses_what_the_kernels_do_not_take():
    from uno_amd import _native
    D = dev()
    B, T_in, F, Cm, P, T = 2, 3, 2, 4, 12, 4
    z = lambda *s: torch.zeros(*s, device=D)
    given, pred, target, feat, w, bias = z(B, T_in, P), z(B, T, P), z(B, T, P), z(F, P), z(Cm, T_in + F), z(Cm)
    gh, sums, gL, gpred, gframe = z(B, Cm, P), torch.ones(B, T, 2, device=D), torch.ones(1, device=D), z(B, T, P), z(B, P)
    parts = _native.rollout_lift_bwd_ws(B, T_in, F, Cm, P, T, D)
    _native.rollout_lift(given, pred, feat, w, bias, 1)                                                    # the good calls
    _native.rollout_lift_backward(gh, given, pred, target, feat, w, sums, gL, gpred, gframe, parts, 1)
    _native.rollout_loss_seed(pred, target, sums, gL, gframe)
    wide = z(B, T_in, 2 * P)
    for bad in (given.double(), wide[:, :, ::2], z(B, T_in, P + 1), given.cpu()):                          # dtype, density, shape, device
        with pytest.raises(RuntimeError):
            _native.rollout_lift(bad, pred, feat, w, bias, 1)
        with pytest.raises(RuntimeError):
            _native.rollout_lift_backward(gh, bad, pred, target, feat, w, sums, gL, gpred, gframe, parts, 1)
    for bad in (gh.double(), z(B, Cm, 2 * P)[:, :, ::2], z(B, Cm + 1, P), gh.cpu()):
        with pytest.raises(RuntimeError):
            _native.rollout_lift_backward(bad, given, pred, target, feat, w, sums, gL, gpred, gframe, parts, 1)
    with pytest.raises(RuntimeError):
        _native.rollout_lift(given, pred, feat, z(Cm, T_in + F + 1), bias, 1)                             # weight columns
    with pytest.raises(RuntimeError):
        _native.rollout_lift_backward(gh, given, pred, target, feat, w, sums, gL, gpred, gframe, parts[:8], 1)      # a workspace too small
    with pytest.raises(RuntimeError):
        _native.rollout_lift_backward(gh, given, pred, target, feat, w, sums, gL, gpred, z(B, P + 1), parts, 1)
    with pytest.raises(RuntimeError):
        _native.rollout_loss_seed(pred, target, sums.double(), gL, gframe)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _native.rollout_lift(given, pred, feat, w, bias, T)                                                # t = T
    with pytest.raises(RuntimeError, match="bad sizes"):
        _native.rollout_lift_backward(gh, given, pred, target, feat, w, sums, gL, gpred, gframe, parts, T)
    with pytest.raises(RuntimeError, match="at most 32"):
        _native.rollout_lift(z(B, 31, P), pred, feat, z(Cm, 33), bias, 1)                                  # C = 33
    with pytest.raises(RuntimeError, match="<= 32"):
        _native.rollout_lift_bwd_ws(B, 31, 2, Cm, P, T, D)
    with pytest.raises(RuntimeError, match="at most 64"):
        _native.rollout_lift(given, pred, feat, z(65, T_in + F), z(65), 1)                                 # Cm = 65
    with pytest.raises(RuntimeError, match="at most 256"):
        _native.rollout_lift(given, z(B, 257, P), feat, w, bias, 1)


# ------------------------------------------------------------------------------------------------------------------ model level
def test_golden_case_native_on_the_device():
    from uno_amd.harness import UNO, ns2d_rollout_loss
    c = Case(load_cases("harness_ns.npz")[0], "ns2d")
    torch.manual_seed(21)
    model = UNO(14, 4)
    check_init(model, c)
    model = model.to(dev())
    xx, yy = torch.from_numpy(c.xx).to(dev()), torch.from_numpy(c.yy).to(dev())
    loss = ns2d_rollout_loss(model, xx, yy, T_f=2, step=1, native=True)
    loss.backward()
    d = abs(float(loss.detach()) - float(c.loss)) / abs(float(c.loss))
    print(f"[ns2d golden, native training roll-out] loss against the recorded loss {d:.2e}")
    assert d < 1e-5
    check_grads(model, c, 5e-4)


def _flat_grads(model):
    return torch.cat([(torch.view_as_real(p.grad) if p.is_complex() else p.grad).detach().double().cpu().reshape(-1) for p in model.parameters()])


@pytest.mark.parametrize("name", ["UNO", "UNO_P"])
def test_native_against_default_with_float64_as_the_judge(name):
    """Measured on the MI355X (printed): the figures are in the module docstring."""
    from oracle import spectral_oracle as so
    from uno_amd import harness
    from uno_amd.harness import ns2d_rollout_loss
    T_f = 12
    torch.manual_seed(5)
    m32 = getattr(harness, name)(14, 4, block_cls=so.OracleOperatorBlock2d)
    state = {k: v.clone() for k, v in m32.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    xx, yy = torch.randn(2, 64, 64, 10, generator=g), torch.randn(2, 64, 64, T_f, generator=g)
    m64 = so.to_float64(m32)
    l64 = ns2d_rollout_loss(m64, xx.double(), yy.double(), T_f)
    l64.backward()
    g64, l64 = _flat_grads(m64), float(l64.detach())
    model = getattr(harness, name)(14, 4)
    model.load_state_dict(state)
    model = model.to(dev())
    err = {}
    for native in (False, True):
        for _ in range(2):                      # the second pass is the steady state (weight gradients batched over the roll-out)
            model.zero_grad(set_to_none=True)
            loss = ns2d_rollout_loss(model, xx.to(dev()), yy.to(dev()), T_f, native=native)
            loss.backward()
        err[native] = (float((_flat_grads(model) - g64).norm() / g64.norm()), abs(float(loss.detach()) - l64) / abs(l64))
    print(f"[{name}, T_f = {T_f}] against float64: default gradient {err[False][0]:.2e} loss {err[False][1]:.2e}; "
          f"native gradient {err[True][0]:.2e} loss {err[True][1]:.2e}")
    assert err[True][0] <= 2 * err[False][0]
    assert err[True][1] <= 2 * err[False][1]


@pytest.mark.parametrize("capturable", [False, True])
def test_graphed_step_on_the_native_loss_equals_the_eager_step(capturable):
    from uno_amd.harness import UNO, ComplexAdam, ns2d_rollout_loss
    D = dev()

    def make(cap):
        torch.manual_seed(5)
        m = UNO(14, 4).to(D)
        return m, ComplexAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=cap)
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(2, 64, 64, 10, generator=g).to(D), torch.randn(2, 64, 64, 3, generator=g).to(D)) for _ in range(3)]
    gs, _ = assert_graphed_step_equals_eager(make, lambda m, a, b: ns2d_rollout_loss(m, a, b, T_f=3, step=1, native=True), batches, capturable)
    assert gs.opt_in_graph == capturable
