"""uno_rel_l2_forward / uno_rel_l2_backward (K20, uno_amd/csrc/rel_l2_loss.hip) through harness.LpLoss and harness.losses.rel_l2 on the
MI355X: value, per-row ratios and the gradient against float64 on the host from the same float32 inputs.

Bounds: 1e-5 relative for the value and for every `ratio` entry - the project's bound for a loss value (TOL_PRED of the harness tests) -
and 1e-5 by conftest.rel_err for the gradient.  Ceilings, not targets.  Measured on the MI355X (the largest of value, ratio and
gradient error over the four flag combinations, printed per case):
    case                 value / ratio   gradient
    1x1                  1.9e-8          7.5e-8
    3x49                 6.9e-8          8.6e-8
    2x20011              5.2e-8          5.0e-8
    2x1600               4.4e-8          1.1e-7
    2x8200               9.0e-8          7.9e-8
    4x4096-slice7of40    1.1e-7          6.8e-8
    2x1023-pitch1024     9.8e-8          6.4e-8
    1x4099               8.3e-8          9.7e-8
    1x300001             7.4e-8          3.2e-8
    2x30x30-crop         1.1e-7          7.0e-8      (the stock path)

The cases are the smallest at which the kernels can go wrong; what each exercises is written beside it."""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
FLAGS = [(True, True), (False, True), (True, False), (False, False)]          # (size_average, reduction)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# name -> (B, N, layout).  layout: how x and y lie in memory (make_views)
CASES = {
    "1x1": (1, 1, "dense"),                       # the smallest problem
    "3x49": (3, 49, "dense"),                     # odd N: rows 1 and 2 start misaligned - 4-byte loads
    "2x20011": (2, 20011, "dense"),               # five chunks with a ragged last one, 4-byte loads
    "2x1600": (2, 1600, "dense"),                 # Darcy at S = 40: one chunk, 16-byte loads
    "2x8200": (2, 8200, "dense"),                 # 16-byte loads over three chunks, the last of 8 elements
    "4x4096-slice7of40": (4, 4096, "slice"),      # out[..., 7] of a (4, 4096, 40) tensor: element stride 40 in both operands
    "2x1023-pitch1024": (2, 1023, "pitch"),       # N % 4 != 0 on aligned rows: 16-byte loads + three single elements; dense gradient rows misaligned
    "1x4099": (1, 4099, "dense"),                 # B = 1, N % 4 != 0: a second chunk of three single elements, 16-byte loads and stores
    "1x300001": (1, 300001, "dense"),             # beyond 64 * 4096 elements: 64 larger chunks
    "2x30x30-crop": (2, 900, "crop"),             # a cropped plane (three strides): the stock path, still right
}


def make_views(name, x, y):
    """host (B, N) tensors -> device tensors that hold the same values in the case's layout, as LpLoss is handed them"""
    B, N, layout = CASES[name]
    xd, yd = x.to(dev()), y.to(dev())
    if layout == "dense":
        return xd, yd
    if layout == "slice":                           # ns_train_3d.py:58-61: k, l = out[..., t], y[..., t]; k.view(B, -1)
        bx, by = (torch.randn(B, 64, 64, 40, generator=torch.Generator().manual_seed(s)).to(dev()) for s in (11, 12))
        bx[..., 7], by[..., 7] = xd.view(B, 64, 64), yd.view(B, 64, 64)
        return bx[..., 7].view(B, -1), by[..., 7].view(B, -1)
    if layout == "pitch":
        bx, by = (torch.randn(B, N + 1, generator=torch.Generator().manual_seed(s)).to(dev()) for s in (13, 14))
        bx[:, :N], by[:, :N] = xd, yd
        return bx[:, :N], by[:, :N]
    bx, by = (torch.randn(B, 32, 32, generator=torch.Generator().manual_seed(s)).to(dev()) for s in (15, 16))
    bx[:, :30, :30], by[:, :30, :30] = xd.view(B, 30, 30), yd.view(B, 30, 30)
    return bx[:, :30, :30], by[:, :30, :30]


@functools.lru_cache(maxsize=None)
def problem(name, seed=0, equal_row=None, zero_row=None):
    """(x, y, u) on the host - u a random upstream vector - and the float64 results from them (computed once, never modified)"""
    B, N, _ = CASES[name]
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + N)
    y = torch.randn(B, N, generator=g)
    x = y + 0.1 * torch.randn(B, N, generator=g)
    u = torch.randn(B, generator=g)
    if equal_row is not None:
        x[equal_row] = y[equal_row]
    if zero_row is not None:
        y[zero_row] = 0
    x64, y64 = x.double(), y.double()
    num, den = ((x64 - y64) ** 2).sum(1), (y64 ** 2).sum(1)
    ratio = num.sqrt() / den.sqrt()
    unit = (x64 - y64) / (num.sqrt() * den.sqrt()).unsqueeze(1)         # d ratio_b / d x_b
    return x, y, u, {"ratio": ratio, "unit": unit}


def lp_loss(**kw):
    from uno_amd.harness import LpLoss
    return LpLoss(**kw)


def run(name, x, y, u, size_average, reduction):
    """LpLoss(size_average, reduction) forward and backward on the case's layout -> (value, gradient at x as (B, N)), device tensors"""
    B, N, layout = CASES[name]
    xv, yv = make_views(name, x, y)
    leaf = xv.detach().clone().requires_grad_(True) if layout == "dense" else None
    if leaf is None:                                # the views' base is the leaf: the gradient comes back through the view
        base = xv._base.detach().clone().requires_grad_(True)
        xv = {"slice": lambda b: b[..., 7].view(B, -1), "pitch": lambda b: b[:, :N], "crop": lambda b: b[:, :30, :30]}[layout](base)
    else:
        xv = leaf
    out = lp_loss(size_average=size_average, reduction=reduction)(xv, yv)
    (out if reduction else (out * u.to(dev())).sum()).backward()
    if leaf is not None:
        return out.detach(), leaf.grad.view(B, N)
    grad = {"slice": lambda b: b[..., 7], "pitch": lambda b: b[:, :N], "crop": lambda b: b[:, :30, :30]}[layout](base.grad)
    return out.detach(), grad.reshape(B, N)


def expected(want, u, size_average, reduction):
    B = want["ratio"].shape[0]
    if not reduction:
        return want["ratio"], want["unit"] * u.double().unsqueeze(1)
    value = want["ratio"].mean() if size_average else want["ratio"].sum()
    return value, want["unit"] * (1.0 / B if size_average else 1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(name):
    """Measured on the MI355X: the figures are in the module docstring."""
    x, y, u, want = problem(name)
    worst_v = worst_g = 0.0
    for size_average, reduction in FLAGS:
        value, grad = run(name, x, y, u, size_average, reduction)
        v64, g64 = expected(want, u, size_average, reduction)
        assert value.is_cuda and value.dtype == torch.float32 and value.shape == v64.shape
        ev = float(((value.double().cpu() - v64).abs() / v64.abs()).max())
        eg = float(rel_err(grad.double().cpu().numpy(), g64.numpy()))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    print(f"[lp_loss {name}] value / ratio {worst_v:.2e}, gradient {worst_g:.2e}")
    assert worst_v <= TOL and worst_g <= TOL


def test_native_path_is_taken_where_it_applies_and_only_there(monkeypatch):
    """every case but the cropped plane reaches uno_rel_l2_forward; the crop, float64, p = 1 and a target that requires grad do not"""
    from uno_amd import _native
    calls = []
    real = _native.rel_l2_forward
    monkeypatch.setattr(_native, "rel_l2_forward", lambda *a: (calls.append(1), real(*a))[1])
    for name in CASES:
        x, y, u, _ = problem(name)
        xv, yv = make_views(name, x, y)
        before = len(calls)
        lp_loss(size_average=False)(xv, yv)
        assert len(calls) - before == (0 if CASES[name][2] == "crop" else 1), name
    x, y, _, _ = problem("3x49")
    xd, yd = x.to(dev()), y.to(dev())
    before = len(calls)
    lp_loss(size_average=False)(xd.double(), yd.double())
    lp_loss(p=1, size_average=False)(xd, yd)
    lp_loss(size_average=False)(xd, yd.clone().requires_grad_(True))
    lp_loss(size_average=False)(x, y)                                     # host tensors
    assert len(calls) == before
    with torch.no_grad():                                                 # no gradient is recorded: the target's flag does not matter
        lp_loss(size_average=False)(xd, yd.clone().requires_grad_(True))
    assert len(calls) == before + 1


def test_chunk_counts_are_a_function_of_n_alone():
    from uno_amd import _native
    L = _native.lib()
    chunks = lambda B, N: L.uno_rel_l2_ws_bytes(B, N) // (8 * B)
    assert [chunks(2, n) for n in (1, 4096, 4097, 20011, 262144, 262145, 300001, 10 ** 9)] == [1, 1, 2, 5, 64, 64, 64, 64]
    assert chunks(7, 20011) == chunks(1, 20011) and L.uno_rel_l2_ws_bytes(0, 5) == 0 and L.uno_rel_l2_ws_bytes(2, 0) == 0


def test_rel_l2_returns_the_ratios_and_takes_a_summed_gradient():
    """harness.losses.rel_l2 -> (B,); `.sum().backward()` hands the kernel one expanded value"""
    from uno_amd.harness.losses import rel_l2
    x, y, u, want = problem("2x8200")
    xd = x.to(dev()).requires_grad_(True)
    r = rel_l2(xd, y.to(dev()))
    assert r.shape == (2,)
    r.sum().backward()
    assert float(((r.detach().double().cpu() - want["ratio"]).abs() / want["ratio"]).max()) <= TOL
    assert rel_err(xd.grad.double().cpu().numpy(), want["unit"].numpy()) <= TOL


def test_a_row_with_x_equal_to_y_gets_a_zero_gradient():
    x, y, u, want = problem("3x49", equal_row=1)
    for size_average, reduction in FLAGS:
        value, grad = run("3x49", x, y, u, size_average, reduction)
        assert bool((grad[1] == 0).all()) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(value).all())
        keep = torch.tensor([0, 2])
        _, g64 = expected(want, u, size_average, reduction)
        assert rel_err(grad[keep].double().cpu().numpy(), g64[keep].numpy()) <= TOL


def test_a_zero_target_row_gives_inf_as_stock_and_leaves_the_other_rows_alone():
    from uno_amd.harness import lp_loss_rel_sum
    x, y, u, want = problem("2x1600", zero_row=0)
    value, grad = run("2x1600", x, y, u, False, False)
    assert float(value[0]) == float("inf")
    assert abs(float(value[1]) - float(want["ratio"][1])) <= TOL * float(want["ratio"][1])
    assert rel_err(grad[1].double().cpu().numpy(), (want["unit"][1] * float(u[1])).numpy()) <= TOL
    total, _ = run("2x1600", x, y, u, False, True)
    assert float(total) == float("inf") == float(lp_loss_rel_sum(x.to(dev()), y.to(dev())))
    z = torch.zeros(1, 10, device=dev())
    assert torch.isnan(lp_loss(size_average=False)(z, z))               # 0 / 0, as torch.norm(.) / torch.norm(.) gives


def same_bits(a, b):
    # (inf == inf and the comparison is of bits, not values: view as integers)
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def both_passes(xd, yd, ud):
    """forward and backward of the three reductions on device tensors -> [ratios, sum, mean, their three gradients]"""
    out = []
    grads = []
    for size_average, reduction in ((True, False), (False, True), (True, True)):
        leaf = xd.detach().requires_grad_(True)
        v = lp_loss(size_average=size_average, reduction=reduction)(leaf, yd)
        (v if reduction else (v * ud).sum()).backward()
        out.append(v.detach().reshape(-1))
        grads.append(leaf.grad)
    return out + grads


@pytest.mark.parametrize("name", ["3x49", "2x20011", "2x8200", "4x4096-slice7of40"])
def test_two_calls_give_the_same_bits(name):
    x, y, u, _ = problem(name)
    xv, yv = make_views(name, x, y)
    assert same_bits(both_passes(xv, yv, u.to(dev())), both_passes(xv, yv, u.to(dev())))


def test_reserved_cus_do_not_change_the_bits():
    from uno_amd import _native
    x, y, u, _ = problem("2x20011")
    xd, yd, ud = x.to(dev()), y.to(dev()), u.to(dev())
    before = both_passes(xd, yd, ud)
    prev = _native.reserve_cus(16)
    try:
        under = both_passes(xd, yd, ud)
    finally:
        _native.reserve_cus(prev)
    assert same_bits(before, under)


def test_graph_replay_of_forward_and_backward_gives_the_eager_bits_on_fresh_inputs():
    name = "2x8200"
    x, y, u, _ = problem(name)
    fx, fy, fu, want = problem(name, seed=1)
    sx, sy, su = x.to(dev()), y.to(dev()), u.to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # eager warm-up off the default stream, as capture requires
        both_passes(sx, sy, su)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = both_passes(sx, sy, su)
    sx.copy_(fx.to(dev()))
    sy.copy_(fy.to(dev()))
    su.copy_(fu.to(dev()))
    graph.replay()
    torch.cuda.synchronize()
    eager = both_passes(fx.to(dev()), fy.to(dev()), fu.to(dev()))
    assert same_bits(captured, eager)
    assert float(((captured[0].double().cpu() - want["ratio"]).abs() / want["ratio"]).max()) <= TOL
    assert rel_err(captured[4].double().cpu().numpy(), want["unit"].numpy()) <= TOL


@pytest.mark.parametrize("name", ["3x49", "2x20011", "2x1023-pitch1024", "1x4099", "4x4096-slice7of40"])
def test_outputs_and_workspace_stay_inside_their_allocations(name, monkeypatch):
    """the forward record (sums, ratio, total and the workspace in one allocation) and the gradient each sit between two poisoned 64 KiB
    guard bands (tests/test_hip_redzone.py): the bands are untouched after a forward and a backward pass."""
    from test_hip_redzone import RedZone
    from uno_amd import _native
    x, y, u, want = problem(name)
    xv, yv = make_views(name, x, y)
    zone = RedZone(monkeypatch)
    record = _native.rel_l2_forward(xv, yv)
    sums, ratio, total = _native.rel_l2_views(record, xv.shape[0])
    gx = _native.rel_l2_backward(xv, yv, sums, u.to(dev()), 1.0)
    assert zone.check(f"rel_l2 {name}") == 2
    assert float(((ratio.double().cpu() - want["ratio"]).abs() / want["ratio"]).max()) <= TOL
    assert abs(float(total) - float(want["ratio"].sum())) <= TOL * float(want["ratio"].sum())
    assert rel_err(gx.double().cpu().numpy(), (want["unit"] * u.double().unsqueeze(1)).numpy()) <= TOL


@pytest.mark.parametrize("name", ["3x49", "2x20011", "1x4099", "4x4096-slice7of40"])
def test_results_do_not_depend_on_what_empty_memory_held(name, monkeypatch):
    """plain, 0xFF- and 0x7F-filled torch.empty memory (tests/test_hip_uninit.py): finite, bit-equal values and gradients"""
    from test_hip_redzone import _same
    from test_hip_uninit import BYTES, Poison
    x, y, u, _ = problem(name)
    xv, yv = make_views(name, x, y)
    ud = u.to(dev())
    plain = both_passes(xv, yv, ud)
    torch.cuda.synchronize()
    for byte in BYTES:
        with monkeypatch.context() as patch:
            zone = Poison(patch, byte)
            got = both_passes(xv, yv, ud)
            n = zone.check(f"lp_loss {name} under 0x{byte:02X}")
        _same(got, plain, f"lp_loss {name} under 0x{byte:02X}")
        assert n >= 6, n                            # three passes of the forward record and the gradient


def test_binding_refuses_what_the_kernels_do_not_take():
    from uno_amd import _native
    x = torch.zeros(2, 12, device=dev())
    for bad in (x.double(), x[:, :8], x.cpu()):                                 # dtype, shape, device of one operand
        with pytest.raises(RuntimeError):
            _native.rel_l2_forward(x, bad)
    for bad in (x.double(), x.cpu(), x.view(2, 3, 4), x[:, :0]):                # dtype, device, rank, no elements in both
        with pytest.raises(RuntimeError):
            _native.rel_l2_forward(bad, bad)
    sums, _, _ = _native.rel_l2_views(_native.rel_l2_forward(x + 1, x + 2), 2)
    g = torch.ones(2, device=dev())
    for bad_sums, bad_g in ((sums[:1], g), (sums.double(), g), (sums.reshape(-1), g), (sums, torch.ones(3, device=dev())), (sums, g.double()), (sums, g.cpu())):
        with pytest.raises(RuntimeError):
            _native.rel_l2_backward(x + 1, x + 2, bad_sums, bad_g)
    L = _native.lib()
    p = _native._ptr(x)
    assert L.uno_rel_l2_forward(p, 12, 1, p, 12, 1, p, p, p, p, 2, 0, None) < 0 and b"bad sizes" in L.uno_last_error()
    assert L.uno_rel_l2_forward(p, -12, 1, p, 12, 1, p, p, p, p, 2, 12, None) < 0 and b"strides" in L.uno_last_error()
    assert L.uno_rel_l2_forward(p, 12, 1, None, 12, 1, p, p, p, p, 2, 12, None) < 0 and b"null" in L.uno_last_error()
    assert L.uno_rel_l2_backward(p, 12, 1, p, 12, 1, p, p, 2, 1.0, p, 2, 12, None) < 0 and b"g_per_row" in L.uno_last_error()
    assert L.uno_rel_l2_forward(None, 0, 0, None, 0, 0, None, None, None, None, 0, 5, None) == 0          # B == 0: nothing to do
    assert L.uno_rel_l2_backward(None, 0, 0, None, 0, 0, None, None, 0, 1.0, None, 0, 5, None) == 0
