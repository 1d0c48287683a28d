"""Short-row window calls (uno_channel_mix2_rows, uno_channel_mix2_rows_grad, uno_channel_wgrad2_rows, uno_channel_mix_act_padded_rows,
uno_dgelu_rows): the two ends of the NS-3D models on the time window inside the padded tensors (reference navier_stokes_uno3d.py:304-318,
358-382).  Every windowed call is compared with float64 on the CPU from a contiguous crop, as tests/test_hip_window.py does for the image
windows.  pytest -m gpu

Bounds: those of the dense kernels (tests/test_hip_channel_mix.py) - 2e-6 for outputs and input gradients, 2e-5 for weight and bias
gradients (relative L2 against float64)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL_OUT, TOL_W = 2e-6, 2e-5

# (rows, cols, pitch, col0, extra elements at the end of every plane)
GEOMS = [
    (25, 9, 10, 0, 0), (25, 9, 10, 1, 0),            # T9
    (64, 10, 12, 0, 0), (64, 10, 14, 2, 0),          # T10, and padded on both sides
    (49, 20, 24, 0, 0), (49, 20, 28, 4, 0),          # T20, and padded on both sides
    (7, 40, 52, 6, 0),                               # a T40-like window
    (3, 1, 5, 2, 0),                                 # one column
    (300, 33, 33, 0, 0),                             # the window is the plane, odd width
    (1024, 64, 70, 3, 0),                            # several workgroups
    (49, 20, 28, 4, 37),                             # a tail behind the rows of every plane
]
CHANNELS = [(4, 2, 8), (16, 8, 32), (64, 32, 128), (5, 3, 7), (1, 0, 1)]
# the full product of the geometries and the channel sets at B = 2, and one case at B = 1
CASES = [(g, c, 2) for g in GEOMS for c in CHANNELS]
CASES += [(GEOMS[3], (16, 8, 32), 1)]
IDS = ["r{}c{}p{}o{}t{}-{}_{}_{}-B{}".format(*g, *c, B) for g, c, B in CASES]
POISON = -3.0e30


def rel(a, b):
    d = (a.double().cpu() - b.double().cpu()).norm().item()
    n = b.double().norm().item()
    return d / n if n > 0 else d


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def crop64(t, geom):
    """(B, C, plane) -> float64 CPU (B, C, rows * cols): the window as a contiguous tensor"""
    rows, cols, pitch, col0, _ = geom
    B, C = t.shape[:2]
    return t[:, :, :rows * pitch].reshape(B, C, rows, pitch)[..., col0:col0 + cols].reshape(B, C, rows * cols).double().cpu()


def border(t, geom):
    """the border columns of the rows of every plane, and the tail behind the rows"""
    rows, cols, pitch, col0, _ = geom
    v = t[:, :, :rows * pitch].reshape(*t.shape[:2], rows, pitch)
    return torch.cat([v[..., :col0].reshape(-1), v[..., col0 + cols:].reshape(-1)]), t[:, :, rows * pitch:]


def operands(geom, ch, B, seed):
    rows, cols, pitch, col0, extra = geom
    C1, C2, Co = ch
    g = torch.Generator().manual_seed(seed)
    plane = rows * pitch + extra
    x1 = torch.randn(B, C1, plane, generator=g).cuda()
    x2 = torch.randn(B, C2, plane, generator=g).cuda() if C2 else None
    w = (torch.randn(Co, C1 + C2, generator=g) / (C1 + C2) ** 0.5).cuda()
    b = torch.randn(Co, generator=g).cuda()
    gy = torch.randn(B, Co, rows * cols, generator=g).cuda()
    return x1, x2, w, b, gy, plane


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("act", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("geom,ch,B", CASES, ids=IDS)
def test_forward_on_the_window_against_float64(geom, ch, B, act):
    from uno_amd import _native
    x1, x2, w, b, _, plane = operands(geom, ch, B, 11)
    keep1, keep2 = x1.clone(), None if x2 is None else x2.clone()
    win = geom[:4]
    y = _native.channel_mix2_rows(x1, x2, w, b, win, act_in=act)
    a1 = crop64(x1, geom)
    xs = torch.cat([gelu64(a1) if act else a1] + ([crop64(x2, geom)] if x2 is not None else []), 1)
    ref = torch.matmul(w.double().cpu(), xs) + b.double().cpu().view(1, -1, 1)
    e = rel(y, ref)
    print(f"forward {geom} {ch} B={B} act={act}: {e:.2e}")
    assert y.shape == (B, ch[2], geom[0] * geom[1]) and e < TOL_OUT
    assert torch.equal(x1, keep1) and (x2 is None or torch.equal(x2, keep2))          # the sources are read only
    # repeated calls, and a call with compute units set aside, give the same bits
    for _ in range(9):
        assert bits_equal(_native.channel_mix2_rows(x1, x2, w, b, win, act_in=act), y)
    prev = _native.reserve_cus(16)
    try:
        assert bits_equal(_native.channel_mix2_rows(x1, x2, w, b, win, act_in=act), y)
    finally:
        assert _native.reserve_cus(prev) == 16
    # a bias-free call
    y0 = _native.channel_mix2_rows(x1, x2, w, None, win, act_in=act)
    assert rel(y0, ref - b.double().cpu().view(1, -1, 1)) < TOL_OUT


@pytest.mark.parametrize("act", [False, True], ids=["plain", "dgelu"])
@pytest.mark.parametrize("geom,ch,B", CASES, ids=IDS)
def test_input_gradients_whole_planes_in_one_pass(geom, ch, B, act):
    from uno_amd import _native
    from uno_amd._native import _opt, _ptr, _stream, lib
    rows, cols, pitch, col0, extra = geom
    C1, C2, Co = ch
    x1, x2, w, _, gy, plane = operands(geom, ch, B, 12)
    keep = x1.clone()

    def call(fill):
        g1 = torch.full((B, C1, plane), fill).cuda()
        g2 = torch.full((B, C2, plane), fill).cuda() if C2 else None
        rc = lib().uno_channel_mix2_rows_grad(_ptr(gy), _ptr(w), C1, _opt(x1 if act else None), _ptr(g1), _opt(g2), B, C1 + C2, Co,
                                              rows, cols, pitch, col0, plane, _stream(gy))
        assert rc == 0, lib().uno_last_error()
        return g1, g2

    g1, g2 = call(POISON)
    gx = torch.matmul(w.double().cpu().t(), gy.double().cpu())
    r1 = gx[:, :C1] * (dgelu64(crop64(x1, geom)) if act else 1.0)
    e1 = rel(crop64(g1, geom), r1)
    print(f"input gradient {geom} {ch} B={B} dgelu={act}: g1 {e1:.2e}", end="")
    assert e1 < TOL_OUT
    outs = [g1]
    if C2:
        e2 = rel(crop64(g2, geom), gx[:, C1:])
        print(f", g2 {e2:.2e}", end="")
        assert e2 < TOL_OUT
        outs.append(g2)
    print()
    for t in outs:
        cols_out, tail = border(t, geom)
        assert torch.equal(cols_out.view(torch.int32), torch.zeros_like(cols_out).view(torch.int32))         # exactly +0.0f
        assert tail.numel() == B * t.shape[1] * extra and bool((tail == POISON).all())                       # the tail is not touched
    assert torch.equal(x1, keep)
    # what the outputs held does not matter; repeated calls and reserved compute units give the same bits
    for fill in (float("nan"), 7.25):
        h1, h2 = call(fill)
        n = rows * pitch
        assert bits_equal(h1[:, :, :n], g1[:, :, :n]) and (not C2 or bits_equal(h2[:, :, :n], g2[:, :, :n]))
    for _ in range(9):
        h1, h2 = call(POISON)
        assert bits_equal(h1, g1) and (not C2 or bits_equal(h2, g2))
    prev = _native.reserve_cus(16)
    try:
        h1, h2 = call(POISON)
        assert bits_equal(h1, g1) and (not C2 or bits_equal(h2, g2))
    finally:
        assert _native.reserve_cus(prev) == 16
    # the first source's gradient alone (g2 == NULL)
    if C2:
        only, none = _native.channel_mix2_rows_grad(gy, w, C1, geom[:4], plane, need_g2=False, dgelu_of=x1 if act else None)
        assert none is None and bits_equal(only[:, :, :rows * pitch], g1[:, :, :rows * pitch])


@pytest.mark.parametrize("act", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("geom,ch,B", CASES, ids=IDS)
def test_weight_gradient_on_the_window_against_float64(geom, ch, B, act):
    from uno_amd import _native
    C1, C2, Co = ch
    x1, x2, w, _, gy, plane = operands(geom, ch, B, 13)
    # operands with a mean: an entry of a weight gradient is one dot product over B * rows * cols pixels, and between zero-mean operands it is
    # a cancellation residue - the single entry of the 1 -> 1 layer on (25, 9, 10, 0) is -0.0092 out of sum |terms| = 280, where torch's own
    # float32 sum is 1.2e-4 off and this kernel 2.2e-4 (7e-9 of sum |terms|); a relative bound says nothing of such an entry
    x1, gy = x1 + 0.5, gy + 0.5
    x2 = None if x2 is None else x2 + 0.5
    keep1 = x1.clone()
    win = geom[:4]
    gw, gb = _native.channel_wgrad2_rows(gy, x1, x2, win, need_bias=True, act_x=act)
    a1 = crop64(x1, geom)
    xs = torch.cat([gelu64(a1) if act else a1] + ([crop64(x2, geom)] if x2 is not None else []), 1)
    rw = torch.einsum("bop,bip->oi", gy.double().cpu(), xs)
    rb = gy.double().cpu().sum((0, 2))
    ew, eb = rel(gw, rw), rel(gb, rb)
    print(f"weight gradient {geom} {ch} B={B} act={act}: gw {ew:.2e}, gb {eb:.2e}")
    assert gw.shape == (Co, C1 + C2) and ew < TOL_W and eb < TOL_W
    assert torch.equal(x1, keep1)
    # accumulate: added to what the buffers hold; otherwise what they held does not matter
    base_w, base_b = torch.randn(Co, C1 + C2).cuda(), torch.randn(Co).cuda()
    aw, ab = base_w.clone(), base_b.clone()
    _native.channel_wgrad2_rows(gy, x1, x2, win, need_bias=True, act_x=act, out_w=aw, out_b=ab, accumulate=True)
    assert rel(aw, base_w.double().cpu() + rw) < TOL_W and rel(ab, base_b.double().cpu() + rb) < TOL_W
    for fill in (float("nan"), 7.25):
        fw, fb = torch.full((Co, C1 + C2), fill).cuda(), torch.full((Co,), fill).cuda()
        _native.channel_wgrad2_rows(gy, x1, x2, win, need_bias=True, act_x=act, out_w=fw, out_b=fb, accumulate=False)
        assert bits_equal(fw, gw) and bits_equal(fb, gb)
    for _ in range(9):
        hw, hb = _native.channel_wgrad2_rows(gy, x1, x2, win, need_bias=True, act_x=act)
        assert bits_equal(hw, gw) and bits_equal(hb, gb)
    prev = _native.reserve_cus(16)
    try:
        hw, hb = _native.channel_wgrad2_rows(gy, x1, x2, win, need_bias=True, act_x=act)
        assert bits_equal(hw, gw) and bits_equal(hb, gb)
    finally:
        assert _native.reserve_cus(prev) == 16
    nw, nb = _native.channel_wgrad2_rows(gy, x1, x2, win, need_bias=False, act_x=act)
    assert nb is None and bits_equal(nw, gw)


@pytest.mark.parametrize("act", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("geom,ch,B", [c for c in CASES if c[0][4] == 0], ids=[i for i, c in zip(IDS, CASES) if c[0][4] == 0])
def test_padded_activation_and_its_backward(geom, ch, B, act):
    """uno_channel_mix_act_padded_rows writes the dense pre-activation and the zero-padded activation; uno_dgelu_rows takes the padded
    gradient back to the dense pre-activation"""
    from uno_amd import _native
    from uno_amd._native import _opt, _ptr, _stream, lib
    rows, cols, pitch, col0, _ = geom
    Ci, Co = ch[0] + ch[1], ch[2]
    g = torch.Generator().manual_seed(14)
    x = torch.randn(B, Ci, rows * cols, generator=g).cuda()
    w, b = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).cuda(), torch.randn(Co, generator=g).cuda()
    keep = x.clone()
    win = geom[:4]
    y, actp = _native.channel_mix_act_padded_rows(x, w, b, win, act_in=act, keep_y=True)
    ref = torch.matmul(w.double().cpu(), gelu64(x.double().cpu()) if act else x.double().cpu()) + b.double().cpu().view(1, -1, 1)
    ey, ea = rel(y, ref), rel(crop64(actp, geom), gelu64(ref))
    print(f"padded activation {geom} {Ci}->{Co} B={B} act_in={act}: y {ey:.2e}, act {ea:.2e}")
    assert actp.shape == (B, Co, rows * pitch) and ey < TOL_OUT and ea < TOL_OUT
    pad, tail = border(actp, geom)
    assert tail.numel() == 0 and torch.equal(pad.view(torch.int32), torch.zeros_like(pad).view(torch.int32))       # +0.0f on both sides
    assert torch.equal(x, keep)
    dense = _native.channel_mix(x, w, b, act_in=act)
    print(f"    y against the dense uno_channel_mix call: {rel(y, dense):.2e}, bit-equal: {bits_equal(y, dense)}")
    assert rel(y, dense) < 2 * TOL_OUT          # (two float32 sums in different orders, each within TOL_OUT of float64)
    # without the dense output; pre-filled outputs; repeats; reserved compute units
    none, act2 = _native.channel_mix_act_padded_rows(x, w, b, win, act_in=act, keep_y=False)
    assert none is None and bits_equal(act2, actp)
    for fill in (float("nan"), 7.25):
        fy, fa = torch.full_like(y, fill), torch.full_like(actp, fill)
        rc = lib().uno_channel_mix_act_padded_rows(_ptr(x), _ptr(w), _opt(b), _ptr(fy), _ptr(fa), B, Ci, Co, rows, cols, pitch, col0,
                                                   1 if act else 0, _stream(x))
        assert rc == 0 and bits_equal(fy, y) and bits_equal(fa, actp)
    for _ in range(9):
        hy, ha = _native.channel_mix_act_padded_rows(x, w, b, win, act_in=act)
        assert bits_equal(hy, y) and bits_equal(ha, actp)
    prev = _native.reserve_cus(16)
    try:
        hy, ha = _native.channel_mix_act_padded_rows(x, w, b, win, act_in=act)
        assert bits_equal(hy, y) and bits_equal(ha, actp)
    finally:
        assert _native.reserve_cus(prev) == 16
    if act:
        return
    # backward of the padding and the GELU
    gp = torch.randn(B, Co, rows * pitch, generator=g).cuda()
    keep_g = gp.clone()
    gz = _native.dgelu_rows(y, gp, win)
    ez = rel(gz, dgelu64(y.double().cpu()) * crop64(gp, geom))
    print(f"dgelu {geom}: {ez:.2e}")
    assert ez < TOL_OUT and torch.equal(gp, keep_g)
    for _ in range(9):
        assert bits_equal(_native.dgelu_rows(y, gp, win), gz)


def test_dgelu_rows_with_a_tail_behind_the_rows():
    from uno_amd import _native
    geom = GEOMS[-1]
    rows, cols, pitch, col0, extra = geom
    g = torch.Generator().manual_seed(15)
    pre = torch.randn(2, 5, rows * cols, generator=g).cuda()
    gp = torch.randn(2, 5, rows * pitch + extra, generator=g).cuda()
    gz = _native.dgelu_rows(pre, gp, geom[:4])
    assert rel(gz, dgelu64(pre.double().cpu()) * crop64(gp, geom)) < TOL_OUT
