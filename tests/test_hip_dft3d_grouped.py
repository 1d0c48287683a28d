"""The 3-D transforms as stages of their own (uno_dft3d_forward_grouped / uno_dft3d_inverse_grouped) with a grouped placement on the
spectrum side, and the two-source 3-D layer built on them (uno_spectral_conv3d_forward2 / _backward2).  pytest -m gpu

A grouped call runs the kernel, the launch and the data of the plain call on the same source: only the address of the spectrum moves.
So every comparison of a grouped with a plain call here is BIT equality, and the rest of the shared spectrum tensor must keep the bits
it had (NaN before the first source is written).  The forward cases run under the red-zone fixture (tests/test_hip_redzone.py): a store
outside the spectrum tensor fails the test instead of corrupting memory.  The plain stage calls are held to float64 with the references
and bounds of tests/dft3d_instances.py (derived there) - the first direct test of the transform dispatch outside the whole layer.

Cases (D1, D2, D3; m1, m2, m3), dispatch per tests/dft3d_instances.kernel_name (asserted below):
    V  (12,10,6; 5,4,3)  B=4, Ca=12, Cb=20   48 / 80 volumes: K1v <1,1,false,1> / K3v <1,1,1,2,false>
    P  (9,10,7; 3,4,3)   B=2, Ca=3,  Cb=5    plane path, odd axes
    T  (9,10,40; 3,4,3)  B=2, Ca=24, Cb=24   plane path because D3 > 32
    G  (44,6,4; 41,2,2)  B=2, Ca=1,  Cb=2    leading axis on the any-mode kernel (m1 > 40), overlapping corners
    M  (12,10,6; 5,4,3)  B=4, Ca=8,  Cb=16   32 volumes -> plane path, 64 -> K1v, in one spectrum tensor"""
import numpy as np
import pytest
import torch

import dft3d_instances as d3
from test_hip_redzone import RedZone
from uno_amd import _native

pytestmark = pytest.mark.gpu

CASES = {
    "V": ((12, 10, 6), (5, 4, 3), 4, 12, 20),
    "P": ((9, 10, 7), (3, 4, 3), 2, 3, 5),
    "T": ((9, 10, 40), (3, 4, 3), 2, 24, 24),
    "G": ((44, 6, 4), (41, 2, 2), 2, 1, 2),
    "M": ((12, 10, 6), (5, 4, 3), 4, 8, 16),
}
K1V, K3V = "uno::dft3d_fwd_volume_kernel<1, 1, false, 1>", "uno::dft3d_inv_volume_kernel<1, 1, 1, 2, false>"


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _sources(key, seed):
    grid, modes, B, Ca, Cb = CASES[key]
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, Ca, *grid, generator=g).to(dev())
    b = torch.randn(B, Cb, *grid, generator=g).to(dev())
    return grid, modes, B, Ca, Cb, a, b


def test_the_cases_take_the_paths_their_names_say():
    """host only: the geometry mirror of the dispatch"""
    def name(direction, key, C):
        grid, modes, B, _, _ = CASES[key]
        return d3.kernel_name(direction, (B * C, *grid, *modes))
    assert name("fwd", "V", 12) == name("fwd", "V", 20) == name("fwd", "V", 32) == K1V
    assert name("inv", "V", 12) == name("inv", "V", 20) == name("inv", "V", 32) == K3V
    for key in ("P", "T", "G"):
        _, _, _, Ca, Cb = CASES[key]
        assert {name(d, key, C) for d in ("fwd", "inv") for C in (Ca, Cb, Ca + Cb)} == {d3.PLANE_PATH}, key
    assert name("fwd", "M", 8) == d3.PLANE_PATH and name("fwd", "M", 16) == K1V
    assert CASES["G"][1][0] > 40 and 2 * CASES["G"][1][0] > CASES["G"][0][0]           # the any-mode leading axis, overlapping corners


@pytest.mark.parametrize("adjoint", [False, True], ids=["plain-dft", "adjoint"])
@pytest.mark.parametrize("key", list(CASES))
def test_grouped_forward_writes_its_channel_range_and_nothing_else(key, adjoint, monkeypatch):
    zone = RedZone(monkeypatch)
    grid, modes, B, Ca, Cb, a, b = _sources(key, 1)
    scale = 1.0 if adjoint else 1.0 / (grid[0] * grid[1] * grid[2])
    spec = torch.empty((B, Ca + Cb, 4, *modes), dtype=torch.complex64, device=dev())
    torch.view_as_real(spec).fill_(float("nan"))
    nan_bits = _bits(spec).clone()
    plain_a = _native.dft3d_forward(a, modes=modes, scale=scale, adjoint=adjoint)
    plain_b = _native.dft3d_forward(b, modes=modes, scale=scale, adjoint=adjoint)
    assert plain_a.shape == (B, Ca, 4, *modes) and not bool(torch.isnan(torch.view_as_real(plain_a)).any())
    out = _native.dft3d_forward(a, out=spec, scale=scale, adjoint=adjoint, group=Ca, offset=0)
    assert out is spec
    assert _same_bits(spec[:, :Ca], plain_a)
    assert torch.equal(_bits(spec[:, Ca:]), nan_bits[:, Ca:])           # the other source's channels: untouched, still the NaN written above
    _native.dft3d_forward(b, out=spec, scale=scale, adjoint=adjoint, group=Cb, offset=Ca)
    assert _same_bits(spec[:, Ca:], plain_b)
    assert _same_bits(spec[:, :Ca], plain_a)
    assert zone.check(f"grouped forward {key}") >= 5


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("key", ["V", "P", "G"])
def test_grouped_inverse_reads_its_channel_range_where_it_lies(key, weighted):
    grid, modes, B, Ca, Cb = CASES[key]
    g = torch.Generator().manual_seed(2)
    spec = torch.randn(B, Ca + Cb, 4, *modes, dtype=torch.complex64, generator=g).to(dev())
    before = spec.clone()
    want = _native.dft3d_inverse(spec[:, Ca:].contiguous(), grid, scale=0.5, weighted=weighted)
    got = _native.dft3d_inverse(spec, grid, scale=0.5, weighted=weighted, group=Cb, offset=Ca)
    assert got.shape == (B, Cb, *grid) and _same_bits(got, want)
    want = _native.dft3d_inverse(spec[:, :Ca].contiguous(), grid, scale=0.5, weighted=weighted)
    got = _native.dft3d_inverse(spec, grid, scale=0.5, weighted=weighted, group=Ca, offset=0)
    assert _same_bits(got, want)
    assert _same_bits(spec, before)


@pytest.mark.parametrize("key", ["V", "P"])
def test_plain_stage_calls_against_float64(key):
    """group = 0: forward (both `adjoint` values) and inverse (both `weighted` values) within forward_bound / inverse_bound of the
    float64 transforms of tests/dft3d_instances.py"""
    grid, modes, B, Ca, _ = CASES[key]
    D1, D2, D3 = grid
    m1, m2, m3 = modes
    n = B * Ca
    shape = (n, *grid, *modes)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, *grid)).astype(np.float32)
    S = d3.truncated_dft3(x, m1, m2, m3)
    l1 = np.abs(x.astype(np.float64)).sum(axis=(1, 2, 3))
    xd = torch.from_numpy(x).to(dev()).view(B, Ca, *grid)
    for adjoint in (False, True):
        scale = 1.0 if adjoint else 1.0 / (D1 * D2 * D3)
        c = d3.so.hermitian_weights(D3, m3) if adjoint else np.ones(m3)
        got = _native.dft3d_forward(xd, modes=modes, scale=scale, adjoint=adjoint).view(n, 4, *modes).cpu().numpy()
        excess = d3.worst_excess(got, d3.corner_major(S * (scale * c), m1, m2), d3.forward_bound(shape, l1, scale, c))
        print(f"[{key}] forward, adjoint={adjoint}: worst |error| / bound {excess:.3f}")
        assert excess <= 1.0
    O = (rng.standard_normal((n, 4, *modes)) + 1j * rng.standard_normal((n, 4, *modes))).astype(np.complex64)
    Od = torch.from_numpy(O).to(dev()).view(B, Ca, 4, *modes)
    for weighted in (False, True):
        scale = 1.0 / (D1 * D2 * D3) if not weighted else 1.0
        c = d3.so.hermitian_weights(D3, m3) if weighted else np.ones(m3)
        got = _native.dft3d_inverse(Od, grid, scale=scale, weighted=weighted).view(n, *grid).cpu().numpy()
        Oc = d3.corner_cat(O)
        excess = d3.worst_excess(got, scale * d3.truncated_idft3(Oc, D1, D2, D3, c), d3.inverse_bound(shape, Oc, scale, c))
        print(f"[{key}] inverse, weighted={weighted}: worst |error| / bound {excess:.3f}")
        assert excess <= 1.0


@pytest.mark.parametrize("key", ["V", "P"])
def test_two_source_layer_equals_the_layer_on_the_concatenation(key, monkeypatch):
    """uno_spectral_conv3d_forward2 / _backward2 against the one-source calls on torch.cat: xtrunc, y, gx1 | gx2 and the four gw bit-equal
    (every kernel sees the same values per volume; each source takes the transform path the concatenation takes)"""
    zone = RedZone(monkeypatch)
    grid, modes, B, Ca, Cb, a, b = _sources(key, 4)
    Co = 12 if key == "V" else 2
    out = (grid[0] + 2, grid[1], grid[2] + 2)
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(Ca + Cb, Co, *modes, dtype=torch.complex64, generator=g).to(dev()) for _ in range(4)]
    gy = torch.randn(B, Co, *out, generator=g).to(dev())
    y1, xt1 = _native.spectral_conv3d_forward(torch.cat([a, b], dim=1), ws, *out)
    y2, xt2 = _native.spectral_conv3d_forward2(a, b, ws, *out)
    assert _same_bits(xt2, xt1) and _same_bits(y2, y1)
    gx, gw = _native.spectral_conv3d_backward(gy, xt1, ws, *grid)
    gx1, gx2, gw2 = _native.spectral_conv3d_backward2(gy, xt2, ws, Ca, *grid)
    assert _same_bits(gx1, gx[:, :Ca]) and _same_bits(gx2, gx[:, Ca:])
    assert all(_same_bits(p, q) for p, q in zip(gw2, gw))
    gx1, gx2, gw2 = _native.spectral_conv3d_backward2(gy, xt2, ws, Ca, *grid, need_gx=False)
    assert gx1 is None and gx2 is None and all(_same_bits(p, q) for p, q in zip(gw2, gw))
    assert zone.check(f"two-source layer {key}") >= 10
