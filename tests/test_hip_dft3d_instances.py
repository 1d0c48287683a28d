"""Every reachable instantiation of the one-workgroup-per-volume 3-D transforms K1v / K3v runs against float64.  pytest -m gpu

dft3d_fwd_volume_kernel<MT2, NBW, NARROW, U> and dft3d_inv_volume_kernel<MTS, U, NWT, NK2, A4> (csrc/dft3d_volume.hip) are 16 + 64 compiled
kernels, picked per call from the axis lengths and mode counts; 9 + 48 of them can be reached (test_dft3d_instances_cpu.py proves that
the table and its UNREACHABLE list partition the compiled set).  tests/golden/dft3d_instances.json (tools/dft3d_instance_shapes.py)
holds for each reachable one the smallest volume that reaches it and a stressed one (odd axes, ragged k-steps and mode tiles, corners
without a gap, the Nyquist bin, the largest LDS footprint ...), all with 48 volumes.  The C ABI has no bare 3-D transform, so each
kernel is reached through uno_spectral_conv3d_forward / _backward with channel counts that leave it alone on 48 volumes and make its
output observable (the mode GEMM takes a channel count of 1).  One case per table entry and form:

  forward, herm = 0    B = 48, Ci = Co = 1, the entry's grid going in: the returned truncated spectrum IS the kernel's output (rfftn, norm="forward", corner-major)
  inverse, herm = 1    the same call, the entry's grid coming out: y is the weighted inverse of xtrunc w; the float64 reference starts from the DEVICE's xtrunc
  forward, herm = 1    backward with B = 1, Ci = 1, Co = 48, no input gradient and an xtrunc of all 1 + 0j: the weight gradients are the
                       adjoint spectrum of gy itself (conj(1) gO, one term per entry), in so.spectral_conv3d_dense_bwd's convention
  inverse, herm = 0    backward with B = 1, Ci = 48, Co = 1: gx.  A COMPOSITE: gy is one volume, its transform takes the plane path, and
                       the bound is the sum of both stages' bounds (dft3d_instances.input_gradient_case)

Every case asserts that

  * the outputs live between guard bands filled with 0xA5 (RedZone of test_hip_redzone.py): an entry that is never written keeps the
    pattern, a store past the end damages a band;
  * the launch records hold exactly the kernel the entry names for the transform under test, so a dispatch change - or a slip of the
    Python mirror of the geometry that wrote the table - reads "regenerate the table";
  * everything is finite, and relative L2 against float64 is below the TOL = 2e-5 of test_hip_spectral3d.py;
  * per entry, |got - ref| <= the worst-case float32 accumulation bound of that entry's three-axis sum (dft3d_instances.forward_bound /
    inverse_bound: derived, and confirmed on the float32 FFT by the CPU module), which a wrong value in a ragged last k-step, a Nyquist
    slot or a narrow T block cannot hide behind the energy of the rest;
  * what the later-wins masks kill is exactly zero.  These kernels take no geometry whose corners overlap (2 m <= D in both `applies`
    functions), so for them the masks are all ones, which is what each case asserts.

The transform of a call that is NOT under test works on dft3d_instances.safe_grid (the layer resamples), so that a case does not lean on
an edge of a second kernel.

Single cases: the geometries one step beyond the LDS limit and a 47-volume call take the plane path and are right; the largest entry
of each direction gives the same bits twice."""
import numpy as np
import pytest
import torch

import dft3d_instances as d3
from conftest import rel_err
from oracle import spectral_oracle as so
from test_hip_redzone import RedZone

pytestmark = pytest.mark.gpu
TOL = 2e-5                  # test_hip_spectral3d.py's
TABLE = d3.load_table()
KERNELS = [e for e in TABLE if e["name"] != d3.PLANE_PATH]
REGENERATE = "dispatch changed: regenerate tests/golden/dft3d_instances.json (tools/dft3d_instance_shapes.py)"


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _profiled(fn):
    from uno_amd import _native
    _native.profile_begin(64)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ran = [n for n, _, _ in _native.profile_end()]
    return out, ran


def _volume_kernels(ran, direction):
    return [n for n in ran if f"dft3d_{direction}_volume_kernel" in n]


def _weights(e, n):
    m1, m2, m3 = e["shape"][4:]
    return d3.complex_input(e, (n, 4, m1, m2, m3), 1)


def _forward_call(x, w, dout):
    """x (B, D1, D2, D3), w (4, m1, m2, m3): Ci = Co = 1 -> (y (B, *dout), xtrunc (B, 4, m1, m2, m3), launch records)"""
    from uno_amd import _native
    xd, wd = cu(x[:, None]), [cu(w[k][None, None]) for k in range(4)]
    (y, xt), ran = _profiled(lambda: _native.spectral_conv3d_forward(xd, wd, *dout))
    return y[:, 0], xt[:, 0], ran


def _report(e, what, got, ref, bound):
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got.view(np.float32)))
    err, excess = rel_err(got, ref), d3.worst_excess(got, ref, bound)
    print(f"{d3.entry_id(e)} {what}: rel L2 {err:.3g}, worst |got - ref| / bound {excess:.3g}")
    assert err < TOL
    assert excess <= 1.0


def _no_overlap(e):
    """the later-wins masks of the entry's geometry are all ones (nothing for them to kill)"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    assert so._keep3d(D1, D2, m1, m2).all()


@pytest.mark.parametrize("herm", [0, 1])
@pytest.mark.parametrize("entry", [e for e in KERNELS if e["dir"] == "fwd"], ids=d3.entry_id)
def test_forward_instance_against_float64(entry, herm, monkeypatch):
    from uno_amd import _native
    n, D1, D2, D3, m1, m2, m3 = entry["shape"]
    x, ref, bound = d3.forward_case(entry, herm)
    _no_overlap(entry)
    if herm == 0:
        w = _weights(entry, 1)[0]
        zone = RedZone(monkeypatch)
        _, xt, ran = _forward_call(x, w, d3.safe_grid(entry))
        got = xt.cpu().numpy()
    else:
        # the adjoint on the output gradient: gy (1, 48, D1, D2, D3), xtrunc = 1 + 0j -> gw[c][0, o] = conj(1) gO[0, o, c]
        gy = cu(x[None])
        ones = torch.ones((1, 1, 4, m1, m2, m3), dtype=torch.complex64, device=dev())
        wd = [cu(v) for v in _weights(entry, n).transpose(1, 0, 2, 3, 4)[:, None]]                  # four (Ci = 1, Co = 48, m1, m2, m3)
        zone = RedZone(monkeypatch)
        (gx, gws), ran = _profiled(lambda: _native.spectral_conv3d_backward(gy, ones, wd, D1, D2, D3, need_gx=False))
        assert gx is None
        got = torch.stack([g[0] for g in gws], dim=1).cpu().numpy()
    assert zone.check(d3.entry_id(entry)) >= 2
    assert _volume_kernels(ran, "fwd") == [entry["name"]], f"{REGENERATE}; ran {ran}"
    _report(entry, f"herm {herm}", got, ref, bound)


@pytest.mark.parametrize("herm", [1, 0])
@pytest.mark.parametrize("entry", [e for e in KERNELS if e["dir"] == "inv"], ids=d3.entry_id)
def test_inverse_instance_against_float64(entry, herm, monkeypatch):
    """herm = 0 is a composite: see the module's docstring"""
    from uno_amd import _native
    n, D1, D2, D3, m1, m2, m3 = entry["shape"]
    _no_overlap(entry)
    if herm == 1:
        x, w = d3.other_input(entry, (n, *d3.safe_grid(entry))), _weights(entry, 1)[0]
        zone = RedZone(monkeypatch)
        y, xt, ran = _forward_call(x, w, (D1, D2, D3))
        ref, bound = d3.inverse_case(entry, xt.cpu().numpy(), w)
        got = y.cpu().numpy()
    else:
        gy, w = d3.other_input(entry, d3.safe_grid(entry)), _weights(entry, n)
        ref, bound = d3.input_gradient_case(entry, gy, w)
        gyd = cu(gy[None, None])
        wd = [cu(v) for v in w.transpose(1, 0, 2, 3, 4)[:, :, None]]                                # four (Ci = 48, Co = 1, m1, m2, m3)
        xt = torch.zeros((1, n, 4, m1, m2, m3), dtype=torch.complex64, device=dev())
        zone = RedZone(monkeypatch)
        (gx, _), ran = _profiled(lambda: _native.spectral_conv3d_backward(gyd, xt, wd, D1, D2, D3, need_gw=False))
        assert not _volume_kernels(ran, "fwd"), ran                                                  # one volume: the plane path
        got = gx[0].cpu().numpy()
    assert zone.check(d3.entry_id(entry)) >= 2
    assert _volume_kernels(ran, "inv") == [entry["name"]], f"{REGENERATE}; ran {ran}"
    _report(entry, f"herm {herm}", got, ref, bound)


def _whole_call_against_float64(e, n_vol, directions, monkeypatch):
    """the forward call on n_vol volumes of e's geometry: the transforms of `directions` must take the plane path, and the truncated
    spectrum and the output must be within TOL of float64 (dft3d_instances.truncated_dft3 / truncated_idft3: the dense oracle's sums)"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    x, w = d3.volumes_input(e)[:n_vol], _weights(e, 1)[0]
    zone = RedZone(monkeypatch)
    y, xt, ran = _forward_call(x, w, (D1, D2, D3))
    assert zone.check(d3.entry_id(e)) >= 2
    for direction in directions:
        assert not _volume_kernels(ran, direction), ran
    X = d3.truncated_dft3(x, m1, m2, m3) / (D1 * D2 * D3)
    keep = so._keep3d(D1, D2, m1, m2)
    y_ref = d3.truncated_idft3(X * d3.corner_cat(w[None].astype(np.complex128)) * keep[None, :, :, None], D1, D2, D3, so.hermitian_weights(D3, m3))
    y, xt = y.cpu().numpy(), xt.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(xt.view(np.float32)))
    err_x, err_y = rel_err(xt, d3.corner_major(X, m1, m2)), rel_err(y, y_ref)
    print(f"{d3.entry_id(e)} on {n_vol} volumes, plane path: rel L2 {err_x:.3g} (xtrunc), {err_y:.3g} (y)")
    assert err_x < TOL and err_y < TOL


@pytest.mark.parametrize("entry", [e for e in TABLE if e["name"] == d3.PLANE_PATH], ids=d3.entry_id)
def test_one_step_beyond_the_lds_limit_takes_the_plane_path(entry, monkeypatch):
    """the fall-back is chosen, for the transform whose limit the geometry passes, and the call is right"""
    assert d3.kernel_name(entry["dir"], tuple(entry["shape"])) == d3.PLANE_PATH
    _whole_call_against_float64(entry, entry["shape"][0], [entry["dir"]], monkeypatch)


@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_47_volumes_take_the_plane_path(direction, monkeypatch):
    """one volume fewer than VOL_MIN_VOLUMES on a geometry that otherwise fits both kernels"""
    fits = [e for e in KERNELS if e["dir"] == direction and e["role"] == "stressed"
            and d3.kernel_name("fwd", tuple(e["shape"])) != d3.PLANE_PATH != d3.kernel_name("inv", tuple(e["shape"]))]
    _whole_call_against_float64(fits[0], d3.VOL_MIN_VOLUMES - 1, ["fwd", "inv"], monkeypatch)


@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_largest_entry_is_deterministic(direction):
    e = max((e for e in KERNELS if e["dir"] == direction), key=lambda e: (np.prod(e["shape"][1:4]), e["name"]))
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    x, w = d3.volumes_input(e), _weights(e, 1)[0]
    y1, xt1, ran1 = _forward_call(x, w, (D1, D2, D3))
    y2, xt2, ran2 = _forward_call(x, w, (D1, D2, D3))
    assert _volume_kernels(ran1, direction) == _volume_kernels(ran2, direction) == [e["name"]], f"{REGENERATE}; ran {ran1}"
    assert torch.equal(xt1, xt2) if direction == "fwd" else torch.equal(y1, y2)
