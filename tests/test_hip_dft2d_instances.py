"""Every compiled instantiation of the pruned 2-D transforms K1 / K3 runs against float64.  pytest -m gpu

dft2d_fwd_kernel<NT, MT, VEC, R4, BF16>, dft2d_fwd_ft_kernel / dft2d_fwd_ht_kernel<NT, MT, R4>, dft2d_inv_kernel<KS, JT, BF16, TAB> and
dft2d_inv_ft_kernel<KS, JT> are 450 kernels, picked per call from the mode counts, the image width and the device's CU count.
tests/golden/dft2d_instances.json (tools/dft2d_instance_shapes.py) holds for each one that a call can reach a shape with the fewest
row tiles and a tall one (five row tiles or more, ragged last tile: several waves share an image); test_dft2d_instances_cpu.py proves
that the table and its UNREACHABLE list partition the compiled set.  One case per table entry:

  * the outputs live between guard bands filled with 0xA5 (RedZone of test_hip_redzone.py): an entry that is never written keeps
    the pattern (-2.9e-16 as a float: neither the reference's value nor the exact zero of a masked row), a store past the end damages
    a band;
  * the kernel that ran is the one the entry names (the library's launch records), so a dispatch change reads "regenerate the table"
    instead of silently moving the coverage;
  * relative L2 against the float64 oracle below TOL = 2e-5, as in test_hip_spectral2d.py (same flags, scales and references as its
    test_dft2d_forward_stage / test_dft2d_inverse_stage); images WRITTEN as bfloat16 cannot be that close to float64 (their final
    rounding alone is 1.1e-3 rms), they keep the TOL_BF16 = 3e-3 that test_hip_b16_transforms.py asserts for such images;
  * per entry, |got - ref| <= the worst-case float32 accumulation bound of that entry's sum (dft2d_instances.forward_bound /
    inverse_reference: derived, and confirmed on the float32 FFT by the CPU module), which a wrong or missing value in a ragged last
    mode tile cannot hide behind the energy of the rest; rows the later-wins mask kills are exactly zero.

And one grouped-layout case per template: two sources written into one spectrum tensor (out=, channel_offset), then the inverse of a
channel sub-range, bit-equal to the matching slice of the whole inverse (test_plane_kernels_grouped_spectrum_layout covers the
plane-batched kernels only)."""
import numpy as np
import pytest
import torch

import dft2d_instances as di
from conftest import rel_err
from test_hip_redzone import RedZone

pytestmark = pytest.mark.gpu
TOL = 2e-5
TOL_BF16 = 3e-3         # images written as bfloat16 (half an ulp is 2^-9 ... 2^-8 relative per element): test_hip_b16_transforms.py's
TABLE = di.load_table()
_TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


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


@pytest.mark.parametrize("entry", TABLE, ids=di.entry_id)
def test_instance_against_float64(entry, monkeypatch):
    from uno_amd import _native
    n, H, W, m1, m2 = entry["shape"]
    tdt = _TDT[entry["dtype"]]
    if entry["dir"] == "fwd":
        x = di.forward_input(entry)
        ref, bound, dead = di.forward_reference(entry, x)
        xd = cu(x).to(tdt)                                  # exact: x is already rounded to bf16 where the entry is bf16
        zone = RedZone(monkeypatch)
        got, ran = _profiled(lambda: _native.dft2d_forward(xd, m1, m2, scale=di.FWD_SCALE, hermitian_cols=True, mask_overlap=True))
    else:
        O = di.inverse_input(entry)
        ref, bound = di.inverse_reference(entry, O)
        Od = cu(O)
        zone = RedZone(monkeypatch)
        got, ran = _profiled(lambda: _native.dft2d_inverse(Od, H, W, scale=di.INV_SCALE, hermitian_cols=True, mask_overlap=True, dtype=tdt))
    assert zone.check(di.entry_id(entry)) == 1
    assert ran == [entry["name"]], f"dispatch changed: regenerate tests/golden/dft2d_instances.json (tools/dft2d_instance_shapes.py); ran {ran}"
    got = (got.float() if entry["dir"] == "inv" else got).cpu().numpy()
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got.view(np.float32)))
    err, excess = rel_err(got, ref), di.worst_excess(got, ref, bound)
    print(f"{di.entry_id(entry)}: rel L2 {err:.3g}, worst |got - ref| / bound {excess:.3g}")
    if entry["dir"] == "fwd":
        assert np.all(got[:, :, dead, :] == 0), "a spectrum row that the later-wins mask kills is not exactly zero"
    assert err < (TOL_BF16 if entry["dir"] == "inv" and entry["dtype"] == "bf16" else TOL)
    assert excess <= 1.0


def _grouped_entries():
    """per template, the tall float32 entry with the smallest image"""
    out = []
    for t in di.TEMPLATES:
        mine = [e for e in TABLE if di.template_of(e["name"]) == t and e["dtype"] == "f32" and e["shape"][1] >= 65]
        out.append(min(mine, key=lambda e: (e["shape"][1] * e["shape"][2], e["name"])))
    return out


@pytest.mark.parametrize("entry", _grouped_entries(), ids=lambda e: di.template_of(e["name"]))
def test_grouped_spectrum_layout(entry, monkeypatch):
    """two-source blocks: the kernels honour the (group, stride, offset) spectrum layout"""
    from uno_amd import _native
    _, H, W, m1, m2 = entry["shape"]
    B, C1, C2 = 2, 3, 2
    rng = np.random.default_rng(di.entry_seed(entry))
    x1 = rng.standard_normal((B, C1, H, W)).astype(np.float32)
    x2 = rng.standard_normal((B, C2, H, W)).astype(np.float32)
    x1d, x2d = cu(x1), cu(x2)
    zone = RedZone(monkeypatch)
    spec = torch.zeros((B, C1 + C2, 2 * m1, m2), dtype=torch.complex64, device=dev())

    def forward():
        _native.dft2d_forward(x1d, m1, m2, out=spec, channel_offset=0)
        _native.dft2d_forward(x2d, m1, m2, out=spec, channel_offset=C1)
    _, ran_fwd = _profiled(forward)
    ref = di.so.truncated_rfft2_dense(np.concatenate([x1, x2], axis=1), m1, m2) * (H * W)
    assert rel_err(spec.cpu().numpy(), ref) < TOL

    def inverse():
        return (_native.dft2d_inverse(spec, H, W, scale=1.0), _native.dft2d_inverse(spec, H, W, scale=1.0, channels=C1, channel_offset=0),
                _native.dft2d_inverse(spec, H, W, scale=1.0, channels=C2, channel_offset=C1))
    (whole, part1, part2), ran_inv = _profiled(inverse)
    assert zone.check(di.entry_id(entry)) == 4
    assert torch.equal(part1, whole[:, :C1]) and torch.equal(part2, whole[:, C1:])
    ran = ran_fwd if entry["dir"] == "fwd" else ran_inv
    assert ran == [entry["name"]] * len(ran) and len(ran) == (2 if entry["dir"] == "fwd" else 3), \
        f"dispatch changed: regenerate tests/golden/dft2d_instances.json; ran {ran_fwd + ran_inv}"
