"""K1-FD (csrc/dft2d_fwd_fd_kernel.h): the forward transform that also writes the banded resampling of its input, from one read.

Kernel level - _native.dft2d_forward_resample against two float64 references:
  spectrum         the dense truncated DFT of the oracle, at the bound tests/test_hip_spectral2d.py holds dft2d_forward to (relative L2
                   error < 2e-5);
  resampled image  A x B^T evaluated in float64 with the float32 weights the kernels apply.  The bound is measured, not chosen: K7
                   (resample_forward / resample_adjoint, the kernel the fused call replaces) runs on the same input inside the test,
                   and the fused kernel's relative L2 error may be at most twice K7's - both are float32 sums of the same <= 9 + 9
                   products taken in a different order (K7: rows, then columns; here: columns, then rows), nothing else differs.
Shapes: H in {16, 30, 33, 46} = one tile, a 14-row last tile, a 1-row last tile, three tiles with rows carried across two seams; W the
narrowest (416, even) and the widest (447, odd) admitted row; the forward 2:1 operator and the adjoint of the 1:2 up-sampling; 1, 5 and
4 k + 1 images (a partial last workgroup); modes (18, 18) and (4, 5); both sweep directions; reserved CUs.

Block level - OperatorBlock_2D with block2d.FUSE_FORWARD_RESAMPLE on and off (down-sampling block: forward; up-sampling one- and
two-source blocks: backward), against each other and against the oracle block on the host."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import spectral_oracle as so
from test_hip_redzone import RedZone
from test_hip_uninit import Poison

pytestmark = pytest.mark.gpu
TOL = 2e-5              # tests/test_hip_spectral2d.py: every stage against the float64 dense oracle
K7_FACTOR = 2.0         # the resampled image: at most twice K7's own error against the same float64 reference
WMIN, WMAX = 416, 447   # the admitted rows


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _operators(H, W, adjoint):
    """(A (Ho, H), B (Wo, W)) float64 from the float32 weights, (Ho, Wo) = (H // 2, W // 2)"""
    from uno_amd.resample import _matrix
    Ho, Wo = H // 2, W // 2
    if adjoint:
        return _matrix(Ho, H).t().double(), _matrix(Wo, W).t().double()
    return _matrix(H, Ho).double(), _matrix(W, Wo).double()


def _k7(x, adjoint):
    from uno_amd.resample import resample_adjoint, resample_forward
    H, W = x.shape[-2:]
    return (resample_adjoint if adjoint else resample_forward)(x, H // 2, W // 2)


def _fused(x, m1, m2, adjoint, scale=0.5, herm=False, mask=False):
    from uno_amd import _native
    from uno_amd.resample import fused_resample_tables
    H, W = x.shape[-2:]
    Ho, Wo = H // 2, W // 2
    tabs = fused_resample_tables(H, W, Ho, Wo, str(x.device), adjoint)
    assert tabs is not None
    assert _native.dft2d_forward_resample_applies(x.shape[0] * x.shape[1], H, W, m1, m2, Ho, Wo, tabs[1].shape[1])
    return _native.dft2d_forward_resample(x, m1, m2, Ho, Wo, tabs, scale, herm, mask)


def _spectrum_ref(x, m1, m2, scale, herm, mask):
    H, W = x.shape[-2:]
    ref = so.truncated_rfft2_dense(x, m1, m2) * (H * W) * scale
    if herm:
        ref = ref * so.hermitian_weights(W, m2)[None, None, None, :]
    if mask:
        ref = ref * so.later_wins_mask(H, m1)[None, None, :, None]
    return ref


def _check(x, m1, m2, adjoint, herm, what):
    """one fused call on x (n, 1, H, W) against both references; -> (spectrum, image) of the call"""
    H, W = x.shape[-2:]
    xd = torch.from_numpy(x).to(dev())
    spec, img = _fused(xd, m1, m2, adjoint, 0.5, herm, herm)
    assert tuple(spec.shape) == (x.shape[0], 1, 2 * m1, m2) and tuple(img.shape) == (x.shape[0], 1, H // 2, W // 2)
    e_spec = rel_err(spec.cpu().numpy(), _spectrum_ref(x, m1, m2, 0.5, herm, herm))
    A, B = _operators(H, W, adjoint)
    ref = torch.einsum("ih,nchw,jw->ncij", A, torch.from_numpy(x).double(), B).numpy()
    e_new, e_k7 = rel_err(img.cpu().numpy(), ref), rel_err(_k7(xd, adjoint).cpu().numpy(), ref)
    print(f"[fwd_resample] {what}: spectrum {e_spec:.2e} (< {TOL:.0e}); image fused {e_new:.2e}, K7 {e_k7:.2e} (bound {K7_FACTOR * e_k7:.2e})")
    assert e_spec < TOL
    assert e_new <= K7_FACTOR * e_k7
    return spec, img


class _Pinned:
    """sweep direction of the K1 family pinned for the block ("forward" / "reversed"), restored afterwards"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from uno_amd import _native
        self.prev = _native.sweep_direction(self.mode, 1) if self.mode == "reversed" else _native.lib().uno_sweep_alternation(0)

    def __exit__(self, *exc):
        from uno_amd import _native
        _native.lib().uno_sweep_alternation(self.prev)


# n_img and the mode class rotate over the shapes so that every value meets every H
CASES = [(H, W, adjoint) for H in (16, 30, 33, 46) for W in (WMIN, WMAX) for adjoint in (False, True)]


@pytest.mark.parametrize("H,W,adjoint", CASES, ids=[f"{h}x{w}{'T' if a else ''}" for h, w, a in CASES])
def test_fused_call_against_float64_and_k7(H, W, adjoint):
    k = CASES.index((H, W, adjoint))
    n = (1, 5)[(k + k // 4) % 2]
    m1, m2 = (18, 18) if (H >= 30 and k % 2 == 0) else (4, 5)
    x = np.random.default_rng(4000 + k).standard_normal((n, 1, H, W)).astype(np.float32)
    with _Pinned("forward"):
        spec, img = _check(x, m1, m2, adjoint, herm=adjoint, what=f"{n} x {H}x{W} modes ({m1}, {m2}) adjoint={adjoint}")
    with _Pinned("reversed"):            # only the order of the images changes
        spec_r, img_r = _fused(torch.from_numpy(x).to(dev()), m1, m2, adjoint, 0.5, adjoint, adjoint)
    assert torch.equal(spec, spec_r) and torch.equal(img, img_r)


@pytest.mark.parametrize("direction", ["forward", "reversed"])
def test_partial_last_workgroup(direction):
    """four images per workgroup once the images fill the CUs: 4 k + 1 images leave the last workgroup - the FIRST under the reversed
    sweep - with one"""
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    n, H, W = 4 * cus + 1, 16, WMIN
    x = np.random.default_rng(5).standard_normal((n, 1, H, W)).astype(np.float32)
    with _Pinned(direction):
        _check(x, 4, 5, False, herm=False, what=f"{n} images, {direction}")


def test_reserved_cus():
    """8 usable CUs: 33 images are eight workgroups of four and one of one; three tiles per image"""
    from uno_amd import _native
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    x = np.random.default_rng(6).standard_normal((33, 1, 46, WMAX)).astype(np.float32)
    prev = _native.reserve_cus(cus - 8)
    try:
        spec, img = _check(x, 18, 18, True, herm=True, what="33 images on 8 CUs")
    finally:
        _native.reserve_cus(prev)
    spec2, img2 = _fused(torch.from_numpy(x).to(dev()), 18, 18, True, 0.5, True, True)
    assert torch.equal(spec, spec2) and torch.equal(img, img2)          # the geometry changes nothing but the grouping


def test_grouped_spectrum_layout_and_determinism():
    from uno_amd import _native
    from uno_amd.resample import fused_resample_tables
    B, C1, Ct, H, W, m1, m2 = 2, 3, 5, 33, WMAX, 4, 5
    x = torch.randn(B, C1, H, W, device=dev())
    tabs = fused_resample_tables(H, W, H // 2, W // 2, str(x.device), False)
    plain, img = _native.dft2d_forward_resample(x, m1, m2, H // 2, W // 2, tabs, 0.25)
    out = torch.zeros(B, Ct, 2 * m1, m2, dtype=torch.complex64, device=dev())
    got, img2 = _native.dft2d_forward_resample(x, m1, m2, H // 2, W // 2, tabs, 0.25, out=out, channel_offset=2)
    assert got is out and torch.equal(out[:, 2:], plain) and not bool(out[:, :2].any())
    assert torch.equal(img, img2)                                       # two launches: bit for bit
    assert torch.equal(plain, _native.dft2d_forward(x, m1, m2, 0.25)) or rel_err(plain.cpu().numpy(), _native.dft2d_forward(x, m1, m2, 0.25).cpu().numpy()) < TOL


def test_red_zone(monkeypatch):
    """sentinels around every output the call allocates (spectrum and image), ragged last tile, partial last column group"""
    rz = RedZone(monkeypatch)
    for H, W, adjoint, n in ((33, WMAX, False, 5), (46, WMIN, True, 3), (16, WMAX, True, 1)):
        x = torch.randn(n, 1, H, W, device=dev())
        _fused(x, 4, 5, adjoint)
        _fused(x, 18 if H >= 30 else 4, 18 if H >= 30 else 4, adjoint, herm=True, mask=True)
    rz.check("dft2d_forward_resample")


@pytest.mark.parametrize("byte", [0xFF, 0x7F], ids=["ff", "7f"])
def test_outputs_do_not_depend_on_what_empty_memory_held(monkeypatch, byte):
    """the outputs start from NaN-patterned torch.empty memory (and the call follows launches that left their own data in the LDS): every
    element is written, none is read before"""
    x = torch.randn(5, 1, 33, WMAX, device=dev())
    clean = [_fused(x, 18, 18, a, herm=a, mask=a) for a in (False, True)]
    ps = Poison(monkeypatch, byte)
    dirty = [_fused(x, 18, 18, a, herm=a, mask=a) for a in (False, True)]
    assert ps.check("dft2d_forward_resample") >= 4
    for (s0, i0), (s1, i1) in zip(clean, dirty):
        assert bool(torch.isfinite(torch.view_as_real(s1)).all()) and bool(torch.isfinite(i1).all())
        assert torch.equal(s0, s1) and torch.equal(i0, i1)


# ------------------------------------------------------------------------------------------------------------------ block level
def _block_run(blk, xs, gy, cat):
    y = blk.forward_cat(xs) if cat else blk(xs[0])
    return [y.detach()] + [g.detach() for g in torch.autograd.grad(y, list(xs) + list(blk.parameters()), gy)]


@pytest.mark.parametrize("kind", ["down", "up", "up_cat"])
def test_operator_block_with_and_without_the_fused_call(kind, monkeypatch):
    """down: 46 x 447 -> 23 x 223 (the fused call in the forward pass, conv0's class); up / up_cat: 23 x 223 -> 46 x 447 (in the backward
    pass of the one- and the two-source block, conv5's class).  Switch on against switch off, and both against the oracle block."""
    from uno_amd import _native, block2d
    from uno_amd.integral_operators import OperatorBlock_2D
    torch.manual_seed(11)
    hw, out_hw = ((46, WMAX), (23, WMAX // 2)) if kind == "down" else ((23, WMAX // 2), (46, WMAX))
    chans = (2, 2) if kind == "up_cat" else (2,)
    ref = so.OracleOperatorBlock2d(sum(chans), 3, out_hw[0], out_hw[1], 4, 4)
    blk = OperatorBlock_2D(sum(chans), 3, out_hw[0], out_hw[1], 4, 4)
    blk.load_state_dict(ref.state_dict(), strict=True)
    blk = blk.to(dev())
    xs_cpu = [torch.randn(1, c, *hw, requires_grad=True) for c in chans]
    xs = [t.detach().to(dev()).requires_grad_(True) for t in xs_cpu]
    y_ref = ref(torch.cat(xs_cpu, dim=1))
    gy = torch.randn_like(y_ref)
    want = [y_ref.detach()] + [g for g in torch.autograd.grad(y_ref, xs_cpu + list(ref.parameters()), gy)]

    runs = {}
    for on in (True, False):
        monkeypatch.setattr(block2d, "FUSE_FORWARD_RESAMPLE", on)
        _native.profile_begin(256)
        try:
            runs[on] = _block_run(blk, xs, gy.to(dev()), kind == "up_cat")
            torch.cuda.synchronize()
        finally:
            names = [n for n, _, _ in _native.profile_end()]
        assert any("dft2d_fwd_fd_kernel" in n for n in names) == on, names
    gmax = max(float(torch.linalg.vector_norm(w)) for w in want[1:])
    for i, (a, b, w) in enumerate(zip(runs[True], runs[False], want)):
        n = float(torch.linalg.vector_norm(w))
        e_on, e_off = float(torch.linalg.vector_norm(a.cpu() - w)), float(torch.linalg.vector_norm(b.cpu() - w))
        e_ab = float(torch.linalg.vector_norm(a - b))
        print(f"[fwd_resample block {kind}] tensor {i}: on/off {e_ab / max(n, 1e-30):.2e}, on/oracle {e_on / max(n, 1e-30):.2e}, off/oracle {e_off / max(n, 1e-30):.2e}")
        floor = 0.0 if i == 0 else 1e-6 * gmax
        assert e_ab <= TOL * n + floor
        assert e_on <= TOL * n + floor and e_off <= TOL * n + floor
