"""K1-FD (csrc/dft2d_fwd_fd_kernel.h) on its second window of row lengths, 192 .. 223 floats - the 223^2 level of the Darcy model, two
output columns per lane.  The structure, references and tolerances of tests/test_hip_fwd_resample.py (the 416 .. 447 window), unchanged:

Kernel level - _native.dft2d_forward_resample against
  spectrum         the float64 dense truncated DFT of the oracle at relative L2 error < 2e-5, and _native.dft2d_forward (K1 alone) at the
                   same bound;
  resampled image  A x B^T in float64 with the float32 weights of resample._matrix: at most twice the error of K7 (resample_forward /
                   resample_adjoint, the kernel the fused call replaces) on the same input; K7's result itself is then within the sum of
                   the two errors.
Shapes: W at both ends of the window (192: Wo = 96, even; 223: Wo = 111, the model's); H in {17, 33, 40, 223} = a 1-row last tile, a
1-row third tile, an 8-row third tile, the model's 14 tiles; the forward 2:1 operator and the adjoint of the 1:2 up-sampling; 1, 3 and 9
images, 4 k + 1 images once the images fill the CUs (a partial last workgroup), reserved CUs; the three mode classes instantiated,
(18, 18) / (17, 18) -> <2, 3, 1>, (8, 8) -> <1, 1, 2>, (4, 4) -> <1, 1, 1>; both sweep directions.  Every output starts from 0xFF bytes
(NaN) as in tests/test_hip_uninit.py.

Block level - one row length just outside each end (191, 224): dft2d_forward_resample_applies refuses it and OperatorBlock_2D still matches
the oracle block through the K7 + K1 pair; inside the window the block launches the fused kernel and matches as well."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import spectral_oracle as so
from test_hip_fwd_resample import K7_FACTOR, TOL, _Pinned, _k7, _operators, _spectrum_ref
from test_hip_redzone import RedZone
from test_hip_uninit import Poison

pytestmark = pytest.mark.gpu
WMIN, WMAX = 192, 223   # the admitted rows of the second window
MODES = [(18, 18), (8, 8), (4, 4)]          # <2, 3, 1>, <1, 1, 2>, <1, 1, 1>


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _fused(x, m1, m2, adjoint, scale=0.5, herm=False, mask=False):
    from uno_amd import _native
    from uno_amd.resample import fused_resample_tables
    H, W = x.shape[-2:]
    Ho, Wo = H // 2, W // 2
    tabs = fused_resample_tables(H, W, Ho, Wo, str(x.device), adjoint)
    assert tabs is not None
    assert _native.dft2d_forward_resample_applies(x.shape[0] * x.shape[1], H, W, m1, m2, Ho, Wo, tabs[1].shape[1])
    return _native.dft2d_forward_resample(x, m1, m2, Ho, Wo, tabs, scale, herm, mask)


def _check(x, m1, m2, adjoint, herm, what):
    """one fused call on x (n, 1, H, W) against the float64 references, K1 alone and K7 alone; -> (spectrum, image) of the call"""
    from uno_amd import _native
    H, W = x.shape[-2:]
    xd = torch.from_numpy(x).to(dev())
    spec, img = _fused(xd, m1, m2, adjoint, 0.5, herm, herm)
    assert tuple(spec.shape) == (x.shape[0], 1, 2 * m1, m2) and tuple(img.shape) == (x.shape[0], 1, H // 2, W // 2)
    e_spec = rel_err(spec.cpu().numpy(), _spectrum_ref(x, m1, m2, 0.5, herm, herm))
    k1 = _native.dft2d_forward(xd, m1, m2, 0.5, herm, herm)
    e_k1 = rel_err(spec.cpu().numpy(), k1.cpu().numpy())
    A, B = _operators(H, W, adjoint)
    ref = torch.einsum("ih,nchw,jw->ncij", A, torch.from_numpy(x).double(), B).numpy()
    k7 = _k7(xd, adjoint).cpu().numpy()
    e_new, e_k7, e_pair = rel_err(img.cpu().numpy(), ref), rel_err(k7, ref), rel_err(img.cpu().numpy(), k7)
    print(f"[fwd_resample_223] {what}: spectrum {e_spec:.2e} vs float64, {e_k1:.2e} vs K1 (< {TOL:.0e}); image fused {e_new:.2e}, "
          f"K7 {e_k7:.2e} (bound {K7_FACTOR * e_k7:.2e}), fused vs K7 {e_pair:.2e}")
    assert e_spec < TOL and e_k1 < TOL
    assert e_new <= K7_FACTOR * e_k7
    assert e_pair <= (1.0 + K7_FACTOR) * e_k7 * 1.001       # the triangle inequality on the two bounds above, no bound of its own
    return spec, img


# n_img and the mode class rotate over the shapes so that every value meets every H and both operators
CASES = [(H, W, adjoint) for H in (17, 33, 40, 223) for W in (WMIN, WMAX) for adjoint in (False, True)]


@pytest.mark.parametrize("H,W,adjoint", CASES, ids=[f"{h}x{w}{'T' if a else ''}" for h, w, a in CASES])
def test_fused_call_against_float64_k1_and_k7(H, W, adjoint, monkeypatch):
    k = CASES.index((H, W, adjoint))
    n = (1, 3, 9)[(k + k // 4) % 3]
    m1, m2 = MODES[(k + k // 2) % 3]
    m1 = min(m1, H)                             # 17 rows: (17, 18), still <2, 3, 1>
    x = np.random.default_rng(7000 + k).standard_normal((n, 1, H, W)).astype(np.float32)
    ps = Poison(monkeypatch, 0xFF)
    with _Pinned("forward"):
        spec, img = _check(x, m1, m2, adjoint, herm=adjoint, what=f"{n} x {H}x{W} modes ({m1}, {m2}) adjoint={adjoint}")
    with _Pinned("reversed"):            # only the order of the images changes
        spec_r, img_r = _fused(torch.from_numpy(x).to(dev()), m1, m2, adjoint, 0.5, adjoint, adjoint)
    assert ps.check("dft2d_forward_resample") >= 4
    assert torch.equal(spec, spec_r) and torch.equal(img, img_r)


@pytest.mark.parametrize("modes", MODES, ids=["2_3_1", "1_1_2", "1_1_1"])
@pytest.mark.parametrize("adjoint", [False, True], ids=["fwd", "adj"])
def test_every_mode_class_at_the_model_shape(modes, adjoint, monkeypatch):
    """3 x 223 x 223 -> 111 x 111, each instantiation with each operator, flags as the call sites pass them (forward pass: none; backward:
    hermitian_cols and mask_overlap); the launch record names the two-column instantiation"""
    from uno_amd import _native
    m1, m2 = modes
    x = np.random.default_rng(100 * m1 + adjoint).standard_normal((3, 1, 223, 223)).astype(np.float32)
    ps = Poison(monkeypatch, 0xFF)
    _native.profile_begin(64)
    try:
        _check(x, m1, m2, adjoint, herm=adjoint, what=f"3 x 223x223 modes {modes} adjoint={adjoint}")
        torch.cuda.synchronize()
    finally:
        names = [n for n, _, _ in _native.profile_end()]
    assert ps.check("dft2d_forward_resample") >= 2
    cls = {(18, 18): "2, 3, 1", (8, 8): "1, 1, 2", (4, 4): "1, 1, 1"}[modes]
    assert any(f"dft2d_fwd_fd_kernel<{cls}, 2>" in n for n in names), names


@pytest.mark.parametrize("adjoint", [False, True], ids=["fwd", "adj"])
def test_non_zero_rows_only_in_the_last_tile(adjoint, monkeypatch):
    """40 rows = three tiles; only rows 32 .. 39 are non-zero: the carried output rows reach the last tile as exact zeros and the rows the
    first tiles complete are stored as zeros"""
    x = np.zeros((3, 1, 40, WMAX), dtype=np.float32)
    x[:, :, 32:] = np.random.default_rng(31).standard_normal((3, 1, 8, WMAX)).astype(np.float32)
    ps = Poison(monkeypatch, 0xFF)
    spec, img = _check(x, 8, 8, adjoint, herm=adjoint, what=f"rows 32 .. 39 only, adjoint={adjoint}")
    assert ps.check("dft2d_forward_resample") >= 2
    A, _ = _operators(40, WMAX, adjoint)
    dead = (A[:, 32:] == 0).all(1)              # output rows no non-zero input row reaches
    assert bool(dead.any()) and not bool(img[:, :, dead.to(img.device)].any())


@pytest.mark.parametrize("direction", ["forward", "reversed"])
def test_partial_last_workgroup(direction, monkeypatch):
    """four images per workgroup once the images fill the CUs: 4 k + 1 images leave the last workgroup - the FIRST under the reversed
    sweep - with one"""
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    n, H, W = 4 * cus + 1, 17, WMIN
    x = np.random.default_rng(5).standard_normal((n, 1, H, W)).astype(np.float32)
    ps = Poison(monkeypatch, 0xFF)
    with _Pinned(direction):
        _check(x, 4, 4, False, herm=False, what=f"{n} images, {direction}")
    assert ps.check("dft2d_forward_resample") >= 2


def test_reserved_cus(monkeypatch):
    """8 usable CUs: 33 images are eight workgroups of four and one of one; three tiles per image"""
    from uno_amd import _native
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    x = np.random.default_rng(6).standard_normal((33, 1, 40, WMAX)).astype(np.float32)
    ps = Poison(monkeypatch, 0xFF)
    prev = _native.reserve_cus(cus - 8)
    try:
        spec, img = _check(x, 18, 18, True, herm=True, what="33 images on 8 CUs")
    finally:
        _native.reserve_cus(prev)
    spec2, img2 = _fused(torch.from_numpy(x).to(dev()), 18, 18, True, 0.5, True, True)
    assert ps.check("dft2d_forward_resample") >= 4
    assert torch.equal(spec, spec2) and torch.equal(img, img2)          # the geometry changes nothing but the grouping


def test_grouped_spectrum_layout_and_determinism():
    from uno_amd import _native
    from uno_amd.resample import fused_resample_tables
    B, C1, Ct, H, W, m1, m2 = 3, 3, 5, 33, WMAX, 18, 18
    x = torch.randn(B, C1, H, W, device=dev())
    tabs = fused_resample_tables(H, W, H // 2, W // 2, str(x.device), False)
    plain, img = _native.dft2d_forward_resample(x, m1, m2, H // 2, W // 2, tabs, 0.25)
    out = torch.zeros(B, Ct, 2 * m1, m2, dtype=torch.complex64, device=dev())
    got, img2 = _native.dft2d_forward_resample(x, m1, m2, H // 2, W // 2, tabs, 0.25, out=out, channel_offset=2)
    assert got is out and torch.equal(out[:, 2:], plain) and not bool(out[:, :2].any())
    assert torch.equal(img, img2)                                       # two launches: bit for bit


def test_red_zone(monkeypatch):
    """sentinels around every output the call allocates (spectrum and image), ragged last tile, partial last column group"""
    rz = RedZone(monkeypatch)
    for H, W, adjoint, n in ((33, WMAX, False, 9), (40, WMIN, True, 3), (17, WMAX, True, 1), (223, WMAX, False, 3)):
        x = torch.randn(n, 1, H, W, device=dev())
        _fused(x, 4, 4, adjoint)
        _fused(x, 8, 8, adjoint, herm=True, mask=True)
        _fused(x, min(18, H), 18, adjoint, herm=True, mask=True)
    rz.check("dft2d_forward_resample")


# ------------------------------------------------------------------------------------------------------------------ the ends of the window
@pytest.mark.parametrize("W", [WMIN - 1, WMAX + 1])
def test_rows_outside_the_window_are_refused(W):
    from uno_amd import _native
    from uno_amd.resample import fused_resample_tables
    for adjoint in (False, True):
        tabs = fused_resample_tables(40, W, 20, W // 2, str(dev()), adjoint)
        assert tabs is not None                 # the tables exist: it is the kernel's window that refuses
        for m1, m2 in MODES:
            assert not _native.dft2d_forward_resample_applies(3, 40, W, m1, m2, 20, W // 2, tabs[1].shape[1])
    for Win in (WMIN, WMAX):
        assert _native.dft2d_forward_resample_applies(3, 40, Win, 8, 8, 20, Win // 2, 9)
        assert not _native.dft2d_forward_resample_applies(3, 40, Win, 8, 8, 20, 129, 9)       # more output columns than two per lane hold
        assert not _native.dft2d_forward_resample_applies(3, 40, Win, 8, 8, 20, Win // 2, 10)  # a wider band than the compiled taps


def _block_run(blk, x, gy):
    y = blk(x)
    return [y.detach()] + [g.detach() for g in torch.autograd.grad(y, [x] + list(blk.parameters()), gy)]


@pytest.mark.parametrize("kind,W", [("down", WMIN - 1), ("down", WMAX + 1), ("up", WMIN - 1), ("up", WMAX + 1), ("down", WMAX), ("up", WMAX)],
                         ids=["down191", "down224", "up191", "up224", "down223", "up223"])
def test_operator_block_outside_and_inside_the_window(kind, W, monkeypatch):
    """down: 40 x W -> 20 x W // 2 (the fused call would sit in the forward pass); up: the reverse (in the backward pass).  Outside the
    window the block runs the K7 + K1 pair, inside it the fused kernel; both match the oracle block at the bound of
    tests/test_hip_fwd_resample.py's block test"""
    from uno_amd import _native
    from uno_amd.integral_operators import OperatorBlock_2D
    torch.manual_seed(13)
    hw, out_hw = ((40, W), (20, W // 2)) if kind == "down" else ((20, W // 2), (40, W))
    ref = so.OracleOperatorBlock2d(2, 3, out_hw[0], out_hw[1], 4, 4)
    blk = OperatorBlock_2D(2, 3, out_hw[0], out_hw[1], 4, 4)
    blk.load_state_dict(ref.state_dict(), strict=True)
    blk = blk.to(dev())
    x_cpu = torch.randn(1, 2, *hw, requires_grad=True)
    x = x_cpu.detach().to(dev()).requires_grad_(True)
    y_ref = ref(x_cpu)
    gy = torch.randn_like(y_ref)
    want = [y_ref.detach()] + [g for g in torch.autograd.grad(y_ref, [x_cpu] + list(ref.parameters()), gy)]
    ps = Poison(monkeypatch, 0xFF)
    _native.profile_begin(256)
    try:
        got = _block_run(blk, x, gy.to(dev()))
        torch.cuda.synchronize()
    finally:
        names = [n for n, _, _ in _native.profile_end()]
    assert ps.check("OperatorBlock_2D") >= 4
    inside = WMIN <= W <= WMAX
    assert any("dft2d_fwd_fd_kernel" in n for n in names) == inside, names
    if not inside:
        assert any("resample" in n for n in names), names          # K7 ran
    gmax = max(float(torch.linalg.vector_norm(w)) for w in want[1:])
    for i, (a, w) in enumerate(zip(got, want)):
        n = float(torch.linalg.vector_norm(w))
        e = float(torch.linalg.vector_norm(a.cpu() - w))
        print(f"[fwd_resample_223 block {kind} W={W}] tensor {i}: vs oracle {e / max(n, 1e-30):.2e}")
        assert e <= TOL * n + (0.0 if i == 0 else 1e-6 * gmax)
