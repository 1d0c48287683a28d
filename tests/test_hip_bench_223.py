"""K1-FD at the geometries the headline step launches it with on the 223^2 level, the whole launch at bench size against float64 -
the companion of tests/test_hip_bench_shapes.py (K3A_CASES is the pattern) for the two-column instantiations of
csrc/dft2d_fwd_fd_kernel.h.  The names that ran join that module's COVERED set, which its last test holds against the kernels one step
of every bench workload launches (this file sorts - and so runs - before it).  pytest -m gpu

Reference: integral_operators.py:187 (rfft2, norm="forward", truncated) and :240-242 (bicubic / align_corners / antialias resampling)
of a down-sampling block's input, and the adjoints the backward pass of an up-sampling block applies to its output gradient."""
import numpy as np
import pytest
import torch

import test_hip_bench_shapes as shapes
from conftest import rel_err
from oracle import spectral_oracle as so

pytestmark = pytest.mark.gpu
TOL = shapes.TOL

FD_CASES = {    # (images, modes, adjoint operators, hermitian columns + overlap mask, scale, channel group / stride / offset of the spectrum)
    # conv1 forward with the shared transform: c0 (16 x 128 channels) at conv5's modes into channels 128 .. 255 of conv5's spectrum
    "conv1_forward_shared": (16 * 128, 18, False, False, 1.0 / (223 * 223), (128, 256, 128)),
    # ... and with the sharing switch off: conv1's own modes
    "conv1_forward": (16 * 128, 8, False, False, 1.0 / (223 * 223), None),
    # conv4 backward: the gradient at conv4's output, its spectrum (Hermitian weights, later-wins mask) and its adjoint resampling
    "conv4_backward": (16 * 128, 8, True, True, 1.0, None),
}


@pytest.mark.parametrize("case", list(FD_CASES))
def test_c2_darcy_fused_forward_resample_full_size(case):
    from uno_amd import _native
    from uno_amd import resample as rs
    n, m, adjoint, herm, scale, group = FD_CASES[case]
    H, Ho = 223, 111
    d = shapes.dev()
    g = torch.Generator(device=d).manual_seed(n + m + adjoint)
    x = torch.randn(n // 128, 128, H, H, device=d, generator=g)
    tabs = rs.fused_resample_tables(H, H, Ho, Ho, str(d), adjoint)
    assert tabs is not None and _native.dft2d_forward_resample_applies(n, H, H, m, m, Ho, Ho, tabs[1].shape[1])
    out = None if group is None else torch.full((n // 128, group[1], 2 * m, m), complex(float("nan"), float("nan")), dtype=torch.complex64, device=d)
    (spec, img), ran = shapes._run_profiled(lambda: _native.dft2d_forward_resample(x, m, m, Ho, Ho, tabs, scale, herm, herm, out=out,
                                                                                    channel_offset=0 if group is None else group[2]))
    names = {k for k in ran if shapes._spectral(k)}
    assert any("dft2d_fwd_fd_kernel" in k and k.rstrip(">").endswith(", 2") for k in names), ran
    if group is not None:
        assert bool(torch.isnan(torch.view_as_real(spec[:, :group[2]])).all())          # the other source's channels are not touched
        spec = spec[:, group[2]:]
    A = (rs._matrix(Ho, H).t() if adjoint else rs._matrix(H, Ho)).double().numpy()          # (Ho, H), square grids: rows == columns
    idx = sorted(set(np.linspace(0, n - 1, 24).astype(int).tolist()))
    for i in idx:
        b, c = divmod(i, 128)
        xi = x[b, c].cpu().numpy()
        ref_s = so.truncated_rfft2_dense(xi[None, None], m, m)[0, 0] * (H * H) * scale
        if herm:
            ref_s = ref_s * so.hermitian_weights(H, m)[None, :] * so.later_wins_mask(H, m)[:, None]
        assert rel_err(spec[b, c].cpu().numpy(), ref_s) < TOL, (case, i)
        assert rel_err(img[b, c].cpu().double().numpy(), A @ xi.astype(np.float64) @ A.T) < TOL, (case, i)
    shapes.COVERED.update(names)
