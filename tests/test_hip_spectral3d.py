"""Parity of the 3-D HIP spectral convolution (C ABI) vs golden vectors and the dense oracle.  pytest -m gpu
Tolerance: relative L2 <= 2e-5 (float32 path, measured ~3e-7)."""
import numpy as np
import pytest
import torch

from conftest import Case, load_cases, rel_err
from oracle import spectral_oracle as so

Z3, NAMES3 = load_cases("spectral3d.npz")
ZB, NAMESB = load_cases("blocks.npz")
TOL = 2e-5


def test_later_wins_mask_is_separable():
    """CPU: the 3-D later-wins mask of the ordered corner writes (integral_operators.py:410-421) factorises
    into one 1-D mask per axis - what the kernels apply."""
    for (Ho, Wo, m1, m2) in [(8, 8, 6, 6), (12, 12, 4, 4), (8, 12, 6, 4), (12, 8, 4, 7), (7, 7, 7, 7), (9, 6, 5, 4)]:
        full = so._keep3d(Ho, Wo, m1, m2)
        sep = np.outer(so.later_wins_mask(Ho, m1), so.later_wins_mask(Wo, m2))
        assert np.array_equal(full, sep), (Ho, Wo, m1, m2)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def corner_major(X, m1, m2):
    """(B,C,2m1,2m2,m3) -> (B,C,4,m1,m2,m3) in weights1..4 order."""
    parts = [X[:, :, :m1, :m2], X[:, :, m1:, :m2], X[:, :, :m1, m2:], X[:, :, m1:, m2:]]
    return np.stack(parts, axis=2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES3)
def test_golden_3d_forward_backward(name):
    from uno_amd.spectral3d import spectral_conv3d
    c = Case(Z3, name)
    meta = [int(v) for v in c.meta]
    dout = meta[6:9]
    x = cu(c.x).requires_grad_(True)
    ws = [cu(getattr(c, f"w{k}")).requires_grad_(True) for k in range(1, 5)]
    y = spectral_conv3d(x, ws, *dout)
    assert y.dtype == torch.float32 and tuple(y.shape) == c.y.shape
    assert rel_err(y.detach().cpu().numpy(), c.y) < TOL
    y.backward(cu(c.gy))
    assert rel_err(x.grad.cpu().numpy(), c.gx) < TOL
    for k in range(4):
        ref = getattr(c, f"gw{k + 1}")
        got = ws[k].grad.cpu().numpy()
        assert rel_err(got, ref) < TOL, k
        assert np.all(got[ref == 0] == 0)           # overwritten corner entries get exactly zero gradient


SEEDED3 = [
    # B, Ci, Co, (H,W,T), (Ho,Wo,To), (m1,m2,m3)
    (2, 4, 3, (16, 16, 10), (16, 16, 10), (6, 6, 4)),
    (1, 8, 8, (32, 32, 13), (24, 24, 15), (11, 11, 5)),
    (2, 3, 5, (9, 20, 7), (11, 14, 12), (4, 7, 4)),
    (1, 2, 2, (8, 8, 6), (8, 8, 6), (4, 4, 4)),        # Nyquist bin on T, full rows on H, W
    (1, 4, 4, (64, 64, 20), (64, 64, 20), (16, 16, 8)),    # BASELINE config 4 geometry (few channels)
]


# >= 192 (sample, channel) volumes on both sides: the one-workgroup-per-volume kernels K1v / K3v (csrc/dft3d_volume.hip)
VOLUME3 = [
    (4, 48, 48, (16, 16, 10), (16, 16, 10), (6, 6, 4)),       # 16-byte pieces only
    (6, 32, 32, (12, 20, 20), (12, 20, 20), (4, 7, 8)),       # + the 4-column block of T = 20; all 16 interleaved columns
    (4, 48, 64, (9, 15, 7), (11, 13, 12), (4, 6, 4)),         # odd axis lengths (no N/2 plane / row), resampling
    (2, 96, 96, (8, 40, 6), (8, 40, 6), (3, 18, 3)),          # two kappa tiles and two slot tiles along dim2
    (2, 96, 96, (40, 8, 6), (40, 8, 6), (18, 3, 3)),          # ... along dim1
    (2, 96, 96, (8, 8, 26), (8, 8, 26), (3, 3, 8)),           # two 16-column blocks along T
    (1, 192, 192, (16, 12, 21), (12, 16, 19), (6, 6, 8)),     # two T blocks, the second one narrow on the way in
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SEEDED3 + VOLUME3)
def test_seeded_3d_vs_dense_oracle(cfg):
    from uno_amd import _native
    from uno_amd.spectral3d import spectral_conv3d
    B, Ci, Co, din, dout, modes = cfg
    rng = np.random.default_rng(B + Ci * 7 + sum(din) + sum(modes))
    x = rng.standard_normal((B, Ci, *din)).astype(np.float32)
    sc = (1 / (2 * Ci)) ** 0.5
    ws = [(sc * (rng.standard_normal((Ci, Co, *modes)) + 1j * rng.standard_normal((Ci, Co, *modes)))).astype(np.complex64)
          for _ in range(4)]
    gy = rng.standard_normal((B, Co, *dout)).astype(np.float32)
    y_ref, X = so.spectral_conv3d_dense(x, ws, *dout)
    gx_ref, gws_ref, _, _ = so.spectral_conv3d_dense_bwd(gy, X, ws, *din)
    xd = cu(x).requires_grad_(True)
    wd = [cu(w).requires_grad_(True) for w in ws]
    y = spectral_conv3d(xd, wd, *dout)
    y.backward(cu(gy))
    assert rel_err(y.detach().cpu().numpy(), y_ref) < TOL
    assert rel_err(xd.grad.cpu().numpy(), gx_ref) < TOL
    for k in range(4):
        assert rel_err(wd[k].grad.cpu().numpy(), gws_ref[k]) < TOL, k
    # the saved truncated spectrum is rfftn(x, norm="forward") on the corners, corner-major
    _, xt = _native.spectral_conv3d_forward(cu(x), [cu(w) for w in ws], *dout)
    assert rel_err(xt.cpu().numpy(), corner_major(X, modes[0], modes[1])) < TOL


def _random_volume_cases(n, seed):
    """Seeded random geometries inside the range of the per-volume kernels (>= 48 volumes on both sides (these cases have >= 192), no corner overlap,
    2 m3 <= 16, axis lengths <= 40 / 40 / 32): odd and even lengths, resampling in every axis.  Together with VOLUME3 these reach 7 of the
    9 reachable instantiations of K1v and 15 of the 48 of K3v; test_hip_dft3d_instances.py runs every one of them, entry by entry."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        din = (int(rng.integers(4, 41)), int(rng.integers(4, 41)), int(rng.integers(5, 33)))       # T >= 5: one 16-byte piece per row
        dout = tuple(int(max(lo, min(hi, d + rng.integers(-6, 7)))) for d, lo, hi in zip(din, (4, 4, 5), (40, 40, 32)))
        m1 = int(rng.integers(1, min(din[0], dout[0]) // 2 + 1))
        m2 = int(rng.integers(1, min(din[1], dout[1]) // 2 + 1))
        m3 = int(rng.integers(1, min(8, min(din[2], dout[2]) // 2 + 1) + 1))
        C = int(rng.choice([192, 200, 256]))
        out.append((1, C, C, din, dout, (m1, m2, m3)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", _random_volume_cases(10, 2026), ids=lambda c: "x".join(map(str, c[3])) + "-" + "x".join(map(str, c[4])) + "-m" + "x".join(map(str, c[5])))
def test_volume_kernels_random_geometry(cfg):
    """K1v / K3v (one workgroup per volume) on random geometries against the dense float64 oracle: forward, the saved truncated
    spectrum, the input gradient (weights of few channels would make the einsum the expensive part: Ci = Co >= 192 only to reach
    the kernels' volume count, so the weights are block-diagonal copies of a 4-channel layer)."""
    from uno_amd import _native
    B, Ci, Co, din, dout, modes = cfg
    rng = np.random.default_rng(sum(din) * 131 + sum(dout) * 17 + sum(modes))
    x = rng.standard_normal((B, Ci, *din)).astype(np.float32)
    gy = rng.standard_normal((B, Co, *dout)).astype(np.float32)
    g = 4
    small = [((1 / (2 * g)) ** 0.5 * (rng.standard_normal((g, g, *modes)) + 1j * rng.standard_normal((g, g, *modes)))).astype(np.complex64)
             for _ in range(4)]
    ws = []
    for w in small:                                            # block-diagonal (Ci, Co) weights
        full = np.zeros((Ci, Co, *modes), np.complex64)
        for k in range(Ci // g):
            full[k * g:(k + 1) * g, k * g:(k + 1) * g] = w
        ws.append(full)
    _native.profile_begin(64)
    y, xt = _native.spectral_conv3d_forward(cu(x), [cu(w) for w in ws], *dout)
    gx, gws = _native.spectral_conv3d_backward(cu(gy), xt, [cu(w) for w in ws], *din)
    torch.cuda.synchronize()
    ran = [name for name, _, _ in _native.profile_end()]
    assert sum("dft3d_fwd_volume_kernel" in n for n in ran) == 2 and sum("dft3d_inv_volume_kernel" in n for n in ran) == 2, ran
    y, gx, xt = y.cpu().numpy(), gx.cpu().numpy(), xt.cpu().numpy()
    for k in range(0, Ci // g, max(1, Ci // g // 3)):          # a few channel groups through the dense oracle
        sl = slice(k * g, (k + 1) * g)
        y_ref, X = so.spectral_conv3d_dense(x[:, sl], small, *dout)
        gx_ref, _, _, _ = so.spectral_conv3d_dense_bwd(gy[:, sl], X, small, *din)
        assert rel_err(y[:, sl], y_ref) < TOL, (k, "y")
        assert rel_err(gx[:, sl], gx_ref) < TOL, (k, "gx")
        assert rel_err(xt[:, sl], corner_major(X, modes[0], modes[1])) < TOL, (k, "xt")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in NAMESB if n.startswith("b3d_")])
def test_operator_block_3d_golden(name):
    from uno_amd.integral_operators import OperatorBlock_3D
    c = Case(ZB, name)
    meta = [int(v) for v in c.meta]
    B, Ci, Co = meta[:3]
    dout, modes, nrm, nl = meta[6:9], meta[9:12], meta[12], meta[13]
    blk = OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=bool(nrm), Non_Lin=bool(nl))
    blk.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c.sub("sd").items()}, strict=True)
    blk = blk.to(dev())
    x = cu(c.x).requires_grad_(True)
    y = blk(x)
    assert rel_err(y.detach().cpu().numpy(), c.y) < 1e-4
    y.backward(cu(c.gy))
    assert rel_err(x.grad.cpu().numpy(), c.gx) < 2e-4
    params = dict(blk.named_parameters())
    floor = 1e-5 * float(np.linalg.norm(c.gy))
    for k, g in c.sub("grad").items():
        got = params[k].grad.cpu().numpy()
        assert np.linalg.norm((got - g).ravel()) <= 2e-4 * np.linalg.norm(g.ravel()) + floor, k


@pytest.mark.gpu
def test_module_3d_interface():
    from uno_amd.integral_operators import SpectralConv3d_Uno
    torch.manual_seed(0)
    conv = SpectralConv3d_Uno(2, 3, 8, 8, 6, 3, 3, 2).to(dev())
    x = torch.randn(2, 2, 10, 10, 8, device=dev())
    assert tuple(conv(x).shape) == (2, 3, 8, 8, 6)
    assert tuple(conv(x, 12, 10, 9).shape) == (2, 3, 12, 10, 9)
    assert (conv.dim1, conv.dim2, conv.dim3) == (12, 10, 9)
    with pytest.raises(RuntimeError):
        conv(x.cpu())
    with pytest.raises(RuntimeError):
        conv(x, 2, 10, 9)           # modes1 = 3 > 2 output rows
    with pytest.raises(RuntimeError):
        conv(x, 12, 10, 1)          # modes3 = 2 > 1//2+1


RESAMPLE3D = [  # B, C, (D1, D2, D3) -> (M1, M2, M3): down, up, same, the NS-3D model's own size changes
    (2, 4, (16, 16, 13), (16, 16, 13)), (2, 4, (16, 12, 13), (12, 16, 15)), (1, 8, (8, 8, 15), (16, 16, 23)),
    (1, 8, (16, 16, 23), (12, 12, 26)), (1, 2, (64, 64, 13), (48, 48, 13)), (1, 2, (48, 48, 26), (64, 64, 26)),
    (1, 4, (32, 32, 13), (16, 16, 15)), (2, 16, (6, 6, 4), (4, 4, 7)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", RESAMPLE3D)
def test_fft_resample3d_matches_the_reference_op_sequence(cfg):
    """The FFT crop / resample of pointwise_op_3D (reference integral_operators.py:448-463) on the pruned-DFT kernels vs the
    reference's own op sequence (rfftn, four corner copies into an input-sized zero spectrum, irfftn(s=size)) in float64 on the
    host: forward and input gradient, including the sizes where the reference misplaces the negative frequencies."""
    from uno_amd.spectral3d import _FftResample3dFn, _resample3d_plan
    B, C, din, dout = cfg
    g = torch.Generator().manual_seed(sum(din) * 7 + sum(dout))
    x = torch.randn(B, C, *din, generator=g)
    gy = torch.randn(B, C, *dout, generator=g)

    xr = x.double().requires_grad_(True)
    spec = torch.fft.rfftn(xr, dim=[-3, -2, -1])
    kept = torch.zeros_like(spec)
    h1, h2, h3 = dout[0] // 2, dout[1] // 2, dout[2] // 2
    for rows in (slice(None, h1), slice(-h1, None)):
        for cols in (slice(None, h2), slice(-h2, None)):
            kept[:, :, rows, cols, :h3] = spec[:, :, rows, cols, :h3]
    yr = torch.fft.irfftn(kept, s=dout)
    yr.backward(gy.double())

    plan = _resample3d_plan(din, dout, dev())
    assert plan is not None
    xd = x.to(dev()).requires_grad_(True)
    y = _FftResample3dFn.apply(xd, dout, plan)
    y.backward(gy.to(dev()))
    assert y.shape == yr.shape
    assert rel_err(y.detach().cpu().numpy(), yr.detach().numpy()) < TOL
    assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) < TOL


@pytest.mark.gpu
def test_3d_any_mode_count_vs_dense_oracle():
    """modes beyond the MFMA kernels' range on every axis role: modes1 = 42 (> 40, leading axis: any-mode K5 / K6) and plane modes
    (m2, m3) = (4, 50) (> 48 half-spectrum bins: any-mode plane transforms)."""
    from uno_amd.spectral3d import spectral_conv3d
    for (B, Ci, Co, H, W, T, Ho, Wo, To, m1, m2, m3) in [(1, 1, 2, 44, 8, 6, 44, 8, 6, 42, 4, 3), (1, 2, 1, 6, 10, 100, 6, 10, 100, 3, 4, 50)]:
        g = torch.Generator().manual_seed(H + T)
        x = torch.randn(B, Ci, H, W, T, generator=g)
        ws = [0.2 * torch.randn(Ci, Co, m1, m2, m3, dtype=torch.cfloat, generator=g) for _ in range(4)]
        gy = torch.randn(B, Co, Ho, Wo, To, generator=g)
        xd = x.to(dev()).requires_grad_(True)
        wd = [w.to(dev()).requires_grad_(True) for w in ws]
        y = spectral_conv3d(xd, wd, Ho, Wo, To)
        y.backward(gy.to(dev()))
        y_ref, X = so.spectral_conv3d_dense(x.numpy(), [w.numpy() for w in ws], Ho, Wo, To)
        gx_ref, gws_ref = so.spectral_conv3d_dense_bwd(gy.numpy(), X, [w.numpy() for w in ws], H, W, T)[:2]
        assert rel_err(y.detach().cpu().numpy(), y_ref) < 2e-5
        assert rel_err(xd.grad.cpu().numpy(), gx_ref) < 2e-5
        for got, ref in zip(wd, gws_ref):
            assert rel_err(got.grad.cpu().numpy(), ref) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [((15, 15, 9), (7, 7, 6)), ((8, 64, 40), (8, 48, 30)), ((9, 9, 7), (12, 12, 9))])
def test_pointwise_op_3d_outside_the_pruned_dft_range_matches_the_reference_sequence(cfg):
    """pointwise_op_3D for grids the pruned-DFT resampling kernels do not take (odd kept-row counts, (W, T) planes over 1792 elements):
    `_resample3d_plan` is None: the layer raises, and with STOCK_FFT_RESAMPLE3D = True runs the stock rocFFT sequence with the corner copies as one mask multiplication -
    compared here with the reference's own op sequence (integral_operators.py:439-467) on the host, forward and every gradient
    (these shapes were skipped by the bench-shape test and compared nowhere)."""
    from uno_amd.integral_operators import pointwise_op_3D
    from uno_amd.spectral3d import _resample3d_plan
    din, dout = cfg
    dev = torch.device("cuda:0")
    assert _resample3d_plan(din, dout, dev) is None
    torch.manual_seed(0)
    ref = so.OraclePointwise3d(4, 3, *dout)
    mod = pointwise_op_3D(4, 3, *dout)
    mod.load_state_dict(ref.state_dict(), strict=True)
    mod = mod.to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, *din, generator=g)
    gy = torch.randn(2, 3, *dout, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = ref(xr, *dout)
    yr.backward(gy)
    xd = x.to(dev).requires_grad_(True)
    import uno_amd.integral_operators as io
    with pytest.raises(RuntimeError, match="outside the range of the"):
        mod(xd, *dout)                              # default: no silent dispatch to rocFFT
    io.STOCK_FFT_RESAMPLE3D = True
    try:
        y = mod(xd, *dout)
        y.backward(gy.to(dev))
    finally:
        io.STOCK_FFT_RESAMPLE3D = False
    assert rel_err(y.detach().cpu().numpy(), yr.detach().numpy()) < 2e-5
    assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) < 2e-5
    assert rel_err(mod.conv.weight.grad.cpu().numpy(), ref.conv.weight.grad.numpy()) < 2e-5
    assert rel_err(mod.conv.bias.grad.cpu().numpy(), ref.conv.bias.grad.numpy()) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("normalize,non_lin", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("geom", [((16, 16, 10), (12, 12, 16)), ((32, 32, 13), (16, 16, 15)), ((16, 16, 12), (16, 16, 12)), ((24, 24, 9), (36, 36, 14))])
def test_operator_block_3d_one_buffer_equals_branch_sum(geom, normalize, non_lin):
    """OperatorBlock_3D in one buffer (_OperatorBlock3dFn: the point-wise branch's last transform accumulates into the spectral branch's
    output and writes the GELU; the transposed 1x1x1 convolution accumulates into the spectral branch's input gradient) against the
    same module's two branches run separately and summed by stock ops (reference integral_operators.py:506-512)."""
    import torch.nn.functional as F
    from uno_amd import _native
    from uno_amd.integral_operators import OperatorBlock_3D, instance_norm_gelu
    from uno_amd.spectral3d import _resample3d_plan
    din, dout = geom
    dev = torch.device("cuda:0")
    assert _resample3d_plan(din, dout, dev) is not None
    torch.manual_seed(7)
    blk = OperatorBlock_3D(4, 3, *dout, 4, 4, 3, Normalize=normalize, Non_Lin=non_lin).to(dev)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 4, *din, generator=g).to(dev)
    gy = torch.randn(2, 3, *dout, generator=g).to(dev)
    # separate branches
    xr = x.clone().requires_grad_(True)
    out = blk.conv(xr, *dout) + blk.w(xr, *dout)
    out = instance_norm_gelu(out, blk.normalize_layer, non_lin) if normalize else (F.gelu(out) if non_lin else out)
    out.backward(gy)
    ref = [xr.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
    blk.zero_grad(set_to_none=True)
    # one buffer
    xd = x.clone().requires_grad_(True)
    _native.profile_begin(256)
    y = blk(xd, *dout)
    y.backward(gy)
    names = [r[0] for r in _native.profile_end()]
    assert any("dft2d_inv_plane_kernel<acc>" in n for n in names), names
    got = [xd.grad] + [p.grad for p in blk.parameters()]
    assert rel_err(y.detach().cpu().numpy(), out.detach().cpu().numpy()) < 1e-5
    for a, b in zip(got, ref):
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
        assert float((a - b).norm()) <= 1e-5 * float(b.norm()) + 1e-7, (a.shape,)
