"""One forward transform for a tensor with two spectral consumers (block2d.SpectrumShare, csrc/spectrum_crop.hip).  pytest -m gpu

The Darcy model's c0 is transformed by conv1 (modes 8) and, as the second source of its two-source form, by conv5 (modes 18) on the same
223^2 grid; with SHARE_FORWARD_SPECTRUM conv1 transforms it once at modes 18 into conv5's spectrum and copies its own corner blocks out.
  a. the crop kernel against indexing on the host, bit for bit, NaN-filled destinations, plain and grouped layouts;
  b. the cropped sub-spectrum against the float64 rfft2 truncated to the smaller mode counts (tolerance of tests/test_hip_spectral2d.py);
  c. a small UNO_9 forward + loss + backward with the switch on and off: prediction, loss and every parameter gradient per element at
     the 1e-4 relative bound of tests/test_hip_headline_parity.py, and one forward transform fewer in the library's launch records -
     at S = 72 (the smallest grid the fixed mode counts allow) and at S = 421, one sample, width 8, where c0 is 223 wide and the
     half-tile and the resampling transforms (K1-HT, K1-FD) are the ones selected."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5               # tests/test_hip_spectral2d.py, forward transform stage


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _crop_host(src, m1, m2):
    """(..., 2 M1, M2) -> (..., 2 m1, m2): lo rows 0 .. m1 - 1, the last m1 rows of the hi corner, columns 0 .. m2 - 1"""
    M1 = src.shape[-2] // 2
    return torch.cat([src[..., :m1, :m2], src[..., 2 * M1 - m1:, :m2]], dim=-2)


def _nan_filled(shape):
    return torch.full(shape, complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev())


def _bits(t):
    return torch.view_as_real(t.contiguous()).view(torch.int32)


CROPS = [((18, 18), (8, 8)), ((18, 18), (18, 18)), ((5, 7), (1, 1)), ((20, 12), (3, 12))]


# ------------------------------------------------------------------------------------------------ a. the kernel
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("modes", CROPS)
def test_crop_plain_layout_is_bit_equal_to_host_indexing(modes, n):
    from uno_amd import _native
    (M1, M2), (m1, m2) = modes
    g = torch.Generator().manual_seed(100 * M1 + m1 + n)
    src = torch.randn(n, 2 * M1, M2, dtype=torch.complex64, generator=g).to(dev())
    got = _native.spectrum_crop(src, m1, m2)
    assert got.shape == (n, 2 * m1, m2)
    assert torch.equal(_bits(got), _bits(_crop_host(src, m1, m2)))


@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("modes", CROPS)
def test_crop_grouped_layouts_are_bit_equal_and_touch_nothing_else(modes, n):
    """n batch entries of (group 3, stride 5, offset 2) - three channels at channels 2 .. 4 of five - on the source side, the destination
    plain and in the same grouped layout; every destination element outside the group keeps its NaN"""
    from uno_amd import _native
    (M1, M2), (m1, m2) = modes
    G, STRIDE, OFF = 3, 5, 2
    g = torch.Generator().manual_seed(7 * M1 + m2 + n)
    src = torch.randn(n, STRIDE, 2 * M1, M2, dtype=torch.complex64, generator=g).to(dev())
    ref = _crop_host(src[:, OFF:OFF + G], m1, m2)
    plain = _nan_filled((n, G, 2 * m1, m2))
    _native.spectrum_crop(src, m1, m2, out=plain, channels=G, channel_offset=OFF)
    assert torch.equal(_bits(plain), _bits(ref))
    fresh = _native.spectrum_crop(src, m1, m2, channels=G, channel_offset=OFF)
    assert fresh.shape == ref.shape and torch.equal(_bits(fresh), _bits(ref))
    grouped = _nan_filled((n, STRIDE, 2 * m1, m2))
    _native.spectrum_crop(src, m1, m2, out=grouped, channels=G, channel_offset=OFF, out_channel_offset=OFF)
    assert torch.equal(_bits(grouped[:, OFF:OFF + G]), _bits(ref))
    assert bool(torch.isnan(torch.view_as_real(grouped[:, :OFF])).all())


def test_crop_rejects_bad_arguments():
    from uno_amd import _native
    src = torch.zeros(2, 4, 10, 6, dtype=torch.complex64, device=dev())
    with pytest.raises(RuntimeError):
        _native.spectrum_crop(src, 6, 3)                    # more rows than the source holds
    with pytest.raises(RuntimeError):
        _native.spectrum_crop(src, 2, 7)
    with pytest.raises(RuntimeError):
        _native.spectrum_crop(src, 2, 3, channels=3, channel_offset=2)
    with pytest.raises(RuntimeError):
        _native.spectrum_crop(src, 2, 3, out=torch.zeros(2, 2, 4, 3, dtype=torch.complex64, device=dev()), channels=3)
    lib = _native.lib()
    p = _native._ptr(src)
    assert lib.uno_spectrum_crop(p, p, 2, 5, 6, 2, 3, 0, 0, 0, 0, 0, 0, None) < 0 and b"alias" in lib.uno_last_error()
    assert lib.uno_spectrum_crop(None, None, 0, 5, 6, 2, 3, 0, 0, 0, 0, 0, 0, None) == 0


# ------------------------------------------------------------------------------------------------ b. against the float64 rfft2
@pytest.mark.parametrize("hw", [(40, 223), (37, 38)])
def test_cropped_forward_transform_matches_float64_rfft2(hw):
    from uno_amd import _native
    H, W = hw
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(5, 1, H, W, generator=g)
    big = _native.dft2d_forward(x.to(dev()), 18, 18, scale=1.0 / (H * W))
    got = _native.spectrum_crop(big, 8, 8).cpu().numpy()
    X = torch.fft.rfft2(x.double(), norm="forward")
    ref = torch.cat([X[..., :8, :8], X[..., -8:, :8]], dim=-2).numpy()
    assert got.shape == ref.shape
    err = rel_err(got, ref)
    print(f"{H}x{W}: modes (18, 18) cropped to (8, 8) vs float64 rfft2: {err:.3e}")
    assert err < TOL
    # ... and the transform at modes (8, 8) itself sees the same reference
    assert rel_err(_native.dft2d_forward(x.to(dev()), 8, 8, scale=1.0 / (H * W)).cpu().numpy(), ref) < TOL


# ------------------------------------------------------------------------------------------------ c. the model, switch on / off
def _step(S, batch, share):
    from uno_amd import _native, block2d
    from uno_amd.harness import UNO_9, lp_loss_rel_sum, synthetic_darcy_batch
    prev = block2d.SHARE_FORWARD_SPECTRUM
    block2d.SHARE_FORWARD_SPECTRUM = share
    try:
        torch.manual_seed(7)
        model = UNO_9(3, 8, pad=5).to(dev())
        a, u = synthetic_darcy_batch(batch, S, 4321, dev())
        _native.profile_begin(4096)
        try:
            out = model(a)
            loss = lp_loss_rel_sum(out.reshape(batch, -1), u.reshape(batch, -1))
            loss.backward()
            torch.cuda.synchronize()
        finally:
            names = [n for n, _, _ in _native.profile_end()]
    finally:
        block2d.SHARE_FORWARD_SPECTRUM = prev
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return out.detach(), float(loss.detach()), grads, names


def _assert_close(a, b, what):
    """tests/test_hip_headline_parity.py's 1e-4 relative bound, in its own form (L2 norm of the difference against the tensor's) AND per
    element: |a - b| <= 1e-4 of the tensor's largest magnitude (an element near a zero crossing has no relative error of its own in
    float32; the largest element is the scale the rounding of every sum in the tensor is proportional to)"""
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), what
    scale = float(b.abs().max())
    worst = float((a - b).abs().max())
    assert worst <= 1e-4 * scale, (what, worst, scale)
    assert float(torch.linalg.vector_norm(a - b)) <= 1e-4 * float(torch.linalg.vector_norm(b)), what
    return worst / max(scale, 1e-30)


@pytest.mark.parametrize("S,batch", [(72, 2), (421, 1)])
def test_model_step_with_shared_spectrum_equals_step_without(S, batch):
    out0, loss0, g0, names0 = _step(S, batch, False)
    out1, loss1, g1, names1 = _step(S, batch, True)
    worst = _assert_close(out1, out0, "prediction")
    assert abs(loss1 - loss0) <= 1e-4 * abs(loss0)
    for k in g0:
        if k in ("conv1.w.conv.bias", "conv4.w.conv.bias"):
            # the 1x1-convolution biases in front of an InstanceNorm have a true gradient of exactly zero: both sides hold rounding residue,
            # which has no relative error (the headline parity test leaves the same two out of its bound)
            continue
        worst = max(worst, _assert_close(g1[k], g0[k], k))
    print(f"S = {S}: shared vs own transforms, largest element difference relative to the tensor's largest element: {worst:.3e}")
    fwd0 = [n for n in names0 if "dft2d_fwd" in n]
    fwd1 = [n for n in names1 if "dft2d_fwd" in n]
    assert len(fwd1) == len(fwd0) - 1, (fwd0, fwd1)
    assert sum("spectrum_crop" in n for n in names1) == 1 and not any("spectrum_crop" in n for n in names0)
    assert len(names1) == len(names0), (len(names0), len(names1))         # one transform fewer, one crop more, nothing else moved
    if S == 421:
        assert any("dft2d_fwd_ht_kernel" in n for n in fwd1) and any("dft2d_fwd_fd_kernel" in n for n in fwd1), fwd1
