"""Host-side checks of the any-grid FFT resample (uno_fft_resample3d_any) and of the harness Uno3D_T40: which grids the two predicates
take, argument validation of the entry point before anything touches a device, and the reference's state_dict layout.  No GPU."""
import ctypes

import pytest
import torch

from oracle import spectral_oracle as so

# (din, dout) of the two Uno3D_T40 layers outside the pruned-DFT kernels' range at S = 64, T_in = 10 (conv7, conv8), per padding
T40_OUT_OF_RANGE = {
    3: [((32, 32, 31), (48, 48, 41)), ((48, 48, 41), (64, 64, 52))],
    2: [((32, 32, 28), (48, 48, 38)), ((48, 48, 38), (64, 64, 48))],
}
PINNED_REFUSED = [((15, 15, 9), (7, 7, 6)), ((8, 64, 40), (8, 48, 30)), ((9, 9, 7), (12, 12, 9)), ((12, 10, 8), (8, 6, 6))]

# state_dict keys of the reference's Uno3D_T40 (navier_stokes_uno3d.py:54-103), in registration order
_BLOCKS = ["conv0", "conv1", "conv2", "conv3", "conv6", "conv7", "conv8"]
_NORMALIZED = {"conv0", "conv3", "conv7"}
REFERENCE_KEYS = ["fc.weight", "fc.bias", "fc0.weight", "fc0.bias"]
for _b in _BLOCKS:
    REFERENCE_KEYS += [f"{_b}.conv.weights{i}" for i in (1, 2, 3, 4)] + [f"{_b}.w.conv.weight", f"{_b}.w.conv.bias"]
    if _b in _NORMALIZED:
        REFERENCE_KEYS += [f"{_b}.normalize_layer.weight", f"{_b}.normalize_layer.bias"]
REFERENCE_KEYS += ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


def in_range(din, dout):
    """the pruned-DFT plan's own range test (uno_amd/spectral3d.py: _resample3d_plan), evaluated without a device"""
    from uno_amd.spectral3d import _kept_indices
    k1, k2 = _kept_indices(din[0], dout[0]), _kept_indices(din[1], dout[1])
    m3 = min(dout[2] // 2, din[2] // 2 + 1)
    return (len(k1) >= 2 and len(k1) % 2 == 0 and len(k1) <= 80 and len(k2) >= 2 and len(k2) % 2 == 0 and len(k2) <= 48
            and 1 <= m3 <= 16 and 16 <= din[1] * din[2] <= 1792 and 16 <= dout[1] * dout[2] <= 1792 and din[2] <= 64 and dout[2] <= 64)


def test_in_range_helper_is_the_plan_s_rule():
    """the helper above and _resample3d_plan agree (the plan is only built for grids it accepts; a refused grid needs no device)"""
    from uno_amd.spectral3d import _resample3d_plan
    for din, dout in PINNED_REFUSED + T40_OUT_OF_RANGE[3] + T40_OUT_OF_RANGE[2]:
        assert not in_range(din, dout)
        assert _resample3d_plan(din, dout, "cpu") is None


def _traced_grids(cls, pad):
    torch.manual_seed(0)
    model = cls(6, 2, pad=pad, block_cls=so.OracleOperatorBlock3d)
    seen = []
    hooks = [m.register_forward_hook(lambda mod, a, out, n=n: seen.append((n, tuple(a[0].shape[-3:]), tuple(out.shape[-3:]))))
             for n, m in model.named_children() if isinstance(m, so.OracleOperatorBlock3d)]
    with torch.no_grad():
        out = model(torch.randn(1, 64, 64, 10, 1))
    for h in hooks:
        h.remove()
    return seen, out


@pytest.mark.parametrize("pad", [2, 3])
def test_every_layer_of_the_3d_models_has_a_native_path(pad):
    from uno_amd.harness import Uno3D_T20, Uno3D_T40
    from uno_amd.spectral3d import resample3d_any_applies
    for cls, t_out in ((Uno3D_T40, 40), (Uno3D_T20, 20)):
        seen, out = _traced_grids(cls, pad)
        assert tuple(out.shape) == (1, 64, 64, t_out, 1)
        assert [n for n, _, _ in seen] == ["conv0", "conv1", "conv2", "conv3", "conv6", "conv7", "conv8"]
        for name, din, dout in seen:
            assert in_range(din, dout) or resample3d_any_applies(din, dout), (cls.__name__, name, din, dout)
        if cls is Uno3D_T40:
            assert [(din, dout) for n, din, dout in seen if n in ("conv7", "conv8")] == T40_OUT_OF_RANGE[pad]
    for din, dout in T40_OUT_OF_RANGE[pad]:
        assert not in_range(din, dout) and resample3d_any_applies(din, dout)


def test_predicate_range():
    from uno_amd.spectral3d import resample3d_any_applies
    for din, dout in PINNED_REFUSED:
        assert resample3d_any_applies(din, dout)
    assert resample3d_any_applies((128, 128, 64), (96, 96, 64)) and resample3d_any_applies((2, 2, 2), (128, 128, 128))
    assert not resample3d_any_applies((129, 16, 16), (16, 16, 16))
    assert not resample3d_any_applies((16, 16, 16), (16, 129, 16))
    assert not resample3d_any_applies((16, 16, 16), (16, 16, 129))
    assert not resample3d_any_applies((16, 16, 1), (16, 16, 8)) and not resample3d_any_applies((16, 16, 8), (1, 16, 8))


def test_switches_default_off():
    import uno_amd.integral_operators as io
    assert io.NATIVE_RESAMPLE3D_ANY is False and io.STOCK_FFT_RESAMPLE3D is False
    w = io.pointwise_op_3D(2, 2, 8, 8, 8)
    assert not hasattr(w, "native_any_grid")
    blk = io.OperatorBlock_3D(2, 2, 8, 8, 8, 2, 2, 2)
    assert io.enable_native_resample3d_any(blk) is blk and blk.w.native_any_grid is True
    io.enable_native_resample3d_any(blk, False)
    assert blk.w.native_any_grid is False


def test_entry_point_validates_on_the_host():
    from uno_amd import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nul = ctypes.c_void_p(0)

    def call(x, f, n_vol, din, dout, J1, J2, m3):
        return lib.uno_fft_resample3d_any(x, p, p, n_vol, *din, *dout, J1, f, p, J2, p, p, m3, 1.0, 0, 1, None)

    assert call(nul, p, 1, (9, 9, 7), (12, 12, 9), 9, 9, 4) < 0 and b"null" in lib.uno_last_error()
    assert call(p, nul, 1, (9, 9, 7), (12, 12, 9), 9, 9, 4) < 0 and b"null" in lib.uno_last_error()
    assert call(p, p, 1, (129, 9, 7), (12, 12, 9), 9, 9, 4) < 0 and b"2 ... 128" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 7), (12, 12, 1), 9, 9, 1) < 0 and b"2 ... 128" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 7), (12, 12, 9), 0, 9, 4) < 0 and b"1 ... 128" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 7), (12, 12, 9), 9, 129, 4) < 0 and b"1 ... 128" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 7), (12, 12, 9), 9, 9, 5) < 0 and b"n/2+1" in lib.uno_last_error()       # 5 > 7 // 2 + 1
    assert call(p, p, 1, (9, 9, 7), (12, 12, 9), 9, 9, 0) < 0 and b"n/2+1" in lib.uno_last_error()
    assert call(p, p, -1, (9, 9, 7), (12, 12, 9), 9, 9, 4) < 0 and b"volume count" in lib.uno_last_error()
    assert call(nul, nul, 0, (9, 9, 7), (12, 12, 9), 9, 9, 4) == 0                                       # zero volumes: a no-op
    assert lib.uno_fft_resample3d_any_ws_bytes(3, 9, 12, 9, 9, 4) == 8 * 3 * (9 + 12) * 9 * 4


def test_binding_refuses_host_tensors():
    from uno_amd import _native
    t = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        _native.fft_resample3d_any(torch.zeros(1, 4, 4, 4), (4, 4, 4), (t, t), (t, t), 2, 1.0, adjoint=False)


def test_uno3d_t40_loads_the_reference_state_dict_layout():
    from uno_amd.harness import Uno3D_T40
    from uno_amd.integral_operators import pointwise_op_3D
    torch.manual_seed(0)
    model = Uno3D_T40(6, 4, pad=3)
    assert list(model.state_dict().keys()) == REFERENCE_KEYS
    w = 4
    shapes = {"fc.weight": (w // 2, 6), "fc0.weight": (w, w // 2), "conv0.conv.weights1": (w, 2 * w, 20, 20, 4),
              "conv3.conv.weights4": (8 * w, 16 * w, 6, 6, 7), "conv7.conv.weights2": (8 * w, 2 * w, 14, 14, 10),
              "conv8.conv.weights3": (4 * w, 2 * w, 20, 20, 14), "conv8.w.conv.weight": (2 * w, 4 * w, 1, 1, 1),
              "fc1.weight": (4 * w, 3 * w), "fc2.weight": (1, 4 * w)}
    sd = model.state_dict()
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    state = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    assert list(state) == REFERENCE_KEYS
    model.load_state_dict(state, strict=True)
    # built on product blocks the model opts every point-wise layer into the any-grid kernels; on other blocks it sets nothing
    pw = [m for m in model.modules() if isinstance(m, pointwise_op_3D)]
    assert len(pw) == 7 and all(m.native_any_grid is True for m in pw)
    other = Uno3D_T40(6, 2, pad=3, block_cls=so.OracleOperatorBlock3d)
    assert not any(hasattr(m, "native_any_grid") for m in other.modules())
