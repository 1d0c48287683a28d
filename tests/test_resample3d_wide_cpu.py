"""Host-side checks of the wide-axis FFT resample (uno_fft_resample3d_wide): which grids its predicate takes, which kernel family the
plan chooser picks under each opt-in, argument validation of the entry points before anything touches a device, and the unchanged stock
path of pointwise_op_3D on the CPU.  No GPU."""
import ctypes

import pytest
import torch

from oracle import spectral_oracle as so

# (din, dout) of the layers of Uno3D_T20_256 / Uno3D_T10_256 outside the pruned-DFT range at S = 256, T_in = 10
MODEL_GRIDS = [
    ((256, 256, 12), (64, 64, 12)), ((64, 64, 24), (256, 256, 24)),         # T20_256, pad 2: conv0, conv8
    ((256, 256, 16), (64, 64, 16)), ((16, 16, 28), (64, 64, 32)), ((64, 64, 32), (256, 256, 32)),      # T20_256, pad 3 both sides: conv0, conv7, conv8
    ((64, 64, 12), (256, 256, 12)),                                         # T10_256, pad 2: conv8 (conv0 as T20_256's)
    ((64, 64, 10), (256, 256, 10)),                                         # T10_256, pad 0: conv8
]
# the operator cases of tests/test_hip_resample3d_wide.py
OPERATOR_GRIDS = [
    ((256, 8, 6), (64, 8, 6)), ((8, 256, 6), (8, 64, 6)), ((64, 8, 6), (256, 8, 8)), ((8, 64, 6), (8, 256, 8)),
    ((129, 5, 7), (255, 7, 9)), ((200, 130, 5), (50, 33, 4)), ((6, 255, 64), (5, 131, 63)), ((9, 9, 7), (12, 12, 9)),
    ((32, 32, 31), (48, 48, 41)), ((15, 15, 9), (7, 7, 6)), ((256, 16, 12), (64, 4, 12)), ((64, 16, 12), (256, 64, 12)),
]


def test_predicate_takes_the_models_and_the_operator_grids():
    from uno_amd.spectral3d import resample3d_wide_applies
    for din, dout in MODEL_GRIDS + OPERATOR_GRIDS:
        assert resample3d_wide_applies(din, dout), (din, dout)


def test_predicate_range():
    from uno_amd.spectral3d import resample3d_wide_applies
    base = [(16, 16, 16), (16, 16, 16)]
    for side in (0, 1):
        for axis in (0, 1, 2):
            grids = [list(g) for g in base]
            grids[side][axis] = 257
            assert not resample3d_wide_applies(*grids), grids
    assert not resample3d_wide_applies((16, 16, 65), (16, 16, 16)) and not resample3d_wide_applies((16, 16, 16), (16, 16, 65))
    assert not resample3d_wide_applies((16, 16, 1), (16, 16, 8)) and not resample3d_wide_applies((16, 16, 8), (1, 16, 8))
    assert resample3d_wide_applies((256, 256, 64), (256, 256, 62)) and resample3d_wide_applies((2, 2, 2), (256, 256, 64))
    assert resample3d_wide_applies((16, 256, 64), (16, 256, 64))        # (32 bins: the module never asks for the 33 that the entry point may refuse)


def test_switches_default_off():
    import uno_amd.integral_operators as io
    assert io.NATIVE_RESAMPLE3D_WIDE is False and io.NATIVE_RESAMPLE3D_ANY is False and io.STOCK_FFT_RESAMPLE3D is False
    blk = io.OperatorBlock_3D(2, 2, 8, 8, 8, 2, 2, 2)
    assert not hasattr(blk.w, "native_wide_grid")
    assert io.enable_native_resample3d_wide(blk) is blk and blk.w.native_wide_grid is True and not hasattr(blk.w, "native_any_grid")
    io.enable_native_resample3d_wide(blk, False)
    assert blk.w.native_wide_grid is False


def test_plan_chooser_picks_the_oldest_family_that_applies(monkeypatch):
    """pruned in range; any-grid with only the old opt-in; wide with only the new one; nothing without an opt-in.  The tables go to the
    'device' through _native.table_to_device, replaced here: no device is touched."""
    import uno_amd.integral_operators as io
    from uno_amd import _native
    monkeypatch.setattr(_native, "table_to_device", lambda t, device: t)
    dev = "test-host"
    in_range, any_only, wide_only = ((16, 16, 12), (32, 32, 12)), ((32, 32, 31), (48, 48, 41)), ((256, 256, 12), (64, 64, 12))

    def family(w, grids):
        plan, fam = io._resample3d_kernels(w, *grids, dev)
        assert (plan is None) == (fam is None)
        return fam

    none, old, new, both = (io.pointwise_op_3D(2, 2, 8, 8, 8) for _ in range(4))
    old.native_any_grid = True
    new.native_wide_grid = True
    both.native_any_grid = both.native_wide_grid = True
    assert [family(none, g) for g in (in_range, any_only, wide_only)] == ["pruned", None, None]
    assert [family(old, g) for g in (in_range, any_only, wide_only)] == ["pruned", "any", None]
    assert [family(new, g) for g in (in_range, any_only, wide_only)] == ["pruned", "wide", "wide"]
    assert [family(both, g) for g in (in_range, any_only, wide_only)] == ["pruned", "any", "wide"]       # a grid an older family takes keeps it
    monkeypatch.setattr(io, "NATIVE_RESAMPLE3D_WIDE", True)
    assert [family(none, g) for g in (in_range, any_only, wide_only)] == ["pruned", "wide", "wide"]
    plan, fam = io._resample3d_kernels(none, *wide_only, dev)
    assert fam == "wide" and plan[0].numel() == 32 and plan[1].numel() == 32 and plan[2] == 6
    assert io._resample3d_kernels(none, (300, 300, 12), (64, 64, 12), dev) == (None, None)       # no family takes a 300 x 12 plane


def _lib():
    from uno_amd import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(64)
    return lib, ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0), buf


def test_entry_point_validates_on_the_host():
    lib, p, nul, _keep = _lib()

    def call(x, f, n_vol, din, dout, J1, J2, m3):
        return lib.uno_fft_resample3d_wide(x, p, p, n_vol, *din, *dout, J1, f, p, J2, p, p, m3, 1.0, 0, 1, None)

    ok = ((9, 9, 7), (12, 12, 9))
    assert call(nul, p, 1, *ok, 9, 9, 4) < 0 and b"null" in lib.uno_last_error()
    assert call(p, nul, 1, *ok, 9, 9, 4) < 0 and b"null" in lib.uno_last_error()
    for side in (0, 1):
        for axis in (0, 1):
            grids = [list(g) for g in ok]
            grids[side][axis] = 257
            assert call(p, p, 1, *grids, 9, 9, 4) < 0
            assert b"uno_fft_resample3d_wide:" in lib.uno_last_error() and b"2 ... 256" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 65), (12, 12, 9), 9, 9, 4) < 0 and b"2 ... 64" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 7), (12, 12, 65), 9, 9, 4) < 0 and b"2 ... 64" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 7), (12, 12, 257), 9, 9, 4) < 0 and b"2 ... 64" in lib.uno_last_error()
    assert call(p, p, 1, (9, 9, 7), (12, 12, 1), 9, 9, 1) < 0 and b"2 ... 64" in lib.uno_last_error()
    assert call(p, p, 1, *ok, 0, 9, 4) < 0 and b"1 ... 256" in lib.uno_last_error()
    assert call(p, p, 1, *ok, 9, 0, 4) < 0 and b"1 ... 256" in lib.uno_last_error()
    assert call(p, p, 1, *ok, 257, 9, 4) < 0 and b"1 ... 256" in lib.uno_last_error()
    assert call(p, p, 1, *ok, 9, 257, 4) < 0 and b"1 ... 256" in lib.uno_last_error()
    assert call(p, p, 1, *ok, 9, 9, 5) < 0 and b"n/2+1" in lib.uno_last_error()       # 5 > 7 // 2 + 1
    assert call(p, p, 1, *ok, 9, 9, 0) < 0 and b"n/2+1" in lib.uno_last_error()
    assert call(p, p, -1, *ok, 9, 9, 4) < 0 and b"volume count" in lib.uno_last_error()
    assert call(p, p, 1 << 23, *ok, 9, 9, 4) < 0 and b"volume count" in lib.uno_last_error()      # 2^23 x 256 planes: past a 32-bit count
    # inside every bound, but K3w would keep (256 + 256) rows of 40 complex: refused with the limit named, nothing launched
    assert call(p, p, 1, (16, 256, 64), (16, 256, 64), 16, 256, 33) == -2
    assert b"LDS" in lib.uno_last_error() and b"163840" in lib.uno_last_error()
    assert call(nul, nul, 0, *ok, 9, 9, 4) == 0                                        # zero volumes: a no-op
    assert call(nul, nul, 0, (256, 256, 12), (64, 64, 12), 32, 32, 6) == 0 and call(nul, nul, 0, (64, 64, 32), (256, 256, 32), 64, 64, 16) == 0
    assert call(nul, nul, 0, (256, 256, 64), (256, 256, 64), 256, 256, 32) == 0
    assert lib.uno_fft_resample3d_wide_ws_bytes(3, 256, 64, 32, 32, 6) == 8 * 3 * (256 + 64) * 32 * 6
    assert lib.uno_fft_resample3d_wide_ws_bytes(1 << 20, 256, 256, 256, 256, 33) == 8 * (1 << 20) * 512 * 256 * 33      # 64-bit


def test_acc_entry_point_refuses_aliases_on_the_host():
    lib, p, nul, buf = _lib()
    q = ctypes.c_void_p(ctypes.addressof(buf) + 16)
    r = ctypes.c_void_p(ctypes.addressof(buf) + 32)

    def call(x, y, y_act, n_vol=1, din=(9, 9, 7), dout=(12, 12, 9)):
        return lib.uno_fft_resample3d_wide_acc(x, y, y_act, p, n_vol, *din, *dout, 9, p, p, 9, p, p, 4, 1.0, 0, 1, None)

    assert call(p, q, q) < 0 and b"y_act must not alias y" in lib.uno_last_error()
    assert call(p, p, r) < 0 and b"x must not alias y" in lib.uno_last_error()
    assert call(p, q, p) < 0 and b"x must not alias y_act" in lib.uno_last_error()
    assert b"uno_fft_resample3d_wide_acc" in lib.uno_last_error()
    assert call(nul, q, r) < 0 and b"null" in lib.uno_last_error()
    assert call(p, q, r, din=(257, 9, 7)) < 0 and b"2 ... 256" in lib.uno_last_error()
    assert call(nul, nul, nul, n_vol=0) == 0


def test_the_any_grid_entry_point_keeps_its_range():
    lib, p, nul, _keep = _lib()
    rc = lib.uno_fft_resample3d_any(p, p, p, 1, 256, 9, 7, 12, 12, 9, 9, p, p, 9, p, p, 4, 1.0, 0, 1, None)
    assert rc < 0 and b"2 ... 128" in lib.uno_last_error()
    from uno_amd.spectral3d import RESAMPLE3D_ANY_MAX_AXIS, resample3d_any_applies
    assert RESAMPLE3D_ANY_MAX_AXIS == 128 and not resample3d_any_applies((256, 256, 12), (64, 64, 12))


def test_binding_refuses_host_tensors():
    from uno_amd import _native
    t = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        _native.fft_resample3d_wide(torch.zeros(1, 4, 4, 4), (4, 4, 4), (t, t), (t, t), 2, 1.0, adjoint=False)


def test_pointwise_op_3d_on_the_cpu_is_the_stock_path():
    """CPU tensors take the reference's op sequence whatever the switches say: a long-axis grid equals the oracle"""
    import uno_amd.integral_operators as io
    torch.manual_seed(3)
    ours, ref = io.pointwise_op_3D(3, 2, 64, 8, 6), so.OraclePointwise3d(3, 2, 64, 8, 6)
    io.enable_native_resample3d_wide(ours)
    ref.load_state_dict(ours.state_dict(), strict=True)
    x = torch.randn(2, 3, 256, 8, 6)
    a, b = ours(x), ref(x)
    assert a.shape == (2, 2, 64, 8, 6)
    assert torch.equal(a, b)
