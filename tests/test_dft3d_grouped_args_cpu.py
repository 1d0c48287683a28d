"""The stage-level 3-D transforms (uno_dft3d_forward_grouped / _inverse_grouped / uno_dft3d_ws_bytes) and the two-source 3-D layer
(uno_spectral_conv3d_forward2 / _backward2): what they check on the host.  Every refused call returns a negative code and a message that
names the argument, before any launch - no device is needed (the pointers are host bytes no call gets to read).
pytest -m "not gpu" """
import ctypes
import re

from dft2d_instances import LIBRARY, dynamic_symbols
from uno_amd import _native

NEW = ("uno_dft3d_ws_bytes", "uno_dft3d_forward_grouped", "uno_dft3d_inverse_grouped", "uno_spectral_conv3d_forward2",
       "uno_spectral_conv3d_backward2")
GRID, MODES = (12, 10, 6), (5, 4, 3)


def _pointers():
    buf = ctypes.create_string_buffer(64)
    arr = (ctypes.c_void_p * 4)(*([ctypes.addressof(buf)] * 4))
    return buf, ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0), arr


def _refused(rc, lib, *names):
    msg = lib.uno_last_error().decode()
    assert rc < 0, (rc, msg)
    for n in names:
        assert re.search(r"\b" + re.escape(n) + r"\b", msg), (n, msg)


def test_the_five_symbols_are_exported():
    _native.lib()
    exported = set(dynamic_symbols(LIBRARY))
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    assert set(NEW) <= set(_native._SIGNATURES)


def test_ws_bytes_is_the_plane_paths_workspace():
    lib = _native.lib()
    for n_vol, D1, m2, m3 in ((48, 12, 4, 3), (6, 9, 4, 3), (2, 44, 2, 2), (1 << 20, 64, 32, 8)):
        assert lib.uno_dft3d_ws_bytes(n_vol, D1, m2, m3) == 8 * n_vol * D1 * 2 * m2 * m3
    assert lib.uno_dft3d_ws_bytes(0, 12, 4, 3) == 0


def test_stage_calls_validate_on_the_host():
    lib = _native.lib()
    buf, p, nul, _ = _pointers()
    for fn, first, second in ((lib.uno_dft3d_forward_grouped, "x", "spec"), (lib.uno_dft3d_inverse_grouped, "spec", "y")):
        def call(a=p, b=p, ws=p, n_vol=8, grid=GRID, modes=MODES, group=0, stride=0, offset=0):
            return fn(a, b, ws, n_vol, *grid, *modes, 1.0, 0, group, stride, offset, None)

        _refused(call(a=nul), lib, "null", first)
        _refused(call(b=nul), lib, "null", second)
        _refused(call(ws=nul), lib, "null", "ws")
        _refused(call(modes=(5, 4, 5)), lib, "modes3")                      # 5 > 6 // 2 + 1
        _refused(call(modes=(13, 4, 3)), lib, "modes1")
        _refused(call(n_vol=-1), lib, "n_vol")
        _refused(call(group=0, stride=8), lib, "group")                     # grouped arguments without a group
        _refused(call(group=0, offset=1), lib, "group")
        _refused(call(group=4, stride=8, offset=-1), lib, "offset")
        _refused(call(group=4, stride=8, offset=5), lib, "stride", "offset", "group")       # offset + group > stride
        _refused(call(group=4, stride=3), lib, "stride")
        _refused(call(n_vol=9, group=4, stride=8), lib, "n_vol", "group")   # n_vol % group != 0
        # nothing to do: success without touching the device, whatever the pointers
        assert call(a=nul, b=nul, ws=nul, n_vol=0) == 0
        assert call(a=nul, b=nul, ws=nul, n_vol=0, group=4, stride=8, offset=4) == 0
        _refused(call(n_vol=0, group=4, stride=8, offset=5), lib, "stride")         # ... but not whatever the grouping


def test_two_source_layer_calls_validate_on_the_host():
    lib = _native.lib()
    buf, p, nul, arr = _pointers()
    Ci, Co = 6, 4

    def fwd(x1=p, x2=p, C1=2, w=arr, y=p, xt=p, ws=p, B=2, grid=GRID, out=GRID, modes=MODES):
        return lib.uno_spectral_conv3d_forward2(x1, x2, C1, w, y, xt, ws, B, Ci, Co, *grid, *out, *modes, None)

    def bwd(gy=p, xt=p, w=arr, gx1=p, gx2=ctypes.c_void_p(ctypes.addressof(buf) + 32), C1=2, gw=arr, ws=p, B=2, grid=GRID, out=GRID, modes=MODES):
        return lib.uno_spectral_conv3d_backward2(gy, xt, w, gx1, gx2, C1, gw, ws, B, Ci, Co, *grid, *out, *modes, None)

    for call in (fwd, bwd):
        _refused(call(C1=0), lib, "C1")
        _refused(call(C1=Ci), lib, "C1")
        _refused(call(C1=-1), lib, "C1")
        _refused(call(modes=(5, 4, 5)), lib, "modes3")
        _refused(call(ws=nul), lib, "null")
    assert fwd(B=0) == 0 and bwd(B=0, gw=None) == 0                       # an empty batch: nothing to do
    _refused(fwd(x1=nul), lib, "null")
    _refused(fwd(y=nul), lib, "null")
    _refused(bwd(gy=nul), lib, "null")
    _refused(bwd(gx1=nul), lib, "gx1")
    _refused(bwd(gx1=p, gx2=p), lib, "gx1", "gx2", "alias")
    # one source (x2 / gx2 NULL) is the one-source call: its own checks answer, C1 is not looked at
    _refused(fwd(x2=nul, C1=0, modes=(5, 4, 5)), lib, "modes3")
    assert fwd(x2=nul, C1=0, B=0) == 0
    assert bwd(gx2=nul, C1=0, B=0, gw=None) == 0
