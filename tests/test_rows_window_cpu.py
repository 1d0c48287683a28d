"""The short-row window entry points without a device: argument validation before any launch, the census of the windows the NS-3D models
would pass, and the stock fallbacks of channel_mix_cat(last_window=) / gelu_channel_mix_pad_last and of the models' opt-in."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from oracle import spectral_oracle as so
from uno_amd import _native
from uno_amd.harness import models
from uno_amd.pointwise import channel_mix, channel_mix_cat, gelu_channel_mix, gelu_channel_mix_pad_last


@pytest.fixture(scope="module")
def lib():
    from uno_amd import build
    build.build()
    return _native.lib()


BUF = ctypes.create_string_buffer(64)
P = ctypes.cast(BUF, ctypes.c_void_p)
NUL = ctypes.c_void_p(0)


def _calls(L, B, C1, Ci, Co, rows, cols, pitch, col0, plane, p=P, skip=()):
    """the five entry points (but `skip`) on one geometry -> (name, return code, message).  Every call made here with non-null pointers
    has an argument its entry point refuses: nothing is ever launched on the dummy buffer."""
    out = []
    for name, rc in (
        ("uno_channel_mix2_rows", lambda: L.uno_channel_mix2_rows(p, p, C1, p, p, p, B, Ci, Co, rows, cols, pitch, col0, plane, 0, None)),
        ("uno_channel_mix2_rows_grad", lambda: L.uno_channel_mix2_rows_grad(p, p, C1, NUL, p, p, B, Ci, Co, rows, cols, pitch, col0, plane, None)),
        ("uno_channel_wgrad2_rows", lambda: L.uno_channel_wgrad2_rows(p, p, p, C1, p, p, p, B, Ci, Co, rows, cols, pitch, col0, plane, 0, 0, None)),
        ("uno_channel_mix_act_padded_rows", lambda: L.uno_channel_mix_act_padded_rows(p, p, p, p, p, B, Ci, Co, rows, cols, pitch, col0, 0, None)),
        ("uno_dgelu_rows", lambda: L.uno_dgelu_rows(p, p, p, B * Co, rows, cols, pitch, col0, plane, None)),
    ):
        if name not in skip:
            code = rc()
            out.append((name, code, L.uno_last_error()))
    return out


def test_the_limits_are_refused_with_a_message_that_names_them(lib):
    bad = {
        "col0 + cols > pitch": (25, 9, 10, 2, 250),
        "pitch > 256": (25, 9, 257, 0, 25 * 257),
        "rows * pitch >= 2^24": (65536, 200, 256, 0, 1 << 24),
        "cols < 1": (25, 0, 10, 0, 250),
        "col0 < 0": (25, 9, 10, -1, 250),
    }
    for why, (rows, cols, pitch, col0, plane) in bad.items():
        for name, code, msg in _calls(lib, 1, 2, 3, 4, rows, cols, pitch, col0, plane):
            assert code < 0, (why, name)
            assert name.encode() in msg and b"col0 + cols <= pitch <= 256" in msg and b"rows * pitch < 2^24" in msg, (why, name, msg)
    # a plane that does not hold rows * pitch elements (the padded-activation call has dense planes of exactly that size)
    for name, code, msg in _calls(lib, 1, 2, 3, 4, 25, 9, 10, 1, 249, skip=("uno_channel_mix_act_padded_rows",)):
        assert code < 0 and b"plane >= rows * pitch" in msg, (name, msg)
    # channel counts
    for C1, Ci, Co in ((0, 3, 4), (2, 1025, 4), (2, 3, 0)):
        skip = ("uno_dgelu_rows",) + (("uno_channel_mix_act_padded_rows",) if C1 == 0 else ())       # (no channel counts / no C1)
        for name, code, msg in _calls(lib, 1, C1, Ci, Co, 25, 9, 10, 1, 250, skip=skip):
            assert code < 0 and b"Ci <= 1024" in msg, (name, C1, Ci, Co, msg)
    assert lib.uno_channel_mix2_rows(P, P, 2, P, P, P, -1, 3, 4, 25, 9, 10, 1, 250, 0, None) < 0 and b"bad sizes" in lib.uno_last_error()
    assert lib.uno_dgelu_rows(P, P, P, -1, 25, 9, 10, 1, 250, None) < 0 and b"bad sizes" in lib.uno_last_error()
    assert lib.uno_channel_wgrad2_rows(P, P, P, 2, P, P, P, 1, 3, 4, 25, 9, 10, 1, 250, 0, 2, None) < 0 and b"accumulate" in lib.uno_last_error()


def test_null_pointers_are_refused_and_empty_problems_succeed(lib):
    for name, code, msg in _calls(lib, 1, 2, 3, 4, 25, 9, 10, 1, 250, p=NUL):
        assert code < 0 and b"null" in msg, (name, msg)
    # one missing operand each (the optional ones - bias, x2, g2, gb, y, dgelu_of - may be null)
    L = lib
    assert L.uno_channel_mix2_rows(P, NUL, 3, NUL, NUL, P, 1, 3, 4, 25, 9, 10, 1, 250, 0, None) < 0 and b"null" in L.uno_last_error()
    assert L.uno_channel_mix2_rows_grad(P, P, 2, NUL, NUL, NUL, 1, 3, 4, 25, 9, 10, 1, 250, None) < 0 and b"null" in L.uno_last_error()
    assert L.uno_channel_wgrad2_rows(P, P, P, 2, P, NUL, NUL, 1, 3, 4, 25, 9, 10, 1, 250, 0, 0, None) < 0 and b"null" in L.uno_last_error()
    assert L.uno_channel_mix_act_padded_rows(P, P, NUL, NUL, NUL, 1, 3, 4, 25, 9, 10, 1, 0, None) < 0 and b"null" in L.uno_last_error()
    assert L.uno_dgelu_rows(P, NUL, P, 4, 25, 9, 10, 1, 250, None) < 0 and b"null" in L.uno_last_error()
    # B == 0 or rows == 0: nothing to do, nothing is touched
    for B, rows in ((0, 25), (1, 0), (0, 0)):
        for name, code, msg in _calls(lib, B, 2, 3, 4, rows, 9, 10, 1, rows * 10, p=NUL):
            assert code == 0, (name, B, rows, msg)
    # ... but an empty problem on a geometry outside the range is still refused
    assert L.uno_channel_mix2_rows(NUL, NUL, 2, NUL, NUL, NUL, 0, 3, 4, 25, 9, 300, 1, 7500, 0, None) < 0


def _model_windows(cls, S, T, pad, both, width=2):
    """(head window, lift window, Ci, Co) as Uno3D_T20.forward forms them: (rows, cols, pitch, col0)"""
    padding = int(pad * 0.1 * T)
    d3 = T + (2 if both else 1) * padding
    grids, crop = cls._plan(S, S, d3, padding)
    Tp = grids[-1][2]
    head = (S * S, Tp - 2 * crop, Tp, crop) if both else (S * S, Tp - crop, Tp, 0)
    lift = (S * S, T, d3, padding if both else 0)
    return head, lift, 3 * width, 4 * width


def _accepted(L, win, Ci, Co):
    rows, cols, pitch, col0 = win
    plane = rows * pitch
    ok = _native.rows_window_ok(rows, cols, pitch, col0, plane, Ci, Co)
    # B = 0: the library validates the geometry and returns before it looks at a pointer
    rc = L.uno_channel_mix2_rows(NUL, NUL, Ci - 1, NUL, NUL, NUL, 0, Ci, Co, rows, cols, pitch, col0, plane, 0, None)
    assert ok == (rc == 0), (win, ok, rc, L.uno_last_error())
    return ok


def test_census_every_window_of_the_3d_models_is_inside_the_range(lib):
    seen = 0
    for f in ("model_census.json", "model_census_256.json"):
        census = json.load(open(os.path.join(ROOT, "tests", "golden", f)))
        for key, c in census.items():
            if not c["cls"].startswith("Uno3D") or c["kwargs"].get("pad", 0) == 0:
                continue
            cls = getattr(models, c["cls"])
            _, S, _, T, _ = c["input"]
            head, lift, Ci, Co = _model_windows(cls, S, T, c["kwargs"]["pad"], bool(c["kwargs"].get("pad_both", False)), c["args"][1])
            assert head[1] == c["out"][3] or c["kwargs"].get("pad_both"), (key, head, c["out"])       # the kept length is the output's
            assert 0 < head[1] <= head[2] and _accepted(lib, head, Ci, Co), (key, head)
            assert _accepted(lib, lift, c["args"][0] * 2, c["args"][1]), (key, lift)
            seen += 1
    assert seen >= 20
    # S = 256 with every plan up to Uno3D_T40's (T = 10 -> 40 kept steps of up to 64), at the default widths
    for cls in (models.Uno3D_T20, models.Uno3D_T10, models.Uno3D_T40, models.Uno3D_T20_256, models.Uno3D_T10_256):
        for pad in (1, 2, 3):
            for both in (False, True):
                head, lift, _, _ = _model_windows(cls, 256, 10, pad, both)
                for width in (2, 8, 32):
                    assert _accepted(lib, head, 3 * width, 4 * width), (cls.__name__, pad, both, head)
                    assert _accepted(lib, lift, 12, width), (cls.__name__, pad, both, lift)
    assert not _accepted(lib, (65536, 200, 256, 0), 24, 32)                 # rows * pitch = 2^24
    assert not _accepted(lib, (64, 250, 260, 4), 24, 32)


@pytest.mark.parametrize("col0,cols,Tp", [(0, 10, 13), (3, 10, 16), (0, 12, 12), (1, 9, 10)])
@pytest.mark.parametrize("gelu_first", [False, True])
def test_channel_mix_cat_last_window_on_cpu_is_the_stock_expression(col0, cols, Tp, gelu_first):
    g = torch.Generator().manual_seed(col0 + cols)
    x1 = torch.randn(2, 4, 5, 6, Tp, generator=g, requires_grad=True)
    x2 = torch.randn(2, 2, 5, 6, Tp, generator=g, requires_grad=True)
    fc = torch.nn.Linear(6, 8)
    out = channel_mix_cat([x1, x2], fc.weight, fc.bias, gelu_first=gelu_first, last_window=(col0, cols))
    gy = torch.randn(out.shape, generator=g)
    got = torch.autograd.grad(out, [x1, x2, fc.weight, fc.bias], gy)
    cat = torch.cat([F.gelu(x1) if gelu_first else x1, x2], dim=1)[..., col0:col0 + cols].contiguous()
    ref = channel_mix(cat, fc.weight, fc.bias)
    want = torch.autograd.grad(ref, [x1, x2, fc.weight, fc.bias], gy)
    assert out.shape == (2, 8, 5, 6, cols) and torch.equal(out, ref)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # without a window the call is the one it always was
    assert torch.equal(channel_mix_cat([x1, x2], fc.weight, fc.bias, gelu_first=gelu_first),
                       channel_mix(torch.cat([F.gelu(x1) if gelu_first else x1, x2], 1), fc.weight, fc.bias))


@pytest.mark.parametrize("pl,pr", [(0, 3), (2, 2), (0, 0), (1, 0)])
def test_gelu_channel_mix_pad_last_on_cpu_is_the_stock_expression(pl, pr):
    g = torch.Generator().manual_seed(pl * 7 + pr)
    pre = torch.randn(2, 12, 5, 6, 10, generator=g, requires_grad=True)
    fc0 = torch.nn.Linear(12, 4)
    out = gelu_channel_mix_pad_last(pre, fc0.weight, fc0.bias, pl, pr)
    ref = F.pad(F.gelu(gelu_channel_mix(pre, fc0.weight, fc0.bias)), [pl, pr, 0, 0, 0, 0])
    gy = torch.randn(out.shape, generator=g)
    got = torch.autograd.grad(out, [pre, fc0.weight, fc0.bias], gy)
    want = torch.autograd.grad(ref, [pre, fc0.weight, fc0.bias], gy)
    assert out.shape == (2, 4, 5, 6, 10 + pl + pr) and torch.equal(out, ref)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_other_dtypes_take_the_stock_ops():
    x1, x2 = torch.randn(1, 2, 3, 3, 8, dtype=torch.float64), torch.randn(1, 1, 3, 3, 8, dtype=torch.float64)
    fc = torch.nn.Linear(3, 4).double()
    out = channel_mix_cat([x1, x2], fc.weight, fc.bias, last_window=(1, 6))
    assert out.dtype == torch.float64 and torch.equal(out, channel_mix(torch.cat([x1, x2], 1)[..., 1:7].contiguous(), fc.weight, fc.bias))
    pre = torch.randn(1, 3, 3, 3, 8, dtype=torch.float64)
    assert torch.equal(gelu_channel_mix_pad_last(pre, fc.weight, fc.bias, 1, 2), F.pad(F.gelu(gelu_channel_mix(pre, fc.weight, fc.bias)), [1, 2]))


@pytest.mark.parametrize("cls,T,both", [(models.Uno3D_T10, 10, False), (models.Uno3D_T10, 10, True), (models.Uno3D_T20, 10, False)])
def test_a_model_with_native_ends_on_cpu_or_on_oracle_blocks_is_unchanged(cls, T, both, monkeypatch):
    assert models.NATIVE_ENDS_3D is False and cls.native_ends is False
    torch.manual_seed(3)
    model = cls(6, 2, pad=3, pad_both=both, block_cls=so.OracleOperatorBlock3d)
    x = torch.randn(1, 32, 32, T, 1, generator=torch.Generator().manual_seed(4))

    def run():
        model.zero_grad(set_to_none=True)
        out = model(x)
        out.square().mean().backward()
        return out.detach().clone(), [p.grad.clone() for p in model.parameters()]
    out0, g0 = run()
    assert models.enable_native_ends_3d(model) is model and model.native_ends is True
    assert not model._native_ends(x)                       # host tensors, oracle blocks
    out1, g1 = run()
    monkeypatch.setattr(models, "NATIVE_ENDS_3D", True)
    out2, g2 = run()
    assert torch.equal(out0, out1) and torch.equal(out0, out2)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(g0, g1, g2))
    models.enable_native_ends_3d(model, False)
    assert model.native_ends is False
    # a product-block model on the host does not take the device path either
    prod = cls(6, 2, pad=3, pad_both=both)
    models.enable_native_ends_3d(prod)
    assert prod.native_ends and not prod._native_ends(x)
