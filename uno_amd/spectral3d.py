"""3-D spectral convolution on the HIP path (SpectralConv3d_Uno.forward, reference
integral_operators.py:385-427): rfftn over (H, W, T) restricted to the four low-frequency corners ->
per-mode channel mixing with weights1..4 -> zero-padded irfftn, with a custom autograd adjoint that
saves only the truncated input spectrum.  Also pointwise_op_3D's FFT resampling on the pruned-DFT, the any-grid and the wide-axis kernels
(plans + Functions) and the 3-D operator block in one buffer, on one tensor or on the two sources of a skip connection."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _native
from .pointwise import _mix2_forward, _mix2_input_grads, _plain, _wgrad_into


def _dense(t):         # (torch's strided copy for every layout; the one-buffer block below goes through pointwise._plain)
    if t.is_complex() and t.is_conj():
        t = t.resolve_conj()
    if t.is_neg():
        t = t.resolve_neg()
    return t.contiguous()


class _SpectralConv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, w2, w3, w4, d1, d2, d3):
        x = _dense(x)
        ws = [_dense(w) for w in (w1, w2, w3, w4)]
        y, xt = _native.spectral_conv3d_forward(x, ws, int(d1), int(d2), int(d3))
        ctx.save_for_backward(xt, *ws)
        ctx.in_dims = tuple(x.shape[-3:])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xt, *ws = ctx.saved_tensors
        need_gx = ctx.needs_input_grad[0]
        need_gw = any(ctx.needs_input_grad[1:5])
        gx, gws = _native.spectral_conv3d_backward(_dense(gy), xt, ws, *ctx.in_dims, need_gx=need_gx, need_gw=need_gw)
        gws = gws or [None] * 4
        return (gx, *gws, None, None, None)


def spectral_conv3d(x, weights, dim1, dim2, dim3):
    return _SpectralConv3dFn.apply(x, *weights, dim1, dim2, dim3)


def _kept_indices(n_in: int, n_out: int):
    """Spectrum indices along a complex axis that survive the reference's corner copies into an input-sized zero spectrum
    (`ft_u[:h] = ft[:h]`, `ft_u[-h:] = ft[-h:]`, h = n_out // 2 - with Python's `-0:` meaning everything) and irfftn's trimming
    to n_out entries (integral_operators.py:450-463)."""
    h = n_out // 2
    idx = set(range(0, min(h, n_in)))
    idx |= set(range(n_in)) if h == 0 else set(range(max(n_in - h, 0), n_in))
    return sorted(r for r in idx if r < min(n_in, n_out))


RESAMPLE3D_ANY_MAX_AXIS = 128       # the any-grid kernels keep whole (W, T) planes in LDS: every axis length in 2 ... 128


def _modes3(din, dout):
    return min(dout[2] // 2, din[2] // 2 + 1)


def _resample3d_pruned_applies(din, dout) -> bool:
    """True inside the pruned-DFT kernels' range: an even number of kept rows per complex axis (at most 80 / 48), at most 16 bins,
    (W, T) planes of 16 ... 1792 elements with T <= 64."""
    k1, k2 = _kept_indices(din[0], dout[0]), _kept_indices(din[1], dout[1])
    return (len(k1) >= 2 and len(k1) % 2 == 0 and len(k1) <= 80 and len(k2) >= 2 and len(k2) % 2 == 0 and len(k2) <= 48
            and 1 <= _modes3(din, dout) <= 16 and 16 <= din[1] * din[2] <= 1792 and 16 <= dout[1] * dout[2] <= 1792
            and din[2] <= 64 and dout[2] <= 64)


def resample3d_any_applies(din, dout) -> bool:
    """True when the any-grid kernels (uno_fft_resample3d_any) take the FFT crop / resample din -> dout: every axis length in 2 ... 128
    (then every kept-row count is in 1 ... 128 and 1 <= modes3 <= n/2 + 1).  A host predicate: no device, no library call."""
    din, dout = tuple(int(v) for v in din), tuple(int(v) for v in dout)
    if len(din) != 3 or len(dout) != 3 or not all(2 <= v <= RESAMPLE3D_ANY_MAX_AXIS for v in (*din, *dout)):
        return False
    k1, k2 = _kept_indices(din[0], dout[0]), _kept_indices(din[1], dout[1])
    return len(k1) >= 1 and len(k2) >= 1 and 1 <= _modes3(din, dout) <= din[2] // 2 + 1


RESAMPLE3D_WIDE_MAX_AXIS = 256      # the wide-axis kernels: the two leading (complex) axes in 2 ... 256 ...
RESAMPLE3D_WIDE_MAX_LAST = 64       # ... and the last (real) axis in 2 ... 64


def resample3d_wide_applies(din, dout) -> bool:
    """True when the wide-axis kernels (uno_fft_resample3d_wide) take the FFT crop / resample din -> dout: leading axes of 2 ... 256 and a
    last axis of 2 ... 64 (then every kept-row count is in 1 ... 256 and modes3 <= 32, which keeps the kernels' LDS need inside a CU's:
    the entry point's own refusal needs the 33 bins only a hand-made call can ask for).  A host predicate: no device, no library call."""
    din, dout = tuple(int(v) for v in din), tuple(int(v) for v in dout)
    if len(din) != 3 or len(dout) != 3 or not all(2 <= v <= RESAMPLE3D_WIDE_MAX_AXIS for v in (*din[:2], *dout[:2])) \
            or not all(2 <= v <= RESAMPLE3D_WIDE_MAX_LAST for v in (din[2], dout[2])):
        return False
    k1, k2 = _kept_indices(din[0], dout[0]), _kept_indices(din[1], dout[1])
    return len(k1) >= 1 and len(k2) >= 1 and 1 <= _modes3(din, dout) <= din[2] // 2 + 1


_RESAMPLE3D_PLANS = {}
_FAMILY_APPLIES = {"pruned": _resample3d_pruned_applies, "any": resample3d_any_applies, "wide": resample3d_wide_applies}


def _cached_plan(family: str, din, dout, device):
    """(f1, f2, m3) of the kernel family ("pruned" | "any" | "wide") for din -> dout, or None outside its range (no device is touched
    then); the tables are cached per (family, grids, device)."""
    key = (family, tuple(din), tuple(dout), str(device))
    if key not in _RESAMPLE3D_PLANS:
        plan = None
        if _FAMILY_APPLIES[family](din, dout):
            t1 = _native.table_to_device(torch.tensor(_kept_indices(din[0], dout[0]), dtype=torch.int32), device)
            t2 = _native.table_to_device(torch.tensor(_kept_indices(din[1], dout[1]), dtype=torch.int32), device)
            plan = (t1, t2, _modes3(din, dout))
        _RESAMPLE3D_PLANS[key] = plan
    return _RESAMPLE3D_PLANS[key]


def _resample3d_plan(din, dout, device):
    """(f1, f2, m3) for _native.fft_resample3d, or None when the shape is outside the kernels' range (odd row counts, too many
    rows or bins, planes too large): the caller then takes the any-grid kernels (_resample3d_plan_any) where it is opted in."""
    return _cached_plan("pruned", din, dout, device)


def _resample3d_plan_any(din, dout, device):
    """(f1, f2, m3) for _native.fft_resample3d_any, or None when resample3d_any_applies says no."""
    return _cached_plan("any", din, dout, device)


def _resample3d_plan_wide(din, dout, device):
    """(f1, f2, m3) for _native.fft_resample3d_wide, or None when resample3d_wide_applies says no."""
    return _cached_plan("wide", din, dout, device)


class _FftResample3dFn(torch.autograd.Function):
    """irfftn(corner-copy(rfftn(x)), s=size) of pointwise_op_3D on the pruned-DFT kernels (K1p, K5, K6, K3p with explicit
    frequency tables); backward is the transpose: the same kernels with sizes swapped and the Hermitian weights on the other side."""
    resample = staticmethod(_native.fft_resample3d)

    @staticmethod
    def forward(ctx, x, size, plan):
        t1, t2, m3 = plan
        ctx.plan, ctx.din, ctx.dout = plan, tuple(x.shape[-3:]), tuple(size)
        scale = 1.0 / (size[0] * size[1] * size[2])
        return ctx._forward_cls.resample(_plain(x), size, (t1, t1), (t2, t2), m3, scale, adjoint=False)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        t1, t2, m3 = ctx.plan
        scale = 1.0 / (ctx.dout[0] * ctx.dout[1] * ctx.dout[2])
        return ctx._forward_cls.resample(_plain(gy), ctx.din, (t1, t1), (t2, t2), m3, scale, adjoint=True), None, None


class _FftResample3dAnyFn(_FftResample3dFn):
    """_FftResample3dFn on the any-grid kernels (K1a, K5a, K3a: any kept-row counts, axes of 2 ... 128); backward is the adjoint call."""
    resample = staticmethod(_native.fft_resample3d_any)


class _FftResample3dWideFn(_FftResample3dFn):
    """_FftResample3dFn on the wide-axis kernels (K1w, K5w, K3w: leading axes of 2 ... 256, long-axis sums on the MFMA)."""
    resample = staticmethod(_native.fft_resample3d_wide)


# kernel family -> (autograd Function of the resample alone, library call); _OperatorBlock3dFn takes the family's name
RESAMPLE3D_FAMILIES = {
    "pruned": (_FftResample3dFn, _native.fft_resample3d),
    "any": (_FftResample3dAnyFn, _native.fft_resample3d_any),
    "wide": (_FftResample3dWideFn, _native.fft_resample3d_wide),
}


class _OperatorBlock3dFn(torch.autograd.Function):
    """s = SpectralConv3d_Uno(x) + pointwise_op_3D(x) in ONE buffer (reference integral_operators.py:506-512: `x1_out = self.conv(...);
    x2_out = self.w(...); x_out = x1_out + x2_out`, then F.gelu for blocks without normalisation).

    The spectral branch's inverse transform writes s; the point-wise branch - 1x1x1 convolution (K8), then the reference's FFT crop /
    resample on the pruned-DFT kernels - ends in a plane-batched inverse transform that ACCUMULATES into s and, for a block whose sum is
    followed directly by the GELU, writes the activation in the same pass (uno_fft_resample3d_acc; `family` "any" / "wide" with a plan of
    _resample3d_plan_any / _resample3d_plan_wide: uno_fft_resample3d_any_acc / uno_fft_resample3d_wide_acc).  Backward: the spectral branch
    writes grad_x, the transposed 1x1x1 convolution accumulates into it.  The element-wise sum (three passes over the output), the
    GELU (two) and autograd's sum of the two input gradients (three over the input) are gone."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, w4, cw, cb, dims, plan, fuse_gelu, family):
        ctx.leaves = (cw, cb)
        resample = RESAMPLE3D_FAMILIES[family][1]
        x = _plain(x)
        ws = [_plain(w) for w in (w1, w2, w3, w4)]
        B, Ci = x.shape[0], x.shape[1]
        din = tuple(x.shape[2:])
        Co = cw.shape[0]
        cwm = _plain(cw).reshape(Co, Ci)
        cbp = None if cb is None else _plain(cb)
        s, xt = _native.spectral_conv3d_forward(x, ws, *dims)
        t = _native.channel_mix(x.view(B, Ci, -1), cwm, cbp).view(B, Co, *din)
        t1, t2, m3 = plan
        scale = 1.0 / (dims[0] * dims[1] * dims[2])
        if fuse_gelu:
            s, out = resample(t, dims, (t1, t1), (t2, t2), m3, scale, adjoint=False, out=s, act=True)
        else:
            out = resample(t, dims, (t1, t1), (t2, t2), m3, scale, adjoint=False, out=s)
        ctx.save_for_backward(xt, *ws, cwm, x, s if fuse_gelu else None)
        ctx.geom = (din, tuple(dims), plan, cb is not None, tuple(cw.shape), resample)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xt, w1, w2, w3, w4, cwm, x, pre = ctx.saved_tensors
        din, dims, plan, has_bias, cw_shape, resample = ctx.geom
        g = _plain(g)
        if pre is not None:
            g = torch.ops.aten.gelu_backward(g, pre)
        B, Co = g.shape[0], g.shape[1]
        Ci = cwm.shape[1]
        need_gx = ctx.needs_input_grad[0]
        need_gw = any(ctx.needs_input_grad[1:5])
        need_gc = ctx.needs_input_grad[5] or (has_bias and ctx.needs_input_grad[6])
        gx, gws = _native.spectral_conv3d_backward(g, xt, [w1, w2, w3, w4], *din, need_gx=need_gx, need_gw=need_gw)
        gws = gws or [None] * 4
        gcw = gcb = None
        if need_gx or need_gc:
            t1, t2, m3 = plan
            scale = 1.0 / (dims[0] * dims[1] * dims[2])
            g_t = resample(g, din, (t1, t1), (t2, t2), m3, scale, adjoint=True).view(B, Co, -1)
            if need_gx:
                _native.channel_mix(g_t, cwm, None, transpose_w=True, out=gx.view(B, Ci, -1))        # accumulates into the spectral branch's gx
            if need_gc:
                gcw, gcb = _wgrad_into(ctx.leaves, g_t, x.view(B, Ci, -1), None, ctx.needs_input_grad[5], has_bias and ctx.needs_input_grad[6])
                gcw = None if gcw is None else gcw.view(cw_shape)
        return (gx, *gws, gcw, gcb, None, None, None, None)


class _OperatorBlock3dCatFn(torch.autograd.Function):
    """_OperatorBlock3dFn on torch.cat([x1, x2], dim=1), never built (the inner skip connections of the NS-3D models, reference
    navier_stokes_uno3d.py `torch.cat([x_c, skip], dim=1)` ahead of an OperatorBlock_3D).

    Spectral branch: each source is transformed into its channel range of the one truncated spectrum, and its gradient out of its range of
    the gradient spectrum (uno_spectral_conv3d_forward2 / _backward2).  1x1x1 convolution: the two-source channel-mix calls of
    pointwise.py (one launch where the sources split at a multiple of 16 / 64 channels, two accumulating one-source launches
    otherwise).  The resample and the accumulate / GELU epilogue are the one-source Function's.  Both sources are saved as they are."""

    @staticmethod
    def forward(ctx, x1, x2, w1, w2, w3, w4, cw, cb, dims, plan, fuse_gelu, family):
        ctx.leaves = (cw, cb)
        resample = RESAMPLE3D_FAMILIES[family][1]
        x1, x2 = _plain(x1), _plain(x2)
        ws = [_plain(w) for w in (w1, w2, w3, w4)]
        B, C1, C2 = x1.shape[0], x1.shape[1], x2.shape[1]
        din = tuple(x1.shape[2:])
        Co = cw.shape[0]
        cwm = _plain(cw).reshape(Co, C1 + C2)
        cbp = None if cb is None else _plain(cb)
        s, xt = _native.spectral_conv3d_forward2(x1, x2, ws, *dims)
        t = _mix2_forward(x1.view(B, C1, -1), x2.view(B, C2, -1), cwm, cbp).view(B, Co, *din)
        t1, t2, m3 = plan
        scale = 1.0 / (dims[0] * dims[1] * dims[2])
        if fuse_gelu:
            s, out = resample(t, dims, (t1, t1), (t2, t2), m3, scale, adjoint=False, out=s, act=True)
        else:
            out = resample(t, dims, (t1, t1), (t2, t2), m3, scale, adjoint=False, out=s)
        ctx.save_for_backward(xt, *ws, cwm, x1, x2, s if fuse_gelu else None)
        ctx.geom = (din, tuple(dims), plan, cb is not None, tuple(cw.shape), resample)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xt, w1, w2, w3, w4, cwm, x1, x2, pre = ctx.saved_tensors
        din, dims, plan, has_bias, cw_shape, resample = ctx.geom
        g = _plain(g)
        if pre is not None:
            g = torch.ops.aten.gelu_backward(g, pre)
        B, Co = g.shape[0], g.shape[1]
        C1, C2 = x1.shape[1], x2.shape[1]
        need_gx = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        need_gw = any(ctx.needs_input_grad[2:6])
        need_gc = ctx.needs_input_grad[6] or (has_bias and ctx.needs_input_grad[7])
        gx1, gx2, gws = _native.spectral_conv3d_backward2(g, xt, [w1, w2, w3, w4], C1, *din, need_gx=need_gx, need_gw=need_gw)
        gws = gws or [None] * 4
        gcw = gcb = None
        if need_gx or need_gc:
            t1, t2, m3 = plan
            scale = 1.0 / (dims[0] * dims[1] * dims[2])
            g_t = resample(g, din, (t1, t1), (t2, t2), m3, scale, adjoint=True).view(B, Co, -1)
            if need_gx:         # accumulates into the spectral branch's gx1 / gx2
                _mix2_input_grads(g_t, cwm, C1, out1=gx1.view(B, C1, -1), out2=gx2.view(B, C2, -1))
            if need_gc:
                gcw, gcb = _wgrad_into(ctx.leaves, g_t, x1.view(B, C1, -1), x2.view(B, C2, -1), ctx.needs_input_grad[6],
                                       has_bias and ctx.needs_input_grad[7])
                gcw = None if gcw is None else gcw.view(cw_shape)
        if not ctx.needs_input_grad[0]:
            gx1 = None
        if not ctx.needs_input_grad[1]:
            gx2 = None
        return (gx1, gx2, *gws, gcw, gcb, None, None, None, None)
