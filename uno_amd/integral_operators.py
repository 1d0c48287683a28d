"""MI355X-native drop-in for the operator blocks of U-NO (module name kept: model code does
``from integral_operators import *`` - reference darcy_flow_uno2d.py:10, navier_stokes_uno2d.py:9,
navier_stokes_uno3d.py:6).

Same classes, constructor / forward signatures, attribute names, parameter names, shapes,
dtypes and registration order as the reference's integral_operators.py, so a reference
``state_dict`` loads with ``strict=True`` and seed-for-seed initialisation matches.  What differs is
what runs underneath the spectral convolutions:

    rFFT -> truncated-mode complex channel mixing -> zero-padded iRFFT

is executed by hand-written gfx950 kernels behind the C ABI in include/uno_spectral.h (pruned
forward DFT, per-mode complex MFMA GEMM, pruned inverse DFT; custom autograd with the same kernel
family).  The full spectrum is never materialised.  There is no CPU fallback for these layers: a
tensor that is not on a HIP device raises ``RuntimeError``.

The rest of an operator block runs on the same library for float32 device tensors: the point-wise branch (1x1
convolution = channel-mix kernels, bicubic anti-aliased resampling = banded separable kernels) accumulates into the
spectral branch's output buffer, InstanceNorm (+ GELU) is one kernel; only the GELU of non-normalised blocks and the
skip concatenations are stock PyTorch-ROCm ops (SpectralConv1d_Uno runs on the 2-D kernels, one row; pointwise_op_3D's FFT
resampling on the pruned-DFT kernels with explicit frequency tables).  CPU tensors take stock torch ops in these helper
layers (they are not part of the spectral path and the CPU-side harness tests use them with the oracle blocks).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._param_grads import release_pass_state
from .block2d import SpectrumShare, _OperatorBlock2dCatFn, _OperatorBlock2dFn, _SpectralConv2dFn, spectral_conv2d, spectral_conv2d_mixed
from .pointwise import (GradJoin, _dev_act, channel_mix, channel_mix_cat, channel_mix_cat_project, gelu_channel_mix, gelu_channel_mix_pad,
                        gelu_pad2d, gelu_project, gelu_project2, instance_norm_gelu, lift_gelu_pad)
from .resample import resample2d_bicubic_aa
from .spectral3d import (RESAMPLE3D_FAMILIES, _OperatorBlock3dCatFn, _OperatorBlock3dFn, _resample3d_plan, _resample3d_plan_any, _resample3d_plan_wide, spectral_conv3d)

__all__ = [
    "enable_mixed_precision", "enable_native_resample3d_any", "enable_native_resample3d_wide", "enable_one_buffer_any_grid", "GradJoin", "SpectrumShare", "channel_mix_cat_project", "release_pass_state",
    "SpectralConv1d_Uno", "pointwise_op_1D", "OperatorBlock_1D",
    "SpectralConv2d_Uno", "pointwise_op_2D", "OperatorBlock_2D",
    "SpectralConv3d_Uno", "pointwise_op_3D", "OperatorBlock_3D",
]


def enable_mixed_precision(module: nn.Module, enabled: bool = True) -> nn.Module:
    """Let the 2-D spectral layers under `module` take bfloat16 activations (the reference raises on them, integral_operators.py:187,
    and so do these layers unless enabled here).  In that mode a layer reads its complex weights through a half-precision
    (re, im) copy made per call (the parameters themselves - and their gradients - stay complex64: the master copy the
    optimiser updates), transforms bf16 images directly and accumulates in f32 / c64; outputs and input gradients are bf16."""
    for m in module.modules():
        if isinstance(m, SpectralConv2d_Uno):
            m.mixed_precision = bool(enabled)
    return module


def _check_input(x: torch.Tensor, ndim: int, channels: int, who: str):
    if x.dim() != ndim:
        raise RuntimeError(f"{who}: expected a {ndim}-D tensor (batch, channels, *grid), got shape {tuple(x.shape)}")
    if x.shape[1] != channels:
        raise RuntimeError(f"{who}: expected {channels} input channels, got {x.shape[1]}")
    if x.dtype != torch.float32:
        # the reference raises as well: its out_ft is hard-coded cfloat, so a float64 input dies in the
        # einsum (integral_operators.py:179) and half/bfloat16 die in rfft2 (:187)
        raise RuntimeError(f"{who}: input must be float32 (got {x.dtype})")


# --------------------------------------------------------------------------------------------- 2-D
class SpectralConv2d_Uno(nn.Module):
    """2-D Fourier integral operator (reference integral_operators.py:127-207).

    in_codim / out_codim : input / output co-domain dimension (channels; floats are truncated)
    dim1, dim2           : default output grid size
    modes1, modes2       : Fourier modes kept along each axis; modes1 <= min(dim1, input_dim1) and
                           modes2 <= min(dim2, input_dim2)//2 + 1 (defaults dim1//2-1, dim2//2)
    """

    def __init__(self, in_codim, out_codim, dim1, dim2, modes1=None, modes2=None):
        super().__init__()
        in_codim, out_codim = int(in_codim), int(out_codim)
        self.in_channels = in_codim
        self.out_channels = out_codim
        self.dim1 = dim1
        self.dim2 = dim2
        if modes1 is not None:
            self.modes1, self.modes2 = modes1, modes2
        else:
            self.modes1, self.modes2 = dim1 // 2 - 1, dim2 // 2
        self.scale = (1 / (2 * in_codim)) ** (1.0 / 2.0)
        shape = (in_codim, out_codim, self.modes1, self.modes2)
        self.weights1 = nn.Parameter(self.scale * torch.randn(*shape, dtype=torch.cfloat))
        self.weights2 = nn.Parameter(self.scale * torch.randn(*shape, dtype=torch.cfloat))
        self.mixed_precision = False        # enable_mixed_precision(): accept bfloat16 activations (the reference raises)

    def forward(self, x, dim1=None, dim2=None):
        if dim1 is not None:        # persistent override, as in the reference (:182-184)
            self.dim1 = dim1
            self.dim2 = dim2
        if self.mixed_precision and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] == self.in_channels:
            if not self._bf16_kernels():
                # mode counts beyond the MFMA kernels' compiled range run the any-mode forms, which are float32 only: widen the
                # activations for this layer instead of raising at run time (the reference's DEFAULT modes land here)
                return spectral_conv2d(x.float(), self.weights1, self.weights2, self.dim1, self.dim2).to(torch.bfloat16)
            return _SpectralConv2dFn.apply(x, self.weights1, self.weights2, self.dim1, self.dim2, True)
        _check_input(x, 4, self.in_channels, "SpectralConv2d_Uno")
        return spectral_conv2d(x, self.weights1, self.weights2, self.dim1, self.dim2)

    def _bf16_kernels(self):
        """True when the bf16-image transform kernels cover this layer's mode counts (csrc/capi_spectral.hip: modes1 <= 40, modes2 <= 48)."""
        return self.modes1 <= 40 and self.modes2 <= 48


class pointwise_op_2D(nn.Module):
    """1x1 convolution followed by bicubic anti-aliased resampling to (dim1, dim2)
    (reference integral_operators.py:210-243)."""

    def __init__(self, in_codim, out_codim, dim1, dim2):
        super().__init__()
        self.conv = nn.Conv2d(int(in_codim), int(out_codim), 1)
        self.dim1 = int(dim1)
        self.dim2 = int(dim2)

    def forward(self, x, dim1=None, dim2=None):
        if dim1 is None:
            dim1, dim2 = self.dim1, self.dim2
        if not (_dev_act(x) and x.dim() == 4):
            return F.interpolate(self.conv(x), size=(dim1, dim2), mode="bicubic", align_corners=True, antialias=True)
        # HIP path: the resampling is a separable banded operator with the reference's weights (uno_amd/resample.py).
        # It commutes with the 1x1 convolution (both linear, resampling rows sum to 1 so the bias passes through),
        # so the convolution runs on whichever side has fewer pixels.
        if dim1 * dim2 < x.shape[-2] * x.shape[-1]:
            return channel_mix(resample2d_bicubic_aa(x, dim1, dim2), self.conv.weight, self.conv.bias)
        return resample2d_bicubic_aa(channel_mix(x.contiguous(), self.conv.weight, self.conv.bias), dim1, dim2)


class OperatorBlock_2D(nn.Module):
    """gelu( [InstanceNorm]( SpectralConv2d(x) + pointwise(x) ) )  (reference integral_operators.py:246-284)."""

    def __init__(self, in_codim, out_codim, dim1, dim2, modes1, modes2, Normalize=False, Non_Lin=True):
        super().__init__()
        self.conv = SpectralConv2d_Uno(in_codim, out_codim, dim1, dim2, modes1, modes2)
        self.w = pointwise_op_2D(in_codim, out_codim, dim1, dim2)
        self.normalize = Normalize
        self.non_lin = Non_Lin
        if Normalize:
            self.normalize_layer = nn.InstanceNorm2d(int(out_codim), affine=True)

    def forward(self, x, dim1=None, dim2=None, *, join=None, out_join=None, share=None):
        """join / out_join (optional, beyond the reference signature): GradJoin objects of the input / of this block's output - see
        GradJoin and _OperatorBlock2dFn.  share: SpectrumShare of the input, this block being its first spectral consumer."""
        if self.non_lin and not self.normalize:
            return self._branches(x, dim1, dim2, gelu=True, join=join, out_join=out_join, share=share)
        if out_join is not None:            # no GELU straight after the sum: this block leaves no pre-activation tensor to a join
            out_join.void()
        out = self._branches(x, dim1, dim2, join=join, share=share)
        if self.normalize:
            return instance_norm_gelu(out, self.normalize_layer, self.non_lin)
        return out

    def forward_cat(self, xs, dim1=None, dim2=None, defer_gelu=False, defer_grad=None, share=None):
        """self(torch.cat(xs, dim=1), dim1, dim2) for a skip connection (reference darcy_flow_uno2d.py:117-125) - two
        float32 device tensors are consumed in place, the concatenation is never built.  defer_gelu (blocks without
        normalisation only): return the PRE-activation sum; the caller's consumer applies the GELU as it reads it.  share: SpectrumShare of
        xs[1], whose first spectral consumer has transformed it for this block as well (the stock-op path ignores it)."""
        if defer_gelu and (self.normalize or not self.non_lin):
            raise ValueError("defer_gelu needs a block with Non_Lin=True and Normalize=False")
        xs = list(xs)
        conv, w = self.conv, self.w
        d1, d2 = (dim1, dim2) if dim1 is not None else (w.dim1, w.dim2)
        cdims = (dim1, dim2) if dim1 is not None else (conv.dim1, conv.dim2)
        fused = (len(xs) == 2 and all(self._takes(x) for x in xs) and xs[0].dtype == xs[1].dtype
                 and xs[0].shape[0] == xs[1].shape[0] and xs[0].shape[2:] == xs[1].shape[2:]
                 and xs[0].shape[1] + xs[1].shape[1] == conv.in_channels and cdims == (d1, d2)
                 and w.conv.weight.dtype == torch.float32)
        if not fused:
            if defer_grad is not None:      # xs[1]'s gradient reaches its producer through autograd, without the join's gelu' factor
                defer_grad.void()
            if defer_gelu:
                return self._branches(torch.cat(xs, dim=1), dim1, dim2)
            return self.forward(torch.cat(xs, dim=1), dim1, dim2)
        if dim1 is not None:
            conv.dim1, conv.dim2 = dim1, dim2
        out = _OperatorBlock2dCatFn.apply(xs[0], xs[1], conv.weights1, conv.weights2, w.conv.weight, w.conv.bias, int(d1), int(d2),
                                          xs[0].dtype == torch.bfloat16, defer_grad, share)
        if defer_gelu:
            return out
        if self.normalize:
            return instance_norm_gelu(out, self.normalize_layer, self.non_lin)
        return F.gelu(out) if self.non_lin else out

    def _branches(self, x, dim1, dim2, gelu=False, join=None, out_join=None, share=None):
        """conv(x) + w(x) [then GELU when `gelu`: written by the kernel that completes the sum where the fused path runs]"""
        conv, w = self.conv, self.w
        if dim1 is not None:        # the spectral layer keeps a call-time override, the point-wise one does not (:182-184, :236-238)
            conv.dim1, conv.dim2 = dim1, dim2
            d1, d2 = dim1, dim2
        else:
            d1, d2 = w.dim1, w.dim2
        fused = (self._takes(x) and (conv.dim1, conv.dim2) == (d1, d2)
                 and x.shape[1] == conv.in_channels and w.conv.weight.dtype == torch.float32)
        if not fused:               # CPU tensors raise inside the spectral layer; mismatched grids raise at the sum
            for j in (join, out_join):      # stock-op path: nothing here completes a joined gradient or leaves a pre-activation sum
                if j is not None:
                    j.void()
            out = conv(x) + w(x, d1, d2)
            return F.gelu(out) if gelu else out
        return _OperatorBlock2dFn.apply(x, conv.weights1, conv.weights2, w.conv.weight, w.conv.bias, int(d1), int(d2),
                                        x.dtype == torch.bfloat16, bool(gelu), join, out_join, share)

    def _takes(self, x):
        """4-D device tensor the fused block kernels take: float32, or bfloat16 once the spectral layer is in mixed-precision mode."""
        return (x.is_cuda and x.dim() == 4 and
                (x.dtype == torch.float32 or (x.dtype == torch.bfloat16 and getattr(self.conv, "mixed_precision", False)
                                              and self.conv._bf16_kernels())))


# --------------------------------------------------------------------------------------------- 3-D
class SpectralConv3d_Uno(nn.Module):
    """3-D Fourier integral operator (reference integral_operators.py:287-427): rfftn over the last
    three axes, four low-frequency corners (weights1..4 = (lo,lo), (hi,lo), (lo,hi), (hi,hi)),
    zero-padded irfftn to (dim1, dim2, dim3)."""

    def __init__(self, in_codim, out_codim, dim1, dim2, dim3, modes1=None, modes2=None, modes3=None):
        super().__init__()
        in_codim, out_codim = int(in_codim), int(out_codim)
        self.in_channels = in_codim
        self.out_channels = out_codim
        self.dim1, self.dim2, self.dim3 = dim1, dim2, dim3
        if modes1 is not None:
            self.modes1, self.modes2, self.modes3 = modes1, modes2, modes3
        else:
            self.modes1, self.modes2, self.modes3 = dim1, dim2, dim3 // 2 + 1
        self.scale = (1 / (2 * in_codim)) ** (1.0 / 2.0)
        shape = (in_codim, out_codim, self.modes1, self.modes2, self.modes3)
        self.weights1 = nn.Parameter(self.scale * torch.randn(*shape, dtype=torch.cfloat))
        self.weights2 = nn.Parameter(self.scale * torch.randn(*shape, dtype=torch.cfloat))
        self.weights3 = nn.Parameter(self.scale * torch.randn(*shape, dtype=torch.cfloat))
        self.weights4 = nn.Parameter(self.scale * torch.randn(*shape, dtype=torch.cfloat))

    def forward(self, x, dim1=None, dim2=None, dim3=None):
        if dim1 is not None:
            self.dim1, self.dim2, self.dim3 = dim1, dim2, dim3
        _check_input(x, 5, self.in_channels, "SpectralConv3d_Uno")
        return spectral_conv3d(x, [self.weights1, self.weights2, self.weights3, self.weights4],
                               self.dim1, self.dim2, self.dim3)


# pointwise_op_3D on a grid its pruned-DFT resampling kernels do not take (_resample3d_plan is None): False (default) - raise, naming the
# limits; True - run the reference's op sequence on torch.fft (rocFFT on the device: a stock-library dispatch the caller asked for)
STOCK_FFT_RESAMPLE3D = False
# ... and on such a grid with every axis length in 2 ... 128 (resample3d_any_applies): True - run the any-grid HIP kernels
# (uno_fft_resample3d_any: plain-FMA pruned transforms without the row-count / plane-size limits).  Opt-in: the default (False) leaves
# every module as it was; a single module opts in through its `native_any_grid` attribute (enable_native_resample3d_any).  A zero-edit
# user of the reference's navier_stokes_uno3d.py sets this switch once: Uno3D_T40's last two layers are outside the pruned-DFT range.
NATIVE_RESAMPLE3D_ANY = False


def enable_native_resample3d_any(module: nn.Module, enabled: bool = True) -> nn.Module:
    """Let every pointwise_op_3D under `module` run grids outside the pruned-DFT kernels' range on the any-grid HIP kernels
    (sets `native_any_grid`); grids inside the range keep their kernels."""
    for m in module.modules():
        if isinstance(m, pointwise_op_3D):
            m.native_any_grid = bool(enabled)
    return module


# ... and on a grid neither family takes, with the two leading axes in 2 ... 256 and the last in 2 ... 64 (resample3d_wide_applies): True - run
# the wide-axis HIP kernels (uno_fft_resample3d_wide: the long-axis sums on the f32 MFMA).  Opt-in in the same way: per module the attribute
# `native_wide_grid` (enable_native_resample3d_wide).  A zero-edit user of the reference's Uno3D_T20_256 / Uno3D_T10_256 sets this switch
# (and, for pad 3 on both sides, NATIVE_RESAMPLE3D_ANY): their first and last layers resample (256,256,T) <-> (64,64,T).
NATIVE_RESAMPLE3D_WIDE = False


def enable_native_resample3d_wide(module: nn.Module, enabled: bool = True) -> nn.Module:
    """Let every pointwise_op_3D under `module` run grids outside the older kernel families' ranges on the wide-axis HIP kernels (sets
    `native_wide_grid`); a grid the pruned-DFT kernels - or, where opted in, the any-grid kernels - take keeps that family."""
    for m in module.modules():
        if isinstance(m, pointwise_op_3D):
            m.native_wide_grid = bool(enabled)
    return module


def _resample3d_kernels(w, din, dout, device):
    """Which resample kernels the point-wise layer `w` takes for din -> dout: (plan, family).  The families are tried in order - "pruned"
    inside its range; then "any" where the layer is opted in (`native_any_grid` / NATIVE_RESAMPLE3D_ANY) and resample3d_any_applies
    holds; then "wide" where it is opted in (`native_wide_grid` / NATIVE_RESAMPLE3D_WIDE) and resample3d_wide_applies holds - so a grid
    an older family takes keeps that family; else (None, None)."""
    plan = _resample3d_plan(din, dout, device)
    if plan is not None:
        return plan, "pruned"
    if getattr(w, "native_any_grid", False) or NATIVE_RESAMPLE3D_ANY:
        plan = _resample3d_plan_any(din, dout, device)
        if plan is not None:
            return plan, "any"
    if getattr(w, "native_wide_grid", False) or NATIVE_RESAMPLE3D_WIDE:
        plan = _resample3d_plan_wide(din, dout, device)
        if plan is not None:
            return plan, "wide"
    return None, None


class pointwise_op_3D(nn.Module):
    """1x1x1 convolution + the reference's FFT crop/resample (quirks kept bug-for-bug: unnormalised
    forward transform, corners copied into an INPUT-sized zero spectrum, irfftn(s=output dims) that
    trims/zero-pads at the END of each axis, identity trilinear resize) - reference
    integral_operators.py:430-468.  The convolution runs on the channel-mix kernels (K8 / K9) for float32 device
    tensors - MIOpen executes a 1x1x1 Conv3d with its naive direct kernels, 0.9 s of a 2.2 s first NS-3D step - the
    FFT resampling runs on the pruned-DFT kernels (_FftResample3dFn; outside their shape range the layer runs the any-grid kernels where
    `native_any_grid` / NATIVE_RESAMPLE3D_ANY or the wide-axis kernels where `native_wide_grid` / NATIVE_RESAMPLE3D_WIDE opts in, else raises unless STOCK_FFT_RESAMPLE3D allows torch.fft); the trilinear resize to the size the tensor already has is an exact
    identity under align_corners=True and is skipped on the device."""

    def __init__(self, in_codim, out_codim, dim1, dim2, dim3):
        super().__init__()
        self.conv = nn.Conv3d(int(in_codim), int(out_codim), 1)
        self.dim1, self.dim2, self.dim3 = int(dim1), int(dim2), int(dim3)

    def _corner_mask(self, spec, h1, h2, h3):
        """(1, 1, D1, D2, D3/2+1) float mask of the entries the reference copies (integral_operators.py:450-461), cached per shape."""
        key = (tuple(spec.shape[2:]), h1, h2, h3, str(spec.device))
        cache = self.__dict__.setdefault("_mask_cache", {})
        if key not in cache:
            m = torch.zeros((1, 1, *spec.shape[2:]), dtype=torch.float32)
            for rows in (slice(None, h1), slice(-h1, None)):
                for cols in (slice(None, h2), slice(-h2, None)):
                    m[:, :, rows, cols, :h3] = 1.0
            cache[key] = m.to(spec.device)
        return cache[key]

    def forward(self, x, dim1=None, dim2=None, dim3=None):
        if dim1 is None:
            dim1, dim2, dim3 = self.dim1, self.dim2, self.dim3
        on_device = x.is_cuda and x.dtype == torch.float32 and x.dim() == 5
        out = channel_mix(x.contiguous(), self.conv.weight, self.conv.bias) if on_device else self.conv(x)
        if on_device:
            plan, family = _resample3d_kernels(self, out.shape[-3:], (dim1, dim2, dim3), out.device)
            if plan is not None:
                return RESAMPLE3D_FAMILIES[family][0].apply(out, (dim1, dim2, dim3), plan)
        if on_device and not STOCK_FFT_RESAMPLE3D:
            # no silent dispatch to a stock library from a product component: the pruned-DFT resampling kernels do not cover this grid
            raise RuntimeError(
                f"pointwise_op_3D: the FFT crop / resample {tuple(out.shape[-3:])} -> {(dim1, dim2, dim3)} is outside the range of the "
                "pruned-DFT kernels (they take an even number of kept rows per complex axis - at most 80 / 48 - and (W, T) planes of at most "
                "1792 elements with T <= 64); set uno_amd.integral_operators.STOCK_FFT_RESAMPLE3D = True to run this layer's resampling "
                "through torch.fft (rocFFT) instead, or - for axis lengths of 2 ... 128 - uno_amd.integral_operators.NATIVE_RESAMPLE3D_ANY = True "
                "(enable_native_resample3d_any(model) for one model) to run it on the any-grid HIP kernels, or - for leading axes of 2 ... 256 "
                "and a last axis of 2 ... 64 - uno_amd.integral_operators.NATIVE_RESAMPLE3D_WIDE = True (enable_native_resample3d_wide(model)) "
                "to run it on the wide-axis HIP kernels")
        spec = torch.fft.rfftn(out, dim=[-3, -2, -1])
        h1, h2, h3 = dim1 // 2, dim2 // 2, dim3 // 2
        if on_device:
            # the four corner copies into a zero spectrum == one multiplication by a 0 / 1 mask (same values bit for bit;
            # one pass forward and backward instead of zeros_like + 4 slice copies and their CopySlices backward chain)
            return torch.fft.irfftn(spec * self._corner_mask(spec, h1, h2, h3), s=(dim1, dim2, dim3))
        kept = torch.zeros_like(spec)
        for rows in (slice(None, h1), slice(-h1, None)):
            for cols in (slice(None, h2), slice(-h2, None)):
                kept[:, :, rows, cols, :h3] = spec[:, :, rows, cols, :h3]
        out = torch.fft.irfftn(kept, s=(dim1, dim2, dim3))
        return F.interpolate(out, size=(dim1, dim2, dim3), mode="trilinear", align_corners=True)


ONE_BUFFER_3D = True        # OperatorBlock_3D in one buffer (_OperatorBlock3dFn); False: the two branches and stock sum / GELU (A/B switch)
# ... and on a grid outside the pruned-DFT range whose point-wise layer runs the any-grid kernels: True - the same one-buffer form with
# uno_fft_resample3d_any_acc as its last transform - or, where the layer runs the wide-axis kernels (`native_wide_grid` /
# NATIVE_RESAMPLE3D_WIDE), uno_fft_resample3d_wide_acc.  Opt-in like NATIVE_RESAMPLE3D_ANY: the default (False) leaves every block on the two
# branches there; a single block opts in through its `one_buffer_any_grid` attribute (enable_one_buffer_any_grid).
ONE_BUFFER_3D_ANY = False


def enable_one_buffer_any_grid(module: nn.Module, enabled: bool = True) -> nn.Module:
    """Let every OperatorBlock_3D under `module` take the one-buffer form on grids outside the pruned-DFT kernels' range (sets
    `one_buffer_any_grid`; enabling also sets `native_any_grid` on the block's point-wise layer, which the form runs on).  Disabling
    clears the block attribute only.  Grids inside the range keep their kernels."""
    for m in module.modules():
        if isinstance(m, OperatorBlock_3D):
            m.one_buffer_any_grid = bool(enabled)
            if enabled:
                m.w.native_any_grid = True
    return module


class OperatorBlock_3D(nn.Module):
    """gelu( [InstanceNorm3d]( SpectralConv3d(x) + pointwise(x) ) )  (reference integral_operators.py:471-513)."""

    def __init__(self, in_codim, out_codim, dim1, dim2, dim3, modes1, modes2, modes3, Normalize=False, Non_Lin=True):
        super().__init__()
        self.conv = SpectralConv3d_Uno(in_codim, out_codim, dim1, dim2, dim3, modes1, modes2, modes3)
        self.w = pointwise_op_3D(in_codim, out_codim, dim1, dim2, dim3)
        self.normalize = Normalize
        self.non_lin = Non_Lin
        if Normalize:
            self.normalize_layer = nn.InstanceNorm3d(int(out_codim), affine=True)

    def forward(self, x, dim1=None, dim2=None, dim3=None):
        fused = self._fused(x, dim1, dim2, dim3)
        if fused is not None:
            out, activated = fused
            if self.normalize:
                return instance_norm_gelu(out, self.normalize_layer, self.non_lin)
            return out if (activated or not self.non_lin) else F.gelu(out)
        out = self.conv(x, dim1, dim2, dim3) + self.w(x, dim1, dim2, dim3)
        if self.normalize:
            return instance_norm_gelu(out, self.normalize_layer, self.non_lin)
        if self.non_lin:
            out = F.gelu(out)
        return out

    def forward_cat(self, xs, dim1=None, dim2=None, dim3=None):
        """self(torch.cat(xs, dim=1), dim1, dim2, dim3) for a skip connection (reference navier_stokes_uno3d.py: the inputs of the
        up-sampling blocks) - two float32 device tensors of equal batch and grid whose channels sum to in_channels, on a grid where
        forward() would take the one-buffer form, are consumed where they lie (_OperatorBlock3dCatFn): the concatenation is never
        built.  Anything else is forward() on the concatenation."""
        xs = list(xs)
        fused = None
        if (len(xs) == 2 and all(x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 for x in xs) and xs[0].device == xs[1].device
                and xs[0].shape[0] == xs[1].shape[0] and xs[0].shape[2:] == xs[1].shape[2:]
                and xs[0].shape[1] >= 1 and xs[1].shape[1] >= 1):
            fused = self._fused(xs, dim1, dim2, dim3)
        if fused is None:
            return self.forward(torch.cat(xs, dim=1), dim1, dim2, dim3)
        out, activated = fused
        if self.normalize:
            return instance_norm_gelu(out, self.normalize_layer, self.non_lin)
        return out if (activated or not self.non_lin) else F.gelu(out)

    def _fused(self, x, dim1, dim2, dim3):
        """(conv(x) + w(x) [activated], whether the GELU has been applied) through the one-buffer form, or None when the layer has to take
        the two branches separately (CPU tensors, other dtypes, mismatched grids, grids outside the pruned-DFT resampling kernels' range
        unless the block is opted into the one-buffer form there - `one_buffer_any_grid` / ONE_BUFFER_3D_ANY - and its point-wise layer
        into the any-grid or the wide-axis kernels, see _resample3d_kernels).  x: the input, or the list of forward_cat's two sources,
        which then go through the two-source form (_OperatorBlock3dCatFn) under the same conditions."""
        conv, w = self.conv, self.w
        pair =x if isinstance(x, list) else None           # forward_cat: two sources it has checked against each other
        if pair is not None:
            x = pair[0]
            channels = pair[0].shape[1] + pair[1].shape[1]
        else:
            channels = x.shape[1] if x.dim() == 5 else -1
        if not (ONE_BUFFER_3D and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and channels == conv.in_channels
                and w.conv.weight.dtype == torch.float32):
            return None
        if dim1 is not None:        # the spectral layer keeps a call-time override, the point-wise one does not (:391-394, :444-446)
            dims = (int(dim1), int(dim2), int(dim3))
        else:
            dims = (int(w.dim1), int(w.dim2), int(w.dim3))
            if (conv.dim1, conv.dim2, conv.dim3) != dims:
                return None
        din = tuple(x.shape[-3:])
        plan, family = _resample3d_kernels(w, din, dims, x.device)
        if plan is None or (family != "pruned" and not (getattr(self, "one_buffer_any_grid", False) or ONE_BUFFER_3D_ANY)):
            return None
        if dim1 is not None:
            conv.dim1, conv.dim2, conv.dim3 = dim1, dim2, dim3
        gelu = self.non_lin and not self.normalize
        if pair is not None:
            out = _OperatorBlock3dCatFn.apply(pair[0], pair[1], conv.weights1, conv.weights2, conv.weights3, conv.weights4, w.conv.weight,
                                              w.conv.bias, dims, plan, gelu, family)
            return out, gelu
        out = _OperatorBlock3dFn.apply(x, conv.weights1, conv.weights2, conv.weights3, conv.weights4, w.conv.weight, w.conv.bias,
                                       dims, plan, gelu, family)
        return out, gelu


# --------------------------------------------------------------------------------------------- 1-D
# Not on the north-star path and unused by every reference model; the
# names stay importable so `from integral_operators import *` keeps its surface.  Stock torch ops.
class SpectralConv1d_Uno(nn.Module):
    """1-D Fourier layer (reference integral_operators.py:7-72): single corner [:modes1]."""

    def __init__(self, in_codim, out_codim, dim1, modes1=None):
        super().__init__()
        in_codim, out_codim = int(in_codim), int(out_codim)
        self.in_channels, self.out_channels = in_codim, out_codim
        self.dim1 = dim1
        self.modes1 = modes1 if modes1 is not None else dim1 // 2
        self.scale = (1 / (2 * in_codim)) ** (1.0 / 2.0)
        self.weights1 = nn.Parameter(self.scale * torch.randn(in_codim, out_codim, self.modes1, dtype=torch.cfloat))

    def forward(self, x, dim1=None):
        if dim1 is not None:
            self.dim1 = dim1
        if x.is_cuda:
            # the 1-D layer is the 2-D one on a grid of one row: the row DFT of length 1 is the identity, both "corners" are the
            # row of frequency 0 and the later-wins rule keeps the second one - weights1 in both slots, the masked slot's
            # gradient is exactly zero
            _check_input(x, 3, self.in_channels, "SpectralConv1d_Uno")
            w = self.weights1.unsqueeze(2)
            return spectral_conv2d(x.unsqueeze(2), w, w, 1, self.dim1).squeeze(2)
        spec = torch.fft.rfft(x, norm="forward")
        out = torch.zeros(x.shape[0], self.out_channels, self.dim1 // 2 + 1, dtype=torch.cfloat, device=x.device)
        out[:, :, : self.modes1] = torch.einsum("bix,iox->box", spec[:, :, : self.modes1], self.weights1)
        return torch.fft.irfft(out, n=self.dim1, norm="forward")


class pointwise_op_1D(nn.Module):
    """1x1 conv + linear resampling (reference integral_operators.py:75-93; the reference's
    antialias=True is rejected by torch >= 2 for mode='linear', so it is not requested here)."""

    def __init__(self, in_codim, out_codim, dim1):
        super().__init__()
        self.conv = nn.Conv1d(int(in_codim), int(out_codim), 1)
        self.dim1 = int(dim1)

    def forward(self, x, dim1=None):
        if dim1 is None:
            dim1 = self.dim1
        return F.interpolate(self.conv(x), size=dim1, mode="linear", align_corners=True)


class OperatorBlock_1D(nn.Module):
    """reference integral_operators.py:96-124."""

    def __init__(self, in_codim, out_codim, dim1, modes1, Normalize=True, Non_Lin=True):
        super().__init__()
        self.conv = SpectralConv1d_Uno(in_codim, out_codim, dim1, modes1)
        self.w = pointwise_op_1D(in_codim, out_codim, dim1)
        self.normalize = Normalize
        self.non_lin = Non_Lin
        if Normalize:
            self.normalize_layer = nn.InstanceNorm1d(int(out_codim), affine=True)

    def forward(self, x, dim1=None):
        out = self.conv(x, dim1) + self.w(x, dim1)
        if self.normalize:
            out = self.normalize_layer(out)
        if self.non_lin:
            out = F.gelu(out)
        return out
