"""Darcy-flow U-NO (the 5-block "UNO_9" of the reference, darcy_flow_uno2d.py:27-141) built on the
MI355X-native operator blocks.  Sub-module names, shapes and registration order follow the reference,
so its state_dict loads with strict=True.  Differences are host-side hygiene only:
  * the positional grid is built once per (shape, device) and cached on the device instead of being rebuilt
    on the host and copied every forward (reference :135-141);
  * lift and projection run channels-first (the nn.Linear weights applied as batched GEMMs on the
    (B, C, pixels) view), which removes the two full-size permute copies around the U (reference :104, :126);
  * the point-wise projection runs before the crop (they commute), so the crop touches one channel.
The arithmetic is the reference's up to float32 summation order."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..integral_operators import (GradJoin, SpectrumShare, OperatorBlock_2D, OperatorBlock_3D, channel_mix, channel_mix_cat, channel_mix_cat_project,
                                  enable_native_resample3d_any, enable_native_resample3d_wide, enable_one_buffer_any_grid, gelu_channel_mix, gelu_channel_mix_pad, gelu_pad2d, gelu_project, gelu_project2,
                                  lift_gelu_pad)
from ..pointwise import gelu_channel_mix_pad_last

# The two ends of the NS-3D models on the short-row window kernels (csrc/channel_mix_rows.hip): the lift's second layer writes its padded
# activation itself (no F.gelu / F.pad passes) and fc1 reads conv8's output and the resized lift where they lie, through the time window
# the crop keeps (no last skip concatenation, no cropped copy; whole-plane gradients from one backward launch).  Opt-in: the default
# (False) leaves every model on the stock ops bit for bit; a single model opts in through its `native_ends` attribute
# (enable_native_ends_3d).  Product blocks on device tensors only.
NATIVE_ENDS_3D = False


def enable_native_ends_3d(model: nn.Module, enabled: bool = True) -> nn.Module:
    """Opt the NS-3D models inside `model` into the short-row window kernels for their lift and head (sets `native_ends`)."""
    for m in model.modules():
        if isinstance(m, Uno3D_T20):
            m.native_ends = bool(enabled)
    return model


# The INNER skip connections of the NS-3D models (the inputs of conv7 and conv8 of the seven-block models, of their counterparts in the
# nine-block ones) without torch.cat: the next block takes (its predecessor's output, the resized skip tensor) where they lie
# (OperatorBlock_3D.forward_cat).  The last skip (into fc1) is NATIVE_ENDS_3D's.  Opt-in like that switch: the default (False) leaves every
# model on the stock concatenation bit for bit; a single model opts in through its `cat_free_skips` attribute
# (enable_cat_free_skips_3d).  Product blocks on float32 device tensors only.
CAT_FREE_SKIPS_3D = False


def enable_cat_free_skips_3d(model: nn.Module, enabled: bool = True) -> nn.Module:
    """Opt the NS-3D models inside `model` into two-source blocks for their inner skip connections (sets `cat_free_skips`)."""
    for m in model.modules():
        if isinstance(m, Uno3D_T20):
            m.cat_free_skips = bool(enabled)
    return model


def _block_cat(block, xs, *dims):
    """block(torch.cat(xs, dim=1), *dims); product blocks take the sources as they are."""
    if hasattr(block, "forward_cat"):
        return block.forward_cat(xs, *dims)
    return block(torch.cat(list(xs), dim=1), *dims)


def _cached(cache: dict, key, build):
    grid = cache.get(key)
    if grid is None:
        grid = build()
        cache.clear()
        cache[key] = grid
    return grid


class UNO_9(nn.Module):
    """in_width = 3 ([a(x,y), x, y]); width = lifted channel count; pad = domain padding (scaled by
    ceil(S/85)); factor = channel growth per level.  Input (B, S, S, 1) -> output (B, S, S, 1)."""

    def __init__(self, in_width, width, pad=5, factor=1, block_cls=OperatorBlock_2D):
        super().__init__()
        self.in_width = in_width
        self.width = width
        self.padding = pad
        w, f = width, factor
        self.fc_n1 = nn.Linear(in_width, w // 2)
        self.fc0 = nn.Linear(w // 2, w)
        # (in, out, default grid, modes): grids are overridden at call time, modes are fixed
        self.conv0 = block_cls(w, 2 * f * w, 40, 40, 18, 18)
        self.conv1 = block_cls(2 * f * w, 4 * f * w, 20, 20, 8, 8, Normalize=True)
        self.conv2 = block_cls(4 * f * w, 4 * f * w, 20, 20, 8, 8)
        self.conv4 = block_cls(4 * f * w, 2 * f * w, 40, 40, 8, 8, Normalize=True)
        self.conv5 = block_cls(4 * f * w, w, 85, 85, 18, 18)
        self.fc1 = nn.Linear(2 * w, w)
        self.fc2 = nn.Linear(w, 1)
        self._grid_cache = {}

    def get_grid(self, shape, device):
        def build():
            b, sx, sy = shape[0], shape[1], shape[2]
            gx = torch.linspace(0, 1, sx, dtype=torch.float64).to(torch.float32).reshape(1, sx, 1, 1).expand(b, sx, sy, 1)
            gy = torch.linspace(0, 1, sy, dtype=torch.float64).to(torch.float32).reshape(1, 1, sy, 1).expand(b, sx, sy, 1)
            return torch.cat((gx, gy), dim=-1).contiguous().to(device)
        return _cached(self._grid_cache, (tuple(shape[:3]), str(device)), build)

    def forward(self, x):
        S1, S2 = x.shape[1], x.shape[2]
        x = torch.cat((x, self.get_grid(x.shape, x.device).to(x.dtype)), dim=-1).permute(0, 3, 1, 2).contiguous()   # (B, 3, S, S): tiny
        # lift + activation + domain padding: one forward kernel; neither fc_n1's nor fc0's output is stored (both are recomputed from
        # the 3-channel input where the backward pass needs them)
        scale = math.ceil(S2 / 85)
        margin = scale * self.padding
        product = hasattr(self.conv5, "forward_cat")          # MI355X operator blocks (the CPU baseline builds the model on oracle blocks)
        fused = product and self.conv5.non_lin and not self.conv5.normalize
        jl = GradJoin() if fused else None
        lifted = lift_gelu_pad(x, self.fc_n1, self.fc0, margin, margin, grad_join=jl)
        d1, d2 = lifted.shape[-2], lifted.shape[-1]

        if fused:
            # `lifted` and `c0` feed two layers each (skip connections).  Their gradients are JOINED: the later consumer leaves its
            # contribution (a truncated spectrum + accumulating closures) to the first consumer, which transforms the summed spectrum
            # once and returns the complete gradient - no second gradient tensor, no element-wise sum (GradJoin)
            # conv0 / conv2 end in a GELU (no normalisation): the block that completes the gradient of their output (conv1 with the
            # join of c0; conv4, c2's only consumer) applies gelu'(pre) in its last accumulating kernel (`out_join`)
            jc, j2 = GradJoin(), GradJoin()
            c0 = self.conv0(lifted, d1 // 2, d2 // 2, join=jl, out_join=jc)
            # ... and c0's forward TRANSFORM is shared: conv1 transforms it once at conv5's mode counts, into conv5's spectrum, and crops
            # its own (fewer) modes from that; conv5 skips its transform of c0 (SpectrumShare)
            sc = SpectrumShare.for_block(self.conv5, self.conv4.conv.out_channels)
            c1 = self.conv1(c0, d1 // 4, d2 // 4, join=jc, share=sc)
            c2 = self.conv2(c1, d1 // 4, d2 // 4, out_join=j2)
            # skip connections: conv5 consumes cat([conv4 output, c0]) and fc1 cat([conv5 output, lifted]) from their two
            # sources; the concatenations are never built.  conv5's GELU is deferred to its only consumer: fc1 applies it while
            # reading the pre-activation tensor
            skip5 = [self.conv4(c2, d1 // 2, d2 // 2, join=j2), c0]
            # fc2(gelu(fc1(cat([gelu(conv5 pre), lifted])))): one forward kernel (the fc1 pass also reduces its 64 channels to the output)
            # ... on the S1 x S2 domain only (the padding is cropped from the result: its points are never computed)
            out = channel_mix_cat_project([self.conv5.forward_cat(skip5, d1, d2, defer_gelu=True, defer_grad=jc, share=sc), lifted], self.fc1.weight,
                                          self.fc1.bias, self.fc2.weight, self.fc2.bias, gelu_first=True, defer_grad=jl, crop=(S1, S2))
            return out[:, :, :S1, :S2].permute(0, 2, 3, 1).contiguous()
        else:
            c0 = self.conv0(lifted, d1 // 2, d2 // 2)
            c1 = self.conv1(c0, d1 // 4, d2 // 4)
            c2 = self.conv2(c1, d1 // 4, d2 // 4)
            skip5 = [self.conv4(c2, d1 // 2, d2 // 2), c0]
            c5 = channel_mix_cat([_block_cat(self.conv5, skip5, d1, d2), lifted], self.fc1.weight, self.fc1.bias)
        out = gelu_project(c5, self.fc2.weight, self.fc2.bias)
        return out[:, :, :S1, :S2].permute(0, 2, 3, 1).contiguous()     # crop the padding, back to (B, S, S, 1) (one channel: tiny)


class UNO(nn.Module):
    """Navier-Stokes 2-D U-NO (7 blocks, channel growth factor 3/4) - own counterpart of the reference's
    `UNO` (navier_stokes_uno2d.py:145-238): one autoregressive step (B, S, S, T_in) -> (B, S, S, 1).  Input
    channels = T_in + 4 positional features (sin/cos of the two coordinates, :229-238).  Sub-module names and
    registration order follow the reference (state_dict compatible).  Channels-first lift/projection as in UNO_9.

    The NS-2-D family is this class: `UNO_P` and `UNO_S256` contribute their table of blocks, their widths around the U and their
    grids; constructor and forward pass are said here once."""

    # (dim1, dim2, modes1, modes2) of L0 .. L6: the default grids are overridden at call time, the modes are fixed
    _BLOCKS = ((48, 48, 22, 22), (32, 32, 14, 14), (16, 16, 6, 6), (16, 16, 6, 6), (32, 32, 6, 6), (48, 48, 14, 14), (64, 64, 22, 22))
    _LIFT = None            # width of the first lift layer (None: width // 2)
    _FC1 = 4                # fc1 = Linear(2w, _FC1 * w)
    _TWO_SOURCE = False     # fc2 also reads the first lift activation, and the padding is cropped on both sides (UNO_P)

    def __init__(self, in_width, width, pad=0, factor=3 / 4, block_cls=OperatorBlock_2D):
        super().__init__()
        self.in_width, self.width, self.factor, self.padding = in_width, width, factor, pad
        w, f = width, factor
        lift = w // 2 if self._LIFT is None else self._LIFT
        self.fc = nn.Linear(in_width, lift)
        self.fc0 = nn.Linear(lift, w)
        cin = (w, 2 * f * w, 4 * f * w, 8 * f * w, 8 * f * w, 8 * f * w, 4 * f * w)
        cout = (2 * f * w, 4 * f * w, 8 * f * w, 8 * f * w, 4 * f * w, 2 * f * w, w)
        for i, row in enumerate(self._BLOCKS):
            setattr(self, f"L{i}", block_cls(cin[i], cout[i], *row))
        self.fc1 = nn.Linear(2 * w, self._FC1 * w)
        self.fc2 = nn.Linear(self._FC1 * w + (lift if self._TWO_SOURCE else 0), 1)
        self._grid_cache = {}

    def get_grid(self, shape, device):
        def build():
            b, sx, sy = shape[0], shape[1], shape[2]
            gx = torch.linspace(0, 2 * math.pi, sx, dtype=torch.float64).to(torch.float32).reshape(1, sx, 1, 1).expand(b, sx, sy, 1)
            gy = torch.linspace(0, 2 * math.pi, sy, dtype=torch.float64).to(torch.float32).reshape(1, 1, sy, 1).expand(b, sx, sy, 1)
            return torch.cat((torch.sin(gx), torch.sin(gy), torch.cos(gx), torch.cos(gy)), dim=-1).contiguous().to(device)
        return _cached(self._grid_cache, (tuple(shape[:3]), str(device)), build)

    def _grids(self, d1, d2):
        """output grids of L0 .. L6 from the padded grid"""
        a, b, c = (int(d1 * self.factor), int(d2 * self.factor)), (d1 // 2, d2 // 2), (d1 // 4, d2 // 4)
        return a, b, c, c, b, a, (d1, d2)

    def forward(self, x):
        # channels-first input in ONE pass: the cat kernel reads the permuted view of x and the (cached, channels-first) grid features
        z = torch.cat((x.permute(0, 3, 1, 2), self.get_grid(x.shape, x.device).permute(0, 3, 1, 2)), dim=1)
        return self.forward_cf(z).permute(0, 2, 3, 1).contiguous()         # one channel: the permuted view IS contiguous

    def forward_cf(self, x):
        """(B, T_in + 4, S, S) channels-first window + positional features -> (B, 1, S, S).  The roll-out keeps its window in this
        layout (harness.ns2d_rollout_loss): one concatenation per step instead of one for the window and one for the layout."""
        return self.body_cf(channel_mix(x, self.fc.weight, self.fc.bias))

    def body_cf(self, h):
        """Everything after the first lift: h = fc(x), (B, lift width, S, S) channels-first and kept PRE-activation (fc0 and a two-source
        fc2 apply the GELU as they read it) -> (B, 1, S, S).  The native training roll-out (harness.ns2d_rollout_loss(native=True))
        forms h from the frames where they lie and calls this."""
        lifted = F.gelu(gelu_channel_mix(h, self.fc0.weight, self.fc0.bias))
        p = self.padding
        if p != 0:              # (F.pad with zero widths still copies the tensor: 40 copies per roll-out)
            lifted = F.pad(lifted, [p, p, p, p])
        g = self._grids(lifted.shape[-2], lifted.shape[-1])
        c0 = self.L0(lifted, *g[0])
        c1 = self.L1(c0, *g[1])
        if hasattr(self.L6, "forward_cat") and all(b.non_lin and not b.normalize for b in (self.L2, self.L3)):
            # c2 and c3 have ONE consumer each: that block applies gelu'(pre) of its producer in the kernel that completes the
            # gradient (`out_join`, as in UNO_9) - no separate GELU-backward pass for L2 / L3.  (The skip tensors are NOT joined
            # here the way UNO_9 joins them: at 64^2 x 32 samples every kernel of this model is a 10-30 us launch and the joined
            # form trades two big element-wise sums for more small launches - measured 81.4 -> 84.3 ms per step.)
            j2, j3 = GradJoin(), GradJoin()
            c2 = self.L2(c1, *g[2], out_join=j2)
            c3 = self.L3(c2, *g[3], join=j2, out_join=j3)
            c4 = self.L4(c3, *g[4], join=j3)
        else:
            c4 = self.L4(self.L3(self.L2(c1, *g[2]), *g[3]), *g[4])
        c4 = torch.cat([c4, c1], dim=1)
        c5 = torch.cat([self.L5(c4, *g[5]), c0], dim=1)
        c6 = torch.cat([self.L6(c5, *g[6]), lifted], dim=1)
        if p != 0:      # the reference's `UNO` pads both sides but crops one (navier_stokes_uno2d.py:201,217-218); kept
            c6 = c6[..., p:-p, p:-p] if self._TWO_SOURCE else c6[..., :-p, :-p]
        out = channel_mix(c6.contiguous(), self.fc1.weight, self.fc1.bias)
        if self._TWO_SOURCE:
            return gelu_project2(out, h, self.fc2.weight, self.fc2.bias, act2=True)
        return gelu_project(out, self.fc2.weight, self.fc2.bias)


class UNO_P(UNO):
    """Navier-Stokes 2-D U-NO with the more aggressive contraction (grids D/2, D/4, D/8 and back) - own counterpart of the reference's
    `UNO_P` (navier_stokes_uno2d.py:24-138).  Against `UNO`: hard-coded modes 14 / 6 / 3, factor 1, fc1 = Linear(2w, 3w), and fc2 reads
    the concatenation of gelu(fc1(.)) with the FIRST lift activation gelu(fc(x)) (:121-125) - here the two-source projection
    (gelu_project2) on fc1's output and fc's kept pre-activation; the concatenation is never built.  The padding is cropped on both
    sides (:116-117).  Sub-module names, registration order and `get_grid` follow the reference (state_dict compatible)."""

    _BLOCKS = ((32, 32, 14, 14), (16, 16, 6, 6), (8, 8, 3, 3), (8, 8, 3, 3), (16, 16, 3, 3), (32, 32, 6, 6), (64, 64, 14, 14))
    _FC1, _TWO_SOURCE = 3, True
    # output grid of L0 .. L6 as divisors of the padded grid (reference :99-113)
    _DIV = (2, 4, 8, 8, 4, 2, 1)

    def __init__(self, in_width, width, pad=0, factor=1, block_cls=OperatorBlock_2D):
        super().__init__(in_width, width, pad, factor, block_cls)

    def _grids(self, d1, d2):
        return [(d1 // k, d2 // k) for k in self._DIV]


class UNO_S256(UNO_P):
    """Navier-Stokes 2-D U-NO for 256 x 256 simulations - own counterpart of the reference's `UNO_S256` (navier_stokes_uno2d.py:246-337):
    `UNO_P`'s structure with grids D/4, D/16, D/32 and back (4x contraction and expansion per level), modes up to (32, 33), and a first
    lift layer of 16 channels whatever the width (fc2 = Linear(3w + 16, 1))."""

    _BLOCKS = ((64, 64, 32, 33), (16, 16, 8, 9), (8, 8, 4, 5), (8, 8, 4, 5), (16, 16, 4, 5), (64, 64, 8, 9), (256, 256, 32, 32))
    _LIFT = 16
    _DIV = (4, 16, 32, 32, 16, 4, 1)


def _grids3d(d1, d2, bottom, times):
    """Output grids of conv0 .. conv8 of the 3-D models: space contracts to 3/4, 1/2, 1/4 and `bottom` of the padded grid and expands
    back over the same levels; `times` is the time length per block."""
    a, b, c = (int(3 * d1 / 4), int(3 * d2 / 4)), (d1 // 2, d2 // 2), (d1 // 4, d2 // 4)
    return [(*s, t) for s, t in zip((a, b, c, bottom, b, a, (d1, d2)), times)]


class Uno3D_T20(nn.Module):
    """Navier-Stokes 3-D (space-time) U-NO mapping 10 input steps to 20 output steps - own counterpart of the
    reference's `Uno3D_T20` (navier_stokes_uno3d.py:239-409): 7 OperatorBlock_3D that also stretch the time axis,
    skip connections through (identity) trilinear resizes, time-axis padding int(pad * 0.1 * T).
    Input (B, S, S, T, 1) -> output (B, S, S, 2T, 1); in_width = 1 + 5 positional features.

    The NS-3-D family is this class: `Uno3D_T10`, `Uno3D_T9`, `Uno3D_T40` and the nine-block `Uno3D_T20_256` / `Uno3D_T10_256` contribute
    their table of blocks, the width of their first lift layer and their plan of grids; constructor and forward pass are said here once."""

    _NAMES = ("conv0", "conv1", "conv2", "conv3", "conv6", "conv7", "conv8")
    _NORMALIZED = ("conv0", "conv3", "conv7")
    # output channels of every block but the last (which has 2 * width) in units of factor * width; a block's input channels are its
    # predecessor's output plus what the predecessor's skip connection appends
    _WIDTHS = (2, 4, 8, 16, 4, 2)
    # block -> the earlier block whose output is appended to its own (None: the padded lift)
    _SKIPS = {"conv6": "conv1", "conv7": "conv0", "conv8": None}
    # (dim1, dim2, dim3, modes1, modes2, modes3) of conv0 .. conv8: the default grids are overridden at call time, the modes are fixed
    _BLOCKS = ((48, 48, 10, 22, 22, 5), (32, 32, 10, 14, 14, 5), (16, 16, 12, 6, 6, 5), (16, 16, 12, 6, 6, 6), (32, 32, 18, 6, 6, 6),
               (48, 48, 20, 14, 14, 8), (64, 64, 20, 22, 22, 8))

    @staticmethod
    def _lift_width(in_width, width):
        return in_width * 2

    @staticmethod
    def _plan(d1, d2, d3, padding):
        """the output grids of conv0 .. conv8 and the crop of the time axis, from the padded grid and the padding"""
        return _grids3d(d1, d2, (d1 // 4, d2 // 4), (d3, d3, int(d3 * 1.2), int(d3 * 1.2), int(d3 * 1.8), int(2.0 * d3), 2 * d3)), 2 * padding

    def __init__(self, in_width, width, pad=2, factor=1, pad_both=False, block_cls=OperatorBlock_3D):
        super().__init__()
        self.in_width, self.width, self.pad, self.pad_both = in_width, width, pad, pad_both
        w, f = width, factor
        lift = self._lift_width(in_width, w)
        self.fc = nn.Linear(in_width, lift)
        self.fc0 = nn.Linear(lift, w)
        cout = dict(zip(self._NAMES, [m * f * w for m in self._WIDTHS] + [2 * w]))
        cin = w
        for name, row in zip(self._NAMES, self._BLOCKS):
            setattr(self, name, block_cls(cin, cout[name], *row, Normalize=name in self._NORMALIZED))
            cin = cout[name] + (cout.get(self._SKIPS[name], w) if name in self._SKIPS else 0)
        self.fc1 = nn.Linear(3 * w, 4 * w)
        self.fc2 = nn.Linear(4 * w, 1)
        self._grid_cache = {}

    def get_grid(self, shape, device):
        def build():
            b, sx, sy, sz = shape[0], shape[1], shape[2], shape[3]
            lin = lambda hi, n: torch.linspace(0, hi, n, dtype=torch.float64).to(torch.float32)
            gx = lin(2 * math.pi, sx).reshape(1, sx, 1, 1, 1).expand(b, sx, sy, sz, 1)
            gy = lin(2 * math.pi, sy).reshape(1, 1, sy, 1, 1).expand(b, sx, sy, sz, 1)
            gz = lin(1, sz).reshape(1, 1, 1, sz, 1).expand(b, sx, sy, sz, 1)
            return torch.cat((torch.sin(gx), torch.sin(gy), torch.cos(gx), torch.cos(gy), gz), dim=-1).contiguous().to(device)
        return _cached(self._grid_cache, (tuple(shape[:4]), str(device)), build)

    native_ends = False         # enable_native_ends_3d: lift and head on the short-row window kernels

    def _native_ends(self, x):
        """the opted-in ends apply: switch or attribute on, product blocks, device tensors"""
        return bool((NATIVE_ENDS_3D or self.native_ends) and x.is_cuda and x.dtype == torch.float32
                    and isinstance(getattr(self, self._NAMES[-1]), OperatorBlock_3D))

    cat_free_skips = False      # enable_cat_free_skips_3d: the inner skip connections through OperatorBlock_3D.forward_cat

    def _cat_free_skips(self, x):
        """the opted-in inner skips apply: switch or attribute on, product blocks, device tensors"""
        return bool((CAT_FREE_SKIPS_3D or self.cat_free_skips) and x.is_cuda and x.dtype == torch.float32
                    and all(isinstance(getattr(self, n), OperatorBlock_3D) for n in self._NAMES))

    @staticmethod
    def _resize(t, like):
        # the reference resizes every skip tensor with trilinear / align_corners (navier_stokes_uno3d.py:352-372); on the
        # device this is the separable banded kernel (the stock backward kernel alone took 20 ms of a 60 ms step)
        from ..resample import resample3d_trilinear
        return resample3d_trilinear(t, tuple(like.shape[2:]))

    def forward(self, x):
        x = torch.cat((x, self.get_grid(x.shape, x.device)), dim=-1).permute(0, 4, 1, 2, 3).contiguous()
        native = self._native_ends(x)
        if native:      # the padded activation from fc0's own store epilogue
            h = channel_mix(x, self.fc.weight, self.fc.bias)
            self.padding = int(self.pad * 0.1 * h.shape[-1])
            lifted = gelu_channel_mix_pad_last(h, self.fc0.weight, self.fc0.bias, self.padding if self.pad_both else 0, self.padding)
        else:
            lifted = F.gelu(gelu_channel_mix(channel_mix(x, self.fc.weight, self.fc.bias), self.fc0.weight, self.fc0.bias))
            self.padding = int(self.pad * 0.1 * lifted.shape[-1])
            lifted = F.pad(lifted, [self.padding, self.padding, 0, 0, 0, 0] if self.pad_both else [0, self.padding, 0, 0, 0, 0])
        g, crop = self._plan(*lifted.shape[-3:], self.padding)
        outs, c8 = {None: lifted}, lifted
        last = self._NAMES[-1]
        cat_free, skip = self._cat_free_skips(x), None      # skip: the resized tensor the next block takes as its second source
        for name, grid in zip(self._NAMES, g):
            block = getattr(self, name)
            c8 = outs[name] = block(c8, *grid) if skip is None else _block_cat(block, (c8, skip), *grid)
            skip = None
            if name in self._SKIPS and not (native and name == last):
                if cat_free and name != last:
                    skip = self._resize(outs[self._SKIPS[name]], c8)
                else:
                    c8 = torch.cat([c8, self._resize(outs[self._SKIPS[name]], c8)], dim=1)
        if native:      # fc1 on the two sources of the last skip connection, through the time window the crop keeps
            Tp = c8.shape[-1]
            window = None if self.padding == 0 else (crop, Tp - 2 * crop) if self.pad_both else (0, Tp - crop)
            out = channel_mix_cat([c8, self._resize(outs[self._SKIPS[last]], c8)], self.fc1.weight, self.fc1.bias, last_window=window)
            return gelu_project(out, self.fc2.weight, self.fc2.bias).permute(0, 2, 3, 4, 1).contiguous()
        if self.padding != 0:           # (the crop is written from `padding` as the reference writes it: -0 would empty the tensor)
            c8 = c8[..., crop:-crop] if self.pad_both else c8[..., :-crop]
        out = gelu_project(channel_mix(c8.contiguous(), self.fc1.weight, self.fc1.bias), self.fc2.weight, self.fc2.bias)
        return out.permute(0, 2, 3, 4, 1).contiguous()


class Uno3D_T10(Uno3D_T20):
    """Navier-Stokes 3-D U-NO mapping 10 input steps to 10 output steps - own counterpart of the reference's `Uno3D_T10`
    (navier_stokes_uno3d.py:412-602): the T20 network with a time axis that keeps its (padded) length through all seven blocks
    (5 time modes everywhere) and a `padding` crop.  Input (B, S, S, T, 1) -> output (B, S, S, T, 1).  Every layer's grid pair is
    inside the pruned-DFT kernels' range at S <= 64 (tests/test_harness_ns3d_models.py holds the census)."""

    _BLOCKS = ((48, 48, 10, 22, 22, 5), (32, 32, 10, 14, 14, 5), (16, 16, 10, 6, 6, 5), (16, 16, 10, 6, 6, 5), (32, 32, 10, 6, 6, 5),
               (48, 48, 10, 14, 14, 5), (64, 64, 10, 22, 22, 5))

    @staticmethod
    def _plan(d1, d2, d3, padding):
        return _grids3d(d1, d2, (d1 // 4, d2 // 4), (d3,) * 7), padding


class Uno3D_T9(Uno3D_T10):
    """Navier-Stokes 3-D U-NO mapping 6 input steps to 9 output steps - own counterpart of the reference's `Uno3D_T9`
    (navier_stokes_uno3d.py:605-797): modes 20 / 18 / 6 / 6 / 6 / 14 / 20 in space and 3 (4 in conv8) in time, a time axis that grows
    to int(8 * d3 / 6) at conv3 / conv6 and int(9 * d3 / 6) at conv7 / conv8, and an int(9 * padding / 6) crop.  Input
    (B, S, S, 6, 1) -> output (B, S, S, 9, 1).  conv1 keeps 18 modes on the half grid, so S >= 36 (the reference raises below)."""

    _BLOCKS = ((48, 48, 6, 20, 20, 3), (32, 32, 6, 18, 18, 3), (16, 16, 6, 6, 6, 3), (16, 16, 8, 6, 6, 3), (32, 32, 8, 6, 6, 3),
               (48, 48, 9, 14, 14, 3), (64, 64, 9, 20, 20, 4))

    @staticmethod
    def _plan(d1, d2, d3, padding):
        times = (d3, d3, d3, int(8 * d3 / 6), int(8 * d3 / 6), int(9 * d3 / 6), int(9 * d3 / 6))
        return _grids3d(d1, d2, (d1 // 4, d2 // 4), times), int(9 * padding / 6)


class Uno3D_T40(Uno3D_T20):
    """Navier-Stokes 3-D U-NO mapping 10 input steps to 40 output steps - own counterpart of the reference's `Uno3D_T40`
    (navier_stokes_uno3d.py:22-237): the T20 network with a narrower lift (width // 2), a deeper bottom level (conv3 at an eighth of
    the grid), a time axis stretched 1.6 / 2.4 / 3.2 / 4 times and a `4 * padding` crop.  Input (B, S, S, T, 1) -> output
    (B, S, S, 4T, 1).  Its last two layers resample grids outside the pruned-DFT kernels' range ((32,32,31) -> (48,48,41) ->
    (64,64,52) at S = 64, pad 3): on product blocks the model opts its point-wise layers into the any-grid kernels, and with
    `one_buffer_any=True` its blocks into the one-buffer form on those grids (enable_one_buffer_any_grid)."""

    _BLOCKS = ((48, 48, 10, 20, 20, 4), (32, 32, 10, 14, 14, 4), (16, 16, 16, 6, 6, 4), (16, 16, 16, 6, 6, 7), (32, 32, 24, 6, 6, 7),
               (48, 48, 32, 14, 14, 10), (64, 64, 40, 20, 20, 14))

    @staticmethod
    def _lift_width(in_width, width):
        return width // 2

    @staticmethod
    def _plan(d1, d2, d3, padding):
        return _grids3d(d1, d2, (d1 // 8, d2 // 8), (d3, d3, int(d3 * 1.6), int(d3 * 1.6), int(d3 * 2.4), int(3.2 * d3), 4 * d3)), 4 * padding

    def __init__(self, in_width, width, pad=2, factor=1, pad_both=False, block_cls=OperatorBlock_3D, one_buffer_any=False):
        super().__init__(in_width, width, pad, factor, pad_both, block_cls)
        if issubclass(block_cls, OperatorBlock_3D):
            enable_native_resample3d_any(self)
            if one_buffer_any:
                enable_one_buffer_any_grid(self)


class Uno3D_T20_256(Uno3D_T20):
    """Navier-Stokes 3-D U-NO for 256 x 256 simulations, 10 input steps to 20 output steps - own counterpart of the reference's
    `Uno3D_T20_256` (navier_stokes_uno3d.py:993-1181): nine blocks on grids D/4, D/16, D/32 (four times), D/16, D/4, D (4x contraction
    and expansion per level, as the 2-D `UNO_S256`), modes up to (32, 32, 8), a lift of width // 2, normalisation on conv0, conv3,
    conv5 and conv7, the time axis stretched 1.2 / 1.6 / 1.8 / 2 times and a `2 * padding` crop.  Input (B, S, S, T, 1) -> output
    (B, S, S, 2T, 1).  At S = 256 its first and last layers resample (256,256,T) <-> (64,64,T), outside the pruned-DFT and the any-grid
    kernels' ranges: on product blocks the model opts its point-wise layers into the any-grid and the wide-axis kernels, and with
    `one_buffer_any=True` its blocks into the one-buffer form on those grids.  (The reference's `Uno3D_T40_256` and `Uno3D_T9_256` have
    no counterpart: upstream the first cannot run a forward pass and the second cannot be constructed.)"""

    _NAMES = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv8")
    _NORMALIZED = ("conv0", "conv3", "conv5", "conv7")
    _WIDTHS = (2, 4, 8, 16, 16, 8, 4, 2)
    _BLOCKS = ((64, 64, 10, 32, 32, 5), (16, 16, 10, 8, 8, 5), (8, 8, 12, 4, 4, 5), (8, 8, 12, 4, 4, 6), (8, 8, 16, 4, 4, 6),
               (8, 8, 16, 4, 4, 8), (16, 16, 18, 4, 4, 8), (64, 64, 20, 8, 8, 8), (256, 256, 20, 32, 32, 8))
    _DIV = (4, 16, 32, 32, 32, 32, 16, 4, 1)        # output grid of conv0 .. conv8 as divisors of the padded grid (reference :1092-1128)

    @staticmethod
    def _lift_width(in_width, width):
        return width // 2

    @classmethod
    def _plan(cls, d1, d2, d3, padding):
        times = (d3, d3, int(d3 * 1.2), int(d3 * 1.2), int(d3 * 1.6), int(d3 * 1.6), int(d3 * 1.8), int(2.0 * d3), 2 * d3)
        return [(d1 // k, d2 // k, t) for k, t in zip(cls._DIV, times)], 2 * padding

    def __init__(self, in_width, width, pad=2, factor=1, pad_both=False, block_cls=OperatorBlock_3D, one_buffer_any=False):
        super().__init__(in_width, width, pad, factor, pad_both, block_cls)
        if issubclass(block_cls, OperatorBlock_3D):
            enable_native_resample3d_any(self)
            enable_native_resample3d_wide(self)
            if one_buffer_any:
                enable_one_buffer_any_grid(self)


class Uno3D_T10_256(Uno3D_T20_256):
    """Navier-Stokes 3-D U-NO for 256 x 256 simulations, 10 input steps to 10 output steps - own counterpart of the reference's
    `Uno3D_T10_256` (navier_stokes_uno3d.py:1184-1372): `Uno3D_T20_256` with 5 / 4 time modes, a time axis that shrinks to
    int(0.8 * d3) through the five inner blocks and returns to d3, and a `padding` crop.  Input (B, S, S, T, 1) -> output (B, S, S, T, 1)."""

    _BLOCKS = ((64, 64, 10, 32, 32, 5), (16, 16, 10, 8, 8, 4), (8, 8, 8, 4, 4, 4), (8, 8, 8, 4, 4, 4), (8, 8, 8, 4, 4, 4),
               (8, 8, 8, 4, 4, 4), (16, 16, 8, 4, 4, 4), (64, 64, 10, 8, 8, 4), (256, 256, 10, 32, 32, 5))

    @classmethod
    def _plan(cls, d1, d2, d3, padding):
        times = (d3, d3) + (int(0.8 * d3),) * 5 + (d3, d3)
        return [(d1 // k, d2 // k, t) for k, t in zip(cls._DIV, times)], padding
