"""Point-wise layers of the operator blocks and of the models' lift / projection on the channel-mix, GELU-pad and InstanceNorm
kernels: autograd Functions, their functional forms, and GradJoin (one gradient buffer for a tensor with two consumers)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _native
from ._param_grads import _layer_grad_targets, _stack_pointwise


# activation dtypes the device kernels take: float32 (the reference's contract) and bfloat16 (mixed precision, BASELINE.json
# configs[4]: opt-in per spectral layer via enable_mixed_precision - weights, statistics and accumulations stay float32)
_ACT = (torch.float32, torch.bfloat16)


def _dev_act(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype in _ACT


def _plain(t: torch.Tensor) -> torch.Tensor:
    """Materialise lazy conj/neg views and non-contiguous layouts (the C ABI takes dense buffers;
    the reference accepts any strides - integral_operators.py:187 goes through torch.fft)."""
    if t.is_complex() and t.is_conj():
        t = t.resolve_conj()
    if t.is_neg():
        t = t.resolve_neg()
    if t.is_contiguous():
        return t
    # channels-last activations and gradients (what the reference's model files hand over: darcy_flow_uno2d.py:104-107, :126) go
    # through the tiled transposing copy; every other layout through torch's strided copy
    if t.is_cuda and t.dtype == torch.float32 and _native.channels_last_pitch(t) is not None:
        return _native.to_channels_first(t)
    return t.contiguous()


class _ChannelMixFn(torch.autograd.Function):
    """y[b] = W . x[b] + bias on (B, C, pixels) views with the K8 / K9 kernels (csrc/channel_mix.hip, csrc/channel_wgrad.hip)."""

    @staticmethod
    def forward(ctx, x, w, bias, leaves=None):
        x, w = _plain(x), _plain(w)
        y = _native.channel_mix(x, w, None if bias is None else _plain(bias))
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.leaves = leaves
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _plain(gy)
        gx = _native.channel_mix(gy, w, None, transpose_w=True) if ctx.needs_input_grad[0] else None
        gw, gb = _wgrad_into(ctx.leaves, gy, x, None, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        return gx, gw, gb, None


def channel_mix(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """1x1 convolution of a channels-first tensor, y[b] = W . x[b] (+ bias) on the (B, C, pixels) view - no
    layout change, no im2col.  `weight` is a Conv (Co, Ci, 1, ...) or Linear (Co, Ci) weight.  float32 tensors on
    a HIP device run the K8 / K9 kernels; anything else (the CPU-side harness tests, other dtypes) is a stock
    batched matmul - this helper is not part of the spectral path and keeps torch semantics there."""
    B, Ci = x.shape[0], x.shape[1]
    w = weight.reshape(weight.shape[0], Ci)
    xv = x.reshape(B, Ci, -1)
    if _dev_act(x) and w.dtype == torch.float32:
        y = _ChannelMixFn.apply(xv, w, bias, (weight, bias))
    elif bias is not None:
        y = torch.baddbmm(bias.view(1, -1, 1), w.unsqueeze(0).expand(B, -1, -1), xv)
    else:
        y = torch.matmul(w, xv)
    return y.view(B, w.shape[0], *x.shape[2:])


def _wgrad_into(leaves, gy, x1, x2, need_w, need_b, act_x=False, stack=None, window=None):
    """Weight / bias gradient of a channel-mix layer (K9), written in place where the layer's leaf parameters allow it.
    leaves = (weight leaf, bias leaf or None) or None.  -> (gw or None shaped (Co, Ci), gb or None) to return to autograd.
    stack = the _StackSlot of the block's spectral layer when that is batching its weight gradient over the uses of the pass: the
    second stage of this gradient is deferred to the last use as well (_stack_pointwise).  window: see _native.channel_mix2."""
    if not (need_w or need_b):
        return None, None
    has_bias = need_b
    lt = None
    fused = x2 is None or (x1.shape[1] % 64 == 0 and gy.shape[2] >= 64)
    if window is not None:
        if not fused:
            raise RuntimeError("uno_amd: a windowed two-source layer splits its sources at a multiple of 64 channels")
        stack = None
    if stack is not None and fused and leaves is not None and need_w and (leaves[1] is not None) == has_bias and gy.dtype == torch.float32 \
            and all(isinstance(t, torch.Tensor) and t.is_leaf for t in leaves if t is not None):
        out = _stack_pointwise(stack, leaves, gy, x1, x2, has_bias, act_x)
        if out is not NotImplemented:
            return out
    if fused and need_w:
        lt = _layer_grad_targets(leaves, has_bias)        # committed: the call below writes them
    if lt is not None:
        _native.channel_wgrad2(gy, x1, x2, need_bias=has_bias, act_x=act_x, out_w=lt.out_w, out_b=lt.out_b, accumulate=lt.accumulate,
                               window=window)
        return lt.gw, lt.gb
    if window is not None:
        return _native.channel_wgrad2(gy, x1, x2, need_bias=has_bias, act_x=act_x, window=window)
    if x2 is None:
        return _native.channel_wgrad(gy, x1, need_bias=has_bias, act_x=act_x)
    return _mix2_wgrad(gy, x1, x2, has_bias, act_x=act_x)


# The backward pass of `fc2(F.gelu(fc1(cat)))` (reference darcy_flow_uno2d.py:125-131).  True: uno_project_backward where it applies - the
# gradient at fc1's output is formed inside the input-gradient and weight-gradient kernels from fc1's saved output; False: written by
# uno_gelu_project_backward and read back by the two (A/B switch; tools/dev/fusetime.py).
PROJECT_BACKWARD_FUSED = True


class GradJoin:
    """One gradient buffer for a tensor with TWO consumers (a skip connection: reference darcy_flow_uno2d.py:117-127 feeds `x_c0`
    to conv1 and, concatenated, to conv5; `x_fc0` to conv0 and to fc1) instead of two gradient tensors and an element-wise sum.

    The consumer that comes LATER in the forward pass (its backward runs first) is called with `defer_grad=join`: its backward does
    not materialise its contribution; it leaves (a) its truncated gradient spectrum for that input - the inverse transform is
    linear, two spectra on one grid are added in the (tiny) spectral domain and transformed ONCE - and (b) closures that accumulate
    its point-wise contribution into a given buffer.  The consumer that comes FIRST in the forward pass (`join=join`; its backward
    runs last - it depends on everything downstream of its output) merges the spectra into its own before the inverse transform,
    then lets the closures accumulate into its gradient buffer, and returns the complete gradient.  The deferring consumer returns
    None for that input.  Used by the harness models; without a join object every layer behaves as before."""

    def __init__(self):
        self.owner = False          # set by the first consumer's forward when it will produce the joined gradient
        self.spectra = []           # (gX (B, C, 2 m1, m2) c64, grid (H, W)) left by deferring consumers
        self.pending = []           # (callable(out, dgelu_of=None), fusable): accumulate into out (B, C, H, W); a fusable one can also
                                    # multiply the completed sum by gelu'(dgelu_of) in its epilogue
        # the joined tensor is the ACTIVATION of a block without normalisation (`out_join=` of the block that produces it): its
        # pre-activation sum, and whether the gradient handed back to that block has already been multiplied by gelu'(pre)
        self.pre = None
        self.dgelu_applied = False
        # the joined tensor is the output of the lift (lift_gelu_pad(grad_join=)): its backward kernel streams the gradient once and can add
        # a second tensor as it reads.  A deferring consumer whose contribution is a plain windowed tensor then leaves it in `extra` (no
        # accumulation pass into the owner's buffer); the lift's backward takes it.  (tensor, window) pairs.
        self.accepts_extra = False
        self.extra = []

    def reset(self):
        self.owner = False
        self.spectra, self.pending = [], []

    def take_extra(self):
        out, self.extra = self.extra, []
        return out

    def void(self):
        """A consumer or producer that was handed this join cannot honour it (it runs a stock-op path): the fused GELU derivative is
        off for this pass - the producer block applies gelu'(pre) itself to the SUM of the gradients autograd delivers, which is
        correct whatever path each consumer took."""
        self.pre = None
        self.dgelu_applied = False

    def late(self, g):
        """Gradient contribution of a consumer whose backward runs AFTER the owner's (graph order did not put it first, so it could
        not defer): when the owner has already multiplied its result by gelu'(pre) - the producer will then skip its own GELU
        backward - this contribution needs the factor as well."""
        if g is not None and self.dgelu_applied and self.pre is not None:
            g = torch.ops.aten.gelu_backward(g.contiguous(), self.pre.view(g.shape))
        return g

    def merge(self, gX, grid):
        """own gradient spectrum (B, C, 2 m1, m2) + the deferred ones, embedded by frequency into the largest mode box"""
        if not self.spectra:
            return gX
        specs = [gX] + [s for s, g in self.spectra if g == tuple(grid)]
        if len(specs) != len(self.spectra) + 1:
            raise RuntimeError("GradJoin: a deferred gradient spectrum belongs to another grid")
        M1 = max(s.shape[2] // 2 for s in specs)
        M2 = max(s.shape[3] for s in specs)
        base = next((s for s in specs[1:] if s.shape[2] // 2 == M1 and s.shape[3] == M2), None)   # a deferred copy is ours to modify
        if base is None:
            base = torch.zeros((*gX.shape[:2], 2 * M1, M2), dtype=gX.dtype, device=gX.device)
        for s in specs:
            if s is base:
                continue
            m1, m2 = s.shape[2] // 2, s.shape[3]
            base[:, :, :m1, :m2] += s[:, :, :m1]                         # frequencies 0 .. m1 - 1
            base[:, :, 2 * M1 - m1:, :m2] += s[:, :, m1:]                # frequencies -m1 .. -1
        self.spectra = []
        return base

    def apply(self, out, final_dgelu=None):
        """run the deferred accumulations; with final_dgelu (the producer block's pre-activation sum) the LAST one - if it is a
        channel-mix call - also multiplies the completed gradient by gelu'(final_dgelu).  -> True when that happened"""
        fused = False
        n = len(self.pending)
        for k, (fn, fusable) in enumerate(self.pending):
            if final_dgelu is not None and fusable and k == n - 1:
                fn(out, final_dgelu)
                fused = True
            else:
                fn(out)
        self.pending = []
        return fused


# ---- a layer on the channel concatenation of two tensors, never built: one pass over every operand where the kernels' split
# rules allow (csrc/channel_mix.hip, csrc/channel_wgrad.hip: sources split at a multiple of 16 channels, destinations / weight-gradient tiles at 64),
# two accumulating calls otherwise
def _mix2_forward(x1, x2, w, bias, act_in=False, out=None, accumulate=False):
    """Wm . cat(x1, x2) + bias -> (B, Co, P); w (Co, C1 + C2).  out + accumulate: out += ..."""
    C1 = x1.shape[1]
    if C1 % 16 == 0:
        return _native.channel_mix2(x1, x2, w, bias, act_in=act_in, out=out, accumulate=accumulate)
    w1, w2 = w[:, :C1].contiguous(), w[:, C1:].contiguous()
    if out is None:
        out = _native.channel_mix(x1, w1, bias, act_in=act_in)
    elif accumulate:
        _native.channel_mix(x1, w1, bias, act_in=act_in, out=out)        # out= of the one-source call accumulates
    else:
        out.copy_(_native.channel_mix(x1, w1, bias, act_in=act_in))
    _native.channel_mix(x2, w2, None, out=out)
    return out


def _mix2_input_grads(gy, w, C1, dgelu_of=None, out1=None, out2=None):
    """(W[:, :C1]^T gy [* gelu'(dgelu_of)], W[:, C1:]^T gy) from one read of gy; out1 / out2: accumulate into these."""
    if C1 % 64 == 0 and (w.shape[1] - C1) >= 1:
        if out1 is not None and out2 is not None:
            _native.channel_mix2(gy, None, w, None, transpose_w=True, out=out1, out2=out2, split_out=C1, dgelu_of=dgelu_of, accumulate=True)
            return out1, out2
        if out1 is None and out2 is None:
            return _native.channel_mix2(gy, None, w, None, transpose_w=True, split_out=C1, dgelu_of=dgelu_of)
    w1, w2 = w[:, :C1].contiguous(), w[:, C1:].contiguous()
    g1 = _native.channel_mix(gy, w1, None, transpose_w=True, dgelu_of=dgelu_of, out=out1)
    g2 = _native.channel_mix(gy, w2, None, transpose_w=True, out=out2)
    return g1, g2


def _mix2_wgrad(gy, x1, x2, need_bias, act_x=False):
    """gw (Co, C1 + C2), gb of a two-source layer."""
    if x1.shape[1] % 64 == 0 and gy.shape[2] >= 64:
        return _native.channel_wgrad2(gy, x1, x2, need_bias=need_bias, act_x=act_x)
    gw1, gb = _native.channel_wgrad(gy, x1, need_bias=need_bias, act_x=act_x)
    gw2, _ = _native.channel_wgrad(gy, x2, need_bias=False)
    return torch.cat([gw1, gw2], dim=1), gb


def _clear_window_border(g, window):
    """What a windowed kernel did not write of the planes of g (B, C, pixels): the columns right of the window, the rows below it (a
    gradient's consumers - the transforms and resampling of the producing block - read whole planes).  -> g"""
    rows, cols, pitch = window
    _native.clear_border(g.view(g.shape[0], g.shape[1], -1, pitch), rows, cols)
    return g


def _first_source_grad(ctx, x1, w, gy, window=None):
    """W[:, :C1]^T gy [* gelu'(x1)]: the gradient of the first source of a two-source layer, from a launch of its own."""
    return _native.channel_mix(gy, w[:, :x1.shape[1]].contiguous(), None, transpose_w=True, dgelu_of=x1 if ctx.gelu_first else None,
                               window=window)


class _ChannelMixCatFn(torch.autograd.Function):
    """y[b] = W . cat(a1[b], x2[b]) + bias without the concatenation: W[:, :C1] . a1 writes y, W[:, C1:] . x2
    accumulates into it; the input gradients come out as two contiguous tensors (no strided slices of a joint one).
    gelu_first: a1 = gelu(x1) with x1 kept pre-activation - the GELU is applied as K8 / K9 read x1, and the input-gradient
    call returns the gradient of x1 itself (its epilogue multiplies by gelu'(x1)): the activation tensor never exists."""

    @staticmethod
    def forward(ctx, x1, x2, w, bias, gelu_first, defer=None, grid=None, leaves=None):
        ctx.leaves = leaves
        x1, x2, w = _plain(x1), _plain(x2), _plain(w)
        y = _mix2_forward(x1, x2, w, None if bias is None else _plain(bias), act_in=gelu_first)
        ctx.save_for_backward(x1, x2, w)
        ctx.has_bias = bias is not None
        ctx.gelu_first = gelu_first
        ctx.defer = defer if (defer is not None and defer.owner and ctx.needs_input_grad[1]) else None
        ctx.grid = grid
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x1, x2, w = ctx.saved_tensors[:3]
        return _ChannelMixCatFn._backward(ctx, x1, x2, w, _plain(gy)) + (None, None, None, None)

    @staticmethod
    def _backward(ctx, x1, x2, w, gy):
        """(g1, g2, gw, gb) of y = W . cat([gelu](x1), x2) + b for the output gradient gy (shared with the fused-projection form).
        ctx.window (fused-projection form): gy is valid on that window of its planes only; the gradients come out as whole planes
        with a cleared border."""
        window = getattr(ctx, "window", None)
        if window is not None:
            return _ChannelMixCatFn._backward_window(ctx, x1, x2, w, gy, window)
        C1 = x1.shape[1]
        g1 = g2 = None
        if ctx.defer is not None and ctx.defer.owner and ctx.needs_input_grad[1]:     # owner still pending: its backward has not run yet
            # x2's gradient is accumulated later into the buffer of x2's other consumer (GradJoin): no tensor, no sum
            if ctx.needs_input_grad[0]:
                g1 = _first_source_grad(ctx, x1, w, gy)
            w2 = w[:, C1:].contiguous()
            B, C2 = x2.shape[0], x2.shape[1]
            ctx.defer.pending.append((lambda out, dg=None: _native.channel_mix(
                gy, w2, None, transpose_w=True, out=out.view(B, C2, -1), dgelu_of=None if dg is None else dg.view(B, C2, -1),
                dgelu_total=dg is not None), True))
        elif ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            g1, g2 = _mix2_input_grads(gy, w, C1, dgelu_of=x1 if ctx.gelu_first else None)
        elif ctx.needs_input_grad[0]:
            g1 = _first_source_grad(ctx, x1, w, gy)
        elif ctx.needs_input_grad[1]:
            g2 = _native.channel_mix(gy, w[:, C1:].contiguous(), None, transpose_w=True)
        if ctx.defer is not None and g2 is not None:        # the owner's backward came first after all
            g2 = ctx.defer.late(g2)
        gw, gb = _wgrad_into(ctx.leaves, gy, x1, x2, ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3], act_x=ctx.gelu_first)
        return g1, g2, gw, gb

    @staticmethod
    def _backward_window(ctx, x1, x2, w, gy, window):
        C1 = x1.shape[1]
        B, C2 = x2.shape[0], x2.shape[1]
        g1 = g2 = None
        deferred = ctx.defer is not None and ctx.defer.owner and ctx.needs_input_grad[1]
        if deferred and ctx.defer.accepts_extra and ctx.needs_input_grad[0] and C1 % 64 == 0 and not ctx.defer.extra:
            # x2 is the lift's output: both input gradients from ONE pass over gy (two destinations); x2's stays a tensor of its own,
            # valid on the window, that the lift's backward kernel adds to the owner's gradient as it reads the two (no border to clear:
            # that kernel reads the domain only)
            g1, g2w = _native.channel_mix2(gy, None, w, None, transpose_w=True, split_out=C1, dgelu_of=x1 if ctx.gelu_first else None,
                                           window=window)
            _clear_window_border(g1, window)
            ctx.defer.extra.append((g2w, window))
        elif deferred:
            if ctx.needs_input_grad[0]:
                g1 = _clear_window_border(_first_source_grad(ctx, x1, w, gy, window), window)
            w2 = w[:, C1:].contiguous()
            # accumulates into the window of the other consumer's (whole-plane) gradient: nothing to clear.  NOT fusable: a fused
            # gelu'(pre) epilogue would reach the window only, and the border of the joined gradient holds the owner's own non-zero
            # contribution - the owner applies gelu' to the whole plane itself (GradJoin.apply reports "not fused")
            ctx.defer.pending.append((lambda out, dgo=None: _native.channel_mix(
                gy, w2, None, transpose_w=True, out=out.view(B, C2, -1), window=window), False))
        else:
            if ctx.needs_input_grad[0]:
                g1 = _clear_window_border(_first_source_grad(ctx, x1, w, gy, window), window)
            if ctx.needs_input_grad[1]:
                g2 = _clear_window_border(_native.channel_mix(gy, w[:, C1:].contiguous(), None, transpose_w=True, window=window), window)
                if ctx.defer is not None:        # the owner's backward came first after all
                    g2 = ctx.defer.late(g2)
        gw, gb = _wgrad_into(ctx.leaves, gy, x1, x2, ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3], act_x=ctx.gelu_first,
                             window=window)
        return g1, g2, gw, gb


class _ChannelMixCatProjectFn(torch.autograd.Function):
    """out[b, p] = b2 + sum_o w2[o] gelu(y[b, o, p]),  y = W . cat([gelu](x1), x2) + b: the end of the models, `fc2(F.gelu(fc1(cat)))`
    with one output channel (reference darcy_flow_uno2d.py:122-131), in ONE pass - the channel-mix kernel that produces y (kept:
    its GELU derivative is needed backward) also reduces its 64-channel tile to the projected value, so y is not read again."""

    @staticmethod
    def forward(ctx, x1, x2, w, bias, w2, b2, gelu_first, defer=None, leaves=None, window=None):
        ctx.leaves = leaves
        ctx.window = window
        x1, x2, w, w2 = _plain(x1), _plain(x2), _plain(w), _plain(w2)
        y, out = _native.channel_mix2(x1, x2, w, None if bias is None else _plain(bias), act_in=gelu_first,
                                      project=(w2, None if b2 is None else _plain(b2)), window=window)
        ctx.save_for_backward(x1, x2, w, y, w2)
        ctx.has_bias, ctx.has_b2 = bias is not None, b2 is not None
        ctx.gelu_first = gelu_first
        ctx.defer = defer if (defer is not None and defer.owner and ctx.needs_input_grad[1]) else None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x1, x2, w, y, w2 = ctx.saved_tensors
        mode = _ChannelMixCatProjectFn._fused_mode(ctx, x1, x2, y)
        if mode:
            return _ChannelMixCatProjectFn._backward_fused(ctx, x1, x2, w, y, w2, _plain(gout), mode)
        gy, gw2, gb2 = _native.gelu_project_backward(y, w2, _plain(gout), need_bias=ctx.has_b2, window=ctx.window)
        g1, g2, gw, gb = _ChannelMixCatFn._backward(ctx, x1, x2, w, gy)
        return g1, g2, gw, gb, gw2, gb2, None, None, None, None

    @staticmethod
    def _fused_mode(ctx, x1, x2, y):
        """0: the three-call backward pass; 1: uno_project_backward, both input gradients returned; 2: the same with x2's gradient handed
        to the owner of the joined gradient as a second tensor (the lift's backward kernel adds the two as it reads them)."""
        if not PROJECT_BACKWARD_FUSED or x1.dtype != torch.float32 or not all(ctx.needs_input_grad[:3]) or not ctx.needs_input_grad[4]:
            return 0
        B, C1, P = x1.shape
        if not _native.project_backward_applies(B, C1, C1 + x2.shape[1], y.shape[1], P, ctx.window):
            return 0
        if ctx.defer is None:
            return 1
        if ctx.window is not None and ctx.defer.accepts_extra and not ctx.defer.extra:
            return 2
        return 0

    @staticmethod
    def _backward_fused(ctx, x1, x2, w, y, w2, gout, mode):
        window = ctx.window
        need_b = ctx.has_bias and ctx.needs_input_grad[3]
        lt = _layer_grad_targets(ctx.leaves, need_b)        # committed: the call below writes them
        g1, g2, gw, gb, gw2, gb2 = _native.project_backward(
            x1, x2, w, y, w2, gout, act_in=ctx.gelu_first, need_bias=need_b, need_bias2=ctx.has_b2 and ctx.needs_input_grad[5], window=window,
            out_w=None if lt is None else lt.out_w, out_b=None if lt is None else lt.out_b, accumulate=False if lt is None else lt.accumulate)
        if lt is not None:
            gw, gb = lt.gw, lt.gb
        if window is not None:
            _clear_window_border(g1, window)
            if mode == 2:
                ctx.defer.extra.append((g2, window))        # (no border to clear: the lift's backward kernel reads the domain only)
                g2 = None
            else:
                _clear_window_border(g2, window)
        return g1, g2, gw, gb, gw2, gb2, None, None, None, None


def channel_mix_cat_project(xs, weight, bias, weight2, bias2, gelu_first: bool = False, defer_grad=None, crop=None):
    """gelu_project(channel_mix_cat(xs, weight, bias, gelu_first), weight2, bias2) - `fc2(F.gelu(fc1(torch.cat(xs, 1))))` of the
    models - as one forward kernel where the shapes allow (two device tensors split at a multiple of 16 channels, at most 64
    channels between the two layers, ONE output channel).
    crop = (S1, S2): the caller keeps only out[..., :S1, :S2] (the reference removes the domain padding BEFORE these layers,
    darcy_flow_uno2d.py:125): the kernels then work on that window of the padded tensors - forward and backward - and the rest of
    the returned (B, 1, H, W) tensor is undefined.  Ignored where the windowed kernels do not apply."""
    Co = weight.shape[0]
    if (len(xs) == 2 and all(_dev_act(x) for x in xs) and xs[0].dtype == xs[1].dtype and weight.dtype == torch.float32
            and weight2.shape[0] == 1 and Co <= 64 and xs[0].shape[1] % 16 == 0 and weight2.dtype == torch.float32):
        x1, x2 = xs
        B = x1.shape[0]
        w = weight.reshape(Co, -1)
        window = None
        if crop is not None and x1.dim() == 4 and x1.dtype == torch.float32 and x1.shape[1] % 64 == 0:
            H, W = x1.shape[2:]
            rows, cols = int(crop[0]), (int(crop[1]) + 3) & ~3
            if 0 < rows <= H and 260 <= cols <= W and rows * cols < (1 << 24) and (rows < H or cols < W) and tuple(x2.shape[2:]) == (H, W):
                window = (rows, cols, W)
        out = _ChannelMixCatProjectFn.apply(x1.reshape(B, x1.shape[1], -1), x2.reshape(B, x2.shape[1], -1), w, bias,
                                            weight2.reshape(Co), bias2, bool(gelu_first), defer_grad, (weight, bias), window)
        return out.view(B, 1, *x1.shape[2:])
    return gelu_project(channel_mix_cat(xs, weight, bias, gelu_first=gelu_first, defer_grad=defer_grad), weight2, bias2)


def _wgrad_rows_into(leaves, gy, x1, x2, window, need_w, need_b, act_x=False):
    """_wgrad_into for a layer whose sources are read through a short-row window (uno_channel_wgrad2_rows): the same in-place rules
    (INPLACE_PARAM_GRADS, the accumulate path) through _layer_grad_targets."""
    if not (need_w or need_b):
        return None, None
    lt = _layer_grad_targets(leaves, need_b) if need_w else None        # committed: the call below writes them
    if lt is not None:
        _native.channel_wgrad2_rows(gy, x1, x2, window, need_bias=need_b, act_x=act_x, out_w=lt.out_w, out_b=lt.out_b, accumulate=lt.accumulate)
        return lt.gw, lt.gb
    return _native.channel_wgrad2_rows(gy, x1, x2, window, need_bias=need_b, act_x=act_x)


class _ChannelMixCatRowsFn(torch.autograd.Function):
    """y = W . cat([gelu](x1), x2)[..., col0 : col0 + cols] + bias for channels-first tensors whose LAST axis is short (the time axis of
    the NS-3D models: reference navier_stokes_uno3d.py:358-382) with neither the concatenation nor the cropped copy: the kernels read
    the two sources through the window (uno_channel_mix2_rows) and the backward pass returns whole-plane gradients for both - the
    border columns zero - from one launch (uno_channel_mix2_rows_grad), the parameter gradients from uno_channel_wgrad2_rows."""

    @staticmethod
    def forward(ctx, x1, x2, w, bias, gelu_first, window, leaves=None):
        x1, x2, w = _plain(x1), _plain(x2), _plain(w)
        y = _native.channel_mix2_rows(x1, x2, w, None if bias is None else _plain(bias), window, act_in=gelu_first)
        ctx.save_for_backward(x1, x2, w)
        ctx.has_bias, ctx.gelu_first, ctx.window, ctx.leaves = bias is not None, gelu_first, window, leaves
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x1, x2, w = ctx.saved_tensors
        gy = _plain(gy)
        g1 = g2 = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g1, g2 = _native.channel_mix2_rows_grad(gy, w, x1.shape[1], ctx.window, x1.shape[2], need_g2=ctx.needs_input_grad[1],
                                                    dgelu_of=x1 if ctx.gelu_first else None)
            if not ctx.needs_input_grad[0]:         # (the kernel has no form without the first source: its gradient is computed and dropped;
                g1 = None                           # the models always need both)
        gw, gb = _wgrad_rows_into(ctx.leaves, gy, x1, x2, ctx.window, ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3],
                                  act_x=ctx.gelu_first)
        return g1, g2, gw, gb, None, None, None


def _last_window_rows(xs, weight, last_window):
    """(rows, cols, pitch, col0) when the short-row kernels take channel_mix_cat(xs, ..., last_window=), else None"""
    if len(xs) != 2 or not all(x.is_cuda and x.dtype == torch.float32 for x in xs) or weight.dtype != torch.float32:
        return None
    x1, x2 = xs
    if x1.dim() < 3 or x1.shape[0] != x2.shape[0] or x1.shape[2:] != x2.shape[2:] or x2.shape[1] < 1:
        return None
    col0, cols = int(last_window[0]), int(last_window[1])
    pitch = x1.shape[-1]
    rows = 1
    for d in x1.shape[2:-1]:
        rows *= d
    if x1.shape[0] == 0 or rows == 0:
        return None
    if not _native.rows_window_ok(rows, cols, pitch, col0, rows * pitch, x1.shape[1] + x2.shape[1], weight.shape[0]):
        return None
    return rows, cols, pitch, col0


def channel_mix_cat(xs, weight: torch.Tensor, bias: torch.Tensor | None, gelu_first: bool = False, defer_grad=None,
                    last_window=None) -> torch.Tensor:
    """channel_mix(torch.cat(xs, dim=1), weight, bias) - the projection after a skip connection (reference
    darcy_flow_uno2d.py:122-127: `torch.cat([x_c5, x_fc0], dim=1)` then `fc1`) - without materialising the
    concatenation when there are two float32 device tensors.  gelu_first: xs[0] is a PRE-activation tensor and stands
    for gelu(xs[0]) (the block in front deferred its GELU to this consumer).  defer_grad: a GradJoin whose owner is xs[1]'s other
    consumer - xs[1]'s gradient is then accumulated into that consumer's buffer (fused device path only).
    last_window = (col0, cols): the layer is applied to torch.cat(xs, 1)[..., col0 : col0 + cols] (the time-axis crop of the NS-3D models,
    reference navier_stokes_uno3d.py:371-379) -> dense (B, Co, ..., cols); two float32 device tensors inside the short-row kernels' range
    are read where they lie (no concatenation, no cropped copy; defer_grad does not go with it), anything else takes the stock ops."""
    if last_window is not None:
        win = _last_window_rows(xs, weight, last_window)
        if win is not None:
            x1, x2 = xs
            B = x1.shape[0]
            w = weight.reshape(weight.shape[0], -1)
            if defer_grad is not None:          # the window form returns xs[1]'s gradient as a tensor: the join is not honoured
                defer_grad.void()
            y = _ChannelMixCatRowsFn.apply(x1.reshape(B, x1.shape[1], -1), x2.reshape(B, x2.shape[1], -1), w, bias, bool(gelu_first), win,
                                           (weight, bias))
            return y.view(B, w.shape[0], *x1.shape[2:-1], win[1])
        xs = list(xs)
        if defer_grad is not None:
            defer_grad.void()
        if gelu_first:
            xs[0] = F.gelu(xs[0])
        col0, cols = int(last_window[0]), int(last_window[1])
        return channel_mix(torch.cat(xs, dim=1)[..., col0:col0 + cols].contiguous(), weight, bias)
    if len(xs) == 2 and all(_dev_act(x) for x in xs) and xs[0].dtype == xs[1].dtype and weight.dtype == torch.float32:
        x1, x2 = xs
        B = x1.shape[0]
        w = weight.reshape(weight.shape[0], -1)
        y = _ChannelMixCatFn.apply(x1.reshape(B, x1.shape[1], -1), x2.reshape(B, x2.shape[1], -1), w, bias, bool(gelu_first),
                                   defer_grad, tuple(x2.shape[2:]), (weight, bias))
        return y.view(B, w.shape[0], *x1.shape[2:])
    xs = list(xs)
    if defer_grad is not None:
        defer_grad.void()
    if gelu_first:
        xs[0] = F.gelu(xs[0])
    return channel_mix(torch.cat(xs, dim=1), weight, bias)


class _GeluChannelMixFn(torch.autograd.Function):
    """y[b] = W . gelu(pre[b]) + bias with `pre` kept pre-activation (the lift `fc0(F.gelu(fc_n1(x)))`, reference
    darcy_flow_uno2d.py:98-101): GELU on read in K8 / K9, gelu'(pre) in the input-gradient epilogue."""

    @staticmethod
    def forward(ctx, pre, w, bias, leaves=None):
        pre, w = _plain(pre), _plain(w)
        y = _native.channel_mix(pre, w, None if bias is None else _plain(bias), act_in=True)
        ctx.save_for_backward(pre, w)
        ctx.has_bias = bias is not None
        ctx.leaves = leaves
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        pre, w = ctx.saved_tensors
        gy = _plain(gy)
        g_pre = _native.channel_mix(gy, w, None, transpose_w=True, dgelu_of=pre) if ctx.needs_input_grad[0] else None
        gw, gb = _wgrad_into(ctx.leaves, gy, pre, None, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], act_x=True)
        return g_pre, gw, gb, None


def gelu_channel_mix(pre: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """channel_mix(F.gelu(pre), weight, bias) without the activation tensor (float32 device tensors)."""
    B, Ci = pre.shape[0], pre.shape[1]
    w = weight.reshape(weight.shape[0], Ci)
    if _dev_act(pre) and w.dtype == torch.float32:
        y = _GeluChannelMixFn.apply(pre.reshape(B, Ci, -1), w, bias, (weight, bias))
        return y.view(B, w.shape[0], *pre.shape[2:])
    return channel_mix(F.gelu(pre), weight, bias)


class _GeluChannelMixPadFn(torch.autograd.Function):
    """zero-pad(gelu(W . gelu(pre) + bias)): the second lift layer, its activation and the domain padding (reference
    darcy_flow_uno2d.py:100-107) from ONE forward kernel - the layer's store epilogue writes the padded activation and nothing else
    (uno_channel_mix_act_padded without y).  The pre-activation result is not kept: the backward pass RECOMPUTES it from the layer's
    input (32 channels against the 64 it would store and re-read) inside the kernel that multiplies gelu' into the cropped
    gradient (uno_channel_mix_dgelu_padded), then runs the layer's two gradient kernels as in _GeluChannelMixFn."""

    @staticmethod
    def forward(ctx, pre, w, bias, Hp, Wp, leaves=None):
        pre, w = _plain(pre), _plain(w)
        bias = None if bias is None else _plain(bias)
        _, act = _native.channel_mix_act_padded(pre, w, bias, Hp, Wp, act_in=True, keep_y=False)
        ctx.save_for_backward(pre, w, bias)
        ctx.has_bias = bias is not None
        ctx.leaves = leaves
        return act

    @staticmethod
    @once_differentiable
    def backward(ctx, gact):
        pre, w, bias = ctx.saved_tensors
        B, Ci, Co = pre.shape[0], pre.shape[1], w.shape[0]
        gz = _native.channel_mix_dgelu_padded(pre, w, bias, _plain(gact), act_in=True).view(B, Co, -1)
        pre3 = pre.view(B, Ci, -1)
        g_pre = _native.channel_mix(gz, w, None, transpose_w=True, dgelu_of=pre3).view(pre.shape) if ctx.needs_input_grad[0] else None
        gw, gb = _wgrad_into(ctx.leaves, gz, pre3, None, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], act_x=True)
        return g_pre, gw, gb, None, None, None


def gelu_channel_mix_pad(pre: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, pad_h: int, pad_w: int) -> torch.Tensor:
    """gelu_pad2d(gelu_channel_mix(pre, weight, bias), pad_h, pad_w) - `F.pad(F.gelu(fc0(F.gelu(pre))), [0, pad_w, 0, pad_h])` - with the
    activation and the padding written by fc0's own kernel where the shapes allow (4-D float32 device tensor, width >= 260)."""
    if pre.dim() == 4 and _dev_act(pre) and weight.dtype == torch.float32 and pad_h >= 0 and pad_w >= 0:
        Hp, Wp = pre.shape[2] + int(pad_h), pre.shape[3] + int(pad_w)
        if _native.channel_mix_act_padded_ok(pre, Hp, Wp):
            return _GeluChannelMixPadFn.apply(pre, weight.reshape(weight.shape[0], pre.shape[1]), bias, Hp, Wp, (weight, bias))
    return gelu_pad2d(gelu_channel_mix(pre, weight, bias), pad_h, pad_w)


class _GeluChannelMixPadLastFn(torch.autograd.Function):
    """zero-pad along the LAST axis (gelu(W . gelu(pre) + bias)): the second lift layer of the NS-3D models, its activation and the
    time-axis padding (reference navier_stokes_uno3d.py:304-318) from ONE forward kernel whose store epilogue writes the padded
    activation (uno_channel_mix_act_padded_rows).  The dense pre-activation result is kept: the backward pass multiplies gelu' of it
    into the window of the padded gradient (uno_dgelu_rows) and runs the layer's two gradient kernels as in _GeluChannelMixFn."""

    @staticmethod
    def forward(ctx, pre, w, bias, window, leaves=None):
        pre, w = _plain(pre), _plain(w)
        y, act = _native.channel_mix_act_padded_rows(pre, w, None if bias is None else _plain(bias), window, act_in=True, keep_y=True)
        ctx.save_for_backward(pre, w, y)
        ctx.has_bias, ctx.window, ctx.leaves = bias is not None, window, leaves
        return act

    @staticmethod
    @once_differentiable
    def backward(ctx, gact):
        pre, w, y = ctx.saved_tensors
        gz = _native.dgelu_rows(y, _plain(gact), ctx.window)
        g_pre = _native.channel_mix(gz, w, None, transpose_w=True, dgelu_of=pre) if ctx.needs_input_grad[0] else None
        gw, gb = _wgrad_into(ctx.leaves, gz, pre, None, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2], act_x=True)
        return g_pre, gw, gb, None, None


def gelu_channel_mix_pad_last(pre: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, pad_left: int, pad_right: int) -> torch.Tensor:
    """F.pad(F.gelu(gelu_channel_mix(pre, weight, bias)), [pad_left, pad_right]) - the 3-D sibling of gelu_channel_mix_pad: the lift's
    second layer, its GELU and the zero padding of the LAST (time) axis (reference navier_stokes_uno3d.py:304-318) with the activation
    and the padding written by the layer's own kernel for a float32 device tensor inside the short-row kernels' range; the stock ops
    otherwise."""
    pl, pr = int(pad_left), int(pad_right)
    if pre.dim() >= 3 and pre.is_cuda and pre.dtype == torch.float32 and weight.dtype == torch.float32 and pl >= 0 and pr >= 0 and pre.numel() > 0:
        B, Ci, T = pre.shape[0], pre.shape[1], pre.shape[-1]
        rows = pre.numel() // (B * Ci * T)
        pitch = T + pl + pr
        Co = weight.shape[0]
        if _native.rows_window_ok(rows, T, pitch, pl, rows * pitch, Ci, Co):
            act = _GeluChannelMixPadLastFn.apply(pre.reshape(B, Ci, -1), weight.reshape(Co, Ci), bias, (rows, T, pitch, pl), (weight, bias))
            return act.view(B, Co, *pre.shape[2:-1], pitch)
    return F.pad(F.gelu(gelu_channel_mix(pre, weight, bias)), [pl, pr] + [0, 0] * (pre.dim() - 3))


class _LiftFn(torch.autograd.Function):
    """The whole lift - zero-pad(gelu(fc0(gelu(fc_n1(x))))), reference darcy_flow_uno2d.py:98-107 - with neither layer's output stored
    (uno_lift_forward / uno_lift_backward): the first layer has 3 input channels, so every kernel that needs its 32-channel result
    evaluates it from x.  x is data: no gradient for it."""

    @staticmethod
    def forward(ctx, x, w1, b1, w0, b0, Hp, Wp, grad_join=None):
        x, w1, w0 = _plain(x), _plain(w1), _plain(w0)
        b1 = None if b1 is None else _plain(b1)
        b0 = None if b0 is None else _plain(b0)
        ctx.save_for_backward(x, w1, w0, *[t for t in (b1, b0) if t is not None])
        ctx.has = (b1 is not None, b0 is not None)
        ctx.join = None
        if grad_join is not None:
            grad_join.accepts_extra = bool(_native.lift_backward_takes_second(x, w1, w0, Hp, Wp))
            grad_join.extra = []
            ctx.join = grad_join
        return _native.lift_forward(x, w1, b1, w0, b0, Hp, Wp)

    @staticmethod
    @once_differentiable
    def backward(ctx, gact):
        x, w1, w0, *bs = ctx.saved_tensors
        b1 = bs.pop(0) if ctx.has[0] else None
        b0 = bs.pop(0) if ctx.has[1] else None
        gact = _plain(gact)
        g2 = None
        if ctx.join is not None:
            ctx.join.accepts_extra = False
            H, W = x.shape[-2:]
            for t, (rows, cols, pitch) in ctx.join.take_extra():
                t = t.view(gact.shape)
                if g2 is None and rows >= H and cols >= W and pitch == gact.shape[-1]:
                    g2 = t                  # covers the domain on the same planes: the kernel adds it as it reads
                else:                       # (not reached by the harness models) any other extra: a windowed element-wise sum
                    gact = gact.clone()
                    gact[..., :rows, :cols] += t[..., :rows, :cols]
        gw1, gb1, gw0, gb0 = _native.lift_backward(x, w1, b1, w0, b0, gact, g2)
        return None, gw1, gb1, gw0, gb0, None, None, None


def lift_gelu_pad(x: torch.Tensor, fc_n1: nn.Module, fc0: nn.Module, pad_h: int, pad_w: int, grad_join=None) -> torch.Tensor:
    """F.pad(F.gelu(fc0(F.gelu(fc_n1(x)))), [0, pad_w, 0, pad_h]) for a channels-first x (B, Cin, H, W) and two nn.Linear layers, as one
    forward kernel and one backward kernel that store neither intermediate nor their gradients, where the shapes allow (at most 3 input channels, 16 or 32
    in the middle, width >= 260, float32, x without gradient); the layer-by-layer forms otherwise.
    grad_join: the GradJoin of the RESULT (it feeds two layers: reference darcy_flow_uno2d.py:108, :127) - where the one-kernel backward
    runs, a deferring consumer may leave its contribution as a tensor of its own (GradJoin.extra) and that kernel adds it while reading."""
    w1, w0 = fc_n1.weight, fc0.weight
    if x.dim() == 4 and _dev_act(x) and not x.requires_grad and w1.dtype == torch.float32 and w0.dtype == torch.float32 and pad_h >= 0 and pad_w >= 0:
        Hp, Wp = x.shape[2] + int(pad_h), x.shape[3] + int(pad_w)
        if _native.lift_ok(x, w1, w0, Hp, Wp):
            return _LiftFn.apply(x, w1, fc_n1.bias, w0, fc0.bias, Hp, Wp, grad_join)
    if grad_join is not None:
        grad_join.accepts_extra = False
    return gelu_channel_mix_pad(channel_mix(x, w1, fc_n1.bias), w0, fc0.bias, pad_h, pad_w)


class _GeluProjectFn(torch.autograd.Function):
    """out[b, p] = bias + sum_c w[c] gelu(pre[b, c, p]) (K11, csrc/pointwise_fused.hip)."""

    @staticmethod
    def forward(ctx, pre, w, bias):
        pre, w = _plain(pre), _plain(w)
        out = _native.gelu_project_forward(pre, w, None if bias is None else _plain(bias))
        ctx.save_for_backward(pre, w)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        pre, w = ctx.saved_tensors
        gpre, gw, gb = _native.gelu_project_backward(pre, w, _plain(gout), need_bias=ctx.has_bias)
        return gpre, gw, gb


def gelu_project(pre: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """channel_mix(F.gelu(pre), weight, bias) for the models' final projection (reference darcy_flow_uno2d.py:128-131:
    `F.gelu(self.fc1(x))` then `self.fc2`, fc2 = Linear(C, 1)): with ONE output channel on a HIP device the GELU and
    the projection are a single streaming pass (no GELU output tensor, no one-row GEMM)."""
    if weight.shape[0] == 1 and _dev_act(pre) and weight.dtype == torch.float32 and pre.shape[1] <= 1024:
        B, C = pre.shape[0], pre.shape[1]
        out = _GeluProjectFn.apply(pre.reshape(B, C, -1), weight.reshape(C), bias)
        return out.view(B, 1, *pre.shape[2:])
    return channel_mix(F.gelu(pre), weight, bias)


class _GeluProject2Fn(torch.autograd.Function):
    """out[b, p] = bias + sum_c w[c] gelu(pre[b, c, p]) + sum_d w[C1 + d] f(s[b, d, p]) (K11's two-source form)."""

    @staticmethod
    def forward(ctx, pre, s, w, bias, act2):
        pre, s, w = _plain(pre), _plain(s), _plain(w)
        out = _native.gelu_project2_forward(pre, s, w, None if bias is None else _plain(bias), act2)
        ctx.save_for_backward(pre, s, w)
        ctx.has_bias, ctx.act2 = bias is not None, act2
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        pre, s, w = ctx.saved_tensors
        gpre, gs, gw, gb = _native.gelu_project2_backward(pre, s, w, _plain(gout), ctx.act2, need_gs=ctx.needs_input_grad[1],
                                                          need_bias=ctx.has_bias)
        return gpre, gs, gw, gb, None


def gelu_project2(pre: torch.Tensor, s: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, act2: bool = False) -> torch.Tensor:
    """channel_mix(torch.cat([F.gelu(pre), f(s)], 1), weight, bias), f = F.gelu if act2 else the identity - the end of the reference's
    UNO_P / UNO_S256 (navier_stokes_uno2d.py:121-125, 320-324: `fc2(torch.cat([F.gelu(fc1(x)), x_fc], 3))`, fc2 = Linear(C1 + C2, 1)).
    With ONE output channel on a HIP device, float32, both sources are read once by a single streaming pass (K11, two-source form):
    no GELU output, no concatenation, no one-row GEMM.  `s` is the pre-activation of the second source when act2."""
    C1, C2 = pre.shape[1], s.shape[1]
    if (weight.shape[0] == 1 and pre.is_cuda and s.is_cuda and pre.dtype == torch.float32 and s.dtype == torch.float32
            and weight.dtype == torch.float32 and C1 >= 1 and C2 >= 1 and C1 + C2 <= 1024):
        B = pre.shape[0]
        out = _GeluProject2Fn.apply(pre.reshape(B, C1, -1), s.reshape(B, C2, -1), weight.reshape(C1 + C2), bias, bool(act2))
        return out.view(B, 1, *pre.shape[2:])
    return channel_mix(torch.cat([F.gelu(pre), F.gelu(s) if act2 else s], 1), weight, bias)


class _GeluPadFn(torch.autograd.Function):
    """zero-pad(gelu(s)) at the end of the last two axes (K12)."""

    @staticmethod
    def forward(ctx, s, Hp, Wp):
        s = _plain(s)
        ctx.save_for_backward(s)
        return _native.gelu_pad(s, Hp, Wp)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (s,) = ctx.saved_tensors
        return _native.gelu_pad_backward(s, _plain(gy)), None, None


def gelu_pad2d(s: torch.Tensor, pad_h: int, pad_w: int) -> torch.Tensor:
    """F.pad(F.gelu(s), [0, pad_w, 0, pad_h]) - the lift's last activation and the domain padding (reference
    darcy_flow_uno2d.py:103-107) in one pass over the tensor on a HIP device."""
    if _dev_act(s) and s.dim() >= 2 and pad_h >= 0 and pad_w >= 0:
        return _GeluPadFn.apply(s, s.shape[-2] + int(pad_h), s.shape[-1] + int(pad_w))
    return F.pad(F.gelu(s), [0, pad_w, 0, pad_h])


class _InstanceNormGeluFn(torch.autograd.Function):
    """[gelu](InstanceNorm(x) * weight + bias) with K13 (csrc/instnorm.hip); saves x and the per-row mean / rstd."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, gelu):
        x = _plain(x)
        w = None if weight is None else _plain(weight)
        b = None if bias is None else _plain(bias)
        y, mean, rstd = _native.instnorm_forward(x, w, b, eps, gelu)
        ctx.save_for_backward(x, w, b, mean, rstd)
        ctx.gelu = gelu
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w, b, mean, rstd = ctx.saved_tensors
        gx, s1, s2 = _native.instnorm_backward(x, _plain(gy), w, b, mean, rstd, ctx.gelu)
        gw = s2.sum(0) if w is not None and ctx.needs_input_grad[1] else None
        gb = s1.sum(0) if b is not None and ctx.needs_input_grad[2] else None
        return gx, gw, gb, None, None


def instance_norm_gelu(x: torch.Tensor, norm: nn.Module, gelu: bool) -> torch.Tensor:
    """`norm(x)` followed, if `gelu`, by F.gelu - for an nn.InstanceNorm{2,3}d without running statistics on a float32
    HIP tensor both run as one kernel; anything else takes the stock modules."""
    if (_dev_act(x) and isinstance(norm, (nn.InstanceNorm1d, nn.InstanceNorm2d, nn.InstanceNorm3d))
            and not norm.track_running_stats and x.dim() >= 3 and x.shape[1] == norm.num_features):
        if x.numel() // max(x.shape[0] * x.shape[1], 1) <= 1:           # torch.nn.functional.instance_norm refuses this too
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {x.size()}")
        return _InstanceNormGeluFn.apply(x, norm.weight, norm.bias, norm.eps, bool(gelu))
    out = norm(x)
    return F.gelu(out) if gelu else out
