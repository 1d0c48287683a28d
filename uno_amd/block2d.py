"""The 2-D spectral convolution and the 2-D operator block (spectral branch + point-wise branch in one buffer) as autograd
Functions on the pruned-DFT, per-mode GEMM, resampling and channel-mix kernels."""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _native
from ._param_grads import _grad_targets, _note_use, _stack_arrived, _stack_grad_slot, _stack_take, _stack_wanted
from .pointwise import _mix2_forward, _mix2_input_grads, _plain, _wgrad_into
from .resample import fused_resample_tables, resample_adjoint, resample_forward, upsample_add_tables


def _half_weights(w1, w2):
    """(Ci, Co, m1, m2, 2) float16 copies of two complex64 weight tensors (storage format of the mixed-precision kernels).  The copy
    of a parameter is kept on it and re-made only when the parameter changed (its version counter moves with every in-place
    update - the optimiser step): repeated forward passes between updates (evaluation, roll-outs) convert nothing."""
    out = []
    # while a HIP graph is being captured the conversion must be PART of the graph: the optimiser updates the master weights between
    # replays (harness.GraphedStep runs it eagerly), and a copy made at warm-up and found in the cache would never be re-made - the
    # replays would read frozen weights.  The captured conversion re-reads the parameter on every replay.
    capturing = w1.is_cuda and torch.cuda.is_current_stream_capturing()
    with torch.no_grad():
        for w in (w1, w2):
            cached = None if capturing else getattr(w, "_uno_half", None)
            if cached is None or cached[0] != w._version or cached[1].device != w.device or cached[2] != w.data_ptr():
                cached = (w._version, torch.view_as_real(w.detach()).half().contiguous(), w.data_ptr())
                if not capturing:
                    try:
                        w._uno_half = cached
                    except (AttributeError, RuntimeError):
                        pass
            out.append(cached[1])
    return out[0], out[1]


def _xt_slot(stack):
    """where a forward pass leaves its truncated input spectrum: the slot of the layer's stack, or None (a fresh tensor)"""
    return None if stack is None else stack.xt


def _xt_dest(stack, B, Ci, m1, m2, device):
    slot = _xt_slot(stack)
    return torch.empty((B, Ci, 2 * m1, m2), dtype=torch.complex64, device=device) if slot is None else slot


def _block_prologue(ctx, iw, x, Ci, w1, w2, cw, cb, Ho, Wo, half_weights):
    """Common start of the block Functions' forward (x: the plain first source, Ci: all input channels, iw: position of w1 among the
    inputs): takes the layer's stack slot (ctx.stack) -> (w1, w2 plain [as half-precision copies], cwm (Co, Ci), cb, same, mix_last)."""
    B, _, H, W = x.shape
    ctx.stack = _stack_take(w1, (B, Ci, 2 * w1.shape[2], w1.shape[3]), x.device, _stack_wanted(ctx, iw, x, half_weights))
    w1, w2 = _plain(w1), _plain(w2)
    if half_weights:                    # complex64 master weights, read through float16 (re, im) copies
        w1, w2 = _half_weights(w1, w2)
    cwm = _plain(cw).reshape(cw.shape[0], Ci)
    cb = None if cb is None else _plain(cb)
    same = (H, W) == (Ho, Wo)
    return w1, w2, cwm, cb, same, same or Ho * Wo < H * W          # the 1x1 convolution runs on whichever side has fewer pixels


def _pointwise_input_grads(g_src, w, C1, gx1, gx2, geom, dgelu_of=None, dgelu_total=False, g_act=None):
    """The point-wise branch's part of the input gradient(s), ACCUMULATED into gx1 (B, C1, H, W) - the columns [:C1] of w (Co, Ci) -
    and gx2 (the other columns); None: not wanted.  g_src (B, Co, P) is the gradient at the 1x1 convolution's output;
    geom = (H, W, Ho, Wo, same, mix_last).  The transposed channel mix accumulates into the destinations - both from one launch
    where _mix2_input_grads' split rule allows - except in a block that resampled BEFORE the mix (mix_last and not same): there
    it writes fresh tensors on the output grid, whose adjoint resampling accumulates (g_act: gx1's, where the caller has mixed it
    already).  dgelu_of / dgelu_total: channel_mix's, on gx1 (accumulating mix only)."""
    H, W, Ho, Wo, same, mix_last = geom
    B = g_src.shape[0]
    direct = same or not mix_last

    def dest(gx):
        return gx.view(B, gx.shape[1], -1) if direct else None

    g1, g2 = g_act, None
    if gx1 is not None and gx2 is not None:
        g1, g2 = _mix2_input_grads(g_src, w, C1, out1=dest(gx1), out2=dest(gx2))
    else:
        if gx1 is not None and g1 is None:
            g1 = _native.channel_mix(g_src, w if C1 == w.shape[1] else w[:, :C1].contiguous(), None, transpose_w=True, out=dest(gx1),
                                     dgelu_of=dgelu_of, dgelu_total=dgelu_total)
        if gx2 is not None:
            g2 = _native.channel_mix(g_src, w[:, C1:].contiguous(), None, transpose_w=True, out=dest(gx2))
    if not direct:
        for g, gx in ((g1, gx1), (g2, gx2)):
            if gx is not None:
                resample_adjoint(g.view(B, gx.shape[1], Ho, Wo), H, W, out=gx)


class _SpectralConv2dFn(torch.autograd.Function):
    """y = irfft2(corner-mix(rfft2(x)));  saves only the truncated input spectrum."""

    @staticmethod
    def forward(ctx, x, w1, w2, Ho, Wo, half_weights=False):
        ctx.params = (w1, w2)
        x = _plain(x)
        ctx.stack = _stack_take(w1, (x.shape[0], x.shape[1], 2 * w1.shape[2], w1.shape[3]), x.device, _stack_wanted(ctx, 1, x, half_weights))
        w1, w2 = _plain(w1), _plain(w2)
        if half_weights:                    # complex64 master weights, read through float16 (re, im) copies
            w1, w2 = _half_weights(w1, w2)
        y, xt = _native.spectral_conv2d_forward(x, w1, w2, int(Ho), int(Wo), xt_out=_xt_slot(ctx.stack))
        ctx.save_for_backward(xt, w1, w2)
        ctx.in_hw = (x.shape[-2], x.shape[-1])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xt, w1, w2 = ctx.saved_tensors
        gx, gw1, gw2, _ = _spectral_backward(_plain(gy), xt, w1, w2, ctx.in_hw[0], ctx.in_hw[1], ctx.needs_input_grad[0],
                                          ctx.needs_input_grad[1] or ctx.needs_input_grad[2],
                                          ctx.needs_input_grad[1] and ctx.needs_input_grad[2], ctx.params, ctx.stack)
        return gx, gw1, gw2, None, None, None


# Up-sampling blocks (and the input gradient of down-sampling blocks): the inverse transform adds the resampled low-resolution result of
# the point-wise branch in the registers it holds its own result in, before the output tile is written (uno_dft2d_inverse_add), instead
# of K3 writing the block output and the accumulating resampling kernel reading and re-writing it.  False: the two-kernel form (A/B).
FUSE_UPSAMPLE_ADD = True


def _fused_addend(t, H, W, m1, m2, adjoint):
    """(t, operand tables) for _native.dft2d_inverse(addend=): t (B, C, Hs, Ws) float32 is the low-resolution tensor whose resampling to
    (H, W) - resample_forward, or resample_adjoint of an (H, W) input grid when `adjoint` - is to be added to the inverse transform of a
    (B, C, 2 m1, m2) spectrum; None where the fused kernel does not apply (the caller runs the two kernels)."""
    if not FUSE_UPSAMPLE_ADD or t.dtype != torch.float32 or t.dim() != 4 or not t.is_cuda:
        return None
    Hs, Ws = t.shape[-2], t.shape[-1]
    if Hs * Ws >= H * W or not _native.dft2d_inverse_add_applies(t.shape[0] * t.shape[1], H, W, m1, m2, Hs, Ws):
        return None
    tabs = upsample_add_tables(Hs, Ws, H, W, str(t.device), bool(adjoint))
    return None if tabs is None else (t, tabs)


# Down-sampling blocks (and the backward pass of up-sampling blocks): the forward transform of the full-resolution tensor also writes its
# resampling to the coarse grid (uno_dft2d_forward_resample), instead of K7 and K1 reading that tensor one after the other.  False: the
# two kernels (A/B).
FUSE_FORWARD_RESAMPLE = True


def _fused_resample(x, m1, m2, Ho, Wo, adjoint):
    """Tables for _native.dft2d_forward_resample of x (B, C, H, W) -> its spectrum and its resampling to (Ho, Wo) - resample_forward, or
    resample_adjoint for an (Ho, Wo) input grid when `adjoint` - or None where the fused kernel does not apply (the caller runs the two)."""
    if not FUSE_FORWARD_RESAMPLE or x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda:
        return None
    H, W = x.shape[-2], x.shape[-1]
    n = x.shape[0] * x.shape[1]
    if Ho * Wo >= H * W or not _native.dft2d_forward_resample_applies(n, H, W, m1, m2, Ho, Wo, 1):
        return None
    tabs = fused_resample_tables(H, W, Ho, Wo, str(x.device), bool(adjoint))
    if tabs is None or not _native.dft2d_forward_resample_applies(n, H, W, m1, m2, Ho, Wo, tabs[1].shape[1]):
        return None
    return tabs


# A tensor that TWO spectral layers transform on the same grid (the Darcy model's c0: conv1 at modes 8, then conv5 at modes 18 as the second
# source of its two-source form): the corner blocks of the smaller truncation are a subset of the larger one's, so the first consumer
# transforms the tensor ONCE at the larger mode counts, straight into the later consumer's spectrum, and copies its own corner blocks out of
# it (uno_spectrum_crop); the later consumer skips its transform of that source (SpectrumShare).  False: each layer transforms for itself (A/B).
SHARE_FORWARD_SPECTRUM = True


class SpectrumShare:
    """One forward transform for a tensor with TWO spectral consumers on the same grid - the forward-pass counterpart of GradJoin, which
    transforms the sum of the two gradient spectra once.

    Made per forward pass for the LATER consumer - a two-source block that takes the tensor as its second source at channel
    `channel_offset` of its `channels` input channels, with `modes` = (m1, m2) - and handed to both: the FIRST consumer
    (`OperatorBlock_2D(x, share=)`) transforms x at the larger modes into a fresh (B, channels, 2 m1, m2) tensor - the later consumer's
    truncated input spectrum - and crops its own spectrum from it; the later one (`forward_cat(share=)`) takes that tensor, transforms
    its first source into the other channels and skips the second.  Each layer keeps its own spectrum for its backward pass.
    Applies to float32 device tensors and complex64 weights, where the later consumer's modes are no fewer than the first one's in both
    axes and fit the grid; anywhere else - and with SHARE_FORWARD_SPECTRUM off - nothing is left here and both layers run as before."""

    def __init__(self, modes, channels, channel_offset):
        self.modes = (int(modes[0]), int(modes[1]))
        self.channels, self.offset = int(channels), int(channel_offset)
        self.spec = self.src = None

    @classmethod
    def for_block(cls, block, channel_offset):
        """for the two-source OperatorBlock_2D `block` whose second source starts at input channel `channel_offset`"""
        return cls((block.conv.modes1, block.conv.modes2), block.conv.in_channels, channel_offset)

    def reset(self):
        self.spec = self.src = None

    def dest(self, x, m1, m2):
        """First consumer, x (B, C, H, W) plain: (spectrum tensor, M1, M2, channel offset) to transform x into, or None"""
        self.reset()
        M1, M2 = self.modes
        H, W = x.shape[-2], x.shape[-1]
        if not SHARE_FORWARD_SPECTRUM or x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda or m1 > M1 or m2 > M2 \
                or M1 > H or M2 > W // 2 + 1 or self.offset < 0 or self.offset + x.shape[1] != self.channels:
            return None
        self.spec = torch.empty((x.shape[0], self.channels, 2 * M1, M2), dtype=torch.complex64, device=x.device)
        self.src = (x, x._version)              # (holding x keeps its storage from being handed to another tensor meanwhile)
        return self.spec, M1, M2, self.offset

    def take(self, x2, C1, Ci, m1, m2):
        """Later consumer: its (B, Ci, 2 m1, m2) spectrum with x2's part at channels [C1, Ci) in place, or None (it transforms x2 itself)"""
        spec, src = self.spec, self.src
        self.reset()
        if spec is None or (m1, m2) != self.modes or Ci != self.channels or C1 != self.offset:
            return None
        x, version = src
        if x2.data_ptr() != x.data_ptr() or x2.shape != x.shape or x2.stride() != x.stride() or x2.dtype != x.dtype or x2._version != version:
            return None
        return spec


def _source_spectrum(x, xt, m1, m2, dest, rs=None, Ho=0, Wo=0):
    """K1 of a block's plain source x (B, Ci, H, W) into xt (B, Ci, 2 m1, m2), rfft2(norm="forward") truncated; rs (_fused_resample's
    tables): the form that also resamples x to (Ho, Wo) -> that tensor.  dest = SpectrumShare.dest(...): x is transformed at the later
    consumer's modes into its spectrum, and xt is the crop of that (rs then belongs to those modes)."""
    H, W = x.shape[-2], x.shape[-1]
    tgt, k1, k2, off = (xt, m1, m2, 0) if dest is None else dest
    res = None
    if rs is None:
        _native.dft2d_forward(x, k1, k2, 1.0 / (H * W), out=tgt, channel_offset=off)
    else:
        _, res = _native.dft2d_forward_resample(x, k1, k2, Ho, Wo, rs, 1.0 / (H * W), out=tgt, channel_offset=off)
    if dest is not None:
        _native.spectrum_crop(tgt, m1, m2, out=xt, channels=x.shape[1], channel_offset=off)
    return res


def _stage_wgrad(stack, gslot, xt, gO, w1, w2, leaves, both_gw, need_gx):
    """Weight gradient of a spectral layer in the stage-by-stage backward pass, from the truncated spectra xt (input) and gO (output
    gradient; in `gslot` of the layer's stack when that took it).  -> (gX or None, gw1, gw2 as autograd should receive them): the
    input-gradient spectrum gX comes from the same launch when the caller needs it and the weights are complex64 (uno_mode_backward)."""
    if gslot is not None:
        return (None, *_stack_arrived(stack, leaves, w1.shape, both_gw))
    tg = _grad_targets(leaves) if both_gw else None
    _note_use(leaves[0])
    out, acc = (tg.dest, tg.accumulate) if tg else (None, False)
    gX = None
    if need_gx and w1.dtype == torch.complex64:
        gX, (gw1, gw2) = _native.mode_backward(xt, gO, [w1, w2], out=out, accumulate=acc)
        gX = gX.view(xt.shape)
    else:
        gw1, gw2 = _native.mode_wgrad(xt, gO, tuple(w1.shape[:4]), 2, out=out, accumulate=acc)
    if tg:
        gw1, gw2 = tg.returned
    return gX, gw1, gw2


def _spectral_backward(gs, xt, w1, w2, H, W, need_gx, need_gw, both_gw, leaves, stack, join=None, addend=None, k1=None):
    """Backward of the spectral branch: -> (gx or None, gw1, gw2 as autograd should receive them, whether the layer's stack took the call).
    leaves = (weights1, weights2) as the caller passed them (in-place gradient targets); stack = the forward pass's _StackSlot
    or None; join: GradJoin whose deferred spectra are merged into this layer's before the inverse transform; addend: _fused_addend(...)
    of the point-wise branch's contribution to gx (float32 only) - the call then runs stage by stage; k1(out): the caller's form of the
    forward transform of gs (the one that also resamples gs), which also makes the call run stage by stage."""
    B, Co = gs.shape[:2]
    Ci, _, m1, m2 = w1.shape[:4]
    gslot = _stack_grad_slot(stack, Co) if (stack is not None and need_gw) else None
    merging = join is not None and need_gx and bool(join.spectra)
    if addend is not None and not need_gx:
        raise RuntimeError("uno_amd: an addend for the input gradient needs the input gradient")
    if gslot is None and not merging and addend is None and k1 is None and not (need_gx and need_gw and w1.dtype == torch.complex64):
        tg = _grad_targets(leaves) if (need_gw and both_gw) else None
        if need_gw:
            _note_use(leaves[0])
        gx, gw1, gw2 = _native.spectral_conv2d_backward(gs, xt, w1, w2, H, W, need_gx=need_gx, need_gw=need_gw,
                                                        gw_out=tg.dest if tg else None, accumulate_gw=bool(tg and tg.accumulate))
        if tg:
            gw1, gw2 = tg.returned
        return gx, gw1, gw2, False
    # stage by stage: the gradient spectrum goes to its slot of the layer's stack and / or the deferred gradient spectra of x's
    # other consumer are added to this layer's before ONE inverse transform
    gO = _native.dft2d_forward(gs, m1, m2, 1.0, True, True, out=gslot) if k1 is None else k1(gslot)
    gX, gw1, gw2 = _stage_wgrad(stack, gslot, xt, gO, w1, w2, leaves, both_gw, need_gx) if need_gw else (None, None, None)
    gx = None
    if need_gx:
        if gX is None:
            gX = _native.mode_mix(gO.view(B, Co, 2, m1 * m2), [w1, w2], 1).view(B, Ci, 2 * m1, m2)
        if merging:
            gX = join.merge(gX, (H, W))
        # addend: the (adjoint-)resampled point-wise contribution joins the transform's result before the tile is written
        gx = _native.dft2d_inverse(gX, H, W, 1.0 / (H * W), False, False, dtype=gs.dtype, addend=addend)
    return gx, gw1, gw2, gslot is not None


class _OperatorBlock2dFn(torch.autograd.Function):
    """s = SpectralConv2d_Uno(x) + pointwise_op_2D(x) in ONE buffer (reference integral_operators.py:270-273:
    `x1_out = self.conv(x, ...); x2_out = self.w(x, ...); x_out = x1_out + x2_out`).

    The spectral branch's inverse DFT writes s; the last kernel of the point-wise branch (the channel mix when the
    block does not up-sample, the resampling otherwise) accumulates into it.  In the backward pass the spectral
    branch writes grad_x and the point-wise branch's last kernel accumulates into that.  Neither sum exists as a
    separate element-wise pass."""

    @staticmethod
    def forward(ctx, x, w1, w2, cw, cb, Ho, Wo, half_weights=False, fuse_gelu=False, join=None, out_join=None, share=None):
        """fuse_gelu (blocks with Non_Lin and no normalisation, reference integral_operators.py:282-283): returns gelu(s); where the
        channel mix is the kernel that completes s (no up-sampling) it writes the activation in the same pass.
        join: GradJoin of x - this block is x's FIRST consumer and returns x's complete gradient (see GradJoin).
        out_join (with fuse_gelu): the GradJoin of this block's OUTPUT; the block leaves its pre-activation sum there, and the
        consumer that completes the output's gradient multiplies it by gelu'(pre) in its last accumulating kernel - this block's
        backward then receives the gradient at the pre-activation sum and runs no GELU-backward pass.
        share: SpectrumShare of x - this block is x's FIRST spectral consumer and transforms x for the later one as well."""
        ctx.leaves = (w1, w2, cw, cb)
        ctx.join = None
        if join is not None:
            join.reset()
            if ctx.needs_input_grad[0]:
                join.owner = True
                ctx.join = join
        x = _plain(x)
        B, Ci, H, W = x.shape
        Co = cw.shape[0]
        w1, w2, cwm, cb, same, mix_last = _block_prologue(ctx, 1, x, Ci, w1, w2, cw, cb, Ho, Wo, half_weights)
        m1, m2 = w1.shape[2], w1.shape[3]
        # x has a later spectral consumer with at least as many modes: K1 runs at ITS modes into its spectrum, xt is cropped from that
        dest = share.dest(x, m1, m2) if (share is not None and not half_weights and w1.dtype == torch.complex64) else None
        k1m = (m1, m2) if dest is None else dest[1:3]
        t = fused = None
        if not mix_last and not half_weights and x.dtype == torch.float32:
            # up-sampling block: the 1x1 convolution first, its result joins the inverse transform's (one pass over the output)
            t = _native.channel_mix(x.view(B, Ci, -1), cwm, cb).view(B, Co, H, W)
            fused = _fused_addend(t, Ho, Wo, m1, m2, False)
        if fused is not None:
            xt = _xt_dest(ctx.stack, B, Ci, m1, m2, x.device)
            _source_spectrum(x, xt, m1, m2, dest)
            O = _native.mode_mix(xt.view(B, Ci, 2, m1 * m2), [w1, w2], 0)
            s = _native.dft2d_inverse(O.view(B, Co, 2 * m1, m2), Ho, Wo, 1.0, True, True, addend=fused)
        elif mix_last and not same and not half_weights and (rs := _fused_resample(x, *k1m, Ho, Wo, False)) is not None:
            # down-sampling block: the forward transform writes the resampled input of the 1x1 convolution from the same read of x
            xt = _xt_dest(ctx.stack, B, Ci, m1, m2, x.device)
            pre_act = _source_spectrum(x, xt, m1, m2, dest, rs, Ho, Wo)
            O = _native.mode_mix(xt.view(B, Ci, 2, m1 * m2), [w1, w2], 0)
            s = _native.dft2d_inverse(O.view(B, Co, 2 * m1, m2), Ho, Wo, 1.0, True, True)
        else:
            pre_act = None
            if mix_last and not same:
                # (where the fused transform above does not apply) the resampling kernel (K7) runs right BEFORE the forward transform (K1)
                # that reads the same tensor: the two walk the images in opposite order (launch alternation), so what K7 read last is
                # still cached when K1 starts
                pre_act = resample_forward(x, Ho, Wo)
            if dest is None:
                s, xt = _native.spectral_conv2d_forward(x, w1, w2, Ho, Wo, xt_out=_xt_slot(ctx.stack))
            else:           # the composite's three stages, with the shared transform as the first
                xt = _xt_dest(ctx.stack, B, Ci, m1, m2, x.device)
                _source_spectrum(x, xt, m1, m2, dest)
                O = _native.mode_mix(xt.view(B, Ci, 2, m1 * m2), [w1, w2], 0)
                s = _native.dft2d_inverse(O.view(B, Co, 2 * m1, m2), Ho, Wo, 1.0, True, True)
        out = s
        if fused is not None:
            act = x
            if fuse_gelu:
                out = F.gelu(s)
        elif mix_last:
            act = x if same else pre_act
            if fuse_gelu:
                _, out = _native.channel_mix2(act.view(B, Ci, -1), None, cwm, cb, out=s.view(B, Co, -1), accumulate=True, y_act=True)
                out = out.view(B, Co, Ho, Wo)
            else:
                _native.channel_mix(act.view(B, Ci, -1), cwm, cb, out=s.view(B, Co, -1))
        else:
            act = x
            if t is None:
                t = _native.channel_mix(x.view(B, Ci, -1), cwm, cb).view(B, Co, H, W)
            resample_forward(t, Ho, Wo, out=s)
            if fuse_gelu:
                out = F.gelu(s)
        ctx.save_for_backward(xt, w1, w2, cwm, act, s if fuse_gelu else None)
        ctx.geom = (H, W, same, mix_last, cb is not None, tuple(cw.shape))
        ctx.out_join = None
        if fuse_gelu and out_join is not None:
            out_join.pre, out_join.dgelu_applied = s, False
            ctx.out_join = out_join
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gs):
        xt, w1, w2, cwm, act, pre = ctx.saved_tensors
        H, W, same, mix_last, has_bias, cw_shape = ctx.geom
        gs = _plain(gs)
        if pre is not None:                 # the block's GELU: gradient at the pre-activation sum
            oj = ctx.out_join
            if oj is not None and oj.dgelu_applied and oj.pre is not None and oj.pre.data_ptr() == pre.data_ptr():
                oj.dgelu_applied = False    # the consumer's last kernel already multiplied by gelu'(pre)
            else:
                gs = torch.ops.aten.gelu_backward(gs, pre)
            if oj is not None:
                oj.pre = None
        B, Co, Ho, Wo = gs.shape
        Ci = cwm.shape[1]
        need_gx = ctx.needs_input_grad[0]
        need_gw = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need_gc = ctx.needs_input_grad[3] or (has_bias and ctx.needs_input_grad[4])
        join = ctx.join
        lw1, lw2, lcw, lcb = ctx.leaves
        # down-sampling block (forward: act = R x; s += Wm act): the point-wise part of gx is the ADJOINT resampling of Wm^T gs, an
        # up-sampling - it joins the spectral part inside the inverse transform (one pass over gx) where the fused kernel applies
        g_act = addend = g_t = k1 = None
        if not mix_last:
            rs = _fused_resample(gs, w1.shape[2], w1.shape[3], H, W, True) if w1.dtype == torch.complex64 else None
            if rs is None:
                g_t = resample_adjoint(gs, H, W).view(B, Co, -1)        # right before the K1 that reads gs as well (see forward)
            else:
                # up-sampling block: the transform of gs writes its adjoint resampling from the same read (g_t: taken from `both` below)
                both = []

                def k1(out):
                    both.extend(_native.dft2d_forward_resample(gs, w1.shape[2], w1.shape[3], H, W, rs, 1.0, True, True, out=out))
                    return both[0]
        if mix_last and not same and need_gx and gs.dtype == torch.float32:
            g_act = _native.channel_mix(gs.view(B, Co, -1), cwm, None, transpose_w=True).view(B, Ci, Ho, Wo)
            addend = _fused_addend(g_act, H, W, w1.shape[2], w1.shape[3], True)
        gx, gw1, gw2, stacked = _spectral_backward(gs, xt, w1, w2, H, W, need_gx, need_gw, ctx.needs_input_grad[1] and ctx.needs_input_grad[2],
                                                   (lw1, lw2), ctx.stack, join, addend, k1)
        if k1 is not None:
            g_t = both[1].view(B, Co, -1)
        pstack = ctx.stack if stacked else None         # the 1x1 convolution's weight gradient follows the spectral layer's stack
        gcw = gcb = None
        # x is the activation of a fused-GELU block (join.pre): the gradient this block returns must be multiplied by gelu'(pre).
        # The LAST kernel that accumulates into gx does it - a deferred closure if any is pending, else this block's own
        # transposed channel mix where that comes last; otherwise a separate pass at the end
        xpre = join.pre if (join is not None and need_gx) else None
        own_last = xpre is not None and not join.pending
        dg_view = xpre.view(B, Ci, -1) if own_last else None
        # forward: act = R x; s += Wm act + b (mix_last), or t = Wm x + b; s += R t.  Only the mix that accumulates into gx itself
        # (no resampling after it) can apply gelu'
        direct = same or not mix_last
        g_src = gs.view(B, Co, -1) if mix_last else g_t
        if need_gx and (direct or addend is None):
            _pointwise_input_grads(g_src, cwm, Ci, gx, None, (H, W, Ho, Wo, same, mix_last), dgelu_of=dg_view if direct else None,
                                   dgelu_total=own_last and direct, g_act=g_act)
        dg_done = own_last and direct
        if need_gc:
            gcw, gcb = _wgrad_into((lcw, lcb), g_src, act.view(B, Ci, -1), None, ctx.needs_input_grad[3],
                                   has_bias and ctx.needs_input_grad[4], stack=pstack)
            gcw = None if gcw is None else gcw.view(cw_shape)
        if join is not None:
            if need_gx:
                # the point-wise contributions of x's other consumer accumulate into this buffer (the last one applies gelu'(pre))
                dg_done = join.apply(gx, xpre if not dg_done else None) or dg_done
                if xpre is not None:
                    if not dg_done:
                        gx = torch.ops.aten.gelu_backward(gx, xpre)
                    join.dgelu_applied = True
            join.reset()
        return gx, gw1, gw2, gcw, gcb, None, None, None, None, None, None, None


class _OperatorBlock2dCatFn(torch.autograd.Function):
    """_OperatorBlock2dFn for an input that the reference builds with torch.cat([x1, x2], dim=1) (skip connections,
    reference darcy_flow_uno2d.py:117-125), without building it: K1 transforms the two sources into the channel ranges
    of one truncated spectrum, the point-wise branch mixes the two sources with the two column blocks of the 1x1
    weight, and the backward pass returns the two input gradients as separate contiguous tensors (no strided slices
    of a joint gradient to copy or accumulate)."""

    @staticmethod
    def forward(ctx, x1, x2, w1, w2, cw, cb, Ho, Wo, half_weights=False, defer=None, share=None):
        ctx.leaves = (w1, w2, cw, cb)
        ctx.defer = defer if (defer is not None and defer.owner and ctx.needs_input_grad[1]) else None
        x1, x2 = _plain(x1), _plain(x2)
        B, C1, H, W = x1.shape
        C2 = x2.shape[1]
        Ci, Co, m1, m2 = w1.shape
        w1, w2, cwm, cb, same, mix_last = _block_prologue(ctx, 2, x1, Ci, w1, w2, cw, cb, Ho, Wo, half_weights)
        # spectral branch, stage by stage (the composite entry point takes a single source)
        # x2's first consumer may have left this layer's spectrum with x2's channels in place (SpectrumShare): x2 is not transformed again
        shared = share.take(x2, C1, Ci, m1, m2) if (share is not None and not half_weights and x2.dtype == torch.float32
                                                    and w1.dtype == torch.complex64) else None
        xt = shared if (shared is not None and ctx.stack is None) else _xt_dest(ctx.stack, B, Ci, m1, m2, x1.device)
        _native.dft2d_forward(x1, m1, m2, 1.0 / (H * W), out=xt, channel_offset=0)
        if shared is None:
            _native.dft2d_forward(x2, m1, m2, 1.0 / (H * W), out=xt, channel_offset=C1)
        elif shared is not xt:      # the layer's stack keeps its uses' spectra in one tensor: a copy of the truncated spectrum into the slot
            xt[:, C1:].copy_(shared[:, C1:])
        O = _native.mode_mix(xt.view(B, Ci, 2, m1 * m2), [w1, w2], 0)
        t = fused = None
        if not mix_last and not half_weights and x1.dtype == torch.float32:
            # up-sampling block: the 1x1 convolution first, its result joins the inverse transform's (one pass over the output)
            t = _mix2_forward(x1.view(B, C1, -1), x2.view(B, C2, -1), cwm, cb).view(B, Co, H, W)
            fused = _fused_addend(t, Ho, Wo, m1, m2, False)
        s = _native.dft2d_inverse(O.view(B, Co, 2 * m1, m2), Ho, Wo, 1.0, True, True, dtype=x1.dtype, addend=fused)
        # point-wise branch accumulates into s
        if fused is not None:
            a1, a2 = x1, x2
        elif mix_last:
            a1 = x1 if same else resample_forward(x1, Ho, Wo)
            a2 = x2 if same else resample_forward(x2, Ho, Wo)
            _mix2_forward(a1.view(B, C1, -1), a2.view(B, C2, -1), cwm, cb, out=s.view(B, Co, -1), accumulate=True)
        else:
            a1, a2 = x1, x2
            if t is None:
                t = _mix2_forward(x1.view(B, C1, -1), x2.view(B, C2, -1), cwm, cb).view(B, Co, H, W)
            resample_forward(t, Ho, Wo, out=s)
        ctx.save_for_backward(xt, w1, w2, cwm, a1, a2)
        ctx.geom = (H, W, same, mix_last, cb is not None, tuple(cw.shape))
        return s

    @staticmethod
    @once_differentiable
    def backward(ctx, gs):
        xt, w1, w2, cwm, a1, a2 = ctx.saved_tensors
        H, W, same, mix_last, has_bias, cw_shape = ctx.geom
        gs = _plain(gs)
        B, Co, Ho, Wo = gs.shape
        Ci, _, m1, m2 = w1.shape[:4]
        C1, C2 = a1.shape[1], a2.shape[1]
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_gw = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        need_gc = ctx.needs_input_grad[4] or (has_bias and ctx.needs_input_grad[5])
        lw1, lw2, lcw, lcb = ctx.leaves
        both_gw = ctx.needs_input_grad[2] and ctx.needs_input_grad[3]
        gslot = _stack_grad_slot(ctx.stack, Co) if (ctx.stack is not None and need_gw) else None
        # gradient at the 1x1 convolution's output and the gradient spectrum: from one read of gs where the fused transform applies, else K7
        # right before the K1 that reads gs as well (_OperatorBlock2dFn.forward)
        rs = _fused_resample(gs, m1, m2, H, W, True) if (not mix_last and w1.dtype == torch.complex64) else None
        if rs is not None:
            gO, g_src = _native.dft2d_forward_resample(gs, m1, m2, H, W, rs, 1.0, True, True, out=gslot)      # c (.) keep (.) DFT_trunc(gs), R^T gs
            g_src = g_src.view(B, Co, -1)
        else:
            g_src = gs.view(B, Co, -1) if mix_last else resample_adjoint(gs, H, W).view(B, Co, -1)
            gO = _native.dft2d_forward(gs, m1, m2, 1.0, True, True, out=gslot)             # c (.) keep (.) DFT_trunc(gs)
        gXp, gw1, gw2 = _stage_wgrad(ctx.stack, gslot, xt, gO, w1, w2, (lw1, lw2), both_gw, need1 or need2) if need_gw else (None, None, None)
        gx1 = gx2 = None
        defer = ctx.defer if (need2 and ctx.defer is not None and ctx.defer.owner) else None    # owner's backward still to come
        if need1 or need2:
            gX = gXp if gXp is not None else _native.mode_mix(gO.view(B, Co, 2, m1 * m2), [w1, w2], 1).view(B, Ci, 2 * m1, m2)
            if need1:
                gx1 = _native.dft2d_inverse(gX, H, W, 1.0 / (H * W), False, False, channels=C1, channel_offset=0, dtype=gs.dtype)
            if defer is not None:
                # x2's gradient is completed by x2's first consumer (GradJoin): leave the spectrum, transform nothing
                defer.spectra.append((gX[:, C1:].contiguous(), (H, W)))
            elif need2:
                gx2 = _native.dft2d_inverse(gX, H, W, 1.0 / (H * W), False, False, channels=C2, channel_offset=C1, dtype=gs.dtype)
        gcw = gcb = None
        geom = (H, W, Ho, Wo, same, mix_last)
        if defer is not None:
            # point-wise part of x2's gradient: accumulated into the joined buffer later (where its mix accumulates itself it can
            # apply the owner's gelu'); x1's part now
            cw2 = cwm[:, C1:].contiguous()

            def x2_part(out, dg=None):
                _pointwise_input_grads(g_src, cw2, C2, out, None, geom, dgelu_of=None if dg is None else dg.view(B, C2, -1),
                                       dgelu_total=dg is not None)
            defer.pending.append((x2_part, same or not mix_last))
            _pointwise_input_grads(g_src, cwm, C1, gx1, None, geom)
        else:
            _pointwise_input_grads(g_src, cwm, C1, gx1, gx2, geom)
        if need_gc:
            gcw, gcb = _wgrad_into((lcw, lcb), g_src, a1.view(B, C1, -1), a2.view(B, C2, -1), ctx.needs_input_grad[4],
                                   has_bias and ctx.needs_input_grad[5])
            gcw = None if gcw is None else gcw.view(cw_shape)
        if ctx.defer is not None and gx2 is not None:       # the owner's backward came first after all
            gx2 = ctx.defer.late(gx2)
        return gx1, gx2, gw1, gw2, gcw, gcb, None, None, None, None, None


def spectral_conv2d(x, weights1, weights2, dim1, dim2):
    """Functional form of SpectralConv2d_Uno.forward (reference integral_operators.py:181-207)."""
    return _SpectralConv2dFn.apply(x, weights1, weights2, dim1, dim2)


def spectral_conv2d_mixed(x, weights1, weights2, dim1, dim2):
    """Mixed-precision form of the 2-D Fourier integral operator (BASELINE.json config 5: bf16 activations, half-precision
    weight storage, f32 accumulation).  Opt-in: the reference - and SpectralConv2d_Uno.forward here - raise on bf16 input
    (integral_operators.py:187).

    x (B, Ci, H, W) bfloat16 -> (B, Co, dim1, dim2) bfloat16; gradients: gx bfloat16, weights in their own dtype.
    weights1/2: complex64 (Ci, Co, m1, m2), or their half-precision storage (Ci, Co, m1, m2, 2) float16 (re, im), which the
    per-mode GEMM reads as it is (widened in registers; 33 MB at the C5 size).  The pruned DFT kernels read / write the bf16
    tensors directly; the truncated spectrum, the per-mode GEMM and every accumulation are f32 / c64, so the result equals the
    f32 operator applied to the widened inputs, rounded once (to nearest even) on the way out - tests/test_hip_mixed.py."""
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"spectral_conv2d_mixed: input must be bfloat16 (got {x.dtype})")
    for w in (weights1, weights2):
        if w.dtype == torch.float16 and w.shape[-1] != 2:
            raise RuntimeError("spectral_conv2d_mixed: half-precision weights are stored as (..., 2) = (re, im)")
    if weights1.dtype == torch.float16:
        return _SpectralConv2dHalfFn.apply(x, weights1, weights2, dim1, dim2)
    return _SpectralConv2dFn.apply(x, weights1, weights2, dim1, dim2)


class _SpectralConv2dHalfFn(torch.autograd.Function):
    """spectral_conv2d_mixed with the weights GIVEN in half-precision (re, im) storage: K2 reads them as they are (no widened
    copy); their gradients are accumulated in complex64 and returned rounded once to the storage format."""

    @staticmethod
    def forward(ctx, x, w1h, w2h, Ho, Wo):
        x, w1h, w2h = _plain(x), _plain(w1h), _plain(w2h)
        y, xt = _native.spectral_conv2d_forward(x, w1h, w2h, int(Ho), int(Wo))
        ctx.save_for_backward(xt, w1h, w2h)
        ctx.in_hw = (x.shape[-2], x.shape[-1])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xt, w1h, w2h = ctx.saved_tensors
        need_gx = ctx.needs_input_grad[0]
        need_gw = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gx, gw1, gw2 = _native.spectral_conv2d_backward(_plain(gy), xt, w1h, w2h, ctx.in_hw[0], ctx.in_hw[1],
                                                        need_gx=need_gx, need_gw=need_gw)
        if need_gw:
            gw1, gw2 = torch.view_as_real(gw1).half(), torch.view_as_real(gw2).half()
        return gx, gw1, gw2, None, None
