"""Training step of the Darcy workload (reference train_darcy.py:47-56) with data parallelism over
one process per GPU.

Every sample is independent through the network (batch is a free index of the mode contraction,
InstanceNorm is per sample, the loss is a per-sample sum), so the minibatch is sharded across ranks
and the only exchange is ONE gradient all-reduce per step (RCCL over xGMI on MI355X, gloo in the CPU
tests).  All gradients live in a single flat float32 buffer (complex grads as interleaved re/im), so
that exchange is one large collective on a few hundred MB instead of a per-parameter stream:
xGMI all-reduce is per-link bandwidth bound, large messages are what it wants.  The reference loss
is a SUM over the batch, hence gradients are SUMMED over ranks: the update equals the single-process
update on the concatenated global batch."""
from __future__ import annotations

import time

import torch
import torch.distributed as dist
from torch.autograd.function import once_differentiable

from .losses import NATIVE_STEP_ERRORS_MAX_T, RolloutErrors, StepErrors, _step_errors_stock, lp_loss_rel_sum, step_errors, step_losses
from .optim import ComplexAdam


def synthetic_darcy_batch(batch, S, seed, device, dtype=torch.float32):
    """Synthetic Darcy pair of the benchmark shape: coefficient field a ~ U[0,1) (B,S,S,1) and target
    u ~ U[0,1) (B,S,S); generated on the host from a seeded generator."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.rand(batch, S, S, 1, generator=g, dtype=dtype)
    u = torch.rand(batch, S, S, generator=g, dtype=dtype)
    return a.to(device), u.to(device)


class FlatGradients:
    """Backs every parameter's .grad with a view into one flat float32 buffer, and sums that buffer across the
    data-parallel group in a few large buckets while the backward pass is still running.

    Buckets are contiguous slices of the flat buffer (~`bucket_mb` each), numbered in the order the backward pass
    completes them (last-registered parameters first).  A post-accumulate hook on every parameter counts its
    bucket down; a complete bucket is all-reduced asynchronously (RCCL runs it on its own stream, overlapping the
    rest of the backward), always in bucket order so that every rank issues the same sequence of collectives.
    finish() issues whatever is left (parameters that took no part in this backward) and waits."""

    def __init__(self, params, bucket_mb: float = 32.0, comm_dtype=None):
        """comm_dtype: None - buckets travel as float32 (the default: bit-equal to a single process on the global batch up to summation
        order); torch.bfloat16 - a bucket is rounded to bfloat16 for the exchange and widened into the float32 buffer afterwards: half
        the bytes on the links (the 3.8 GB gradient of Uno3D_T20 at width 32 is link-bound at 8 ranks), gradient
        entries good to ~2^-8 relative.  The optimiser state and the update stay float32."""
        self.comm_dtype = comm_dtype
        self.params = [p for p in params if p.requires_grad]
        sizes = [p.numel() * (2 if p.is_complex() else 1) for p in self.params]
        dev = self.params[0].device
        n_cplx = sum(1 for p in self.params if p.is_complex())
        self.flat = torch.zeros(sum(sizes) + n_cplx, dtype=torch.float32, device=dev)      # + room for the alignment gaps
        offsets = []
        self.views = []
        off = 0
        for p, n in zip(self.params, sizes):
            if p.is_complex() and off % 2:
                off += 1                    # view_as_complex needs an even element offset (odd count of real entries in front)
            seg = self.flat[off:off + n]
            if p.is_complex():
                view = torch.view_as_complex(seg.view(*p.shape, 2))
            else:
                assert p.dtype == torch.float32
                view = seg.view(p.shape)
            p.grad = None
            p._uno_grad_buffer = view       # where the weight-gradient kernels write this parameter's gradient (_param_grads._grad_targets)
            self.views.append(view)
            offsets.append(off)
            off += n
        # buckets: walk the parameters backwards, close a bucket once it holds bucket_mb
        limit = int(bucket_mb * (1 << 20) / 4)
        self.buckets = []               # (start, end) element ranges, in issue order
        self._bucket_of = {}
        end = off
        count = 0
        members = []
        for i in range(len(self.params) - 1, -1, -1):
            members.append(i)
            count += sizes[i]
            if count >= limit or i == 0:
                for j in members:
                    self._bucket_of[j] = len(self.buckets)
                self.buckets.append((offsets[i], end))
                end = offsets[i]
                count = 0
                members = []
        self._bucket_params = [sum(1 for b in self._bucket_of.values() if b == k) for k in range(len(self.buckets))]
        self._pending = list(self._bucket_params)
        self._next = 0                  # next bucket to issue
        self._works = []
        self._group = None
        self._armed = False
        self._hooks = []
        self.trace = None               # set to [] to record, per issued bucket, the host time since arm() (bench.py `comm`)
        self._t_arm = 0.0

    def zero_(self):
        """Start of a step: every .grad is released (None).  `.flat` is NOT cleared here: it is valid only after finish() / collect()
        of the pass that follows (which also zero the segments of parameters that received no gradient).  The backward pass then writes each gradient ONCE into its view of the
        flat buffer - the library's weight-gradient kernels write there directly and autograd adopts an alias of the view as
        .grad (no zero fill, no `.grad +=` pass); gradients that arrive as ordinary tensors (a few small ones: normalisation
        affines, the final projection) are copied in by collect()."""
        for p in self.params:
            p.grad = None

    def collect(self, only=None):
        """Make every existing .grad live in the flat buffer: a gradient that autograd produced outside it is copied into its view
        and .grad re-pointed (called per parameter by the bucket hooks, and for all parameters at the end of a backward pass)."""
        pairs = zip(self.params, self.views) if only is None else ((self.params[only], self.views[only]),)
        for p, view in pairs:
            g = p.grad
            if g is None:
                if only is None:            # end of a pass: a parameter that took no part in it contributes ZERO to the sum over ranks
                    view.zero_()            # (zero_() does not clear the buffer, so its segment still holds an earlier step's values)
            elif g.data_ptr() != view.data_ptr():
                view.copy_(g)
                p.grad = view.view(view.shape)

    # ------------------------------------------------------------------ overlapped all-reduce
    def arm(self, group=None, force=False):
        """Call before backward(): enables the bucket hooks for this backward if the group has more than one rank."""
        if self._works:                 # the previous pass neither finished nor aborted (it raised and the caller went on)
            self.abort()
        self._armed = bool(dist.is_available() and dist.is_initialized() and (force or dist.get_world_size(group) > 1))
        if not self._armed:
            return
        self._group = group
        self._t_arm = time.perf_counter()
        self._pending = list(self._bucket_params)
        self._next = 0
        self._works = []
        if not self._hooks:
            for i, p in enumerate(self.params):
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(i)))

    def _make_hook(self, i):
        k = self._bucket_of[i]

        def hook(_param):
            if self._armed:
                self.collect(i)             # the gradient must be in the flat buffer before its bucket is sent
                self._pending[k] -= 1
                self._issue_ready()
        return hook

    def _issue(self, k):
        a, b = self.buckets[k]
        if self.trace is not None:
            self.trace.append(time.perf_counter() - self._t_arm)
        if self.comm_dtype is None:
            self._works.append((dist.all_reduce(self.flat[a:b], op=dist.ReduceOp.SUM, group=self._group, async_op=True), None, a, b))
        else:
            low = self.flat[a:b].to(self.comm_dtype)        # rounded copy (stream-ordered behind the kernels that wrote the bucket)
            self._works.append((dist.all_reduce(low, op=dist.ReduceOp.SUM, group=self._group, async_op=True), low, a, b))

    def _issue_ready(self):
        while self._next < len(self.buckets) and self._pending[self._next] <= 0:
            self._issue(self._next)
            self._next += 1

    def finish(self):
        """Call after backward(): issues the buckets that are still open and waits for all of them."""
        self.collect()
        if not self._armed:
            return
        while self._next < len(self.buckets):
            self._issue(self._next)
            self._next += 1
        for w, low, a, b in self._works:
            w.wait()
            if low is not None:
                self.flat[a:b].copy_(low)                   # widened sum back into the float32 buffer the optimiser reads
        self._works = []
        self._armed = False

    def abort(self):
        """A backward pass that raised (out of memory, a user interrupt): wait for the collectives already issued - every rank issued the
        same ones up to its failure or will hang with us, which is the caller's to handle - and return to the un-armed state, so that the
        next arm() starts from bucket 0 with full counters.  The flat buffer holds a partial gradient: zero_() + a new pass overwrite it."""
        for w, low, a, b in self._works:
            try:
                w.wait()
            except Exception:
                pass
        self._works = []
        self._armed = False
        self._next = 0
        self._pending = list(self._bucket_params)

    def all_reduce_sum(self, group=None, force=False):
        """One blocking SUM over the whole buffer (no overlap)."""
        self.collect()
        if dist.is_available() and dist.is_initialized() and (force or dist.get_world_size(group) > 1):
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)


def ns2d_rollout_loss(model, xx, yy, T_f, step=1, native=False, loss=None):
    """Autoregressive loss of the NS-2D training step (reference ns_train_2d.py:46-62): the model predicts
    `step` frames from the last T_in, the prediction is appended to the input window, the per-step relative
    L2 losses are summed; ONE backward runs through the whole unrolled chain.

    native=True (opt-in): the same loss and gradients without a window tensor - the first lift reads the frames where they lie and
    the loss comes from the roll-out's own sums (_rollout_loss_native).  It needs step == 1, a model with fc / body_cf / get_grid,
    T_in + features <= 32, a first lift of at most 64 channels and T_f <= 256, and raises where that does not hold.

    loss: a loss object called on the (B, S, S, step) prediction and target of every step instead of the relative L2 (an HsLoss of layout
    "bhwt", summing over the batch), through the window-by-window forms; the native roll-out's step loss is fused relative L2, so
    loss together with native=True raises."""
    if native and loss is not None:
        raise ValueError("ns2d_rollout_loss: loss= and native=True conflict - the native training roll-out computes its own fused relative-L2 "
                         "step loss; pass native=False to train on another loss")
    if native:
        return _rollout_loss_native(model, xx, yy, T_f, step)
    B = yy.shape[0]
    step_loss = (lambda im, y: lp_loss_rel_sum(im.reshape(B, -1), y.reshape(B, -1))) if loss is None else loss
    loss = 0
    if step == 1 and hasattr(model, "forward_cf") and hasattr(model, "get_grid"):
        # the window lives channels-first next to the model's positional features: per step ONE concatenation
        # [frames 1.., new frame, features] instead of the channels-last window, its layout change and the feature concatenation
        T_in = xx.shape[-1]
        z = torch.cat((xx.permute(0, 3, 1, 2), model.get_grid(xx.shape, xx.device).permute(0, 3, 1, 2)), dim=1)
        for t in range(T_f):
            im = model.forward_cf(z)                                # (B, 1, S, S)
            loss = loss + step_loss(im.permute(0, 2, 3, 1), yy[..., t:t + 1])
            if t + 1 < T_f:
                z = torch.cat((z[:, 1:T_in], im, z[:, T_in:]), dim=1)
        return loss
    for t in range(0, T_f, step):
        im = model(xx)
        loss = loss + step_loss(im, yy[..., t:t + step])
        xx = torch.cat((xx[..., step:], im), dim=-1)
    return loss


# Limits of the native training roll-out (uno_rollout_lift / uno_rollout_lift_backward): input channels of the first lift, its width, steps
NATIVE_ROLLOUT_MAX_C, NATIVE_ROLLOUT_MAX_CM, NATIVE_ROLLOUT_MAX_T = 32, 64, 256


class _RolloutTrain:
    """State of ONE native training roll-out (reference ns_train_2d.py:46-68), shared by the three autograd Functions below.

    The window of step t is T_in consecutive frames of the sequence "the T_in given frames, then the predictions":
        given (B, T_in, S, S)        channels-first copy of the input frames
        pred, target, gpred (B, T, S, S)   time-major; pred[:, t] is recorded as step t's output arrives
        feat (F, S, S)               the model's positional features, one table for all batch entries (get_grid expands it)
    so no window is ever built: the first lift reads the frames where they lie (K19), its backward adds each predicted frame's
    gradient into gpred (K19-B) and leaves its weight sums as blocks in `parts` - one channel_wgrad_finish per training step.  The loss
    is totals[0] of rollout_finish over the chunk sums that recording the frames left in `ws`.

    Every kernel call has a stock-op restatement for CPU tensors and other dtypes (as channel_mix has): the same three Functions then
    run without a device, `parts` holding one summed (Cm, C + 1) block per step."""

    def __init__(self, model, xx, yy, T_f):
        B, S1, S2, T_in = xx.shape
        w = model.fc.weight
        grid = model.get_grid(xx.shape, xx.device)                                  # (B, S, S, F), the same table for every b
        self.B, self.T_in, self.F, self.T, self.P, self.Cm = B, T_in, grid.shape[-1], T_f, S1 * S2, w.shape[0]
        self.C = T_in + self.F
        self.native = xx.is_cuda and xx.dtype == torch.float32 and w.dtype == torch.float32
        self.given = xx.permute(0, 3, 1, 2).contiguous()
        self.feat = grid[0].permute(2, 0, 1).to(xx.dtype).contiguous() if self.F else None
        self.target = yy[..., :T_f].permute(0, 3, 1, 2).contiguous()
        self.pred = torch.empty_like(self.target)
        self.gpred = self.gL = self.sums = None
        if self.native:
            from .. import _native
            self.ws = _native.rollout_ws(B, self.P, T_f, xx.device)
            self.record = _native.rollout_record(B, T_f, xx.device)
            self.parts = _native.rollout_lift_bwd_ws(B, T_in, self.F, self.Cm, self.P, T_f, xx.device)
        else:
            self.parts = xx.new_zeros((T_f, self.Cm, self.C + 1))

    def _window(self, t):
        """stock: the T_in frames of window t, (B, T_in, S, S)"""
        lo = max(0, self.T_in - t)                              # that many of them are given frames
        return torch.cat((self.given[:, self.T_in - lo:], self.pred[:, t - (self.T_in - lo):t]), dim=1) if lo < self.T_in else self.given

    def lift(self, w, bias, t):
        """h_t = fc(window t, features), (B, Cm, S, S)"""
        if self.native:
            from .. import _native
            return _native.rollout_lift(self.given, self.pred, self.feat, w, bias, t)
        h = torch.einsum("mk,bkxy->bmxy", w[:, :self.T_in], self._window(t)) + bias.view(1, -1, 1, 1)
        if self.F:
            h = h + torch.einsum("mf,fxy->mxy", w[:, self.T_in:], self.feat)
        return h

    def record_frame(self, im, t):
        """pred[:, t] = the model's output of step t (and, on the device, the step's chunk sums of the loss)"""
        if self.native:
            from .. import _native
            _native.rollout_advance(self.given, im.contiguous(), self.target, self.pred, self.ws, self.T_in, t, False)
        else:
            self.pred[:, t] = im.reshape(self.B, *self.pred.shape[2:])

    def finish(self):
        """-> the loss sum_t sum_b ||pred - target|| / ||target||; keeps the sums (B, T, 2) the backward pass needs"""
        if self.native:
            from .. import _native
            self.sums, _, totals = _native.rollout_finish(self.ws, self.B, self.P, self.T, record=self.record)
            return totals[0].clone()
        d = self.pred - self.target
        self.sums = torch.stack(((d * d).sum((2, 3)), (self.target * self.target).sum((2, 3))), dim=-1)
        return (self.sums[..., 0].sqrt() / self.sums[..., 1].sqrt()).sum()

    def _loss_term(self, q):
        """stock: gL d / (||d|| ||y||) of step q, 0 where ||d|| = 0 (the backward of torch.linalg.vector_norm)"""
        num, den = self.sums[:, q, 0], self.sums[:, q, 1]
        scale = torch.where(num == 0, torch.zeros_like(num), self.gL / (num.sqrt() * den.sqrt()))
        return scale.view(-1, 1, 1) * (self.pred[:, q] - self.target[:, q])

    def seed(self, gL):
        """Start of the backward pass: keep gL, clear gpred -> the gradient of the LAST frame (its loss term: no lift follows it)"""
        self.gL = gL.detach().reshape(1).to(self.pred.dtype).clone()
        self.gpred = torch.zeros_like(self.pred)
        if self.native:
            from .. import _native
            gframe = torch.empty((self.B, 1, *self.pred.shape[2:]), dtype=self.pred.dtype, device=self.pred.device)
            _native.rollout_loss_seed(self.pred, self.target, self.sums, self.gL, gframe)
            return gframe
        return self._loss_term(self.T - 1).unsqueeze(1)

    def lift_backward(self, gh, w, t):
        """Backward of lift(t): window t's weight sums into `parts`, the older predicted frames' gradients into gpred -> the COMPLETE
        gradient of step t - 1's output (None for t = 0).  Must be called in DESCENDING t after seed()."""
        if self.gpred is None:
            raise RuntimeError("ns2d_rollout_loss(native=True): the roll-out's backward pass must start at its loss")
        if self.native:
            from .. import _native
            gframe = torch.empty((self.B, 1, *self.pred.shape[2:]), dtype=self.pred.dtype, device=self.pred.device)
            _native.rollout_lift_backward(gh.contiguous(), self.given, self.pred, self.target, self.feat, w, self.sums, self.gL, self.gpred,
                                          gframe, self.parts, t)
            return gframe if t >= 1 else None
        T_in = self.T_in
        self.parts[t, :, :T_in] = torch.einsum("bmxy,bkxy->mk", gh, self._window(t))
        if self.F:
            self.parts[t, :, T_in:self.C] = torch.einsum("bmxy,fxy->mf", gh, self.feat)
        self.parts[t, :, self.C] = gh.sum((0, 2, 3))
        if t == 0:
            return None
        gx = torch.einsum("mk,bmxy->bkxy", w[:, :T_in], gh)
        for k in range(max(0, T_in - t), T_in - 1):
            self.gpred[:, t + k - T_in] += gx[:, k]
        return ((self.gpred[:, t - 1] + gx[:, T_in - 1]) + self._loss_term(t - 1)).unsqueeze(1)

    def wgrad_finish(self):
        """-> gw (Cm, C), gb (Cm): the sum of every window's blocks, ONE launch on the device"""
        if self.native:
            from .. import _native
            return _native.channel_wgrad_finish(self.parts, self.C, self.Cm, True)
        total = self.parts.sum(0)
        return total[:, :self.C].contiguous(), total[:, self.C].contiguous()


# The chain h_t -> body -> im_t -> h_{t+1} makes autograd run the three Functions in REVERSE step order: _RolloutLastFn first, then
# _RolloutStepFn of step T - 2 ... 0, then _RolloutFirstFn (h_0 has no other producer, and every later node hangs on it through im_0).
# That order is what the accumulation relies on: when step t's node runs, every later window has added its share to gpred[:, t].
class _RolloutFirstFn(torch.autograd.Function):
    """(w, b) -> h_0.  backward: window 0's weight sums, then the ONE finish over all windows' blocks -> gw, gb."""

    @staticmethod
    def forward(ctx, w, bias, state):
        ctx.state = state
        ctx.save_for_backward(w)
        return state.lift(w, bias, 0)

    @staticmethod
    @once_differentiable
    def backward(ctx, gh):
        (w,) = ctx.saved_tensors
        ctx.state.lift_backward(gh, w, 0)
        gw, gb = ctx.state.wgrad_finish()
        return gw, gb, None


class _RolloutStepFn(torch.autograd.Function):
    """(im_t, w, b) -> h_{t+1}: record the frame, lift the next window.  backward: K19-B -> the gradient of im_t; None for w / b, whose
    blocks wait in the workspace for _RolloutFirstFn."""

    @staticmethod
    def forward(ctx, im, w, bias, state, t):
        ctx.state, ctx.t = state, t
        ctx.save_for_backward(w)
        state.record_frame(im, t)
        return state.lift(w, bias, t + 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, gh):
        (w,) = ctx.saved_tensors
        return ctx.state.lift_backward(gh, w, ctx.t + 1), None, None, None, None


class _RolloutLastFn(torch.autograd.Function):
    """im_{T-1} -> loss: record the frame, finish the sums.  backward: store gL, clear gpred -> the last frame's loss gradient."""

    @staticmethod
    def forward(ctx, im, state):
        ctx.state = state
        state.record_frame(im, state.T - 1)
        return state.finish()

    @staticmethod
    @once_differentiable
    def backward(ctx, gL):
        return ctx.state.seed(gL), None


def _rollout_loss_native(model, xx, yy, T_f, step):
    """ns2d_rollout_loss(native=True): no silent fallback - whatever the native path does not cover raises."""
    limits = (f"step == 1, a model with fc / body_cf / get_grid, (B, S, S, T) tensors of one dtype and device, T_in + features <= "
              f"{NATIVE_ROLLOUT_MAX_C}, a first lift of at most {NATIVE_ROLLOUT_MAX_CM} channels, 1 <= T_f <= {NATIVE_ROLLOUT_MAX_T} within yy")
    ok = (step == 1 and all(hasattr(model, a) for a in ("fc", "body_cf", "get_grid")) and xx.dim() == 4 and yy.dim() == 4
          and xx.dtype == yy.dtype and xx.device == yy.device and xx.dtype.is_floating_point and xx.numel() > 0
          and 1 <= T_f <= min(NATIVE_ROLLOUT_MAX_T, yy.shape[-1]) and getattr(model.fc, "bias", None) is not None)
    if ok:
        F = model.get_grid(xx.shape, xx.device).shape[-1]
        w = model.fc.weight
        ok = w.dim() == 2 and w.shape[1] == xx.shape[-1] + F and w.shape[1] <= NATIVE_ROLLOUT_MAX_C and w.shape[0] <= NATIVE_ROLLOUT_MAX_CM \
            and w.dtype == xx.dtype and w.device == xx.device
    if not ok:
        raise RuntimeError(f"ns2d_rollout_loss(native=True) needs {limits} (got step = {step}, T_f = {T_f}, {type(model).__name__}, "
                           f"xx {tuple(xx.shape)} {xx.dtype}, yy {tuple(yy.shape)} {yy.dtype})")
    state = _RolloutTrain(model, xx.detach(), yy.detach(), T_f)
    w, bias = model.fc.weight, model.fc.bias
    h = _RolloutFirstFn.apply(w, bias, state)
    for t in range(T_f - 1):
        h = _RolloutStepFn.apply(model.body_cf(h), w, bias, state, t)
    return _RolloutLastFn.apply(model.body_cf(h), state)


def _rollout_native_applies(model, xx, yy, T_f, step):
    return (step == 1 and hasattr(model, "forward_cf") and hasattr(model, "get_grid") and xx.dim() == 4 and yy.dim() == 4
            and xx.is_cuda and yy.is_cuda and xx.dtype == torch.float32 and yy.dtype == torch.float32
            and 1 <= T_f <= NATIVE_STEP_ERRORS_MAX_T and yy.shape[0] > 0 and xx[0].numel() > 0)


def ns2d_rollout_errors(model, xx, yy, T_f, step=1, return_pred=False) -> RolloutErrors:
    """The evaluation roll-out of the NS-2D loop (reference ns_train_2d.py:86-117, 133-168) under no_grad: the model runs T_f / step
    times, each prediction goes back into the input window, and the prediction is measured against yy[..., :T_f] - per time step
    (`errors.step_sum` is the reference's val_l2_step / test_l2_step for one batch, the number that selects checkpoints) and as a
    whole trajectory (`errors.full_sum`, its test_l2).  xx (B, S, S, T_in), yy (B, S, S, >= T_f).  No host synchronisation; the
    model's training mode is left as it is (ns2d_evaluate switches it).

    float32 device tensors, step == 1, a model with forward_cf / get_grid, T_f <= 256 and B > 0 take the native path: the window is
    built once channels-first next to the model's positional features (as ns2d_rollout_loss builds it), the ground truth is copied
    once to time-major order, and between two forward passes ONE launch (uno_rollout_advance, K18) takes the step's sums, stores the
    frame into the prediction and moves the window in place; one finish launch after the last step gives the five quantities.
    Everything else takes the stock path, the reference's loop written out; with step > 1 its per-step quantities are still per
    time slice (the reference's loss there is per group of `step` frames)."""
    if T_f < 1 or step < 1 or T_f % step or yy.shape[-1] < T_f:
        raise RuntimeError(f"ns2d_rollout_errors: T_f = {T_f} must be a positive multiple of step = {step} within the {yy.shape[-1]} frames of yy")
    with torch.no_grad():
        xx, yy = xx.detach(), yy.detach()
        if not _rollout_native_applies(model, xx, yy, T_f, step):
            pred = None
            for t in range(0, T_f, step):
                im = model(xx)
                pred = im if pred is None else torch.cat((pred, im), -1)
                xx = torch.cat((xx[..., step:], im), dim=-1)
            return RolloutErrors(_step_errors_stock(pred, yy[..., :T_f]), pred if return_pred else None)
        record, pred = _rollout_native(model, xx, yy, T_f, return_pred)
        return _rollout_result(record, pred, yy.shape[0], T_f)


def _rollout_native(model, xx, yy, T_f, return_pred):
    """The native roll-out (call under no_grad) -> (the flat record of the five quantities, _native.rollout_record; the time-major
    prediction (B, T_f, S, S) or None)"""
    from .. import _native
    B, T_in = xx.shape[0], xx.shape[-1]
    P = xx.shape[1] * xx.shape[2]
    grid = model.get_grid(xx.shape, xx.device)
    # (B, T_in + features, S, S), DENSE in that order (a plain cat of the two permuted views would come out channels-last in memory)
    z = torch.empty((B, T_in + grid.shape[-1], xx.shape[1], xx.shape[2]), dtype=torch.float32, device=xx.device)
    torch.cat((xx.permute(0, 3, 1, 2), grid.permute(0, 3, 1, 2)), dim=1, out=z)
    target = yy[..., :T_f].permute(0, 3, 1, 2).contiguous()                                                     # (B, T_f, S, S): time-major
    pred = torch.empty_like(target) if return_pred else None
    ws = _native.rollout_ws(B, P, T_f, xx.device)
    for t in range(T_f):
        im = model.forward_cf(z).contiguous()                   # (B, 1, S, S): complete before the launch below overwrites its input
        _native.rollout_advance(z, im, target, pred, ws, T_in, t, t + 1 < T_f)
    record = _native.rollout_record(B, T_f, xx.device)
    _native.rollout_finish(ws, B, P, T_f, record=record)
    return record, pred


def _rollout_result(record, pred, B, T_f) -> RolloutErrors:
    from .. import _native
    sums, rel, totals = _native.rollout_views(record, B, T_f)
    errors = StepErrors(sums, rel[:, :T_f], rel[:, T_f], totals[0], totals[1])
    return RolloutErrors(errors, pred.permute(0, 2, 3, 1) if pred is not None else None)


def ns2d_evaluate(model, batches, T_f, step=1):
    """Validation / test pass of the NS-2D loop (reference ns_train_2d.py:86-117, 133-168): eval mode, no_grad, per batch one
    ns2d_rollout_errors; -> (sum of the per-step errors, sum of the whole-trajectory errors) over all batches as 0-dim device tensors
    (no host synchronisation).  The previous training mode is restored.  The caller divides by nval * (T_f / step) and by nval."""
    was_training = model.training
    model.eval()
    step_total = full_total = None
    try:
        for xx, yy in batches:
            e = ns2d_rollout_errors(model, xx, yy, T_f, step).errors
            step_total = e.step_sum if step_total is None else step_total + e.step_sum
            full_total = e.full_sum if full_total is None else full_total + e.full_sum
    finally:
        model.train(was_training)
    return step_total, full_total


def ns3d_step_error(out, y):
    """The number the reference's NS-3D loop prints and selects checkpoints by (ns_train_3d.py:55-62): the sum over the time steps
    of the per-step relative L2 error summed over the batch.  out, y: (B, S, S, T_f); a 0-dim device tensor, no gradient."""
    return step_errors(out, y).step_sum


def ns3d_loss(model, x, y, with_step_error=False, native=False):
    """Space-time loss of the NS-3D training step (reference ns_train_3d.py:53,64): one forward, global relative L2.
    with_step_error=True: -> (loss, step error), the latter from the same forward's detached output under no_grad (:55-62).
    native=True (opt-in): loss and step error come from ONE step_losses call - two launches forward, one backward on device tensors."""
    B, S, T_f = x.shape[0], x.shape[1], y.shape[-1]
    out = model(x).view(B, S, S, T_f)
    if native:
        e = step_losses(out, y.reshape(B, S, S, T_f))
        return (e.full_sum, e.step_sum.detach()) if with_step_error else e.full_sum
    loss = lp_loss_rel_sum(out.reshape(B, -1), y.reshape(B, -1))
    if not with_step_error:
        return loss
    with torch.no_grad():
        return loss, ns3d_step_error(out.detach(), y.reshape(B, S, S, T_f))


def ns3d_evaluate(model, batches):
    """Validation pass of the NS-3D loop (reference ns_train_3d.py:82-98): eval mode, no_grad, the per-batch step errors summed on the
    device (no host synchronisation); the previous training mode is restored.  The caller divides by nval * T_f."""
    was_training = model.training
    model.eval()
    total = None
    try:
        with torch.no_grad():
            for x, y in batches:
                B, S, T_f = x.shape[0], x.shape[1], y.shape[-1]
                err = ns3d_step_error(model(x).view(B, S, S, T_f), y.reshape(B, S, S, T_f))
                total = err if total is None else total + err
    finally:
        model.train(was_training)
    return total


class GraphedStep:
    """Forward + loss + backward of one training step captured ONCE into a HIP graph (torch.cuda.CUDAGraph = hipGraph on ROCm)
    and replayed per step.  With a capturable optimiser (ComplexAdam(capturable=True): step count on the device, bias corrections
    evaluated there - reference Adam.py:27-52 takes them from state['step'] on the host) the update is part of the graph too; with
    any other optimiser it runs eagerly after the replay.
    Single rank only: no gradient all-reduce is issued between the replay and the update (DarcyTrainer is the data-parallel step).

    For launch-bound steps: the NS-2D roll-out (reference ns_train_2d.py:46-68) issues ~7400 kernels of 5-40 us per step and
    the host needs ~95 ms to enqueue them - as long as the device needs to run them.  A replay has no per-launch host work.
    Every kernel of this package launches on torch's current stream and allocates through torch's caching allocator, so
    the capture sees all of them (including the event fork / join onto the spectral backward's side stream); one-time set-up
    (twiddle tables, resampling tables, side streams) happens in the eager warm-up steps that precede the capture.

        gs = GraphedStep(model, opt, lambda xx, yy: ns2d_rollout_loss(model, xx, yy, 40), (xx0, yy0))
        loss = gs.step(xx, yy)        # device tensor, no host synchronisation
    """

    def __init__(self, model, opt, loss_fn, example_inputs, warmup: int = 2):
        if not torch.cuda.is_available():
            raise RuntimeError("GraphedStep needs the GPU (HIP graph capture)")
        self.model, self.opt, self.loss_fn = model, opt, loss_fn
        self.opt_in_graph = bool(getattr(opt, "capturable", False))
        if self.opt_in_graph:
            opt.init_state()                            # moments and step counters exist before the capture (nothing to re-zero on replay)
        self.static_in = tuple(t.clone() for t in example_inputs)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # eager warm-up off the default stream, as capture requires
            for _ in range(warmup):
                opt.zero_grad(set_to_none=True)
                loss_fn(*self.static_in).backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        opt.zero_grad(set_to_none=True)                 # .grad tensors are created inside the capture: static across replays
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_loss = loss_fn(*self.static_in)
            self.static_loss.backward()
            if self.opt_in_graph:
                self.opt.step()
        self._params = [p for g in opt.param_groups for p in g["params"] if p.requires_grad]

    def step(self, *inputs):
        for dst, src in zip(self.static_in, inputs):
            dst.copy_(src, non_blocking=True)
        if self.opt_in_graph:
            self.opt.sync_hyper()                       # lr / eps / weight decay live on the device: a scheduler's edit reaches the replay
        self.graph.replay()                             # gradients are overwritten by the captured backward
        if self.opt_in_graph:
            torch.autograd.graph.increment_version(self._params)       # the replayed update wrote the parameters through raw pointers
        else:
            self.opt.step()
        return self.static_loss.detach().clone()        # the graph-owned scalar is overwritten by the next replay


class GraphedRollout:
    """The whole native evaluation roll-out (ns2d_rollout_errors: window build, target transpose, T_f forward passes with one
    uno_rollout_advance each, the finish launch) captured ONCE into a HIP graph and replayed per batch - GraphedStep's recipe, forward
    only.  A replay has no per-launch host work: it pays where the host's enqueueing is the longer side (small batches and widths); at
    UNO(14, 32), 64^2, batch 32 the device is, and replay and eager call take the same time.  Parameters are read through their pointers: a replay after an optimiser step (or a load_state_dict) sees the new weights.
    The model's training mode at construction is the captured one.

        gr = GraphedRollout(model, 40, (xx0, yy0))
        e = gr.errors(xx, yy).errors          # device tensors, no host synchronisation
        step_total, full_total = gr.evaluate(val_batches)

    Every batch must have the example's shapes (a last, smaller batch goes through ns2d_rollout_errors)."""

    def __init__(self, model, T_f, example_inputs, return_pred=False, warmup: int = 1):
        if not torch.cuda.is_available():
            raise RuntimeError("GraphedRollout needs the GPU (HIP graph capture)")
        xx, yy = example_inputs
        if not _rollout_native_applies(model, xx, yy, T_f, 1):
            raise RuntimeError("GraphedRollout captures the native roll-out only: float32 device tensors (B, S, S, T), a model with "
                               f"forward_cf / get_grid, 1 <= T_f <= {NATIVE_STEP_ERRORS_MAX_T}, a non-empty batch")
        self.model, self.T_f, self.return_pred = model, T_f, return_pred
        self.static_in = (xx.clone(), yy.clone())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # eager warm-up off the default stream, as capture requires (it also builds
            for _ in range(max(1, warmup)):             # the cached grid features and operand tables: at least one pass)
                ns2d_rollout_errors(model, *self.static_in, T_f, return_pred=return_pred)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self._record, self._pred = _rollout_native(model, *self.static_in, T_f, return_pred)

    def _replay(self, xx, yy):
        for dst, src in zip(self.static_in, (xx, yy)):
            if dst.shape != src.shape:
                raise RuntimeError(f"GraphedRollout: captured for {tuple(dst.shape)}, got {tuple(src.shape)}")
            if src.data_ptr() != dst.data_ptr():        # (a batch loaded straight into gr.static_in needs no copy)
                dst.copy_(src, non_blocking=True)
        self.graph.replay()

    def errors(self, xx, yy) -> RolloutErrors:
        """-> RolloutErrors of this batch; clones (one of the record of the five quantities, one of the prediction): the graph-owned
        tensors are overwritten by the next replay"""
        self._replay(xx, yy)
        return _rollout_result(self._record.clone(), self._pred.clone() if self._pred is not None else None, xx.shape[0], self.T_f)

    def evaluate(self, batches):
        """as ns2d_evaluate: -> (sum of the per-step errors, sum of the whole-trajectory errors) over the batches"""
        total = None
        for xx, yy in batches:
            self._replay(xx, yy)
            totals = self._record[-2:]
            total = totals.clone() if total is None else total + totals
        return total[0], total[1]


class DarcyTrainer:
    """model + ComplexAdam + flat-gradient data parallelism.  step(a, u) runs forward, relative-L2 loss,
    backward, gradient all-reduce and the optimiser update; it returns the (device) loss tensor and
    never synchronises with the host."""

    def __init__(self, model, lr=1e-3, weight_decay=1e-3, group=None, force_collectives=False, bucket_mb=32.0, comm_dtype=None,
                 comm_cus=None):
        self.model = model
        self.group = group
        self.force_collectives = force_collectives      # tests: run the collectives even in a 1-rank group
        self.grads = FlatGradients(model.parameters(), bucket_mb=bucket_mb, comm_dtype=comm_dtype)
        # more than one rank: RCCL's all-reduce kernels run beside the backward pass - the library's device-sized launch geometries leave
        # them `comm_cus` compute units (default 16, UNO_COMM_CUS overrides; a single rank reserves none)
        self.comm_cus = 0
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1 and next(model.parameters()).is_cuda:
            import os
            from .. import _native
            self.comm_cus = int(os.environ.get("UNO_COMM_CUS", 16 if comm_cus is None else comm_cus))
            _native.reserve_cus(self.comm_cus)
        self.opt = ComplexAdam(model.parameters(), lr=lr, weight_decay=weight_decay)
        self.broadcast_parameters()

    def broadcast_parameters(self):
        if dist.is_available() and dist.is_initialized() and (self.force_collectives or dist.get_world_size(self.group) > 1):
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                dist.broadcast(torch.view_as_real(t.data) if t.is_complex() else t.data, src=0, group=self.group)

    def step_with(self, loss_closure):
        """zero grads -> loss_closure() -> backward with bucketed gradient all-reduce overlapped -> optimiser update."""
        self.grads.zero_()
        loss = loss_closure()
        self.grads.arm(self.group, self.force_collectives)
        try:
            loss.backward()
        except BaseException:
            self.grads.abort()          # collectives in flight are waited for, the bucket state is reset: the next step starts clean
            from ..integral_operators import release_pass_state
            release_pass_state()        # (autograd skips a failed pass's final callbacks: its in-place gradient map would linger)
            raise
        self.grads.finish()
        self.opt.step()
        return loss.detach()

    def step(self, a, u):
        B, S = a.shape[0], a.shape[1]
        return self.step_with(lambda: lp_loss_rel_sum(self.model(a).reshape(B, -1), u.reshape(B, -1)))

    def step_blocking(self, a, u):
        """The same step with the exchange NOT overlapped: backward first, then one blocking all-reduce of the whole flat
        buffer (the comparison figure of bench.py's `comm` object)."""
        B = a.shape[0]
        self.grads.zero_()
        loss = lp_loss_rel_sum(self.model(a).reshape(B, -1), u.reshape(B, -1))
        loss.backward()
        self.grads.all_reduce_sum(self.group, self.force_collectives)
        self.opt.step()
        return loss.detach()
