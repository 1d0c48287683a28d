from typing import NamedTuple, Optional

import torch


def lp_loss_rel_sum(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Sum over the batch of ||pred_b - target_b||_2 / ||target_b||_2 - what the reference trains on:
    LpLoss(size_average=False)(out, y) (utilities3.py:86-100, train_darcy.py:42,53)."""
    n = pred.shape[0]
    diff = torch.linalg.vector_norm(pred.reshape(n, -1) - target.reshape(n, -1), ord=2, dim=1)
    return (diff / torch.linalg.vector_norm(target.reshape(n, -1), ord=2, dim=1)).sum()


def _rows(t: torch.Tensor) -> Optional[torch.Tensor]:
    """t seen as (B, N) without a copy - a row stride and an element stride - or None where that needs more than two strides
    (a cropped plane) or there is nothing to sum"""
    if t.dim() < 1 or t.shape[0] == 0 or t.numel() == 0:
        return None
    try:
        return t.view(t.shape[0], -1)
    except RuntimeError:
        return None


def _native_rows(x: torch.Tensor, y: torch.Tensor):
    """(x, y) as the (B, N) views the native loss takes, or None: float32 device tensors of one shape, a target that needs no gradient"""
    if not (x.is_cuda and y.is_cuda and x.device == y.device and x.dtype == torch.float32 and y.dtype == torch.float32
            and x.shape == y.shape and not (y.requires_grad and torch.is_grad_enabled())):
        return None
    xr, yr = _rows(x), _rows(y)
    return None if xr is None or yr is None else (xr, yr)


class _RelL2Fn(torch.autograd.Function):
    """(x, y) as (B, N) views -> the ratios (B,) (reduce = 0), their sum (1) or their mean (2), 0-dim: uno_rel_l2_forward /
    uno_rel_l2_backward (K20).  The upstream gradient stays on the device; a reduced result hands the kernel ONE scalar."""

    @staticmethod
    def forward(ctx, x, y, reduce):
        from .. import _native
        record = _native.rel_l2_forward(x, y)           # [sums (B, 2) | ratio (B) | total (1) | workspace]
        ctx.save_for_backward(x, y, record)
        ctx.reduce = reduce
        B = x.shape[0]
        if reduce == 0:
            return record[2 * B:3 * B]
        return record[3 * B] if reduce == 1 else record[3 * B] / B

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .. import _native
        if not ctx.needs_input_grad[0]:
            return None, None, None
        x, y, record = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.to(torch.float32)
        if g.dim() == 1 and g.shape[0] > 1 and g.stride(0) == 0:        # the gradient of `.sum()`: one value expanded over the rows
            g = g[:1]
        elif not g.is_contiguous():
            g = g.contiguous()
        return _native.rel_l2_backward(x, y, record, g, 1.0 / x.shape[0] if ctx.reduce == 2 else 1.0), None, None


def rel_l2(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """||x_b - y_b||_2 / ||y_b||_2 for every batch entry b, (B,), differentiable in x - `LpLoss(reduction=False)(x, y)` of the reference
    (utilities3.py:86-100).  float32 device tensors whose (B, -1) view is a row stride plus an element stride (dense tensors, and the
    time slices `out[..., t]` of ns_train_3d.py:58-61) with a target that needs no gradient take the native kernels (K20: two launches
    forward, one backward, fixed summation order, no host synchronisation); everything else - CPU, other dtypes, a target that
    requires grad, views of more than two strides - the stock ops of lp_loss_rel_sum."""
    rows = _native_rows(x, y)
    if rows is None:
        n = x.shape[0]
        diff = torch.linalg.vector_norm(x.reshape(n, -1) - y.reshape(n, -1), ord=2, dim=1)
        return diff / torch.linalg.vector_norm(y.reshape(n, -1), ord=2, dim=1)
    return _RelL2Fn.apply(rows[0], rows[1], 0)


class LpLoss(object):
    """The reference's loss object (utilities3.py:75-103) - same constructor, `rel` and `__call__` - on the native relative-L2 kernels
    where they apply (p == 2 and the conditions of rel_l2); sum and mean are the kernel's own total, so a training step's loss costs
    two launches forward and one backward.  Other p and everything rel_l2 leaves to stock ops run as the reference writes them."""

    def __init__(self, d=2, p=2, size_average=True, reduction=True):
        super(LpLoss, self).__init__()
        assert d > 0 and p > 0
        self.d = d
        self.p = p
        self.reduction = reduction
        self.size_average = size_average

    def rel(self, x, y):
        rows = _native_rows(x, y) if self.p == 2 else None
        if rows is not None:
            return _RelL2Fn.apply(rows[0], rows[1], 0 if not self.reduction else (2 if self.size_average else 1))
        n = x.size()[0]
        ratio = torch.linalg.vector_norm(x.reshape(n, -1) - y.reshape(n, -1), ord=self.p, dim=1) \
            / torch.linalg.vector_norm(y.reshape(n, -1), ord=self.p, dim=1)
        if self.reduction:
            return torch.mean(ratio) if self.size_average else torch.sum(ratio)
        return ratio

    def __call__(self, x, y):
        return self.rel(x, y)


class StepErrors(NamedTuple):
    """Relative L2 errors of a (B, ..., T) prediction per time step and for the whole trajectory (device tensors)."""
    sums: torch.Tensor          # (B, T, 2): [sum (pred - target)^2, sum target^2] of every time slice
    per_step: torch.Tensor      # (B, T): ||pred_t - target_t|| / ||target_t||
    full: torch.Tensor          # (B,): the same ratio over the whole trajectory
    step_sum: torch.Tensor      # 0-dim: sum over batch and steps of per_step - the reference's temp_step_loss
    full_sum: torch.Tensor      # 0-dim: sum over the batch of full - LpLoss(size_average=False) of the whole trajectory


class RolloutErrors(NamedTuple):
    """What one evaluation roll-out of the NS-2D loop yields (harness.ns2d_rollout_errors)."""
    errors: StepErrors          # of the T_f predicted frames against the ground truth
    pred: Optional[torch.Tensor]        # (B, S, S, T_f) prediction - on the native path a view of the time-major buffer - or None


NATIVE_STEP_ERRORS_MAX_T = 256


def _step_errors_stock(pred: torch.Tensor, target: torch.Tensor) -> StepErrors:
    """Slice by slice as the reference's loops do (ns_train_3d.py:55-62, ns_train_2d.py:133-150)."""
    B, T = pred.shape[0], pred.shape[-1]
    sums = torch.empty((B, T, 2), dtype=pred.dtype, device=pred.device)
    per_step = torch.empty((B, T), dtype=pred.dtype, device=pred.device)
    step_sum = torch.zeros((), dtype=pred.dtype, device=pred.device)
    for t in range(T):
        k, l = pred[..., t].reshape(B, -1), target[..., t].reshape(B, -1)
        d = k - l
        sums[:, t, 0], sums[:, t, 1] = (d * d).sum(dim=1), (l * l).sum(dim=1)
        per_step[:, t] = torch.linalg.vector_norm(d, ord=2, dim=1) / torch.linalg.vector_norm(l, ord=2, dim=1)
        step_sum = step_sum + per_step[:, t].sum()
    p, y = pred.reshape(B, -1), target.reshape(B, -1)
    full = torch.linalg.vector_norm(p - y, ord=2, dim=1) / torch.linalg.vector_norm(y, ord=2, dim=1)
    return StepErrors(sums, per_step, full, step_sum, full.sum())


def step_errors(pred: torch.Tensor, target: torch.Tensor) -> StepErrors:
    """Per-time-step and whole-trajectory relative L2 errors of pred against target, both (B, ..., T) - the numbers the reference's
    NS-3D loop prints and selects checkpoints by (`sum_t LpLoss(size_average=False)(out[..., t], y[..., t])`, ns_train_3d.py:55-62,
    84-98) and its 2-D test loop reports (ns_train_2d.py:133-150).  Forward only (the reference computes them under no_grad; the
    training loss is lp_loss_rel_sum).  float32 device tensors with T <= 256 take one native pass (uno_rel_l2_steps: two launches,
    fixed summation order); CPU tensors, other dtypes and longer time axes the stock slice-by-slice form.  No host synchronisation."""
    if pred.shape != target.shape or pred.dim() < 2:
        raise RuntimeError(f"step_errors: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be equal (B, ..., T) shapes")
    pred, target = pred.detach(), target.detach()
    if not (pred.is_cuda and target.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32
            and 1 <= pred.shape[-1] <= NATIVE_STEP_ERRORS_MAX_T and pred.shape[0] > 0 and pred[0].numel() > 0):
        return _step_errors_stock(pred, target)
    from .. import _native
    sums, rel, totals = _native.rel_l2_steps(pred.contiguous(), target.contiguous())
    T = pred.shape[-1]
    return StepErrors(sums, rel[:, :T], rel[:, T], totals[0], totals[1])


class _StepLossesFn(torch.autograd.Function):
    """(pred, target) dense (B, ..., T) -> (sums, rel, step_sum, full_sum): uno_rel_l2_steps forward (K17), uno_rel_l2_steps_backward
    (K17-B) for the gradients of the two sums.  The upstream gradients stay on the device."""

    @staticmethod
    def forward(ctx, pred, target):
        from .. import _native
        sums, rel, totals = _native.rel_l2_steps(pred, target)
        ctx.save_for_backward(pred, target, sums)
        ctx.mark_non_differentiable(sums, rel)
        ctx.set_materialize_grads(False)                # a sum nobody used arrives as None: NULL for the kernel, no zero fill
        return sums, rel, totals[0], totals[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _g_sums, _g_rel, g_step, g_full):
        from .. import _native
        if not ctx.needs_input_grad[0]:
            return None, None
        pred, target, sums = ctx.saved_tensors
        g_step, g_full = (None if g is None else g.to(torch.float32).reshape(1).contiguous() for g in (g_step, g_full))
        return _native.rel_l2_steps_backward(pred, target, sums, g_full, g_step), None


def step_losses(pred: torch.Tensor, target: torch.Tensor) -> StepErrors:
    """step_errors whose `full_sum` (the NS-3D training loss, LpLoss(size_average=False) of the whole trajectory) and `step_sum` (the
    per-step metric) carry gradient to pred: ONE pass over (pred, target) gives both, one more launch their gradient (K17 / K17-B) -
    the reference's loop computes the two in T + 1 separate loss calls (ns_train_3d.py:55-64).  The other fields carry no gradient.
    Same fall-back rule as step_errors: CPU tensors, other dtypes, T > 256 and empty tensors take the stock slice-by-slice form, through
    which autograd differentiates all five fields.  No gradient reaches target on the native path (it is detached)."""
    if pred.shape != target.shape or pred.dim() < 2:
        raise RuntimeError(f"step_losses: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be equal (B, ..., T) shapes")
    if not (pred.is_cuda and target.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32
            and 1 <= pred.shape[-1] <= NATIVE_STEP_ERRORS_MAX_T and pred.shape[0] > 0 and pred[0].numel() > 0):
        return _step_errors_stock(pred, target)
    sums, rel, step_sum, full_sum = _StepLossesFn.apply(pred.contiguous(), target.detach().contiguous())
    T = pred.shape[-1]
    return StepErrors(sums, rel[:, :T], rel[:, T], step_sum, full_sum)
