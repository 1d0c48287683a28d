from typing import NamedTuple, Optional

import torch


def lp_loss_rel_sum(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Sum over the batch of ||pred_b - target_b||_2 / ||target_b||_2 - what the reference trains on:
    LpLoss(size_average=False)(out, y) (utilities3.py:86-100, train_darcy.py:42,53)."""
    n = pred.shape[0]
    diff = torch.linalg.vector_norm(pred.reshape(n, -1) - target.reshape(n, -1), ord=2, dim=1)
    return (diff / torch.linalg.vector_norm(target.reshape(n, -1), ord=2, dim=1)).sum()


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
