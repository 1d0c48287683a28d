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


SOBOLEV_LAYOUTS = ("bhw", "bhwt", "bthw")
_HALF_WEIGHTS = {}


def _sobolev_views(x, y, layout, who):
    """-> the (B, T, H, W) views of x and y"""
    if layout not in SOBOLEV_LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {', '.join(SOBOLEV_LAYOUTS)}")
    for name, t in (("x", x), ("y", y)):
        if t.dim() != len(layout):
            raise ValueError(f"{who}: {name} {tuple(t.shape)} is not a {layout!r} tensor of {len(layout)} axes")
        if not t.is_floating_point():
            raise ValueError(f"{who}: {name} must be a real floating-point tensor (got {t.dtype})")
    if x.shape != y.shape:
        raise ValueError(f"{who}: prediction {tuple(x.shape)} and target {tuple(y.shape)} differ")
    if layout == "bhwt":
        return x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    return (x, y) if layout == "bthw" else (x.unsqueeze(1), y.unsqueeze(1))


def _sobolev_refusal(x, y):
    """None where K25 takes these (B, T, H, W) views, or why it does not"""
    from .. import _native
    lo, hi = _native.SOBOLEV_MIN, _native.SOBOLEV_MAX
    for name, t in (("the input", x), ("the target", y)):
        if not t.is_cuda:
            return f"{name} is on {t.device}, the kernel runs on the GPU"
        if t.dtype != torch.float32:
            return f"{name} is {t.dtype}, the kernel takes float32"
        if min(t.stride()) < 0:
            return f"{name} has a negative stride {t.stride()}"
    if y.device != x.device:
        return f"input on {x.device}, target on {y.device}"
    if y.requires_grad and torch.is_grad_enabled():
        return "the target requires grad, the kernel has no gradient for it"
    H, W = x.shape[2:]
    if not (lo <= H <= hi and lo <= W <= hi):
        return f"frames of {H} x {W}: the kernel takes {lo} ... {hi} points per axis"
    if x.shape[1] < 1:
        return "no frame per sample"
    return None


def _half_weights(H, W, k, a, device, dtype):
    """(H, W // 2 + 1) on `device`: the weight of every mode of the half spectrum rfft2 returns - the table's row |ky| in fftfreq order,
    times the Hermitian weight, over (H W)^2; built in float64, cached per (H, W, k, a, device, dtype)"""
    from .spectra import _sobolev_a, sobolev_weights
    key = (H, W, int(k), _sobolev_a(k, a), str(device), dtype)
    if key not in _HALF_WEIGHTS:
        from .. import _native
        r = torch.arange(H)
        wt = sobolev_weights(H, W, k, a)[torch.minimum(r, H - r)] * 2.0
        wt[:, 0] *= 0.5
        if W % 2 == 0:
            wt[:, W // 2] *= 0.5
        _HALF_WEIGHTS[key] = _native.table_to_device((wt / (float(H) * W) ** 2).to(dtype), device)
    return _HALF_WEIGHTS[key]


def _sobolev_stock(x, y, k, a, per_frame):
    """(B, T, H, W) views of any float dtype and device -> the ratios by the definition, on rfft2; differentiable by autograd"""
    B, T, H, W = x.shape
    wt = _half_weights(H, W, k, a, x.device, x.dtype)
    D, Y = torch.fft.rfft2(x - y, dim=(-2, -1)), torch.fft.rfft2(y, dim=(-2, -1))
    num = (wt * (D.real * D.real + D.imag * D.imag)).sum(dim=(-2, -1))
    den = (wt * (Y.real * Y.real + Y.imag * Y.imag)).sum(dim=(-2, -1))
    if not per_frame:
        num, den = num.sum(dim=1), den.sum(dim=1)
    return torch.sqrt(num) / torch.sqrt(den)


class _SobolevFn(torch.autograd.Function):
    """(x, y) as (B, T, H, W) views and the device weight table -> the ratios (reduce = 0), their sum (1) or their mean (2), 0-dim:
    uno_sobolev_forward / uno_sobolev_backward (K25).  The weighted difference spectrum is stored only when x needs a gradient; the
    upstream gradient stays on the device, and a reduced result hands the kernel ONE scalar."""

    @staticmethod
    def forward(ctx, x, y, w2, per_frame, reduce, need_grad):
        from .. import _native
        record, z = _native.sobolev_forward(x, y, w2, per_frame, want_z=need_grad)
        B, T = x.shape[:2]
        if need_grad:
            ctx.save_for_backward(record, z)
            ctx.like = x.detach()                # its shape and strides only
        ctx.per_frame, ctx.reduce = per_frame, reduce
        _, ratio, total = _native.sobolev_views(record, B, T, per_frame)
        if reduce == 0:
            return ratio
        return total[0] if reduce == 1 else total[0] / max(1, ratio.numel())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .. import _native
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        record, z = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.to(torch.float32)
        if g.numel() > 1 and all(s == 0 for s in g.stride()):      # the gradient of `.sum()`: one value expanded over the rows
            g = g[(0,) * g.dim()]
        g = g.reshape(-1) if g.is_contiguous() else g.contiguous().reshape(-1)
        rows = ctx.like.shape[0] * (ctx.like.shape[1] if ctx.per_frame else 1)
        gx = _native.sobolev_backward(z, record, g, ctx.like, ctx.per_frame, 1.0 / max(1, rows) if ctx.reduce == 2 else 1.0)
        return gx, None, None, None, None, None


NATIVE_SOBOLEV_MAX_SIDE, NATIVE_SOBOLEV_MAX_WORK = 256, 1.1e9


def sobolev_native_default(B, T, H, W) -> bool:
    """whether `native=None` takes K25 at this shape: only where its forward + backward measured faster than the stock ops
    (tools/sobolev_loss_time.py, profiles/sobolev_loss_time.txt).  The kernel's transforms are dense sums, B T H W (W + 2 H)
    multiply-adds per source, against rocFFT's H W log(H W): it won 1.7 ... 3.6 times at up to 128 points a side (up to 1.01 G
    multiply-adds) and at 256^2 with 16 frames (0.81 G), tied at 256^2 with 40 frames (2.01 G: 0.91 and 1.03 of the stock time in two
    runs), and lost at 256^2 with 80 frames (4.03 G), at 512^2 and - but for a 2 % win at 16 frames - at 421^2, where one workgroup's
    serial chain of row tiles sets the time.  So: at most 256 points a side and at most 1.1 G multiply-adds per call; `native=True` still takes the kernel at every shape it applies to."""
    return max(H, W) <= NATIVE_SOBOLEV_MAX_SIDE and float(B) * T * H * W * (W + 2 * H) <= NATIVE_SOBOLEV_MAX_WORK


def _sobolev(x, y, layout, k, a, per_frame, native, reduce, who):
    xv, yv = _sobolev_views(x, y, layout, who)
    B, T = xv.shape[:2]
    per_frame = bool(per_frame)
    if B == 0 or xv.numel() == 0:               # nothing to transform: empty ratios that still hang on x
        if native:
            why = _sobolev_refusal(xv, yv)
            if why is not None:
                raise RuntimeError(f"{who}(native=True): {why}")
        ratio = xv.flatten(2).sum(dim=2) if per_frame else xv.flatten(1).sum(dim=1)
        return ratio if reduce == 0 else ratio.sum()
    why = _sobolev_refusal(xv, yv)
    if native and why is not None:
        raise RuntimeError(f"{who}(native=True): {why}")
    if native is None:
        native = why is None and sobolev_native_default(B, T, *xv.shape[2:])
    if native:
        from .spectra import sobolev_table
        w2 = sobolev_table(xv.shape[2], xv.shape[3], k, a, xv.device, torch.float32)
        need = xv.requires_grad and torch.is_grad_enabled()
        out = _SobolevFn.apply(xv, yv.detach(), w2, per_frame, reduce, need)
    else:
        if yv.dtype != xv.dtype or yv.device != xv.device:
            raise ValueError(f"{who}: prediction ({xv.dtype}, {xv.device}) and target ({yv.dtype}, {yv.device}) differ")
        out = _sobolev_stock(xv, yv, k, a, per_frame)
        if reduce:
            out = out.sum() if reduce == 1 else out.mean()
    if reduce == 0 and per_frame and layout == "bhw":
        out = out[:, 0]
    return out


def sobolev_rel(x, y, layout="bhw", k=1, a=None, per_frame=False, native=None):
    """The relative Sobolev (H^k) error of x against y, differentiable in x.  With X = fft2(x) / (H W) over integer wavenumbers and
    w2 = spectra.sobolev_weights(H, W, k, a) read at (|ky|, |kx|):

        num[b, t] = sum_k w2 |X - Y|^2,  den[b, t] = sum_k w2 |Y|^2       (both Hermitian halves)
        (B,)   sqrt(sum_t num) / sqrt(sum_t den)        per_frame=False
        (B, T) sqrt(num) / sqrt(den)                    per_frame=True ((B,) for layout "bhw")

    k = 0 is the reference's relative L2 over the flattened sample (Parseval).  layout: "bhw" (B, H, W), "bhwt" (B, H, W, T) or "bthw"
    (B, T, H, W); views (time slices, [::r, ::r] sub-sampling) are read where they lie.  native: None - the kernel (K25: two launches
    forward, one backward, fixed summation order, no host synchronisation) where it applies and measured faster
    (sobolev_native_default: up to 256 points a side and 1.1 G multiply-adds per call), else stock ops; True - the kernel, a
    RuntimeError saying why where it does not apply; False - stock ops: the same definition on torch.fft.rfft2 in the input's dtype,
    differentiable by autograd, which serves CPU tensors, other dtypes, grids outside 8 ... 512 points per axis and a target that
    requires grad.  No clamping; no gradient reaches y on the native path."""
    return _sobolev(x, y, layout, k, a, per_frame, native, 0, "sobolev_rel")


class HsLoss(object):
    """The relative Sobolev loss as a loss object in LpLoss's shape - `rel` and `__call__`; sum (size_average=False) and mean come from
    the kernel's own total, so a training step's loss costs two launches forward and one backward.  k = 1 is H^1, k = 2 H^2; a: the
    coefficients a_1 ... a_k of spectra.sobolev_weights (default 1); layout and native: as sobolev_rel's."""

    def __init__(self, k=1, a=None, layout="bhw", size_average=True, reduction=True, native=None):
        super(HsLoss, self).__init__()
        if layout not in SOBOLEV_LAYOUTS:
            raise ValueError(f"layout {layout!r}: one of {', '.join(SOBOLEV_LAYOUTS)}")
        from .spectra import _sobolev_a
        self.k = int(k)
        self.a = None if a is None else _sobolev_a(k, a)
        self.layout = layout
        self.reduction = reduction
        self.size_average = size_average
        self.native = native

    def rel(self, x, y):
        return _sobolev(x, y, self.layout, self.k, self.a, False, self.native, 0 if not self.reduction else (2 if self.size_average else 1),
                        "HsLoss")

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
