"""``from Adam import Adam`` -> ComplexAdam (uno_amd/harness/optim.py): the reference optimiser's update - second moment from
g * conj(g), coupled weight decay, per-parameter bias correction - as one multi-tensor kernel per step on the device."""
from uno_amd.harness.optim import ComplexAdam

__all__ = ["Adam"]


class Adam(ComplexAdam):
    """The call the training scripts make: Adam(params, lr=..., weight_decay=..., amsgrad=False).  max_grad_norm / skip_nonfinite: ComplexAdam's guarded step (global
    gradient-norm clipping and the skip of a non-finite step, on the device)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, capturable=False, max_grad_norm=None,
                 skip_nonfinite=None):
        if amsgrad:
            raise ValueError("Adam(amsgrad=True) is not available: the reference's AMSGrad branch takes torch.maximum of the second moments, "
                             "which it keeps complex for the spectral weights, and torch.maximum does not accept complex tensors - it "
                             "cannot run for any U-NO model there either")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable, max_grad_norm=max_grad_norm,
                         skip_nonfinite=skip_nonfinite)
