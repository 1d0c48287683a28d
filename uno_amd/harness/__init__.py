"""Own counterparts of the reference's callers of the hot path:
the Darcy U-NO model, the relative-L2 loss, the complex-modulus Adam and the (data-parallel)
training step, the data generators, and - in `fit` and `data` - the reference's three training loops and two
loaders restated epoch for epoch on these pieces, so that the hot path can be driven, measured and trained with
end to end without the reference checkout."""
from .models import UNO, UNO_9, UNO_P, UNO_S256, Uno3D_T9, Uno3D_T10, Uno3D_T20, Uno3D_T40  # noqa: F401
from .optim import ComplexAdam  # noqa: F401
from .losses import HsLoss, LpLoss, RolloutErrors, StepErrors, lp_loss_rel_sum, rel_l2, sobolev_rel, step_errors, step_losses  # noqa: F401
from .data import DeviceDataset, MatReader, load_darcy, load_ns  # noqa: F401
from .mixed import MixedDarcyTrainer  # noqa: F401
from .train import DarcyTrainer, GraphedRollout, GraphedStep, ns2d_evaluate, ns2d_rollout_errors, ns2d_rollout_loss, ns3d_evaluate, ns3d_loss, ns3d_step_error, synthetic_darcy_batch  # noqa: F401
from .datagen import GaussianRF, generate_ns_dataset, navier_stokes_2d  # noqa: F401
from .darcy_datagen import darcy_grf, generate_darcy_dataset, solve_gwf, spline_matrix, threshold  # noqa: F401
from .spectra import SpectralErrors, energy_spectrum, n_shells, shell_index, sobolev_weights, spectral_errors  # noqa: F401
from . import workloads  # noqa: F401,E402

_FIT = ("EpochRecord", "FitRecord", "fit_darcy", "fit_ns2d", "fit_ns3d")
_PREDICT = ("LayerPlan", "Prediction", "Predictor", "check_resolution", "load_model", "read_record")


def __getattr__(name):
    """the epoch runners and the predict stage on first use: `python -m uno_amd.harness.fit` (`... .predict`) runs that module as a
    script, which must not be imported before"""
    if name in _FIT:
        from . import fit
        return getattr(fit, name)
    if name in _PREDICT:
        from . import predict
        return getattr(predict, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
