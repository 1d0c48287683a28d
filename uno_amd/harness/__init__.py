"""Own counterparts of the reference's callers of the hot path:
the Darcy U-NO model, the relative-L2 loss, the complex-modulus Adam and the (data-parallel)
training step.  They exist so the hot path can be driven and measured end to end; they are not a
re-implementation of the reference's training scripts."""
from .models import UNO, UNO_9, UNO_P, UNO_S256, Uno3D_T9, Uno3D_T10, Uno3D_T20, Uno3D_T40  # noqa: F401
from .optim import ComplexAdam  # noqa: F401
from .losses import LpLoss, RolloutErrors, StepErrors, lp_loss_rel_sum, rel_l2, step_errors  # noqa: F401
from .mixed import MixedDarcyTrainer  # noqa: F401
from .train import DarcyTrainer, GraphedRollout, GraphedStep, ns2d_evaluate, ns2d_rollout_errors, ns2d_rollout_loss, ns3d_evaluate, ns3d_loss, ns3d_step_error, synthetic_darcy_batch  # noqa: F401
from .datagen import GaussianRF, generate_ns_dataset, navier_stokes_2d  # noqa: F401
from .darcy_datagen import darcy_grf, generate_darcy_dataset, solve_gwf, spline_matrix, threshold  # noqa: F401
from . import workloads  # noqa: F401,E402
