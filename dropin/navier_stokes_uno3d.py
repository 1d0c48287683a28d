"""``from navier_stokes_uno3d import Uno3D_T40, ...`` -> the harness models: the reference's constructor arguments, sub-module names
and state_dict layout on the native 3-D layers (uno_amd/harness/models.py); ns_train_3d.py runs on them unchanged.  Of the reference's
four `*_256` classes the two that work upstream are here - `Uno3D_T20_256` and `Uno3D_T10_256`, whose first and last layers run on the
wide-axis resample kernels at S = 256.  `Uno3D_T40_256` and `Uno3D_T9_256` have no counterpart because there is nothing to be compatible
with: upstream `Uno3D_T40_256.forward` raises AttributeError (it calls a lift layer `fc` that its constructor never creates) and
`Uno3D_T9_256.__init__` raises TypeError."""
from uno_amd.harness.models import Uno3D_T9, Uno3D_T10, Uno3D_T10_256, Uno3D_T20, Uno3D_T20_256, Uno3D_T40  # noqa: F401

__all__ = ["Uno3D_T40", "Uno3D_T20", "Uno3D_T10", "Uno3D_T9", "Uno3D_T20_256", "Uno3D_T10_256"]
