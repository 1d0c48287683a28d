"""``from navier_stokes_uno3d import Uno3D_T40, ...`` -> the harness models: the reference's constructor arguments, sub-module names
and state_dict layout on the native 3-D layers (uno_amd/harness/models.py); ns_train_3d.py runs on them unchanged.  The `*_256`
variants have no counterpart."""
from uno_amd.harness.models import Uno3D_T9, Uno3D_T10, Uno3D_T20, Uno3D_T40  # noqa: F401

__all__ = ["Uno3D_T40", "Uno3D_T20", "Uno3D_T10", "Uno3D_T9"]
