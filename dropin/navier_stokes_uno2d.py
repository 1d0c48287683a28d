"""``from navier_stokes_uno2d import UNO, UNO_P, UNO_S256`` -> the harness models: the reference's constructor arguments, sub-module
names and state_dict layout on the fused native layers (uno_amd/harness/models.py); ns_train_2d.py runs on them unchanged."""
from uno_amd.harness.models import UNO, UNO_P, UNO_S256  # noqa: F401

__all__ = ["UNO", "UNO_P", "UNO_S256"]
