"""``from darcy_flow_uno2d import UNO_9`` -> the harness model: the reference's constructor arguments, sub-module names and state_dict
layout on the fused native layers (uno_amd/harness/models.py).  With this directory ahead of the reference checkout on the path,
train_darcy.py and darcy_flow_main.py's imports resolve here unchanged."""
import torch.nn as nn

from uno_amd.harness.models import UNO_9  # noqa: F401

__all__ = ["UNO_9", "UNO_11"]


class UNO_11(nn.Module):
    """Importable because darcy_flow_main.py imports the name.  The reference's UNO_11 cannot be constructed: it hands its fourth
    block a `residual` argument that OperatorBlock_2D does not take, so its constructor ends in a TypeError.  So does this one."""

    def __init__(self, in_width, width, pad=5, factor=1):
        super().__init__()
        raise TypeError("UNO_11 cannot be built: the reference's constructor passes `residual=True` to OperatorBlock_2D, which has no "
                        "such parameter, and raises this error too; use UNO_9")
