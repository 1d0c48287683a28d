"""``from utilities3 import *`` -> LpLoss on the native relative-L2 kernels (uno_amd/harness/losses.py) and a MatReader with the
reference's method names (uno_amd/harness/data.py), because data_load_darcy.py and data_load_navier_stocks.py import it."""
import torch

from uno_amd.harness.data import MatReader  # noqa: F401
from uno_amd.harness.losses import LpLoss  # noqa: F401

__all__ = ["LpLoss", "MatReader", "device"]

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
