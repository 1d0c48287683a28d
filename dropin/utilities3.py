"""``from utilities3 import *`` -> LpLoss on the native relative-L2 kernels (uno_amd/harness/losses.py) and a MatReader with the
reference's method names, because data_load_darcy.py and data_load_navier_stocks.py import it."""
import numpy as np
import torch

from uno_amd.harness.losses import LpLoss  # noqa: F401

__all__ = ["LpLoss", "MatReader", "device"]

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class MatReader(object):
    """Fields of a MATLAB file as arrays or tensors.  Files up to format v7 are read with scipy.io.loadmat; v7.3 files are HDF5 and
    are opened with h5py, whose arrays come with their axes reversed and are turned back.  Both libraries are imported when a file
    is opened, so importing this module needs neither."""

    def __init__(self, file_path, to_torch=True, to_cuda=False, to_float=True):
        self.to_torch, self.to_cuda, self.to_float = to_torch, to_cuda, to_float
        self.file_path = file_path
        self.data, self.old_mat = None, None
        self._load_file()

    def _load_file(self):
        try:
            import scipy.io
            self.data, self.old_mat = scipy.io.loadmat(self.file_path), True
        except (ImportError, NotImplementedError, ValueError):         # no scipy, or a v7.3 (HDF5) file
            import h5py
            self.data, self.old_mat = h5py.File(self.file_path, "r"), False

    def load_file(self, file_path):
        self.file_path = file_path
        self._load_file()

    def read_field(self, field):
        x = self.data[field]
        if not self.old_mat:
            x = np.asarray(x[()])
            x = x.transpose(tuple(reversed(range(x.ndim))))
        if self.to_float:
            x = x.astype(np.float32)
        if self.to_torch:
            x = torch.from_numpy(np.ascontiguousarray(x))
            if self.to_cuda:
                x = x.cuda()
        return x

    def set_cuda(self, to_cuda):
        self.to_cuda = to_cuda

    def set_torch(self, to_torch):
        self.to_torch = to_torch

    def set_float(self, to_float):
        self.to_float = to_float
