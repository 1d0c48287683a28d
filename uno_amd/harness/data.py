"""Datasets for the epoch runners (harness.fit): the reference's two loaders restated (data_load_darcy.py, data_load_navier_stocks.py:
the files harness.darcy_datagen and harness.datagen write), the MatReader they read through, and a dataset that lives on the device -
the reference's DataLoader hands every batch over from pageable host memory, one `x.cuda()` per batch and epoch."""
import numpy as np
import torch


class MatReader(object):
    """Fields of a MATLAB file as arrays or tensors, with the reference's method names (utilities3.py).  Files up to format v7 are read
    with scipy.io.loadmat; v7.3 files are HDF5 and are opened with h5py, whose arrays come with their axes reversed and are turned
    back.  Both libraries are imported when a file is opened, so importing this module needs neither."""

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


def load_darcy(path, r, ntrain, ntest):
    """-> x_train (ntrain, s, s, 1), y_train (ntrain, s, s), x_test (ntest, s, s, 1), y_test (ntest, s, s), float32 on the host, as
    data_load_darcy.py:22-41: every r-th grid point of the fields `coeff` and `sol`, the first ntrain samples and the last ntest ones,
    the coefficient with a channel axis.  s = (n - 1) // r + 1 for the file's n x n grid (the reference writes n = 421 out)."""
    reader = MatReader(path)
    coeff, sol = reader.read_field("coeff"), reader.read_field("sol")
    if not 1 <= ntrain <= coeff.shape[0] or not 1 <= ntest <= coeff.shape[0]:
        raise ValueError(f"load_darcy: ntrain = {ntrain} and ntest = {ntest} must lie within the {coeff.shape[0]} samples of {path}")
    s = (coeff.shape[1] - 1) // r + 1
    x_train, y_train = coeff[:ntrain, ::r, ::r][:, :s, :s], sol[:ntrain, ::r, ::r][:, :s, :s]
    x_test, y_test = coeff[-ntest:, ::r, ::r][:, :s, :s], sol[-ntest:, ::r, ::r][:, :s, :s]
    return x_train.reshape(ntrain, s, s, 1), y_train, x_test.reshape(ntest, s, s, 1), y_test


def _resize(frames, size):
    """(n, s, s, t) -> (n, size, size, t), bilinear with align_corners=True as data_load_navier_stocks.py:43-54 (the identity at size == s)"""
    return torch.nn.functional.interpolate(frames.permute(0, 3, 1, 2), size=(size, size), mode="bilinear",
                                           align_corners=True).permute(0, 2, 3, 1)


def load_ns(path, train, test, sample_num=1000, batch=20, T_in=10, T=10, size=64):
    """-> train_a (., size, size, T_in), train_u (., size, size, T), test_a, test_u, float32 on the host, as
    data_load_navier_stocks.py:24-72: the fields u0, u1, ... of the file (one per generation batch of `batch` samples, (batch, s, s,
    frames)), frames [0, T_in) as input and [T_in, T_in + T) as target, resized to size x size.  The split is by WHOLE generation
    batches: a batch goes to the training part while the samples counted so far, its own included, do not exceed `train`, and to
    the test part otherwise (`test` is not read - the reference does not read it either)."""
    reader = MatReader(path)
    parts = {"train": ([], []), "test": ([], [])}
    seen = 0
    for i in range(sample_num // batch):
        seen += batch
        u = reader.read_field("u" + str(i))
        a, b = parts["train" if seen <= train else "test"]
        a.append(_resize(u[:, :, :, :T_in], size))
        b.append(_resize(u[:, :, :, T_in:T_in + T], size))
    return tuple(torch.cat(lst, dim=0) if lst else None for key in ("train", "test") for lst in parts[key])


class DeviceDataset:
    """(x, y) with equal leading sizes, resident on `device` for the whole run.  batches() draws a permutation ON the device and
    gathers each batch there: no host memory is touched and nothing is read back per batch or per epoch."""

    def __init__(self, x, y, device=None):
        if x.shape[0] != y.shape[0] or x.shape[0] == 0:
            raise ValueError(f"DeviceDataset: x {tuple(x.shape)} and y {tuple(y.shape)} need the same, non-zero number of samples")
        device = x.device if device is None else torch.device(device)
        self.x, self.y = x.to(device).contiguous(), y.to(device).contiguous()
        self.device = self.x.device

    def __len__(self):
        return self.x.shape[0]

    def batches(self, batch_size, shuffle=True, generator=None):
        """yields (x[idx], y[idx]) over one pass: every sample once, the last batch short where batch_size does not divide the sample
        count (torch's DataLoader keeps it by default).  generator: a torch.Generator on this dataset's device."""
        n = len(self)
        if batch_size < 1:
            raise ValueError(f"DeviceDataset.batches: batch_size = {batch_size}")
        order = torch.randperm(n, device=self.device, generator=generator) if shuffle else None
        for lo in range(0, n, batch_size):
            hi = min(n, lo + batch_size)
            if order is None:
                yield self.x[lo:hi], self.y[lo:hi]
            else:
                idx = order[lo:hi]
                yield self.x.index_select(0, idx), self.y.index_select(0, idx)
