"""uno_amd - MI355X-native spectral-convolution hot path of U-NO (ashiq24/UNO).

Package layout (only what the path needs):
  csrc/                  hand-written gfx950 kernels + the C ABI (include/uno_spectral.h)
  build.py               hipcc build of lib/libuno_spectral.so
  _native.py             ctypes binding of the C ABI
  integral_operators.py  host-side mirror of the reference's operator-block interface (the nn.Module classes), on top of
  block2d.py, spectral3d.py, pointwise.py: the autograd Functions of the 2-D / 3-D blocks and of the point-wise layers
  _param_grads.py        in-place parameter gradients: the gradient-target, per-pass and spectrum-stack records behind the layers'
                         weight-gradient calls (the one user of autograd's private entry points)
  harness/               own counterparts of the reference callers (UNO_9, Adam, LpLoss, DDP step)
"""
__version__ = "0.1.0"
