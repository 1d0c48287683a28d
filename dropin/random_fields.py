"""``from random_fields import GaussianRF`` (the import of the reference's ns_datagen.py:3) -> uno_amd/harness/datagen.py: the 2-D
Gaussian random field of random_fields-2.py on torch.fft (its torch.ifft call is gone from PyTorch since 1.8)."""
from uno_amd.harness.datagen import GaussianRF

__all__ = ["GaussianRF"]
