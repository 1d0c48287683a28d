"""Inputs shared by tests/test_darcy_datagen_cpu.py and tests/test_hip_darcy_solver.py, built with the checker (tests/darcy_reference.py)
alone and cached: each reference is computed once and never modified.

thresholded(K): B = 3 thresholded fields (12 | 4) of GRF(2, 3, K) on the cell centres with a non-symmetric right-hand side.  The seeds were
chosen at development time so that sample 0's spline to the nodes has a NEGATIVE face coefficient while the matrix stays positive
definite; the tests assert both."""
import functools
import math

import torch

import darcy_reference as ref

SEEDS = {8: 0, 9: 12, 18: 4, 35: 2}
U64 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def thresholded(K):
    """(coef (3, K, K) on the centres, F (3, K, K) on the centres, nodal coef, nodal F), float64"""
    g = torch.Generator().manual_seed(SEEDS[K])
    xi = torch.randn(3, K, K, dtype=torch.float64, generator=g)
    u = torch.stack([ref.grf(2, 3, xi[b]) for b in range(3)])
    coef = torch.where(u >= 0, 12.0, 4.0).to(torch.float64)
    F = 1.0 + 0.5 * torch.randn(3, K, K, dtype=torch.float64, generator=g)
    return coef, F, torch.stack([ref.to_nodes(c) for c in coef]), torch.stack([ref.to_nodes(f) for f in F])


@functools.lru_cache(maxsize=None)
def direct(K):
    """per sample of thresholded(K): (the checker's nodal solution in the input's orientation, lambda_min(A), the smallest face coefficient)"""
    _, _, cn, fn = thresholded(K)
    out = []
    for b in range(3):
        P, A = ref.solve_nodal(cn[b], fn[b])
        out.append((P.T.contiguous(), float(torch.linalg.eigvalsh(A)[0]), ref.face_min(cn[b])))
    return out


@functools.lru_cache(maxsize=None)
def lognormal(K, B=3, seed=5):
    """nodal planes (coef (B, K, K) = exp of a smooth random field, F (B, K, K)) for the sizes without a dense matrix"""
    g = torch.Generator().manual_seed(seed + K)
    k = torch.arange(K, dtype=torch.float64)
    decay = 3.0 * (math.pi ** 2 * (k[:, None] ** 2 + k[None, :] ** 2) + 9.0) ** -1.0
    D = ref.idct_matrix(K)
    u = D @ (K * decay * torch.randn(B, K, K, dtype=torch.float64, generator=g)) @ D.T
    return torch.exp(u), 1.0 + 0.5 * torch.randn(B, K, K, dtype=torch.float64, generator=g)


def lambda_min_laplacian(K):
    """the smallest eigenvalue of the unit-coefficient 5-point matrix on the K-grid"""
    return (K - 1) ** 2 * 8.0 * math.sin(math.pi / (2 * (K - 1))) ** 2


def interior_norm(F):
    return float(F[1:-1, 1:-1].norm())
