"""An independent float64 restatement of the reference's Darcy generator (the MATLAB files GRF.m, demo.m, solve_gwf.m) for the tests of
uno_amd.harness.darcy_datagen and the K23 kernels.  It shares no code with the package and is built differently on purpose:

  spline     piecewise cubics a + b t + c t^2 + d t^3 per interval as ONE dense linear system (interpolation at both ends of every
             interval, continuous first and second derivatives at the interior knots, equal cubic terms in the first two and the last
             two intervals: not-a-knot) - the package solves for second derivatives instead
  DCT        the orthonormal inverse DCT-II written from its cosine formula, entry by entry in the angle
  solve_gwf  solve_gwf.m:16-35 step by step: the (K-2)^2 x (K-2)^2 matrix assembled block by block (dense), the right-hand side taken
             column-major, a direct solve, the solution refilled row-major, the zero border, the spline back and the final transpose
  apply      one row of that matrix at a time without forming it: diagonal times p minus the four neighbour terms (the package sums
             face coefficient times difference)

Everything is torch float64 on the CPU."""
import functools
import math

import torch

F64 = torch.float64


def centres(K):
    return torch.tensor([(2 * i - 1) / (2 * K) for i in range(1, K + 1)], dtype=F64)


def nodes(K):
    return torch.tensor([i / (K - 1) for i in range(K)], dtype=F64)


def spline_matrix(xf, xt):
    """(len(xt), len(xf)): values at xt of the not-a-knot cubic splines through the unit vectors on xf; the end cubics extrapolate"""
    xf, xt = xf.to(F64), xt.to(F64)
    m = xf.numel()
    n_int = m - 1
    h = xf[1:] - xf[:-1]
    A = torch.zeros(4 * n_int, 4 * n_int, dtype=F64)
    rhs = torch.zeros(4 * n_int, m, dtype=F64)
    row = 0
    for i in range(n_int):                  # t = (x - x_i) / h_i in [0, 1]: value a at t = 0, a + b + c + d at t = 1
        A[row, 4 * i] = 1.0
        rhs[row, i] = 1.0
        row += 1
        A[row, 4 * i:4 * i + 4] = 1.0
        rhs[row, i + 1] = 1.0
        row += 1
    for i in range(n_int - 1):              # first and second derivative in x: (b + 2 c + 3 d) / h_i = b' / h_{i+1}, (2 c + 6 d) / h_i^2 = 2 c' / h_{i+1}^2
        A[row, 4 * i + 1], A[row, 4 * i + 2], A[row, 4 * i + 3], A[row, 4 * i + 5] = 1 / h[i], 2 / h[i], 3 / h[i], -1 / h[i + 1]
        row += 1
        A[row, 4 * i + 2], A[row, 4 * i + 3], A[row, 4 * i + 6] = 2 / h[i] ** 2, 6 / h[i] ** 2, -2 / h[i + 1] ** 2
        row += 1
    A[row, 3], A[row, 7] = 1 / h[0] ** 3, -1 / h[1] ** 3
    row += 1
    A[row, 4 * (n_int - 2) + 3], A[row, 4 * (n_int - 1) + 3] = 1 / h[n_int - 2] ** 3, -1 / h[n_int - 1] ** 3
    row += 1
    assert row == 4 * n_int
    coef = torch.linalg.solve(A, rhs)       # (4 n_int, m): the polynomial coefficients per unit vector
    out = torch.zeros(xt.numel(), m, dtype=F64)
    for q in range(xt.numel()):
        i = 0
        while i < n_int - 1 and xt[q] >= xf[i + 1]:
            i += 1
        t = (xt[q] - xf[i]) / h[i]
        out[q] = coef[4 * i] + t * coef[4 * i + 1] + t * t * coef[4 * i + 2] + t * t * t * coef[4 * i + 3]
    return out


@functools.lru_cache(maxsize=None)
def idct_matrix(s):
    """(cached: callers do not modify it)  D with idct2(L) = D L D^T (orthonormal inverse DCT-II): x[m] = sqrt(1/s) X[0] + sqrt(2/s) sum_{k>=1} X[k] cos(pi (2 m + 1) k / (2 s))"""
    D = torch.zeros(s, s, dtype=F64)
    for m in range(s):
        for k in range(s):
            D[m, k] = (math.sqrt(1.0 / s) if k == 0 else math.sqrt(2.0 / s)) * math.cos(math.pi * (2 * m + 1) * k / (2.0 * s))
    return D


def grf(alpha, tau, xi):
    """GRF.m:13-21 for a given xi (s, s)"""
    s = xi.shape[-1]
    k = torch.arange(s, dtype=F64)
    K1, K2 = torch.meshgrid(k, k, indexing="xy")
    coef = tau ** (alpha - 1) * (math.pi ** 2 * (K1 ** 2 + K2 ** 2) + tau ** 2) ** (-alpha / 2)
    L = s * coef * xi.to(F64)
    L[0, 0] = 0.0
    D = idct_matrix(s)
    return D @ L @ D.T


def to_nodes(v):
    """solve_gwf.m:8-12 for one plane (K, K): rows are y, columns are x, the same spline along both"""
    K = v.shape[-1]
    S = spline_matrix(centres(K), nodes(K))
    return S @ v.to(F64) @ S.T


def assemble(c):
    """solve_gwf.m:16-32: A ((K-2)^2, (K-2)^2) dense from the NODAL coefficient c (K, K); block (j, j) belongs to column j of c"""
    K = c.shape[-1]
    n = K - 2
    A = torch.zeros(n * n, n * n, dtype=F64)
    for j in range(1, K - 1):               # 0-based column of c; block j - 1
        o = (j - 1) * n
        for i in range(1, K - 1):
            r = o + i - 1
            A[r, r] = ((c[i - 1, j] + c[i, j]) / 2 + (c[i + 1, j] + c[i, j]) / 2 + (c[i, j - 1] + c[i, j]) / 2 + (c[i, j + 1] + c[i, j]) / 2)
            if i < K - 2:
                A[r, r + 1] = A[r + 1, r] = -(c[i, j] + c[i + 1, j]) / 2
            if j != K - 2:
                A[r, r + n] = A[r + n, r] = -(c[i, j] + c[i, j + 1]) / 2
    return A * (K - 1) ** 2


def solve_nodal(c, F):
    """solve_gwf.m:14-33 from nodal planes: (the nodal solution (K, K) in the orientation of c, A)"""
    K = c.shape[-1]
    n = K - 2
    A = assemble(c)
    rhs = F[1:K - 1, 1:K - 1].T.reshape(-1)             # F(:): column-major
    x = torch.linalg.solve(A, rhs)
    M = x.reshape(n, n)                                 # vec2mat: refilled row by row
    P = torch.zeros(K, K, dtype=F64)
    P[1:K - 1, 1:K - 1] = M
    return P, A                                         # P as solve_gwf.m:33 holds it: the transpose of the nodal field


def solve_nodal_sparse(c, F):
    """solve_nodal for grids whose dense matrix would not fit: the same entries in the same ordering as assemble, held sparse, and a
    sparse DIRECT solve (SuperLU).  Returns the nodal solution as solve_nodal does (transposed)."""
    import numpy as np
    import scipy.sparse
    import scipy.sparse.linalg
    K = c.shape[-1]
    n = K - 2
    c = c.numpy()
    rows, cols, vals = [], [], []
    for j in range(1, K - 1):
        o = (j - 1) * n
        i = np.arange(1, K - 1)
        r = o + i - 1
        rows.append(r); cols.append(r)
        vals.append((c[i - 1, j] + c[i, j]) / 2 + (c[i + 1, j] + c[i, j]) / 2 + (c[i, j - 1] + c[i, j]) / 2 + (c[i, j + 1] + c[i, j]) / 2)
        lo = -(c[i[:-1], j] + c[i[:-1] + 1, j]) / 2
        rows += [r[:-1], r[:-1] + 1]; cols += [r[:-1] + 1, r[:-1]]; vals += [lo, lo]
        if j != K - 2:
            off = -(c[i, j] + c[i, j + 1]) / 2
            rows += [r, r + n]; cols += [r + n, r]; vals += [off, off]
    A = scipy.sparse.csc_matrix((np.concatenate(vals) * (K - 1) ** 2, (np.concatenate(rows), np.concatenate(cols))), shape=(n * n, n * n))
    x = scipy.sparse.linalg.spsolve(A, F.numpy()[1:K - 1, 1:K - 1].T.reshape(-1))
    P = torch.zeros(K, K, dtype=F64)
    P[1:K - 1, 1:K - 1] = torch.from_numpy(x.reshape(n, n))
    return P, A


def solve_gwf(coef, F=None):
    """solve_gwf.m:4-37 for one plane (K, K) on the cell centres"""
    K = coef.shape[-1]
    F = torch.ones(K, K, dtype=F64) if F is None else F
    P, _ = solve_nodal(to_nodes(coef), to_nodes(F))
    S = spline_matrix(nodes(K), centres(K))
    return (S @ P @ S.T).T                              # interp2(...)'


def apply(c, p):
    """(A p) (n, n) for nodal c (K, K) and interior p (n, n), row by row of solve_gwf.m:20-27 without the matrix"""
    K = c.shape[-1]
    n = K - 2
    q = torch.zeros(K, K, dtype=F64)
    q[1:-1, 1:-1] = p
    I = slice(1, K - 1)
    c0 = c[I, I]
    fN, fS, fW, fE = (c[0:K - 2, I] + c0) / 2, (c[2:K, I] + c0) / 2, (c0 + c[I, 0:K - 2]) / 2, (c0 + c[I, 2:K]) / 2
    out = (fN + fS + fW + fE) * p - fN * q[0:K - 2, I] - fS * q[2:K, I] - fW * q[I, 0:K - 2] - fE * q[I, 2:K]
    assert out.shape == (n, n)
    return out * (K - 1) ** 2


def face_min(c):
    """the smallest face coefficient of the nodal plane c (K, K) among the faces the matrix uses"""
    K = c.shape[-1]
    I = slice(1, K - 1)
    return float(min(((c[0:K - 1, I] + c[1:K, I]) / 2).min(), ((c[I, 0:K - 1] + c[I, 1:K]) / 2).min()))
