"""The Darcy-flow data generator without a GPU (uno_amd/harness/darcy_datagen.py, the uno_darcy_* entry points): the spline and DCT tables
against scipy, the random field against its formula on the same draw, the stock path (the K23 iteration in float64 torch operations)
against the checker tests/darcy_reference.py - a literal restatement of solve_gwf.m with a dense direct solve - on thresholded inputs
whose splined face coefficients are negative, the .mat file through dropin's MatReader, the CLI, and the host-side argument checks.

The solve's bound is derived: |P - P*|_2 <= |b - A P|_2 / lambda_min(A) <= 2 rtol |b|_2 / lambda_min(A); the iteration stops at a recursive
residual of rtol |b| and 2 covers its float64 drift from the true residual (below 1e-10 |b| against rtol = 1e-8)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
import darcy_cases as dc
import darcy_reference as ref

RTOL = 1e-8


@pytest.mark.parametrize("K", [8, 9, 35, 421])
def test_spline_matrices_equal_scipy_and_their_rows_sum_to_one(K):
    interpolate = pytest.importorskip("scipy.interpolate")
    import numpy as np
    from uno_amd.harness import spline_matrix
    centres, nodes = ref.centres(K), ref.nodes(K)
    for xf, xt in ((centres, nodes), (nodes, centres)):
        S = spline_matrix(xf, xt)
        want = torch.from_numpy(interpolate.CubicSpline(xf.numpy(), np.eye(K), bc_type="not-a-knot", extrapolate=True)(xt.numpy()))
        assert tuple(S.shape) == (K, K) and S.dtype == torch.float64
        assert float((S - want).abs().max()) <= 1e-12
        assert float((S.sum(dim=1) - 1).abs().max()) <= 1e-13
    assert float(nodes[0]) < float(centres[0]) and float(nodes[-1]) > float(centres[-1])        # the end nodes are extrapolated
    if K <= 35:         # the checker's own spline, built as one dense system of polynomial coefficients, agrees
        assert float((ref.spline_matrix(centres, nodes) - spline_matrix(centres, nodes)).abs().max()) <= 1e-12


@pytest.mark.parametrize("s", [8, 35, 64])
def test_dct_table_and_the_random_field_equal_idctn_of_the_formula(s):
    fft = pytest.importorskip("scipy.fft")
    from uno_amd.harness import darcy_grf
    from uno_amd.harness.darcy_datagen import dct_matrix
    g = torch.Generator().manual_seed(s)
    L = torch.randn(s, s, dtype=torch.float64, generator=g)
    D = dct_matrix(s)
    assert float((D @ L @ D.T - torch.from_numpy(fft.idctn(L.numpy(), norm="ortho"))).abs().max()) <= 1e-12
    assert float((D - ref.idct_matrix(s)).abs().max()) <= 1e-14
    alpha, tau = 2, 3
    xi = torch.randn(3, s, s, dtype=torch.float64, generator=g)
    k = torch.arange(s, dtype=torch.float64)
    coef = tau ** (alpha - 1) * (math.pi ** 2 * (k[:, None] ** 2 + k[None, :] ** 2) + tau ** 2) ** (-alpha / 2)
    Lx = s * coef * xi
    Lx[:, 0, 0] = 0
    u = darcy_grf(alpha, tau, s, xi=xi)
    assert tuple(u.shape) == (3, s, s) and u.dtype == torch.float64
    for b in range(3):
        assert float((u[b] - torch.from_numpy(fft.idctn(Lx[b].numpy(), norm="ortho"))).abs().max()) <= 1e-12
        assert float((u[b] - ref.grf(alpha, tau, xi[b])).abs().max()) <= 1e-12
    assert float(u.mean(dim=(1, 2)).abs().max()) <= 1e-12
    drawn = darcy_grf(alpha, tau, s, n=2, generator=torch.Generator().manual_seed(1))
    again = darcy_grf(alpha, tau, s, xi=torch.randn(2, s, s, dtype=torch.float64, generator=torch.Generator().manual_seed(1)))
    assert torch.equal(drawn, again)


def test_threshold():
    from uno_amd.harness import threshold
    u = torch.tensor([[-1.0, 0.0], [2.0, -0.0]], dtype=torch.float64)
    assert threshold(u).tolist() == [[4.0, 12.0], [12.0, 12.0]] and threshold(u).dtype == torch.float64
    assert threshold(u.float(), lo=3.0).tolist() == [[3.0, 12.0], [12.0, 12.0]]


@pytest.mark.parametrize("K", [9, 18, 35])
def test_stock_path_against_the_literal_restatement(K):
    from uno_amd.harness import solve_gwf
    coef, F, cn, fn = dc.thresholded(K)
    assert float((coef - coef.transpose(1, 2)).abs().max()) > 0 and float((F - F.transpose(1, 2)).abs().max()) > 0
    _, lam0, face0 = dc.direct(K)[0]
    assert face0 < 0 and lam0 > 0           # negative face coefficients, a positive definite matrix
    # the nodal solve under the derived bound
    from uno_amd.harness.darcy_datagen import _stock_solve
    P, iters, relres, status = _stock_solve(cn, fn, RTOL, 500)
    assert status.tolist() == [1, 1, 1] and bool((relres <= RTOL).all())
    for b in range(3):
        want, lam, face = dc.direct(K)[b]
        assert lam > 0
        err, bound = float((P[b] - want).norm()), 2 * RTOL * dc.interior_norm(fn[b]) / lam
        print(f"K={K} sample {b}: {int(iters[b])} iterations, smallest face {face:.3g}, lambda_min {lam:.4g}, error / bound = {err / bound:.3g}")
        assert err <= bound
    # the whole function, transfers included: the spline back has norm <= |S|_2^2 on the nodal error
    got, info = solve_gwf(coef, F, rtol=RTOL, return_info=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, K, K) and info["converged"].tolist() == [True] * 3
    S = ref.spline_matrix(ref.nodes(K), ref.centres(K))
    s2 = float(torch.linalg.matrix_norm(S, 2)) ** 2
    for b in range(3):
        want = ref.solve_gwf(coef[b], F[b])
        flipped = ref.solve_gwf(coef[b].T.contiguous(), F[b].T.contiguous())
        # a lost or an extra transposition anywhere cannot pass: the transposed problem has another answer
        assert float((flipped - want).norm() / want.norm()) > 1e-2
        assert float((flipped.T - want).norm() / want.norm()) < 1e-10          # (and the restatement itself is equivariant)
        bound = s2 * 2 * RTOL * dc.interior_norm(fn[b]) / dc.direct(K)[b][1] + 1e-13 * float(want.norm())
        assert float((got[b] - want).norm()) <= bound
    one = solve_gwf(coef[0], F[0], rtol=RTOL)
    assert tuple(one.shape) == (K, K) and torch.equal(one, got[0])
    f32 = solve_gwf(coef.float(), rtol=RTOL)
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (3, K, K)


def test_sparse_checker_has_the_dense_checkers_entries():
    pytest.importorskip("scipy")
    _, _, cn, fn = dc.thresholded(18)
    P, A = ref.solve_nodal(cn[0], fn[0])
    Ps, As = ref.solve_nodal_sparse(cn[0], fn[0])
    assert torch.equal(torch.from_numpy(As.toarray()), A) and float((P - Ps).abs().max()) <= 1e-13 * float(P.abs().max())
    p = P[1:-1, 1:-1].T.contiguous()
    assert float((ref.apply(cn[0], p) - fn[0][1:-1, 1:-1]).norm()) <= 1e-11 * dc.interior_norm(fn[0])


def test_iteration_limit_and_the_native_switch_on_the_cpu():
    from uno_amd.harness import solve_gwf
    coef, F, _, _ = dc.thresholded(18)
    with pytest.raises(RuntimeError, match=r"sample 0 did not reach.*3 iterations"):
        solve_gwf(coef, F, max_iter=3)
    p, info = solve_gwf(coef, F, max_iter=3, return_info=True)
    assert info["converged"].tolist() == [False] * 3 and info["iterations"].tolist() == [3] * 3 and bool(torch.isfinite(p).all())
    with pytest.raises(RuntimeError, match="8 ... 512"):
        solve_gwf(coef, F, native=True)
    zero, info = solve_gwf(coef, torch.zeros_like(F), return_info=True)
    assert float(zero.abs().max()) == 0 and info["iterations"].tolist() == [0] * 3 and info["converged"].tolist() == [True] * 3


@pytest.fixture(scope="module")
def lib():
    from uno_amd import build, _native
    build.build()
    return _native.lib()


def test_entry_points_are_declared_and_bound(lib):
    from uno_amd import _native
    for name in ("uno_darcy_ws_bytes", "uno_darcy_table_pitch", "uno_darcy_transform", "uno_darcy_apply", "uno_darcy_solve"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.uno_abi_version() == _native.ABI_VERSION == 14
    assert _native.DARCY_SIZES == (8, 512)
    hdr = open(os.path.join(ROOT, "include", "uno_spectral.h")).read()
    assert "#define UNO_SPECTRAL_ABI_VERSION 14" in hdr and "WITHOUT an ABI bump" in hdr


def test_argument_errors_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    r = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    err = lib.uno_last_error
    solve, apply_, transform = lib.uno_darcy_solve, lib.uno_darcy_apply, lib.uno_darcy_transform
    good = [p, q, r, p, p, p, p]
    for k in range(7):
        args = list(good)
        args[k] = nul
        assert solve(*args, 1, 35, 1e-10, 500, 8, None) < 0 and b"null" in err() and b"uno_darcy_solve" in err(), k
    for K in (7, 513, 0, -35):
        assert solve(*good, 1, K, 1e-10, 500, 8, None) < 0 and b"8 ... 512" in err(), K
        assert apply_(p, q, r, 1, K, None) < 0 and b"8 ... 512" in err(), K
    assert solve(*good, -1, 35, 1e-10, 500, 8, None) < 0 and b"batch" in err()
    for rtol in (0.0, -1e-3, float("nan"), float("inf")):
        assert solve(*good, 1, 35, rtol, 500, 8, None) < 0 and b"rtol" in err(), rtol
    for mi in (0, -1):
        assert solve(*good, 1, 35, 1e-10, mi, 8, None) < 0 and b"max_iter" in err()
    assert solve(*good, 1, 35, 1e-10, 500, 0, None) < 0 and b"check_every" in err()
    assert solve(p, q, p, p, p, p, p, 1, 35, 1e-10, 500, 8, None) < 0 and b"alias" in err()
    assert solve(nul, nul, nul, nul, nul, nul, nul, 0, 35, 1e-10, 500, 8, None) == 0          # an empty batch: nothing to do, nothing touched
    assert apply_(nul, q, r, 1, 35, None) < 0 and b"null" in err()
    assert apply_(p, q, q, 1, 35, None) < 0 and b"alias" in err()
    assert apply_(p, q, r, -1, 35, None) < 0 and b"batch" in err()
    assert apply_(nul, nul, nul, 0, 35, None) == 0
    assert transform(nul, p, q, r, nul, 1, 35, 0, None) < 0 and b"null" in err()
    assert transform(p, q, q, r, nul, 1, 35, 0, None) < 0 and b"different" in err()
    for N in (0, 513, -1):
        assert transform(p, q, r, p, nul, 1, N, 1, None) < 0 and b"1 ... 512" in err(), N
    assert transform(p, q, r, p, nul, -1, 35, 1, None) < 0 and b"batch" in err()
    assert transform(nul, nul, nul, nul, nul, 0, 35, 1, None) == 0


def test_workspace_size_is_positive_and_monotone(lib):
    for K in (8, 9, 35, 421, 512):
        prev = 0
        for B in (1, 2, 3, 16, 17):
            b = lib.uno_darcy_ws_bytes(B, K)
            assert b > prev and b >= 48 * B * (K - 2) ** 2
            prev = b
    for B in (1, 16):
        sizes = [lib.uno_darcy_ws_bytes(B, K) for K in range(8, 513)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.uno_darcy_ws_bytes(65535, 512) > 2 ** 32                               # 64-bit
    assert lib.uno_darcy_ws_bytes(1, 7) == 0 and lib.uno_darcy_ws_bytes(1, 513) == 0 and lib.uno_darcy_ws_bytes(-1, 35) == 0
    assert [lib.uno_darcy_table_pitch(N) for N in (0, 1, 6, 64, 65, 512, 513)] == [0, 64, 64, 64, 128, 512, 0]


def test_bindings_refuse_cpu_tensors_and_name_the_sizes(lib):
    from uno_amd import _native
    z = torch.zeros(1, 35, 35, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="HIP device"):
        _native.darcy_solve(z, z)
    with pytest.raises(RuntimeError, match="HIP device"):
        _native.darcy_apply(z, torch.zeros(1, 33, 33, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device"):
        _native.darcy_transform(_native.darcy_table(torch.eye(35, dtype=torch.float64)), z)
    assert tuple(_native.darcy_table(torch.eye(35)).shape) == (64, 64)
    assert _native.darcy_supported(8) and _native.darcy_supported(512) and not _native.darcy_supported(7) and not _native.darcy_supported(513)


def _load_data_darcy(reader, r, ntrain, ntest):
    """data_load_darcy.py:27-39 restated: sub-sample by r, keep the first ntrain and the last ntest samples, add the channel axis"""
    s = int(((421 - 1) / r) + 1)
    x_train = reader.read_field("coeff")[:ntrain, ::r, ::r][:, :s, :s]
    y_train = reader.read_field("sol")[:ntrain, ::r, ::r][:, :s, :s]
    x_test = reader.read_field("coeff")[-ntest:, ::r, ::r][:, :s, :s]
    y_test = reader.read_field("sol")[-ntest:, ::r, ::r][:, :s, :s]
    return x_train.reshape(ntrain, s, s, 1), y_train, x_test.reshape(ntest, s, s, 1), y_test


def test_dataset_at_421_through_the_mat_reader(tmp_path):
    pytest.importorskip("scipy")
    from uno_amd.harness import generate_darcy_dataset
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from utilities3 import MatReader
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    path = str(tmp_path / "darcy.mat")
    coeff, sol = generate_darcy_dataset(path, n_samples=2, s=421, bsize=1, seed=3, device="cpu")       # (bsize 1: two batches)
    assert coeff.shape == sol.shape == (2, 421, 421) and coeff.dtype.name == sol.dtype.name == "float32"
    assert set(torch.from_numpy(coeff).unique().tolist()) == {4.0, 12.0}
    assert (coeff[0] != coeff[1]).any() and float(sol.min()) >= -1e-6 and float(sol.max()) > 1e-3        # (f = 1: the solution is positive)
    x_train, y_train, x_test, y_test = _load_data_darcy(MatReader(path), 2, 1, 1)
    assert tuple(x_train.shape) == (1, 211, 211, 1) and tuple(y_train.shape) == (1, 211, 211) and x_train.dtype == y_train.dtype == torch.float32
    assert torch.equal(x_train[0, :, :, 0], torch.from_numpy(coeff[0, ::2, ::2])) and torch.equal(y_train[0], torch.from_numpy(sol[0, ::2, ::2]))
    assert torch.equal(x_test[0, :, :, 0], torch.from_numpy(coeff[1, ::2, ::2])) and torch.equal(y_test[0], torch.from_numpy(sol[1, ::2, ::2]))


def test_cli_smoke_and_a_ragged_last_batch(tmp_path):
    io = pytest.importorskip("scipy.io")
    path = str(tmp_path / "cli.mat")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "uno_amd.harness.darcy_datagen", "--out", path, "--samples", "5", "--size", "35", "--bsize", "2", "--lo", "3",
                        "--seed", "1", "--device", "cpu"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "wrote 5 samples" in r.stdout
    data = io.loadmat(path)
    assert data["coeff"].shape == (5, 35, 35) and data["sol"].shape == (5, 35, 35) and data["sol"].dtype.name == "float32"
    assert set(torch.from_numpy(data["coeff"]).unique().tolist()) == {3.0, 12.0}
    from uno_amd.harness import generate_darcy_dataset
    coeff, sol = generate_darcy_dataset(str(tmp_path / "l.mat"), n_samples=3, s=18, kind="lognorm", bsize=2, seed=2, device="cpu")
    assert coeff.shape == (3, 18, 18) and float(coeff.min()) > 0 and len(torch.from_numpy(coeff).unique()) > 100
    with pytest.raises(ValueError, match="kind"):
        generate_darcy_dataset(str(tmp_path / "x.mat"), n_samples=1, s=18, kind="other", device="cpu")
