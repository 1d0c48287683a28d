"""The Sobolev loss off the GPU: harness.spectra.sobolev_weights and the stock-op path of harness.losses.sobolev_rel / HsLoss against the
float64 definition over the full spectrum (tests/sobolev_reference.py), the closed-form gradient, the layouts, the argument checks of the
K25 entry points (which return before touching a device), and `fit --loss` on the CPU (the models get the oracle's operator blocks, as
tests/test_fit_cpu.py builds them: the spectral layers have no CPU path in the product)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import sobolev_reference as ref

from uno_amd.harness import HsLoss, lp_loss_rel_sum, sobolev_rel, sobolev_weights

GRIDS = [(8, 9), (9, 9), (16, 16), (21, 16)]


def frames(B, T, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * H + W)
    return torch.randn(B, T, H, W, generator=g, dtype=torch.float64), torch.randn(B, T, H, W, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("H,W", GRIDS)
def test_weights_against_the_brute_force_weight(H, W):
    r, c = np.minimum(np.arange(H), H - np.arange(H)), np.minimum(np.arange(W), W - np.arange(W))
    for k, a in ((0, None), (1, None), (2, None), (1, 0.5), (2, (0.5, 0.25)), (3, None)):
        w2 = sobolev_weights(H, W, k, a)
        assert w2.dtype == torch.float64 and w2.shape == (H // 2 + 1, W // 2 + 1)
        assert np.array_equal(w2.numpy()[r][:, c], ref.weight_full(H, W, k, a))       # every mode (ky, kx) takes w2[|ky|][|kx|]
    assert torch.equal(sobolev_weights(H, W, 0), torch.ones(H // 2 + 1, W // 2 + 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        sobolev_weights(H, W, 2, (1.0,))


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("H,W", GRIDS)
def test_stock_path_against_the_definition(H, W, k):
    x, y = frames(2, 3, H, W)
    for per_frame in (False, True):
        got = sobolev_rel(x, y, "bthw", k=k, per_frame=per_frame)
        want = ref.ratio_f64(x.numpy(), y.numpy(), k, per_frame=per_frame)
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    a = (0.5, 0.25)[:k]
    got = sobolev_rel(x, y, "bthw", k=k, a=a)
    assert np.abs(got.numpy() - ref.ratio_f64(x.numpy(), y.numpy(), k, a)).max() <= 1e-12
    assert sobolev_rel(x, y, "bthw", k=k, native=False).equal(sobolev_rel(x, y, "bthw", k=k))
    with pytest.raises(RuntimeError, match="on cpu"):
        sobolev_rel(x, y, "bthw", k=k, native=True)


@pytest.mark.parametrize("H,W", GRIDS)
def test_order_zero_is_the_relative_l2_of_the_reference(H, W):
    x, y = frames(3, 2, H, W)
    got = HsLoss(k=0, layout="bthw", size_average=False)(x, y)
    assert abs(float(got) - float(lp_loss_rel_sum(x, y))) <= 1e-12 * float(got)
    assert abs(float(HsLoss(k=0, layout="bthw")(x, y)) - float(got) / 3) <= 1e-12


def test_gradcheck_and_the_closed_form_gradient():
    x, y = frames(2, 2, 8, 9, seed=3)
    for k in (0, 1, 2):
        for per_frame in (False, True):
            xg = x.clone().requires_grad_(True)
            assert torch.autograd.gradcheck(lambda t: sobolev_rel(t, y, "bthw", k=k, per_frame=per_frame), (xg,))
            g = torch.rand((2, 2) if per_frame else (2,), dtype=torch.float64, generator=torch.Generator().manual_seed(k)) + 0.5
            (sobolev_rel(xg, y, "bthw", k=k, per_frame=per_frame) * g).sum().backward()
            want = ref.grad_f64(x.numpy(), y.numpy(), g.numpy(), k, per_frame=per_frame)
            assert np.abs(xg.grad.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # no gradient where the prediction equals the target (num == 0) would be 0 / 0: the stock path follows torch.sqrt there; the
    # native rule (zero) is tested on the device


def test_layouts_and_a_subsampled_view():
    g = torch.Generator().manual_seed(5)
    B, T, H, W = 2, 3, 9, 10
    big = torch.randn(B, 2 * H, 2 * W, T, generator=g, dtype=torch.float64)
    y = torch.randn(B, T, H, W, generator=g, dtype=torch.float64)
    x_bhwt = big[:, ::2, ::2]                                                 # (B, H, W, T) view
    x_bthw = x_bhwt.permute(0, 3, 1, 2).contiguous()
    want = ref.ratio_f64(x_bthw.numpy(), y.numpy(), 1, per_frame=True)
    assert np.abs(sobolev_rel(x_bthw, y, "bthw", per_frame=True).numpy() - want).max() <= 1e-12
    assert np.abs(sobolev_rel(x_bhwt, y.permute(0, 2, 3, 1), "bhwt", per_frame=True).numpy() - want).max() <= 1e-12
    one = sobolev_rel(x_bhwt[..., 1], y[:, 1], "bhw")
    assert one.shape == (B,) and np.abs(one.numpy() - want[:, 1]).max() <= 1e-12
    assert sobolev_rel(x_bhwt[..., 1], y[:, 1], "bhw", per_frame=True).shape == (B,)
    with pytest.raises(ValueError):
        sobolev_rel(x_bthw, y, "bhw")
    with pytest.raises(ValueError):
        sobolev_rel(x_bthw, y, "btwh")
    with pytest.raises(ValueError):
        sobolev_rel(x_bthw, y[:, :2], "bthw")
    empty = sobolev_rel(torch.zeros(0, 3, 8, 8), torch.zeros(0, 3, 8, 8), "bthw", per_frame=True)
    assert empty.shape == (0, 3)


def test_entry_points_check_their_arguments_without_a_device():
    from uno_amd import _native
    L = _native.lib()
    assert {"uno_sobolev_ws_bytes", "uno_sobolev_forward", "uno_sobolev_backward"} <= set(_native.EXPORTED_SYMBOLS)
    assert L.uno_abi_version() == 14
    nul, one = ctypes.c_void_p(0), ctypes.c_void_p(64)                         # `one`: never dereferenced - every call returns before a launch

    def fwd(B=1, T=1, H=8, W=8, x=one, w2=one, xs=(64, 64, 8, 1), ys=(64, 64, 8, 1), per_frame=0):
        return L.uno_sobolev_forward(x, *xs, one, *ys, w2, one, one, one, nul, one, B, T, H, W, per_frame, None)

    def bwd(B=1, T=1, H=8, W=8, z=one, gs=(64, 64, 8, 1), per_row=0):
        return L.uno_sobolev_backward(z, one, one, per_row, 1.0, 0, one, *gs, B, T, H, W, None)

    def err():
        return L.uno_last_error().decode()
    assert fwd(x=nul) == -1 and "null pointer" in err()
    assert fwd(w2=nul) == -1 and "null pointer" in err()
    assert bwd(z=nul) == -1 and "null pointer" in err()
    for bad in (dict(H=7), dict(H=513), dict(W=7), dict(W=513), dict(T=0), dict(B=-1)):
        assert fwd(**bad) == -1 and "bad sizes" in err() and "512" in err()
        assert bwd(**bad) == -1 and "bad sizes" in err()
    assert fwd(xs=(64, 64, -8, 1)) == -1 and "negative" in err()
    assert fwd(ys=(64, -64, 8, 1)) == -1 and "negative" in err()
    assert bwd(gs=(64, 64, 8, -1)) == -1 and "negative" in err()
    assert fwd(per_frame=2) == -1 and bwd(per_row=2) == -1
    assert fwd(B=0, x=nul, w2=nul) == 0 and bwd(B=0, z=nul) == 0              # nothing to do: no pointer is looked at
    assert L.uno_sobolev_ws_bytes(2, 3, 64, 32) == 8 * 2 * 3 * 2               # (num, den) per frame and band of 16 half-spectrum columns
    assert L.uno_sobolev_ws_bytes(2, 3, 512, 512) == 8 * 2 * 3 * 17
    for bad in ((2, 3, 7, 32), (2, 3, 64, 513), (0, 3, 64, 32), (2, 0, 64, 32)):
        assert L.uno_sobolev_ws_bytes(*bad) == 0


def test_default_dispatch_follows_the_measurements():
    """profiles/sobolev_loss_time.txt: the shapes at which the kernel's forward + backward measured faster than stock ops, and those at
    which it did not"""
    from uno_amd.harness.losses import sobolev_native_default
    faster = [(32, 1, 64, 64), (8, 20, 64, 64), (16, 1, 128, 128), (8, 20, 128, 128), (8, 20, 85, 85), (16, 1, 256, 256)]
    slower = [(4, 20, 256, 256), (4, 1, 421, 421), (32, 1, 421, 421), (4, 1, 512, 512)]
    assert all(sobolev_native_default(*s) for s in faster) and not any(sobolev_native_default(*s) for s in slower)
    # a 2 % win between two losses at the same grid, and a tie (0.91 and 1.03 of the stock time in two runs): not kept
    assert not sobolev_native_default(16, 1, 421, 421) and not sobolev_native_default(2, 20, 256, 256)


# --------------------------------------------------------------------------------------------------------------------- fit --loss
def _oracle_models(monkeypatch):
    """fit.main builds its model through fit._model: on the CPU with the oracle's operator blocks"""
    from oracle import spectral_oracle as so
    from uno_amd.harness import fit, models

    def build(args, default_cls):
        kw = {"pad": args.pad} if args.pad is not None else {}
        return getattr(models, args.model or default_cls)(args.in_width, args.width, block_cls=so.OracleOperatorBlock2d, **kw)
    monkeypatch.setattr(fit, "_model", build)
    return fit


def _figures(rec):
    return [(e.train, e.val) for e in rec.epochs] + [rec.test, rec.best_val]


def test_fit_darcy_loss_flag_on_the_cpu(tmp_path, monkeypatch):
    scipy_io = pytest.importorskip("scipy.io")
    fit = _oracle_models(monkeypatch)
    g = torch.Generator().manual_seed(41)
    data = str(tmp_path / "darcy.mat")
    scipy_io.savemat(data, {"coeff": torch.rand(4, 72, 72, generator=g).numpy(), "sol": torch.rand(4, 72, 72, generator=g).numpy()})

    def run(name, *extra):
        out = str(tmp_path / f"{name}.pt")
        rec = fit.main(["darcy", "--data", data, "--width", "4", "--pad", "5", "--ntrain", "2", "--nval", "1", "--ntest", "1", "--batch-size", "2",
                        "--epochs", "1", "--seed", "7", "--device", "cpu", "--out", out, *extra])
        with open(out + ".json") as f:
            return rec, json.load(f)
    plain, rec_plain = run("plain")
    l2, rec_l2 = run("l2", "--loss", "l2")
    assert _figures(l2) == _figures(plain) and rec_l2 == rec_plain and rec_plain["loss"] == "l2" and "hs_a" not in rec_plain
    h1, rec_h1 = run("h1", "--loss", "h1", "--hs-a", "0.5")
    assert rec_h1["loss"] == "h1" and rec_h1["hs_a"] == [0.5]
    assert h1.epochs[0].train != plain.epochs[0].train and np.isfinite(h1.epochs[0].train)      # the objective changed ...
    assert h1.epochs[0].val != plain.epochs[0].val and 0 < h1.test[0] < 10                       # ... the figures are still relative L2
    with pytest.raises(SystemExit):
        run("bad", "--loss", "h2", "--hs-a", "0.5")
    with pytest.raises(SystemExit):
        run("bad", "--hs-a", "0.5")


def test_fit_ns2d_h1_takes_the_window_rollout_on_the_cpu(tmp_path, monkeypatch):
    scipy_io = pytest.importorskip("scipy.io")
    fit = _oracle_models(monkeypatch)
    from uno_amd.harness import ns2d_rollout_loss
    data = str(tmp_path / "ns.mat")
    scipy_io.savemat(data, {"u0": torch.randn(3, 64, 64, 12, generator=torch.Generator().manual_seed(42)).numpy()})
    out = str(tmp_path / "ns2d.pt")
    rec = fit.main(["ns2d", "--data", data, "--width", "4", "--size", "64", "--gen-batch", "3", "--t-in", "10", "--t-f", "2", "--ntrain", "1",
                    "--nval", "1", "--ntest", "1", "--batch-size", "1", "--epochs", "1", "--seed", "7", "--device", "cpu", "--loss", "h1", "--out", out])
    with open(out + ".json") as f:
        assert json.load(f)["loss"] == "h1"
    assert np.isfinite(rec.epochs[0].train) and len(rec.test) == 2
    with pytest.raises(ValueError, match="native=True conflict"):
        ns2d_rollout_loss(None, None, torch.zeros(1, 8, 8, 2), 2, native=True, loss=HsLoss(layout="bhwt"))
