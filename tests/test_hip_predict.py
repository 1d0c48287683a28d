"""The predict stage (uno_amd/harness/predict.py) on the MI355X: uno_rollout_advance without ground truth (K18's no-sums form), the
free-running NS-2D roll-out built on it, models at grids other than their design grid, and the command lines fit -> predict end to end.

Kernel level: the no-sums call must leave the window and `pred` with the bits the with-target call leaves on the same inputs (the
with-target form is held against float64 and the reference's concatenation by tests/test_hip_rollout.py); no tolerance.

Other resolutions: the product model on the device against the same weights on the oracle's blocks on the host, at the bounds the
project holds the same comparison to at the design grid - TOL_PRED of tests/test_harness_ns2d_models.py (1e-5) for the 2-D models, of
tests/test_hip_ns3d_models.py (1e-4) for the 3-D one.  Measured on the MI355X (printed per case): 1.2e-7 for UNO(14, 4) at 96^2, 2.3e-7 /
2.0e-7 for UNO_9(3, 8, pad=5) at 85^2 / 86^2, 1.0e-6 for Uno3D_T20(6, 2, pad=3) at 80^2 x 10 (conv8 on the any-grid family).

End to end: the mean of predict's per-sample errors against the figure fit's test pass printed, at RTOL_PRINTED of tests/dropin_loops.py
(the same kernels on the same samples and weights; the batch composition may differ).  Measured: predict's means and fit's figures were
the same floats in all three loops."""
import ctypes
import json

import numpy as np
import pytest
import torch

import dropin_loops
from conftest import rel_err
from dropin_loops import RTOL_PRINTED
from oracle import spectral_oracle as so

pytestmark = pytest.mark.gpu
TOL_PRED_2D, TOL_PRED_3D = 1e-5, 1e-4


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- K18 without sums
B_, T_, GUARD = 3, 4, 64
# P: 35 (P % 4 != 0: the 4-byte path) and 64 (16-byte lanes) as one chunk; 4100: five chunks, the last of one 16-byte lane
K18_CASES = [(P, T_in, extra, shift, with_pred) for P in (35, 64, 4100) for T_in in (1, 2, 5, 9) for extra in (0, 4) for shift in (0, 1)
             for with_pred in ((True, False) if shift else (True,))]


def nan_pred(B, T, P):
    """(the buffer: pred and a guard band after it, all NaN; pred (B, T, P), a view of its head)"""
    buf = torch.full((B * T * P + GUARD,), float("nan"), device=dev())
    return buf, buf[:B * T * P].view(B, T, P)


def test_no_sums_form_leaves_the_bits_of_the_with_target_call():
    """every case in one test (each is two launches): P, T_in below / at / past the four-frame unrolled loop, with and without feature
    channels, shift 0 / 1, pred given / None; step t = 2 of T = 4.  Only slice t of pred may change; the guard band stays NaN."""
    from uno_amd import _native
    g = torch.Generator().manual_seed(18)
    t = 2
    for P, T_in, extra, shift, with_pred in K18_CASES:
        C = T_in + extra
        window = torch.randn(B_, C, P, generator=g).to(dev())
        frame = torch.randn(B_, P, generator=g).to(dev())
        target = torch.randn(B_, T_, P, generator=g).to(dev())
        wa, wb = window.clone(), window.clone()
        (bufa, pa), (bufb, pb) = nan_pred(B_, T_, P), nan_pred(B_, T_, P)
        _native.rollout_advance(wa, frame, target, pa if with_pred else None, _native.rollout_ws(B_, P, T_, dev()), T_in, t, shift)
        _native.rollout_advance(wb, frame, None, pb if with_pred else None, None, T_in, t, shift)
        case = (P, T_in, C, shift, with_pred)
        assert bits(wa, wb), case
        assert bits(bufa, bufb), case
        want = torch.full_like(bufb, float("nan"))
        if with_pred:
            want[:B_ * T_ * P].view(B_, T_, P)[:, t] = frame
        assert bits(bufb, want), case
        if extra:
            assert bits(wb[:, T_in:], window[:, T_in:]), case              # the feature channels are never touched
        if not shift:
            assert bits(wb, window), case


def test_no_sums_form_takes_more_than_256_steps():
    from uno_amd import _native
    g = torch.Generator().manual_seed(19)
    P, T = 35, 300
    window, frame = torch.randn(1, 3, P, generator=g).to(dev()), torch.randn(1, P, generator=g).to(dev())
    buf, pred = nan_pred(1, T, P)
    before = window.clone()
    _native.rollout_advance(window, frame, None, pred, None, 2, T - 1, True)
    want = torch.full_like(buf, float("nan"))
    want[(T - 1) * P:T * P] = frame[0]
    assert bits(buf, want)
    assert bits(window, torch.stack((before[0, 1], frame[0], before[0, 2]))[None])
    with pytest.raises(RuntimeError, match="at most 256"):                  # the cap stays where a workspace is
        _native.rollout_advance(window, frame, torch.zeros(1, T, P, device=dev()), pred, torch.empty(8 * 300, dtype=torch.uint8, device=dev()),
                                2, 0, True)


def test_no_sums_form_refusals_and_the_empty_batch():
    from uno_amd import _native
    P = 16
    window, frame, pred = torch.zeros(2, 3, P, device=dev()), torch.zeros(2, P, device=dev()), torch.zeros(2, 4, P, device=dev())
    with pytest.raises(RuntimeError, match="a workspace without a target"):
        _native.rollout_advance(window, frame, None, pred, _native.rollout_ws(2, P, 4, dev()), 2, 0, True)
    with pytest.raises(RuntimeError, match="a target without a workspace"):
        _native.rollout_advance(window, frame, pred.clone(), pred, None, 2, 0, True)
    with pytest.raises(RuntimeError, match="neither pred nor shift"):
        _native.rollout_advance(window, frame, None, None, None, 2, 0, False)
    # ... and the entry point's own refusals, below the binding's
    L = _native.lib()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    null = ctypes.c_void_p(0)
    ws = _native.rollout_ws(2, P, 4, dev())
    for args, words in (((ptr(window), ptr(frame), null, ptr(pred), ptr(ws), 2, 3, 2, P, 4, 0, 1, null), b"target and ws go together"),
                        ((ptr(window), ptr(frame), ptr(pred), null, null, 2, 3, 2, P, 4, 0, 1, null), b"target and ws go together"),
                        ((ptr(window), ptr(frame), null, null, null, 2, 3, 2, P, 4, 0, 0, null), b"pred or shift must ask for something"),
                        ((ptr(window), ptr(frame), null, ptr(pred), null, 2, 3, 2, P, 4, 4, 1, null), b"bad sizes")):
        assert L.uno_rollout_advance(*args) == -1 and words in L.uno_last_error(), words
    # B == 0: returns before any pointer is looked at or anything is launched
    empty = torch.zeros(0, 3, P, device=dev())
    _native.rollout_advance(empty, torch.zeros(0, P, device=dev()), None, torch.zeros(0, 4, P, device=dev()), None, 2, 0, True)
    assert L.uno_rollout_advance(null, null, null, null, null, 0, 3, 2, P, 300, 299, 1, null) == 0
    torch.cuda.synchronize()
    assert float(window.abs().sum()) == 0 and float(pred.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------- free-running roll-out
@pytest.fixture(scope="module")
def ns2d():
    """the recorded tiny NS-2D configuration (UNO(14, 4), 64^2, T_in 10, T_f 2) with five seeded samples: batches of 2, 2 and 1"""
    from uno_amd.harness import models
    cfg = dropin_loops.record()["loops"]["ns2d"]
    model = dropin_loops.build_model(cfg, models).to(dev()).eval()
    g = torch.Generator().manual_seed(int(cfg["data_seed"]))
    S, T_in, T_f = int(cfg["x_shape"][1]), int(cfg["x_shape"][3]), int(cfg["T_f"])
    xx, yy = torch.randn(5, S, S, T_in, generator=g).to(dev()), torch.randn(5, S, S, T_f, generator=g).to(dev())
    return model, xx, yy, T_f


def test_rollout_with_targets_is_ns2d_rollout_errors_bit_for_bit(ns2d):
    from uno_amd.harness import Predictor, ns2d_rollout_errors
    model, xx, yy, T_f = ns2d
    r = Predictor(model, batch_size=2).ns2d(xx, T_f, yy)
    assert r.pred.shape == (5, 64, 64, T_f) and r.err_step.shape == (5, T_f) and r.err_full.shape == (5,)
    with torch.no_grad():
        for lo, hi in ((0, 2), (2, 4), (4, 5)):
            want = ns2d_rollout_errors(model, xx[lo:hi], yy[lo:hi], T_f, return_pred=True)
            assert bits(r.pred[lo:hi], want.pred.cpu())
            assert bits(r.err_step[lo:hi], want.errors.per_step.cpu()) and bits(r.err_full[lo:hi], want.errors.full.cpu())


def test_rollout_without_targets_and_past_t_f(ns2d):
    """no yy: the same frames; horizon = T_f + 3: the first T_f frames are those, the rest continue from them - each is forward_cf on
    the window assembled by hand from the frames before it; errors are reported for the T_f steps that have a target"""
    from uno_amd.harness import Predictor
    model, xx, yy, T_f = ns2d
    p = Predictor(model, batch_size=2)
    measured = p.ns2d(xx, T_f, yy)
    free = p.ns2d(xx, T_f)
    assert free.err_step is None and free.err_full is None and bits(free.pred, measured.pred)
    H = T_f + 3
    longer = p.ns2d(xx, H, yy)
    assert longer.pred.shape == (5, 64, 64, H) and bits(longer.pred[..., :T_f], measured.pred)
    assert bits(longer.err_step, measured.err_step) and bits(longer.err_full, measured.err_full)
    assert bits(p.ns2d(xx, H).pred, longer.pred)
    T_in = xx.shape[-1]
    feat = model.get_grid(xx[:2].shape, dev()).permute(0, 3, 1, 2)
    with torch.no_grad():
        for lo, hi in ((0, 2), (2, 4), (4, 5)):
            frames = torch.cat((xx[lo:hi].permute(0, 3, 1, 2), longer.pred[lo:hi].permute(0, 3, 1, 2).to(dev())), dim=1)
            for t in range(T_f, H):
                z = torch.cat((frames[:, t:t + T_in], feat[:hi - lo]), dim=1).contiguous()
                assert bits(model.forward_cf(z)[:, 0], frames[:, T_in + t]), (lo, t)


def test_rollout_from_a_graph_equals_eager_bit_for_bit(ns2d):
    """batches of 2, 2 and 1: the first captures and replays, the second replays with new inputs, the third runs eagerly"""
    from uno_amd.harness import Predictor
    model, xx, yy, T_f = ns2d
    H = T_f + 1
    eager = Predictor(model, batch_size=2).ns2d(xx, H, yy)
    p = Predictor(model, batch_size=2, graph=True)
    graphed = p.ns2d(xx, H, yy)
    assert len(p._replays) == 1
    for a, b in ((eager.pred, graphed.pred), (eager.err_step, graphed.err_step), (eager.err_full, graphed.err_full)):
        assert bits(a, b)
    order = torch.tensor([2, 3, 0, 1, 4], device=dev())             # the captured graph once more, with the two full batches swapped
    again = p.ns2d(xx[order], H, yy[order])
    assert len(p._replays) == 1
    for a, b in ((eager.pred, again.pred), (eager.err_step, again.err_step), (eager.err_full, again.err_full)):
        assert bits(a[order.cpu()], b)
    free = p.ns2d(xx, H)
    assert len(p._replays) == 2 and bits(free.pred, eager.pred)


# ------------------------------------------------------------------------------------------------------------ other resolutions
def twins(name, in_width, width, seed, **kw):
    """(the product model on the device, the same weights on the oracle's blocks on the host), both through load_model"""
    from uno_amd.harness import load_model, models
    cls = getattr(models, name)
    block = so.OracleOperatorBlock3d if issubclass(cls, models.Uno3D_T20) else so.OracleOperatorBlock2d
    torch.manual_seed(seed)
    state = cls(in_width, width, block_cls=block, **kw).state_dict()
    return (load_model(state, model=name, in_width=in_width, width=width, device=dev(), **kw),
            load_model(state, model=name, in_width=in_width, width=width, block_cls=block, **kw))


def test_uno_at_96_where_it_is_designed_for_64():
    """Measured on the MI355X: 1.19e-07 (bound 1e-5)."""
    from uno_amd.harness import Predictor
    product, oracle = twins("UNO", 14, 4, 41)
    xx = torch.randn(1, 96, 96, 10, generator=torch.Generator().manual_seed(42))
    got, want = Predictor(product).ns2d(xx, 1).pred, Predictor(oracle).ns2d(xx, 1).pred
    e = rel_err(got.numpy(), want.numpy())
    print(f"[UNO(14, 4) at 96^2] product against oracle blocks: {e:.2e}")
    assert got.shape == (1, 96, 96, 1) and e < TOL_PRED_2D


@pytest.mark.parametrize("S", [85, 86])
def test_uno9_on_both_sides_of_the_padding_scale(S):
    """the padding scale ceil(S / 85) is 1 at 85 and 2 at 86 (padded grids 90 and 96).  Measured on the MI355X: 2.30e-07 at 85, 2.04e-07 at 86 (bound 1e-5)."""
    from uno_amd.harness import Predictor
    product, oracle = twins("UNO_9", 3, 8, 43, pad=5)
    x = torch.rand(1, S, S, 1, generator=torch.Generator().manual_seed(44))
    got, want = Predictor(product).darcy(x).pred, Predictor(oracle).darcy(x).pred
    e = rel_err(got.numpy(), want.numpy())
    print(f"[UNO_9(3, 8, pad=5) at {S}^2] product against oracle blocks: {e:.2e}")
    assert got.shape == (1, S, S) and e < TOL_PRED_2D


def test_uno3d_t20_at_80_runs_conv8_on_the_any_grid_kernels():
    """S = 80, T_in = 10: conv8 resamples (60, 60, 26) -> (80, 80, 26), outside the pruned-DFT range - the default model raises there,
    load_model's runs it on the any-grid family.  Measured on the MI355X: 1.01e-06 (bound 1e-4)."""
    from uno_amd.harness import Predictor, check_resolution, models
    product, oracle = twins("Uno3D_T20", 6, 2, 45, pad=3)
    assert {lp.name: lp.family for lp in check_resolution(product, 80, 10)}["conv8"] == "any"
    x = torch.randn(1, 80, 80, 10, 1, generator=torch.Generator().manual_seed(46))
    default = models.Uno3D_T20(6, 2, pad=3).to(dev()).eval()
    with pytest.raises(RuntimeError, match="outside the range of the pruned-DFT kernels"), torch.no_grad():
        default(x.to(dev()))
    got, want = Predictor(product).ns3d(x).pred, Predictor(oracle).ns3d(x).pred
    e = rel_err(got.numpy(), want.numpy())
    print(f"[Uno3D_T20(6, 2, pad=3) at 80^2 x 10] product against oracle blocks: {e:.2e}")
    assert got.shape == (1, 80, 80, 20) and e < TOL_PRED_3D


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """a tiny Darcy file (7 samples, n = 85) and a tiny NS file (7 samples, s = 64, 30 frames), from torch on the host"""
    scipy_io = pytest.importorskip("scipy.io")
    d = tmp_path_factory.mktemp("predict")
    g = torch.Generator().manual_seed(50)
    darcy, ns = str(d / "darcy.mat"), str(d / "ns.mat")
    scipy_io.savemat(darcy, {"coeff": (3 + 9 * (torch.rand(7, 85, 85, generator=g) > 0.5)).numpy().astype(np.float32),
                             "sol": torch.rand(7, 85, 85, generator=g).numpy()})
    scipy_io.savemat(ns, {"u0": torch.randn(7, 64, 64, 30, generator=g).numpy()})
    return d, darcy, ns


COUNTS = ["--ntrain", "4", "--nval", "2", "--ntest", "1"]


def fit_then_predict(loop, fit_args, predict_args, files, capsys):
    from uno_amd.harness import MatReader, fit, predict
    d = files[0]
    weights, out = str(d / f"{loop}.pt"), str(d / f"{loop}_pred.mat")
    rec = fit.main([loop, *fit_args, *COUNTS, "--batch-size", "2", "--epochs", "1", "--seed", "7", "--out", weights])
    capsys.readouterr()
    summary = predict.main([loop, "--weights", weights, *predict_args, "--split", "test", "--out", out])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["split"] == "test" and line["n"] == 1 and line["out"] == out
    ids = torch.arange(7).reshape(7, 1)
    test_cut = fit._split(ids, ids, 4, 2, 1, 7)[2][0].reshape(-1)
    reader = MatReader(out)
    assert reader.read_field("index").reshape(-1).tolist() == test_cut.tolist() == summary["index"].tolist()
    with open(weights + ".json") as f:
        assert json.load(f)["test"] == list(rec.test)
    return rec, summary, reader, weights


def test_darcy_command_lines_end_to_end(files, capsys):
    _, darcy, _ = files
    rec, summary, reader, _ = fit_then_predict("darcy", ["--data", darcy, "--width", "4", "--pad", "5"], ["--data", darcy], files, capsys)
    err = reader.read_field("err").reshape(-1)
    print(f"[darcy] predict {float(err.mean())!r}, fit's test pass {rec.test[0]!r}")
    assert reader.read_field("pred").shape == (1, 85, 85)
    assert np.allclose(float(err.mean()), rec.test[0], rtol=RTOL_PRINTED) and np.allclose(summary["err"], rec.test[0], rtol=RTOL_PRINTED)


def test_ns2d_command_lines_end_to_end_with_the_default_in_width(files, capsys):
    """no --in-width: the default must be the one UNO's four positional features need"""
    _, _, ns = files
    data = ["--data", ns, "--gen-batch", "7", "--t-f", "2"]
    rec, summary, reader, _ = fit_then_predict("ns2d", [*data, "--width", "4"], ["--data", ns], files, capsys)
    step, full = reader.read_field("err_step"), reader.read_field("err_full").reshape(-1)
    print(f"[ns2d] predict {float(step.mean())!r}, {float(full.mean())!r}; fit's test pass {rec.test!r}")
    assert reader.read_field("pred").shape == (1, 64, 64, 2) and step.shape == (1, 2)
    assert np.allclose([float(step.mean()), float(full.mean())], rec.test, rtol=RTOL_PRINTED)
    assert np.allclose([summary["err_step"], summary["err_full"]], rec.test, rtol=RTOL_PRINTED)


def test_ns3d_command_lines_end_to_end_and_at_another_size(files, capsys):
    from uno_amd.harness import predict
    _, _, ns = files
    data = ["--data", ns, "--gen-batch", "7", "--t-f", "20"]
    rec, summary, reader, weights = fit_then_predict("ns3d", [*data, "--width", "2", "--pad", "3"], ["--data", ns], files, capsys)
    step, full = reader.read_field("err_step"), reader.read_field("err_full").reshape(-1)
    assert reader.read_field("pred").shape == (1, 64, 64, 20) and step.shape == (1, 20)
    assert np.allclose([float(full.mean()), float(step.mean())], rec.test, rtol=RTOL_PRINTED)
    at80 = predict.main(["ns3d", "--weights", weights, "--data", ns, "--split", "test", "--size", "80"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["size"] == 80 and at80["result"].pred.shape == (1, 80, 80, 20) and at80["index"].tolist() == summary["index"].tolist()
    assert torch.isfinite(at80["result"].pred).all() and torch.isfinite(at80["result"].err_full).all()
    print(f"[ns3d] predict {float(full.mean())!r}, {float(step.mean())!r}; fit's test pass {rec.test!r}; at 80^2 {float(at80['result'].err_full.mean())!r}")
