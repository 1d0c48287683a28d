"""The NS-2D evaluation roll-out (reference ns_train_2d.py:86-117, 133-168) without a GPU: the stock path of
harness.ns2d_rollout_errors against the reference's own numbers (the `ns2d` case of tests/golden/harness_ns.npz: its recorded `loss` is
the sum of the per-step errors, its `pred` the two predicted frames), ns2d_evaluate's sums and mode handling, the fall-backs, and the
argument checks of uno_rollout_advance / uno_rollout_finish (no launch: as tests/test_step_errors_cpu.py)."""
import ctypes
import functools

import pytest
import torch

from conftest import Case, load_cases, rel_err
from oracle import spectral_oracle as so
from uno_amd.harness import UNO, GraphedRollout, RolloutErrors, StepErrors, ns2d_evaluate, ns2d_rollout_errors

Z, _ = load_cases("harness_ns.npz")
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def golden():
    """(model on oracle blocks, xx, yy, the case) - built once, never modified"""
    c = Case(Z, "ns2d")
    torch.manual_seed(21)
    model = UNO(14, 4, block_cls=so.OracleOperatorBlock2d)
    return model, torch.from_numpy(c.xx), torch.from_numpy(c.yy), c


def float64_errors(pred, yy):
    """the five quantities in float64 from a (B, S, S, T) prediction and target"""
    B, T = pred.shape[0], pred.shape[-1]
    p64, y64 = pred.double().reshape(B, -1, T), yy.double().reshape(B, -1, T)
    num, den = ((p64 - y64) ** 2).sum(1), (y64 ** 2).sum(1)
    per_step = num.sqrt() / den.sqrt()
    full = num.sum(1).sqrt() / den.sum(1).sqrt()
    return {"sums": torch.stack((num, den), -1), "per_step": per_step, "full": full, "step_sum": per_step.sum(), "full_sum": full.sum()}


def worst(e, want):
    out = 0.0
    for k, w in want.items():
        got = getattr(e, k).double()
        assert got.shape == w.shape, k
        out = max(out, float(((got - w).abs() / w.abs()).max()))
    return out


def test_stock_path_reproduces_the_reference_rollout():
    model, xx, yy, c = golden()
    r = ns2d_rollout_errors(model, xx, yy, T_f=2, return_pred=True)
    assert isinstance(r, RolloutErrors) and isinstance(r.errors, StepErrors)
    e = r.errors
    assert e.sums.shape == (1, 2, 2) and e.per_step.shape == (1, 2) and e.full.shape == (1,) and e.step_sum.dim() == 0 and e.full_sum.dim() == 0
    assert not any(t.requires_grad for t in e) and not r.pred.requires_grad
    d_loss = abs(float(e.step_sum) - float(c.loss)) / abs(float(c.loss))
    d_pred = rel_err(r.pred.numpy(), c.pred)
    want = float64_errors(torch.from_numpy(c.pred), yy)
    d_full = abs(float(e.full_sum) - float(want["full_sum"])) / float(want["full_sum"])
    print(f"[ns2d golden] step_sum against the recorded loss {d_loss:.2e}, pred {d_pred:.2e}, full_sum against float64 {d_full:.2e}")
    assert d_loss <= TOL and d_pred <= TOL and d_full <= TOL
    assert worst(e, want) <= TOL
    assert ns2d_rollout_errors(model, xx, yy, T_f=2).pred is None


def test_rollout_leaves_the_training_mode_alone():
    model, xx, yy, _ = golden()
    for mode in (True, False):
        model.train(mode)
        ns2d_rollout_errors(model, xx, yy, T_f=1)
        assert model.training == mode
    model.train()


def test_ns2d_evaluate_sums_the_batches_and_restores_the_mode():
    model, xx, yy, _ = golden()
    two = torch.cat((xx, xx.flip(1)), 0), torch.cat((yy, yy.flip(1)), 0)
    for T_f in (1, 2):
        parts = [ns2d_rollout_errors(model, two[0][i:i + 1], two[1][i:i + 1], T_f).errors for i in range(2)]
        model.train()
        step_total, full_total = ns2d_evaluate(model, [(two[0][:1], two[1][:1]), (two[0][1:], two[1][1:])], T_f)
        assert model.training
        assert step_total.dim() == 0 and full_total.dim() == 0 and not step_total.requires_grad
        assert abs(float(step_total) - float(parts[0].step_sum + parts[1].step_sum)) <= TOL * float(step_total)
        assert abs(float(full_total) - float(parts[0].full_sum + parts[1].full_sum)) <= TOL * float(full_total)
        # one batch of two equals two batches of one
        whole = ns2d_evaluate(model, [two], T_f)
        assert abs(float(whole[0]) - float(step_total)) <= TOL * float(step_total) and abs(float(whole[1]) - float(full_total)) <= TOL * float(full_total)
    model.eval()
    ns2d_evaluate(model, [(xx, yy)], 1)
    assert not model.training
    model.train()


def test_evaluate_restores_the_mode_when_the_model_raises():
    model, xx, yy, _ = golden()
    model.train()
    with pytest.raises(RuntimeError):
        ns2d_evaluate(model, [(xx[..., :3], yy)], 1)           # 3 + 4 input channels: fc refuses
    assert model.training


class TwoFrames(torch.nn.Module):
    """a model that predicts `step` frames from the window (no forward_cf: the stock path)"""

    def __init__(self, T_in, step, dtype):
        super().__init__()
        torch.manual_seed(3)
        self.fc = torch.nn.Linear(T_in, step, dtype=dtype)

    def forward(self, x):
        return self.fc(x)


def reference_loop(model, xx, yy, T_f, step):
    """ns_train_2d.py:141-152 -> the concatenated prediction"""
    with torch.no_grad():
        for t in range(0, T_f, step):
            im = model(xx)
            pred = im if t == 0 else torch.cat((pred, im), -1)
            xx = torch.cat((xx[..., step:], im), dim=-1)
    return pred


@pytest.mark.parametrize("step,dtype", [(2, torch.float32), (1, torch.float64), (2, torch.float64)])
def test_step_two_and_float64_take_the_stock_path(step, dtype):
    g = torch.Generator().manual_seed(4)
    xx, yy = torch.randn(2, 5, 7, 6, generator=g).to(dtype), torch.randn(2, 5, 7, 4, generator=g).to(dtype)
    model = TwoFrames(6, step, dtype)
    r = ns2d_rollout_errors(model, xx, yy, T_f=4, step=step, return_pred=True)
    assert r.pred.shape == (2, 5, 7, 4) and r.pred.dtype == dtype and r.errors.per_step.dtype == dtype
    assert torch.equal(r.pred, reference_loop(model, xx, yy, 4, step))
    assert worst(r.errors, float64_errors(r.pred, yy)) <= TOL
    with pytest.raises(RuntimeError):
        ns2d_rollout_errors(model, xx, yy, T_f=3, step=2)       # not a multiple of step
    with pytest.raises(RuntimeError):
        ns2d_rollout_errors(model, xx, yy, T_f=5, step=1)       # beyond yy


@pytest.fixture(scope="module")
def lib():
    from uno_amd import build, _native
    build.build()
    return _native.lib()


def test_argument_errors_are_reported_without_a_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    good = (1, 6, 2, 4, 3, 0, 1, None)                  # B, C, T_in, P, T, t, shift, stream
    for k in (0, 1, 2, 4):                               # window, frame, target, ws in turn; pred (3) may be null
        ptrs = [nul if i == k else p for i in range(5)]
        assert lib.uno_rollout_advance(*ptrs, *good) < 0 and b"null" in lib.uno_last_error()
    for k in range(4):                                   # ws, sums, rel, totals
        ptrs = [nul if i == k else p for i in range(4)]
        assert lib.uno_rollout_finish(*ptrs, 1, 4, 3, None) < 0 and b"null" in lib.uno_last_error()
    bad = {
        "B < 0": (-1, 6, 2, 4, 3, 0, 1, None), "P < 1": (1, 6, 2, 0, 3, 0, 1, None), "C < 1": (1, 0, 1, 4, 3, 0, 1, None),
        "T_in < 1": (1, 6, 0, 4, 3, 0, 1, None), "T_in > C": (1, 6, 7, 4, 3, 0, 1, None), "T < 1": (1, 6, 2, 4, 0, 0, 1, None),
        "t < 0": (1, 6, 2, 4, 3, -1, 1, None), "t = T": (1, 6, 2, 4, 3, 3, 1, None),
    }
    for what, args in bad.items():
        assert lib.uno_rollout_advance(p, p, p, p, p, *args) < 0 and b"bad sizes" in lib.uno_last_error(), what
    assert lib.uno_rollout_advance(p, p, p, p, p, 1, 6, 2, 4, 257, 0, 1, None) < 0 and b"at most 256" in lib.uno_last_error()
    assert lib.uno_rollout_finish(p, p, p, p, 1, 4, 257, None) < 0 and b"at most 256" in lib.uno_last_error()
    assert lib.uno_rollout_finish(p, p, p, p, 1, 0, 3, None) < 0 and b"bad sizes" in lib.uno_last_error()
    assert lib.uno_rollout_finish(p, p, p, p, -1, 4, 3, None) < 0 and b"bad sizes" in lib.uno_last_error()
    assert lib.uno_rollout_finish(p, p, p, p, 1, 4, 0, None) < 0 and b"bad sizes" in lib.uno_last_error()
    # an empty batch is a no-op that succeeds without touching the device
    assert lib.uno_rollout_advance(nul, nul, nul, nul, nul, 0, 6, 2, 4, 3, 0, 1, None) == 0
    assert lib.uno_rollout_finish(nul, nul, nul, nul, 0, 4, 3, None) == 0


def test_workspace_size_is_positive_linear_and_never_shrinks_with_the_pixel_count(lib):
    for T in (1, 3, 40, 256):
        last = 0
        for P in (1, 49, 1024, 1025, 4096, 20011, 65536, 65537, 1 << 20, 1 << 24):
            ws = lib.uno_rollout_ws_bytes(2, P, T)
            assert ws > 0 and ws % 8 == 0 and ws >= last, (T, P, ws, last)
            assert lib.uno_rollout_ws_bytes(6, P, T) == 3 * ws and ws == T * lib.uno_rollout_ws_bytes(2, P, 1)
            last = ws
    # about 1024 pixels per chunk, at most 64 chunks: a function of P alone
    chunks = {P: lib.uno_rollout_ws_bytes(1, P, 1) // 8 for P in (1, 1024, 1025, 4096, 20011, 65536, 65537, 1 << 24)}
    assert chunks == {1: 1, 1024: 1, 1025: 2, 4096: 4, 20011: 20, 65536: 64, 65537: 64, 1 << 24: 64}
    assert lib.uno_rollout_ws_bytes(0, 100, 3) == 0 and lib.uno_rollout_ws_bytes(2, 0, 3) == 0
    assert lib.uno_rollout_ws_bytes(2, 100, 0) == 0 and lib.uno_rollout_ws_bytes(2, 100, 257) == 0


def test_binding_refuses_host_tensors():
    from uno_amd import _native
    w, f, y = torch.zeros(1, 3, 4), torch.zeros(1, 4), torch.zeros(1, 2, 4)
    with pytest.raises(RuntimeError):
        _native.rollout_advance(w, f, y, None, torch.zeros(64, dtype=torch.uint8), 2, 0, True)
    with pytest.raises(RuntimeError):
        _native.rollout_finish(torch.zeros(64, dtype=torch.uint8), 1, 4, 2)


def test_graphed_rollout_refuses_host_tensors():
    """without a HIP device there is nothing to capture; with one, host tensors are not the native path - RuntimeError either way"""
    model, xx, yy, _ = golden()
    with pytest.raises(RuntimeError, match="native roll-out only" if torch.cuda.is_available() else "needs the GPU"):
        GraphedRollout(model, 2, (xx, yy))
