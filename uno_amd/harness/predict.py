"""From a weights file to predictions: what a U-NO user does right after training (the reference's notebooks do it by hand), at any
resolution the model's modes fit and for any horizon, with a command line around it:

    python -m uno_amd.harness.predict {darcy,ns2d,ns3d} --weights W.pt [--record W.pt.json | --model ... --in-width ... --width ...]
           --data FILE [--split test|val|train|all] [--sub r | --size S] [--t-in n] [--horizon H | --calls k] [--batch-size b] [--graph]
           [--out PRED.mat] [--no-pred] [--spectra]

  load_model        builds the class a checkpoint record names (harness.fit writes one beside the weights) or the caller names - weights
                    the reference's own scripts saved have no record - loads the state_dict strictly and leaves the model in eval mode;
                    3-D models on product blocks are opted into the any-grid and the wide-axis resample kernels, so a grid outside the
                    pruned-DFT range runs natively instead of raising
  check_resolution  walks the model's plan of grids for (S, T_in) BEFORE any launch: one ValueError names the first layer whose modes
                    do not fit its grids, or the first 3-D layer no native resample family takes (the reference dies there with a shape
                    error out of a slice assignment)
  Predictor         darcy / ns2d / ns3d in batches (a short last batch included) under no_grad and eval mode; with targets also the
                    per-sample relative L2 errors, taken from what the native loss kernels write per row (K20 `ratio`, K17 / K18
                    `rel`); ONE read-back per call.  ns2d is the free-running roll-out: the channels-first window moves in place and
                    the frames are recorded time-major, one K18 launch per step, with or without ground truth and past T_f.  ns3d(calls=k)
                    chains k calls: a call's last T_in output frames are the next call's input.  spectra=True adds the shell-binned
                    energy spectra (harness.spectra, K24) of every predicted frame and, where there are targets, of the true frames and
                    of the difference, computed per batch on the device into the same flat buffer as the predictions.

The runners import nothing from the oracle; `block_cls` lets a caller build a model on other blocks (the CPU tests do)."""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import NamedTuple, Optional

import torch

from ..integral_operators import OperatorBlock_3D, enable_native_resample3d_any, enable_native_resample3d_wide, pointwise_op_3D
from ..spectral3d import _resample3d_pruned_applies, resample3d_any_applies, resample3d_wide_applies
from . import models
from .data import DeviceDataset, load_darcy, load_ns
from .losses import NATIVE_STEP_ERRORS_MAX_T, _step_errors_stock, rel_l2, step_errors
from .spectra import _spectra, n_shells

MODEL_CLASSES = ("UNO_9", "UNO", "UNO_P", "UNO_S256", "Uno3D_T20", "Uno3D_T10", "Uno3D_T9", "Uno3D_T40", "Uno3D_T20_256", "Uno3D_T10_256")
_CTOR_KEYS = ("in_width", "width", "pad", "factor", "pad_both")


# ------------------------------------------------------------------------------------------------------------------------ load_model
def read_record(path) -> dict:
    """the checkpoint record harness.fit wrote beside the weights; a ValueError names what it lacks"""
    try:
        with open(path) as f:
            rec = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"checkpoint record {path}: cannot be read ({e})") from None
    return _checked_record(rec, str(path))


def _checked_record(rec, where):
    if not isinstance(rec, dict):
        raise ValueError(f"checkpoint record {where}: not a JSON object")
    for key in ("model", "ctor"):
        if key not in rec:
            raise ValueError(f"checkpoint record {where}: no \"{key}\" entry (harness.fit writes it; name the model explicitly otherwise)")
    for key in ("in_width", "width"):
        if key not in rec["ctor"]:
            raise ValueError(f"checkpoint record {where}: its \"ctor\" has no \"{key}\"")
    return rec


def _model_class(name):
    if isinstance(name, type):
        return name
    if name not in MODEL_CLASSES:
        raise ValueError(f"model {name!r}: no such class in uno_amd.harness.models ({', '.join(MODEL_CLASSES)})")
    return getattr(models, name)


def load_model(weights, record=None, *, block_cls=None, device=None, **ctor):
    """-> the model of a weights file, in eval mode.

    weights: a path torch.load reads, or a state_dict.  record: the checkpoint record (a dict, or the path of the .json harness.fit wrote);
    None: `<weights>.json` where that file exists.  Without a record the constructor is named explicitly: model= (a class of
    harness.models or its name), in_width=, width= and optionally pad=, factor=, pad_both=.  Explicit arguments beside a record must
    agree with it: a weights file built one way does not load another, and the ValueError says which argument disagrees instead of
    load_state_dict's list of shapes.  block_cls: the operator block to build on (default: the product's).  device: where the model goes."""
    where = "the record"
    if record is None and isinstance(weights, (str, os.PathLike)) and os.path.exists(str(weights) + ".json") and "model" not in ctor:
        record = str(weights) + ".json"
    if isinstance(record, (str, os.PathLike)):
        where, record = str(record), read_record(record)
    elif record is not None:
        record = _checked_record(record, where)
    unknown = sorted(set(ctor) - set(_CTOR_KEYS) - {"model"})
    if unknown:
        raise ValueError(f"load_model: unknown constructor argument(s) {unknown}; it takes model, {', '.join(_CTOR_KEYS)}")
    name = ctor.pop("model", None)
    if record is None:
        if name is None:
            raise ValueError("load_model: no checkpoint record (none given, none beside the weights) and no model= argument: a bare "
                             "state_dict does not say which class and constructor arguments it belongs to")
        kw = dict(ctor)
    else:
        recorded = record["model"]
        if name is not None and _model_class(name).__name__ != recorded:
            raise ValueError(f"load_model: model={_model_class(name).__name__} contradicts {where}, which names {recorded}")
        name = recorded
        kw = dict(record["ctor"])
        for k, v in ctor.items():
            if k in kw and kw[k] != v:
                raise ValueError(f"load_model: {k}={v!r} contradicts {where}, which holds {k}={kw[k]!r}")
            kw[k] = v
    cls = _model_class(name)
    for key in ("in_width", "width"):
        if key not in kw:
            raise ValueError(f"load_model: {cls.__name__} needs {key}= (no record supplies it)")
    if "pad_both" in kw and not issubclass(cls, models.Uno3D_T20):
        raise ValueError(f"load_model: pad_both is an argument of the 3-D models, not of {cls.__name__}")
    if block_cls is not None:
        kw["block_cls"] = block_cls
    model = cls(**kw)
    state = torch.load(weights, map_location="cpu") if isinstance(weights, (str, os.PathLike)) else weights
    model.load_state_dict(state, strict=True)
    if _on_product_blocks_3d(model):        # a grid outside the pruned-DFT kernels' range: natively, not a RuntimeError
        enable_native_resample3d_any(model)
        enable_native_resample3d_wide(model)
    if device is not None:
        model = model.to(device)
    return model.eval()


def _on_product_blocks_3d(model):
    return isinstance(model, models.Uno3D_T20) and isinstance(getattr(model, model._NAMES[-1]), OperatorBlock_3D)


# ------------------------------------------------------------------------------------------------------------------ resolution check
class LayerPlan(NamedTuple):
    """one operator block at a requested resolution"""
    name: str
    din: tuple                  # the grid it reads
    dout: tuple                 # the grid it writes
    modes: tuple
    family: Optional[str]       # 3-D product blocks: the resample kernels its point-wise layer takes ("pruned" | "any" | "wide")


def _layers(model, S, T_in):
    """[(block name, input grid, output grid)] of the model's forward pass on an S x S (x T_in) input, and its output time length"""
    if isinstance(model, models.Uno3D_T20):
        if T_in is None or T_in < 1:
            raise ValueError(f"{type(model).__name__}: the resolution check needs T_in >= 1 (got {T_in})")
        padding = int(model.pad * 0.1 * T_in)
        d3 = T_in + (2 if model.pad_both else 1) * padding
        grids, crop = model._plan(S, S, d3, padding)
        t_out = grids[-1][2] - ((2 if model.pad_both else 1) * crop if padding != 0 else 0)
        names = model._NAMES
        din = (S, S, d3)
    elif isinstance(model, models.UNO_9):
        d = S + math.ceil(S / 85) * model.padding
        names = ("conv0", "conv1", "conv2", "conv4", "conv5")
        grids, din, t_out = [(d // 2,) * 2, (d // 4,) * 2, (d // 4,) * 2, (d // 2,) * 2, (d, d)], (d, d), 1
    elif isinstance(model, models.UNO):
        d = S + 2 * model.padding
        names = tuple(f"L{i}" for i in range(len(model._BLOCKS)))
        grids, din, t_out = [tuple(g) for g in model._grids(d, d)], (d, d), 1
    else:
        raise ValueError(f"{type(model).__name__}: not a model of uno_amd.harness.models, no plan of grids to walk")
    out = []
    for name, dout in zip(names, grids):
        out.append((name, tuple(din), tuple(dout)))
        din = dout
    return out, t_out


def _resample_family(w, din, dout):
    """the kernel family pointwise_op_3D `w` takes for din -> dout, as _resample3d_kernels decides it (host predicates only), or None"""
    from .. import integral_operators as io
    if _resample3d_pruned_applies(din, dout):
        return "pruned"
    if (getattr(w, "native_any_grid", False) or io.NATIVE_RESAMPLE3D_ANY) and resample3d_any_applies(din, dout):
        return "any"
    if (getattr(w, "native_wide_grid", False) or io.NATIVE_RESAMPLE3D_WIDE) and resample3d_wide_applies(din, dout):
        return "wide"
    return None


def check_resolution(model, S, T_in=None):
    """-> [LayerPlan] of `model` on an S x S input (3-D models: S x S x T_in), touching no device.  Raises ONE ValueError that names the
    first layer whose modes do not fit its input or output grid (modes1 <= rows; on the last axis modes <= n // 2 + 1; the 3-D models'
    second axis is a full one), then the first 3-D layer on product blocks whose FFT resample no native kernel family takes."""
    S = int(S)
    who = f"{type(model).__name__} at {S} x {S}" + (f" x {T_in}" if isinstance(model, models.Uno3D_T20) else "")
    if S < 1:
        raise ValueError(f"{who}: the grid must be positive")
    layers, t_out = _layers(model, S, T_in)
    plan = []
    for name, din, dout in layers:
        conv = getattr(model, name).conv
        modes = tuple(int(getattr(conv, f"modes{k + 1}")) for k in range(len(din)))
        last = len(din) - 1
        for axis, m in enumerate(modes):
            for role, grid in (("input", din), ("output", dout)):
                room = grid[axis] // 2 + 1 if axis == last else grid[axis]
                if not 1 <= m <= room:
                    kind = f"{m} modes on axis {axis + 1}, which need a grid of at least {2 * (m - 1) if axis == last else m} points"
                    raise ValueError(f"{who}: layer {name} keeps {kind}; its {role} grid {grid} has {grid[axis]} "
                                     f"(the layer maps {din} -> {dout}); choose a larger grid")
        plan.append(LayerPlan(name, din, dout, modes, None))
    if t_out < 1:
        raise ValueError(f"{who}: the time axis of {layers[-1][2][2]} points is cropped to {t_out}: no output frame is left")
    if _on_product_blocks_3d(model):
        for i, lp in enumerate(plan):
            w = getattr(model, lp.name).w
            if not isinstance(w, pointwise_op_3D):
                continue
            family = _resample_family(w, lp.din, lp.dout)
            if family is None:
                raise ValueError(f"{who}: layer {lp.name} resamples {lp.din} -> {lp.dout}, which no native kernel family takes (pruned-DFT: "
                                 "even kept-row counts up to 80 / 48 and planes up to 1792 elements; any-grid: axes of 2 ... 128; wide-axis: "
                                 "leading axes of 2 ... 256 and a last axis of 2 ... 64 - the latter two where the layer is opted in, as "
                                 "load_model does)")
            plan[i] = lp._replace(family=family)
    return plan


# ------------------------------------------------------------------------------------------------------------------------ Predictor
class Prediction(NamedTuple):
    """What a Predictor method returns, on the host.  Errors are relative L2, per sample; None where no targets were given."""
    pred: torch.Tensor                          # darcy (n, s, s); ns2d (n, s, s, H); ns3d (n, s, s, T)
    err: Optional[torch.Tensor] = None          # darcy: (n,)
    err_step: Optional[torch.Tensor] = None     # ns2d / ns3d: (n, T) per time step of the T frames that have a target
    err_full: Optional[torch.Tensor] = None     # ns2d / ns3d: (n,) over those T frames as one trajectory
    spec_pred: Optional[torch.Tensor] = None    # spectra=True: E(k) of every predicted frame, darcy (n, K); ns2d / ns3d (n, frames, K)
    spec_true: Optional[torch.Tensor] = None    # ... of the target frames, darcy (n, K); ns2d / ns3d (n, T, K)
    spec_err: Optional[torch.Tensor] = None     # ... of prediction - target on those frames


class _Replay:
    """fn(*inputs) -> tuple of tensors, captured once into a HIP graph for the example's shapes (GraphedRollout's recipe: an eager warm-up
    on a side stream - it also builds the cached grid features and operand tables - then the capture, all under no_grad).  Parameters
    are read through their pointers.  run() returns the graph-owned results: the caller copies them out before the next replay."""

    def __init__(self, fn, example_inputs):
        self.static_in = tuple(t.clone() for t in example_inputs)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            fn(*self.static_in)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.static_out = fn(*self.static_in)

    def run(self, *inputs):
        for dst, src in zip(self.static_in, inputs):
            dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.static_out


def _ns2d_native_applies(model, xx, yy):
    return (hasattr(model, "forward_cf") and hasattr(model, "get_grid") and xx.dim() == 4 and xx.is_cuda and xx.dtype == torch.float32
            and xx.shape[0] > 0 and xx[0].numel() > 0 and (yy is None or (yy.is_cuda and yy.dtype == torch.float32)))


def _frame_spectra(pred, target):
    """pred (B, F, H, W), target (B, T, H, W) with T <= F or None, views of any strides -> (B, (F + 2 T) K): per sample the spectra of
    the F predicted frames, then of the T target frames, then of the difference on those T frames (K24 where it applies: the measured
    frames in one call with the target, the frames past it in one without)"""
    B, F = pred.shape[:2]
    T = 0 if target is None else target.shape[1]
    if not T:
        return _spectra(pred, None, None, "Predictor").reshape(B, -1)
    e = _spectra(pred[:, :T], target, None, "Predictor")
    sp = e[:, :, 0] if F == T else torch.cat((e[:, :, 0], _spectra(pred[:, T:], None, None, "Predictor")[:, :, 0]), dim=1)
    return torch.cat((sp.reshape(B, -1), e[:, :, 1].reshape(B, -1), e[:, :, 2].reshape(B, -1)), dim=1)


def _ns2d_native(model, xx, yy, H, spectra=False):
    """The free-running roll-out of one batch (call under no_grad): xx (B, S, S, T_in), yy (B, S, S, T) with T <= min(H, 256) or None ->
    (pred (B, H, S, S) time-major, rel (B, T + 1) or None).  ns2d_rollout_errors' native form, which stops at the ground truth's end:
    here the steps that have a target take K18 with it, the others K18 without (no sums); every step but the last moves the window.
    spectra=True: a third result, _frame_spectra of the time-major pred and target as they lie."""
    from .. import _native
    B, S1, S2, T_in = xx.shape
    P = S1 * S2
    grid = model.get_grid(xx.shape, xx.device)
    # (B, T_in + features, S, S), DENSE in that order (a plain cat of the two permuted views would come out channels-last in memory)
    z = torch.empty((B, T_in + grid.shape[-1], S1, S2), dtype=torch.float32, device=xx.device)
    torch.cat((xx.permute(0, 3, 1, 2), grid.permute(0, 3, 1, 2)), dim=1, out=z)
    pred = torch.empty((B, H, S1, S2), dtype=torch.float32, device=xx.device)
    T = 0 if yy is None else yy.shape[-1]
    target = measured = ws = None
    if T:
        target = yy.permute(0, 3, 1, 2).contiguous()                    # (B, T, S, S): time-major
        measured = pred if T == H else torch.empty_like(target)         # K18 with a target writes pred in the target's layout
        ws = _native.rollout_ws(B, P, T, xx.device)
    for t in range(H):
        im = model.forward_cf(z).contiguous()                           # (B, 1, S, S): complete before the launch below overwrites its input
        if t < T:
            _native.rollout_advance(z, im, target, measured, ws, T_in, t, t + 1 < H)
        else:
            _native.rollout_advance(z, im, None, pred, None, T_in, t, t + 1 < H)
    if not T:
        return (pred, None, _frame_spectra(pred, None)) if spectra else (pred, None)
    if measured is not pred:
        pred[:, :T].copy_(measured)
    _, rel, _ = _native.rollout_finish(ws, B, P, T)
    return (pred, rel, _frame_spectra(pred, target)) if spectra else (pred, rel)


def _ns2d_stock(model, xx, yy, H):
    """the reference's loop written out (ns_train_2d.py:141-157 without its loss): -> (pred (B, S, S, >= H), rel (B, T + 1) or None)"""
    pred = None
    while pred is None or pred.shape[-1] < H:
        im = model(xx)
        pred = im if pred is None else torch.cat((pred, im), -1)
        xx = torch.cat((xx[..., im.shape[-1]:], im), dim=-1)
    if yy is None or yy.shape[-1] == 0:
        return pred, None
    T = yy.shape[-1]
    e = _step_errors_stock(pred[..., :T], yy)
    return pred, torch.cat((e.per_step, e.full.reshape(-1, 1)), dim=1)


class Predictor:
    """Predictions of `model` in batches of `batch_size` (the last one short where it does not divide the sample count), under no_grad
    and in eval mode (the model's previous mode is restored).  Inputs: tensors on any device, or a DeviceDataset (its y is the target
    unless one is passed); every batch is moved to the model's device.  Results come back on the host, after ONE read-back per call.
    graph=True (device models): full-size batches are replayed from one HIP graph per input shape, a short batch runs eagerly.
    Every method checks the resolution first (check_resolution): a grid the model cannot run raises before any launch."""

    def __init__(self, model, batch_size=16, graph=False):
        if batch_size < 1:
            raise ValueError(f"Predictor: batch_size = {batch_size}")
        self.model, self.batch_size = model, int(batch_size)
        self.device = next(model.parameters()).device
        self.graph = bool(graph)
        if self.graph and self.device.type != "cuda":
            raise RuntimeError("graph=True needs the model on the GPU (HIP graph capture)")
        self._replays, self._checked = {}, set()

    # ---- shared machinery
    def _check(self, S, T_in=None):
        if (S, T_in) not in self._checked:
            check_resolution(self.model, S, T_in)
            self._checked.add((S, T_in))

    @staticmethod
    def _inputs(x, y):
        if isinstance(x, DeviceDataset):
            x, y = x.x, (x.y if y is None else y)
        if y is not None and y.shape[0] != x.shape[0]:
            raise ValueError(f"Predictor: {x.shape[0]} inputs and {y.shape[0]} targets")
        if x.shape[0] == 0:
            raise ValueError("Predictor: no sample to predict")
        return x, y

    def _run(self, kind, x, y, per_pred, per_err, batch_fn, extra=(), per_spec=0):
        """batch_fn(xb, yb) -> (prediction (B, *per_pred), errors (B, per_err) or None[, spectra (B, per_spec)]) per batch into ONE flat
        device buffer [predictions | errors | spectra]; -> its host copy as (pred (n, *per_pred), err (n, per_err) or None, spectra
        (n, per_spec) or None)"""
        n, dev = x.shape[0], self.device
        np_ = math.prod(per_pred)
        flat = torch.empty((n * (np_ + per_err + per_spec),), dtype=torch.float32, device=dev)
        pred = flat[:n * np_].view(n, *per_pred)
        err = flat[n * np_:n * (np_ + per_err)].view(n, per_err) if per_err else None
        spec = flat[n * (np_ + per_err):].view(n, per_spec) if per_spec else None
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                for lo in range(0, n, self.batch_size):
                    hi = min(n, lo + self.batch_size)
                    xb = x[lo:hi].to(dev, dtype=torch.float32, non_blocking=True)
                    yb = None if y is None else y[lo:hi].to(dev, dtype=torch.float32, non_blocking=True)
                    if self.graph and hi - lo == self.batch_size:
                        key = (kind, tuple(xb.shape), None if yb is None else tuple(yb.shape), *extra, *(("spectra",) if per_spec else ()))
                        ins = (xb,) if yb is None else (xb, yb)
                        if key not in self._replays:
                            self._replays[key] = _Replay((lambda a, b=None: batch_fn(a, b)), ins)
                        res = self._replays[key].run(*ins)
                    else:
                        res = batch_fn(xb, yb)
                    pred[lo:hi].copy_(res[0].reshape(hi - lo, *per_pred))
                    if err is not None:
                        err[lo:hi].copy_(res[1].reshape(hi - lo, per_err))
                    if spec is not None:
                        spec[lo:hi].copy_(res[2].reshape(hi - lo, per_spec))
        finally:
            self.model.train(was_training)
        host = flat.cpu()                                       # the call's one read-back
        return (host[:n * np_].view(n, *per_pred), (host[n * np_:n * (np_ + per_err)].view(n, per_err) if per_err else None),
                (host[n * (np_ + per_err):].view(n, per_spec) if per_spec else None))

    @staticmethod
    def _spec_fields(spec, F, T, K):
        """the three spectra fields of a Prediction from _frame_spectra's rows: F predicted frames, T of them measured"""
        if spec is None:
            return {}
        n = spec.shape[0]
        out = {"spec_pred": spec[:, :F * K].view(n, F, K)}
        if T:
            out["spec_true"] = spec[:, F * K:(F + T) * K].view(n, T, K)
            out["spec_err"] = spec[:, (F + T) * K:].view(n, T, K)
        return out

    # ---- the three loops
    def darcy(self, x, y=None, spectra=False) -> Prediction:
        """x (n, s, s, 1) [, y (n, s, s)] -> pred (n, s, s), err (n,): the error is K20's `ratio` on device tensors.  spectra=True:
        spec_pred (n, K) and, with y, spec_true and spec_err"""
        x, y = self._inputs(x, y)
        if x.dim() != 4 or x.shape[-1] != 1:
            raise ValueError(f"Predictor.darcy: x {tuple(x.shape)} is not (n, s, s, 1)")
        n, s1, s2 = x.shape[:3]
        self._check(s2)

        def batch(xb, yb):
            B = xb.shape[0]
            out = self.model(xb).reshape(B, s1, s2)
            err = None if yb is None else rel_l2(out.reshape(B, -1), yb.reshape(B, -1))
            if not spectra:
                return out, err
            return out, err, _frame_spectra(out.unsqueeze(1), None if yb is None else yb.reshape(B, 1, s1, s2))

        K = n_shells(s1, s2)
        pred, err, spec = self._run("darcy", x, y, (s1, s2), 0 if y is None else 1, batch,
                                    per_spec=(K * (1 if y is None else 3)) if spectra else 0)
        fields = {k: v[:, 0] for k, v in self._spec_fields(spec, 1, 0 if y is None else 1, K).items()}
        return Prediction(pred, err=None if err is None else err[:, 0], **fields)

    def ns2d(self, xx, horizon=None, yy=None, spectra=False) -> Prediction:
        """The free-running roll-out: xx (n, S, S, T_in) -> pred (n, S, S, horizon), any horizon >= 1 (default: yy's length).  yy
        (n, S, S, T): the first min(T, horizon) predicted frames are measured against it - err_step (n, T), err_full (n,) from K18's
        `rel` - and the roll-out goes on past them.  float32 on a device model with forward_cf takes the native form (one K18 launch per
        step, at most 256 measured steps); CPU models, models without forward_cf or with more than one output frame the stock loop.
        spectra=True: spec_pred (n, horizon, K) and, with yy, spec_true and spec_err (n, T, K)."""
        xx, yy = self._inputs(xx, yy)
        if xx.dim() != 4:
            raise ValueError(f"Predictor.ns2d: xx {tuple(xx.shape)} is not (n, S, S, T_in)")
        if horizon is None:
            if yy is None:
                raise ValueError("Predictor.ns2d: a horizon, or targets whose length is the horizon")
            horizon = yy.shape[-1]
        H = int(horizon)
        if H < 1:
            raise ValueError(f"Predictor.ns2d: horizon = {horizon}")
        n, S1, S2, _ = xx.shape
        self._check(S2)
        T = 0 if yy is None else min(int(yy.shape[-1]), H)
        if yy is not None:
            yy = yy[..., :T]
        native = self.device.type == "cuda" and hasattr(self.model, "forward_cf") and hasattr(self.model, "get_grid")
        if native and T > NATIVE_STEP_ERRORS_MAX_T:
            raise ValueError(f"Predictor.ns2d: {T} measured steps, the native roll-out measures at most {NATIVE_STEP_ERRORS_MAX_T} (pass fewer "
                             "target frames; the horizon itself is free)")

        def batch(xb, yb):
            if native and _ns2d_native_applies(self.model, xb, yb):
                return _ns2d_native(self.model, xb, yb if T else None, H, spectra)
            p, rel = _ns2d_stock(self.model, xb, yb if T else None, H)
            p = p[..., :H].permute(0, 3, 1, 2)
            return (p, rel, _frame_spectra(p, yb.permute(0, 3, 1, 2) if T else None)) if spectra else (p, rel)

        K = n_shells(S1, S2)
        pred, rel, spec = self._run("ns2d", xx, yy if T else None, (H, S1, S2), T + 1 if T else 0, batch, extra=(H,),
                                    per_spec=(H + 2 * T) * K if spectra else 0)
        pred = pred.permute(0, 2, 3, 1)                         # the reference's layout, a view of the time-major frames
        fields = self._spec_fields(spec, H, T, K)
        return Prediction(pred, **fields) if rel is None else Prediction(pred, err_step=rel[:, :T], err_full=rel[:, T], **fields)

    def ns3d(self, x, calls=1, y=None, spectra=False) -> Prediction:
        """x (n, S, S, T_in[, 1]) -> pred (n, S, S, calls * T_out).  calls > 1 chains the model: a call's last T_in output frames are
        the next call's input (plain slices).  y (n, S, S, T) with T <= calls * T_out: the first T frames are measured - err_step
        (n, T), err_full (n,), K17's `rel` on device tensors.  spectra=True: spec_pred (n, calls * T_out, K) and, with y, spec_true and
        spec_err (n, T, K), from the (B, S, S, frames) tensors as they lie."""
        x, y = self._inputs(x, y)
        if x.dim() == 4:
            x = x.reshape(*x.shape, 1)
        if x.dim() != 5 or x.shape[-1] != 1:
            raise ValueError(f"Predictor.ns3d: x {tuple(x.shape)} is not (n, S, S, T_in, 1)")
        calls = int(calls)
        if calls < 1:
            raise ValueError(f"Predictor.ns3d: calls = {calls}")
        n, S1, S2, T_in = x.shape[:4]
        self._check(S2, T_in)
        T_out = _layers(self.model, S2, T_in)[1]
        if calls > 1 and T_out < T_in:
            raise ValueError(f"Predictor.ns3d: {type(self.model).__name__} gives {T_out} frames from {T_in}: too few to feed the next call")
        total = calls * T_out
        T = 0 if y is None else int(y.shape[-1])
        if T > total:
            raise ValueError(f"Predictor.ns3d: {T} target frames, {calls} call(s) predict {total}")

        def batch(xb, yb):
            B, outs = xb.shape[0], []
            for _ in range(calls):
                out = self.model(xb).view(B, S1, S2, T_out)
                outs.append(out)
                xb = out[..., T_out - T_in:].reshape(B, S1, S2, T_in, 1)
            out = outs[0] if calls == 1 else torch.cat(outs, dim=-1)
            if yb is None:
                return (out, None, _frame_spectra(out.permute(0, 3, 1, 2), None)) if spectra else (out, None)
            yb = yb.reshape(B, S1, S2, T)
            e = step_errors(out if T == total else out[..., :T], yb)
            rel = torch.cat((e.per_step, e.full.reshape(-1, 1)), dim=1)
            return (out, rel, _frame_spectra(out.permute(0, 3, 1, 2), yb.permute(0, 3, 1, 2))) if spectra else (out, rel)

        K = n_shells(S1, S2)
        pred, rel, spec = self._run("ns3d", x, y, (S1, S2, total), T + 1 if T else 0, batch, extra=(calls,),
                                    per_spec=(total + 2 * T) * K if spectra else 0)
        fields = self._spec_fields(spec, total, T, K)
        return Prediction(pred, **fields) if rel is None else Prediction(pred, err_step=rel[:, :T], err_full=rel[:, T], **fields)


# ---------------------------------------------------------------------------------------------------------------------- command line
def write_mat(path, result: Prediction, index, with_pred=True):
    """`pred` (unless with_pred is False), `err` or `err_step` / `err_full`, the spectra a spectra=True call added (`spec_pred`, `spec_true`,
    `spec_err` and their wavenumbers `k`) and `index` (the samples' places in the file's order) as a MATLAB v5 file:
    harness.data.MatReader reads it back"""
    import scipy.io
    fields = {"index": torch.as_tensor(index).to(torch.int64).numpy()}
    if with_pred:
        fields["pred"] = result.pred.contiguous().numpy()
    for key in ("err", "err_step", "err_full", "spec_pred", "spec_true", "spec_err"):
        v = getattr(result, key)
        if v is not None:
            fields[key] = v.contiguous().numpy()
    if result.spec_pred is not None:
        fields["k"] = torch.arange(result.spec_pred.shape[-1], dtype=torch.int64).numpy()
    scipy.io.savemat(path, fields)


def _parser():
    ap = argparse.ArgumentParser(prog="python -m uno_amd.harness.predict",
                                 description="Predict and evaluate from a weights file, at any resolution and horizon (GPU only)")
    ap.add_argument("loop", choices=("darcy", "ns2d", "ns3d"))
    ap.add_argument("--weights", required=True, help="the state_dict harness.fit (or the reference's scripts) saved")
    ap.add_argument("--record", default=None, help="the checkpoint record (default: <weights>.json where it exists)")
    ap.add_argument("--model", default=None, help="without a record: class of uno_amd.harness.models")
    ap.add_argument("--in-width", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--pad", type=int, default=None)
    ap.add_argument("--factor", type=float, default=None)
    ap.add_argument("--data", required=True, help="the file harness.darcy_datagen (darcy) or harness.datagen (ns2d, ns3d) wrote")
    ap.add_argument("--split", choices=("test", "val", "train", "all"), default="test",
                    help="which part of fit's split (re-created from the record's counts and seed); all: every sample read")
    ap.add_argument("--ntrain", type=int, default=None, help="without a record: the split's counts and seed")
    ap.add_argument("--nval", type=int, default=None)
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--sub", type=int, default=None, help="darcy: keep every sub-th grid point (default: the record's)")
    ap.add_argument("--size", type=int, default=None, help="ns2d / ns3d: resize the frames to size x size (default: the record's)")
    ap.add_argument("--samples", type=int, default=None, help="samples to read from the file (default: the record's, else the split's sum)")
    ap.add_argument("--gen-batch", type=int, default=None, help="ns2d / ns3d: the generator's batch size (default: the record's, else 20)")
    ap.add_argument("--t-in", type=int, default=None, help="input frames (default: the record's, else 10)")
    ap.add_argument("--horizon", type=int, default=None, help="ns2d: frames to predict (default: the record's t_f)")
    ap.add_argument("--calls", type=int, default=1, help="ns3d: chained calls")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--graph", action="store_true", help="replay full-size batches from a HIP graph")
    ap.add_argument("--out", default=None, help="a .mat file for pred, err (err_step, err_full) and index")
    ap.add_argument("--no-pred", action="store_true", help="leave the predictions out of --out")
    ap.add_argument("--spectra", action="store_true", help="also the shell-binned energy spectra: spec_pred, spec_true, spec_err and k in --out")
    ap.add_argument("--device", default=None)
    return ap


def main(argv=None) -> dict:
    from .fit import _split_cuts
    ap = _parser()
    a = ap.parse_args(argv)
    if a.loop == "ns2d" and a.calls != 1:
        ap.error("--calls belongs to ns3d; ns2d takes --horizon")
    if a.loop != "ns2d" and a.horizon is not None:
        ap.error("--horizon belongs to ns2d" + ("; ns3d takes --calls" if a.loop == "ns3d" else ""))
    if a.loop == "darcy" and a.size is not None or a.loop != "darcy" and a.sub is not None:
        ap.error("--sub belongs to darcy, --size to ns2d / ns3d")
    if a.no_pred and a.out is None:
        ap.error("--no-pred without --out writes nothing")
    record_path = a.record if a.record is not None else (a.weights + ".json" if os.path.exists(a.weights + ".json") and a.model is None else None)
    try:
        rec = read_record(record_path) if record_path is not None else None
    except ValueError as e:
        ap.error(str(e))
    if rec is None and (a.model is None or a.in_width is None or a.width is None):
        ap.error(f"no checkpoint record (--record, or {a.weights}.json): name the constructor with --model, --in-width and --width")
    if rec is not None and rec.get("loop", a.loop) != a.loop:
        ap.error(f"{record_path} records a {rec['loop']} run, not {a.loop}")
    known = rec or {}

    def setting(name, default=None):
        given = getattr(a, name)
        if given is not None:
            return given
        return known[name] if known.get(name) is not None else default

    counts = [setting(k) for k in ("ntrain", "nval", "ntest")]
    if a.split != "all" and (None in counts or setting("seed") is None):
        ap.error(f"--split {a.split} re-creates fit's split: without a record it needs --ntrain, --nval, --ntest and --seed (or --split all)")
    total = sum(counts) if None not in counts else None
    samples = setting("samples", total)
    if samples is None:
        ap.error("how many samples to read: --samples (no record and no split counts say it)")
    if not torch.cuda.is_available():
        raise SystemExit("uno_amd.harness.predict: the command line runs the product blocks, which need the GPU")
    device = torch.device(a.device if a.device else "cuda")

    ctor = {k: v for k, v in (("model", a.model), ("in_width", a.in_width), ("width", a.width), ("pad", a.pad), ("factor", a.factor)) if v is not None}
    try:
        model = load_model(a.weights, rec, device=device, **ctor)
    except ValueError as e:
        raise SystemExit(str(e))
    t_in = setting("t_in", 10)
    if a.loop == "darcy":
        sub = setting("sub", 1)
        x, y, _, _ = load_darcy(a.data, sub, samples, 1)
        where = {"sub": sub, "grid": int(x.shape[1])}
    else:
        size = setting("size", 64)
        frames = setting("horizon", known.get("t_f", 10)) if a.loop == "ns2d" else None
        T_read = min(frames, NATIVE_STEP_ERRORS_MAX_T) if a.loop == "ns2d" else NATIVE_STEP_ERRORS_MAX_T
        x, y, _, _ = load_ns(a.data, samples, 0, sample_num=samples, batch=setting("gen_batch", 20), T_in=t_in, T=T_read, size=size)
        if x is None:
            raise SystemExit(f"{samples} samples hold no whole generation batch of --gen-batch {setting('gen_batch', 20)}: nothing was read from {a.data}")
        if x.shape[-1] != t_in:
            raise SystemExit(f"{a.data} holds {x.shape[-1]} frames per sample: fewer than --t-in {t_in}")
        where = {"size": size}
    n = x.shape[0]
    if a.split == "all":
        index = torch.arange(n)
    else:
        if total > n:
            raise SystemExit(f"the split's {counts[0]} + {counts[1]} + {counts[2]} samples exceed the {n} read from {a.data}")
        index = dict(zip(("train", "val", "test"), _split_cuts(n, *counts, setting("seed"))))[a.split]
        if index.numel() == 0:
            raise SystemExit(f"--split {a.split}: that part of the split is empty")
    x, y = x[index], y[index]
    predictor = Predictor(model, batch_size=a.batch_size, graph=a.graph)
    try:
        if a.loop == "darcy":
            result = predictor.darcy(x, y, spectra=a.spectra)
        elif a.loop == "ns2d":
            result = predictor.ns2d(x, frames, y if y.shape[-1] else None, spectra=a.spectra)
        else:
            T_out = _layers(model, int(x.shape[2]), t_in)[1] * a.calls
            y = y[..., :T_out]
            result = predictor.ns3d(x, a.calls, y if y.shape[-1] else None, spectra=a.spectra)
    except ValueError as e:
        raise SystemExit(str(e))
    summary = {"loop": a.loop, "model": type(model).__name__, "split": a.split, "n": int(index.numel()), **where}
    if a.loop != "darcy":
        summary["frames"] = int(result.pred.shape[-1])
    if result.err is not None:
        summary["err"] = float(result.err.double().mean())
    if result.err_step is not None:
        summary["measured_frames"] = int(result.err_step.shape[1])
        summary["err_step"], summary["err_full"] = float(result.err_step.double().mean()), float(result.err_full.double().mean())
    if result.spec_pred is not None:
        summary["spectra"] = int(result.spec_pred.shape[-1])
    if a.out is not None:
        write_mat(a.out, result, index, with_pred=not a.no_pred)
        summary["out"] = a.out
    print(json.dumps(summary))
    return {**summary, "result": result, "index": index}


if __name__ == "__main__":
    main()
