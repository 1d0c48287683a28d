"""Epoch runners: the reference's three training loops (train_darcy.py:35-100, ns_train_2d.py:34-168, ns_train_3d.py:34-147) restated
epoch for epoch on this package's pieces, and a command line around them:

    python -m uno_amd.harness.fit {darcy,ns2d,ns3d} --data FILE ... --out W.pt

The command line saves the best state_dict bare, as the reference does (its loops load the file unchanged), and beside it W.pt.json: the
model class, its constructor arguments, the data settings, the split and the run's figures - what harness.predict needs to use the file.

Kept from each loop: Adam(lr, weight_decay) with StepLR(step, gamma) stepped where that loop steps it (after the training batches for
Darcy and NS-3D; after the validation pass - hence on even epochs only - for NS-2D), the figures it prints (both Navier-Stokes loops
validate on even epochs only), the best validation figure selecting the saved state_dict, and the test pass on those best weights.

Left out - host-side habits only, the arithmetic of an epoch is the reference's:
  * `x.cuda()` from pageable memory per batch: a DeviceDataset keeps a split on the device (any iterable of (x, y) batches is taken too;
    its batches are moved to the model's device where they are not there already, in the order the iterable gives them);
  * `loss.item()` per batch: batch losses are summed on the device, ONE read-back per phase (training, validation, test) and epoch;
  * `gc.collect()` per batch and `torch.cuda.empty_cache()` per epoch;
  * T_f + 1 loss calls per NS-3D batch: `ns3d_loss(native=True)` takes loss and step error from one pass (K17 / K17-B).
Device tensors take the native loss paths (K20 through LpLoss for Darcy, the native roll-out for NS-2D, step_losses for NS-3D);
`native=False` switches each back to stock ops.  loss=HsLoss(...) (command line: --loss h1 / h2) replaces the TRAINING objective of a
loop by the relative Sobolev loss (losses.HsLoss, K25 on device tensors); validation and test figures stay the reference's relative
L2, so records stay comparable.  graph=True replays every full-size training batch through a GraphedStep whose
optimiser update is inside the graph (and NS-2D's evaluation roll-outs through a GraphedRollout); a short last batch runs eagerly.

max_grad_norm= / skip_nonfinite= (command line: --clip-norm X, --no-skip-nonfinite) guard every update through ComplexAdam: the global
gradient norm is clipped and a step with a non-finite norm is skipped, both on the device (K26 and the guarded K10; inside the graph
when graph=True); an epoch's figures (mean and largest pre-clip norm, clipped and skipped steps) cost ONE more read-back per epoch.
checkpoint=(path, every) (--save-every N: <out>.ckpt) writes, after every `every`-th epoch, all that the run needs to go on: model,
optimiser and scheduler state, the record so far, the batch-order generator and torch's random states.  resume=path (--resume)
continues from it and gives the weights, optimiser state and figures of the uninterrupted run (EpochRecord.seconds apart); it refuses
a checkpoint written under other settings.

The runners take any model with the reference's call convention and import nothing from the oracle."""
from __future__ import annotations

import argparse
import json
import os
import time
from dataclasses import asdict, dataclass, field
from typing import List, Optional, Tuple

import torch

from .data import DeviceDataset, load_darcy, load_ns
from .losses import HsLoss, LpLoss, _step_errors_stock, lp_loss_rel_sum, step_errors
from .optim import ComplexAdam
from .train import GraphedRollout, GraphedStep, ns2d_rollout_errors, ns2d_rollout_loss, ns3d_evaluate, ns3d_loss, ns3d_step_error


@dataclass
class EpochRecord:
    epoch: int
    lr: float                       # the learning rate the epoch's updates ran with
    seconds: float
    train: float
    val: Optional[float]            # None: the loop does not validate in this epoch
    # with max_grad_norm / skip_nonfinite only (ComplexAdam.clip_stats() of the epoch's updates):
    grad_norm: Optional[float] = None       # the mean pre-clip gradient norm of the steps whose norm was finite
    grad_norm_max: Optional[float] = None
    clipped: int = 0                # steps whose gradient was scaled down
    skipped: int = 0                # steps left out because their norm was not finite


@dataclass
class FitRecord:
    """What a runner returns: one EpochRecord per epoch, the best validation figure and its epoch, the test figures on the best
    weights (Darcy: (test_l2,); NS-2D: (per-step, whole trajectory); NS-3D: (whole trajectory, per-step) - each loop's own print
    order), and the best state_dict where no weight_path was given."""
    epochs: List[EpochRecord] = field(default_factory=list)
    best_epoch: int = -1
    best_val: float = 100000.0
    test: Tuple[float, ...] = ()
    state_dict: Optional[dict] = None


def _device_of(model):
    return next(model.parameters()).device


def _batches(data, batch_size, shuffle, generator, device):
    """one pass over a split: a DeviceDataset's own batches, or the iterable's in its order, on `device`"""
    if isinstance(data, DeviceDataset):
        if batch_size is None:
            raise ValueError("a DeviceDataset split needs batch_size")
        yield from data.batches(batch_size, shuffle=shuffle, generator=generator)
        return
    for x, y in data:
        yield (x if x.device == device else x.to(device, non_blocking=True)), (y if y.device == device else y.to(device, non_blocking=True))


class _Counted:
    """an iterable of batches that counts the samples it hands out"""

    def __init__(self, batches):
        self.batches, self.samples = batches, 0

    def __iter__(self):
        for x, y in self.batches:
            self.samples += int(x.shape[0])
            yield x, y


class _Sum:
    """batch figures summed on the device; read() is the phase's one read-back"""

    def __init__(self):
        self.total, self.count = None, 0

    def add(self, value, n):
        value = value.detach()
        self.total = value if self.total is None else self.total + value
        self.count += int(n)

    def read(self):
        """-> the sums as a list of floats (one device read for all of them)"""
        if self.total is None:
            raise ValueError("an empty split: no batch to train or evaluate on")
        return self.total.reshape(-1).tolist()


class _Trainer:
    """optimiser + scheduler + the training step of one runner, eager or replayed"""

    def __init__(self, model, loss_fn, lr, weight_decay, scheduler_step, scheduler_gamma, graph, max_grad_norm=None, skip_nonfinite=None):
        self.model, self.loss_fn = model, loss_fn
        self.graph = bool(graph) and _device_of(model).type == "cuda"
        if graph and not self.graph:
            raise RuntimeError("graph=True needs the model on the GPU (HIP graph capture)")
        guard = {k: v for k, v in (("max_grad_norm", max_grad_norm), ("skip_nonfinite", skip_nonfinite)) if v is not None}
        self.opt = ComplexAdam(model.parameters(), lr=lr, weight_decay=weight_decay, capturable=self.graph, **guard)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.opt, step_size=scheduler_step, gamma=scheduler_gamma)
        self.extra = None           # a second figure of the step (NS-3D: the step error), set by loss_fn
        self._graphed, self._shapes, self._extra_static = None, None, None

    def lr(self):
        return float(self.opt.param_groups[0]["lr"])

    def clip_fields(self):
        """the EpochRecord fields of the guard, from the optimiser's counters since the last call (one read-back; none unguarded)"""
        if not self.opt.guarded:
            return {}
        s = self.opt.clip_stats()
        return {"grad_norm": s["grad_norm"], "grad_norm_max": s["grad_norm_max"], "clipped": s["clipped"], "skipped": s["skipped"]}

    def _eager(self, x, y):
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss_fn(x, y)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def step(self, x, y):
        """-> the batch's loss (device tensor, detached); self.extra holds loss_fn's second figure where it has one"""
        if not self.graph:
            return self._eager(x, y)
        if self._graphed is None:
            self._graphed, self._shapes = GraphedStep(self.model, self.opt, self.loss_fn, (x, y)), (x.shape, y.shape)
            self._extra_static = self.extra         # graph-owned: rewritten by every replay
        if (x.shape, y.shape) == self._shapes:
            loss = self._graphed.step(x, y)
            self.extra = None if self._extra_static is None else self._extra_static.clone()
            return loss
        # a short last batch: eagerly, with the captured gradients set aside (the graph's update reads them where they lie)
        params = [p for g in self.opt.param_groups for p in g["params"]]
        kept = [p.grad for p in params]
        for p in params:
            p.grad = None
        loss = self._eager(x, y)
        for p, g in zip(params, kept):
            p.grad = g
        return loss


class _Best:
    """the weights of the best validation epoch: saved to a path (as the reference does) or kept in memory"""

    def __init__(self, model, weight_path, record, epochs):
        if epochs < 1:
            raise ValueError(f"epochs = {epochs}: a run needs at least one epoch (epoch 0 is the first that validates)")
        self.model, self.path, self.record = model, weight_path, record

    def offer(self, val, epoch, log, announce):
        if self.record.best_val > val:
            log(announce, self.record.best_val - val)
            self.record.best_val, self.record.best_epoch = val, epoch
            if self.path is not None:
                torch.save(self.model.state_dict(), self.path)
            else:
                self.record.state_dict = {k: v.detach().clone() for k, v in self.model.state_dict().items()}

    def restore(self):
        if self.record.best_epoch < 0:
            raise RuntimeError(f"no validation figure was below the starting value {self.record.best_val} (a NaN or inf loss?): no weights "
                               "were kept, so there is nothing to run the test pass on")
        self.model.load_state_dict(torch.load(self.path, map_location=_device_of(self.model)) if self.path is not None
                                   else self.record.state_dict)


CHECKPOINT_FORMAT = 1


class _Checkpoint:
    """The state of a run at an epoch boundary, written to `path` after every `every`-th epoch (a temporary file, then os.replace: a
    process lost while writing leaves the previous checkpoint), and read back by begin() when `resume` names one."""

    def __init__(self, settings, checkpoint, resume, model, trainer, record, generator):
        self.path, self.every = (None, 0) if checkpoint is None else (str(checkpoint[0]), int(checkpoint[1]))
        if checkpoint is not None and self.every < 1:
            raise ValueError(f"checkpoint=(path, every): every = {checkpoint[1]}")
        self.settings = dict(settings, skip_nonfinite=trainer.opt.skip_nonfinite, graph=trainer.graph)
        self.resume, self.model, self.trainer, self.record, self.generator = resume, model, trainer, record, generator

    def begin(self) -> int:
        """-> the first epoch to run: 0, or the checkpoint's next epoch with everything else restored from it"""
        if self.resume is None:
            return 0
        device = _device_of(self.model)
        ck = torch.load(self.resume, map_location="cpu")
        if ck.get("format") != CHECKPOINT_FORMAT:
            raise ValueError(f"resume: {self.resume} is not a checkpoint of format {CHECKPOINT_FORMAT}")
        was = ck["settings"]
        for k in list(self.settings) + [k for k in was if k not in self.settings]:
            if k not in was or k not in self.settings or was[k] != self.settings[k]:
                raise ValueError(f"resume: setting {k} is {self.settings.get(k)!r} here and {was.get(k)!r} in {self.resume}")
        if (ck["generator"] is None) != (self.generator is None):
            raise ValueError(f"resume: setting generator is {'given' if self.generator is not None else 'None'} here, not so in {self.resume}")
        self.model.load_state_dict(ck["model"])
        self.trainer.opt.load_state_dict(ck["optimizer"])
        self.trainer.scheduler.load_state_dict(ck["scheduler"])
        if self.trainer.graph:
            self.trainer.opt.init_state()           # moments and counters from the loaded state, before the capture
        rec = ck["record"]
        self.record.epochs = [EpochRecord(**e) for e in rec["epochs"]]
        self.record.best_epoch, self.record.best_val = rec["best_epoch"], rec["best_val"]
        self.record.state_dict = None if rec["state_dict"] is None else {k: v.to(device) for k, v in rec["state_dict"].items()}
        if self.generator is not None:
            self.generator.set_state(ck["generator"])
        torch.set_rng_state(ck["rng_cpu"])
        if device.type == "cuda":
            torch.cuda.set_rng_state(ck["rng_device"], device)
        return int(ck["epoch"])

    def epoch_done(self, ep):
        if self.path is None or (ep + 1) % self.every:
            return
        device = _device_of(self.model)
        rec = self.record
        ck = {"format": CHECKPOINT_FORMAT, "settings": self.settings, "epoch": ep + 1, "model": self.model.state_dict(),
              "optimizer": self.trainer.opt.state_dict(), "scheduler": self.trainer.scheduler.state_dict(),
              "record": {"epochs": [asdict(e) for e in rec.epochs], "best_epoch": rec.best_epoch, "best_val": rec.best_val,
                         "state_dict": rec.state_dict},
              "generator": None if self.generator is None else self.generator.get_state(), "rng_cpu": torch.get_rng_state(),
              "rng_device": torch.cuda.get_rng_state(device) if device.type == "cuda" else None}
        torch.save(ck, self.path + ".tmp")
        os.replace(self.path + ".tmp", self.path)


def _run_settings(loop, loss, user, **kw):
    """what a checkpoint is checked against: the runner's own arguments, then the caller's (the command line's)"""
    return {"loop": loop, **kw, "loss": None if loss is None else type(loss).__name__, **(user or {})}


def _evaluate(model, batches, figures):
    """eval mode, no_grad: figures(model, x, y) -> 1-D device tensor per batch, summed -> (list of floats, sample count); one read-back"""
    was_training = model.training
    model.eval()
    total = _Sum()
    try:
        with torch.no_grad():
            for x, y in batches:
                total.add(figures(model, x, y), x.shape[0])
    finally:
        model.train(was_training)
    return total.read(), total.count


def fit_darcy(model, train, val, test, batch_size=None, epochs=150, lr=1e-4, scheduler_step=50, scheduler_gamma=0.5, weight_decay=1e-3,
              weight_path=None, native=True, graph=False, generator=None, log=print, loss=None, max_grad_norm=None, skip_nonfinite=None,
              checkpoint=None, resume=None, settings=None) -> FitRecord:
    """train_darcy.py:35-100.  train / val / test: a DeviceDataset (batch_size then applies, training batches shuffled) or an iterable
    of (x (B, s, s, 1), y (B, s, s)) batches.  Figures: sums of per-sample relative L2 errors over the split's sample count.  loss: an
    HsLoss of layout "bhw" the training batches are scored with instead (called on (B, s, s) prediction and target; the training
    figure is then its sum over the sample count); validation and test stay relative L2.  max_grad_norm, skip_nonfinite, checkpoint,
    resume: see the module text (the same for the three runners); settings: a dict stored in the checkpoint beside the runner's own
    arguments and compared on resume (the command line's)."""
    device = _device_of(model)
    myloss = LpLoss(size_average=False) if native else lp_loss_rel_sum

    def loss_fn(x, y):
        B = x.shape[0]
        return myloss(model(x).reshape(B, -1), y.reshape(B, -1))

    def train_fn(x, y):
        return loss(model(x).reshape(y.shape), y)

    trainer = _Trainer(model, loss_fn if loss is None else train_fn, lr, weight_decay, scheduler_step, scheduler_gamma, graph, max_grad_norm,
                       skip_nonfinite)
    record = FitRecord()
    best = _Best(model, weight_path, record, epochs)
    ckpt = _Checkpoint(_run_settings("darcy", loss, settings, batch_size=batch_size, lr=lr, scheduler_step=scheduler_step,
                                     scheduler_gamma=scheduler_gamma, weight_decay=weight_decay, native=native, max_grad_norm=max_grad_norm),
                       checkpoint, resume, model, trainer, record, generator)
    t1 = time.perf_counter()
    for ep in range(ckpt.begin(), epochs):
        model.train()
        t1 = time.perf_counter()
        lr_now = trainer.lr()
        total = _Sum()
        for x, y in _batches(train, batch_size, True, generator, device):
            total.add(trainer.step(x, y), x.shape[0])
        trainer.scheduler.step()
        train_l2 = total.read()[0] / total.count
        (v,), nval = _evaluate(model, _batches(val, batch_size, False, None, device), lambda m, x, y: loss_fn(x, y).reshape(1))
        val_l2 = v / nval
        t2 = time.perf_counter()
        best.offer(val_l2, ep, log, "..Saving Model..")
        log(ep, t2 - t1, train_l2, val_l2)
        record.epochs.append(EpochRecord(ep, lr_now, t2 - t1, train_l2, val_l2, **trainer.clip_fields()))
        ckpt.epoch_done(ep)
    best.restore()
    (t,), ntest = _evaluate(model, _batches(test, batch_size, False, None, device), lambda m, x, y: loss_fn(x, y).reshape(1))
    record.test = (t / ntest,)
    log(epochs - 1, time.perf_counter() - t1, "Test Error", record.test[0])
    return record


def fit_ns2d(model, train, val, test, T_f=10, step=1, batch_size=None, epochs=150, lr=1e-4, scheduler_step=100, scheduler_gamma=0.5,
             weight_decay=1e-3, weight_path=None, native=True, graph=False, generator=None, log=print, loss=None, max_grad_norm=None,
             skip_nonfinite=None, checkpoint=None, resume=None, settings=None) -> FitRecord:
    """ns_train_2d.py:34-168.  Batches: xx (B, S, S, T_in), yy (B, S, S, T_f).  Odd epochs train only; even epochs validate, step the
    scheduler and offer their weights.  native: the cat-free training roll-out (ns2d_rollout_loss(native=True)) and the native
    evaluation roll-out; native=False: the reference's window-by-window forms.  graph=True needs the native evaluation roll-out's
    conditions (GraphedRollout) and step == 1.  loss: an HsLoss of layout "bhwt" every training step's frames are scored with instead,
through the window-by-window roll-out (the native training roll-out has its own fused relative-L2 step loss); the evaluation
roll-outs stay as `native` says, in relative L2."""
    device = _device_of(model)
    per = T_f / step

    def loss_fn(xx, yy):
        if loss is not None:
            return ns2d_rollout_loss(model, xx, yy, T_f, step, native=False, loss=loss)
        return ns2d_rollout_loss(model, xx, yy, T_f, step, native=native)

    def errors(m, xx, yy):
        if native:
            e = ns2d_rollout_errors(m, xx, yy, T_f, step).errors
            return torch.stack((e.step_sum, e.full_sum))
        # the reference's own evaluation: the loss of every group of `step` frames, and the whole trajectory
        B, loss, pred = yy.shape[0], 0, None
        for t in range(0, T_f, step):
            im = m(xx)
            loss = loss + lp_loss_rel_sum(im.reshape(B, -1), yy[..., t:t + step].reshape(B, -1))
            pred = im if pred is None else torch.cat((pred, im), -1)
            xx = torch.cat((xx[..., step:], im), dim=-1)
        return torch.stack((loss, lp_loss_rel_sum(pred.reshape(B, -1), yy.reshape(B, -1))))

    trainer = _Trainer(model, loss_fn, lr, weight_decay, scheduler_step, scheduler_gamma, graph, max_grad_norm, skip_nonfinite)
    rollout = {}                    # graph=True: the captured evaluation roll-out, by batch shape

    def errors_graphed(m, xx, yy):
        key = (tuple(xx.shape), tuple(yy.shape))
        if not rollout:
            rollout[key] = GraphedRollout(m, T_f, (xx, yy))         # (called under eval mode: the captured one)
        if key not in rollout:
            return errors(m, xx, yy)
        e = rollout[key].errors(xx, yy).errors
        return torch.stack((e.step_sum, e.full_sum))

    figures = errors_graphed if trainer.graph and native and step == 1 else errors
    record = FitRecord()
    best = _Best(model, weight_path, record, epochs)
    ckpt = _Checkpoint(_run_settings("ns2d", loss, settings, T_f=T_f, step=step, batch_size=batch_size, lr=lr, scheduler_step=scheduler_step,
                                     scheduler_gamma=scheduler_gamma, weight_decay=weight_decay, native=native, max_grad_norm=max_grad_norm),
                       checkpoint, resume, model, trainer, record, generator)
    for ep in range(ckpt.begin(), epochs):
        model.train()
        t1 = time.perf_counter()
        lr_now = trainer.lr()
        total = _Sum()
        for xx, yy in _batches(train, batch_size, True, generator, device):
            total.add(trainer.step(xx, yy), yy.shape[0])
        train_loss = total.read()[0] / total.count / per
        if ep % 2 == 1:
            t2 = time.perf_counter()
            log("epochs", ep, "time", t2 - t1, "train_loss", train_loss)
            record.epochs.append(EpochRecord(ep, lr_now, t2 - t1, train_loss, None, **trainer.clip_fields()))
            ckpt.epoch_done(ep)
            continue
        (v, _), nval = _evaluate(model, _batches(val, batch_size, False, None, device), figures)
        val_loss = v / nval / per
        t2 = time.perf_counter()
        trainer.scheduler.step()
        best.offer(val_loss, ep, log, "model saved")
        log("epochs", ep, "time", t2 - t1, "train_loss ", train_loss, "val_loss", val_loss)
        record.epochs.append(EpochRecord(ep, lr_now, t2 - t1, train_loss, val_loss, **trainer.clip_fields()))
        ckpt.epoch_done(ep)
    log("Traning Ended")
    best.restore()
    (s, f), ntest = _evaluate(model, _batches(test, batch_size, False, None, device), figures)
    record.test = (s / ntest / per, f / ntest)
    log("Test set Evaluation ", "Test_loss", record.test[0], record.test[1])
    return record


def fit_ns3d(model, train, val, test, T_f=10, batch_size=None, epochs=150, lr=1e-4, scheduler_step=50, scheduler_gamma=0.5,
             weight_decay=1e-3, weight_path=None, native=True, graph=False, generator=None, log=print, loss=None, max_grad_norm=None,
             skip_nonfinite=None, checkpoint=None, resume=None, settings=None) -> FitRecord:
    """ns_train_3d.py:34-147.  Batches: x (B, S, S, T_in, 1), y (B, S, S, T_f).  The training figure is the per-step error of every
    batch's own forward pass; validation (per-step error) runs on even epochs only; the test pass reports the whole-trajectory and the
    per-step error.  native: loss and step error of a training batch from ONE step_losses call; native=False: lp_loss_rel_sum and the
    slice-by-slice metric.  loss: an HsLoss of layout "bhwt" the training batches are scored with instead (called on the (B, S, S, T_f)
prediction and target); the training figure stays the per-step relative L2 error of the same forward pass."""
    device = _device_of(model)

    def loss_fn(x, y):
        if loss is not None:
            B, S = x.shape[0], x.shape[1]
            out, yv = model(x).view(B, S, S, T_f), y.reshape(B, S, S, T_f)
            with torch.no_grad():
                trainer.extra = step_errors(out.detach(), yv).step_sum if native else ns3d_step_error(out.detach(), yv)
            return loss(out, yv)
        value, trainer.extra = ns3d_loss(model, x, y, with_step_error=True, native=native)
        return value

    def figures(m, x, y):
        B, S = x.shape[0], x.shape[1]
        e = (step_errors if native else _step_errors_stock)(m(x).view(B, S, S, T_f), y.reshape(B, S, S, T_f))
        return torch.stack((e.full_sum, e.step_sum))

    trainer = _Trainer(model, loss_fn, lr, weight_decay, scheduler_step, scheduler_gamma, graph, max_grad_norm, skip_nonfinite)
    record = FitRecord()
    best = _Best(model, weight_path, record, epochs)
    ckpt = _Checkpoint(_run_settings("ns3d", loss, settings, T_f=T_f, batch_size=batch_size, lr=lr, scheduler_step=scheduler_step,
                                     scheduler_gamma=scheduler_gamma, weight_decay=weight_decay, native=native, max_grad_norm=max_grad_norm),
                       checkpoint, resume, model, trainer, record, generator)
    for ep in range(ckpt.begin(), epochs):
        t1 = time.perf_counter()
        lr_now = trainer.lr()
        model.train()
        total = _Sum()
        for x, y in _batches(train, batch_size, True, generator, device):
            trainer.step(x, y)
            total.add(trainer.extra, x.shape[0])
        trainer.scheduler.step()
        train_loss = total.read()[0] / (total.count * T_f)
        if ep % 2 == 1:
            t2 = time.perf_counter()
            log("epochs", ep, "time", t2 - t1, "train_loss ", train_loss)
            record.epochs.append(EpochRecord(ep, lr_now, t2 - t1, train_loss, None, **trainer.clip_fields()))
            ckpt.epoch_done(ep)
            continue
        if native:
            counted = _Counted(_batches(val, batch_size, False, None, device))
            val_loss = ns3d_evaluate(model, counted).item() / (counted.samples * T_f)
        else:
            (_, v), nval = _evaluate(model, _batches(val, batch_size, False, None, device), figures)
            val_loss = v / (nval * T_f)
        t2 = time.perf_counter()
        log("epochs", ep, "time", t2 - t1, "train_loss ", train_loss, "Val_loss  ", val_loss)
        best.offer(val_loss, ep, log, "model saved")
        record.epochs.append(EpochRecord(ep, lr_now, t2 - t1, train_loss, val_loss, **trainer.clip_fields()))
        ckpt.epoch_done(ep)
    log("Traning Ended")
    best.restore()
    (f, s), ntest = _evaluate(model, _batches(test, batch_size, False, None, device), figures)
    record.test = (f / ntest, s / (ntest * T_f))
    log("*** Test error: ", record.test[0], record.test[1])
    return record


# ---------------------------------------------------------------------------------------------------------------------- command line
RECORD_FORMAT = 1           # of the settings file main() writes beside the weights (<out>.json)


def _split_cuts(n, ntrain, nval, ntest, seed):
    """the sample indices of [train | val | test] among n samples: one shuffle under `seed`, then three cuts (harness.predict
    re-creates a run's split from its record through this)"""
    order = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return order[:ntrain], order[ntrain:ntrain + nval], order[ntrain + nval:ntrain + nval + ntest]


def _split(a, u, ntrain, nval, ntest, seed):
    """shuffle once, then [train | val | test] as the reference's main scripts cut them (darcy_flow_main.py, ns_uno*_main.py)"""
    n = a.shape[0]
    if ntrain + nval + ntest > n:
        raise SystemExit(f"--ntrain {ntrain} + --nval {nval} + --ntest {ntest} exceed the {n} samples read")
    return [(a[i], u[i]) for i in _split_cuts(n, ntrain, nval, ntest, seed)]


def _model(args, default_cls):
    from . import models
    name = args.model or default_cls
    if not hasattr(models, name):
        raise SystemExit(f"model {name}: no such class in uno_amd.harness.models (the 3-D classes are per output length: --t-f 9, 10, 20 or 40, "
                         "or name one with --model)")
    kw = {}
    if args.pad is not None:
        kw["pad"] = args.pad
    if args.factor is not None:
        kw["factor"] = args.factor
    return getattr(models, name)(args.in_width, args.width, **kw)


def checkpoint_record(a, model, record) -> dict:
    """What the bare state_dict does not say (settings only): the loop, the model's class and constructor arguments as they were passed,
    how the data were read and split, and the run's figures.  harness.predict builds the model and re-creates the split from it."""
    ctor = {"in_width": int(a.in_width), "width": int(a.width)}
    if a.pad is not None:
        ctor["pad"] = int(a.pad)
    if a.factor is not None:
        ctor["factor"] = float(a.factor)
    data = {"sub": int(a.sub)} if a.loop == "darcy" else {"size": int(a.size), "samples": a.samples, "gen_batch": int(a.gen_batch)}
    return {"format": RECORD_FORMAT, "loop": a.loop, "model": type(model).__name__, "ctor": ctor, "t_in": int(a.t_in), "t_f": int(a.t_f), **data,
            "ntrain": int(a.ntrain), "nval": int(a.nval), "ntest": int(a.ntest), "seed": int(a.seed),
            **_loss_record(a), **_guard_record(a, record),
            "best_epoch": int(record.best_epoch), "best_val": float(record.best_val), "test": [float(v) for v in record.test]}


LOSSES = {"l2": 0, "h1": 1, "h2": 2}       # --loss: the order k of the training objective (0: the loop's own relative L2)


def _loss_record(a) -> dict:
    """the training objective as the record holds it (harness.predict ignores it)"""
    name = getattr(a, "loss", "l2")
    hs_a = getattr(a, "hs_a", None)
    return {"loss": name, **({"hs_a": [float(v) for v in hs_a]} if name != "l2" and hs_a else {})}


def _guard_record(a, record) -> dict:
    """the guard's settings and what it did (harness.predict ignores them; absent from records written before they existed)"""
    clip = getattr(a, "clip_norm", None)
    skip = clip is not None and not getattr(a, "no_skip_nonfinite", False)
    return {"clip_norm": None if clip is None else float(clip), "skip_nonfinite": bool(skip),
            "skipped_steps": int(sum(e.skipped for e in record.epochs))}


def _hs_loss(a):
    """None for --loss l2, else the HsLoss of the loop's layout, summed over the batch as the loops sum their losses"""
    k = LOSSES[a.loss]
    if k == 0:
        if a.hs_a:
            raise SystemExit("--hs-a goes with --loss h1 or h2")
        return None
    if a.hs_a is not None and len(a.hs_a) != k:
        raise SystemExit(f"--loss {a.loss} takes {k} coefficient{'s' if k > 1 else ''} (--hs-a got {len(a.hs_a)})")
    return HsLoss(k=k, a=a.hs_a, layout="bhw" if a.loop == "darcy" else "bhwt", size_average=False, native=False if a.stock_loss else None)


def write_record(path, rec):
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def main(argv=None) -> FitRecord:
    ap = argparse.ArgumentParser(prog="python -m uno_amd.harness.fit", description="Train a U-NO model from a dataset file (.mat)")
    ap.add_argument("loop", choices=("darcy", "ns2d", "ns3d"))
    ap.add_argument("--data", required=True, help="the file harness.darcy_datagen (darcy) or harness.datagen (ns2d, ns3d) wrote")
    ap.add_argument("--model", default=None, help="class of uno_amd.harness.models (default: UNO_9 / UNO / Uno3D_T<t-f>)")
    ap.add_argument("--in-width", type=int, default=None, help="input channels incl. positional features (default: 3 / T_in + 4 / 6)")
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--pad", type=int, default=None)
    ap.add_argument("--factor", type=float, default=None)
    ap.add_argument("--ntrain", type=int, required=True)
    ap.add_argument("--nval", type=int, required=True)
    ap.add_argument("--ntest", type=int, required=True)
    ap.add_argument("--sub", type=int, default=1, help="darcy: keep every sub-th grid point")
    ap.add_argument("--size", type=int, default=64, help="ns2d / ns3d: resize the frames to size x size")
    ap.add_argument("--samples", type=int, default=None, help="ns2d / ns3d: samples in the file (default: ntrain + nval + ntest)")
    ap.add_argument("--gen-batch", type=int, default=20, help="ns2d / ns3d: the generator's batch size (samples per field of the file)")
    ap.add_argument("--t-in", type=int, default=10)
    ap.add_argument("--t-f", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=150)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--scheduler-step", type=int, default=None, help="default: the loop's own (50 / 100 / 50)")
    ap.add_argument("--scheduler-gamma", type=float, default=0.5)
    ap.add_argument("--weight-decay", type=float, default=1e-3)
    ap.add_argument("--graph", action="store_true", help="replay full-size training batches from a HIP graph")
    ap.add_argument("--stock-loss", action="store_true", help="the stock-op loss paths instead of the native ones")
    ap.add_argument("--loss", choices=tuple(LOSSES), default="l2", help="the training objective: relative L2 (the reference's), or the relative "
                    "Sobolev loss H^1 / H^2; validation and test figures stay relative L2")
    ap.add_argument("--hs-a", type=float, nargs="+", default=None, metavar="A", help="--loss h1 / h2: the coefficients a_1 [a_2] (default 1)")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="X", help="clip the global gradient norm to X (on the device) and skip "
                    "the steps whose norm is not finite")
    ap.add_argument("--no-skip-nonfinite", action="store_true", help="with --clip-norm: take a step with a non-finite gradient norm anyway")
    ap.add_argument("--save-every", type=int, default=None, metavar="N", help="write <out>.ckpt after every N-th epoch")
    ap.add_argument("--resume", action="store_true", help="continue from <out>.ckpt (same settings, --epochs may differ)")
    ap.add_argument("--seed", type=int, default=10001, help="of the weights, the split and the batch order")
    ap.add_argument("--device", default=None)
    ap.add_argument("--out", required=True, help="where the best state_dict goes")
    a = ap.parse_args(argv)
    if a.clip_norm is not None and not a.clip_norm > 0:
        ap.error(f"--clip-norm {a.clip_norm}: a positive number")
    if a.no_skip_nonfinite and a.clip_norm is None:
        ap.error("--no-skip-nonfinite goes with --clip-norm")
    if a.save_every is not None and a.save_every < 1:
        ap.error(f"--save-every {a.save_every}: a positive number of epochs")
    if a.resume and not os.path.exists(a.out + ".ckpt"):
        ap.error(f"--resume: there is no {a.out}.ckpt")
    # what a checkpoint must agree with: every setting but how long to run and where to write
    cli = {k: v for k, v in sorted(vars(a).items()) if k not in ("epochs", "resume", "save_every", "device")}

    device = torch.device(a.device if a.device else ("cuda" if torch.cuda.is_available() else "cpu"))
    total = a.ntrain + a.nval + a.ntest
    if a.loop == "darcy":
        x, y, _, _ = load_darcy(a.data, a.sub, total, 1)            # the file's first `total` samples; _split cuts them
        default_cls, a.in_width = "UNO_9", 3 if a.in_width is None else a.in_width
    else:
        samples = total if a.samples is None else a.samples
        xa, ya, xb, yb = load_ns(a.data, samples, 0, sample_num=samples, batch=a.gen_batch, T_in=a.t_in, T=a.t_f, size=a.size)
        x, y = xa, ya
        if x is None:
            raise SystemExit(f"{samples} samples hold no whole generation batch of --gen-batch {a.gen_batch}: nothing was read from {a.data}")
        if y.shape[-1] != a.t_f:
            raise SystemExit(f"{a.data} holds {x.shape[-1] + y.shape[-1]} frames per sample: fewer than --t-in {a.t_in} + --t-f {a.t_f}")
        if a.loop == "ns3d":
            x = x.reshape(*x.shape, 1)
        default_cls = "UNO" if a.loop == "ns2d" else f"Uno3D_T{a.t_f}"         # the 3-D classes are per output length: T9, T10, T20, T40
        # (the 2-D family's get_grid appends FOUR features - sin and cos of both coordinates)
        a.in_width = (a.t_in + 4 if a.loop == "ns2d" else 6) if a.in_width is None else a.in_width
    parts = [DeviceDataset(p, q, device) for p, q in _split(x, y, a.ntrain, a.nval, a.ntest, a.seed)]
    torch.manual_seed(a.seed)
    model = _model(a, default_cls).to(device)
    gen = torch.Generator(device=device).manual_seed(a.seed)
    common = dict(batch_size=a.batch_size, epochs=a.epochs, lr=a.lr, scheduler_gamma=a.scheduler_gamma, weight_decay=a.weight_decay,
                  weight_path=a.out, native=not a.stock_loss, graph=a.graph, generator=gen)
    hs = _hs_loss(a)
    if hs is not None:
        common["loss"] = hs
    if a.clip_norm is not None:
        common.update(max_grad_norm=a.clip_norm, skip_nonfinite=not a.no_skip_nonfinite)
    if a.save_every is not None:
        common["checkpoint"] = (a.out + ".ckpt", a.save_every)
    if a.save_every is not None or a.resume:
        common["settings"] = cli
    if a.resume:
        common["resume"] = a.out + ".ckpt"
    if a.scheduler_step is not None:
        common["scheduler_step"] = a.scheduler_step
    try:
        if a.loop == "darcy":
            record = fit_darcy(model, *parts, **common)
        elif a.loop == "ns2d":
            record = fit_ns2d(model, *parts, T_f=a.t_f, **common)
        else:
            record = fit_ns3d(model, *parts, T_f=a.t_f, **common)
    except ValueError as e:
        if a.resume and str(e).startswith("resume:"):
            raise SystemExit(f"--{e}") from None
        raise
    write_record(a.out + ".json", checkpoint_record(a, model, record))
    return record


if __name__ == "__main__":
    main()
