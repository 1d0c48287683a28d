"""Adam with the semantics of the reference's optimiser (Adam.py:27-52), which differ from
torch.optim.Adam on complex parameters: the second moment is built from g * conj(g) (the squared
complex modulus, one real number per complex entry), weight decay is the coupled L2 form
(g += wd * p).  Implemented with multi-tensor (_foreach) ops over real views so a step is a handful
of launches instead of a Python loop of complex sqrt/addcdiv per parameter.  Parameters on a HIP device are
updated by the one-pass multi-tensor K10 kernel (csrc/adam.hip: 24 tensors per launch, one native call per step bucket)."""
from __future__ import annotations

import math

import torch
from torch.optim.optimizer import Optimizer


class ComplexAdam(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False, max_grad_norm=None,
                 skip_nonfinite=None):
        """capturable: keep the step count of the device parameters ON THE DEVICE (one counter per parameter group, advanced by the
        update itself), so that step() can be recorded in a HIP graph (harness.GraphedStep) - the bias corrections of the reference
        (Adam.py:27-52: from state['step']) are then evaluated on the device in double.  All device parameters of a group must take
        part in every step (they share the counter); state[p]['step'] is that counter tensor.  lr, eps and weight_decay are read by
        the update from three doubles ON THE DEVICE as well (sync_hyper() refreshes them from the param group whenever they changed):
        a scheduler that edits group['lr'] (reference ns_train_2d.py:37,113: StepLR) takes effect on the next replay of a captured
        step, exactly as on the eager path.

        max_grad_norm / skip_nonfinite (default: on when max_grad_norm is given) guard the step: the L2 norm over EVERY parameter of
        EVERY group that has a gradient is taken first (in double), the gradients enter the update scaled by
        coef = min(1, max_grad_norm / (norm + 1e-6)) - torch.nn.utils.clip_grad_norm_'s formula; the .grad tensors themselves are not
        rewritten - and a step whose norm is not finite changes nothing: parameters, moments and step counts stay bit for bit.  The
        threshold is the FIRST group's group['max_grad_norm'] (one global norm has one threshold).  Device parameters: K26 + the
        guarded K10 (csrc/adam.hip), no host read, capturable; they use the device step counter exactly as capturable=True does, with
        its constraints (only a counter on the device can stand still on a skipped step without the host knowing).  Host parameters:
        the same in stock ops, with one bool() on the host.  A guarded optimiser takes host parameters or device parameters, not both,
        and device parameters and gradients must be contiguous float32 / complex64: anything else raises instead of leaving a tensor out
        of the norm.  Under FlatGradients the norm is over what .grad holds when step() runs: the reduced sums after finish().
        last_grad_norm: the pre-clip norm of the last step (a float64 tensor on the parameters' device); clip_stats(): the counters
        since the last call (ONE host read)."""
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("invalid Adam hyper-parameter")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm = {max_grad_norm}: a positive number, or None")
        self.skip_nonfinite = bool(max_grad_norm is not None if skip_nonfinite is None else skip_nonfinite)
        self.guarded = max_grad_norm is not None or self.skip_nonfinite
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if self.guarded:
            defaults["max_grad_norm"] = None if max_grad_norm is None else float(max_grad_norm)
        super().__init__(params, defaults)
        self._plans = {}            # per param group: pointer tables of the device tensors (not part of state_dict)
        self.capturable = bool(capturable)
        # per group INDEX: (int32 step counter, float32[4] scratch, float64[3] (lr, eps, weight_decay), the three as last uploaded)
        self._dev_counters = {}
        # guarded, device: K26's record, its threshold (device double + the value last uploaded), its scratch and pointer table
        self._clip = None
        self._norm_plan = None
        # guarded, host: steps, clipped, skipped, non-finite, sum and max of the finite norms; the last norm
        self._host_stats = [0, 0, 0, 0, 0.0, 0.0]
        self._host_norm = None

    def _device_step(self, group, params, step, lr, beta1, beta2, eps, wd, guard=None):
        """K10 over all device tensors of the group in one native call; the pointer tables are rebuilt only when a
        parameter or gradient buffer moved (FlatGradients keeps them fixed)."""
        from .. import _native
        # one plan per set of buffers (the pointer tuple is the key): step buckets of one group never evict each other, and a
        # plan is rebuilt only when a parameter, gradient or moment buffer moved (e.g. load_state_dict replaces the moments)
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr())
                    for p in params)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 4:
                self._plans.clear()
            plan = _native.AdamPlan([p.data for p in params], [p.grad for p in params],
                                    [self.state[p]["exp_avg"] for p in params], [self.state[p]["exp_avg_sq"] for p in params])
            self._plans[key] = plan
        if step is None:            # capturable: the group's device counter and device hyper-parameters
            ctr, scal, hyper, _ = self._dev_counters[self._group_index(group)]
            if guard is not None:
                plan.step_guarded(ctr, scal, lr, beta1, beta2, eps, wd, hyper, guard, self.skip_nonfinite)
            else:
                plan.step_dev(ctr, scal, lr, beta1, beta2, eps, wd, hyper=hyper)
        else:
            plan.step(step, lr, beta1, beta2, eps, wd)
        # the kernel writes the parameters through raw pointers: tell autograd they changed (version counters guard saved tensors
        # and key the half-precision weight copies of the mixed-precision layers)
        torch.autograd.graph.increment_version(params)

    def _group_index(self, group):
        for i, g in enumerate(self.param_groups):
            if g is group:
                return i
        raise RuntimeError("ComplexAdam: unknown parameter group")

    def _counter(self, group, device):
        """The group's device-side step counter (+ scratch and hyper-parameters), created on first use.  A count that already exists
        in the group's state - an int from non-capturable steps, or the tensor load_state_dict() put there - is carried over:
        the bias corrections continue from it (reference Adam.py resumes from state['step'])."""
        gi = self._group_index(group)
        entry = self._dev_counters.get(gi)
        if entry is None:
            start = 0
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    start = max(start, int(st["step"]))            # (a one-off host read when the counter is created)
            ctr = torch.full((1,), start, dtype=torch.int32, device=device)
            now = (float(group["lr"]), float(group["eps"]), float(group["weight_decay"]))
            entry = [ctr, torch.zeros(4, dtype=torch.float32, device=device), torch.tensor(now, dtype=torch.float64).to(device), now]
            self._dev_counters[gi] = entry
        return entry

    def sync_hyper(self):
        """Upload (lr, eps, weight_decay) of every capturable group to the device if they changed since the last upload.  step() calls
        it when no stream capture is running; harness.GraphedStep calls it before every replay."""
        for gi, entry in self._dev_counters.items():
            g = self.param_groups[gi]
            now = (float(g["lr"]), float(g["eps"]), float(g["weight_decay"]))
            if entry[3] != now:
                entry[2].copy_(torch.tensor(now, dtype=torch.float64))
                entry[3] = now
        if self._clip is not None and self._clip["uploaded"] != self._max_norm():
            self._clip["uploaded"] = self._max_norm()
            self._clip["max_norm"].copy_(torch.tensor([self._clip["uploaded"]], dtype=torch.float64))

    # ------------------------------------------------------------------------------------------------------------ the guarded step
    def _max_norm(self) -> float:
        """the threshold as K26 takes it: +inf never clips (skip_nonfinite alone)"""
        m = self.param_groups[0].get("max_grad_norm")
        return math.inf if m is None else float(m)

    @staticmethod
    def _describe(gi, i, p):
        return f"parameter {i} of group {gi} (shape {tuple(p.shape)}, {p.dtype}, {p.device})"

    def _clip_buffers(self, device):
        """K26's record, threshold and scratch (one partial per 1024 floats of EVERY parameter that can have a gradient), created once:
        before a capture when init_state() ran"""
        if self._clip is None or self._clip["state"].device != device:
            from .. import _native
            ps = [p for g in self.param_groups for p in g["params"] if p.requires_grad]
            n = _native.grad_norm_partials([p.numel() for p in ps], [p.is_complex() for p in ps])
            self._clip = {"state": torch.zeros(_native.GRAD_NORM_RECORD, dtype=torch.float64, device=device),
                          "max_norm": torch.tensor([self._max_norm()], dtype=torch.float64).to(device), "uploaded": self._max_norm(),
                          "scratch": torch.empty(max(n, 1), dtype=torch.float64, device=device)}
        return self._clip

    def _guarded_params(self):
        """[(group index, index in the group, parameter)] of every parameter with a gradient; raises on what the norm cannot take"""
        found = [(gi, i, p) for gi, g in enumerate(self.param_groups) for i, p in enumerate(g["params"]) if p.grad is not None]
        on_dev = [p.is_cuda for _, _, p in found]
        if any(on_dev) and not all(on_dev):
            gi, i, p = found[on_dev.index(not on_dev[0])]
            raise RuntimeError(f"ComplexAdam(max_grad_norm / skip_nonfinite): host and device parameters in one optimiser - {self._describe(gi, i, p)} "
                               f"is not where parameter {found[0][1]} of group {found[0][0]} ({found[0][2].device}) is; one norm is taken on one device")
        for gi, i, p in found:
            if p.is_cuda:
                if p.dtype not in (torch.float32, torch.complex64) or p.grad.dtype != p.dtype:
                    raise RuntimeError(f"ComplexAdam(max_grad_norm / skip_nonfinite): {self._describe(gi, i, p)} with a {p.grad.dtype} gradient - the "
                                       "device norm takes float32 / complex64 parameters and gradients only")
                if not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError(f"ComplexAdam(max_grad_norm / skip_nonfinite): {self._describe(gi, i, p)} or its gradient is not contiguous")
            elif p.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128) or p.grad.dtype != p.dtype:
                raise RuntimeError(f"ComplexAdam(max_grad_norm / skip_nonfinite): {self._describe(gi, i, p)} with a {p.grad.dtype} gradient - the "
                                   "host norm takes float32 / float64 / complex64 / complex128 parameters and gradients only")
        return found

    def _guarded_step(self):
        found = self._guarded_params()
        if not found:
            return
        if found[0][2].is_cuda:
            from .. import _native
            device = found[0][2].device
            for gi, _, p in found:
                self._init_param_state(p)["step"] = self._counter(self.param_groups[gi], device)[0]
            clip = self._clip_buffers(device)
            if not torch.cuda.is_current_stream_capturing():
                self.sync_hyper()
            grads = [p.grad for _, _, p in found]
            key = tuple((g.data_ptr(), g.numel(), 1 if g.is_complex() else 0) for g in grads)
            if self._norm_plan is None or self._norm_plan.key != key:
                self._norm_plan = _native.GradNormPlan(grads)
            if self._norm_plan.partials > clip["scratch"].numel():
                raise RuntimeError("ComplexAdam: the gradient-norm scratch is smaller than the gradients (a parameter was added after init_state?)")
            self._norm_plan.run(clip["max_norm"], self.skip_nonfinite, clip["scratch"], clip["state"])
            for gi, group in enumerate(self.param_groups):
                ps = [p for g, _, p in found if g == gi]
                if ps:
                    self._device_step(group, ps, None, group["lr"], *group["betas"], group["eps"], group["weight_decay"], guard=clip["state"])
            return
        # host: the same figures in stock ops
        total = torch.zeros((), dtype=torch.float64)
        for _, _, p in found:
            total = total + self._real(p.grad).double().square().sum()
        norm = float(total.sqrt())
        finite = math.isfinite(norm)
        c = self._max_norm() / (norm + 1e-6) if finite else 1.0
        coef = c if c < 1.0 else 1.0
        clipped = float(torch.tensor(coef, dtype=torch.float32)) < 1.0         # as K26 counts: by the coefficient rounded to float
        st = self._host_stats
        self._host_norm = torch.tensor(norm, dtype=torch.float64)
        st[0] += 1
        st[3] += 0 if finite else 1
        if finite:
            st[4] += norm
            st[5] = max(st[5], norm)
        if not finite and self.skip_nonfinite:
            st[2] += 1
            return
        st[1] += 1 if clipped else 0
        for gi, group in enumerate(self.param_groups):
            buckets = {}
            for g, _, p in found:
                if g == gi:
                    s = self._init_param_state(p)
                    s["step"] += 1
                    buckets.setdefault(s["step"], []).append(p)
            for t, plist in buckets.items():
                gs = [self._real(p.grad) for p in plist]
                if coef < 1.0:
                    # a float32 gradient times a Python number: the number is rounded to float once, as K26 rounds its coefficient
                    gs = torch._foreach_mul(gs, coef)
                self._host_update(plist, gs, t, group["lr"], *group["betas"], group["eps"], group["weight_decay"])

    @property
    def last_grad_norm(self):
        """the pre-clip norm of the last guarded step: a float64 tensor where the parameters are (no host read); None before the first"""
        if self._clip is not None:
            return self._clip["state"][0]
        return self._host_norm

    def clip_stats(self) -> dict:
        """The guard's figures since the last call, then reset: steps, clipped, skipped, nonfinite, grad_norm (mean of the finite
        pre-clip norms; None when there was none) and grad_norm_max.  ONE host read for device parameters."""
        if not self.guarded:
            raise RuntimeError("ComplexAdam.clip_stats: the optimiser was built without max_grad_norm / skip_nonfinite")
        if self._clip is not None:
            steps, clipped, skipped, nonfinite, total, top = self._clip["state"][3:].tolist()
            self._clip["state"][3:].zero_()
        else:
            steps, clipped, skipped, nonfinite, total, top = self._host_stats
            self._host_stats = [0, 0, 0, 0, 0.0, 0.0]
        good = int(steps) - int(nonfinite)
        return {"steps": int(steps), "clipped": int(clipped), "skipped": int(skipped), "nonfinite": int(nonfinite),
                "grad_norm": total / good if good else None, "grad_norm_max": top if good else None}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # the loaded state replaced the moment tensors and the step entries: plans and device counters are rebuilt from it on next use
        self._plans.clear()
        self._dev_counters.clear()
        if self._clip is not None:
            self._clip["uploaded"] = None          # (the loaded group may carry another max_grad_norm)
        if not self.capturable:
            # a capturable checkpoint keeps ONE shared int32 device tensor as the step of every parameter, and torch hands `step` entries
            # over un-cloned: `st["step"] += 1` per parameter would then advance that shared tensor once per PARAMETER per step (and an
            # in-memory state_dict would alias the source optimiser's live counter).  Host integers here.
            for st in self.state.values():
                if isinstance(st.get("step"), torch.Tensor):
                    st["step"] = int(st["step"])

    @staticmethod
    def _real(t):
        return torch.view_as_real(t) if t.is_complex() else t

    def _init_param_state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(self._real(p))
            # one real second-moment entry per (possibly complex) parameter entry
            st["exp_avg_sq"] = torch.zeros(p.shape, dtype=st["exp_avg"].dtype, device=p.device)
        return st

    def init_state(self):
        """Allocate every parameter's moments (and, when capturable, the device step counters) NOW instead of at the first step():
        an allocation + zero fill recorded inside a HIP graph would be replayed with it."""
        for group in self.param_groups:
            for p in group["params"]:
                if not p.requires_grad:
                    continue
                st = self._init_param_state(p)
                if (self.capturable or self.guarded) and p.is_cuda and p.dtype in (torch.float32, torch.complex64):
                    st["step"] = self._counter(group, p.device)[0]
                    if self.guarded:
                        self._clip_buffers(p.device)
        self.sync_hyper()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.guarded:
            self._guarded_step()
            return loss
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
            # parameters are bucketed by their own step count (the reference keeps a per-parameter step and bias correction,
            # Adam.py:27-52): a parameter whose grad was None on some steps simply lands in another bucket
            host, devb = {}, {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self._init_param_state(p)
                on_dev = p.is_cuda and p.dtype in (torch.float32, torch.complex64) and p.is_contiguous() and p.grad.is_contiguous()
                if self.capturable and on_dev:
                    st["step"] = self._counter(group, p.device)[0]
                    devb.setdefault(None, []).append(p)
                    continue
                st["step"] += 1
                if on_dev:
                    devb.setdefault(st["step"], []).append(p)
                else:
                    host.setdefault(st["step"], []).append(p)
            if None in devb and not torch.cuda.is_current_stream_capturing():
                self.sync_hyper()
            for t, dev_p in devb.items():
                self._device_step(group, dev_p, t, lr, beta1, beta2, eps, wd)
            for t, plist in host.items():
                self._host_update(plist, [self._real(p.grad) for p in plist], t, lr, beta1, beta2, eps, wd)
        return loss

    def _host_update(self, plist, gs, t, lr, beta1, beta2, eps, wd):
        """the update of the parameters `plist` (all at step count t) from the real views `gs` of their gradients, in stock ops"""
        ps = [self._real(p) for p in plist]
        ms = [self.state[p]["exp_avg"] for p in plist]
        vs = [self.state[p]["exp_avg_sq"] for p in plist]
        cplx = [p.is_complex() for p in plist]
        bc1 = 1 - beta1 ** t
        bc2 = 1 - beta2 ** t
        if wd != 0:
            gs = torch._foreach_add(gs, ps, alpha=wd)
        torch._foreach_mul_(ms, beta1)
        torch._foreach_add_(ms, gs, alpha=1 - beta1)
        sq = torch._foreach_mul(gs, gs)
        sq = [s.sum(-1) if c else s for s, c in zip(sq, cplx)]       # |g|^2 for complex entries
        torch._foreach_mul_(vs, beta2)
        torch._foreach_add_(vs, sq, alpha=1 - beta2)
        denom = torch._foreach_sqrt(vs)
        torch._foreach_div_(denom, math.sqrt(bc2))
        torch._foreach_add_(denom, eps)
        denom = [d.unsqueeze(-1) if c else d for d, c in zip(denom, cplx)]
        torch._foreach_addcdiv_(ps, ms, denom, value=-lr / bc1)
