"""In-place parameter gradients: what a gradient target is (_GradTargets, and _layer_grad_targets for the weight and optional bias of a
1x1 layer), the state of the backward passes in flight (_Pass and its records) and the spectrum stacks that batch a spectral
layer's weight gradient over its uses in one graph (_SpectrumStack; a forward pass holds a _StackSlot of it).  The only module
that touches autograd's private entry points (the id of the running graph task, the engine's final-callback queue): the layers
call _grad_targets, _layer_grad_targets, _stack_take, _stack_grad_slot, _stack_arrived, _note_use and release_pass_state, read
the records' fields and do not look inside the pass state."""
import threading
import time
import warnings
from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import torch

from . import _native


# Weight-gradient kernels write a parameter's gradient where it will live instead of handing autograd fresh tensors to sum:
#   * FIRST contribution to a parameter in a backward pass: the kernel writes (beta = 0) into the parameter's registered buffer
#     (`_uno_grad_buffer`, set by harness.FlatGradients: a view into the flat all-reduce buffer) or into a fresh tensor, and the
#     backward returns an ALIAS of it - autograd adopts the alias as .grad when the pass ends (no zero fill, no `.grad +=` pass;
#     post-accumulate hooks - the bucketed all-reduce - fire as usual);
#   * LATER contributions in the same pass (a layer used several times in one graph: the 40-step roll-out of ns_train_2d.py:46-68
#     sums 40 gradients per weight; autograd would add them one by one in the input buffer of the parameter's AccumulateGrad
#     node): the kernel adds (beta = 1) into that same tensor and the backward returns None for the parameter.
# A parameter that already HAS a .grad when the pass starts (accumulation across passes) takes the ordinary path.
INPLACE_PARAM_GRADS = True


@dataclass(eq=False, slots=True)
class _Summed:
    """A parameter whose gradient this pass is summing in place."""
    tensor: torch.Tensor        # where the gradient is being summed
    param: torch.Tensor
    count: int                  # contributions so far
    nested: bool                # touched by a nested pass (see _end_of_pass)


@dataclass(eq=False, slots=True)
class _StackInFlight:
    """A spectrum stack that a backward call of this pass has reached."""
    stack: "_SpectrumStack"
    leaves: tuple               # (weights1, weights2) leaves
    wshape: tuple
    slots: list                 # slots whose gradient spectrum arrived in this pass


@dataclass(eq=False, slots=True)
class _UseCount:
    leaf: torch.Tensor          # weights1 leaf of a spectral layer
    n: int                      # the layer's backward calls of this pass, stacked or not


@dataclass(eq=False, slots=True)
class _Pass:
    """State of one backward pass in flight."""
    id: int                                                 # autograd's graph-task id
    born: float = field(default_factory=time.monotonic)
    acc: dict = field(default_factory=dict)                 # id(parameter) -> _Summed
    stacks: dict = field(default_factory=dict)              # id(stack) -> _StackInFlight
    uses: dict = field(default_factory=dict)                # id(weights1 leaf) -> _UseCount


# The backward passes in flight, keyed by autograd's graph-task id (a nested pass - re-entrant activation checkpointing,
# torch.autograd.grad inside a hook - is its own task with its own state; the outer pass finds its state untouched when it resumes)
_PASSES = {}
_PASSES_LOCK = threading.Lock()
_STALE_PASS_SECONDS = 3600.0
_SWEPT = {}                 # ids of swept passes (bounded): a pass that shows up again after its state was released must not go on silently


def release_pass_state():
    """Drop the state of every backward pass on record.  For a training loop that caught an exception out of loss.backward(): autograd
    skips the final callbacks of a pass that raised, so its entry would otherwise wait for the time-based sweep.  Only call while no
    backward pass is running on any thread of this process (harness.DarcyTrainer does, from its except path)."""
    with _PASSES_LOCK:
        _PASSES.clear()


def _sweep_stale_passes():
    """Autograd skips a pass's final callbacks when the pass raises (an out-of-memory error the training loop catches and retries):
    its entry would stay in _PASSES for ever - graph-task ids are never reused - keep its gradient buffers alive and push every
    parameter it recorded off the in-place path.  Called from a thread that is NOT inside a backward pass; an entry older than
    _STALE_PASS_SECONDS seen from there belongs to no pass that could still be running (a live pass of another thread is younger
    than that by orders of magnitude: the longest step of this package is a fraction of a second).  Should a live pass be swept after
    all (an hour in a debugger), it raises at its next contribution instead of training on a partial gradient (_SWEPT)."""
    now = time.monotonic()
    with _PASSES_LOCK:
        for tid in [t for t, ps in _PASSES.items() if now - ps.born > _STALE_PASS_SECONDS]:
            _PASSES.pop(tid, None)
            _SWEPT[tid] = now
        while len(_SWEPT) > 256:
            _SWEPT.pop(next(iter(_SWEPT)))


# The pass state hangs on two private entry points of autograd (the id of the running graph task, the engine's final-callback
# queue).  Should a torch release drop either, the library falls back to the ordinary path - every weight-gradient kernel returns
# its gradient as a fresh tensor and autograd accumulates - instead of failing: slower (one zero fill + one add per parameter
# and use), same results.
_current_graph_task_id = getattr(torch._C, "_current_graph_task_id", None)
_queue_callback = getattr(getattr(torch.autograd.Variable, "_execution_engine", None), "queue_callback", None)
_PASS_STATE_AVAILABLE = _current_graph_task_id is not None and _queue_callback is not None


def _graph_task_id() -> int:
    return _current_graph_task_id() if _PASS_STATE_AVAILABLE else -1


def _pass_state():
    """The _Pass of the running backward pass (registered with the engine on first use), or None outside a pass."""
    tid = _graph_task_id()
    if tid < 0:
        if _PASSES:
            _sweep_stale_passes()
        return None
    ps = _PASSES.get(tid)
    if ps is None:
        if tid in _SWEPT:
            # wall-clock age is only a heuristic for "this pass raised": a LIVE pass that was paused for longer than the limit (debugger,
            # contended device) lost its in-place accumulation map when it was swept - later contributions would overwrite earlier ones
            raise RuntimeError(f"uno_amd: backward pass {tid} was idle for more than {_STALE_PASS_SECONDS:.0f} s and its in-place gradient "
                               "state was released; raise uno_amd._param_grads._STALE_PASS_SECONDS or set INPLACE_PARAM_GRADS = False")
        if _PASSES:
            _sweep_stale_passes()              # (a pass that raised never ran its callback; see there)
        with _PASSES_LOCK:
            ps = _PASSES.get(tid)
            if ps is None:
                ps = _PASSES[tid] = _Pass(tid)
                # final callbacks belong to the graph task that is current when they are queued: this one runs when THIS pass completes
                _queue_callback(lambda: _end_of_pass(tid))
    return ps


def _end_of_pass(tid):
    """End of a backward pass (engine callback: every node, AccumulateGrad included, has run).  A parameter that received SEVERAL
    contributions in place must now have a .grad that aliases the tensor they were summed in; if it does not, autograd replaced
    that tensor on the way (a gradient for the same parameter from a path outside this library was added out of place) and the
    later in-place contributions would be missing - fail loudly instead of training on a wrong gradient.
    Spectral layers: remember how often each was used in this pass (the next forward passes stack that many spectra, see
    _SpectrumStack), and finish the stacks of which only a part of the uses was back-propagated."""
    with _PASSES_LOCK:
        ps = _PASSES.pop(tid, None)
    if ps is None:
        return
    for use in ps.uses.values():
        if not getattr(use.leaf, "_uno_nostack", False):
            use.leaf._uno_uses = use.n
    for fl in ps.stacks.values():
        _stack_flush_partial(fl.stack, fl.leaves, fl.wshape, fl.slots)
    for s in ps.acc.values():
        # nested: a pass that ran INSIDE this one gave the parameter a .grad of its own before this pass's AccumulateGrad ran; the
        # tensor summed here was then added to that .grad as a whole (complete: AccumulateGrad runs after every contribution)
        if s.count > 1 and not s.nested and s.param.grad is not None and s.param.grad.data_ptr() != s.tensor.data_ptr():
            raise RuntimeError("uno_amd: a parameter's gradient was accumulated in place by the library's kernels, but autograd also "
                               "received gradients for it from other operations and replaced the buffer; set "
                               "uno_amd._param_grads.INPLACE_PARAM_GRADS = False for this model")


def _on_device(p) -> bool:
    """The kernels write device memory: only a parameter that lives there takes the in-place path."""
    return p.is_cuda


def _grad_plan(p, ps):
    """('acc', tensor): later contribution of this pass | ('new', registered buffer or None): first contribution | None: ordinary path"""
    if not (INPLACE_PARAM_GRADS and _PASS_STATE_AVAILABLE) or not isinstance(p, torch.Tensor) or not p.is_leaf or not p.requires_grad or not _on_device(p):
        return None
    if ps is None:
        return None
    acc = ps.acc.get(id(p))
    if acc is not None:
        return "acc", acc.tensor
    if p.grad is not None:
        return None
    if len(_PASSES) > 1:
        # another pass is in flight (this one is nested in it, or the other way round): if it is summing this parameter's gradient
        # in place, its tensor - possibly the registered buffer - must not be overwritten by a beta = 0 write from here
        busy = False
        for other in list(_PASSES.values()):
            rec = other.acc.get(id(p)) if other is not ps else None
            if rec is not None:
                rec.nested = True
                busy = True
        if busy:
            return None
    buf = getattr(p, "_uno_grad_buffer", None)
    if buf is not None and (buf.shape != p.shape or buf.dtype != p.dtype or buf.device != p.device or not buf.is_contiguous()):
        buf = None
    return "new", buf


class _GradTargets(NamedTuple):
    """Where ONE kernel call writes the gradients of the parameters it produces together.  All or nothing: every parameter's plan
    (_grad_plan) is a first contribution, or every one is a later contribution; otherwise there is no record (_grad_targets gives
    None, nothing is noted in the pass state, and the caller takes the fresh-tensor path)."""
    dest: tuple                 # the tensors the call writes, in the order of the parameters
    accumulate: bool            # the call adds (a later contribution of the pass) instead of overwriting (the first)
    returned: tuple             # what the backward hands autograd for each: an alias of dest on the first contribution, None later


def _grad_targets(params):
    """_GradTargets of the parameters ONE kernel call writes together, or None: ordinary path (see _GradTargets for the rule)."""
    ps = _pass_state()
    plans = [_grad_plan(p, ps) for p in params]
    if any(pl is None for pl in plans) or len({pl[0] for pl in plans}) != 1:
        return None
    if plans[0][0] == "acc":
        for p in params:
            ps.acc[id(p)].count += 1
        return _GradTargets(tuple(pl[1] for pl in plans), True, (None,) * len(plans))
    dest = []
    for p, pl in zip(params, plans):
        buf = pl[1] if pl[1] is not None else torch.empty(p.shape, dtype=p.dtype, device=p.device)
        ps.acc[id(p)] = _Summed(buf, p, 1, False)
        dest.append(buf)
    return _GradTargets(tuple(dest), False, tuple(buf.view(buf.shape) for buf in dest))


class _LayerGradTargets(NamedTuple):
    """_GradTargets of the weight and optional bias of a 1x1 layer, as its kernels and its backward take them."""
    out_w: torch.Tensor
    out_b: Optional[torch.Tensor]       # None: the layer has no bias
    accumulate: bool
    gw: Optional[torch.Tensor]          # for autograd: viewed (Co, Ci) | None on a later contribution
    gb: Optional[torch.Tensor]


def _layer_grad_targets(leaves, has_bias):
    """leaves = (weight leaf, bias leaf or None) of a 1x1 layer, or None; has_bias: the call produces the bias gradient.
    -> _LayerGradTargets, or None: the leaves are unknown, the bias leaf's presence does not match has_bias (its gradient is not
    wanted, or there is nowhere to put it), or _grad_targets gives none.  Not None: committed, the caller's kernel call writes them."""
    if leaves is None or (leaves[1] is not None) != has_bias:
        return None
    tg = _grad_targets([leaves[0]] + ([leaves[1]] if has_bias else []))
    if tg is None:
        return None
    gw = tg.returned[0]
    return _LayerGradTargets(tg.dest[0], tg.dest[1] if has_bias else None, tg.accumulate,
                             None if gw is None else gw.view(gw.shape[0], -1), tg.returned[1] if has_bias else None)


# ---- weight gradient of a spectral layer that is used SEVERAL times in one graph (the 40-step roll-out of ns_train_2d.py:46-68
# calls every layer 40 times before one backward), batched over the uses.
# gW[i, o, mode] = sum_t sum_b conj(X_t[b, i, mode]) gO_t[b, o, mode]: executed per use that is 40 per-mode GEMMs with K = batch
# (32) that each read and re-write the whole weight gradient (2 x 16-26 MB for 8-16 MB of operands: 68 us per call, 15 ms of the
# 88 ms NS-2D step).  Instead the layer keeps the truncated spectra of its uses in ONE tensor (T, B, Ci, 2 m1, m2) - K1 of use t
# writes slot t in the forward pass, K1 of the output gradient writes slot t of a second tensor in the backward pass - and the use
# whose backward comes LAST runs one GEMM with K = T B over both and hands the complete gradient to autograd (the other uses
# return None for the weights).  Nothing is copied; the spectra were saved for the backward pass anyway.
# How many slots to provide is the number of uses the layer saw in the previous backward pass (`_uno_uses` on the weights1 parameter,
# stacked or not; the first pass runs use by use, a pass with more uses than slots fills several stacks and the next one is sized
# for all of them).  A stack is closed for new uses once a backward pass touched it or the weights changed; a pass that
# back-propagates only some of a stack's uses finishes it at the end of the pass (gradient added to .grad directly) and turns the
# stacking off for that layer.
TIME_BATCHED_WGRAD = True


class _PointwiseInfo(NamedTuple):
    """The block's 1x1 convolution whose split-K partial sums a stack holds (_SpectrumStack.P)."""
    Ci: int
    Co: int
    has_bias: bool
    leaves: tuple               # (weight leaf, bias leaf or None)


class _SpectrumStack:
    __slots__ = ("X", "G", "n", "sealed", "done", "version", "P", "Pinfo")

    def __init__(self, cap, shape, device, version):
        self.X = torch.empty((cap, *shape), dtype=torch.complex64, device=device)     # truncated input spectra, slot per use
        self.G = None               # truncated output-gradient spectra (allocated for the slots in use when the first one arrives)
        self.P = None               # (n, floats) split-K partial sums of the block's 1x1 convolution weight gradient, row per use
        self.Pinfo = None           # _PointwiseInfo of those
        self.n = 0                  # slots handed out
        self.sealed = False         # a backward pass has started on it: no new uses
        self.done = False           # its gradient has been produced: late backward calls (retain_graph) run on their own
        self.version = version


class _StackSlot(NamedTuple):
    """One use's place in its layer's stack."""
    stack: _SpectrumStack
    slot: int

    @property
    def xt(self):
        """where the forward pass leaves this use's truncated input spectrum"""
        return self.stack.X[self.slot]


def _stack_take(leaf, shape, device, wanted):
    """Forward pass of a spectral layer: _StackSlot for this use's truncated input spectrum, or None (layer used once per pass,
    no gradient wanted, stacking off)."""
    if not (TIME_BATCHED_WGRAD and wanted and INPLACE_PARAM_GRADS and _PASS_STATE_AVAILABLE) or not isinstance(leaf, torch.Tensor) or not leaf.is_leaf:
        return None
    cap = getattr(leaf, "_uno_uses", 0)
    # the per-mode GEMM addresses an operand with 32-bit byte offsets: a stack (and the stack of output-gradient spectra) stays under 2 GiB
    per_slot = 8 * shape[0] * max(shape[1], leaf.shape[1]) * shape[2] * shape[3]
    cap = min(cap, (2 ** 31 - 4096) // max(per_slot, 1))
    if cap < 2 or getattr(leaf, "_uno_nostack", False):
        return None
    st = getattr(leaf, "_uno_stack", None)
    if st is None or st.sealed or st.n >= st.X.shape[0] or tuple(st.X.shape[1:]) != tuple(shape) or st.X.device != device \
            or st.version != leaf._version:
        st = _SpectrumStack(cap, shape, device, leaf._version)
        try:
            leaf._uno_stack = st
        except (AttributeError, RuntimeError):
            return None
    st.n += 1
    return _StackSlot(st, st.n - 1)


def _stack_grad_slot(use, Co):
    """Backward pass of the use `use` (_StackSlot): where K1 writes the truncated spectrum of its output gradient, or None when the
    stack is finished."""
    st, slot = use
    if st.done:
        return None
    st.sealed = True
    if st.G is None:
        T, B, _, r2, m2 = st.X.shape
        st.G = torch.empty((st.n, B, Co, r2, m2), dtype=torch.complex64, device=st.X.device)
    return st.G[slot]


def _stack_wgrad(st, lo, hi, leaves, wshape, in_place):
    xt, go = st.X[lo:hi].flatten(0, 1), st.G[lo:hi].flatten(0, 1)
    tg = _grad_targets(leaves) if in_place else None
    gw1, gw2 = _native.mode_wgrad(xt, go, tuple(wshape[:4]), 2, out=tg.dest if tg else None, accumulate=bool(tg and tg.accumulate))
    return tg.returned if tg else (gw1, gw2)


def _count_use(ps, leaf):
    ps.uses.setdefault(id(leaf), _UseCount(leaf, 0)).n += 1


def _stack_arrived(use, leaves, wshape, in_place):
    """The gradient spectrum of the use `use` (_StackSlot) is in its slot.  -> (gw1, gw2) when it was the last of the stack's uses,
    else (None, None)."""
    st, slot = use
    ps = _pass_state()
    _count_use(ps, leaves[0])                   # every use of the pass counts: the next stacks hold them all
    rec = ps.stacks.setdefault(id(st), _StackInFlight(st, leaves, wshape, []))
    rec.slots.append(slot)
    if len(rec.slots) < st.n:
        return None, None
    del ps.stacks[id(st)]
    out = _stack_wgrad(st, 0, st.n, leaves, wshape, in_place)
    st.done, st.G = True, None
    return out


def _stack_pointwise(stack, leaves, gy, x1, x2, has_bias, act_x):
    """The 1x1 convolution's weight gradient of a block whose spectral layer is stacked: K9's first stage leaves this use's split-K
    partial sums in row `slot` of the stack's (n, floats) buffer, and the use that completes the stack runs ONE second stage over
    all rows (the roll-out ran 40 second stages of ~5 us per layer; their read-modify-write of the gradient goes with them).
    -> (gw (Co, Ci), gb) for autograd ((None, None) until the last use), or NotImplemented: take the ordinary path for this call."""
    st, slot = stack
    B, Co, P = gy.shape
    Ci = x1.shape[1] + (x2.shape[1] if x2 is not None else 0)
    nf = _native.channel_wgrad_partial_floats(B, Ci, Co, P)
    if st.P is None:
        if st.Pinfo is not None:
            return NotImplemented               # the stack's buffer has been consumed (late call on a retained graph)
        st.P = torch.empty((st.n, nf), dtype=torch.float32, device=gy.device)
        st.Pinfo = _PointwiseInfo(Ci, Co, has_bias, leaves)
    info = st.Pinfo
    fits = st.P.shape[1] == nf and (info.Ci, info.Co, info.has_bias) == (Ci, Co, has_bias)
    if fits:
        _native.channel_wgrad2(gy, x1, x2, need_bias=has_bias, act_x=act_x, partials_out=st.P[slot])
    else:
        st.P[slot].zero_()                      # another grid than the stack's other uses: this use is computed on its own
    if not st.done:
        return (None, None) if fits else NotImplemented
    # the spectral half of this backward call completed the stack: every row is written
    lt = _layer_grad_targets(info.leaves, info.has_bias)
    gw, gb = _native.channel_wgrad_finish(st.P, info.Ci, info.Co, info.has_bias, out_w=lt.out_w if lt else None,
                                          out_b=lt.out_b if lt else None, accumulate=bool(lt and lt.accumulate))
    st.P = None
    if not fits:
        _native.channel_wgrad2(gy, x1, x2, need_bias=info.has_bias, act_x=act_x, out_w=gw, out_b=gb, accumulate=True)
    return (lt.gw, lt.gb) if lt else (gw, gb)


def _runs(slots):
    """(lo, hi) of each run of consecutive entries of the sorted list `slots`: slots lo .. hi - 1."""
    lo = 0
    for k in range(1, len(slots) + 1):
        if k == len(slots) or slots[k] != slots[k - 1] + 1:
            yield slots[lo], slots[k - 1] + 1
            lo = k


def _add_to_grad(p, g):
    if p.grad is None:
        p.grad = g
    else:
        p.grad.add_(g)


def _stack_flush_partial(st, leaves, wshape, slots):
    """End of a pass that back-propagated only `slots` of the stack's uses: their weight gradient goes to .grad directly (the
    parameters' AccumulateGrad nodes have run), the remaining uses - if a later pass reaches them - run one by one."""
    slots = sorted(slots)
    with torch.no_grad():
        tot = None
        for lo, hi in _runs(slots):
            g = _stack_wgrad(st, lo, hi, leaves, wshape, False)
            tot = g if tot is None else (tot[0] + g[0], tot[1] + g[1])
        for p, g in zip(leaves, tot):
            _add_to_grad(p, g)
        if st.P is not None:                    # the block's 1x1 convolution: second stage over the rows that were written
            info = st.Pinfo
            ptot = None
            for lo, hi in _runs(slots):
                g = _native.channel_wgrad_finish(st.P[lo:hi], info.Ci, info.Co, info.has_bias)
                ptot = g if ptot is None else (ptot[0] + g[0], (ptot[1] + g[1]) if info.has_bias else None)
            for p, g in ((info.leaves[0], ptot[0]), (info.leaves[1] if info.has_bias else None, ptot[1])):
                if p is not None:
                    _add_to_grad(p, g.view(p.shape))
            st.P = None
    st.done, st.G = True, None
    leaves[0]._uno_uses, leaves[0]._uno_nostack = 0, True
    warnings.warn("uno_amd: a backward pass covered only some of the uses of a spectral layer whose weight gradient is batched "
                  "over its uses (TIME_BATCHED_WGRAD); the gradient of this pass was added to .grad after the pass (gradient hooks "
                  "did not see it) and the batching is now off for this layer", RuntimeWarning, stacklevel=2)


def _note_use(leaf):
    """A spectral layer's backward ran outside a stack: count it (what the next forward passes size their stack by)."""
    ps = _pass_state()
    if ps is not None and isinstance(leaf, torch.Tensor) and leaf.is_leaf:
        _count_use(ps, leaf)


def _stack_wanted(ctx, iw, x, half_weights):
    return bool(ctx.needs_input_grad[iw] and ctx.needs_input_grad[iw + 1] and x.dtype == torch.float32 and not half_weights)
