"""Whole-model parity of the workloads bench.py times BESIDE the headline, at the geometry it times them.  pytest -m gpu

    c3      UNO(14, 32), 64^2, batch 32, two roll-out steps                 (bench.workload_kernel_names: c3_ns2d)
    c4_w8   Uno3D_T20(6, 8, pad=3), 64 x 64 x 10 -> 20, batch 8             (c4_ns3d_w8)
    c4_w32  Uno3D_T20(6, 32, pad=3), the same                               (c4_ns3d_w32)
    c5_f32  UNO_9(3, 64, pad=5), 1024^2 (padded 1089^2), batch 4, float32   (c5_model_f32)

tests/test_hip_headline_parity.py holds the Darcy headline to its oracle the way it is timed; this module does the same for these four.
  (a) the whole model: product blocks on the device (P) against the SAME model on the oracle's blocks in FLOAT64 on the host (R64,
      weights = the float32 initial values cast up): prediction, loss and every parameter gradient per element.  Three passes from the
      same weights: a fresh backward pass, a second one (the roll-out's weight gradients are batched over its uses from the second
      pass on - _param_grads.TIME_BATCHED_WGRAD -, plans are cached), and one step driven the way the workload drives it
      (zero_grad / backward / optimiser step, or DarcyTrainer.step), whose gradients are read back from .grad after the update;
  (b) each operator block on its own at full size, and the lift / projection ends, so that a failure names the layer;
  (c) the optimiser over each model's parameter set;
  (d) the last test: every kernel INSTANTIATION (template arguments kept) that one step of the workload launches also ran inside one of
      these comparisons.

Bounds.  Nothing is taken from what the kernels achieve.  For every compared tensor floor = rel_err(R32, R64), R32 being the oracle
model in float32 on the host (the reference's op sequence at the precision the reference runs it); the product passes when
rel_err(P, R64) <= max(project bound, 4 * floor), project bound = 1e-4 for a whole model and 5e-5 for a block (the headline test's
numbers), plus that test's absolute term 1e-6 * gmax for gradients.  4 = the allowance for a float32 pipeline whose rounding differs
in kind (DFT by matrix against FFT, summation order, fused epilogues) while being of the same precision.  A parameter whose TRUE
gradient is zero (the 1x1-convolution bias in front of an InstanceNorm) is recognised from R64 (||g|| <= 1e-12 gmax), their number per
model is asserted, and the product's residue is held to 4 * max(R32's residue, 1e-6 gmax).  Measured figures: docs/experiments.md."""
import gc
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import spectral_oracle as so

pytestmark = pytest.mark.gpu
MODEL_TOL, BLOCK_TOL, FLOOR_FACTOR = 1e-4, 5e-5, 4.0
RAN = set()          # full names (template arguments kept, uno:: stripped) of every kernel launched inside a comparison of this module
COMPARED = set()     # workloads whose whole-model comparison ran in this session
# workload: (bench.workload_kernel_names key, lr, weight decay, parameters with an exactly-zero gradient)
WORKLOADS = {"c3": ("c3_ns2d", 1e-3, 1e-4, 0), "c4_w8": ("c4_ns3d_w8", 1e-3, 1e-4, 3), "c4_w32": ("c4_ns3d_w32", 1e-3, 1e-4, 3),
             "c5_f32": ("c5_model_f32", 1e-3, 1e-3, 2)}
# kernels that compute nothing a comparison could check (at most three, each with its reason)
NOTHING_TO_COMPARE = ()


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _profiled(fn):
    from uno_amd import _native
    _native.profile_begin(200000)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        RAN.update(n.replace("uno::", "") for n, _, _ in _native.profile_end())
    return out


def _r(t):
    t = t.detach().cpu()
    return (torch.view_as_real(t) if t.is_complex() else t).double()       # (.double() on a complex tensor drops the imaginary part)


def _err(a, b):
    """(||a - b||, ||b||) in float64"""
    a, b = _r(a), _r(b)
    return float(torch.linalg.vector_norm(a - b)), float(torch.linalg.vector_norm(b))


def _rel(a, b):
    e, n = _err(a, b)
    return e / n if n > 0 else e


# ------------------------------------------------------------------------------------------------ the workloads
def build_model(wl, block_cls=None):
    from uno_amd.harness import UNO, UNO_9, Uno3D_T20
    kw = {} if block_cls is None else {"block_cls": block_cls}
    torch.manual_seed(0)
    if wl == "c3":
        return UNO(14, 32, **kw)
    if wl in ("c4_w8", "c4_w32"):
        return Uno3D_T20(6, int(wl[4:]), pad=3, **kw)
    return UNO_9(3, 64, pad=5, **kw)


def oracle_blocks(wl):
    return so.OracleOperatorBlock3d if wl.startswith("c4") else so.OracleOperatorBlock2d


def make_inputs(wl):
    from uno_amd.harness import synthetic_darcy_batch
    g = torch.Generator().manual_seed(1234)
    if wl == "c3":
        return torch.randn(32, 64, 64, 10, generator=g), torch.randn(32, 64, 64, 40, generator=g)
    if wl.startswith("c4"):
        return torch.randn(8, 64, 64, 10, 1, generator=g), torch.randn(8, 64, 64, 20, generator=g)
    return synthetic_darcy_batch(4, 1024, 1234, "cpu")


def workload_loss(wl, model, inp):
    from uno_amd.harness import lp_loss_rel_sum, ns2d_rollout_loss, ns3d_loss
    if wl == "c3":
        return ns2d_rollout_loss(model, inp[0], inp[1], T_f=2, step=1)
    if wl.startswith("c4"):
        return ns3d_loss(model, inp[0], inp[1])
    B = inp[0].shape[0]
    return lp_loss_rel_sum(model(inp[0]).reshape(B, -1), inp[1].reshape(B, -1))


def forward_backward(wl, model, inp, with_pred=True):
    """-> (prediction or None, loss); the gradients are in .grad.  The prediction is the output of the model call inside the loss (a
    forward hook); the NS-2D roll-out calls model.forward_cf, not the module, so its first-step prediction is a forward of its own."""
    seen = []
    pred = None
    if wl == "c3":
        if with_pred:
            with torch.no_grad():
                pred = model(inp[0])
        loss = workload_loss(wl, model, inp)
    else:
        h = model.register_forward_hook(lambda m, a, out: seen.append(out.detach()))
        try:
            loss = workload_loss(wl, model, inp)
        finally:
            h.remove()
        pred = seen[0]
    loss.backward()
    return pred, loss.detach()


def host_reference(wl, log=print):
    """R64 (prediction, loss, gradients of the oracle model in float64) + per-tensor floors rel_err(R32, R64) + R32's gradient norms, and
    the float32 initial weights.  R32 itself is dropped before this returns."""
    t0 = time.time()
    inp = make_inputs(wl)
    m32 = build_model(wl, oracle_blocks(wl))
    state = {k: v.clone() for k, v in m32.state_dict().items()}
    m64 = so.to_float64(m32)
    pred32, loss32 = forward_backward(wl, m32, inp)
    t32 = time.time() - t0
    pred64, loss64 = forward_backward(wl, m64, tuple(t.double() for t in inp))
    assert pred64.dtype == torch.float64 and loss64.dtype == torch.float64
    ref = {"pred": pred64, "loss": float(loss64), "grads": {}, "floor": {}, "norm32": {}, "state": state, "inputs": inp}
    ref["floor"]["pred"] = _rel(pred32, pred64)
    ref["floor"]["loss"] = abs(float(loss32) - float(loss64)) / abs(float(loss64))
    p32 = dict(m32.named_parameters())
    for k, p in m64.named_parameters():
        assert p.grad is not None and p.grad.dtype in (torch.float64, torch.complex128), k
        ref["grads"][k] = p.grad
        ref["floor"][k] = _rel(p32[k].grad, p.grad)
        ref["norm32"][k] = float(torch.linalg.vector_norm(_r(p32[k].grad)))
        p32[k].grad = None
    norms = {k: float(torch.linalg.vector_norm(_r(g))) for k, g in ref["grads"].items()}
    ref["gmax"] = max(norms.values())
    ref["zero"] = sorted(k for k, n in norms.items() if n <= 1e-12 * ref["gmax"])
    worst = max((k for k in norms if k not in ref["zero"]), key=lambda k: ref["floor"][k])
    log(f"[{wl}] host reference: R32 {t32:.0f} s, R32 + R64 {time.time() - t0:.0f} s; floor(pred) {ref['floor']['pred']:.2e}, floor(loss) "
        f"{ref['floor']['loss']:.2e}, worst gradient floor {ref['floor'][worst]:.2e} ({worst}); zero-gradient parameters {ref['zero']}, "
        f"R32 residue there <= {max([ref['norm32'][k] for k in ref['zero']] + [0.0]) / ref['gmax']:.1e} gmax")
    del m32, m64, p32
    gc.collect()
    return ref


def compare_to_reference(tag, ref, pred, loss, grads, tol=MODEL_TOL, log=print):
    """-> list of failures (empty: within bounds).  Prints the worst gradient and its floor."""
    bad = []
    fl = ref["floor"]
    if pred is not None:
        e = _rel(pred, ref["pred"])
        if not e <= max(tol, FLOOR_FACTOR * fl["pred"]):
            bad.append((tag, "prediction", e, fl["pred"]))
    el = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    if not el <= max(tol, FLOOR_FACTOR * fl["loss"]):
        bad.append((tag, "loss", el, fl["loss"]))
    gmax = ref["gmax"]
    worst = ("", 0.0, 0.0)
    assert set(grads) == set(ref["grads"])
    for k, gr in ref["grads"].items():
        g = grads[k]
        assert g is not None, (tag, k, "no gradient")
        if k in ref["zero"]:
            n = float(torch.linalg.vector_norm(_r(g)))
            if not n <= FLOOR_FACTOR * max(ref["norm32"][k], 1e-6 * gmax):
                bad.append((tag, k, "residue of an exactly-zero gradient", n / gmax, ref["norm32"][k] / gmax))
            continue
        e, n = _err(g, gr)
        if e / n > worst[1]:
            worst = (k, e / n, fl[k])
        if not e <= max(tol, FLOOR_FACTOR * fl[k]) * n + 1e-6 * gmax:
            bad.append((tag, k, e / n, fl[k]))
    log(f"[{tag}] loss rel {el:.2e} (floor {fl['loss']:.2e}); worst parameter gradient {worst[0]}: rel_err(P, R64) {worst[1]:.2e}, "
        f"floor {worst[2]:.2e}" + ("" if pred is None else f"; prediction {_rel(pred, ref['pred']):.2e} (floor {fl['pred']:.2e})"))
    return bad


@pytest.fixture(scope="module", params=list(WORKLOADS))
def reference(request):
    """R64 and the floors of one workload, computed once and freed before the next workload's"""
    ref = host_reference(request.param)
    ref["wl"] = request.param
    yield ref
    ref.clear()
    gc.collect()


# ------------------------------------------------------------------------------------------------ (a) whole model
def test_workload_model_matches_float64_oracle(reference):
    from uno_amd.harness import ComplexAdam, DarcyTrainer
    ref, wl = reference, reference["wl"]
    key, lr, wd, n_zero = WORKLOADS[wl]
    assert len(ref["zero"]) == n_zero and all(k.endswith(".w.conv.bias") for k in ref["zero"]), ref["zero"]
    prod = build_model(wl)
    prod.load_state_dict(ref["state"], strict=True)
    prod = prod.to(dev())
    inp = tuple(t.to(dev()) for t in ref["inputs"])
    grads = lambda: {k: p.grad for k, p in prod.named_parameters()}
    bad = []
    # pass 1: fresh model; pass 2: same weights, gradients cleared - time-batched / in-place weight gradients, cached plans
    for it in (1, 2):
        for p in prod.parameters():
            p.grad = None
        pred, loss = _profiled(lambda: forward_backward(wl, prod, inp, with_pred=(it == 1)))
        bad += compare_to_reference(f"{wl} pass {it}", ref, pred, loss, grads())
    # pass 3: the step as the workload drives it.  The optimiser runs for the first time here, after the backward pass, so the gradients
    # left in .grad belong to the weights R64 was evaluated at
    if wl == "c5_f32":
        tr = DarcyTrainer(prod, lr=lr, weight_decay=wd)
        seen = []
        h = prod.register_forward_hook(lambda m, a, out: seen.append(out.detach()))
        loss = _profiled(lambda: tr.step(*inp))
        h.remove()
        pred = seen[0]
    else:
        opt = ComplexAdam(prod.parameters(), lr=lr, weight_decay=wd)

        def step():
            opt.zero_grad(set_to_none=True)
            seen = []
            h = prod.register_forward_hook(lambda m, a, out: seen.append(out.detach()))
            loss = workload_loss(wl, prod, inp)
            h.remove()
            loss.backward()
            opt.step()
            return (seen[0] if seen else None), loss.detach()
        pred, loss = _profiled(step)
    bad += compare_to_reference(f"{wl} pass 3 (driven step)", ref, pred, loss, grads())
    moved = sum(float(torch.linalg.vector_norm(_r(p) - _r(ref["state"][k]))) > 0 for k, p in prod.named_parameters())
    assert moved == len(ref["grads"]), "the driven step's optimiser did not update every parameter"
    COMPARED.add(wl)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (b) blocks and ends
def _block_case(tag, ob32, blk, xs, gy, run, ref_run, log=print):
    """ob32: oracle block (float32, freshly initialised); blk: product block; xs: host inputs (float32), gy: output gradient.
    run(blk, device inputs) / ref_run(oracle block, host inputs) -> y.  y, every input gradient and every parameter gradient."""
    blk.load_state_dict(ob32.state_dict(), strict=True)
    blk = blk.to(dev())
    ob64 = so.to_float64(ob32)
    out = {}
    for name, ob, cast in (("r32", ob32, lambda t: t.clone()), ("r64", ob64, lambda t: t.double())):
        xr = [cast(x).requires_grad_(True) for x in xs]
        y = ref_run(ob, xr)
        y.backward(cast(gy))
        out[name] = (y.detach(), [x.grad for x in xr], {k: p.grad for k, p in ob.named_parameters()})
    xd = [x.to(dev()).requires_grad_(True) for x in xs]

    def go():
        y = run(blk, xd)
        y.backward(gy.to(dev()))
        return y
    y = _profiled(go)
    (y32, gx32, gp32), (y64, gx64, gp64) = out["r32"], out["r64"]
    assert y64.dtype == torch.float64
    bad = []
    checks = [("y", y, y32, y64)] + [(f"gx{i}", xd[i].grad, gx32[i], gx64[i]) for i in range(len(xs))]
    for what, p_, r32, r64 in checks:
        e, fl = _rel(p_, r64), _rel(r32, r64)
        if not e <= max(BLOCK_TOL, FLOOR_FACTOR * fl):
            bad.append((tag, what, e, fl))
    norms = {k: float(torch.linalg.vector_norm(_r(g))) for k, g in gp64.items()}
    gmax = max(norms.values())
    worst = ("", 0.0, 0.0)
    for k, p in blk.named_parameters():
        if norms[k] <= 1e-12 * gmax:
            assert k == "w.conv.bias" and blk.normalize, (tag, k)
            n, n32 = float(torch.linalg.vector_norm(_r(p.grad))), float(torch.linalg.vector_norm(_r(gp32[k])))
            if not n <= FLOOR_FACTOR * max(n32, 1e-6 * gmax):
                bad.append((tag, k, "residue of an exactly-zero gradient", n / gmax, n32 / gmax))
            continue
        (e, n), fl = _err(p.grad, gp64[k]), _rel(gp32[k], gp64[k])
        if e / n > worst[1]:
            worst = (k, e / n, fl)
        if not e <= max(BLOCK_TOL, FLOOR_FACTOR * fl) * n + 1e-6 * gmax:
            bad.append((tag, k, e / n, fl))
    log(f"[{tag}] y {_rel(y, y64):.2e} (floor {_rel(y32, y64):.2e}); worst parameter gradient {worst[0]}: {worst[1]:.2e} (floor {worst[2]:.2e})")
    assert not bad, bad


C3_BLOCKS = [   # Ci, Co, H -> Ho, modes of UNO(14, 32) on 64^2 (uno_amd/harness/models.py: L0 .. L6), batch 32
    (32, 48, 64, 48, 22), (48, 96, 48, 32, 14), (96, 192, 32, 16, 6), (192, 192, 16, 16, 6),
    (192, 96, 16, 32, 6), (192, 48, 32, 48, 14), (96, 32, 48, 64, 22),
]


@pytest.mark.parametrize("layer", range(7), ids=[f"L{i}" for i in range(7)])
def test_c3_blocks_full_size(layer):
    """OperatorBlock_2D of UNO(14, 32) at batch 32.  L5 / L6 take the concatenation of two tensors as the model hands it to them
    (torch.cat, then the block's ordinary forward)."""
    from uno_amd.integral_operators import OperatorBlock_2D
    Ci, Co, H, Ho, m = C3_BLOCKS[layer]
    torch.manual_seed(300 + layer)
    ob = so.OracleOperatorBlock2d(Ci, Co, Ho, Ho, m, m)
    blk = OperatorBlock_2D(Ci, Co, Ho, Ho, m, m)
    g = torch.Generator().manual_seed(310 + layer)
    gy = torch.randn(32, Co, Ho, Ho, generator=g)
    if layer >= 5:
        xs = [torch.randn(32, Ci // 2, H, H, generator=g) for _ in range(2)]
        f = lambda b, x: b(torch.cat(x, dim=1), Ho, Ho)
    else:
        xs = [torch.randn(32, Ci, H, H, generator=g)]
        f = lambda b, x: b(x[0], Ho, Ho)
    _block_case(f"c3 L{layer}", ob, blk, xs, gy, f, f)


def _t20_blocks(w):
    # (Ci, Co, din, dout, modes, Normalize) of Uno3D_T20(6, w, pad=3) on (8, 64, 64, 10): conv0, 1, 2, 3, 6, 7, 8
    return [
        (w, 2 * w, (64, 64, 13), (48, 48, 13), (22, 22, 5), True), (2 * w, 4 * w, (48, 48, 13), (32, 32, 13), (14, 14, 5), False),
        (4 * w, 8 * w, (32, 32, 13), (16, 16, 15), (6, 6, 5), False), (8 * w, 16 * w, (16, 16, 15), (16, 16, 15), (6, 6, 6), True),
        (16 * w, 4 * w, (16, 16, 15), (32, 32, 23), (6, 6, 6), False), (8 * w, 2 * w, (32, 32, 23), (48, 48, 26), (14, 14, 8), True),
        (4 * w, 2 * w, (48, 48, 26), (64, 64, 26), (22, 22, 8), False),
    ]


@pytest.mark.parametrize("w", [8, 32])
@pytest.mark.parametrize("layer", range(7), ids=["conv0", "conv1", "conv2", "conv3", "conv6", "conv7", "conv8"])
def test_c4_blocks_full_size(w, layer):
    """OperatorBlock_3D of Uno3D_T20(6, w, pad=3) at batch 8 (InstanceNorm3d on conv0, conv3, conv7)"""
    from uno_amd.integral_operators import OperatorBlock_3D
    Ci, Co, din, dout, modes, norm = _t20_blocks(w)[layer]
    torch.manual_seed(400 + w + layer)
    ob = so.OracleOperatorBlock3d(Ci, Co, *dout, *modes, Normalize=norm)
    blk = OperatorBlock_3D(Ci, Co, *dout, *modes, Normalize=norm)
    g = torch.Generator().manual_seed(410 + w + layer)
    xs = [torch.randn(8, Ci, *din, generator=g)]
    gy = torch.randn(8, Co, *dout, generator=g)
    f = lambda b, x: b(x[0], *dout)
    _block_case(f"c4 w{w} block {layer}", ob, blk, xs, gy, f, f)


D5 = 1089
C5_BLOCKS = {   # Ci, Co, H -> Ho, modes, Normalize of UNO_9(3, 64, pad=5) on the padded 1089^2 grid, batch 4
    "conv0": (64, 128, D5, D5 // 2, 18, False), "conv1": (128, 256, D5 // 2, D5 // 4, 8, True),
    "conv4": (256, 128, D5 // 4, D5 // 2, 8, True), "conv5": (256, 64, D5 // 2, D5, 18, False),
}


@pytest.mark.parametrize("name", list(C5_BLOCKS))
def test_c5_blocks_full_size(name):
    """OperatorBlock_2D of the 1024^2 model at batch 4.  conv5 through the two-source form the model uses (two 128-channel sources,
    the concatenation never built, GELU deferred): its pre-activation sum against the oracle block's two branches."""
    from uno_amd.integral_operators import OperatorBlock_2D
    Ci, Co, H, Ho, m, norm = C5_BLOCKS[name]
    torch.manual_seed(500 + len(name) + Ci)
    ob = so.OracleOperatorBlock2d(Ci, Co, Ho, Ho, m, m, Normalize=norm)
    blk = OperatorBlock_2D(Ci, Co, Ho, Ho, m, m, Normalize=norm)
    g = torch.Generator().manual_seed(510 + Ci + Ho)
    gy = torch.randn(4, Co, Ho, Ho, generator=g)
    if name == "conv5":
        xs = [torch.randn(4, Ci // 2, H, H, generator=g) for _ in range(2)]
        run = lambda b, x: b.forward_cat(x, Ho, Ho, defer_gelu=True)

        def ref_run(o, x):
            xc = torch.cat(x, dim=1)
            return o.conv(xc, Ho, Ho) + o.w(xc, Ho, Ho)
    else:
        xs = [torch.randn(4, Ci, H, H, generator=g)]
        run = ref_run = lambda b, x: b(x[0], Ho, Ho)
    _block_case(f"c5 {name}", ob, blk, xs, gy, run, ref_run)


def _ends_case(tag, dims, pdims, B, c_in, c_mid, c_lift, c_cat, c_hid, pad_t, log=print):
    """Lift fc0(gelu(fc(x))) -> gelu [-> pad of the time axis] and projection fc2(gelu(fc1(c))) of UNO / Uno3D_T20, channels-first on the
    device against nn.Linear on the channels-last tensors in float64 on the host (the weight gradients are sums over all pixels)."""
    from uno_amd.integral_operators import channel_mix, gelu_channel_mix, gelu_project
    nd = len(dims)
    to_last, to_first = (0, *range(2, nd + 2), 1), (0, nd + 1, *range(1, nd + 1))
    torch.manual_seed(len(tag))
    lin = {"fc": torch.nn.Linear(c_in, c_mid), "fc0": torch.nn.Linear(c_mid, c_lift), "fc1": torch.nn.Linear(c_cat, c_hid),
           "fc2": torch.nn.Linear(c_hid, 1)}
    l32 = {k: v for k, v in lin.items()}
    l64 = {k: torch.nn.Linear(v.in_features, v.out_features).double() for k, v in lin.items()}
    for k in lin:
        l64[k].load_state_dict({n: t.double() for n, t in lin[k].state_dict().items()})
    ld = {k: torch.nn.Linear(v.in_features, v.out_features).to(dev()) for k, v in lin.items()}
    for k in lin:
        ld[k].load_state_dict(lin[k].state_dict())
    g = torch.Generator().manual_seed(len(tag) + 1)
    x = torch.randn(B, c_in, *dims, generator=g)
    odims = (*dims[:-1], dims[-1] + pad_t)
    gl = torch.randn(B, c_lift, *odims, generator=g)
    c = torch.randn(B, c_cat, *pdims, generator=g)           # the projection's own grid (the 3-D model: 20 output steps)
    go = torch.randn(B, 1, *pdims, generator=g)
    padding = [0, pad_t] + [0, 0] * (nd - 1)
    res = {}
    for name, L, cast in (("r32", l32, lambda t: t.clone()), ("r64", l64, lambda t: t.double())):
        for m_ in L.values():
            m_.zero_grad(set_to_none=True)
        xr, cr = cast(x).requires_grad_(True), cast(c).requires_grad_(True)
        lifted = F.gelu(L["fc0"](F.gelu(L["fc"](xr.permute(*to_last))))).permute(*to_first)
        if pad_t:
            lifted = F.pad(lifted, padding)
        lifted.backward(cast(gl))
        out = L["fc2"](F.gelu(L["fc1"](cr.permute(*to_last)))).permute(*to_first)
        out.backward(cast(go))
        res[name] = {"lifted": lifted.detach(), "out": out.detach(), "gx": xr.grad, "gc": cr.grad,
                     **{f"{k}.{n}": p.grad.clone() for k, m_ in L.items() for n, p in m_.named_parameters()}}
    xd, cd = x.to(dev()).requires_grad_(True), c.to(dev()).requires_grad_(True)

    def run():
        lifted = F.gelu(gelu_channel_mix(channel_mix(xd, ld["fc"].weight, ld["fc"].bias), ld["fc0"].weight, ld["fc0"].bias))
        if pad_t:
            lifted = F.pad(lifted, padding)
        lifted.backward(gl.to(dev()))
        out = gelu_project(channel_mix(cd, ld["fc1"].weight, ld["fc1"].bias), ld["fc2"].weight, ld["fc2"].bias)
        out.backward(go.to(dev()))
        return lifted, out
    lifted, out = _profiled(run)
    got = {"lifted": lifted, "out": out, "gx": xd.grad, "gc": cd.grad,
           **{f"{k}.{n}": p.grad for k, m_ in ld.items() for n, p in m_.named_parameters()}}
    bad, worst = [], ("", 0.0, 0.0)
    for k, v in got.items():
        e, fl = _rel(v, res["r64"][k]), _rel(res["r32"][k], res["r64"][k])
        if e > worst[1]:
            worst = (k, e, fl)
        if not e <= max(2e-5, FLOOR_FACTOR * fl):            # 2e-5: the headline test's bound for these ends
            bad.append((tag, k, e, fl))
    log(f"[{tag}] worst {worst[0]}: {worst[1]:.2e} (floor {worst[2]:.2e})")
    assert not bad, bad


def test_c3_lift_and_projection_ends_full_size():
    """UNO(14, 32): fc 14 -> 16, fc0 16 -> 32 on (32, 14, 64, 64); fc1 64 -> 128, fc2 128 -> 1 on cat([L6 output, lifted])"""
    _ends_case("c3 ends", (64, 64), (64, 64), 32, 14, 16, 32, 64, 128, 0)


@pytest.mark.parametrize("w", [8, 32])
def test_c4_lift_and_projection_ends_full_size(w):
    """Uno3D_T20(6, w, pad=3): fc 6 -> 12, fc0 12 -> w on (8, 6, 64, 64, 10), time axis padded by 3; fc1 3w -> 4w, fc2 4w -> 1 on the
    cropped (8, 3w, 64, 64, 20) tensor"""
    _ends_case(f"c4 w{w} ends", (64, 64, 10), (64, 64, 20), 8, 6, 12, w, 3 * w, 4 * w, 3)


# ------------------------------------------------------------------------------------------------ (c) optimiser
@pytest.mark.parametrize("wl", list(WORKLOADS))
def test_workload_optimiser_full_size(wl):
    """ComplexAdam over the workload's parameter set with its own lr / weight decay: two steps against the oracle's restatement of the
    reference Adam (Adam.py:27-52); bound as in test_headline_optimiser_full_size"""
    from uno_amd.harness import ComplexAdam
    _, lr, wd, _ = WORKLOADS[wl]
    params = [p.detach().clone() for p in build_model(wl).parameters()]
    g = torch.Generator().manual_seed(2)
    grads = [[torch.randn(p.shape, dtype=p.dtype, generator=g) * 0.1 for p in params] for _ in range(2)]
    ref_p = [p.clone() for p in params]
    m_ = [torch.zeros_like(p) for p in params]
    v_ = [torch.zeros_like(p) for p in params]
    for step in (1, 2):
        so.reference_adam_step(ref_p, grads[step - 1], m_, v_, step, lr, 0.9, 0.999, 1e-8, wd)
    del m_, v_
    dp = [torch.nn.Parameter(p.to(dev())) for p in params]
    opt = ComplexAdam(dp, lr=lr, weight_decay=wd)

    def run():
        for step in (0, 1):
            for p, gr in zip(dp, grads[step]):
                p.grad = gr.to(dev())
            opt.step()
    _profiled(run)
    for i, (p, r, p0) in enumerate(zip(dp, ref_p, params)):
        e, n = _err(p, r)
        assert e <= 1e-6 * n + 1e-9, (wl, i, e / n)
        assert _err(p, p0)[0] > 0, (wl, i, "parameter not updated")


# ------------------------------------------------------------------------------------------------ (d) census
def test_zz_every_kernel_instantiation_of_the_workload_steps_was_oracle_checked():
    """Every kernel instantiation - full name, template arguments kept - that ONE step of c3 / c4 (both widths) / c5 float32 launches at
    the geometry bench.py times (bench.workload_kernel_names: launch records of a run made here) also ran inside a comparison of this
    module: not only the spectral kernels, also the channel-mix families, InstanceNorm, the element-wise ends and the optimiser."""
    if len(COMPARED) < len(WORKLOADS):
        pytest.skip("the whole-model comparisons of this module did not all run in this session")
    import bench
    census = bench.workload_kernel_names(dev())
    assert len(NOTHING_TO_COMPARE) <= 3
    missing = {}
    for wl, (key, _, _, _) in WORKLOADS.items():
        names = {n.replace("uno::", "") for n in census[key]}
        assert len(names) > 10, (key, names)
        print(f"[census] {key}: {len(names)} distinct kernel instantiations in one step")
        miss = sorted(names - RAN - set(NOTHING_TO_COMPARE))
        if miss:
            missing[key] = miss
    assert not missing, f"kernel instantiations of bench workloads that no full-size oracle comparison of this module launched: {missing}"
