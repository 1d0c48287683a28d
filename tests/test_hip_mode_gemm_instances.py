"""Every kernel and launch plan of the per-mode complex GEMM K2 / K4 (csrc/mode_gemm.hip) runs against float64.  pytest -m gpu

9 LDS-staged kernels mode_gemm_kernel<QC, PIPE, BH, ACC>, 9 4x4x1 kernels mode_gemm_blocks_kernel<MTW, NTW, PF, BH, ACC> with their
run-time arguments KS and adjacent_modes (30 configurations), and 4 pair kernels mode_gemm_blocks_pair_kernel<MA, NA, 4, ACCB> that run
both GEMMs of a backward pass: 74 declared configurations, 66 of which a call can reach (test_mode_gemm_instances_cpu.py proves the
partition).  tests/golden/mode_gemm_instances.json (tools/mode_gemm_instance_shapes.py) holds for each reachable one - and for each op
of its flavour - the smallest shape that reaches it and a stressed one (ragged M, N, K and last mode group, more than one tile, idle
workgroups in the XCD map, 2 and 4 corners).  Which configuration a shape takes is asked of the library (_native.mode_gemm_plan /
mode_backward_plan: the plan function the launchers use), not mirrored here.

Single launches, one case per entry through _native.mode_mix / mode_wgrad:
  * outputs (for accumulating calls the caller's buffers too) live between guard bands (RedZone of test_hip_redzone.py), intact afterwards;
  * the launch records hold exactly one K2 kernel, the one the plan names, and the plan is the one the table recorded;
  * everything finite, relative L2 against the float64 einsum below test_hip_spectral2d.TOL, and every entry within the derived float32
    bound of mode_gemm_instances.reference_and_bound (printed: worst |got - ref| / bound);
  * accumulating calls give base + product for a random non-zero base;
  * the stressed shape twice gives the same bits.
Pair launches: _native.mode_backward equals mode_mix(op 1) and mode_wgrad bit for bit, float64 within the bounds, with and without
accumulation, from one launch of the pair kernel the plan names.
Isolation: NaN in one (row, mode) element of A, or one (column, mode) element of B, turns exactly the outputs that depend on it into NaN
and leaves every other output bit-identical - on one stressed entry per compiled single kernel.
Degenerate calls: B = 0, and 1 x 1 x 1 channels on one mode."""
import numpy as np
import pytest
import torch

import mode_gemm_instances as mg
from test_hip_redzone import RedZone
from test_hip_spectral2d import TOL

pytestmark = pytest.mark.gpu
TABLE = mg.load_table()
SINGLES = [e for e in TABLE if mg.family_of(e["config"]) != "pair"]
PAIRS = [e for e in TABLE if mg.family_of(e["config"]) == "pair"]
DEVICE_REFERENCE_ABOVE = 2000000          # multiply-adds above which the float64 reference is formed on the device (and spot-checked on the host)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _profiled(fn):
    from uno_amd import _native
    _native.profile_begin(64)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ran = [n for n, _, _ in _native.profile_end()]
    return out, [n for n in ran if "mode_gemm" in n]


def _reference_device(shape):
    B, Ci, Co, nc, Mc = shape
    return dev() if B * Ci * Co * nc * Mc > DEVICE_REFERENCE_ABOVE else torch.device("cpu")


def _case(op, shape, half, acc):
    device = _reference_device(shape)
    c = mg.case(op, shape, half=half, acc=acc, device=device)
    if device.type != "cpu":
        mg.host_slice_check(c["A"], c["Bm"], c["ref"], c["base"])
    return c


def _call(op, A, Bm, base, half):
    """one _native call on operands in GEMM form -> (result in GEMM form (M, N, nc, Mc), K2 launch records).  Outputs - and the buffers an
    accumulating call adds into - are allocated here, under whatever RedZone is active."""
    from uno_amd import _native
    nc, Mc = A.shape[2:]
    first, second = mg.call_tensors(op, A, Bm, half)
    if op == 2:
        xt, go = cu(first), cu(second)
        shape = (xt.shape[1], go.shape[1], Mc)
        out = None
        if base is not None:
            out = [torch.empty(shape, dtype=torch.complex64, device=dev()) for _ in range(nc)]
            for c in range(nc):
                out[c].copy_(cu(base[:, :, c]))
        res, ran = _profiled(lambda: _native.mode_wgrad(xt, go, shape, nc, out=out, accumulate=base is not None))
    else:
        inp, ws = cu(first), [cu(w) for w in second]
        res, ran = _profiled(lambda: _native.mode_mix(inp, ws, op))
    return mg.to_gemm_form(op, res), ran


def _compare(what, got, c):
    """finite, relative L2, per-entry bound; prints the figures first"""
    ref = c["ref"]
    got = got.to(ref.device)
    assert got.shape == ref.shape
    finite = bool(torch.isfinite(torch.view_as_real(got)).all())
    err, ratio = mg.rel_l2(got, ref), mg.worst_ratio(got, ref, c["bound_re"], c["bound_im"])
    print(f"{what}: rel L2 {err:.3g}, worst |got - ref| / bound {ratio:.3g}")
    assert finite
    assert err < TOL
    assert ratio <= 1.0


@pytest.mark.parametrize("entry", SINGLES, ids=mg.entry_id)
def test_single_launch_against_float64(entry, monkeypatch):
    flavour, op, shape = mg.flavour_of(entry["config"]), entry["op"], tuple(entry["shape"])
    plan = mg.entry_plan(entry)
    assert list(plan) == entry["plan"] and mg.config_of_plan(plan) == entry["config"], mg.REGENERATE
    c = _case(op, shape, flavour == "half", flavour == "acc")
    zone = RedZone(monkeypatch)
    got, ran = _call(op, c["A"], c["Bm"], c["base"], flavour == "half")
    assert zone.check(mg.entry_id(entry)) >= 1
    assert ran == [plan.kernel], f"{mg.REGENERATE}; ran {ran}"
    _compare(mg.entry_id(entry), got, c)
    if entry["role"] == "stressed":
        again, ran2 = _call(op, c["A"], c["Bm"], c["base"], flavour == "half")
        assert zone.check(mg.entry_id(entry)) >= 1
        assert ran2 == ran and torch.equal(again, got)


# ---------------------------------------------------------------------------------------------------------------- pair launches
def _pair_operands(shape, seed):
    """X (B, Ci, nc, Mc), gO (B, Co, nc, Mc), W (Ci, Co, nc, Mc) complex64 such that both roles' GEMM operands have their own magnitude per
    row of A and per column of B: X per input channel (role b's rows), W per input channel (role a's columns), gO per batch entry (role
    a's rows) times per output channel (role b's columns), each factor 10 ** U(-1, 1)"""
    B, Ci, Co, nc, Mc = shape
    rng = np.random.default_rng(seed)
    cplx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    mag = lambda n, span: 10.0 ** rng.uniform(-span, span, size=n)
    X = (cplx(B, Ci, nc, Mc) * mag(Ci, 2.0)[None, :, None, None]).astype(np.complex64)
    W = (cplx(Ci, Co, nc, Mc) * mag(Ci, 2.0)[:, None, None, None]).astype(np.complex64)
    gO = (cplx(B, Co, nc, Mc) * mag(B, 1.0)[:, None, None, None] * mag(Co, 1.0)[None, :, None, None]).astype(np.complex64)
    return X, gO, W


@pytest.mark.parametrize("entry", PAIRS, ids=mg.entry_id)
def test_pair_launch_against_singles_and_float64(entry, monkeypatch):
    from uno_amd import _native
    acc, shape = mg.flavour_of(entry["config"]) == "acc", tuple(entry["shape"])
    B, Ci, Co, nc, Mc = shape
    pp = mg.entry_plan(entry)
    assert [*pp[:4], *pp.a, *pp.b] == entry["plan"] and mg.config_of_pair_plan(pp) == entry["config"], mg.REGENERATE
    X, gO, W = _pair_operands(shape, mg.entry_seed(entry))
    base = mg.base_values((Ci, Co, nc, Mc), mg.entry_seed(entry)) if acc else None
    device = _reference_device(shape)
    # role a (op 1): A = gO, Bm[k = o, n = i] = conj(W[i, o]); role b (op 2): A[m = i, k = b] = conj(X[b, i]), Bm = gO
    A_a, Bm_a = gO, np.ascontiguousarray(np.conj(W).transpose(1, 0, 2, 3))
    A_b, Bm_b = np.ascontiguousarray(np.conj(X).transpose(1, 0, 2, 3)), gO
    ca = dict(zip(("ref", "bound_re", "bound_im"), mg.reference_and_bound(A_a, Bm_a, None, device)))
    cb = dict(zip(("ref", "bound_re", "bound_im"), mg.reference_and_bound(A_b, Bm_b, base, device)))
    if device.type != "cpu":
        mg.host_slice_check(A_a, Bm_a, ca["ref"])
        mg.host_slice_check(A_b, Bm_b, cb["ref"], base)
    xt, go, ws = cu(X), cu(gO), [cu(W[:, :, c]) for c in range(nc)]

    def buffers():
        if not acc:
            return None
        out = [torch.empty((Ci, Co, Mc), dtype=torch.complex64, device=dev()) for _ in range(nc)]
        for c in range(nc):
            out[c].copy_(cu(base[:, :, c]))
        return out

    zone = RedZone(monkeypatch)
    out = buffers()
    (gX, gws), ran = _profiled(lambda: _native.mode_backward(xt, go, ws, out=out, accumulate=acc))
    assert zone.check(mg.entry_id(entry)) >= 2
    assert ran == pp.kernels and len(ran) == 1 and "pair" in ran[0], f"{mg.REGENERATE}; ran {ran}"
    gX = gX.view(B, Ci, nc, Mc)
    gW = torch.stack(gws, dim=2)
    _compare(mg.entry_id(entry) + " input gradient", gX, ca)
    _compare(mg.entry_id(entry) + " weight gradient", gW, cb)
    # the two single launches: the same kernel bodies, bit for bit
    gX1, ran_a = _profiled(lambda: _native.mode_mix(go, ws, 1))
    gw1, ran_b = _profiled(lambda: _native.mode_wgrad(xt, go, (Ci, Co, Mc), nc, out=buffers(), accumulate=acc))
    assert ran_a == [pp.a.kernel] and ran_b == [pp.b.kernel]
    assert torch.equal(gX1, gX)
    assert torch.equal(torch.stack(gw1, dim=2), gW)


# ---------------------------------------------------------------------------------------------------------------- isolation
def _one_stressed_entry_per_kernel():
    """... with the widest K split the kernel has in the table (plan[7] = KS): the LDS reduction and the most ragged K ranges per wave"""
    picked = {}
    for e in sorted(SINGLES, key=lambda e: -e["plan"][7]):
        if e["role"] == "stressed" and not e["config"].endswith("huge_out"):
            picked.setdefault(e["config"].split("/KS")[0].rsplit("/padded", 1)[0], e)
    return list(picked.values())


ISOLATION = _one_stressed_entry_per_kernel()


def test_isolation_covers_every_compiled_single_kernel():
    assert len({mg.entry_plan(e).kernel for e in ISOLATION}) == len(ISOLATION) == 18


@pytest.mark.parametrize("entry", ISOLATION, ids=mg.entry_id)
def test_nan_in_one_element_reaches_exactly_its_outputs(entry):
    """the kernels' comments promise that modes and rows past the end "never mix with valid ones" and that dead K steps are selected away,
    not multiplied by zero; more generally out[m, n, mode] depends on row m of A and column n of B of that mode alone.  The poisoned
    element is the last row (column), last k, last mode of the last corner: the ragged tails of every axis."""
    flavour, op, shape = mg.flavour_of(entry["config"]), entry["op"], tuple(entry["shape"])
    half = flavour == "half"
    c = mg.case(op, shape, half=half, acc=flavour == "acc")
    kernel = mg.entry_plan(entry).kernel
    clean, ran = _call(op, c["A"], c["Bm"], c["base"], half)
    assert ran == [kernel] and bool(torch.isfinite(torch.view_as_real(clean)).all())
    nan = np.complex64(complex(float("nan"), float("nan")))
    for which in ("A", "Bm"):
        A, Bm = c["A"].copy(), c["Bm"].copy()
        hit = torch.zeros(clean.shape, dtype=torch.bool, device=clean.device)
        if which == "A":
            A[-1, -1, -1, -1] = nan
            hit[-1, :, -1, -1] = True
        else:
            Bm[-1, -1, -1, -1] = nan
            hit[:, -1, -1, -1] = True
        got, ran = _call(op, A, Bm, c["base"], half)
        assert ran == [kernel]
        parts = torch.view_as_real(got)
        assert bool(torch.isnan(parts[hit]).all()), f"NaN in {which}: an output that depends on it is not NaN"
        same = torch.view_as_real(got).view(torch.int32)[~hit] == torch.view_as_real(clean).view(torch.int32)[~hit]
        assert bool(same.all()), f"NaN in {which}: {int((~same).sum())} parts of outputs that do not depend on it changed"


# ---------------------------------------------------------------------------------------------------------------- degenerate calls
@pytest.mark.parametrize("shape", [(0, 3, 4, 2, 5), (0, 17, 33, 4, 27)])
def test_empty_batch(shape, monkeypatch):
    from uno_amd import _native
    B, Ci, Co, nc, Mc = shape
    d = dev()
    ws = [torch.randn(Ci, Co, Mc, dtype=torch.complex64, device=d) for _ in range(nc)]
    xt = torch.zeros((0, Ci, nc, Mc), dtype=torch.complex64, device=d)
    go = torch.zeros((0, Co, nc, Mc), dtype=torch.complex64, device=d)
    zone = RedZone(monkeypatch)
    for op, inp, cout in ((0, xt, Co), (1, go, Ci)):
        assert _native.mode_gemm_plan(op, *shape).family == 0
        out, ran = _profiled(lambda: _native.mode_mix(inp, ws, op))
        assert tuple(out.shape) == (0, cout, nc, Mc) and ran == []
    # the weight gradient of no samples: exact zeros over whatever the buffers held (the guard pattern) ...
    gws, ran = _profiled(lambda: _native.mode_wgrad(xt, go, (Ci, Co, Mc), nc))
    assert ran == [] and all(bool((torch.view_as_real(g) == 0).all()) for g in gws)
    # ... and nothing at all when accumulating
    base = [torch.randn(Ci, Co, Mc, dtype=torch.complex64, device=d) for _ in range(nc)]
    out = [torch.empty((Ci, Co, Mc), dtype=torch.complex64, device=d) for _ in range(nc)]
    for o, b in zip(out, base):
        o.copy_(b)
    gws, ran = _profiled(lambda: _native.mode_wgrad(xt, go, (Ci, Co, Mc), nc, out=out, accumulate=True))
    assert ran == [] and all(torch.equal(g, b) for g, b in zip(gws, base))
    gX, gws = _native.mode_backward(xt, go, ws, out=out, accumulate=True)
    assert tuple(gX.shape) == (0, Ci, nc * Mc) and all(torch.equal(g, b) for g, b in zip(gws, base))
    assert zone.check("empty batch") >= 1


@pytest.mark.parametrize("nc", [1, 2, 4])
@pytest.mark.parametrize("op", [0, 1, 2])
def test_one_by_one_by_one_on_one_mode(op, nc, monkeypatch):
    """Ci = Co = B = 1 with one mode per corner: a single complex product per corner (one rounding per real product and addition)"""
    shape = (1, 1, 1, nc, 1)
    c = mg.case(op, shape)
    zone = RedZone(monkeypatch)
    got, ran = _call(op, c["A"], c["Bm"], None, False)
    assert zone.check("1 x 1 x 1") >= 1
    from uno_amd import _native
    assert ran == [_native.mode_gemm_plan(op, *shape).kernel]
    _compare(f"1x1x1 op {op}, {nc} corners", got, c)
