"""CPU side of the per-mode GEMM instances suite (no GPU): the table tests/golden/mode_gemm_instances.json and the UNREACHABLE list below
partition the declared configuration space of mode_gemm_instances.py; every entry still gets the recorded plan from the library; the
plan query is a pure function of its arguments and is what the launchers decided before it existed; the 2 GiB operand guard answers
from the library itself; and the per-entry float32 bound is not so tight that a correct complex64 evaluation fails it.

THE SCAN BOX (mode_gemm_instances.SCAN_CHANNELS / SCAN_CORNERS / SCAN_GROUPS): B, Ci, Co each from 19 values between 1 and 256, 1 / 2 / 4
corners, the 33 mode counts around the padded edges of 1, 2, 3, 5, 12, 47, 48, 50 and 64 mode groups per corner, no limit on the work:
every combination goes through uno_mode_gemm_plan and through uno_mode_backward_plan once (about 0.7 million calls each)."""
import ctypes

import numpy as np
import pytest
import torch

import mode_gemm_instances as mg

# Declared configurations that no call reaches, each with its reason; test_partition_and_unreachable holds the scan box to it.  All
# are pair launches whose input-gradient role a neither splits K nor has the adjacent-modes map of the weight-gradient role b.  Both
# roles see the same nc corners of g mode groups; role b exists only with Ci, Co >= 16, so role a has K = Co >= 16 and splits K
# whenever it has fewer than 2048 tasks and is not adjacent.  With t_a, t_b the roles' tiles per mode group, a role is adjacent
# iff g >= 48 and ceil(nc g / 4) t >= 200.
_NO_B_ONLY = "role b adjacent needs g >= 48; role a is then not adjacent only with ceil(nc g / 4) t_a < 200, under 800 tasks: it splits K"
_NO_A_ONLY = ("t_b = ceil(Ci / 16) ceil(Co / 8) >= 2 ceil(Ci / 16) is never below t_a (ceil(Ci / 16) for B <= 8, ceil(Ci / 8) for 9 <= B <= 15; B >= 16 "
              "needs Co > 32, t_b >= 5 ceil(Ci / 16) >= 2 ceil(Ci / 8)): where role a is adjacent, role b is too")
UNREACHABLE = {mg.pair_config(v, flavour, 1, adj, badj): why
               for v in mg.PAIR_VARIANTS for flavour in mg.PAIR_FLAVOURS for adj, badj, why in ((0, 1, _NO_B_ONLY), (1, 0, _NO_A_ONLY))}

TABLE = mg.load_table()
SINGLES = [e for e in TABLE if mg.family_of(e["config"]) != "pair"]
PAIRS = [e for e in TABLE if mg.family_of(e["config"]) == "pair"]


# ---------------------------------------------------------------------------------------------------------------- the parent's logic
# A transcription of launch_mode_gemm / blocks_plan / blocks_grid / launch_blocks_t / launch_mode_gemm_pair as they stood BEFORE the plan
# function existed (each launcher decided inline), kept for test_plan_equals_the_parents_inline_logic alone: nothing else may use it.
def _parent_plan(M, N, K, nc, Mc):
    """-> the plan's ints [0, 4 ... 8, 12 ... 15] (family, qc, pipe, variant, KS, adjacent, grid x y z, lds)"""
    groups = (Mc + 15) // 16
    padded = 16 * groups * 5 > Mc * 6
    short_k = K <= 32 and M >= 16 and N >= 16
    huge_out = short_k and 8.0 * M * N * Mc * nc > 200e6
    tiles = ((N + 15) // 16) * ((M + 15) // 16)
    narrow = nc * groups * tiles < 512 and K >= 96 and K % 2 == 0
    if not padded and not huge_out:
        wide_m = M > 8
        tm, tn = (16, 8) if wide_m else (8, 16)
        tiles_per_group = ((M + tm - 1) // tm) * ((N + tn - 1) // tn)
        tasks = nc * groups * tiles_per_group
        adjacent = groups >= 48 and ((nc * groups + 3) // 4) * tiles_per_group >= 200
        KS = 1 if (short_k or adjacent) else 4 if (tasks < 1024 and K >= 32) else 2 if (tasks < 2048 and K >= 16) else 1
        variant = 0 if short_k else 1 if wide_m else 2
        MTW, NTW = ((4, 4), (4, 2), (2, 4))[variant]
        ngroups, mgroups = (N + 4 * NTW - 1) // (4 * NTW), (M + 4 * MTW - 1) // (4 * MTW)
        per_wg = 1 if adjacent else 4 // KS
        per_group = ((ngroups + per_wg - 1) // per_wg) * mgroups
        sub = 4 // KS
        wg_groups = (nc * groups + sub - 1) // sub if adjacent else nc * groups
        return (2, 0, 0, variant, KS, int(adjacent), ((wg_groups + 7) // 8) * 8 * per_group, 1, 1, 4 * MTW * NTW * 8 * 64 * 4 if KS > 1 else 0)
    qc = 8 if narrow else 16
    nq = (Mc + qc - 1) // qc
    pipe = narrow and nc * nq <= 32
    sb, out = 2 * 2 * qc * (8 * 16 + 64 // qc), 16 * 16 * (qc + 1) * 2
    return (1, qc, int(pipe), -1, 0, 0, nc * nq, (N + 15) // 16, (M + 15) // 16, max((2 if pipe else 1) * sb, out) * 4)


def _parent_pair(a, b):
    """launch_mode_gemm_pair's decision from the two roles' _parent_plan: (paired, Ga, grid, lds)"""
    if a[0] != 2 or b[0] != 2 or a[3] == 0 or b[3] != 0:
        return (0, 0, 0, 0)
    return (1, a[6], a[6] + b[6], max(a[9], b[9]))


_COMPARED = (0, 4, 5, 6, 7, 8, 12, 13, 14, 15)


# ---------------------------------------------------------------------------------------------------------------- the scans
@pytest.fixture(scope="module")
def scans():
    """both plan queries over the scan box, once: ({ints: first shape} of uno_mode_gemm_plan, the same of uno_mode_backward_plan, the
    points where a plan is not what _parent_plan / _parent_pair say)"""
    modes = mg.mode_counts(mg.SCAN_GROUPS)
    single, pair, differ = {}, {}, []
    for shape, ints in mg.scan_plans(mg.SCAN_CHANNELS, mg.SCAN_CORNERS, modes, None):
        single.setdefault(ints, shape)
        B, Ci, Co, nc, Mc = shape
        if (ints[0], *ints[4:9], *ints[12:16]) != _parent_plan(B, Co, Ci, nc, Mc):
            differ.append((shape, ints))
    for shape, ints in mg.scan_plans(mg.SCAN_CHANNELS, mg.SCAN_CORNERS, modes, None, pair=True):
        pair.setdefault(ints, shape)
        B, Ci, Co, nc, Mc = shape
        a, b = _parent_plan(B, Ci, Co, nc, Mc), _parent_plan(Ci, Co, B, nc, Mc)
        if (ints[4], *ints[8:13], *ints[16:20]) != a or (ints[20], *ints[24:29], *ints[32:36]) != b or ints[:4] != _parent_pair(a, b):
            differ.append((shape, ints))
    return single, pair, differ


def test_declared_space():
    space = mg.declared_space()
    assert len(space) == len(set(space)) == 12 + 30 + 32
    kernels = {c.split("/")[0] + "/" + c.split("/")[1] for c in space}
    assert len(kernels) == 9 + 9 + 4                      # the compiled kernels: 9 LDS-staged, 9 blocks, 4 pair


def test_partition_and_unreachable(scans):
    """table + UNREACHABLE = the declared space, disjoint, nothing skipped; the scan box reaches no UNREACHABLE configuration (in either
    flavour: the flavour does not enter the decision, test_flavour_and_op_do_not_change_the_decision) and nothing outside the space"""
    space = set(mg.declared_space())
    table = {e["config"] for e in TABLE}
    assert not table & set(UNREACHABLE), sorted(table & set(UNREACHABLE))
    assert table | set(UNREACHABLE) == space, f"neither in the table nor UNREACHABLE: {sorted(space - table - set(UNREACHABLE))}; not declared: {sorted((table | set(UNREACHABLE)) - space)}"
    assert all(isinstance(why, str) and why for why in UNREACHABLE.values())
    single, pair, _ = scans
    seen = {mg.config_of_plan(mg.plan_from_ints(i)) for i in single}
    seen |= {mg.config_of_pair_plan(mg.plan_from_ints(i, pair=True)) for i in pair} - {None}
    assert seen <= space, sorted(seen - space)
    plain = lambda c: c.replace("/acc/", "/plain/").replace("/half/", "/plain/")
    reached = {c for c in UNREACHABLE if plain(c) in seen}
    assert not reached, f"reachable after all: {sorted(reached)}"
    # and every reachable configuration's plain form is met by the box or sits in the table with a confirmed shape (huge_out: beyond the box)
    assert {plain(c) for c in table if not c.endswith("huge_out")} <= seen


def test_table_demonstrably_includes_the_rare_configurations():
    table = {e["config"] for e in TABLE}
    for flavour in mg.FLAVOURS:
        assert mg.lds_config(8, 0, flavour, "padded") in table              # mode_gemm_kernel<8, false, ...>
        assert mg.lds_config(16, 0, flavour, "padded") in table and mg.lds_config(16, 0, flavour, "huge_out") in table
        for v in range(3):
            assert mg.blocks_config(v, flavour, 1, 1) in table              # every adjacent_modes = 1 configuration


def test_every_configuration_has_its_shapes():
    """per configuration and op of its flavour: the smallest and a stressed shape; stressed shapes meet all criteria (pair: both roles) and
    have 2 and 4 corners between them in every family"""
    from uno_amd import _native
    for config in {e["config"] for e in TABLE}:
        mine = [e for e in TABLE if e["config"] == config]
        ops = [None] if mg.family_of(config) == "pair" else mg.FLAVOUR_OPS[mg.flavour_of(config)]
        assert sorted((e.get("op"), e["role"]) for e in mine) == sorted((op, role) for op in ops for role in ("smallest", "stressed")), config
    for e in TABLE:
        B, Ci, Co, nc, Mc = e["shape"]
        if e["role"] != "stressed":
            continue
        assert nc in (2, 4)
        if e["config"].endswith("huge_out"):
            M, N, K = mg.gemm_dims(e["op"], B, Ci, Co)
            assert M % 4 and N % 4 and Mc % 16 and K % 2 and K > 8 and (nc * ((Mc + 15) // 16)) % 8
        elif mg.family_of(e["config"]) == "pair":
            pp = mg.entry_plan(e)
            strict = "aKS2/aadj0/badj1" not in e["config"] or "pair<4, 2, 4>" not in e["config"]           # see stress_failures
            assert not mg.stress_failures((pp.a.M, pp.a.N, pp.a.K), nc, Mc, pp.a, min_K=16, strict_rows=strict), mg.entry_id(e)
            assert not mg.stress_failures((pp.b.M, pp.b.N, pp.b.K), nc, Mc, pp.b), mg.entry_id(e)
        else:
            assert not mg.stress_failures(mg.gemm_dims(e["op"], B, Ci, Co), nc, Mc, mg.entry_plan(e)), mg.entry_id(e)
    for family in ("lds", "blocks", "pair"):
        assert {e["shape"][3] for e in TABLE if e["role"] == "stressed" and mg.family_of(e["config"]) == family} == {2, 4}
    # only the huge_out entries are large
    for e in TABLE:
        B, Ci, Co, nc, Mc = e["shape"]
        if e["config"].endswith("huge_out"):
            M, N, K = mg.gemm_dims(e["op"], B, Ci, Co)
            assert 200e6 < 8 * M * N * nc * Mc < 201e6 and K <= 32
        else:
            assert B * Ci * Co * nc * Mc <= 1e8


@pytest.mark.parametrize("entry", TABLE, ids=mg.entry_id)
def test_entry_is_still_current(entry):
    plan = mg.entry_plan(entry)
    ints = [*plan[:4], *plan.a, *plan.b] if mg.family_of(entry["config"]) == "pair" else list(plan)
    assert ints == entry["plan"], mg.REGENERATE
    config = mg.config_of_pair_plan(plan) if mg.family_of(entry["config"]) == "pair" else mg.config_of_plan(plan)
    assert config == entry["config"], mg.REGENERATE


def test_plan_equals_the_parents_inline_logic(scans):
    """the launch decisions are what they were before one plan function made them: every plan of the scan box (and of the table's shapes,
    which include the huge_out ones) against the transcription of the parent commit's inline logic"""
    from uno_amd import _native
    k = _native.MODE_GEMM_PLAN_INTS
    assert not scans[2], f"{len(scans[2])} plans of the scan box differ from the parent's logic, first: {scans[2][:3]}"
    for e in SINGLES:
        B, Ci, Co, nc, Mc = e["shape"]
        want = _parent_plan(*mg.gemm_dims(e["op"], B, Ci, Co), nc, Mc)
        assert tuple(e["plan"][i] for i in _COMPARED) == want, (mg.entry_id(e), want)
    for ints, (B, Ci, Co, nc, Mc) in [(tuple(e["plan"]), tuple(e["shape"])) for e in PAIRS]:
        a, b = _parent_plan(B, Ci, Co, nc, Mc), _parent_plan(Ci, Co, B, nc, Mc)
        assert tuple(ints[4 + i] for i in _COMPARED) == a and tuple(ints[4 + k + i] for i in _COMPARED) == b, ((B, Ci, Co, nc, Mc), ints)
        assert tuple(ints[:4]) == _parent_pair(a, b), ((B, Ci, Co, nc, Mc), ints)


def _sample(seed, n):
    rng = np.random.default_rng(seed)
    modes = mg.mode_counts(mg.SCAN_GROUPS)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    return [(pick(mg.SCAN_CHANNELS), pick(mg.SCAN_CHANNELS), pick(mg.SCAN_CHANNELS), pick(mg.SCAN_CORNERS), pick(modes)) for _ in range(n)]


def test_plan_is_a_pure_function():
    """the same arguments give the same answer, whatever was asked in between; the two roles of uno_mode_backward_plan are the two single
    plans (paired or not), and a pair is reported only for two 4x4x1 plans"""
    from uno_amd import _native
    shapes = _sample(11, 3000)
    first = [(_native.mode_gemm_plan(1, *s), _native.mode_gemm_plan(2, *s, accumulate=True), _native.mode_backward_plan(*s, accumulate=True)) for s in shapes]
    for s, (a, b, pp) in zip(reversed(shapes), reversed(first)):
        assert _native.mode_backward_plan(*s, accumulate=True) == pp and _native.mode_gemm_plan(2, *s, accumulate=True) == b and _native.mode_gemm_plan(1, *s) == a
        assert pp.a == a and pp.b == b
        if pp.paired:
            assert a.family == b.family == 2 and (pp.Ga, pp.grid, pp.lds) == (a.grid_x, a.grid_x + b.grid_x, max(a.lds, b.lds))
        else:
            assert (pp.Ga, pp.grid, pp.lds) == (0, 0, 0)
            assert pp.kernels == [b.kernel, a.kernel]


def test_flavour_and_op_do_not_change_the_decision():
    """the decision depends on (M, N, K, corners, modes) alone: every op and flavour that gives the same GEMM gives the same plan but for
    the half / acc flags - which is why one scan with op 0 and complex64 weights speaks for all of them"""
    from uno_amd import _native
    for B, Ci, Co, nc, Mc in _sample(12, 3000):
        base = _native.mode_gemm_plan(0, B, Ci, Co, nc, Mc)
        M, N, K = mg.gemm_dims(0, B, Ci, Co)
        for op in (0, 1, 2):
            for half, acc in ((False, False), (True, False), (False, True), (True, True)):
                got = _native.mode_gemm_plan(op, *mg.call_dims(op, M, N, K), nc, Mc, w_half=half, accumulate=acc)
                h, a = int(half and op != 2), int(acc and op == 2)
                assert got == base._replace(half=h, acc=a), (op, half, acc, (B, Ci, Co, nc, Mc))
        plain, acc = _native.mode_backward_plan(B, Ci, Co, nc, Mc), _native.mode_backward_plan(B, Ci, Co, nc, Mc, accumulate=True)
        assert acc == plain._replace(b=plain.b._replace(acc=1))


def test_degenerate_plans_and_argument_errors():
    from uno_amd import _native
    lib = _native.lib()
    for op in (0, 1, 2):
        p = _native.mode_gemm_plan(op, 0, 3, 4, 2, 5)
        assert p.family == 0 and p.kernel is None and set(p) == {0}
    pp = _native.mode_backward_plan(0, 3, 4, 2, 5)
    assert not pp.paired and pp.kernels == []
    buf = (ctypes.c_int * _native.MODE_BACKWARD_PLAN_INTS)()
    g, b = lib.uno_mode_gemm_plan, lib.uno_mode_backward_plan
    for call, needle in ((lambda: g(0, 1, 1, 1, 2, 1, 0, 0, None), b"null"), (lambda: g(3, 1, 1, 1, 2, 1, 0, 0, buf), b"op must be"),
                         (lambda: g(0, 1, 0, 1, 2, 1, 0, 0, buf), b"bad sizes"), (lambda: g(0, -1, 1, 1, 2, 1, 0, 0, buf), b"bad sizes"),
                         (lambda: g(0, 1, 1, 1, 5, 1, 0, 0, buf), b"ncorner"), (lambda: b(1, 1, 1, 2, 0, 0, buf), b"bad sizes"),
                         (lambda: b(1, 1, 1, 2, 1, 0, None), b"null")):
        rc = call()
        assert rc == -1 and needle in lib.uno_last_error(), (rc, lib.uno_last_error())


def test_two_gib_operand_guard():
    """byte offsets inside an operand are 32-bit: an operand of 2 GiB per corner is refused with code -2 and "spans" in the message - by
    the real calls (before anything touches a device: placeholder pointers, as in test_capi_symbols.py) and by the plan queries, which plan
    the same call with one mode fewer.  One corner, so that the operand is the whole tensor: B x C x modes x 8 bytes = 2^31."""
    from uno_amd import _native
    lib = _native.lib()
    raw = ctypes.create_string_buffer(64)
    p = ctypes.cast(raw, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 4)(p.value, p.value, p.value, p.value)
    B, C, Mc = 256, 256, 4096
    assert B * C * Mc * 8 == 2 ** 31
    plan = (ctypes.c_int * _native.MODE_BACKWARD_PLAN_INTS)()
    calls = {
        "uno_mode_mix op 0 (the activations)": lambda m: lib.uno_mode_mix(p, arr, p, 0, B, C, 4, 1, m, None),
        "uno_mode_mix op 1 (the output gradient)": lambda m: lib.uno_mode_mix(p, arr, p, 1, B, 4, C, 1, m, None),
        "uno_mode_mix op 0 (the weights)": lambda m: lib.uno_mode_mix(p, arr, p, 0, 4, B, C, 1, m, None),
        "uno_mode_wgrad (the activations)": lambda m: lib.uno_mode_wgrad(p, p, arr, B, C, 4, 1, m, None),
        "uno_mode_wgrad (the output gradient)": lambda m: lib.uno_mode_wgrad(p, p, arr, B, 4, C, 1, m, None),
        "uno_mode_backward": lambda m: lib.uno_mode_backward(p, p, arr, p, arr, B, C, 4, 1, m, 0, None),
    }
    for what, call in calls.items():
        rc = call(Mc)
        assert rc == -2 and b"spans" in lib.uno_last_error(), (what, rc, lib.uno_last_error())
    queries = {
        "plan op 0 (the activations)": lambda m: lib.uno_mode_gemm_plan(0, B, C, 4, 1, m, 0, 0, plan),
        "plan op 1 (the output gradient)": lambda m: lib.uno_mode_gemm_plan(1, B, 4, C, 1, m, 0, 0, plan),
        "plan op 0 (the weights)": lambda m: lib.uno_mode_gemm_plan(0, 4, B, C, 1, m, 0, 0, plan),
        "plan op 2 (the activations)": lambda m: lib.uno_mode_gemm_plan(2, B, C, 4, 1, m, 0, 1, plan),
        "plan op 2 (the output gradient)": lambda m: lib.uno_mode_gemm_plan(2, B, 4, C, 1, m, 0, 0, plan),
        "backward plan": lambda m: lib.uno_mode_backward_plan(B, C, 4, 1, m, 0, plan),
    }
    for what, query in queries.items():
        rc = query(Mc)
        assert rc == -2 and b"spans" in lib.uno_last_error(), (what, rc, lib.uno_last_error())
        assert query(Mc - 1) == 0 and plan[0] in (0, 1, 2), (what, lib.uno_last_error())
    with pytest.raises(RuntimeError, match="spans"):
        _native.mode_gemm_plan(0, B, C, 4, 1, Mc)
    assert _native.mode_gemm_plan(0, B, C, 4, 1, Mc - 1).family == 2


# ---------------------------------------------------------------------------------------------------------------- the bound
SLICE_ABOVE = 2000000          # multiply-adds above which the complex64 check takes the first rows and columns of the entry


def _float32_ratio(op, shape, half, acc):
    """a complex64 torch.einsum of the entry's operands (the CPU's own float32 arithmetic and order) against the float64 reference:
    worst |c64 - ref| / bound"""
    A, Bm = mg.gemm_operands(op, shape, half=half)
    M, N = A.shape[0], Bm.shape[1]
    if A.shape[1] * M * N * A.shape[2] * A.shape[3] > SLICE_ABOVE:
        A, Bm = A[:3], Bm[:, :3]
    base = mg.base_values((A.shape[0], Bm.shape[1], *A.shape[2:]), mg.shape_seed(op, shape)) if acc else None
    ref, bre, bim = mg.reference_and_bound(A, Bm, base)
    got = torch.einsum("mkcq,kncq->mncq", torch.from_numpy(A), torch.from_numpy(Bm))
    if acc:
        got = got + torch.from_numpy(base)
    assert got.dtype == torch.complex64
    assert mg.rel_l2(got, ref) < 2e-5
    return mg.worst_ratio(got, ref, bre, bim)


@pytest.mark.parametrize("entry", TABLE, ids=mg.entry_id)
def test_bound_holds_for_a_float32_reference(entry):
    flavour = mg.flavour_of(entry["config"])
    if mg.family_of(entry["config"]) == "pair":
        ratios = [_float32_ratio(1, entry["shape"], False, False), _float32_ratio(2, entry["shape"], False, flavour == "acc")]
    else:
        ratios = [_float32_ratio(entry["op"], entry["shape"], flavour == "half", flavour == "acc")]
    assert max(ratios) <= 1.0, ratios


def test_accumulating_bound_needs_the_base_term_outside_the_sums():
    """what reference_and_bound's docstring says about u |base|: with it multiplied by gamma_n a correctly rounded float32 `base + p` fails"""
    A = np.full((1, 1, 1, 1), 1e-3 + 0j, dtype=np.complex64)
    Bm = np.full((1, 1, 1, 1), 1e-3 + 0j, dtype=np.complex64)
    base = np.full((1, 1, 1, 1), 1.0 + 1.0j, dtype=np.complex64)
    ref, bre, _ = mg.reference_and_bound(A, Bm, base)
    got = torch.from_numpy(A * Bm + base)
    err = float((got.to(torch.complex128) - ref).real.abs())
    assert 0 < err <= float(bre)
    assert err > mg.gamma(1) * (float(abs(A[0, 0, 0, 0].real * Bm[0, 0, 0, 0].real)) + mg.U * 1.0)
