"""Shared by tools/mode_gemm_instance_shapes.py, test_mode_gemm_instances_cpu.py and test_hip_mode_gemm_instances.py: the declared
configuration space of the per-mode complex GEMM K2 / K4 (csrc/mode_gemm.hip), the table of shapes that reach every configuration a call
can reach (tests/golden/mode_gemm_instances.json), seeded inputs, the float64 reference and the per-entry float32 bound.

There is NO Python copy of the dispatch here: which kernel and which run-time configuration a shape takes is asked of the library
(_native.mode_gemm_plan / mode_backward_plan, the plan function the launchers themselves use).  Nothing in this module needs a GPU.

A CONFIGURATION is what the launch decision can vary, written as a string:

    lds<QC, PIPE>/FLAVOUR/REASON            mode_gemm_kernel<QC, PIPE, BH, ACC>; REASON: why the 4x4x1 form was refused
    blocks<MTW, NTW, PF>/FLAVOUR/KSk/adja   mode_gemm_blocks_kernel<MTW, NTW, PF, BH, ACC> with the run-time arguments KS = k, adjacent_modes = a
    pair<MA, NA, 4>/FLAVOUR/aKSk/aadja/badjb   mode_gemm_blocks_pair_kernel<MA, NA, 4, ACCB>: role a (input gradient) with KS = k and
                                            adjacent_modes = a, role b (weight gradient, <4, 4, 2>, KS = 1) with adjacent_modes = b

FLAVOUR: plain, half (fp16 weights, BH) or acc (accumulating, ACC; for the pair: of role b)."""
import functools
import json
import os
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "mode_gemm_instances.json")
REGENERATE = "dispatch changed: regenerate the table tests/golden/mode_gemm_instances.json (tools/mode_gemm_instance_shapes.py)"
U = 2.0 ** -24                                      # unit roundoff of float32

# ---------------------------------------------------------------------------------------------------------------- declared space
FLAVOURS = ("plain", "half", "acc")
# ops a flavour is run through: fp16 weights exist for the forward mix and the input gradient, accumulation for the weight gradient
FLAVOUR_OPS = {"plain": (0, 1, 2), "half": (0, 1), "acc": (2,)}
LDS_KERNELS = ((16, 0), (8, 0), (8, 1))                                     # (QC, PIPE): 3 x 3 flavours = 9 compiled kernels
LDS_REASONS = {(16, 0): ("padded", "huge_out"), (8, 0): ("padded",), (8, 1): ("padded",)}      # 8 modes need K >= 96, huge_out K <= 32
VARIANTS = ("4, 4, 2", "4, 2, 4", "2, 4, 4")                                # <MTW, NTW, PF>: 3 x 3 flavours = 9 compiled kernels
# (KS, adjacent_modes) per variant: <4, 4, 2> is the short-K form and never splits K; adjacent mode groups never split K either
BLOCKS_RUNTIME = {0: ((1, 0), (1, 1)), 1: ((1, 0), (2, 0), (4, 0), (1, 1)), 2: ((1, 0), (2, 0), (4, 0), (1, 1))}
PAIR_VARIANTS = (1, 2)                                                      # role a's variant; x ACCB = 4 compiled kernels
PAIR_FLAVOURS = ("plain", "acc")


def lds_config(qc, pipe, flavour, reason):
    return "lds<{}, {}>/{}/{}".format(qc, "true" if pipe else "false", flavour, reason)


def blocks_config(variant, flavour, KS, adjacent):
    return "blocks<{}>/{}/KS{}/adj{}".format(VARIANTS[variant], flavour, KS, adjacent)


def pair_config(variant, flavour, KS, adjacent, b_adjacent):
    return "pair<{}>/{}/aKS{}/aadj{}/badj{}".format(VARIANTS[variant], flavour, KS, adjacent, b_adjacent)


def declared_space():
    """every configuration the sources can express: 12 LDS-staged, 30 blocks and 32 pair configurations"""
    out = []
    for flavour in FLAVOURS:
        for qc, pipe in LDS_KERNELS:
            out += [lds_config(qc, pipe, flavour, r) for r in LDS_REASONS[(qc, pipe)]]
        for v in range(3):
            out += [blocks_config(v, flavour, ks, adj) for ks, adj in BLOCKS_RUNTIME[v]]
    for flavour in PAIR_FLAVOURS:
        for v in PAIR_VARIANTS:
            out += [pair_config(v, flavour, ks, adj, badj) for ks, adj in BLOCKS_RUNTIME[v] for badj in (0, 1)]
    return out


def flavour_of(config):
    return config.split("/")[1]


def family_of(config):
    """lds, blocks or pair"""
    return config[:config.index("<")]


def config_of_plan(plan):
    """the configuration string of a _native.ModeGemmPlan (None: nothing is launched).  A call that is both padded and huge_out counts as
    padded (the first of the two conditions the plan tests)."""
    flavour = "half" if plan.half else "acc" if plan.acc else "plain"
    if plan.family == 1:
        return lds_config(plan.qc, plan.pipe, flavour, "padded" if plan.refused & 1 else "huge_out")
    if plan.family == 2:
        return blocks_config(plan.variant, flavour, plan.KS, plan.adjacent)
    return None


def config_of_pair_plan(pp):
    """the configuration string of a _native.ModeBackwardPlan, None where the two GEMMs are launched one by one"""
    if not pp.paired:
        return None
    return pair_config(pp.a.variant, "acc" if pp.b.acc else "plain", pp.a.KS, pp.a.adjacent, pp.b.adjacent)


def gemm_dims(op, B, Ci, Co):
    """the role mapping of mode_gemm_params (capi_spectral.hip): op -> (M, N, K)
        op 0  O[b,o]  = sum_i X[b,i] W[i,o]              M = B,  N = Co, K = Ci
        op 1  gX[b,i] = sum_o gO[b,o] conj(W[i,o])       M = B,  N = Ci, K = Co
        op 2  gW[i,o] = sum_b conj(X[b,i]) gO[b,o]       M = Ci, N = Co, K = B"""
    return ((B, Co, Ci), (B, Ci, Co), (Ci, Co, B))[op]


def call_dims(op, M, N, K):
    """the inverse of gemm_dims: (B, Ci, Co)"""
    return ((M, K, N), (M, N, K), (K, M, N))[op]


# ---------------------------------------------------------------------------------------------------------------- table
def load_table():
    with open(TABLE) as fh:
        return json.load(fh)


def entry_id(e):
    tail = "x".join(str(v) for v in e["shape"])
    return "{}-{}-{}-{}".format(e["config"].replace(" ", ""), "op%d" % e["op"] if "op" in e else "bwd", e["role"], tail)


def entry_seed(e):
    return zlib.crc32(repr((e["config"], e.get("op"), e["role"], tuple(e["shape"]))).encode())


def entry_plan(e):
    """the library's plan for the entry's shape, now"""
    from uno_amd import _native
    B, Ci, Co, nc, Mc = e["shape"]
    flavour = flavour_of(e["config"])
    if family_of(e["config"]) == "pair":
        return _native.mode_backward_plan(B, Ci, Co, nc, Mc, accumulate=flavour == "acc")
    return _native.mode_gemm_plan(e["op"], B, Ci, Co, nc, Mc, w_half=flavour == "half", accumulate=flavour == "acc")


# ---------------------------------------------------------------------------------------------------------------- inputs
def _scaled_complex(rng, shape, scale_axis):
    """complex64 standard normals, each index of `scale_axis` with its own magnitude 10 ** U(-2, 2): small outputs next to large ones"""
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    mag = 10.0 ** rng.uniform(-2.0, 2.0, size=shape[scale_axis])
    return (v * mag.reshape([-1 if a == scale_axis else 1 for a in range(len(shape))])).astype(np.complex64)


def shape_seed(op, shape):
    """a seed from the GEMM a call amounts to (stable across processes, unlike hash()): entries of different ops and flavours that are the
    same GEMM share their operands, so a reference serves several of them"""
    B, Ci, Co, nc, Mc = shape
    return zlib.crc32(repr((gemm_dims(op, B, Ci, Co), nc, Mc)).encode())


def gemm_operands(op, shape, half=False):
    """-> (A (M, K, nc, Mc), Bm (K, N, nc, Mc)) complex64 in GEMM form: out[m, n] = sum_k A[m, k] Bm[k, n] per corner and mode, the
    conjugations of ops 1 / 2 already applied.  Each row m of A and each column n of Bm has its own magnitude.  half (ops 0 / 1, where Bm
    holds the weights): Bm's parts are rounded to half precision - the values the device stores - and widened again."""
    B, Ci, Co, nc, Mc = shape
    M, N, K = gemm_dims(op, B, Ci, Co)
    rng = np.random.default_rng(shape_seed(op, shape))
    A = _scaled_complex(rng, (M, K, nc, Mc), 0)
    Bm = _scaled_complex(rng, (K, N, nc, Mc), 1)
    if half:
        assert op != 2
        Bm = (Bm.real.astype(np.float16).astype(np.float32) + 1j * Bm.imag.astype(np.float16).astype(np.float32)).astype(np.complex64)
    return A, Bm


def call_tensors(op, A, Bm, half=False):
    """the tensors of the _native call from the GEMM form:
        op 0 -> (X (B, Ci, nc, Mc), [W_c (Ci, Co, Mc)])         mode_mix(X, W, 0)
        op 1 -> (gO (B, Co, nc, Mc), [W_c (Ci, Co, Mc)])        mode_mix(gO, W, 1): Bm[k = o, n = i] = conj(W[i, o])
        op 2 -> (X (B, Ci, nc, Mc), gO (B, Co, nc, Mc))         mode_wgrad(X, gO): A[m = i, k = b] = conj(X[b, i])
    half: the weights as (Ci, Co, Mc, 2) float16 (re, im) pairs."""
    nc = A.shape[2]
    if op == 2:
        return np.ascontiguousarray(np.conj(A).transpose(1, 0, 2, 3)), np.ascontiguousarray(Bm)
    W = Bm if op == 0 else np.conj(Bm).transpose(1, 0, 2, 3)                  # (Ci, Co, nc, Mc)
    ws = [np.ascontiguousarray(W[:, :, c]) for c in range(nc)]
    if half:
        ws = [np.stack([w.real, w.imag], axis=-1).astype(np.float16) for w in ws]
    return np.ascontiguousarray(A), ws


def base_values(shape_mn, seed):
    """what an accumulating call finds in its output: random, non-zero, (M, N, nc, Mc) complex64 in GEMM form"""
    rng = np.random.default_rng(seed + 7)
    return (rng.standard_normal(shape_mn) + 1j * rng.standard_normal(shape_mn)).astype(np.complex64)


# ---------------------------------------------------------------------------------------------------------------- reference, bound
def gamma(K):
    n = 2 * K + 6
    return n * U / (1.0 - n * U)


def reference_and_bound(A, Bm, base=None, device="cpu"):
    """-> (ref (M, N, nc, Mc) complex128, bound_re, bound_im float64), torch tensors on `device`.

    ref = sum_k A[m, k] Bm[k, n] (+ base), a plain float64 einsum per corner.

    The bound.  A part of an output is a sum of 2 K real products: Re = sum_k (Re a Re b - Im a Im b), Im = sum_k (Re a Im b + Im a Re b).
    A float32 evaluation in ANY order, products fused into the additions or rounded on their own, is off by at most gamma_n times the sum
    of the moduli of its terms (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), n = the number of roundings on a
    term's way to the result: at most 2 K - 1 additions and the product's own rounding = 2 K, plus 6 for what the kernels do beyond one
    chain - the reduction of a K split (up to 3 more additions), the accumulating add's rounding of the product sum, slack.  So

        |Re err| <= gamma_n sum_k (|Re a||Re b| + |Im a||Im b|),   |Im err| <= gamma_n sum_k (|Re a||Im b| + |Im a||Re b|),
        gamma_n = n u / (1 - n u),  u = 2^-24,  n = 2 K + 6.

    Accumulating calls return fl(base + p) for the computed product sum p: that rounding is at most u |base + p| <= u |base| + u |p|; the
    second term is part of the slack above, the first is added to the bound per part: + u |Re base|, + u |Im base|.  (Adding u |base|
    INSIDE the sums, to be multiplied by gamma_n, would leave about u^2 |base| and fail a correctly rounded float32 addition wherever
    |base| is much larger than the product; test_mode_gemm_instances_cpu.py shows a complex64 evaluation within this bound.)
    Sums and bound are float64, from the inputs; nothing here is fitted to the kernels."""
    a = torch.from_numpy(A).to(device).to(torch.complex128)
    b = torch.from_numpy(Bm).to(device).to(torch.complex128)
    nc = a.shape[2]
    ref = torch.stack([torch.einsum("mkq,knq->mnq", a[:, :, c], b[:, :, c]) for c in range(nc)], dim=2)
    ar, ai, br, bi = a.real.abs(), a.imag.abs(), b.real.abs(), b.imag.abs()
    dot = lambda x, y: torch.einsum("mkcq,kncq->mncq", x, y)
    g = gamma(a.shape[1])
    bound_re, bound_im = g * (dot(ar, br) + dot(ai, bi)), g * (dot(ar, bi) + dot(ai, br))
    if base is not None:
        bs = torch.from_numpy(base).to(device).to(torch.complex128)
        ref = ref + bs
        bound_re, bound_im = bound_re + U * bs.real.abs(), bound_im + U * bs.imag.abs()
    return ref, bound_re, bound_im


@functools.lru_cache(maxsize=2)
def _cached_reference(op_is_2, shape, half, device):
    op = 2 if op_is_2 else 0
    A, Bm = gemm_operands(op, shape, half=half)
    return (A, Bm, *reference_and_bound(A, Bm, None, device))


def case(op, shape, half=False, acc=False, device="cpu"):
    """everything a comparison of one call needs, in GEMM form: {A, Bm, base (None unless acc), ref, bound_re, bound_im}.  Calls that are
    the same GEMM (shape_seed) share operands, reference and sums - the last two are kept -, the base is added per call."""
    B, Ci, Co, nc, Mc = shape
    M, N, K = gemm_dims(op, B, Ci, Co)
    canon = 2 if op == 2 else 0
    A, Bm, ref, bre, bim = _cached_reference(op == 2, (*call_dims(canon, M, N, K), nc, Mc), bool(half), str(device))
    out = {"A": A, "Bm": Bm, "base": None, "ref": ref, "bound_re": bre, "bound_im": bim}
    if acc:
        out["base"] = base_values((M, N, nc, Mc), shape_seed(op, shape))
        bs = torch.from_numpy(out["base"]).to(device).to(torch.complex128)
        out["ref"], out["bound_re"], out["bound_im"] = ref + bs, bre + U * bs.real.abs(), bim + U * bs.imag.abs()
    return out


def host_slice_check(A, Bm, ref, base=None, rows=2, cols=3):
    """a reference formed on the device: its first rows / columns against the host's float64 einsum, to 1e-12 relative"""
    a, b = A[:rows].astype(np.complex128), Bm[:, :cols].astype(np.complex128)
    want = np.einsum("mkcq,kncq->mncq", a, b)
    if base is not None:
        want = want + base[:rows, :cols]
    got = ref[:rows, :cols].cpu().numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def worst_ratio(got, ref, bound_re, bound_im):
    """max over entries and parts of |got - ref| / bound; got: complex64 tensor in GEMM form on ref's device.  <= 1 passes"""
    d = got.to(torch.complex128) - ref
    return float(torch.maximum((d.real.abs() / bound_re).max(), (d.imag.abs() / bound_im).max()))


def rel_l2(got, ref):
    return float(torch.linalg.vector_norm(got.to(torch.complex128) - ref) / torch.linalg.vector_norm(ref))


def to_gemm_form(op, out):
    """a call's result as (M, N, nc, Mc): ops 0 / 1 return (B, C, nc, Mc) - that is it; op 2 returns nc tensors (Ci, Co, Mc)"""
    return out if op != 2 else torch.stack(list(out), dim=2)


# ---------------------------------------------------------------------------------------------------------------- scans of the plan query
def mode_counts(group_counts):
    """modes per corner around the edges of the `padded` rule for each number g of 16-mode groups: the smallest count that is not padded
    (ceil(40 g / 3): 14, 27, 40 ...), the largest that is, a group with one mode, and a group one mode short of full"""
    out = set()
    for g in group_counts:
        first = -(-40 * g // 3)
        out |= {first, 16 * g - 1, 16 * (g - 1) + 1}
        if first - 1 > 16 * (g - 1):
            out.add(first - 1)
    return sorted(out)


# THE BOX of the exhaustive scans (test_mode_gemm_instances_cpu.py: what UNREACHABLE is proved over, and where the refactored plan is
# compared with the parent commit's inline logic; tools/mode_gemm_instance_shapes.py: where pair configurations beyond its fine box are
# looked for): B, Ci, Co each from SCAN_CHANNELS - 1, the edges of the 8- and 16-wide tiles, of K <= 32 / >= 16 / >= 32 / >= 96 / even,
# ragged values, and channel counts wide enough for 2048 tasks on 47 mode groups -, 1 / 2 / 4 corners, mode_counts(SCAN_GROUPS) modes per
# corner (up to 1024), no limit on the work.  About 0.7 million calls of each query.
SCAN_CHANNELS = (1, 3, 7, 8, 9, 16, 17, 31, 32, 33, 49, 64, 65, 81, 97, 98, 130, 163, 256)
SCAN_CORNERS = (1, 2, 4)
SCAN_GROUPS = (1, 2, 3, 5, 12, 47, 48, 50, 64)


def scan_plans(channels, corners, modes, work_max, pair=False):
    """every (B, Ci, Co) in channels^3, nc in corners, Mc in modes with B Ci Co nc Mc <= work_max, through the library's plan query:
    uno_mode_gemm_plan(op 0, complex64 weights) or, pair=True, uno_mode_backward_plan(accumulate = 0).  Yields ((B, Ci, Co, nc, Mc), ints).
    The box is symmetric in the three sizes, so op 0 meets every (M, N, K) that ops 1 and 2 would."""
    import ctypes
    from uno_amd import _native
    lib = _native.lib()
    n = _native.MODE_BACKWARD_PLAN_INTS if pair else _native.MODE_GEMM_PLAN_INTS
    buf = (ctypes.c_int * n)()
    channels = sorted(channels)
    for nc in corners:
        for Mc in modes:
            budget = work_max // (nc * Mc) if work_max is not None else 1 << 62
            for B in channels:
                if B > budget:
                    break
                for Ci in channels:
                    if B * Ci > budget:
                        break
                    for Co in channels:
                        if B * Ci * Co > budget:
                            break
                        rc = lib.uno_mode_backward_plan(B, Ci, Co, nc, Mc, 0, buf) if pair else lib.uno_mode_gemm_plan(0, B, Ci, Co, nc, Mc, 0, 0, buf)
                        assert rc == 0, lib.uno_last_error()
                        yield (B, Ci, Co, nc, Mc), tuple(buf)


def plan_from_ints(ints, pair=False):
    from uno_amd import _native
    if not pair:
        return _native.ModeGemmPlan(*ints)
    k = _native.MODE_GEMM_PLAN_INTS
    return _native.ModeBackwardPlan(*ints[:4], _native.ModeGemmPlan(*ints[4:4 + k]), _native.ModeGemmPlan(*ints[4 + k:]))


# ---------------------------------------------------------------------------------------------------------------- stress criteria
def stress_failures(op_dims, nc, Mc, plan, min_K=1, strict_rows=True):
    """why (M, N, K, nc, Mc) under `plan` is NOT a stressed shape (empty list: it is one).  The criteria, all at once:
      * M and N are no multiples of 4 (so none of 16 either) and span more than one tile (16 x 16 outputs; <4, 2, 4>: 16 x 8; <2, 4, 4>,
        which serves M <= 8: 4 x 16), the last tile ragged; more than one 16-mode group per corner;
      * the last mode group of a corner is partly empty: Mc is no multiple of 16 (4x4x1 form: still under the padded limit, or the plan
        would not be this one) and none of the LDS form's QC;
      * K is no multiple of 8 nor of KS x PF; K is odd where the plan allows (the 8-mode LDS form takes even K only); the LDS form has more than one K chunk of 8; K is below the
        prefetch depth PF where the plan allows it (KS = 1: K in 1 ... PF - 1; a split K is at least 16 long);
      * the number of mode-group sets dealt to the 8 XCDs (4x4x1 form), or of mode chunks (LDS form), is no multiple of 8.
    min_K: the shortest K the caller's situation allows (the input-gradient role of a pair launch has K = Co >= 16).
    strict_rows=False: <4, 2, 4> with M in 9 ... 15 - one ragged 16-row tile - passes (a pair launch whose <4, 2, 4> role splits K in two
    beside an adjacent weight-gradient role has fewer than 800 tasks and K = Co < 32, and then M = B >= 16 would make it <4, 4, 2>)."""
    M, N, K = op_dims
    why = []
    if M % 4 == 0 or N % 4 == 0:
        why.append("M or N a multiple of 4")
    # more than one tile of a wave / workgroup along M and N, the last one ragged (<2, 4, 4> serves M <= 8: more than one 4-row tile),
    # and more than one mode group per corner
    tile_m, tile_n = (16, 16) if plan.family == 1 else ((16, 16), (16 if strict_rows else 8, 8), (4, 16))[plan.variant]
    if M <= tile_m or N <= tile_n:
        why.append("a single tile along M or N")
    if Mc <= 16:
        why.append("a single mode group per corner")
    if Mc % 16 == 0 or (plan.family == 1 and Mc % plan.qc == 0):
        why.append("whole last mode group")
    if plan.family == 1:
        if K % 8 == 0 or (plan.qc == 16 and K % 2 == 0):
            why.append("K a multiple of 8, or even where odd is possible")
        if K <= 8:
            why.append("a single K chunk")
        if (nc * ((Mc + plan.qc - 1) // plan.qc)) % 8 == 0:
            why.append("mode chunks a multiple of 8")
    else:
        pf = 2 if plan.variant == 0 else 4
        if K % 8 == 0 or K % (plan.KS * pf) == 0 or K % 2 == 0:
            why.append("K even or a multiple of KS x PF")
        if plan.KS == 1 and pf > 2 and K >= pf and min_K < pf:
            why.append("K not below the prefetch depth")
        if pf == 2 and K < 3:
            why.append("K = 1: no K loop to speak of (a prefetch depth of 2 leaves only that below it; the smallest shapes have it)")
        groups = nc * ((Mc + 15) // 16)
        sets = (groups + 4 // plan.KS - 1) // (4 // plan.KS) if plan.adjacent else groups
        if sets % 8 == 0:
            why.append("mode-group sets a multiple of 8")
    return why
