"""Shared by tools/dft3d_instance_shapes.py, test_dft3d_instances_cpu.py and test_hip_dft3d_instances.py: a Python mirror of the host-side
geometry of the one-workgroup-per-volume 3-D transforms K1v / K3v (csrc/dft3d_volume.hip: vol_shape, vol_inv_shape, the two `applies`
functions and the two dispatchers), the table of shapes that reach every instantiation a call can reach
(tests/golden/dft3d_instances.json), the census of the instantiations compiled into the library (symbol names only), and the
float64 references with their per-entry float32 bounds.

No GPU is needed for anything in this module."""
import functools
import json
import os
import re
import zlib

import numpy as np

import dft2d_instances as di
from oracle import spectral_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "dft3d_instances.json")
LIBRARY = di.LIBRARY
# template -> kinds of its arguments in order (i: int, b: bool), as ProfScope prints them
TEMPLATES = {"dft3d_fwd_volume_kernel": "iibi",        # <MT2, NBW, NARROW, U>
             "dft3d_inv_volume_kernel": "iiiib"}       # <MTS, U, NWT, NK2, A4>
PLANE_PATH = "plane path"                               # the `name` of a geometry that neither `applies` function takes
VOL_LDS_LIMIT = 160 * 1024                              # dft3d_volume.hip: VOL_LDS_LIMIT
VOL_MIN_VOLUMES = 48                                    # dft3d_volume.hip: VOL_MIN_VOLUMES
EPS = di.EPS
BOUND_SLACK = 24          # the constant of the per-entry bound: 8 per axis, as dft2d_instances.BOUND_SLACK is 16 for two (see forward_bound)
MIX_ROUNDINGS = 3         # one float32 complex product in front of a transform (see inverse_bound)
worst_excess = di.worst_excess


# ---------------------------------------------------------------------------------------------------------------- geometry mirror
def fwd_geometry(D1, D2, D3, m1, m2, m3):
    """vol_shape (dft3d_volume.hip)"""
    g = {"nslot1": (D1 + 1) // 2, "nslot2": (D2 + 1) // 2}
    g["U"] = (g["nslot2"] + 15) // 16
    g["MT2"], g["MT1"] = (m2 + 15) // 16, (m1 + 15) // 16
    nblk = (D3 + 15) // 16
    g["rem"] = D3 - 16 * (nblk - 1)
    g["NARROW"] = 1 if g["rem"] <= 4 else 0
    g["NBW"] = nblk - g["NARROW"]
    g["KA"] = 4 * g["NBW"] + g["NARROW"]
    g["C2"] = 2 * m2 * 2 * m3
    g["NT"] = (g["C2"] + 31) // 32
    RP = 32 * g["NT"]
    while (RP & 63) != 32 or RP <= g["C2"]:
        RP += 32
    g["RP"] = RP
    g["nks1"] = (g["nslot1"] + 3) // 4
    g["lds"] = 2 * g["nslot1"] * RP * 4 + g["nks1"] * g["MT1"] * 64 * 8
    return g


def inv_geometry(D1, D2, D3, m1, m2, m3):
    """vol_inv_shape (dft3d_volume.hip)"""
    g = {"nslot1": (D1 + 1) // 2, "nslot2": (D2 + 1) // 2}
    g["MTS"], g["U"], g["NWT"] = (g["nslot1"] + 15) // 16, (g["nslot2"] + 15) // 16, (D3 + 15) // 16
    g["nk1"], g["nk2"] = (m1 + 3) // 4, (m2 + 3) // 4
    g["NK2"] = (g["nk2"] + 1) & ~1
    g["C2"] = 2 * m2 * 2 * m3
    g["NT"] = (g["C2"] + 31) // 32
    g["RP"] = 32 * g["NT"] + 8
    g["A4"] = D3 % 4 == 0
    g["lds"] = D1 * g["RP"] * 4 + g["nk1"] * g["MTS"] * 64 * 8 + g["MTS"] * 16 * 8
    return g


def _common_limits(n_vol, D1, D2, D3, m1, m2, m3, max_d1):
    if n_vol < VOL_MIN_VOLUMES:
        return False
    if D1 < 4 or D2 < 4 or D3 < 2 or D1 > max_d1 or D2 > 64 or D3 > 32:
        return False
    if 2 * m1 > D1 or 2 * m2 > D2 or m1 > 32 or m2 > 32 or 2 * m3 > 16 or m3 > D3 // 2 + 1:
        return False
    return D1 * D2 * D3 * 4 < 1 << 31


def fwd_applies(n_vol, D1, D2, D3, m1, m2, m3, lds_limit=VOL_LDS_LIMIT):
    """vol3d_fwd_applies; lds_limit=None leaves the LDS condition out (what "one step beyond the limit" is measured against)"""
    if not _common_limits(n_vol, D1, D2, D3, m1, m2, m3, 128):
        return False
    g = fwd_geometry(D1, D2, D3, m1, m2, m3)
    if g["NBW"] < 1 or g["NBW"] > 2 or g["U"] > 2:
        return False
    return lds_limit is None or g["lds"] <= lds_limit


def inv_applies(n_vol, D1, D2, D3, m1, m2, m3, lds_limit=VOL_LDS_LIMIT):
    """vol3d_inv_applies"""
    if not _common_limits(n_vol, D1, D2, D3, m1, m2, m3, 64):
        return False
    return lds_limit is None or inv_geometry(D1, D2, D3, m1, m2, m3)["lds"] <= lds_limit


def format_name(template, args):
    """the name ProfScope records for an instantiation: uno::dft3d_inv_volume_kernel<2, 2, 2, 8, true>"""
    kinds = TEMPLATES[template]
    assert len(args) == len(kinds), (template, args)
    txt = [str(int(a)) if k == "i" else ("true" if a else "false") for a, k in zip(args, kinds)]
    return "uno::{}<{}>".format(template, ", ".join(txt))


FWD_CASES = [(mt2, nbw, narrow, u) for u in (1, 2) for mt2 in (1, 2) for nbw in (1, 2) for narrow in (0, 1)]     # launch_dft3d_fwd_volume
INV_CASES = [(mts, u, nwt, nk2, a4) for mts in (1, 2) for u in (1, 2) for nwt in (1, 2) for nk2 in (2, 4, 6, 8) for a4 in (False, True)]


def kernel_name(direction, shape):
    """the kernel fwd_transform3d / inv_transform3d (capi_spectral.hip) launch for (n_vol, D1, D2, D3, m1, m2, m3): the ProfScope name of a
    K1v / K3v instantiation, or PLANE_PATH"""
    if direction == "fwd":
        if not fwd_applies(*shape):
            return PLANE_PATH
        g = fwd_geometry(*shape[1:])
        args = (g["MT2"], g["NBW"], g["NARROW"], g["U"])
        assert args in FWD_CASES, f"launch_dft3d_fwd_volume has no case for {args}: {shape}"
        return format_name("dft3d_fwd_volume_kernel", (args[0], args[1], bool(args[2]), args[3]))
    if not inv_applies(*shape):
        return PLANE_PATH
    g = inv_geometry(*shape[1:])
    args = (g["MTS"], g["U"], g["NWT"], g["NK2"], g["A4"])
    assert args in INV_CASES, f"launch_dft3d_inv_volume has no case for {args}: {shape}"
    return format_name("dft3d_inv_volume_kernel", args)


def lds_bytes(direction, shape):
    return (fwd_geometry if direction == "fwd" else inv_geometry)(*shape[1:])["lds"]


# ---------------------------------------------------------------------------------------------------------------- table, census
def load_table():
    with open(TABLE) as fh:
        return json.load(fh)


def entry_id(e):
    name = e["name"].replace("uno::", "").replace("_volume_kernel", "").replace(" ", "")
    return "{}-{}-{}-{}".format(e["dir"], e["role"], "x".join(str(v) for v in e["shape"][1:]), name)


def entry_seed(e):
    """a seed derived from the entry's values (stable across processes, unlike hash())"""
    return zlib.crc32(repr((e["name"], e["dir"], tuple(e["shape"]))).encode())


def template_of(name):
    return name[len("uno::"):name.index("<")]


_MANGLED = re.compile(r"^_ZN3uno\d+(__device_stub__)?(dft3d_[a-z]+_volume_kernel)I((?:L[ib]\d+E)+)EEvNS_11Vol3dParamsENS_\d+Vol(?:Inv)?ShapeE$")


def compiled_instances(path=LIBRARY):
    """-> set of ProfScope names of the K1v / K3v instantiations compiled into the library.  Each __global__ instantiation appears as the
    kernel's handle and as its host-side __device_stub__; both must be there."""
    seen = {}
    for sym in di.dynamic_symbols(path):
        m = _MANGLED.match(sym)
        if not m or m.group(2) not in TEMPLATES:
            continue
        args = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(3))]
        seen.setdefault(format_name(m.group(2), args), set()).add(bool(m.group(1)))
    lone = sorted(n for n, kinds in seen.items() if kinds != {False, True})
    assert not lone, f"instantiations with only a handle or only a stub in .dynsym: {lone[:5]}"
    return set(seen)


# ---------------------------------------------------------------------------------------------------------------- coverage
def coverage_of(e):
    """the edges of the kernels' run-time quantities that one table entry sits on (names of COVERAGE)"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    d = e["dir"]
    out = {f"{d}: {'odd' if D1 & 1 else 'even'} D1", f"{d}: {'odd' if D2 & 1 else 'even'} D2"}
    if ((D1 + 1) // 2) % 4:
        out.add(f"{d}: nslot1 % 4 != 0")
    if 17 <= m1 <= 32 and m1 % 16:
        out.add(f"{d}: m1 in 17..32, not a multiple of 16")
    if m1 % 4:
        out.add(f"{d}: m1 % 4 != 0")
    if 2 * m1 == D1:
        out.add(f"{d}: 2 m1 = D1")
    if 2 * m2 == D2:
        out.add(f"{d}: 2 m2 = D2")
    if D3 % 2 == 0 and m3 == D3 // 2 + 1:
        out.add(f"{d}: m3 = D3 / 2 + 1, D3 even")
    if m3 == 8:
        out.add(f"{d}: m3 = 8")
    if d == "fwd":
        rem = fwd_geometry(D1, D2, D3, m1, m2, m3)["rem"]
        if 1 <= rem <= 4:
            out.add("fwd: rem in 1..4")
        if rem == 5:
            out.add("fwd: rem = 5")
        if 65 <= D1 <= 128:
            out.add("fwd: D1 in 65..128")
    else:
        if D3 % 4:
            out.add(f"inv: D3 % 4 = {D3 % 4}")
        if D1 == 64:
            out.add("inv: D1 = 64")
    return out


# what the stressed entries of the table must include between them, in each direction
COVERAGE = [f"{d}: {what}" for d in ("fwd", "inv")
            for what in ("odd D1", "even D1", "odd D2", "even D2", "nslot1 % 4 != 0", "m1 in 17..32, not a multiple of 16", "m1 % 4 != 0",
                         "2 m1 = D1", "2 m2 = D2", "m3 = D3 / 2 + 1, D3 even", "m3 = 8")]
COVERAGE += ["fwd: rem in 1..4", "fwd: rem = 5", "fwd: D1 in 65..128", "inv: D3 % 4 = 1", "inv: D3 % 4 = 2", "inv: D3 % 4 = 3", "inv: D1 = 64"]


# ---------------------------------------------------------------------------------------------------------------- reference
def volumes_input(e):
    """48 real volumes (n, D1, D2, D3) float32"""
    n, D1, D2, D3 = e["shape"][:4]
    return np.random.default_rng(entry_seed(e)).standard_normal((n, D1, D2, D3)).astype(np.float32)


def complex_input(e, shape, salt):
    rng = np.random.default_rng(entry_seed(e) + salt)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def corner_major(X, m1, m2):
    """(n, 2 m1, 2 m2, m3) -> (n, 4, m1, m2, m3) in weights1..4 order (lo, lo), (hi, lo), (lo, hi), (hi, hi)"""
    return np.stack([X[:, :m1, :m2], X[:, m1:, :m2], X[:, :m1, m2:], X[:, m1:, m2:]], axis=1)


def corner_cat(Xc):
    """the inverse of corner_major"""
    return np.concatenate([np.concatenate([Xc[:, 0], Xc[:, 2]], axis=2), np.concatenate([Xc[:, 1], Xc[:, 3]], axis=2)], axis=1)


def truncated_dft3(x, m1, m2, m3):
    """float64, unnormalised: S[v, j, k, n] = sum_{h,w,t} x[v, h, w, t] e^{-2 pi i (K1[j] h / D1 + K2[k] w / D2 + n t / D3)} on the corner rows
    of the two complex axes - so.truncated_rfft3_dense times D1 D2 D3, as matrix products (test_dft3d_instances_cpu.py compares the two)"""
    D1, D2, D3 = x.shape[-3:]
    Fh = so._dft(so.corner_rows(D1, m1), D1, -1.0)
    Fw = so._dft(so.corner_rows(D2, m2), D2, -1.0)
    Ft = so._dft(np.arange(m3), D3, -1.0)
    a = (x.astype(np.float64).reshape(-1, D3) @ Ft.T).reshape(x.shape[0], D1, D2, m3)
    a = np.tensordot(Fw, a, axes=([1], [2]))                    # (2 m2, n, D1, m3): each stage is one matrix product
    return np.tensordot(Fh, a, axes=([1], [2])).transpose(2, 0, 1, 3)


def truncated_idft3(O, D1, D2, D3, c):
    """float64: y[v, h, w, t] = Re sum_{j,k,n} c_n O[v, j, k, n] e^{+2 pi i (...)}, O (n, 2 m1, 2 m2, m3) - the inverse half of
    so.spectral_conv3d_dense (the corners of these kernels never overlap: 2 m <= D, the later-wins masks are all ones)"""
    m1, m2, m3 = O.shape[1] // 2, O.shape[2] // 2, O.shape[3]
    Gh = so._dft(so.corner_rows(D1, m1), D1, +1.0)
    Gw = so._dft(so.corner_rows(D2, m2), D2, +1.0)
    Gt = so._dft(np.arange(m3), D3, +1.0)
    U = np.tensordot(Gh, O.astype(np.complex128), axes=([0], [1]))       # (D1, n, 2 m2, m3)
    U = np.tensordot(Gw, U, axes=([0], [2])) * c                         # (D2, D1, n, m3)
    U = U.reshape(-1, m3)
    y = (U.real @ Gt.real - U.imag @ Gt.imag).reshape(D2, D1, O.shape[0], D3)
    return np.ascontiguousarray(y.transpose(2, 1, 0, 3))


@functools.lru_cache(maxsize=2)
def _forward_spectrum(key):
    e = {"name": key[0], "dir": key[1], "shape": list(key[2])}
    x = volumes_input(e)
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    return x, truncated_dft3(x, m1, m2, m3), np.abs(x.astype(np.float64)).sum(axis=(1, 2, 3))


def forward_case(e, herm):
    """-> (x (n, D1, D2, D3) float32, ref (n, 4, m1, m2, m3) complex128, bound) of one forward transform.  herm = 0: rfftn(norm="forward")
    on the corners (scale 1 / (D1 D2 D3)); herm = 1: the adjoint of the weighted inverse (scale 1, Hermitian weights c_n on the T modes).
    The two share the input and the float64 sums (the last one computed is kept)."""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    x, S, l1 = _forward_spectrum((e["name"], e["dir"], tuple(e["shape"])))
    scale = 1.0 if herm else 1.0 / (D1 * D2 * D3)
    c = so.hermitian_weights(D3, m3) if herm else np.ones(m3)
    return x, corner_major(S * (scale * c), m1, m2), forward_bound(e["shape"], l1, scale, c)


def forward_bound(shape, l1, scale, c):
    """|got - ref| of one (complex) spectrum entry (j, k, n) in float32 arithmetic:

        (D1 + D2 + D3 + 24) 2^-24 scale c_n sum_{h,w,t} |x[h, w, t]|                 per volume

    dft2d_instances.forward_bound with one more axis.  The entry is a sum of D1 D2 D3 products x f_t f_w f_h with |f| <= 1.  A float32
    evaluation in any order - three stages of D3, D2 and D1 terms, the kernels' paired form whose stages have half as many, or an FFT -
    rounds a term's path at most once per addition it passes through (D3 - 1, D2 - 1 and D1 - 1), plus per axis the twiddle factor's own
    rounding and the roundings of one complex product (two products, one addition, and a pairing / twist step in front of it: 8 per axis
    is generous), and the final scaling.  First order in 2^-24 ((D1 + D2 + D3 + 24) 2^-24 < 2e-5 everywhere).  The constant is not fitted
    to anything."""
    n, D1, D2, D3, m1, m2, m3 = shape
    per_vol = (D1 + D2 + D3 + BOUND_SLACK) * EPS * scale * np.asarray(l1)
    return per_vol[:, None, None, None, None] * np.asarray(c)[None, None, None, None, :] * np.ones((1, 4, m1, m2, 1))


def inverse_bound(shape, O, scale, c, extra=0):
    """|got - ref| of one output value of the inverse of O (n, 2 m1, 2 m2, m3):

        (2 m1 + 2 m2 + 2 m3 + 24 + extra) 2^-24 scale sum_{j,k,n} c_n (|Re O| + |Im O|)      per volume

    by the count of dft2d_instances.inverse_reference with one more axis: a value is a sum over 2 m1 x 2 m2 x m3 complex terms, each
    bounded by c_n (|Re O| + |Im O|).  extra = MIX_ROUNDINGS where O is itself a float32 complex product a b of the values the reference
    multiplies in float64: each component of the product carries at most two roundings of |a| |b|, so the modulus of its error is below
    2 sqrt(2) 2^-24 |a b| <= 3 2^-24 (|Re O| + |Im O|)."""
    n, D1, D2, D3, m1, m2, m3 = shape
    O64 = np.asarray(O, dtype=np.complex128)
    s = ((np.abs(O64.real) + np.abs(O64.imag)) * c).sum(axis=(1, 2, 3))
    return ((2 * m1 + 2 * m2 + 2 * m3 + BOUND_SLACK + extra) * EPS * scale * s)[:, None, None, None] * np.ones((1, D1, D2, D3))


def inverse_case(e, xt, w):
    """the weighted inverse (herm = 1) of the forward call: y = irfftn of xt w on the corners.  xt (n, 4, m1, m2, m3) is the DEVICE's truncated
    spectrum and w (4, m1, m2, m3) the weights; the product is formed here in float64, so the forward transform's rounding is not charged
    to the inverse (the product's own float32 rounding is: MIX_ROUNDINGS).  -> (ref (n, D1, D2, D3), bound)"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    O = corner_cat(xt.astype(np.complex128) * w.astype(np.complex128)[None])
    c = so.hermitian_weights(D3, m3)
    return truncated_idft3(O, D1, D2, D3, c), inverse_bound(e["shape"], O, 1.0, c, MIX_ROUNDINGS)


def safe_grid(e):
    """the grid of the OTHER transform of a call (the one not under test): even axes, one whole 16-column T block, wide enough for the
    entry's modes - a geometry of the kind test_hip_spectral3d.py runs, so that a case does not lean on an edge of a second kernel"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    return max(8, 2 * m1), max(8, 2 * m2), 16


def input_gradient_case(e, gy, w):
    """the unweighted inverse (herm = 0) as the backward pass runs it, a COMPOSITE: gy (Do1, Do2, Do3), ONE volume, goes through the adjoint
    forward transform on the plane path, gX[i] = gO conj(w[i]) for the n input channels, and gx[i] = Re iDFT(gX[i]) / (D1 D2 D3) on K3v.
    The reference is that chain in float64; the bound is the sum of both stages' bounds: inverse_bound of gX, plus the forward bound of
    every gO entry (times |w[i]|) carried through the inverse, whose factors have modulus one.  -> (ref (n, D1, D2, D3), bound)"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    Do1, Do2, Do3 = gy.shape
    c = so.hermitian_weights(Do3, m3)
    gO = truncated_dft3(gy[None], m1, m2, m3) * c                                         # (1, 2 m1, 2 m2, m3)
    wc = corner_cat(w.astype(np.complex128))                                              # (n, 2 m1, 2 m2, m3)
    gX = gO * np.conj(wc)
    scale = 1.0 / (D1 * D2 * D3)
    ref = truncated_idft3(gX, D1, D2, D3, np.ones(m3)) * scale
    dgO = (Do1 + Do2 + Do3 + BOUND_SLACK) * EPS * np.abs(gy.astype(np.float64)).sum() * c   # forward_bound of the one volume, per T mode
    carried = scale * (np.abs(wc) * dgO).sum(axis=(1, 2, 3))
    return ref, inverse_bound(e["shape"], gX, scale, np.ones(m3), MIX_ROUNDINGS) + carried[:, None, None, None]


def other_input(e, shape):
    """seeded float32 data for the transform that is not under test"""
    return np.random.default_rng(entry_seed(e) + 2).standard_normal(shape).astype(np.float32)
