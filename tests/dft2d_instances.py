"""Shared by test_dft2d_instances_cpu.py and test_hip_dft2d_instances.py: the table of shapes that reach every compiled instantiation
of the pruned 2-D transforms K1 / K3 (tests/golden/dft2d_instances.json, written by tools/dft2d_instance_shapes.py), the census of the
instantiations compiled into the library (symbol names only), and the float64 reference with its per-entry float32 bound.

No GPU is needed for anything in this module."""
import json
import os
import re
import struct
import zlib

import numpy as np

from oracle import spectral_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "dft2d_instances.json")
LIBRARY = os.path.join(ROOT, "uno_amd", "lib", "libuno_spectral.so")
# template -> kinds of its arguments in order (i: int, b: bool), as ProfScope prints them
TEMPLATES = {"dft2d_fwd_kernel": "iibib", "dft2d_fwd_ft_kernel": "iii", "dft2d_fwd_ht_kernel": "iii",
             "dft2d_inv_kernel": "iibb", "dft2d_inv_ft_kernel": "ii"}
FWD_SCALE, INV_SCALE = 0.5, 0.25
EPS = 2.0 ** -24
BOUND_SLACK = 16          # the constant of the per-entry bound (see forward_bound)


def load_table():
    with open(TABLE) as fh:
        return json.load(fh)


def entry_id(e):
    return "{}-{}-{}-{}".format(e["dir"], e["dtype"], "x".join(str(v) for v in e["shape"]), e["name"].replace("uno::", "").replace(" ", ""))


def entry_seed(e):
    """a seed derived from the entry's values (stable across processes, unlike hash())"""
    return zlib.crc32(repr((e["name"], e["dir"], tuple(e["shape"]), e["dtype"])).encode())


def template_of(name):
    return name[len("uno::"):name.index("<")]


def format_name(template, args):
    """the name ProfScope records for an instantiation: uno::dft2d_inv_kernel<3, 2, false, true>"""
    kinds = TEMPLATES[template]
    assert len(args) == len(kinds), (template, args)
    txt = [str(int(a)) if k == "i" else ("true" if a else "false") for a, k in zip(args, kinds)]
    return "uno::{}<{}>".format(template, ", ".join(txt))


# ---------------------------------------------------------------------------------------------------------------- census
def dynamic_symbols(path):
    """names in the .dynsym section of a little-endian ELF64 shared object"""
    with open(path, "rb") as fh:
        data = fh.read()
    assert data[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for _, sh_type, _, _, offset, size, link, _, _, entsize in sections:
        if sh_type != 11:                   # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for pos in range(offset, offset + size, entsize):
            st_name, = struct.unpack_from("<I", data, pos)
            end = data.index(b"\0", str_off + st_name)
            names.append(data[str_off + st_name:end].decode())
    return names


_MANGLED = re.compile(r"^_ZN3uno\d+(__device_stub__)?(dft2d_[a-z0-9_]+_kernel)I((?:L[ib]\d+E)+)EEvNS_11Dft2dParamsE$")


def compiled_instances(path=LIBRARY):
    """-> set of ProfScope names of the censused templates' instantiations compiled into the library.  Each __global__ instantiation
    appears as the kernel's handle and as its host-side __device_stub__; both must be there."""
    seen = {}
    for sym in dynamic_symbols(path):
        m = _MANGLED.match(sym)
        if not m or m.group(2) not in TEMPLATES:
            continue
        args = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(3))]
        seen.setdefault(format_name(m.group(2), args), set()).add(bool(m.group(1)))
    lone = sorted(n for n, kinds in seen.items() if kinds != {False, True})
    assert not lone, f"instantiations with only a handle or only a stub in .dynsym: {lone[:5]}"
    return set(seen)


# ---------------------------------------------------------------------------------------------------------------- reference
def bf16_round(a):
    """float32 array rounded to the nearest bfloat16 (ties to even), as float32"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def forward_input(e):
    n, H, W, m1, m2 = e["shape"]
    x = np.random.default_rng(entry_seed(e)).standard_normal((n, 1, H, W)).astype(np.float32)
    return bf16_round(x) if e["dtype"] == "bf16" else x


def inverse_input(e):
    n, H, W, m1, m2 = e["shape"]
    rng = np.random.default_rng(entry_seed(e))
    return (rng.standard_normal((n, 1, 2 * m1, m2)) + 1j * rng.standard_normal((n, 1, 2 * m1, m2))).astype(np.complex64)


def forward_reference(e, x):
    """float64 spectrum of test_dft2d_forward_stage (hermitian_cols = mask_overlap = True, scale 0.5) and the per-entry bound."""
    n, H, W, m1, m2 = e["shape"]
    c, keep = so.hermitian_weights(W, m2), so.later_wins_mask(H, m1)
    ref = so.truncated_rfft2_dense(x, m1, m2) * (H * W) * FWD_SCALE * c[None, None, None, :] * keep[None, None, :, None]
    return ref, forward_bound(e, x), keep == 0


def forward_bound(e, x):
    """|got - ref| of one (complex) spectrum entry (j, l) in float32 arithmetic:

        (H + W + 16) 2^-24 scale c_l sum_{h,w} |x[h, w]|                 per image

    The entry is a sum of H W products x f_w f_h with |f| <= 1.  A float32 evaluation - in any order: a row transform of W terms then a
    column transform of H terms, or an FFT, whose chains are shorter - rounds each term's path at most once per addition it passes
    through (W - 1 in the row stage, H - 1 in the column stage), plus the two twiddle factors' own rounding, the two complex products
    and the final scaling: fewer than H + W + 16 roundings of relative size 2^-24 on a term bounded by |x|.  First order in 2^-24
    ((H + W) 2^-24 < 1e-3 at every table shape).  The constant 16 is not fitted to anything."""
    n, H, W, m1, m2 = e["shape"]
    c = so.hermitian_weights(W, m2)
    s = np.abs(x.astype(np.float64)).sum(axis=(-2, -1))                               # (n, 1)
    return (H + W + BOUND_SLACK) * EPS * FWD_SCALE * s[:, :, None, None] * c[None, None, None, :] * np.ones((1, 1, 2 * m1, 1))


def inverse_reference(e, O):
    """float64 images of test_dft2d_inverse_stage (hermitian_cols = mask_overlap = True, scale 0.25) and the per-entry bound:

        (2 m1 + 2 m2 + 16) 2^-24 scale sum_{j,l} c_l (|Re O[j, l]| + |Im O[j, l]|)      per image  [+ 2^-8 |ref| for a bf16 image]

    by the same count as forward_bound: a pixel is a sum over 2 m1 x m2 complex terms (two real products each: chains of 2 m1 and
    2 m2 real additions), each bounded by c_l (|Re O| + |Im O|)."""
    n, H, W, m1, m2 = e["shape"]
    c, keep = so.hermitian_weights(W, m2), so.later_wins_mask(H, m1)
    Gh = so._dft(so.corner_rows(H, m1), H, +1.0)
    Gw = so._dft(np.arange(m2), W, +1.0)
    O64 = O.astype(np.complex128)
    U = np.einsum("bojl,jh->bohl", O64 * keep[None, None, :, None], Gh)
    ref = INV_SCALE * np.einsum("bohl,lw->bohw", U * c, Gw).real
    s = ((np.abs(O64.real) + np.abs(O64.imag)) * c).sum(axis=(-2, -1))                 # (n, 1)
    bound = (2 * m1 + 2 * m2 + BOUND_SLACK) * EPS * INV_SCALE * s[:, :, None, None] * np.ones((1, 1, H, W))
    if e["dtype"] == "bf16":
        bound = bound + 2.0 ** -8 * np.abs(ref)
    return ref, bound


def worst_excess(got, ref, bound):
    """max over entries of |got - ref| / bound (complex entries: the modulus of the difference); <= 1 passes"""
    return float((np.abs(np.asarray(got) - ref) / bound).max())
