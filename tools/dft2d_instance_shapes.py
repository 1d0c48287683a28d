"""For every compiled instantiation of the pruned 2-D transforms K1 / K3, find one or two small shapes that dispatch to it, and write
them to tests/golden/dft2d_instances.json (GPU box; tests/test_dft2d_instances_cpu.py and tests/test_hip_dft2d_instances.py read it).

usage: python tools/dft2d_instance_shapes.py [--out FILE]

The kernel of a call is picked from (n_img, H, W, m1, m2, dtype) and the device's CU count by dft2d() (csrc/capi_spectral.hip),
launch_dft2d_fwd / launch_fwd_t / fwd_ft_geometry / fwd_ht_geometry (dft2d_fwd*.h*), dispatch_inv_range / launch_inv_t / inv_ft_geometry /
inv_geometry (dft2d_inv_kernel.h) and dft2d_b16_applies (dft2d_b16.hip).  This tool does not model those rules: it walks candidate
families chosen to cross each of their conditions, calls _native.dft2d_forward / dft2d_inverse with the library's launch records on,
and keeps for each recorded name the first (narrowest) shape with the fewest row tiles and the first shape with at least five row
tiles and H % 16 != 0 (several waves per image: the cross-wave reduction of K1, the carried partial line of K3).  Every return code
is checked (the binding raises) and the tool stops at the first non-finite result.  The file holds names recorded from this library
and shapes chosen here, nothing else.

Families (all with n_img < 128, m1 <= 40, m2 <= 48: the plane-batched and any-mode forms stay out):
  m1    one per MT = JT = ceil(2 m1 / 16) class, 2 m1 never a multiple of 16
  m2    one per KS = ceil(m2 / 4) class, which also fixes NT = ceil(m2 / 16) and R4; 17 is there because <NT = 2, VEC = false> exists
        only at W = 32, m2 = 17
  W     <= 32: VEC = false.  W % 8 != 0: the full-tile forms (K1: up to 160 columns and NT MT 512 <= 16 W).  W % 8 == 0: the register
        forms.  W >= 200, odd: K1's half-tile form.  W < 64: bf16 images that the bf16-MFMA transforms turn away (as do H < 16,
        m2 > 32 and NT MT > 8).  K3 without the twiddle table: the narrowest W % 8 == 0 whose table (nwt KS 512 bytes) no longer fits
        next to one wave's staging buffer and the row twiddles (inv_lds_bytes against INV_LDS_BUDGET); the image count drops below
        3 where that takes to stay under 4 MiB of image data
  H     m1 + 1 (the fewest row tiles m1 allows; rows of the two corners overlap, so the later-wins mask is at work), and a tall one
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from uno_amd import _native

TEMPLATES = ("dft2d_fwd_kernel", "dft2d_fwd_ft_kernel", "dft2d_fwd_ht_kernel", "dft2d_inv_kernel", "dft2d_inv_ft_kernel")
M1 = {5: 77, 11: 83, 19: 77, 27: 83, 35: 93}                # m1 -> its tall H
M2 = (3, 6, 11, 13, 17, 23, 27, 30, 35, 38, 43, 45)
WIDTHS = (30, 32, 37, 40, 45, 56, 61, 75, 91, 96, 101, 133, 157, 160, 192, 203, 301, 421, 477)
MAX_IMAGE_BYTES = 4 << 20
# dft2d_inv_kernel.h: INV_LDS_BUDGET, and one wave's staging buffer 2 x 16 x STG_RS floats
INV_LDS_BUDGET, INV_STAGE_BYTES = 160 * 1024 - 2048, 2 * 16 * 68 * 4


def width_without_table(H, m2):
    """narrowest W % 8 == 0 at which K3's operand-layout twiddle table does not fit beside one wave (inv_lds_bytes)"""
    KS = (m2 + 3) // 4
    W = 8 * ((2 * m2 + 7) // 8)
    while (((W >> 1) + 16) >> 4) * KS * 512 + INV_STAGE_BYTES + 8 * H <= INV_LDS_BUDGET:
        W += 8
    return W


def candidates():
    """(dir, dtype, tall, (n, H, W, m1, m2)) in the order they are tried"""
    for direction in ("fwd", "inv"):
        for dtype in ("f32", "bf16"):
            for m1, tall_h in M1.items():
                for m2 in M2:
                    for tall, n, H in ((False, 3, m1 + 1), (True, 5, tall_h)):
                        widths = [W for W in WIDTHS if m2 <= W // 2 + 1]
                        if direction == "inv" and dtype == "f32":
                            widths.append(width_without_table(H, m2))
                        for W in widths:
                            k = n
                            while k > 1 and k * H * W * 4 > MAX_IMAGE_BYTES:
                                k -= 1
                            if k * H * W * 4 <= MAX_IMAGE_BYTES:
                                yield direction, dtype, tall, (k, H, W, m1, m2)


def launch(direction, dtype, shape, dev):
    n, H, W, m1, m2 = shape
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator(device="cpu").manual_seed(n + 7 * H + 11 * W + 13 * m1 + 17 * m2)
    _native.profile_begin(64)
    try:
        if direction == "fwd":
            x = torch.randn(n, 1, H, W, generator=g).to(dev).to(tdt)
            out = _native.dft2d_forward(x, m1, m2, scale=0.5, hermitian_cols=True, mask_overlap=True)
            out = torch.view_as_real(out)
        else:
            O = torch.randn(n, 1, 2 * m1, m2, dtype=torch.complex64, generator=g).to(dev)
            out = _native.dft2d_inverse(O, H, W, scale=0.25, dtype=tdt)
        torch.cuda.synchronize()
    finally:
        ran = [name for name, _, _ in _native.profile_end()]
    if not bool(torch.isfinite(out.float()).all()):
        raise SystemExit(f"non-finite result: {direction} {dtype} {shape} ran {ran}")
    return ran


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "dft2d_instances.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    found = {}                  # (name, dir, dtype, tall) -> shape
    calls = 0
    for direction, dtype, tall, shape in candidates():
        ran = launch(direction, dtype, shape, dev)
        calls += 1
        if len(ran) != 1 or not any(ran[0].startswith(f"uno::{t}<") for t in TEMPLATES):
            continue                # another kernel family took the call (the bf16-MFMA transforms)
        found.setdefault((ran[0], direction, dtype, tall), shape)
    entries = [{"name": name, "dir": direction, "shape": list(shape), "dtype": dtype}
               for (name, direction, dtype, tall), shape in sorted(found.items(), key=lambda kv: (kv[0][1], kv[0][0], kv[0][3]))]
    with open(a.out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    names = {e["name"] for e in entries}
    print(f"{calls} calls, {len(entries)} entries, {len(names)} instantiations -> {a.out}")
    for t in TEMPLATES:
        mine = {n for n in names if n.startswith(f"uno::{t}<")}
        both = sum(1 for n in mine if sum(1 for e in entries if e["name"] == n) == 2)
        print(f"  {t}: {len(mine)} instantiations, {both} of them with a tall shape too")


if __name__ == "__main__":
    main()
