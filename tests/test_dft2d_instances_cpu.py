"""Census of the compiled instantiations of the pruned 2-D transforms K1 / K3 (no GPU needed).

tests/golden/dft2d_instances.json (tools/dft2d_instance_shapes.py) names one or two shapes per instantiation, and
tests/test_hip_dft2d_instances.py runs each of them against float64.  Here: the names of that table plus the UNREACHABLE table below
are EXACTLY the instantiations of dft2d_fwd_kernel, dft2d_fwd_ft_kernel, dft2d_fwd_ht_kernel, dft2d_inv_kernel and
dft2d_inv_ft_kernel that the built library holds (read from its .dynsym: symbol names only), so a new instantiation without a shape,
or a dispatch change that strands one, fails here.  And the per-entry bound of the GPU test is checked against the float32 FFT of
the same inputs, so that it is known to be a bound that a correct float32 evaluation keeps, independently of the kernels."""
import collections

import numpy as np
import torch

import dft2d_instances as di

TABLE = di.load_table()
UNREACHABLE_CAP = 45        # a tenth of the matrix; beyond it, dead instantiations are a finding to report, not a table to grow

# (template, argument tuples, the dispatcher inequality that excludes them)
_FT_DEAD = [(1, 5), (2, 3), (2, 4), (2, 5), (3, 2), (3, 3), (3, 4), (3, 5)]
UNREACHABLE_GROUPS = [
    ("dft2d_fwd_kernel", [(3, mt, False, 0, b) for mt in range(1, 6) for b in (False, True)],
     "VEC = false needs ((W - 1) >> 1) < 16, i.e. W <= 32 (launch_dft2d_fwd, dft2d_fwd.hip:12); NT = 3 needs m2 >= 33, and "
     "check_modes2d (capi_spectral.hip:18) wants m2 <= W / 2 + 1, i.e. W >= 64"),
    ("dft2d_fwd_ft_kernel", [(nt, mt, r4) for nt, mt in _FT_DEAD for r4 in (0, 1, 2)],
     "fwd_ft_geometry (dft2d_fwd_ft_kernel.h:216-222): W % 8 != 0 and W <= FT_MAXW = 160 leave W <= 159, and the reduction slots "
     "want NT MT 512 <= 16 W <= 2544, i.e. NT MT <= 4"),
    ("dft2d_fwd_ht_kernel", [(3, mt, r4) for mt in (4, 5) for r4 in (0, 1, 2)],
     "fwd_ht_geometry (dft2d_fwd_ht_kernel.h:289-291): NT MT >= 12 keeps the unpaired column stage (MPh = MT), whose reduction "
     "slots want NT MT 512 >= 6144 floats in a buffer of s0 + 15 seg; the run limits QL + QR + 3 <= 256 and len_in + 3 <= 256 of "
     "line 289 hold seg <= 260 and s0 <= 260 (ht_split, :33-48), i.e. the buffer to 4160 floats"),
]
UNREACHABLE = {di.format_name(t, a): why for t, args, why in UNREACHABLE_GROUPS for a in args}


def test_unreachable_table_is_argued_and_capped():
    assert len(UNREACHABLE) == sum(len(args) for _, args, _ in UNREACHABLE_GROUPS)          # no name listed twice
    assert len(UNREACHABLE) <= UNREACHABLE_CAP, len(UNREACHABLE)
    for name, why in UNREACHABLE.items():
        assert ".h" in why and ":" in why and len(why) > 80, f"{name}: an entry needs the inequality that excludes it, with file and line"


def test_table_is_well_formed():
    seen = set()
    for e in TABLE:
        assert set(e) == {"name", "dir", "shape", "dtype"}, e
        assert di.template_of(e["name"]) in di.TEMPLATES and e["dir"] == ("fwd" if "_fwd_" in e["name"] else "inv")
        assert e["dtype"] in ("f32", "bf16")
        n, H, W, m1, m2 = e["shape"]
        # off the plane-batched and any-mode forms, valid mode counts, at most 4 MiB of image data
        assert 1 <= n < 128 and 1 <= m1 <= min(H, 40) and 1 <= m2 <= min(W // 2 + 1, 48), e
        assert n * H * W * 4 <= 4 << 20, e
        key = (e["name"], e["dir"], tuple(e["shape"]), e["dtype"])
        assert key not in seen, e
        seen.add(key)
    per_name = collections.Counter(e["name"] for e in TABLE)
    assert max(per_name.values()) <= 2
    # the second shape of a name is the tall one: at least five row tiles, ragged last tile
    for name in per_name:
        hs = sorted(e["shape"][1] for e in TABLE if e["name"] == name)
        if len(hs) == 2:
            assert hs[1] >= 65 and hs[1] % 16 != 0 and hs[0] < hs[1], (name, hs)


def test_table_and_unreachable_partition_the_compiled_set():
    compiled = di.compiled_instances()
    assert 400 <= len(compiled) <= 500, f"{len(compiled)} instantiations read from .dynsym: the parser sees too little or too much"
    per_template = collections.Counter(di.template_of(n) for n in compiled)
    assert set(per_template) == set(di.TEMPLATES), per_template
    named = {e["name"] for e in TABLE}
    both = sorted(named & set(UNREACHABLE))
    assert not both, f"listed as unreachable but recorded by a launch: {both}"
    missing = sorted(compiled - named - set(UNREACHABLE))
    assert not missing, (f"{len(missing)} compiled instantiations have no shape in tests/golden/dft2d_instances.json "
                         f"(regenerate it with tools/dft2d_instance_shapes.py): {missing[:8]}")
    gone = sorted((named | set(UNREACHABLE)) - compiled)
    assert not gone, f"{len(gone)} names are not compiled into the library any more: {gone[:8]}"


# ---------------------------------------------------------------------------------------------------------------- the bound
def _fft32_forward(e, x):
    """the reference's own float32 path: torch.fft.rfft2 of the image, cropped to the corner rows and the first m2 columns"""
    n, H, W, m1, m2 = e["shape"]
    X = torch.fft.rfft2(torch.from_numpy(x)).numpy()
    rows = di.so.corner_rows(H, m1)
    c = di.so.hermitian_weights(W, m2).astype(np.float32)
    keep = di.so.later_wins_mask(H, m1).astype(np.float32)
    return X[:, :, rows, :m2] * np.float32(di.FWD_SCALE) * c[None, None, None, :] * keep[None, None, :, None]


def _fft32_inverse(e, O):
    """torch.fft.irfft2 of the zero-filled spectrum, the corners assigned in the reference's order (the later one wins)"""
    n, H, W, m1, m2 = e["shape"]
    full = torch.zeros((n, 1, H, W // 2 + 1), dtype=torch.complex64)
    Ot = torch.from_numpy(O)
    full[:, :, :m1, :m2] = Ot[:, :, :m1]
    full[:, :, H - m1:, :m2] = Ot[:, :, m1:]
    return (torch.fft.irfft2(full, s=(H, W), norm="forward") * di.INV_SCALE).numpy()


def test_per_entry_bound_sees_one_unwritten_value():
    """The other side of the bound: one entry of the last mode column (forward) / image column (inverse) left at the guard pattern
    (0xA5A5A5A5 is -2.9e-16 as a float) in an otherwise exact result fails it.  The entry taken is the one of median magnitude, so
    the bound sits below the typical value of a single entry at the table's shapes, not just below the largest."""
    poison = np.frombuffer(b"\xa5" * 4, dtype=np.float32)[0]
    for e in TABLE[::10]:
        if e["dir"] == "fwd":
            ref, bound, _ = di.forward_reference(e, di.forward_input(e))
        else:
            ref, bound = di.inverse_reference(e, di.inverse_input(e))
        last = np.abs(ref[..., -1])
        live = np.sort(last[last > 0])
        idx = np.unravel_index(np.argmin(np.abs(last - live[len(live) // 2])), last.shape) + (ref.shape[-1] - 1,)
        got = ref.copy()
        got[idx] = poison
        assert di.worst_excess(got, ref, bound) > 1.0, di.entry_id(e)


def test_float32_fft_stays_inside_the_per_entry_bound():
    """The bound of test_hip_dft2d_instances.py is derived, not measured (dft2d_instances.forward_bound); this confirms at every
    table entry that a correct float32 evaluation of the same sum - the FFT the reference runs - stays inside it, bf16 rounding of the
    output included."""
    worst = {"fwd": 0.0, "inv": 0.0}
    for e in TABLE:
        if e["dir"] == "fwd":
            x = di.forward_input(e)
            ref, bound, dead = di.forward_reference(e, x)
            got = _fft32_forward(e, x)
            assert np.all(got[:, :, dead, :] == 0)
        else:
            O = di.inverse_input(e)
            ref, bound = di.inverse_reference(e, O)
            got = _fft32_inverse(e, O)
            if e["dtype"] == "bf16":
                got = di.bf16_round(got)
        r = di.worst_excess(got, ref, bound)
        assert r <= 1.0, f"{di.entry_id(e)}: float32 FFT misses the bound by a factor {r:.3g}"
        worst[e["dir"]] = max(worst[e["dir"]], r)
    print("largest |fft32 - ref| / bound:", worst)
