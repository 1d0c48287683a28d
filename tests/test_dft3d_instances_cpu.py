"""Census of the compiled instantiations of the one-workgroup-per-volume 3-D transforms K1v / K3v (no GPU needed).

tests/golden/dft3d_instances.json (tools/dft3d_instance_shapes.py) names two shapes per instantiation that a call can reach, and
tests/test_hip_dft3d_instances.py runs each of them against float64.  Here: the names of that table plus the UNREACHABLE table below
are EXACTLY the instantiations of dft3d_fwd_volume_kernel and dft3d_inv_volume_kernel that the built library holds (read from its
.dynsym: symbol names only), so a new instantiation without a shape, or a dispatch change that strands one, fails here.  The Python
mirror of the host-side geometry (dft3d_instances.py) names every table entry's kernel, reaches nothing outside the table on a walk over
the kernels' whole range, and is consistent with itself; the stressed entries sit on every edge of dft3d_instances.COVERAGE.  And the
per-entry bounds of the GPU test are checked against the float32 FFT of the same inputs, so that they are known to be bounds that a
correct float32 evaluation keeps, independently of the kernels."""
import collections

import numpy as np
import torch

import dft3d_instances as d3
from oracle import spectral_oracle as so

TABLE = d3.load_table()
KERNELS = [e for e in TABLE if e["name"] != d3.PLANE_PATH]
VOLUMES = 12

# (template, argument tuples, the dispatcher inequality that excludes them)
UNREACHABLE_GROUPS = [
    ("dft3d_fwd_volume_kernel", [(2, nbw, narrow, 1) for nbw in (1, 2) for narrow in (False, True)],
     "MT2 = 2 needs m2 >= 17 (vol_shape, dft3d_volume.hip:118), vol3d_fwd_applies wants 2 m2 <= D2 (dft3d_volume.hip:138), so D2 >= 34, "
     "nslot2 >= 17 and U = ceil(nslot2 / 16) = 2 (dft3d_volume.hip:116-117)"),
    ("dft3d_fwd_volume_kernel", [(1, 2, True, 1), (1, 2, True, 2), (2, 2, True, 2)],
     "NBW = 2 with NARROW needs three 16-column blocks, the last one of at most 4 columns (vol_shape, dft3d_volume.hip:120-122), i.e. "
     "D3 >= 33, and vol3d_fwd_applies turns D3 > 32 away (dft3d_volume.hip:137)"),
    ("dft3d_inv_volume_kernel", [(mts, 1, nwt, nk2, a4) for mts in (1, 2) for nwt in (1, 2) for nk2 in (6, 8) for a4 in (False, True)],
     "NK2 in {6, 8} needs nk2 = ceil(m2 / 4) >= 5, i.e. m2 >= 17 (vol_inv_shape, dft3d_volume.hip:505-506), vol3d_inv_applies wants "
     "2 m2 <= D2 (dft3d_volume.hip:518), so D2 >= 34, nslot2 >= 17 and U = ceil(nslot2 / 16) = 2 (dft3d_volume.hip:500-502)"),
]
UNREACHABLE = {d3.format_name(t, a): why for t, args, why in UNREACHABLE_GROUPS for a in args}


def test_unreachable_table_is_argued():
    assert len(UNREACHABLE) == sum(len(args) for _, args, _ in UNREACHABLE_GROUPS)          # no name listed twice
    per_template = collections.Counter(d3.template_of(n) for n in UNREACHABLE)
    assert per_template == {"dft3d_fwd_volume_kernel": 7, "dft3d_inv_volume_kernel": 16}, per_template
    for name, why in UNREACHABLE.items():
        assert ".hip:" in why and len(why) > 80, f"{name}: an entry needs the inequality that excludes it, with file and line"


def test_table_is_well_formed():
    seen = set()
    for e in TABLE:
        assert set(e) == {"name", "dir", "role", "shape"}, e
        n, D1, D2, D3, m1, m2, m3 = e["shape"]
        assert n == d3.VOL_MIN_VOLUMES and n * D1 * D2 * D3 * 4 < 16 << 20, e
        assert 1 <= m1 <= D1 // 2 and 1 <= m2 <= D2 // 2 and 1 <= m3 <= D3 // 2 + 1, e
        applies = d3.fwd_applies if e["dir"] == "fwd" else d3.inv_applies
        if e["name"] == d3.PLANE_PATH:
            # one step beyond the LDS limit: everything else about the geometry is inside the kernels' range
            assert e["role"] == "beyond-lds" and applies(*e["shape"], lds_limit=None) and not applies(*e["shape"]), e
            assert d3.lds_bytes(e["dir"], e["shape"]) > d3.VOL_LDS_LIMIT
        else:
            assert e["role"] in ("smallest", "stressed", "largest-lds") and applies(*e["shape"]), e
            assert d3.template_of(e["name"]) == f"dft3d_{e['dir']}_volume_kernel"
        key = (e["name"], e["dir"], tuple(e["shape"]))
        assert key not in seen, e
        seen.add(key)
    for name in {e["name"] for e in KERNELS}:
        mine = [e for e in KERNELS if e["name"] == name]
        assert len(mine) == 2 and mine[0]["role"] == "smallest" and mine[1]["role"] in ("stressed", "largest-lds"), mine
        assert np.prod(mine[0]["shape"][1:4]) <= np.prod(mine[1]["shape"][1:4])
    assert collections.Counter(e["role"] for e in TABLE)["beyond-lds"] == 2 == collections.Counter(e["role"] for e in TABLE)["largest-lds"]


def test_table_and_unreachable_partition_the_compiled_set():
    compiled = d3.compiled_instances()
    per_template = collections.Counter(d3.template_of(n) for n in compiled)
    assert per_template == {"dft3d_fwd_volume_kernel": 16, "dft3d_inv_volume_kernel": 64}, per_template
    # the cases the two dispatchers spell out are the compiled set
    spelled = {d3.format_name("dft3d_fwd_volume_kernel", (a, b, bool(c), d)) for a, b, c, d in d3.FWD_CASES}
    spelled |= {d3.format_name("dft3d_inv_volume_kernel", args) for args in d3.INV_CASES}
    assert spelled == compiled, sorted(spelled ^ compiled)[:8]
    named = {e["name"] for e in KERNELS}
    both = sorted(named & set(UNREACHABLE))
    assert not both, f"listed as unreachable but in the table: {both}"
    missing = sorted(compiled - named - set(UNREACHABLE))
    assert not missing, (f"{len(missing)} compiled instantiations have no shape in tests/golden/dft3d_instances.json "
                         f"(regenerate it with tools/dft3d_instance_shapes.py): {missing[:8]}")
    gone = sorted((named | set(UNREACHABLE)) - compiled)
    assert not gone, f"{len(gone)} names are not compiled into the library any more: {gone[:8]}"
    reach = collections.Counter(d3.template_of(n) for n in named)
    assert reach == {"dft3d_fwd_volume_kernel": 9, "dft3d_inv_volume_kernel": 48}, reach


def test_mirror_names_every_entry_and_reaches_nothing_else():
    for e in TABLE:
        assert d3.kernel_name(e["dir"], tuple(e["shape"])) == e["name"], f"regenerate tests/golden/dft3d_instances.json: {e}"
    # a walk over the kernels' range, every tile-count class of every axis at both of its ends: nothing outside the table is reached
    named = {e["name"] for e in TABLE}
    reached = set()
    for direction in ("fwd", "inv"):
        for D1 in (4, 5, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129):
            for D2 in range(4, 66):
                for D3 in range(2, 34):
                    for m2 in (1, 8, 9, 16, 17, 24, 25, 32):
                        if 2 * m2 <= D2:
                            reached.add(d3.kernel_name(direction, (48, D1, D2, D3, 1, m2, 1)))
    assert reached == named, sorted(reached ^ named)
    assert not reached & set(UNREACHABLE)


def test_mirror_is_consistent_with_itself():
    for e in KERNELS:
        n, D1, D2, D3, m1, m2, m3 = e["shape"]
        if e["dir"] == "fwd":
            g = d3.fwd_geometry(*e["shape"][1:])
            assert (g["RP"] & 63) == 32 and g["C2"] < g["RP"] <= g["C2"] + 64          # the first pad float of a row exists
            assert 16 * (g["NBW"] + g["NARROW"]) >= D3 > 16 * (g["NBW"] + g["NARROW"] - 1) and 1 <= g["rem"] <= 16
            assert (g["rem"] <= 4) == bool(g["NARROW"]) and g["KA"] * 4 >= D3 - 12 * g["NARROW"]
            assert 4 * g["nks1"] >= g["nslot1"] > 4 * (g["nks1"] - 1) and 16 * g["MT1"] >= m1 and 16 * g["MT2"] >= m2
        else:
            g = d3.inv_geometry(*e["shape"][1:])
            assert g["RP"] % 16 == 8 and g["RP"] >= g["C2"] + 8
            assert 16 * g["MTS"] >= g["nslot1"] > 16 * (g["MTS"] - 1) and 16 * g["NWT"] >= D3 > 16 * (g["NWT"] - 1)
            assert g["NK2"] % 2 == 0 and g["NK2"] - 1 <= g["nk2"] <= g["NK2"] and 4 * g["nk2"] >= m2 > 4 * (g["nk2"] - 1)
            assert 4 * g["nk1"] >= m1 > 4 * (g["nk1"] - 1)
        assert 16 * g["U"] >= g["nslot2"] > 16 * (g["U"] - 1) and 2 * g["nslot1"] in (D1, D1 + 1)
        assert 32 * g["NT"] >= g["C2"] > 32 * (g["NT"] - 1) and g["lds"] <= d3.VOL_LDS_LIMIT


def test_stressed_entries_cover_the_edges():
    stressed = [e for e in KERNELS if e["role"] != "smallest"]
    have = set().union(*(d3.coverage_of(e) for e in stressed))
    missing = [c for c in d3.COVERAGE if c not in have]
    assert not missing, missing
    for direction in ("fwd", "inv"):
        top, = [e for e in TABLE if e["dir"] == direction and e["role"] == "largest-lds"]
        beyond, = [e for e in TABLE if e["dir"] == direction and e["role"] == "beyond-lds"]
        lds = d3.lds_bytes(direction, top["shape"])
        assert lds == max(d3.lds_bytes(direction, e["shape"]) for e in KERNELS if e["dir"] == direction)
        assert d3.VOL_LDS_LIMIT - 2048 < lds <= d3.VOL_LDS_LIMIT < d3.lds_bytes(direction, beyond["shape"])
        # one step: the two differ in one of D1, m1, m2, m3 (D2, D3 only follow the modes)
        assert sum(a != b for a, b in zip(np.take(top["shape"], [1, 4, 5, 6]), np.take(beyond["shape"], [1, 4, 5, 6]))) == 1


# ---------------------------------------------------------------------------------------------------------------- the references
def test_matrix_product_references_equal_the_oracle():
    """dft3d_instances.truncated_dft3 / truncated_idft3 are the dense oracle's sums written as matrix products"""
    for e in [KERNELS[1], KERNELS[-1]]:
        n, D1, D2, D3, m1, m2, m3 = e["shape"]
        x = d3.volumes_input(e)[:2]
        S = d3.truncated_dft3(x, m1, m2, m3)
        X = so.truncated_rfft3_dense(x[:, None], m1, m2, m3)[:, 0]
        assert np.abs(S / (D1 * D2 * D3) - X).max() <= 1e-12 * np.abs(X).max()
        w = d3.complex_input(e, (4, m1, m2, m3), 1)
        y, _ = so.spectral_conv3d_dense(x[:, None], [v[None, None] for v in w], D1, D2, D3)
        mine = d3.truncated_idft3(X * d3.corner_cat(w[None].astype(np.complex128)), D1, D2, D3, so.hermitian_weights(D3, m3))
        assert np.abs(mine - y[:, 0]).max() <= 1e-12 * np.abs(y).max()
        Xc = d3.corner_major(X, m1, m2)
        assert Xc.shape == (2, 4, m1, m2, m3) and np.array_equal(d3.corner_cat(Xc), X)


# ---------------------------------------------------------------------------------------------------------------- the bounds
def _crop(X, D1, D2, m1, m2, m3):
    return X[:, so.corner_rows(D1, m1)][:, :, so.corner_rows(D2, m2)][..., :m3]


def _fft32_forward(e, x, herm):
    """the reference's own float32 path: torch.fft.rfftn of the volumes, cropped to the corners"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    X = _crop(torch.fft.rfftn(torch.from_numpy(x), dim=(1, 2, 3)).numpy(), D1, D2, m1, m2, m3)
    c = (so.hermitian_weights(D3, m3) if herm else np.ones(m3)).astype(np.float32)
    return d3.corner_major(X * np.float32(1.0 if herm else 1.0 / (D1 * D2 * D3)) * c, m1, m2)


def _fft32_inverse(e, O, herm, scale):
    """torch.fft.irfftn of the zero-filled spectrum O (n, 2 m1, 2 m2, m3) complex64; irfftn weights the bins as herm = 1 does, so the
    unweighted form divides them out first (by 1 or 2: exact)"""
    n, D1, D2, D3, m1, m2, m3 = e["shape"]
    if not herm:
        O = O / so.hermitian_weights(D3, m3).astype(np.float32)
    full = torch.zeros((O.shape[0], D1, D2, D3 // 2 + 1), dtype=torch.complex64)
    rows, cols = torch.from_numpy(so.corner_rows(D1, m1)), torch.from_numpy(so.corner_rows(D2, m2))
    full[:, rows[:, None], cols[None, :], :m3] = torch.from_numpy(np.ascontiguousarray(O)).to(torch.complex64)
    return (torch.fft.irfftn(full, s=(D1, D2, D3), dim=(1, 2, 3), norm="forward") * np.float32(scale)).numpy()


def _weights(e, n):
    m1, m2, m3 = e["shape"][4:]
    return d3.complex_input(e, (n, 4, m1, m2, m3), 1)


def test_float32_fft_stays_inside_the_per_entry_bounds():
    """The bounds of test_hip_dft3d_instances.py are derived, not measured (dft3d_instances.forward_bound / inverse_bound); this confirms at
    every table entry, in the four forms the GPU test runs, that a correct float32 evaluation of the same sums - the FFT the reference
    runs - stays inside them.  (The first VOLUMES of an entry's 48 volumes: the bounds are per volume, and the float32 FFTs are what takes
    the time here.)"""
    worst = collections.defaultdict(float)
    for e in KERNELS:
        n, D1, D2, D3, m1, m2, m3 = e["shape"]
        if e["dir"] == "fwd":
            for herm in (0, 1):
                x, ref, bound = (a[:VOLUMES] for a in d3.forward_case(e, herm))
                r = d3.worst_excess(_fft32_forward(e, x, herm), ref, bound)
                assert r <= 1.0, f"{d3.entry_id(e)} herm {herm}: float32 FFT misses the bound by a factor {r:.3g}"
                worst["fwd", herm] = max(worst["fwd", herm], r)
        else:
            # herm = 1: the inverse of (a float32 truncated spectrum) x (weights), the product formed in float32 as the mode GEMM does
            x = d3.other_input(e, (VOLUMES, *d3.safe_grid(e)))
            xt = _fft32_forward({"shape": [VOLUMES, *x.shape[1:], m1, m2, m3]}, x, 0)
            w = _weights(e, 1)[0]
            ref, bound = d3.inverse_case(e, xt, w)
            r = d3.worst_excess(_fft32_inverse(e, d3.corner_cat(xt * w[None]), 1, 1.0), ref, bound)
            assert r <= 1.0, f"{d3.entry_id(e)} herm 1: float32 FFT misses the bound by a factor {r:.3g}"
            worst["inv", 1] = max(worst["inv", 1], r)
            # herm = 0, the composite: adjoint forward transform of one volume, the weights, the unweighted inverse - all in float32
            gy, wn = d3.other_input(e, d3.safe_grid(e)), _weights(e, n)[:VOLUMES]
            ref, bound = d3.input_gradient_case(e, gy, wn)
            gO = d3.corner_cat(_fft32_forward({"shape": [1, *gy.shape, m1, m2, m3]}, gy[None], 1))
            got = _fft32_inverse(e, gO * np.conj(d3.corner_cat(wn)), 0, 1.0 / (D1 * D2 * D3))
            r = d3.worst_excess(got, ref, bound)
            assert r <= 1.0, f"{d3.entry_id(e)} herm 0: float32 FFT misses the bound by a factor {r:.3g}"
            worst["inv", 0] = max(worst["inv", 0], r)
    print("largest |fft32 - ref| / bound:", dict(worst))


def test_per_entry_bound_sees_one_unwritten_value():
    """The other side of the bounds: one entry of the last T mode (forward) / last column (inverse) left at the guard pattern (0xA5A5A5A5
    is -2.9e-16 as a float) in an otherwise exact result fails them.  The entry taken is the one of median magnitude, so the bound sits
    below the typical value of a single entry at the table's shapes, not just below the largest."""
    poison = np.frombuffer(b"\xa5" * 4, dtype=np.float32)[0]
    for e in KERNELS[::5]:
        if e["dir"] == "fwd":
            _, ref, bound = d3.forward_case(e, 0)
        else:
            x = d3.other_input(e, (e["shape"][0], *d3.safe_grid(e)))
            xt = _fft32_forward({"shape": [*x.shape, *e["shape"][4:]]}, x, 0)
            ref, bound = d3.inverse_case(e, xt, _weights(e, 1)[0])
        last = np.abs(ref[..., -1])
        live = np.sort(last[last > 0])
        idx = np.unravel_index(np.argmin(np.abs(last - live[len(live) // 2])), last.shape) + (ref.shape[-1] - 1,)
        got = ref.copy()
        got[idx] = poison
        assert d3.worst_excess(got, ref, bound) > 1.0, d3.entry_id(e)
