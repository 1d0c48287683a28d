"""For every instantiation of the one-workgroup-per-volume 3-D transforms K1v / K3v that a call can reach, find two shapes that dispatch
to it, and write them to tests/golden/dft3d_instances.json (no GPU; tests/test_dft3d_instances_cpu.py and
tests/test_hip_dft3d_instances.py read the file).

usage: python tools/dft3d_instance_shapes.py [--out FILE]

The kernel of a call is picked from (n_vol, D1, D2, D3, m1, m2, m3) by vol3d_fwd_applies / vol3d_inv_applies and launch_dft3d_fwd_volume /
launch_dft3d_inv_volume (csrc/dft3d_volume.hip).  tests/dft3d_instances.py mirrors those rules in Python (the GPU test compares the
mirror's name with the launch record of every entry); this tool walks the geometries the rules accept and keeps, per instantiation,

  smallest   the volume with the fewest elements that reaches it (ties: the fewest modes, then the smallest axes in order), and
  stressed   a ragged one: taken from a seeded sample of the instantiation's geometries (mode counts drawn at their upper limits a third
             of the time) that is no larger than 20 000 elements or twice the smallest volume.  The entries of dft3d_instances.COVERAGE
             (odd and even axes, ragged k-steps and mode tiles, corners without a gap, the Nyquist bin, every D3 % 4, D1 beyond the
             inverse's range ...) are served first, each by the sample that sits on the most edges at once (stress() below: the COVERAGE
             items plus ragged last tiles; samples that give a wave more than one slot or plane, so that the software-pipelined loops
             run, go before all others); the instantiations left over take their sample with the most edges.  The geometry with the largest LDS footprint that `applies` still accepts is found by
             an exhaustive walk over (D1, m1, m2, m3) and becomes the stressed entry of its instantiation.

and, per direction, the geometry one step beyond that largest footprint (one of D1, m1, m2, m3 raised until the LDS need passes
VOL_LDS_LIMIT, the smallest excess taken), recorded with the name "plane path".  Every entry has n_vol = VOL_MIN_VOLUMES = 48."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dft3d_instances as d3

N_VOL = d3.VOL_MIN_VOLUMES
MAX_D1 = {"fwd": 128, "inv": 64}
STRESSED_ELEMS = 20000
SAMPLES = 600
APPLIES = {"fwd": d3.fwd_applies, "inv": d3.inv_applies}


def volume(shape):
    return shape[1] * shape[2] * shape[3]


def order(shape):
    return (volume(shape), shape[4] * shape[5] * shape[6]) + tuple(shape[1:])


def smallest_shapes(direction):
    """name -> smallest shape.  The name depends on the modes only through the class of m2 (MT2 / NK2), and the LDS need grows with every
    mode count: the least m2 of each class with m1 = m3 = 1 is enough."""
    best = {}
    for D1 in range(4, MAX_D1[direction] + 1):
        for D2 in range(4, 65):
            for D3 in range(2, 33):
                for m2 in (1, 9, 17, 25):
                    shape = (N_VOL, D1, D2, D3, 1, m2, 1)
                    if not APPLIES[direction](*shape):
                        continue
                    name = d3.kernel_name(direction, shape)
                    if name not in best or order(shape) < order(best[name]):
                        best[name] = shape
    return best


def largest_lds(direction):
    """(the accepted geometry with the largest LDS footprint, the geometry one step beyond it).  The footprint depends on D1 and the mode
    counts only; D2 and D3 are the smallest that admit the modes (D3 even, so that the forward transform has a whole 16-byte piece)."""
    best = None
    for D1 in range(4, MAX_D1[direction] + 1):
        for m1 in range(1, min(32, D1 // 2) + 1):
            for m2 in range(1, 33):
                for m3 in range(1, 9):
                    shape = (N_VOL, D1, max(4, 2 * m2), max(6, 2 * m3 - 2), m1, m2, m3)
                    if not APPLIES[direction](*shape):
                        continue
                    key = (d3.lds_bytes(direction, shape), -volume(shape), tuple(-v for v in shape))
                    if best is None or key > best[0]:
                        best = (key, shape)
    top = best[1]
    beyond = []
    for axis in (1, 4, 5, 6):
        shape = list(top)
        while True:
            shape[axis] += 1
            shape[2], shape[3] = max(shape[2], 2 * shape[5]), max(shape[3], 2 * shape[6] - 2)
            if not APPLIES[direction](*shape, lds_limit=None):
                break                                      # this axis leaves the kernels' range before the LDS need passes the limit
            if d3.lds_bytes(direction, shape) > d3.VOL_LDS_LIMIT:
                beyond.append((d3.lds_bytes(direction, shape), tuple(shape)))
                break
    assert beyond, f"{direction}: no neighbour of {top} passes the LDS limit inside the kernels' range"
    return top, min(beyond)[1]


def samples(direction, name, smallest, rng):
    """seeded geometries of one instantiation, no larger than the cap"""
    cap = max(STRESSED_ELEMS, 2 * volume(smallest))
    out = set()
    tries = 0
    while len(out) < SAMPLES and tries < 400 * SAMPLES:
        tries += 1
        D1, D2, D3 = rng.randint(4, MAX_D1[direction]), rng.randint(4, 64), rng.randint(2, 32)
        if D1 * D2 * D3 > cap:
            continue
        top = (min(32, D1 // 2), min(32, D2 // 2), min(8, D3 // 2 + 1))
        m1, m2, m3 = (t if rng.random() < 1 / 3 else rng.randint(1, t) for t in top)
        shape = (N_VOL, D1, D2, D3, m1, m2, m3)
        if d3.kernel_name(direction, shape) == name:
            out.add(shape)
    return sorted(out)


def edges(direction, shape):
    return d3.coverage_of({"dir": direction, "shape": shape})


def stress(direction, shape):
    """how many edges a geometry sits on: the COVERAGE ones, and what makes the loops of the kernels run more than once or end ragged -
    more than one and more than two slots / planes per wave (8 waves), an axis without an N/2 partner, a ragged last dim2 k-step, slot
    tile and T block, a last slot tile that is filled up to its last four lanes"""
    n, D1, D2, D3, m1, m2, m3 = shape
    per_wave = (D1 + 1) // 2 if direction == "fwd" else D1
    nslot2 = (D2 + 1) // 2
    more = [per_wave > 8, per_wave > 16, D1 % 2 == 1, D2 % 2 == 1, m2 % 4 != 0, nslot2 % 16 != 0, D3 % 16 != 0]
    # (counted twice: the last slot tile is ragged AND its lanes 12 .. 15 hold rows - K3v's store-data hazard showed in those lanes only)
    return len(edges(direction, shape)) + sum(more) + 2 * (nslot2 % 16 >= 13)


def build_table():
    entries = []
    for direction in ("fwd", "inv"):
        small = smallest_shapes(direction)
        top, beyond = largest_lds(direction)
        stressed = {d3.kernel_name(direction, top): top}
        pools = {}
        for name in sorted(small):
            rng = random.Random(d3.entry_seed({"name": name, "dir": direction, "shape": small[name]}))
            pools[name] = [s for s in samples(direction, name, small[name], rng) if s != small[name]]
            assert pools[name], name

        def rank(shape):
            per_wave = (shape[1] + 1) // 2 if direction == "fwd" else shape[1]
            return (per_wave <= 8, -stress(direction, shape)) + order(shape)      # first of all: the software-pipelined loops run
        for want in (c for c in d3.COVERAGE if c.startswith(direction)):
            if any(want in edges(direction, s) for s in stressed.values()):
                continue
            able = [(rank(s), name, s) for name in pools if name not in stressed for s in pools[name] if want in edges(direction, s)]
            assert able, f"no sampled geometry of a free instantiation sits on '{want}'"
            _, name, shape = min(able)
            stressed[name] = shape
        for name in pools:
            if name not in stressed:
                stressed[name] = min(pools[name], key=rank)
        for name in sorted(small):
            entries.append({"name": name, "dir": direction, "role": "smallest", "shape": list(small[name])})
            entries.append({"name": name, "dir": direction, "role": "largest-lds" if stressed[name] == top else "stressed",
                            "shape": list(stressed[name])})
        entries.append({"name": d3.PLANE_PATH, "dir": direction, "role": "beyond-lds", "shape": list(beyond)})
    return entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=d3.TABLE)
    a = ap.parse_args()
    entries = build_table()
    with open(a.out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    for direction in ("fwd", "inv"):
        mine = [e for e in entries if e["dir"] == direction]
        names = {e["name"] for e in mine} - {d3.PLANE_PATH}
        print(f"{direction}: {len(names)} instantiations, {len(mine)} entries, largest volume {max(volume(e['shape']) for e in mine)} elements, "
              f"largest LDS footprint {max(d3.lds_bytes(direction, e['shape']) for e in mine if e['name'] != d3.PLANE_PATH)} bytes")
    print(f"-> {a.out}")


if __name__ == "__main__":
    main()
