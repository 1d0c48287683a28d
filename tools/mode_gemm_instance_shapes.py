#!/usr/bin/env python3
"""Write tests/golden/mode_gemm_instances.json: for every configuration of the per-mode GEMM (tests/mode_gemm_instances.py: kernel,
flavour and run-time arguments) that a call can reach, the smallest shape that reaches it and a stressed one.  Needs the built library and
no GPU: which configuration a shape takes is asked of the library's plan query (uno_mode_gemm_plan / uno_mode_backward_plan), never
worked out here.

    python tools/mode_gemm_instance_shapes.py [--out FILE]

Search box ("the fine box"; symmetric in B, Ci, Co, so one scan with op 0 meets every (M, N, K) of the three ops; each entry is then confirmed with its own
op and flavour): the three sizes from CHANNELS, 1 / 2 / 4 corners, the modes per corner of mode_gemm_instances.mode_counts(GROUPS), and
M N K corners modes <= WORK_MAX multiply-adds.  "Smallest" means smallest in that box by M N K corners modes (ties: the smaller tuple).
A stressed shape meets ALL of mode_gemm_instances.stress_failures and has 2 or 4 corners: ops 0 and 2 and the plain pair prefer 2, op 1 and the
accumulating pair 4, and take the other where the preferred count cannot reach the configuration.

huge_out entries (K <= 32, an output above 200 MB) are searched on their own: the smallest output over the limit with M, N >= 16, at K = 1
(smallest) and at K = 9 with the stressed shape's other properties.  They are the only large entries.

Configurations (and stressed shapes) that the fine box does not reach are looked for in the scan box of the CPU test
(mode_gemm_instances.SCAN_CHANNELS, SCAN_CORNERS, SCAN_GROUPS) up to WIDE_WORK_MAX multiply-adds: a pair whose input-gradient role does
not split K needs 2048 tasks, which fewer than 48 mode groups per corner give only with hundreds of modes and wide layers; the stressed
shape of the 8-mode unpipelined LDS form needs 4 x 65 modes, K >= 96 and more than one tile.

A configuration of the declared space that gets no entry must be listed in UNREACHABLE of tests/test_mode_gemm_instances_cpu.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mode_gemm_instances as mg

CHANNELS = sorted(set(range(1, 21)) | {24, 31, 32, 33, 48, 49, 64, 65, 96, 97, 98, 100, 128, 130, 140})
CORNERS = (1, 2, 4)
GROUPS = sorted(set(range(1, 13)) | {16, 24, 31, 47, 48, 49, 50})
WORK_MAX = 2500000
WIDE_WORK_MAX = 100000000   # pair configurations that need more (2048 tasks on fewer than 48 mode groups ...): the scan box of the CPU test
HUGE_BYTES = 200e6          # the huge_out limit of the plan, here only to aim the search: the plan query decides


def _work(shape):
    B, Ci, Co, nc, Mc = shape
    return B * Ci * Co * nc * Mc


def _better(best, key, shape):
    if key not in best or (_work(shape), shape) < (_work(best[key]), best[key]):
        best[key] = shape


def single_entries():
    from uno_amd import _native
    smallest, stressed = {}, {}
    fine = mg.scan_plans(CHANNELS, CORNERS, mg.mode_counts(GROUPS), WORK_MAX)
    wide = mg.scan_plans(mg.SCAN_CHANNELS, mg.SCAN_CORNERS, mg.mode_counts(mg.SCAN_GROUPS), WIDE_WORK_MAX)
    for scan in (fine, wide):
        found, found_stressed = set(smallest), {c for c, _ in stressed}       # the wide box only adds what the fine one does not reach
        for shape, ints in scan:
            plan = mg.plan_from_ints(ints)
            config = mg.config_of_plan(plan)
            B, Ci, Co, nc, Mc = shape
            gemm = (plan.M, plan.N, plan.K, nc, Mc)                     # the shape in GEMM terms: what the decision depends on
            if config not in found:
                _better(smallest, config, gemm)
            if config not in found_stressed and nc in (2, 4) and not mg.stress_failures((plan.M, plan.N, plan.K), nc, Mc, plan):
                _better(stressed, (config, nc), gemm)
    entries = []
    for config in mg.declared_space():
        if mg.family_of(config) == "pair" or config.endswith("huge_out"):
            continue
        flavour = mg.flavour_of(config)
        plain = config.replace("/" + flavour + "/", "/plain/")
        if plain not in smallest:
            continue
        for op in mg.FLAVOUR_OPS[flavour]:
            prefer = (4, 2) if op == 1 else (2, 4)
            picks = [("smallest", smallest[plain])]
            picks += [("stressed", stressed[(plain, nc)]) for nc in prefer if (plain, nc) in stressed][:1]
            for role, (M, N, K, nc, Mc) in picks:
                entries.append(_confirmed(config, op, role, (*mg.call_dims(op, M, N, K), nc, Mc)))
    return entries


def _confirmed(config, op, role, shape):
    """the table entry, after asking the library for this very call (op, flavour) and finding the configuration"""
    e = {"config": config, "op": op, "role": role, "shape": list(shape)}
    plan = mg.entry_plan(e)
    assert mg.config_of_plan(plan) == config, (e, plan)
    e["plan"] = list(plan)
    return e


def huge_entries():
    """lds<16, false>/*/huge_out: the smallest output over the limit, not padded, M, N >= 16"""
    from uno_amd import _native
    entries = []
    for role, K, ok in (("smallest", 1, lambda M, N, nc, Mc: True),
                        ("stressed", 9, lambda M, N, nc, Mc: M % 4 and N % 4 and Mc % 16 and nc in (2, 4) and (nc * ((Mc + 15) // 16)) % 8)):
        best = None
        for nc in CORNERS:
            for M in range(16, 141):
                for N in range(M, 141):
                    Mc = int(HUGE_BYTES // (8 * M * N * nc)) + 1
                    while 16 * ((Mc + 15) // 16) * 5 > Mc * 6:          # skip padded counts (aim only: confirmed below)
                        Mc += 1
                    if Mc > 4096 or not ok(M, N, nc, Mc):
                        continue
                    cand = (M * N * nc * Mc, (M, N, K, nc, Mc))
                    if best is None or cand < best:
                        best = cand
        M, N, K, nc, Mc = best[1]
        plan = _native.mode_gemm_plan(0, M, K, N, nc, Mc)
        assert plan.family == 1 and plan.refused == 2, plan
        below = _native.mode_gemm_plan(0, M, K, N, nc, Mc - 1)
        assert below.refused != 2, "not the smallest mode count over the limit"
        for flavour in mg.FLAVOURS:
            for op in mg.FLAVOUR_OPS[flavour]:
                entries.append(_confirmed(mg.lds_config(16, 0, flavour, "huge_out"), op, role, (*mg.call_dims(op, M, N, K), nc, Mc)))
    return entries


def pair_entries():
    smallest, stressed, relaxed = {}, {}, {}
    fine = mg.scan_plans(CHANNELS, CORNERS, mg.mode_counts(GROUPS), WORK_MAX, pair=True)
    wide = mg.scan_plans(mg.SCAN_CHANNELS, mg.SCAN_CORNERS, mg.mode_counts(mg.SCAN_GROUPS), WIDE_WORK_MAX, pair=True)
    for scan in (fine, wide):
        found_fine = set(smallest)                  # the wide box only adds configurations the fine one does not reach
        found_fine_stressed = {c for c, _ in stressed}
        for shape, ints in scan:
            if not ints[0]:
                continue
            pp = mg.plan_from_ints(ints, pair=True)
            config = mg.config_of_pair_plan(pp)
            B, Ci, Co, nc, Mc = shape
            if config not in found_fine:
                _better(smallest, config, shape)
            if config not in found_fine_stressed and nc in (2, 4) and not mg.stress_failures((pp.b.M, pp.b.N, pp.b.K), nc, Mc, pp.b):
                if not mg.stress_failures((pp.a.M, pp.a.N, pp.a.K), nc, Mc, pp.a, min_K=16):
                    _better(stressed, (config, nc), shape)
                elif not mg.stress_failures((pp.a.M, pp.a.N, pp.a.K), nc, Mc, pp.a, min_K=16, strict_rows=False):
                    _better(relaxed, (config, nc), shape)
    for key, shape in relaxed.items():              # one ragged row tile where no shape of the boxes has more (see stress_failures)
        if not any((key[0], nc) in stressed for nc in (2, 4)):
            stressed[key] = shape
    entries = []
    for config in mg.declared_space():
        if mg.family_of(config) != "pair":
            continue
        flavour = mg.flavour_of(config)
        plain = config.replace("/" + flavour + "/", "/plain/")
        if plain not in smallest:
            continue
        prefer = (4, 2) if flavour == "acc" else (2, 4)
        picks = [("smallest", smallest[plain])]
        picks += [("stressed", stressed[(plain, nc)]) for nc in prefer if (plain, nc) in stressed][:1]
        for role, shape in picks:
            e = {"config": config, "role": role, "shape": list(shape)}
            pp = mg.entry_plan(e)
            assert mg.config_of_pair_plan(pp) == config, (e, pp)
            e["plan"] = [*pp[:4], *pp.a, *pp.b]
            entries.append(e)
    return entries


def build_table():
    return single_entries() + huge_entries() + pair_entries()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=mg.TABLE)
    a = ap.parse_args()
    entries = build_table()
    with open(a.out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    have = {e["config"] for e in entries}
    missing = [c for c in mg.declared_space() if c not in have]
    no_stress = sorted({e["config"] for e in entries} - {e["config"] for e in entries if e["role"] == "stressed"})
    print(f"{len(entries)} entries, {len(have)} of {len(mg.declared_space())} configurations reached")
    for c in missing:
        print("  no shape in the box reaches", c)
    for c in no_stress:
        print("  no stressed shape in the box for", c)


if __name__ == "__main__":
    main()
