"""CPU side of tests/test_hip_launch_state.py: the two process-wide setters round-trip without a device (they touch no GPU state; the
library loads here as tests/test_capi_symbols.py loads it), and a census of csrc: every launcher that takes a sweep direction from
next_sweep_reversed has a case in that file's DIRECTION_CASES, so a new sweep-taking family without a test fails here."""
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "uno_amd", "csrc")
BITS = {"SWEEP_K1": 1, "SWEEP_K3": 2, "SWEEP_K7": 4, "SWEEP_K8": 8, "SWEEP_K9": 16, "SWEEP_NORM": 32, "SWEEP_PROJ": 64, "SWEEP_LIFT": 128}

NORM_CASES = [f"norm_{form}_{act}{dt}" for form in ("reg", "sweep") for act in ("gelu", "plain") for dt in ("", "_bf16")]
# (source file, family, the launcher's occurrence in that file) -> the DIRECTION_CASES that launch it
LAUNCHERS = {
    ("dft2d_fwd_ft_kernel.h", "SWEEP_K1", 0): ["k1_ft"],
    ("dft2d_fwd_ht_kernel.h", "SWEEP_K1", 0): ["k1_ht"],
    ("dft2d_inv_kernel.h", "SWEEP_K3", 0): ["k3", "k3_bf16"],                 # launch_inv_k
    ("dft2d_inv_kernel.h", "SWEEP_K3", 1): ["k3_ft"],                         # launch_inv_t: the full-tile form
    ("dft2d_inv_add_kernel.h", "SWEEP_K3", 0): ["k3a_inverse_add"],
    ("resample2d.hip", "SWEEP_K7", 0): ["k7_down", "k7_up", "k7_accumulate", "k7_down_bf16", "k7_up_bf16", "k7_accumulate_bf16"],
    ("channel_mix.hip", "SWEEP_K8", 0): ["k8_generic", "k8_generic_act_in", "k8_wide128", "k8_split", "k8_split_bf16",
                                         "k8_two_sources_two_destinations", "k8_window", "k8_act_padded_dgelu_padded",
                                         "lift_unfused_virtual_input"],                                    # launch_channel_mix2
    ("channel_wgrad.hip", "SWEEP_K9", 0): ["lift_unfused_virtual_input"],                                  # launch_channel_wgrad_vh
    ("channel_wgrad.hip", "SWEEP_K9", 1): ["k9_vector", "k9_narrow", "k9_few_in", "k9_split", "k9_wgrad2", "k9_window"],   # launch_channel_wgrad2
    ("instnorm.hip", "SWEEP_NORM", 0): NORM_CASES,                                                         # launch_instnorm_fwd
    ("instnorm.hip", "SWEEP_NORM", 1): NORM_CASES,                                                         # launch_instnorm_bwd
    ("pointwise_fused.hip", "SWEEP_PROJ", 0): ["proj_backward", "proj_backward_win"],
    ("lift_bwd.hip", "SWEEP_LIFT", 0): ["lift_forward_backward", "lift_backward2"],                        # launch_lift_forward_fused
    ("lift_bwd.hip", "SWEEP_LIFT", 1): ["lift_forward_backward", "lift_backward2"],                        # launch_lift_backward_fused
}


@pytest.fixture(scope="module")
def lib():
    from uno_amd import build, _native
    build.build()
    return _native.lib()


def _found():
    out = []
    for name in sorted(os.listdir(CSRC)):
        if name == "capi.hip" or not name.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        text = re.sub(r"//[^\n]*", "", text)                     # (uno_common.h's declaration survives: it names no SWEEP_ constant)
        count = {}
        for fam in re.findall(r"next_sweep_reversed\(\s*(SWEEP_[A-Z0-9]+)\s*\)", text):
            out.append((name, fam, count.get(fam, 0)))
            count[fam] = count.get(fam, 0) + 1
        assert len(re.findall(r"next_sweep_reversed\(", text)) == sum(count.values()) + (1 if name == "uno_common.h" else 0), \
            f"{name}: a next_sweep_reversed call whose family this census cannot read"
    return out


def test_every_sweep_taking_launcher_has_a_direction_case():
    from test_hip_launch_state import DIRECTION_CASES
    found = _found()
    assert len(found) >= 14
    assert sorted(found) == sorted(LAUNCHERS), "the launchers that call next_sweep_reversed changed: give the new one a case in " \
        "tests/test_hip_launch_state.py (DIRECTION_CASES) and list it in LAUNCHERS"
    for (name, fam, k), cases in LAUNCHERS.items():
        assert cases, (name, fam, k)
        for c in cases:
            assert c in DIRECTION_CASES, c
            assert DIRECTION_CASES[c][0] & BITS[fam], f"{c} is not registered under {fam}"
    listed = {c for cases in LAUNCHERS.values() for c in cases}
    assert listed == set(DIRECTION_CASES), sorted(set(DIRECTION_CASES) - listed)


def test_family_bits_match_the_header():
    text = open(os.path.join(CSRC, "uno_common.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"(SWEEP_[A-Z0-9]+) = (\d+)", text))
    assert enum == BITS


def test_sweep_alternation_round_trip(lib):
    f = lib.uno_sweep_alternation
    first = f(255)
    try:
        assert first == 255                                 # the default: every family alternates
        assert f(0) == 255 and f(1) == 0
        assert f(8) == 255                                  # enable == 1 is stored as 255
        assert f(255) == 8                                  # other values 0 .. 255: a mask
        assert f(256 | 255) == 255 and f(256 | 8) == 511    # bit 8: pinned reversed, returned as set
        assert f(1024 | 256 | 3) == (256 | 8)               # higher bits are dropped
        assert f(-1) == (256 | 3) and f(-256) == 255        # negative values keep their meaning: the low eight bits, never the pin
        assert f(256 | 3) == 0
        assert f(256) == (256 | 3)                          # pinned with an empty mask: every launch front to back
        assert f(255) == 256
    finally:
        f(first)


def test_sweep_direction_binding(lib):
    from uno_amd import _native
    first = lib.uno_sweep_alternation(255)
    try:
        assert _native.sweep_direction("reversed") == 255
        assert _native.sweep_direction("forward") == 511
        assert _native.sweep_direction("reversed", mask=32) == 0
        assert _native.sweep_direction("alternate", mask=24) == (256 | 32)
        assert _native.sweep_direction("alternate") == 24
        assert _native.sweep_alternation(True) is True      # the older switch is unchanged: on / off
        assert _native.sweep_alternation(False) is True and lib.uno_sweep_alternation(255) == 0
        for bad in (("sideways", 255), ("reversed", 256), ("reversed", -1), ("alternate", 1)):
            with pytest.raises(ValueError):
                _native.sweep_direction(*bad)
        assert lib.uno_sweep_alternation(255) == 255
    finally:
        lib.uno_sweep_alternation(first)


def test_reserve_cus_round_trip(lib):
    f = lib.uno_reserve_cus
    first = f(0)
    try:
        assert first == 0
        assert f(16) == 0 and f(248) == 16
        assert f(-5) == 248 and f(0) == 0                   # negative: clamped to 0
        from uno_amd import _native
        assert _native.reserve_cus(7) == 0 and _native.reserve_cus(0) == 7
    finally:
        f(first)
