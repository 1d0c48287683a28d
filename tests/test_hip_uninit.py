"""No result may depend on what torch.empty memory held before the call.

The parity tests compare values, the red-zone fixture (tests/test_hip_redzone.py) guards stores, the NaN-wrapped inputs guard reads.
None of them sees a kernel that leaves part of a result unwritten, or sums a workspace row nobody wrote: the caching allocator hands
back the block the previous call of the same shape just freed, which holds the right values.  Here every device tensor that the
library takes from torch.empty / torch.empty_like arrives filled with a chosen byte, between the red-zone fixture's two 64 KiB guard
bands:

    0xFF    NaN as float32, bfloat16, float16, float64 and complex64; -1 as int32
    0x7F    3.39e38 - finite and huge - as float32 and bfloat16, NaN as float16, 2139062143 as int32: for code that swallows a NaN
            (fmaxf, `x > 0 ? ... : ...`) and for workspace words read as integers

Kernel level: the float64 parity bodies of the other test files, imported and re-run unchanged under both bytes at their smallest
ragged cases - reference and tolerance are theirs, none is introduced here.  Every one of them asserts `error < bound`, `torch.equal`
or an integer-bit comparison, all of which fail on a NaN (checked body by body when this file was written).  One blind spot, covered
by the other byte: where a bfloat16 kernel is compared with its float32 twin and BOTH leave the same element unwritten, 0x7F reads as
the same huge value on both sides.
Module and model level: each workload runs three times - on ordinary memory, under 0xFF, under 0x7F - and its results (outputs, input
and parameter gradients or updated parameters, losses: what the caller's contract defines, no padded intermediate) must be finite
and bit-equal across the three.

Every test asserts how many poisoned allocations it saw, so that a body which stops allocating through the fixture fails instead of
passing vacuously; the model-level minima are the counts measured on the MI355X when this file was written.  A CPU census pins the
assumption all of this rests on: the library allocates device memory through no other call.  Out of scope: memory the library takes
from hipMalloc itself (operand tables), graph-captured paths (the fills would be captured; the eager paths run the same kernels).
pytest -m gpu"""
import ast
import inspect
import os
import re

import pytest
import torch

import test_hip_adam as t_adam
import test_hip_bf16_block as t_bf16
import test_hip_block3d_any as t_block3d_any
import test_hip_channel_mix as t_mix
import test_hip_fused_upsample as t_upsample
import test_hip_gelu_project2 as t_proj2
import test_hip_instnorm as t_norm
import test_hip_layout as t_layout
import test_hip_pointwise_fused as t_fused
import test_hip_project_backward as t_projbwd
import test_hip_resample as t_resample
import test_hip_resample3d_any as t_resample3d_any
import test_hip_rollout as t_rollout
import test_hip_rollout_train as t_rollout_train
import test_hip_spectral2d as t_spec2d
import test_hip_spectral3d as t_spec3d
import test_hip_step_errors as t_step_errors
import test_hip_window as t_window
from test_hip_redzone import GUARD, RedZone, _lift_and_window_pass, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES = [0xFF, 0x7F]
BYTE_IDS = ["ff", "7f"]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ 1. the fixture
class Poison(RedZone):
    """RedZone whose torch.empty / empty_like bodies are filled with `byte`; zeros / zeros_like stay zero, the guard bands and the
    512-byte alignment are RedZone's.  check() verifies the guards and returns the number of POISONED allocations since the last
    check; `served` then holds the number of all allocations the fixture made (zeros included)."""

    def __init__(self, monkeypatch, byte):
        super().__init__(monkeypatch)
        self.byte, self.poisoned, self.served = int(byte), 0, 0

    def _fill(self, t, before):
        if len(self.records) > before:              # a guarded allocation (host tensors and keyword forms pass through unguarded)
            raw, nbytes = self.records[-1]
            raw[GUARD:GUARD + nbytes].fill_(self.byte)
            self.poisoned += 1
        return t

    def empty(self, *size, dtype=None, device=None, **kw):
        before = len(self.records)
        return self._fill(super().empty(*size, dtype=dtype, device=device, **kw), before)

    def empty_like(self, t, **kw):
        before = len(self.records)
        return self._fill(super().empty_like(t, **kw), before)

    def check(self, what):
        self.served = super().check(what)
        n, self.poisoned = self.poisoned, 0
        return n


@pytest.fixture(params=BYTES, ids=BYTE_IDS)
def poison(request, monkeypatch):
    return Poison(monkeypatch, request.param)


# ------------------------------------------------------------------------------------------------------------------ 2. self-tests
def test_the_two_bytes_mean_what_the_tests_rely_on():
    """CPU: a byte-filled buffer seen as each dtype the kernels read"""
    def seen(byte, dtype):
        return torch.full((64,), byte, dtype=torch.uint8).view(dtype)
    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        assert bool(torch.isnan(seen(0xFF, dtype)).all()), dtype
    c = torch.view_as_real(seen(0xFF, torch.complex64))
    assert bool(torch.isnan(c).all())
    assert bool((seen(0xFF, torch.int32) == -1).all())
    for dtype in (torch.float32, torch.bfloat16):
        v = seen(0x7F, dtype).double()
        assert bool(torch.isfinite(seen(0x7F, dtype)).all()) and bool(((v > 3.38e38) & (v < 3.40e38)).all()), dtype
    assert bool(torch.isnan(seen(0x7F, torch.float16)).all())
    assert bool((seen(0x7F, torch.int32) == 2139062143).all())
    # the remaining two: finite and far beyond any value of the workloads (a sum that takes one in fails its bound)
    assert bool(torch.isfinite(seen(0x7F, torch.float64)).all()) and bool((seen(0x7F, torch.float64) > 1e300).all())
    c = torch.view_as_real(seen(0x7F, torch.complex64))
    assert bool(torch.isfinite(c).all()) and bool((c > 3.38e38).all())


@pytest.mark.gpu
def test_fixture_poisons_empty_and_leaves_zeros(poison):
    byte = poison.byte
    like = torch.ones((3, 5), dtype=torch.bfloat16, device=dev())
    for t in (torch.empty((7, 33), dtype=torch.float32, device=dev()), torch.empty(1001, dtype=torch.uint8, device=dev()),
              torch.empty((2, 3, 5), dtype=torch.complex64, device=dev()), torch.empty_like(like)):
        assert t.data_ptr() % 512 == 0
        assert bool((t.contiguous().view(-1).view(torch.uint8) == byte).all())
    for t in (torch.zeros((7, 33), dtype=torch.float32, device=dev()), torch.zeros_like(like)):
        assert t.data_ptr() % 512 == 0
        assert bool((t.view(-1).view(torch.uint8) == 0).all())
    assert torch.empty((4,), dtype=torch.float32).device.type == "cpu"          # host tensors pass through
    assert poison.check("self-test") == 4 and poison.served == 6
    # a result with ONE element left unwritten fails through the helper the workload tests use
    full = torch.arange(35, dtype=torch.float32, device=dev()).view(5, 7)
    part = torch.empty((5, 7), dtype=torch.float32, device=dev())
    part.view(-1)[:34] = full.view(-1)[:34]
    with pytest.raises(AssertionError, match="non-finite result" if byte == 0xFF else "reached the result"):
        _same([part], [full], "one element unwritten")
    part.view(-1)[34] = 34.0
    _same([part], [full], "all written")
    # and the guards are still RedZone's
    torch.as_strided(part.view(-1), (36,), (1,)).fill_(1.0)
    with pytest.raises(AssertionError, match="damaged guard band"):
        poison.check("deliberate overrun")


# ------------------------------------------------------------------------------------------------------------------ 3. census
_VIA_FIXTURE = {"empty", "empty_like", "zeros", "zeros_like"}


def allocation_offences(source, name="<source>"):
    """ways of allocating that the fixture would not see, or would pass through unpoisoned, in one Python source text"""
    found = []
    for pat, why in ((r"\.new_empty\(", "Tensor.new_empty"), (r"empty_strided", "empty_strided")):
        for m in re.finditer(pat, source):
            found.append(f"{name}:{source.count(chr(10), 0, m.start()) + 1}: {why}")
    tree = ast.parse(source)
    called = {id(n.func) for n in ast.walk(tree) if isinstance(n, ast.Call)}
    for n in ast.walk(tree):
        if isinstance(n, ast.ImportFrom) and n.module == "torch":
            for a in n.names:
                if a.name in _VIA_FIXTURE or a.name == "*":
                    found.append(f"{name}:{n.lineno}: from torch import {a.name} (a name bound before the fixture patches torch)")
        is_torch_alloc = (isinstance(n, ast.Attribute) and n.attr in ("empty", "empty_like") and isinstance(n.value, ast.Name)
                          and n.value.id == "torch")
        if is_torch_alloc and id(n) not in called:
            found.append(f"{name}:{n.lineno}: torch.{n.attr} taken as a value, not called")
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in ("empty", "empty_like") \
                and isinstance(n.func.value, ast.Name) and n.func.value.id == "torch":
            # RedZone guards torch.empty(size, dtype=, device=) and torch.empty_like(t); any other keyword goes to torch as it is
            extra = sorted({k.arg for k in n.keywords} - ({"dtype", "device"} if n.func.attr == "empty" else set()))
            if extra:
                found.append(f"{name}:{n.lineno}: torch.{n.func.attr}({', '.join(str(e) + '=' for e in extra)}) passes the fixture unpoisoned")
    return found


def test_the_library_allocates_device_memory_through_the_fixtures_calls_only():
    """CPU: every .py file under uno_amd/ - no Tensor.new_empty, no empty_strided, no `from torch import empty...`, no torch.empty with
    pin_memory= / memory_format= (or any keyword besides dtype and device), no torch.empty_like with keywords"""
    bad = ["x.new_empty((3,))", "torch.empty_strided((2, 2), (2, 1))", "from torch import empty", "from torch import zeros_like as z",
           "torch.empty(3, device=d, pin_memory=True)", "torch.empty((3,),\n   memory_format=torch.channels_last)",
           "torch.empty_like(x, dtype=torch.float32)", "make = torch.empty"]
    for text in bad:                                        # the detector itself
        assert allocation_offences("import torch\n" + text), text
    assert not allocation_offences("import torch\ny = torch.empty((B, C), dtype=x.dtype, device=x.device)\nz = torch.empty_like(y)\n")
    found, files, calls = [], 0, 0
    for folder, _, names in os.walk(os.path.join(ROOT, "uno_amd")):
        for fname in sorted(names):
            if fname.endswith(".py"):
                path = os.path.join(folder, fname)
                with open(path, encoding="utf-8") as f:
                    source = f.read()
                files += 1
                calls += len(re.findall(r"\btorch\.empty(?:_like)?\(", source))
                found += allocation_offences(source, os.path.relpath(path, ROOT))
    assert files >= 10 and calls >= 80, (files, calls)      # the census looked at the library (79 calls in _native.py alone)
    assert not found, "\n".join(found)


# ------------------------------------------------------------------------------------------------------------------ 4. kernel level
def K(name, fn, *args, count="poisoned"):
    return pytest.param((fn, args, count), id=name + "-" + re.sub(r"[^0-9A-Za-z]+", "_", repr(args)).strip("_"))


def _product(name, fn, *lists):
    """the cases of every combination of one entry per list; an entry that is a LIST stands for several positional arguments"""
    cases = [()]
    for values in lists:
        cases = [c + (tuple(v) if isinstance(v, list) else (v,)) for c in cases for v in values]
    return [K(name, fn, *c) for c in cases]


BOOLS = [False, True]
# The cases are the ones the issue of this file names: the one or two smallest ragged entries of each test's own parameter list.
# Where it left the choice open: the smallest entry of TWO that each two-source test accepts ((2, 64, 64, 64, 3); (1, 64, 192, 256, 130)
# for the weight gradient, which needs 64 pixels); of WINDOWS the smallest plane, (9, 264, 264, 9) - where the window is the whole plane -
# and the smallest window, (7, 260, 301, 11), which has a border that a windowed kernel leaves unwritten; the smallest dense and the
# smallest windowed entry of the projection backward's CASES; the two smallest SHAPES of gelu_project2.
# test_every_reused_case_is_one_of_the_reused_tests_own (CPU) holds every tuple to the current lists.
WIN_SMALL = [(9, 264, 264, 9), (7, 260, 301, 11)]
KERNEL_CASES = (
    _product("dft2d_forward", t_spec2d.test_dft2d_forward_stage, [(2, 21, 18, 4, 5), (5, 37, 91, 6, 9), (128, 5, 7, 2, 4)], [(False, False), (True, True)])
    + _product("dft2d_inverse", t_spec2d.test_dft2d_inverse_stage, [(2, 21, 18, 4, 5), (5, 37, 91, 6, 9), (128, 5, 7, 2, 4)], [(False, False), (True, True)])
    + _product("mode_gemms", t_spec2d.test_mode_gemms, [(5, 7, 9, 2, (3, 11)), (17, 115, 45, 2, (3, 4))])
    + [K("paired_backward_gemms", t_spec2d.test_paired_backward_gemms_equal_the_two_single_launches, 3, 20, 12, 5, 4, True),
       K("conv2d_seeded", t_spec2d.test_seeded_vs_dense_oracle, (3, 5, 3, 37, 50, 29, 31, 9, 13)),
       K("conv2d_any_mode", t_spec2d.test_any_mode_count_vs_dense_oracle, (1, 1, 2, 50, 50, 42, 44, 42, 10)),
       K("conv3d_seeded", t_spec3d.test_seeded_3d_vs_dense_oracle, t_spec3d.SEEDED3[2]),
       K("conv3d_volume", t_spec3d.test_seeded_3d_vs_dense_oracle, t_spec3d.VOLUME3[2]),
       K("fft_resample3d", t_spec3d.test_fft_resample3d_matches_the_reference_op_sequence, t_spec3d.RESAMPLE3D[0]),
       K("fft_resample3d_any", t_resample3d_any.test_any_grid_resample_matches_the_reference_op_sequence, t_resample3d_any.OPERATOR_CASES[0])]
    + _product("resample3d_any_act", t_block3d_any.test_activation_form, [t_block3d_any.CASES[0]], BOOLS)
    + _product("k8_forward", t_mix.test_forward, [[2, 3, 5, 17], [4, 100, 36, 4097], [2, 3, 17, 1025]], BOOLS)
    + _product("k8_transposed", t_mix.test_transposed, [[2, 3, 5, 17], [4, 100, 36, 4097], [2, 3, 17, 1025]])
    + _product("k9_wgrad", t_mix.test_wgrad, [[2, 3, 5, 17], [4, 100, 36, 4097], [2, 3, 17, 1025]])
    + _product("k8_two_source", t_mix.test_two_source_forward, [[2, 64, 64, 64, 3]], BOOLS)
    + _product("k8_two_destination", t_mix.test_two_destination_input_gradients, [[2, 64, 64, 64, 3]], BOOLS)
    + _product("k9_two_source", t_mix.test_two_source_wgrad, [[1, 64, 192, 256, 130]], BOOLS)
    + [K("k9_two_stage", t_mix.test_wgrad_first_stage_then_one_second_stage, 1, 192, 0, 96, 77, False)]
    + _product("k8_fused_projection", t_mix.test_fused_projection, [[2, 64, 64, 33, 77]], BOOLS)
    + [K("k8_split_wide", t_mix.test_split_bf16_wide_layers, 2, 160, 0, 128, 300),
       K("k8_split_64", t_mix.test_split_bf16_64_channel_tiles, 2, 96, 64, 64, 515)]
    # (not the "accumulate" variant, nor the accumulating 64-channel forms of the windowed input gradient below: they add into tensors
    # the test made and take nothing from torch.empty - nothing for this file to see; the 128-channel accumulating form stays, its
    # pre-split weights live in a poisoned scratch buffer)
    + _product("k8_bf16", t_bf16.test_channel_mix_bf16, [(3, 5, 7, 50)], ["plain", "transpose", "act_in", "dgelu"])
    + _product("k9_bf16", t_bf16.test_channel_wgrad_bf16, [(3, 5, 7, 50)], BOOLS)
    + _product("instnorm_bf16", t_bf16.test_instnorm_bf16, [(3, 6, 7)], BOOLS)
    + [K("gelu_pad_bf16", t_bf16.test_gelu_pad_bf16, (2, 33, 35, 40, 47))]
    + _product("win_forward", t_window.test_forward_window_equals_dense_on_the_crop, [list(w) for w in WIN_SMALL],
               [[64, 64, 64, True], [32, 0, 40, False], [128, 0, 128, False], [64, 64, 64, False], [16, 16, 24, True]])
    + _product("win_projection", t_window.test_fused_projection_window, [list(w) for w in WIN_SMALL])
    + _product("win_input_gradient", t_window.test_input_gradient_window, [list(w) for w in WIN_SMALL],
               [[64, 64, True, 0], [64, 32, False, 0], [128, 128, True, 1], [128, 64, False, 0]])
    + _product("win_weight_gradient", t_window.test_weight_gradient_window, [list(w) for w in WIN_SMALL],
               [[64, 64, 64, True], [64, 0, 64, False], [128, 128, 128, False], [64, 64, 32, False], [128, 0, 256, True]])
    + _product("win_gelu_project_backward", t_window.test_gelu_project_backward_window, [list(w) for w in WIN_SMALL])
    + [K("lift_padded_activation", t_window.test_lift_with_padded_activation, 2, 16, 40, 9, 300, 0, 5),
       K("whole_lift", t_window.test_whole_lift_without_stored_intermediates, 2, 1, 16, 24, 9, 300, 0, 5, True),
       K("lift_backward2", t_window.test_lift_backward_adds_a_second_gradient_as_it_reads, 1, 1, 130, 263, 1, 2),
       K("project_backward_dense", t_projbwd.test_project_backward_against_float64, 3, 64, 64, 48, 34000, True),
       K("project_backward_window", t_projbwd.test_project_backward_against_float64, 3, 64, 64, 64, (130, 264, 270, 133), True)]
    + _product("gelu_project2", t_proj2.test_gelu_project2, [[1, 1, 1, (1,)], [2, 5, 3, (3, 7)]], BOOLS, BOOLS, BOOLS)
    + _product("gelu_project", t_fused.test_gelu_project, [[2, 5, (3, 7)]], BOOLS)
    + [K("gelu_pad", t_fused.test_gelu_pad, (2, 3), (5, 7), (2, 3))]
    + _product("instnorm", t_norm.test_instance_norm_gelu, [(2, 3, 5, 7), (1, 2, 300, 300)], BOOLS, BOOLS)
    + _product("resample2d", t_resample.test_resample_forward_backward_vs_torch_cpu, [((7, 3), (5, 2)), ((36, 1000), (18, 500))])
    + [K("resample2d_accumulate", t_resample.test_resample_accumulates_into_out, ((20, 18), (41, 37))),
       K("resample3d_trilinear", t_resample.test_trilinear_resample_vs_torch_cpu, ((8, 10, 6), (8, 10, 11))),
       K("transposing_copy", t_layout.test_transposing_copy_both_directions, (3, 5, 37, 41)),
       K("rel_l2_steps", t_step_errors.test_against_float64, (3, 49, 9)),
       K("rollout_advance", t_rollout.test_all_steps_against_the_reference_update_and_float64, (3, 7, 3, 49, 4)),
       K("rollout_train", t_rollout_train.test_all_windows_against_float64, (3, 3, 4, 5, 49, 5)),
       K("rollout_train", t_rollout_train.test_all_windows_against_float64, (1, 28, 4, 3, 1028, 2)),
       K("inverse_add", t_upsample.test_fused_inverse_add_matches_two_kernels_and_float64, (4, 100, 105, 200, 210, 6, 5, False)),
       # K10 updates parameters and moments in place and takes no scratch: its only allocations are the moments, from torch.zeros.  The
       # case pins that under the fixture (zeros stay zero, the guards of the moments hold); it cannot see a poisoned tensor
       K("adam", t_adam.test_adam_kernel_matches_cpu_path, (33, 5, 3), True, count="served")]
)


def _own_cases(fn, args):
    """args of one call of a parametrised test function -> [(names, values, listed values)] per parametrize mark"""
    bound = dict(zip(inspect.signature(fn).parameters, args))
    out = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [s.strip() for s in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        listed = [tuple(getattr(v, "values", None) or (v if len(names) > 1 else (v,))) for v in mark.args[1]]
        out.append((names, tuple(bound[n] for n in names), listed))
    return out


def test_every_reused_case_is_one_of_the_reused_tests_own():
    """CPU: each tuple above is an entry of the parameter lists of the function it is handed to (a list edited later cannot leave this
    file running a shape nobody else checks, or a function with one argument fewer)"""
    assert len(KERNEL_CASES) >= 100
    for p in KERNEL_CASES:
        fn, args, _ = p.values[0]
        assert len(args) == len(inspect.signature(fn).parameters), p.id
        marks = _own_cases(fn, args)
        assert marks, p.id
        for names, got, listed in marks:
            assert got in listed, (p.id, names, got)
    assert min(t_window.WINDOWS, key=lambda w: w[3] * w[2]) == WIN_SMALL[0] and min(t_window.WINDOWS, key=lambda w: w[0] * w[1]) == WIN_SMALL[1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_parity_body_on_poisoned_memory(poison, case):
    fn, args, count = case
    fn(*args)
    n = poison.check(f"{fn.__module__}.{fn.__name__}{args} under 0x{poison.byte:02X}")
    print(f"[uninit 0x{poison.byte:02X}] {fn.__name__}{args}: {n} poisoned of {poison.served} allocations")
    assert (n if count == "poisoned" else poison.served) >= 1, "the body allocated nothing through the fixture: a vacuous case"


# ------------------------------------------------------------------------------------------------------------------ 5. modules and models
def _three_runs(monkeypatch, workload, minimum, what):
    """plain, 0xFF, 0x7F: finite, bit-equal results; at least `minimum` poisoned allocations in each poisoned run"""
    plain = workload()
    torch.cuda.synchronize()
    for byte in BYTES:
        with monkeypatch.context() as patch:
            zone = Poison(patch, byte)
            got = workload()
            n = zone.check(f"{what} under 0x{byte:02X}")
        print(f"[uninit 0x{byte:02X}] {what}: {n} poisoned of {zone.served} allocations (minimum {minimum})")
        assert len(got) == len(plain) and len(got) > 0
        _same(got, plain, f"{what} under 0x{byte:02X}")
        assert n >= minimum, f"{what}: {n} poisoned allocations, {minimum} when this test was written"


def _grads(module):
    return [p.grad for p in module.parameters()]


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("geom", [(37, 37, 55, 55), (55, 55, 37, 37), (70, 66, 35, 33)])
def test_operator_block_2d(monkeypatch, geom, normalize):
    """up-sampling, down-sampling (both with the fused resample-add where it applies) and a non-square block, one source and the
    two-source forward_cat form with 64 + 16 channels"""
    from uno_amd.integral_operators import OperatorBlock_2D
    H, W, Ho, Wo = geom

    def workload():
        torch.manual_seed(3)
        blk = OperatorBlock_2D(6, 5, Ho, Wo, 5, 6, Normalize=normalize).to(dev())
        x = torch.randn(2, 6, H, W, device=dev(), requires_grad=True)
        y = blk(x)
        y.square().sum().backward()
        two = OperatorBlock_2D(80, 7, Ho, Wo, 5, 6, Normalize=normalize).to(dev())
        a = torch.randn(2, 64, H, W, device=dev(), requires_grad=True)
        b = torch.randn(2, 16, H, W, device=dev(), requires_grad=True)
        y2 = two.forward_cat([a, b], Ho, Wo)
        y2.square().sum().backward()
        return [y.detach(), x.grad] + _grads(blk) + [y2.detach(), a.grad, b.grad] + _grads(two)
    _three_runs(monkeypatch, workload, MINIMA["block2d", geom, normalize], f"OperatorBlock_2D {geom} normalize={normalize}")


@pytest.mark.gpu
def test_lift_and_windowed_projection(monkeypatch):
    """the lift kernels and the windowed fc1 - GELU - fc2 path (widths >= 260): the planes whose borders are left uncleared on the
    promise that the lift's backward kernel reads the domain only"""
    _three_runs(monkeypatch, lambda: _lift_and_window_pass(False), MINIMA["lift_window"], "lift + windowed projection")


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["f32", "mixed"])
def test_darcy_training_steps(monkeypatch, mixed):
    """two whole UNO_9 steps at the ragged S = 75 (padded 80, levels 40 / 20): losses and updated parameters"""
    from uno_amd.harness import DarcyTrainer, UNO_9, synthetic_darcy_batch
    from uno_amd.harness.mixed import MixedDarcyTrainer

    def workload():
        torch.manual_seed(0)
        model = UNO_9(3, 16, pad=5).to(dev())
        tr = (MixedDarcyTrainer if mixed else DarcyTrainer)(model, lr=1e-3, weight_decay=1e-3)
        a, u = synthetic_darcy_batch(2, 75, 5, dev())
        losses = [tr.step(a, u) for _ in range(2)]
        return losses + [p.detach().clone() for p in model.parameters()]
    _three_runs(monkeypatch, workload, MINIMA["darcy", mixed], f"Darcy steps mixed={mixed}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,width,native", [("UNO", 8, False), ("UNO", 8, True), ("UNO_P", 4, False)],
                         ids=["UNO-default", "UNO-native", "UNO_P-default"])
def test_ns2d_training_steps(monkeypatch, name, width, native):
    """three NS-2D roll-out steps at 64^2, T_f = 3 (the third runs on the spectrum stacks sized by the first two): the window loop and
    the window-free native roll-out; UNO_P ends in the two-source GELU projection"""
    from uno_amd import harness

    def workload():
        torch.manual_seed(0)
        model = getattr(harness, name)(14, width).to(dev())
        opt = harness.ComplexAdam(model.parameters(), lr=1e-3, weight_decay=1e-3)
        xx, yy = torch.randn(2, 64, 64, 10, device=dev()), torch.randn(2, 64, 64, 3, device=dev())
        losses = []
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            loss = harness.ns2d_rollout_loss(model, xx, yy, 3, native=native)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        return losses + [p.detach().clone() for p in model.parameters()]
    _three_runs(monkeypatch, workload, MINIMA["ns2d", name, native], f"NS-2D steps {name} native={native}")


@pytest.mark.gpu
def test_ns2d_rollout_errors(monkeypatch):
    from uno_amd.harness import UNO, ns2d_rollout_errors

    def workload():
        torch.manual_seed(5)
        model = UNO(14, 4).to(dev())
        xx, yy = torch.randn(2, 64, 64, 10, device=dev()), torch.randn(2, 64, 64, 3, device=dev())
        r = ns2d_rollout_errors(model, xx, yy, 3, return_pred=True)
        return list(r.errors) + [r.pred]
    _three_runs(monkeypatch, workload, MINIMA["ns2d_errors"], "NS-2D evaluation roll-out")


@pytest.mark.gpu
def test_ns3d_training_steps(monkeypatch):
    """two NS-3D steps of Uno3D_T20 at 32 x 32 x 10 with the per-time-step error of each step's output"""
    from uno_amd.harness import ComplexAdam, Uno3D_T20, ns3d_loss

    def workload():
        torch.manual_seed(0)
        model = Uno3D_T20(6, 4, pad=3).to(dev())
        opt = ComplexAdam(model.parameters(), lr=1e-3, weight_decay=1e-3)
        x, y = torch.randn(2, 32, 32, 10, 1, device=dev()), torch.randn(2, 32, 32, 20, device=dev())
        out = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            loss, err = ns3d_loss(model, x, y, with_step_error=True)
            loss.backward()
            opt.step()
            out += [loss.detach(), err]
        return out + [p.detach().clone() for p in model.parameters()]
    _three_runs(monkeypatch, workload, MINIMA["ns3d"], "NS-3D steps")


@pytest.mark.gpu
def test_operator_block_3d_one_buffer_any_grid(monkeypatch):
    """a block opted into the one-buffer form on the any-grid kernels (as tests/test_hip_block3d_any.py opts in), (15, 15, 9) -> (7, 7, 6)"""
    from uno_amd.integral_operators import OperatorBlock_3D, enable_one_buffer_any_grid
    from uno_amd.spectral3d import _resample3d_plan
    din, dout = (15, 15, 9), (7, 7, 6)
    assert _resample3d_plan(din, dout, dev()) is None

    def workload():
        torch.manual_seed(17)
        blk = enable_one_buffer_any_grid(OperatorBlock_3D(4, 3, *dout, 3, 3, 3)).to(dev())
        x = torch.randn(2, 4, *din, device=dev(), requires_grad=True)
        y = blk(x, *dout)
        assert type(y.grad_fn).__name__ == "_OperatorBlock3dFnBackward"         # the one-buffer form ran, not the two branches
        y.square().sum().backward()
        return [y.detach(), x.grad] + _grads(blk)
    _three_runs(monkeypatch, workload, MINIMA["block3d_any"], "OperatorBlock_3D one buffer, any grid")


# poisoned allocations per workload, as counted on the MI355X when this file was written (each run of a workload gave the same count
# under both bytes); a workload that allocates less than this through the fixture has changed and must be looked at again
MINIMA = {
    ("block2d", (37, 37, 55, 55), False): 31, ("block2d", (37, 37, 55, 55), True): 43, ("block2d", (55, 55, 37, 37), False): 36,
    ("block2d", (55, 55, 37, 37), True): 47, ("block2d", (70, 66, 35, 33), False): 36, ("block2d", (70, 66, 35, 33), True): 47,
    "lift_window": 18, ("darcy", False): 176, ("darcy", True): 178,
    ("ns2d", "UNO", False): 837, ("ns2d", "UNO", True): 843, ("ns2d", "UNO_P", False): 846, "ns2d_errors": 127, "ns3d": 338, "block3d_any": 17,
}
