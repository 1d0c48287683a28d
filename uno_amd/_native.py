"""ctypes binding of libuno_spectral.so (C ABI: include/uno_spectral.h).

This is the host side of the drop-in boundary: plain pointers, sizes and a hipStream_t cross
it, nothing torch-typed.  There is NO fallback: if the library is missing or a call fails the
error is raised to the caller (RuntimeError, as the reference surfaces torch RuntimeErrors).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import threading
from typing import NamedTuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libuno_spectral.so")
ABI_VERSION = 14

_lib = None
_lock = threading.Lock()

_fp = C.c_void_p
_i = C.c_int
_SIGNATURES = {
    "uno_abi_version": (C.c_int, []),
    "uno_last_error": (C.c_char_p, []),
    "uno_dft2d_any_ws_bytes": (C.c_longlong, [_i] * 5),
    "uno_scratch_provide": (C.c_int, [_fp, C.c_longlong]),
    "uno_spectral_conv2d_fwd_ws_bytes": (C.c_longlong, [_i] * 5),
    "uno_spectral_conv2d_bwd_ws_bytes": (C.c_longlong, [_i] * 5),
    "uno_spectral_conv2d_forward": (C.c_int, [_fp] * 6 + [_i] * 9 + [_fp]),
    "uno_spectral_conv2d_backward": (C.c_int, [_fp] * 8 + [_i] * 9 + [_fp]),
    "uno_spectral_conv2d_forward_bf16": (C.c_int, [_fp] * 6 + [_i] * 9 + [_fp]),
    "uno_spectral_conv2d_backward_bf16": (C.c_int, [_fp] * 8 + [_i] * 9 + [_fp]),
    "uno_fft_resample3d_ws_bytes": (C.c_longlong, [_i] * 6),
    "uno_fft_resample3d": (C.c_int, [_fp] * 3 + [_i] * 8 + [_fp, _fp, _i, _fp, _fp, _i, C.c_float, _i, _i, _fp]),
    "uno_fft_resample3d_acc": (C.c_int, [_fp] * 4 + [_i] * 8 + [_fp, _fp, _i, _fp, _fp, _i, C.c_float, _i, _i, _fp]),
    "uno_fft_resample3d_any_ws_bytes": (C.c_longlong, [_i] * 6),
    "uno_fft_resample3d_any": (C.c_int, [_fp] * 3 + [_i] * 8 + [_fp, _fp, _i, _fp, _fp, _i, C.c_float, _i, _i, _fp]),
    "uno_fft_resample3d_any_acc": (C.c_int, [_fp] * 4 + [_i] * 8 + [_fp, _fp, _i, _fp, _fp, _i, C.c_float, _i, _i, _fp]),
    "uno_fft_resample3d_wide_ws_bytes": (C.c_longlong, [_i] * 6),
    "uno_fft_resample3d_wide": (C.c_int, [_fp] * 3 + [_i] * 8 + [_fp, _fp, _i, _fp, _fp, _i, C.c_float, _i, _i, _fp]),
    "uno_fft_resample3d_wide_acc": (C.c_int, [_fp] * 4 + [_i] * 8 + [_fp, _fp, _i, _fp, _fp, _i, C.c_float, _i, _i, _fp]),
    "uno_dft2d_forward": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float, _i, _i, _fp]),
    "uno_dft2d_forward_bf16": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float, _i, _i, _fp]),
    "uno_dft2d_inverse_bf16": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float, _i, _i, _fp]),
    "uno_dft2d_inverse": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float, _i, _i, _fp]),
    "uno_reserve_cus": (C.c_int, [_i]),
    "uno_sweep_alternation": (C.c_int, [_i]),
    "uno_dft2d_inverse_add_applies": (C.c_int, [_i] * 7),
    "uno_dft2d_forward_resample_applies": (C.c_int, [_i] * 8),
    "uno_dft2d_forward_resample": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float] + [_i] * 5 + [_fp, _i, _i, _fp, _fp, _i, _fp, _fp, _fp]),
    "uno_dft2d_inverse_add": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _fp, _fp]),
    "uno_dft2d_forward_grouped": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float] + [_i] * 5 + [_fp]),
    "uno_dft2d_inverse_grouped": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float] + [_i] * 5 + [_fp]),
    "uno_spectrum_crop": (C.c_int, [_fp, _fp] + [_i] * 11 + [_fp]),
    "uno_mode_mix": (C.c_int, [_fp, C.POINTER(_fp), _fp] + [_i] * 6 + [_fp]),
    "uno_mode_wgrad": (C.c_int, [_fp, _fp, C.POINTER(_fp)] + [_i] * 5 + [_fp]),
    "uno_mode_backward": (C.c_int, [_fp, _fp, C.POINTER(_fp), _fp, C.POINTER(_fp)] + [_i] * 6 + [_fp]),
    "uno_mode_gemm_plan": (C.c_int, [_i] * 8 + [C.POINTER(_i)]),
    "uno_mode_backward_plan": (C.c_int, [_i] * 6 + [C.POINTER(_i)]),
    "uno_spectral_conv3d_fwd_ws_bytes": (C.c_longlong, [_i] * 8),
    "uno_spectral_conv3d_bwd_ws_bytes": (C.c_longlong, [_i] * 8),
    "uno_spectral_conv3d_forward": (C.c_int, [_fp, C.POINTER(_fp), _fp, _fp, _fp] + [_i] * 12 + [_fp]),
    "uno_spectral_conv3d_backward": (C.c_int, [_fp, _fp, C.POINTER(_fp), _fp, C.POINTER(_fp), _fp] + [_i] * 12 + [_fp]),
    "uno_cdft_axis": (C.c_int, [_fp, _fp] + [_i] * 6 + [C.c_float, _i, _fp]),
    "uno_dft3d_ws_bytes": (C.c_longlong, [_i] * 4),
    "uno_dft3d_forward_grouped": (C.c_int, [_fp, _fp, _fp] + [_i] * 7 + [C.c_float] + [_i] * 4 + [_fp]),
    "uno_dft3d_inverse_grouped": (C.c_int, [_fp, _fp, _fp] + [_i] * 7 + [C.c_float] + [_i] * 4 + [_fp]),
    "uno_spectral_conv3d_forward2": (C.c_int, [_fp, _fp, _i, C.POINTER(_fp), _fp, _fp, _fp] + [_i] * 12 + [_fp]),
    "uno_spectral_conv3d_backward2": (C.c_int, [_fp, _fp, C.POINTER(_fp), _fp, _fp, _i, C.POINTER(_fp), _fp] + [_i] * 12 + [_fp]),
    "uno_resample2d": (C.c_int, [_fp, _fp, _fp] + [_i] * 5 + [_fp, _fp, _i, _fp, _fp, _i, _fp, _fp, _i, _i, _fp]),
    "uno_channel_mix": (C.c_int, [_fp, _fp, _fp, _fp, _i, _i, _i, C.c_longlong, _i, _i, _i, _fp, _fp]),
    "uno_channel_wgrad_ws_bytes": (C.c_longlong, [_i, _i, _i, C.c_longlong]),
    "uno_channel_wgrad": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, C.c_longlong, _i, _fp]),
    "uno_channel_mix2": (C.c_int, [_fp, _fp, _i, _fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, C.c_longlong, _i, _i, _i, _fp, _fp, _fp, _fp, _fp]),
    "uno_channel_wgrad2": (C.c_int, [_fp, _fp, _fp, _i, _fp, _fp, _fp, _i, _i, _i, C.c_longlong, _i, _i, _fp]),
    "uno_channel_mix2_win": (C.c_int, [_fp, _fp, _i, _fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _i, _i, _i, C.c_longlong, _i, _i, _i, _fp, _fp, _fp, _fp, _fp]),
    "uno_channel_mix_ws_bytes": (C.c_longlong, [_i, _i, C.c_longlong, _i]),
    "uno_clear_border": (C.c_int, [_fp, C.c_longlong, _i, _i, _i, _i, _fp]),
    "uno_channel_mix_act_padded": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _fp]),
    "uno_lift_forward": (C.c_int, [_fp] * 6 + [_i] * 8 + [_fp]),
    "uno_lift_bwd_ws_bytes": (C.c_longlong, [_i] * 6),
    "uno_lift_backward": (C.c_int, [_fp] * 11 + [_i] * 8 + [_fp]),
    "uno_lift_backward2": (C.c_int, [_fp] * 12 + [_i] * 8 + [_fp]),
    "uno_lift_backward_takes_second": (C.c_int, [_i] * 8),
    "uno_channel_mix_dgelu_padded": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _fp]),
    "uno_channel_wgrad2_win": (C.c_int, [_fp, _fp, _fp, _i, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, C.c_longlong, _i, _i, _fp]),
    "uno_gelu_project_backward_win": (C.c_int, [_fp] * 7 + [_i, _i, _i, _i, _i, C.c_longlong, _fp]),
    "uno_channel_wgrad_finish": (C.c_int, [_fp, _fp, _fp, _i, _i, C.c_longlong, _i, _fp]),
    "uno_mode_wgrad_acc": (C.c_int, [_fp, _fp, C.POINTER(_fp)] + [_i] * 6 + [_fp]),
    "uno_spectral_conv2d_backward_acc": (C.c_int, [_fp] * 8 + [_i] * 11 + [_fp]),
    "uno_upload_table": (C.c_void_p, [_fp, C.c_longlong]),
    "uno_project_backward_applies": (C.c_int, [_i] * 7 + [C.c_longlong]),
    "uno_project_backward_ws_bytes": (C.c_longlong, [_i, _i, _i, C.c_longlong]),
    "uno_project_backward": (C.c_int, [_fp, _fp, _i] + [_fp] * 11 + [_i] * 6 + [C.c_longlong, _i, _i, _fp]),
    "uno_gelu_project_forward": (C.c_int, [_fp, _fp, _fp, _fp, _i, _i, C.c_longlong, _fp]),
    "uno_gelu_project_bwd_ws_bytes": (C.c_longlong, [_i, _i, C.c_longlong]),
    "uno_gelu_project_backward": (C.c_int, [_fp] * 7 + [_i, _i, C.c_longlong, _fp]),
    "uno_gelu_project2_forward": (C.c_int, [_fp] * 5 + [_i, _i, _i, C.c_longlong, _i, _fp]),
    "uno_gelu_project2_bwd_ws_bytes": (C.c_longlong, [_i, _i, _i, C.c_longlong]),
    "uno_gelu_project2_backward": (C.c_int, [_fp] * 9 + [_i, _i, _i, C.c_longlong, _i, _fp]),
    "uno_rel_l2_steps_ws_bytes": (C.c_longlong, [_i, C.c_longlong, _i]),
    "uno_rel_l2_steps": (C.c_int, [_fp] * 6 + [_i, C.c_longlong, _i, _fp]),
    "uno_rel_l2_steps_backward": (C.c_int, [_fp] * 6 + [_i, C.c_longlong, _i, _fp]),
    "uno_rel_l2_ws_bytes": (C.c_longlong, [_i, C.c_longlong]),
    "uno_rel_l2_forward": (C.c_int, [_fp, C.c_longlong, C.c_longlong] * 2 + [_fp] * 4 + [_i, C.c_longlong, _fp]),
    "uno_rel_l2_backward": (C.c_int, [_fp, C.c_longlong, C.c_longlong] * 2 + [_fp, _fp, _i, C.c_float, _fp, _i, C.c_longlong, _fp]),
    "uno_shell_spectrum_ws_bytes": (C.c_longlong, [_i] * 5),
    "uno_shell_spectrum": (C.c_int, [_fp] + [C.c_longlong] * 4 + [_fp] + [C.c_longlong] * 4 + [_fp, _fp, _i, _i, _i, _i, _fp]),
    "uno_sobolev_ws_bytes": (C.c_longlong, [_i] * 4),
    "uno_sobolev_forward": (C.c_int, [_fp] + [C.c_longlong] * 4 + [_fp] + [C.c_longlong] * 4 + [_fp] * 6 + [_i] * 5 + [_fp]),
    "uno_sobolev_backward": (C.c_int, [_fp, _fp, _fp, _i, C.c_float, _i, _fp] + [C.c_longlong] * 4 + [_i] * 4 + [_fp]),
    "uno_rollout_ws_bytes": (C.c_longlong, [_i, C.c_longlong, _i]),
    "uno_rollout_advance": (C.c_int, [_fp] * 5 + [_i, _i, _i, C.c_longlong, _i, _i, _i, _fp]),
    "uno_rollout_finish": (C.c_int, [_fp] * 4 + [_i, C.c_longlong, _i, _fp]),
    "uno_rollout_lift": (C.c_int, [_fp] * 6 + [_i, _i, _i, _i, C.c_longlong, _i, _i, _fp]),
    "uno_rollout_lift_bwd_ws_bytes": (C.c_longlong, [_i, _i, _i, _i, C.c_longlong, _i]),
    "uno_rollout_lift_backward": (C.c_int, [_fp] * 11 + [_i, _i, _i, _i, C.c_longlong, _i, _i, _fp]),
    "uno_rollout_loss_seed": (C.c_int, [_fp] * 5 + [_i, C.c_longlong, _i, _fp]),
    "uno_gelu_pad": (C.c_int, [_fp, _fp, _fp] + [_i] * 6 + [_fp]),
    "uno_transpose_batched": (C.c_int, [_fp, _fp, _i, C.c_longlong, _i] + [C.c_longlong] * 4 + [_fp]),
    "uno_instnorm_forward": (C.c_int, [_fp] * 6 + [C.c_longlong, _i, C.c_longlong, C.c_float, _i, _fp]),
    "uno_instnorm_backward": (C.c_int, [_fp] * 9 + [C.c_longlong, _i, C.c_longlong, _i, _fp]),
    "uno_adam_step": (C.c_int, [_fp, _fp, _fp, _fp, C.c_longlong, _i] + [C.c_double] * 5 + [_i, _fp]),
    "uno_adam_step_multi": (C.c_int, [_i, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(C.c_longlong),
                                      C.POINTER(_i)] + [C.c_double] * 5 + [_i, _fp]),
    "uno_adam_step_multi_dev": (C.c_int, [_i, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(C.c_longlong),
                                          C.POINTER(_i)] + [C.c_double] * 5 + [_fp, _fp, _fp, _fp]),
    "uno_grad_norm_ws_bytes": (C.c_longlong, [_i, C.POINTER(C.c_longlong), C.POINTER(_i)]),
    "uno_grad_norm": (C.c_int, [_i, C.POINTER(_fp), C.POINTER(C.c_longlong), C.POINTER(_i), _fp, _i, _fp, C.c_longlong, _fp, _fp]),
    "uno_adam_step_multi_guarded": (C.c_int, [_i, C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(_fp), C.POINTER(C.c_longlong),
                                              C.POINTER(_i)] + [C.c_double] * 5 + [_fp, _fp, _fp, _fp, _i, _fp]),
    "uno_spectral_conv2d_forward_mixed": (C.c_int, [_fp] * 6 + [_i] * 9 + [_fp]),
    "uno_spectral_conv2d_backward_mixed": (C.c_int, [_fp] * 8 + [_i] * 9 + [_fp]),
    "uno_mode_mix_f16w": (C.c_int, [_fp, C.POINTER(_fp), _fp] + [_i] * 6 + [_fp]),
    "uno_dft2d_forward_grouped_bf16": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float] + [_i] * 5 + [_fp]),
    "uno_dft2d_inverse_grouped_bf16": (C.c_int, [_fp, _fp] + [_i] * 5 + [C.c_float] + [_i] * 5 + [_fp]),
    "uno_resample2d_bf16": (C.c_int, [_fp, _fp, _fp] + [_i] * 5 + [_fp, _fp, _i, _fp, _fp, _i, _fp, _fp, _i, _i, _fp]),
    "uno_channel_mix_bf16": (C.c_int, [_fp, _fp, _fp, _fp, _i, _i, _i, C.c_longlong, _i, _i, _i, _fp, _fp]),
    "uno_channel_wgrad_bf16": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, C.c_longlong, _i, _fp]),
    "uno_channel_mix2_bf16": (C.c_int, [_fp, _fp, _i, _fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, C.c_longlong, _i, _i, _i, _fp, _fp, _fp, _fp, _fp]),
    "uno_channel_wgrad2_bf16": (C.c_int, [_fp, _fp, _fp, _i, _fp, _fp, _fp, _i, _i, _i, C.c_longlong, _i, _i, _fp]),
    "uno_gelu_project_forward_bf16": (C.c_int, [_fp, _fp, _fp, _fp, _i, _i, C.c_longlong, _fp]),
    "uno_gelu_project_backward_bf16": (C.c_int, [_fp] * 7 + [_i, _i, C.c_longlong, _fp]),
    "uno_gelu_pad_bf16": (C.c_int, [_fp, _fp, _fp] + [_i] * 6 + [_fp]),
    "uno_instnorm_forward_bf16": (C.c_int, [_fp] * 6 + [C.c_longlong, _i, C.c_longlong, C.c_float, _i, _fp]),
    "uno_instnorm_backward_bf16": (C.c_int, [_fp] * 9 + [C.c_longlong, _i, C.c_longlong, _i, _fp]),
    "uno_channel_mix2_rows": (C.c_int, [_fp, _fp, _i, _fp, _fp, _fp] + [_i] * 7 + [C.c_longlong, _i, _fp]),
    "uno_channel_mix2_rows_grad": (C.c_int, [_fp, _fp, _i, _fp, _fp, _fp] + [_i] * 7 + [C.c_longlong, _fp]),
    "uno_channel_wgrad2_rows": (C.c_int, [_fp, _fp, _fp, _i, _fp, _fp, _fp] + [_i] * 7 + [C.c_longlong, _i, _i, _fp]),
    "uno_channel_mix_act_padded_rows": (C.c_int, [_fp] * 5 + [_i] * 8 + [_fp]),
    "uno_dgelu_rows": (C.c_int, [_fp, _fp, _fp, C.c_longlong, _i, _i, _i, _i, C.c_longlong, _fp]),
    "uno_ns2d_ws_bytes": (C.c_longlong, [_i, _i]),
    "uno_ns2d_forward": (C.c_int, [_fp, _fp, _fp, _i, _i, _fp]),
    "uno_ns2d_inverse": (C.c_int, [_fp, _fp, _fp, _i, _i, _fp]),
    "uno_ns2d_steps": (C.c_int, [_fp, _fp, _i, _fp, _i, _i, C.c_longlong, C.c_double, C.c_double, _fp]),
    "uno_darcy_ws_bytes": (C.c_longlong, [_i, _i]),
    "uno_darcy_table_pitch": (C.c_int, [_i]),
    "uno_darcy_transform": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp]),
    "uno_darcy_apply": (C.c_int, [_fp, _fp, _fp, _i, _i, _fp]),
    "uno_darcy_solve": (C.c_int, [_fp] * 7 + [_i, _i, C.c_double, _i, _i, _fp]),
    "uno_profile_begin": (C.c_int, [_i]),
    "uno_profile_end": (C.c_int, []),
    "uno_profile_get": (C.c_int, [_i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """Load (once) and return the native library; raises if it is not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"uno_amd: native library {LIB_PATH} is missing - build it with "
                        "`python -m uno_amd.build` (hipcc, gfx950); there is no CPU fallback")
                h = C.CDLL(LIB_PATH)
                for name, (res, args) in _SIGNATURES.items():
                    fn = getattr(h, name)
                    fn.restype = res
                    fn.argtypes = args
                if h.uno_abi_version() != ABI_VERSION:
                    raise RuntimeError(f"uno_amd: ABI mismatch, library {h.uno_abi_version()} != binding {ABI_VERSION}")
                _lib = h
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().uno_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def _ptr(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


def _opt(t):
    """pointer of an optional tensor (None: NULL)"""
    return _ptr(t) if t is not None else C.c_void_p(0)


def _count(lead) -> int:
    """product of the leading dimensions"""
    n = 1
    for d in lead:
        n *= d
    return n


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _scratch:
    """`bytes` of device scratch taken from torch's caching allocator (stream-ordered: the block is reused only by later work on this
    stream), registered for this thread (uno_scratch_provide) for the duration of the call and cleared afterwards; the library
    allocates nothing."""

    def __init__(self, device, nbytes):
        self.bytes, self.device, self.buf = nbytes, device, None

    def __enter__(self):
        if self.bytes > 0:
            self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
            _check(lib().uno_scratch_provide(_ptr(self.buf), self.bytes), "uno_scratch_provide")
        return self

    def __exit__(self, *exc):
        if self.bytes > 0:
            lib().uno_scratch_provide(None, 0)
        return False


class _any_mode_scratch(_scratch):
    """Scratch of the any-mode transforms (mode counts beyond the MFMA kernels' range: the reference's DEFAULT modes):
    `needs` = (n_img, H, W, m1, m2) of every transform the call may run; the largest requirement is taken."""

    def __init__(self, device, *needs):
        L = lib()
        _scratch.__init__(self, device, max((int(L.uno_dft2d_any_ws_bytes(*[int(v) for v in n])) for n in needs), default=0))


class _mix_scratch(_scratch):
    """Scratch of the wide channel-mix layers (uno_channel_mix_ws_bytes: the weights pre-split for the bf16 matrix pipe)."""

    def __init__(self, device, Ci, Co, P, bf16):
        _scratch.__init__(self, device, int(lib().uno_channel_mix_ws_bytes(int(Ci), int(Co), int(P), 1 if bf16 else 0)))


def _require(t: torch.Tensor, dtype, name: str, dense: bool = True):
    """a device tensor of `dtype`; dense=False: of any strides (the transposing copy reads channels-last views)"""
    if not t.is_cuda:
        raise RuntimeError(f"uno_amd: {name} must live on a HIP device (got {t.device})"
                           + ("; the spectral convolution runs only on the MI355X kernels" if dense else ""))
    if t.dtype != dtype:
        raise RuntimeError(f"uno_amd: {name} must be {dtype} (got {t.dtype})")
    if dense and not t.is_contiguous():
        raise RuntimeError(f"uno_amd: {name} must be contiguous")


def _entry(name: str, bf16: bool):
    """the float32 entry point `name`, or its bfloat16 twin `name`_bf16"""
    return getattr(lib(), name + "_bf16" if bf16 else name)


def _act_dtype(t, name):
    """f32, or bf16 for the mixed-precision entry points (activations bf16, everything else f32 / c64)."""
    bf16 = t.dtype == torch.bfloat16
    _require(t, torch.bfloat16 if bf16 else torch.float32, name)
    return bf16


def _weights_half(w1, w2, bf16):
    """True when the complex weights come as (..., 2) float16 (re, im) storage (mixed precision: bf16 activations only)."""
    if w1.dtype == torch.float16:
        if not bf16:
            raise RuntimeError("uno_amd: half-precision weight storage goes with bfloat16 activations")
        for w, name in ((w1, "weights1"), (w2, "weights2")):
            _require(w, torch.float16, name)
            if w.dim() != 5 or w.shape[-1] != 2:
                raise RuntimeError("uno_amd: half-precision weights are stored as (Ci, Co, m1, m2, 2) = (re, im)")
        return True
    _require(w1, torch.complex64, "weights1")
    _require(w2, torch.complex64, "weights2")
    return False


def _complex_grad_buffers(out, shape, n: int, device, accumulate: bool):
    """n fresh complex64 weight-gradient tensors of `shape`, or the given ones validated -> (list, accumulate: False for fresh ones)"""
    if out is None:
        return [torch.empty(shape, dtype=torch.complex64, device=device) for _ in range(n)], False
    gws = list(out)
    for t in gws:
        _require(t, torch.complex64, "weight-gradient buffer")
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("uno_amd: weight-gradient buffer has the wrong shape")
    return gws, accumulate


def _real_grad_buffers(out_w, out_b, Ci: int, Co: int, need_bias: bool, device, accumulate: bool):
    """fresh float32 gw (Co, Ci) / gb (Co) or None, or out_w / out_b validated -> (gw, gb, accumulate: False for fresh ones)"""
    if out_w is None:
        gw = torch.empty((Co, Ci), dtype=torch.float32, device=device)
        return gw, (torch.empty((Co,), dtype=torch.float32, device=device) if need_bias else None), False
    gw, gb = out_w, (out_b if need_bias else None)
    _require(gw, torch.float32, "weight-gradient buffer")
    if gw.numel() != Co * Ci or (need_bias and (gb is None or gb.numel() != Co)):
        raise RuntimeError("uno_amd: gradient buffers do not match the layer")
    if gb is not None:
        _require(gb, torch.float32, "bias-gradient buffer")
    return gw, gb, accumulate


def spectral_conv2d_forward(x, w1, w2, Ho: int, Wo: int, xt_out=None):
    """-> (y (B,Co,Ho,Wo) in x's dtype (f32 | bf16), xtrunc (B,Ci,2*m1,m2) c64).  xt_out: dense complex64 tensor of that shape to
    write the truncated input spectrum into (a slot of a layer's time stack) instead of a fresh one."""
    bf16 = _act_dtype(x, "x")
    wh = _weights_half(w1, w2, bf16)
    B, Ci, H, W = x.shape
    Ci2, Co, m1, m2 = w1.shape[:4]
    if Ci2 != Ci or tuple(w2.shape) != tuple(w1.shape):
        raise RuntimeError(f"uno_amd: weight shapes {tuple(w1.shape)} / {tuple(w2.shape)} do not match input channels {Ci}")
    L = lib()
    with torch.cuda.device(x.device):
        y = torch.empty((B, Co, Ho, Wo), dtype=x.dtype, device=x.device)
        if xt_out is None:
            xt = torch.empty((B, Ci, 2 * m1, m2), dtype=torch.complex64, device=x.device)
        else:
            xt = xt_out
            _require(xt, torch.complex64, "xtrunc buffer")
            if tuple(xt.shape) != (B, Ci, 2 * m1, m2):
                raise RuntimeError("uno_amd: xtrunc buffer has the wrong shape")
        ws = torch.empty(max(1, L.uno_spectral_conv2d_fwd_ws_bytes(B, Ci, Co, m1, m2)), dtype=torch.uint8, device=x.device)
        fn = L.uno_spectral_conv2d_forward_mixed if wh else _entry("uno_spectral_conv2d_forward", bf16)
        with _any_mode_scratch(x.device, (B * Ci, H, W, m1, m2), (B * Co, Ho, Wo, m1, m2)):
            rc = fn(_ptr(x), _ptr(w1), _ptr(w2), _ptr(y), _ptr(xt), _ptr(ws), B, Ci, Co, H, W, Ho, Wo, m1, m2, _stream(x))
    _check(rc, "uno_spectral_conv2d_forward")
    return y, xt


def spectral_conv2d_backward(gy, xt, w1, w2, H: int, W: int, need_gx=True, need_gw=True, gw_out=None, accumulate_gw=False):
    """-> (gx or None (gy's dtype: f32 | bf16), gw1 or None, gw2 or None (c64)).
    gw_out = (gw1, gw2): write (accumulate_gw: add) the weight gradients into these complex64 tensors instead of fresh ones."""
    bf16 = _act_dtype(gy, "grad_output")
    _require(xt, torch.complex64, "xtrunc")
    wh = _weights_half(w1, w2, bf16)
    B, Co, Ho, Wo = gy.shape
    Ci, Co2, m1, m2 = w1.shape[:4]
    if Co2 != Co:
        raise RuntimeError("uno_amd: grad_output channels do not match the weights")
    L = lib()
    with torch.cuda.device(gy.device):
        gx = torch.empty((B, Ci, H, W), dtype=gy.dtype, device=gy.device) if need_gx else None
        gw1, gw2, accumulate_gw = None, None, accumulate_gw and need_gw
        if need_gw:
            (gw1, gw2), accumulate_gw = _complex_grad_buffers(gw_out, (Ci, Co, m1, m2), 2, gy.device, accumulate_gw)
        ws = torch.empty(max(1, L.uno_spectral_conv2d_bwd_ws_bytes(B, Ci, Co, m1, m2)), dtype=torch.uint8, device=gy.device)
        with _any_mode_scratch(gy.device, (B * Co, Ho, Wo, m1, m2), (B * Ci, H, W, m1, m2)):
            rc = L.uno_spectral_conv2d_backward_acc(_ptr(gy), _ptr(xt), _ptr(w1), _ptr(w2), _opt(gx), _opt(gw1), _opt(gw2),
                                                    _ptr(ws), B, Ci, Co, H, W, Ho, Wo, m1, m2, 2 if wh else (1 if bf16 else 0),
                                                    1 if accumulate_gw else 0, _stream(gy))
    _check(rc, "uno_spectral_conv2d_backward")
    return gx, gw1, gw2


def _fft_resample3d(family: str, x, out_size, f1, f2, m3, scale, adjoint, out, act):
    """fft_resample3d / fft_resample3d_any / fft_resample3d_wide (family "" / "_any" / "_wide"): the kernel families take the same arguments"""
    name = "uno_fft_resample3d" + family
    _require(x, torch.float32, "x")
    *lead, D1, D2, D3 = x.shape
    M1, M2, M3 = (int(v) for v in out_size)
    n = _count(lead)
    for t in (*f1, *f2):
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError("uno_amd: frequency tables must be contiguous int32 device tensors")
    J1, J2 = f1[0].numel(), f2[0].numel()
    if family and (f1[1].numel() != J1 or f2[1].numel() != J2):       # the pruned-DFT entry point alone takes tables of its own per side
        raise RuntimeError("uno_amd: the forward and inverse frequency tables of an axis must have the same length")
    L = lib()
    with torch.cuda.device(x.device):
        ws = torch.empty(max(1, getattr(L, name + "_ws_bytes")(n, D1, M1, J1, J2, int(m3))), dtype=torch.uint8, device=x.device)
        if out is not None:
            _require(out, torch.float32, "out")
            if tuple(out.shape) != (*lead, M1, M2, M3) or not out.is_contiguous():
                raise RuntimeError(f"uno_amd: out must be a contiguous {(*lead, M1, M2, M3)} tensor")
            ya = torch.empty_like(out) if act else None
            fn, dst, res = getattr(L, name + "_acc"), (_ptr(out), _opt(ya)), ((out, ya) if act else out)
        else:
            res = torch.empty((*lead, M1, M2, M3), dtype=torch.float32, device=x.device)
            fn, dst = getattr(L, name), (_ptr(res),)
        rc = fn(_ptr(x), *dst, _ptr(ws), n, D1, D2, D3, M1, M2, M3, J1, _ptr(f1[0]), _ptr(f1[1]), J2, _ptr(f2[0]), _ptr(f2[1]),
                int(m3), float(scale), int(adjoint), int(not adjoint), _stream(x))
    _check(rc, name + ("_acc" if out is not None else ""))
    return res


def fft_resample3d(x, out_size, f1, f2, m3: int, scale: float, adjoint: bool, out=None, act=False):
    """x (..., D1, D2, D3) f32 -> (..., M1, M2, M3): pruned DFT with row frequencies f1[0] / f2[0] (int32 device tensors) along
    axes 1 / 2 and m3 half-spectrum bins, pruned inverse DFT with f1[1] / f2[1]; adjoint=True: Hermitian weights on the
    forward side instead of the inverse side (the transpose of the operator with sizes and tables swapped).
    out: ACCUMULATE into this (..., M1, M2, M3) tensor (returned); act: also return gelu(out) written in the same pass -> (out, act)."""
    return _fft_resample3d("", x, out_size, f1, f2, m3, scale, adjoint, out, act)


def fft_resample3d_any(x, out_size, f1, f2, m3: int, scale: float, adjoint: bool, out=None, act=False):
    """fft_resample3d on the any-grid kernels (uno_fft_resample3d_any / _acc): any number of kept rows, any 1 <= m3 <= n/2 + 1, axis
    lengths 2 ... 128.  Same tables, the same adjoint convention and the same `out` / `act`; the forward and inverse tables of an axis
    must have the same length."""
    return _fft_resample3d("_any", x, out_size, f1, f2, m3, scale, adjoint, out, act)


def fft_resample3d_wide(x, out_size, f1, f2, m3: int, scale: float, adjoint: bool, out=None, act=False):
    """fft_resample3d on the wide-axis kernels (uno_fft_resample3d_wide / _acc): the two leading axes of 2 ... 256, the last of 2 ... 64,
    any number of kept rows, any 1 <= m3 <= n/2 + 1; the long-axis sums run on the f32 MFMA.  Arguments as fft_resample3d_any."""
    return _fft_resample3d("_wide", x, out_size, f1, f2, m3, scale, adjoint, out, act)


def dft2d_forward(images, m1, m2, scale=1.0, hermitian_cols=False, mask_overlap=False, out=None, channel_offset=0):
    """images (..., H, W) f32 -> spectra (..., 2*m1, m2) c64.  With `out` (B, Ctot, 2*m1, m2) and images (B, C1, H, W) the
    spectra go to channels [channel_offset, channel_offset + C1) of `out`.  bf16 images: plain form only."""
    bf16 = _act_dtype(images, "images")
    *lead, H, W = images.shape
    n = _count(lead)
    if out is None:
        spec = torch.empty((*lead, 2 * m1, m2), dtype=torch.complex64, device=images.device)
        with torch.cuda.device(images.device):
            fn = _entry("uno_dft2d_forward", bf16)
            with _any_mode_scratch(images.device, (n, H, W, m1, m2)):
                rc = fn(_ptr(images), _ptr(spec), n, H, W, m1, m2, float(scale), int(hermitian_cols), int(mask_overlap), _stream(images))
        _check(rc, "uno_dft2d_forward")
        return spec
    _require(out, torch.complex64, "out")
    if images.dim() != 4 or out.dim() != 4 or out.shape[0] != images.shape[0] or tuple(out.shape[2:]) != (2 * m1, m2) \
            or channel_offset < 0 or channel_offset + images.shape[1] > out.shape[1]:
        raise RuntimeError("uno_amd: out must be (B, Ctot, 2*m1, m2) with room for the image channels at channel_offset")
    with torch.cuda.device(images.device):
        fn = _entry("uno_dft2d_forward_grouped", bf16)
        with _any_mode_scratch(images.device, (n, H, W, m1, m2)):
            rc = fn(_ptr(images), _ptr(out), n, H, W, m1, m2, float(scale), int(hermitian_cols),
                    int(mask_overlap), images.shape[1], out.shape[1], int(channel_offset), _stream(images))
    _check(rc, "uno_dft2d_forward_grouped")
    return out


def spectrum_crop(src, m1, m2, out=None, channels=None, channel_offset=0, out_channel_offset=0):
    """The truncation to (m1, m2) modes of spectra (..., 2*M1, M2) c64 truncated to (M1, M2) >= (m1, m2): a copy of the corner blocks
    (uno_spectrum_crop) -> (..., 2*m1, m2).  With `channels` = C1 and src (B, Ctot, 2*M1, M2) only the channels
    [channel_offset, channel_offset + C1) are taken -> (B, C1, 2*m1, m2); with `out` (B, Cout, 2*m1, m2) they go to its channels
    [out_channel_offset, out_channel_offset + C1)."""
    _require(src, torch.complex64, "src")
    *lead, R2, M2 = src.shape
    M1 = R2 // 2
    if R2 != 2 * M1 or not (1 <= m1 <= M1 and 1 <= m2 <= M2):
        raise RuntimeError(f"uno_amd: spectrum_crop of {tuple(src.shape)} to modes ({m1}, {m2}): need an even row count and 1 <= modes <= the source's")
    sg = ss = so = dg = ds = do = 0
    if channels is not None or out is not None:
        if src.dim() != 4:
            raise RuntimeError("uno_amd: spectrum_crop of a channel range needs src (B, Ctot, 2*M1, M2)")
        C1 = src.shape[1] - channel_offset if channels is None else int(channels)
        if channel_offset < 0 or C1 < 1 or channel_offset + C1 > src.shape[1]:
            raise RuntimeError("uno_amd: src must hold the requested channel range")
        lead = [src.shape[0], C1]
        sg, ss, so = C1, src.shape[1], int(channel_offset)
    if out is None:
        out = torch.empty((*lead, 2 * m1, m2), dtype=torch.complex64, device=src.device)
    else:
        _require(out, torch.complex64, "out")
        if out.dim() != 4 or out.shape[0] != lead[0] or tuple(out.shape[2:]) != (2 * m1, m2) or out_channel_offset < 0 \
                or out_channel_offset + lead[1] > out.shape[1] or out.device != src.device:
            raise RuntimeError("uno_amd: out must be (B, Cout, 2*m1, m2) with room for the channels at out_channel_offset")
        dg, ds, do = lead[1], out.shape[1], int(out_channel_offset)
    with torch.cuda.device(src.device):
        rc = lib().uno_spectrum_crop(_ptr(src), _ptr(out), _count(lead), M1, M2, int(m1), int(m2), sg, ss, so, dg, ds, do, _stream(src))
    _check(rc, "uno_spectrum_crop")
    return out


def reserve_cus(n: int) -> int:
    """Set aside n compute units for communication kernels running beside the library's (uno_reserve_cus); returns the previous value."""
    return int(lib().uno_reserve_cus(int(n)))


def sweep_alternation(enable: bool) -> bool:
    """Alternating sweep direction of consecutive launches (uno_sweep_alternation); returns the previous setting."""
    return bool(lib().uno_sweep_alternation(1 if enable else 0))


def sweep_direction(mode: str, mask: int = 255) -> int:
    """Direction of the sweep-taking launches of the families in `mask` (the SWEEP_* bits of csrc/uno_common.h; the others run front to
    back): "alternate" (the default: every other launch of a thread reversed), "forward" (every launch front to back) or "reversed"
    (every launch reversed, the per-thread counter untouched).  Returns the previous raw setting of uno_sweep_alternation, which
    lib().uno_sweep_alternation(value) restores."""
    if mode not in ("alternate", "forward", "reversed") or not 0 <= int(mask) <= 255:
        raise ValueError(f"uno_amd: sweep_direction({mode!r}, {mask!r}): mode is alternate | forward | reversed, mask 0 .. 255")
    value = {"alternate": int(mask), "forward": 0, "reversed": 256 | int(mask)}[mode]
    if value == 1:
        raise ValueError("uno_amd: sweep_direction('alternate', 1): the C entry point reads 1 as 'every family' (255)")
    return int(lib().uno_sweep_alternation(value))


def dft2d_inverse_add_applies(n_img, H, W, m1, m2, Hs, Ws) -> bool:
    """True where dft2d_inverse(..., addend=) runs the fused kernel (K3 + up-sampled addend, csrc/dft2d_inv_add_kernel.h)."""
    return bool(lib().uno_dft2d_inverse_add_applies(int(n_img), int(H), int(W), int(m1), int(m2), int(Hs), int(Ws)))


def dft2d_forward_resample_applies(n_img, H, W, m1, m2, Ho, Wo, KW) -> bool:
    """True where dft2d_forward_resample runs (K1 + down-sampled image, csrc/dft2d_fwd_fd_kernel.h)."""
    return bool(lib().uno_dft2d_forward_resample_applies(int(n_img), int(H), int(W), int(m1), int(m2), int(Ho), int(Wo), int(KW)))


def dft2d_forward_resample(images, m1, m2, Ho, Wo, tables, scale=1.0, hermitian_cols=False, mask_overlap=False, out=None, channel_offset=0):
    """dft2d_forward of float32 images (..., H, W) and, from the same read, their banded resampling to (..., Ho, Wo)
    (uno_dft2d_forward_resample; the caller checked dft2d_forward_resample_applies).  tables = (col_start, col_wt, row_tiles, row_op) of
    resample.fused_resample_tables; `out` / channel_offset: dft2d_forward's.  -> (spectra, resampled)."""
    _require(images, torch.float32, "images")
    col_start, col_wt, row_tiles, row_op = tables
    *lead, H, W = images.shape
    n = _count(lead)
    group = stride = 0
    if out is None:
        spec = torch.empty((*lead, 2 * m1, m2), dtype=torch.complex64, device=images.device)
    else:
        _require(out, torch.complex64, "out")
        if images.dim() != 4 or out.dim() != 4 or out.shape[0] != images.shape[0] or tuple(out.shape[2:]) != (2 * m1, m2) \
                or channel_offset < 0 or channel_offset + images.shape[1] > out.shape[1]:
            raise RuntimeError("uno_amd: out must be (B, Ctot, 2*m1, m2) with room for the image channels at channel_offset")
        spec, group, stride = out, images.shape[1], out.shape[1]
    res = torch.empty((*lead, Ho, Wo), dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        rc = lib().uno_dft2d_forward_resample(_ptr(images), _ptr(spec), n, H, W, m1, m2, float(scale), int(hermitian_cols), int(mask_overlap),
                                              int(group), int(stride), int(channel_offset), _ptr(res), int(Ho), int(Wo), _ptr(col_start),
                                              _ptr(col_wt), int(col_wt.shape[1]), _ptr(row_tiles), _ptr(row_op), _stream(images))
    _check(rc, "uno_dft2d_forward_resample")
    return spec, res


def dft2d_inverse(spec, H, W, scale=1.0, hermitian_cols=True, mask_overlap=True, channels=None, channel_offset=0,
                  dtype=torch.float32, addend=None):
    """spectra (..., 2*m1, m2) c64 -> images (..., H, W) f32 (or bf16 with dtype=torch.bfloat16, plain form only).  With `channels` = C1 and spec (B, Ctot, 2*m1, m2) only the
    channels [channel_offset, channel_offset + C1) are transformed -> (B, C1, H, W).
    addend = (t (..., Hs, Ws) f32, (tile_p0, row_op, col_v0, col_op)): images += the banded up-sampling of t, in the same pass
    (uno_dft2d_inverse_add; the caller checked dft2d_inverse_add_applies)."""
    _require(spec, torch.complex64, "spec")
    *lead, r2, m2 = spec.shape
    m1 = r2 // 2
    if addend is not None:
        t, (p0, rowop, v0, colop) = addend
        _require(t, torch.float32, "addend")
        if channels is not None or dtype != torch.float32 or tuple(t.shape[:-2]) != tuple(lead):
            raise RuntimeError("uno_amd: dft2d_inverse(addend=) takes the plain float32 form with one addend image per spectrum")
        n = _count(lead)
        img = torch.empty((*lead, H, W), dtype=torch.float32, device=spec.device)
        with torch.cuda.device(spec.device):
            rc = lib().uno_dft2d_inverse_add(_ptr(spec), _ptr(img), n, H, W, m1, m2, float(scale), int(hermitian_cols), int(mask_overlap),
                                             _ptr(t), t.shape[-2], t.shape[-1], _ptr(p0), _ptr(rowop), _ptr(v0), _ptr(colop), _stream(spec))
        _check(rc, "uno_dft2d_inverse_add")
        return img
    if channels is None:
        n = _count(lead)
        if dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("uno_amd: images are float32 or bfloat16")
        img = torch.empty((*lead, H, W), dtype=dtype, device=spec.device)
        with torch.cuda.device(spec.device):
            fn = _entry("uno_dft2d_inverse", dtype == torch.bfloat16)
            with _any_mode_scratch(spec.device, (n, H, W, m1, m2)):
                rc = fn(_ptr(spec), _ptr(img), n, H, W, m1, m2, float(scale), int(hermitian_cols), int(mask_overlap), _stream(spec))
        _check(rc, "uno_dft2d_inverse")
        return img
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("uno_amd: images are float32 or bfloat16")
    if spec.dim() != 4 or channel_offset < 0 or channels < 1 or channel_offset + channels > spec.shape[1]:
        raise RuntimeError("uno_amd: spec must be (B, Ctot, 2*m1, m2) holding the requested channel range")
    B = spec.shape[0]
    img = torch.empty((B, channels, H, W), dtype=dtype, device=spec.device)
    with torch.cuda.device(spec.device):
        fn = _entry("uno_dft2d_inverse_grouped", dtype == torch.bfloat16)
        with _any_mode_scratch(spec.device, (B * channels, H, W, m1, m2)):
            rc = fn(_ptr(spec), _ptr(img), B * channels, H, W, m1, m2, float(scale), int(hermitian_cols),
                    int(mask_overlap), int(channels), spec.shape[1], int(channel_offset), _stream(spec))
    _check(rc, "uno_dft2d_inverse_grouped")
    return img


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def mode_mix(inp, weights, op: int):
    """inp (B, Cin, ncorner, modes) c64; weights: list of (Ci, Co, modes...) c64."""
    _require(inp, torch.complex64, "spectrum")
    half = weights[0].dtype == torch.float16
    for w in weights:
        _require(w, torch.float16 if half else torch.complex64, "weights")
    B = inp.shape[0]
    Ci, Co = weights[0].shape[:2]
    nc = len(weights)
    Mc = weights[0][0, 0].numel() // (2 if half else 1)
    cout = Co if op == 0 else Ci
    out = torch.empty((B, cout, *inp.shape[2:]), dtype=torch.complex64, device=inp.device)
    with torch.cuda.device(inp.device):
        fn = lib().uno_mode_mix_f16w if half else lib().uno_mode_mix
        rc = fn(_ptr(inp), _ptr_array(weights), _ptr(out), op, B, Ci, Co, nc, Mc, _stream(inp))
    _check(rc, "uno_mode_mix")
    return out


def mode_wgrad(xt, go, weight_shape, ncorner: int, out=None, accumulate: bool = False):
    """out: list of `ncorner` complex64 tensors of `weight_shape` to write (accumulate: add) the gradients into."""
    _require(xt, torch.complex64, "xtrunc")
    _require(go, torch.complex64, "grad spectrum")
    B, Ci = xt.shape[:2]
    Co = go.shape[1]
    gws, accumulate = _complex_grad_buffers(out, weight_shape, ncorner, xt.device, accumulate)
    Mc = gws[0][0, 0].numel()
    with torch.cuda.device(xt.device):
        rc = lib().uno_mode_wgrad_acc(_ptr(xt), _ptr(go), _ptr_array(gws), B, Ci, Co, ncorner, Mc, 1 if accumulate else 0, _stream(xt))
    _check(rc, "uno_mode_wgrad")
    return gws


def mode_backward(xt, go, weights, out=None, accumulate: bool = False):
    """Both per-mode GEMMs of a backward pass in one launch (uno_mode_backward): xt (B, Ci, ncorner, modes) and go (B, Co, ncorner, modes)
    c64 (any trailing shape with ncorner * modes entries per channel), weights: list of ncorner (Ci, Co, modes...) c64
    -> (gX (B, Ci, ncorner * modes) c64, [gw per corner]); out / accumulate as in mode_wgrad."""
    _require(xt, torch.complex64, "xtrunc")
    _require(go, torch.complex64, "grad spectrum")
    for w in weights:
        _require(w, torch.complex64, "weights")
    B, Ci = xt.shape[:2]
    Co = go.shape[1]
    nc = len(weights)
    Mc = weights[0][0, 0].numel()
    gws, accumulate = _complex_grad_buffers(out, weights[0].shape, nc, xt.device, accumulate)
    gX = torch.empty((B, Ci, nc * Mc), dtype=torch.complex64, device=xt.device)
    with torch.cuda.device(xt.device):
        rc = lib().uno_mode_backward(_ptr(xt), _ptr(go), _ptr_array(list(weights)), _ptr(gX), _ptr_array(gws), B, Ci, Co, nc, Mc,
                                     1 if accumulate else 0, _stream(xt))
    _check(rc, "uno_mode_backward")
    return gX, gws


MODE_GEMM_PLAN_INTS, MODE_BACKWARD_PLAN_INTS = 16, 36          # UNO_MODE_GEMM_PLAN_INTS, UNO_MODE_BACKWARD_PLAN_INTS
_MODE_GEMM_VARIANTS = ("4, 4, 2", "4, 2, 4", "2, 4, 4")


class ModeGemmPlan(NamedTuple):
    """What one per-mode GEMM launches (uno_mode_gemm_plan; the fields in the order of its int array, include/uno_spectral.h)."""
    family: int         # 0: nothing to launch, 1: LDS-staged mode_gemm_kernel, 2: 4x4x1 mode_gemm_blocks_kernel
    M: int
    N: int
    K: int
    qc: int
    pipe: int
    variant: int
    KS: int
    adjacent: int
    refused: int        # bit 0: padded, bit 1: huge_out
    half: int
    acc: int
    grid_x: int
    grid_y: int
    grid_z: int
    lds: int

    @property
    def kernel(self):
        """the kernel's name as the launch records (profile_end) and rocprofv3 print it; None when nothing is launched"""
        flags = "{}, {}".format("true" if self.half else "false", "true" if self.acc else "false")
        if self.family == 1:
            return "uno::mode_gemm_kernel<{}, {}, {}>".format(self.qc, "true" if self.pipe else "false", flags)
        if self.family == 2:
            return "uno::mode_gemm_blocks_kernel<{}, {}>".format(_MODE_GEMM_VARIANTS[self.variant], flags)
        return None


class ModeBackwardPlan(NamedTuple):
    """What uno_mode_backward launches (uno_mode_backward_plan): one pair launch, or role b's kernel and then role a's."""
    paired: int
    Ga: int
    grid: int
    lds: int
    a: ModeGemmPlan     # the input gradient (op 1)
    b: ModeGemmPlan     # the weight gradient (op 2)

    @property
    def kernels(self):
        """the kernel names in launch order"""
        if self.paired:
            return ["uno::mode_gemm_blocks_pair_kernel<{}, {}>".format(_MODE_GEMM_VARIANTS[self.a.variant], "true" if self.b.acc else "false")]
        return [k for k in (self.b.kernel, self.a.kernel) if k is not None]


def mode_gemm_plan(op: int, B: int, Ci: int, Co: int, ncorner: int, modes_per_corner: int, w_half: bool = False,
                   accumulate: bool = False) -> ModeGemmPlan:
    """The launch decision of mode_mix (op 0 / 1) / mode_wgrad (op 2) for these sizes, from the library's own plan function; no device
    is touched.  Raises what the real call raises for bad sizes."""
    buf = (C.c_int * MODE_GEMM_PLAN_INTS)()
    rc = lib().uno_mode_gemm_plan(op, B, Ci, Co, ncorner, modes_per_corner, 1 if w_half else 0, 1 if accumulate else 0, buf)
    _check(rc, "uno_mode_gemm_plan")
    return ModeGemmPlan(*buf)


def mode_backward_plan(B: int, Ci: int, Co: int, ncorner: int, modes_per_corner: int, accumulate: bool = False) -> ModeBackwardPlan:
    """The launch decision of mode_backward for these sizes (uno_mode_backward_plan); no device is touched."""
    buf = (C.c_int * MODE_BACKWARD_PLAN_INTS)()
    rc = lib().uno_mode_backward_plan(B, Ci, Co, ncorner, modes_per_corner, 1 if accumulate else 0, buf)
    _check(rc, "uno_mode_backward_plan")
    v = list(buf)
    return ModeBackwardPlan(*v[:4], ModeGemmPlan(*v[4:4 + MODE_GEMM_PLAN_INTS]), ModeGemmPlan(*v[4 + MODE_GEMM_PLAN_INTS:]))


def spectral_conv3d_forward(x, ws_, Ho: int, Wo: int, To: int):
    """x (B,Ci,H,W,T) f32, ws_ = [weights1..4] (Ci,Co,m1,m2,m3) c64 -> (y, xtrunc (B,Ci,4,m1,m2,m3) c64)."""
    _require(x, torch.float32, "x")
    if len(ws_) != 4:
        raise RuntimeError("uno_amd: the 3-D spectral convolution takes four weight tensors")
    for w in ws_:
        _require(w, torch.complex64, "weights")
        if tuple(w.shape) != tuple(ws_[0].shape):
            raise RuntimeError("uno_amd: weights1..4 must have one shape")
    B, Ci, H, W, T = x.shape
    Ci2, Co, m1, m2, m3 = ws_[0].shape
    if Ci2 != Ci:
        raise RuntimeError(f"uno_amd: weight shape {tuple(ws_[0].shape)} does not match input channels {Ci}")
    L = lib()
    with torch.cuda.device(x.device):
        y = torch.empty((B, Co, Ho, Wo, To), dtype=torch.float32, device=x.device)
        xt = torch.empty((B, Ci, 4, m1, m2, m3), dtype=torch.complex64, device=x.device)
        scratch = torch.empty(max(1, L.uno_spectral_conv3d_fwd_ws_bytes(B, Ci, Co, H, Ho, m1, m2, m3)), dtype=torch.uint8,
                              device=x.device)
        # (the (W, T) planes go through the 2-D transforms with modes (m2, m3): beyond the MFMA range they take the any-mode form)
        with _any_mode_scratch(x.device, (B * Ci * H, W, T, m2, m3), (B * Co * Ho, Wo, To, m2, m3)):
            rc = L.uno_spectral_conv3d_forward(_ptr(x), _ptr_array(ws_), _ptr(y), _ptr(xt), _ptr(scratch), B, Ci, Co,
                                               H, W, T, Ho, Wo, To, m1, m2, m3, _stream(x))
    _check(rc, "uno_spectral_conv3d_forward")
    return y, xt


def spectral_conv3d_backward(gy, xt, ws_, H: int, W: int, T: int, need_gx=True, need_gw=True):
    _require(gy, torch.float32, "grad_output")
    _require(xt, torch.complex64, "xtrunc")
    for w in ws_:
        _require(w, torch.complex64, "weights")
    B, Co, Ho, Wo, To = gy.shape
    Ci, Co2, m1, m2, m3 = ws_[0].shape
    if Co2 != Co:
        raise RuntimeError("uno_amd: grad_output channels do not match the weights")
    L = lib()
    with torch.cuda.device(gy.device):
        gx = torch.empty((B, Ci, H, W, T), dtype=torch.float32, device=gy.device) if need_gx else None
        gws = [torch.empty_like(w) for w in ws_] if need_gw else None
        scratch = torch.empty(max(1, L.uno_spectral_conv3d_bwd_ws_bytes(B, Ci, Co, H, Ho, m1, m2, m3)), dtype=torch.uint8,
                              device=gy.device)
        with _any_mode_scratch(gy.device, (B * Co * Ho, Wo, To, m2, m3), (B * Ci * H, W, T, m2, m3)):
            rc = L.uno_spectral_conv3d_backward(_ptr(gy), _ptr(xt), _ptr_array(ws_), _opt(gx),
                                                _ptr_array(gws) if need_gw else None, _ptr(scratch), B, Ci, Co,
                                                H, W, T, Ho, Wo, To, m1, m2, m3, _stream(gy))
    _check(rc, "uno_spectral_conv3d_backward")
    return gx, gws


def spectral_conv3d_forward2(x1, x2, ws_, Ho: int, Wo: int, To: int):
    """spectral_conv3d_forward on the channel concatenation of x1 (B,C1,H,W,T) and x2 (B,C2,H,W,T), which is not built
    -> (y, xtrunc (B,C1+C2,4,m1,m2,m3) c64)."""
    _require(x1, torch.float32, "x1")
    _require(x2, torch.float32, "x2")
    if x1.device != x2.device or x1.shape[0] != x2.shape[0] or x1.shape[2:] != x2.shape[2:]:
        raise RuntimeError(f"uno_amd: the two sources {tuple(x1.shape)} and {tuple(x2.shape)} must share device, batch and grid")
    if len(ws_) != 4:
        raise RuntimeError("uno_amd: the 3-D spectral convolution takes four weight tensors")
    for w in ws_:
        _require(w, torch.complex64, "weights")
        if tuple(w.shape) != tuple(ws_[0].shape):
            raise RuntimeError("uno_amd: weights1..4 must have one shape")
    B, C1, H, W, T = x1.shape
    Ci = C1 + x2.shape[1]
    Ci2, Co, m1, m2, m3 = ws_[0].shape
    if Ci2 != Ci:
        raise RuntimeError(f"uno_amd: weight shape {tuple(ws_[0].shape)} does not match input channels {C1} + {x2.shape[1]}")
    L = lib()
    with torch.cuda.device(x1.device):
        y = torch.empty((B, Co, Ho, Wo, To), dtype=torch.float32, device=x1.device)
        xt = torch.empty((B, Ci, 4, m1, m2, m3), dtype=torch.complex64, device=x1.device)
        scratch = torch.empty(max(1, L.uno_spectral_conv3d_fwd_ws_bytes(B, Ci, Co, H, Ho, m1, m2, m3)), dtype=torch.uint8,
                              device=x1.device)
        with _any_mode_scratch(x1.device, (B * max(C1, Ci - C1) * H, W, T, m2, m3), (B * Co * Ho, Wo, To, m2, m3)):
            rc = L.uno_spectral_conv3d_forward2(_ptr(x1), _ptr(x2), C1, _ptr_array(ws_), _ptr(y), _ptr(xt), _ptr(scratch), B, Ci, Co,
                                                H, W, T, Ho, Wo, To, m1, m2, m3, _stream(x1))
    _check(rc, "uno_spectral_conv3d_forward2")
    return y, xt


def spectral_conv3d_backward2(gy, xt, ws_, C1: int, H: int, W: int, T: int, need_gx=True, need_gw=True):
    """-> (gx1 (B,C1,H,W,T), gx2 (B,Ci-C1,H,W,T), [gw1..4]); need_gx=False: (None, None, ...)."""
    _require(gy, torch.float32, "grad_output")
    _require(xt, torch.complex64, "xtrunc")
    for w in ws_:
        _require(w, torch.complex64, "weights")
    B, Co, Ho, Wo, To = gy.shape
    Ci, Co2, m1, m2, m3 = ws_[0].shape
    if Co2 != Co:
        raise RuntimeError("uno_amd: grad_output channels do not match the weights")
    if not 0 < C1 < Ci:
        raise RuntimeError(f"uno_amd: the first source's channel count {C1} must lie inside (0, {Ci})")
    L = lib()
    with torch.cuda.device(gy.device):
        gx1 = torch.empty((B, C1, H, W, T), dtype=torch.float32, device=gy.device) if need_gx else None
        gx2 = torch.empty((B, Ci - C1, H, W, T), dtype=torch.float32, device=gy.device) if need_gx else None
        gws = [torch.empty_like(w) for w in ws_] if need_gw else None
        scratch = torch.empty(max(1, L.uno_spectral_conv3d_bwd_ws_bytes(B, Ci, Co, H, Ho, m1, m2, m3)), dtype=torch.uint8,
                              device=gy.device)
        with _any_mode_scratch(gy.device, (B * Co * Ho, Wo, To, m2, m3), (B * max(C1, Ci - C1) * H, W, T, m2, m3)):
            rc = L.uno_spectral_conv3d_backward2(_ptr(gy), _ptr(xt), _ptr_array(ws_), _opt(gx1), _opt(gx2), C1,
                                                 _ptr_array(gws) if need_gw else None, _ptr(scratch), B, Ci, Co,
                                                 H, W, T, Ho, Wo, To, m1, m2, m3, _stream(gy))
    _check(rc, "uno_spectral_conv3d_backward2")
    return gx1, gx2, gws


def _grouping3d(n_vol: int, group: int, spec, who: str):
    """(group, stride) to hand to a 3-D stage call on spec (B, stride, 4, m1, m2, m3); group <= 0: plain, (0, 0)"""
    if spec.dim() != 6 or spec.shape[2] != 4:
        raise RuntimeError(f"uno_amd: {who}: the spectrum tensor must be (batch, channels, 4, m1, m2, m3), got {tuple(spec.shape)}")
    if group <= 0:
        if spec.shape[0] * spec.shape[1] != n_vol:
            raise RuntimeError(f"uno_amd: {who}: {n_vol} volumes against {spec.shape[0] * spec.shape[1]} spectra")
        return 0, 0
    if n_vol % group or n_vol // group != spec.shape[0]:
        raise RuntimeError(f"uno_amd: {who}: {n_vol} volumes in groups of {group} against a spectrum batch of {spec.shape[0]}")
    return group, spec.shape[1]


def dft3d_forward(x, modes=None, scale: float = 1.0, adjoint: bool = False, out=None, group: int = 0, offset: int = 0):
    """uno_dft3d_forward_grouped: x (..., D1, D2, D3) f32 -> truncated corner-major spectra.  Plain (group = 0): a fresh
    (*lead, 4, m1, m2, m3) c64 tensor for modes = (m1, m2, m3).  Grouped: x (B, group, D1, D2, D3) is written into channels
    [offset, offset + group) of out (B, stride, 4, m1, m2, m3) c64, the rest of which is left untouched; returns out."""
    _require(x, torch.float32, "x")
    *lead, D1, D2, D3 = x.shape
    n_vol = _count(lead)
    if out is None:
        m1, m2, m3 = modes
        out = torch.empty((n_vol, 1, 4, m1, m2, m3), dtype=torch.complex64, device=x.device)
        result = out.view(*lead, 4, m1, m2, m3)
    else:
        _require(out, torch.complex64, "spectrum")
        result = out
    m1, m2, m3 = out.shape[3:]
    group, stride = _grouping3d(n_vol, group, out, "dft3d_forward")
    L = lib()
    with torch.cuda.device(x.device):
        scratch = torch.empty(max(1, L.uno_dft3d_ws_bytes(n_vol, D1, m2, m3)), dtype=torch.uint8, device=x.device)
        with _any_mode_scratch(x.device, (n_vol * D1, D2, D3, m2, m3)):
            rc = L.uno_dft3d_forward_grouped(_ptr(x), _ptr(out), _ptr(scratch), n_vol, D1, D2, D3, m1, m2, m3, float(scale),
                                             1 if adjoint else 0, group, stride, offset, _stream(x))
    _check(rc, "uno_dft3d_forward_grouped")
    return result


def dft3d_inverse(spec, dims, scale: float = 1.0, weighted: bool = False, group: int = 0, offset: int = 0):
    """uno_dft3d_inverse_grouped: spec (B, C, 4, m1, m2, m3) c64 -> volumes (B, C, D1, D2, D3) f32 (plain), or - grouped - the
    volumes (B, group, D1, D2, D3) of channels [offset, offset + group) of spec, which is read where it lies."""
    _require(spec, torch.complex64, "spectrum")
    D1, D2, D3 = (int(d) for d in dims)
    B, C = spec.shape[:2]
    m1, m2, m3 = spec.shape[3:]
    n_vol = B * (group if group > 0 else C)
    group, stride = _grouping3d(n_vol, group, spec, "dft3d_inverse")
    L = lib()
    with torch.cuda.device(spec.device):
        y = torch.empty((B, n_vol // B if B else 0, D1, D2, D3), dtype=torch.float32, device=spec.device)
        scratch = torch.empty(max(1, L.uno_dft3d_ws_bytes(n_vol, D1, m2, m3)), dtype=torch.uint8, device=spec.device)
        with _any_mode_scratch(spec.device, (n_vol * D1, D2, D3, m2, m3)):
            rc = L.uno_dft3d_inverse_grouped(_ptr(spec), _ptr(y), _ptr(scratch), n_vol, D1, D2, D3, m1, m2, m3, float(scale),
                                             1 if weighted else 0, group, stride, offset, _stream(spec))
    _check(rc, "uno_dft3d_inverse_grouped")
    return y


def resample2d(x, Ho: int, Wo: int, tabH, tabW, tilesH=None, out=None):
    """x (..., H, W) f32 -> (..., Ho, Wo); tabX = (start int32 [out], weights f32 [out, K]) band tables on x.device;
    tilesH = (p0 int32 [ntiles], dense weights f32 [ntiles, NP, 16]) enables the fused single-pass kernel.
    out: accumulate into this (..., Ho, Wo) tensor instead of allocating the result."""
    bf16 = _act_dtype(x, "x")
    *lead, H, W = x.shape
    n = _count(lead)
    sH, wH = tabH
    sW, wW = tabW
    accumulate = out is not None
    if accumulate:
        _require(out, x.dtype, "out")
        if tuple(out.shape) != (*lead, Ho, Wo):
            raise RuntimeError(f"uno_amd: out has shape {tuple(out.shape)}, expected {(*lead, Ho, Wo)}")
    else:
        out = torch.empty((*lead, Ho, Wo), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        tmp = torch.empty(max(1, n * min(Ho * W, H * Wo)), dtype=torch.float32, device=x.device)
        if tilesH is not None:
            tp0, tw = tilesH
            targs = (_ptr(tp0), _ptr(tw), tw.shape[1])
        else:
            targs = (C.c_void_p(0), C.c_void_p(0), 0)
        fn = _entry("uno_resample2d", bf16)
        rc = fn(_ptr(x), _ptr(out), _ptr(tmp), n, H, W, Ho, Wo, _ptr(sH), _ptr(wH), wH.shape[1],
                _ptr(sW), _ptr(wW), wW.shape[1], *targs, 1 if accumulate else 0, _stream(x))
    _check(rc, "uno_resample2d")
    return out


def _window_fits(rows: int, cols: int, pitch: int, plane: int) -> bool:
    """the window rule of the _win entry points (uno_spectral.h, ABI 10)"""
    return not (rows < 1 or cols % 4 or cols < 260 or pitch < cols or (rows - 1) * pitch + cols > plane or rows * cols >= 1 << 24)


def _window_args(window, plane: int, bf16: bool):
    """(rows, cols, pitch) of a windowed call: the tensors' last axis is a whole plane of `plane` elements."""
    rows, cols, pitch = (int(v) for v in window)
    if bf16:
        raise RuntimeError("uno_amd: pixel windows are float32 only")
    if not _window_fits(rows, cols, pitch, plane):
        raise RuntimeError(f"uno_amd: window rows={rows} cols={cols} pitch={pitch} does not fit a plane of {plane} elements "
                           "(cols: a multiple of 4, 260 <= cols <= pitch; rows * cols < 2^24)")
    return rows, cols, pitch


def channel_mix(x, w, bias=None, transpose_w: bool = False, out=None, act_in: bool = False, dgelu_of=None, dgelu_total: bool = False,
                window=None):
    """x (B, Ci, P) f32, w (Co, Ci) (or (Ci, Co) with transpose_w) -> y (B, Co, P) = Wm x + bias;
    out: accumulate into this (B, Co, P) tensor instead; act_in: x := gelu(x) as it is read; dgelu_of (B, Co, P): the
    product is multiplied by gelu'(dgelu_of) - with dgelu_total (and out) the completed sum out + product is.
    window = (rows, cols, pitch): the call works on that window of planes of P elements (see channel_mix2)."""
    if window is not None:
        return channel_mix2(x, None, w, bias, transpose_w=transpose_w, out=out, act_in=act_in, dgelu_of=dgelu_of,
                            accumulate=(2 if (dgelu_total and dgelu_of is not None) else 1) if out is not None else 0, window=window)
    bf16 = _act_dtype(x, "x")
    _require(w, torch.float32, "weight")
    if bias is not None:
        _require(bias, torch.float32, "bias")
    B, Ci, P = x.shape
    Co = w.shape[1] if transpose_w else w.shape[0]
    if (w.shape[0] if transpose_w else w.shape[1]) != Ci:
        raise RuntimeError(f"uno_amd: weight {tuple(w.shape)} does not match {Ci} input channels")
    accumulate = out is not None
    if accumulate:
        _require(out, x.dtype, "out")
        if tuple(out.shape) != (B, Co, P):
            raise RuntimeError(f"uno_amd: out has shape {tuple(out.shape)}, expected {(B, Co, P)}")
        y = out
    else:
        y = torch.empty((B, Co, P), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _mix_scratch(x.device, Ci, Co, P, bf16):
        if dgelu_of is not None:
            _require(dgelu_of, x.dtype, "dgelu_of")
            if tuple(dgelu_of.shape) != (B, Co, P):
                raise RuntimeError(f"uno_amd: dgelu_of has shape {tuple(dgelu_of.shape)}, expected {(B, Co, P)}")
        rc = _entry("uno_channel_mix", bf16)(_ptr(x), _ptr(w), _opt(bias), _ptr(y), B, Ci, Co, P, 1 if transpose_w else 0,
                                             (2 if (dgelu_total and dgelu_of is not None) else 1) if accumulate else 0,
                                             1 if act_in else 0, _opt(dgelu_of), _stream(x))
    _check(rc, "uno_channel_mix")
    return y


def clear_border(t, rows: int, cols: int):
    """t (..., Hp, Wp) float32 contiguous: everything outside t[..., :rows, :cols] := 0, in place (-> t)."""
    _require(t, torch.float32, "tensor")
    Hp, Wp = t.shape[-2:]
    n = t.numel() // max(1, Hp * Wp)
    with torch.cuda.device(t.device):
        rc = lib().uno_clear_border(_ptr(t), n, Hp, Wp, int(rows), int(cols), _stream(t))
    _check(rc, "uno_clear_border")
    return t


def channel_mix_act_padded_ok(x, Hp: int, Wp: int) -> bool:
    """shape rules of uno_channel_mix_act_padded for x (B, Ci, H, W)"""
    H, W = x.shape[-2:]
    return x.dtype == torch.float32 and 260 <= W <= Wp and H <= Hp and H * W < (1 << 24)


def channel_mix_act_padded(x, w, bias, Hp: int, Wp: int, act_in: bool = False, keep_y: bool = True):
    """x (B, Ci, H, W) f32, w (Co, Ci) -> y (B, Co, H, W) = w . [gelu](x) + bias (None with keep_y=False: not stored) and
    act (B, Co, Hp, Wp) = zero-pad(gelu(y))."""
    _require(x, torch.float32, "x")
    _require(w, torch.float32, "weight")
    if bias is not None:
        _require(bias, torch.float32, "bias")
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    if w.shape[1] != Ci:
        raise RuntimeError(f"uno_amd: weight {tuple(w.shape)} does not match {Ci} input channels")
    y = torch.empty((B, Co, H, W), dtype=x.dtype, device=x.device) if keep_y else None
    act = torch.empty((B, Co, Hp, Wp), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().uno_channel_mix_act_padded(_ptr(x), _ptr(w), _opt(bias), _opt(y), _ptr(act),
                                              B, Ci, Co, H, W, int(Hp), int(Wp), 1 if act_in else 0, _stream(x))
    _check(rc, "uno_channel_mix_act_padded")
    return y, act


def lift_ok(x, w1, w0, Hp: int, Wp: int) -> bool:
    """shape rules of uno_lift_forward / uno_lift_backward for x (B, Cin, H, W)"""
    if x.dim() != 4 or x.dtype != torch.float32:
        return False
    H, W = x.shape[-2:]
    return (1 <= x.shape[1] <= 3 and w1.shape[0] in (16, 32) and w1.shape[1] == x.shape[1] and w0.shape[1] == w1.shape[0]
            and 260 <= W <= Wp and H <= Hp and H * W < (1 << 24))


def lift_forward(x, w1, b1, w0, b0, Hp: int, Wp: int):
    """act (B, Co, Hp, Wp) = zero-pad(gelu(w0 . gelu(w1 . x + b1) + b0)) - nothing else is stored (uno_lift_forward)."""
    for t, n in ((x, "x"), (w1, "weight 1"), (w0, "weight 0")) + tuple((t, "bias") for t in (b1, b0) if t is not None):
        _require(t, torch.float32, n)
    B, Cin, H, W = x.shape
    Cm, Co = w1.shape[0], w0.shape[0]
    act = torch.empty((B, Co, Hp, Wp), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().uno_lift_forward(_ptr(x), _ptr(w1), _opt(b1), _ptr(w0), _opt(b0),
                                    _ptr(act), B, Cin, Cm, Co, H, W, int(Hp), int(Wp), _stream(x))
    _check(rc, "uno_lift_forward")
    return act


def lift_backward_takes_second(x, w1, w0, Hp: int, Wp: int) -> bool:
    B, Cin, H, W = x.shape
    return bool(lib().uno_lift_backward_takes_second(B, Cin, w1.shape[0], w0.shape[0], H, W, int(Hp), int(Wp)))


def lift_backward(x, w1, b1, w0, b0, g_act, g_act2=None):
    """-> gw1 (Cm, Cin), gb1 (Cm) or None, gw0 (Co, Cm), gb0 (Co) or None (uno_lift_backward / uno_lift_backward2).
    g_act2: a second gradient of the padded activation (same shape, valid on the domain) added as the kernel reads (fused kernel only)."""
    _require(g_act, torch.float32, "grad_output")
    B, Cin, H, W = x.shape
    Cm, Co = w1.shape[0], w0.shape[0]
    Hp, Wp = g_act.shape[-2:]
    if tuple(g_act.shape[:2]) != (B, Co):
        raise RuntimeError("uno_amd: grad_output does not match the lift")
    if g_act2 is not None:
        _require(g_act2, torch.float32, "second grad_output")
        if tuple(g_act2.shape) != tuple(g_act.shape):
            raise RuntimeError("uno_amd: the two gradients of the lift's output disagree in shape")
    dev = x.device
    gw1 = torch.empty((Cm, Cin), dtype=torch.float32, device=dev)
    gw0 = torch.empty((Co, Cm), dtype=torch.float32, device=dev)
    gb1 = torch.empty((Cm,), dtype=torch.float32, device=dev) if b1 is not None else None
    gb0 = torch.empty((Co,), dtype=torch.float32, device=dev) if b0 is not None else None
    with torch.cuda.device(dev):
        ws = torch.empty(max(1, lib().uno_lift_bwd_ws_bytes(B, Cin, Cm, Co, H, W)), dtype=torch.uint8, device=dev)
        rc = lib().uno_lift_backward2(_ptr(x), _ptr(w1), _opt(b1), _ptr(w0), _opt(b0),
                                     _ptr(g_act), _opt(g_act2), _ptr(gw1), _opt(gb1), _ptr(gw0),
                                     _opt(gb0), _ptr(ws), B, Cin, Cm, Co, H, W, int(Hp), int(Wp), _stream(x))
    _check(rc, "uno_lift_backward")
    return gw1, gb1, gw0, gb0


def channel_mix_dgelu_padded(x, w, bias, g_padded, act_in: bool = False):
    """gz (B, Co, H, W) = gelu'(w . [gelu](x) + bias) * g_padded[..., :H, :W]: the layer recomputed from its input x (B, Ci, H, W)."""
    _require(x, torch.float32, "x")
    _require(w, torch.float32, "weight")
    _require(g_padded, torch.float32, "grad_output")
    if bias is not None:
        _require(bias, torch.float32, "bias")
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    if w.shape[1] != Ci or g_padded.dim() != 4 or g_padded.shape[:2] != (B, Co) or g_padded.shape[2] < H or g_padded.shape[3] < W:
        raise RuntimeError("uno_amd: weight / grad_output do not match the layer")
    Hp, Wp = g_padded.shape[2:]
    gz = torch.empty((B, Co, H, W), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().uno_channel_mix_dgelu_padded(_ptr(x), _ptr(w), _opt(bias), _ptr(g_padded), _ptr(gz),
                                                B, Ci, Co, H, W, int(Hp), int(Wp), 1 if act_in else 0, _stream(x))
    _check(rc, "uno_channel_mix_dgelu_padded")
    return gz


def channel_mix2_ok(C1: int, Co1, Co: int, P: int) -> bool:
    """shape rules of the fused two-source / two-destination forms (csrc/channel_mix.hip, csrc/channel_wgrad.hip)"""
    if C1 is not None and (C1 < 16 or C1 % 16):
        return False
    if Co1 is not None and (Co1 < 64 or Co1 % 64):
        return False
    return True


def channel_mix2(x1, x2, w, bias=None, transpose_w: bool = False, out=None, out2=None, split_out: int | None = None,
                 act_in: bool = False, dgelu_of=None, y_act: bool = False, accumulate: bool = False, project=None, window=None):
    """uno_channel_mix2: y = Wm . cat(x1, x2) + bias in one pass (x2 may be None).
    split_out = Co1: the output channels go to two tensors (B, Co1, P), (B, Co - Co1, P) -> returns (y1, y2);
    y_act: also return gelu(y) as a second tensor -> (y, act); act_in / dgelu_of act on x1 / y1 only;
    out (and out2): write (accumulate=True: add) into the given tensors instead of allocating;
    project = (w2 (Co,), b2 (1,) or None): also return proj (B, P) = b2 + sum_o w2[o] gelu(y[:, o]) -> (y, proj)  (Co <= 64).
    window = (rows, cols, pitch): every tensor's last axis is a whole plane of P elements of which the call reads and writes only
    the window - rows x cols points, row r at r * pitch (uno_channel_mix2_win; float32; fresh outputs are torch.empty planes whose
    elements outside the window are left as they are).  accumulate = 2 (with out and dgelu_of, one destination): gelu' multiplies
    the completed sum."""
    bf16 = _act_dtype(x1, "x1")
    _require(w, torch.float32, "weight")
    if x2 is not None:
        _require(x2, x1.dtype, "x2")
        if x2.shape[0] != x1.shape[0] or x2.shape[2] != x1.shape[2]:
            raise RuntimeError("uno_amd: the two sources disagree in batch / pixel count")
    if bias is not None:
        _require(bias, torch.float32, "bias")
    B, C1, P = x1.shape
    Ci = C1 + (x2.shape[1] if x2 is not None else 0)
    Co = w.shape[1] if transpose_w else w.shape[0]
    if (w.shape[0] if transpose_w else w.shape[1]) != Ci:
        raise RuntimeError(f"uno_amd: weight {tuple(w.shape)} does not match {Ci} input channels")
    Co1 = Co if split_out is None else int(split_out)
    if out is None:
        y1 = torch.empty((B, Co1, P), dtype=x1.dtype, device=x1.device)
        y2 = torch.empty((B, Co - Co1, P), dtype=x1.dtype, device=x1.device) if split_out is not None else None
    else:
        y1, y2 = out, out2
        _require(y1, x1.dtype, "out")
        if tuple(y1.shape) != (B, Co1, P) or (split_out is not None and (y2 is None or tuple(y2.shape) != (B, Co - Co1, P))):
            raise RuntimeError("uno_amd: output tensors do not match (B, Co1, P) / (B, Co - Co1, P)")
        if y2 is not None:
            _require(y2, x1.dtype, "out2")
    act = torch.empty((B, Co, P), dtype=x1.dtype, device=x1.device) if y_act else None
    if dgelu_of is not None:
        _require(dgelu_of, x1.dtype, "dgelu_of")
        if tuple(dgelu_of.shape) != (B, Co1, P):
            raise RuntimeError(f"uno_amd: dgelu_of has shape {tuple(dgelu_of.shape)}, expected {(B, Co1, P)}")
    proj = pw = pb = None
    if project is not None:
        pw, pb = project
        _require(pw, torch.float32, "projection weight")
        if pw.numel() != Co:
            raise RuntimeError(f"uno_amd: projection weight has {pw.numel()} entries for {Co} channels")
        if pb is not None:
            _require(pb, torch.float32, "projection bias")
        proj = torch.empty((B, P), dtype=x1.dtype, device=x1.device)
    acc_flag = int(accumulate) if out is not None else 0
    if acc_flag == 2 and (dgelu_of is None or window is None):
        raise RuntimeError("uno_amd: accumulate = 2 goes with dgelu_of (windowed one-destination calls)")
    with torch.cuda.device(x1.device), _mix_scratch(x1.device, Ci, Co, P if window is None else window[0] * window[1], bf16):
        if window is not None:
            fn, size = lib().uno_channel_mix2_win, (*_window_args(window, P, bf16), P)
        else:
            fn, size = _entry("uno_channel_mix2", bf16), (P,)
        rc = fn(_ptr(x1), _opt(x2), C1, _ptr(w), _opt(bias), _ptr(y1), _opt(y2), Co1, _opt(act),
                B, Ci, Co, *size, 1 if transpose_w else 0, acc_flag, 1 if act_in else 0,
                _opt(dgelu_of), _opt(pw), _opt(pb), _opt(proj), _stream(x1))
    _check(rc, "uno_channel_mix2")
    if split_out is not None:
        return y1, y2
    if project is not None:
        return y1, proj
    return (y1, act) if y_act else y1


def channel_wgrad_partial_floats(B: int, Ci: int, Co: int, P: int) -> int:
    """floats of split-K partial sums one weight-gradient call of this shape leaves (a whole number of (Co, Ci + 1) blocks)"""
    return int(lib().uno_channel_wgrad_ws_bytes(B, Ci, Co, P)) // 4


def channel_wgrad_finish(parts, Ci: int, Co: int, need_bias: bool, out_w=None, out_b=None, accumulate: bool = False):
    """Second stage alone: `parts` = float32 tensor holding consecutive (Co, Ci + 1) blocks of partial sums (channel_wgrad2(...,
    partials_out=row) for every row) -> gw (Co, Ci), gb (Co) or None, written (accumulate: added) into out_w / out_b when given."""
    _require(parts, torch.float32, "partial sums")
    blk = Co * (Ci + 1)
    if parts.numel() == 0 or parts.numel() % blk:
        raise RuntimeError("uno_amd: the partial sums are not a whole number of (Co, Ci + 1) blocks")
    gw, gb, accumulate = _real_grad_buffers(out_w, out_b, Ci, Co, need_bias, parts.device, accumulate)
    with torch.cuda.device(parts.device):
        rc = lib().uno_channel_wgrad_finish(_ptr(parts), _ptr(gw), _opt(gb), Ci, Co,
                                            parts.numel() // blk, 1 if accumulate else 0, _stream(parts))
    _check(rc, "uno_channel_wgrad_finish")
    return gw, gb


def channel_wgrad2(gy, x1, x2, need_bias: bool = True, act_x: bool = False, out_w=None, out_b=None, accumulate: bool = False,
                   partials_out=None, window=None):
    """gy (B, Co, P), x1 (B, C1, P), x2 (B, C2, P) or None -> gw (Co, C1 + C2), gb (Co) or None: the weight gradient of a
    (two-source) layer from one launch (act_x: x1 := gelu(x1) as it is read).  out_w / out_b: write (accumulate: add) into these
    float32 tensors of Co * Ci / Co elements instead of fresh ones (out_b is required with need_bias when out_w is given).
    partials_out: a dense float32 tensor of channel_wgrad_partial_floats() elements - the first stage only, its partial sums left
    there for channel_wgrad_finish (-> None, None).
    window = (rows, cols, pitch): the sums run over that window of the tensors' planes (uno_channel_wgrad2_win, see channel_mix2)."""
    bf16 = _act_dtype(gy, "grad_output")
    _require(x1, gy.dtype, "x1")
    B, Co, P = gy.shape
    if window is not None:
        if partials_out is not None:
            raise RuntimeError("uno_amd: windowed weight gradients run both stages")
        win = _window_args(window, P, bf16)
    C1 = x1.shape[1]
    C2 = 0
    if x2 is not None:
        _require(x2, gy.dtype, "x2")
        C2 = x2.shape[1]
        if x2.shape[0] != B or x2.shape[2] != P:
            raise RuntimeError("uno_amd: grad_output and the sources disagree in batch / pixel count")
    if x1.shape[0] != B or x1.shape[2] != P:
        raise RuntimeError("uno_amd: grad_output and the sources disagree in batch / pixel count")
    Ci = C1 + C2
    L = lib()
    if partials_out is not None:
        _require(partials_out, torch.float32, "partial-sum buffer")
        if partials_out.numel() != channel_wgrad_partial_floats(B, Ci, Co, P):
            raise RuntimeError("uno_amd: partial-sum buffer has the wrong size")
        with torch.cuda.device(gy.device):
            rc = _entry("uno_channel_wgrad2", bf16)(_ptr(gy), _ptr(x1), _opt(x2), C1, C.c_void_p(0), C.c_void_p(0),
                                                    _ptr(partials_out), B, Ci, Co, P, 1 if act_x else 0, 3, _stream(gy))
        _check(rc, "uno_channel_wgrad2")
        return None, None
    gw, gb, accumulate = _real_grad_buffers(out_w, out_b, Ci, Co, need_bias, gy.device, accumulate)
    with torch.cuda.device(gy.device):
        if window is not None:
            fn, size, Pl = L.uno_channel_wgrad2_win, (*win, P), win[0] * win[1]
        else:
            fn, size, Pl = _entry("uno_channel_wgrad2", bf16), (P,), P
        ws = torch.empty(max(1, L.uno_channel_wgrad_ws_bytes(B, Ci, Co, Pl)), dtype=torch.uint8, device=gy.device)
        rc = fn(_ptr(gy), _ptr(x1), _opt(x2), C1, _ptr(gw), _opt(gb),
                _ptr(ws), B, Ci, Co, *size, 1 if act_x else 0, 1 if accumulate else 0, _stream(gy))
    _check(rc, "uno_channel_wgrad2")
    return gw, gb


def rows_window_ok(rows: int, cols: int, pitch: int, col0: int, plane: int, Ci: int = 1, Co: int = 1) -> bool:
    """the accepted range of the short-row window entry points (uno_spectral.h: uno_channel_mix2_rows and its family)"""
    return (rows >= 0 and cols >= 1 and col0 >= 0 and col0 + cols <= pitch <= 256 and rows * pitch < (1 << 24) and plane >= rows * pitch
            and 1 <= Ci <= 1024 and Co >= 1)


def _rows_args(window, plane: int):
    rows, cols, pitch, col0 = (int(v) for v in window)
    return rows, cols, pitch, col0, int(plane)


def channel_mix2_rows(x1, x2, w, bias, window, act_in: bool = False):
    """uno_channel_mix2_rows: x1 (B, C1, plane), x2 (B, C2, plane) or None read through window = (rows, cols, pitch, col0), w (Co, C1 + C2)
    -> y (B, Co, rows * cols) dense = w . cat([gelu](x1), x2) + bias."""
    for t, n in ((x1, "x1"), (w, "weight")) + (((x2, "x2"),) if x2 is not None else ()) + (((bias, "bias"),) if bias is not None else ()):
        _require(t, torch.float32, n)
    B, C1, plane = x1.shape
    Ci = C1 + (x2.shape[1] if x2 is not None else 0)
    Co = w.shape[0]
    if w.shape[1] != Ci or (x2 is not None and (x2.shape[0] != B or x2.shape[2] != plane)):
        raise RuntimeError("uno_amd: weight / sources of a short-row layer disagree")
    geo = _rows_args(window, plane)
    y = torch.empty((B, Co, geo[0] * geo[1]), dtype=torch.float32, device=x1.device)
    with torch.cuda.device(x1.device):
        rc = lib().uno_channel_mix2_rows(_ptr(x1), _opt(x2), C1, _ptr(w), _opt(bias), _ptr(y), B, Ci, Co, *geo, 1 if act_in else 0, _stream(x1))
    _check(rc, "uno_channel_mix2_rows")
    return y


def channel_mix2_rows_grad(gy, w, C1: int, window, plane: int, need_g2: bool = True, dgelu_of=None):
    """uno_channel_mix2_rows_grad: gy (B, Co, rows * cols) dense -> (g1 (B, C1, plane), g2 (B, Ci - C1, plane) or None): w^T gy inside
    the window, +0 in the border columns of the first rows * pitch elements of every plane; what lies beyond is zeroed here (plane >
    rows * pitch does not occur in the models)."""
    _require(gy, torch.float32, "grad_output")
    _require(w, torch.float32, "weight")
    B, Co, _ = gy.shape
    Ci = w.shape[1]
    geo = _rows_args(window, plane)
    whole = geo[0] * geo[2] == plane
    g1 = torch.empty((B, C1, plane), dtype=torch.float32, device=gy.device)
    g2 = torch.empty((B, Ci - C1, plane), dtype=torch.float32, device=gy.device) if (need_g2 and Ci > C1) else None
    if not whole:
        for t in (g1, g2):
            if t is not None:
                t[:, :, geo[0] * geo[2]:].zero_()
    if dgelu_of is not None:
        _require(dgelu_of, torch.float32, "dgelu_of")
        if tuple(dgelu_of.shape) != (B, C1, plane):
            raise RuntimeError("uno_amd: dgelu_of does not match the first source")
    with torch.cuda.device(gy.device):
        rc = lib().uno_channel_mix2_rows_grad(_ptr(gy), _ptr(w), C1, _opt(dgelu_of), _ptr(g1), _opt(g2), B, Ci, Co, *geo, _stream(gy))
    _check(rc, "uno_channel_mix2_rows_grad")
    return g1, g2


def channel_wgrad2_rows(gy, x1, x2, window, need_bias: bool = True, act_x: bool = False, out_w=None, out_b=None, accumulate: bool = False):
    """uno_channel_wgrad2_rows: gy (B, Co, rows * cols) dense, x1 / x2 on the window -> gw (Co, Ci), gb (Co) or None; out_w / out_b /
    accumulate as channel_wgrad2."""
    for t, n in ((gy, "grad_output"), (x1, "x1")) + (((x2, "x2"),) if x2 is not None else ()):
        _require(t, torch.float32, n)
    B, Co, _ = gy.shape
    C1, plane = x1.shape[1], x1.shape[2]
    Ci = C1 + (x2.shape[1] if x2 is not None else 0)
    geo = _rows_args(window, plane)
    gw, gb, accumulate = _real_grad_buffers(out_w, out_b, Ci, Co, need_bias, gy.device, accumulate)
    if B == 0 or geo[0] == 0:
        if not accumulate:
            gw.zero_()
            if gb is not None:
                gb.zero_()
        return gw, gb
    L = lib()
    with torch.cuda.device(gy.device):
        ws = torch.empty(max(1, L.uno_channel_wgrad_ws_bytes(B, Ci, Co, geo[0] * geo[1])), dtype=torch.uint8, device=gy.device)
        rc = L.uno_channel_wgrad2_rows(_ptr(gy), _ptr(x1), _opt(x2), C1, _ptr(gw), _opt(gb), _ptr(ws), B, Ci, Co, *geo,
                                       1 if act_x else 0, 1 if accumulate else 0, _stream(gy))
    _check(rc, "uno_channel_wgrad2_rows")
    return gw, gb


def channel_mix_act_padded_rows(x, w, bias, window, act_in: bool = False, keep_y: bool = True):
    """uno_channel_mix_act_padded_rows: x (B, Ci, rows * cols) dense, window = (rows, cols, pitch, col0) -> y (B, Co, rows * cols) =
    w . [gelu](x) + bias (None with keep_y=False) and act (B, Co, rows * pitch) = gelu(y) in columns [col0, col0 + cols), zero elsewhere."""
    for t, n in ((x, "x"), (w, "weight")) + (((bias, "bias"),) if bias is not None else ()):
        _require(t, torch.float32, n)
    B, Ci, P = x.shape
    Co = w.shape[0]
    rows, cols, pitch, col0 = (int(v) for v in window)
    if w.shape[1] != Ci or rows * cols != P:
        raise RuntimeError("uno_amd: weight / window do not match the layer")
    y = torch.empty((B, Co, P), dtype=torch.float32, device=x.device) if keep_y else None
    act = torch.empty((B, Co, rows * pitch), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().uno_channel_mix_act_padded_rows(_ptr(x), _ptr(w), _opt(bias), _opt(y), _ptr(act), B, Ci, Co, rows, cols, pitch, col0,
                                                   1 if act_in else 0, _stream(x))
    _check(rc, "uno_channel_mix_act_padded_rows")
    return y, act


def dgelu_rows(pre, g_padded, window):
    """uno_dgelu_rows: pre (B, C, rows * cols) dense, g_padded (B, C, plane) -> gz = gelu'(pre) * g_padded[window], dense."""
    _require(pre, torch.float32, "pre-activation")
    _require(g_padded, torch.float32, "grad_output")
    B, Cc, P = pre.shape
    geo = _rows_args(window, g_padded.shape[2])
    if tuple(g_padded.shape[:2]) != (B, Cc) or geo[0] * geo[1] != P:
        raise RuntimeError("uno_amd: grad_output / window do not match the pre-activation")
    gz = torch.empty_like(pre)
    with torch.cuda.device(pre.device):
        rc = lib().uno_dgelu_rows(_ptr(pre), _ptr(g_padded), _ptr(gz), B * Cc, *geo, _stream(pre))
    _check(rc, "uno_dgelu_rows")
    return gz


def channel_wgrad(gy, x, need_bias: bool = True, act_x: bool = False):
    """gy (B, Co, P), x (B, Ci, P) -> gw (Co, Ci), gb (Co) or None; act_x: x := gelu(x) as it is read."""
    bf16 = _act_dtype(gy, "grad_output")
    _require(x, gy.dtype, "x")
    B, Co, P = gy.shape
    B2, Ci, P2 = x.shape
    if (B2, P2) != (B, P):
        raise RuntimeError("uno_amd: grad_output and x disagree in batch / pixel count")
    L = lib()
    gw = torch.empty((Co, Ci), dtype=torch.float32, device=x.device)
    gb = torch.empty((Co,), dtype=torch.float32, device=x.device) if need_bias else None
    with torch.cuda.device(x.device):
        ws = torch.empty(max(1, L.uno_channel_wgrad_ws_bytes(B, Ci, Co, P)), dtype=torch.uint8, device=x.device)
        rc = _entry("uno_channel_wgrad", bf16)(_ptr(gy), _ptr(x), _ptr(gw), _opt(gb), _ptr(ws), B, Ci, Co, P, 1 if act_x else 0, _stream(x))
    _check(rc, "uno_channel_wgrad")
    return gw, gb


def adam_step(p, g, m, v, step: int, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float):
    """In-place Adam update of one parameter tensor p (float32 or complex64) with gradient g, first moment m (real
    view shape) and second moment v (p.shape, real)."""
    cplx = p.is_complex()
    pr, gr = (torch.view_as_real(p), torch.view_as_real(g)) if cplx else (p, g)
    for t, name in ((pr, "param"), (gr, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
        _require(t, torch.float32, name)
    if gr.numel() != pr.numel() or m.numel() != pr.numel() or v.numel() != p.numel():
        raise RuntimeError("uno_amd: Adam state shapes do not match the parameter")
    with torch.cuda.device(p.device):
        rc = lib().uno_adam_step(_ptr(pr), _ptr(gr), _ptr(m), _ptr(v), p.numel(), 1 if cplx else 0, lr, beta1, beta2, eps,
                                 weight_decay, int(step), _stream(pr))
    _check(rc, "uno_adam_step")


def gelu_project_forward(pre, w, bias=None):
    """pre (B, C, P) f32, w (C,), bias (1,) or None -> out (B, P) = bias + sum_c w[c] gelu(pre[:, c])."""
    bf16 = _act_dtype(pre, "pre")
    _require(w, torch.float32, "weight")
    if bias is not None:
        _require(bias, torch.float32, "bias")
    B, Cc, P = pre.shape
    if w.numel() != Cc:
        raise RuntimeError(f"uno_amd: weight has {w.numel()} entries for {Cc} channels")
    out = torch.empty((B, P), dtype=pre.dtype, device=pre.device)
    with torch.cuda.device(pre.device):
        rc = _entry("uno_gelu_project_forward", bf16)(_ptr(pre), _ptr(w), _opt(bias), _ptr(out), B, Cc, P, _stream(pre))
    _check(rc, "uno_gelu_project_forward")
    return out


def gelu_project_backward(pre, w, gout, need_bias=True, window=None):
    """-> gpre (B, C, P), gw (C,), gb (1,) or None.  window = (rows, cols, pitch): on that window of the planes (see channel_mix2)."""
    bf16 = _act_dtype(pre, "pre")
    _require(w, torch.float32, "weight")
    _require(gout, pre.dtype, "grad_output")
    B, Cc, P = pre.shape
    if tuple(gout.shape) != (B, P):
        raise RuntimeError("uno_amd: grad_output shape does not match (batch, pixels)")
    L = lib()
    gpre = torch.empty_like(pre)
    gw = torch.empty((Cc,), dtype=torch.float32, device=pre.device)
    gb = torch.empty((1,), dtype=torch.float32, device=pre.device) if need_bias else None
    with torch.cuda.device(pre.device):
        if window is not None:
            win = _window_args(window, P, bf16)
            fn, size, Pl = L.uno_gelu_project_backward_win, (*win, P), win[0] * win[1]
        else:
            fn, size, Pl = _entry("uno_gelu_project_backward", bf16), (P,), P
        ws = torch.empty(max(1, L.uno_gelu_project_bwd_ws_bytes(B, Cc, Pl)), dtype=torch.uint8, device=pre.device)
        rc = fn(_ptr(pre), _ptr(w), _ptr(gout), _ptr(gpre), _ptr(gw), _opt(gb), _ptr(ws), B, Cc, *size,
                _stream(pre))
    _check(rc, "uno_gelu_project_backward")
    return gpre, gw, gb


def _project2_operands(pre, s, w):
    _require(pre, torch.float32, "pre")
    _require(s, torch.float32, "s")
    _require(w, torch.float32, "weight")
    B, C1, P = pre.shape
    if s.dim() != 3 or s.shape[0] != B or s.shape[2] != P:
        raise RuntimeError(f"uno_amd: second source {tuple(s.shape)} does not match (batch, *, pixels) of {tuple(pre.shape)}")
    C2 = s.shape[1]
    if w.numel() != C1 + C2:
        raise RuntimeError(f"uno_amd: weight has {w.numel()} entries for {C1} + {C2} channels")
    return B, C1, C2, P


def gelu_project2_forward(pre, s, w, bias=None, act2=False):
    """pre (B, C1, P), s (B, C2, P) f32, w (C1 + C2,), bias (1,) or None -> out (B, P) = bias + sum_c w[c] gelu(pre[:, c])
    + sum_d w[C1 + d] f(s[:, d]), f = gelu if act2 else the identity (K11, two-source form)."""
    B, C1, C2, P = _project2_operands(pre, s, w)
    if bias is not None:
        _require(bias, torch.float32, "bias")
    out = torch.empty((B, P), dtype=torch.float32, device=pre.device)
    with torch.cuda.device(pre.device):
        rc = lib().uno_gelu_project2_forward(_ptr(pre), _ptr(s), _ptr(w), _opt(bias), _ptr(out), B, C1, C2, P, 1 if act2 else 0, _stream(pre))
    _check(rc, "uno_gelu_project2_forward")
    return out


def gelu_project2_backward(pre, s, w, gout, act2=False, need_gs=True, need_bias=True):
    """-> gpre (B, C1, P), gs (B, C2, P) or None, gw (C1 + C2,), gb (1,) or None."""
    B, C1, C2, P = _project2_operands(pre, s, w)
    _require(gout, torch.float32, "grad_output")
    if tuple(gout.shape) != (B, P):
        raise RuntimeError("uno_amd: grad_output shape does not match (batch, pixels)")
    L = lib()
    gpre = torch.empty_like(pre)
    gs = torch.empty_like(s) if need_gs else None
    gw = torch.empty((C1 + C2,), dtype=torch.float32, device=pre.device)
    gb = torch.empty((1,), dtype=torch.float32, device=pre.device) if need_bias else None
    with torch.cuda.device(pre.device):
        ws = torch.empty(max(1, L.uno_gelu_project2_bwd_ws_bytes(B, C1, C2, P)), dtype=torch.uint8, device=pre.device)
        rc = L.uno_gelu_project2_backward(_ptr(pre), _ptr(s), _ptr(w), _ptr(gout), _ptr(gpre), _opt(gs), _ptr(gw), _opt(gb), _ptr(ws),
                                          B, C1, C2, P, 1 if act2 else 0, _stream(pre))
    _check(rc, "uno_gelu_project2_backward")
    return gpre, gs, gw, gb


def rel_l2_steps(pred, target):
    """pred, target dense f32 (B, ..., T), 1 <= T <= 256 -> sums (B, T, 2), rel (B, T + 1), totals (2,) (uno_rel_l2_steps, K17):
    sums[b][t] = [sum (pred - target)^2, sum target^2] over the middle axes, rel[b][t] = sqrt(num) / sqrt(den) with rel[b][T] the
    whole-trajectory ratio, totals = [sum of the per-step ratios, sum of the whole-trajectory ratios].  Forward only; launches on the
    current stream and allocates through torch, so it can be captured into a hipGraph."""
    _require(pred, torch.float32, "pred")
    _require(target, torch.float32, "target")
    if pred.shape != target.shape or pred.device != target.device:
        raise RuntimeError(f"uno_amd: pred {tuple(pred.shape)} on {pred.device} and target {tuple(target.shape)} on {target.device} differ")
    if pred.dim() < 2:
        raise RuntimeError(f"uno_amd: step errors take (batch, ..., time) tensors (got {tuple(pred.shape)})")
    B, T = pred.shape[0], pred.shape[-1]
    P = _count(pred.shape[1:-1])
    L = lib()
    with torch.cuda.device(pred.device):
        sums = torch.empty((B, T, 2), dtype=torch.float32, device=pred.device)
        rel = torch.empty((B, T + 1), dtype=torch.float32, device=pred.device)
        totals = torch.zeros((2,), dtype=torch.float32, device=pred.device) if B == 0 else torch.empty((2,), dtype=torch.float32, device=pred.device)
        ws = torch.empty(max(1, L.uno_rel_l2_steps_ws_bytes(B, P, T)), dtype=torch.uint8, device=pred.device)
        rc = L.uno_rel_l2_steps(_ptr(pred), _ptr(target), _ptr(sums), _ptr(rel), _ptr(totals), _ptr(ws), B, P, T, _stream(pred))
    _check(rc, "uno_rel_l2_steps")
    return sums, rel, totals


def rel_l2_steps_backward(pred, target, sums, g_full=None, g_step=None):
    """The gradient of rel_l2_steps' totals at pred, dense like pred (uno_rel_l2_steps_backward, K17-B: one launch): g_full is the
    upstream gradient of totals[1] (the whole-trajectory loss), g_step that of totals[0] (the per-step sum) - one f32 element each on
    the device, never read by the host; None counts as 0.  sums: (B, T, 2) of the forward call.  A term whose num is 0 is 0."""
    _require(pred, torch.float32, "pred")
    _require(target, torch.float32, "target")
    _require(sums, torch.float32, "sums")
    if pred.shape != target.shape or pred.device != target.device or pred.dim() < 2:
        raise RuntimeError(f"uno_amd: pred {tuple(pred.shape)} on {pred.device} and target {tuple(target.shape)} on {target.device} must be "
                           f"equal (batch, ..., time) tensors on one device")
    B, T = pred.shape[0], pred.shape[-1]
    P = _count(pred.shape[1:-1])
    if sums.shape != (B, T, 2) or sums.device != pred.device:
        raise RuntimeError(f"uno_amd: sums {tuple(sums.shape)} on {sums.device} is not the (B, T, 2) = ({B}, {T}, 2) sums of the forward call "
                           f"on {pred.device}")
    for name, g in (("g_full", g_full), ("g_step", g_step)):
        if g is not None:
            _require(g, torch.float32, name)
            if g.numel() != 1 or g.device != pred.device:
                raise RuntimeError(f"uno_amd: {name} {tuple(g.shape)} on {g.device} must be one element on {pred.device}")
    with torch.cuda.device(pred.device):
        gx = torch.empty_like(pred)
        rc = lib().uno_rel_l2_steps_backward(_ptr(pred), _ptr(target), _ptr(sums), _opt(g_full), _opt(g_step), _ptr(gx), B, P, T, _stream(pred))
    _check(rc, "uno_rel_l2_steps_backward")
    return gx


def _rel_l2_operands(x, y):
    """x, y: f32 (B, N) on one device, of any two strides (a row stride and an element stride) -> (B, N)"""
    _require(x, torch.float32, "x", dense=False)
    _require(y, torch.float32, "y", dense=False)
    if x.dim() != 2 or x.shape != y.shape or x.device != y.device:
        raise RuntimeError(f"uno_amd: the relative L2 loss takes two (B, N) tensors on one device (got {tuple(x.shape)} on {x.device} "
                           f"and {tuple(y.shape)} on {y.device})")
    if x.shape[1] < 1:
        raise RuntimeError(f"uno_amd: the relative L2 loss needs at least one element per row (got {tuple(x.shape)})")
    return x.shape[0], x.shape[1]


def _raw_stream(t):
    """the current stream of t's device as an integer handle (torch's raw accessor where it exists: no Stream object is built)"""
    get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    return C.c_void_p(get(t.device.index)) if get is not None and t.device.index is not None else _stream(t)


def _on_device(device):
    """a context in which `device` is current - torch.cuda.device(), or nothing where it already is (the loss is called once per
    roll-out step, and its host time is what it costs: this spares the context's two device switches)"""
    return contextlib.nullcontext() if device.index == torch.cuda.current_device() else torch.cuda.device(device)


def rel_l2_views(record, B):
    """-> sums (B, 2), ratio (B,), total (1,): views of a rel_l2_forward record"""
    return record[:2 * B].view(B, 2), record[2 * B:3 * B], record[3 * B:3 * B + 1]


def rel_l2_forward(x, y):
    """x, y f32 (B, N) views (row stride, element stride) -> ONE flat f32 record [sums (B, 2) | ratio (B) | total (1) | workspace]
    (rel_l2_views): sums = [sum (x - y)^2, sum y^2], ratio = sqrt(num) / sqrt(den), total = sum of ratio (uno_rel_l2_forward, K20: two
    launches, fixed summation order).  One allocation: the call sits between two model passes 40 times per NS-2D roll-out, and its
    host time is what it costs there.  Launches on the current stream and allocates through torch, so it can be captured into a hipGraph."""
    B, N = _rel_l2_operands(x, y)
    L = lib()
    head = (3 * B + 2) // 2 * 2                     # the workspace holds float2: an even offset
    with _on_device(x.device):
        record = torch.empty((head + L.uno_rel_l2_ws_bytes(B, N) // 4,), dtype=torch.float32, device=x.device)
        if B == 0:
            record.zero_()
        base = record.data_ptr()
        rc = L.uno_rel_l2_forward(_ptr(x), x.stride(0), x.stride(1), _ptr(y), y.stride(0), y.stride(1), base, base + 8 * B, base + 12 * B,
                                  base + 4 * head, B, N, _raw_stream(x))
    _check(rc, "uno_rel_l2_forward")
    return record


def rel_l2_backward(x, y, sums, g, scale=1.0):
    """The gradient of rel_l2_forward's ratio (or total) at x, dense (B, N): g * scale * (x - y) / (sqrt(num) sqrt(den)) (uno_rel_l2_backward,
    K20: one launch).  sums: (B, 2) from the forward call, or its whole record (which begins with them).  g: f32 on the device, (B,) -
    one value per row - or one element, which every row takes; it is not read by the host.  Rows with num == 0 get a zero gradient."""
    B, N = _rel_l2_operands(x, y)
    _require(sums, torch.float32, "sums")
    _require(g, torch.float32, "g")
    if (sums.shape != (B, 2) and (sums.dim() != 1 or sums.numel() < 3 * B + 1)) or sums.device != x.device or g.device != x.device:
        raise RuntimeError(f"uno_amd: sums {tuple(sums.shape)} on {sums.device} is neither the (B, 2) = ({B}, 2) sums nor the record of the "
                           f"forward call on {x.device}")
    if g.numel() != 1 and g.shape != (B,):
        raise RuntimeError(f"uno_amd: g {tuple(g.shape)} holds neither one value nor one per row ({B})")
    per_row = 0 if g.numel() == 1 else 1
    with _on_device(x.device):
        gx = torch.empty((B, N), dtype=torch.float32, device=x.device)
        rc = lib().uno_rel_l2_backward(_ptr(x), x.stride(0), x.stride(1), _ptr(y), y.stride(0), y.stride(1), _ptr(sums), _ptr(g), per_row,
                                       float(scale), _ptr(gx), B, N, _raw_stream(x))
    _check(rc, "uno_rel_l2_backward")
    return gx


SHELL_SPECTRUM_MIN, SHELL_SPECTRUM_MAX = 8, 512


def shell_spectrum_ws_floats(B, T, H, W, with_target) -> int:
    """floats of scratch one shell_spectrum call of these sizes needs (uno_shell_spectrum_ws_bytes; 0 for sizes out of range)"""
    return int(lib().uno_shell_spectrum_ws_bytes(int(B), int(T), int(H), int(W), 1 if with_target else 0)) // 4


def shell_spectrum(x, y=None, out=None, ws=None):
    """x [, y]: f32 device tensors seen as (B, T, H, W) frames through any four non-negative strides (permuted and sub-sampled views
    are read where they lie), 8 <= H, W <= 512 -> shell-binned energy spectra (B, T, 1, K), or (B, T, 3, K) = [E_x, E_y, E_{x - y}] with
    y (uno_shell_spectrum, K24: two launches, fixed summation order).  out: a dense f32 tensor of that shape to write; ws: f32 scratch
    of at least shell_spectrum_ws_floats() elements.  Forward only; launches on the current stream and allocates through torch, so it
    can be captured into a hipGraph."""
    _require(x, torch.float32, "x", dense=False)
    if x.dim() != 4:
        raise RuntimeError(f"uno_amd: the shell spectrum takes (B, T, H, W) views (got {tuple(x.shape)})")
    if y is not None:
        _require(y, torch.float32, "y", dense=False)
        if y.shape != x.shape or y.device != x.device:
            raise RuntimeError(f"uno_amd: x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device} differ")
    B, T, H, W = x.shape
    if not (SHELL_SPECTRUM_MIN <= H <= SHELL_SPECTRUM_MAX and SHELL_SPECTRUM_MIN <= W <= SHELL_SPECTRUM_MAX) or T < 1:
        raise RuntimeError(f"uno_amd: the shell spectrum takes T >= 1 frames of {SHELL_SPECTRUM_MIN} ... {SHELL_SPECTRUM_MAX} points per axis "
                           f"(got {tuple(x.shape)})")
    for name, t in (("x", x), ("y", y)):
        if t is not None and min(t.stride()) < 0:
            raise RuntimeError(f"uno_amd: {name} has a negative stride {t.stride()}")
    K = (math.isqrt(4 * ((H // 2) ** 2 + (W // 2) ** 2)) + 1) // 2 + 1          # round(hypot(H // 2, W // 2)) + 1, in integers
    nspec = 1 if y is None else 3
    L = lib()
    need = shell_spectrum_ws_floats(B, T, H, W, y is not None)
    with _on_device(x.device):
        if out is None:
            out = torch.empty((B, T, nspec, K), dtype=torch.float32, device=x.device)
        else:
            _require(out, torch.float32, "out")
            if out.shape != (B, T, nspec, K) or out.device != x.device:
                raise RuntimeError(f"uno_amd: out {tuple(out.shape)} on {out.device} is not ({B}, {T}, {nspec}, {K}) on {x.device}")
        if ws is None:
            ws = torch.empty((max(1, need),), dtype=torch.float32, device=x.device)
        else:
            _require(ws, torch.float32, "ws")
            if ws.numel() < need or ws.device != x.device:
                raise RuntimeError(f"uno_amd: ws holds {ws.numel()} floats on {ws.device}, the call needs {need} on {x.device}")
        ys = (0, 0, 0, 0) if y is None else y.stride()
        rc = L.uno_shell_spectrum(_ptr(x), *x.stride(), _opt(y), *ys, _ptr(out), _ptr(ws), B, T, H, W, _raw_stream(x))
    _check(rc, "uno_shell_spectrum")
    return out


SOBOLEV_MIN, SOBOLEV_MAX = 8, 512


def sobolev_ws_floats(B, T, H, W) -> int:
    """floats of scratch one sobolev_forward call of these sizes needs (uno_sobolev_ws_bytes; 0 for sizes out of range)"""
    return int(lib().uno_sobolev_ws_bytes(int(B), int(T), int(H), int(W))) // 4


def sobolev_views(record, B, T, per_frame):
    """-> sums (B, T, 2), ratio (B,) or (B, T), total (1,): views of a sobolev_forward record"""
    n, r = B * T, (B * T if per_frame else B)
    return record[:2 * n].view(B, T, 2), (record[2 * n:2 * n + r].view(B, T) if per_frame else record[2 * n:2 * n + r]), \
        record[2 * n + r:2 * n + r + 1]


def _sobolev_frames(t, name):
    _require(t, torch.float32, name, dense=False)
    if t.dim() != 4:
        raise RuntimeError(f"uno_amd: the Sobolev loss takes (B, T, H, W) views (got {name} {tuple(t.shape)})")
    if min(t.stride()) < 0:
        raise RuntimeError(f"uno_amd: {name} has a negative stride {t.stride()}")


def sobolev_forward(x, y, w2, per_frame=False, want_z=False):
    """x, y: f32 device tensors seen as (B, T, H, W) frames through any four non-negative strides, 8 <= H, W <= 512; w2: the f32 device
    weight table (H // 2 + 1, W // 2 + 1) -> (record, z): ONE flat f32 record [sums (B, T, 2) | ratio | total (1) | workspace]
    (sobolev_views) and, with want_z, the weighted difference spectrum (B, T, H, W // 2 + 1, 2) the backward call reads - else None
    (uno_sobolev_forward, K25: two launches, fixed summation order).  Launches on the current stream and allocates through torch, so it
    can be captured into a hipGraph."""
    _sobolev_frames(x, "x")
    _sobolev_frames(y, "y")
    _require(w2, torch.float32, "w2")
    B, T, H, W = x.shape
    if y.shape != x.shape or y.device != x.device or w2.device != x.device:
        raise RuntimeError(f"uno_amd: x {tuple(x.shape)} on {x.device}, y {tuple(y.shape)} on {y.device} and w2 on {w2.device} differ")
    if not (SOBOLEV_MIN <= H <= SOBOLEV_MAX and SOBOLEV_MIN <= W <= SOBOLEV_MAX) or T < 1:
        raise RuntimeError(f"uno_amd: the Sobolev loss takes T >= 1 frames of {SOBOLEV_MIN} ... {SOBOLEV_MAX} points per axis "
                           f"(got {tuple(x.shape)})")
    if w2.shape != (H // 2 + 1, W // 2 + 1):
        raise RuntimeError(f"uno_amd: w2 {tuple(w2.shape)} is not the ({H // 2 + 1}, {W // 2 + 1}) table of {H} x {W} frames")
    L = lib()
    rows = B * T if per_frame else B
    head = (2 * B * T + rows + 1 + 1) // 2 * 2          # the workspace holds float2: an even offset
    with _on_device(x.device):
        record = torch.empty((head + sobolev_ws_floats(B, T, H, W),), dtype=torch.float32, device=x.device)
        z = torch.empty((B, T, H, W // 2 + 1, 2), dtype=torch.float32, device=x.device) if want_z else None
        if B == 0:
            record.zero_()
        base = record.data_ptr()
        rc = L.uno_sobolev_forward(_ptr(x), *x.stride(), _ptr(y), *y.stride(), _ptr(w2), base, base + 8 * B * T, base + 8 * B * T + 4 * rows,
                                   _opt(z), base + 4 * head, B, T, H, W, 1 if per_frame else 0, _raw_stream(x))
    _check(rc, "uno_sobolev_forward")
    return record, z


def sobolev_backward(z, sums, g, like, per_frame=False, scale=1.0):
    """The gradient of sobolev_forward's ratio (or total) at x: g * scale * irfft2-of-z / (H W sqrt(num den)) per row of the grouping, zero
    where num == 0 (uno_sobolev_backward, K25: one launch).  z: from the forward call; sums: its (B, T, 2) sums or its whole record (which
    begins with them); g: f32 on the device, one value or one per row of the grouping, never read by the host; like: the (B, T, H, W)
    view whose gradient this is - the result has its layout (torch.empty_like) and is written through its four strides."""
    _require(z, torch.float32, "z")
    _require(sums, torch.float32, "sums")
    _require(g, torch.float32, "g")
    B, T, H, W = like.shape
    if z.shape != (B, T, H, W // 2 + 1, 2) or z.device != like.device or sums.device != like.device or g.device != like.device:
        raise RuntimeError(f"uno_amd: z {tuple(z.shape)} on {z.device} is not the spectrum of {tuple(like.shape)} frames on {like.device}")
    if sums.numel() < 2 * B * T:
        raise RuntimeError(f"uno_amd: sums {tuple(sums.shape)} holds fewer than (B, T, 2) = ({B}, {T}, 2) values")
    rows = B * T if per_frame else B
    if g.numel() != 1 and g.numel() != rows:
        raise RuntimeError(f"uno_amd: g {tuple(g.shape)} holds neither one value nor one per row ({rows})")
    with _on_device(like.device):
        gx = torch.empty_like(like)
        rc = lib().uno_sobolev_backward(_ptr(z), _ptr(sums), _ptr(g), 0 if g.numel() == 1 else 1, float(scale), 1 if per_frame else 0,
                                        _ptr(gx), *gx.stride(), B, T, H, W, _raw_stream(like))
    _check(rc, "uno_sobolev_backward")
    return gx


def rollout_ws(B, P, T, device):
    """The workspace of one roll-out of T steps over (B, P) frames (uno_rollout_ws_bytes): rollout_advance fills it step by step,
    rollout_finish reads it."""
    return torch.empty(max(1, lib().uno_rollout_ws_bytes(int(B), int(P), int(T))), dtype=torch.uint8, device=device)


def _rollout_ws_check(ws, B, P, T):
    _require(ws, torch.uint8, "ws")
    need = lib().uno_rollout_ws_bytes(B, P, T)
    if ws.numel() < need:
        raise RuntimeError(f"uno_amd: the roll-out workspace holds {ws.numel()} bytes, {need} are needed (rollout_ws)")


def rollout_advance(window, frame, target, pred, ws, T_in, t, shift):
    """One step of the NS-2D evaluation roll-out (uno_rollout_advance, K18), all dense f32 on one device: window (B, C, ...) channels-first
    with the frames in channels [0, T_in); frame: the model's prediction, B x P values (P = the window's pixels per channel); target
    (B, T, ...) time-major; pred like target, or None; ws from rollout_ws.  Writes the chunk sums of step t into ws, pred[:, t] = frame,
    and with `shift` moves the window's frames up by one IN PLACE with `frame` as the newest.  Launches on the current stream.

    target = None together with ws = None (a free-running roll-out): the same pass with no sums - pred[:, t] = frame and the shift, of
    which at least one must be asked for.  pred's time length is then free (no cap of 256 steps: that is the workspace's)."""
    if (target is None) != (ws is None):
        raise RuntimeError("uno_amd: rollout_advance takes target and ws together, or neither (the pass without sums): got "
                           + ("a workspace without a target" if target is None else "a target without a workspace"))
    if target is None and pred is None and not shift:
        raise RuntimeError("uno_amd: rollout_advance without a target has nothing to do: neither pred nor shift asks for anything")
    layout = target if target is not None else pred         # the (B, T, ...) time-major tensor that sets T; None: shift only
    named = [(window, "window"), (frame, "frame")] + [(x, n) for x, n in ((target, "target"), (pred, "pred")) if x is not None]
    for x, name in named:
        _require(x, torch.float32, name)
        if x.device != window.device:
            raise RuntimeError(f"uno_amd: {name} lives on {x.device}, the window on {window.device}")
    if window.dim() < 3 or (layout is not None and layout.dim() < 3):
        raise RuntimeError(f"uno_amd: the roll-out takes a (batch, channels, ...) window and a (batch, time, ...) target "
                           f"(got {tuple(window.shape)} and {tuple(layout.shape)})")
    B, Cw = window.shape[0], window.shape[1]
    P = _count(window.shape[2:])
    T = layout.shape[1] if layout is not None else int(t) + 1
    if frame.dim() < 2 or frame.shape[0] != B or frame.numel() != B * P:
        raise RuntimeError(f"uno_amd: frame {tuple(frame.shape)} does not hold one value per pixel of the window {tuple(window.shape)}")
    if layout is not None and (layout.shape[0] != B or _count(layout.shape[2:]) != P):
        raise RuntimeError(f"uno_amd: {'target' if target is not None else 'pred'} {tuple(layout.shape)} does not match the window "
                           f"{tuple(window.shape)}")
    if pred is not None and target is not None and pred.shape != target.shape:
        raise RuntimeError(f"uno_amd: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    L = lib()
    if ws is not None:
        if ws.device != window.device:
            raise RuntimeError(f"uno_amd: ws lives on {ws.device}, the window on {window.device}")
        _rollout_ws_check(ws, B, P, T)
    with torch.cuda.device(window.device):
        rc = L.uno_rollout_advance(_ptr(window), _ptr(frame), _opt(target), _opt(pred), _opt(ws), B, Cw, int(T_in), P, T, int(t),
                                   1 if shift else 0, _stream(window))
    _check(rc, "uno_rollout_advance")


def rollout_record(B, T, device):
    """One flat f32 tensor that holds sums (B, T, 2), rel (B, T + 1) and totals (2) back to back (rollout_views): a graph replay's
    results are taken out of the graph's memory with ONE clone."""
    n = 2 * B * T + B * (T + 1) + 2
    return torch.zeros((n,), dtype=torch.float32, device=device) if B == 0 else torch.empty((n,), dtype=torch.float32, device=device)


def rollout_views(record, B, T):
    """-> sums (B, T, 2), rel (B, T + 1), totals (2,): views of a rollout_record"""
    a, b = 2 * B * T, 2 * B * T + B * (T + 1)
    return record[:a].view(B, T, 2), record[a:b].view(B, T + 1), record[b:b + 2]


def rollout_finish(ws, B, P, T, record=None):
    """After the last rollout_advance of a roll-out: -> sums (B, T, 2), rel (B, T + 1), totals (2,) as rel_l2_steps returns them
    (uno_rollout_finish: K17's finish launch on K18's workspace), views of one rollout_record (`record`, or a fresh one).  Launches on
    the current stream and allocates through torch."""
    B, P, T = int(B), int(P), int(T)
    _rollout_ws_check(ws, B, P, T)
    L = lib()
    with torch.cuda.device(ws.device):
        if record is None:
            record = rollout_record(B, T, ws.device)
        else:
            _require(record, torch.float32, "record")
            if record.device != ws.device or record.numel() != 2 * B * T + B * (T + 1) + 2:
                raise RuntimeError(f"uno_amd: the record holds {record.numel()} floats on {record.device}: not a rollout_record of ({B}, {T})")
        sums, rel, totals = rollout_views(record, B, T)
        rc = L.uno_rollout_finish(_ptr(ws), _ptr(sums), _ptr(rel), _ptr(totals), B, P, T, _stream(ws))
    _check(rc, "uno_rollout_finish")
    return sums, rel, totals


def _rollout_lift_operands(given, pred, feat, w, target=None):
    """shape / dtype / device / density checks shared by the training roll-out's calls -> (B, T_in, F, Cm, P, T)"""
    named = [(given, "given"), (pred, "pred"), (w, "weight")] + ([(feat, "feat")] if feat is not None else []) \
        + ([(target, "target")] if target is not None else [])
    for x, name in named:
        _require(x, torch.float32, name)
        if x.device != given.device:
            raise RuntimeError(f"uno_amd: {name} lives on {x.device}, the given frames on {given.device}")
    if given.dim() < 3 or pred.dim() < 3 or w.dim() != 2:
        raise RuntimeError(f"uno_amd: the roll-out lift takes (batch, T_in, ...) given frames, a (batch, time, ...) prediction and a (Cm, C) "
                           f"weight (got {tuple(given.shape)}, {tuple(pred.shape)} and {tuple(w.shape)})")
    B, T_in = given.shape[0], given.shape[1]
    P = _count(given.shape[2:])
    T = pred.shape[1]
    if pred.shape[0] != B or _count(pred.shape[2:]) != P:
        raise RuntimeError(f"uno_amd: pred {tuple(pred.shape)} does not match the given frames {tuple(given.shape)}")
    if target is not None and target.shape != pred.shape:
        raise RuntimeError(f"uno_amd: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    F = 0
    if feat is not None:
        if feat.dim() < 2 or _count(feat.shape[1:]) != P:
            raise RuntimeError(f"uno_amd: feat {tuple(feat.shape)} is not a (features, ...) table over the {P} pixels of a frame")
        F = feat.shape[0]
    Cm = w.shape[0]
    if w.shape[1] != T_in + F:
        raise RuntimeError(f"uno_amd: weight {tuple(w.shape)} does not have {T_in} + {F} columns")
    return B, T_in, F, Cm, P, T


def rollout_lift(given, pred, feat, w, bias, t, out=None):
    """The first lift of window t of the NS-2D training roll-out (uno_rollout_lift, K19), all dense f32 on one device: given (B, T_in, ...),
    pred (B, T, ...) time-major with steps 0 ... t - 1 recorded, feat (F, ...) or None, w (Cm, T_in + F), bias (Cm,) or None
    -> h (B, Cm, ...) (written into `out` when given).  Launches on the current stream."""
    B, T_in, F, Cm, P, T = _rollout_lift_operands(given, pred, feat, w)
    if bias is not None:
        _require(bias, torch.float32, "bias")
        if bias.device != given.device or bias.numel() != Cm:
            raise RuntimeError(f"uno_amd: bias {tuple(bias.shape)} on {bias.device} does not go with the weight {tuple(w.shape)}")
    with torch.cuda.device(given.device):
        if out is None:
            out = torch.empty((B, Cm, *given.shape[2:]), dtype=torch.float32, device=given.device)
        else:
            _require(out, torch.float32, "out")
            if out.device != given.device or out.numel() != B * Cm * P:
                raise RuntimeError(f"uno_amd: out {tuple(out.shape)} on {out.device} does not hold ({B}, {Cm}, {P}) values")
        rc = lib().uno_rollout_lift(_ptr(given), _ptr(pred), _opt(feat), _ptr(w), _opt(bias), _ptr(out), B, T_in, F, Cm, P, T, int(t),
                                    _stream(given))
    _check(rc, "uno_rollout_lift")
    return out


def rollout_lift_bwd_ws(B, T_in, F, Cm, P, T, device):
    """The weight-sum workspace of one training roll-out (uno_rollout_lift_bwd_ws_bytes): a float32 tensor holding the (Cm, C + 1) blocks
    of all T windows back to back - rollout_lift_backward fills window t's, ONE channel_wgrad_finish(ws, C, Cm, ...) sums them all."""
    n = lib().uno_rollout_lift_bwd_ws_bytes(int(B), int(T_in), int(F), int(Cm), int(P), int(T)) // 4
    if n <= 0 and B > 0:
        raise RuntimeError(f"uno_amd: the roll-out lift takes T_in + F <= 32 input channels, Cm <= 64 lifted channels and T <= 256 steps "
                           f"(got T_in = {T_in}, F = {F}, Cm = {Cm}, T = {T}, P = {P})")
    return torch.empty((max(1, n),), dtype=torch.float32, device=device)


def rollout_lift_backward(gh, given, pred, target, feat, w, sums, gL, gpred, gframe, parts, t):
    """The backward of rollout_lift for window t in ONE launch (uno_rollout_lift_backward, K19-B), all dense f32 on one device: gh
    (B, Cm, ...); sums (B, T, 2) of rollout_finish; gL one float on the device; gpred like pred (+= for the window's older predicted
    frames); gframe B x P values (written for t >= 1: the complete gradient of the model's output of step t - 1 - the windows must be
    walked in descending t); parts from rollout_lift_bwd_ws (block t written).  Launches on the current stream."""
    B, T_in, F, Cm, P, T = _rollout_lift_operands(given, pred, feat, w, target)
    for x, name in ((gh, "grad_output"), (sums, "sums"), (gL, "gL"), (gpred, "gpred"), (gframe, "gframe"), (parts, "parts")):
        _require(x, torch.float32, name)
        if x.device != given.device:
            raise RuntimeError(f"uno_amd: {name} lives on {x.device}, the given frames on {given.device}")
    if gh.dim() < 3 or gh.shape[0] != B or gh.shape[1] != Cm or gh.numel() != B * Cm * P:
        raise RuntimeError(f"uno_amd: grad_output {tuple(gh.shape)} is not ({B}, {Cm}, {P} pixels)")
    if gpred.shape != pred.shape:
        raise RuntimeError(f"uno_amd: gpred {tuple(gpred.shape)} and pred {tuple(pred.shape)} differ")
    if gframe.numel() != B * P or sums.numel() != 2 * B * T or gL.numel() != 1:
        raise RuntimeError(f"uno_amd: gframe {tuple(gframe.shape)}, sums {tuple(sums.shape)} or gL {tuple(gL.shape)} do not go with "
                           f"({B}, {T}, {P} pixels)")
    L = lib()
    need = L.uno_rollout_lift_bwd_ws_bytes(B, T_in, F, Cm, P, T)
    if parts.numel() * 4 < need:
        raise RuntimeError(f"uno_amd: the weight-sum workspace holds {parts.numel() * 4} bytes, {need} are needed (rollout_lift_bwd_ws)")
    with torch.cuda.device(given.device):
        rc = L.uno_rollout_lift_backward(_ptr(gh), _ptr(given), _ptr(pred), _ptr(target), _opt(feat), _ptr(w), _ptr(sums), _ptr(gL),
                                         _ptr(gpred), _ptr(gframe), _ptr(parts), B, T_in, F, Cm, P, T, int(t), _stream(given))
    _check(rc, "uno_rollout_lift_backward")


def rollout_loss_seed(pred, target, sums, gL, gframe):
    """gframe (B x P values) = the gradient of sum_b ||pred - target|| / ||target|| of the LAST step at pred[:, T - 1], times gL
    (uno_rollout_loss_seed); pred, target (B, T, ...) time-major, sums (B, T, 2) of rollout_finish, gL one float on the device."""
    for x, name in ((pred, "pred"), (target, "target"), (sums, "sums"), (gL, "gL"), (gframe, "gframe")):
        _require(x, torch.float32, name)
        if x.device != pred.device:
            raise RuntimeError(f"uno_amd: {name} lives on {x.device}, pred on {pred.device}")
    if pred.dim() < 3 or target.shape != pred.shape:
        raise RuntimeError(f"uno_amd: pred {tuple(pred.shape)} and target {tuple(target.shape)} are not one (batch, time, ...) shape")
    B, T = pred.shape[0], pred.shape[1]
    P = _count(pred.shape[2:])
    if gframe.numel() != B * P or sums.numel() != 2 * B * T or gL.numel() != 1:
        raise RuntimeError(f"uno_amd: gframe {tuple(gframe.shape)}, sums {tuple(sums.shape)} or gL {tuple(gL.shape)} do not go with "
                           f"({B}, {T}, {P} pixels)")
    with torch.cuda.device(pred.device):
        rc = lib().uno_rollout_loss_seed(_ptr(pred), _ptr(target), _ptr(sums), _ptr(gL), _ptr(gframe), B, P, T, _stream(pred))
    _check(rc, "uno_rollout_loss_seed")


class _DeviceView:
    """a library-owned device allocation seen through the CUDA array interface"""
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2}


def table_to_device(t: torch.Tensor, device) -> torch.Tensor:
    """A host-built operand table on the device.  Outside a graph capture: `t.to(device)`.  While the current stream is being captured
    (a shape first seen inside a capture) the copy torch would make is not permitted: the table then goes through uno_upload_table
    (an allocation of the library's own, uploaded under the relaxed capture mode, never freed - the callers cache per shape)."""
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_current_stream_capturing():
        return t.to(device)
    t = t.contiguous()
    if t.numel() == 0:
        return torch.empty(t.shape, dtype=t.dtype, device=device)
    typestr = {torch.float32: "<f4", torch.int32: "<i4", torch.int64: "<i8", torch.float64: "<f8"}[t.dtype]
    with torch.cuda.device(device):
        ptr = lib().uno_upload_table(C.c_void_p(t.data_ptr()), t.numel() * t.element_size())
    if not ptr:
        _check(-5, "uno_upload_table")
    return torch.as_tensor(_DeviceView(ptr, t.shape, typestr), device=device)


def _project_geometry(window, P: int):
    if window is None:
        return (0, 0, 0, P), P
    rows, cols, pitch = _window_args(window, P, False)
    return (rows, cols, pitch, P), rows * cols


def project_backward_applies(B: int, C1: int, Ci: int, Co: int, P: int, window=None) -> bool:
    """Does uno_project_backward take fc1 (Ci -> Co, sources split at C1; C1 = Ci: one source) on planes of P elements [on that window]?"""
    geo = (0, 0, 0, P)
    if window is not None:
        geo = (*(int(v) for v in window), P)
        if not _window_fits(*geo):
            return False
    return bool(lib().uno_project_backward_applies(B, C1, Ci, Co, *geo))


def project_backward(x1, x2, w, pre, w2, gout, act_in: bool = False, need_bias: bool = True, need_bias2: bool = True, window=None,
                     out_w=None, out_b=None, accumulate: bool = False):
    """The backward pass of `fc2(gelu(fc1(cat([gelu](x1), x2))))` (uno_project_backward, ABI 12): x1 (B, C1, P), x2 (B, C2, P) or None,
    w (Co, C1 + C2), pre (B, Co, P) = fc1's output, w2 (Co), gout (B, P) -> g1, g2 (or None), gw (Co, Ci), gb (Co) or None, gw2 (Co),
    gb2 (1) or None.  The gradient at fc1's output is formed inside the two kernels.  window: see channel_mix2 (elements outside the
    window of the fresh g1 / g2 are left as they are).  out_w / out_b / accumulate: as channel_wgrad2."""
    for t, name in ((x1, "x1"), (w, "weight"), (pre, "pre"), (w2, "weight2"), (gout, "grad_output")):
        _require(t, torch.float32, name)
    B, C1, P = x1.shape
    C2 = 0
    if x2 is not None:
        _require(x2, torch.float32, "x2")
        C2 = x2.shape[1]
        if x2.shape[0] != B or x2.shape[2] != P:
            raise RuntimeError("uno_amd: the two sources disagree in batch / pixel count")
    Ci, Co = C1 + C2, pre.shape[1]
    if tuple(pre.shape) != (B, Co, P) or tuple(gout.shape) != (B, P) or w.numel() != Co * Ci or w2.numel() != Co:
        raise RuntimeError("uno_amd: project_backward: operand shapes do not match the two layers")
    geo, Pl = _project_geometry(window, P)
    L = lib()
    g1 = torch.empty_like(x1)
    g2 = torch.empty_like(x2) if x2 is not None else None
    gw, gb, accumulate = _real_grad_buffers(out_w, out_b, Ci, Co, need_bias, x1.device, accumulate)
    gw2 = torch.empty((Co,), dtype=torch.float32, device=x1.device)
    gb2 = torch.empty((1,), dtype=torch.float32, device=x1.device) if need_bias2 else None
    with torch.cuda.device(x1.device):
        ws = torch.empty(max(1, L.uno_project_backward_ws_bytes(B, Ci, Co, Pl)), dtype=torch.uint8, device=x1.device)
        rc = L.uno_project_backward(_ptr(x1), _opt(x2), C1, _ptr(w), _ptr(pre), _ptr(w2), _ptr(gout),
                                    _ptr(g1), _opt(g2), _ptr(gw), _opt(gb),
                                    _ptr(gw2), _opt(gb2), _ptr(ws), B, Ci, Co, *geo,
                                    1 if act_in else 0, 1 if accumulate else 0, _stream(x1))
    _check(rc, "uno_project_backward")
    return g1, g2, gw, gb, gw2, gb2


def _gelu_pad(s, gy, out, Hp: int, Wp: int):
    """uno_gelu_pad: out = zero-pad(gelu(s)) to (Hp, Wp), or with gy (..., Hp, Wp) the backward form gelu'(s) * gy[..., :H, :W]"""
    *lead, H, W = s.shape
    with torch.cuda.device(s.device):
        rc = _entry("uno_gelu_pad", s.dtype == torch.bfloat16)(_ptr(s), _opt(gy), _ptr(out), _count(lead), H, W, Hp, Wp,
                                                               0 if gy is None else 1, _stream(s))
    _check(rc, "uno_gelu_pad")
    return out


def gelu_pad(s, Hp: int, Wp: int):
    """s (..., H, W) f32 -> (..., Hp, Wp) = zero-pad(gelu(s)) at the end of both axes."""
    _act_dtype(s, "s")
    return _gelu_pad(s, None, torch.empty((*s.shape[:-2], Hp, Wp), dtype=s.dtype, device=s.device), Hp, Wp)


def gelu_pad_backward(s, gy):
    """gs (..., H, W) = gelu'(s) * gy[..., :H, :W]."""
    _act_dtype(s, "s")
    _require(gy, s.dtype, "grad_output")
    return _gelu_pad(s, gy, torch.empty_like(s), *gy.shape[-2:])


def channels_last_pitch(t):
    """(pitch, batch stride) in elements if `t` (B, C, *grid) is stored channels-LAST - unit stride over the channels, the grid
    points dense at one common pitch >= C (a channel slice of a wider channels-last tensor qualifies), any batch stride - else None."""
    if t.dim() < 3 or t.shape[1] < 2 or t.stride(1) != 1:
        return None
    ld = t.stride(-1)
    if ld < t.shape[1]:
        return None
    run = ld
    for d in range(t.dim() - 1, 1, -1):
        if t.shape[d] != 1 and t.stride(d) != run:
            return None
        run *= t.shape[d]
    if t.shape[0] > 1 and t.stride(0) < (run // ld - 1) * ld + t.shape[1]:
        return None
    return ld, t.stride(0)


def to_channels_first(t):
    """A channels-last f32 activation (see channels_last_pitch) as a contiguous (B, C, *grid) tensor, by the tiled transposing copy."""
    _require(t, torch.float32, "activation", dense=False)
    ld, sb = channels_last_pitch(t)
    B, Cc = t.shape[:2]
    P = _count(t.shape[2:])
    out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    with torch.cuda.device(t.device):
        rc = lib().uno_transpose_batched(_ptr(t), _ptr(out), B, P, Cc, ld, sb if B > 1 else 0, P, Cc * P, _stream(t))
    _check(rc, "uno_transpose_batched")
    return out


def instnorm_forward(x, gamma, beta, eps: float, gelu: bool):
    """x (B, C, *grid) f32 -> y, mean (B*C), rstd (B*C)."""
    bf16 = _act_dtype(x, "x")
    for t, name in ((gamma, "weight"), (beta, "bias")):
        if t is not None:
            _require(t, torch.float32, name)
    B, Cc = x.shape[0], x.shape[1]
    rows = B * Cc
    N = x.numel() // max(rows, 1)
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _entry("uno_instnorm_forward", bf16)(_ptr(x), _opt(gamma), _opt(beta), _ptr(y), _ptr(mean), _ptr(rstd), rows, Cc, N,
                                                  float(eps), 1 if gelu else 0, _stream(x))
    _check(rc, "uno_instnorm_forward")
    return y, mean, rstd


def instnorm_backward(x, gy, gamma, beta, mean, rstd, gelu: bool):
    """-> gx, s1 (B, C), s2 (B, C): sums over the batch of s1 / s2 are the bias / weight gradients."""
    bf16 = _act_dtype(x, "x")
    _require(gy, x.dtype, "grad_output")
    B, Cc = x.shape[0], x.shape[1]
    rows = B * Cc
    N = x.numel() // max(rows, 1)
    gx = torch.empty_like(x)
    s1 = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    s2 = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _entry("uno_instnorm_backward", bf16)(_ptr(x), _ptr(gy), _opt(gamma), _opt(beta), _ptr(mean), _ptr(rstd), _ptr(gx), _ptr(s1),
                                                   _ptr(s2), rows, Cc, N, 1 if gelu else 0, _stream(x))
    _check(rc, "uno_instnorm_backward")
    return gx, s1, s2


class AdamPlan:
    """Pointer tables of a fixed set of parameter tensors (params, grads, moments must not be re-allocated): one
    native call per optimiser step."""

    def __init__(self, params, grads, ms, vs):
        self.device = params[0].device
        self.n = len(params)
        reals = []
        for p, g, m, v in zip(params, grads, ms, vs):
            cplx = p.is_complex()
            pr, gr = (torch.view_as_real(p), torch.view_as_real(g)) if cplx else (p, g)
            for t, name in ((pr, "param"), (gr, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
                _require(t, torch.float32, name)
            if gr.numel() != pr.numel() or m.numel() != pr.numel() or v.numel() != p.numel():
                raise RuntimeError("uno_amd: Adam state shapes do not match the parameter")
            reals.append((pr, gr, m, v, p.numel(), 1 if cplx else 0))
        # parameters and moments are kept alive; gradient buffers are NOT (a plan must not pin the gradients of a step that
        # released them, e.g. zero_grad(set_to_none=True)): the caller re-validates the pointer tuple (`key`) before every use
        self._keep = [(r[0], r[2], r[3]) for r in reals]
        arr = _fp * self.n
        self.p = arr(*[r[0].data_ptr() for r in reals])
        self.g = arr(*[r[1].data_ptr() for r in reals])
        self.m = arr(*[r[2].data_ptr() for r in reals])
        self.v = arr(*[r[3].data_ptr() for r in reals])
        self.sizes = (C.c_longlong * self.n)(*[r[4] for r in reals])
        self.cplx = (_i * self.n)(*[r[5] for r in reals])
        self.key = tuple((r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), r[3].data_ptr()) for r in reals)

    def step(self, step: int, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float):
        with torch.cuda.device(self.device):
            rc = lib().uno_adam_step_multi(self.n, self.p, self.g, self.m, self.v, self.sizes, self.cplx, lr, beta1, beta2, eps,
                                           weight_decay, int(step), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _check(rc, "uno_adam_step_multi")

    def step_dev(self, counter, scalars, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, hyper=None):
        """the update with the step count on the device (`counter`: int32 tensor of one element, advanced here; `scalars`: four floats
        of scratch; `hyper`: None or a float64 tensor (lr, eps, weight_decay) read at execution time instead of the arguments):
        capturable in a HIP graph"""
        if scalars.numel() < 4 or scalars.dtype != torch.float32 or counter.dtype != torch.int32:
            raise RuntimeError("uno_amd: Adam device scratch must be an int32 counter and four float32 scalars")
        if hyper is not None and (hyper.dtype != torch.float64 or hyper.numel() < 3 or hyper.device != self.device):
            raise RuntimeError("uno_amd: Adam device hyper-parameters must be three float64 values on the parameters' device")
        with torch.cuda.device(self.device):
            rc = lib().uno_adam_step_multi_dev(self.n, self.p, self.g, self.m, self.v, self.sizes, self.cplx, lr, beta1, beta2, eps,
                                               weight_decay, _ptr(counter), _ptr(scalars), _opt(hyper),
                                               C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _check(rc, "uno_adam_step_multi_dev")

    def step_guarded(self, counter, scalars, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, hyper, clip_state,
                     skip_nonfinite: bool):
        """step_dev under the record GradNormPlan.run wrote for this step (`clip_state`): gradients scaled by its clip coefficient; a
        non-finite norm leaves parameters, moments and `counter` untouched when skip_nonfinite"""
        if scalars.numel() < 4 or scalars.dtype != torch.float32 or counter.dtype != torch.int32:
            raise RuntimeError("uno_amd: Adam device scratch must be an int32 counter and four float32 scalars")
        if hyper is not None and (hyper.dtype != torch.float64 or hyper.numel() < 3 or hyper.device != self.device):
            raise RuntimeError("uno_amd: Adam device hyper-parameters must be three float64 values on the parameters' device")
        _clip_record_ok(clip_state, self.device)
        with torch.cuda.device(self.device):
            rc = lib().uno_adam_step_multi_guarded(self.n, self.p, self.g, self.m, self.v, self.sizes, self.cplx, lr, beta1, beta2, eps,
                                                   weight_decay, _ptr(counter), _ptr(scalars), _opt(hyper), _ptr(clip_state),
                                                   1 if skip_nonfinite else 0, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _check(rc, "uno_adam_step_multi_guarded")


# K26's state record (include/uno_spectral.h: UNO_GRAD_NORM_*)
GRAD_NORM_RECORD = 9
GRAD_NORM_FIELDS = ("norm", "coef", "finite", "steps", "clipped", "skipped", "nonfinite", "sum", "max")


def _clip_record_ok(state, device):
    if state.dtype != torch.float64 or state.numel() != GRAD_NORM_RECORD or state.device != device or not state.is_contiguous():
        raise RuntimeError(f"uno_amd: the gradient-norm record must be {GRAD_NORM_RECORD} contiguous float64 values on the gradients' device")


def grad_norm_partials(sizes, cplx) -> int:
    """doubles of scratch K26 needs for tensors of these entry counts (one per 1024 floats of each tensor)"""
    n = len(sizes)
    b = lib().uno_grad_norm_ws_bytes(n, (C.c_longlong * n)(*sizes), (_i * n)(*[1 if c else 0 for c in cplx]))
    if b < 0:
        _check(-1, "uno_grad_norm_ws_bytes")
    return b // 8


class GradNormPlan:
    """Pointer table of a fixed list of gradient tensors (float32 / complex64, contiguous, one device) for K26.  The gradients are not
    kept alive: the caller re-validates `key` before every use, as with AdamPlan."""

    def __init__(self, grads):
        self.device = grads[0].device
        self.n = len(grads)
        reals = []
        for g in grads:
            gr = torch.view_as_real(g) if g.is_complex() else g
            _require(gr, torch.float32, "grad")
            if gr.device != self.device:
                raise RuntimeError("uno_amd: the gradients of one norm must share a device")
            reals.append((gr.data_ptr(), g.numel(), 1 if g.is_complex() else 0))
        self.g = (_fp * self.n)(*[r[0] for r in reals])
        self.sizes = (C.c_longlong * self.n)(*[r[1] for r in reals])
        self.cplx = (_i * self.n)(*[r[2] for r in reals])
        self.partials = lib().uno_grad_norm_ws_bytes(self.n, self.sizes, self.cplx) // 8
        self.key = tuple(reals)

    def run(self, max_norm, skip_nonfinite: bool, scratch, state):
        """stage 1 + stage 2 on the current stream.  max_norm: one float64 on the device; scratch: float64, at least self.partials
        entries (never read before it is written); state: the GRAD_NORM_RECORD float64 record"""
        _clip_record_ok(state, self.device)
        if max_norm.dtype != torch.float64 or max_norm.numel() != 1 or max_norm.device != self.device:
            raise RuntimeError("uno_amd: max_norm must be one float64 value on the gradients' device")
        if scratch.dtype != torch.float64 or scratch.device != self.device or not scratch.is_contiguous() or scratch.numel() < self.partials:
            raise RuntimeError(f"uno_amd: the gradient-norm scratch must hold {self.partials} contiguous float64 values on the gradients' device")
        with torch.cuda.device(self.device):
            rc = lib().uno_grad_norm(self.n, self.g, self.sizes, self.cplx, _ptr(max_norm), 1 if skip_nonfinite else 0, _ptr(scratch),
                                     8 * scratch.numel(), _ptr(state), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _check(rc, "uno_grad_norm")


NS2D_SIZES = (32, 64, 128, 256)


def ns2d_supported(N: int) -> bool:
    """True for the grid sizes the K22 kernels take: a power of two in 32 ... 256"""
    return N in NS2D_SIZES


def ns2d_workspace(B: int, N: int, device):
    """the scratch of the three ns2d calls for (B, N): uint8, uno_ns2d_ws_bytes(B, N) bytes, uninitialised"""
    return torch.empty(max(1, int(lib().uno_ns2d_ws_bytes(int(B), int(N)))), dtype=torch.uint8, device=device)


def _ns2d_args(t, dtype, name, ws):
    """(B, N, workspace) of a state (B, N, N/2 + 1) c64 or a field (B, N, N) f32"""
    _require(t, dtype, name)
    if t.dim() != 3 or t.shape[2] != (t.shape[1] if dtype == torch.float32 else t.shape[1] // 2 + 1):
        raise RuntimeError(f"uno_amd: {name} must be " + ("(B, N, N) float32" if dtype == torch.float32 else "(B, N, N/2 + 1) complex64")
                           + f" (got {tuple(t.shape)})")
    B, N = int(t.shape[0]), int(t.shape[1])
    if not ns2d_supported(N):
        raise RuntimeError(f"uno_amd: the native Navier-Stokes solver takes N in {NS2D_SIZES} (a power of two in 32 ... 256), got N={N}")
    if ws is None:
        ws = ns2d_workspace(B, N, t.device)
    else:
        _require(ws, torch.uint8, "workspace")
        if ws.numel() < lib().uno_ns2d_ws_bytes(B, N):
            raise RuntimeError("uno_amd: workspace smaller than uno_ns2d_ws_bytes(B, N)")
    return B, N, ws


def ns2d_forward(w, out=None, ws=None):
    """w (B, N, N) f32 -> rfft2(w) (B, N, N/2 + 1) c64 (uno_ns2d_forward, K22); out / ws: the result / scratch tensors to use"""
    B, N, ws = _ns2d_args(w, torch.float32, "w", ws)
    w_h = torch.empty((B, N, N // 2 + 1), dtype=torch.complex64, device=w.device) if out is None else out
    _require(w_h, torch.complex64, "w_h")
    if tuple(w_h.shape) != (B, N, N // 2 + 1):
        raise RuntimeError("uno_amd: w_h has the wrong shape")
    with torch.cuda.device(w.device):
        rc = lib().uno_ns2d_forward(_ptr(w), _ptr(w_h), _ptr(ws), B, N, _stream(w))
    _check(rc, "uno_ns2d_forward")
    return w_h


def ns2d_inverse(w_h, out=None, ws=None):
    """w_h (B, N, N/2 + 1) c64 -> irfft2(w_h, s=(N, N)) (B, N, N) f32 (uno_ns2d_inverse, K22); w_h is only read"""
    B, N, ws = _ns2d_args(w_h, torch.complex64, "w_h", ws)
    w = torch.empty((B, N, N), dtype=torch.float32, device=w_h.device) if out is None else out
    _require(w, torch.float32, "w")
    if tuple(w.shape) != (B, N, N):
        raise RuntimeError("uno_amd: w has the wrong shape")
    with torch.cuda.device(w_h.device):
        rc = lib().uno_ns2d_inverse(_ptr(w_h), _ptr(w), _ptr(ws), B, N, _stream(w_h))
    _check(rc, "uno_ns2d_inverse")
    return w


def ns2d_steps(w_h, f_h, n_steps: int, visc: float, delta_t: float, ws=None):
    """n_steps Crank-Nicolson steps of the reference's navier_stokes_2d on the state w_h (B, N, N/2 + 1) c64, in place (uno_ns2d_steps,
    K22: three launches per step from one C loop).  f_h: the forcing's half spectrum, (N, N/2 + 1) shared or (B, N, N/2 + 1) per sample."""
    B, N, ws = _ns2d_args(w_h, torch.complex64, "w_h", ws)
    _require(f_h, torch.complex64, "f_h")
    if tuple(f_h.shape) not in ((N, N // 2 + 1), (B, N, N // 2 + 1)) or f_h.device != w_h.device:
        raise RuntimeError(f"uno_amd: f_h must be ({N}, {N // 2 + 1}) or ({B}, {N}, {N // 2 + 1}) complex64 on the state's device")
    with torch.cuda.device(w_h.device):
        rc = lib().uno_ns2d_steps(_ptr(w_h), _ptr(f_h), 1 if f_h.dim() == 3 else 0, _ptr(ws), B, N, int(n_steps), float(visc), float(delta_t),
                                  _stream(w_h))
    _check(rc, "uno_ns2d_steps")
    return w_h


DARCY_SIZES = (8, 512)


def darcy_supported(K: int) -> bool:
    """True for the grid sizes the K23 kernels take: 8 ... 512"""
    return DARCY_SIZES[0] <= int(K) <= DARCY_SIZES[1]


def darcy_workspace(B: int, K: int, device):
    """the scratch of darcy_solve for (B, K): uint8, uno_darcy_ws_bytes(B, K) bytes, uninitialised"""
    return torch.empty(max(8, int(lib().uno_darcy_ws_bytes(int(B), int(K)))), dtype=torch.uint8, device=device)


def darcy_table(M: torch.Tensor, device=None) -> torch.Tensor:
    """the (N, N) matrix of a K23-T transform as the kernel reads it: zero-padded to (pitch, pitch), pitch = uno_darcy_table_pitch(N)"""
    N = int(M.shape[0])
    pitch = int(lib().uno_darcy_table_pitch(N))
    if M.dim() != 2 or M.shape[1] != N or pitch == 0:
        raise RuntimeError(f"uno_amd: a transform table is (N, N) with N in 1 ... 512 (got {tuple(M.shape)})")
    out = torch.zeros((pitch, pitch), dtype=M.dtype)
    out[:N, :N] = M.detach().cpu()
    return out if device is None else table_to_device(out, device)


def _darcy_planes(t, name, K=None):
    _require(t, torch.float64, name)
    if t.dim() != 3 or t.shape[1] != t.shape[2] or (K is not None and t.shape[1] != K):
        raise RuntimeError(f"uno_amd: {name} must be (B, {'K' if K is None else K}, {'K' if K is None else K}) float64 (got {tuple(t.shape)})")
    return int(t.shape[0]), int(t.shape[1])


def _darcy_size(K):
    if not darcy_supported(K):
        raise RuntimeError(f"uno_amd: the native Darcy solver takes grids of 8 ... 512 nodes a side, got K={K}")


def darcy_transform(table, x, post=None, out=None):
    """post o (M x[b] M^T) for x (B, N, N), float32 or float64 (uno_darcy_transform, K23-T); table: darcy_table(M) on x's device"""
    if x.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"uno_amd: x must be float32 or float64 (got {x.dtype})")
    _require(x, x.dtype, "x")
    _require(table, x.dtype, "table")
    if x.dim() != 3 or x.shape[1] != x.shape[2]:
        raise RuntimeError(f"uno_amd: x must be (B, N, N) (got {tuple(x.shape)})")
    B, N = int(x.shape[0]), int(x.shape[1])
    pitch = int(lib().uno_darcy_table_pitch(N))
    if pitch == 0 or tuple(table.shape) != (pitch, pitch):
        raise RuntimeError(f"uno_amd: the table of an N={N} transform is ({pitch}, {pitch}) with N in 1 ... 512 (got {tuple(table.shape)})")
    if post is not None:
        _require(post, x.dtype, "post")
        if tuple(post.shape) != (N, N):
            raise RuntimeError("uno_amd: post has the wrong shape")
    y = torch.empty_like(x) if out is None else out
    _require(y, x.dtype, "out")
    if tuple(y.shape) != tuple(x.shape):
        raise RuntimeError("uno_amd: out has the wrong shape")
    tmp = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = lib().uno_darcy_transform(_ptr(table), _ptr(x), _ptr(y), _ptr(tmp), _opt(post), B, N, 1 if x.dtype == torch.float32 else 0,
                                       _stream(x))
    _check(rc, "uno_darcy_transform")
    return y


def darcy_apply(coef, p):
    """A p (B, K-2, K-2) for the nodal coefficient coef (B, K, K) and p (B, K-2, K-2), float64 (uno_darcy_apply, K23-A)"""
    B, K = _darcy_planes(coef, "coef")
    _darcy_size(K)
    _require(p, torch.float64, "p")
    if tuple(p.shape) != (B, K - 2, K - 2) or p.device != coef.device:
        raise RuntimeError(f"uno_amd: p must be ({B}, {K - 2}, {K - 2}) float64 on coef's device")
    ap = torch.empty_like(p)
    with torch.cuda.device(coef.device):
        rc = lib().uno_darcy_apply(_ptr(coef), _ptr(p), _ptr(ap), B, K, _stream(coef))
    _check(rc, "uno_darcy_apply")
    return ap


def darcy_solve(coef, F, rtol: float = 1e-10, max_iter: int = 500, check_every: int = 8, ws=None, out=None):
    """The nodal solution (B, K, K) of the 5-point system of the nodal coefficient coef and right-hand side F, both (B, K, K) float64
    (uno_darcy_solve, K23) -> (P, iterations (B) int32, relative residual (B) float64, status (B) int32: 1 converged, 0 max_iter
    reached, 2 breakdown).  The three small tensors are still on the device: reading them is the caller's synchronisation."""
    B, K = _darcy_planes(coef, "coef")
    _darcy_size(K)
    _darcy_planes(F, "F", K)
    if int(F.shape[0]) != B or F.device != coef.device:
        raise RuntimeError("uno_amd: F must have coef's shape and device")
    if ws is None:
        ws = darcy_workspace(B, K, coef.device)
    else:
        _require(ws, torch.uint8, "workspace")
        if ws.numel() < lib().uno_darcy_ws_bytes(B, K):
            raise RuntimeError("uno_amd: workspace smaller than uno_darcy_ws_bytes(B, K)")
    P = torch.empty_like(coef) if out is None else out
    _require(P, torch.float64, "out")
    if tuple(P.shape) != (B, K, K):
        raise RuntimeError("uno_amd: out has the wrong shape")
    iters = torch.empty(B, dtype=torch.int32, device=coef.device)
    relres = torch.empty(B, dtype=torch.float64, device=coef.device)
    status = torch.empty(B, dtype=torch.int32, device=coef.device)
    with torch.cuda.device(coef.device):
        rc = lib().uno_darcy_solve(_ptr(coef), _ptr(F), _ptr(P), _ptr(iters), _ptr(relres), _ptr(status), _ptr(ws), B, K, float(rtol),
                                   int(max_iter), int(check_every), _stream(coef))
    _check(rc, "uno_darcy_solve")
    return P, iters, relres, status


def profile_begin(max_records: int = 100000):
    _check(lib().uno_profile_begin(int(max_records)), "uno_profile_begin")


def profile_end():
    """-> list of (kernel name, milliseconds, algorithmic bytes), one per kernel launch recorded."""
    L = lib()
    n = L.uno_profile_end()
    out = []
    name = C.create_string_buffer(64)
    ms, by = C.c_double(), C.c_double()
    for i in range(n):
        _check(L.uno_profile_get(i, name, 64, C.byref(ms), C.byref(by)), "uno_profile_get")
        out.append((name.value.decode(), ms.value, by.value))
    return out
