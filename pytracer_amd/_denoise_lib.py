"""Loader for libptrace_denoise.so (include/ptrace_denoise.h: an edge-avoiding filter for noisy radiance frames): its table for
``_addon.Addon``, and its parameter structure."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_denoise.h declares
EXPORTS = ("pt_rays_denoise_version", "pt_rays_denoise_last_error", "pt_rays_denoise_bytes", "pt_rays_denoise_workspace_bytes",
           "pt_rays_denoise_device", "pt_rays_denoise")

ABI_MAJOR, ABI_MINOR = 1, 8

DN_SAME_SHAPE, DN_WRAP_X = 1, 2  # PT_DN_* of the header
# the defaults of every Python entry point (``sigma_point`` is in world units: the plane distance, per step, at which a tap's
# weight halves)
DEFAULTS = dict(passes=4, sigma_point=0.1, normal_power_log2=5, sigma_colour=float("inf"), same_shape=True, wrap_x=False)


class DenoiseParams(C.Structure):
    """``pt_denoise_params`` of include/ptrace_denoise.h."""
    _fields_ = [("passes", C.c_int), ("normal_power_log2", C.c_int), ("flags", C.c_int), ("sigma_point", C.c_double),
                ("sigma_colour", C.c_double)]


def flags_of(same_shape=True, wrap_x=False, flags=None) -> int:
    """The ``PT_DN_*`` bits of two booleans; ``flags=`` (an int) is passed as it is, for the library to check."""
    if flags is not None:
        return _addon.c_int(flags, "flags")
    return (DN_SAME_SHAPE if same_shape else 0) | (DN_WRAP_X if wrap_x else 0)


def params(passes=4, sigma_point=0.1, normal_power_log2=5, sigma_colour=float("inf"), same_shape=True, wrap_x=False, flags=None) -> DenoiseParams:
    """``pt_denoise_params`` from the values as they are: the library checks them."""
    return DenoiseParams(_addon.c_int(passes, "passes"), _addon.c_int(normal_power_log2, "normal_power_log2"), flags_of(same_shape, wrap_x, flags),
                         float(sigma_point), float(sigma_colour))


_vp, _ll, _sz, _i, _pp = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(DenoiseParams)
_SIGNATURES = (
    ("pt_rays_denoise_version", _i, []),
    ("pt_rays_denoise_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_denoise_bytes", _sz, [_ll]),
    ("pt_rays_denoise_workspace_bytes", _sz, [_i, _i, _pp]),
    ("pt_rays_denoise_device", _i, [_i, _i, _i, _pp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_denoise", _i, [_i, _i, _i, _pp, _vp, _vp, _vp, _vp, _vp, _sz]),
)
# PTRACE_DENOISE_LIB: an alternative build of the same C-ABI library (for instance one made with -DPT_DN_DIRECT)
_ADDON = _addon.Addon("libptrace_denoise.so", "PTRACE_DENOISE_LIB", "ray-library interface", "pt_rays_denoise_version", "pt_rays_denoise_last_error",
                      ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
