"""Loader for libptrace_variance.so (include/ptrace_variance.h: luminance moments, a per-pixel variance and a variance-guided
filter): its table for ``_addon.Addon``, and its parameter structure."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_variance.h declares
EXPORTS = ("pt_rays_variance_version", "pt_rays_variance_last_error", "pt_rays_variance_bytes", "pt_rays_variance_plane_bytes",
           "pt_rays_variance_workspace_bytes", "pt_rays_variance_moments_device", "pt_rays_variance_estimate_device",
           "pt_rays_variance_filter_device", "pt_rays_variance_moments", "pt_rays_variance_estimate", "pt_rays_variance_filter")

ABI_MAJOR, ABI_MINOR = 1, 10

VR_SAME_SHAPE, VR_WRAP_X = 1, 2  # PT_VR_* of the header
MAX_HISTORY = 2 ** 20
# the defaults of every Python entry point.  ``sigma_luminance`` scales the standard deviation a luminance difference is measured in
# (profiles/variance_kernel.txt records the sweep it was chosen from); ``epsilon`` keeps that scale from 0; ``min_history``: below
# it the estimate is spatial; ``normal_min`` and ``point_tolerance`` are the accumulate query's two hard tests, for that estimate.
DEFAULTS = dict(passes=4, sigma_point=0.1, normal_power_log2=5, sigma_luminance=1.0, epsilon=1e-10, min_history=4, normal_min=0.9,
                point_tolerance=0.05, same_shape=True, wrap_x=False)


class VarianceParams(C.Structure):
    """``pt_variance_params`` of include/ptrace_variance.h."""
    _fields_ = [("passes", C.c_int), ("normal_power_log2", C.c_int), ("flags", C.c_int), ("min_history", C.c_int), ("sigma_point", C.c_double),
                ("sigma_luminance", C.c_double), ("epsilon", C.c_double), ("normal_min", C.c_double), ("point_tolerance", C.c_double)]


def flags_of(same_shape=True, wrap_x=False, flags=None) -> int:
    """The ``PT_VR_*`` bits of two booleans; ``flags=`` (an int) is passed as it is, for the library to check."""
    if flags is not None:
        return _addon.c_int(flags, "flags")
    return (VR_SAME_SHAPE if same_shape else 0) | (VR_WRAP_X if wrap_x else 0)


def params(passes=4, sigma_point=0.1, normal_power_log2=5, sigma_luminance=1.0, epsilon=1e-10, min_history=4, normal_min=0.9,
           point_tolerance=0.05, same_shape=True, wrap_x=False, flags=None) -> VarianceParams:
    """``pt_variance_params`` from the values as they are: the library checks them."""
    return VarianceParams(_addon.c_int(passes, "passes"), _addon.c_int(normal_power_log2, "normal_power_log2"), flags_of(same_shape, wrap_x, flags),
                          _addon.c_int(min_history, "min_history"), float(sigma_point), float(sigma_luminance), float(epsilon), float(normal_min),
                          float(point_tolerance))


_vp, _ll, _sz, _i, _pp = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(VarianceParams)
_SIGNATURES = (
    ("pt_rays_variance_version", _i, []),
    ("pt_rays_variance_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_variance_bytes", _sz, [_ll]),
    ("pt_rays_variance_plane_bytes", _sz, [_ll]),
    ("pt_rays_variance_workspace_bytes", _sz, [_i, _i, _pp]),
    ("pt_rays_variance_moments_device", _i, [_i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    ("pt_rays_variance_estimate_device", _i, [_i, _i, _i, _pp] + [_vp] * 5 + [_vp, _sz, _vp]),
    ("pt_rays_variance_filter_device", _i, [_i, _i, _i, _pp] + [_vp] * 5 + [_vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_variance_moments", _i, [_i, _i, _i, _vp, _vp, _vp, _sz]),
    ("pt_rays_variance_estimate", _i, [_i, _i, _i, _pp] + [_vp] * 5 + [_vp, _sz]),
    ("pt_rays_variance_filter", _i, [_i, _i, _i, _pp] + [_vp] * 5 + [_vp, _sz, _vp, _sz]),
)
# PTRACE_VARIANCE_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_variance.so", "PTRACE_VARIANCE_LIB", "ray-library interface", "pt_rays_variance_version",
                      "pt_rays_variance_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
