"""Loader for libptrace_weighted.so (include/ptrace_weighted.h: the accumulation over frames weighted by the samples each frame took,
colour and luminance moments in one launch): its table for ``_addon.Addon``, and its two structures."""
from __future__ import annotations

import ctypes as C

from . import _addon, _temporal_lib

# every symbol include/ptrace_weighted.h declares
EXPORTS = ("pt_rays_weighted_version", "pt_rays_weighted_last_error", "pt_rays_weighted_bytes", "pt_rays_weighted_count_bytes",
           "pt_rays_weighted_clear_device", "pt_rays_weighted_accumulate_device", "pt_rays_weighted_accumulate")

ABI_MAJOR, ABI_MINOR = 1, 12

WA_SAME_SHAPE, WA_BLEND_WEIGHT = 1, 2  # PT_WA_* of the header
MAX_HISTORY = 2 ** 20
# the defaults of every Python entry point.  ``max_weight``: the cap the unweighted path reaches at the project's defaults,
# ``max_history`` 32 times the shaders' 4 samples
DEFAULTS = dict(max_history=32, same_shape=True, blend_weight=False, normal_min=0.9, point_tolerance=0.05, max_weight=128.0)


class WeightedParams(C.Structure):
    """``pt_weighted_params`` of include/ptrace_weighted.h."""
    _fields_ = [("max_history", C.c_int), ("flags", C.c_int), ("normal_min", C.c_double), ("point_tolerance", C.c_double),
                ("max_weight", C.c_double)]


# ``pt_weighted_camera`` has the layout of ``pt_temporal_camera``: the camera the previous frame was seen from
WeightedCamera = _temporal_lib.TemporalCamera
camera = _temporal_lib.camera


def flags_of(same_shape=True, blend_weight=False, flags=None) -> int:
    """The ``PT_WA_*`` bits of two booleans; ``flags=`` (an int) is passed as it is, for the library to check."""
    if flags is not None:
        return _addon.c_int(flags, "flags")
    return (WA_SAME_SHAPE if same_shape else 0) | (WA_BLEND_WEIGHT if blend_weight else 0)


def params(max_history=32, same_shape=True, blend_weight=False, normal_min=0.9, point_tolerance=0.05, max_weight=128.0,
           flags=None) -> WeightedParams:
    """``pt_weighted_params`` from the values as they are: the library checks them."""
    return WeightedParams(_addon.c_int(max_history, "max_history"), flags_of(same_shape, blend_weight, flags), float(normal_min),
                          float(point_tolerance), float(max_weight))


_vp, _ll, _sz, _i, _pp, _pc = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(WeightedParams), C.POINTER(WeightedCamera)
_SIGNATURES = (
    ("pt_rays_weighted_version", _i, []),
    ("pt_rays_weighted_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_weighted_bytes", _sz, [_ll]),
    ("pt_rays_weighted_count_bytes", _sz, [_ll]),
    ("pt_rays_weighted_clear_device", _i, [_i, _ll, _vp, _sz, _vp]),
    ("pt_rays_weighted_accumulate_device", _i, [_i, _i, _i, _pp, _pc] + [_vp] * 11 + [_vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_weighted_accumulate", _i, [_i, _i, _i, _pp, _pc] + [_vp] * 11 + [_vp, _sz, _vp, _sz, _vp, _sz]),
)
# PTRACE_WEIGHTED_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_weighted.so", "PTRACE_WEIGHTED_LIB", "ray-library interface", "pt_rays_weighted_version",
                      "pt_rays_weighted_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
