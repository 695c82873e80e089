"""Loader for libptrace_gradient.so (include/ptrace_gradient.h: probes of this frame to be gathered in the previous world, the share of
its history every pixel keeps, and the motion accumulation with that share applied): its table for ``_addon.Addon``, its structures
and its tables."""
from __future__ import annotations

import ctypes as C

from . import _addon, _motion_lib, _temporal_lib, _weighted_lib

# every symbol include/ptrace_gradient.h declares
EXPORTS = ("pt_rays_gradient_version", "pt_rays_gradient_last_error", "pt_rays_gradient_strata", "pt_rays_gradient_keep_bytes",
           "pt_rays_gradient_bytes", "pt_rays_gradient_count_bytes", "pt_rays_gradient_table_bytes", "pt_rays_gradient_clear_device",
           "pt_rays_gradient_probes_device", "pt_rays_gradient_probes", "pt_rays_gradient_keep_device", "pt_rays_gradient_keep",
           "pt_rays_gradient_accumulate_device", "pt_rays_gradient_accumulate")

ABI_MAJOR, ABI_MINOR = 1, 14

GR_SAME_SHAPE, GR_BLEND_WEIGHT = 1, 2  # PT_GR_* of the header
MAX_HISTORY = 2 ** 20
MAX_SHAPES = 2 ** 20
RECORD = 24  # doubles per shape in the motion table: 192 bytes
MAX_STRATUM, MAX_RADIUS = 16, 4
# the defaults of the accumulation: the motion accumulate query's;  and those of the probes and of keep
DEFAULTS = dict(_motion_lib.DEFAULTS)
KEEP_DEFAULTS = dict(stratum=3, radius=1, gain=8.0, same_shape_probes=True)


class GradientParams(C.Structure):
    """``pt_gradient_params`` of include/ptrace_gradient.h."""
    _fields_ = [("stratum", C.c_int), ("radius", C.c_int), ("flags", C.c_int), ("gain", C.c_double)]


# ``pt_gradient_history`` has the layout of the weighted query's params, ``pt_gradient_camera`` that of the temporal query's camera
GradientHistory = _weighted_lib.WeightedParams
GradientCamera = _temporal_lib.TemporalCamera
camera = _temporal_lib.camera
history = _weighted_lib.params
tables = _motion_lib.tables


def params(stratum=3, radius=1, gain=8.0, same_shape_probes=True, flags=None) -> GradientParams:
    """``pt_gradient_params`` from the values as they are: the library checks them.  ``flags=`` (an int) is passed as it is."""
    bits = _addon.c_int(flags, "flags") if flags is not None else (GR_SAME_SHAPE if same_shape_probes else 0)
    return GradientParams(_addon.c_int(stratum, "stratum"), _addon.c_int(radius, "radius"), bits, float(gain))


def strata(width: int, height: int, stratum: int) -> int:
    """``ceil(width / stratum) * ceil(height / stratum)``: the probes of a frame (``ValueError`` for what the library refuses)."""
    width, height, stratum = int(width), int(height), int(stratum)
    if width < 0 or height < 0 or width * height > 2 ** 31 - 1:
        raise ValueError(f"a frame of {width} x {height} records")
    if not 1 <= stratum <= MAX_STRATUM:
        raise ValueError(f"stratum={stratum}: 1 to 16")
    return ((width + stratum - 1) // stratum) * ((height + stratum - 1) // stratum)


_vp, _ll, _sz, _i, _u64 = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.c_ulonglong
_pp, _ph, _pc = C.POINTER(GradientParams), C.POINTER(GradientHistory), C.POINTER(GradientCamera)
_SIGNATURES = (
    ("pt_rays_gradient_version", _i, []),
    ("pt_rays_gradient_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_gradient_strata", _ll, [_i, _i, _i]),
    ("pt_rays_gradient_keep_bytes", _sz, [_ll]),
    ("pt_rays_gradient_bytes", _sz, [_ll]),
    ("pt_rays_gradient_count_bytes", _sz, [_ll]),
    ("pt_rays_gradient_table_bytes", _sz, [_i]),
    ("pt_rays_gradient_clear_device", _i, [_i, _ll, _vp, _sz, _vp]),
    ("pt_rays_gradient_probes_device", _i, [_i, _i, _i, _i, _u64, _i, _u64] + [_vp] * 3 + [_i, _vp, _vp] + [_vp, _sz] * 4 + [_vp]),
    ("pt_rays_gradient_probes", _i, [_i, _i, _i, _i, _u64, _i, _u64] + [_vp] * 3 + [_i, _vp, _vp] + [_vp, _sz] * 4),
    ("pt_rays_gradient_keep_device", _i, [_i, _i, _i, _pp] + [_vp] * 4 + [_vp, _sz, _vp]),
    ("pt_rays_gradient_keep", _i, [_i, _i, _i, _pp] + [_vp] * 4 + [_vp, _sz]),
    ("pt_rays_gradient_accumulate_device", _i, [_i, _i, _i, _ph, _pc] + [_vp] * 11 + [_i, _vp, _vp, _vp] + [_vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_gradient_accumulate", _i, [_i, _i, _i, _ph, _pc] + [_vp] * 11 + [_i, _vp, _vp, _vp] + [_vp, _sz, _vp, _sz, _vp, _sz]),
)
# PTRACE_GRADIENT_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_gradient.so", "PTRACE_GRADIENT_LIB", "ray-library interface", "pt_rays_gradient_version",
                      "pt_rays_gradient_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
