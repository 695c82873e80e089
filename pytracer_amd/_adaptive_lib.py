"""Loader for libptrace_adaptive.so (include/ptrace_adaptive.h: sample counts from a variance plane, their prefix sum, and a gather
whose sample count is a per-record plane): its table for ``_addon.Addon``, and its two parameter structures."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_adaptive.h declares
EXPORTS = ("pt_rays_adaptive_version", "pt_rays_adaptive_args_bytes", "pt_rays_adaptive_last_error", "pt_rays_adaptive_bytes",
           "pt_rays_adaptive_plane_offset", "pt_rays_adaptive_offsets_bytes", "pt_rays_adaptive_offsets_workspace_bytes",
           "pt_rays_adaptive_workspace_bytes", "pt_rays_adaptive_counts_device", "pt_rays_adaptive_offsets_device",
           "pt_rays_adaptive_gather_device", "pt_rays_adaptive_counts", "pt_rays_adaptive_offsets", "pt_rays_adaptive_gather")

ABI_MAJOR, ABI_MINOR = 1, 11

ADAPTIVE_COUNT, ADAPTIVE_TAKEN, ADAPTIVE_ALL = 1, 2, 3  # PT_ADAPTIVE_* of the header
MAX_SAMPLES = 2 ** 20
# the defaults of every Python entry point that makes counts.  ``tolerance`` is the relative standard error of the luminance a pixel
# is sampled down to and ``luminance_floor`` the least luminance it is relative to (profiles/adaptive_kernel.txt records the sweep
# they were chosen from); ``gain`` scales every count.
DEFAULTS = dict(min_samples=1, max_samples=32, tolerance=0.05, luminance_floor=1.0, gain=1.0)


class CountParams(C.Structure):
    """``pt_adaptive_count_params`` of include/ptrace_adaptive.h."""
    _fields_ = [("min_samples", C.c_int), ("max_samples", C.c_int), ("tolerance", C.c_double), ("luminance_floor", C.c_double),
                ("gain", C.c_double)]


class AdaptiveParams(C.Structure):
    """``pt_adaptive_params`` of include/ptrace_adaptive.h."""
    _fields_ = [("num_of_rays", C.c_int), ("max_depth", C.c_int), ("rr_limit", C.c_int), ("depth0", C.c_int), ("init_state", C.c_ulonglong),
                ("init_seq", C.c_ulonglong), ("background", C.c_double * 3), ("capacity", C.c_longlong)]


def count_params(min_samples=1, max_samples=32, tolerance=0.05, luminance_floor=1.0, gain=1.0) -> CountParams:
    """``pt_adaptive_count_params`` from the values as they are: the library checks them."""
    return CountParams(_addon.c_int(min_samples, "min_samples"), _addon.c_int(max_samples, "max_samples"), float(tolerance),
                       float(luminance_floor), float(gain))


def params(num_of_rays, max_depth, rr_limit, depth0, init_state, init_seq, background, capacity) -> AdaptiveParams:
    bg, c_int = _addon.background3(background), _addon.c_int
    mask = 2 ** 64 - 1  # (every value of the 64-bit range is legal and wraps, as pcg_streams has it)
    capacity = int(capacity)
    if not -2 ** 63 <= capacity < 2 ** 63:
        raise ValueError(f"capacity={capacity} does not fit a C long long")
    return AdaptiveParams(c_int(num_of_rays, "num_of_rays"), c_int(max_depth, "max_depth"), c_int(rr_limit, "russian_roulette_limit"),
                          c_int(depth0, "depth"), int(init_state) & mask, int(init_seq) & mask, bg, capacity)


_vp, _ll, _sz, _i = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int
_cp, _pp = C.POINTER(CountParams), C.POINTER(AdaptiveParams)
_SIGNATURES = (
    ("pt_rays_adaptive_version", _i, []),
    ("pt_rays_adaptive_args_bytes", _sz, []),
    ("pt_rays_adaptive_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_adaptive_bytes", _sz, [_ll, _i]),
    ("pt_rays_adaptive_plane_offset", _ll, [_ll, _i, _i, _i]),
    ("pt_rays_adaptive_offsets_bytes", _sz, [_ll]),
    ("pt_rays_adaptive_offsets_workspace_bytes", _sz, [_ll]),
    ("pt_rays_adaptive_workspace_bytes", _sz, [_i, _ll, _ll, _i, _i, _i]),
    ("pt_rays_adaptive_counts_device", _i, [_i, _ll, _cp, _vp, _vp, _vp, _vp, _sz, _vp]),
    ("pt_rays_adaptive_offsets_device", _i, [_i, _ll, _vp, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_adaptive_gather_device", _i, [_i, _vp, _sz] + [_vp] * 6 + [_ll, _pp, _i, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_adaptive_counts", _i, [_i, _ll, _cp, _vp, _vp, _vp, _vp, _sz]),
    ("pt_rays_adaptive_offsets", _i, [_i, _ll, _vp, _vp, _sz]),
    ("pt_rays_adaptive_gather", _i, [_i, _vp, _sz] + [_vp] * 6 + [_ll, _pp, _i, _vp, _sz]),
)
# PTRACE_ADAPTIVE_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_adaptive.so", "PTRACE_ADAPTIVE_LIB", "ray-library interface", "pt_rays_adaptive_version",
                      "pt_rays_adaptive_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
