"""Loader for libptrace_scatter.so (include/ptrace_scatter.h: BRDF.scatter_ray and the Russian roulette for hit records): its
table for ``_addon.Addon``.  The library takes the slot table ``_surface_lib``'s makes."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_scatter.h declares
EXPORTS = ("pt_rays_scatter_version", "pt_rays_scatter_args_bytes", "pt_rays_scatter_last_error", "pt_rays_scatter_bytes",
           "pt_rays_scatter_plane_offset", "pt_rays_scatter_device", "pt_rays_scatter")

ABI_MAJOR, ABI_MINOR = 1, 2

_vp, _ll, _sz, _i = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int
_SIGNATURES = (
    ("pt_rays_scatter_version", _i, []),
    ("pt_rays_scatter_args_bytes", _sz, []),
    ("pt_rays_scatter_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_scatter_bytes", _sz, [_ll, _i]),
    ("pt_rays_scatter_plane_offset", _ll, [_ll, _i, _i, _i]),
    ("pt_rays_scatter_device", _i, [_i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _vp, _sz, _vp]),
    ("pt_rays_scatter", _i, [_i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _vp, _sz]),
)
# PTRACE_SCATTER_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_scatter.so", "PTRACE_SCATTER_LIB", "ray-library interface", "pt_rays_scatter_version",
                      "pt_rays_scatter_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
