"""Loader for libptrace_surface.so (include/ptrace_surface.h: the material and the point-light shading of hit records): its
table for ``_addon.Addon``, and ``rgb`` for the colour arguments."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_surface.h declares
EXPORTS = ("pt_rays_surface_version", "pt_rays_surface_args_bytes", "pt_rays_surface_last_error", "pt_rays_slots_bytes",
           "pt_rays_slots_device", "pt_rays_surface_bytes", "pt_rays_surface_plane_offset", "pt_rays_surface_device",
           "pt_rays_surface", "pt_rays_shade_lights_device", "pt_rays_shade_lights")

ABI_MAJOR = 1
_D3 = C.c_double * 3

_vp, _ll, _sz, _i = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int
_SIGNATURES = (
    ("pt_rays_surface_version", _i, []),
    ("pt_rays_surface_args_bytes", _sz, []),
    ("pt_rays_surface_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_slots_bytes", _sz, [_vp, _sz]),
    ("pt_rays_slots_device", _i, [_i, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_surface_bytes", _sz, [_ll, _i]),
    ("pt_rays_surface_plane_offset", _ll, [_ll, _i, _i, _i]),
    ("pt_rays_surface_device", _i, [_i, _vp, _sz, _vp, _vp, _vp, _ll, _i, _vp, _sz, _vp]),
    ("pt_rays_surface", _i, [_i, _vp, _sz, _vp, _vp, _ll, _i, _vp, _sz]),
    ("pt_rays_shade_lights_device", _i, [_i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _sz, _vp]),
    ("pt_rays_shade_lights", _i, [_i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _sz]),
)
# PTRACE_SURFACE_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_surface.so", "PTRACE_SURFACE_LIB", "ray-library interface", "pt_rays_surface_version",
                      "pt_rays_surface_last_error", ABI_MAJOR, 0, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check


def rgb(color) -> C.Array:
    """Three doubles for the ``ambient`` / ``background`` arguments, from an (r, g, b) sequence or a ``Color``."""
    if hasattr(color, "r"):
        color = (color.r, color.g, color.b)
    r, g, b = (float(x) for x in color)
    return _D3(r, g, b)
