"""Loader for libptrace_radiance.so (include/ptrace_radiance.h: ``PathTracer.__call__`` for batches of a caller's own rays):
its table for ``_addon.Addon``, and its params structure."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_radiance.h declares
EXPORTS = ("pt_rays_radiance_version", "pt_rays_radiance_args_bytes", "pt_rays_radiance_last_error", "pt_rays_radiance_bytes",
           "pt_rays_radiance_plane_offset", "pt_rays_radiance_workspace_bytes", "pt_rays_radiance_device", "pt_rays_radiance")

ABI_MAJOR, ABI_MINOR = 1, 3


class RadianceParams(C.Structure):
    """``pt_radiance_params`` of include/ptrace_radiance.h."""
    _fields_ = [("num_of_rays", C.c_int), ("max_depth", C.c_int), ("rr_limit", C.c_int), ("depth0", C.c_int),
                ("background", C.c_double * 3)]


def params(num_of_rays, max_depth, rr_limit, depth0, background) -> RadianceParams:
    bg, c_int = _addon.background3(background), _addon.c_int
    return RadianceParams(c_int(num_of_rays, "num_of_rays"), c_int(max_depth, "max_depth"), c_int(rr_limit, "russian_roulette_limit"),
                          c_int(depth0, "depth"), bg)


_vp, _ll, _sz, _i, _pp = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(RadianceParams)
_SIGNATURES = (
    ("pt_rays_radiance_version", _i, []),
    ("pt_rays_radiance_args_bytes", _sz, []),
    ("pt_rays_radiance_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_radiance_bytes", _sz, [_ll, _i]),
    ("pt_rays_radiance_plane_offset", _ll, [_ll, _i, _i, _i]),
    ("pt_rays_radiance_workspace_bytes", _sz, [_i, _ll, _i, _i, _i]),
    ("pt_rays_radiance_device", _i, [_i, _vp, _sz, _vp, _vp, _vp, _vp, _ll, _pp, _i, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_radiance", _i, [_i, _vp, _sz, _vp, _vp, _vp, _ll, _pp, _i, _vp, _sz]),
)
# PTRACE_RADIANCE_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_radiance.so", "PTRACE_RADIANCE_LIB", "ray-library interface", "pt_rays_radiance_version",
                      "pt_rays_radiance_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
