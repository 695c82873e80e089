"""Loader for libptrace_gather.so (include/ptrace_gather.h: the mean radiance over the hemisphere of batches of surface
points): its table for ``_addon.Addon``, and its params structure."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_gather.h declares
EXPORTS = ("pt_rays_gather_version", "pt_rays_gather_args_bytes", "pt_rays_gather_last_error", "pt_rays_gather_bytes",
           "pt_rays_gather_plane_offset", "pt_rays_gather_workspace_bytes", "pt_rays_gather_device", "pt_rays_gather")

ABI_MAJOR, ABI_MINOR = 1, 4


class GatherParams(C.Structure):
    """``pt_gather_params`` of include/ptrace_gather.h."""
    _fields_ = [("samples", C.c_int), ("num_of_rays", C.c_int), ("max_depth", C.c_int), ("rr_limit", C.c_int), ("depth0", C.c_int),
                ("init_state", C.c_ulonglong), ("init_seq", C.c_ulonglong), ("background", C.c_double * 3)]


def params(samples, num_of_rays, max_depth, rr_limit, depth0, init_state, init_seq, background) -> GatherParams:
    bg, c_int = _addon.background3(background), _addon.c_int
    mask = 2 ** 64 - 1  # (every value of the 64-bit range is legal and wraps, as pcg_streams has it)
    return GatherParams(c_int(samples, "samples"), c_int(num_of_rays, "num_of_rays"), c_int(max_depth, "max_depth"),
                        c_int(rr_limit, "russian_roulette_limit"), c_int(depth0, "depth"), int(init_state) & mask, int(init_seq) & mask, bg)


_vp, _ll, _sz, _i, _pp = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(GatherParams)
_SIGNATURES = (
    ("pt_rays_gather_version", _i, []),
    ("pt_rays_gather_args_bytes", _sz, []),
    ("pt_rays_gather_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_gather_bytes", _sz, [_ll, _i]),
    ("pt_rays_gather_plane_offset", _ll, [_ll, _i, _i, _i]),
    ("pt_rays_gather_workspace_bytes", _sz, [_i, _ll, _i, _i, _i, _i]),
    ("pt_rays_gather_device", _i, [_i, _vp, _sz, _vp, _vp, _vp, _vp, _ll, _pp, _i, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_gather", _i, [_i, _vp, _sz, _vp, _vp, _vp, _vp, _ll, _pp, _i, _vp, _sz]),
)
# PTRACE_GATHER_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_gather.so", "PTRACE_GATHER_LIB", "ray-library interface", "pt_rays_gather_version",
                      "pt_rays_gather_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
