"""Loader for libptrace_sh.so (include/ptrace_sh.h: order-2 spherical-harmonic radiance probes at free points, and their
evaluation): its table for ``_addon.Addon``, and its params structure."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_sh.h declares
EXPORTS = ("pt_rays_sh_version", "pt_rays_sh_args_bytes", "pt_rays_sh_last_error", "pt_rays_sh_dirs_bytes",
           "pt_rays_sh_directions_device", "pt_rays_sh_directions", "pt_rays_sh_bytes", "pt_rays_sh_plane_offset",
           "pt_rays_sh_workspace_bytes", "pt_rays_sh_project_device", "pt_rays_sh_project", "pt_rays_sh_eval_bytes",
           "pt_rays_sh_eval_device", "pt_rays_sh_eval")

ABI_MAJOR, ABI_MINOR = 1, 6


class ShParams(C.Structure):
    """``pt_sh_params`` of include/ptrace_sh.h."""
    _fields_ = [("samples", C.c_int), ("num_of_rays", C.c_int), ("max_depth", C.c_int), ("rr_limit", C.c_int), ("depth0", C.c_int),
                ("init_state", C.c_ulonglong), ("init_seq", C.c_ulonglong), ("background", C.c_double * 3)]


def params(samples, num_of_rays=1, max_depth=10, rr_limit=3, depth0=1, init_state=42, init_seq=54, background=(0.0, 0.0, 0.0)) -> ShParams:
    bg, c_int = _addon.background3(background), _addon.c_int
    mask = 2 ** 64 - 1  # (every value of the 64-bit range is legal and wraps, as pcg_streams has it)
    return ShParams(c_int(samples, "samples"), c_int(num_of_rays, "num_of_rays"), c_int(max_depth, "max_depth"),
                    c_int(rr_limit, "russian_roulette_limit"), c_int(depth0, "depth"), int(init_state) & mask, int(init_seq) & mask, bg)


_vp, _ll, _sz, _i, _pp = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(ShParams)
_SIGNATURES = (
    ("pt_rays_sh_version", _i, []),
    ("pt_rays_sh_args_bytes", _sz, []),
    ("pt_rays_sh_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_sh_dirs_bytes", _sz, [_ll, _i]),
    ("pt_rays_sh_directions_device", _i, [_i, _vp, _ll, _pp, _vp, _sz, _vp]),
    ("pt_rays_sh_directions", _i, [_i, _vp, _ll, _pp, _vp, _sz]),
    ("pt_rays_sh_bytes", _sz, [_ll, _i]),
    ("pt_rays_sh_plane_offset", _ll, [_ll, _i, _i, _i]),
    ("pt_rays_sh_workspace_bytes", _sz, [_i, _ll, _pp]),
    ("pt_rays_sh_project_device", _i, [_i, _vp, _sz, _vp, _vp, _vp, _ll, _pp, _i, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_sh_project", _i, [_i, _vp, _sz, _vp, _vp, _vp, _ll, _pp, _i, _vp, _sz]),
    ("pt_rays_sh_eval_bytes", _sz, [_ll]),
    ("pt_rays_sh_eval_device", _i, [_i, _vp, _ll, _vp, _vp, _ll, _i, _vp, _sz, _vp]),
    ("pt_rays_sh_eval", _i, [_i, _vp, _ll, _vp, _vp, _ll, _i, _vp, _sz]),
)
# PTRACE_SH_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_sh.so", "PTRACE_SH_LIB", "ray-library interface", "pt_rays_sh_version", "pt_rays_sh_last_error",
                      ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
