"""Loader for libptrace_bake.so (include/ptrace_bake.h: surface points from (shape, u, v), and light maps over a shape's
(u, v) grid): its table for ``_addon.Addon``, and its params structure."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_bake.h declares
EXPORTS = ("pt_rays_bake_version", "pt_rays_bake_args_bytes", "pt_rays_bake_last_error", "pt_rays_points_bytes",
           "pt_rays_surface_points_device", "pt_rays_surface_points", "pt_rays_bake_bytes", "pt_rays_bake_plane_offset",
           "pt_rays_bake_workspace_bytes", "pt_rays_bake_device", "pt_rays_bake")

ABI_MAJOR, ABI_MINOR = 1, 5


class BakeParams(C.Structure):
    """``pt_bake_params`` of include/ptrace_bake.h."""
    _fields_ = [("shape", C.c_int), ("side", C.c_int), ("W", C.c_int), ("H", C.c_int), ("col0", C.c_int), ("row0", C.c_int),
                ("w", C.c_int), ("h", C.c_int), ("jitter", C.c_int), ("samples", C.c_int), ("num_of_rays", C.c_int),
                ("max_depth", C.c_int), ("rr_limit", C.c_int), ("depth0", C.c_int), ("init_state", C.c_ulonglong),
                ("init_seq", C.c_ulonglong), ("background", C.c_double * 3)]


def params(shape, side, width, height, window, jitter, samples, num_of_rays, max_depth, rr_limit, depth0, init_state, init_seq,
           background) -> BakeParams:
    """``window``: ``(col0, row0, w, h)``, or ``None`` for the whole map."""
    bg, c_int = _addon.background3(background), _addon.c_int
    mask = 2 ** 64 - 1  # (every value of the 64-bit range is legal and wraps, as pcg_streams has it)
    col0, row0, w, h = (0, 0, width, height) if window is None else window
    return BakeParams(c_int(shape, "shape"), c_int(side, "side"), c_int(width, "width"), c_int(height, "height"), c_int(col0, "window col0"),
                      c_int(row0, "window row0"), c_int(w, "window width"), c_int(h, "window height"), int(bool(jitter)),
                      c_int(samples, "samples"), c_int(num_of_rays, "num_of_rays"), c_int(max_depth, "max_depth"),
                      c_int(rr_limit, "russian_roulette_limit"), c_int(depth0, "depth"), int(init_state) & mask, int(init_seq) & mask, bg)


_vp, _ll, _sz, _i, _pp = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(BakeParams)
_SIGNATURES = (
    ("pt_rays_bake_version", _i, []),
    ("pt_rays_bake_args_bytes", _sz, []),
    ("pt_rays_bake_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_points_bytes", _sz, [_ll]),
    ("pt_rays_surface_points_device", _i, [_i, _vp, _sz, _vp, _vp, _vp, _ll, _vp, _sz, _vp]),
    ("pt_rays_surface_points", _i, [_i, _vp, _sz, _vp, _vp, _vp, _ll, _vp, _sz]),
    ("pt_rays_bake_bytes", _sz, [_ll, _i]),
    ("pt_rays_bake_plane_offset", _ll, [_ll, _i, _i, _i]),
    ("pt_rays_bake_workspace_bytes", _sz, [_i, _pp]),
    ("pt_rays_bake_device", _i, [_i, _vp, _sz, _pp, _i, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_bake", _i, [_i, _vp, _sz, _pp, _i, _vp, _sz]),
)
# PTRACE_BAKE_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_bake.so", "PTRACE_BAKE_LIB", "ray-library interface", "pt_rays_bake_version",
                      "pt_rays_bake_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
