"""Loader for libptrace_lit.so (include/ptrace_lit.h: hit records shaded from a lattice of SH radiance probes): its table for
``_addon.Addon``, and its lattice structure."""
from __future__ import annotations

import ctypes as C

from . import _addon

# every symbol include/ptrace_lit.h declares
EXPORTS = ("pt_rays_lit_version", "pt_rays_lit_args_bytes", "pt_rays_lit_last_error", "pt_rays_lit_bytes", "pt_rays_lit_coeffs_bytes",
           "pt_rays_lit_eval_device", "pt_rays_lit_eval", "pt_rays_lit_shade_device", "pt_rays_lit_shade")

ABI_MAJOR, ABI_MINOR = 1, 7


class LitGrid(C.Structure):
    """``pt_lit_grid`` of include/ptrace_lit.h."""
    _fields_ = [("origin", C.c_double * 3), ("step", C.c_double * 3), ("dims", C.c_int * 3)]


def grid(origin, step, dims) -> LitGrid:
    """``pt_lit_grid`` from three origins, three steps and three counts, as they are: the library checks them."""
    return LitGrid((C.c_double * 3)(*[float(x) for x in origin]), (C.c_double * 3)(*[float(x) for x in step]),
                   (C.c_int * 3)(*[_addon.c_int(x, "dims") for x in dims]))


def rgb(color) -> C.Array:
    """Three doubles from a ``Color`` or three numbers."""
    return _addon.background3(color)


_vp, _ll, _sz, _i, _gp = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(LitGrid)
_d3 = C.POINTER(C.c_double)
_SIGNATURES = (
    ("pt_rays_lit_version", _i, []),
    ("pt_rays_lit_args_bytes", _sz, []),
    ("pt_rays_lit_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_lit_bytes", _sz, [_ll]),
    ("pt_rays_lit_coeffs_bytes", _sz, [_gp]),
    ("pt_rays_lit_eval_device", _i, [_i, _gp, _vp, _sz, _vp, _vp, _vp, _ll, _i, _vp, _sz, _vp]),
    ("pt_rays_lit_eval", _i, [_i, _gp, _vp, _sz, _vp, _vp, _vp, _ll, _i, _vp, _sz]),
    ("pt_rays_lit_shade_device", _i, [_i, _vp, _sz, _vp, _sz, _gp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _ll, _d3, _vp, _sz, _vp]),
    ("pt_rays_lit_shade", _i, [_i, _vp, _sz, _gp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _ll, _d3, _vp, _sz]),
)
# PTRACE_LIT_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_lit.so", "PTRACE_LIT_LIB", "ray-library interface", "pt_rays_lit_version", "pt_rays_lit_last_error",
                      ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
