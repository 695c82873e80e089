"""Loader for libptrace_rays.so (include/ptrace_rays.h: closest-hit and any-hit queries for a caller's own rays): its table
for ``_addon.Addon``, and ``scene_args``, the scene's argument block every add-on is handed."""
from __future__ import annotations

import ctypes as C

from . import _addon, _lib

# every symbol include/ptrace_rays.h declares
EXPORTS = ("pt_rays_version", "pt_rays_args_bytes", "pt_rays_bytes", "pt_rays_plane_offset", "pt_rays_trace_device",
           "pt_rays_trace", "pt_rays_last_error")

ABI_MAJOR = 1

_vp, _ll, _sz, _i = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int
_SIGNATURES = (
    ("pt_rays_version", _i, []),
    ("pt_rays_args_bytes", _sz, []),
    ("pt_rays_bytes", _sz, [_ll, _i, _i]),
    ("pt_rays_plane_offset", _ll, [_ll, _i, _i, _i, _i]),
    ("pt_rays_trace_device", _i, [_i, _vp, _sz, _vp, _ll, _i, _i, _vp, _sz, _vp]),
    ("pt_rays_trace", _i, [_i, _vp, _sz, _vp, _ll, _i, _i, _vp, _sz]),
    ("pt_rays_last_error", _i, [C.c_char_p, _sz]),
)
# PTRACE_RAYS_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_rays.so", "PTRACE_RAYS_LIB", "ray-batch ABI", "pt_rays_version", "pt_rays_last_error", ABI_MAJOR, 0,
                      _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check


def scene_args(handle) -> C.Array:
    """The scene's argument block (``pt_scene_kernel_args`` of libptrace.so) as the bytes ``pt_rays_trace*`` take.  Sized by
    THIS library's ``pt_rays_args_bytes``: two libraries from different builds disagree here, loudly."""
    block = C.create_string_buffer(int(lib().pt_rays_args_bytes()))
    _lib.check(_lib.lib().pt_scene_kernel_args(handle, block, len(block)))
    return block
