"""Loader for libptrace_surface.so (include/ptrace_surface.h: the material and the point-light shading of hit records).

Like libptrace_rays.so the library links to nothing of the project's and loads nothing itself: it is handed the scene's
argument block (``_rays_lib.scene_args``; all three libraries come from one build of the tree, and each refuses a block of
another size).  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

# PTRACE_SURFACE_LIB: an alternative build of the same C-ABI library (mutation runs; as PTRACE_RAYS_LIB for libptrace_rays.so)
_LIB_PATH = os.environ.get("PTRACE_SURFACE_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libptrace_surface.so")
_surf = None

# every symbol include/ptrace_surface.h declares
EXPORTS = ("pt_rays_surface_version", "pt_rays_surface_args_bytes", "pt_rays_surface_last_error", "pt_rays_slots_bytes",
           "pt_rays_slots_device", "pt_rays_surface_bytes", "pt_rays_surface_plane_offset", "pt_rays_surface_device",
           "pt_rays_surface", "pt_rays_shade_lights_device", "pt_rays_shade_lights")

ABI_MAJOR = 1
_D3 = C.c_double * 3


def lib_path() -> str:
    return _LIB_PATH


def lib():
    """The loaded library; raises if it has not been built (``python -m pytracer_amd.build``)."""
    global _surf
    if _surf is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} is missing: the HIP extension has not been built. "
                              "Run `python -m pytracer_amd.build` (needs hipcc); there is no CPU fallback.")
        _lib.lib()  # first: ONE HIP runtime per process, the one libptrace.so bound to (shared with torch unless standalone())
        L = C.CDLL(_LIB_PATH)
        vp, ll, sz, i = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int
        L.pt_rays_surface_version.restype, L.pt_rays_surface_version.argtypes = i, []
        L.pt_rays_surface_args_bytes.restype, L.pt_rays_surface_args_bytes.argtypes = sz, []
        L.pt_rays_surface_last_error.restype, L.pt_rays_surface_last_error.argtypes = i, [C.c_char_p, sz]
        L.pt_rays_slots_bytes.restype, L.pt_rays_slots_bytes.argtypes = sz, [vp, sz]
        L.pt_rays_slots_device.restype, L.pt_rays_slots_device.argtypes = i, [i, vp, sz, vp, sz, vp]
        L.pt_rays_surface_bytes.restype, L.pt_rays_surface_bytes.argtypes = sz, [ll, i]
        L.pt_rays_surface_plane_offset.restype, L.pt_rays_surface_plane_offset.argtypes = ll, [ll, i, i, i]
        L.pt_rays_surface_device.restype = i
        L.pt_rays_surface_device.argtypes = [i, vp, sz, vp, vp, vp, ll, i, vp, sz, vp]
        L.pt_rays_surface.restype = i
        L.pt_rays_surface.argtypes = [i, vp, sz, vp, vp, ll, i, vp, sz]
        L.pt_rays_shade_lights_device.restype = i
        L.pt_rays_shade_lights_device.argtypes = [i, vp, sz, vp, vp, vp, vp, vp, vp, ll, vp, vp, vp, sz, vp]
        L.pt_rays_shade_lights.restype = i
        L.pt_rays_shade_lights.argtypes = [i, vp, sz, vp, vp, vp, vp, vp, ll, vp, vp, vp, sz]
        ver = int(L.pt_rays_surface_version())
        if ver >> 16 != ABI_MAJOR:
            raise ImportError(f"{_LIB_PATH} implements ray-library interface {ver >> 16}.{ver & 0xFFFF}; this package needs {ABI_MAJOR}.x: "
                              "rebuild with `python -m pytracer_amd.build --force`")
        _surf = L
    return _surf


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().pt_rays_surface_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != 0:
        raise _lib.PtraceError(rc, last_error())


def rgb(color) -> C.Array:
    """Three doubles for the ``ambient`` / ``background`` arguments, from an (r, g, b) sequence or a ``Color``."""
    if hasattr(color, "r"):
        color = (color.r, color.g, color.b)
    r, g, b = (float(x) for x in color)
    return _D3(r, g, b)
