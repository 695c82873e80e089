"""Loader for libptrace_scatter.so (include/ptrace_scatter.h: BRDF.scatter_ray and the Russian roulette for hit records).

Like the other two add-ons the library links to nothing of the project's and loads nothing itself: it is handed the scene's
argument block (``_rays_lib.scene_args``; all four libraries come from one build of the tree, and each refuses a block of
another size) and the slot table ``_surface_lib`` makes.  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

# PTRACE_SCATTER_LIB: an alternative build of the same C-ABI library (mutation runs; as PTRACE_SURFACE_LIB for libptrace_surface.so)
_LIB_PATH = os.environ.get("PTRACE_SCATTER_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libptrace_scatter.so")
_scat = None

# every symbol include/ptrace_scatter.h declares
EXPORTS = ("pt_rays_scatter_version", "pt_rays_scatter_args_bytes", "pt_rays_scatter_last_error", "pt_rays_scatter_bytes",
           "pt_rays_scatter_plane_offset", "pt_rays_scatter_device", "pt_rays_scatter")

ABI_MAJOR, ABI_MINOR = 1, 2


def lib_path() -> str:
    return _LIB_PATH


def lib():
    """The loaded library; raises if it has not been built (``python -m pytracer_amd.build``)."""
    global _scat
    if _scat is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} is missing: the HIP extension has not been built. "
                              "Run `python -m pytracer_amd.build` (needs hipcc); there is no CPU fallback.")
        _lib.lib()  # first: ONE HIP runtime per process, the one libptrace.so bound to (shared with torch unless standalone())
        L = C.CDLL(_LIB_PATH)
        vp, ll, sz, i = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int
        L.pt_rays_scatter_version.restype, L.pt_rays_scatter_version.argtypes = i, []
        L.pt_rays_scatter_args_bytes.restype, L.pt_rays_scatter_args_bytes.argtypes = sz, []
        L.pt_rays_scatter_last_error.restype, L.pt_rays_scatter_last_error.argtypes = i, [C.c_char_p, sz]
        L.pt_rays_scatter_bytes.restype, L.pt_rays_scatter_bytes.argtypes = sz, [ll, i]
        L.pt_rays_scatter_plane_offset.restype, L.pt_rays_scatter_plane_offset.argtypes = ll, [ll, i, i, i]
        L.pt_rays_scatter_device.restype = i
        L.pt_rays_scatter_device.argtypes = [i, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, ll, i, i, vp, sz, vp]
        L.pt_rays_scatter.restype = i
        L.pt_rays_scatter.argtypes = [i, vp, sz, vp, vp, vp, vp, vp, vp, vp, ll, i, i, vp, sz]
        ver = int(L.pt_rays_scatter_version())
        if ver >> 16 != ABI_MAJOR or (ver & 0xFFFF) < ABI_MINOR:
            raise ImportError(f"{_LIB_PATH} implements ray-library interface {ver >> 16}.{ver & 0xFFFF}; this package needs "
                              f"{ABI_MAJOR}.{ABI_MINOR} or later: rebuild with `python -m pytracer_amd.build --force`")
        _scat = L
    return _scat


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().pt_rays_scatter_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != 0:
        raise _lib.PtraceError(rc, last_error())
