"""Loader for libptrace_rays.so (include/ptrace_rays.h: closest-hit and any-hit queries for a caller's own rays).

The add-on library has no link dependency on libptrace.so and loads nothing itself: this module hands it the scene's
argument block, which ``_lib``'s ``pt_scene_kernel_args`` fills (``scene_args``).  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

# PTRACE_RAYS_LIB: an alternative build of the same C-ABI library (mutation runs; as PTRACE_LIB for libptrace.so)
_LIB_PATH = os.environ.get("PTRACE_RAYS_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libptrace_rays.so")
_rays = None

# every symbol include/ptrace_rays.h declares
EXPORTS = ("pt_rays_version", "pt_rays_args_bytes", "pt_rays_bytes", "pt_rays_plane_offset", "pt_rays_trace_device",
           "pt_rays_trace", "pt_rays_last_error")

ABI_MAJOR = 1


def lib_path() -> str:
    return _LIB_PATH


def lib():
    """The loaded library; raises if it has not been built (``python -m pytracer_amd.build``)."""
    global _rays
    if _rays is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} is missing: the HIP extension has not been built. "
                              "Run `python -m pytracer_amd.build` (needs hipcc); there is no CPU fallback.")
        _lib.lib()  # first: ONE HIP runtime per process, the one libptrace.so bound to (shared with torch unless standalone())
        L = C.CDLL(_LIB_PATH)
        L.pt_rays_version.restype = C.c_int
        L.pt_rays_version.argtypes = []
        L.pt_rays_args_bytes.restype = C.c_size_t
        L.pt_rays_args_bytes.argtypes = []
        L.pt_rays_bytes.restype = C.c_size_t
        L.pt_rays_bytes.argtypes = [C.c_longlong, C.c_int, C.c_int]
        L.pt_rays_plane_offset.restype = C.c_longlong
        L.pt_rays_plane_offset.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int]
        L.pt_rays_trace_device.restype = C.c_int
        L.pt_rays_trace_device.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_void_p]
        L.pt_rays_trace.restype = C.c_int
        L.pt_rays_trace.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        L.pt_rays_last_error.restype = C.c_int
        L.pt_rays_last_error.argtypes = [C.c_char_p, C.c_size_t]
        ver = int(L.pt_rays_version())
        if ver >> 16 != ABI_MAJOR:
            raise ImportError(f"{_LIB_PATH} implements ray-batch ABI {ver >> 16}.{ver & 0xFFFF}; this package needs {ABI_MAJOR}.x: "
                              "rebuild with `python -m pytracer_amd.build --force`")
        _rays = L
    return _rays


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().pt_rays_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != 0:
        raise _lib.PtraceError(rc, last_error())


def scene_args(handle) -> C.Array:
    """The scene's argument block (``pt_scene_kernel_args`` of libptrace.so) as the bytes ``pt_rays_trace*`` take.  Sized by
    THIS library's ``pt_rays_args_bytes``: two libraries from different builds disagree here, loudly."""
    block = C.create_string_buffer(int(lib().pt_rays_args_bytes()))
    _lib.check(_lib.lib().pt_scene_kernel_args(handle, block, len(block)))
    return block
