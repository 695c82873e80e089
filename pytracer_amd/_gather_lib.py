"""Loader for libptrace_gather.so (include/ptrace_gather.h: the mean radiance over the hemisphere of batches of surface points).

Like the other add-ons the library links to nothing of the project's and loads nothing itself: it is handed the scene's
argument block (``_rays_lib.scene_args``; all six libraries come from one build of the tree, and each refuses a block of
another size).  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

# PTRACE_GATHER_LIB: an alternative build of the same C-ABI library (mutation runs; as PTRACE_RADIANCE_LIB for libptrace_radiance.so)
_LIB_PATH = os.environ.get("PTRACE_GATHER_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libptrace_gather.so")
_gat = None

# every symbol include/ptrace_gather.h declares
EXPORTS = ("pt_rays_gather_version", "pt_rays_gather_args_bytes", "pt_rays_gather_last_error", "pt_rays_gather_bytes",
           "pt_rays_gather_plane_offset", "pt_rays_gather_workspace_bytes", "pt_rays_gather_device", "pt_rays_gather")

ABI_MAJOR, ABI_MINOR = 1, 4


class GatherParams(C.Structure):
    """``pt_gather_params`` of include/ptrace_gather.h."""
    _fields_ = [("samples", C.c_int), ("num_of_rays", C.c_int), ("max_depth", C.c_int), ("rr_limit", C.c_int), ("depth0", C.c_int),
                ("init_state", C.c_ulonglong), ("init_seq", C.c_ulonglong), ("background", C.c_double * 3)]


def params(samples, num_of_rays, max_depth, rr_limit, depth0, init_state, init_seq, background) -> GatherParams:
    bg = (background.r, background.g, background.b) if hasattr(background, "r") else tuple(background)
    if len(bg) != 3:
        raise ValueError("background must be a Color or three numbers")

    def c_int(x, what):
        x = int(x)
        if not -2 ** 31 <= x < 2 ** 31:
            raise ValueError(f"{what}={x} does not fit a C int")
        return x

    mask = 2 ** 64 - 1  # (every value of the 64-bit range is legal and wraps, as pcg_streams has it)
    return GatherParams(c_int(samples, "samples"), c_int(num_of_rays, "num_of_rays"), c_int(max_depth, "max_depth"),
                        c_int(rr_limit, "russian_roulette_limit"), c_int(depth0, "depth"), int(init_state) & mask, int(init_seq) & mask,
                        (C.c_double * 3)(*[float(x) for x in bg]))


def lib_path() -> str:
    return _LIB_PATH


def lib():
    """The loaded library; raises if it has not been built (``python -m pytracer_amd.build``)."""
    global _gat
    if _gat is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} is missing: the HIP extension has not been built. "
                              "Run `python -m pytracer_amd.build` (needs hipcc); there is no CPU fallback.")
        _lib.lib()  # first: ONE HIP runtime per process, the one libptrace.so bound to (shared with torch unless standalone())
        L = C.CDLL(_LIB_PATH)
        vp, ll, sz, i = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int
        pp = C.POINTER(GatherParams)
        L.pt_rays_gather_version.restype, L.pt_rays_gather_version.argtypes = i, []
        L.pt_rays_gather_args_bytes.restype, L.pt_rays_gather_args_bytes.argtypes = sz, []
        L.pt_rays_gather_last_error.restype, L.pt_rays_gather_last_error.argtypes = i, [C.c_char_p, sz]
        L.pt_rays_gather_bytes.restype, L.pt_rays_gather_bytes.argtypes = sz, [ll, i]
        L.pt_rays_gather_plane_offset.restype, L.pt_rays_gather_plane_offset.argtypes = ll, [ll, i, i, i]
        L.pt_rays_gather_workspace_bytes.restype, L.pt_rays_gather_workspace_bytes.argtypes = sz, [i, ll, i, i, i, i]
        L.pt_rays_gather_device.restype = i
        L.pt_rays_gather_device.argtypes = [i, vp, sz, vp, vp, vp, vp, ll, pp, i, vp, sz, vp, sz, vp]
        L.pt_rays_gather.restype = i
        L.pt_rays_gather.argtypes = [i, vp, sz, vp, vp, vp, vp, ll, pp, i, vp, sz]
        ver = int(L.pt_rays_gather_version())
        if ver >> 16 != ABI_MAJOR or (ver & 0xFFFF) < ABI_MINOR:
            raise ImportError(f"{_LIB_PATH} implements ray-library interface {ver >> 16}.{ver & 0xFFFF}; this package needs "
                              f"{ABI_MAJOR}.{ABI_MINOR} or later: rebuild with `python -m pytracer_amd.build --force`")
        _gat = L
    return _gat


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().pt_rays_gather_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != 0:
        raise _lib.PtraceError(rc, last_error())
