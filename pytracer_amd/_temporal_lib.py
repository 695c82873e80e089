"""Loader for libptrace_temporal.so (include/ptrace_temporal.h: last frame's radiance reprojected onto this frame's hits): its table
for ``_addon.Addon``, and its two structures."""
from __future__ import annotations

import ctypes as C

from . import _addon, abi

# every symbol include/ptrace_temporal.h declares
EXPORTS = ("pt_rays_temporal_version", "pt_rays_temporal_last_error", "pt_rays_temporal_bytes", "pt_rays_temporal_count_bytes",
           "pt_rays_temporal_clear_device", "pt_rays_temporal_accumulate_device", "pt_rays_temporal_accumulate")

ABI_MAJOR, ABI_MINOR = 1, 9

TA_SAME_SHAPE = 1  # PT_TA_* of the header
MAX_HISTORY = 2 ** 20
# the defaults of every Python entry point (``point_tolerance`` is in world units: the distance from the pixel's tangent plane)
DEFAULTS = dict(max_history=32, same_shape=True, normal_min=0.9, point_tolerance=0.05)


class TemporalParams(C.Structure):
    """``pt_temporal_params`` of include/ptrace_temporal.h."""
    _fields_ = [("max_history", C.c_int), ("flags", C.c_int), ("normal_min", C.c_double), ("point_tolerance", C.c_double)]


class TemporalCamera(C.Structure):
    """``pt_temporal_camera`` of include/ptrace_temporal.h: the camera the previous frame was seen from."""
    _fields_ = [("kind", C.c_int), ("invm", C.c_double * 12), ("screen_distance", C.c_double), ("aspect_ratio", C.c_double)]


def flags_of(same_shape=True, flags=None) -> int:
    """The ``PT_TA_*`` bits of a boolean; ``flags=`` (an int) is passed as it is, for the library to check."""
    if flags is not None:
        return _addon.c_int(flags, "flags")
    return TA_SAME_SHAPE if same_shape else 0


def params(max_history=32, same_shape=True, normal_min=0.9, point_tolerance=0.05, flags=None) -> TemporalParams:
    """``pt_temporal_params`` from the values as they are: the library checks them."""
    return TemporalParams(_addon.c_int(max_history, "max_history"), flags_of(same_shape, flags), float(normal_min), float(point_tolerance))


def camera(cam) -> TemporalCamera:
    """``pt_temporal_camera`` of a camera object (a ``PerspectiveCamera`` or an ``OrthogonalCamera`` with ``transformation.invm``,
    ``aspect_ratio`` and, for the first, ``screen_distance``), of ``(kind, invm12, screen_distance, aspect_ratio)`` as they are, or
    of a :class:`TemporalCamera` (returned as it is)."""
    if isinstance(cam, TemporalCamera):
        return cam
    if isinstance(cam, (tuple, list)):
        kind, invm, distance, aspect = cam
        invm = [float(x) for x in invm]
        if len(invm) != 12:
            raise ValueError(f"invm holds rows 0..2 of a 4x4 matrix: 12 numbers, not {len(invm)}")
        return TemporalCamera(_addon.c_int(kind, "kind"), (C.c_double * 12)(*invm), float(distance), float(aspect))
    from . import flatten

    name = type(cam).__name__
    invm = flatten._affine12(cam.transformation.invm, "camera transformation.invm")
    if name == "PerspectiveCamera":
        return TemporalCamera(abi.CAMERA_PERSPECTIVE, (C.c_double * 12)(*invm), float(cam.screen_distance), float(cam.aspect_ratio))
    if name == "OrthogonalCamera":
        return TemporalCamera(abi.CAMERA_ORTHOGONAL, (C.c_double * 12)(*invm), 1.0, float(cam.aspect_ratio))
    raise flatten.UnsupportedSceneError(f"unknown camera class {name!r}")


_vp, _ll, _sz, _i, _pp, _pc = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalCamera)
_SIGNATURES = (
    ("pt_rays_temporal_version", _i, []),
    ("pt_rays_temporal_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_temporal_bytes", _sz, [_ll]),
    ("pt_rays_temporal_count_bytes", _sz, [_ll]),
    ("pt_rays_temporal_clear_device", _i, [_i, _ll, _vp, _sz, _vp]),
    ("pt_rays_temporal_accumulate_device", _i, [_i, _i, _i, _pp, _pc] + [_vp] * 9 + [_vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_temporal_accumulate", _i, [_i, _i, _i, _pp, _pc] + [_vp] * 9 + [_vp, _sz, _vp, _sz]),
)
# PTRACE_TEMPORAL_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_temporal.so", "PTRACE_TEMPORAL_LIB", "ray-library interface", "pt_rays_temporal_version",
                      "pt_rays_temporal_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
