"""Loader for libptrace_motion.so (include/ptrace_motion.h: the weighted accumulation over frames with a motion per shape, so that the
history of a shape that moved is fetched where that surface point was): its table for ``_addon.Addon``, its structures and its tables."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _addon, _temporal_lib, _weighted_lib

# every symbol include/ptrace_motion.h declares
EXPORTS = ("pt_rays_motion_version", "pt_rays_motion_last_error", "pt_rays_motion_bytes", "pt_rays_motion_count_bytes",
           "pt_rays_motion_table_bytes", "pt_rays_motion_clear_device", "pt_rays_motion_accumulate_device", "pt_rays_motion_accumulate")

ABI_MAJOR, ABI_MINOR = 1, 13

MA_SAME_SHAPE, MA_BLEND_WEIGHT = 1, 2  # PT_MA_* of the header
MAX_HISTORY = 2 ** 20
MAX_SHAPES = 2 ** 20
RECORD = 24  # doubles per shape in the motion table: 192 bytes
# the defaults of every Python entry point: the weighted accumulate query's
DEFAULTS = dict(_weighted_lib.DEFAULTS)

# ``pt_motion_params`` has the layout of ``pt_weighted_params``, ``pt_motion_camera`` that of ``pt_temporal_camera``
MotionParams = _weighted_lib.WeightedParams
MotionCamera = _temporal_lib.TemporalCamera
camera = _temporal_lib.camera
flags_of = _weighted_lib.flags_of
params = _weighted_lib.params


def tables(moved, motion):
    """The two tables as the library takes them -> ``(n_shapes, moved int32[n_shapes] or None, motion float64[n_shapes, 24] or
    None)``.  ``None`` for both: nothing moved.  ``motion`` may come as ``[S, 24]`` or flat; its rows are those of ``moved``."""
    if moved is None and motion is None:
        return 0, None, None
    if moved is None or motion is None:
        raise ValueError("moved and motion come together (or neither: nothing moved)")
    moved = np.ascontiguousarray(moved, dtype=np.int32).reshape(-1)
    motion = np.ascontiguousarray(motion, dtype=np.float64)
    if motion.size != moved.shape[0] * RECORD:
        raise ValueError(f"a motion table of {motion.size} values for {moved.shape[0]} shapes: {RECORD} per shape")
    return int(moved.shape[0]), moved, motion.reshape(-1, RECORD)


_vp, _ll, _sz, _i, _pp, _pc = C.c_void_p, C.c_longlong, C.c_size_t, C.c_int, C.POINTER(MotionParams), C.POINTER(MotionCamera)
_SIGNATURES = (
    ("pt_rays_motion_version", _i, []),
    ("pt_rays_motion_last_error", _i, [C.c_char_p, _sz]),
    ("pt_rays_motion_bytes", _sz, [_ll]),
    ("pt_rays_motion_count_bytes", _sz, [_ll]),
    ("pt_rays_motion_table_bytes", _sz, [_i]),
    ("pt_rays_motion_clear_device", _i, [_i, _ll, _vp, _sz, _vp]),
    ("pt_rays_motion_accumulate_device", _i, [_i, _i, _i, _pp, _pc] + [_vp] * 11 + [_i, _vp, _vp] + [_vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    ("pt_rays_motion_accumulate", _i, [_i, _i, _i, _pp, _pc] + [_vp] * 11 + [_i, _vp, _vp] + [_vp, _sz, _vp, _sz, _vp, _sz]),
)
# PTRACE_MOTION_LIB: an alternative build of the same C-ABI library
_ADDON = _addon.Addon("libptrace_motion.so", "PTRACE_MOTION_LIB", "ray-library interface", "pt_rays_motion_version",
                      "pt_rays_motion_last_error", ABI_MAJOR, ABI_MINOR, _SIGNATURES)
lib, lib_path, last_error, check = _ADDON.lib, _ADDON.lib_path, _ADDON.last_error, _ADDON.check
