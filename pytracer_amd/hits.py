"""Hit-record frames: what ``World.ray_intersection`` (world.py:51-69) returns for every primary ray of
``ImageTracer.fire_all_rays`` (imagetracer.py:60-110), as numpy views over the one buffer ``pt_render_hits`` fills.

Layout (include/ptrace.h): planar, every plane ``[nsamp, rows, W]`` with ``nsamp = max(S, 1)**2`` and sample
``k = sub_row * S + sub_col``; the int32 shape plane first, then the selected fp64 planes.  Nothing here copies: ``point``,
``normal``, ``uv``, ``ray_origin`` and ``ray_dir`` are strided views with the component as LAST axis.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import abi
from .hostmodel import Vec


@dataclass
class Vec2d:
    u: float = 0.0
    v: float = 0.0


@dataclass
class HitRay:
    """The primary ray of a sample (ray.py:29-50 as plain data)."""
    origin: Vec
    dir: Vec
    tmin: float = 1e-5
    tmax: float = float("inf")
    depth: int = 0


@dataclass
class HitRecord:
    """The fields of the reference's ``HitRecord`` (hitrecord.py:27-46) as plain data, plus the index of the shape in
    ``World.shapes`` (the reference carries the shape's material instead: ``HitFrame.materials`` / ``world.shapes[i].material``)."""
    world_point: Vec
    normal: Vec
    surface_point: Vec2d
    t: float
    ray: Optional[HitRay]
    shape_index: int


_CHANNEL_OF = {"t": abi.HIT_T, "point": abi.HIT_POINT, "normal": abi.HIT_NORMAL, "uv": abi.HIT_UV,
               "ray_origin": abi.HIT_RAY, "ray_dir": abi.HIT_RAY}


class HitFrame:
    """Views over a hit-record buffer (``buf``: ``pt_hits_bytes`` bytes, a contiguous ``uint8`` array -- or ``None`` for a
    zeroed one, which tests and host-side producers fill through the views)."""

    def __init__(self, buf, params: abi.Params, channels=abi.HIT_ALL):
        self.channels = abi.hit_channels(channels)
        self.params = abi.copy_params(params)
        S = int(params.samples_per_side)
        self.samples_per_side = S
        self.nsamp = S * S if S > 0 else 1
        self.rows = len(abi.rows_for_rank(params.height, params.row_block, params.n_ranks, params.rank))
        self.width = int(params.width)
        self.nbytes = abi.hits_bytes(params, self.channels)
        if buf is None:
            buf = np.zeros(self.nbytes, dtype=np.uint8)
        buf = np.asarray(buf)
        if buf.dtype != np.uint8 or buf.ndim != 1:
            buf = buf.reshape(-1).view(np.uint8)
        if buf.nbytes < self.nbytes:
            raise ValueError(f"hit-record buffer too small: {buf.nbytes} < {self.nbytes} bytes")
        if not buf.flags.c_contiguous:
            raise ValueError("the hit-record buffer must be contiguous")
        self.buffer = buf
        n = self.nsamp * self.rows * self.width
        self._shape3 = (self.nsamp, self.rows, self.width)
        self.shape_index = buf[: n * 4].view(np.int32).reshape(self._shape3)

    # -- planes -----------------------------------------------------------------------------------------------------------
    def _planes(self, channel: int, first: int, count: int) -> np.ndarray:
        if not self.channels & channel:
            name = next(k for k, v in abi.HIT_NAMES.items() if v == channel)
            raise KeyError(f"channel {name!r} was not selected for this hit frame (channels = {self.channels:#x})")
        n = self.nsamp * self.rows * self.width
        off = abi.hits_plane_offset(self.params, self.channels, channel, first)
        return self.buffer[off: off + n * 8 * count].view(np.float64).reshape((count,) + self._shape3)

    def has(self, name: str) -> bool:
        return bool(self.channels & _CHANNEL_OF[name])

    @property
    def hit(self) -> np.ndarray:
        """``[nsamp, rows, W]`` bool: the sample's ray hit a shape."""
        return self.shape_index >= 0

    @property
    def t(self) -> np.ndarray:
        return self._planes(abi.HIT_T, 0, 1)[0]

    @property
    def point(self) -> np.ndarray:
        return np.moveaxis(self._planes(abi.HIT_POINT, 0, 3), 0, -1)

    @property
    def normal(self) -> np.ndarray:
        return np.moveaxis(self._planes(abi.HIT_NORMAL, 0, 3), 0, -1)

    @property
    def uv(self) -> np.ndarray:
        return np.moveaxis(self._planes(abi.HIT_UV, 0, 2), 0, -1)

    @property
    def ray_origin(self) -> np.ndarray:
        return np.moveaxis(self._planes(abi.HIT_RAY, 0, 3), 0, -1)

    @property
    def ray_dir(self) -> np.ndarray:
        return np.moveaxis(self._planes(abi.HIT_RAY, 3, 3), 0, -1)

    def planes(self) -> dict:
        """name -> view, for every selected channel (what the ``hits`` command writes into its ``.npz``)."""
        out = {"shape_index": self.shape_index}
        for name in ("t", "point", "normal", "uv", "ray_origin", "ray_dir"):
            if self.has(name):
                out[name] = getattr(self, name)
        return out

    # -- scalar access ------------------------------------------------------------------------------------------------------
    def record(self, col: int, row: int, k: int = 0) -> Optional[HitRecord]:
        """The ``HitRecord`` of sample ``k`` of pixel (``col``, local ``row``), or ``None`` on a miss -- what
        ``world.ray_intersection(tracer.fire_ray(col, row, ...))`` returns.  Fields of channels that were not selected are
        zero (``ray``: ``None``)."""
        i = int(self.shape_index[k, row, col])
        if i < 0:
            return None
        f = float

        def vec(name):
            if not self.has(name):
                return Vec(0.0, 0.0, 0.0)
            v = getattr(self, name)[k, row, col]
            return Vec(f(v[0]), f(v[1]), f(v[2]))

        uv = self.uv[k, row, col] if self.has("uv") else (0.0, 0.0)
        ray = HitRay(vec("ray_origin"), vec("ray_dir")) if self.has("ray_origin") else None
        return HitRecord(world_point=vec("point"), normal=vec("normal"), surface_point=Vec2d(f(uv[0]), f(uv[1])),
                         t=f(self.t[k, row, col]) if self.has("t") else 0.0, ray=ray, shape_index=i)

    def materials(self, world) -> np.ndarray:
        """``[nsamp, rows, W]`` object array: ``world.shapes[i].material`` where a shape was hit, ``None`` elsewhere."""
        table = np.empty(len(world.shapes) + 1, dtype=object)
        for i, shape in enumerate(world.shapes):
            table[i] = shape.material
        table[len(world.shapes)] = None
        return table[np.where(self.shape_index >= 0, self.shape_index, len(world.shapes))]
