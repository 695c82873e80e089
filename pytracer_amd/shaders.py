"""Two worked hit shaders: renderers of a user's own that get the GPU for their tracing half.

A *hit shader* is any object with a ``world`` attribute and a method ``shade_hits(frame) -> [nsamp, H, W, 3]``:
``GpuImageTracer.fire_all_rays(shader)`` renders the hit-record frame of its camera on the device
(:class:`pytracer_amd.hits.HitFrame`: what ``world.ray_intersection`` returns for every primary ray), calls ``shade_hits``
once, and reduces the samples the way imagetracer.py:83-101 does.  ``hit_channels`` (optional) names the planes it reads.

Each shader below is ALSO a plain ``Ray -> Color`` callable, as every renderer of the reference is (render.py:36-39), so
that the two routes can be compared: ``__call__(ray)`` is ``shade_record(self.world.ray_intersection(ray))`` -- it needs a
world that can intersect rays (pytracer's ``World``; the parameter holders of :mod:`pytracer_amd.hostmodel` cannot) -- and
``shade_hits`` is the numpy form of the same arithmetic, operation for operation, so both give the same bits.
"""
from __future__ import annotations

import numpy as np

from . import abi
from .hostmodel import BLACK, Color


class _HitShader:
    hit_channels = abi.HIT_ALL

    def __init__(self, world, background_color: Color = BLACK):
        self.world = world
        self.background_color = background_color

    def shade_record(self, record) -> Color:  # pragma: no cover  (abstract)
        raise NotImplementedError

    def __call__(self, ray) -> Color:
        intersect = getattr(self.world, "ray_intersection", None)
        if not callable(intersect):
            raise TypeError(f"{type(self.world).__name__} has no ray_intersection(ray): it is a parameter holder that cannot "
                            f"trace a ray.  Hand {type(self).__name__} to GpuImageTracer.fire_all_rays (the device traces), or "
                            "give it a pytracer World")
        return self.shade_record(intersect(ray))

    def _background(self, frame) -> np.ndarray:
        bg = self.background_color
        out = np.empty(frame.shape_index.shape + (3,), dtype=np.float64)
        out[...] = (bg.r, bg.g, bg.b)
        return out


class NormalShader(_HitShader):
    """The surface normal as a colour, ``0.5 n + 0.5`` per component; the background colour where nothing is hit."""

    hit_channels = abi.HIT_NORMAL

    def shade_record(self, record) -> Color:
        if record is None:
            return self.background_color
        n = record.normal
        return Color(0.5 * n.x + 0.5, 0.5 * n.y + 0.5, 0.5 * n.z + 0.5)

    def shade_hits(self, frame) -> np.ndarray:
        out = self._background(frame)
        hit = frame.hit
        out[hit] = 0.5 * frame.normal[hit] + 0.5
        return out


class DepthShader(_HitShader):
    """Grey by distance: 1 at ``t <= near`` falling linearly to 0 at ``t >= far``; the background colour on a miss."""

    hit_channels = abi.HIT_T

    def __init__(self, world, near: float = 0.0, far: float = 10.0, background_color: Color = BLACK):
        super().__init__(world, background_color)
        if not far > near:
            raise ValueError("far must be larger than near")
        self.near, self.far = float(near), float(far)

    def shade_record(self, record) -> Color:
        if record is None:
            return self.background_color
        d = (record.t - self.near) / (self.far - self.near)
        g = 1.0 - min(max(d, 0.0), 1.0)
        return Color(g, g, g)

    def shade_hits(self, frame) -> np.ndarray:
        out = self._background(frame)
        hit = frame.hit
        d = (frame.t[hit] - self.near) / (self.far - self.near)
        g = 1.0 - np.minimum(np.maximum(d, 0.0), 1.0)
        out[hit] = g[:, None]
        return out
