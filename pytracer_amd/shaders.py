"""Three worked hit shaders: renderers of a user's own that get the GPU for their tracing half.

A *hit shader* is any object with a ``world`` attribute and a method ``shade_hits(frame) -> [nsamp, H, W, 3]``:
``GpuImageTracer.fire_all_rays(shader)`` renders the hit-record frame of its camera on the device
(:class:`pytracer_amd.hits.HitFrame`: what ``world.ray_intersection`` returns for every primary ray), calls ``shade_hits``
once, and reduces the samples the way imagetracer.py:83-101 does.  ``hit_channels`` (optional) names the planes it reads.

Each shader below is ALSO a plain ``Ray -> Color`` callable, as every renderer of the reference is (render.py:36-39), so
that the two routes can be compared: ``__call__(ray)`` is ``shade_record(self.world.ray_intersection(ray))`` -- it needs a
world that can intersect rays (pytracer's ``World``; the parameter holders of :mod:`pytracer_amd.hostmodel` cannot) -- and
``shade_hits`` is the numpy form of the same arithmetic, operation for operation, so both give the same bits.

:class:`PointLightShader` is the reference's ``PointLightRenderer`` (render.py:157-193) put together from the public pieces:
trace (the hit-record frame), then shade (``WorldQueries.point_light_radiance``: materials, shadow rays and the light sum on
the device), with nothing but arrays in between.
"""
from __future__ import annotations

import math

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


def pigment_color(pigment, uv) -> Color:
    """``pigment.get_color(uv)`` (materials.py:50-100) for a pigment that may be a parameter holder (hostmodel): by its
    fields, as :mod:`pytracer_amd.flatten` reads them."""
    name = type(pigment).__name__
    if name == "UniformPigment":
        return pigment.color
    if name == "CheckeredPigment":
        iu, iv = int(math.floor(uv.u * pigment.num_of_steps)), int(math.floor(uv.v * pigment.num_of_steps))
        return pigment.color1 if iu % 2 == iv % 2 else pigment.color2
    if name == "ImagePigment":
        image = pigment.image
        col, row = min(int(uv.u * image.width), image.width - 1), min(int(uv.v * image.height), image.height - 1)
        return image.get_pixel(col, row)
    raise TypeError(f"unknown pigment class {name!r}")


def _unit(x, y, z):
    n = math.sqrt(x * x + y * y + z * z)
    return x / n, y / n, z / n


def _normalized_dot(a, b) -> float:
    (ax, ay, az), (bx, by, bz) = _unit(*a), _unit(*b)
    return ax * bx + ay * by + az * bz


class PointLightShader(_HitShader):
    """``PointLightRenderer`` (render.py:157-193) as a hit shader: ``background_color`` where nothing is hit, else
    ``ambient_color`` + emitted + one term per point light the hit point sees.  ``tracer``: the ``GpuImageTracer`` whose cached
    device scene answers (``tracer.world_queries(world)``); it may be ``None`` for a shader that is only ever called ray by ray.

    ``__call__(ray)`` is the same arithmetic in Python floats with ``x * x`` for ``x**2`` (what the device multiplies;
    SURVEY.md H2), on a world that has ``ray_intersection(ray)`` and ``is_point_visible(point, observer_pos)``; the record's
    material is ``record.material`` or ``world.shapes[record.shape_index].material``."""

    hit_channels = abi.HIT_ALL

    def __init__(self, world, tracer=None, background_color: Color = BLACK, ambient_color: Color = None):
        super().__init__(world, background_color)
        self.tracer = tracer
        self.ambient_color = ambient_color if ambient_color is not None else Color(0.1, 0.1, 0.1)

    def shade_hits(self, frame) -> np.ndarray:
        if self.tracer is None:
            raise TypeError("PointLightShader.shade_hits needs the tracer whose device scene holds the world: PointLightShader(world, tracer)")
        return self.tracer.world_queries(self.world).point_light_radiance(frame, None, self.ambient_color, self.background_color)

    def __call__(self, ray) -> Color:
        for method in ("ray_intersection", "is_point_visible"):
            if not callable(getattr(self.world, method, None)):
                raise TypeError(f"{type(self.world).__name__} has no {method}: it is a parameter holder that cannot trace a ray.  Hand "
                                "PointLightShader to GpuImageTracer.fire_all_rays (the device traces), or give it a pytracer World")
        return self.shade_record(self.world.ray_intersection(ray), ray)

    def shade_record(self, record, ray) -> Color:
        if record is None:
            return self.background_color
        material = getattr(record, "material", None) or self.world.shapes[record.shape_index].material
        uv, wp, nrm = record.surface_point, record.world_point, record.normal
        em = pigment_color(material.emitted_radiance, uv)
        amb = self.ambient_color
        r, g, b = amb.r + em.r, amb.g + em.g, amb.b + em.b
        brdf = material.brdf
        specular = type(brdf).__name__ == "SpecularBRDF"
        normal, out_dir = (nrm.x, nrm.y, nrm.z), (-ray.dir.x, -ray.dir.y, -ray.dir.z)
        for light in self.world.point_lights:
            lp = light.position
            if not self.world.is_point_visible(point=lp, observer_pos=wp):
                continue
            dx, dy, dz = wp.x - lp.x, wp.y - lp.y, wp.z - lp.z
            dist = math.sqrt(dx * dx + dy * dy + dz * dz)
            inv = 1.0 / dist
            in_dir = (dx * inv, dy * inv, dz * inv)
            cos_theta = max(0.0, _normalized_dot((-in_dir[0], -in_dir[1], -in_dir[2]), normal))
            q = light.linear_radius / dist
            factor = q * q if light.linear_radius > 0 else 1.0
            pc = pigment_color(brdf.pigment, uv)
            if specular:  # materials.py:164-173
                th_in, th_out = math.acos(_normalized_dot(normal, in_dir)), math.acos(_normalized_dot(normal, out_dir))
                bc = (pc.r, pc.g, pc.b) if abs(th_in - th_out) < brdf.threshold_angle_rad else (0.0, 0.0, 0.0)
            else:  # materials.py:129-130
                k = 1.0 / math.pi
                bc = (pc.r * k, pc.g * k, pc.b * k)
            lc = light.color
            r, g, b = r + bc[0] * lc.r * cos_theta * factor, g + bc[1] * lc.g * cos_theta * factor, b + bc[2] * lc.b * cos_theta * factor
        return Color(r, g, b)
