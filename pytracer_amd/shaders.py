"""Five worked hit shaders: renderers of a user's own that get the GPU for their tracing half.

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

:class:`PathTracerShader` is the reference's ``PathTracer`` (render.py:99-139) with one ray per hit, put together the same way:
trace, then per depth scatter (``WorldQueries.scatter``: pigments, Russian roulette and ``brdf.scatter_ray`` on the device, every
sample's generator carried along) and trace again (``WorldQueries.ray_intersections`` on the scattered block), and at the end
the recursion's sums in numpy.

:class:`PathRadianceShader` is ``PathTracer`` with any number of rays per hit: the frame's primary rays go to one radiance
query (``WorldQueries.path_radiance``), which walks every sample's tree depth-first on the device.

:class:`DenoisedGatherShader` trades rays for a guided filter: a few hemisphere rays per hit (``WorldQueries.hemisphere_radiance``),
the edge-avoiding filter of include/ptrace_denoise.h on that mean (``WorldQueries.denoised``), then the material.

:class:`TemporalGatherShader` trades rays for time as well: between the gather and the filter, last frame's accumulated mean is
reprojected onto this frame's hits and blended in (``rays.TemporalAccumulator``; include/ptrace_temporal.h).
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


def sample_streams(pcg, frame) -> np.ndarray:
    """``uint64[2, n]``: the generator of every sample of ``frame`` where its path starts -- sample ``k`` of pixel
    ``i = row * W + col`` owns ``PCG(S0, Q0 + i * S**2 + k)`` with (S0, Q0) the seeds of ``pcg``, entered behind the sample's two
    jitter draws when ``samples_per_side > 0`` (the fused path tracer's ``pcg_mode="sample"``)."""
    from . import flatten
    from .rays import pcg_streams

    s0, q0 = flatten.recover_seeds(pcg, True)
    p = frame.params
    grow = np.asarray(abi.rows_for_rank(p.height, p.row_block, p.n_ranks, p.rank), dtype=np.uint64)
    with np.errstate(over="ignore"):
        pix = grow[:, None] * np.uint64(frame.width) + np.arange(frame.width, dtype=np.uint64)[None, :]
        seq = np.uint64(q0 & (2 ** 64 - 1)) + pix[None] * np.uint64(frame.nsamp) + np.arange(frame.nsamp, dtype=np.uint64)[:, None, None]
    return pcg_streams(s0, seq.reshape(-1), 2 if frame.samples_per_side > 0 else 0)


def _check_sample_streams(shader_name: str, tracer, alternative: str) -> None:
    """The ``pcg_mode`` combinations without a generator per sample, refused in ``PathTracerShader``'s words."""
    if tracer is None:
        return
    mode, S = getattr(tracer, "pcg_mode", "sample"), int(getattr(tracer, "samples_per_side", 0))
    if mode == "seq" or (mode == "auto" and S > 0):  # ("auto" jitters a hit-record frame from the serial stream)
        raise ValueError(f'{shader_name} needs a generator per sample, not pcg_mode="{mode}" (one serial stream for the whole '
                         f'frame): build the tracer with pcg_mode="sample", or {alternative}')
    if mode == "pixel" and S > 1:
        raise ValueError(f'{shader_name} needs a generator per sample, not pcg_mode="pixel" with {S * S} samples (a pixel\'s samples '
                         f'share one stream in program order): build the tracer with pcg_mode="sample", or {alternative}')


class PathTracerShader(_HitShader):
    """``PathTracer`` (render.py:99-139) with ``num_of_rays=1`` as a hit shader, breadth-first: all samples of the frame take
    their first bounce together, then their second, ... down to ``max_depth``; then the recursion unwinds in numpy with the
    reference's own operations, ``cum = 0.0 + weight * child`` and ``emitted + cum * (1.0 / num_of_rays)`` (black beyond
    ``max_depth``, ``background_color`` on a miss, ``emitted`` where the roulette ends a path).

    Streams: sample ``k`` of pixel ``i = row * W + col`` owns ``PCG(S0, Q0 + i * S**2 + k)`` with (S0, Q0) the seeds of ``pcg``,
    entered behind the sample's two jitter draws when ``samples_per_side > 0`` -- the fused path tracer's ``pcg_mode="sample"``
    (csrc/pt_path.h: path_start_sample, path_seed_round).  Handed to a ``GpuImageTracer(..., pcg=PCG(S0, Q0),
    pcg_mode="sample")`` -- the tracer's generator jitters the hit-record frame, so it has to have this shader's seeds -- the
    frame is the one ``fire_all_rays(PathTracer(world, background_color, PCG(S0, Q0), 1, max_depth, limit))`` renders, byte
    for byte.

    What cannot be walked breadth-first is refused with a ``ValueError`` that names the alternative: ``num_of_rays != 1`` (the
    children of a hit draw from ONE stream depth-first), a tracer with ``pcg_mode="seq"`` (one serial stream for the whole
    frame) and ``pcg_mode="pixel"`` with more than one sample (a pixel's samples share a stream in program order).

    ``__call__(ray)`` is the same arithmetic ray by ray, drawing from ``pcg`` itself, on a world that can intersect."""

    hit_channels = abi.HIT_ALL
    _ALTERNATIVE = ("hand the fused renderer to the tracer instead: GpuImageTracer.fire_all_rays(PathTracer(world, background_color, pcg, "
                    "num_of_rays, max_depth, russian_roulette_limit)) renders every num_of_rays and pcg_mode on the device")

    def __init__(self, world, tracer=None, background_color: Color = BLACK, pcg=None, num_of_rays: int = 1, max_depth: int = 10,
                 russian_roulette_limit: int = 3):
        super().__init__(world, background_color)
        from .hostmodel import PCG

        if int(num_of_rays) != 1:
            raise ValueError(f"PathTracerShader traces one ray per hit, not num_of_rays={num_of_rays}: the children of a hit draw from one "
                             f"stream depth-first, which cannot be walked breadth-first; {self._ALTERNATIVE}")
        self.tracer = tracer
        self.pcg = pcg if pcg is not None else PCG()
        self.num_of_rays, self.max_depth, self.russian_roulette_limit = 1, int(max_depth), int(russian_roulette_limit)
        self._check_tracer()

    def _check_tracer(self) -> None:
        _check_sample_streams("PathTracerShader", self.tracer, self._ALTERNATIVE)

    def _queries(self):
        if self.tracer is None:
            raise TypeError("PathTracerShader.shade_hits needs the tracer whose device scene holds the world: PathTracerShader(world, tracer, ...)")
        return self.tracer.world_queries(self.world)

    def sample_streams(self, frame) -> np.ndarray:
        """``uint64[2, n]``: the generator of every sample of ``frame`` where its path starts (behind the two jitter draws)."""
        return sample_streams(self.pcg, frame)

    def shade_hits(self, frame) -> np.ndarray:
        from .rays import SCAT_ALL

        self._check_tracer()
        q = self._queries()
        bg = self.background_color
        bg = np.array((bg.r, bg.g, bg.b), dtype=np.float64)
        shape3 = frame.shape_index.shape
        hits, dirs, pcg = frame, None, self.sample_streams(frame)
        levels = []
        for depth in range(self.max_depth + 1):
            sc = q.scatter(hits, dirs, pcg, roulette=depth >= self.russian_roulette_limit, channels=SCAT_ALL)
            status = np.asarray(sc.status).reshape(-1)
            levels.append((status, np.asarray(sc.weight).reshape(-1, 3), np.asarray(sc.emitted).reshape(-1, 3),
                           depth >= self.russian_roulette_limit))
            if depth == self.max_depth or not np.any(status == 1):  # (a child beyond max_depth is black without a query)
                break
            hits, dirs, pcg = q.ray_intersections(sc.rays.T, channels="point,normal,uv"), sc.dirs, sc.pcg
        # render.py:135-139 from the deepest call upwards.  (A path that ends at a hit without the roulette ended on a black BRDF
        # pigment: the reference still adds its empty sum, emitted + 0.0 * (1.0 / num_of_rays).)
        k = 1.0 / self.num_of_rays
        val = np.zeros((status.shape[0], 3), dtype=np.float64)
        for status, weight, emitted, roulette in reversed(levels):
            cum = 0.0 + weight * val
            ended = emitted if roulette else emitted + 0.0 * k
            val = np.where((status == 1)[:, None], emitted + cum * k, np.where((status == 0)[:, None], ended, bg[None, :]))
        return val.reshape(shape3 + (3,))

    # -- ray by ray ---------------------------------------------------------------------------------------------------------
    def __call__(self, ray) -> Color:
        if not callable(getattr(self.world, "ray_intersection", None)):
            raise TypeError(f"{type(self.world).__name__} has no ray_intersection(ray): it is a parameter holder that cannot trace a ray.  "
                            "Hand PathTracerShader to GpuImageTracer.fire_all_rays (the device traces), or give it a pytracer World")
        return self._radiance(ray, int(getattr(ray, "depth", 0)))

    def _radiance(self, ray, depth: int) -> Color:
        from .hits import HitRay
        from .hostmodel import Vec

        if depth > self.max_depth:
            return Color(0.0, 0.0, 0.0)
        record = self.world.ray_intersection(ray)
        if record is None:
            return self.background_color
        material = getattr(record, "material", None) or self.world.shapes[record.shape_index].material
        uv, wp, nrm = record.surface_point, record.world_point, record.normal
        hc, em = pigment_color(material.brdf.pigment, uv), pigment_color(material.emitted_radiance, uv)
        r, g, b = hc.r, hc.g, hc.b
        lum = max(max(r, g), b)
        if depth >= self.russian_roulette_limit:  # render.py:116-123
            q = max(0.05, 1 - lum)
            if self.pcg.random_float() > q:
                f = 1.0 / (1.0 - q)
                r, g, b = r * f, g * f, b * f
            else:
                return em
        cr = cg = cb = 0.0
        if lum > 0.0:
            d = ray.dir
            o, nd, tmin = scatter_ray(material.brdf, self.pcg, (d.x, d.y, d.z), (wp.x, wp.y, wp.z), (nrm.x, nrm.y, nrm.z))
            child = self._radiance(HitRay(Vec(*o), Vec(*nd), tmin, float("inf"), depth + 1), depth + 1)
            cr, cg, cb = cr + r * child.r, cg + g * child.g, cb + b * child.b
        k = 1.0 / self.num_of_rays
        return Color(em.r + cr * k, em.g + cg * k, em.b + cb * k)


class PathRadianceShader(_HitShader):
    """``PathTracer`` (render.py:99-139) with ANY ``num_of_rays >= 1`` as a hit shader, depth-first on the device:
    ``shade_hits(frame)`` hands the frame's own primary rays (``ray_origin``, ``ray_dir``, ``tmin = 1e-5``, ``tmax = inf``) to
    ``WorldQueries.path_radiance`` (include/ptrace_radiance.h), every sample with the generator :func:`sample_streams` gives it
    -- the streams of :class:`PathTracerShader` and of the fused path tracer's ``pcg_mode="sample"``.  So, handed to a
    ``GpuImageTracer(..., pcg=PCG(S0, Q0), pcg_mode="sample")``, the frame is the one ``fire_all_rays(PathTracer(world,
    background_color, PCG(S0, Q0), num_of_rays, max_depth, limit))`` renders.

    The radiance query RE-TRACES the primary ray: of the hit-record frame only the rays are read (``hit_channels`` asks for
    nothing else), and the first hit is found a second time inside the walk.  Starting the walk from the records is a follow-up.

    A tracer with ``pcg_mode="seq"``, or ``pcg_mode="pixel"`` with more than one sample, is refused as by
    :class:`PathTracerShader`.  ``__call__(ray)`` is the same recursion in Python floats, drawing from ``pcg`` itself, on a
    world that can intersect."""

    hit_channels = abi.HIT_RAY
    _ALTERNATIVE = PathTracerShader._ALTERNATIVE

    def __init__(self, world, tracer=None, background_color: Color = BLACK, pcg=None, num_of_rays: int = 1, max_depth: int = 10,
                 russian_roulette_limit: int = 3):
        super().__init__(world, background_color)
        from .hostmodel import PCG

        if int(num_of_rays) < 1:
            raise ValueError(f"PathRadianceShader needs num_of_rays >= 1, not {num_of_rays}")
        if int(max_depth) < 0:
            raise ValueError(f"PathRadianceShader needs max_depth >= 0, not {max_depth}")
        self.tracer = tracer
        self.pcg = pcg if pcg is not None else PCG()
        self.num_of_rays, self.max_depth, self.russian_roulette_limit = int(num_of_rays), int(max_depth), int(russian_roulette_limit)
        self.last_radiance = None  # the RayRadiance of the last shade_hits (its n_rays plane: the rays the walk traced)
        _check_sample_streams("PathRadianceShader", tracer, self._ALTERNATIVE)

    def shade_hits(self, frame) -> np.ndarray:
        _check_sample_streams("PathRadianceShader", self.tracer, self._ALTERNATIVE)
        if self.tracer is None:
            raise TypeError("PathRadianceShader.shade_hits needs the tracer whose device scene holds the world: PathRadianceShader(world, tracer, ...)")
        q = self.tracer.world_queries(self.world)
        shape3 = frame.shape_index.shape
        res = q.path_radiance(np.asarray(frame.ray_origin).reshape(-1, 3), sample_streams(self.pcg, frame), np.asarray(frame.ray_dir).reshape(-1, 3),
                              self.num_of_rays, self.max_depth, self.russian_roulette_limit, self.background_color, 0, "all", 1e-5, float("inf"))
        self.last_radiance = res
        return np.asarray(res.radiance).reshape(shape3 + (3,))

    # -- ray by ray ---------------------------------------------------------------------------------------------------------
    def __call__(self, ray) -> Color:
        if not callable(getattr(self.world, "ray_intersection", None)):
            raise TypeError(f"{type(self.world).__name__} has no ray_intersection(ray): it is a parameter holder that cannot trace a ray.  "
                            "Hand PathRadianceShader to GpuImageTracer.fire_all_rays (the device traces), or give it a pytracer World")
        return self._radiance(ray, int(getattr(ray, "depth", 0)))

    def _radiance(self, ray, depth: int) -> Color:
        from .hits import HitRay
        from .hostmodel import Vec

        if depth > self.max_depth:
            return Color(0.0, 0.0, 0.0)
        record = self.world.ray_intersection(ray)
        if record is None:
            return self.background_color
        material = getattr(record, "material", None) or self.world.shapes[record.shape_index].material
        uv, wp, nrm = record.surface_point, record.world_point, record.normal
        hc, em = pigment_color(material.brdf.pigment, uv), pigment_color(material.emitted_radiance, uv)
        r, g, b = hc.r, hc.g, hc.b
        lum = max(max(r, g), b)
        if depth >= self.russian_roulette_limit:  # render.py:116-123
            q = max(0.05, 1 - lum)
            if self.pcg.random_float() > q:
                f = 1.0 / (1.0 - q)
                r, g, b = r * f, g * f, b * f
            else:
                return em
        cr = cg = cb = 0.0
        if lum > 0.0:
            d = ray.dir
            for _ in range(self.num_of_rays):  # render.py:126-137
                o, nd, tmin = scatter_ray(material.brdf, self.pcg, (d.x, d.y, d.z), (wp.x, wp.y, wp.z), (nrm.x, nrm.y, nrm.z))
                child = self._radiance(HitRay(Vec(*o), Vec(*nd), tmin, float("inf"), depth + 1), depth + 1)
                cr, cg, cb = cr + r * child.r, cg + g * child.g, cb + b * child.b
        k = 1.0 / self.num_of_rays
        return Color(em.r + cr * k, em.g + cg * k, em.b + cb * k)


class ProbeLitShader(_HitShader):
    """A world lit by a lattice of SH radiance probes, as a hit shader: ``background_color`` where nothing is hit, else
    ``emitted + brdf_color * E`` with ``E`` the eight probes of ``grid`` (a :class:`pytracer_amd.rays.ProbeGrid`) around the hit
    point blended and evaluated -- the cosine-weighted hemisphere mean around the normal for a ``DiffuseBRDF``, the radiance from
    the mirror direction for a ``SpecularBRDF``.  No ray is scattered: a frame costs its hit frame plus one kernel
    (``WorldQueries.probe_lit_radiance``; include/ptrace_lit.h).  ``probes``: the :class:`pytracer_amd.rays.ProbeSet` of
    ``grid.points()``; ``tracer``: the ``GpuImageTracer`` whose cached device scene answers (``None`` for a shader that is only
    ever called ray by ray).  The world may be a baked one (``scenes.baked_world``): a black BRDF leaves its emitted map as it is.

    ``__call__(ray)`` is the numpy mirror (``rays.lit_shade_host``'s arithmetic for one record) on a world that has
    ``ray_intersection(ray)``; the record's material is ``record.material`` or ``world.shapes[record.shape_index].material``."""

    hit_channels = abi.HIT_ALL

    def __init__(self, world, grid, probes, tracer=None, background_color: Color = BLACK):
        super().__init__(world, background_color)
        if probes.n != grid.n:
            raise ValueError(f"{probes.n} probes for a lattice of {grid.n}")
        self.grid, self.probes, self.tracer = grid, probes, tracer

    def shade_hits(self, frame) -> np.ndarray:
        if self.tracer is None:
            raise TypeError("ProbeLitShader.shade_hits needs the tracer whose device scene holds the world: ProbeLitShader(world, grid, probes, tracer)")
        return self.tracer.world_queries(self.world).probe_lit_radiance(self.grid, self.probes, frame, None, self.background_color)

    def __call__(self, ray) -> Color:
        if not callable(getattr(self.world, "ray_intersection", None)):
            raise TypeError(f"{type(self.world).__name__} has no ray_intersection(ray): it is a parameter holder that cannot trace a ray.  "
                            "Hand ProbeLitShader to GpuImageTracer.fire_all_rays (the device traces), or give it a pytracer World")
        return self.shade_record(self.world.ray_intersection(ray), ray)

    def shade_record(self, record, ray) -> Color:
        from .rays import SH_HEMISPHERE, SH_RADIANCE, _unit_rows, lit_eval_host, mirror_directions

        if record is None:
            return self.background_color
        material = getattr(record, "material", None) or self.world.shapes[record.shape_index].material
        uv, wp, nrm = record.surface_point, record.world_point, record.normal
        pc, em = pigment_color(material.brdf.pigment, uv), pigment_color(material.emitted_radiance, uv)
        normal = np.array([[nrm.x, nrm.y, nrm.z]], dtype=np.float64)
        if type(material.brdf).__name__ == "SpecularBRDF":
            towards, kind = mirror_directions(np.array([[ray.dir.x, ray.dir.y, ray.dir.z]], dtype=np.float64), normal), SH_RADIANCE
        else:
            towards, kind = _unit_rows(normal), SH_HEMISPHERE
        e = lit_eval_host(self.grid, self.probes, np.array([[wp.x, wp.y, wp.z]], dtype=np.float64), towards, kind)[0]
        return Color(em.r + pc.r * float(e[0]), em.g + pc.g * float(e[1]), em.b + pc.b * float(e[2]))


class DenoisedGatherShader(_HitShader):
    """One-bounce global illumination with few rays and a guided filter, as a hit shader: the hit frame, then
    ``WorldQueries.hemisphere_radiance`` with ``samples`` rays per pixel, then the edge-avoiding filter of
    include/ptrace_denoise.h on that mean ``E`` (``WorldQueries.denoised``, guided by the frame's own ``shape_index``, ``point`` and
    ``normal``), then ``emitted + brdf_color * E`` with the colours of ``WorldQueries.materials``; ``background_color`` where
    nothing is hit.  The filter sees ``E`` and not the final colour, so a checkered pigment stays sharp.  The frame must hold ONE
    sample per pixel (``samples_per_side`` 0 or 1).

    ``samples``, ``init_state``, ``init_seq``, ``max_depth`` and ``russian_roulette_limit`` are the gather's (its rays have
    ``Ray.depth = 1``: the children of a camera ray's hit); ``params`` are the filter's (``passes``, ``sigma_point``,
    ``normal_power_log2``, ``sigma_colour``, ``same_shape``).  ``filtered=False`` leaves the filter out: the noisy frame it replaces.
    ``last_gather`` is the :class:`pytracer_amd.rays.GatheredRadiance` of the last frame.

    ``__call__(ray)`` is the UNFILTERED value of one ray -- a filter has no meaning for a single record: ``emitted + brdf_color *
    E`` with ``E`` the mean of ``samples`` one-ray ``PathRadianceShader`` walks from the hit, drawn from this shader's own ``pcg``."""

    hit_channels = abi.HIT_ALL

    def __init__(self, world, tracer=None, samples: int = 4, background_color: Color = BLACK, init_state: int = 42, init_seq: int = 54,
                 max_depth: int = 10, russian_roulette_limit: int = 3, filtered: bool = True, pcg=None, **params):
        super().__init__(world, background_color)
        from ._denoise_lib import DEFAULTS
        from .hostmodel import PCG

        if int(samples) < 1:
            raise ValueError(f"DenoisedGatherShader needs samples >= 1, not {samples}")
        unknown = set(params) - (set(DEFAULTS) - {"wrap_x"})
        if unknown:
            raise TypeError(f"DenoisedGatherShader: unknown filter parameter(s) {sorted(unknown)}")
        self.tracer, self.samples, self.filtered, self.params = tracer, int(samples), bool(filtered), dict(params)
        self.init_state, self.init_seq = int(init_state), int(init_seq)
        self.max_depth, self.russian_roulette_limit = int(max_depth), int(russian_roulette_limit)
        self.pcg = pcg if pcg is not None else PCG()
        self.last_gather = None

    def shade_hits(self, frame) -> np.ndarray:
        if self.tracer is None:
            raise TypeError("DenoisedGatherShader.shade_hits needs the tracer whose device scene holds the world: DenoisedGatherShader(world, tracer, ...)")
        index = np.asarray(frame.shape_index)
        if index.ndim != 3 or index.shape[0] != 1:
            raise ValueError(f"DenoisedGatherShader filters one record per pixel, not a frame of {index.shape}: build the tracer with samples_per_side=0 or 1")
        q = self.tracer.world_queries(self.world)
        gathered = q.hemisphere_radiance(frame, self.samples, self.init_state, None, 1, self.max_depth, self.russian_roulette_limit,
                                         self.background_color, 1, "none", init_seq=self.init_seq)
        self.last_gather = gathered
        e = q.denoised(gathered, frame, **self.params)[None] if self.filtered else np.asarray(gathered.radiance)
        mat = q.materials(frame)
        lit = np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * e
        return np.where(np.asarray(mat.hit)[..., None], lit, self._background(frame))

    def __call__(self, ray) -> Color:
        if not callable(getattr(self.world, "ray_intersection", None)):
            raise TypeError(f"{type(self.world).__name__} has no ray_intersection(ray): it is a parameter holder that cannot trace a ray.  "
                            "Hand DenoisedGatherShader to GpuImageTracer.fire_all_rays (the device traces), or give it a pytracer World")
        from .hits import HitRay
        from .hostmodel import DiffuseBRDF, UniformPigment, Vec

        record = self.world.ray_intersection(ray)
        if record is None:
            return self.background_color
        material = getattr(record, "material", None) or self.world.shapes[record.shape_index].material
        uv, wp, nrm, d = record.surface_point, record.world_point, record.normal, ray.dir
        pc, em = pigment_color(material.brdf.pigment, uv), pigment_color(material.emitted_radiance, uv)
        walk = PathRadianceShader(self.world, None, self.background_color, self.pcg, 1, self.max_depth, self.russian_roulette_limit)
        white = DiffuseBRDF(UniformPigment(Color(1.0, 1.0, 1.0)))
        r = g = b = 0.0
        for _ in range(self.samples):
            o, nd, tmin = scatter_ray(white, self.pcg, (d.x, d.y, d.z), (wp.x, wp.y, wp.z), (nrm.x, nrm.y, nrm.z))
            c = walk._radiance(HitRay(Vec(*o), Vec(*nd), tmin, float("inf"), 1), 1)
            r, g, b = r + c.r, g + c.g, b + c.b
        k = 1.0 / self.samples
        return Color(em.r + pc.r * (r * k), em.g + pc.g * (g * k), em.b + pc.b * (b * k))


class TemporalGatherShader(DenoisedGatherShader):
    """:class:`DenoisedGatherShader` over a sequence of frames: the hit frame, then ``WorldQueries.hemisphere_radiance`` with
    ``samples`` rays per pixel, then the accumulation of include/ptrace_temporal.h on that mean ``E``
    (``rays.TemporalAccumulator.update``: last frame's accumulated ``E`` reprojected through last frame's camera and blended in), then
    the filter (when ``filtered``), then ``emitted + brdf_color * E``.  The camera is the tracer's at the time of the call: move it
    between two ``fire_all_rays``.  Frame ``f`` (``frame_no``, counted from 0) draws fresh generators: its gather starts at stream
    ``init_seq + f * m * samples``, ``m`` the frame's pixels, so no two frames share a stream.

    ``params`` are told apart by name -- the filter's ``passes``, ``sigma_point``, ``normal_power_log2``, ``sigma_colour``,
    ``same_shape``; the accumulation's ``max_history``, ``normal_min``, ``point_tolerance`` and ``history_same_shape`` (its
    ``same_shape``) -- and anything else is a ``TypeError``.  ``accumulate=False`` renders the frame ``frame_no`` WOULD be without
    its history, and leaves history and ``frame_no`` as they are: the frame to compare with.  ``reset()`` starts a new sequence.
    ``accumulator.count`` holds the history lengths of the last frame."""

    def __init__(self, world, tracer=None, samples: int = 4, background_color: Color = BLACK, init_state: int = 42, init_seq: int = 54,
                 max_depth: int = 10, russian_roulette_limit: int = 3, filtered: bool = True, pcg=None, accumulate: bool = True, **params):
        from ._denoise_lib import DEFAULTS as FILTER
        from ._temporal_lib import DEFAULTS as HISTORY

        mine = {"history_same_shape" if k == "same_shape" else k for k in HISTORY}
        unknown = set(params) - (set(FILTER) - {"wrap_x"}) - mine
        if unknown:
            raise TypeError(f"TemporalGatherShader: unknown filter or accumulation parameter(s) {sorted(unknown)}")
        history = {("same_shape" if k == "history_same_shape" else k): params.pop(k) for k in sorted(mine) if k in params}
        super().__init__(world, tracer, samples, background_color, init_state, init_seq, max_depth, russian_roulette_limit, filtered, pcg, **params)
        self.history_params, self.accumulate = history, bool(accumulate)
        self.accumulator, self.frame_no = None, 0

    def reset(self) -> None:
        self.frame_no = 0
        if self.accumulator is not None:
            self.accumulator.reset()

    def shade_hits(self, frame) -> np.ndarray:
        from .rays import TemporalAccumulator

        if self.tracer is None:
            raise TypeError("TemporalGatherShader.shade_hits needs the tracer whose device scene holds the world: TemporalGatherShader(world, tracer, ...)")
        index = np.asarray(frame.shape_index)
        if index.ndim != 3 or index.shape[0] != 1:
            raise ValueError(f"TemporalGatherShader keeps one record per pixel, not a frame of {index.shape}: build the tracer with samples_per_side=0 or 1")
        q = self.tracer.world_queries(self.world)
        seq = self.init_seq + self.frame_no * (index.shape[1] * index.shape[2]) * self.samples
        gathered = q.hemisphere_radiance(frame, self.samples, self.init_state, None, 1, self.max_depth, self.russian_roulette_limit,
                                         self.background_color, 1, "none", init_seq=seq)
        self.last_gather = gathered
        e = np.asarray(gathered.radiance)[0]
        if self.accumulate:
            if self.accumulator is None or self.accumulator.queries.scene is not q.scene:
                self.accumulator = TemporalAccumulator(q, **self.history_params)
            e = self.accumulator.update(e, frame, self.tracer.camera)
            self.frame_no += 1
        if self.filtered:
            e = q.denoised(e, frame, **self.params)
        mat = q.materials(frame)
        lit = np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * e[None]
        return np.where(np.asarray(mat.hit)[..., None], lit, self._background(frame))


class VarianceGuidedGatherShader(DenoisedGatherShader):
    """:class:`TemporalGatherShader` with a filter that knows how noisy every pixel still is: the hit frame, then
    ``WorldQueries.hemisphere_radiance`` with ``samples`` rays per pixel, then ``rays.VarianceAccumulator.update`` (the accumulation of
    that mean ``E`` AND of its luminance moments, and the variance of include/ptrace_variance.h from them), then the variance-guided
    filter (``WorldQueries.variance_filtered``, when ``filtered``), then ``emitted + brdf_color * E``.  The camera, the frame numbers
    and the generators are :class:`TemporalGatherShader`'s.

    ``params`` are told apart by name -- the filter's ``passes``, ``sigma_point``, ``normal_power_log2``, ``sigma_luminance``,
    ``epsilon``, ``same_shape``; the accumulation's and the estimate's ``max_history``, ``min_history``, ``normal_min``,
    ``point_tolerance`` and ``history_same_shape`` (their ``same_shape``) -- and anything else is a ``TypeError``.
    ``accumulate=False`` filters the frame ``frame_no`` WOULD be without its history by the single-frame route (a spatial variance
    estimate), and leaves history and ``frame_no`` as they are.  ``reset()`` starts a new sequence.  ``accumulator.count`` holds the
    history lengths and ``last_variance`` the variance (before the filter) of the last accumulated frame."""

    FILTER_KEYS = ("passes", "sigma_point", "normal_power_log2", "sigma_luminance", "epsilon", "same_shape")
    HISTORY_KEYS = ("max_history", "min_history", "normal_min", "point_tolerance", "history_same_shape")

    def __init__(self, world, tracer=None, samples: int = 4, background_color: Color = BLACK, init_state: int = 42, init_seq: int = 54,
                 max_depth: int = 10, russian_roulette_limit: int = 3, filtered: bool = True, pcg=None, accumulate: bool = True, **params):
        unknown = set(params) - set(self.FILTER_KEYS) - set(self.HISTORY_KEYS)
        if unknown:
            raise TypeError(f"VarianceGuidedGatherShader: unknown filter or accumulation parameter(s) {sorted(unknown)}")
        super().__init__(world, tracer, samples, background_color, init_state, init_seq, max_depth, russian_roulette_limit, filtered, pcg)
        self.params = {k: params[k] for k in self.FILTER_KEYS if k in params}
        self.history_params = {("same_shape" if k == "history_same_shape" else k): params[k] for k in self.HISTORY_KEYS if k in params}
        self.accumulate = bool(accumulate)
        self.accumulator, self.frame_no, self.last_variance = None, 0, None

    def reset(self) -> None:
        self.frame_no = 0
        if self.accumulator is not None:
            self.accumulator.reset()

    def shade_hits(self, frame) -> np.ndarray:
        from .rays import VarianceAccumulator

        if self.tracer is None:
            raise TypeError("VarianceGuidedGatherShader.shade_hits needs the tracer whose device scene holds the world: "
                            "VarianceGuidedGatherShader(world, tracer, ...)")
        index = np.asarray(frame.shape_index)
        if index.ndim != 3 or index.shape[0] != 1:
            raise ValueError(f"VarianceGuidedGatherShader keeps one record per pixel, not a frame of {index.shape}: build the tracer with "
                             "samples_per_side=0 or 1")
        q = self.tracer.world_queries(self.world)
        seq = self.init_seq + self.frame_no * (index.shape[1] * index.shape[2]) * self.samples
        gathered = q.hemisphere_radiance(frame, self.samples, self.init_state, None, 1, self.max_depth, self.russian_roulette_limit,
                                         self.background_color, 1, "none", init_seq=seq)
        self.last_gather = gathered
        e, variance = np.asarray(gathered.radiance)[0], None
        if self.accumulate:
            if self.accumulator is None or self.accumulator.queries.scene is not q.scene:
                self.accumulator = VarianceAccumulator(q, **self.history_params)
            e, variance = self.accumulator.update(e, frame, self.tracer.camera)
            self.last_variance = variance
            self.frame_no += 1
        if self.filtered:
            estimate = {} if self.accumulate else {k: v for k, v in self.history_params.items() if k in ("min_history", "normal_min", "point_tolerance")}
            e, _ = q.variance_filtered(e, frame, variance=variance, **self.params, **estimate)
        mat = q.materials(frame)
        lit = np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * e[None]
        return np.where(np.asarray(mat.hit)[..., None], lit, self._background(frame))


class AdaptiveGatherShader(VarianceGuidedGatherShader):
    """:class:`VarianceGuidedGatherShader` whose rays go where the estimate is still noisy: frame 0 is its uniform gather of
    ``samples`` rays per pixel; from frame 1 on the previous frame's accumulated ``E`` and its variance (before the filter) give a
    sample count per pixel (``WorldQueries.sample_counts``, include/ptrace_adaptive.h) and the gather is the ragged one
    (``WorldQueries.hemisphere_radiance_ragged``).  The counts are read at THIS frame's pixels from LAST frame's planes: the camera
    is assumed to move little between two frames, as the accumulation assumes it.  Frame ``f`` starts at the stream behind
    everything the frames before it drew, so no two frames share a stream.

    ``min_samples`` must be at least 1: a hit pixel without a sample would hand the accumulation a black estimate.  ``params``:
    :class:`VarianceGuidedGatherShader` 's, and the counts' ``min_samples``, ``max_samples``, ``tolerance``, ``luminance_floor``,
    ``gain``; ``budget`` (samples per frame, or ``None``) caps every ragged gather -- a total beyond it is truncated in record order.
    ``last_counts`` holds the counts of the last frame (``None`` for a uniform one), ``last_total`` the samples it took.

    OUT OF SCOPE here: ``rays.TemporalAccumulator`` weights every frame equally whatever it cost, so a pixel's 32-sample frame counts as much
    as its 1-sample frame.  :class:`WeightedAdaptiveGatherShader` weights frames by their samples (include/ptrace_weighted.h)."""

    COUNT_KEYS = ("min_samples", "max_samples", "tolerance", "luminance_floor", "gain")

    def __init__(self, world, tracer=None, samples: int = 4, background_color: Color = BLACK, init_state: int = 42, init_seq: int = 54,
                 max_depth: int = 10, russian_roulette_limit: int = 3, filtered: bool = True, pcg=None, accumulate: bool = True, budget=None,
                 **params):
        from ._adaptive_lib import DEFAULTS

        count_params = dict(DEFAULTS, **{k: params.pop(k) for k in self.COUNT_KEYS if k in params})
        if int(count_params["min_samples"]) < 1:
            raise ValueError(f"AdaptiveGatherShader needs min_samples >= 1, not {count_params['min_samples']}")
        try:
            super().__init__(world, tracer, samples, background_color, init_state, init_seq, max_depth, russian_roulette_limit, filtered, pcg,
                             accumulate, **params)
        except TypeError as e:
            raise TypeError(str(e).replace("VarianceGuidedGatherShader", "AdaptiveGatherShader")) from None
        self.count_params, self.budget = count_params, None if budget is None else int(budget)
        self.last_counts, self.last_total, self._next_seq, self._previous = None, 0, self.init_seq, None

    def reset(self) -> None:
        super().reset()
        self.last_counts, self.last_total, self._next_seq, self._previous = None, 0, self.init_seq, None

    def shade_hits(self, frame) -> np.ndarray:
        from .rays import VarianceAccumulator

        if self.tracer is None:
            raise TypeError("AdaptiveGatherShader.shade_hits needs the tracer whose device scene holds the world: AdaptiveGatherShader(world, tracer, ...)")
        index = np.asarray(frame.shape_index)
        if index.ndim != 3 or index.shape[0] != 1:
            raise ValueError(f"AdaptiveGatherShader keeps one record per pixel, not a frame of {index.shape}: build the tracer with samples_per_side=0 or 1")
        q = self.tracer.world_queries(self.world)
        m = index.shape[1] * index.shape[2]
        if self._previous is not None and self._previous[1].size == m:
            e_prev, var_prev = self._previous
            counts = q.sample_counts(e_prev, frame, var_prev, **self.count_params)
            gathered = q.hemisphere_radiance_ragged(frame, counts[None], self.budget, self.init_state, None, 1, self.max_depth,
                                                    self.russian_roulette_limit, self.background_color, 1, "taken", init_seq=self._next_seq)
            total = int(np.maximum(counts, 0).sum(dtype=np.int64))
            self.last_counts, self.last_total = counts, int(np.asarray(gathered.taken).sum(dtype=np.int64))
        else:
            gathered = q.hemisphere_radiance(frame, self.samples, self.init_state, None, 1, self.max_depth, self.russian_roulette_limit,
                                             self.background_color, 1, "none", init_seq=self._next_seq)
            total = m * self.samples
            self.last_counts, self.last_total = None, int((index >= 0).sum()) * self.samples
        self.last_gather = gathered
        e, variance = np.asarray(gathered.radiance)[0], None
        if self.accumulate:
            if self.accumulator is None or self.accumulator.queries.scene is not q.scene:
                self.accumulator = VarianceAccumulator(q, **self.history_params)
            e, variance = self.accumulator.update(e, frame, self.tracer.camera)
            self.last_variance, self._previous = variance, (e, variance)
            self.frame_no += 1
            self._next_seq += total  # (the streams this frame's records were given, taken or not)
        if self.filtered:
            estimate = {} if self.accumulate else {k: v for k, v in self.history_params.items() if k in ("min_history", "normal_min", "point_tolerance")}
            e, _ = q.variance_filtered(e, frame, variance=variance, **self.params, **estimate)
        mat = q.materials(frame)
        lit = np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * e[None]
        return np.where(np.asarray(mat.hit)[..., None], lit, self._background(frame))


class WeightedAdaptiveGatherShader(AdaptiveGatherShader):
    """:class:`AdaptiveGatherShader` whose accumulation weights every frame by the samples it took
    (``rays.WeightedAccumulator``, include/ptrace_weighted.h): a pixel's 31-sample frame counts 31 times its 1-sample frame, and the
    accumulation and the variance estimate are two launches where :class:`AdaptiveGatherShader` makes four.  Frame 0 hands the
    accumulator a plane that is ``samples`` at the hit records; every later frame hands it the ragged gather's ``taken`` plane.

    ``min_samples = 0`` is legal here: a record that took no sample has weight 0, so its (black) radiance is never read into the
    history, which is reprojected and carried as it was.  For the same reason a ``budget`` that runs out leaves the history of the
    records it cut off untouched, where :class:`AdaptiveGatherShader` blends them in as black.

    ``params``: :class:`AdaptiveGatherShader` 's, and the accumulation's ``max_weight`` (the cap of a history's weight; default
    128) and ``blend_weight`` (the history's weight is the blend of the taps' weights, not their largest)."""

    HISTORY_KEYS = AdaptiveGatherShader.HISTORY_KEYS + ("max_weight", "blend_weight")

    def __init__(self, world, tracer=None, samples: int = 4, background_color: Color = BLACK, init_state: int = 42, init_seq: int = 54,
                 max_depth: int = 10, russian_roulette_limit: int = 3, filtered: bool = True, pcg=None, accumulate: bool = True, budget=None,
                 **params):
        least = params.pop("min_samples", None)
        if least is not None and int(least) < 0:
            raise ValueError(f"WeightedAdaptiveGatherShader needs min_samples >= 0, not {least}")
        try:
            super().__init__(world, tracer, samples, background_color, init_state, init_seq, max_depth, russian_roulette_limit, filtered, pcg,
                             accumulate, budget, **params)
        except TypeError as e:
            raise TypeError(str(e).replace("AdaptiveGatherShader", "WeightedAdaptiveGatherShader")) from None
        if least is not None:
            self.count_params["min_samples"] = int(least)

    def shade_hits(self, frame) -> np.ndarray:
        from .rays import WeightedAccumulator

        if self.tracer is None:
            raise TypeError("WeightedAdaptiveGatherShader.shade_hits needs the tracer whose device scene holds the world: "
                            "WeightedAdaptiveGatherShader(world, tracer, ...)")
        index = np.asarray(frame.shape_index)
        if index.ndim != 3 or index.shape[0] != 1:
            raise ValueError(f"WeightedAdaptiveGatherShader keeps one record per pixel, not a frame of {index.shape}: build the tracer with "
                             "samples_per_side=0 or 1")
        q = self.tracer.world_queries(self.world)
        m = index.shape[1] * index.shape[2]
        if self._previous is not None and self._previous[1].size == m:
            e_prev, var_prev = self._previous
            counts = q.sample_counts(e_prev, frame, var_prev, **self.count_params)
            gathered = q.hemisphere_radiance_ragged(frame, counts[None], self.budget, self.init_state, None, 1, self.max_depth,
                                                    self.russian_roulette_limit, self.background_color, 1, "taken", init_seq=self._next_seq)
            total = int(np.maximum(counts, 0).sum(dtype=np.int64))
            taken = np.asarray(gathered.taken, dtype=np.int32).reshape(index.shape[1:])
            self.last_counts, self.last_total = counts, int(taken.sum(dtype=np.int64))
        else:
            gathered = q.hemisphere_radiance(frame, self.samples, self.init_state, None, 1, self.max_depth, self.russian_roulette_limit,
                                             self.background_color, 1, "none", init_seq=self._next_seq)
            total = m * self.samples
            taken = np.where(index[0] >= 0, self.samples, 0).astype(np.int32)
            self.last_counts, self.last_total = None, int((index >= 0).sum()) * self.samples
        self.last_gather = gathered
        e, variance = np.asarray(gathered.radiance)[0], None
        if self.accumulate:
            if self.accumulator is None or self.accumulator.queries.scene is not q.scene:
                self.accumulator = WeightedAccumulator(q, **self.history_params)
            e, variance = self.accumulator.update(e, frame, self.tracer.camera, samples=taken)
            self.last_variance, self._previous = variance, (e, variance)
            self.frame_no += 1
            self._next_seq += total  # (the streams this frame's records were given, taken or not)
        if self.filtered:
            estimate = {} if self.accumulate else {k: v for k, v in self.history_params.items() if k in ("min_history", "normal_min", "point_tolerance")}
            e, _ = q.variance_filtered(e, frame, variance=variance, **self.params, **estimate)
        mat = q.materials(frame)
        lit = np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * e[None]
        return np.where(np.asarray(mat.hit)[..., None], lit, self._background(frame))


class MovingWorldGatherShader(VarianceGuidedGatherShader):
    """:class:`VarianceGuidedGatherShader` for a world whose shapes move between frames, on a ``rays.MotionAccumulator``
    (include/ptrace_motion.h): the hit frame, a uniform gather of ``samples`` rays per pixel, the motion accumulate query -- which
    fetches the history of a shape that moved where that surface point WAS -- the variance estimate, the variance-guided filter
    (when ``filtered``) and the material.  ``world`` is the caller's to replace between frames (or to give its shapes new
    transformations): the accumulator keeps the shapes of the frame before and derives the motion (``rays.shape_motion``), and the
    history survives the new device scene every such frame brings.  ``static=``: the indices of shapes that move ONTO THEMSELVES (a
    sphere spinning about its centre, a plane sliding in its own plane): ``E`` is light arriving at a place, and their history
    stays where the light is.

    ``params``: :class:`VarianceGuidedGatherShader` 's, and the accumulation's ``max_weight`` and ``blend_weight``.  ``follow = False``
    (an attribute, set before the first frame) runs the same sequence on a ``rays.WeightedAccumulator``, for comparison.

    ADAPTIVE COUNTS STAY OUT: ``WorldQueries.sample_counts`` reads last frame's planes at this frame's pixels, which for a moving
    shape is a reprojection question of its own; every frame here is a uniform gather."""

    HISTORY_KEYS = VarianceGuidedGatherShader.HISTORY_KEYS + ("max_weight", "blend_weight")

    def __init__(self, world, tracer=None, samples: int = 4, background_color: Color = BLACK, init_state: int = 42, init_seq: int = 54,
                 max_depth: int = 10, russian_roulette_limit: int = 3, filtered: bool = True, pcg=None, accumulate: bool = True, static=(),
                 **params):
        try:
            super().__init__(world, tracer, samples, background_color, init_state, init_seq, max_depth, russian_roulette_limit, filtered, pcg,
                             accumulate, **params)
        except TypeError as e:
            raise TypeError(str(e).replace("VarianceGuidedGatherShader", "MovingWorldGatherShader")) from None
        self.static, self.follow = tuple(static), True

    def shade_hits(self, frame) -> np.ndarray:
        from .rays import MotionAccumulator, WeightedAccumulator

        if self.tracer is None:
            raise TypeError("MovingWorldGatherShader.shade_hits needs the tracer whose device scene holds the world: "
                            "MovingWorldGatherShader(world, tracer, ...)")
        index = np.asarray(frame.shape_index)
        if index.ndim != 3 or index.shape[0] != 1:
            raise ValueError(f"MovingWorldGatherShader keeps one record per pixel, not a frame of {index.shape}: build the tracer with "
                             "samples_per_side=0 or 1")
        q = self.tracer.world_queries(self.world)
        seq = self.init_seq + self.frame_no * (index.shape[1] * index.shape[2]) * self.samples
        gathered = q.hemisphere_radiance(frame, self.samples, self.init_state, None, 1, self.max_depth, self.russian_roulette_limit,
                                         self.background_color, 1, "none", init_seq=seq)
        self.last_gather = gathered
        e, variance = np.asarray(gathered.radiance)[0], None
        if self.accumulate:
            taken = np.where(index[0] >= 0, self.samples, 0).astype(np.int32)
            if self.follow:
                if self.accumulator is None:
                    self.accumulator = MotionAccumulator(q, static=self.static, **self.history_params)
                e, variance = self.accumulator.update(e, frame, self.tracer.camera, samples=taken, world=self.world, queries=q)
            else:  # (for comparison: the same sequence reprojected through the camera only)
                if self.accumulator is None:
                    self.accumulator = WeightedAccumulator(q, **self.history_params)
                self.accumulator.queries = q
                e, variance = self.accumulator.update(e, frame, self.tracer.camera, samples=taken)
            self.last_variance = variance
            self.frame_no += 1
        if self.filtered:
            estimate = {} if self.accumulate else {k: v for k, v in self.history_params.items() if k in ("min_history", "normal_min", "point_tolerance")}
            e, _ = q.variance_filtered(e, frame, variance=variance, **self.params, **estimate)
        mat = q.materials(frame)
        lit = np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * e[None]
        return np.where(np.asarray(mat.hit)[..., None], lit, self._background(frame))


class GradientGatherShader(MovingWorldGatherShader):
    """:class:`MovingWorldGatherShader` on a ``rays.GradientAccumulator`` (include/ptrace_gradient.h): besides following the shapes
    that moved, the history of a pixel shortens where the LIGHT changed -- under the shadow of a shape that moved, in its reflection.
    Per frame after the first: one probe per stratum of this frame, gathered in the PREVIOUS world with this frame's streams, says
    how much of ``E`` changed because the world did, free of sampling noise; the accumulation keeps that much less of the history.
    On a static world every bit is :class:`MovingWorldGatherShader`'s.

    The tracer drops the previous world's device scene when it opens this frame's, so the shader keeps a copy of the previous world's
    shapes, opens a device scene of its own for the probes' gather and closes it before the frame is done.

    ``params``: :class:`MovingWorldGatherShader`'s, and ``stratum``, ``radius``, ``gain`` and ``same_shape_probes``.  ``follow_light =
    False`` (an attribute, set before the first frame) is the parent, for comparison; ``follow = False`` the grandparent.  Shapes that
    ROTATE give their probes a turned normal and hence other sample directions: their gradient contains sampling noise."""

    HISTORY_KEYS = MovingWorldGatherShader.HISTORY_KEYS + ("stratum", "radius", "gain", "same_shape_probes")

    def __init__(self, world, tracer=None, samples: int = 4, background_color: Color = BLACK, init_state: int = 42, init_seq: int = 54,
                 max_depth: int = 10, russian_roulette_limit: int = 3, filtered: bool = True, pcg=None, accumulate: bool = True, static=(),
                 **params):
        try:
            super().__init__(world, tracer, samples, background_color, init_state, init_seq, max_depth, russian_roulette_limit, filtered, pcg,
                             accumulate, static, **params)
        except TypeError as e:
            raise TypeError(str(e).replace("MovingWorldGatherShader", "GradientGatherShader")) from None
        self.follow_light, self._before = True, None

    def reset(self) -> None:
        super().reset()
        self._before = None

    def shade_hits(self, frame) -> np.ndarray:
        import copy

        from . import flatten
        from .device import DeviceScene
        from .rays import GradientAccumulator, WorldQueries

        keep_keys = GradientAccumulator.KEEP_KEYS
        if not (self.follow_light and self.follow and self.accumulate):
            held = self.history_params
            self.history_params = {k: v for k, v in held.items() if k not in keep_keys}
            try:
                return super().shade_hits(frame)
            finally:
                self.history_params = held
        if self.tracer is None:
            raise TypeError("GradientGatherShader.shade_hits needs the tracer whose device scene holds the world: "
                            "GradientGatherShader(world, tracer, ...)")
        index = np.asarray(frame.shape_index)
        if index.ndim != 3 or index.shape[0] != 1:
            raise ValueError(f"GradientGatherShader keeps one record per pixel, not a frame of {index.shape}: build the tracer with "
                             "samples_per_side=0 or 1")
        q = self.tracer.world_queries(self.world)
        seq = self.init_seq + self.frame_no * (index.shape[1] * index.shape[2]) * self.samples
        gathered = q.hemisphere_radiance(frame, self.samples, self.init_state, None, 1, self.max_depth, self.russian_roulette_limit,
                                         self.background_color, 1, "none", init_seq=seq)
        self.last_gather = gathered
        e = np.asarray(gathered.radiance)[0]
        taken = np.where(index[0] >= 0, self.samples, 0).astype(np.int32)
        if self.accumulator is None:
            self.accumulator = GradientAccumulator(q, static=self.static, **self.history_params)
        probe = dict(samples=self.samples, init_state=self.init_state, init_seq=seq, max_depth=self.max_depth,
                     russian_roulette_limit=self.russian_roulette_limit, background=self.background_color, depth=1)
        old_scene = None
        if self._before is not None and self.accumulator.frames > 0:  # (the tracer has closed that scene: one of the shader's own)
            old_scene = DeviceScene(flatten.flatten_world(self._before), q.scene.device)
            probe["queries"] = WorldQueries(old_scene)
        try:
            e, variance = self.accumulator.update(e, frame, self.tracer.camera, samples=taken, world=self.world, queries=q, probe=probe)
        finally:
            if old_scene is not None:
                old_scene.close()
            self.accumulator._prev_queries = None  # (its scene is the tracer's to close)
        self._before = copy.copy(self.world)
        self._before.shapes = [copy.copy(s) for s in self.world.shapes]
        self.last_variance = variance
        self.frame_no += 1
        if self.filtered:
            e, _ = q.variance_filtered(e, frame, variance=variance, **self.params)
        mat = q.materials(frame)
        lit = np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * e[None]
        return np.where(np.asarray(mat.hit)[..., None], lit, self._background(frame))


def scatter_ray(brdf, pcg, in_dir, point, normal):
    """``brdf.scatter_ray`` (materials.py:132-152, 175-196; the orthonormal basis of geometry.py:247-262) in Python floats with
    ``x * x`` for ``x**2``, for a BRDF that may be a parameter holder (by class name) -> (origin, direction, tmin)."""
    nx, ny, nz = normal
    if type(brdf).__name__ == "SpecularBRDF":
        rd, nn = _unit(*in_dir), _unit(nx, ny, nz)
        dp = nn[0] * rd[0] + nn[1] * rd[1] + nn[2] * rd[2]
        return point, (rd[0] - dp * (2.0 * nn[0]), rd[1] - dp * (2.0 * nn[1]), rd[2] - dp * (2.0 * nn[2])), 1e-5
    sign = 1.0 if nz > 0.0 else -1.0
    a = -1.0 / (sign + nz)
    b = nx * ny * a
    e1 = (1.0 + sign * nx * nx * a, sign * b, -sign * nx)
    e2 = (b, sign + ny * ny * a, -ny)
    cts = pcg.random_float()
    ct, st = math.sqrt(cts), math.sqrt(1.0 - cts)
    phi = 2.0 * math.pi * pcg.random_float()
    cp, sp = math.cos(phi), math.sin(phi)
    return point, tuple(ct * (cp * e1[i]) + ct * (sp * e2[i]) + st * normal[i] for i in range(3)), 1.0e-3
