"""Ray batches: ``World.ray_intersection`` (world.py:51-69) and ``World.is_point_visible`` (world.py:71-80) for a caller's
own rays, many at a time, on the device (include/ptrace_rays.h, libptrace_rays.so).

A hit shader gets its first hits from ``GpuImageTracer.fire_all_hits``; its second question -- a shadow ray to a light, a
mirror bounce, an ambient-occlusion probe -- goes through ``DeviceScene.trace_rays`` / ``occluded`` / ``points_visible``
(or ``GpuImageTracer.world_queries(world)``, the same on the tracer's cached scene).

Its third -- the hit's material, and its colour under the scene's point lights -- goes through ``DeviceScene.surface`` /
``shade_lights`` (include/ptrace_surface.h, libptrace_surface.so), or ``WorldQueries.materials`` / ``point_light_radiance``,
which take a :class:`RayHits` or a hit-record frame as it is: :class:`SurfaceColors` views the answer.

Its fourth -- the bounce: the Russian roulette and ``brdf.scatter_ray`` of every record, each with a generator of its own
carried from bounce to bounce -- goes through ``DeviceScene.scatter`` (include/ptrace_scatter.h, libptrace_scatter.so) or
``WorldQueries.scatter``: :class:`ScatteredRays` views the answer, whose ray block goes straight back into ``trace_rays``.
:func:`pcg_streams` makes the generators.

Its fifth -- the whole recursion: ``PathTracer(world, background, pcg_i, ...)(ray_i)`` for every ray of a batch, walked
depth-first on the device -- goes through ``DeviceScene.radiance`` (include/ptrace_radiance.h, libptrace_radiance.so) or
``WorldQueries.path_radiance``: :class:`RayRadiance` views the answer.

Its sixth -- the gather: the mean radiance arriving over the hemisphere of every record (an irradiance probe, a light-map
texel), ``samples`` cosine-weighted rays per record made, walked and averaged on the device in a fixed order -- goes through
``DeviceScene.gather`` (include/ptrace_gather.h, libptrace_gather.so) or ``WorldQueries.hemisphere_radiance``:
:class:`GatheredRadiance` views the answer.

Its seventh -- the bake: a light map over a shape's ``(u, v)`` grid, every texel the gather of ``samples`` points INSIDE the texel
(the surface points are made on the device from ``(shape, u, v)``; a map baked in windows is the map baked whole) -- goes
through ``DeviceScene.surface_points`` / ``DeviceScene.bake`` (include/ptrace_bake.h, libptrace_bake.so) or
``WorldQueries.surface_points`` / ``light_map`` / ``outgoing_map``: :class:`BakedMap` views the answer, and
``scenes.baked_world`` turns maps into a world ``FlatRenderer`` renders with its indirect light in place.

Its eighth -- the probe: the radiance arriving at a free point of the world from every direction, as the 27 coefficients of the
nine real spherical-harmonic functions of bands 0 - 2 per colour channel; the cosine-weighted hemisphere mean for ANY normal
follows from them without a new ray, so a shape that a baked world does not know can be lit from the probes around it -- goes
through ``DeviceScene.sh_project`` / ``sh_directions`` / ``sh_eval`` (include/ptrace_sh.h, libptrace_sh.so) or
``WorldQueries.radiance_probes`` / ``probe_directions`` / ``probe_map`` / ``outgoing_probe_map``: :class:`ProbeSet` views the
answer, :class:`ProbeGrid` places probes on a lattice and blends them.

Its ninth -- the lattice on the device: per record the eight probes around its point blended and evaluated in one kernel, alone
(``DeviceScene.lit_eval``, ``ProbeGrid.evaluate``) or fused with the material look-up into ``emitted + brdf_color * E``
(``DeviceScene.lit_shade``, ``WorldQueries.probe_lit_radiance``; include/ptrace_lit.h, libptrace_lit.so).  :func:`lit_eval_host` and
:func:`lit_shade_host` are the numpy mirrors that define the bits; ``shaders.ProbeLitShader`` renders frames with it.

Its tenth -- a remedy for noise other than more rays: an edge-avoiding a-trous filter over a frame or a light map, guided by the
records' ``shape``, ``point`` and ``normal`` (``DeviceScene.denoise``, ``WorldQueries.denoised`` / ``denoised_light_map``;
include/ptrace_denoise.h, libptrace_denoise.so).  :func:`denoise_host` is the numpy mirror that defines the bits;
``shaders.DenoisedGatherShader`` renders frames with it.

Its eleventh -- the filter's companion, which trades rays for time: last frame's accumulated mean reprojected onto this frame's hit
points through last frame's camera, checked against the records and blended with the new samples (``DeviceScene.temporal``,
``WorldQueries.accumulated``, :class:`TemporalAccumulator`; include/ptrace_temporal.h, libptrace_temporal.so).
:func:`temporal_host` is the numpy mirror that defines the bits; ``shaders.TemporalGatherShader`` renders sequences with it.

Layout: planar.  A batch is ``[8, n]`` float64 -- origin xyz, direction xyz, tmin, tmax, the fields of ``Ray`` (ray.py:29-50);
a result is one buffer, the int32 shape plane first (padded to 8 bytes), then the selected fp64 planes of ``n`` values each.
"""
from __future__ import annotations

import numpy as np

from . import abi

RAY_CHANNELS = abi.HIT_T | abi.HIT_POINT | abi.HIT_NORMAL | abi.HIT_UV
MAX_RAYS = 2 ** 31 - 1
_PLANES = {abi.HIT_T: 1, abi.HIT_POINT: 3, abi.HIT_NORMAL: 3, abi.HIT_UV: 2}
_CHANNEL_OF = {"t": abi.HIT_T, "point": abi.HIT_POINT, "normal": abi.HIT_NORMAL, "uv": abi.HIT_UV}


SURF_BRDF_COLOR, SURF_EMITTED, SURF_ALL = 1, 2, 3  # PT_SURF_* of include/ptrace_surface.h
_SURF_OF = {"brdf_color": SURF_BRDF_COLOR, "emitted": SURF_EMITTED}


SCAT_WEIGHT, SCAT_EMITTED, SCAT_ALL = 1, 2, 3  # PT_SCAT_* of include/ptrace_scatter.h
SCAT_RAYS, SCAT_PCG = 4, 8  # plane selectors of scatter_plane_offset (always written: not channel bits)
_SCAT_OF = {"weight": SCAT_WEIGHT, "emitted": SCAT_EMITTED}
_PCG_MULT = 6364136223846793005


RAD_PCG, RAD_COUNT, RAD_ALL = 1, 2, 3  # PT_RAD_* of include/ptrace_radiance.h
_RAD_OF = {"pcg": RAD_PCG, "count": RAD_COUNT}


GATHER_COUNT, GATHER_ALL = 1, 1  # PT_GATHER_* of include/ptrace_gather.h
_GATHER_OF = {"count": GATHER_COUNT}


ADAPTIVE_COUNT, ADAPTIVE_TAKEN, ADAPTIVE_ALL = 1, 2, 3  # PT_ADAPTIVE_* of include/ptrace_adaptive.h
_ADAPTIVE_OF = {"count": ADAPTIVE_COUNT, "taken": ADAPTIVE_TAKEN}
MAX_SAMPLES = 2 ** 20  # PT_ADAPTIVE_MAX_SAMPLES


BAKE_COUNT, BAKE_ALL = 1, 1  # PT_BAKE_* of include/ptrace_bake.h
_BAKE_OF = {"count": BAKE_COUNT}


SH_COUNT, SH_ALL = 1, 1  # PT_SH_* of include/ptrace_sh.h
SH_RADIANCE, SH_HEMISPHERE = 0, 1  # the evaluation's kinds
SH_COEFFS = 27  # planes of coefficients: plane 3 j + ch
_SH_OF = {"count": SH_COUNT}
# the basis' constants: ONE fp64 literal each, as the header states them
SH_K0, SH_K1, SH_K2, SH_K3, SH_K4 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
SH_BAND_FACTORS = (1.0,) + (2.0 / 3.0,) * 3 + (0.25,) * 5  # A_j of PT_SH_HEMISPHERE


def _parse_channels(channels, names_to_bits, all_bits, what) -> int:
    """The channel bits of a ``what`` batch from an int, names (``"a"``, ``"a,b"``), ``"all"`` or ``"none"``."""
    has = f"a {what} batch has the channel{'s' if len(names_to_bits) > 1 else ''}"
    if isinstance(channels, str):
        names = [x.strip().lower() for x in channels.split(",") if x.strip()]
        if names == ["all"]:
            return all_bits
        if names == ["none"]:
            return 0
        unknown = [x for x in names if x not in names_to_bits]
        if unknown:
            raise ValueError(f"{has} {', '.join(names_to_bits)}; not {', '.join(unknown)}")
        return sum({names_to_bits[x] for x in names})
    bits = int(channels)
    if bits < 0 or bits & ~all_bits:
        raise ValueError(f"{has} {', '.join(f'{k} ({v})' for k, v in names_to_bits.items())}; not {bits:#x}")
    return bits


class _BatchViews:
    """What the views over an add-on's result buffer share: the constructor's checks, the look-up of a selected channel's
    planes, and ``has``.  A subclass names its channels (``_names``, ``_all``), itself (``_what``; ``_unit``: what it counts) and
    the two mirrors of its library's size functions (``_bytes``, ``_offset``)."""
    _unit = "records"

    def __init__(self, buf, n: int, channels, shape):
        self.channels = _parse_channels(channels, self._names, self._all, self._what)
        self.n = int(n)
        self.shape = (self.n,) if shape is None else tuple(int(x) for x in shape)
        if int(np.prod(self.shape, dtype=np.int64)) != self.n:
            raise ValueError(f"shape {self.shape} does not hold {self.n} {self._unit}")
        self.nbytes = self._bytes(self.n, self.channels)
        buf = np.asarray(buf)
        if buf.dtype != np.uint8 or buf.ndim != 1:
            buf = buf.reshape(-1).view(np.uint8)
        if buf.nbytes < self.nbytes:
            raise ValueError(f"{self._what} buffer too small: {buf.nbytes} < {self.nbytes} bytes")
        self.buffer = buf

    def _plane_views(self, channel: int, count: int, dtype) -> np.ndarray:
        """``[count, n]``: the planes of a selected channel."""
        if not self.channels & channel:
            name = next(k for k, v in self._names.items() if v == channel)
            raise KeyError(f"channel {name!r} was not selected for this {self._what} batch (channels = {self.channels:#x})")
        off = self._offset(self.n, self.channels, channel, 0)
        return self.buffer[off: off + self.n * 8 * count].view(dtype).reshape(count, self.n)

    def _colour(self, channel: int) -> np.ndarray:
        return np.moveaxis(self._plane_views(channel, 3, np.float64).reshape((3,) + self.shape), 0, -1)

    def has(self, name: str) -> bool:
        return bool(self.channels & self._names[name])


def ray_channels(channels) -> int:
    """``PT_HIT_*`` bits a ray batch can carry, from an int, names (``"normal,t"``) or ``"all"`` (= t, point, normal, uv: the
    rays themselves are the caller's)."""
    if isinstance(channels, str) and channels.strip().lower() == "all":
        return RAY_CHANNELS
    bits = abi.hit_channels(channels)
    if bits & ~RAY_CHANNELS:
        raise ValueError(f"a ray batch has the channels t, point, normal, uv; not {bits & ~RAY_CHANNELS:#x}")
    return bits


def _ok(n: int, channels: int, anyhit: bool) -> bool:
    return 0 <= n <= MAX_RAYS and channels >= 0 and not channels & ~RAY_CHANNELS and not (anyhit and channels)


def rays_bytes(n: int, channels: int, anyhit: bool = False) -> int:
    """Mirror of ``pt_rays_bytes``: 0 for arguments the library refuses."""
    if not _ok(n, channels, anyhit):
        return 0
    return ((n * 4 + 7) & ~7) + n * 8 * sum(k for bit, k in _PLANES.items() if channels & bit)


def rays_plane_offset(n: int, channels: int, anyhit: bool, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_plane_offset`` (bytes; ``channel`` 0: the int32 plane; < 0: not selected)."""
    if not _ok(n, channels, anyhit):
        return -1
    if channel == 0:
        return 0 if component == 0 else -1
    if channel not in _PLANES or not channels & channel or not 0 <= component < _PLANES[channel]:
        return -1
    before = sum(k for bit, k in _PLANES.items() if bit < channel and channels & bit)
    return ((n * 4 + 7) & ~7) + n * 8 * (before + component)


def ray_planes(origins, dirs=None, tmin=1e-5, tmax=float("inf")) -> np.ndarray:
    """The ``[8, n]`` input block from ``[n, 3]`` origins and directions (``tmin`` / ``tmax``: scalars or ``[n]``; the defaults
    are ``Ray``'s, ray.py:44-45), or from one ``[n, 8]`` array of (origin, dir, tmin, tmax) rows."""
    o = np.asarray(origins, dtype=np.float64)
    if dirs is None:
        if o.ndim != 2 or o.shape[1] != 8:
            raise ValueError(f"rays must be [n, 8] (origin, dir, tmin, tmax), not {o.shape}")
        return np.ascontiguousarray(o.T)
    d = np.asarray(dirs, dtype=np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError(f"origins and dirs must both be [n, 3], not {o.shape} and {d.shape}")
    block = np.empty((8, o.shape[0]), dtype=np.float64)
    block[0:3] = o.T
    block[3:6] = d.T
    block[6] = tmin
    block[7] = tmax
    return block


def visibility_rays(points, observer) -> np.ndarray:
    """The rays of ``World.is_point_visible(point, observer)`` (world.py:71-80) for ``[n, 3]`` points, as an ``[8, n]`` block:
    from the observer, ``dir = point - observer``, ``tmin = 1e-2 / dir.norm()`` with the norm as geometry.py computes it
    (``sqrt(x*x + y*y + z*z)``), ``tmax = 1.0`` -- each operation as the reference orders it, so the rays are the
    reference's to the bit.  ``observer``: one point or ``[n, 3]``."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ob = np.broadcast_to(np.asarray(observer, dtype=np.float64).reshape(-1, 3), p.shape)
    dx, dy, dz = p[:, 0] - ob[:, 0], p[:, 1] - ob[:, 1], p[:, 2] - ob[:, 2]
    block = np.empty((8, p.shape[0]), dtype=np.float64)
    block[0:3] = ob.T
    block[3], block[4], block[5] = dx, dy, dz
    with np.errstate(divide="ignore", invalid="ignore"):
        block[6] = 1e-2 / np.sqrt(dx * dx + dy * dy + dz * dz)
    block[7] = 1.0
    return block


class RayHits:
    """Views over the buffer of a closest-hit batch (``buf``: ``pt_rays_bytes`` bytes, contiguous ``uint8``).  Nothing here
    copies: ``point``, ``normal`` and ``uv`` are strided views ``[n, components]``."""

    def __init__(self, buf, n: int, channels=RAY_CHANNELS):
        self.channels = ray_channels(channels)
        self.n = int(n)
        self.nbytes = rays_bytes(self.n, self.channels, False)
        buf = np.asarray(buf)
        if buf.dtype != np.uint8 or buf.ndim != 1:
            buf = buf.reshape(-1).view(np.uint8)
        if buf.nbytes < self.nbytes:
            raise ValueError(f"ray-batch buffer too small: {buf.nbytes} < {self.nbytes} bytes")
        self.buffer = buf
        self.shape_index = buf[: self.n * 4].view(np.int32)

    def _planes(self, channel: int, count: int) -> np.ndarray:
        if not self.channels & channel:
            name = next(k for k, v in _CHANNEL_OF.items() if v == channel)
            raise KeyError(f"channel {name!r} was not selected for this batch (channels = {self.channels:#x})")
        off = rays_plane_offset(self.n, self.channels, False, channel, 0)
        return self.buffer[off: off + self.n * 8 * count].view(np.float64).reshape(count, self.n)

    def has(self, name: str) -> bool:
        return bool(self.channels & _CHANNEL_OF[name])

    @property
    def hit(self) -> np.ndarray:
        return self.shape_index >= 0

    @property
    def t(self) -> np.ndarray:
        return self._planes(abi.HIT_T, 1)[0]

    @property
    def point(self) -> np.ndarray:
        return self._planes(abi.HIT_POINT, 3).T

    @property
    def normal(self) -> np.ndarray:
        return self._planes(abi.HIT_NORMAL, 3).T

    @property
    def uv(self) -> np.ndarray:
        return self._planes(abi.HIT_UV, 2).T

    def planes(self) -> dict:
        """name -> view, for every selected channel (what the ``rays`` command writes into its ``.npz``)."""
        out = {"shape_index": self.shape_index}
        for name in ("t", "point", "normal", "uv"):
            if self.has(name):
                out[name] = getattr(self, name)
        return out


def surface_channels(channels) -> int:
    """``PT_SURF_*`` bits from an int, names (``"emitted"``, ``"brdf_color,emitted"``), ``"all"`` or ``"none"``."""
    return _parse_channels(channels, _SURF_OF, SURF_ALL, "surface")


def surface_bytes(n: int, channels: int) -> int:
    """Mirror of ``pt_rays_surface_bytes``: 0 for arguments the library refuses."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= SURF_ALL):
        return 0
    return ((n * 4 + 7) & ~7) + n * 24 * bin(channels).count("1")


def surface_plane_offset(n: int, channels: int, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_surface_plane_offset`` (bytes; ``channel`` 0: the int32 plane of BRDF kinds; < 0: not selected)."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= SURF_ALL):
        return -1
    if channel == 0:
        return 0 if component == 0 else -1
    if channel not in (SURF_BRDF_COLOR, SURF_EMITTED) or not channels & channel or not 0 <= component < 3:
        return -1
    before = 3 if channel == SURF_EMITTED and channels & SURF_BRDF_COLOR else 0
    return ((n * 4 + 7) & ~7) + n * 8 * (before + component)


class SurfaceColors(_BatchViews):
    """Views over the buffer of a surface batch (``buf``: ``pt_rays_surface_bytes`` bytes, contiguous ``uint8``): the BRDF kind
    of every record's material (``abi.BRDF_*``; -1 where nothing was hit) and the selected colours.  Nothing here copies:
    ``brdf_color`` and ``emitted`` are strided views with the component as last axis.  ``shape``: what the records' axis is
    viewed as (a frame's ``[nsamp, rows, W]``); default ``[n]``."""

    _names, _all, _what = _SURF_OF, SURF_ALL, "surface"
    _bytes, _offset = staticmethod(surface_bytes), staticmethod(surface_plane_offset)

    def __init__(self, buf, n: int, channels=SURF_ALL, shape=None):
        super().__init__(buf, n, channels, shape)
        self.brdf_kind = self.buffer[: self.n * 4].view(np.int32).reshape(self.shape)

    @property
    def hit(self) -> np.ndarray:
        return self.brdf_kind >= 0

    @property
    def brdf_color(self) -> np.ndarray:
        """``material.brdf.pigment.get_color(uv)`` per record; zeros where nothing was hit."""
        return self._colour(SURF_BRDF_COLOR)

    @property
    def emitted(self) -> np.ndarray:
        """``material.emitted_radiance.get_color(uv)`` per record; zeros where nothing was hit."""
        return self._colour(SURF_EMITTED)

    def planes(self) -> dict:
        out = {"brdf_kind": self.brdf_kind}
        for name in ("brdf_color", "emitted"):
            if self.has(name):
                out[name] = getattr(self, name)
        return out


def scatter_channels(channels) -> int:
    """``PT_SCAT_*`` bits from an int, names (``"weight"``, ``"weight,emitted"``), ``"all"`` or ``"none"``."""
    return _parse_channels(channels, _SCAT_OF, SCAT_ALL, "scatter")


def scatter_bytes(n: int, channels: int) -> int:
    """Mirror of ``pt_rays_scatter_bytes``: 0 for arguments the library refuses."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= SCAT_ALL):
        return 0
    return ((n * 4 + 7) & ~7) + n * 8 * (10 + 3 * bin(channels).count("1"))


def scatter_plane_offset(n: int, channels: int, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_scatter_plane_offset`` (bytes; ``channel`` 0: the int32 status plane, ``SCAT_RAYS``: the eight ray
    planes, ``SCAT_PCG``: state and increment, ``SCAT_WEIGHT`` / ``SCAT_EMITTED``; < 0: not selected)."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= SCAT_ALL):
        return -1
    pad = (n * 4 + 7) & ~7
    if channel == 0:
        return 0 if component == 0 else -1
    if component < 0:
        return -1
    if channel == SCAT_RAYS:
        return pad + n * 8 * component if component < 8 else -1
    if channel == SCAT_PCG:
        return pad + n * 8 * (8 + component) if component < 2 else -1
    if channel not in (SCAT_WEIGHT, SCAT_EMITTED) or not channels & channel or component >= 3:
        return -1
    before = 3 if channel == SCAT_EMITTED and channels & SCAT_WEIGHT else 0
    return pad + n * 8 * (10 + before + component)


class ScatteredRays(_BatchViews):
    """Views over the buffer of a scatter batch (``buf``: ``pt_rays_scatter_bytes`` bytes, contiguous ``uint8``).  Nothing here
    copies.  ``status``: -1 no hit, 0 terminated (by the roulette or a black BRDF pigment: the record's value is ``emitted``),
    1 scattered; ``rays``: the ``[8, n]`` block ``trace_rays`` reads (a dead ray where ``status != 1``: it hits nothing);
    ``pcg_state`` / ``pcg_inc``: every record's generator behind its draws; ``weight`` (the BRDF pigment's colour behind the
    roulette's compensation) and ``emitted`` with the component as last axis.  ``shape``: what the records' axis is viewed as."""

    _names, _all, _what = _SCAT_OF, SCAT_ALL, "scatter"
    _bytes, _offset = staticmethod(scatter_bytes), staticmethod(scatter_plane_offset)

    def __init__(self, buf, n: int, channels=SCAT_ALL, shape=None):
        super().__init__(buf, n, channels, shape)
        buf = self.buffer
        self.status = buf[: self.n * 4].view(np.int32).reshape(self.shape)
        off = scatter_plane_offset(self.n, self.channels, SCAT_RAYS, 0)
        self.rays = buf[off: off + self.n * 64].view(np.float64).reshape(8, self.n)
        pcg = buf[off + self.n * 64: off + self.n * 80].view(np.uint64).reshape(2, self.n)
        self.pcg = pcg  # [2, n]: what the next scatter takes as it is
        self.pcg_state, self.pcg_inc = pcg[0].reshape(self.shape), pcg[1].reshape(self.shape)

    @property
    def scattered(self) -> np.ndarray:
        return self.status == 1

    @property
    def dirs(self) -> np.ndarray:
        """``[n, 3]``: the scattered directions -- the next step's ``dirs`` (a view of three of the ray planes)."""
        return self.rays[3:6].T

    @property
    def weight(self) -> np.ndarray:
        return self._colour(SCAT_WEIGHT)

    @property
    def emitted(self) -> np.ndarray:
        return self._colour(SCAT_EMITTED)

    def planes(self) -> dict:
        out = {"status": self.status, "rays": self.rays, "pcg_state": self.pcg_state, "pcg_inc": self.pcg_inc}
        for name in ("weight", "emitted"):
            if self.has(name):
                out[name] = getattr(self, name)
        return out


def radiance_channels(channels) -> int:
    """``PT_RAD_*`` bits from an int, names (``"pcg"``, ``"pcg,count"``), ``"all"`` or ``"none"``."""
    return _parse_channels(channels, _RAD_OF, RAD_ALL, "radiance")


def radiance_bytes(n: int, channels: int) -> int:
    """Mirror of ``pt_rays_radiance_bytes``: 0 for arguments the library refuses."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= RAD_ALL):
        return 0
    return n * 8 * (3 + (2 if channels & RAD_PCG else 0) + (1 if channels & RAD_COUNT else 0))


def radiance_plane_offset(n: int, channels: int, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_radiance_plane_offset`` (bytes; ``channel`` 0: the three radiance planes, ``RAD_PCG``: state and
    increment, ``RAD_COUNT``; < 0: not selected)."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= RAD_ALL) or component < 0:
        return -1
    if channel == 0:
        return n * 8 * component if component < 3 else -1
    if channel == RAD_PCG and channels & RAD_PCG:
        return n * 8 * (3 + component) if component < 2 else -1
    if channel == RAD_COUNT and channels & RAD_COUNT:
        return n * 8 * (3 + (2 if channels & RAD_PCG else 0)) if component < 1 else -1
    return -1


class RayRadiance(_BatchViews):
    """Views over the buffer of a radiance batch (``buf``: ``pt_rays_radiance_bytes`` bytes, contiguous ``uint8``).  Nothing
    here copies.  ``radiance``: ``PathTracer(...)(ray)`` per ray with the component as last axis; ``pcg`` (``[2, n]``),
    ``pcg_state`` / ``pcg_inc``: every ray's generator behind its draws; ``n_rays``: the rays handed to a world query for it
    (``uint64``).  ``shape``: what the rays' axis is viewed as (a frame's ``[nsamp, rows, W]``); default ``[n]``."""

    _names, _all, _what, _unit = _RAD_OF, RAD_ALL, "radiance", "rays"
    _bytes, _offset = staticmethod(radiance_bytes), staticmethod(radiance_plane_offset)

    def __init__(self, buf, n: int, channels=RAD_ALL, shape=None):
        super().__init__(buf, n, channels, shape)
        self.radiance = np.moveaxis(self.buffer[: self.n * 24].view(np.float64).reshape((3,) + self.shape), 0, -1)

    @property
    def pcg(self) -> np.ndarray:
        return self._plane_views(RAD_PCG, 2, np.uint64)

    @property
    def pcg_state(self) -> np.ndarray:
        return self.pcg[0].reshape(self.shape)

    @property
    def pcg_inc(self) -> np.ndarray:
        return self.pcg[1].reshape(self.shape)

    @property
    def n_rays(self) -> np.ndarray:
        return self._plane_views(RAD_COUNT, 1, np.uint64)[0].reshape(self.shape)

    def planes(self) -> dict:
        """name -> view, for every selected channel (what the ``radiance`` command writes into its ``.npz``)."""
        out = {"radiance": self.radiance}
        if self.has("pcg"):
            out["pcg_state"], out["pcg_inc"] = self.pcg_state, self.pcg_inc
        if self.has("count"):
            out["n_rays"] = self.n_rays
        return out


def gather_channels(channels) -> int:
    """``PT_GATHER_*`` bits from an int, a name (``"count"``), ``"all"`` or ``"none"``."""
    return _parse_channels(channels, _GATHER_OF, GATHER_ALL, "gather")


def gather_bytes(n: int, channels: int) -> int:
    """Mirror of ``pt_rays_gather_bytes``: 0 for arguments the library refuses."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= GATHER_ALL):
        return 0
    return n * 8 * (3 + (1 if channels & GATHER_COUNT else 0))


def gather_plane_offset(n: int, channels: int, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_gather_plane_offset`` (bytes; ``channel`` 0: the three radiance planes, ``GATHER_COUNT``; < 0: not
    selected)."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= GATHER_ALL) or component < 0:
        return -1
    if channel == 0:
        return n * 8 * component if component < 3 else -1
    if channel == GATHER_COUNT and channels & GATHER_COUNT:
        return n * 24 if component < 1 else -1
    return -1


class GatheredRadiance(_BatchViews):
    """Views over the buffer of a gather batch (``buf``: ``pt_rays_gather_bytes`` bytes, contiguous ``uint8``).  Nothing here
    copies.  ``radiance``: per record the mean of ``PathTracer(...)(ray)`` over its ``samples`` hemisphere rays, summed in sample
    order, with the component as last axis; ``n_rays``: the rays handed to a world query for the record (``uint64``).  ``shape``:
    what the records' axis is viewed as (a frame's ``[nsamp, rows, W]``); default ``[n]``."""

    _names, _all, _what = _GATHER_OF, GATHER_ALL, "gather"
    _bytes, _offset = staticmethod(gather_bytes), staticmethod(gather_plane_offset)

    def __init__(self, buf, n: int, channels=GATHER_ALL, shape=None):
        super().__init__(buf, n, channels, shape)
        self.radiance = np.moveaxis(self.buffer[: self.n * 24].view(np.float64).reshape((3,) + self.shape), 0, -1)

    def has(self, name: str) -> bool:  # (any other name is a channel this batch does not have, not an error)
        return name in _GATHER_OF and super().has(name)

    @property
    def n_rays(self) -> np.ndarray:
        return self._plane_views(GATHER_COUNT, 1, np.uint64)[0].reshape(self.shape)

    def planes(self) -> dict:
        """name -> view, for every selected channel (what the ``gather`` command writes into its ``.npz``)."""
        out = {"radiance": self.radiance}
        if self.has("count"):
            out["n_rays"] = self.n_rays
        return out


def adaptive_channels(channels) -> int:
    """``PT_ADAPTIVE_*`` bits from an int, names (``"count"``, ``"taken"``, ``"count,taken"``), ``"all"`` or ``"none"``."""
    return _parse_channels(channels, _ADAPTIVE_OF, ADAPTIVE_ALL, "adaptive")


def adaptive_bytes(n: int, channels: int) -> int:
    """Mirror of ``pt_rays_adaptive_bytes``: 0 for arguments the library refuses.  The ``taken`` plane (int32) is padded to 8 bytes."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= ADAPTIVE_ALL):
        return 0
    return n * 24 + (n * 8 if channels & ADAPTIVE_COUNT else 0) + ((n * 4 + 7) // 8 * 8 if channels & ADAPTIVE_TAKEN else 0)


def adaptive_plane_offset(n: int, channels: int, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_adaptive_plane_offset`` (bytes; ``channel`` 0: the three radiance planes, ``ADAPTIVE_COUNT``,
    ``ADAPTIVE_TAKEN``; < 0: not selected)."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= ADAPTIVE_ALL) or component < 0:
        return -1
    if channel == 0:
        return n * 8 * component if component < 3 else -1
    if component > 0:
        return -1
    if channel == ADAPTIVE_COUNT and channels & ADAPTIVE_COUNT:
        return n * 24
    if channel == ADAPTIVE_TAKEN and channels & ADAPTIVE_TAKEN:
        return n * 24 + (n * 8 if channels & ADAPTIVE_COUNT else 0)
    return -1


class RaggedRadiance(_BatchViews):
    """Views over the buffer of a ragged gather (``buf``: ``pt_rays_adaptive_bytes`` bytes, contiguous ``uint8``).  Nothing here
    copies.  ``radiance``: per record the mean of ``PathTracer(...)(ray)`` over the ``taken`` hemisphere rays it was given, summed in
    sample order, with the component as last axis (black where ``taken`` is 0); ``n_rays``: the rays handed to a world query for the
    record (``uint64``); ``taken``: the samples the record took (``int32``).  ``shape``: what the records' axis is viewed as."""

    _names, _all, _what = _ADAPTIVE_OF, ADAPTIVE_ALL, "adaptive"
    _bytes, _offset = staticmethod(adaptive_bytes), staticmethod(adaptive_plane_offset)

    def __init__(self, buf, n: int, channels=ADAPTIVE_ALL, shape=None):
        super().__init__(buf, n, channels, shape)
        self.radiance = np.moveaxis(self.buffer[: self.n * 24].view(np.float64).reshape((3,) + self.shape), 0, -1)

    def has(self, name: str) -> bool:  # (any other name is a channel this batch does not have, not an error)
        return name in _ADAPTIVE_OF and super().has(name)

    @property
    def n_rays(self) -> np.ndarray:
        return self._plane_views(ADAPTIVE_COUNT, 1, np.uint64)[0].reshape(self.shape)

    @property
    def taken(self) -> np.ndarray:
        if not self.channels & ADAPTIVE_TAKEN:
            raise KeyError(f"channel 'taken' was not selected for this adaptive batch (channels = {self.channels:#x})")
        off = adaptive_plane_offset(self.n, self.channels, ADAPTIVE_TAKEN)
        return self.buffer[off: off + self.n * 4].view(np.int32).reshape(self.shape)

    def planes(self) -> dict:
        """name -> view, for every selected channel."""
        out = {"radiance": self.radiance}
        if self.has("count"):
            out["n_rays"] = self.n_rays
        if self.has("taken"):
            out["taken"] = self.taken
        return out


def bake_channels(channels) -> int:
    """``PT_BAKE_*`` bits from an int, a name (``"count"``), ``"all"`` or ``"none"``."""
    return _parse_channels(channels, _BAKE_OF, BAKE_ALL, "bake")


def bake_bytes(texels: int, channels: int) -> int:
    """Mirror of ``pt_rays_bake_bytes`` (``texels`` = w * h of the baked rectangle): 0 for arguments the library refuses."""
    if not (0 <= texels <= MAX_RAYS and 0 <= channels <= BAKE_ALL):
        return 0
    return texels * 8 * (3 + (1 if channels & BAKE_COUNT else 0))


def bake_plane_offset(texels: int, channels: int, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_bake_plane_offset`` (bytes; ``channel`` 0: the three radiance planes, ``BAKE_COUNT``; < 0: not
    selected)."""
    if not (0 <= texels <= MAX_RAYS and 0 <= channels <= BAKE_ALL) or component < 0:
        return -1
    if channel == 0:
        return texels * 8 * component if component < 3 else -1
    if channel == BAKE_COUNT and channels & BAKE_COUNT:
        return texels * 24 if component < 1 else -1
    return -1


class BakedMap(_BatchViews):
    """Views over the buffer of a bake (``buf``: ``pt_rays_bake_bytes(w * h)`` bytes, contiguous ``uint8``) of a ``w x h``
    rectangle of texels, row-major: row ``r`` is ``v``, column ``c`` is ``u`` -- an ``ImagePigment``'s ``(col, row)``.  Nothing here
    copies.  ``radiance``: ``[h, w, 3]``, per texel the mean of ``PathTracer(...)(ray)`` over its samples, summed in sample order;
    ``n_rays``: ``[h, w]`` uint64, the rays handed to a world query for the texel."""

    _names, _all, _what, _unit = _BAKE_OF, BAKE_ALL, "bake", "texels"
    _bytes, _offset = staticmethod(bake_bytes), staticmethod(bake_plane_offset)

    def __init__(self, buf, width: int, height: int, channels=BAKE_ALL):
        self.width, self.height = int(width), int(height)
        super().__init__(buf, self.width * self.height, channels, (self.height, self.width))
        self.radiance = np.moveaxis(self.buffer[: self.n * 24].view(np.float64).reshape((3,) + self.shape), 0, -1)

    def has(self, name: str) -> bool:  # (any other name is a channel this bake does not have, not an error)
        return name in _BAKE_OF and super().has(name)

    @property
    def n_rays(self) -> np.ndarray:
        return self._plane_views(BAKE_COUNT, 1, np.uint64)[0].reshape(self.shape)

    def planes(self) -> dict:
        """name -> view, for every selected channel."""
        out = {"radiance": self.radiance}
        if self.has("count"):
            out["n_rays"] = self.n_rays
        return out


def sh_channels(channels) -> int:
    """``PT_SH_*`` bits from an int, a name (``"count"``), ``"all"`` or ``"none"``."""
    return _parse_channels(channels, _SH_OF, SH_ALL, "probe")


def sh_bytes(n: int, channels: int) -> int:
    """Mirror of ``pt_rays_sh_bytes``: 0 for arguments the library refuses."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= SH_ALL):
        return 0
    return n * 8 * (SH_COEFFS + (1 if channels & SH_COUNT else 0))


def sh_plane_offset(n: int, channels: int, channel: int, component: int = 0) -> int:
    """Mirror of ``pt_rays_sh_plane_offset`` (bytes; ``channel`` 0: the 27 coefficient planes, component ``3 j + ch``;
    ``SH_COUNT``; < 0: not selected)."""
    if not (0 <= n <= MAX_RAYS and 0 <= channels <= SH_ALL) or component < 0:
        return -1
    if channel == 0:
        return n * 8 * component if component < SH_COEFFS else -1
    if channel == SH_COUNT and channels & SH_COUNT:
        return n * 8 * SH_COEFFS if component < 1 else -1
    return -1


def sh_dirs_bytes(n: int, samples: int) -> int:
    """Mirror of ``pt_rays_sh_dirs_bytes``."""
    if not (0 <= n <= MAX_RAYS and samples >= 1 and n * samples <= MAX_RAYS):
        return 0
    return n * samples * 24


def sh_basis(dirs) -> np.ndarray:
    """``[..., 3]`` directions -> ``[..., 9]``: the nine real SH functions of bands 0 - 2 as include/ptrace_sh.h states them
    (the literals, the order of the products; the directions are not normalised) -- the library's bits, in numpy."""
    d = np.asarray(dirs, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = np.empty(d.shape[:-1] + (9,), dtype=np.float64)
    out[..., 0] = SH_K0
    out[..., 1] = SH_K1 * y
    out[..., 2] = SH_K1 * z
    out[..., 3] = SH_K1 * x
    out[..., 4] = SH_K2 * (x * y)
    out[..., 5] = SH_K2 * (y * z)
    out[..., 6] = SH_K3 * (3.0 * (z * z) - 1.0)
    out[..., 7] = SH_K2 * (x * z)
    out[..., 8] = SH_K4 * (x * x - y * y)
    return out


def sh_evaluate(coefficients, dirs, kind: int = SH_RADIANCE) -> np.ndarray:
    """The evaluation of include/ptrace_sh.h in numpy, operation for operation: ``coefficients`` ``[..., 9, 3]`` and ``dirs``
    ``[..., 3]`` (record by record) -> ``[..., 3]``."""
    if kind not in (SH_RADIANCE, SH_HEMISPHERE):
        raise ValueError(f"kind {kind}: an evaluation is SH_RADIANCE (0) or SH_HEMISPHERE (1)")
    c = np.asarray(coefficients, dtype=np.float64)
    y = sh_basis(dirs)
    out = np.zeros(np.broadcast_shapes(c.shape[:-2], y.shape[:-1]) + (3,), dtype=np.float64)
    for j in range(9):
        a = SH_BAND_FACTORS[j] if kind == SH_HEMISPHERE else 1.0
        out = out + (a * y[..., j])[..., None] * c[..., j, :]
    return out


class ProbeSet(_BatchViews):
    """Views over the buffer of a probe batch (``buf``: ``pt_rays_sh_bytes`` bytes, contiguous ``uint8``).  Nothing here copies.
    ``coefficients``: ``[..., 9, 3]``, per probe the order-2 SH coefficients ``c[j][ch]`` of the radiance arriving there;
    ``block``: the same memory as the ``[27, n]`` planes the library reads (plane ``3 j + ch``); ``n_rays``: the rays handed to a
    world query for the probe (``uint64``).  ``shape``: what the probes' axis is viewed as; default ``[n]``.  ``evaluator``:
    ``DeviceScene.sh_eval`` of the scene the probes came from (the evaluation reads no scene: any device scene's will do)."""

    _names, _all, _what, _unit = _SH_OF, SH_ALL, "probe", "probes"
    _bytes, _offset = staticmethod(sh_bytes), staticmethod(sh_plane_offset)

    def __init__(self, buf, n: int, channels=SH_ALL, shape=None, evaluator=None):
        super().__init__(buf, n, channels, shape)
        self.evaluator = evaluator
        self.block = self.buffer[: self.n * 8 * SH_COEFFS].view(np.float64).reshape(SH_COEFFS, self.n)
        self.coefficients = np.moveaxis(self.block.reshape((9, 3) + self.shape), (0, 1), (-2, -1))

    def has(self, name: str) -> bool:  # (any other name is a channel this batch does not have, not an error)
        return name in _SH_OF and super().has(name)

    @property
    def n_rays(self) -> np.ndarray:
        return self._plane_views(SH_COUNT, 1, np.uint64)[0].reshape(self.shape)

    def planes(self) -> dict:
        """name -> view, for every selected channel (what the ``probes`` command writes into its ``.npz``)."""
        out = {"coefficients": self.coefficients}
        if self.has("count"):
            out["n_rays"] = self.n_rays
        return out

    def _eval(self, dirs, index, kind) -> np.ndarray:
        if self.evaluator is None:
            raise ValueError("this ProbeSet has no evaluator: pass evaluator=DeviceScene.sh_eval (or use rays.sh_evaluate on the host)")
        d = np.asarray(dirs, dtype=np.float64)
        if d.ndim < 1 or d.shape[-1] != 3:
            raise ValueError(f"expected [..., 3] directions, not {d.shape}")
        lead = d.shape[:-1]
        if index is not None:
            index = np.broadcast_to(np.asarray(index), lead).reshape(-1)
        out = self.evaluator(self.block, planar(d, 3), index, kind)
        return np.ascontiguousarray(out.T).reshape(lead + (3,))

    def radiance(self, dirs, index=None) -> np.ndarray:
        """The band-limited radiance arriving from ``dirs`` (``[..., 3]``; used as they are) at probe ``index`` (one value or
        one per record; ``None``: record ``r`` reads probe ``r``) -> ``[..., 3]``, on the device (``sh_eval``)."""
        return self._eval(dirs, index, SH_RADIANCE)

    def hemisphere_mean(self, normals, index=None) -> np.ndarray:
        """``(1 / pi) *`` the integral of the radiance times the cosine over the hemisphere around ``normals`` (``[..., 3]``, unit
        length) at probe ``index`` -- what a gather record or a light-map texel holds -> ``[..., 3]``, on the device."""
        return self._eval(normals, index, SH_HEMISPHERE)


class ProbeGrid:
    """A lattice of probe positions on the host: ``dims = (nx, ny, nz)`` points from ``origin`` in steps of ``step`` (one number
    or three).  Probe ``(ix, iy, iz)`` has the index ``(iz * ny + iy) * nx + ix``."""

    def __init__(self, origin, step, dims):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3)
        self.step = np.broadcast_to(np.asarray(step, dtype=np.float64), (3,)).copy()
        self.dims = tuple(int(x) for x in dims)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError(f"dims must be three counts of at least 1, not {dims}")
        if not np.all(self.step > 0.0):
            raise ValueError(f"step must be positive, not {step}")
        self.n = self.dims[0] * self.dims[1] * self.dims[2]

    def points(self) -> np.ndarray:
        """``[n, 3]``: the probes' positions in index order -- the ``points`` of ``radiance_probes``."""
        nx, ny, nz = self.dims
        iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        idx = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3).astype(np.float64)
        return self.origin + idx * self.step

    def corners(self, points):
        """``(index [m, 8], weight [m, 8])``: the eight probes around every point and their trilinear weights (a point outside
        the lattice takes the nearest cell's border)."""
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        top = np.maximum(np.asarray(self.dims) - 2, 0)
        g = (p - self.origin) / self.step
        near = np.rint(g)
        g = np.where(np.abs(g - near) <= 4.0 * np.finfo(np.float64).eps * np.maximum(np.abs(g), 1.0), near, g)  # a lattice point is ON it
        i0 = np.clip(np.floor(g), 0, top).astype(np.int64)
        f = np.clip(g - i0, 0.0, 1.0)
        i1 = np.minimum(i0 + 1, np.asarray(self.dims) - 1)
        nx, ny, _ = self.dims
        index = np.empty((p.shape[0], 8), dtype=np.int64)
        weight = np.empty((p.shape[0], 8), dtype=np.float64)
        for c in range(8):
            bx, by, bz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            ix, iy, iz = (i1 if bx else i0)[:, 0], (i1 if by else i0)[:, 1], (i1 if bz else i0)[:, 2]
            index[:, c] = (iz * ny + iy) * nx + ix
            weight[:, c] = (f[:, 0] if bx else 1.0 - f[:, 0]) * (f[:, 1] if by else 1.0 - f[:, 1]) * (f[:, 2] if bz else 1.0 - f[:, 2])
        return index, weight

    def blend(self, probes: "ProbeSet", points) -> "ProbeSet":
        """Per point the coefficients blended from the eight probes around it by trilinear weights (numpy) -> a :class:`ProbeSet`
        of one record per point, whose ``radiance`` / ``hemisphere_mean`` (``index=None``) evaluate the blend."""
        if probes.n != self.n:
            raise ValueError(f"{probes.n} probes for a lattice of {self.n}")
        p = np.asarray(points, dtype=np.float64)
        lead = p.shape[:-1]
        index, weight = self.corners(p)
        m = index.shape[0]
        buf = np.zeros(max(sh_bytes(m, 0), 8), dtype=np.uint8)
        out = ProbeSet(buf, m, 0, shape=lead, evaluator=probes.evaluator)
        block = probes.block
        for c in range(8):
            out.block[:] = out.block + weight[:, c][None, :] * block[:, index[:, c]]
        return out

    def evaluate(self, probes: "ProbeSet", points, dirs, kind: int = SH_RADIANCE, active=None) -> np.ndarray:
        """What ``blend(probes, points)`` evaluated towards ``dirs`` gives -- ``radiance`` (``kind=SH_RADIANCE``) or
        ``hemisphere_mean`` (``SH_HEMISPHERE``) -- in every bit, on the device in ONE kernel (``DeviceScene.lit_eval`` of the scene
        ``probes.evaluator`` belongs to; include/ptrace_lit.h): no blended block is made.  ``points``, ``dirs``: ``[..., 3]``;
        ``active``: optional int32 per record, negative = zeros -> ``[..., 3]``.  A NaN point gives zeros."""
        if probes.n != self.n:
            raise ValueError(f"{probes.n} probes for a lattice of {self.n}")
        scene = getattr(probes.evaluator, "__self__", None)
        if scene is None or not callable(getattr(scene, "lit_eval", None)):
            raise ValueError("this ProbeSet has no device scene behind its evaluator: pass evaluator=DeviceScene.sh_eval (or use rays.lit_eval_host)")
        p, d = np.asarray(points, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
        if p.ndim < 1 or p.shape[-1] != 3 or d.shape != p.shape:
            raise ValueError(f"expected [..., 3] points and as many directions, not {p.shape} and {d.shape}")
        out = scene.lit_eval(self, probes.block, planar(p, 3), planar(d, 3), active, kind)
        return np.ascontiguousarray(out.T).reshape(p.shape)


def _unit_rows(a) -> np.ndarray:
    """``Vec.normalize`` / ``Normal.normalize`` (geometry.py:130-136, 219-225) per row, with ``x * x`` for ``x**2`` as the device."""
    x, y, z = a[..., 0], a[..., 1], a[..., 2]
    with np.errstate(all="ignore"):  # (a record without a hit holds a zero normal: NaN, as on the device)
        return a / np.sqrt(x * x + y * y + z * z)[..., None]


def mirror_directions(dirs, normals) -> np.ndarray:
    """The direction ``SpecularBRDF.scatter_ray`` (materials.py:186-192) sends a ray arriving along ``dirs`` at ``normals``
    (``[..., 3]`` both), as the device's ``scatter_ray`` forms it: ``rd - (nn . rd) * (2.0 * nn)`` of the two normalised vectors."""
    rd, nn = _unit_rows(np.asarray(dirs, dtype=np.float64)), _unit_rows(np.asarray(normals, dtype=np.float64))
    dp = nn[..., 0] * rd[..., 0] + nn[..., 1] * rd[..., 1] + nn[..., 2] * rd[..., 2]
    return rd - dp[..., None] * (2.0 * nn)


def lit_eval_host(grid: ProbeGrid, probes: ProbeSet, points, dirs, kind: int = SH_RADIANCE, active=None) -> np.ndarray:
    """The numpy mirror of the lit query (include/ptrace_lit.h), made of ``ProbeGrid.corners`` / ``blend`` and :func:`sh_evaluate``
    alone: ``[m, 3]`` points and directions -> ``[m, 3]``.  The one case numpy leaves undefined follows the library's rule: a NaN
    coordinate gives ``+0.0`` (the record is blended at the lattice's origin, then replaced); ``active < 0`` gives zeros."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    nan = np.isnan(p).any(axis=1)
    with np.errstate(all="ignore"):
        blended = grid.blend(probes, np.where(nan[:, None], grid.origin[None, :], p))
        out = sh_evaluate(blended.coefficients, d, kind)
    out[nan] = 0.0
    if active is not None:
        out[np.asarray(active).reshape(-1) < 0] = 0.0
    return out


def lit_shade_host(grid: ProbeGrid, probes: ProbeSet, materials, point, normal, dirs, background=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The numpy mirror of the shade query (include/ptrace_lit.h), operation for operation.  ``materials``: the records'
    :class:`SurfaceColors` (``WorldQueries.materials``: BRDF kind, ``brdf_color``, ``emitted``); ``point``, ``normal``, ``dirs``:
    ``[..., 3]`` as a hit frame or a :class:`RayHits` has them -> ``[..., 3]``: ``background`` where nothing was hit, else
    ``emitted + brdf_color * E`` with ``E`` the blend at ``point`` (:meth:`ProbeGrid.corners`, :meth:`ProbeGrid.blend`) evaluated
    (:func:`sh_evaluate`) as the hemisphere mean around the normalised normal (``DiffuseBRDF``) or as the radiance from
    :func:`mirror_directions` (``SpecularBRDF``).  Records without a hit are not evaluated; a NaN point gives ``E = +0.0``."""
    kind = np.asarray(materials.brdf_kind)
    lead = kind.shape
    kind = kind.reshape(-1)
    p = np.asarray(point, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    bg = (background.r, background.g, background.b) if hasattr(background, "r") else tuple(float(x) for x in background)
    out = np.empty((kind.shape[0], 3), dtype=np.float64)
    out[:] = bg
    pc, em = np.asarray(materials.brdf_color).reshape(-1, 3), np.asarray(materials.emitted).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for brdf, sh_kind in ((abi.BRDF_DIFFUSE, SH_HEMISPHERE), (abi.BRDF_SPECULAR, SH_RADIANCE)):
            rows = np.flatnonzero(kind == brdf)
            if rows.size == 0:
                continue
            towards = _unit_rows(nrm[rows]) if brdf == abi.BRDF_DIFFUSE else mirror_directions(d[rows], nrm[rows])
            out[rows] = em[rows] + pc[rows] * lit_eval_host(grid, probes, p[rows], towards, sh_kind)
    return out.reshape(lead + (3,))


DENOISE_KERNEL = (0.0625, 0.25, 0.375, 0.25, 0.0625)  # h of include/ptrace_denoise.h: the B3 spline; every product of two is exact


def denoise_host(colour, shape, normal, point, width: int, height: int, passes: int = 4, sigma_point: float = 0.1, normal_power_log2: int = 5,
                 sigma_colour: float = float("inf"), same_shape: bool = True, wrap_x: bool = False) -> np.ndarray:
    """The numpy mirror of the denoise query (include/ptrace_denoise.h), operation for operation: vectorised per tap over the whole
    frame, the taps in the header's order (``dy`` outer, ``dx`` inner), every sum in that order.  ``colour``, ``normal``, ``point``:
    ``width * height`` records of 3 in row-major order (any leading shape), ``shape``: as many int32, negative = copied ->
    ``[height, width, 3]``.  Refuses what the library refuses, with a ``ValueError``."""
    W, H, passes, e = int(width), int(height), int(passes), int(normal_power_log2)
    sigma_point, sigma_colour = float(sigma_point), float(sigma_colour)
    if W < 0 or H < 0 or W * H > MAX_RAYS:
        raise ValueError(f"a frame of {W} x {H} records")
    if not 1 <= passes <= 10 or not 0 <= e <= 10:
        raise ValueError(f"passes={passes} (1 to 10), normal_power_log2={e} (0 to 10)")
    if not sigma_point > 0.0 or not sigma_colour > 0.0:
        raise ValueError(f"sigma_point={sigma_point}, sigma_colour={sigma_colour}: a sigma is positive (or inf)")
    cur = np.array(colour, dtype=np.float64).reshape(H, W, 3)
    sh = np.asarray(shape, dtype=np.int32).reshape(H, W)
    nrm = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    pnt = np.asarray(point, dtype=np.float64).reshape(H, W, 3)
    if W * H == 0:
        return cur
    active = sh >= 0
    rows, cols = np.arange(H), np.arange(W)
    with np.errstate(all="ignore"):
        unit = nrm / np.sqrt(nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1] + nrm[..., 2] * nrm[..., 2])[..., None]
        for i in range(passes):
            s = 2 ** i
            sps = sigma_point * float(s)
            sc = sigma_colour * 2.0 ** -i
            sc2 = sc * sc
            total, wsum = np.zeros((H, W, 3)), np.zeros((H, W))
            for dy in range(-2, 3):
                qy = rows + s * dy
                in_y = (qy >= 0) & (qy < H)
                qy = np.clip(qy, 0, H - 1)
                for dx in range(-2, 3):
                    k = DENOISE_KERNEL[dx + 2] * DENOISE_KERNEL[dy + 2]
                    if dx == 0 and dy == 0:
                        total, wsum = total + k * cur, wsum + k
                        continue
                    qx = cols + s * dx
                    if wrap_x:
                        qx, in_x = qx % W, np.ones(W, dtype=bool)
                    else:
                        in_x = (qx >= 0) & (qx < W)
                        qx = np.clip(qx, 0, W - 1)
                    at = np.ix_(qy, qx)
                    sq, nq, pq, cq = sh[at], unit[at], pnt[at], cur[at]
                    take = in_y[:, None] & in_x[None, :] & (sq >= 0)
                    if same_shape:
                        take = take & (sq == sh)
                    c = unit[..., 0] * nq[..., 0] + unit[..., 1] * nq[..., 1] + unit[..., 2] * nq[..., 2]
                    c = np.where(c > 0.0, c, 0.0)
                    for _ in range(e):
                        c = c * c
                    d = pq - pnt
                    dz = unit[..., 0] * d[..., 0] + unit[..., 1] * d[..., 1] + unit[..., 2] * d[..., 2]
                    t = dz / sps
                    wp = 1.0 / (1.0 + t * t)
                    dc = cq - cur
                    d2 = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                    wc = 1.0 / (1.0 + d2 / sc2)
                    w = ((k * c) * wp) * wc
                    take = take & (w > 0.0)
                    total = np.where(take[..., None], total + w[..., None] * cq, total)
                    wsum = np.where(take, wsum + w, wsum)
            cur = np.where(active[..., None], total / wsum[..., None], cur)
    return cur


def temporal_project_host(prev_camera, points, width: int, height: int):
    """Steps 2 to 5 of include/ptrace_temporal.h, operation for operation: where ``points`` (``[..., 3]``) were on the screen of
    ``prev_camera`` (anything ``_temporal_lib.camera`` takes), in pixels of a ``width x height`` frame -> ``(fx, fy, ok)``;
    ``ok`` is False where there is no history (behind the camera, off the screen, NaN) and ``fx``, ``fy`` mean nothing there."""
    from . import _temporal_lib

    cam = _temporal_lib.camera(prev_camera)
    if cam.kind not in (abi.CAMERA_ORTHOGONAL, abi.CAMERA_PERSPECTIVE):
        raise ValueError(f"unknown camera kind {cam.kind}")
    m, d, a = [float(x) for x in cam.invm], float(cam.screen_distance), float(cam.aspect_ratio)
    p = np.asarray(points, dtype=np.float64)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        qx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
        qy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7]
        qz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]
        if cam.kind == abi.CAMERA_PERSPECTIVE:
            tn = qx + d
            s = d / tn
            u = (1.0 - (qy * s) / a) * 0.5
            v = (1.0 + qz * s) * 0.5
        else:
            tn = qx + 1.0
            u = (1.0 - qy / a) * 0.5
            v = (1.0 + qz) * 0.5
        fx = u * float(int(width)) - 0.5
        fy = (1.0 - v) * float(int(height)) - 0.5
        ok = (tn > 0.0) & (fx > -1.0) & (fx < float(int(width))) & (fy > -1.0) & (fy < float(int(height)))
    return fx, fy, ok


def temporal_host(colour, shape, normal, point, prev_colour, prev_shape, prev_normal, prev_point, prev_count, prev_camera, width: int,
                  height: int, max_history: int = 32, same_shape: bool = True, normal_min: float = 0.9, point_tolerance: float = 0.05,
                  _tap_order=(0, 1, 2, 3)):
    """The numpy mirror of the accumulate query (include/ptrace_temporal.h), operation for operation: vectorised per tap over the
    whole frame, the four taps in the header's order, every sum in that order.  The planes: ``width * height`` records in row-major
    order (any leading shape), the previous frame's like the current one's plus ``prev_count``; ``prev_camera``: anything
    ``_temporal_lib.camera`` takes -> ``(out [height, width, 3] float64, count [height, width] int32)``.  Refuses what the library
    refuses, with a ``ValueError``.  (``_tap_order`` is for the test that the order of the sums reaches the bits.)"""
    W, H, max_history = int(width), int(height), int(max_history)
    normal_min, point_tolerance = float(normal_min), float(point_tolerance)
    if W < 0 or H < 0 or W * H > MAX_RAYS:
        raise ValueError(f"a frame of {W} x {H} records")
    if not 1 <= max_history <= 2 ** 20:
        raise ValueError(f"max_history={max_history}: 1 to 2^20")
    if not -1.0 <= normal_min <= 1.0 or not point_tolerance > 0.0:
        raise ValueError(f"normal_min={normal_min} (a cosine, -1 to 1), point_tolerance={point_tolerance} (positive, or inf)")
    cur = np.array(colour, dtype=np.float64).reshape(H, W, 3)
    sh = np.asarray(shape, dtype=np.int32).reshape(H, W)
    nrm = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    pnt = np.asarray(point, dtype=np.float64).reshape(H, W, 3)
    pcol = np.asarray(prev_colour, dtype=np.float64).reshape(H, W, 3)
    psh = np.asarray(prev_shape, dtype=np.int32).reshape(H, W)
    pnrm = np.asarray(prev_normal, dtype=np.float64).reshape(H, W, 3)
    ppnt = np.asarray(prev_point, dtype=np.float64).reshape(H, W, 3)
    pcnt = np.asarray(prev_count, dtype=np.int32).reshape(H, W)
    fx, fy, ok = temporal_project_host(prev_camera, pnt, W, H)
    if W * H == 0:
        return cur, np.zeros((H, W), dtype=np.int32)
    hit = sh >= 0
    ok = ok & hit
    with np.errstate(all="ignore"):
        unit = nrm / np.sqrt(nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1] + nrm[..., 2] * nrm[..., 2])[..., None]
        punit = pnrm / np.sqrt(pnrm[..., 0] * pnrm[..., 0] + pnrm[..., 1] * pnrm[..., 1] + pnrm[..., 2] * pnrm[..., 2])[..., None]
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        bx, by = (1.0 - ax, ax), (1.0 - ay, ay)
        hs, ws = np.zeros((H, W, 3)), np.zeros((H, W))
        nmax, some = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=bool)
        for t in _tap_order:
            x, y = x0 + (t & 1), y0 + (t >> 1)
            take = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            at = (np.clip(y, 0, H - 1), np.clip(x, 0, W - 1))
            sq, nq, nu, pq, cq = psh[at], pcnt[at].astype(np.int64), punit[at], ppnt[at], pcol[at]
            take = take & (nq > 0) & (sq >= 0)
            if same_shape:
                take = take & (sq == sh)
            c = unit[..., 0] * nu[..., 0] + unit[..., 1] * nu[..., 1] + unit[..., 2] * nu[..., 2]
            d = pq - pnt
            dz = unit[..., 0] * d[..., 0] + unit[..., 1] * d[..., 1] + unit[..., 2] * d[..., 2]
            b = bx[t & 1] * by[t >> 1]
            take = take & (c >= normal_min) & (np.abs(dz) <= point_tolerance) & (b > 0.0)
            hs = np.where(take[..., None], hs + b[..., None] * cq, hs)
            ws = np.where(take, ws + b, ws)
            nmax = np.where(take, np.maximum(nmax, nq), nmax)
            some = some | take
        n = np.minimum(nmax + 1, max_history)
        alpha = 1.0 / n.astype(np.float64)
        hist = hs / ws[..., None]
        out = np.where(some[..., None], hist + (cur - hist) * alpha[..., None], cur)
    count = np.where(hit, np.where(some, n, 1), 0).astype(np.int32)
    return out, count


# ---- the mirrors of the variance queries (include/ptrace_variance.h) -------------------------------------------------------------------
def _luminance(c) -> np.ndarray:
    """``lum(c)`` of include/ptrace_variance.h over ``[..., 3]``: ``Color.luminosity`` written with comparisons."""
    c0, c1, c2 = c[..., 0], c[..., 1], c[..., 2]
    mx = np.where(c1 > c0, c1, c0)
    mx = np.where(c2 > mx, c2, mx)
    mn = np.where(c1 < c0, c1, c0)
    mn = np.where(c2 < mn, c2, mn)
    with np.errstate(all="ignore"):
        return (mx + mn) / 2.0


def _variance_params(W, H, passes=4, sigma_point=0.1, normal_power_log2=5, sigma_luminance=1.0, epsilon=1e-10, min_history=4, normal_min=0.9,
                     point_tolerance=0.05, same_shape=True, wrap_x=False):
    """The checks of ``pt_variance_params`` and of the frame, as ``ValueError`` s -> the values as Python numbers."""
    passes, e, min_history = int(passes), int(normal_power_log2), int(min_history)
    sigma_point, sigma_luminance, epsilon = float(sigma_point), float(sigma_luminance), float(epsilon)
    normal_min, point_tolerance = float(normal_min), float(point_tolerance)
    if W < 0 or H < 0 or W * H > MAX_RAYS:
        raise ValueError(f"a frame of {W} x {H} records")
    if not 1 <= passes <= 10 or not 0 <= e <= 10:
        raise ValueError(f"passes={passes} (1 to 10), normal_power_log2={e} (0 to 10)")
    if not 1 <= min_history <= 2 ** 20:
        raise ValueError(f"min_history={min_history}: 1 to 2^20")
    if not sigma_point > 0.0 or not sigma_luminance > 0.0:
        raise ValueError(f"sigma_point={sigma_point}, sigma_luminance={sigma_luminance}: a sigma is positive (or inf)")
    if not (epsilon > 0.0 and epsilon < float("inf")):
        raise ValueError(f"epsilon={epsilon}: positive and finite")
    if not -1.0 <= normal_min <= 1.0 or not point_tolerance > 0.0:
        raise ValueError(f"normal_min={normal_min} (a cosine, -1 to 1), point_tolerance={point_tolerance} (positive, or inf)")
    return passes, e, min_history, sigma_point, sigma_luminance, epsilon, normal_min, point_tolerance, bool(same_shape), bool(wrap_x)


def luminance_moments_host(colour, shape, width: int, height: int) -> np.ndarray:
    """The numpy mirror of the moments query (include/ptrace_variance.h): ``(l, l * l, 0)`` per record, zeros where ``shape`` is
    negative -> ``[height, width, 3]``."""
    W, H = int(width), int(height)
    if W < 0 or H < 0 or W * H > MAX_RAYS:
        raise ValueError(f"a frame of {W} x {H} records")
    col = np.asarray(colour, dtype=np.float64).reshape(H, W, 3)
    hit = np.asarray(shape, dtype=np.int32).reshape(H, W) >= 0
    with np.errstate(all="ignore"):
        l = _luminance(col)
        l2 = l * l
    out = np.zeros((H, W, 3))
    out[..., 0], out[..., 1] = np.where(hit, l, 0.0), np.where(hit, l2, 0.0)
    return out


# ---- the mirror of the weighted accumulate query (include/ptrace_weighted.h) ------------------------------------------------------------
def weighted_host(colour, samples, shape, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count, prev_camera,
                  width: int, height: int, max_history: int = 32, same_shape: bool = True, blend_weight: bool = False, normal_min: float = 0.9,
                  point_tolerance: float = 0.05, max_weight: float = 128.0, keep=None):
    """The numpy mirror of the weighted accumulate query (include/ptrace_weighted.h), operation for operation: the projection and
    the four taps of :func:`temporal_host`, in its order, for the colour, the luminance moments and the weight at once.  The planes
    as :func:`temporal_host` takes them, plus ``samples`` (int32 per record, or ``None``: one everywhere) and ``prev_moments``
    (``[..., 3]``: M1, M2 and the accumulated weight S) -> ``(out [height, width, 3] float64, moments [height, width, 3] float64,
    count [height, width] int32)``.  Refuses what the library refuses, with a ``ValueError``.  ``keep`` (float64 per record, or
    ``None``) is not part of that query: it is the one insertion of include/ptrace_gradient.h into step 5, which
    :func:`gradient_accumulate_host` passes; with ``None`` nothing here differs from what it was."""
    W, H, max_history = int(width), int(height), int(max_history)
    normal_min, point_tolerance, max_weight = float(normal_min), float(point_tolerance), float(max_weight)
    if W < 0 or H < 0 or W * H > MAX_RAYS:
        raise ValueError(f"a frame of {W} x {H} records")
    if not 1 <= max_history <= 2 ** 20:
        raise ValueError(f"max_history={max_history}: 1 to 2^20")
    if not -1.0 <= normal_min <= 1.0 or not point_tolerance > 0.0:
        raise ValueError(f"normal_min={normal_min} (a cosine, -1 to 1), point_tolerance={point_tolerance} (positive, or inf)")
    if not max_weight >= 0.0:
        raise ValueError(f"max_weight={max_weight}: not negative (or inf)")
    cur = np.array(colour, dtype=np.float64).reshape(H, W, 3)
    k = np.ones((H, W), dtype=np.int32) if samples is None else np.asarray(samples, dtype=np.int32).reshape(H, W)
    sh = np.asarray(shape, dtype=np.int32).reshape(H, W)
    nrm = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    pnt = np.asarray(point, dtype=np.float64).reshape(H, W, 3)
    pcol = np.asarray(prev_colour, dtype=np.float64).reshape(H, W, 3)
    pmom = np.asarray(prev_moments, dtype=np.float64).reshape(H, W, 3)
    psh = np.asarray(prev_shape, dtype=np.int32).reshape(H, W)
    pnrm = np.asarray(prev_normal, dtype=np.float64).reshape(H, W, 3)
    ppnt = np.asarray(prev_point, dtype=np.float64).reshape(H, W, 3)
    pcnt = np.asarray(prev_count, dtype=np.int32).reshape(H, W)
    fx, fy, ok = temporal_project_host(prev_camera, pnt, W, H)
    if W * H == 0:
        return cur, np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.int32)
    hit = sh >= 0
    ok = ok & hit
    with np.errstate(all="ignore"):
        unit = nrm / np.sqrt(nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1] + nrm[..., 2] * nrm[..., 2])[..., None]
        punit = pnrm / np.sqrt(pnrm[..., 0] * pnrm[..., 0] + pnrm[..., 1] * pnrm[..., 1] + pnrm[..., 2] * pnrm[..., 2])[..., None]
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        bx, by = (1.0 - ax, ax), (1.0 - ay, ay)
        hs, hm, ws, smax = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
        nmax, some = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=bool)
        for t in range(4):
            x, y = x0 + (t & 1), y0 + (t >> 1)
            take = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            at = (np.clip(y, 0, H - 1), np.clip(x, 0, W - 1))
            sq, nq, nu, pq, cq, mq = psh[at], pcnt[at].astype(np.int64), punit[at], ppnt[at], pcol[at], pmom[at]
            take = take & (nq > 0) & (sq >= 0)
            if same_shape:
                take = take & (sq == sh)
            c = unit[..., 0] * nu[..., 0] + unit[..., 1] * nu[..., 1] + unit[..., 2] * nu[..., 2]
            d = pq - pnt
            dz = unit[..., 0] * d[..., 0] + unit[..., 1] * d[..., 1] + unit[..., 2] * d[..., 2]
            b = bx[t & 1] * by[t >> 1]
            take = take & (c >= normal_min) & (np.abs(dz) <= point_tolerance) & (b > 0.0)
            hs = np.where(take[..., None], hs + b[..., None] * cq, hs)
            hm = np.where(take[..., None], hm + b[..., None] * mq, hm)  # (M1, M2 and S: three sums of their own)
            ws = np.where(take, ws + b, ws)
            nmax = np.where(take, np.maximum(nmax, nq), nmax)
            smax = np.where(take & (mq[..., 2] > smax), mq[..., 2], smax)
            some = some | take
        l = _luminance(cur)
        l2 = l * l
        kd = k.astype(np.float64)
        hist = hs / ws[..., None]
        m1, m2 = hm[..., 0] / ws, hm[..., 1] / ws
        Sh = hm[..., 2] / ws if blend_weight else smax
        Sh = np.where(Sh > 0.0, Sh, 0.0)
        Sh = np.where(Sh > max_weight, max_weight, Sh)
        if keep is not None:  # (include/ptrace_gradient.h: the history's weight and length shrink where the light changed)
            kp = np.asarray(keep, dtype=np.float64).reshape(H, W)
            kp = np.where(kp >= 0.0, kp, 0.0)
            kp = np.where(kp > 1.0, 1.0, kp)
            Sh = kp * Sh
            nmax = np.floor(kp * nmax.astype(np.float64)).astype(np.int64)
        total = Sh + kd
        alpha = kd / total
        blended = hist + (cur - hist) * alpha[..., None]
        M1 = m1 + (l - m1) * alpha
        M2 = m2 + (l2 - m2) * alpha
    took = k > 0
    fresh = hit & ~some  # (step 4)
    out = np.where((some & took)[..., None], blended, np.where((some & ~took)[..., None], hist, cur))
    moments = np.zeros((H, W, 3))
    for plane, new, carried, first in ((0, M1, m1, l), (1, M2, m2, l2), (2, total, Sh, kd)):
        moments[..., plane] = np.where(some & took, new, np.where(some, carried, np.where(fresh & took, first, 0.0)))
    count = np.where(some & took, np.minimum(nmax + 1, max_history), np.where(some, np.minimum(nmax, max_history), np.where(fresh & took, 1, 0)))
    return out, moments, count.astype(np.int32)


# ---- the mirror of the motion accumulate query (include/ptrace_motion.h) ---------------------------------------------------------------
def shape_motion(prev_world, world, static=()):
    """The tables of the motion accumulate query for two worlds that hold the same shapes, in the same order, under transformations
    that may differ -> ``(moved int32[S], motion float64[S, 24])``.  Per shape: ``motion[s][0:12]`` are rows 0..2 of
    ``A = prev.transformation * cur.transformation.inverse()``, which takes a point of the shape in THIS frame's world to where that
    surface point was in the PREVIOUS frame's; ``motion[s][12:21]`` is the transpose of the linear part of
    ``cur.transformation * prev.transformation.inverse()`` (the host model's own ``Transformation`` product: its bits are the
    definition), which carries a normal the same way; ``moved[s]`` is 0 where both matrices of the two transformations are equal
    element for element, and for every index in ``static``.

    WHAT BELONGS IN ``static``.  ``E`` is light arriving at a place.  A shape that moves ONTO ITSELF -- a sphere spinning about an
    axis through its centre, a plane sliding in its own plane -- carries no light with it: list it in ``static`` and the history
    stays where the light is.  Left in the table, its history would be fetched from the surface point that turned into this place,
    which the light of another place fell on.

    Raises ``ValueError`` when the worlds differ in the number or the kinds of their shapes."""
    before, now = list(prev_world.shapes), list(world.shapes)
    if len(before) != len(now):
        raise ValueError(f"the previous world has {len(before)} shapes, this one {len(now)}: a motion needs the same shapes in both")
    static = {int(s) for s in static}
    moved, motion = np.zeros(len(now), dtype=np.int32), np.zeros((len(now), 24))
    for s, (a, b) in enumerate(zip(before, now)):
        if type(a) is not type(b):
            raise ValueError(f"shape {s} was a {type(a).__name__} and is a {type(b).__name__}: a motion needs the same shapes in both")
        ta, tb = a.transformation, b.transformation
        forward = (ta * tb.inverse()).m
        back = (tb * ta.inverse()).m
        motion[s, :12] = [forward[i][j] for i in range(3) for j in range(4)]
        motion[s, 12:21] = [back[j][i] for i in range(3) for j in range(3)]
        same = all(ta.m[i][j] == tb.m[i][j] and ta.invm[i][j] == tb.invm[i][j] for i in range(4) for j in range(4))
        moved[s] = 0 if same or s in static else 1
    return moved, motion


def _motion_tables(moved, motion):
    """``(n_shapes, moved, motion [S, 24])`` of two tables, checked as the library checks them (``ValueError``)."""
    from . import _motion_lib

    n, moved, motion = _motion_lib.tables(moved, motion)
    if n > _motion_lib.MAX_SHAPES:
        raise ValueError(f"n_shapes={n}: 0 to 2^20")
    return n, moved, motion


def move_records_host(shape, normal, point, moved, motion):
    """Step 1 of include/ptrace_motion.h on the host, operation for operation: a record whose shape index ``s`` lies in
    ``0 <= s < len(moved)`` with ``moved[s] != 0`` gets ``pm = A_s * point`` and ``nm = N_s * normal`` (each row summed in the header's
    order); every other record keeps its point and normal bit for bit, and no table entry is read for it -> ``(normal, point)`` in
    the shapes they came in."""
    n, moved, motion = _motion_tables(moved, motion)
    nrm = np.array(normal, dtype=np.float64)
    pnt = np.array(point, dtype=np.float64)
    sh = np.asarray(shape, dtype=np.int32).reshape(-1)
    nf, pf = nrm.reshape(-1, 3), pnt.reshape(-1, 3)
    if n == 0 or sh.shape[0] == 0:
        return nrm, pnt
    listed = (sh >= 0) & (sh < n)
    s = np.where(listed, sh, 0)
    mv = listed & (moved[s] != 0)
    t = motion[s]  # [m, 24]
    px, py, pz = pf[:, 0], pf[:, 1], pf[:, 2]
    nx, ny, nz = nf[:, 0], nf[:, 1], nf[:, 2]
    with np.errstate(all="ignore"):
        pm = [((t[:, 4 * i] * px + t[:, 4 * i + 1] * py) + t[:, 4 * i + 2] * pz) + t[:, 4 * i + 3] for i in range(3)]
        nm = [(t[:, 12 + 3 * i] * nx + t[:, 13 + 3 * i] * ny) + t[:, 14 + 3 * i] * nz for i in range(3)]
    new_p, new_n = np.stack(pm, axis=-1), np.stack(nm, axis=-1)
    pf[mv], nf[mv] = new_p[mv], new_n[mv]
    return nrm, pnt


def motion_host(colour, samples, shape, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count, prev_camera,
                moved, motion, width: int, height: int, **params):
    """The numpy mirror of the motion accumulate query (include/ptrace_motion.h), operation for operation: step 1 is
    :func:`move_records_host`, everything after it is :func:`weighted_host` on the moved records (contract D of the header is how
    this mirror is made; contract C -- nothing moved, nothing changes -- follows).  The planes and ``params`` as
    :func:`weighted_host` takes them, plus ``moved`` (int32 per shape) and ``motion`` (``[S, 24]``), or ``None`` for both -> ``(out
    [height, width, 3] float64, moments [height, width, 3] float64, count [height, width] int32)``.  Refuses what the library refuses,
    with a ``ValueError``."""
    nm, pm = move_records_host(shape, normal, point, moved, motion)
    return weighted_host(colour, samples, shape, nm, pm, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count, prev_camera,
                         width, height, **params)


# ---- the mirrors of the gradient accumulate query (include/ptrace_gradient.h) ----------------------------------------------------------
_U64 = (1 << 64) - 1


def gradient_probe_offsets(phase: int, strata: int):
    """The hash of include/ptrace_gradient.h for the strata ``0 .. strata - 1`` of frame ``phase`` -> the uint64 ``x`` after its last
    step, of which ``x & 0xffff`` and ``(x >> 16) & 0xffff`` place the probe in its stratum."""
    with np.errstate(over="ignore"):
        j = np.arange(int(strata), dtype=np.uint64)
        x = np.uint64((int(phase) * 0x9E3779B97F4A7C15 + 0x2545F4914F6CDD1D) & _U64) + j * np.uint64(0xD1B54A32D192ED03)
        for _ in range(2):
            x = x ^ (x >> np.uint64(32))
            x = x * np.uint64(0xD6E8FEB86659FD93)
        return x ^ (x >> np.uint64(32))


def gradient_probes_host(shape, normal, point, moved, motion, width: int, height: int, stratum: int = 3, phase: int = 0, samples: int = 1,
                         init_seq: int = 54):
    """The numpy mirror of the probes query (include/ptrace_gradient.h), operation for operation: one probe per ``stratum x stratum``
    block of the frame, at the pixel the hash of ``(phase, stratum index)`` picks, carried into the previous world by
    :func:`move_records_host` -> ``(probe_index int32[ns], probe_point [ns, 3], probe_normal [ns, 3], probe_seq uint64[ns])``; a probe
    on a miss has index -1 and zeros.  Refuses what the library refuses, with a ``ValueError``."""
    from . import _gradient_lib

    W, H, s, K = int(width), int(height), int(stratum), int(samples)
    ns = _gradient_lib.strata(W, H, s)
    if K < 1:
        raise ValueError(f"samples={K}: at least 1")
    _motion_tables(moved, motion)
    if W * H == 0:
        return np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.uint64)
    sh = np.asarray(shape, dtype=np.int32).reshape(-1)
    gw = (W + s - 1) // s
    j = np.arange(ns, dtype=np.int64)
    sy, sx = j // gw, j % gw
    sw, shh = np.minimum(s, W - sx * s), np.minimum(s, H - sy * s)
    x = gradient_probe_offsets(phase, ns)
    ox = ((x & np.uint64(0xffff)) % sw.astype(np.uint64)).astype(np.int64)
    oy = (((x >> np.uint64(16)) & np.uint64(0xffff)) % shh.astype(np.uint64)).astype(np.int64)
    r = (sy * s + oy) * W + sx * s + ox
    nm, pm = move_records_host(sh[r], np.asarray(normal, dtype=np.float64).reshape(-1, 3)[r], np.asarray(point, dtype=np.float64).reshape(-1, 3)[r],
                               moved, motion)
    hit = sh[r] >= 0
    with np.errstate(over="ignore"):
        seq = np.uint64(int(init_seq) & _U64) + r.astype(np.uint64) * np.uint64(K & _U64)
    return (np.where(hit, r, -1).astype(np.int32), np.where(hit[:, None], pm, 0.0), np.where(hit[:, None], nm, 0.0),
            np.where(hit, seq, np.uint64(0)))


def gradient_keep_host(colour, shape, probe_index, probe_old, width: int, height: int, stratum: int = 3, radius: int = 1, gain: float = 8.0,
                       same_shape_probes: bool = True) -> np.ndarray:
    """The numpy mirror of the keep query (include/ptrace_gradient.h), operation for operation: per pixel the sums of ``|lc - lo|`` and
    of ``max(lc, lo)`` over the probes of the ``(2 radius + 1)^2`` strata around it, ``dy`` then ``dx``, and ``1 - clamp(gain * num /
    den)`` -> ``keep [height, width]`` float64.  A probe index outside ``[0, m)`` is skipped and nothing is read there.  Refuses what
    the library refuses, with a ``ValueError``."""
    from . import _gradient_lib

    W, H, s, R, gain = int(width), int(height), int(stratum), int(radius), float(gain)
    ns = _gradient_lib.strata(W, H, s)
    if not 0 <= R <= _gradient_lib.MAX_RADIUS:
        raise ValueError(f"radius={R}: 0 to 4")
    if not gain >= 0.0:
        raise ValueError(f"gain={gain}: not negative (or inf)")
    m = W * H
    if m == 0:
        return np.ones((H, W))
    col = np.asarray(colour, dtype=np.float64).reshape(m, 3)
    sh = np.asarray(shape, dtype=np.int32).reshape(m)
    idx = np.asarray(probe_index, dtype=np.int32).reshape(-1).astype(np.int64)
    old = np.asarray(probe_old, dtype=np.float64).reshape(-1, 3)
    if idx.shape[0] != ns or old.shape[0] != ns:
        raise ValueError(f"a {W} x {H} frame in strata of {s} has {ns} probes, not {idx.shape[0]} indices and {old.shape[0]} old colours")
    gw, gh = (W + s - 1) // s, (H + s - 1) // s
    ys, xs = np.divmod(np.arange(m, dtype=np.int64), W)
    gx, gy = xs // s, ys // s
    vouched = (idx >= 0) & (idx < m)
    q_of = np.where(vouched, idx, 0)
    with np.errstate(all="ignore"):
        lc_of, lo_of = _luminance(col[q_of]), _luminance(old)
        d_of = lc_of - lo_of
        d_of = np.where(d_of < 0.0, 0.0 - d_of, d_of)
        mx_of = np.where(lc_of > lo_of, lc_of, lo_of)
        num, den = np.zeros(m), np.zeros(m)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                tx, ty = gx + dx, gy + dy
                inside = (tx >= 0) & (tx < gw) & (ty >= 0) & (ty < gh)
                j = np.where(inside, ty * gw + tx, 0)
                take = inside & vouched[j]
                if same_shape_probes:
                    take = take & (sh[q_of[j]] == sh)
                num = np.where(take, num + d_of[j], num)
                den = np.where(take, den + mx_of[j], den)
        lam = gain * (num / den)
        lam = np.where(lam > 0.0, lam, 0.0)
        lam = np.where(lam > 1.0, 1.0, lam)
        keep = 1.0 - lam
    return np.where(sh >= 0, keep, 1.0).reshape(H, W)


def gradient_accumulate_host(colour, samples, shape, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count,
                             prev_camera, moved, motion, keep, width: int, height: int, **params):
    """The numpy mirror of the gradient accumulate query (include/ptrace_gradient.h), operation for operation: :func:`motion_host`
    with the one insertion into step 5 -- ``keep`` (float64 per record) clamped to [0, 1] multiplies the history's weight ``Sh`` and,
    under a floor, its length ``nmax``; ``None``: :func:`motion_host` in every bit (contract E) -> ``(out [height, width, 3],
    moments [height, width, 3], count [height, width] int32)``."""
    if keep is not None and np.asarray(keep).size != int(width) * int(height):
        raise ValueError(f"a {width} x {height} frame has {int(width) * int(height)} records, not {np.asarray(keep).size} keep values")
    nm, pm = move_records_host(shape, normal, point, moved, motion)
    return weighted_host(colour, samples, shape, nm, pm, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count, prev_camera,
                         width, height, keep=keep, **params)


def _wrapped_columns(cols, offset, W, wrap_x):
    """Columns ``cols + offset`` of a frame ``W`` wide -> (the columns, clipped or wrapped into the frame; which of them exist)."""
    qx = cols + offset
    if wrap_x:
        return qx % W, np.ones(qx.shape, dtype=bool)
    return np.clip(qx, 0, W - 1), (qx >= 0) & (qx < W)


def variance_estimate_host(moments, count, shape, normal, point, width: int, height: int, **params) -> np.ndarray:
    """The numpy mirror of the estimate query (include/ptrace_variance.h), operation for operation: vectorised per tap over the whole
    frame, the 49 taps in the header's order.  ``moments``: ``[..., 3]`` (the third channel is not read), ``count`` and ``shape``:
    int32, ``normal`` and ``point``: ``[..., 3]``, all ``width * height`` records; ``params``: ``min_history``, ``normal_min``,
    ``point_tolerance``, ``same_shape``, ``wrap_x`` (the filter's are checked and not used) -> ``[height, width]``."""
    W, H = int(width), int(height)
    _, _, min_history, _, _, _, normal_min, point_tolerance, same_shape, wrap_x = _variance_params(W, H, **params)
    mom = np.asarray(moments, dtype=np.float64).reshape(H, W, 3)
    cnt = np.asarray(count, dtype=np.int32).reshape(H, W)
    sh = np.asarray(shape, dtype=np.int32).reshape(H, W)
    nrm = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    pnt = np.asarray(point, dtype=np.float64).reshape(H, W, 3)
    if W * H == 0:
        return np.zeros((H, W))
    rows, cols = np.arange(H), np.arange(W)
    mu1, mu2 = mom[..., 0], mom[..., 1]
    with np.errstate(all="ignore"):
        unit = nrm / np.sqrt(nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1] + nrm[..., 2] * nrm[..., 2])[..., None]
        s1, s2, k = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
        for dy in range(-3, 4):
            qy = rows + dy
            in_y = (qy >= 0) & (qy < H)
            qy = np.clip(qy, 0, H - 1)
            for dx in range(-3, 4):
                qx, in_x = _wrapped_columns(cols, dx, W, wrap_x)
                at = np.ix_(qy, qx)
                take = in_y[:, None] & in_x[None, :]
                if dx != 0 or dy != 0:
                    sq, nq, pq = sh[at], unit[at], pnt[at]
                    take = take & (sq >= 0) & (cnt[at] >= 1)
                    if same_shape:
                        take = take & (sq == sh)
                    c = unit[..., 0] * nq[..., 0] + unit[..., 1] * nq[..., 1] + unit[..., 2] * nq[..., 2]
                    d = pq - pnt
                    dz = unit[..., 0] * d[..., 0] + unit[..., 1] * d[..., 1] + unit[..., 2] * d[..., 2]
                    take = take & (c >= normal_min) & (np.abs(dz) <= point_tolerance)
                s1 = np.where(take, s1 + mu1[at], s1)
                s2 = np.where(take, s2 + mu2[at], s2)
                k = np.where(take, k + 1.0, k)
        mean = s1 / k
        spatial = s2 / k - mean * mean
        v = np.where(cnt >= min_history, mu2 - mu1 * mu1, spatial)
        v = np.where(v > 0.0, v, 0.0)
        v = v / cnt.astype(np.float64)
    return np.where((sh < 0) | (cnt < 1), 0.0, v)


def variance_filter_host(colour, variance, shape, normal, point, width: int, height: int, **params):
    """The numpy mirror of the filter query (include/ptrace_variance.h), operation for operation: vectorised per tap over the whole
    frame, the taps in the header's order (``dy`` outer, ``dx`` inner), every sum in that order.  ``colour``, ``normal``, ``point``:
    ``width * height`` records of 3 in row-major order (any leading shape), ``variance``: as many fp64, ``shape``: as many int32,
    negative = copied; ``params``: ``passes``, ``sigma_point``, ``normal_power_log2``, ``sigma_luminance``, ``epsilon``,
    ``same_shape``, ``wrap_x`` (the estimate's are checked and not used) -> ``(colour [height, width, 3], variance [height, width])``.
    Refuses what the library refuses, with a ``ValueError``."""
    W, H = int(width), int(height)
    passes, e, _, sigma_point, sigma_luminance, epsilon, _, _, same_shape, wrap_x = _variance_params(W, H, **params)
    cur = np.array(colour, dtype=np.float64).reshape(H, W, 3)
    var = np.array(variance, dtype=np.float64).reshape(H, W)
    sh = np.asarray(shape, dtype=np.int32).reshape(H, W)
    nrm = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    pnt = np.asarray(point, dtype=np.float64).reshape(H, W, 3)
    if W * H == 0:
        return cur, var
    active = sh >= 0
    rows, cols = np.arange(H), np.arange(W)
    sl2 = sigma_luminance * sigma_luminance
    sl_inf = sl2 == float("inf")
    with np.errstate(all="ignore"):
        unit = nrm / np.sqrt(nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1] + nrm[..., 2] * nrm[..., 2])[..., None]
        for i in range(passes):
            s = 2 ** i
            sps = sigma_point * float(s)
            # the prefiltered variance: 3x3 at step 1, the centre a tap like the others
            gs, gw = np.zeros((H, W)), np.zeros((H, W))
            for dy in range(-1, 2):
                qy = rows + dy
                in_y = (qy >= 0) & (qy < H)
                qy = np.clip(qy, 0, H - 1)
                for dx in range(-1, 2):
                    kw = (0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)
                    qx, in_x = _wrapped_columns(cols, dx, W, wrap_x)
                    at = np.ix_(qy, qx)
                    sq, vq = sh[at], var[at]
                    take = in_y[:, None] & in_x[None, :] & (sq >= 0) & (vq >= 0.0)
                    if same_shape:
                        take = take & (sq == sh)
                    gs = np.where(take, gs + kw * vq, gs)
                    gw = np.where(take, gw + kw, gw)
            g = np.where(gw > 0.0, gs / gw, 0.0)
            den = sl2 * g + epsilon
            lum = _luminance(cur)
            total, wsum, vs = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
            for dy in range(-2, 3):
                qy = rows + s * dy
                in_y = (qy >= 0) & (qy < H)
                qy = np.clip(qy, 0, H - 1)
                for dx in range(-2, 3):
                    k = DENOISE_KERNEL[dx + 2] * DENOISE_KERNEL[dy + 2]
                    if dx == 0 and dy == 0:
                        total, wsum, vs = total + k * cur, wsum + k, vs + (k * k) * var
                        continue
                    qx, in_x = _wrapped_columns(cols, s * dx, W, wrap_x)
                    at = np.ix_(qy, qx)
                    sq, nq, pq, cq, lq, vq = sh[at], unit[at], pnt[at], cur[at], lum[at], var[at]
                    take = in_y[:, None] & in_x[None, :] & (sq >= 0)
                    if same_shape:
                        take = take & (sq == sh)
                    c = unit[..., 0] * nq[..., 0] + unit[..., 1] * nq[..., 1] + unit[..., 2] * nq[..., 2]
                    c = np.where(c > 0.0, c, 0.0)
                    for _ in range(e):
                        c = c * c
                    d = pq - pnt
                    dz = unit[..., 0] * d[..., 0] + unit[..., 1] * d[..., 1] + unit[..., 2] * d[..., 2]
                    t = dz / sps
                    wp = 1.0 / (1.0 + t * t)
                    dl = lq - lum
                    dl2 = dl * dl
                    if sl_inf:
                        wl = np.where(dl2 < float("inf"), 1.0, float("nan"))
                    else:
                        wl = 1.0 / (1.0 + dl2 / den)
                    w = ((k * c) * wp) * wl
                    take = take & (w > 0.0)
                    total = np.where(take[..., None], total + w[..., None] * cq, total)
                    wsum = np.where(take, wsum + w, wsum)
                    vs = np.where(take, vs + (w * w) * vq, vs)
            cur = np.where(active[..., None], total / wsum[..., None], cur)
            var = np.where(active, vs / (wsum * wsum), var)
    return cur, var


# ---- the mirrors of the adaptive queries (include/ptrace_adaptive.h) -------------------------------------------------------------------
def _count_params(min_samples=1, max_samples=32, tolerance=0.05, luminance_floor=1.0, gain=1.0):
    """The checks of ``pt_adaptive_count_params``, as ``ValueError`` s -> the values as Python numbers."""
    lo, hi = int(min_samples), int(max_samples)
    tolerance, floor, gain = float(tolerance), float(luminance_floor), float(gain)
    if not 0 <= lo <= hi <= MAX_SAMPLES:
        raise ValueError(f"min_samples={lo}, max_samples={hi}: 0 <= min <= max <= 2^20")
    if not tolerance > 0.0:
        raise ValueError(f"tolerance={tolerance}: positive (or inf)")
    if not (floor > 0.0 and floor < float("inf")):
        raise ValueError(f"luminance_floor={floor}: positive and finite")
    if not (gain > 0.0 and gain < float("inf")):
        raise ValueError(f"gain={gain}: positive and finite")
    return lo, hi, tolerance, floor, gain


def sample_counts_host(variance, colour, shape, **params) -> np.ndarray:
    """The numpy mirror of the counts query (include/ptrace_adaptive.h), bit for bit: per pixel ``ceil(gain * variance / (tolerance
    * max(lum(colour), luminance_floor))^2)`` clamped into ``[min_samples, max_samples]``; ``max_samples`` where the variance is
    negative or NaN; 0 where ``shape`` is negative.  ``variance`` ``[...]``, ``colour`` ``[..., 3]``, ``shape`` ``[...]`` ->
    ``int32`` shaped like ``variance``."""
    lo, hi, tolerance, floor, gain = _count_params(**params)
    v = np.asarray(variance, dtype=np.float64)
    col = np.asarray(colour, dtype=np.float64).reshape(-1, 3)
    index = np.asarray(shape, dtype=np.int32).reshape(-1)
    flat = v.reshape(-1)
    if col.shape[0] != flat.shape[0] or index.shape[0] != flat.shape[0]:
        raise ValueError(f"{flat.shape[0]} variances, {col.shape[0]} colours and {index.shape[0]} shape indices")
    with np.errstate(all="ignore"):
        l = _luminance(col)
        l = np.where(l > floor, l, floor)
        tl = tolerance * l
        want = (gain * flat) / (tl * tl)
        ok = (flat >= 0.0) & (want < float(hi))
        w = np.where(ok, want, 0.0)
        t = w.astype(np.int64)
        k = t + (t.astype(np.float64) < w)
    k = np.maximum(k, lo)
    out = np.where(ok, k, hi)
    return np.where(index < 0, 0, out).astype(np.int32).reshape(v.shape)


def sample_offsets_host(counts) -> np.ndarray:
    """The numpy mirror of the offsets query: ``int64[n + 1]``, the exclusive prefix sum of ``max(counts, 0)``; the last value is
    the total."""
    c = np.asarray(counts).reshape(-1).astype(np.int64)
    out = np.zeros(c.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.maximum(c, 0), out=out[1:])
    return out


def samples_taken_host(counts, offsets, capacity) -> np.ndarray:
    """``K_i = min(max(counts[i], 0), max(capacity - offsets[i], 0))`` of include/ptrace_adaptive.h: what a ragged gather whose
    sample planes hold ``capacity`` samples takes per record -- a batch beyond ``capacity`` is truncated in record order."""
    c = np.maximum(np.asarray(counts).reshape(-1).astype(np.int64), 0)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if off.shape[0] != c.shape[0] + 1:
        raise ValueError(f"{c.shape[0]} counts need {c.shape[0] + 1} offsets, not {off.shape[0]}")
    return np.minimum(c, np.maximum(int(capacity) - off[:-1], 0)).astype(np.int32)


def gain_for_budget(variance, colour, shape, budget, **params) -> float:
    """The largest ``gain`` (a positive finite double) at which :func:`sample_counts_host` of these planes sums to no more than
    ``budget`` -- the total is monotone in ``gain``, so this is a bisection over the doubles (by their bit patterns: the result is
    exact, the next double above it exceeds the budget unless nothing finite does).  A ``ValueError`` if even the smallest gain
    exceeds it (``min_samples`` alone costs more).  For experiments that compare at equal cost, not for the hot path: it runs the
    mirror some 62 times.  ``params``: the count query's, without ``gain``."""
    if "gain" in params:
        raise TypeError("gain_for_budget finds the gain: do not pass one")
    budget = int(budget)

    def total(bits: int) -> int:
        gain = float(np.array([bits], dtype=np.int64).view(np.float64)[0])
        return int(sample_counts_host(variance, colour, shape, gain=gain, **params).astype(np.int64).sum())

    lo, hi = 1, int(np.array([np.finfo(np.float64).max]).view(np.int64)[0])  # the smallest and the largest positive finite double
    if total(lo) > budget:
        raise ValueError(f"no gain keeps the total within {budget} samples: the least it can be is {total(lo)}")
    if total(hi) > budget:
        while hi - lo > 1:  # total(lo) <= budget < total(hi)
            mid = (lo + hi) // 2
            if total(mid) <= budget:
                lo = mid
            else:
                hi = mid
    else:
        lo = hi
    return float(np.array([lo], dtype=np.int64).view(np.float64)[0])


def texel_centres(width: int, height: int, window=None) -> np.ndarray:
    """``[h, w, 2]``: ``(u, v)`` at the centres of the texels of ``window`` (``(col0, row0, w, h)``; ``None``: all) of a
    ``width x height`` map, as the bake forms them: ``(col + 0.5) * (1.0 / width)``, ``(row + 0.5) * (1.0 / height)``."""
    col0, row0, w, h = (0, 0, int(width), int(height)) if window is None else (int(x) for x in window)
    u = (np.arange(col0, col0 + w, dtype=np.float64) + 0.5) * (1.0 / int(width))
    v = (np.arange(row0, row0 + h, dtype=np.float64) + 0.5) * (1.0 / int(height))
    out = np.empty((h, w, 2), dtype=np.float64)
    out[..., 0], out[..., 1] = u[None, :], v[:, None]
    return out


def stream_numbers(seqs) -> np.ndarray:
    """``uint64[n]`` from stream numbers of any size and sign, wrapped into the 64-bit range as :func:`pcg_streams` wraps them
    (a signed array like the C cast; Python ints modulo 2^64): the ``seqs`` plane of a gather batch."""
    if isinstance(seqs, np.ndarray) and seqs.dtype.kind in "iu":
        return np.ascontiguousarray(seqs.astype(np.uint64).reshape(-1))
    return np.array([int(x) & (2 ** 64 - 1) for x in np.atleast_1d(np.asarray(seqs, dtype=object)).reshape(-1)], dtype=np.uint64)


def pcg_streams(init_state, init_seqs, skip: int = 0) -> np.ndarray:
    """``uint64[2, n]``: state and increment of ``PCG(init_state, seq)`` (pcg.py:25-41; csrc/pt_math.h: pcg_seed) for every
    ``seq`` of ``init_seqs``, ``skip`` draws in -- the generators a scatter batch carries.  Every value of the 64-bit range is
    legal and wraps, as the C arithmetic does: ``inc = (seq << 1) | 1``, ``state = (inc + init_state) * M + inc``, then the
    jump ``state * A + inc * G`` with the two coefficients of ``skip`` steps (the generator is a linear congruential one)."""
    from .hostmodel import pcg_advance

    skip = int(skip)
    if skip < 0:
        raise ValueError("skip must not be negative")
    if isinstance(init_seqs, np.ndarray) and init_seqs.dtype.kind in "iu":
        seqs = init_seqs.astype(np.uint64).reshape(-1)  # (a signed array wraps like the C cast)
    else:  # Python ints of any size (numpy would turn a list with values beyond 2^63 into floats)
        seqs = np.array([int(x) & (2 ** 64 - 1) for x in np.atleast_1d(np.asarray(init_seqs, dtype=object)).reshape(-1)], dtype=np.uint64)
    s0 = np.uint64(int(init_state) & (2 ** 64 - 1))
    mult = np.uint64(_PCG_MULT)
    out = np.empty((2, seqs.shape[0]), dtype=np.uint64)
    with np.errstate(over="ignore"):
        inc = (seqs << np.uint64(1)) | np.uint64(1)
        state = (inc + s0) * mult + inc
        if skip:
            a, g = np.uint64(pcg_advance(1, 0, skip)), np.uint64(pcg_advance(0, 1, skip))
            state = state * a + inc * g
    out[0], out[1] = state, inc
    return out


def planar(values, components: int) -> np.ndarray:
    """``[..., components]`` -> the ``[components, n]`` planes the library reads.  The strided views of a :class:`RayHits` or
    a hit-record frame ARE such planes seen from the other side: for them this is a view, not a copy."""
    a = np.asarray(values, dtype=np.float64)
    if a.ndim < 1 or a.shape[-1] != components:
        raise ValueError(f"expected [..., {components}], not {a.shape}")
    return np.ascontiguousarray(np.moveaxis(a, -1, 0)).reshape(components, -1)


def _one_record_frame(values, hits, taker: str):
    """``values`` (a :class:`GatheredRadiance`, a :class:`BakedMap` or an array) and ``hits`` (a hit frame, a :class:`RayHits` or
    ``(points, normals, shape)``) as the frame ``taker`` reads: ONE record per pixel -> ``(values [H, W, 3] or [m, 3], shape
    indices [m], normals, points, width, height)``."""
    if isinstance(hits, (tuple, list)):
        if len(hits) != 3:
            raise ValueError("hits as arrays are (points, normals, shape)")
        points, normals, index = hits
    else:
        points, normals, index = hits.point, hits.normal, hits.shape_index
    index = np.asarray(index)
    v = np.asarray(values.radiance if hasattr(values, "radiance") else values, dtype=np.float64)
    for what, a, lead in (("values", v, v.ndim - 1), ("hits", index, index.ndim)):
        if lead == 3 and a.shape[0] != 1:
            raise ValueError(f"{what} hold {a.shape[0]} samples per pixel: {taker} takes one record per pixel (average the samples first)")
    if v.ndim == 4:
        v = v[0]
    if index.ndim == 3:
        index = index[0]
    if v.ndim == 3 and v.shape[-1] == 3:
        height, width = v.shape[:2]
    elif index.ndim == 2 and v.size == index.size * 3:
        height, width = index.shape
    else:
        raise ValueError(f"no frame in values {v.shape} and shape indices {index.shape}: pass the values as [H, W, 3]")
    if index.size not in (1, height * width):
        raise ValueError(f"{index.size} shape indices for a frame of {height} x {width}")
    index = np.broadcast_to(index.reshape(-1) if index.size > 1 else index.reshape(()), (height * width,))
    return v, index, normals, points, width, height


class WorldQueries:
    """``World.ray_intersection`` / ``World.is_point_visible`` in batches on a device scene (``GpuImageTracer.world_queries``),
    and what a renderer does with the records: their materials, their colour under the world's point lights."""

    def __init__(self, scene):
        self.scene = scene

    def ray_intersections(self, rays, dirs=None, channels=RAY_CHANNELS, tmin=1e-5, tmax=float("inf")) -> RayHits:
        """``[n, 8]`` rays (or ``[n, 3]`` origins and ``dirs``) -> :class:`RayHits`, the ``HitRecord`` of every ray."""
        return self.scene.trace_rays(ray_planes(rays, dirs, tmin, tmax), channels)

    def are_points_visible(self, points, observer) -> np.ndarray:
        """``[n]`` bool: ``world.is_point_visible(points[i], observer)``."""
        return self.scene.points_visible(points, observer)

    def materials(self, hits, channels=SURF_ALL) -> SurfaceColors:
        """The material of every record of ``hits`` (a :class:`RayHits` or a :class:`pytracer_amd.hits.HitFrame` with the
        ``uv`` channel): ``brdf.pigment.get_color(uv)``, ``emitted_radiance.get_color(uv)`` and the BRDF's kind ->
        :class:`SurfaceColors`, shaped like ``hits.shape_index``."""
        bits = surface_channels(channels)
        out = self.scene.surface(hits.shape_index, hits.uv if bits else None, bits)
        return SurfaceColors(out.buffer, out.n, bits, shape=hits.shape_index.shape)

    def point_light_radiance(self, hits, dirs=None, ambient=(0.1, 0.1, 0.1), background=(0.0, 0.0, 0.0)) -> np.ndarray:
        """``PointLightRenderer(world, background, ambient)(ray)`` (render.py:157-193) for every record of ``hits`` -- a
        :class:`RayHits` or a hit-record frame with ``point``, ``normal`` and ``uv`` -- where ``dirs`` are the directions of
        the rays that were traced (default: a frame's ``ray_dir``) -> ``hits.shape_index.shape + (3,)``."""
        if dirs is None:
            if not hasattr(hits, "ray_dir"):
                raise ValueError("dirs= is needed: a ray batch does not carry the rays it was traced from")
            dirs = hits.ray_dir
        out = self.scene.shade_lights(hits.shape_index, hits.point, hits.normal, hits.uv, dirs, ambient, background)
        return out.reshape(hits.shape_index.shape + (3,))

    def probe_lit_radiance(self, grid: "ProbeGrid", probes: "ProbeSet", hits, dirs=None, background=(0.0, 0.0, 0.0)) -> np.ndarray:
        """Every record of ``hits`` shaded from the lattice ``grid`` of ``probes``: ``background`` where nothing was hit, else
        ``emitted + brdf_color * E``, ``E`` the eight probes around the hit point blended and evaluated towards the normal
        (``DiffuseBRDF``: the hemisphere mean) or the mirror direction (``SpecularBRDF``: the radiance) -- one kernel on the device
        (``DeviceScene.lit_shade``), :func:`lit_shade_host` in every bit.  ``hits``: a :class:`RayHits` or a hit-record frame with
        ``point``, ``normal`` and ``uv``, or a mapping of plain arrays ``shape_index``, ``point``, ``normal``, ``uv``; ``dirs``: the
        directions of the rays that were traced (default: a frame's ``ray_dir``) -> ``hits.shape_index.shape + (3,)``."""
        if probes.n != grid.n:
            raise ValueError(f"{probes.n} probes for a lattice of {grid.n}")
        if isinstance(hits, dict):
            from types import SimpleNamespace

            hits = SimpleNamespace(**{k: np.asarray(v) for k, v in hits.items()})
        if dirs is None:
            if not hasattr(hits, "ray_dir"):
                raise ValueError("dirs= is needed: a ray batch does not carry the rays it was traced from")
            dirs = hits.ray_dir
        index = np.asarray(hits.shape_index)
        out = self.scene.lit_shade(grid, probes.block, index, hits.point, hits.normal, hits.uv, dirs, background)
        return out.reshape(index.shape + (3,))

    def scatter(self, hits, dirs, pcg, roulette: bool = False, channels=SCAT_ALL) -> ScatteredRays:
        """The bounce of ``PathTracer.__call__`` (render.py:107-134, one child) for every record of ``hits`` -- a
        :class:`RayHits` or a hit-record frame with ``point``, ``normal`` and ``uv``: the roulette (where ``roulette`` says that
        ``ray.depth >= russian_roulette_limit`` holds) and ``brdf.scatter_ray``, drawing from ``pcg`` (``uint64[2, n]``: every
        record's generator, :func:`pcg_streams` or the ``pcg`` of the scatter before).  ``dirs``: the directions of the rays
        that were traced (``None``: a frame's ``ray_dir``) -> :class:`ScatteredRays`, shaped like ``hits.shape_index``."""
        if dirs is None:
            if not hasattr(hits, "ray_dir"):
                raise ValueError("dirs= is needed: a ray batch does not carry the rays it was traced from")
            dirs = hits.ray_dir
        bits = scatter_channels(channels)
        out = self.scene.scatter(hits.shape_index, hits.point, hits.normal, hits.uv, dirs, pcg, roulette, bits)
        return ScatteredRays(out.buffer, out.n, bits, shape=hits.shape_index.shape)

    def path_radiance(self, rays, pcg, dirs=None, num_of_rays: int = 1, max_depth: int = 10, russian_roulette_limit: int = 3,
                      background=(0.0, 0.0, 0.0), depth: int = 0, channels=RAD_ALL, tmin=1e-5, tmax=float("inf")) -> RayRadiance:
        """``PathTracer(world, background, pcg_i, num_of_rays, max_depth, russian_roulette_limit)(ray_i)`` (render.py:99-139;
        the defaults are ``PathTracer``'s) for ``[n, 8]`` rays (or ``[n, 3]`` origins and ``dirs``) with ``Ray.depth = depth``,
        each drawing from its own generator (``pcg``: ``uint64[2, n]``, :func:`pcg_streams`), walked depth-first on the
        device -> :class:`RayRadiance`."""
        return self.scene.radiance(ray_planes(rays, dirs, tmin, tmax), pcg, num_of_rays, max_depth, russian_roulette_limit, background,
                                   depth, channels)

    def hemisphere_radiance(self, hits, samples, init_state: int = 42, seqs=None, num_of_rays: int = 1, max_depth: int = 10,
                            russian_roulette_limit: int = 3, background=(0.0, 0.0, 0.0), depth: int = 0, channels="all", normals=None,
                            active=None, init_seq: int = 54) -> GatheredRadiance:
        """The mean radiance arriving over the hemisphere of every record: ``samples`` rays per record, sample ``k`` of record
        ``i`` being ``DiffuseBRDF.scatter_ray`` at the record's point and normal (``Ray.depth = depth``) drawn from
        ``PCG(init_state, seqs[i] + k)`` and followed by ``PathTracer(world, background, that generator, num_of_rays, max_depth,
        russian_roulette_limit)``; the mean is taken on the device, strictly in sample order.  ``hits``: a :class:`RayHits` or a
        hit-record frame with ``point`` and ``normal`` -- its ``shape_index`` says which records are skipped (no hit: radiance 0,
        count 0).  Or plain arrays: ``hits`` the ``[..., 3]`` points and ``normals=`` the ``[..., 3]`` normals (``active=``: an
        optional int32 array, negative = skipped).  ``seqs=None``: record ``i`` starts at stream ``init_seq + i * samples``, which
        keeps all streams disjoint -> :class:`GatheredRadiance`, shaped like the records."""
        if normals is None:
            if not (hasattr(hits, "point") and hasattr(hits, "normal")):
                raise ValueError("hits must carry point and normal (a RayHits or a hit frame), or pass the points with normals=")
            points, normals, shape = hits.point, hits.normal, np.asarray(hits.shape_index).shape
            if active is None:
                active = hits.shape_index
        else:
            points = np.asarray(hits, dtype=np.float64)
            shape = points.shape[:-1]
        bits = gather_channels(channels)
        out = self.scene.gather(planar(points, 3), planar(normals, 3), samples, init_state, seqs, active, num_of_rays, max_depth,
                                russian_roulette_limit, background, depth, bits, init_seq=init_seq)
        return GatheredRadiance(out.buffer, out.n, bits, shape=shape)

    def sample_counts(self, values, hits, variance, **params) -> np.ndarray:
        """How many hemisphere rays every pixel should get next, from how noisy its estimate still is -- on the device
        (``DeviceScene.sample_counts``), :func:`sample_counts_host` in every bit.  ``values`` and ``hits``: as :meth:`denoised`
        takes them, ONE record per pixel, the estimate ``E``; ``variance``: ``[H, W]``, the variance of ``values`` per pixel (what
        :class:`VarianceAccumulator` returns).  ``params``: ``min_samples``, ``max_samples``, ``tolerance``, ``luminance_floor``,
        ``gain`` -> ``int32 [H, W]``, 0 where nothing was hit."""
        v, index, _, _, width, height = _one_record_frame(values, hits, "the sample counts")
        if np.asarray(variance).size != height * width:
            raise ValueError(f"a variance of {np.asarray(variance).shape} for a frame of {height} x {width}")
        counts = self.scene.sample_counts(np.asarray(variance).reshape(-1), v.reshape(-1, 3), np.ascontiguousarray(index, dtype=np.int32), **params)
        return counts.reshape(height, width)

    def hemisphere_radiance_ragged(self, hits, counts, capacity=None, init_state: int = 42, seqs=None, num_of_rays: int = 1,
                                   max_depth: int = 10, russian_roulette_limit: int = 3, background=(0.0, 0.0, 0.0), depth: int = 0,
                                   channels="all", normals=None, active=None, init_seq: int = 54) -> RaggedRadiance:
        """:meth:`hemisphere_radiance` with a sample count PER RECORD (``counts``: int32, shaped like the records; zero and negative:
        no samples, black): the offsets query and the ragged gather of include/ptrace_adaptive.h, one behind the other.  Record
        ``i``'s sample ``k`` draws from ``PCG(init_state, seqs[i] + k)``; ``seqs=None``: ``init_seq + offsets[i]``, which keeps all
        streams disjoint.  Every record's radiance and count are, bit for bit, what :meth:`hemisphere_radiance` returns for it alone
        with ``samples = taken[i]``.  ``capacity``: the hard ray budget -- a total beyond it is truncated in record order;
        ``None``: the total itself, read back once from the offsets -> :class:`RaggedRadiance`, shaped like the records."""
        if normals is None:
            if not (hasattr(hits, "point") and hasattr(hits, "normal")):
                raise ValueError("hits must carry point and normal (a RayHits or a hit frame), or pass the points with normals=")
            points, normals, shape = hits.point, hits.normal, np.asarray(hits.shape_index).shape
            if active is None:
                active = hits.shape_index
        else:
            points = np.asarray(hits, dtype=np.float64)
            shape = points.shape[:-1]
        bits = adaptive_channels(channels)
        counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int32)
        offsets = self.scene.sample_offsets(counts)
        if capacity is None:
            capacity = int(offsets[-1])
        out = self.scene.gather_ragged(planar(points, 3), planar(normals, 3), counts, offsets, capacity, init_state, seqs, active, num_of_rays,
                                       max_depth, russian_roulette_limit, background, depth, bits, init_seq=init_seq)
        return RaggedRadiance(out.buffer, out.n, bits, shape=shape)

    def surface_points(self, shape, uv, side=1):
        """The world point and unit normal at ``uv`` (``[..., 2]``) of ``World.shapes[shape]`` (``shape``: one index, or one per
        record), on the side the shape's local normal points to (``side=1``) or the other (``-1``; one value, or one per record)
        -> ``(points, normals)``, each ``[..., 3]``: what :meth:`hemisphere_radiance` takes as ``hits`` and ``normals=``."""
        uv = np.asarray(uv, dtype=np.float64)
        if uv.ndim < 1 or uv.shape[-1] != 2:
            raise ValueError(f"uv must be [..., 2], not {uv.shape}")
        lead = uv.shape[:-1]
        n = int(np.prod(lead, dtype=np.int64))
        shapes = np.broadcast_to(np.asarray(shape, dtype=np.int32), lead).reshape(-1)
        sides = np.broadcast_to(np.asarray(side, dtype=np.int32), lead).reshape(-1)
        out = self.scene.surface_points(shapes, uv.reshape(n, 2), sides)
        return out[0:3].T.reshape(lead + (3,)), out[3:6].T.reshape(lead + (3,))

    def light_map(self, shape: int, width: int, height: int, samples: int, side: int = 1, jitter: bool = True, window=None,
                  depth: int = 1, init_state: int = 42, init_seq: int = 54, num_of_rays: int = 1, max_depth: int = 10,
                  russian_roulette_limit: int = 3, background=(0.0, 0.0, 0.0), channels="all") -> BakedMap:
        """The light map of ``World.shapes[shape]`` over its ``(u, v)`` square, ``width x height`` texels (or the ``window``
        ``(col0, row0, w, h)`` of them): per texel the mean radiance arriving over the hemisphere of ``samples`` points of the
        texel (``jitter=False``: its centre), texel ``t`` of the whole map drawing from the streams ``init_seq + t * samples +
        k`` -- a map baked in windows is the map baked whole.  ``depth``: the hemisphere rays' ``Ray.depth``; the default 1 means
        they are the children of a depth-0 hit, a camera ray's.  The other parameters are ``PathTracer``'s -> :class:`BakedMap`."""
        return self.scene.bake(shape, width, height, samples, side, jitter, window, init_state, init_seq, num_of_rays, max_depth,
                               russian_roulette_limit, background, depth, channels)

    def outgoing_map(self, shape: int, width: int, height: int, samples: int, side: int = 1, jitter: bool = True, **kw) -> np.ndarray:
        """``[height, width, 3]``: what a ``DiffuseBRDF`` shape sends out at every texel, ``emitted(uv_c) + brdf_color(uv_c) *
        light_map`` with the material's colours at the texel centres ``uv_c`` (:meth:`materials`) -- render.py:139 for a hit there,
        with the converged mean in place of ``num_of_rays`` children.  Composed on the host.  ``kw``: :meth:`light_map`'s."""
        from types import SimpleNamespace

        kw.pop("window", None)
        kw["channels"] = "none"
        centres = texel_centres(width, height)
        index = np.full(centres.shape[:-1], int(shape), dtype=np.int32)
        mat = self.materials(SimpleNamespace(shape_index=index, uv=centres))
        if not np.all(np.asarray(mat.brdf_kind) == abi.BRDF_DIFFUSE):
            raise ValueError(f"shape {shape} has no DiffuseBRDF: what a mirror sends out depends on where it is seen from, a map cannot hold it")
        baked = self.light_map(shape, width, height, samples, side, jitter, **kw)
        return np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * np.asarray(baked.radiance)

    def denoised(self, values, hits, **params) -> np.ndarray:
        """``values`` filtered by the edge-avoiding a-trous filter of include/ptrace_denoise.h, guided by ``hits`` -- on the device
        (``DeviceScene.denoise``), :func:`denoise_host` in every bit.  ``values``: a :class:`GatheredRadiance`, a :class:`BakedMap`
        or a ``[H, W, 3]`` array -- the DEMODULATED signal, ``E`` before ``emitted + brdf_color * E``, so that pigments stay sharp;
        ``hits``: a hit-record frame with ONE sample per pixel, a :class:`RayHits` whose records are the frame's ``H * W`` in
        row-major order, or ``(points, normals, shape)`` arrays (``shape``: one index or one per record).  More samples per pixel
        are a ``ValueError``: average them first.  ``params``: ``passes``, ``sigma_point``, ``normal_power_log2``,
        ``sigma_colour``, ``same_shape``, ``wrap_x`` -> ``[H, W, 3]``."""
        v, index, normals, points, width, height = _one_record_frame(values, hits, "the filter")
        return self.scene.denoise(v.reshape(-1, 3), index, np.asarray(normals).reshape(-1, 3), np.asarray(points).reshape(-1, 3), width, height, **params)

    def denoised_light_map(self, shape: int, width: int, height: int, samples: int, wrap_u=None, **kw) -> np.ndarray:
        """:meth:`light_map` of ``World.shapes[shape]`` (the whole map), then :meth:`surface_points` at the texel centres as guides,
        then :meth:`denoised` -> ``[height, width, 3]``.  ``wrap_u``: the first and the last column are neighbours (default: for a
        sphere, whose ``u`` is the longitude; not for a plane).  ``kw``: the filter's ``passes``, ``sigma_point``,
        ``normal_power_log2``, ``sigma_colour`` and ``same_shape``; everything else is :meth:`light_map`'s."""
        fpar = {k: kw.pop(k) for k in ("passes", "sigma_point", "normal_power_log2", "sigma_colour", "same_shape") if k in kw}
        if kw.get("window") is not None:
            raise ValueError("a window of a map has no neighbours beyond its edge: filter the whole map")
        kw.setdefault("channels", "none")
        baked = self.light_map(shape, width, height, samples, **kw)
        points, normals = self.surface_points(shape, texel_centres(width, height), kw.get("side", 1))
        if wrap_u is None:
            wrap_u = int(self.scene.flat.kind[int(shape)]) == abi.SHAPE_SPHERE
        return self.denoised(baked, (points, normals, int(shape)), wrap_x=bool(wrap_u), **fpar)

    def accumulated(self, values, hits, prev: "TemporalHistory", prev_camera, **params) -> "TemporalHistory":
        """``values`` blended with the previous frame's accumulated values where this frame's ``hits`` were seen before -- on the
        device (``DeviceScene.temporal``), :func:`temporal_host` in every bit.  ``values`` and ``hits``: as :meth:`denoised` takes
        them, ONE record per pixel, the DEMODULATED signal; ``prev``: the :class:`TemporalHistory` of the previous frame (what this
        method returned for it, or ``TemporalHistory.empty`` at the start); ``prev_camera``: the camera that frame was seen from.
        ``params``: ``max_history``, ``same_shape``, ``normal_min``, ``point_tolerance`` -> the :class:`TemporalHistory` of this
        frame: ``colour`` ``[H, W, 3]`` is the accumulated frame, ``count`` ``[H, W]`` the history lengths."""
        v, index, normals, points, width, height = _one_record_frame(values, hits, "the accumulation")
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(height, width)
        normals = np.asarray(normals, dtype=np.float64).reshape(height, width, 3)
        points = np.asarray(points, dtype=np.float64).reshape(height, width, 3)
        if np.asarray(prev.count).shape != (height, width):
            raise ValueError(f"a history of {np.asarray(prev.count).shape} for a frame of {height} x {width}")
        out, count = self.scene.temporal(v.reshape(-1, 3), index.reshape(-1), normals.reshape(-1, 3), points.reshape(-1, 3),
                                         np.asarray(prev.colour).reshape(-1, 3), np.asarray(prev.shape_index).reshape(-1),
                                         np.asarray(prev.normal).reshape(-1, 3), np.asarray(prev.point).reshape(-1, 3),
                                         np.asarray(prev.count).reshape(-1), prev_camera, width, height, **params)
        return TemporalHistory(out, index, normals, points, count)

    def accumulated_weighted(self, values, samples, hits, prev: "WeightedHistory", prev_camera, **params) -> "WeightedHistory":
        """:meth:`accumulated` with every frame weighted by the samples it took, for ``values`` and their luminance moments at once --
        on the device (``DeviceScene.weighted``), :func:`weighted_host` in every bit.  ``samples``: ``[H, W]`` int32, what this
        frame took per record (``None``: one everywhere; 0: nothing, the reprojected history is carried); ``prev``: the
        :class:`WeightedHistory` of the previous frame (or ``WeightedHistory.empty``).  ``params``: those of
        ``_weighted_lib.DEFAULTS`` -> the :class:`WeightedHistory` of this frame."""
        v, index, normals, points, width, height = _one_record_frame(values, hits, "the accumulation")
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(height, width)
        normals = np.asarray(normals, dtype=np.float64).reshape(height, width, 3)
        points = np.asarray(points, dtype=np.float64).reshape(height, width, 3)
        if np.asarray(prev.count).shape != (height, width):
            raise ValueError(f"a history of {np.asarray(prev.count).shape} for a frame of {height} x {width}")
        if samples is not None:
            samples = np.asarray(samples)
            if samples.size != height * width:
                raise ValueError(f"{samples.size} sample counts for a frame of {height} x {width}")
            samples = samples.reshape(-1)
        out, moments, count = self.scene.weighted(v.reshape(-1, 3), samples, index.reshape(-1), normals.reshape(-1, 3), points.reshape(-1, 3),
                                                  np.asarray(prev.colour).reshape(-1, 3), np.asarray(prev.moments).reshape(-1, 3),
                                                  np.asarray(prev.shape_index).reshape(-1), np.asarray(prev.normal).reshape(-1, 3),
                                                  np.asarray(prev.point).reshape(-1, 3), np.asarray(prev.count).reshape(-1), prev_camera, width,
                                                  height, **params)
        return WeightedHistory(out, index, normals, points, count, moments)

    def accumulated_moving(self, values, samples, hits, prev: "WeightedHistory", prev_camera, motion, **params) -> "WeightedHistory":
        """:meth:`accumulated_weighted` for a world whose shapes moved since the previous frame -- on the device
        (``DeviceScene.motion``), :func:`motion_host` in every bit.  ``motion``: ``(moved, motion)`` as :func:`shape_motion` returns
        them, or ``None``: nothing moved.  A record whose shape moved is carried into the previous frame's world before it is
        projected onto the previous screen and tested against the taps; the :class:`WeightedHistory` returned holds this frame's
        own records, unmoved, as the next frame's guides."""
        v, index, normals, points, width, height = _one_record_frame(values, hits, "the accumulation")
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(height, width)
        normals = np.asarray(normals, dtype=np.float64).reshape(height, width, 3)
        points = np.asarray(points, dtype=np.float64).reshape(height, width, 3)
        if np.asarray(prev.count).shape != (height, width):
            raise ValueError(f"a history of {np.asarray(prev.count).shape} for a frame of {height} x {width}")
        if samples is not None:
            samples = np.asarray(samples)
            if samples.size != height * width:
                raise ValueError(f"{samples.size} sample counts for a frame of {height} x {width}")
            samples = samples.reshape(-1)
        moved, table = (None, None) if motion is None else motion
        out, moments, count = self.scene.motion(v.reshape(-1, 3), samples, index.reshape(-1), normals.reshape(-1, 3), points.reshape(-1, 3),
                                                np.asarray(prev.colour).reshape(-1, 3), np.asarray(prev.moments).reshape(-1, 3),
                                                np.asarray(prev.shape_index).reshape(-1), np.asarray(prev.normal).reshape(-1, 3),
                                                np.asarray(prev.point).reshape(-1, 3), np.asarray(prev.count).reshape(-1), prev_camera, moved,
                                                table, width, height, **params)
        return WeightedHistory(out, index, normals, points, count, moments)

    def accumulated_gradient(self, values, samples, hits, prev: "WeightedHistory", prev_camera, motion, keep, **params) -> "WeightedHistory":
        """:meth:`accumulated_moving` with the share of its history every pixel keeps -- on the device
        (``DeviceScene.gradient_accumulate``), :func:`gradient_accumulate_host` in every bit.  ``keep``: ``[H, W]`` float64 as
        ``DeviceScene.gradient_keep`` returns it (1: the light did not change, 0: the history counts for nothing), or ``None``:
        :meth:`accumulated_moving` in every bit."""
        v, index, normals, points, width, height = _one_record_frame(values, hits, "the accumulation")
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(height, width)
        normals = np.asarray(normals, dtype=np.float64).reshape(height, width, 3)
        points = np.asarray(points, dtype=np.float64).reshape(height, width, 3)
        if np.asarray(prev.count).shape != (height, width):
            raise ValueError(f"a history of {np.asarray(prev.count).shape} for a frame of {height} x {width}")
        if samples is not None:
            samples = np.asarray(samples)
            if samples.size != height * width:
                raise ValueError(f"{samples.size} sample counts for a frame of {height} x {width}")
            samples = samples.reshape(-1)
        if keep is not None:
            keep = np.asarray(keep, dtype=np.float64)
            if keep.size != height * width:
                raise ValueError(f"{keep.size} keep values for a frame of {height} x {width}")
            keep = keep.reshape(-1)
        moved, table = (None, None) if motion is None else motion
        out, moments, count = self.scene.gradient_accumulate(v.reshape(-1, 3), samples, index.reshape(-1), normals.reshape(-1, 3),
                                                             points.reshape(-1, 3), np.asarray(prev.colour).reshape(-1, 3),
                                                             np.asarray(prev.moments).reshape(-1, 3), np.asarray(prev.shape_index).reshape(-1),
                                                             np.asarray(prev.normal).reshape(-1, 3), np.asarray(prev.point).reshape(-1, 3),
                                                             np.asarray(prev.count).reshape(-1), prev_camera, moved, table, keep, width, height,
                                                             **params)
        return WeightedHistory(out, index, normals, points, count, moments)

    def variance_filtered(self, values, hits, variance=None, count=None, **params):
        """``values`` filtered by the variance-guided a-trous filter of include/ptrace_variance.h, guided by ``hits`` -- on the
        device (``DeviceScene.variance_filter``), :func:`variance_filter_host` in every bit.  ``values`` and ``hits``: as
        :meth:`denoised` takes them, ONE record per pixel, the DEMODULATED signal; ``variance``: ``[H, W]``, the variance of
        ``values`` per pixel (what :class:`VarianceAccumulator` returns).  ``variance=None`` is the single-frame route, for one
        gather or one light map: the luminance moments of this frame, ``count`` 1 everywhere (so the estimate is the spatial one
        over a 7x7 window; ``count=``: other history lengths ``[H, W]``), then the filter.  ``params``: those of
        ``_variance_lib.DEFAULTS`` -> ``(colour [H, W, 3], variance [H, W])``."""
        v, index, normals, points, width, height = _one_record_frame(values, hits, "the filter")
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        normals, points = np.asarray(normals).reshape(-1, 3), np.asarray(points).reshape(-1, 3)
        if variance is None:
            moments = self.scene.variance_moments(v.reshape(-1, 3), index, width, height)
            count = np.ones(height * width, dtype=np.int32) if count is None else np.asarray(count, dtype=np.int32).reshape(-1)
            if count.shape[0] != height * width:
                raise ValueError(f"{count.shape[0]} history lengths for a frame of {height} x {width}")
            variance = self.scene.variance_estimate(moments.reshape(-1, 3), count, index, normals, points, width, height, **params)
        elif count is not None:
            raise ValueError("count= goes with variance=None (a variance handed in is used as it is)")
        if np.asarray(variance).size != height * width:
            raise ValueError(f"a variance of {np.asarray(variance).shape} for a frame of {height} x {width}")
        return self.scene.variance_filter(v.reshape(-1, 3), np.asarray(variance).reshape(-1), index, normals, points, width, height, **params)

    def radiance_probes(self, points, samples, init_state: int = 42, init_seq: int = 54, seqs=None, active=None, num_of_rays: int = 1,
                        max_depth: int = 10, russian_roulette_limit: int = 3, background=(0.0, 0.0, 0.0), depth: int = 1,
                        channels="all") -> ProbeSet:
        """The order-2 spherical-harmonic coefficients of the radiance arriving at every point of ``points`` (``[..., 3]``, free
        points of the world: no surface, no normal): ``samples`` rays per probe, sample ``k`` of probe ``i`` uniform on the sphere
        from ``PCG(init_state, seqs[i] + k)`` and followed by ``PathTracer(world, background, that generator, num_of_rays,
        max_depth, russian_roulette_limit)``; projected on the device, strictly in sample order.  ``seqs=None``: probe ``i``
        starts at stream ``init_seq + i * samples``.  ``active``: an optional int32 array, negative = skipped.  ``depth``: the
        rays' ``Ray.depth``; the default 1 (as :meth:`light_map`) means they are the rays a depth-0 hit at that point would
        send -> :class:`ProbeSet`, shaped like the points."""
        points = np.asarray(points, dtype=np.float64)
        if points.ndim < 1 or points.shape[-1] != 3:
            raise ValueError(f"points must be [..., 3], not {points.shape}")
        bits = sh_channels(channels)
        out = self.scene.sh_project(planar(points, 3), samples, init_state, init_seq, seqs, active, num_of_rays, max_depth,
                                    russian_roulette_limit, background, depth, bits)
        return ProbeSet(out.buffer, out.n, bits, shape=points.shape[:-1], evaluator=self.scene.sh_eval)

    def probe_directions(self, n: int, samples: int, init_state: int = 42, init_seq: int = 54, seqs=None) -> np.ndarray:
        """``[n, samples, 3]``: the directions the samples of ``n`` probes take, made on the device by the function the
        projection uses (what :meth:`surface_points` is for the bake)."""
        out = self.scene.sh_directions(n, samples, init_state, init_seq, seqs)
        return np.ascontiguousarray(out.T).reshape(int(n), int(samples), 3)

    def probe_map(self, shape: int, width: int, height: int, probes: ProbeSet, probe: int = 0, side: int = 1) -> np.ndarray:
        """``[height, width, 3]``: the light map of ``World.shapes[shape]`` as ONE probe sees it -- ``probes.hemisphere_mean`` at
        the normals of the texel centres (:meth:`surface_points`).  For a shape small against its distance to everything else:
        the probe stands for every point of it."""
        _, normals = self.surface_points(shape, texel_centres(width, height), side)
        return probes.hemisphere_mean(normals, index=int(probe))

    def outgoing_probe_map(self, shape: int, width: int, height: int, probes: ProbeSet, probe: int = 0, side: int = 1) -> np.ndarray:
        """``[height, width, 3]``: what a ``DiffuseBRDF`` shape sends out at every texel when lit by one probe, ``emitted(uv_c) +
        brdf_color(uv_c) * probe_map`` (:meth:`outgoing_map` with :meth:`probe_map` in place of a bake): a map for
        ``scenes.baked_world``."""
        from types import SimpleNamespace

        centres = texel_centres(width, height)
        index = np.full(centres.shape[:-1], int(shape), dtype=np.int32)
        mat = self.materials(SimpleNamespace(shape_index=index, uv=centres))
        if not np.all(np.asarray(mat.brdf_kind) == abi.BRDF_DIFFUSE):
            raise ValueError(f"shape {shape} has no DiffuseBRDF: what a mirror sends out depends on where it is seen from, a map cannot hold it")
        return np.asarray(mat.emitted) + np.asarray(mat.brdf_color) * self.probe_map(shape, width, height, probes, probe, side)


# ---- accumulation over frames (include/ptrace_temporal.h) ---------------------------------------------------------------------------
class TemporalHistory:
    """What one frame hands to the next: the accumulated ``colour`` ``[H, W, 3]``, the guides it was made for (``shape_index``
    ``[H, W]`` int32, ``normal`` and ``point`` ``[H, W, 3]``) and the history lengths ``count`` ``[H, W]`` int32."""

    def __init__(self, colour, shape_index, normal, point, count):
        self.colour, self.shape_index, self.normal, self.point, self.count = colour, shape_index, normal, point, count

    @classmethod
    def empty(cls, width: int, height: int) -> "TemporalHistory":
        """The history before the first frame: every length 0, so nothing of it is ever read."""
        h, w = int(height), int(width)
        return cls(np.zeros((h, w, 3)), np.full((h, w), -1, dtype=np.int32), np.zeros((h, w, 3)), np.zeros((h, w, 3)),
                   np.zeros((h, w), dtype=np.int32))


class DeviceGuides:
    """The guides of a frame that lies in HBM: ``shape_index`` (``m`` int32), ``normal`` and ``point`` (``[3, m]`` fp64) as
    ``DeviceBuffer`` s, device tensors or raw addresses.  ``keep``: whatever owns the memory (held, not used)."""

    def __init__(self, shape_index, normal, point, keep=None):
        self.shape_index, self.normal, self.point, self.keep = shape_index, normal, point, keep

    @classmethod
    def of_hit_buffer(cls, buffer, params, channels=abi.HIT_ALL) -> "DeviceGuides":
        """The planes of a hit-record frame of ONE sample per pixel that ``DeviceScene.render_hits_into`` wrote into ``buffer``."""
        channels = abi.hit_channels(channels)
        if not (channels & abi.HIT_POINT and channels & abi.HIT_NORMAL):
            raise ValueError("the hit frame must carry the point and normal channels")
        base = int(buffer.data_ptr()) if callable(getattr(buffer, "data_ptr", None)) else int(buffer)
        return cls(base, base + abi.hits_plane_offset(params, channels, abi.HIT_NORMAL, 0),
                   base + abi.hits_plane_offset(params, channels, abi.HIT_POINT, 0), keep=buffer)

    def addresses(self) -> tuple:
        return tuple(int(x.data_ptr()) if callable(getattr(x, "data_ptr", None)) else int(x) for x in (self.shape_index, self.normal, self.point))


class TemporalAccumulator:
    """The accumulate query over a sequence of frames: ``update(values, hits, camera)`` blends this frame's demodulated ``values``
    with what the previous ``update`` left, reprojected through the previous camera (``WorldQueries.accumulated``), and keeps the
    result, this frame's guides, the history lengths and the camera for the next call.  ONE sample per pixel, like
    ``WorldQueries.denoised``.  It starts from a history of zero lengths, so the first frame takes the path of every other.
    ``params``: ``max_history``, ``same_shape``, ``normal_min``, ``point_tolerance``.

    ``device=False``: ``values`` and ``hits`` as ``WorldQueries.accumulated`` takes them; ``update`` returns the accumulated ``E``
    ``[H, W, 3]`` and ``count`` holds the lengths ``[H, W]``; the history is kept on the host and staged by every call.

    ``device=True``: everything stays in HBM.  ``values``: the ``[3, m]`` fp64 planes of a device gather (a ``DeviceBuffer`` or a
    raw address), ``hits``: a :class:`DeviceGuides`, with ``width=`` and ``height=``; the one launch is enqueued on ``stream``.
    Two colour and two count buffers are ping-ponged: ``update`` returns the colour ``DeviceBuffer`` it wrote (``[3, m]``; valid
    until the next but one ``update``), ``count`` is the count buffer.  The previous frame's guides are read where the caller left
    them: alternate two hit buffers."""

    def __init__(self, queries, device: bool = False, stream=None, **params):
        from ._temporal_lib import DEFAULTS

        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"TemporalAccumulator: unknown accumulation parameter(s) {sorted(unknown)}")
        if stream is not None and not device:
            raise ValueError("stream= goes with device=True (host frames are staged and synchronous)")
        self.queries, self.device, self.stream, self.params = queries, bool(device), stream, dict(params)
        self._buffers, self._m = None, -1
        self.reset()

    def reset(self) -> None:
        """Forget the history: the next ``update`` starts a sequence."""
        self._prev, self._camera, self.count, self.frames = None, None, None, 0

    def update(self, values, hits, camera, width=None, height=None):
        from . import _temporal_lib

        cam = _temporal_lib.camera(camera)
        cam = _temporal_lib.TemporalCamera.from_buffer_copy(cam)  # (the caller's camera may move on)
        if not self.device:
            if width is not None or height is not None:
                raise ValueError("width= and height= go with device=True (a host frame brings its own)")
            prev, prev_camera = self._prev, self._camera
            if prev is None:
                _, _, _, _, w, h = _one_record_frame(values, hits, "the accumulation")
                prev, prev_camera = TemporalHistory.empty(w, h), cam
            new = self.queries.accumulated(values, hits, prev, prev_camera, **self.params)
            self._prev, self._camera, self.count = new, cam, new.count
            self.frames += 1
            return new.colour
        from .devmem import DeviceBuffer

        if width is None or height is None:
            raise ValueError("device=True needs width= and height=: planes in HBM do not say what frame they are")
        if not isinstance(hits, DeviceGuides):
            raise TypeError(f"device=True takes hits as a DeviceGuides, not {type(hits).__name__}")
        scene = self.queries.scene
        m = int(width) * int(height)
        if self._buffers is None or self._m != m:
            self._buffers = [(DeviceBuffer((3, max(m, 1)), np.float64, scene.device), DeviceBuffer((max(m, 1),), np.int32, scene.device))
                             for _ in range(2)]
            self._m = m
            self.reset()
        out, out_count = self._buffers[self.frames & 1]
        prev_colour, prev_count = self._buffers[(self.frames & 1) ^ 1]
        prev, prev_camera = self._prev, self._camera
        if prev is None:  # (lengths of 0: neither the other colour buffer nor the guides handed in as the previous ones are read)
            scene.temporal_clear(prev_count, m, self.stream)
            prev, prev_camera = hits, cam
        elif set(prev.addresses()) & set(hits.addresses()):
            raise ValueError("this frame's guides lie where the previous frame's did: alternate two hit buffers")
        scene.temporal(values, hits.shape_index, hits.normal, hits.point, prev_colour, prev.shape_index, prev.normal, prev.point, prev_count,
                       prev_camera, width, height, device=True, stream=self.stream, out=out, out_count=out_count, **self.params)
        self._prev, self._camera, self.count = hits, cam, out_count
        self.frames += 1
        return out


class VarianceAccumulator:
    """The accumulate query twice over a sequence of frames -- once for the demodulated ``values``, once for their luminance moments
    (``DeviceScene.variance_moments``; the same guides, cameras and parameters, so the same taps and the same ``count``) -- and the
    variance estimate of include/ptrace_variance.h from the accumulated moments: ``update(values, hits, camera)`` returns
    ``(accumulated E, variance)``, the two inputs of ``WorldQueries.variance_filtered`` / ``DeviceScene.variance_filter``.  It owns
    two :class:`TemporalAccumulator` s (``colour`` and ``moments``).  ``params``: ``max_history`` (the accumulation's),
    ``min_history`` (the estimate's), and ``same_shape``, ``normal_min``, ``point_tolerance``, which both read.

    ``device=False``: ``values`` and ``hits`` as ``WorldQueries.accumulated`` takes them; ``update`` returns ``E`` ``[H, W, 3]`` and
    the variance ``[H, W]``; ``count`` holds the lengths ``[H, W]``.

    ``device=True``: everything stays in HBM, with the buffer lifetimes of :class:`TemporalAccumulator`: ``values`` are ``[3, m]``
    fp64 planes, ``hits`` a :class:`DeviceGuides` (alternate two hit buffers), with ``width=`` and ``height=``; the four launches
    are enqueued on ``stream``; ``update`` returns the colour ``DeviceBuffer`` (``[3, m]``) and the variance ``DeviceBuffer``
    (``[m]``), both valid until the next but one ``update``; ``count`` is the count buffer."""

    HISTORY_KEYS = ("max_history", "same_shape", "normal_min", "point_tolerance")
    ESTIMATE_KEYS = ("min_history", "same_shape", "normal_min", "point_tolerance")

    def __init__(self, queries, device: bool = False, stream=None, **params):
        unknown = set(params) - set(self.HISTORY_KEYS) - set(self.ESTIMATE_KEYS)
        if unknown:
            raise TypeError(f"VarianceAccumulator: unknown accumulation or estimate parameter(s) {sorted(unknown)}")
        self.history_params = {k: v for k, v in params.items() if k in self.HISTORY_KEYS}
        self.estimate_params = {k: v for k, v in params.items() if k in self.ESTIMATE_KEYS}
        self.queries, self.device, self.stream = queries, bool(device), stream
        self.colour = TemporalAccumulator(queries, device, stream, **self.history_params)
        self.moments = TemporalAccumulator(queries, device, stream, **self.history_params)
        self._scratch, self._m = None, -1
        self.count = None

    @property
    def frames(self) -> int:
        return self.colour.frames

    def reset(self) -> None:
        """Forget the history: the next ``update`` starts a sequence."""
        self.colour.reset()
        self.moments.reset()
        self.count = None

    def update(self, values, hits, camera, width=None, height=None):
        scene = self.queries.scene
        if not self.device:
            if width is not None or height is not None:
                raise ValueError("width= and height= go with device=True (a host frame brings its own)")
            v, index, normals, points, w, h = _one_record_frame(values, hits, "the accumulation")
            index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
            moments = scene.variance_moments(v.reshape(-1, 3), index, w, h)
            guides = (np.asarray(points).reshape(h, w, 3), np.asarray(normals).reshape(h, w, 3), index.reshape(h, w))
            colour = self.colour.update(v.reshape(h, w, 3), guides, camera)
            mu = self.moments.update(moments, guides, camera)
            self.count = self.colour.count
            variance = scene.variance_estimate(np.asarray(mu).reshape(-1, 3), np.asarray(self.count).reshape(-1), index, guides[1].reshape(-1, 3),
                                               guides[0].reshape(-1, 3), w, h, **self.estimate_params)
            return colour, variance
        from .devmem import DeviceBuffer

        if width is None or height is None:
            raise ValueError("device=True needs width= and height=: planes in HBM do not say what frame they are")
        if not isinstance(hits, DeviceGuides):
            raise TypeError(f"device=True takes hits as a DeviceGuides, not {type(hits).__name__}")
        m = int(width) * int(height)
        if self._scratch is None or self._m != m:
            self._scratch = (DeviceBuffer((3, max(m, 1)), np.float64, scene.device),
                             [DeviceBuffer((max(m, 1),), np.float64, scene.device) for _ in range(2)])
            self._m = m
        frame, variances = self._scratch
        out_variance = variances[self.colour.frames & 1]
        scene.variance_moments(values, hits.shape_index, width, height, device=True, stream=self.stream, out=frame)
        colour = self.colour.update(values, hits, camera, width, height)
        mu = self.moments.update(frame, hits, camera, width, height)
        self.count = self.colour.count
        scene.variance_estimate(mu, self.count, hits.shape_index, hits.normal, hits.point, width, height, device=True, stream=self.stream,
                                out=out_variance, **self.estimate_params)
        return colour, out_variance


# ---- accumulation weighted by samples (include/ptrace_weighted.h) ----------------------------------------------------------------------
class WeightedHistory(TemporalHistory):
    """:class:`TemporalHistory` plus ``moments`` ``[H, W, 3]``: the accumulated luminance moments M1, M2 and the accumulated weight S."""

    def __init__(self, colour, shape_index, normal, point, count, moments):
        super().__init__(colour, shape_index, normal, point, count)
        self.moments = moments

    @classmethod
    def empty(cls, width: int, height: int) -> "WeightedHistory":
        """The history before the first frame: every length 0, so nothing of it is ever read."""
        base = TemporalHistory.empty(width, height)
        return cls(base.colour, base.shape_index, base.normal, base.point, base.count, np.zeros((int(height), int(width), 3)))


class WeightedAccumulator:
    """The counterpart of :class:`VarianceAccumulator` on the weighted accumulate query (include/ptrace_weighted.h): every frame
    counts by the samples it took.  ``update(values, hits, camera, samples=None)`` returns ``(accumulated E, variance)`` from TWO
    launches -- ``DeviceScene.weighted``, which finds the taps once and blends colour, luminance moments and weight, and
    ``DeviceScene.variance_estimate`` on its moments and lengths -- where :class:`VarianceAccumulator` makes four.  ``samples``: what
    this frame took per record (int32; ``None``: one everywhere; 0: nothing was sampled there, the reprojected history is carried
    and the record's colour is never read into it).  ``params``: ``max_history``, ``max_weight``, ``blend_weight`` (the
    accumulation's), ``min_history`` (the estimate's), and ``same_shape``, ``normal_min``, ``point_tolerance``, which both read.
    ``count`` holds the history lengths, ``weight`` the accumulated weights S, ``frames`` the number of updates since ``reset()``.

    ``device=False``: ``values`` and ``hits`` as ``WorldQueries.accumulated`` takes them, ``samples`` ``[H, W]``; ``update`` returns
    ``E`` ``[H, W, 3]`` and the variance ``[H, W]``; ``count`` and ``weight`` are ``[H, W]``.

    ``device=True``: everything stays in HBM, with the buffer lifetimes of :class:`TemporalAccumulator`: ``values`` are ``[3, m]``
    fp64 planes, ``samples`` ``m`` int32 (a ``DeviceBuffer`` or a raw address, such as the ``TAKEN`` plane of a ragged gather),
    ``hits`` a :class:`DeviceGuides` (alternate two hit buffers), with ``width=`` and ``height=``; the two launches are enqueued on
    ``stream``; ``update`` returns the colour ``DeviceBuffer`` (``[3, m]``) and the variance ``DeviceBuffer`` (``[m]``), both valid
    until the next but one ``update``; ``count`` is the count buffer, ``weight`` the address of the S plane of the moments buffer
    (``moments``, ``[3, m]``)."""

    HISTORY_KEYS = ("max_history", "max_weight", "blend_weight", "same_shape", "normal_min", "point_tolerance")
    ESTIMATE_KEYS = ("min_history", "same_shape", "normal_min", "point_tolerance")

    def __init__(self, queries, device: bool = False, stream=None, **params):
        unknown = set(params) - set(self.HISTORY_KEYS) - set(self.ESTIMATE_KEYS)
        if unknown:
            raise TypeError(f"WeightedAccumulator: unknown accumulation or estimate parameter(s) {sorted(unknown)}")
        if stream is not None and not device:
            raise ValueError("stream= goes with device=True (host frames are staged and synchronous)")
        self.history_params = {k: v for k, v in params.items() if k in self.HISTORY_KEYS}
        self.estimate_params = {k: v for k, v in params.items() if k in self.ESTIMATE_KEYS}
        self.queries, self.device, self.stream = queries, bool(device), stream
        self._buffers, self._m = None, -1
        self.reset()

    def reset(self) -> None:
        """Forget the history: the next ``update`` starts a sequence."""
        self._prev, self._camera, self.count, self.weight, self.moments, self.frames = None, None, None, None, None, 0

    def update(self, values, hits, camera, samples=None, width=None, height=None):
        from . import _weighted_lib

        scene = self.queries.scene
        cam = _weighted_lib.camera(camera)
        cam = _weighted_lib.WeightedCamera.from_buffer_copy(cam)  # (the caller's camera may move on)
        if not self.device:
            if width is not None or height is not None:
                raise ValueError("width= and height= go with device=True (a host frame brings its own)")
            prev, prev_camera = self._prev, self._camera
            if prev is None:
                _, _, _, _, w, h = _one_record_frame(values, hits, "the accumulation")
                prev, prev_camera = WeightedHistory.empty(w, h), cam
            new = self.queries.accumulated_weighted(values, samples, hits, prev, prev_camera, **self.history_params)
            h, w = np.asarray(new.count).shape
            variance = scene.variance_estimate(np.asarray(new.moments).reshape(-1, 3), np.asarray(new.count).reshape(-1),
                                               new.shape_index.reshape(-1), new.normal.reshape(-1, 3), new.point.reshape(-1, 3), w, h,
                                               **self.estimate_params)
            self._prev, self._camera, self.count, self.moments = new, cam, new.count, new.moments
            self.weight = np.asarray(new.moments)[..., 2]
            self.frames += 1
            return new.colour, variance
        from .devmem import DeviceBuffer

        if width is None or height is None:
            raise ValueError("device=True needs width= and height=: planes in HBM do not say what frame they are")
        if not isinstance(hits, DeviceGuides):
            raise TypeError(f"device=True takes hits as a DeviceGuides, not {type(hits).__name__}")
        m = int(width) * int(height)
        if self._buffers is None or self._m != m:
            n = max(m, 1)
            self._buffers = [(DeviceBuffer((3, n), np.float64, scene.device), DeviceBuffer((3, n), np.float64, scene.device),
                              DeviceBuffer((n,), np.int32, scene.device), DeviceBuffer((n,), np.float64, scene.device)) for _ in range(2)]
            self._m = m
            self.reset()
        out, out_moments, out_count, out_variance = self._buffers[self.frames & 1]
        prev_colour, prev_moments, prev_count, _ = self._buffers[(self.frames & 1) ^ 1]
        prev, prev_camera = self._prev, self._camera
        if prev is None:  # (lengths of 0: neither the other buffers nor the guides handed in as the previous ones are read)
            scene.weighted_clear(prev_count, m, self.stream)
            prev, prev_camera = hits, cam
        elif set(prev.addresses()) & set(hits.addresses()):
            raise ValueError("this frame's guides lie where the previous frame's did: alternate two hit buffers")
        scene.weighted(values, samples, hits.shape_index, hits.normal, hits.point, prev_colour, prev_moments, prev.shape_index, prev.normal,
                       prev.point, prev_count, prev_camera, width, height, device=True, stream=self.stream, out=out, out_moments=out_moments,
                       out_count=out_count, **self.history_params)
        scene.variance_estimate(out_moments, out_count, hits.shape_index, hits.normal, hits.point, width, height, device=True, stream=self.stream,
                                out=out_variance, **self.estimate_params)
        self._prev, self._camera, self.count, self.moments = hits, cam, out_count, out_moments
        self.weight = int(out_moments.data_ptr()) + 16 * m  # (plane 2 of [3, m] fp64)
        self.frames += 1
        return out, out_variance


# ---- accumulation that follows the shapes that moved (include/ptrace_motion.h) -----------------------------------------------------
def _snapshot(world):
    """The shapes of ``world`` as they are now (shallow copies: each keeps its kind and the transformation it has), so that a caller
    who gives a shape of the same ``World`` a new transformation for the next frame is seen to have moved it."""
    import copy
    from types import SimpleNamespace

    return SimpleNamespace(shapes=[copy.copy(s) for s in world.shapes])


class MotionAccumulator(WeightedAccumulator):
    """:class:`WeightedAccumulator` on the motion accumulate query (include/ptrace_motion.h): the history of a shape that moved
    between two frames is fetched where that surface point was.  ``update(values, hits, camera, samples=None, world=None,
    motion=None, queries=None)`` returns ``(accumulated E, variance)`` from TWO launches, ``DeviceScene.motion`` and
    ``DeviceScene.variance_estimate``.

    ``world=``: this frame's ``World``; the accumulator keeps the previous one and calls :func:`shape_motion` (with ``static``, the
    shapes that move onto themselves -- see there).  ``motion=``: ``(moved, motion)``, a table of the caller's, instead.  Neither:
    nothing moved, and every bit is :class:`WeightedAccumulator`'s.  ``queries=`` replaces the queries object: every frame of a
    moving world has a device scene of its own, and the accumulation reads none.  Everything else, ``device=True`` and its buffer
    lifetimes included, is :class:`WeightedAccumulator`'s; on the device the tables are uploaded by ``DeviceScene.motion_table`` and
    kept until the next but one ``update``."""

    def __init__(self, queries, device: bool = False, stream=None, static=(), **params):
        self.static = tuple(static)
        self._world, self._tables = None, [None, None]
        try:
            super().__init__(queries, device, stream, **params)
        except TypeError as e:
            raise TypeError(str(e).replace("WeightedAccumulator", "MotionAccumulator")) from None

    def reset(self) -> None:
        """Forget the history and the previous world: the next ``update`` starts a sequence."""
        super().reset()
        self._world = None

    def update(self, values, hits, camera, samples=None, world=None, motion=None, queries=None, width=None, height=None):
        from . import _motion_lib

        if queries is not None:
            self.queries = queries
        if world is not None and motion is not None:
            raise ValueError("world= (the accumulator derives the motion) or motion= (a table of the caller's), not both")
        if world is not None and self._world is not None and self._prev is not None:
            motion = shape_motion(self._world, world, self.static)
        scene = self.queries.scene
        cam = _motion_lib.camera(camera)
        cam = _motion_lib.MotionCamera.from_buffer_copy(cam)  # (the caller's camera may move on)
        if not self.device:
            if width is not None or height is not None:
                raise ValueError("width= and height= go with device=True (a host frame brings its own)")
            prev, prev_camera = self._prev, self._camera
            if prev is None:
                _, _, _, _, w, h = _one_record_frame(values, hits, "the accumulation")
                prev, prev_camera = WeightedHistory.empty(w, h), cam
            new = self.queries.accumulated_moving(values, samples, hits, prev, prev_camera, motion, **self.history_params)
            h, w = np.asarray(new.count).shape
            variance = scene.variance_estimate(np.asarray(new.moments).reshape(-1, 3), np.asarray(new.count).reshape(-1),
                                               new.shape_index.reshape(-1), new.normal.reshape(-1, 3), new.point.reshape(-1, 3), w, h,
                                               **self.estimate_params)
            self._prev, self._camera, self.count, self.moments = new, cam, new.count, new.moments
            self.weight = np.asarray(new.moments)[..., 2]
            self._world = None if world is None else _snapshot(world)
            self.frames += 1
            return new.colour, variance
        from .devmem import DeviceBuffer

        if width is None or height is None:
            raise ValueError("device=True needs width= and height=: planes in HBM do not say what frame they are")
        if not isinstance(hits, DeviceGuides):
            raise TypeError(f"device=True takes hits as a DeviceGuides, not {type(hits).__name__}")
        m = int(width) * int(height)
        if self._buffers is None or self._m != m:
            n = max(m, 1)
            self._buffers = [(DeviceBuffer((3, n), np.float64, scene.device), DeviceBuffer((3, n), np.float64, scene.device),
                              DeviceBuffer((n,), np.int32, scene.device), DeviceBuffer((n,), np.float64, scene.device)) for _ in range(2)]
            self._m = m
            self.reset()
            motion = None  # (a new frame size starts a sequence: nothing to follow)
        out, out_moments, out_count, out_variance = self._buffers[self.frames & 1]
        prev_colour, prev_moments, prev_count, _ = self._buffers[(self.frames & 1) ^ 1]
        prev, prev_camera = self._prev, self._camera
        if prev is None:  # (lengths of 0: neither the other buffers nor the guides handed in as the previous ones are read)
            scene.motion_clear(prev_count, m, self.stream)
            prev, prev_camera = hits, cam
        elif set(prev.addresses()) & set(hits.addresses()):
            raise ValueError("this frame's guides lie where the previous frame's did: alternate two hit buffers")
        moved_dev, motion_dev = (None, None) if motion is None else scene.motion_table(*motion)
        self._tables[self.frames & 1] = (moved_dev, motion_dev)  # (held while the launch that reads them may be in flight)
        scene.motion(values, samples, hits.shape_index, hits.normal, hits.point, prev_colour, prev_moments, prev.shape_index, prev.normal,
                     prev.point, prev_count, prev_camera, moved_dev, motion_dev, width, height, device=True, stream=self.stream, out=out,
                     out_moments=out_moments, out_count=out_count, **self.history_params)
        scene.variance_estimate(out_moments, out_count, hits.shape_index, hits.normal, hits.point, width, height, device=True, stream=self.stream,
                                out=out_variance, **self.estimate_params)
        self._prev, self._camera, self.count, self.moments = hits, cam, out_count, out_moments
        self.weight = int(out_moments.data_ptr()) + 16 * m  # (plane 2 of [3, m] fp64)
        self._world = None if world is None else _snapshot(world)
        self.frames += 1
        return out, out_variance


# ---- accumulation that also follows the light (include/ptrace_gradient.h) ------------------------------------------------------------
class GradientAccumulator(MotionAccumulator):
    """:class:`MotionAccumulator` on the gradient accumulate query (include/ptrace_gradient.h): the history of a pixel shortens where
    the LIGHT changed -- under a shadow that moved, in the reflection of a shape that did.  ``update(values, hits, camera,
    samples=None, world=None, motion=None, queries=None, probe=None)`` returns ``(accumulated E, variance)``.  From the second frame
    on, with ``probe=``, it makes FIVE launches: ``DeviceScene.gradient_probes`` picks one pixel per stratum of this frame and carries
    it into the previous world; ``DeviceScene.gather`` ON THE PREVIOUS FRAME'S SCENE gathers there with this frame's streams, so that
    what differs from this frame's ``values`` at those pixels is what the world's change did, free of sampling noise;
    ``DeviceScene.gradient_keep`` spreads that over the frame; ``DeviceScene.gradient_accumulate`` is the motion accumulate query with
    the history's weight and length multiplied by it; ``DeviceScene.variance_estimate`` as before.

    ``probe=``: how ``values`` was gathered -- ``dict(samples=K, init_state=42, init_seq=54, num_of_rays=1, max_depth=10,
    russian_roulette_limit=3, background=(0, 0, 0), depth=0)``, the arguments of ``DeviceScene.gather`` for THIS frame (a uniform
    gather: record ``i`` has the streams ``init_seq + i * K ..``; adaptive and ragged counts stay out) -- and optionally ``queries=``,
    a ``WorldQueries`` on the previous world's scene when the one the accumulator kept from the previous ``update`` has been closed.
    With no ``probe=``, or on a first frame, every bit is :class:`MotionAccumulator`'s.  The PREVIOUS frame's device scene must stay
    open until this frame's ``update`` has enqueued its gather (``device=True``: until that gather has run).

    ``params``: :class:`MotionAccumulator`'s, and ``stratum`` (1..16), ``radius`` (0..4), ``gain`` and ``same_shape_probes``.  ``keep``
    holds the last keep plane (``[H, W]``, or the ``DeviceBuffer``; ``None`` when the last update made none).  ``device=True`` keeps
    every plane in HBM on the one stream, with the buffer lifetimes of :class:`WeightedAccumulator`; the probe planes and the keep
    plane alternate between two sets like the outputs.  Shapes that ROTATE give their probes a turned normal, hence other sample
    directions: their gradient contains sampling noise."""

    KEEP_KEYS = ("stratum", "radius", "gain", "same_shape_probes")
    PROBE_KEYS = ("samples", "init_state", "init_seq", "num_of_rays", "max_depth", "russian_roulette_limit", "background", "depth", "queries")

    def __init__(self, queries, device: bool = False, stream=None, static=(), **params):
        from . import _gradient_lib

        self.keep_params = dict(_gradient_lib.KEEP_DEFAULTS)
        self.keep_params.update({k: params.pop(k) for k in self.KEEP_KEYS if k in params})
        self._prev_queries, self._probe_buffers, self.keep = None, [None, None], None
        try:
            super().__init__(queries, device, stream, static, **params)
        except TypeError as e:
            raise TypeError(str(e).replace("MotionAccumulator", "GradientAccumulator")) from None

    def reset(self) -> None:
        """Forget the history, the previous world and its scene: the next ``update`` starts a sequence."""
        super().reset()
        self._prev_queries, self.keep = None, None

    def update(self, values, hits, camera, samples=None, world=None, motion=None, queries=None, probe=None, width=None, height=None):
        from . import _gradient_lib

        if probe is not None:
            unknown = set(probe) - set(self.PROBE_KEYS)
            if unknown or "samples" not in probe:
                raise TypeError(f"GradientAccumulator: probe= takes samples= and any of {self.PROBE_KEYS[1:]}, not {sorted(unknown)}")
        before = self._prev_queries if probe is None or probe.get("queries") is None else probe["queries"]
        first = self._prev is None or (self.device and (self._buffers is None or self._m != int(width or 0) * int(height or 0)))
        if probe is None or first or before is None:  # (nothing to compare with: the motion query, bit for bit)
            result = super().update(values, hits, camera, samples=samples, world=world, motion=motion, queries=queries, width=width, height=height)
            self._prev_queries, self.keep = self.queries, None
            return result
        if queries is not None:
            self.queries = queries
        if world is not None and motion is not None:
            raise ValueError("world= (the accumulator derives the motion) or motion= (a table of the caller's), not both")
        if world is not None and self._world is not None:
            motion = shape_motion(self._world, world, self.static)
        scene = self.queries.scene
        cam = _gradient_lib.GradientCamera.from_buffer_copy(_gradient_lib.camera(camera))  # (the caller's camera may move on)
        K = int(probe["samples"])
        init_seq = int(probe.get("init_seq", 54))
        gather = dict(init_state=probe.get("init_state", 42), num_of_rays=probe.get("num_of_rays", 1), max_depth=probe.get("max_depth", 10),
                      russian_roulette_limit=probe.get("russian_roulette_limit", 3), background=probe.get("background", (0.0, 0.0, 0.0)),
                      depth=probe.get("depth", 0), channels="none")
        spread = {k: v for k, v in self.keep_params.items() if k != "stratum"}
        stratum = self.keep_params["stratum"]
        moved, table = (None, None) if motion is None else motion
        if not self.device:
            if width is not None or height is not None:
                raise ValueError("width= and height= go with device=True (a host frame brings its own)")
            v, index, normals, points, w, h = _one_record_frame(values, hits, "the accumulation")
            index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
            normals, points = np.asarray(normals, dtype=np.float64).reshape(-1, 3), np.asarray(points, dtype=np.float64).reshape(-1, 3)
            at, where, facing, seqs = scene.gradient_probes(index, normals, points, moved, table, w, h, stratum=stratum, phase=self.frames,
                                                            samples=K, init_seq=init_seq)
            old = before.scene.gather(planar(where, 3), planar(facing, 3), K, seqs=seqs, active=at, **gather).radiance
            keep = scene.gradient_keep(v.reshape(-1, 3), index, at, old, w, h, stratum=stratum, **spread)
            new = self.queries.accumulated_gradient(values, samples, hits, self._prev, self._camera, motion, keep, **self.history_params)
            variance = scene.variance_estimate(np.asarray(new.moments).reshape(-1, 3), np.asarray(new.count).reshape(-1),
                                               new.shape_index.reshape(-1), new.normal.reshape(-1, 3), new.point.reshape(-1, 3), w, h,
                                               **self.estimate_params)
            self._prev, self._camera, self.count, self.moments = new, cam, new.count, new.moments
            self.weight = np.asarray(new.moments)[..., 2]
            self._world = None if world is None else _snapshot(world)
            self._prev_queries, self.keep = self.queries, keep
            self.frames += 1
            return new.colour, variance
        if not isinstance(hits, DeviceGuides):
            raise TypeError(f"device=True takes hits as a DeviceGuides, not {type(hits).__name__}")
        m = int(width) * int(height)
        out, out_moments, out_count, out_variance = self._buffers[self.frames & 1]
        prev_colour, prev_moments, prev_count, _ = self._buffers[(self.frames & 1) ^ 1]
        prev, prev_camera = self._prev, self._camera
        if set(prev.addresses()) & set(hits.addresses()):
            raise ValueError("this frame's guides lie where the previous frame's did: alternate two hit buffers")
        moved_dev, motion_dev = (None, None) if motion is None else scene.motion_table(*motion)
        self._tables[self.frames & 1] = (moved_dev, motion_dev)  # (held while the launches that read them may be in flight)
        ns = _gradient_lib.strata(width, height, stratum)
        held = self._probe_buffers[self.frames & 1]
        probes = scene.gradient_probes(hits.shape_index, hits.normal, hits.point, moved_dev, motion_dev, width, height, stratum=stratum,
                                       phase=self.frames, samples=K, init_seq=init_seq, device=True, stream=self.stream,
                                       out=None if held is None or held["ns"] != ns else held["probes"])
        old = before.scene.gather(probes[1], probes[2], K, seqs=probes[3], active=probes[0], device=True, stream=self.stream, n=ns,
                                  out=None if held is None or held["ns"] != ns else held["old"], **gather)
        keep = scene.gradient_keep(values, hits.shape_index, probes[0], old, width, height, stratum=stratum, device=True, stream=self.stream,
                                   out=None if held is None or held["m"] != m else held["keep"], **spread)
        self._probe_buffers[self.frames & 1] = dict(ns=ns, m=m, probes=probes, old=old, keep=keep)
        scene.gradient_accumulate(values, samples, hits.shape_index, hits.normal, hits.point, prev_colour, prev_moments, prev.shape_index,
                                  prev.normal, prev.point, prev_count, prev_camera, moved_dev, motion_dev, keep, width, height, device=True,
                                  stream=self.stream, out=out, out_moments=out_moments, out_count=out_count, **self.history_params)
        scene.variance_estimate(out_moments, out_count, hits.shape_index, hits.normal, hits.point, width, height, device=True, stream=self.stream,
                                out=out_variance, **self.estimate_params)
        self._prev, self._camera, self.count, self.moments = hits, cam, out_count, out_moments
        self.weight = int(out_moments.data_ptr()) + 16 * m  # (plane 2 of [3, m] fp64)
        self._world = None if world is None else _snapshot(world)
        self._prev_queries, self.keep = self.queries, keep
        self.frames += 1
        return out, out_variance
