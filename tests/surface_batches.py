"""Worlds, hit records and their expected materials and point-light colours for the surface tests (tests/test_surface_host.py,
tests/test_gpu_surface.py).

Per world one batch of records: ``oracle.world_intersect`` of the frame's pixel-centre primary rays, then of the mirror
bounces off their hits (the construction of tests/ray_batches.py).  The records are the ORACLE's and are fed to the device as
host arrays, so (u, v) is glibc's on both sides and everything expected here is compared bit for bit:

* materials: ``oracle.pigment(scene, i, emitted, u, v)`` and ``scene.brdf_kind[i]``;
* lights: ``oracle.radiance(scene, params, Pcg(), ray)`` with ``RENDERER_POINTLIGHT`` and the batch's ambient and background.

All in the oracle's ``x * x`` mode (the device multiplies where the reference writes ``x**2``), computed once per
process and shared; nothing here is modified by a test."""
import math

import numpy as np

from pytracer_amd import abi, flatten, rays as rb, scenes
from pytracer_amd import hostmodel as hm

from . import ray_batches as B
from . import scene_families as F

AMBIENT, BACKGROUND = (0.1, 0.125, 0.05), (0.25, 0.5, 0.125)
# the two lights of test_tile_culling_is_invisible (tests/test_gpu_parity.py): one without, one with a linear radius
TWO_LIGHTS = (((-2.0, 3.0, 6.0), (1.0, 0.9, 0.8), 0.0), ((1.0, -4.0, 5.0), (0.2, 0.3, 0.9), 2.0))
# name -> frame width, height
WORLDS = {"demo": (40, 30), "c2_lights": (48, 27), "wide300_lights": (48, 27), "c2": (48, 27),
          "pigments": F.GOLDEN_SIZE, "lights": F.GOLDEN_SIZE}
SIZES = (1, 63, 64, 65, 255, 256, 257, 1001)  # of the subsets of the c2_lights batch: last wave / block partly idle, odd int32 padding

_worlds, _batches = {}, {}


def with_two_lights(world):
    for pos, col, radius in TWO_LIGHTS:
        world.add_light(hm.PointLight(hm.Vec(*pos), hm.Color(*col), radius))
    return world


def host_world(name):
    """-> (hostmodel World, camera)"""
    w, h = WORLDS[name]
    if name == "demo":
        return scenes.demo_world()
    if name in ("pigments", "lights"):
        world, camera, _, _ = F.family_world(name, F.GOLDEN_SEEDS[name])
        return world, camera
    world = scenes.synthetic_world(300, with_plane=True, wide=True) if name.startswith("wide300") else scenes.synthetic_world(32, with_plane=True)
    return (with_two_lights(world) if name.endswith("_lights") else world), scenes.synthetic_camera(w, h)


def world(name):
    """-> (FlatScene, Camera)"""
    if name not in _worlds:
        wd, cam = host_world(name)
        _worlds[name] = (flatten.flatten_world(wd), flatten.flatten_camera(cam))
    return _worlds[name]


def pointlight_params(ambient=AMBIENT, background=BACKGROUND):
    return abi.make_params(8, 8, abi.RENDERER_POINTLIGHT, ambient=ambient, background=background)


def expected_colors(orc, flat, rays, ambient=AMBIENT, background=BACKGROUND) -> np.ndarray:
    """``PointLightRenderer(world, background, ambient)(ray)`` per ``[n, 8]`` ray -> ``[n, 3]``."""
    par = pointlight_params(ambient, background)
    return np.array([orc.radiance(flat, par, orc.Pcg(), r)[0] for r in np.ascontiguousarray(rays, dtype=np.float64)]).reshape(-1, 3)


def expected_materials(orc, flat, rec) -> dict:
    """brdf_kind / brdf_color / emitted as a surface batch holds them, for the records of a ``RayHits``."""
    n = rec.n
    kind = np.full(n, -1, np.int32)
    pc, em = np.zeros((n, 3)), np.zeros((n, 3))
    uv = np.array(rec.uv)
    for i in np.flatnonzero(rec.hit):
        s = int(rec.shape_index[i])
        kind[i] = int(flat.brdf_kind[s])
        pc[i] = orc.pigment(flat, s, False, float(uv[i, 0]), float(uv[i, 1]))
        em[i] = orc.pigment(flat, s, True, float(uv[i, 0]), float(uv[i, 1]))
    return {"brdf_kind": kind, "brdf_color": pc, "emitted": em}


def mirror_bounces(first, rec) -> np.ndarray:
    """``d - 2 (d.n) n`` from the hit point, tmin 1e-3, off every hit of ``rec`` (the records of the ``[n, 8]`` rays ``first``)."""
    hit = rec.hit & np.isfinite(rec.point).all(axis=1) & np.isfinite(rec.normal).all(axis=1)
    p, nrm, d = rec.point[hit], rec.normal[hit], first[hit, 3:6]
    dn = d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1] + d[:, 2] * nrm[:, 2]
    bounce = np.empty((p.shape[0], 8))
    bounce[:, 0:3], bounce[:, 3:6] = p, d - 2.0 * dn[:, None] * nrm
    bounce[:, 6], bounce[:, 7] = 1e-3, np.inf
    return bounce


def batch(orc, name) -> dict:
    """-> {"rays": [n, 8], "rec": RayHits (the oracle's records), "materials": {...}, "colors": [n, 3], "n_primary": int}"""
    if name in _batches:
        return _batches[name]
    old = orc.lib().pto_get_sqr_mode()
    orc.set_sqr_mode(orc.SQR_MUL)
    try:
        flat, cam = world(name)
        w, h = WORLDS[name]
        first = np.array([orc.tracer_fire_ray(cam, w, h, col, row) for row in range(h) for col in range(w)])
        rays = np.vstack([first, mirror_bounces(first, B.expected(orc, flat, first))])
        rec = B.expected(orc, flat, rays)
        out = {"rays": rays, "rec": rec, "materials": expected_materials(orc, flat, rec), "colors": expected_colors(orc, flat, rays),
               "n_primary": first.shape[0]}
        for a in [rays, out["colors"], rec.buffer] + list(out["materials"].values()):
            a.setflags(write=False)
        _batches[name] = out
        return out
    finally:
        orc.set_sqr_mode(old)


def specular_margins(orc, name) -> list:
    """Over every (record on a specular shape, light the record's point sees) pair of the batch: ``|th_in - th_out|`` minus the
    shape's threshold, the quantity whose SIGN is the one thing a libm call (acos) decides in the lights kernel."""
    b = batch(orc, name)
    flat = world(name)[0]
    rec, rays = b["rec"], b["rays"]
    lpos = np.asarray(flat.light_pos, dtype=np.float64).reshape(3, -1).T
    out = []
    for i in np.flatnonzero(rec.hit):
        s = int(rec.shape_index[i])
        if int(flat.brdf_kind[s]) != abi.BRDF_SPECULAR:
            continue
        wp, nrm = rec.point[i], rec.normal[i]
        for lp in lpos:
            if not orc.is_point_visible(flat, lp, wp):
                continue
            out.append(_angle_gap(wp - lp, nrm, -rays[i, 3:6]) - float(flat.brdf_param[s]))
    return out


def _angle_gap(in_dir, normal, out_dir) -> float:
    def ndot(a, b):
        a, b = a / math.sqrt(float(a @ a)), b / math.sqrt(float(b @ b))
        return max(-1.0, min(1.0, float(a @ b)))

    return abs(math.acos(ndot(normal, in_dir)) - math.acos(ndot(normal, out_dir)))


# ---- the aimed specular cases: a mirror configuration e away from perfect, around the BRDF's threshold -------------------------
THRESHOLD = math.pi / 1800.0
AIMED_E = (THRESHOLD / 2, THRESHOLD - 1e-6, THRESHOLD + 1e-6)
AIMED_RADII = (0.0, 2.0)
AIMED = [(e, radius) for e in AIMED_E for radius in AIMED_RADII]


def aimed_case(e, radius):
    """A specular plane at z = 0, an eye at ``2 (-sin b, 0, cos b)`` looking at the origin, a light at ``3 (sin a, 0, cos a)``
    with ``a = b = pi/2 - e/2``: in the reference in_dir points AT the surface, so th_in = pi - a, th_out = b and
    ``|th_in - th_out| = e``.  -> (FlatScene, the ``[1, 8]`` ray)"""
    a = b = math.pi / 2 - e / 2
    wd = hm.World()
    wd.add_shape(hm.Plane(hm.Transformation(), hm.Material(hm.SpecularBRDF(hm.UniformPigment(hm.Color(0.5, 0.6, 0.7))),
                                                          hm.UniformPigment(hm.Color(0.01, 0.02, 0.03)))))
    wd.add_light(hm.PointLight(hm.Vec(3 * math.sin(a), 0.0, 3 * math.cos(a)), hm.Color(1.0, 0.9, 0.8), radius))
    eye = np.array([-2 * math.sin(b), 0.0, 2 * math.cos(b)])
    ray = np.concatenate([eye, -eye, [1e-5, np.inf]])[None]
    return flatten.flatten_world(wd), ray


def record_planes(rec):
    """The five arguments of ``DeviceScene.shade_lights`` in front of the directions, from a ``RayHits``."""
    return rec.shape_index, rec.point, rec.normal, rec.uv
