"""Worlds, entry rays with generators, and their expected radiance for the radiance-query tests (tests/test_radiance_host.py,
tests/test_gpu_radiance.py).

Entry rays per world: the batch ``scatter_batches.records`` / ``surface_batches.batch`` provide -- the frame's pixel-centre
primary rays, then the mirror bounces off their hits, which start ON a surface -- ray ``i`` with the generator
``PCG(S0, Q0 + i)``.  Expected, per ray: ``oracle.radiance(scene, params, pcg, ray, depth)`` in the oracle's ``x * x`` mode --
the colour, the generator's words afterwards, the rays the oracle traced.

Besides the worlds of those helpers there is ``mirrors``: six spheres and a plane, every BRDF a ``SpecularBRDF`` with a uniform
pigment below 1, inside one large emissive sphere.  No ``sin`` / ``cos`` (no diffuse bounce) and no ``atan2`` / ``acos`` (no
pigment reads (u, v)) is ever evaluated there, so the device and the oracle agree bit for bit, at every depth.

Computed once per process and shared; nothing here is modified by a test."""
import numpy as np

from pytracer_amd import abi, flatten
from pytracer_amd import hostmodel as hm

from . import ray_batches as B
from . import scatter_batches as X
from . import surface_batches as S

S0, Q0 = X.S0, X.Q0
BACKGROUND = (0.25, 0.5, 0.125)
WORLDS = ("demo", "c2", "pigments", "roulette4", "wide300_lights", "mirrors")
MIRRORS_SIZE = (32, 24)
TOL = 1e-5  # tests/test_gpu_parity.py's bar: relative, per channel

_worlds, _records, _expected = {}, {}, {}


def mirrors_world():
    """-> (hostmodel World, camera)"""
    def mirror(r, g, b, er=0.0, eg=0.0, eb=0.0):
        return hm.Material(hm.SpecularBRDF(hm.UniformPigment(hm.Color(r, g, b))), hm.UniformPigment(hm.Color(er, eg, eb)))

    world = hm.World()
    world.add_shape(hm.Sphere(hm.scaling(hm.Vec(40.0, 40.0, 40.0)), mirror(0.3, 0.2, 0.1, 0.9, 0.8, 0.7)))  # the emissive shell
    world.add_shape(hm.Plane(hm.translation(hm.Vec(0.0, 0.0, -1.0)), mirror(0.6, 0.7, 0.8)))
    balls = (((3.0, 0.0, 0.0), 1.0, (0.9, 0.5, 0.4)), ((2.5, 2.1, 0.2), 0.8, (0.4, 0.9, 0.5)), ((2.5, -2.1, -0.1), 0.9, (0.5, 0.4, 0.9)),
             ((4.5, 1.0, 1.6), 0.7, (0.8, 0.8, 0.3)), ((4.5, -1.2, 1.4), 0.6, (0.3, 0.8, 0.8)), ((1.8, 0.6, -0.6), 0.4, (0.95, 0.95, 0.95)))
    for (x, y, z), r, (cr, cg, cb) in balls:
        world.add_shape(hm.Sphere(hm.translation(hm.Vec(x, y, z)) * hm.scaling(hm.Vec(r, r, r)), mirror(cr, cg, cb, 0.0, 0.01, 0.02)))
    return world, hm.PerspectiveCamera(screen_distance=1.0, aspect_ratio=MIRRORS_SIZE[0] / MIRRORS_SIZE[1])


def host_world(name):
    if name == "mirrors":
        return mirrors_world()
    return X.host_world(name) if name in X.WORLDS else S.host_world(name)


def world(name):
    """-> (FlatScene, Camera)"""
    if name == "mirrors":
        if name not in _worlds:
            wd, cam = mirrors_world()
            _worlds[name] = (flatten.flatten_world(wd), flatten.flatten_camera(cam))
        return _worlds[name]
    return X.world(name) if name in X.WORLDS else S.world(name)


def records(orc, name) -> dict:
    """-> {"rays": [n, 8], "rec": RayHits (the oracle's records of those rays), "n_primary": int}"""
    if name in X.WORLDS:
        return X.records(orc, name)
    if name != "mirrors":
        return S.batch(orc, name)
    if name not in _records:
        old = orc.lib().pto_get_sqr_mode()
        orc.set_sqr_mode(orc.SQR_MUL)
        try:
            flat, cam = world(name)
            w, h = MIRRORS_SIZE
            first = np.array([orc.tracer_fire_ray(cam, w, h, col, row) for row in range(h) for col in range(w)])
            rays = np.vstack([first, S.mirror_bounces(first, B.expected(orc, flat, first))])
            rec = B.expected(orc, flat, rays)
            rays.setflags(write=False)
            rec.buffer.setflags(write=False)
            assert rec.hit.all() and len(set(rec.shape_index.tolist())) == flat.n_shapes  # (inside the shell: nothing misses)
            assert set(np.asarray(flat.brdf_kind).tolist()) == {abi.BRDF_SPECULAR}
            _records[name] = {"rays": rays, "rec": rec, "n_primary": first.shape[0]}
        finally:
            orc.set_sqr_mode(old)
    return _records[name]


def streams(n: int, first: int = 0) -> np.ndarray:
    return X.streams(n, first)


def params(num_of_rays, max_depth, limit, background=BACKGROUND) -> abi.Params:
    return abi.make_params(8, 8, abi.RENDERER_PATHTRACER, num_of_rays=num_of_rays, max_depth=max_depth, rr_limit=limit, background=background)


def expected(orc, flat, rays, pcg, num_of_rays, max_depth, limit, depth=0, background=BACKGROUND) -> dict:
    """``oracle.radiance`` per ``[n, 8]`` ray with generator ``pcg[:, i]`` -> {"radiance" [n, 3], "pcg" uint64[2, n], "count" uint64[n]}.
    (The caller sets the oracle's ``x * x`` mode.)"""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = rays.shape[0]
    par = params(num_of_rays, max_depth, limit, background)
    rad, gen, count = np.zeros((n, 3)), np.array(pcg, dtype=np.uint64), np.zeros(n, np.uint64)
    g = orc.Pcg()
    for i in range(n):
        g.st[0], g.st[1] = int(gen[0, i]), int(gen[1, i])
        rad[i], c = orc.radiance(flat, par, g, rays[i], depth)
        gen[0, i], count[i] = g.state, c
    return {"radiance": rad, "pcg": gen, "count": count}


def rows(orc, name, limit_n=1001) -> slice:
    """At most ``limit_n`` rays of the world's batch, across its boundary between primary rays and bounces."""
    r = records(orc, name)
    n = r["rays"].shape[0]
    if n <= limit_n:
        return slice(0, n)
    start = max(0, min(r["n_primary"] - limit_n // 2, n - limit_n))
    return slice(start, start + limit_n)


def batch(orc, name, num_of_rays, max_depth, limit, depth=0) -> dict:
    """-> {"rays": [n, 8], "pcg": uint64[2, n], "first": int, "want": expected(...)} for :func:`rows` of the world's batch, ray ``i``
    of the WHOLE batch drawing from ``PCG(S0, Q0 + i)``."""
    key = (name, num_of_rays, max_depth, limit, depth)
    if key not in _expected:
        old = orc.lib().pto_get_sqr_mode()
        orc.set_sqr_mode(orc.SQR_MUL)
        try:
            k = rows(orc, name)
            rays = records(orc, name)["rays"][k]
            pcg = streams(rays.shape[0], k.start)
            want = expected(orc, world(name)[0], rays, pcg, num_of_rays, max_depth, limit, depth)
            for a in [pcg] + list(want.values()):
                a.setflags(write=False)
            _expected[key] = {"rays": rays, "pcg": pcg, "first": k.start, "want": want}
        finally:
            orc.set_sqr_mode(old)
    return _expected[key]


def outliers(got, want, tol=TOL):
    """-> (bool [n]: the ray's radiance is beyond ``tol`` in some channel, or its count or its final state differs; worst relative
    error)."""
    from . import util

    err = util.rel_err(np.asarray(got.radiance), want["radiance"])
    bad = (err > tol).any(axis=1) | ~np.isfinite(np.asarray(got.radiance)).all(axis=1)
    bad |= np.asarray(got.n_rays) != want["count"]
    bad |= np.asarray(got.pcg[0]) != want["pcg"][0]
    return bad, float(err.max()) if err.size else 0.0
