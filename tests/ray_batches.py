"""Worlds, ray batches and their expected results for the ray-batch tests (tests/test_rays_host.py, tests/test_gpu_rays.py).

Per world three batches: the frame's pixel-centre primary rays; mirror bounces off their hits (``d - 2 (d.n) n`` from the
hit point, tmin 1e-3); visibility segments from the hit points to one light.  Everything expected comes from the CPU oracle
in its ``x * x`` mode (the device multiplies where the reference writes ``x**2``), computed once per process
and shared."""
import ctypes as C

import numpy as np

from pytracer_amd import abi, flatten, rays as rb, scenes

# name -> (frame width, height, the light the visibility segments go to)
WORLDS = {
    "demo": (40, 30, (-30.0, 30.0, 30.0)),
    "c2p": (48, 27, (0.0, 0.0, 10.0)),
    "wide300": (48, 27, (0.0, 0.0, 10.0)),
    "wide1500": (32, 18, (0.0, 0.0, 10.0)),
    # dome-less stress worlds of tests/test_gpu_probes.py: (spheres, seed, coord, rmin, rmax), 384 of its trouble-seeking rays
    "stress40": (0, 0, (0.0, 0.0, 100.0)),
    "stress1500": (0, 0, (0.0, 0.0, 100.0)),
}
FRAME_WORLDS = ("demo", "c2p", "wide300", "wide1500")
_STRESS = {"stress40": (40, 0, 10.0, 0.05, 2.0), "stress1500": (1500, 4, 10.0, 0.02, 0.5)}
BATCHES = ("primary", "bounce", "shadow")

_worlds, _batches = {}, {}


def world(name):
    """-> (FlatScene, Camera or None)"""
    if name not in _worlds:
        w, h, _ = WORLDS[name]
        if name == "demo":
            wd, cam = scenes.demo_world()
            _worlds[name] = (flatten.flatten_world(wd), flatten.flatten_camera(cam))
        elif name in _STRESS:
            from tests.test_gpu_probes import _stress_world

            n, seed, coord, rmin, rmax = _STRESS[name]
            _worlds[name] = (flatten.flatten_world(_stress_world(n, seed, coord, rmin, rmax, dome=False)), None)
        else:
            wd = {"c2p": lambda: scenes.synthetic_world(32, with_plane=True),
                  "wide300": lambda: scenes.synthetic_world(300, with_plane=True, wide=True),
                  "wide1500": lambda: scenes.synthetic_world(1500, with_plane=True, wide=True)}[name]()
            _worlds[name] = (flatten.flatten_world(wd), flatten.flatten_camera(scenes.synthetic_camera(w, h)))
    return _worlds[name]


def _first_rays(orc, name) -> np.ndarray:
    flat, cam = world(name)
    if name in _STRESS:
        from tests.test_gpu_probes import _stress_rays, _stress_world

        n, seed, coord, rmin, rmax = _STRESS[name]
        return _stress_rays(_stress_world(n, seed, coord, rmin, rmax, dome=False), 384, seed, coord)[1]
    w, h, _ = WORLDS[name]
    out = np.empty((w * h, 8))
    for row in range(h):
        for col in range(w):
            out[row * w + col] = orc.tracer_fire_ray(cam, w, h, col, row)
    return out


def expected(orc, flat, rays, channels=rb.RAY_CHANNELS) -> rb.RayHits:
    """``oracle.world_intersect`` for ``[n, 8]`` rays as the planes a closest-hit batch holds (miss: -1, +inf, zeros)."""
    L = orc.lib()
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = rays.shape[0]
    want = rb.RayHits(np.zeros(rb.rays_bytes(n, rb.RAY_CHANNELS), dtype=np.uint8), n, rb.RAY_CHANNELS)
    want.shape_index[:] = -1
    want.t[:] = np.inf
    desc, rec = flat.desc(), np.zeros(10)
    po = rec.ctypes.data_as(C.POINTER(C.c_double))
    t, pt, nrm, uv = want.t, want.point, want.normal, want.uv
    for i in range(n):
        if L.pto_world_intersect(C.byref(desc), rays[i].ctypes.data_as(C.POINTER(C.c_double)), po):
            want.shape_index[i] = int(rec[9])
            t[i], pt[i], nrm[i], uv[i] = rec[0], rec[1:4], rec[4:7], rec[7:9]
    if channels == rb.RAY_CHANNELS:
        return want
    some = rb.RayHits(np.zeros(rb.rays_bytes(n, channels), dtype=np.uint8), n, channels)
    for name, plane in some.planes().items():
        plane[...] = want.planes()[name]
    return some


def expected_visible(orc, flat, points, observer) -> np.ndarray:
    """``oracle.is_point_visible(point, observer)`` per point."""
    return np.array([orc.is_point_visible(flat, p, observer) for p in np.asarray(points, dtype=np.float64)], dtype=bool)


def batches(orc, name) -> dict:
    """-> {"primary" | "bounce" | "shadow": {"rays": [n, 8], "want": RayHits}, "points": [m, 3], "light": (3,), "visible": [m] bool}"""
    if name in _batches:
        return _batches[name]
    old = orc.lib().pto_get_sqr_mode()
    orc.set_sqr_mode(orc.SQR_MUL)
    try:
        flat, _ = world(name)
        light = np.array(WORLDS[name][2])
        first = _first_rays(orc, name)
        w0 = expected(orc, flat, first)
        hit = w0.hit & np.isfinite(w0.point).all(axis=1) & np.isfinite(w0.normal).all(axis=1)
        p, nrm, d = w0.point[hit], w0.normal[hit], first[hit, 3:6]
        dn = d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1] + d[:, 2] * nrm[:, 2]
        bounce = np.empty((p.shape[0], 8))
        bounce[:, 0:3], bounce[:, 3:6] = p, d - 2.0 * dn[:, None] * nrm
        bounce[:, 6], bounce[:, 7] = 1e-3, np.inf
        shadow = np.ascontiguousarray(rb.visibility_rays(p, light).T)
        out = {"points": np.array(p), "light": light, "visible": expected_visible(orc, flat, p, light)}
        for key, rays in (("primary", first), ("bounce", bounce), ("shadow", shadow)):
            out[key] = {"rays": rays, "want": w0 if key == "primary" else expected(orc, flat, rays)}
        _batches[name] = out
        return out
    finally:
        orc.set_sqr_mode(old)


def uv_close(got, want) -> bool:
    """A sphere's (u, v): ocml's atan2 / acos against glibc's, the project's bound (tests/test_gpu_probes.py:65, test_gpu_hits.py)."""
    a, b = np.asarray(got), np.asarray(want)
    return bool(np.all(np.abs(a - b) <= 1e-11 * np.maximum(np.abs(a), np.abs(b)) + 1e-300))
