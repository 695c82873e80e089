"""Worlds and rays AIMED at the spheres' true rims, surfaces and insides, with what the CPU oracle answers for them
(tests/test_aimed_rays.py proves the aim on the CPU, tests/test_gpu_aimed_rays.py sends the rays through the device).

The scattered-ray query (csrc/pt_query.h: world_query_lanes) visits only what a conservative fp32 ball filter, the 8- and
64-ball hierarchy or the uniform-grid walk lets through; its margins (csrc/pt_scene_build.h) can only be wrong for a ray
that passes a sphere within rounding.  So every ray here is built from a sphere's own transform: ``FlatScene.m`` is
``[12, n]`` (planar), a shape's 3x4 block is ``m[:, i].reshape(3, 4)`` = ``L | T``.  With a unit vector ``u`` of object
space, ``p = L u + T`` lies ON the surface for any affine transform, ``L w`` with ``w`` perpendicular to ``u`` is tangent
there, and ``inv(L)^T u`` is the outward normal direction.

Ray classes (``cls = i % 5``), ``size = |L u|``:
  0  graze from nearby: through ``p + eps n`` along a unit tangent ``d``, from ``size * U(1, 10)`` back; ``eps = +-size 10^U(-12, -4)``
  1  graze from far: the same with ``eps = +-size 10^U(-9, -4)`` from ``10^U(1, 5) x span`` back (``span``: the world's
     largest |coordinate|; ``grid_far_eo`` is 100 x that coordinate, so the distances straddle it)
  2  from the surface: the origin is ``p`` moved to the fp64 lattice point nearest the surface among its neighbours (a plain
     ``L u + T`` is a few ulp of |T| off, which for a small sphere far from the origin is not "on" it); any direction;
     tmin one of 0, 1e-5, 1e-3
  3  from inside: the origin is ``L (rho u) + T`` with rho one of 0, 0.5, 1 - 1e-9; any direction
  4  axis-aligned graze: direction ``+-e_a``, past the ellipsoid's extreme point along another axis ``b``
     (``u* = L^T b / |L^T b|``: the tangent plane there is perpendicular to ``b``), off it by ``eps b``
Every direction is scaled by ``10^U(-3, 3)``; tmin 1e-5 unless stated, tmax inf.

Everything is deterministic from ``hostmodel.PCG`` (the worlds) and ``np.random.default_rng(seed)`` (the rays).  Expected
values come from the CPU oracle in its ``x * x`` mode, as ``ray_batches.expected`` does."""
import numpy as np

from pytracer_amd import abi, flatten
from pytracer_amd import hostmodel as hm

from . import ray_batches as B

N_RAYS = 1280
CLASSES = ("graze near", "graze far", "from the surface", "from inside", "axis-aligned graze")

# name -> (spheres, [(centre, half extent), ...] clusters, (rmin, rmax) log-uniform, share of sheared spheres)
_O = (0.0, 0.0, 0.0)
WORLDS = {
    "cube40": (40, [(_O, (10.0, 10.0, 10.0))], (0.05, 2.0), 0.0),       # the plain filter
    "cube300": (300, [(_O, (10.0, 10.0, 10.0))], (0.02, 1.0), 0.0),     # the ball hierarchy
    "cube1500": (1500, [(_O, (10.0, 10.0, 10.0))], (0.02, 0.5), 0.0),   # the grid
    "slab1500": (1500, [(_O, (10.0, 10.0, 0.05))], (0.02, 0.3), 0.0),   # a grid one or two cells thick
    "line1500": (1500, [(_O, (30.0, 0.05, 0.05))], (0.02, 0.2), 0.0),   # 64 x 1 x 1-like grids, crowded cells
    "offset1500": (1500, [((3000.0, -2000.0, 1000.0), (5.0, 5.0, 5.0))], (0.02, 0.3), 0.0),  # cmax >> extent
    "twin1500": (1500, [((-40.0, 0.0, 0.0), (3.0, 3.0, 3.0)), ((40.0, 5.0, -3.0), (3.0, 3.0, 3.0))], (0.02, 0.3), 0.0),  # long empty walks
    "shear300": (300, [(_O, (10.0, 10.0, 10.0))], (0.05, 1.0), 0.7),
    "shear1500": (1500, [(_O, (10.0, 10.0, 10.0))], (0.02, 0.4), 0.7),
}
SEEDS = {name: 100 + i for i, name in enumerate(WORLDS)}
EXACT_WORLDS = ("cube40", "shear300", "offset1500")  # the exact test shape by shape: a probe call per target
EXACT_TARGETS = 64

_worlds, _batches, _exact = {}, {}, {}


def world(name) -> abi.FlatScene:
    """Spheres plus one plane below them, no dome."""
    if name in _worlds:
        return _worlds[name]
    n, clusters, (rmin, rmax), sheared = WORLDS[name]
    g = hm.PCG(1000 + SEEDS[name], 7)
    r = g.random_float
    V = hm.Vec
    mat = hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(0.5, 0.5, 0.5))), hm.UniformPigment(hm.BLACK))
    w = hm.World()
    for i in range(n):
        (cx, cy, cz), (hx, hy, hz) = clusters[i % len(clusters)]
        rad = rmin * (rmax / rmin) ** r()
        t = hm.translation(V(cx + hx * 2.0 * (r() - 0.5), cy + hy * 2.0 * (r() - 0.5), cz + hz * 2.0 * (r() - 0.5)))
        if r() < sheared:
            a, b, c, d = r(), r(), r(), r()
            T = (t * hm.scaling(V(rad * (0.3 + 2 * a), rad, rad * (0.3 + 2 * b))) * hm.rotation_z(360 * r()) * hm.rotation_x(360 * r())
                 * hm.scaling(V(1.0, 0.2 + 3 * c, 0.2 + 3 * d)))
        else:
            T = t * hm.scaling(V(rad, rad, rad))
        w.add_shape(hm.Sphere(T, mat))
    floor = min(c[2] - h[2] for c, h in clusters) - 4.0 * rmax
    cx, cy = clusters[0][0][0], clusters[0][0][1]
    w.add_shape(hm.Plane(hm.translation(V(cx, cy, floor)), mat))
    _worlds[name] = flatten.flatten_world(w)
    return _worlds[name]


def sphere_indices(flat) -> np.ndarray:
    return np.nonzero(np.asarray(flat.kind) == abi.SHAPE_SPHERE)[0]


def sphere_transforms(flat):
    """-> (L [ns, 3, 3], T [ns, 3]) of the spheres (planes are never aimed at), in ``sphere_indices`` order."""
    m = np.asarray(flat.m, dtype=np.float64).T.reshape(-1, 3, 4)[sphere_indices(flat)]
    return np.ascontiguousarray(m[:, :, :3]), np.ascontiguousarray(m[:, :, 3])


def span_of(flat) -> float:
    """The world's largest |coordinate| over its spheres."""
    L, T = sphere_transforms(flat)
    return float(np.max(np.abs(T) + np.sqrt((L * L).sum(axis=2))))


def _unit(rng):
    u = rng.normal(size=3)
    return u / np.linalg.norm(u)


def inv3(L):
    """inv of a 3x3 in long double (numpy's linalg has no long double): the adjugate."""
    a = L.astype(np.longdouble)
    c = np.empty((3, 3), dtype=np.longdouble)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[j, i] = a[i1, j1] * a[i2, j2] - a[i1, j2] * a[i2, j1]
    det = a[0, 0] * c[0, 0] + a[0, 1] * c[1, 0] + a[0, 2] * c[2, 0]
    return c / det


def object_point(L, T, o):
    """``inv(L) (o - T)`` in long double: of length 1 on the true surface."""
    return inv3(L) @ (np.asarray(o, dtype=np.float64).astype(np.longdouble) - T.astype(np.longdouble))


_AB = np.array([(a, b) for a in range(-2, 3) for b in range(-64, 65)], dtype=np.float64)


def on_surface(L, T, p) -> np.ndarray:
    """``p`` (fp64, a few ulp of |T| off the surface) -> an fp64 lattice point beside it (within 2 ulp along the coordinate
    the distance to the surface depends on most, 64 ulp along the other two) that lies as near the true surface as such
    points do, measured in long double.  For each step along the two coarser coordinates the third comes from the
    linearised distance; the candidates are then measured exactly."""
    p = np.asarray(p, dtype=np.float64)
    ulp = np.spacing(np.abs(p))
    Li, Tl = inv3(L), T.astype(np.longdouble)

    def off(points):
        q = (points.astype(np.longdouble) - Tl[None, :]) @ Li.T
        return np.sqrt((q * q).sum(axis=1)) - np.longdouble(1.0)

    q0 = object_point(L, T, p)
    g = (Li.T @ (q0 / np.sqrt((q0 * q0).sum()))) * ulp  # change of |q| per ulp along each coordinate
    first, second, third = np.argsort(-np.abs(g.astype(np.float64)))
    lin = off(p[None, :])[0] + _AB[:, 0] * g[first] + _AB[:, 1] * g[second]
    steps = np.zeros((len(_AB), 3))
    steps[:, first], steps[:, second] = _AB[:, 0], _AB[:, 1]
    if g[third] != 0:
        steps[:, third] = np.clip(np.rint((-lin / g[third]).astype(np.float64)), -64, 64)
    cand = p[None, :] + steps * ulp[None, :]  # exact: small multiples of an ulp
    return cand[int(np.argmin(np.abs(off(cand))))]


def aimed(flat, n, seed, span, targets=None):
    """-> (rays [n, 8], target [n] (World.shapes index), cls [n]).  ``targets``: aim at that many distinct spheres only."""
    rng = np.random.default_rng(seed)
    L, T = sphere_transforms(flat)
    idx = sphere_indices(flat)
    pool = np.arange(len(idx))
    if targets is not None and targets < len(pool):
        pool = np.sort(rng.choice(pool, size=targets, replace=False))
    rays, target, cls = np.zeros((n, 8)), np.zeros(n, dtype=np.int64), np.arange(n) % 5
    for i in range(n):
        c = int(cls[i])
        k = int(pool[rng.integers(len(pool))])
        Lk, Tk = L[k], T[k]
        u = _unit(rng)
        tmin = 1e-5
        if c in (0, 1):
            w = np.cross(u, rng.normal(size=3))
            w /= np.linalg.norm(w)
            d = Lk @ w
            d /= np.linalg.norm(d)
            nrm = np.linalg.solve(Lk.T, u)
            nrm /= np.linalg.norm(nrm)
            size = np.linalg.norm(Lk @ u)
            eps = rng.choice([-1.0, 1.0]) * size * 10.0 ** (rng.uniform(-12, -4) if c == 0 else rng.uniform(-9, -4))
            back = size * rng.uniform(1, 10) if c == 0 else span * 10.0 ** rng.uniform(1, 5)
            o = (Lk @ u + Tk) + eps * nrm - d * back
        elif c == 2:
            o = on_surface(Lk, Tk, Lk @ u + Tk)
            d = rng.normal(size=3)
            tmin = (0.0, 1e-5, 1e-3)[rng.integers(3)]
        elif c == 3:
            rho = (0.0, 0.5, 1.0 - 1e-9)[rng.integers(3)]
            o = Lk @ (rho * u) + Tk
            d = rng.normal(size=3)
        else:
            a = int(rng.integers(3))
            b = (a + 1 + int(rng.integers(2))) % 3
            e_b = np.zeros(3)
            e_b[b] = rng.choice([-1.0, 1.0])
            us = Lk.T @ e_b
            us /= np.linalg.norm(us)
            size = np.linalg.norm(Lk @ us)
            eps = rng.choice([-1.0, 1.0]) * size * 10.0 ** rng.uniform(-12, -4)
            d = np.zeros(3)
            d[a] = rng.choice([-1.0, 1.0])
            o = (Lk @ us + Tk) + eps * e_b - d * (size * rng.uniform(1, 10))
        rays[i, 0:3], rays[i, 3:6] = o, d * 10.0 ** rng.uniform(-3, 3)
        rays[i, 6], rays[i, 7] = tmin, np.inf
        target[i] = idx[k]
    return rays, target, cls


def expected(orc, flat, rays):
    """``oracle.world_intersect`` per ray (tmax honoured) in the ``x * x`` mode -> RayHits; any-hit is ``.hit``."""
    old = orc.lib().pto_get_sqr_mode()
    orc.set_sqr_mode(orc.SQR_MUL)
    try:
        return B.expected(orc, flat, rays)
    finally:
        orc.set_sqr_mode(old)


def expected_of_shape(orc, flat, rays, shape) -> np.ndarray:
    """``oracle.shape_intersect`` of one shape, ``x * x`` mode -> [n, 8]: hit, t, point, the normal normalised as
    World.ray_intersection does (world.py:66-68: the components divided by sqrt(x*x + y*y + z*z))."""
    old = orc.lib().pto_get_sqr_mode()
    orc.set_sqr_mode(orc.SQR_MUL)
    try:
        out = np.zeros((len(rays), 8))
        for i, ray in enumerate(rays):
            o = orc.shape_intersect(flat, int(shape), ray)
            if o is not None:
                out[i, 0], out[i, 1:8] = 1.0, o[:7]
        x, y, z = out[:, 5].copy(), out[:, 6].copy(), out[:, 7].copy()
        hit = out[:, 0] != 0
        norm = np.sqrt(x * x + y * y + z * z)
        with np.errstate(all="ignore"):
            for c, v in ((5, x), (6, y), (7, z)):
                out[:, c] = np.where(hit, v / norm, 0.0)
        return out
    finally:
        orc.set_sqr_mode(old)


def segment_ends(orc, flat, rays, want=None):
    """Every ray the oracle hits at t*, four times: tmax = t*, nextafter(t*, inf), t* (1 - 1e-6), t* (1 + 1e-6).
    -> (rays [4 m, 8] in that order, block after block; index [m] of the rays taken)."""
    want = expected(orc, flat, rays) if want is None else want
    took = np.nonzero(want.hit)[0]
    t = want.t[took]
    out = []
    for tmax in (t, np.nextafter(t, np.inf), t * (1.0 - 1e-6), t * (1.0 + 1e-6)):
        seg = rays[took].copy()
        seg[:, 7] = tmax
        out.append(seg)
    return np.concatenate(out), took


def batch(orc, name) -> dict:
    """The world's 1280 aimed rays, their segment ends and what the oracle answers, computed once per process:
    {"rays", "target", "cls", "want": RayHits, "seg": [4 m, 8], "seg_of": [m], "seg_want": RayHits}"""
    if name not in _batches:
        flat = world(name)
        rays, target, cls = aimed(flat, N_RAYS, SEEDS[name], span_of(flat))
        want = expected(orc, flat, rays)
        seg, took = segment_ends(orc, flat, rays, want)
        _batches[name] = {"rays": rays, "target": target, "cls": cls, "want": want, "seg": seg, "seg_of": took,
                          "seg_want": expected(orc, flat, seg)}
    return _batches[name]


def exact_batch(name):
    """1280 aimed rays at 64 targets (or every sphere, where the world has fewer) for the shape-by-shape test."""
    if name not in _exact:
        flat = world(name)
        _exact[name] = aimed(flat, N_RAYS, SEEDS[name] + 1000, span_of(flat), targets=EXACT_TARGETS)
    return _exact[name]


def describe(rays, cls, bad) -> str:
    """Per class how many rays differ, and the first offender in float.hex."""
    bad = np.asarray(bad, dtype=bool)
    cls = np.asarray(cls)
    counts = ", ".join(f"{CLASSES[c]}: {int(bad[cls == c].sum())}/{int((cls == c).sum())}" for c in range(5))
    first = int(np.argmax(bad)) if bad.any() else -1
    row = " ".join(float(v).hex() for v in rays[first]) if first >= 0 else ""
    return f"{int(bad.sum())} of {bad.size} rays differ ({counts}); first: ray {first} class {int(cls[first]) if first >= 0 else -1}: {row}"
