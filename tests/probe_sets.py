"""Probe points, directions and expected SH coefficients for the probe-query tests (tests/test_sh_host.py, tests/test_gpu_sh.py).

Worlds: ``demo``, ``c2``, ``pigments`` and ``mirrors`` of tests/radiance_batches.py.  Probe points per world (:func:`points`): five in
free space -- on a primary ray of the world's frame, between the camera and the ray's first hit -- one inside a sphere, one far
outside the scene, where a ray meets the background or, at best, an unbounded plane or the shell around the world.  Probe ``i`` has the stream number ``SEQ0 + STRIDE * i``.

The direction ``D(g)`` of include/ptrace_sh.h restated with ``math.sqrt`` / ``math.sin`` / ``math.cos`` (:func:`direction`), and the
projection composed in Python from the oracle as it stands, in its ``x * x`` mode (:func:`compose`), per sample ``k`` of a probe:

* ``oracle.Pcg(init_state, (seq + k) mod 2^64)``, two ``random_float`` draws, ``D``;
* ``oracle.radiance(flat, params, g, ray8(x, d), depth0)`` -- ``tmin`` 1e-5, ``tmax`` inf: the colour and the rays the oracle traced;

then ``c[j][ch] = ((((0 + Y_j(d_0) L_0[ch]) + Y_j(d_1) L_1[ch]) + ...) * ((4.0 * pi) * (1.0 / K))`` in numpy's fp64, one product and one
addition per sample (:func:`project`), and the counts' sum.

Computed once per process and shared; nothing here is modified by a test."""
import math

import numpy as np

from pytracer_amd import rays as rb

from . import radiance_batches as R

WORLDS = ("demo", "c2", "pigments", "mirrors")
S0 = 45
SEQ0, STRIDE = 54, 977  # (a stride beyond every K of the tests: the probes' streams are disjoint)
BACKGROUND = R.BACKGROUND
TOL = R.TOL
MAX_OUTLIERS = 1
MASK = 2 ** 64 - 1
EPS = 2.0 ** -52
ORACLE_CASES = ((70, 1, 3, 2), (16, 2, 2, 1))  # (K, num_of_rays, max_depth, limit), at depth0 = 1
FAR = (1.0e3, -2.0e3, 1.5e3)

# the furnace: a unit sphere seen from inside, uniform emission and diffuse albedo below 1, no roulette
FURNACE_LE, FURNACE_RHO = (0.7, 0.5, 1.25), (0.5, 0.25, 0.8)
FURNACE_K, FURNACE_D, FURNACE_DEPTH = 4096, 3, 1
FURNACE_POINTS = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.5), (-0.6, 0.1, 0.05))

_points, _expected, _furnace = {}, {}, {}


def points(orc, name) -> np.ndarray:
    """``[7, 3]``: five points in free space, one inside a sphere, one far outside."""
    if name not in _points:
        from pytracer_amd import abi

        flat = R.world(name)[0]
        b = R.records(orc, name)
        rays, rec, n_primary = b["rays"], b["rec"], b["n_primary"]
        hit = np.flatnonzero(np.asarray(rec.hit)[:n_primary])
        rows = hit[np.linspace(0, hit.size - 1, 5).astype(np.int64)]
        out = []
        for row, frac in zip(rows, (0.5, 0.25, 0.75, 0.9, 0.6)):
            out.append(rays[row, 0:3] + rays[row, 3:6] * (float(rec.t[row]) * frac))
        spheres = [s for s in range(flat.n_shapes) if flat.kind[s] == abi.SHAPE_SPHERE]
        s = min(spheres, key=lambda i: abs(float(flat.m[0, i])))  # the smallest one (by its x scale)
        m = np.asarray(flat.m[:, s]).reshape(3, 4)
        out.append(m[:, 3] + 0.3 * m[:, 0])  # the image of (0.3, 0, 0): inside
        out.append(np.array(FAR))
        pts = np.array(out)
        pts.setflags(write=False)
        _points[name] = pts
    return _points[name]


def many_points(orc, name, n: int) -> np.ndarray:
    """``[n, 3]``: the world's seven points again and again, each round shifted a little further."""
    base = points(orc, name)
    return np.array([base[i % 7] + 0.01 * (i // 7) * np.array([1.0, -1.0, 0.5]) for i in range(n)]).reshape(n, 3)


def seqs(n: int, first: int = SEQ0) -> np.ndarray:
    return rb.stream_numbers([first + STRIDE * i for i in range(n)])


def direction(u1: float, u2: float):
    """``D`` of include/ptrace_sh.h from its two draws, with libm"""
    z = 1.0 - 2.0 * u1
    r = math.sqrt(1.0 - z * z)
    ph = (2.0 * math.pi) * u2
    return (r * math.cos(ph), r * math.sin(ph), z)


def draws(orc, init_state, seq, K):
    """-> ``[n, K, 2]``: ``u1, u2`` of every sample, from ``oracle.Pcg``"""
    out = np.zeros((len(seq), K, 2))
    for i, q in enumerate(seq):
        for k in range(K):
            g = orc.Pcg(int(init_state) & MASK, (int(q) + k) & MASK)
            out[i, k] = (g.random_float(), g.random_float())
    return out


def directions_np(u) -> np.ndarray:
    """``[..., 2]`` draws -> ``[..., 3]``: ``D`` in numpy, operation for operation"""
    u = np.asarray(u, dtype=np.float64)
    z = 1.0 - 2.0 * u[..., 0]
    r = np.sqrt(1.0 - z * z)
    ph = (2.0 * math.pi) * u[..., 1]
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], axis=-1)


def project(dirs, samples, reverse: bool = False) -> np.ndarray:
    """``dirs`` and ``samples`` ``[n, K, 3]`` -> ``[n, 9, 3]``: the projection of include/ptrace_sh.h, one product and one addition
    per sample in ``k`` order (``reverse``: from the last sample to the first -- what a wrong order would give)."""
    dirs, samples = np.asarray(dirs, dtype=np.float64), np.asarray(samples, dtype=np.float64)
    n, K = samples.shape[:2]
    y = rb.sh_basis(dirs)  # [n, K, 9]
    acc = np.zeros((n, 9, 3))
    for k in (range(K - 1, -1, -1) if reverse else range(K)):
        acc = acc + y[:, k, :, None] * samples[:, k, None, :]
    return acc * ((4.0 * math.pi) * (1.0 / K))


def bar(dirs, samples, tol=TOL) -> np.ndarray:
    """``[n, 9, 3]``: ``tol * (4 pi / K) * sum_k |Y_j(d_k)| |L_k[ch]|`` -- relative to the sum of magnitudes, because a coefficient
    may cancel to near zero"""
    K = samples.shape[1]
    y = np.abs(rb.sh_basis(dirs))
    return tol * (4.0 * math.pi / K) * np.einsum("nkj,nkc->njc", y, np.abs(np.asarray(samples)))


def compose(orc, flat, pts, seq, K, num_of_rays, max_depth, limit, depth0=1, init_state=S0, background=BACKGROUND, nudge: bool = False) -> dict:
    """-> {"dirs" [n, K, 3], "samples" [n, K, 3], "sample_counts" uint64 [n, K], "coefficients" [n, 9, 3], "count" uint64 [n], "bar"
    [n, 9, 3]} (the caller sets the oracle's ``x * x`` mode).  ``nudge``: every component of every direction one ``nextafter``
    up -- what another sin / cos might give."""
    n = len(pts)
    par = R.params(num_of_rays, max_depth, limit, background)
    dirs, samples, counts = np.zeros((n, K, 3)), np.zeros((n, K, 3)), np.zeros((n, K), np.uint64)
    for i in range(n):
        for k in range(K):
            g = orc.Pcg(int(init_state) & MASK, (int(seq[i]) + k) & MASK)
            u1, u2 = g.random_float(), g.random_float()
            d = np.array(direction(u1, u2))
            if nudge:
                d = np.nextafter(d, np.inf)
            dirs[i, k] = d
            samples[i, k], counts[i, k] = orc.radiance(flat, par, g, orc.ray8(pts[i], d), depth0)
    with np.errstate(over="ignore"):
        count = counts.sum(axis=1, dtype=np.uint64)
    return {"dirs": dirs, "samples": samples, "sample_counts": counts, "coefficients": project(dirs, samples), "count": count,
            "bar": bar(dirs, samples)}


def expected(orc, name, K, num_of_rays, max_depth, limit, depth0=1, nudge: bool = False) -> dict:
    """:func:`compose` for the world's seven probes, cached."""
    key = (name, K, num_of_rays, max_depth, limit, depth0, nudge)
    if key not in _expected:
        old = orc.lib().pto_get_sqr_mode()
        orc.set_sqr_mode(orc.SQR_MUL)
        try:
            pts = points(orc, name)
            want = compose(orc, R.world(name)[0], pts, seqs(len(pts)), K, num_of_rays, max_depth, limit, depth0, nudge=nudge)
            for a in want.values():
                a.setflags(write=False)
            _expected[key] = want
        finally:
            orc.set_sqr_mode(old)
    return _expected[key]


def outliers(coefficients, count, want):
    """-> (bool [n]: the probe's count differs, or some coefficient is not finite or differs by more than the bar; the worst
    |difference| / bar, where the bar is positive)."""
    c = np.asarray(coefficients, dtype=np.float64)
    diff = np.abs(c - want["coefficients"])
    bad = (~(diff <= want["bar"])).any(axis=(1, 2)) | ~np.isfinite(c).all(axis=(1, 2))
    bad |= np.asarray(count).reshape(-1) != want["count"]
    pos = want["bar"] > 0
    worst = float(np.max(diff[pos] / want["bar"][pos])) if pos.any() else 0.0
    return bad, worst


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the furnace -------------------------------------------------------------------------------------------------------------------
def furnace_world():
    from pytracer_amd import hostmodel as hm

    world = hm.World()
    world.add_shape(hm.Sphere(hm.Transformation(), hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(*FURNACE_RHO))),
                                                                hm.UniformPigment(hm.Color(*FURNACE_LE)))))
    return world


def furnace_radiance(max_depth=FURNACE_D, depth0=FURNACE_DEPTH) -> np.ndarray:
    """``Le * sum_{d = 0}^{max_depth - depth0} rho^d`` per channel: what every ray inside the furnace brings back"""
    return np.array([e * sum(r ** d for d in range(max_depth - depth0 + 1)) for e, r in zip(FURNACE_LE, FURNACE_RHO)])


def furnace_expected(orc) -> dict:
    """:func:`compose` for ``FURNACE_POINTS`` at ``FURNACE_K`` samples, no roulette, cached."""
    if "want" not in _furnace:
        from pytracer_amd import flatten

        old = orc.lib().pto_get_sqr_mode()
        orc.set_sqr_mode(orc.SQR_MUL)
        try:
            pts = np.array(FURNACE_POINTS)
            _furnace["want"] = compose(orc, flatten.flatten_world(furnace_world()), pts, seqs(len(pts)), FURNACE_K, 1, FURNACE_D,
                                       FURNACE_D + 5, FURNACE_DEPTH)
        finally:
            orc.set_sqr_mode(old)
    return _furnace["want"]


def furnace_bounds(coefficients, K=FURNACE_K):
    """The two derived bounds of the furnace on ``[n, 9, 3]`` coefficients -> (band 0's relative error [n, 3], its bound;
    |c_j| / L for j >= 1 [n, 8, 3], its bound).

    Band 0: every sample brings the same L, so ``c_0 = Y0 L K (4 pi / K)`` but for the roundings of the K additions; the check is
    ``|Y0 c_0 - L| <= 1e-13 L`` (the summation's own worst case is ``2 K eps``, 1.8e-12 at K = 4096: the check asks for less).
    Bands 1, 2: the estimator's standard deviation is ``L sqrt(4 pi / K)`` (``E[Y_j^2] = 1 / 4 pi`` under the uniform pdf): six
    sigma."""
    L = furnace_radiance()
    c = np.asarray(coefficients)
    rel0 = np.abs(rb.SH_K0 * c[:, 0, :] - L) / L
    return rel0, 1e-13, np.abs(c[:, 1:, :]) / L, 6.0 * math.sqrt(4.0 * math.pi / K)


# ---- a band-limited field with known coefficients --------------------------------------------------------------------------------------
FIELD_B = (0.3, -0.2, 0.15, -0.35, 0.1, 0.05)  # the terms in x, y, x y, y z, x z, x^2 - y^2 beside 1 + 0.5 z + 0.25 (3 z^2 - 1)


def field(d) -> np.ndarray:
    """``L(d) = 1 + 0.5 z + 0.25 (3 z^2 - 1) +`` one term in each of the other six functions, ``[..., 3]`` -> ``[...]``"""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b = FIELD_B
    return 1.0 + 0.5 * z + 0.25 * (3.0 * z * z - 1.0) + b[0] * x + b[1] * y + b[2] * x * y + b[3] * y * z + b[4] * x * z + b[5] * (x * x - y * y)


def field_coefficients() -> np.ndarray:
    """``[9]``: the field's exact SH coefficients (each polynomial term is one basis function over its constant)"""
    b = FIELD_B
    return np.array([1.0 / rb.SH_K0, b[1] / rb.SH_K1, 0.5 / rb.SH_K1, b[0] / rb.SH_K1, b[2] / rb.SH_K2, b[3] / rb.SH_K2, 0.25 / rb.SH_K3,
                     b[4] / rb.SH_K2, b[5] / rb.SH_K4])


def field_hemisphere(n) -> np.ndarray:
    """``(1 / pi) *`` the integral of ``L cos`` over the hemisphere around the unit vector ``n``, in closed form: the cosine lobe
    scales band 0 by 1, band 1 by 2 / 3 and band 2 by 1 / 4."""
    n = np.asarray(n, dtype=np.float64)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    b = FIELD_B
    return (1.0 + (2.0 / 3.0) * (0.5 * z + b[0] * x + b[1] * y)
            + 0.25 * (0.25 * (3.0 * z * z - 1.0) + b[2] * x * y + b[3] * y * z + b[4] * x * z + b[5] * (x * x - y * y)))


def hemisphere_quadrature(fn, n, n_mu: int = 64, n_phi: int = 64) -> float:
    """``(1 / pi) *`` the integral of ``fn(d) (d . n)`` over the hemisphere around the unit vector ``n``: Gauss-Legendre in
    ``mu = d . n`` over [0, 1], the midpoint rule in the azimuth (exact for the trigonometric polynomials of a band-limited
    field)."""
    n = np.asarray(n, dtype=np.float64)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(n, a)
    e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    x, w = np.polynomial.legendre.leggauss(n_mu)
    mu, wmu = 0.5 * (x + 1.0), 0.5 * w
    phi = (np.arange(n_phi) + 0.5) * (2.0 * math.pi / n_phi)
    s = np.sqrt(1.0 - mu * mu)
    d = (s[:, None, None] * (np.cos(phi)[None, :, None] * e1 + np.sin(phi)[None, :, None] * e2) + mu[:, None, None] * n)
    vals = fn(d) * mu[:, None]
    return float((vals * wmu[:, None]).sum() * (2.0 * math.pi / n_phi) / math.pi)
