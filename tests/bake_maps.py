"""Shapes, surface points and expected light maps for the bake-query tests (tests/test_bake_host.py, tests/test_gpu_bake.py).

Worlds: ``demo``, ``c2`` and ``pigments`` of tests/radiance_batches.py, the first three shapes with a ``DiffuseBRDF`` of each (``demo``
has two, both planes; the others' are spheres).

The surface point ``S(shape, u, v, side)`` of include/ptrace_bake.h restated with ``math.sin`` / ``math.cos``, ``oracle.xform`` and
the ``x * x`` norm (:func:`surface_point`), and the bound a device result is held to (:func:`point_bounds`).

The bake's samples restated from the oracle as it stands, in its ``x * x`` mode (:func:`compose`), per texel ``t`` (global index)
and sample ``k``: ``oracle.Pcg(init_state, init_seq + t K + k)``, two ``random_float`` draws with jitter, ``u = (col + ju) * (1.0 /
W)`` (IEEE ``+``, ``*`` and ``/``: exact on the host), the restated surface point, ``oracle.scatter(DIFFUSE, ...)``,
``oracle.radiance(..., depth0)``; then the ordered mean of tests/gather_batches.py.

Computed once per process and shared; nothing here is modified by a test."""
import math

import numpy as np

from pytracer_amd import abi

from . import gather_batches as G
from . import radiance_batches as R

WORLDS = ("demo", "c2", "pigments")
S0, Q0 = 45, 54
BACKGROUND = R.BACKGROUND
TOL = R.TOL
MASK = 2 ** 64 - 1
EPS = 2.0 ** -52
ORACLE_CASES = ((4, 1, 3, 2), (3, 2, 2, 1))  # (K, num_of_rays, max_depth, limit) on 7 x 5 maps
MAP_W, MAP_H = 7, 5

_expected = {}


def diffuse_shapes(name) -> list:
    """The first three ``World.shapes`` indices of the world whose BRDF is a ``DiffuseBRDF``."""
    flat = R.world(name)[0]
    return [i for i in range(flat.n_shapes) if flat.brdf_kind[i] == abi.BRDF_DIFFUSE][:3]


def all_shapes() -> list:
    return [(name, s) for name in WORLDS for s in diffuse_shapes(name)]


def local_point(kind, u, v, side):
    """-> (p, n_loc) of include/ptrace_bake.h, with libm's sin / cos"""
    if kind == abi.SHAPE_SPHERE:
        th, ph = v * math.pi, (2.0 * math.pi) * u
        p = (math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th))
        return p, (side * p[0], side * p[1], side * p[2])
    return (u, v, 0.0), (0.0, 0.0, float(side))


def surface_point(orc, flat, s, u, v, side=1):
    """-> (point [3], normal [3]): ``T * Point(p)`` and ``(T * Normal(n_loc)).normalize()`` through ``oracle.xform`` and the
    ``x * x`` norm"""
    p, nl = local_point(int(flat.kind[s]), float(u), float(v), side)
    point = orc.xform(flat.m[:, s], 0, p)
    n = orc.xform(flat.invm[:, s], 2, nl)
    norm = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    return point, np.array([n[0] / norm, n[1] / norm, n[2] / norm])


def surface_points(orc, flat, s, uv, side=1):
    """``uv`` [..., 2] -> (points [..., 3], normals [..., 3]); ``s`` and ``side``: one value, or one per record"""
    uv = np.asarray(uv, dtype=np.float64)
    lead = uv.shape[:-1]
    flat_uv = uv.reshape(-1, 2)
    ss = np.broadcast_to(np.asarray(s), lead).reshape(-1)
    sides = np.broadcast_to(np.asarray(side), lead).reshape(-1)
    pts, nrm = np.zeros((flat_uv.shape[0], 3)), np.zeros((flat_uv.shape[0], 3))
    for i, (u, v) in enumerate(flat_uv):
        pts[i], nrm[i] = surface_point(orc, flat, int(ss[i]), u, v, int(sides[i]))
    return pts.reshape(lead + (3,)), nrm.reshape(lead + (3,))


def point_bounds(flat, s, u, v, side=1):
    """-> (bound on |point error| [3], bound on |normal error| [3]) between two evaluations of the definition that differ in
    their ``sin`` / ``cos`` (ocml and glibc: within about 2 ulp each).

    Point, per component i: ``64 eps (sum_j |M_ij| |p_j| + |M_i3|)`` -- 2 ulp per function value, one product, three
    multiply-adds: about 16 eps of the sum of magnitudes; 64 leaves a factor of about 4.

    Normal: the unnormalised ``n' = invM^T n_loc`` has the same kind of bound ``a_i = 64 eps sum_j |invM_ji| |n_loc_j|``; dividing by
    ``|n'|`` (whose own error is at most ``|a|_2``) gives, to first order, ``(a_i + |n_i| |a|_2) / |n'|`` for the unit normal's
    component i (the division's and the square root's half ulps are inside the factor 4)."""
    p, nl = local_point(int(flat.kind[s]), float(u), float(v), side)
    M, IM = np.asarray(flat.m[:, s]).reshape(3, 4), np.asarray(flat.invm[:, s]).reshape(3, 4)
    pb = 64.0 * EPS * (np.abs(M[:, :3]) @ np.abs(np.array(p)) + np.abs(M[:, 3]))
    a = 64.0 * EPS * (np.abs(IM[:, :3]).T @ np.abs(np.array(nl)))
    nprime = IM[:, :3].T @ np.array(nl)
    norm = float(np.sqrt(nprime @ nprime))
    nb = (a + np.abs(nprime / norm) * float(np.sqrt(a @ a))) / norm
    return pb, nb


def window_texels(W, H, window=None):
    """-> (cols [n], rows [n], t [n]) of the window's texels in its own row-major order; ``t`` the GLOBAL index"""
    col0, row0, w, h = (0, 0, W, H) if window is None else window
    rows, cols = np.divmod(np.arange(w * h), w)
    rows, cols = rows + row0, cols + col0
    return cols, rows, rows * W + cols


def sample_uv(orc, W, H, K, jitter=True, window=None, init_state=S0, init_seq=Q0):
    """-> (uv [n, K, 2], seq list[n][K] of Python ints): every sample's ``(u, v)`` as the bake forms it, from ``oracle.Pcg`` draws"""
    cols, rows, t = window_texels(W, H, window)
    n = cols.size
    uv, seqs = np.zeros((n, K, 2)), []
    for i in range(n):
        seqs.append([(init_seq + int(t[i]) * K + k) & MASK for k in range(K)])
        for k in range(K):
            ju = jv = 0.5
            if jitter:
                g = orc.Pcg(init_state & MASK, seqs[i][k])
                ju, jv = g.random_float(), g.random_float()
            uv[i, k] = ((int(cols[i]) + ju) * (1.0 / W), (int(rows[i]) + jv) * (1.0 / H))
    return uv, seqs


def compose(orc, flat, s, W, H, K, num_of_rays, max_depth, limit, side=1, jitter=True, window=None, depth0=1, init_state=S0,
            init_seq=Q0, background=BACKGROUND) -> dict:
    """The bake from the oracle's parts -> {"samples" [n, K, 3], "sample_counts" [n, K], "radiance" [n, 3], "count" uint64 [n], "uv"}
    (the caller sets the oracle's ``x * x`` mode)."""
    uv, seqs = sample_uv(orc, W, H, K, jitter, window, init_state, init_seq)
    n = uv.shape[0]
    par = R.params(num_of_rays, max_depth, limit, background)
    samples, counts = np.zeros((n, K, 3)), np.zeros((n, K), np.uint64)
    for i in range(n):
        for k in range(K):
            g = orc.Pcg(init_state & MASK, seqs[i][k])
            if jitter:
                g.random_float(), g.random_float()
            p, nrm = surface_point(orc, flat, s, uv[i, k, 0], uv[i, k, 1], side)
            ray = orc.scatter(abi.BRDF_DIFFUSE, g, (0.0, 0.0, 1.0), p, nrm, depth0)
            samples[i, k], counts[i, k] = orc.radiance(flat, par, g, ray, depth0)
    with np.errstate(over="ignore"):
        count = counts.sum(axis=1, dtype=np.uint64)
    return {"samples": samples, "sample_counts": counts, "radiance": G.ordered_mean(samples), "count": count, "uv": uv}


def expected(orc, name, s, K, num_of_rays, max_depth, limit, W=MAP_W, H=MAP_H, **kw) -> dict:
    """:func:`compose` for a whole map of a world's shape, cached."""
    key = (name, s, K, num_of_rays, max_depth, limit, W, H, tuple(sorted(kw.items())))
    if key not in _expected:
        old = orc.lib().pto_get_sqr_mode()
        orc.set_sqr_mode(orc.SQR_MUL)
        try:
            want = compose(orc, R.world(name)[0], s, W, H, K, num_of_rays, max_depth, limit, **kw)
            for a in want.values():
                a.setflags(write=False)
            _expected[key] = want
        finally:
            orc.set_sqr_mode(old)
    return _expected[key]


def outliers(got, want, tol=TOL):
    """-> (bool [n]: the texel's radiance is beyond ``tol`` relative in some channel, or not finite, or its count differs; worst
    relative error) for a :class:`pytracer_amd.rays.BakedMap` ``got``"""
    from . import util

    rad = np.asarray(got.radiance).reshape(-1, 3)
    err = util.rel_err(rad, want["radiance"])
    bad = (err > tol).any(axis=1) | ~np.isfinite(rad).all(axis=1)
    bad |= np.asarray(got.n_rays).reshape(-1) != want["count"]
    return bad, float(err.max()) if err.size else 0.0
