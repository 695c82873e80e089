"""Frames of a world in which a shape moves, for the tests of the motion accumulate query (include/ptrace_motion.h): a two-shape hit
frame in numpy, the hostile records of the weighted query's tests laid over it, and motion tables of every kind the interface
names.  Nothing here needs a GPU, and nothing here is modified by a test."""
import numpy as np

from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb

from .test_gpu_temporal import moved as moved_camera
from .test_gpu_weighted import hostile_weights
from .test_temporal_host import cameras, primary_rays
from .test_weighted_host import hostile

NAN, INF = float("nan"), float("inf")
GROUND, SPHERE = 0, 1
TABLES = ("static", "translation", "sheared", "nonfinite", "short")


def two_shape_frame(camera, W, H, cy=0.0):
    """The hit frame of the ground plane z = 0 (shape 0, a normal of length 2 towards the ray's side) and the unit sphere centred at
    (0, ``cy``, 1) (shape 1, an outward normal of length 0.5), seen from ``camera`` through the pixel centres -> (shape [H, W] int32,
    normal [H, W, 3], point [H, W, 3]); a miss has shape -1 and zeros."""
    o, d = primary_rays(camera, W, H)
    centre = np.array([0.0, cy, 1.0])
    with np.errstate(all="ignore"):
        tp = -o[..., 2] / d[..., 2]
        tp = np.where(tp > 0.0, tp, INF)
        oc = o - centre
        a = (d * d).sum(-1)
        b = (oc * d).sum(-1)
        c = (oc * oc).sum(-1) - 1.0
        disc = b * b - a * c
        ts = (-b - np.sqrt(np.where(disc > 0.0, disc, 0.0))) / a
        ts = np.where((disc > 0.0) & (ts > 0.0), ts, INF)
    t = np.minimum(tp, ts)
    hit = np.isfinite(t)
    point = np.where(hit[..., None], o + np.where(hit, t, 0.0)[..., None] * d, 0.0)
    on_sphere = hit & (ts <= tp)
    shape = np.where(on_sphere, SPHERE, GROUND).astype(np.int32)
    shape[~hit] = -1
    up = np.where(d[..., 2:3] < 0.0, 2.0, -2.0) * np.array([0.0, 0.0, 1.0])
    normal = np.where(on_sphere[..., None], 0.5 * (point - centre), up)
    normal = np.where(hit[..., None], normal, 0.0)
    point[..., 2] = np.where(hit & ~on_sphere, 0.0, point[..., 2])
    return shape, normal, point


def record(transformation):
    """A row of the motion table from a host-model ``Transformation`` T that takes this frame's points to the previous frame's:
    rows 0..2 of ``T.m``, then the transpose of the linear part of ``T.invm``, then three values that are never read."""
    m, inv = transformation.m, transformation.invm
    return [m[i][j] for i in range(3) for j in range(4)] + [inv[j][i] for i in range(3) for j in range(3)] + [NAN, -INF, 1e300]


def shear(k):
    """x' = x + k y, with its inverse."""
    m, inv = hm._identity(), hm._identity()
    m[0][1], inv[0][1] = k, -k
    return hm.Transformation(m, inv)


def table(kind, dy=0.3):
    """-> (moved int32[S], motion float64[S, 24]) of one of ``TABLES``.  The sphere (shape 1) is what moves: by ``dy`` along y since the
    previous frame under "translation" (so the way back is -``dy``), by a rotation with a non-uniform scale and a shear under
    "sheared" (where the ground slides a little too); "static" moves nothing and holds NaN rows that must never be read;
    "nonfinite" has a NaN and an infinity among the entries of a moved row; "short" has ONE row, fewer than the sphere's index."""
    back = hm.translation(hm.Vec(0.0, -dy, 0.0))
    if kind == "static":
        return np.zeros(2, np.int32), np.full((2, 24), NAN)
    if kind == "translation":
        return np.array([0, 1], np.int32), np.array([[NAN] * 24, record(back)])
    if kind == "sheared":
        odd = hm.translation(hm.Vec(0.1, -dy, 0.05)) * hm.rotation_z(7.0) * hm.rotation_x(-3.0) * hm.scaling(hm.Vec(1.1, 0.9, 1.25)) * shear(0.2)
        return np.array([1, 1], np.int32), np.array([record(hm.translation(hm.Vec(0.02, -0.01, 0.0))), record(odd)])
    if kind == "nonfinite":
        rows = np.array([record(hm.translation(hm.Vec(0.01, 0.0, 0.0))), record(back)])
        rows[1, 5], rows[1, 14], rows[0, 3] = NAN, INF, -INF
        return np.array([1, -7], np.int32), rows  # (any non-zero word means moved)
    if kind == "short":
        return np.array([1], np.int32), np.array([record(hm.translation(hm.Vec(0.02, -0.01, 0.0)))])
    raise KeyError(kind)


_frames = {}


def inputs(W, Hh, kind, how, seed, dy=0.3):
    """-> (the camera before, the eleven planes of ``weighted_host`` / ``motion_host`` up to ``prev_count``): the previous frame is the
    two-shape world seen from the camera of ``kind``, the current one the world with the sphere ``dy`` further along y seen from
    that camera moved ``how``; both made hostile (shape indices -1, -2^31, 1000 and 2^31 - 1, normals and points of any kind), with
    hostile history lengths, weights and sample counts.  Computed once per case and shared."""
    key = (W, Hh, kind, how, seed, dy)
    if key not in _frames:
        before = cameras(aspect=W / Hh)[kind]
        rng = np.random.default_rng(seed)
        pcol, pshape, pnormal, ppoint, pcount = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *two_shape_frame(before, W, Hh, 0.0), seed=seed + 1,
                                                        counts=True)
        col, shape, normal, point = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *two_shape_frame(moved_camera(before, how), W, Hh, dy), seed=seed + 2)
        pmoments, samples = hostile_weights(Hh, W, seed + 3)
        _frames[key] = before, (col, samples, shape, normal, point, pcol, pmoments, pshape, pnormal, ppoint, pcount)
    return _frames[key]


def clean_pair(kind, dy, W=48, H=36):
    """Two frames nobody tampered with: the camera of ``kind`` at rest, the sphere at cy = 0 and then at cy = ``dy``, a previous
    history of length 1 whose colour tells the shapes apart -> (camera, the eleven planes, the sphere's pixels in the current frame)."""
    camera = cameras(aspect=W / H)[kind]
    pshape, pnormal, ppoint = two_shape_frame(camera, W, H, 0.0)
    shape, normal, point = two_shape_frame(camera, W, H, dy)
    pcol = np.where((pshape == SPHERE)[..., None], 2.0, 0.5) * np.ones(3)
    col = np.ones((H, W, 3))
    pcount = (pshape >= 0).astype(np.int32)
    lum = rb._luminance(pcol)
    pmoments = np.stack([lum, lum * lum, pcount.astype(np.float64)], axis=-1)
    return camera, (col, None, shape, normal, point, pcol, pmoments, pshape, pnormal, ppoint, pcount), shape == SPHERE
