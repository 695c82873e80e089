"""Rays aimed at the spheres' true rims, surfaces and insides (tests/aimed_rays.py; the aim itself is proven on the CPU by
tests/test_aimed_rays.py) through the device: the exact test shape by shape, the scattered-ray query of libptrace.so
(``lanes_probe``: fp32 ball filter, 8- and 64-ball hierarchy, grid walk) and the ray batches of libptrace_rays.so, against the
CPU oracle in its ``x * x`` mode.  Nine worlds: each structure of the query, flat and elongated grids, a world far from the
origin, two clusters far apart, sheared spheres.

Expected agreement: hit / miss, the shape index, t, point and normal bit for bit (no transcendental function is involved);
a plane's (u, v) bit for bit; a sphere's (u, v) within the project's 1e-11 (``ray_batches.uv_close``).  A conservative
margin that is too small shows as a ray whose winner differs or is missing.  On failure: per class how many rays differ and
the first offender in ``float.hex``."""
import numpy as np
import pytest

from pytracer_amd import abi, rays as rb

from . import aimed_rays as A
from . import ray_batches as B

pytestmark = pytest.mark.gpu
WORLDS = list(A.WORLDS)
PREFIXES = (5, 64 * 3 + 5, 64 * 19 + 5)  # n = 64 k + 5: the last wave holds 5 live rays


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    return device


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o

    o.build()
    o.set_sqr_mode(o.SQR_MUL)
    yield o
    o.set_sqr_mode(o.SQR_POW)


@pytest.fixture(scope="module")
def scene_of(dev):
    """name -> the world's DeviceScene, uploaded once for the module."""
    open_ = {}

    def get(name):
        if name not in open_:
            open_[name] = dev.DeviceScene(A.world(name))
        return open_[name]

    yield get
    for ds in open_.values():
        ds.close()


_full = {}


def _traced(scene_of, orc, name):
    """The world's aimed batch through ``trace_rays`` and ``occluded``, once."""
    if name not in _full:
        planes = rb.ray_planes(A.batch(orc, name)["rays"])
        _full[name] = (scene_of(name).trace_rays(planes), scene_of(name).occluded(planes))
    return _full[name]


def _rows_differ(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    d = a.view(np.uint64) != b.view(np.uint64)
    return d.reshape(d.shape[0], -1).any(axis=1)


def _against(got: rb.RayHits, want: rb.RayHits, flat, rays, cls, what):
    """shape index, t, point, normal and a plane's uv to the bit, a sphere's uv within 1e-11 -> the largest sphere-uv error."""
    bad = got.shape_index != want.shape_index
    assert not bad.any(), f"{what}: hit / miss or another shape: " + A.describe(rays, cls, bad)
    hit = want.hit
    assert hit.any() and np.all(np.isposinf(got.t[~hit]))
    for name in ("t", "point", "normal"):
        bad = _rows_differ(getattr(got, name), getattr(want, name))
        assert not bad.any(), f"{what}: {name}: " + A.describe(rays, cls, bad)
    plane = hit & (np.asarray(flat.kind)[np.where(hit, want.shape_index, 0)] == abi.SHAPE_PLANE)
    bad = _rows_differ(got.uv, want.uv) & (plane | ~hit)
    assert not bad.any(), f"{what}: a plane's uv: " + A.describe(rays, cls, bad)
    sph = hit & ~plane
    a, w = got.uv[sph], want.uv[sph]
    err = np.abs(a - w) / np.maximum(np.maximum(np.abs(a), np.abs(w)), 1e-300)
    worst = float(err.max()) if err.size else 0.0
    if not B.uv_close(a, w):
        i = int(np.nonzero(sph)[0][int(np.argmax(err.max(axis=1)))])
        raise AssertionError(f"{what}: sphere uv beyond 1e-11: ray {i} class {int(cls[i])} got {[float(v).hex() for v in got.uv[i]]} "
                             f"want {[float(v).hex() for v in want.uv[i]]}: {' '.join(float(v).hex() for v in rays[i])}")
    return worst


# ---- 1. the exact test, shape by shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.EXACT_WORLDS)
def test_the_exact_test_of_each_target_equals_the_oracle(scene_of, orc, name):
    flat, ds = A.world(name), scene_of(name)
    rays, target, cls = A.exact_batch(name)
    shapes = np.unique(target)
    assert len(shapes) == min(A.EXACT_TARGETS, A.WORLDS[name][0])
    bad = np.zeros(len(rays), bool)
    hits = 0
    for k in shapes:
        sel = np.nonzero(target == k)[0]
        got = ds.hit_probe(rays[sel], int(k))
        want = A.expected_of_shape(orc, flat, rays[sel], int(k))
        hit = want[:, 0] != 0
        hits += int(hit.sum())
        bad[sel] = (got[:, 0] != 0) != hit
        bad[sel[hit]] |= _rows_differ(got[hit, 1:8], want[hit, 1:8]) | (got[hit, 10] != k)
    print(f"{name}: {hits} of {len(rays)} rays hit their target")
    assert not bad.any(), A.describe(rays, cls, bad)
    assert 0.3 * len(rays) < hits < 0.8 * len(rays)


# ---- 2. the query through both libraries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_lanes_probe_and_ray_batches_closest_hit_equal_the_oracle(scene_of, orc, name):
    flat, ds = A.world(name), scene_of(name)
    b = A.batch(orc, name)
    rays, cls, want = b["rays"], b["cls"], b["want"]
    lanes = ds.lanes_probe(rays, anyhit=False)
    bad = (lanes[:, 0] != 0) != want.hit
    assert not bad.any(), "lanes_probe: hit / miss: " + A.describe(rays, cls, bad)
    hit = want.hit
    bad = np.zeros(len(rays), bool)
    bad[hit] = (lanes[hit, 2] != want.shape_index[hit]) | _rows_differ(lanes[hit, 1], want.t[hit])
    assert not bad.any(), "lanes_probe: the shape or t: " + A.describe(rays, cls, bad)
    worst = _against(_traced(scene_of, orc, name)[0], want, flat, rays, cls, "trace_rays")
    print(f"{name}: {int(hit.sum())} hits of {hit.size}, sphere uv max rel err {worst:.3g}")


# ---- 3. any-hit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_lanes_probe_and_ray_batches_any_hit_on_aimed_rays_and_segment_ends(scene_of, orc, name):
    ds = scene_of(name)
    b = A.batch(orc, name)
    m = len(b["seg_of"])
    for what, rays, cls, want in (("aimed", b["rays"], b["cls"], b["want"].hit),
                                  ("segment ends", b["seg"], np.tile(b["cls"][b["seg_of"]], 4), b["seg_want"].hit)):
        bad = (ds.lanes_probe(rays, anyhit=True)[:, 0] != 0) != want
        assert not bad.any(), f"lanes_probe, {what}: " + A.describe(rays, cls, bad)
        blocked = _traced(scene_of, orc, name)[1] if what == "aimed" else ds.occluded(rb.ray_planes(rays))
        assert blocked.dtype == np.int32 and set(np.unique(blocked)) <= {0, 1}
        bad = (blocked == 1) != want
        assert not bad.any(), f"occluded, {what}: " + A.describe(rays, cls, bad)
    sw = b["seg_want"].hit
    assert sw[m: 2 * m].all() and (sw[:m] != sw[m: 2 * m]).mean() >= 0.5  # (the verdicts compared do flip at t*)


# ---- 4. negative tmin, aimed ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_negative_tmin_on_grazing_and_inside_rays(scene_of, orc, name):
    flat, ds = A.world(name), scene_of(name)
    b = A.batch(orc, name)
    sel = np.isin(b["cls"], (0, 3))
    rays, cls = b["rays"][sel].copy(), b["cls"][sel]
    rays[:, 6] = -1e3
    want = A.expected(orc, flat, rays)
    got = ds.trace_rays(rb.ray_planes(rays))
    _against(got, want, flat, rays, cls, "trace_rays, tmin -1e3")
    assert (got.t[got.hit] < 0).any() and (want.t[want.hit & (cls == 3)] < 0).any()


# ---- 5. batch sizes: a last wave of a few live rays -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WORLDS)
def test_prefixes_with_a_sparse_last_wave_equal_the_full_batch(scene_of, orc, name):
    ds = scene_of(name)
    rows = A.batch(orc, name)["rays"]
    full, blocked = _traced(scene_of, orc, name)
    assert any(1 <= n % 64 <= 16 for n in PREFIXES) and all(n % 64 == 5 and n <= len(rows) for n in PREFIXES)
    for n in PREFIXES:
        part = ds.trace_rays(rb.ray_planes(rows[:n]))
        for pname, plane in part.planes().items():
            assert np.ascontiguousarray(plane).tobytes() == np.ascontiguousarray(full.planes()[pname][:n]).tobytes(), (name, n, pname)
        assert np.array_equal(ds.occluded(rb.ray_planes(rows[:n])), blocked[:n]), (name, n)
