"""Surface and scatter queries on records nobody vouches for (include/ptrace_surface.h, include/ptrace_scatter.h: "a record is
the caller's: nothing about it is assumed"): (u, v) that is negative, huge, infinite or NaN, on every texel boundary and in
checkered cells beyond 2^63; shape indices and slot-table entries that name no record; normals that are not unit vectors;
points at a light, at infinity, at the fp32 prefilter's guard and NaN; directions and generator words of any value.  The records
and what they must give are tests/hostile_records.py's (plain Python, pinned to the oracle by tests/test_hostile_records.py).

Expected agreement: the positions of NaN are equal and every other value is bit-identical (a NaN's sign and payload are not
pinned).  The one exception is the project's existing one: the direction of a diffuse bounce holds ocml's sin / cos against
glibc's -- ``rel=1e-12``, and more than half of them bit-identical from ``MIN_FOR_SHARE`` rows on (tests/test_gpu_scatter.py).
The one libm call of the lights kernel (acos) decides a branch; the helper asserts that every aimed record of the dir class
stays 1e-6 rad clear of its threshold.  Device against device (a caller's slot table against the library's, host form against
device form): byte for byte."""
import ctypes as C

import numpy as np
import pytest

from pytracer_amd import abi, rays as rb

from . import hostile_records as H
from . import scatter_batches as X
from .test_gpu_scatter import MIN_FOR_SHARE

pytestmark = pytest.mark.gpu

SURFACE_CLASSES = ("uv", "shape")
LIGHTS_CLASSES = ("uv", "shape", "normal", "point", "dir")
SCATTER_CLASSES = H.HOSTILE  # (the point class rides along: the scattered ray starts at the point, whatever it is)


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
            open_[name] = dev.DeviceScene(H.world(name)[0])
        return open_[name]

    yield get
    for ds in open_.values():
        ds.close()


def _same(b, what, got, want):
    msg = H.explain(b, what, got, want)
    assert not msg, msg


def _lights(ds, b, **kw):
    return ds.shade_lights(b.shape_index, b.point, b.normal, b.uv, b.dirs, H.AMBIENT, H.BACKGROUND, **kw)


def _scatter(ds, b, roulette, channels="all", **kw):
    return ds.scatter(b.shape_index, b.point, b.normal, b.uv, b.dirs, b.pcg, roulette, channels, **kw)


def _compare_scatter(b, got, want, label):
    """tests/test_gpu_scatter.py's ``_compare`` up to NaN identity, naming the class and the first differing record."""
    _same(b, f"{label}: status", got.status, want["status"])
    _same(b, f"{label}: generator words", got.pcg.T, want["pcg"].T)
    rays = want["rays"]
    for rows, what in (([0, 1, 2], "origin"), ([6], "tmin"), ([7], "tmax")):
        _same(b, f"{label}: {what}", got.rays[rows].T, rays[rows].T)
    _same(b, f"{label}: weight", got.weight, want["weight"])
    _same(b, f"{label}: emitted", got.emitted, want["emitted"])
    diffuse = (want["status"] == 1) & (want["kind"] == abi.BRDF_DIFFUSE)
    g, w = np.array(got.rays[3:6].T), np.array(rays[3:6].T)
    g[diffuse], w[diffuse] = 0.0, 0.0
    _same(b, f"{label}: a mirror direction or a dead ray", g, w)
    g, w = np.ascontiguousarray(got.rays[3:6].T[diffuse]), np.ascontiguousarray(rays[3:6].T[diffuse])
    gn, wn = np.isnan(g), np.isnan(w)
    same_bits = (g.view(np.uint64) == w.view(np.uint64)) | (gn & wn)
    with np.errstate(invalid="ignore", over="ignore"):
        den = np.maximum(np.abs(g), np.abs(w))
        err = np.where(same_bits, 0.0, np.abs(g - w) / np.where(den > 0, den, 1.0))  # (inf against inf of the other sign, NaN against a number: NaN)
    worst = float(np.max(np.where(np.isnan(err), np.inf, err)))
    share = float(same_bits.all(axis=1).mean())
    print(f"{label}: {int(diffuse.sum())} diffuse directions, {share:.1%} bit-identical, worst relative difference {worst:.3g}")
    bad = np.flatnonzero(diffuse)[~(np.where(np.isnan(err), np.inf, err) <= 1e-12).all(axis=1)]
    assert bad.size == 0, f"{label}: {bad.size} diffuse directions beyond 1e-12 (worst {worst:.3g}); first: {b.name(int(bad[0]))}: got {got.rays[3:6, bad[0]]}, want {rays[3:6, bad[0]]}"
    assert diffuse.sum() >= MIN_FOR_SHARE and share > 0.5, f"{label}: only {share:.0%} of the diffuse directions are bit-identical"


# ---- 1. surface: materials of records with any (u, v) and any shape index --------------------------------------------------------
@pytest.mark.parametrize("channels", [0, rb.SURF_BRDF_COLOR, rb.SURF_EMITTED, rb.SURF_ALL])
def test_materials_of_hostile_uv_and_shape_indices(scene_of, orc, channels):
    b = H.batch(orc, H.WORLD, SURFACE_CLASSES)
    want = H.wanted(orc, H.WORLD, SURFACE_CLASSES, "surface")
    got = scene_of(H.WORLD).surface(b.shape_index, b.uv if channels else None, channels)  # (channels = 0: uv is not read, it may be absent)
    assert got.n == b.n and got.channels == channels
    _same(b, "brdf_kind", got.brdf_kind, want["brdf_kind"])
    assert np.array_equal(got.hit, b.hit)
    for bit, key in ((rb.SURF_BRDF_COLOR, "brdf_color"), (rb.SURF_EMITTED, "emitted")):
        if channels & bit:
            _same(b, f"channels={channels} {key}", getattr(got, key), want[key])
        else:
            assert not got.has(key)
    if channels == rb.SURF_ALL:
        assert np.isnan(got.brdf_color).any() and np.isinf(got.brdf_color).any() and (got.brdf_color < 0).any()  # the nonfinite texture was read


# ---- 2. scatter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roulette", [False, True])
def test_scatter_of_hostile_records(scene_of, orc, roulette):
    b = H.batch(orc, H.WORLD, SCATTER_CLASSES)
    want = H.wanted(orc, H.WORLD, SCATTER_CLASSES, "scatter", roulette)
    ds = scene_of(H.WORLD)
    got = _scatter(ds, b, roulette)
    assert got.n == b.n
    _compare_scatter(b, got, want, f"hostile roulette={int(roulette)}")
    # a record with status -1 leaves its generator untouched, whatever its words are
    miss = ~b.hit
    assert miss.sum() > 100 and np.all(got.status[miss] == -1) and np.array_equal(got.pcg[:, miss], b.pcg[:, miss])
    dead = got.status != 1
    assert np.array_equal(got.rays[:, dead], np.tile(X.DEAD_RAY[:, None], (1, int(dead.sum()))))
    # the nonfinite texture: (NaN, .5, .5) and (.5, NaN, .5) get the two different lum values of Python's max order ...
    on = lambda col: np.flatnonzero(b.hit & (b.shape_index == H.NONFINITE_SHAPE) & np.array([H.texel(float(u), 6) == col for u in b.uv[:, 0]]))  # noqa: E731
    assert on(0).size and on(1).size and on(4).size
    if not roulette:
        assert np.all(got.status[on(0)] == 0) and np.all(got.status[on(1)] == 1)  # lum NaN: not > 0.  lum 0.5
    else:
        # ... and (-1, -2, -3) -- lum -1, q 2 -- ends every path, with the roulette's one draw consumed
        assert np.all(got.status[on(4)] == 0) and np.all(got.pcg[0, on(4)] != b.pcg[0, on(4)]) and np.array_equal(got.pcg[1, on(4)], b.pcg[1, on(4)])
        assert np.all(got.status[on(0)] == 0) and np.isnan(got.weight[on(0), 0]).all()  # lum NaN: q = max(0.05, NaN) = 0.05; survivors are compensated, none scatters
    # the output block to trace_rays as it stands: the call returns, every record that is not status 1 answers -1, and so does
    # every scattered record whose direction is NaN, at t = +inf
    nxt = ds.trace_rays(got.rays)
    assert np.all(nxt.shape_index[dead] == -1) and np.all(np.isposinf(nxt.t[dead]))
    nan_dir = ~dead & np.isnan(got.rays[3:6]).any(axis=0)
    assert nan_dir.sum() >= 3, int(nan_dir.sum())
    assert np.all(nxt.shape_index[nan_dir] == -1) and np.all(np.isposinf(nxt.t[nan_dir]))
    assert (nxt.shape_index[~dead] >= 0).sum() > 50  # ... while the ordinary records go on hitting things


# ---- 3. shade_lights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.WORLDS)
def test_point_light_colours_of_hostile_records(scene_of, orc, name):
    b = H.batch(orc, name, LIGHTS_CLASSES)
    want = H.wanted(orc, name, LIGHTS_CLASSES, "lights")
    flat = H.world(name)[0]
    if name != H.WORLD:
        assert flat.n_shapes > 256
    got = _lights(scene_of(name), b)
    assert got.shape == (b.n, 3)
    _same(b, f"{name}: colour", np.ascontiguousarray(got), want)
    assert np.isnan(got).any() and np.array_equal(got[~b.hit], np.tile(np.asarray(H.BACKGROUND), (int((~b.hit).sum()), 1)))
    # exactly at the light without a radius, with a finite normal, on a diffuse shape: cos_theta = max2(0, NaN) = 0 -- a finite colour
    at0 = [i for i in np.flatnonzero(b.of("point")) if "exactly at light 0" in b.label[i] and int(flat.brdf_kind[b.shape_index[i]]) == abi.BRDF_DIFFUSE]
    assert at0 and np.isfinite(got[at0]).all(), got[at0]
    # the last wave: NaN-point lanes (exhaustive query), ordinary lanes (filtered), misses and idle lanes together
    last = np.arange(b.n - b.n % 64, b.n)
    assert np.isnan(b.point[last]).any() and b.of("ordinary")[last].any() and b.of("miss")[last].any() and last.size < 64


@pytest.mark.parametrize("name", H.WORLDS)
def test_a_single_nan_point_at_lane_0_and_at_lane_63(scene_of, orc, name):
    """One lane sends its whole wave through the exhaustive query behind the ballot; the other 63 keep their filtered answer."""
    b = H.lone_nan_points(orc, name)
    assert np.flatnonzero(np.isnan(b.point).any(axis=1)).tolist() == [0, 127]
    want = H.want_lights(orc, H.world(name)[0], b)
    _same(b, f"{name}: colour", np.ascontiguousarray(_lights(scene_of(name), b)), want)


# ---- 4. a caller's slot table ---------------------------------------------------------------------------------------------------
def test_a_callers_slot_table_with_entries_that_name_no_record(scene_of, orc):
    """The raw ``*_device`` entry points with a copy of the library's table in which four entries are -1, n_shapes, INT32_MAX and
    INT32_MIN: records on those shapes answer "no hit" in all three kernels, every other record is byte for byte the answer with
    the library's own table."""
    import torch

    from pytracer_amd import _scatter_lib, _surface_lib

    LS, LX = _surface_lib.lib(), _scatter_lib.lib()
    ds = scene_of(H.WORLD)
    flat = H.world(H.WORLD)[0]
    b = H.batch(orc, H.WORLD, SCATTER_CLASSES)
    n, n_shapes = b.n, int(flat.n_shapes)
    own = ds.slot_table()
    table = np.array(own.numpy()).view(np.int32)
    assert sorted(table[:n_shapes].tolist()) == list(range(n_shapes))
    broken = {1: -1, 4: n_shapes, 6: H.INT32_MAX, 9: H.INT32_MIN}
    for s, value in broken.items():
        table[s] = value
    gone = b.hit & np.isin(b.shape_index, list(broken))
    assert all((b.hit & (b.shape_index == s)).sum() > 5 for s in broken) and (b.hit & ~gone).sum() > 500

    up = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731 (a copy: the batch's arrays are read-only)
    mine = up(table)
    shape, point, normal, uv, dirs = up(b.shape_index), up(rb.planar(b.point, 3)), up(rb.planar(b.normal, 3)), up(rb.planar(b.uv, 2)), up(rb.planar(b.dirs, 3))
    pcg = up(b.pcg.view(np.int64))
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(int(t.data_ptr()))  # noqa: E731
    block = ds.kernel_args()
    amb, bg = _surface_lib.rgb(H.AMBIENT), _surface_lib.rgb(H.BACKGROUND)

    def run(slots):
        out = {}
        buf = torch.zeros(rb.surface_bytes(n, rb.SURF_ALL), dtype=torch.uint8, device="cuda")
        _surface_lib.check(LS.pt_rays_surface_device(ds.device, block, len(block), slots, ptr(shape), ptr(uv), n, rb.SURF_ALL, ptr(buf), buf.numel(), None))
        out["surface"] = rb.SurfaceColors(buf.cpu().numpy(), n)
        buf = torch.zeros(rb.scatter_bytes(n, rb.SCAT_ALL), dtype=torch.uint8, device="cuda")
        _scatter_lib.check(LX.pt_rays_scatter_device(ds.device, block, len(block), slots, ptr(shape), ptr(point), ptr(normal), ptr(uv), ptr(dirs),
                                                     C.c_void_p(int(pcg.data_ptr())), C.c_void_p(int(pcg.data_ptr()) + 8 * n), n, 1, rb.SCAT_ALL,
                                                     ptr(buf), buf.numel(), None))
        out["scatter"] = rb.ScatteredRays(buf.cpu().numpy(), n)
        col = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        _surface_lib.check(LS.pt_rays_shade_lights_device(ds.device, block, len(block), slots, ptr(shape), ptr(point), ptr(normal), ptr(uv), ptr(dirs), n,
                                                          amb, bg, ptr(col), 24 * n, None))
        out["lights"] = col.cpu().numpy().T
        return out

    base, got = run(C.c_void_p(own.data_ptr())), run(ptr(mine))
    # the library's own table through the raw entry points is the library's answer
    _same(b, "lights, own table", np.ascontiguousarray(base["lights"]), H.wanted(orc, H.WORLD, SCATTER_CLASSES, "lights"))
    same = lambda x, y: np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()  # noqa: E731
    keep = ~gone
    # surface: kind -1 and zeros
    sg, sb = got["surface"], base["surface"]
    assert np.all(sg.brdf_kind[gone] == -1) and not sg.brdf_color[gone].view(np.uint64).any() and not sg.emitted[gone].view(np.uint64).any()
    assert np.all(sb.brdf_kind[gone] >= 0)
    assert same(sg.brdf_kind[keep], sb.brdf_kind[keep]) and same(sg.brdf_color[keep], sb.brdf_color[keep]) and same(sg.emitted[keep], sb.emitted[keep])
    # scatter: status -1, the dead ray, the generator unchanged
    xg, xb = got["scatter"], base["scatter"]
    assert np.all(xg.status[gone] == -1) and same(xg.rays[:, gone], np.tile(X.DEAD_RAY[:, None], (1, int(gone.sum())))) and same(xg.pcg[:, gone], b.pcg[:, gone])
    assert not xg.weight[gone].view(np.uint64).any() and not xg.emitted[gone].view(np.uint64).any() and np.all(xb.status[gone] >= 0)
    for key in ("status", "weight", "emitted"):
        assert same(getattr(xg, key)[keep], getattr(xb, key)[keep]), key
    assert same(xg.rays[:, keep], xb.rays[:, keep]) and same(xg.pcg[:, keep], xb.pcg[:, keep])
    # shade_lights: the background
    assert same(got["lights"][gone], np.tile(np.asarray(H.BACKGROUND), (int(gone.sum()), 1))) and same(got["lights"][keep], base["lights"][keep])
    assert not same(base["lights"][gone], got["lights"][gone])


# ---- 5. host form against device form -----------------------------------------------------------------------------------------
def test_the_host_forms_equal_the_device_forms_on_hostile_batches(scene_of, orc):
    """The host forms build their own slot table and stage the planes; the device forms take the scene's table and planes in HBM.
    Byte for byte, but for the padding behind the odd int32 plane (as the chains that stay in HBM compare)."""
    import torch

    ds = scene_of(H.WORLD)
    b = H.batch(orc, H.WORLD, SCATTER_CLASSES)
    n = b.n
    assert n % 2 == 1
    pad = (4 * n + 7) // 8 * 8
    up = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731 (a copy: the batch's arrays are read-only)
    shape, point, normal, uv, dirs = up(b.shape_index), up(rb.planar(b.point, 3)), up(rb.planar(b.normal, 3)), up(rb.planar(b.uv, 2)), up(rb.planar(b.dirs, 3))
    pcg = up(b.pcg.view(np.int64))
    torch.cuda.synchronize()

    def equal(dev_buf, host):
        got = dev_buf.numpy()
        assert got[: 4 * n].tobytes() == host.buffer[: 4 * n].tobytes(), "the int32 plane differs between host form and device form"
        assert got[pad: host.nbytes].tobytes() == host.buffer[pad: host.nbytes].tobytes(), "an fp64 plane differs between host form and device form"

    equal(ds.surface(shape, uv, "all", device=True), ds.surface(b.shape_index, b.uv))
    for roulette in (False, True):
        equal(ds.scatter(shape, point, normal, uv, dirs, pcg, roulette, "all", device=True), _scatter(ds, b, roulette))
    host = _lights(ds, b)
    got = ds.shade_lights(shape, point, normal, uv, dirs, H.AMBIENT, H.BACKGROUND, device=True).numpy()
    assert got.shape == (3, n) and got.T.tobytes() == np.ascontiguousarray(host).tobytes()
