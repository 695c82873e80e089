"""Lit queries on the device (include/ptrace_lit.h, libptrace_lit.so): the blend of the eight probes around a record and its
evaluation in one kernel (``lit_eval``), and the same fused with the material look-up (``lit_shade``) -- against their numpy mirrors
(``rays.lit_eval_host`` / ``lit_shade_host``: ``ProbeGrid.corners``, ``ProbeGrid.blend``, ``sh_evaluate``, the normalisation and the
arrays of ``materials()``), against themselves across entry points and batch shapes, and in the frame they are for.

Expected agreement: bit for bit wherever the expected value is finite; where it is not, NaN where NaN is expected and infinities of
the same sign (``hostile_records.differing``).  The band-limited field: 1e-14 of its closed form, as tests/test_gpu_sh.py has it for
one probe.  The furnace: the slack of ``test_the_flat_frame_of_a_world_lit_by_a_probe``, derived there from the furnace's bounds."""
import math

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import rays as rb

from . import hostile_records as H
from . import probe_sets as P
from . import surface_batches as S

pytestmark = pytest.mark.gpu

BG = (0.25, 0.5, 0.125)
NAN, INF = float("nan"), float("inf")
# origin, step, dims: three different steps; one probe; one row; one layer
GRIDS = (((1.0, -2.0, 0.5), (0.5, 1.0, 2.0), (3, 2, 4)), ((0.5, 0.5, 0.5), 2.0, (1, 1, 1)), ((-1.0, 0.0, 3.0), 0.25, (5, 1, 1)),
         ((0.0, 0.0, 0.0), (1.0, 3.0, 1.0), (2, 2, 1)))


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
def demo(dev):
    with dev.DeviceScene(S.world("demo")[0]) as ds:
        yield ds


def _probes(n, seed, evaluator=None):
    """Coefficients of magnitudes e^-3 .. e^3, as test_the_evaluation_equals_its_numpy_mirror_bit_for_bit draws them."""
    rng = np.random.default_rng(seed)
    probes = rb.ProbeSet(np.zeros(rb.sh_bytes(n, 0), np.uint8), n, 0, evaluator=evaluator)
    probes.block[:] = rng.standard_normal((27, n)) * np.exp(rng.uniform(-3, 3, (27, 1)))
    return probes


def _points(grid, m, seed):
    """``m`` points in eight classes, record ``r`` in class ``r % 8`` -> (points [m, 3], class [m])."""
    rng = np.random.default_rng(seed)
    dims, origin, step = np.asarray(grid.dims), grid.origin, grid.step
    lattice = grid.points()
    cls = np.arange(m) % 8
    pts = np.empty((m, 3))
    for r in range(m):
        on = lattice[rng.integers(0, grid.n)]
        c = cls[r]
        if c == 0:  # strictly inside a cell (a one-probe axis has no inside: within one step of the probe)
            pts[r] = origin + (rng.integers(0, np.maximum(dims - 1, 1)) + rng.uniform(0.05, 0.95, 3)) * step
        elif c == 1:  # exactly on a lattice point
            pts[r] = on
        elif c == 2:  # one ulp either side of it, per axis: the snap
            pts[r] = np.nextafter(on, np.where(rng.integers(0, 2, 3) == 1, INF, -INF))
        elif c == 3:  # outside on one face, inside along the other axes
            pts[r] = origin + rng.uniform(0.0, 1.0, 3) * np.maximum(dims - 1, 1) * step
            axis = (r // 8) % 3
            pts[r, axis] = origin[axis] - step[axis] * rng.uniform(0.1, 30.0) if (r // 24) % 2 else origin[axis] + step[axis] * (dims[axis] - 1 + rng.uniform(0.1, 30.0))
        elif c == 4:  # outside on every face at once
            pts[r] = np.where(rng.integers(0, 2, 3) == 1, origin - 7.0 * step, origin + (dims + 6.0) * step)
        elif c == 5:  # infinite and huge
            pts[r] = ((INF, on[1], on[2]), (on[0], -INF, on[2]), (INF, -INF, INF), (1e300, on[1], -1e300), (1.7e308, -1.7e308, 1e300),
                      (on[0], on[1], 1e300))[(r // 8) % 6]
        elif c == 6:  # NaN: zeros
            pts[r] = ((NAN, on[1], on[2]), (on[0], NAN, on[2]), (on[0], on[1], NAN), (NAN, NAN, NAN), (NAN, INF, -INF))[(r // 8) % 5]
        else:  # an ordinary record that the active plane skips (see _active)
            pts[r] = origin + rng.uniform(0.0, 1.0, 3) * np.maximum(dims - 1, 1) * step
    return pts, cls


def _active(cls):
    act = np.arange(cls.size, dtype=np.int32) % 5
    act[cls == 7] = np.where(np.arange((cls == 7).sum()) % 2 == 0, -1, -2 ** 31)
    return act


def _check(got, want, label):
    bad = H.differing(np.ascontiguousarray(got), np.ascontiguousarray(want))
    assert bad.size == 0, f"{label}: {bad.size} of {len(want)} records differ, first {int(bad[0])}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---- 1. the lit query against its mirror --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 65, 1000])
@pytest.mark.parametrize("origin,step,dims", GRIDS, ids=["3x2x4", "1x1x1", "5x1x1", "2x2x1"])
def test_the_lit_query_equals_its_numpy_mirror_bit_for_bit(demo, origin, step, dims, m):
    grid = rb.ProbeGrid(origin, step, dims)
    probes = _probes(grid.n, 100 + grid.n, demo.sh_eval)
    total = max(m, 16)  # (m = 1: sixteen batches of one record, two of every class)
    pts, cls = _points(grid, total, 1000 + m)
    rng = np.random.default_rng(7 + m)
    dirs = rng.standard_normal((total, 3))
    dirs[::3] /= np.linalg.norm(dirs[::3], axis=1, keepdims=True)  # a third of them unit vectors, the rest of any length
    act = _active(cls)
    zero = (cls == 6) | (cls == 7)
    for kind in (rb.SH_RADIANCE, rb.SH_HEMISPHERE):
        want = rb.lit_eval_host(grid, probes, pts, dirs, kind, act)
        assert not want[zero].any() and np.isfinite(want).all() and np.abs(want[~zero]).min() > 0.0
        if m == 1:
            got = np.concatenate([demo.lit_eval(grid, probes.block, rb.planar(pts[r: r + 1], 3), rb.planar(dirs[r: r + 1], 3), act[r: r + 1], kind).T
                                  for r in range(total)])
        else:
            got = demo.lit_eval(grid, probes.block, rb.planar(pts, 3), rb.planar(dirs, 3), act, kind).T
        _check(got, want, f"dims {dims} m {m} kind {kind}")
        assert not got[zero].any() and not np.signbit(got[zero]).any()  # +0.0, and the neighbours are the mirror's
    # without the active plane the skipped records are ordinary ones; ProbeGrid.evaluate is the same call
    if m > 1:
        plain = grid.evaluate(probes, pts, dirs, rb.SH_HEMISPHERE)
        _check(plain, rb.lit_eval_host(grid, probes, pts, dirs, rb.SH_HEMISPHERE), "no active plane")
        assert np.abs(plain[cls == 7]).min() > 0.0 and not plain[cls == 6].any()
        # a record on a lattice point is that probe in every bit
        on = cls == 1
        index, weight = grid.corners(pts[on])
        assert np.all(weight.max(axis=1) == 1.0)
        probe = index[np.arange(index.shape[0]), weight.argmax(axis=1)]
        _check(plain[on], rb.sh_evaluate(probes.coefficients[probe], dirs[on], rb.SH_HEMISPHERE), "on the lattice")
        # ... and so are most of those one ulp beside it (the snap; where an ulp of the point is more than 4 eps of g, the mirror decides)
        near = cls == 2
        snapped = grid.corners(pts[near])[1].max(axis=1) == 1.0
        assert snapped.mean() > 0.5


def test_refusals_and_empty_batches_through_the_device_scene(demo):
    from pytracer_amd import _lib

    grid = rb.ProbeGrid((0.0, 0.0, 0.0), 1.0, (2, 2, 2))
    probes = _probes(8, 1)
    pts, dirs = np.zeros((3, 4)), np.ones((3, 4))
    with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*kind"):
        demo.lit_eval(grid, probes.block, pts, dirs, None, 2)
    with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*coefficient block"):
        demo.lit_eval(grid, probes.block[:, :7], pts, dirs)
    with pytest.raises(ValueError, match="planar"):
        demo.lit_eval(grid, probes.block, pts, dirs[:, :3])
    with pytest.raises(ValueError, match="device=True"):
        demo.lit_eval(grid, probes.block, pts, dirs, m=4)
    assert demo.lit_eval(grid, probes.block, np.zeros((3, 0)), np.zeros((3, 0))).shape == (3, 0)
    out = demo.lit_shade(grid, probes.block, np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 3)))
    assert out.shape == (0, 3)
    with pytest.raises(ValueError, match="shape indices"):
        demo.lit_shade(grid, probes.block, np.zeros(2, np.int32), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((1, 2)), np.zeros((2, 3)))


# ---- 2. the shade query on hit frames ---------------------------------------------------------------------------------------------
def _scaled_mirror_world():
    """A mirror sphere, a diffuse sphere under a non-uniform scaling (its normals are not unit length), a checkered diffuse plane with a
    checkered glow, and a mirror plane behind them."""
    from pytracer_amd import hostmodel as hm

    world = hm.World()
    world.add_shape(hm.Plane(hm.Transformation(), hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.3, 0.5, 0.1), hm.Color(0.1, 0.2, 0.5), 4)),
                                                            hm.CheckeredPigment(hm.Color(0.0, 0.0, 0.25), hm.Color(0.125, 0.0, 0.0), 3))))
    world.add_shape(hm.Sphere(hm.translation(hm.Vec(0.5, -0.9, 0.8)) * hm.scaling(hm.Vec(0.7, 0.7, 0.7)),
                              hm.Material(hm.SpecularBRDF(hm.UniformPigment(hm.Color(0.9, 0.8, 0.7))), hm.UniformPigment(hm.Color(0.0, 0.01, 0.02)))))
    world.add_shape(hm.Sphere(hm.translation(hm.Vec(0.2, 0.9, 0.7)) * hm.scaling(hm.Vec(1.2, 1.0, 0.6)),
                              hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(0.6, 0.3, 0.9))), hm.UniformPigment(hm.Color(0.05, 0.0, 0.0)))))
    world.add_shape(hm.Plane(hm.translation(hm.Vec(6.0, 0.0, 0.0)) * hm.rotation_y(90.0),
                             hm.Material(hm.SpecularBRDF(hm.UniformPigment(hm.Color(0.5, 0.5, 0.5))), hm.UniformPigment(hm.Color(0.0, 0.0, 0.0)))))
    camera = hm.PerspectiveCamera(screen_distance=1.0, aspect_ratio=24 / 18, transformation=hm.translation(hm.Vec(-1.5, 0.0, 1.0)))
    return world, camera


def _frame_world(name):
    if name == "scaled_mirror":
        return _scaled_mirror_world()
    return S.host_world(name)


@pytest.fixture(scope="module")
def frames(dev):
    """name -> (tracer, world, the 24 x 18 hit frame, its queries), rendered once for the module."""
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.tracer import GpuImageTracer

    made = {}

    def get(name):
        if name not in made:
            world, camera = _frame_world(name)
            tracer = GpuImageTracer(hm.HdrImage(24, 18), camera, samples_per_side=0)
            frame = tracer.fire_all_hits(world)
            made[name] = (tracer, world, frame, tracer.world_queries(world))
        return made[name]

    yield get
    for tracer, _, _, _ in made.values():
        tracer.close()


def _lattice_over(frame, dims=(3, 2, 4)):
    """A lattice over the middle of the frame's hit points, so that records fall inside, on the border and far outside."""
    pts = np.asarray(frame.point)[np.asarray(frame.hit)]
    lo, hi = np.percentile(pts, 25, axis=0), np.percentile(pts, 75, axis=0)
    step = np.maximum((hi - lo) / np.maximum(np.asarray(dims) - 1, 1), 1e-3)
    return rb.ProbeGrid(lo, step, dims)


@pytest.mark.parametrize("name", ["demo", "pigments", "scaled_mirror"])
def test_the_shade_query_on_a_hit_frame_equals_its_mirror(frames, name):
    tracer, world, frame, wq = frames(name)
    grid = _lattice_over(frame)
    probes = _probes(grid.n, 31, wq.scene.sh_eval)
    mat = wq.materials(frame)
    kinds = np.asarray(mat.brdf_kind)
    want = rb.lit_shade_host(grid, probes, mat, frame.point, frame.normal, frame.ray_dir, BG)
    got = wq.probe_lit_radiance(grid, probes, frame, background=BG)
    assert got.shape == frame.shape_index.shape + (3,) == (1, 18, 24, 3)
    _check(got.reshape(-1, 3), want.reshape(-1, 3), name)
    hit = np.asarray(frame.hit)
    assert hit.sum() > 100 and np.isfinite(want).all() and len(np.unique(want[hit], axis=0)) > 50
    if not hit.all():
        assert np.all(got[~hit] == BG)
    if name != "pigments":
        assert (kinds == abi.BRDF_DIFFUSE).any() and (kinds == abi.BRDF_SPECULAR).any()
    if name == "scaled_mirror":
        assert (np.asarray(frame.shape_index) == 2).sum() > 10  # the sphere under the non-uniform scaling is in the frame
    # the mirror direction is the scatter query's, in every bit
    specular = (kinds == abi.BRDF_SPECULAR).reshape(-1)
    if specular.any():
        sc = wq.scatter(frame, None, rb.pcg_streams(42, np.arange(specular.size)), roulette=False)
        went = specular & (np.asarray(sc.status).reshape(-1) == 1)
        assert went.sum() > 10
        mine = rb.mirror_directions(np.asarray(frame.ray_dir).reshape(-1, 3), np.asarray(frame.normal).reshape(-1, 3))
        _check(mine[went], np.asarray(sc.dirs).reshape(-1, 3)[went], f"{name}: mirror directions")
    # a closest-hit batch with dirs=, and plain arrays: the same records, the same bits
    flat_rows = dict(shape_index=np.asarray(frame.shape_index).reshape(-1), point=np.asarray(frame.point).reshape(-1, 3),
                     normal=np.asarray(frame.normal).reshape(-1, 3), uv=np.asarray(frame.uv).reshape(-1, 2))
    again = wq.probe_lit_radiance(grid, probes, flat_rows, dirs=np.asarray(frame.ray_dir).reshape(-1, 3), background=BG)
    _check(again, want.reshape(-1, 3), f"{name}: plain arrays")
    # normals that are not unit length, as the reference's HitRecord has them under a scaling (shapes.py:126, 181): the query normalises
    long_rows = dict(flat_rows, normal=flat_rows["normal"] * np.random.default_rng(3).uniform(0.2, 5.0, (flat_rows["normal"].shape[0], 1)))
    long_want = rb.lit_shade_host(grid, probes, rb.SurfaceColors(mat.buffer, mat.n, mat.channels), flat_rows["point"], long_rows["normal"],
                                  np.asarray(frame.ray_dir).reshape(-1, 3), BG)
    _check(wq.probe_lit_radiance(grid, probes, long_rows, dirs=np.asarray(frame.ray_dir).reshape(-1, 3), background=BG), long_want,
           f"{name}: normals of any length")
    assert np.abs(long_want - want.reshape(-1, 3)).max() <= 1e-9 * np.abs(want).max()  # (the same directions but for a rounding)
    # sub-batches give the whole batch's bits
    rows = want.reshape(-1, 3)
    for lo, hi in ((0, 1), (1, 66), (66, 432)):
        part = wq.probe_lit_radiance(grid, probes, {k: v[lo:hi] for k, v in flat_rows.items()}, dirs=np.asarray(frame.ray_dir).reshape(-1, 3)[lo:hi],
                                     background=BG)
        _check(part, rows[lo:hi], f"{name}: records {lo}..{hi}")


def test_shape_indices_that_name_no_shape_give_the_background(frames):
    tracer, world, frame, wq = frames("demo")
    grid = _lattice_over(frame)
    probes = _probes(grid.n, 32)
    n_shapes = len(world.shapes)
    index = np.asarray(frame.shape_index).reshape(-1).copy()
    wild = np.arange(index.size) % 4 == 1
    index[wild] = np.resize(np.array([-1, n_shapes, 2 ** 31 - 1, -2 ** 31, n_shapes + 1], dtype=np.int32), wild.sum())
    rows = dict(shape_index=index, point=np.asarray(frame.point).reshape(-1, 3), normal=np.asarray(frame.normal).reshape(-1, 3),
                uv=np.asarray(frame.uv).reshape(-1, 2))
    dirs = np.asarray(frame.ray_dir).reshape(-1, 3)
    got = wq.probe_lit_radiance(grid, probes, rows, dirs=dirs, background=BG)
    whole = wq.probe_lit_radiance(grid, probes, frame, background=BG).reshape(-1, 3)
    assert np.all(got[wild] == BG) and P.same_bits(got[~wild], whole[~wild])


def test_hostile_records_equal_the_mirror(dev, orc):
    """The records of tests/hostile_records.py -- hostile (u, v), shape indices, normals, points and directions among ordinary
    records and misses: the pigments are the surface query's, a NaN point gives emitted + colour * 0, and whatever is not finite in
    the mirror is not finite in the same way on the device."""
    classes = ("uv", "shape", "normal", "point", "dir")
    b = H.batch(orc, H.WORLD, classes)
    with dev.DeviceScene(H.world(H.WORLD)[0]) as ds:
        wq = rb.WorldQueries(ds)
        hit_pts = b.point[b.hit & np.isfinite(b.point).all(axis=1)]
        lo, hi = np.percentile(hit_pts, 20, axis=0), np.percentile(hit_pts, 80, axis=0)
        grid = rb.ProbeGrid(lo, np.maximum((hi - lo) / 2.0, 1e-3), (3, 3, 3))
        probes = _probes(grid.n, 33)
        mat = wq.materials(b)
        want = rb.lit_shade_host(grid, probes, mat, b.point, b.normal, b.dirs, BG)
        got = wq.probe_lit_radiance(grid, probes, b, dirs=b.dirs, background=BG)
    message = H.explain(b, "lit", got, want)
    assert not message, message
    nan_point = b.hit & np.isnan(b.point).any(axis=1) & (np.asarray(mat.brdf_kind) >= 0)
    assert nan_point.any() and (~np.isfinite(want)).any() and np.isfinite(want).all(axis=1).sum() > b.n // 2
    zero = np.asarray(mat.emitted)[nan_point] + np.asarray(mat.brdf_color)[nan_point] * 0.0
    assert H.differing(got[nan_point], zero).size == 0
    assert np.all(got[~b.hit] == BG)


# ---- 3. in HBM ---------------------------------------------------------------------------------------------------------------------
def test_planes_inside_a_hit_frame_in_hbm_on_a_stream(dev):
    """``device=True``: the hit frame rendered into a device buffer, the shade query reading its planes where they are, on a stream,
    twice into the same output: the host form's bits.  The lit query from device tensors likewise."""
    import torch

    from pytracer_amd import _lib, flatten
    from pytracer_amd.devmem import DeviceBuffer, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh = 24, 18
    world, camera = _scaled_mirror_world()
    flat, cam = flatten.flatten_world(world), flatten.flatten_camera(camera)
    par = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    n = W * Hh
    st = Stream()
    try:
        with dev.DeviceScene(flat) as ds:
            hits = DeviceBuffer((abi.hits_bytes(par, abi.HIT_ALL),), np.uint8)
            ds.render_hits_into(cam, par, abi.HIT_ALL, hits, stream=st)
            frame = HitFrame(hits.numpy(), par, abi.HIT_ALL)
            grid = _lattice_over(frame)
            probes = _probes(grid.n, 34)
            want = ds.lit_shade(grid, probes.block, frame.shape_index, frame.point, frame.normal, frame.uv, frame.ray_dir, BG)
            to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
            co_d = to_dev(probes.block)
            torch.cuda.synchronize()
            base = hits.data_ptr()
            off = lambda channel, first=0: base + abi.hits_plane_offset(par, abi.HIT_ALL, channel, first)  # noqa: E731
            mine = DeviceBuffer((3, n), np.float64)
            for turn in range(2):
                out = ds.lit_shade(grid, co_d, base, off(abi.HIT_POINT), off(abi.HIT_NORMAL), off(abi.HIT_UV), off(abi.HIT_RAY, 3), BG,
                                   device=True, stream=st, out=mine, n=n)
                assert out is mine and P.same_bits(mine.numpy().T, np.ascontiguousarray(want)), f"turn {turn}"
            fresh = ds.lit_shade(grid, co_d, base, off(abi.HIT_POINT), off(abi.HIT_NORMAL), off(abi.HIT_UV), off(abi.HIT_RAY, 3), BG, device=True, n=n)
            assert P.same_bits(fresh.numpy()[:, :n].T, np.ascontiguousarray(want))
            # the lit query: points and directions as device tensors
            pts, dirs = np.asarray(frame.point).reshape(-1, 3), np.asarray(frame.normal).reshape(-1, 3)
            pts_d, dirs_d, act_d = to_dev(rb.planar(pts, 3)), to_dev(rb.planar(dirs, 3)), to_dev(np.asarray(frame.shape_index).reshape(-1))
            torch.cuda.synchronize()
            ev = ds.lit_eval(grid, co_d, pts_d, dirs_d, act_d, rb.SH_HEMISPHERE, device=True, stream=st)
            assert P.same_bits(ev.numpy()[:, :n], ds.lit_eval(grid, probes.block, rb.planar(pts, 3), rb.planar(dirs, 3), frame.shape_index, rb.SH_HEMISPHERE))
            for kw in (dict(out=DeviceBuffer((3 * n - 1,), np.float64)),):
                with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE"):
                    ds.lit_shade(grid, co_d, base, off(abi.HIT_POINT), off(abi.HIT_NORMAL), off(abi.HIT_UV), off(abi.HIT_RAY, 3), BG, device=True,
                                 stream=st, n=n, **kw)
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*coefficient block"):
                ds.lit_eval(grid, DeviceBuffer((27 * grid.n - 1,), np.float64), pts_d, dirs_d, None, 0, device=True, stream=st)
            with pytest.raises(ValueError, match="n="):
                ds.lit_shade(grid, co_d, base, off(abi.HIT_POINT), off(abi.HIT_NORMAL), off(abi.HIT_UV), off(abi.HIT_RAY, 3), BG, device=True)
            with pytest.raises(ValueError, match="device=True"):
                ds.lit_shade(grid, probes.block, frame.shape_index, frame.point, frame.normal, frame.uv, frame.ray_dir, BG, stream=st)
            st.synchronize()
    finally:
        st.close()


# ---- 4. a band-limited field ---------------------------------------------------------------------------------------------------------
def test_the_trilinear_multiple_of_a_band_limited_field(demo):
    """A (2, 2, 2) lattice whose probe ``i`` holds ``a_i`` times the field of tests/probe_sets.py: at any point the radiance and the
    hemisphere mean are the trilinear blend of the ``a_i`` times the closed forms, to 1e-14."""
    grid = rb.ProbeGrid((0.0, 0.0, 0.0), (1.0, 2.0, 0.5), (2, 2, 2))
    a = np.array([0.5, 1.0, 0.75, 0.25, 0.125, 0.625, 0.375, 0.875])
    probes = rb.ProbeSet(np.zeros(rb.sh_bytes(8, 0), np.uint8), 8, 0, evaluator=demo.sh_eval)
    probes.coefficients[:] = a[:, None, None] * P.field_coefficients()[None, :, None]
    rng = np.random.default_rng(9)
    m = 200
    d = rng.standard_normal((m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    f = rng.uniform(0.0, 1.0, (m, 3))
    f[:8] = [[(c >> k) & 1 for k in range(3)] for c in range(8)]  # the eight corners themselves
    pts = grid.origin + f * grid.step
    tri = np.zeros(m)
    for c in range(8):
        w = np.ones(m)
        for k in range(3):
            w = w * (f[:, k] if (c >> k) & 1 else 1.0 - f[:, k])
        tri = tri + w * a[c]
    rad, hem = grid.evaluate(probes, pts, d, rb.SH_RADIANCE), grid.evaluate(probes, pts, d, rb.SH_HEMISPHERE)
    assert np.abs(rad - (tri * P.field(d))[:, None]).max() <= 1e-14 and np.abs(hem - (tri * P.field_hemisphere(d))[:, None]).max() <= 1e-14
    assert np.abs(rad[:8, 0] - a * P.field(d[:8])).max() <= 1e-14


# ---- 5. what it is for: a world baked once, a shape it does not know lit by probes, one frame ---------------------------------------
def test_a_frame_of_a_baked_world_and_a_sphere_lit_by_a_lattice(dev, orc):
    """The furnace of tests/probe_sets.py; a (2, 2, 2) lattice of probes at ``FURNACE_K`` around the place where the small diffuse
    sphere of ``test_the_flat_frame_of_a_world_lit_by_a_probe`` is then put; the furnace wall baked (``baked_world``: a black BRDF, its
    map as emission).  ``fire_all_rays(ProbeLitShader(...))`` at 48 x 36 is the mirror applied to ``fire_all_hits`` bit for bit; every
    pixel on the small sphere is ``glow + colour * L`` within that test's slack (a blend of probes by weights that are not negative and
    sum to 1 keeps the bounds each probe's coefficients keep); every pixel on the wall is the flat frame's pixel in every bit."""
    from pytracer_amd import flatten, scenes
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.shaders import ProbeLitShader
    from pytracer_amd.tracer import GpuImageTracer

    K, D, depth = P.FURNACE_K, P.FURNACE_D, P.FURNACE_DEPTH
    at, radius, colour, glow = (0.3, 0.1, -0.05), 0.25, (0.6, 0.3, 0.9), (0.0, 0.05, 0.0)
    grid = rb.ProbeGrid(np.array(at) - 0.3, 0.6, (2, 2, 2))
    assert np.sqrt((grid.points() ** 2).sum(axis=1)).max() < 0.9  # every probe inside the furnace
    with dev.DeviceScene(flatten.flatten_world(P.furnace_world())) as ds:
        wq0 = rb.WorldQueries(ds)
        probes = wq0.radiance_probes(grid.points(), K, P.S0, num_of_rays=1, max_depth=D, russian_roulette_limit=D + 5, background=BG, depth=depth)
        wall = wq0.outgoing_map(0, 16, 8, 16, side=-1, max_depth=D, russian_roulette_limit=D + 5, init_state=P.S0)
    rel0, bound0, rest, bound = P.furnace_bounds(probes.coefficients)
    assert rel0.max() <= bound0 and rest.max() <= bound  # (the bounds the slack below is derived from, on these eight probes)
    world = P.furnace_world()
    world.add_shape(hm.Sphere(hm.translation(hm.Vec(*at)) * hm.scaling(hm.Vec(radius, radius, radius)),
                              hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(*colour))), hm.UniformPigment(hm.Color(*glow)))))
    baked = scenes.baked_world(world, {0: wall})
    camera = hm.PerspectiveCamera(screen_distance=1.0, aspect_ratio=48 / 36, transformation=hm.translation(hm.Vec(0.4, 0.0, 0.0)))
    W, Hh = 48, 36
    image, flat_image = hm.HdrImage(W, Hh), hm.HdrImage(W, Hh)
    tracer = GpuImageTracer(image, camera, samples_per_side=0)
    try:
        shader = ProbeLitShader(baked, grid, probes, tracer, hm.Color(*BG))
        tracer.fire_all_rays(shader)
        assert tracer.last_path == "device-hits"
        got = np.array(image.array, dtype=np.float64)
        frame = tracer.fire_all_hits(baked)
        wq = tracer.world_queries(baked)
        want = rb.lit_shade_host(grid, probes, wq.materials(frame), frame.point, frame.normal, frame.ray_dir, BG)[0]
        flat_tracer = GpuImageTracer(flat_image, camera, samples_per_side=0)
        try:
            flat_tracer.fire_all_rays(hm.FlatRenderer(baked))
        finally:
            flat_tracer.close()
    finally:
        tracer.close()
    assert got.shape == (Hh, W, 3) and got.tobytes() == np.ascontiguousarray(want).tobytes()
    index = np.asarray(frame.shape_index)[0]
    on_sphere, on_wall = index == 1, index == 0
    assert on_sphere.sum() > 40 and on_wall.sum() > 1000 and (on_sphere | on_wall).all()
    L = P.furnace_radiance()
    slack = np.array(colour) * L * (1e-13 + 6.0 * math.sqrt(4.0 * math.pi / K) * (3 * (2.0 / 3.0) * rb.SH_K1 + 5 * 0.25 * rb.SH_K2) + 32 * P.EPS)
    off = np.abs(got[on_sphere] - (np.array(glow) + np.array(colour) * L))
    print(f"{int(on_sphere.sum())} pixels on the small sphere: off by at most {(off / slack).max():.3g} of the slack {slack}")
    assert np.all(off <= slack) and len(np.unique(got[on_sphere], axis=0)) > 20
    flat_frame = np.asarray(flat_image.array, dtype=np.float64)
    assert got[on_wall].tobytes() == flat_frame[on_wall].tobytes()  # (a furnace: the wall's map is one colour, Le + rho * L)
    assert np.abs(got[on_wall] - (np.array(P.FURNACE_LE) + np.array(P.FURNACE_RHO) * L)).max() <= 0.05 * L.max()
