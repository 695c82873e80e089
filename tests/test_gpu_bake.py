"""Bake queries on the device (include/ptrace_bake.h, libptrace_bake.so): surface points from (shape, u, v) and light maps over a
shape's (u, v) grid -- against a numpy restatement and the CPU oracle in its ``x * x`` mode (tests/bake_maps.py), against the
libraries there already were (surface points, then the gather; surface points, scatter and radiance, then the host's ordered
sum), and against itself across launch shapes, windows and entry points.

Expected agreement.  Surface points against libm: the bound of ``bake_maps.point_bounds`` (64 eps of the magnitudes that enter a
component).  Against the oracle a diffuse bounce holds ocml's sin / cos against glibc's, and here so does the surface point itself:
radiance to ``TOL = 1e-5`` relative per channel, and a texel beyond it, or not finite, or with another count, is an outlier, of
which a case may hold ONE -- the gather tests' cap.  Device against device: bit for bit, no cap and no tolerance."""
import numpy as np
import pytest

from pytracer_amd import abi, rays as rb

from . import bake_maps as M
from . import gather_batches as G
from . import radiance_batches as R

pytestmark = pytest.mark.gpu

BG = M.BACKGROUND
MAX_OUTLIERS = 1
SHAPES = M.all_shapes()
IDS = [f"{name}-{s}" for name, s in SHAPES]


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
            open_[name] = dev.DeviceScene(R.world(name)[0])
        return open_[name]

    yield get
    for ds in open_.values():
        ds.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bake(ds, s, W, H, K, N, D, limit, side=1, jitter=True, window=None, depth=1, channels="all", **kw):
    return ds.bake(s, W, H, K, side, jitter, window, M.S0, M.Q0, N, D, limit, BG, depth, channels, **kw)


def _same_map(got, want_radiance, want_count, label):
    rad, cnt = np.asarray(got.radiance).reshape(-1, 3), np.asarray(got.n_rays).reshape(-1)
    bad = ~G.same_bits(rad, np.asarray(want_radiance).reshape(-1, 3))
    assert not bad.any(), f"{label}: radiance differs in {int(bad.sum())} of {rad.shape[0]} texels (first: {int(np.flatnonzero(bad)[0])})"
    assert _bits(cnt, np.asarray(want_count, dtype=np.uint64).reshape(-1)), f"{label}: counts differ"


# ---- 1. surface points -----------------------------------------------------------------------------------------------------------
def test_surface_points_against_the_numpy_restatement(scene_of, orc):
    """u over [0, 1) and v over [0.02, 0.98] for every shape of the three worlds, both sides: the device's point and normal within
    ``point_bounds`` of the libm restatement, component by component."""
    worst = 0.0
    g = orc.Pcg(7, 11)
    for name, s in SHAPES:
        flat = R.world(name)[0]
        uv = np.array([[g.random_float() * 0.999, 0.02 + 0.96 * g.random_float()] for _ in range(67)])
        for side in (1, -1):
            pts, nrm = rb.WorldQueries(scene_of(name)).surface_points(s, uv, side)
            want_p, want_n = M.surface_points(orc, flat, s, uv, side)
            for i in range(uv.shape[0]):
                pb, nb = M.point_bounds(flat, s, uv[i, 0], uv[i, 1], side)
                err, bound = np.abs(np.concatenate([pts[i] - want_p[i], nrm[i] - want_n[i]])), np.concatenate([pb, nb])
                assert np.all(err <= bound), (name, s, side, i, pts[i], want_p[i], nrm[i], want_n[i], err, bound)
                worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))  # (a bound of 0: a component that is exact)
            assert np.allclose(np.sum(nrm * nrm, axis=1), 1.0, rtol=0, atol=8 * M.EPS)
    print(f"surface points: worst |device - libm| / bound = {worst:.4f} (bound: 64 eps of the magnitudes)")


@pytest.mark.parametrize("name,s", SHAPES, ids=IDS)
def test_surface_points_round_trip_through_the_oracles_intersection(scene_of, orc, name, s):
    """A ray from ``point + normal`` towards ``-normal`` meets the one shape where it was asked to: (u', v') within 1e-12 of the
    request for v in [0.05, 0.95] (acos amplifies by at most 1 / sin(0.05 pi), about 6.4), and at the centres of 1x1, 7x5 and 64x64
    maps inside the texel that was asked for."""
    flat = R.world(name)[0]
    wq = rb.WorldQueries(scene_of(name))
    g = orc.Pcg(3, 5)
    uv = np.array([[g.random_float() * 0.999, 0.05 + 0.9 * g.random_float()] for _ in range(101)])
    pts, nrm = wq.surface_points(s, uv)
    for i in range(uv.shape[0]):
        hit = orc.shape_intersect(flat, s, orc.ray8(pts[i] + nrm[i], -nrm[i]))
        assert hit is not None and abs(hit[7] - uv[i, 0]) <= 1e-12 and abs(hit[8] - uv[i, 1]) <= 1e-12, (i, uv[i], hit)
    for W, H in ((1, 1), (7, 5), (64, 64)):
        centres = rb.texel_centres(W, H)
        pts, nrm = wq.surface_points(s, centres)
        assert pts.shape == (H, W, 3)
        step = max(1, (W * H) // 256)
        for t in range(0, W * H, step):
            r, c = divmod(t, W)
            hit = orc.shape_intersect(flat, s, orc.ray8(pts[r, c] + nrm[r, c], -nrm[r, c]))
            assert hit is not None and int(hit[7] * W) == c and int(hit[8] * H) == r, (W, H, r, c, hit)


def test_hostile_surface_point_records(scene_of):
    """Both sides; a shape of -1 or n_shapes gives zeros; NaN or infinite uv beside clean records leave the clean ones unchanged."""
    name = "pigments"
    flat, ds = R.world(name)[0], scene_of(name)
    shapes3 = M.diffuse_shapes(name)
    n = 300
    shape = np.array([shapes3[i % 3] for i in range(n)], np.int32)
    uv = np.stack([(np.arange(n) + 0.25) / n, 0.05 + 0.9 * ((np.arange(n) * 7) % n) / n], axis=1)
    side = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int32)
    clean = ds.surface_points(shape, uv, side)
    assert clean.shape == (6, n) and np.isfinite(clean).all() and len(np.unique(clean[0])) > 100
    # both sides: the same point, the opposite normal, exactly; side NULL is +1 and any negative value is -1
    plus, minus = ds.surface_points(shape, uv, None), ds.surface_points(shape, uv, np.full(n, -7, np.int32))
    assert _bits(plus[0:3], minus[0:3]) and np.array_equal(plus[3:6], -minus[3:6]) and _bits(plus, ds.surface_points(shape, uv, np.ones(n, np.int32)))
    even = side == 1
    assert _bits(clean[:, even], plus[:, even]) and _bits(clean[:, ~even], minus[:, ~even])
    # hostile records beside clean ones
    bad_shape, bad_uv = shape.copy(), uv.copy()
    rows = np.arange(1, n, 4)
    kinds = {k: rows[i::5] for i, k in enumerate(("minus_one", "n_shapes", "nan_u", "inf_v", "huge"))}
    bad_shape[kinds["minus_one"]] = -1
    bad_shape[kinds["n_shapes"]] = flat.n_shapes
    bad_uv[kinds["nan_u"], 0] = np.nan
    bad_uv[kinds["inf_v"], 1] = -np.inf
    bad_uv[kinds["huge"]] = [1.0e300, -1.7e308]
    got = ds.surface_points(bad_shape, bad_uv, side)
    others = np.setdiff1d(np.arange(n), rows)
    assert all(k.size >= 10 for k in kinds.values()) and _bits(got[:, others], clean[:, others])
    for k in ("minus_one", "n_shapes"):
        assert not got[:, kinds[k]].any() and not np.signbit(got[:, kinds[k]]).any(), k
    assert np.isnan(got[:, kinds["nan_u"]]).any(axis=0).all() and np.isnan(got[:, kinds["inf_v"]]).any(axis=0).all()
    assert ds.surface_points(np.zeros(0, np.int32), np.zeros((0, 2))).shape == (6, 0)
    with pytest.raises(ValueError, match="pairs"):
        ds.surface_points(shape, uv[:5])
    with pytest.raises(ValueError, match="side"):
        ds.surface_points(shape, uv, side[:5])


# ---- 2. centre mode = surface points, then the gather, bit for bit ----------------------------------------------------------------
MAPS = ((1, 1), (1, 65), (7, 5), (16, 16))  # (W, H)
KS = (1, 3, 64, 70)
NDL = ((1, 3, 2), (2, 2, 1), (10, 2, 3))
CENTRE_CASES = [(SHAPES[(i + 3 * j) % len(SHAPES)], MAPS[i], KS[j], NDL[(i + j) % 3], -1 if (i, j) == (2, 1) else 1)
                for i in range(4) for j in range(4)]


@pytest.mark.parametrize("shape,size,K,ndl,side", CENTRE_CASES,
                         ids=[f"{sh[0]}-{sh[1]}-{sz[0]}x{sz[1]}-K{K}-N{ndl[0]}D{ndl[1]}L{ndl[2]}-side{sd}" for sh, sz, K, ndl, sd in CENTRE_CASES])
def test_centre_mode_equals_surface_points_then_gather_bit_for_bit(scene_of, shape, size, K, ndl, side):
    (name, s), (W, H), (N, D, limit) = shape, size, ndl
    ds = scene_of(name)
    pts, nrm = rb.WorldQueries(ds).surface_points(s, rb.texel_centres(W, H), side)
    seqs = (M.Q0 + K * np.arange(W * H)).astype(np.uint64)  # seq_t = init_seq + t K
    want = ds.gather(rb.planar(pts, 3), rb.planar(nrm, 3), K, M.S0, seqs, None, N, D, limit, BG, 1, "all")
    got = _bake(ds, s, W, H, K, N, D, limit, side=side, jitter=False)
    assert got.radiance.shape == (H, W, 3) and want.n_rays.min() >= K
    _same_map(got, want.radiance, want.n_rays, f"{name} shape {s} {W}x{H} K={K} N={N} D={D} limit={limit} side={side}")


# ---- 3. jitter mode ---------------------------------------------------------------------------------------------------------------
_stand_in = {}


def _diffuse_stand_in(ds, name):
    """A shape index whose scatter query is ``DiffuseBRDF.scatter_ray`` at the record's own point and normal (a diffuse shape
    whose pigment is not black at (0, 0): the scatter goes on)."""
    if name not in _stand_in:
        flat = R.world(name)[0]
        one = np.zeros((1, 3))
        _stand_in[name] = next(i for i in range(flat.n_shapes)
                               if (lambda sc: sc.status[0] == 1 and sc.rays[6, 0] == 1.0e-3)(
                                   ds.scatter([i], one, one + 1.0, np.zeros((1, 2)), one + 1.0, rb.pcg_streams(M.S0, [M.Q0]), False, "none")))
    return _stand_in[name]


@pytest.mark.parametrize("K,N,D,limit", [(4, 1, 3, 2), (3, 2, 2, 1), (70, 1, 2, 0)])
@pytest.mark.parametrize("name,s", SHAPES, ids=IDS)
def test_jitter_mode_equals_the_device_chain_bit_for_bit(scene_of, orc, name, s, K, N, D, limit):
    """The jittered (u, v) from ``oracle.Pcg`` draws on the host (exact arithmetic), then what the libraries there already were do
    with them: ``surface_points``, the scatter query with the generators two draws in, the radiance query, the host's ordered mean."""
    W, H = M.MAP_W, M.MAP_H
    ds = scene_of(name)
    uv, seqs = M.sample_uv(orc, W, H, K)
    n = W * H * K
    pts, nrm = rb.WorldQueries(ds).surface_points(s, uv.reshape(n, 2))
    pcg = rb.pcg_streams(M.S0, [q for row in seqs for q in row], skip=2)
    stand_in = np.full(n, _diffuse_stand_in(ds, name), np.int32)
    sc = ds.scatter(stand_in, pts, nrm, np.zeros((n, 2)), nrm, pcg, False, "none")
    assert np.all(sc.status == 1) and np.all(sc.rays[6] == 1.0e-3) and np.all(sc.rays[7] == np.inf)
    rad = ds.radiance(np.ascontiguousarray(sc.rays), np.ascontiguousarray(sc.pcg), N, D, limit, BG, 1, "count")
    want = G.ordered_mean(np.asarray(rad.radiance).reshape(W * H, K, 3))
    count = np.asarray(rad.n_rays).reshape(W * H, K).sum(axis=1, dtype=np.uint64)
    got = _bake(ds, s, W, H, K, N, D, limit)
    assert len(np.unique(uv.reshape(n, 2), axis=0)) == n and count.min() >= K
    _same_map(got, want, count, f"{name} shape {s} K={K} N={N} D={D} limit={limit}")


@pytest.mark.parametrize("K,N,D,limit", M.ORACLE_CASES)
@pytest.mark.parametrize("name,s", SHAPES, ids=IDS)
def test_jitter_mode_equals_the_oracles_composition(scene_of, orc, name, s, K, N, D, limit):
    want = M.expected(orc, name, s, K, N, D, limit)
    got = _bake(scene_of(name), s, M.MAP_W, M.MAP_H, K, N, D, limit)
    bad, worst = M.outliers(got, want)
    same = G.same_bits(np.asarray(got.radiance).reshape(-1, 3), want["radiance"])
    print(f"bake {name} shape {s} 7x5 K={K} N={N} D={D} limit={limit}: {int(want['count'].sum())} traced, outliers {int(bad.sum())}, "
          f"worst relative error {worst:.3g}, bit-identical {same.mean():.1%}")
    assert want["count"].min() >= K
    assert bad.sum() <= MAX_OUTLIERS, f"{int(bad.sum())} outlier texels ({np.flatnonzero(bad)[:8].tolist()}), worst {worst:.3g}"


# ---- 4. launch shape and tiling ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2_map(scene_of):
    """16 x 16 at K = 5, N = 2 of c2's second diffuse shape: 1280 samples, five workgroups"""
    s = M.diffuse_shapes("c2")[1]
    full = _bake(scene_of("c2"), s, 16, 16, 5, 2, 2, 1)
    assert len(np.unique(full.radiance.reshape(-1, 3), axis=0)) > 100 and full.n_rays.min() >= 5
    return s, full


def test_a_launch_capped_at_one_workgroup_gives_the_same_bits(scene_of, c2_map, monkeypatch):
    s, full = c2_map
    ds = scene_of("c2")
    planes = 16 * 16 * 5 * 32
    assert ds.bake_workspace_bytes(16, 16, 5, 2, 2, 1) == 1280 * 20 * 1 * 8 + planes
    monkeypatch.setenv("PTRACE_BAKE_LANES", "256")
    assert ds.bake_workspace_bytes(16, 16, 5, 2, 2, 1) == 256 * 20 * 1 * 8 + planes
    assert ds.bake_workspace_bytes(16, 16, 5, 1, 4, 1, window=(3, 0, 1, 16)) == 256 * 6 * 3 * 8 + 16 * 5 * 32
    capped = _bake(ds, s, 16, 16, 5, 2, 2, 1)
    monkeypatch.delenv("PTRACE_BAKE_LANES")
    assert capped.buffer.tobytes() == full.buffer.tobytes()


def test_a_map_baked_in_four_windows_is_the_map_baked_whole(scene_of, c2_map):
    s, full = c2_map
    ds = scene_of("c2")
    windows = ((0, 0, 15, 9), (15, 0, 1, 16), (0, 9, 7, 7), (7, 9, 8, 7))  # (col0, row0, w, h); the second is a single column
    covered = np.zeros((16, 16), int)
    for col0, row0, w, h in windows:
        part = _bake(ds, s, 16, 16, 5, 2, 2, 1, window=(col0, row0, w, h))
        assert part.radiance.shape == (h, w, 3)
        _same_map(part, full.radiance[row0: row0 + h, col0: col0 + w], full.n_rays[row0: row0 + h, col0: col0 + w], f"window {(col0, row0, w, h)}")
        covered[row0: row0 + h, col0: col0 + w] += 1
    assert np.all(covered == 1)


def test_a_bake_that_stays_in_hbm_and_the_count_channel(dev, scene_of, c2_map):
    """``bake(device=True)`` with a caller-owned workspace, output buffer and stream, twice into the same buffers: byte for byte the
    host form.  Without PT_BAKE_COUNT the buffer has three planes, and they are the same."""
    from pytracer_amd import _bake_lib, _lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    s, full = c2_map
    ds = scene_of("c2")
    L = _bake_lib.lib()
    st = Stream()
    try:
        need = ds.bake_workspace_bytes(16, 16, 5, 2, 2, 1)
        ws = DeviceBuffer((need,), np.uint8)
        mine = DeviceBuffer((rb.bake_bytes(256, rb.BAKE_ALL),), np.uint8)
        for turn in range(2):
            out = _bake(ds, s, 16, 16, 5, 2, 2, 1, device=True, stream=st, out=mine, workspace=ws)
            assert out is mine
            assert mine.numpy().tobytes() == full.buffer.tobytes(), f"turn {turn}: the bake in HBM differs from the bake through the host form"
        bare = _bake(ds, s, 16, 16, 5, 2, 2, 1, channels="none")
        assert bare.buffer.nbytes == L.pt_rays_bake_bytes(256, 0) == 24 * 256 and full.buffer.nbytes == L.pt_rays_bake_bytes(256, 1) == 32 * 256
        assert bare.buffer.tobytes() == full.buffer[: 24 * 256].tobytes() and not bare.has("count")
        assert L.pt_rays_bake_plane_offset(256, 0, rb.BAKE_COUNT, 0) < 0 and L.pt_rays_bake_plane_offset(256, 1, rb.BAKE_COUNT, 0) == 24 * 256
        small = _bake(ds, s, 16, 16, 5, 2, 2, 1, channels="none", device=True, stream=st)  # the library's own workspace, three planes
        assert small.numpy()[: 24 * 256].tobytes() == bare.buffer.tobytes()
        for kw in (dict(workspace=DeviceBuffer((need - 8,), np.uint8), out=mine), dict(workspace=ws, out=DeviceBuffer((mine.nbytes - 8,), np.uint8))):
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE"):
                _bake(ds, s, 16, 16, 5, 2, 2, 1, device=True, stream=st, **kw)
        with pytest.raises(ValueError, match="device=True"):
            _bake(ds, s, 16, 16, 5, 2, 2, 1, stream=st)
    finally:
        st.close()


# ---- 5. depths --------------------------------------------------------------------------------------------------------------------
def test_depths_at_and_beyond_max_depth(scene_of, orc):
    from pytracer_amd import _lib

    name, s = "pigments", M.diffuse_shapes("pigments")[1]
    ds = scene_of(name)
    K, N, D, limit = 3, 2, 2, 1
    deep = _bake(ds, s, 7, 5, K, N, D, limit, depth=D + 1)
    assert not deep.buffer.any()
    want = M.expected(orc, name, s, K, N, D, limit, depth0=D)
    got = _bake(ds, s, 7, 5, K, N, D, limit, depth=D)
    assert np.all(want["count"] == K) and _bits(np.asarray(got.n_rays).reshape(-1), want["count"])
    bad, worst = M.outliers(got, want)
    assert bad.sum() <= MAX_OUTLIERS, (int(bad.sum()), worst)
    with pytest.raises(_lib.PtraceError, match="PT_ERR_UNSUPPORTED.*64 levels"):
        _bake(ds, s, 7, 5, K, N, 66, limit, depth=1)
    assert _bake(ds, s, 2, 2, 1, 1, 65, 3, depth=1).radiance.shape == (2, 2, 3)  # 64 levels
    for kw, word in ((dict(side=0), "side"), (dict(window=(0, 0, 8, 5)), "rectangle"), (dict(K=0), "samples")):
        args = dict(K=K, side=1, window=None)
        args.update(kw)
        with pytest.raises(_lib.PtraceError, match=f"PT_ERR_INVALID.*{word}"):
            _bake(ds, s, 7, 5, args["K"], N, D, limit, side=args["side"], window=args["window"])
    with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*shapes"):
        _bake(ds, R.world(name)[0].n_shapes, 7, 5, K, N, D, limit)


# ---- 6. furnace -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,depth", [(1, 4, 1), (2, 3, 0), (1, 2, 2)])
def test_a_furnace_seen_from_inside(dev, N, D, depth):
    """A unit sphere seen from inside, uniform emission Le and diffuse albedo rho < 1, no roulette: every hemisphere ray meets the
    sphere again, so every sample -- and every texel -- is ``Le * sum_{d = 0}^{D - depth0} rho^d``."""
    from pytracer_amd import flatten
    from pytracer_amd import hostmodel as hm

    le, rho = (0.7, 0.5, 1.25), (0.5, 0.25, 0.8)
    world = hm.World()
    world.add_shape(hm.Sphere(hm.Transformation(), hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(*rho))), hm.UniformPigment(hm.Color(*le)))))
    with dev.DeviceScene(flatten.flatten_world(world)) as ds:
        got = ds.bake(0, 7, 5, 8, -1, True, None, M.S0, M.Q0, N, D, D + 5, BG, depth, "all")
    want = np.array([e * sum(r ** d for d in range(D - depth + 1)) for e, r in zip(le, rho)])
    err = np.abs(got.radiance - want) / want
    print(f"furnace N={N} D={D} depth={depth}: worst relative error {err.max():.3g}")
    assert err.max() <= 1e-12
    assert np.all(got.n_rays == 8 * sum(N ** d for d in range(D - depth + 1)))


# ---- 7. the baked frame -----------------------------------------------------------------------------------------------------------
def test_the_flat_frame_of_the_baked_world(dev, orc):
    """``outgoing_map`` for the two planes of ``demo``, ``baked_world``, then ``FlatRenderer`` at 48 x 36 through ``GpuImageTracer``:
    the oracle's frame of the baked scene bit for bit, and every pixel whose hit lies on a baked shape is the texel under it."""
    from pytracer_amd import flatten, scenes
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.tracer import GpuImageTracer

    world, camera = R.host_world("demo")
    sizes = {0: (16, 8), 1: (32, 32)}  # shape -> (W, H)
    with dev.DeviceScene(flatten.flatten_world(world)) as ds:
        wq = rb.WorldQueries(ds)
        maps = {i: wq.outgoing_map(i, w, h, 8, init_state=M.S0, num_of_rays=1, max_depth=3, background=BG) for i, (w, h) in sizes.items()}
        with pytest.raises(ValueError, match="DiffuseBRDF"):
            wq.outgoing_map(2, 4, 4, 2)
    assert maps[1].shape == (32, 32, 3) and len(np.unique(maps[1].reshape(-1, 3), axis=0)) > 100 and np.isfinite(maps[1]).all()
    baked = scenes.baked_world(world, maps)
    W, H = 48, 36
    image = hm.HdrImage(W, H)
    tracer = GpuImageTracer(image, camera, samples_per_side=0)
    try:
        tracer.fire_all_rays(hm.FlatRenderer(baked))
    finally:
        tracer.close()
    flat, cam = flatten.flatten_world(baked), flatten.flatten_camera(camera)
    par = flatten.renderer_params(hm.FlatRenderer(baked), W, H, samples_per_side=0)
    want, _ = orc.render(flat, cam, par, sqr_mode=orc.SQR_MUL)
    got = np.asarray(image.array)
    assert got.tobytes() == np.ascontiguousarray(want, dtype=np.float64).tobytes()
    seen = {0: 0, 1: 0}
    for row in range(H):
        for col in range(W):
            hit = orc.world_intersect(flat, orc.tracer_fire_ray(cam, W, H, col, row))
            if hit is None or int(hit[9]) not in maps:
                continue
            m = maps[int(hit[9])]
            h, w = m.shape[:2]
            assert np.array_equal(got[row, col], m[min(int(hit[8] * h), h - 1), min(int(hit[7] * w), w - 1)]), (row, col, hit)
            seen[int(hit[9])] += 1
    assert seen[0] > 100 and seen[1] > 100
