"""Radiance queries on the device (include/ptrace_radiance.h, libptrace_radiance.so): ``PathTracer.__call__`` for batches of a
caller's own rays, against the CPU oracle in its ``x * x`` mode (tests/radiance_batches.py), against the fused path tracer of
libptrace.so and the breadth-first ``PathTracerShader``, and against themselves across batch sizes, channels and entry points.

Expected agreement.  Where no libm call is involved -- the world of mirrors with uniform pigments, rays that miss, entry rays
deeper than ``max_depth`` -- radiance, generator and ray count are compared bit for bit.  A diffuse bounce holds ocml's
sin / cos against glibc's: radiance to ``TOL = 1e-5`` relative per channel, and a ray beyond it, or with another count or final
state (a last-ulp difference may flip a silhouette, checker or roulette decision behind the bounce), is an outlier, of which a
case may hold ONE -- the cap tests/test_gpu_parity.py applies to whole frames.  Device against device: byte for byte."""
import numpy as np
import pytest

from pytracer_amd import abi, rays as rb, shaders
from pytracer_amd import hostmodel as hm

from . import radiance_batches as R
from . import surface_batches as S

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1001)
BG = R.BACKGROUND
MAX_OUTLIERS = 1


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


def _query(ds, rays, pcg, N, D, limit, depth=0, channels="all", **kw):
    return ds.radiance(rb.ray_planes(rays), pcg, N, D, limit, BG, depth, channels, **kw)


def _same(got, want, label):
    """radiance, generator and count bit for bit"""
    bad = ~np.all(np.ascontiguousarray(got.radiance).view(np.uint64) == np.ascontiguousarray(want["radiance"]).view(np.uint64), axis=1)
    assert not bad.any(), f"{label}: radiance differs in {int(bad.sum())} of {got.n} rays (first: {int(np.flatnonzero(bad)[0])})"
    assert _bits(got.pcg, want["pcg"]), f"{label}: generators differ in {int(np.any(got.pcg != want['pcg'], axis=0).sum())} rays"
    assert _bits(got.n_rays, want["count"]), f"{label}: ray counts differ in {int((got.n_rays != want['count']).sum())} rays"


# ---- 1. bit for bit against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,limit", [(1, 5, 0), (3, 3, 1)])
def test_mirrors_equal_the_oracle_bit_for_bit(scene_of, orc, N, D, limit):
    b = R.batch(orc, "mirrors", N, D, limit)
    got = _query(scene_of("mirrors"), b["rays"], b["pcg"], N, D, limit)
    w = b["want"]
    assert w["count"].max() >= (D + 1 if N == 1 else 20) and len(np.unique(w["radiance"], axis=0)) > 100 and np.any(w["pcg"][0] != b["pcg"][0])
    _same(got, w, f"mirrors N={N} D={D} limit={limit}")


@pytest.mark.parametrize("name", R.WORLDS)
def test_misses_and_rays_beyond_max_depth(scene_of, orc, name):
    """A ray that hits nothing: the background, one ray counted, the generator untouched.  ``depth = max_depth + 1``: black, no
    query, no draw, count 0 -- for every ray of the batch."""
    N, D, limit = 3, 2, 0
    b = R.batch(orc, name, N, D, limit)
    ds = scene_of(name)
    rec = R.records(orc, name)["rec"]
    miss = ~np.asarray(rec.hit)[R.rows(orc, name)]
    if name in ("demo", "roulette4"):
        assert miss.sum() > 100
    if miss.any():
        got = _query(ds, b["rays"][miss], b["pcg"][:, miss], N, D, limit)
        assert np.all(got.radiance == np.array(BG)) and np.all(got.n_rays == 1) and _bits(got.pcg, b["pcg"][:, miss])
        _same(got, {k: (v[:, miss] if k == "pcg" else v[miss]) for k, v in b["want"].items()}, f"{name}: misses")
    deep = _query(ds, b["rays"], b["pcg"], N, D, limit, depth=D + 1)
    assert not deep.radiance.any() and not np.signbit(deep.radiance).any() and not deep.n_rays.any() and _bits(deep.pcg, b["pcg"])
    _same(deep, R.batch(orc, name, N, D, limit, D + 1)["want"], f"{name}: depth = max_depth + 1")


@pytest.mark.parametrize("name", R.WORLDS)
def test_entry_rays_at_max_depth(scene_of, orc, name):
    """``depth = max_depth``: one query per ray; a diffuse hit with ``lum > 0`` still draws ``2 * num_of_rays`` numbers for children
    that are black without a query.  The roulette is off (``limit > max_depth``), so the draw counts are the scatter's alone."""
    from pytracer_amd.hostmodel import pcg_advance

    N, D, limit = 3, 2, 9
    b = R.batch(orc, name, N, D, limit, D)
    got = _query(scene_of(name), b["rays"], b["pcg"], N, D, limit, depth=D)
    w = b["want"]
    assert np.all(got.n_rays == 1) and _bits(got.n_rays, w["count"])
    assert _bits(got.pcg, w["pcg"]), f"{name}: generators differ in {int(np.any(got.pcg != w['pcg'], axis=0).sum())} rays"
    bad, worst = R.outliers(got, w)
    # (uniform pigments: no libm call at all; elsewhere ocml's atan2 / acos may move a hit across a checker's or a texel's edge)
    assert bad.sum() <= (0 if name in ("mirrors", "roulette4") else MAX_OUTLIERS), (name, int(bad.sum()), worst)
    # the draws, counted independently of the oracle's recursion: 2 N where its record is a diffuse hit with lum > 0, else none
    flat = R.world(name)[0]
    rec, k = R.records(orc, name)["rec"], R.rows(orc, name)
    draws = np.zeros(got.n, np.int64)
    for j, i in enumerate(range(k.start, k.stop)):
        if rec.hit[i]:
            s = int(rec.shape_index[i])
            lum = float(np.max(orc.pigment(flat, s, False, float(rec.uv[i, 0]), float(rec.uv[i, 1]))))
            draws[j] = 2 * N if lum > 0.0 and int(flat.brdf_kind[s]) == abi.BRDF_DIFFUSE else 0
    want_state = np.array([pcg_advance(int(b["pcg"][0, j]), int(b["pcg"][1, j]), int(draws[j])) for j in range(got.n)], dtype=np.uint64)
    assert _bits(got.pcg[0], want_state)
    if name != "mirrors":
        assert (draws > 0).sum() > 50


# ---- 2. against the oracle with diffuse bounces ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,limit", [(1, 3, 2), (2, 2, 1), (3, 3, 0), (10, 3, 3), (70, 1, 3)])
@pytest.mark.parametrize("name", R.WORLDS)
def test_radiance_equals_the_oracle(scene_of, orc, name, N, D, limit):
    b = R.batch(orc, name, N, D, limit)
    assert b["rays"].shape[0] <= 1001
    got = _query(scene_of(name), b["rays"], b["pcg"], N, D, limit)
    bad, worst = R.outliers(got, b["want"])
    same = np.all(np.ascontiguousarray(got.radiance).view(np.uint64) == np.ascontiguousarray(b["want"]["radiance"]).view(np.uint64), axis=1)
    print(f"radiance {name} N={N} D={D} limit={limit}: {got.n} rays, {int(b['want']['count'].sum())} traced, outliers {int(bad.sum())}, "
          f"worst relative error {worst:.3g}, bit-identical {same.mean():.1%}")
    assert bad.sum() <= MAX_OUTLIERS, f"{name} N={N} D={D} limit={limit}: {int(bad.sum())} outliers (rays {np.flatnonzero(bad)[:8].tolist()}), worst {worst:.3g}"


# ---- 3. device against device, byte for byte -------------------------------------------------------------------------------------
FRAMES = [("demo", 40, 30), ("c2", 48, 27)]


@pytest.mark.parametrize("S_", [0, 2])
@pytest.mark.parametrize("name,W,H", FRAMES)
def test_one_ray_per_hit_equals_the_breadth_first_shader(dev, name, W, H, S_):
    """``path_radiance`` on a frame's own primary rays against ``PathTracerShader`` over that frame (trace, then per depth scatter
    and trace, the sums in numpy), sample by sample, before the reduction."""
    from pytracer_amd.tracer import GpuImageTracer

    world, camera = S.host_world(name)
    assert (W, H) == S.WORLDS[name]
    bg = hm.Color(*BG)
    tracer = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode="sample")
    try:
        frame = tracer.fire_all_hits(world, abi.HIT_ALL)
        old = shaders.PathTracerShader(world, tracer, bg, hm.PCG(45, 54), 1, 3, 2)
        want = np.asarray(old.shade_hits(frame))
        res = tracer.world_queries(world).path_radiance(np.asarray(frame.ray_origin).reshape(-1, 3), old.sample_streams(frame),
                                                        np.asarray(frame.ray_dir).reshape(-1, 3), 1, 3, 2, bg, 0, "all")
        got = np.asarray(res.radiance).reshape(want.shape)
        assert want.shape == (max(S_, 1) ** 2, H, W, 3) and len(np.unique(want.reshape(-1, 3), axis=0)) > 8
        assert _bits(got, want), f"{int(np.any(got != want, axis=-1).sum())} of {want[..., 0].size} samples differ"
    finally:
        tracer.close()


@pytest.mark.parametrize("N,D", [(1, 3), (2, 2), (10, 3)])
@pytest.mark.parametrize("name,W,H", FRAMES)
def test_the_shader_route_equals_the_fused_path_tracer(dev, name, W, H, N, D):
    """``fire_all_rays(PathRadianceShader(...))`` against ``fire_all_rays(PathTracer(...))`` under ``pcg_mode="sample"``: both
    routes run the same device functions under the same flags, on the same rays and the same generators."""
    from pytracer_amd.tracer import GpuImageTracer

    world, camera = S.host_world(name)
    bg = hm.Color(*BG)
    for S_ in (0, 2):
        fused = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode="sample")
        mine = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode="sample")
        try:
            fused.fire_all_rays(hm.PathTracer(world, bg, hm.PCG(45, 54), num_of_rays=N, max_depth=D, russian_roulette_limit=2))
            shader = shaders.PathRadianceShader(world, mine, bg, hm.PCG(45, 54), num_of_rays=N, max_depth=D, russian_roulette_limit=2)
            mine.fire_all_rays(shader)
            assert fused.last_path == "device" and mine.last_path == "device-hits"
            a, b = np.asarray(fused.image.array), np.asarray(mine.image.array)
            assert a.shape == (H, W, 3) and len(np.unique(a.reshape(-1, 3), axis=0)) > 8
            assert _bits(b, a), f"S={S_}: {int(np.any(a != b, axis=-1).sum())} of {W * H} pixels differ"
            counted, fused_rays = int(shader.last_radiance.n_rays.sum()), int(fused.last_stats.n_rays)
            print(f"{name} N={N} D={D} S={S_}: {counted} rays by the RAD_COUNT plane, {fused_rays} by the fused kernels")
            assert abs(counted - fused_rays) <= 8, (S_, counted, fused_rays)
        finally:
            fused.close()
            mine.close()


def test_a_query_that_stays_in_hbm(dev, orc):
    """``radiance(device=True)`` on a torch tensor of rays with a caller-owned workspace, output buffer and stream: byte for byte the
    host route.  An undersized workspace or output: PT_ERR_SIZE before anything runs."""
    import torch

    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    N, D, limit = 2, 2, 1
    b = R.batch(orc, "demo", N, D, limit)
    n = b["rays"].shape[0]
    assert n == 1001
    block = np.ascontiguousarray(rb.ray_planes(b["rays"]))
    ds = dev.DeviceScene(R.world("demo")[0])
    st = Stream()
    try:
        host = ds.radiance(block, b["pcg"], N, D, limit, BG)
        rays_dev = torch.from_numpy(block).cuda()
        pcg_dev = torch.from_numpy(np.array(b["pcg"]).view(np.int64)).cuda()
        torch.cuda.synchronize()
        need = ds.radiance_workspace_bytes(n, N, D)
        assert need > 0 and need % (256 * 20 * 8) == 0
        ws = DeviceBuffer((need,), np.uint8)
        mine = DeviceBuffer((rb.radiance_bytes(n, rb.RAD_ALL),), np.uint8)
        out = ds.radiance(rays_dev, pcg_dev, N, D, limit, BG, device=True, stream=st, out=mine, workspace=ws)
        assert out is mine
        assert mine.numpy().tobytes() == host.buffer.tobytes(), "the query in HBM differs from the query through host arrays"
        # raw addresses, a pair of generator planes, a selected channel, the library's own workspace
        some = ds.radiance(rays_dev.data_ptr(), (pcg_dev.data_ptr(), pcg_dev.data_ptr() + 8 * n), N, D, limit, BG, channels="count",
                           device=True, stream=st, n=n)
        got = rb.RayRadiance(some.numpy(), n, "count")
        assert _bits(got.radiance, host.radiance) and _bits(got.n_rays, host.n_rays)
        for kw in (dict(workspace=DeviceBuffer((need - 8,), np.uint8), out=mine), dict(workspace=ws, out=DeviceBuffer((mine.nbytes - 8,), np.uint8))):
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE"):
                ds.radiance(rays_dev, pcg_dev, N, D, limit, BG, device=True, stream=st, **kw)
        with pytest.raises(ValueError, match="n="):
            ds.radiance(rays_dev.data_ptr(), pcg_dev, N, D, limit, BG, device=True)
        with pytest.raises(ValueError, match="device=True"):
            ds.radiance(block, b["pcg"], N, D, limit, BG, stream=st)
    finally:
        st.close()
        ds.close()


# ---- 4. batch sizes --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2_full(scene_of, orc):
    b = R.batch(orc, "c2", 2, 2, 1)
    return b, _query(scene_of("c2"), b["rays"], b["pcg"], 2, 2, 1)


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_around_the_wave_and_the_block(scene_of, c2_full, n):
    b, full = c2_full
    start = (b["rays"].shape[0] - n) // 2  # (across the boundary between primary rays and bounces)
    k = slice(start, start + n)
    got = _query(scene_of("c2"), b["rays"][k], b["pcg"][:, k], 2, 2, 1)
    assert got.nbytes == 48 * n == got.buffer.nbytes
    assert _bits(got.radiance, full.radiance[k]) and _bits(got.pcg, full.pcg[:, k]) and _bits(got.n_rays, full.n_rays[k])


def test_a_batch_larger_than_the_resident_lanes(scene_of, c2_full, monkeypatch):
    """PTRACE_RADIANCE_LANES caps the lanes of a launch (include/ptrace_radiance.h): at 256 every wave of the one workgroup walks
    four sets of 64 rays one after the other (the last one partly idle), on one workgroup's worth of workspace."""
    b, full = c2_full
    ds = scene_of("c2")
    n = b["rays"].shape[0]
    monkeypatch.setenv("PTRACE_RADIANCE_LANES", "300")  # (rounded down to 256)
    assert ds.radiance_workspace_bytes(n, 2, 2) == 256 * 20 * 2 * 8 and ds.radiance_workspace_bytes(n, 1, 3) == 256 * 6 * 3 * 8
    got = _query(ds, b["rays"], b["pcg"], 2, 2, 1)
    monkeypatch.delenv("PTRACE_RADIANCE_LANES")
    assert n == 1001 and ds.radiance_workspace_bytes(n, 2, 2) == 1024 * 20 * 2 * 8
    assert got.buffer.tobytes() == full.buffer.tobytes()


# ---- 5. channels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [0, rb.RAD_PCG, rb.RAD_COUNT, rb.RAD_ALL])
def test_every_channel_combination_at_the_librarys_offsets(scene_of, orc, channels):
    from pytracer_amd import _radiance_lib

    L = _radiance_lib.lib()
    b = R.batch(orc, "pigments", 2, 2, 1)
    n = 257
    ds = scene_of("pigments")
    full = _query(ds, b["rays"][:n], b["pcg"][:, :n], 2, 2, 1)
    got = _query(ds, b["rays"][:n], b["pcg"][:, :n], 2, 2, 1, channels=channels)
    assert got.buffer.nbytes == L.pt_rays_radiance_bytes(n, channels) == got.nbytes
    plane = lambda sel, comp, dt=np.float64: got.buffer[L.pt_rays_radiance_plane_offset(n, channels, sel, comp):][: 8 * n].view(dt)  # noqa: E731
    for comp in range(3):
        assert _bits(plane(0, comp), np.ascontiguousarray(full.radiance[:, comp]))
    if channels & rb.RAD_PCG:
        assert _bits(plane(rb.RAD_PCG, 0, np.uint64), full.pcg[0]) and _bits(plane(rb.RAD_PCG, 1, np.uint64), full.pcg[1])
    else:
        assert L.pt_rays_radiance_plane_offset(n, channels, rb.RAD_PCG, 0) < 0 and not got.has("pcg")
    if channels & rb.RAD_COUNT:
        assert _bits(plane(rb.RAD_COUNT, 0, np.uint64), full.n_rays)
    else:
        assert L.pt_rays_radiance_plane_offset(n, channels, rb.RAD_COUNT, 0) < 0 and not got.has("count")
    bad, _ = R.outliers(full, {k: (v[:, :n] if k == "pcg" else v[:n]) for k, v in b["want"].items()})
    assert bad.sum() <= MAX_OUTLIERS


# ---- 6. rays nobody vouches for --------------------------------------------------------------------------------------------------
def _hostile(rays):
    """Every eighth ray replaced, in turn, by a ray of NaNs, an infinite origin, an infinite direction, a zero direction and the
    same ray looking backwards (tmin < 0) -> (rays, {kind: rows})"""
    out = np.array(rays)
    rows = np.arange(3, out.shape[0], 8)
    kinds = {"nan": rows[0::5], "inf_origin": rows[1::5], "inf_dir": rows[2::5], "zero_dir": rows[3::5], "behind": rows[4::5]}
    out[kinds["nan"]] = np.nan
    out[kinds["inf_origin"], 0] = np.inf
    out[kinds["inf_dir"], 4] = -np.inf
    out[kinds["zero_dir"], 3:6] = 0.0
    out[kinds["behind"], 6] = -1.0e3
    return out, kinds, rows


@pytest.mark.parametrize("name,N,D,limit", [("c2", 2, 2, 1), ("mirrors", 3, 3, 1)])
def test_rays_nobody_vouches_for(scene_of, orc, name, N, D, limit):
    b = R.batch(orc, name, N, D, limit)
    ds = scene_of(name)
    clean = _query(ds, b["rays"], b["pcg"], N, D, limit)
    rays, kinds, rows = _hostile(b["rays"])
    got = _query(ds, rays, b["pcg"], N, D, limit)  # (the call returns: the walk ends by its counters)
    others = np.setdiff1d(np.arange(rays.shape[0]), rows)
    assert _bits(got.radiance[others], clean.radiance[others]) and _bits(got.pcg[:, others], clean.pcg[:, others])
    assert _bits(got.n_rays[others], clean.n_rays[others])
    for kind in ("nan", "inf_origin", "zero_dir"):  # nothing is hit: the background, one query, no draw
        k = kinds[kind]
        assert np.all(got.radiance[k] == np.array(BG)) and np.all(got.n_rays[k] == 1) and _bits(got.pcg[:, k], b["pcg"][:, k]), kind
    assert np.all(got.n_rays[kinds["inf_dir"]] >= 1) and np.all(got.n_rays <= sum(N ** d for d in range(D + 1)))
    # tmin < 0: the roots behind the origin count, as the reference's test tmin < t < tmax has it
    k = kinds["behind"]
    want = R.expected(orc, R.world(name)[0], rays[k], b["pcg"][:, k], N, D, limit)
    sub = rb.RayRadiance(np.concatenate([np.ascontiguousarray(got.radiance[k].T).view(np.uint8).reshape(-1), np.ascontiguousarray(got.pcg[:, k]).view(np.uint8).reshape(-1),
                                         np.ascontiguousarray(got.n_rays[k]).view(np.uint8).reshape(-1)]), k.size, "all")
    assert np.any(want["radiance"] != clean.radiance[k]) and k.size > 20  # (looking backwards changes what is seen)
    if name == "mirrors":
        _same(sub, want, "mirrors: tmin < 0")
    else:
        bad, worst = R.outliers(sub, want)
        assert bad.sum() <= MAX_OUTLIERS, (int(bad.sum()), worst)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(scene_of, orc):
    from pytracer_amd import _lib, _radiance_lib

    b = R.batch(orc, "c2", 2, 2, 1)
    ds = scene_of("c2")
    rays, pcg = b["rays"][:65], b["pcg"][:, :65]
    for kw, code, word in ((dict(N=0), "PT_ERR_INVALID", "num_of_rays"), (dict(D=65), "PT_ERR_UNSUPPORTED", "fused renderer"),
                           (dict(D=70, depth=5), "PT_ERR_UNSUPPORTED", "4096"), (dict(depth=-1), "PT_ERR_INVALID", "depth"),
                           (dict(D=-1), "PT_ERR_INVALID", "max_depth")):
        args = dict(N=2, D=2, limit=1, depth=0)
        args.update(kw)
        with pytest.raises(_lib.PtraceError, match=f"{code}.*{word}"):
            _query(ds, rays, pcg, args["N"], args["D"], args["limit"], args["depth"])
    assert _query(ds, rays, pcg, 1, 64, 60).n == 65 and _query(ds, rays, pcg, 1, 70, 3, depth=6).n == 65  # 64 levels: accepted
    with pytest.raises(ValueError, match="channels"):
        _query(ds, rays, pcg, 2, 2, 1, channels=4)
    L, block = _radiance_lib.lib(), ds.kernel_args()
    par = _radiance_lib.params(2, 2, 1, 0, BG)
    out = np.zeros(rb.radiance_bytes(65, 3), np.uint8)
    import ctypes as C

    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    planes = np.ascontiguousarray(rb.ray_planes(rays))
    st, inc = np.ascontiguousarray(pcg[0]), np.ascontiguousarray(pcg[1])
    assert L.pt_rays_radiance(0, block, len(block), None, p(st), p(inc), 65, C.byref(par), 3, p(out), out.nbytes) == -1  # null planes
    assert L.pt_rays_radiance(0, block, len(block), p(planes), None, p(inc), 65, C.byref(par), 3, p(out), out.nbytes) == -1
    assert L.pt_rays_radiance(0, block, len(block) - 8, p(planes), p(st), p(inc), 65, C.byref(par), 3, p(out), out.nbytes) == -1  # another build's block
    assert "one build" in _radiance_lib.last_error()
    assert L.pt_rays_radiance(0, block, len(block), p(planes), p(st), p(inc), 0, C.byref(par), 3, None, 0) == 0  # n = 0: nothing launched
    assert L.pt_rays_radiance_device(0, block, len(block), None, p(planes), p(st), p(inc), 65, C.byref(par), 3, None, 0, p(out), out.nbytes, None) == -1
    assert "workspace" in _radiance_lib.last_error()
    assert not out.any()  # nothing ran
