"""Ray batches on the device (include/ptrace_rays.h, libptrace_rays.so): ``World.ray_intersection`` and the test of
``World.is_point_visible`` for a caller's own rays, against the CPU oracle in its ``x * x`` mode, against the frames and the
exhaustive probe of libptrace.so, and against themselves across channels, batch sizes, streams and entry points.

Expected agreement: shape index, t, point and normal bit for bit (no transcendental function is involved); a plane's (u, v)
bit for bit (floor only); a sphere's (u, v) within 1e-11 relative -- ocml's atan2 / acos against glibc's, the project's bound
(tests/test_gpu_probes.py:65, tests/test_gpu_hits.py).  Device against device: byte for byte."""
import ctypes as C

import numpy as np
import pytest

from pytracer_amd import abi, flatten, rays as rb, scenes
from pytracer_amd import hostmodel as hm

from . import ray_batches as B

pytestmark = pytest.mark.gpu
ALL = rb.RAY_CHANNELS


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
            open_[name] = dev.DeviceScene(B.world(name)[0])
        return open_[name]

    yield get
    for ds in open_.values():
        ds.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_planes(got, want):
    for name, plane in want.planes().items():
        assert _bits(got.planes()[name], plane), name


# ---- 1. closest hit against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", B.BATCHES)
@pytest.mark.parametrize("name", list(B.WORLDS))
def test_closest_hit_equals_the_oracle(scene_of, orc, name, batch):
    b = B.batches(orc, name)[batch]
    flat = B.world(name)[0]
    got = scene_of(name).trace_rays(rb.ray_planes(b["rays"]))
    want = b["want"]
    assert np.array_equal(got.shape_index, want.shape_index), f"{int((got.shape_index != want.shape_index).sum())} rays: hit / miss or another shape"
    hit = want.hit
    assert hit.any()
    assert _bits(got.t, want.t) and np.all(np.isposinf(got.t[~hit]))
    assert _bits(got.point, want.point) and _bits(got.normal, want.normal)
    plane = hit & (np.asarray(flat.kind)[np.where(hit, want.shape_index, 0)] == abi.SHAPE_PLANE)
    assert _bits(got.uv[plane], want.uv[plane]) and _bits(got.uv[~hit], want.uv[~hit])  # floor only / zeros
    a, w = got.uv[hit & ~plane], want.uv[hit & ~plane]
    err = np.abs(a - w) / np.maximum(np.maximum(np.abs(a), np.abs(w)), 1e-300)
    print(f"{name} {batch}: {int(hit.sum())} hits of {hit.size}, sphere uv max rel err {err.max() if err.size else 0:.3g}")
    assert B.uv_close(a, w)


# ---- 2. a hit frame's own rays fed back --------------------------------------------------------------------------------------
def _ortho(w, h):
    return flatten.flatten_camera(hm.OrthogonalCamera(w / h, hm.translation(hm.Vec(-1.0, 0.0, 1.5)) * hm.scaling(hm.Vec(1.0, 3.0, 1.7))))


@pytest.mark.parametrize("name,W,H,S,ortho", [("c2p", 161, 97, 0, False), ("c2p", 75, 41, 2, False), ("c2p", 75, 41, 2, True),
                                              ("wide300", 97, 61, 0, True), ("wide300", 97, 61, 2, False)])
def test_a_hit_frames_rays_fed_back_return_the_frame(scene_of, name, W, H, S, ortho):
    ds = scene_of(name)
    cam = _ortho(W, H) if ortho else flatten.flatten_camera(scenes.synthetic_camera(W, H))
    p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=S, pcg_mode=abi.PCG_SAMPLE, path_state=7, path_seq=11)
    frame = ds.render_hits(cam, p, abi.HIT_ALL)
    assert B.world(name)[0].n_shapes > (256 if name == "wide300" else 8)
    n = frame.shape_index.size
    got = ds.trace_rays(rb.ray_planes(frame.ray_origin.reshape(n, 3), frame.ray_dir.reshape(n, 3)))  # tmin 1e-5, tmax inf: Ray's defaults
    assert frame.hit.any() and (ortho or len(np.unique(frame.shape_index)) > 5)
    assert _bits(got.shape_index, frame.shape_index.reshape(n)) and _bits(got.t, frame.t.reshape(n))
    assert _bits(got.point, frame.point.reshape(n, 3)) and _bits(got.normal, frame.normal.reshape(n, 3))
    assert _bits(got.uv, frame.uv.reshape(n, 2))
    # ... and the buffers themselves: the frame's first 1 + 9 planes ARE the batch's buffer (the int32 plane's padding is nobody's)
    pad = (n * 4 + 7) // 8 * 8
    assert got.buffer[: n * 4].tobytes() == frame.buffer[: n * 4].tobytes()
    assert got.buffer[pad:].tobytes() == frame.buffer[pad: got.nbytes].tobytes()


# ---- 3. any-hit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.WORLDS))
def test_any_hit_is_the_negated_visibility(scene_of, orc, name):
    b = B.batches(orc, name)
    ds = scene_of(name)
    seg = rb.ray_planes(b["shadow"]["rays"])
    blocked = ds.occluded(seg)
    assert blocked.dtype == np.int32 and set(np.unique(blocked)) == {0, 1}
    assert np.array_equal(blocked == 0, b["visible"]), f"{int(((blocked == 0) != b['visible']).sum())} of {blocked.size} verdicts differ"
    assert np.array_equal(ds.points_visible(b["points"], b["light"]), b["visible"])
    assert np.array_equal(blocked == 1, ds.trace_rays(seg, 0).hit)  # "a closest hit within tmax exists", same library
    # the same segments without their end: whatever lies BEHIND the point blocks too -- tmax matters
    open_ = seg.copy()
    open_[7] = np.inf
    longer = ds.occluded(open_)
    assert np.all(longer >= blocked) and np.array_equal(longer == 1, ds.trace_rays(open_, 0).hit)
    if name in B.FRAME_WORLDS:
        assert (longer > blocked).any()
    # the bounce batch (tmax = inf) as shadow rays
    bounce = b["bounce"]
    assert np.array_equal(ds.occluded(rb.ray_planes(bounce["rays"])) == 1, bounce["want"].hit)


# ---- 4. channels ---------------------------------------------------------------------------------------------------------------
def test_every_channel_subset_holds_the_planes_of_the_full_batch(scene_of, orc):
    from pytracer_amd import _rays_lib

    R = _rays_lib.lib()
    rays = rb.ray_planes(B.batches(orc, "demo")["bounce"]["rays"])  # (hits and misses)
    n = rays.shape[1]
    ds = scene_of("demo")
    full = ds.trace_rays(rays, ALL)
    assert 0.1 < full.hit.mean() < 0.9
    for channels in range(16):
        got = ds.trace_rays(rays, channels)
        assert got.buffer.nbytes == R.pt_rays_bytes(n, channels, 0)
        assert _bits(got.shape_index, full.shape_index)
        covered = (n * 4 + 7) // 8 * 8
        for bit, k in rb._PLANES.items():
            for comp in range(k):
                off, off_full = R.pt_rays_plane_offset(n, channels, 0, bit, comp), R.pt_rays_plane_offset(n, ALL, 0, bit, comp)
                if channels & bit:
                    assert off == covered and got.buffer[off: off + 8 * n].tobytes() == full.buffer[off_full: off_full + 8 * n].tobytes(), (channels, bit, comp)
                    covered += 8 * n
                else:
                    assert off < 0
        assert covered == got.buffer.nbytes
    with pytest.raises(ValueError):
        ds.trace_rays(rays, abi.HIT_RAY)


# ---- 5. batch sizes, the margin behind the output -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2p", "wide1500"])  # (the per-chunk filter with its few-rays path; the grid walk)
def test_prefixes_of_a_batch_and_the_margin_behind_the_output(scene_of, orc, name):
    import torch

    from pytracer_amd import _rays_lib

    R = _rays_lib.lib()
    if True:
        ds = scene_of(name)
        rows = B.batches(orc, name)["bounce"]["rays"]
        rows = np.concatenate([rows, rows])[:1296]
        assert rows.shape[0] == (1296 if name == "c2p" else 1152)
        full = ds.trace_rays(rb.ray_planes(rows))
        blocked = ds.occluded(rb.ray_planes(rows))
        block = ds.kernel_args()
        for n in (1, 63, 64, 65, 255, 256, 257, rows.shape[0]):
            part = ds.trace_rays(rb.ray_planes(rows[:n]))
            for pname, plane in part.planes().items():
                assert _bits(plane, full.planes()[pname][:n]), (name, n, pname)
            assert np.array_equal(ds.occluded(rb.ray_planes(rows[:n])), blocked[:n]), (name, n)
            # device path: a sentinel-filled buffer, and out_bytes that promise exactly the batch's bytes
            rays_dev = torch.from_numpy(rb.ray_planes(rows[:n])).cuda()
            for anyhit, channels, want in ((0, ALL, part.buffer), (1, 0, blocked[:n].view(np.uint8))):
                need = int(R.pt_rays_bytes(n, channels, anyhit))
                out = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
                _rays_lib.check(R.pt_rays_trace_device(0, block, len(block), C.c_void_p(rays_dev.data_ptr()), n, channels, anyhit,
                                                       C.c_void_p(out.data_ptr()), need, None))
                host = out.cpu().numpy()
                pad = ((n * 4 + 7) // 8 * 8 - n * 4) if not anyhit else need - n * 4  # (the shape plane's padding is nobody's)
                assert host[: n * 4].tobytes() == want[: n * 4].tobytes()
                assert host[n * 4 + pad: need].tobytes() == want[n * 4 + pad: need].tobytes(), (name, n, anyhit)
                assert np.all(host[n * 4: n * 4 + pad] == 0xA5) and np.all(host[need:] == 0xA5), f"{name} n={n} anyhit={anyhit}: wrote outside its planes"
                # one byte too few: refused, nothing written
                out.fill_(0x5A)
                assert R.pt_rays_trace_device(0, block, len(block), C.c_void_p(rays_dev.data_ptr()), n, channels, anyhit,
                                              C.c_void_p(out.data_ptr()), need - 1, None) == -5
                assert bool((out == 0x5A).all())
        # n = 0: PT_OK, nothing written
        out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
        assert R.pt_rays_trace_device(0, block, len(block), C.c_void_p(out.data_ptr()), 0, ALL, 0, C.c_void_p(out.data_ptr()), 4096, None) == 0
        assert bool((out == 0xA5).all())
        empty = ds.trace_rays(np.zeros((8, 0)))
        assert empty.n == 0 and empty.shape_index.size == 0 and ds.occluded(np.zeros((8, 0))).size == 0


# ---- 6. rays that are not ordinary ----------------------------------------------------------------------------------------------
def _probe_rows(h: rb.RayHits):
    """The fields of pt_debug_hit_probe as a batch holds them (the probe leaves zeros in every field of a miss)."""
    out = np.zeros((h.n, 11))
    out[:, 0] = h.hit
    out[:, 1] = np.where(h.hit, h.t, 0.0)
    out[:, 2:5], out[:, 5:8], out[:, 8:10] = h.point, h.normal, h.uv
    out[:, 10] = np.where(h.hit, h.shape_index, 0)
    return out


def test_rays_that_are_not_ordinary_equal_the_exhaustive_probe(dev):
    """The recipe of tests/test_gpu_probes.py::test_filtered_query_with_rays_that_are_not_ordinary, plus negative tmin (an
    ordinary value here: the probes' "tmin < 0 = idle lane" does not carry over)."""
    from tests.test_gpu_probes import _stress_rays, _stress_world

    world = _stress_world(200, 9, 10.0, 0.05, 2.0)
    scene, rays = _stress_rays(world, 640, 9, 10.0)
    rng = np.random.default_rng(9)
    odd = rays.copy()
    idx = np.arange(0, 640, 5)
    for j, i in enumerate(idx):
        c = j % 6
        if c == 0:
            odd[i, 3:6] *= 1e18
            odd[i, 6:8] = 1e-30, np.inf
        elif c == 1:
            odd[i, 3:6] *= 1e-20
            odd[i, 7] = np.inf
        elif c == 2:
            odd[i, 0:3] = 1e19 * rng.normal(size=3)
            odd[i, 3:6] = -odd[i, 0:3]
        elif c == 3:
            odd[i, rng.integers(6)] = np.nan
        elif c == 4:
            odd[i, rng.integers(3)] = np.inf
        else:
            odd[i, 3 + rng.integers(3)] = -np.inf
    neg = np.arange(2, 640, 5)  # negative tmin: roots behind the origin count
    odd[neg[0::2], 6] = -1.0
    odd[neg[1::2], 6] = -1e30
    with dev.DeviceScene(scene) as ds:
        exact = ds.hit_probe(odd, -1)
        got = ds.trace_rays(rb.ray_planes(odd))
        plain = ds.trace_rays(rb.ray_planes(rays))
        blocked = ds.occluded(rb.ray_planes(odd))
    mine = _probe_rows(got)
    same = (mine.view(np.uint64) == exact[:, :11].view(np.uint64)).all(axis=1)
    assert same.all(), f"{int((~same).sum())} of 640 rays differ from the exhaustive query, first at {int(np.argmin(same))}"
    assert exact[idx[0::6], 0].any() and exact[idx[1::6], 0].any()  # (the fallback is exercised by rays that do hit something)
    assert np.array_equal(blocked == 1, exact[:, 0] != 0)
    # negative tmin found hits an ordinary tmin does not
    assert (got.t[neg][got.hit[neg]] < 0).any()
    # the neighbours in the wave did not notice
    untouched = np.ones(640, bool)
    untouched[idx] = False
    untouched[neg] = False
    for name, plane in plain.planes().items():
        assert _bits(got.planes()[name][untouched], plane[untouched]), name


# ---- 7. host path = device path; streams; a frame in flight; clones -----------------------------------------------------------------
def test_streams_a_frame_in_flight_and_clones(dev, orc):
    import torch

    from pytracer_amd.devmem import DeviceBuffer, Stream

    flat = B.world("c2p")[0]
    b = B.batches(orc, "c2p")
    W, H = 640, 360
    cam = flatten.flatten_camera(scenes.synthetic_camera(W, H))
    p = abi.make_params(W, H, abi.RENDERER_PATHTRACER, samples_per_side=2, num_of_rays=1, max_depth=3, pcg_mode=abi.PCG_SAMPLE)
    blocks = [rb.ray_planes(b["bounce"]["rays"]), rb.ray_planes(b["shadow"]["rays"])]
    ds = dev.DeviceScene(flat)
    try:
        alone = ds.render(cam, p)
        want_hits = ds.trace_rays(blocks[0])
        want_blocked = ds.occluded(blocks[1])
        frame = DeviceBuffer((H, W, 3), np.float64)
        s_frame, s1, s2 = Stream(), Stream(), Stream()
        dev_rays = [torch.from_numpy(x).cuda() for x in blocks]
        torch.cuda.synchronize()
        ds.render_into(cam, p, frame.data_ptr(), frame.nbytes, s_frame.handle)  # asynchronous: in flight while the batches go
        out1 = ds.trace_rays(dev_rays[0], ALL, device=True, stream=s1)
        out2 = ds.occluded(dev_rays[1], device=True, stream=s2)
        got_hits = rb.RayHits(out1.numpy(), blocks[0].shape[1], ALL)  # (numpy(): behind the stream the batch ran on)
        got_blocked = out2.numpy()[: blocks[1].shape[1] * 4].view(np.int32)
        frame.rendered_on(s_frame)
        got_frame = frame.numpy()
        _same_planes(got_hits, want_hits)
        assert got_hits.buffer[: got_hits.nbytes].tobytes() == want_hits.buffer.tobytes()
        assert np.array_equal(got_blocked, want_blocked)
        assert got_frame.tobytes() == alone.tobytes(), "the frame changed under concurrent ray batches"
        # synchronous device form (stream = None) and a DeviceBuffer handed in for the output
        mine = DeviceBuffer((rb.rays_bytes(blocks[0].shape[1], abi.HIT_T),), np.uint8)
        assert ds.trace_rays(dev_rays[0], "t", device=True, out=mine) is mine
        assert _bits(rb.RayHits(mine.numpy(), blocks[0].shape[1], "t").t, want_hits.t)
        # a clone has a block of its own, which outlives the original handle
        clone = ds.clone()
        before = bytes(clone.kernel_args())
        assert before != bytes(ds.kernel_args())  # (its own device copy, its own per-camera tables)
        ds.close()
        _same_planes(clone.trace_rays(blocks[0]), want_hits)
        assert np.array_equal(clone.occluded(blocks[1]), want_blocked)
        assert bytes(clone.kernel_args()) == before
        clone.close()
        for x in (frame, out1, out2, mine):
            x.free()
        for s in (s_frame, s1, s2):
            s.close()
    finally:
        ds.close()


# ---- 8. the accessor's size check; the tracer's world_queries ------------------------------------------------------------------------
def test_kernel_args_size_check_and_world_queries_through_the_tracer(scene_of, orc):
    from pytracer_amd import _lib, _rays_lib
    from pytracer_amd.tracer import GpuImageTracer

    L, R = _lib.lib(), _rays_lib.lib()
    ds = scene_of("demo")
    nb = int(R.pt_rays_args_bytes())
    buf = C.create_string_buffer(nb + 8)
    assert L.pt_scene_kernel_args(ds._h, buf, nb - 8) == -1 and L.pt_scene_kernel_args(ds._h, buf, nb + 8) == -1
    assert "bytes" in _lib.last_error()
    assert L.pt_scene_kernel_args(ds._h, None, nb) == -1 and L.pt_scene_kernel_args(None, buf, nb) == -1
    assert L.pt_scene_kernel_args(ds._h, buf, nb) == 0 and bytes(buf)[:nb] == bytes(ds.kernel_args())  # (cached: the same block every time)
    world, camera = scenes.demo_world()
    W, H = 40, 30
    tracer = GpuImageTracer(hm.HdrImage(W, H), camera)
    try:
        frame = tracer.fire_all_hits(world)
        q = tracer.world_queries(world)
        n = W * H
        rays = np.empty((n, 8))
        rays[:, 0:3], rays[:, 3:6] = frame.ray_origin.reshape(n, 3), frame.ray_dir.reshape(n, 3)
        rays[:, 6], rays[:, 7] = 1e-5, np.inf
        rec = q.ray_intersections(rays)
        assert _bits(rec.shape_index, frame.shape_index.reshape(n)) and _bits(rec.t, frame.t.reshape(n))
        assert _bits(rec.point, frame.point.reshape(n, 3)) and _bits(rec.normal, frame.normal.reshape(n, 3)) and _bits(rec.uv, frame.uv.reshape(n, 2))
        assert _bits(q.ray_intersections(rays[:, 0:3], rays[:, 3:6], "normal").normal, rec.normal)
        b = B.batches(orc, "demo")
        assert np.array_equal(q.are_points_visible(b["points"], b["light"]), b["visible"])
        assert q.scene is tracer._scene  # (the tracer's cached device scene: nothing was uploaded twice)
    finally:
        tracer.close()


def test_rays_command_writes_what_the_library_returns(scene_of, orc, tmp_path):
    from click.testing import CliRunner

    from pytracer_amd.cli import cli

    b = B.batches(orc, "demo")
    np.save(tmp_path / "rays.npy", b["bounce"]["rays"])
    out = str(tmp_path / "hits.npz")
    r = CliRunner().invoke(cli, ["rays", "--input", str(tmp_path / "rays.npy"), "--output", out, "--channels", "t,normal", "builtin:demo"])
    assert r.exit_code == 0, r.output
    got, want = np.load(out), b["bounce"]["want"]
    assert sorted(got.files) == ["normal", "shape_index", "t"]
    assert _bits(got["shape_index"], want.shape_index) and _bits(got["t"], want.t) and _bits(got["normal"], want.normal)
    np.save(tmp_path / "seg.npy", b["shadow"]["rays"])
    r = CliRunner().invoke(cli, ["rays", "--input", str(tmp_path / "seg.npy"), "--output", out, "--any-hit", "builtin:demo"])
    assert r.exit_code == 0, r.output
    assert np.array_equal(np.load(out)["blocked"] == 0, b["visible"])
