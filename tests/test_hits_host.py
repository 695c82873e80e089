"""Hit-record frames on the host: the buffer layout, the plan, and the hit-shader route of ``fire_all_rays``.

No GPU: ``pt_hits_bytes`` / ``pt_hits_plane_offset`` and ``pt_debug_plan_hits`` are pure host functions of libptrace.so, and the
hit-shader route is driven through its one seam (``GpuImageTracer._render_hit_frame``) with a ``HitFrame`` the oracle fills.
"""
import ctypes as C

import numpy as np
import pytest

from pytracer_amd import _lib, abi, device, flatten, hits, scenes, shaders
from pytracer_amd import hostmodel as hm
from pytracer_amd.tracer import GpuImageTracer

from . import util

PLANES = ((abi.HIT_T, 1), (abi.HIT_POINT, 3), (abi.HIT_NORMAL, 3), (abi.HIT_UV, 2), (abi.HIT_RAY, 6))  # include/ptrace.h, in bit order


def _layout(p, channels):
    """The layout restated from include/ptrace.h: -> (bytes, {(channel, component): byte offset})."""
    S = p.samples_per_side
    rows = sum(min(p.row_block, p.height - b * p.row_block) for b in range((p.height + p.row_block - 1) // p.row_block)
               if b % p.n_ranks == p.rank)
    n = max(S, 1) ** 2 * rows * p.width
    at = (4 * n + 7) // 8 * 8
    offsets = {(0, 0): 0}
    for bit, k in PLANES:
        if channels & bit:
            for c in range(k):
                offsets[(bit, c)] = at
                at += 8 * n
    return at, offsets


@pytest.mark.parametrize("S", [0, 2, 3])
@pytest.mark.parametrize("channels", [0, abi.HIT_T, abi.HIT_ALL, abi.HIT_NORMAL | abi.HIT_UV, abi.HIT_T | abi.HIT_NORMAL | abi.HIT_RAY,
                                      abi.HIT_POINT | abi.HIT_RAY])
def test_layout_of_the_buffer(S, channels):
    lib = _lib.lib()
    for w, h, part in ((161, 97, {}), (7, 5, {}), (1, 1, {}), (161, 97, dict(row_block=8, n_ranks=3, rank=1)),
                       (33, 97, dict(row_block=5, n_ranks=3, rank=2)), (33, 19, dict(row_block=8, n_ranks=3, rank=0))):
        p = abi.make_params(w, h, abi.RENDERER_PATHTRACER, samples_per_side=S, out_format=abi.OUT_F32, **part)  # (renderer, format: ignored)
        nbytes, offsets = _layout(p, channels)
        assert lib.pt_hits_bytes(C.byref(p), channels) == nbytes == abi.hits_bytes(p, channels)
        for channel in (0,) + tuple(bit for bit, _ in PLANES):
            for comp in range(-1, 7):
                want = offsets.get((channel, comp), -1)
                assert lib.pt_hits_plane_offset(C.byref(p), channels, channel, comp) == want, (channels, channel, comp)
                assert abi.hits_plane_offset(p, channels, channel, comp) == want
        frame = hits.HitFrame(None, p, channels)
        assert frame.shape_index.shape == (max(S, 1) ** 2, len(abi.rows_for_rank(h, p.row_block, p.n_ranks, p.rank)), w)
        assert frame.shape_index.dtype == np.int32 and frame.nbytes == nbytes
        base = frame.buffer.ctypes.data
        for name, bit, comp in (("t", abi.HIT_T, 0), ("point", abi.HIT_POINT, 0), ("normal", abi.HIT_NORMAL, 0), ("uv", abi.HIT_UV, 0),
                                ("ray_origin", abi.HIT_RAY, 0), ("ray_dir", abi.HIT_RAY, 3)):
            if channels & bit:
                view = getattr(frame, name)
                assert view.ctypes.data - base == offsets[(bit, comp)] and not view.flags.owndata  # a view, no copy
                if name != "t":
                    assert view.shape == frame.shape_index.shape + (2 if name == "uv" else 3,)
                    assert view[..., 1].ctypes.data - base == offsets[(bit, comp + 1)]
            else:
                with pytest.raises(KeyError):
                    getattr(frame, name)


def test_unknown_channel_bits_are_refused():
    lib = _lib.lib()
    p = abi.make_params(16, 16, abi.RENDERER_FLAT)
    for bad in (32, 64 | abi.HIT_T, -1, 1 << 20):
        assert lib.pt_hits_plane_offset(C.byref(p), bad, abi.HIT_T, 0) == -1  # PT_ERR_INVALID
        assert lib.pt_hits_bytes(C.byref(p), bad) == 0  # (a size cannot carry an error code: no bytes)
        info = abi.PlanInfo()
        flat = flatten.flatten_world(scenes.synthetic_world(8))
        desc = flat.desc()
        cam = flatten.flatten_camera(scenes.synthetic_camera(16, 16))
        assert lib.pt_debug_plan_hits(C.byref(desc), C.byref(cam), C.byref(p), bad, 256, C.byref(info)) == -1
        with pytest.raises(ValueError):
            abi.hit_channels(bad)
    assert abi.hit_channels("normal, t,uv") == abi.HIT_NORMAL | abi.HIT_T | abi.HIT_UV and abi.hit_channels("all") == abi.HIT_ALL
    with pytest.raises(ValueError):
        abi.hit_channels("colour")


# ---- the plan ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tuning():
    saved = {}

    def set_(name, value):
        saved.setdefault(name, device.get_tuning(name))
        device.set_tuning(name, value)

    yield set_
    for name, value in saved.items():
        device.set_tuning(name, value)


def _ortho_cam(w, h):
    return flatten.flatten_camera(hm.OrthogonalCamera(w / h, hm.translation(hm.Vec(-1.0, 0.0, 1.5)) * hm.scaling(hm.Vec(1.0, 3.0, 1.7))))


def _tiles(w, rows):
    return ((w + 7) // 8) * ((rows + 7) // 8)


def _grid(w, rows, n_cu=256):
    """Four waves = four tiles per workgroup, at most eight workgroups per CU resident (the 8x8 tile kernel's rule)."""
    return max(1, min((_tiles(w, rows) + 3) // 4, 8 * n_cu))


def test_plan_names_the_hits_kernels(tuning):
    c2 = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    cam = flatten.flatten_camera(scenes.synthetic_camera(1280, 720))
    p = abi.make_params(1280, 720, abi.RENDERER_PATHTRACER, pcg_mode=abi.PCG_SEQ)  # (renderer ignored: SEQ is not refused)
    info = device.plan_hits(c2, cam, p)
    assert info.kernels == ["pt_hits_kernel"] and info.kernel == abi.KERNEL_HITS == 7
    assert (info.grid, info.lds_main, info.hier, info.ortho, info.rows, info.npix) == (_grid(1280, 720), 4 * 1 * 8, 0, 0, 720, 1280 * 720)
    assert info.grid * 4 >= min(_tiles(1280, 720), 4 * 8 * 256)
    # few CUs: a grid-stride loop over the tiles
    assert device.plan_hits(c2, cam, p, n_cu=4).grid == 32
    # odd sizes and a 3-rank partition: the rank's rows
    q = abi.make_params(161, 97, abi.RENDERER_FLAT, samples_per_side=2, row_block=8, n_ranks=3, rank=1)
    rows = len(abi.rows_for_rank(97, 8, 3, 1))
    info = device.plan_hits(c2, flatten.flatten_camera(scenes.synthetic_camera(161, 97)), q, channels="t,normal")
    assert (info.main_kernel, info.rows, info.grid) == ("pt_hits_kernel", rows, _grid(161, rows))
    # orthogonal camera: the beam form
    info = device.plan_hits(c2, _ortho_cam(1280, 720), p)
    assert info.kernels == ["pt_hits_kernel<ORTHO>"] and info.ortho == 1 and info.hoist == 0 and info.grid == _grid(1280, 720)
    # more than 256 shapes: cell lists first
    big = flatten.flatten_world(scenes.synthetic_world(300, wide=True))
    info = device.plan_hits(big, cam, p)
    assert info.kernels == ["pt_cell_kernel", "pt_hits_kernel<HIER>"] and info.hier == 1 and info.grid == _grid(1280, 720)
    assert info.lds_main == 4 * ((300 + 63) // 64) * 8
    # ... but not where a rank's tiles would straddle cells (row blocks that are no multiple of 8), nor for parallel rays
    info = device.plan_hits(big, cam, abi.copy_params(p, row_block=5, n_ranks=3, rank=0))
    assert info.kernels == ["pt_hits_kernel"] and info.hier == 0
    assert device.plan_hits(big, _ortho_cam(1280, 720), p).kernels == ["pt_hits_kernel<ORTHO>"]
    # worlds of fewer than four shapes, and cull = 0: every shape through world_query, the same tiles
    demo = flatten.flatten_world(scenes.demo_world()[0])
    info = device.plan_hits(demo, cam, p)
    assert info.kernels == ["pt_hits_kernel<noCULL>"] and info.lds_main == 0 and info.grid == _grid(1280, 720)
    tuning("cull", 0)
    info = device.plan_hits(c2, cam, p)
    assert info.kernels == ["pt_hits_kernel<noCULL>"] and info.lds_main == 0 and info.grid == _grid(1280, 720) and info.kernel == 7
    assert device.plan_hits(big, cam, p).kernels == ["pt_hits_kernel<noCULL>"]
    assert device.plan_hits(c2, _ortho_cam(1280, 720), p).kernels == ["pt_hits_kernel<ORTHO, noCULL>"]
    tuning("cull", 1)
    # the plan of the renderers is what it was: Flat at pixel centres still takes the 16x16 tiles
    assert device.plan(c2, cam, abi.make_params(1280, 720, abi.RENDERER_FLAT)).kernels == ["pt_tile4_kernel<FLAT, LDS>"]


def test_kernel_names_stay_out_of_the_renderers_catalogue():
    from . import variant_catalog as vc

    names = vc.plannable_names()
    assert len(names) == 37 and not any("hits" in n for n in names)


# ---- the hit-shader route -------------------------------------------------------------------------------------------------
class OracleWorld(hm.World):
    """The demo world with a ``ray_intersection`` (world.py:51-69) that asks the oracle: what lets a shader's scalar
    ``__call__`` run through ``_host_loop``.  Test infrastructure: product code never imports the oracle."""

    def __init__(self, world, orc):
        super().__init__()
        self.shapes, self.point_lights = world.shapes, world.point_lights
        self.flat, self.orc = flatten.flatten_world(world), orc

    def ray_intersection(self, ray):
        o, d = ray.origin, ray.dir
        r = self.orc.world_intersect(self.flat, self.orc.ray8([o.x, o.y, o.z], [d.x, d.y, d.z], ray.tmin, ray.tmax))
        if r is None:
            return None
        return hits.HitRecord(world_point=hm.Vec(*r[1:4]), normal=hm.Vec(*r[4:7]), surface_point=hits.Vec2d(r[7], r[8]), t=float(r[0]),
                              ray=ray, shape_index=int(r[9]))


def oracle_frame(orc, flat, cam, params, channels, pcg):
    """The frame ``pt_render_hits`` is specified to produce, from the oracle: jitter drawn from ``pcg`` (SEQ: one generator,
    row-major pixels, sub_row outer, sub_col inner, u before v -- imagetracer.py:80-93)."""
    frame = hits.HitFrame(None, params, channels)
    S, W, H = params.samples_per_side, params.width, params.height
    frame.shape_index[...] = -1
    if frame.has("t"):
        frame.t[...] = np.inf
    for row in range(H):
        for col in range(W):
            for k in range(frame.nsamp):
                up = vp = 0.5
                if S > 0:
                    up = (k % S + pcg.random_float()) / S
                    vp = (k // S + pcg.random_float()) / S
                ray = orc.tracer_fire_ray(cam, W, H, col, row, up, vp)
                if frame.has("ray_origin"):
                    frame.ray_origin[k, row, col], frame.ray_dir[k, row, col] = ray[0:3], ray[3:6]
                r = orc.world_intersect(flat, ray)
                if r is None:
                    continue
                frame.shape_index[k, row, col] = int(r[9])
                for name, val in (("t", r[0]), ("point", r[1:4]), ("normal", r[4:7]), ("uv", r[7:9])):
                    if frame.has(name):
                        getattr(frame, name)[k, row, col] = val
    return frame


class SeamTracer(GpuImageTracer):
    """``fire_all_rays`` with the device replaced at its one seam by a frame the oracle computes."""

    def __init__(self, *a, orc=None, **kw):
        super().__init__(*a, **kw)
        self.orc, self.asked = orc, []

    def _render_hit_frame(self, world, channels):
        self.asked.append(channels)
        params = self._hits_params()
        assert params.pcg_mode == abi.PCG_SEQ
        pcg = self.orc.Pcg(params.jitter_state, params.jitter_seq)  # (a copy: the seam must not advance tracer.pcg)
        return oracle_frame(self.orc, world.flat, flatten.flatten_camera(self.camera), params, channels, pcg)


@pytest.mark.parametrize("S", [0, 2])
@pytest.mark.parametrize("which", ["normal", "depth"])
def test_hit_shader_route_equals_the_host_loop_bit_for_bit(oracle, which, S):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        demo, camera = scenes.demo_world()
        world = OracleWorld(demo, oracle)
        W, H = 24, 16
        bg = hm.Color(0.25, 0.5, 0.125)
        shader = shaders.NormalShader(world, bg) if which == "normal" else shaders.DepthShader(world, 1.0, 12.0, bg)
        fast = SeamTracer(hm.HdrImage(W, H), camera, samples_per_side=S, pcg=hm.PCG(45, 54), pcg_mode="seq", orc=oracle)
        fast.pcg.random()  # (a stream somebody already drew from: the frame continues it)
        fast.fire_all_rays(shader)
        assert fast.last_path == "device-hits" and fast.asked == [shader.hit_channels]
        slow = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S, pcg=hm.PCG(45, 54), pcg_mode="seq")
        slow.pcg.random()
        slow.fire_all_rays(shader.__call__)  # a plain callable Ray -> Color: the interpreter loop, one sample at a time
        assert slow.last_path == "host"
        a, b = fast.image.array, slow.image.array
        assert a.shape == (H, W, 3) and util.bits_equal(a, b)
        assert len(np.unique(a.reshape(-1, 3), axis=0)) > 5  # (the sphere, the ground and the sky plane: the demo world has no miss)
        assert (fast.pcg.state, fast.pcg.inc) == (slow.pcg.state, slow.pcg.inc)
        if S > 0:
            assert fast.pcg.state != hm.PCG(45, 54).state
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def test_hit_shader_route_details(oracle):
    demo, camera = scenes.demo_world()
    world = OracleWorld(demo, oracle)

    class Mine:  # a user's renderer: no hit_channels -> all; [H, W, 3] accepted at S = 0
        def __init__(self, world):
            self.world = world

        def __call__(self, ray):
            raise AssertionError("the hit-shader route never calls the scalar form")

        def shade_hits(self, frame):
            assert frame.has("ray_dir") and frame.has("uv") and frame.nsamp == 1
            return np.where(frame.hit[0][..., None], frame.uv[0][..., :1] * np.ones(3), 0.0)

    t = SeamTracer(hm.HdrImage(8, 8), camera, orc=oracle)  # pcg_mode "auto" means "seq"
    calls = []
    t.fire_all_rays(Mine(world), callback=lambda col, row, tag: calls.append((col, row, tag)), tag="x")
    assert t.last_path == "device-hits" and t.asked == [abi.HIT_ALL] and calls == [(0, 0, "x")]
    rec = oracle_frame(oracle, world.flat, flatten.flatten_camera(camera), t._hits_params(), abi.HIT_ALL, oracle.Pcg()).record(4, 7)
    assert rec is not None and t.image.array[7, 4, 0] == rec.surface_point.u and rec.shape_index == 1 and rec.ray is not None

    class Wrong(Mine):
        def shade_hits(self, frame):
            return np.zeros((3, 8, 8, 3))

    with pytest.raises(ValueError):
        t.fire_all_rays(Wrong(world))
    # a callable without shade_hits goes to the host loop exactly as before; so does one without a world
    seen = []
    t2 = GpuImageTracer(hm.HdrImage(2, 2), camera)
    t2.fire_all_rays(lambda ray: seen.append(ray) or hm.Color(1.0, 2.0, 3.0))
    assert t2.last_path == "host" and len(seen) == 4
    # the worked shaders on a parameter-holder world: a clear TypeError from the scalar form
    with pytest.raises(TypeError, match="ray_intersection"):
        shaders.NormalShader(demo)(seen[0])
    # materials() and record() on a miss
    frame = oracle_frame(oracle, world.flat, flatten.flatten_camera(camera), abi.make_params(8, 8, abi.RENDERER_FLAT), abi.HIT_T, oracle.Pcg())
    mats = frame.materials(demo)
    assert mats.shape == (1, 8, 8) and mats[0, 7, 4] is demo.shapes[1].material
    sky = np.argwhere(frame.shape_index[0] == 0)
    assert len(sky) and mats[0, sky[0][0], sky[0][1]] is demo.shapes[0].material
    empty = hits.HitFrame(None, abi.make_params(4, 4, abi.RENDERER_FLAT), abi.HIT_T)
    empty.shape_index[...] = -1
    assert empty.record(1, 1) is None and empty.materials(demo)[0, 1, 1] is None and not empty.hit.any()


def test_unsupported_world_raises_or_falls_back_to_the_scalar_form():
    class Cube:  # a shape class the device does not know
        transformation, material = hm.Transformation(), hm.Material()

    class World:
        shapes, point_lights = [Cube()], []

        def ray_intersection(self, ray):
            return None

    _, camera = scenes.demo_world()
    shader = shaders.NormalShader(World(), hm.Color(0.5, 0.25, 1.0))
    with pytest.raises(flatten.UnsupportedSceneError):
        GpuImageTracer(hm.HdrImage(3, 2), camera).fire_all_rays(shader)
    t = GpuImageTracer(hm.HdrImage(3, 2), camera, fallback="host")
    t.fire_all_rays(shader)
    assert t.last_path == "host" and np.all(t.image.array == [0.5, 0.25, 1.0])


def test_device_buffer_downloads_behind_its_last_render_stream(monkeypatch):
    """DeviceBuffer.numpy() without a stream waits on the stream the buffer was last rendered on."""
    from pytracer_amd import devmem

    calls = []

    class FakeLib:
        def pt_device_alloc(self, device, nbytes, out):
            out._obj.value = 4096
            return 0

        def pt_device_free(self, device, p):
            return 0

        def pt_device_download(self, device, dst, src, nbytes, stream):
            calls.append(stream.value if stream is not None else None)
            return 0

    monkeypatch.setattr(devmem._lib, "lib", lambda: FakeLib())
    buf = devmem.DeviceBuffer((4,), np.uint8)
    buf.numpy()
    buf.rendered_on(1234)
    buf.numpy()
    st = devmem.Stream.__new__(devmem.Stream)
    st.device, st.handle = 0, 77
    buf.rendered_on(st)
    buf.numpy()
    other = devmem.Stream.__new__(devmem.Stream)
    other.device, other.handle = 0, 99
    buf.numpy(other)
    st.handle = None  # closed: nothing of it is in flight
    buf.numpy()
    other.handle = None
    assert calls == [None, 1234, 77, 99, None]
