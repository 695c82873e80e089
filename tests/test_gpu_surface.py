"""Surface queries on the device (include/ptrace_surface.h, libptrace_surface.so): the materials of hit records and their
colour under the world's point lights, against the CPU oracle in its ``x * x`` mode, against the fused point-light renderer of
libptrace.so, and against themselves across channels, batch sizes and entry points.

Expected agreement: bit for bit, everywhere.  The records are the oracle's own, fed as host arrays, so (u, v) is the same on
both sides; the one libm call of the lights kernel (acos, twice, in the specular comparison) decides a branch and enters no
value, and tests/test_surface_host.py shows that no pair of any batch is near enough to the threshold for it to matter.  Device
against device (the hit-shader route against the fused kernel, the chained route against the host route): byte for byte."""
import numpy as np
import pytest

from pytracer_amd import abi, rays as rb, shaders
from pytracer_amd import hostmodel as hm

from . import surface_batches as S

pytestmark = pytest.mark.gpu


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
            open_[name] = dev.DeviceScene(S.world(name)[0])
        return open_[name]

    yield get
    for ds in open_.values():
        ds.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _diff(got, want) -> str:
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(got.shape[0], -1).any(axis=1))
    return f"{bad.size} of {got.shape[0]} records differ, first {bad[:5].tolist()}"


def _lights(ds, rec, rays, n=None, **kw):
    k = slice(None) if n is None else slice(0, n)
    return ds.shade_lights(rec.shape_index[k], rec.point[k], rec.normal[k], rec.uv[k], rays[k, 3:6], S.AMBIENT, S.BACKGROUND, **kw)


# ---- 1. against the oracle, per world --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.WORLDS))
def test_materials_equal_the_oracle(scene_of, orc, name):
    b = S.batch(orc, name)
    rec, want = b["rec"], b["materials"]
    got = scene_of(name).surface(rec.shape_index, rec.uv)
    assert got.n == rec.n and got.channels == rb.SURF_ALL
    for key in ("brdf_kind", "brdf_color", "emitted"):
        assert _bits(got.planes()[key], want[key]), f"{name} {key}: {_diff(got.planes()[key], want[key])}"
    assert np.array_equal(got.hit, rec.hit)


@pytest.mark.parametrize("name", list(S.WORLDS))
def test_point_light_colours_equal_the_oracle(scene_of, orc, name):
    b = S.batch(orc, name)
    got = _lights(scene_of(name), b["rec"], b["rays"])
    assert got.shape == (b["rec"].n, 3)
    assert _bits(got, b["colors"]), f"{name}: {_diff(got, b['colors'])}"


def test_world_queries_take_ray_hits_and_frames(dev, orc):
    """``WorldQueries.materials`` / ``point_light_radiance`` on a RayHits (the oracle's) and on a device hit-record frame, whose
    colours must be the fused point-light kernel's frame byte for byte."""
    from pytracer_amd import flatten, scenes

    b = S.batch(orc, "c2_lights")
    flat = S.world("c2_lights")[0]
    with dev.DeviceScene(flat) as ds:
        q = rb.WorldQueries(ds)
        mats = q.materials(b["rec"])
        assert _bits(mats.brdf_color, b["materials"]["brdf_color"]) and _bits(mats.brdf_kind, b["materials"]["brdf_kind"])
        assert _bits(q.materials(b["rec"], "emitted").emitted, b["materials"]["emitted"])
        assert _bits(q.point_light_radiance(b["rec"], b["rays"][:, 3:6], S.AMBIENT, S.BACKGROUND), b["colors"])
        with pytest.raises(ValueError, match="dirs"):
            q.point_light_radiance(b["rec"])
        for S_ in (0, 2):
            W, H = 75, 41
            cam2 = flatten.flatten_camera(scenes.synthetic_camera(W, H))
            par = abi.make_params(W, H, abi.RENDERER_POINTLIGHT, samples_per_side=S_, pcg_mode=abi.PCG_SAMPLE, path_state=7, path_seq=11,
                                  ambient=S.AMBIENT, background=S.BACKGROUND)
            frame = ds.render_hits(cam2, abi.copy_params(par, renderer=abi.RENDERER_FLAT), abi.HIT_ALL)
            col = q.point_light_radiance(frame, None, S.AMBIENT, S.BACKGROUND)
            assert col.shape == frame.shape_index.shape + (3,)
            if S_ == 0:
                assert _bits(col[0], ds.render(cam2, par))
            fm = q.materials(frame)
            assert fm.brdf_kind.shape == frame.shape_index.shape and fm.emitted.shape == col.shape and np.array_equal(fm.hit, frame.hit)


# ---- 2. the aimed specular cases: trace_rays, then shade_lights ---------------------------------------------------------------
@pytest.mark.parametrize("e,radius", S.AIMED)
def test_aimed_specular_reflections_around_the_threshold(dev, orc, e, radius):
    flat, ray = S.aimed_case(e, radius)
    want = S.expected_colors(orc, flat, ray)
    with dev.DeviceScene(flat) as ds:
        rec = ds.trace_rays(rb.ray_planes(ray))
        assert rec.hit[0] and rec.shape_index[0] == 0
        got = _lights(ds, rec, ray)
        mat = ds.surface(rec.shape_index, rec.uv)
    assert _bits(got, want), (e, radius, got, want)
    base = np.asarray(S.AMBIENT) + (0.01, 0.02, 0.03)
    assert np.all(got[0] > base) if e < S.THRESHOLD else _bits(got[0], base)
    assert mat.brdf_kind[0] == abi.BRDF_SPECULAR and _bits(mat.brdf_color[0], np.array([0.5, 0.6, 0.7])) and _bits(mat.emitted[0], np.array([0.01, 0.02, 0.03]))


# ---- 3. batch sizes, misses, channels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SIZES)
def test_batch_sizes_around_the_wave_and_the_block(scene_of, orc, n):
    """The last wave and the last block partly idle (idle lanes still enter every ballot of the light loop); an odd n pads the
    int32 plane."""
    b = S.batch(orc, "c2_lights")
    ds = scene_of("c2_lights")
    rec = b["rec"]
    start = b["n_primary"] - n // 2  # (primary rays and bounces both)
    k = slice(start, start + n)
    got = ds.shade_lights(rec.shape_index[k], rec.point[k], rec.normal[k], rec.uv[k], b["rays"][k, 3:6], S.AMBIENT, S.BACKGROUND)
    assert _bits(got, b["colors"][k])
    mat = ds.surface(rec.shape_index[k], rec.uv[k])
    assert mat.nbytes == ((n * 4 + 7) // 8 * 8) + 48 * n
    for key, want in b["materials"].items():
        assert _bits(mat.planes()[key], want[k]), key


def test_misses_only_and_interleaved(scene_of, orc):
    b = S.batch(orc, "c2_lights")
    ds = scene_of("c2_lights")
    rec, n = b["rec"], 1001
    args = (rec.point[:n], rec.normal[:n], rec.uv[:n], b["rays"][:n, 3:6], S.AMBIENT, S.BACKGROUND)
    # nothing but misses: the background everywhere, kind -1 and zeros
    none = np.full(n, -1, np.int32)
    assert _bits(ds.shade_lights(none, *args), np.tile(np.asarray(S.BACKGROUND), (n, 1)))
    mat = ds.surface(none, rec.uv[:n])
    assert np.all(mat.brdf_kind == -1) and not mat.brdf_color.any() and not mat.emitted.any() and not mat.hit.any()
    # every other record a miss: lanes with and without a hit side by side in every wave
    some = np.array(rec.shape_index[:n])
    some[::2] = -1
    miss = some < 0
    want = np.where(miss[:, None], np.asarray(S.BACKGROUND), b["colors"][:n])
    assert _bits(ds.shade_lights(some, *args), want)
    mat = ds.surface(some, rec.uv[:n])
    assert _bits(mat.brdf_kind, np.where(miss, -1, b["materials"]["brdf_kind"][:n]).astype(np.int32))
    assert _bits(mat.brdf_color, np.where(miss[:, None], 0.0, b["materials"]["brdf_color"][:n]))
    assert _bits(mat.emitted, np.where(miss[:, None], 0.0, b["materials"]["emitted"][:n]))
    # demo has natural misses in its batch (covered per world above): here its records in reverse order, as a second interleaving
    d = S.batch(orc, "demo")
    r = d["rec"]
    back = slice(None, None, -1)
    got = scene_of("demo").shade_lights(r.shape_index[back], r.point[back], r.normal[back], r.uv[back], d["rays"][back, 3:6], S.AMBIENT, S.BACKGROUND)
    assert _bits(got, d["colors"][back])


@pytest.mark.parametrize("channels", [0, rb.SURF_BRDF_COLOR, rb.SURF_EMITTED, rb.SURF_ALL])
def test_every_channel_combination_at_the_librarys_offsets(scene_of, orc, channels):
    from pytracer_amd import _surface_lib

    L = _surface_lib.lib()
    b = S.batch(orc, "pigments")
    rec, n = b["rec"], 257
    got = scene_of("pigments").surface(rec.shape_index[:n], rec.uv[:n] if channels else None, channels)
    assert got.buffer.nbytes == L.pt_rays_surface_bytes(n, channels) == got.nbytes
    assert _bits(got.buffer[: 4 * n].view(np.int32), b["materials"]["brdf_kind"][:n])
    for bit, key in ((rb.SURF_BRDF_COLOR, "brdf_color"), (rb.SURF_EMITTED, "emitted")):
        for comp in range(3):
            off = L.pt_rays_surface_plane_offset(n, channels, bit, comp)
            if channels & bit:
                assert _bits(got.buffer[off: off + 8 * n].view(np.float64), np.ascontiguousarray(b["materials"][key][:n, comp]))
            else:
                assert off < 0 and not got.has(key)


# ---- 4. end to end, device against device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H,S_", [("demo", 40, 30, 0), ("demo", 40, 30, 2), ("c2_lights", 48, 27, 0)])
def test_the_hit_shader_route_equals_the_fused_point_light_renderer(dev, name, W, H, S_):
    """``PointLightRenderer`` rebuilt from the public pieces -- hit-record frame, then ``point_light_radiance`` -- against the
    fused kernel, byte for byte: both take (u, v) from the same device arithmetic, so sphere pigments are included."""
    from pytracer_amd.tracer import GpuImageTracer

    world, camera = S.host_world(name)
    assert (W, H) == S.WORLDS[name]
    bg, amb = hm.Color(*S.BACKGROUND), hm.Color(*S.AMBIENT)
    fused = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode="seq")
    mine = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode="seq")
    try:
        fused.fire_all_rays(hm.PointLightRenderer(world, bg, amb))
        mine.fire_all_rays(shaders.PointLightShader(world, mine, bg, amb))
        assert fused.last_path == "device" and mine.last_path == "device-hits"
        a, b = np.asarray(fused.image.array), np.asarray(mine.image.array)
        assert a.shape == (H, W, 3) and len(np.unique(a.reshape(-1, 3), axis=0)) > 50
        assert _bits(b, a), f"{int(np.any(a != b, axis=-1).sum())} pixels differ"
        assert (fused.pcg.state, fused.pcg.inc) == (mine.pcg.state, mine.pcg.inc)
    finally:
        fused.close()
        mine.close()


def test_a_chain_that_stays_in_hbm(dev, orc):
    """trace_rays(device=True) -> surface and shade_lights (device=True) reading planes out of the first buffer by offset, one
    stream, one download each: equal to the host route byte for byte."""
    import torch

    from pytracer_amd.devmem import DeviceBuffer, Stream

    b = S.batch(orc, "wide300_lights")
    flat = S.world("wide300_lights")[0]
    n = 1001
    block = np.ascontiguousarray(rb.ray_planes(b["rays"][:n]))
    ALL = rb.RAY_CHANNELS
    ds = dev.DeviceScene(flat)
    st = Stream()
    try:
        host_rec = ds.trace_rays(block)
        host_col = ds.shade_lights(host_rec.shape_index, host_rec.point, host_rec.normal, host_rec.uv, b["rays"][:n, 3:6], S.AMBIENT, S.BACKGROUND)
        host_mat = ds.surface(host_rec.shape_index, host_rec.uv)
        rays_dev = torch.from_numpy(block).cuda()
        torch.cuda.synchronize()
        table = ds.slot_table()
        assert ds.slot_table() is table  # (cached on the scene)
        rec_dev = ds.trace_rays(rays_dev, ALL, device=True, stream=st)
        base = rec_dev.data_ptr()
        at = lambda ch: base + rb.rays_plane_offset(n, ALL, False, ch, 0)  # noqa: E731
        dirs = rays_dev.data_ptr() + 3 * n * 8  # the direction planes of the ray block itself
        col_dev = ds.shade_lights(base, at(abi.HIT_POINT), at(abi.HIT_NORMAL), at(abi.HIT_UV), dirs, S.AMBIENT, S.BACKGROUND,
                                  device=True, stream=st, n=n)
        mine = DeviceBuffer((rb.surface_bytes(n, rb.SURF_ALL),), np.uint8)
        assert ds.surface(base, at(abi.HIT_UV), "all", device=True, stream=st, out=mine, n=n) is mine
        got_col = col_dev.numpy()  # (numpy(): behind the stream the batch ran on)
        got_mat = rb.SurfaceColors(mine.numpy(), n)
        assert got_col.shape == (3, n) and _bits(got_col.T, host_col)
        assert got_mat.buffer[: 4 * n].tobytes() == host_mat.buffer[: 4 * n].tobytes()
        pad = (4 * n + 7) // 8 * 8
        assert got_mat.buffer[pad: got_mat.nbytes].tobytes() == host_mat.buffer[pad:].tobytes()
        # and the host route is the oracle's, up to what ocml's (u, v) on spheres changes: planes and uniform pigments are exact
        same_uv = np.all(host_rec.uv == b["rec"].uv[:n], axis=1)
        assert same_uv.sum() > n // 4 and _bits(host_col[same_uv], b["colors"][:n][same_uv])
        # raw addresses need n=; an object with data_ptr() and nbytes (a device tensor of n int32) counts its records itself
        with pytest.raises(ValueError, match="n="):
            ds.surface(base, None, "none", device=True)
        shape_dev = torch.from_numpy(np.array(host_rec.shape_index)).cuda()
        torch.cuda.synchronize()
        kinds = ds.surface(shape_dev, None, "none", device=True)  # (stream None: synchronous)
        assert kinds.nbytes == pad and _bits(kinds.numpy()[: 4 * n].view(np.int32), host_mat.brdf_kind)
        with pytest.raises(ValueError, match="device=True"):
            ds.surface(host_rec.shape_index, host_rec.uv, stream=st)
    finally:
        st.close()
        ds.close()
