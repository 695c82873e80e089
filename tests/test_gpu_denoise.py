"""Denoise queries on the device (include/ptrace_denoise.h, libptrace_denoise.so): the edge-avoiding a-trous filter against its numpy
mirror (``rays.denoise_host``), against itself across entry points, streams and launch shapes, and in what it is for -- a gather
frame (``shaders.DenoisedGatherShader``) and a sphere's light map (``WorldQueries.denoised_light_map``).

Expected agreement: bit for bit wherever the expected value is finite; where it is not, NaN where NaN is expected and infinities of
the same sign (``hostile_records.differing``).  The one statistical claim -- the filtered frame is closer to a converged one than the
unfiltered frame it was made from -- is asserted as that and no tighter: any tighter figure would come from the code under test."""
import os

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import rays as rb

from . import hostile_records as H
from . import surface_batches as S
from .test_denoise_host import b3_blur_interior, coplanar_frame, two_shape_frame

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
# 70 x 33 crosses the edges of the 16 x 16 tiles in every sub-lattice at s = 1, 2, 4; 150 x 12 those of the 32-wide alternative tile
# (sub-lattices of 38 columns at s = 4), 70 x 33 those of its 8 rows (9 rows at s = 4)
FRAMES = [(1, 1), (3, 2), (17, 5), (37, 23), (70, 33), (150, 12)]
FLAGS = [(True, False), (True, True), (False, False), (False, True)]  # (same_shape, wrap_x)
POWERS = (0, 5, 10)
SIGMAS = ((INF, INF), (0.3, 0.7), (INF, 0.5), (0.2, INF))  # (sigma_point, sigma_colour)
PAIRS = [(e, s) for e in POWERS for s in SIGMAS]


def parameter_sets():
    """passes 1 .. 5 x both flags on and off: twenty sets, over which the twelve (e, sigmas) pairs rotate (each at least once)."""
    out = []
    for i, (passes, (same, wrap)) in enumerate((p, f) for p in range(1, 6) for f in FLAGS):
        e, (sp, sc) = PAIRS[(7 * i) % 12]
        out.append(dict(passes=passes, same_shape=same, wrap_x=wrap, normal_power_log2=e, sigma_point=sp, sigma_colour=sc))
    return out


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    return device


@pytest.fixture(scope="module")
def demo(dev):
    with dev.DeviceScene(S.world("demo")[0]) as ds:
        yield ds


@pytest.fixture(scope="module")
def demo_frames(dev):
    """(W, H) -> (tracer, world, the hit frame of the demo world at that size, its queries), rendered once for the module."""
    from pytracer_amd import hostmodel as hm
    from pytracer_amd import scenes
    from pytracer_amd.tracer import GpuImageTracer

    made = {}

    def get(W, Hh):
        if (W, Hh) not in made:
            world, camera = scenes.demo_world()
            tracer = GpuImageTracer(hm.HdrImage(W, Hh), camera, samples_per_side=0)
            made[(W, Hh)] = (tracer, world, tracer.fire_all_hits(world), tracer.world_queries(world))
        return made[(W, Hh)]

    yield get
    for tracer, _, _, _ in made.values():
        tracer.close()


def hostile_frame(W, Hh, seed):
    """Guides nobody vouches for: three shapes in patches plus negative and out-of-range indices; normals of any length, zero, NaN and
    infinite; points on a wavy sheet, some NaN and infinite; colours with NaN, inf and 1e300."""
    rng = np.random.default_rng(seed)
    m = W * Hh
    yy, xx = np.mgrid[0:Hh, 0:W]
    shape = ((xx // 5 + yy // 4) % 3).astype(np.int32).reshape(-1)
    point = np.stack([xx * 0.1, yy * 0.1, 0.05 * np.sin(xx * 0.7) * np.cos(yy * 0.9)], axis=-1).reshape(-1, 3) + rng.normal(0, 0.002, (m, 3))
    normal = (np.array([0.0, 0.0, 1.0]) + rng.normal(0, 0.25, (m, 3))) * np.exp(rng.uniform(-2, 2, (m, 1)))
    colour = rng.uniform(0.0, 2.0, (m, 3))
    pick = lambda share: np.flatnonzero(rng.uniform(0, 1, m) < share)  # noqa: E731
    for rows, value in ((pick(0.08), -1), (pick(0.02), -2 ** 31), (pick(0.04), 1000), (pick(0.02), 2 ** 31 - 1)):
        shape[rows] = value
    for rows, value in ((pick(0.03), (0.0, 0.0, 0.0)), (pick(0.02), (NAN, 0.0, 1.0)), (pick(0.02), (0.0, INF, 1.0)), (pick(0.01), (-INF, INF, NAN)),
                        (pick(0.02), (1e200, 1e200, 1e200)), (pick(0.02), (1e-200, 0.0, 1e-200))):
        normal[rows] = value
    for rows, value in ((pick(0.02), (NAN, 0.0, 0.0)), (pick(0.02), (0.0, INF, 0.0)), (pick(0.01), (1e300, -1e300, 1e300))):
        point[rows] = value
    for rows, value in ((pick(0.02), (NAN, 1.0, 1.0)), (pick(0.02), (1.0, INF, 1.0)), (pick(0.02), (1e300, 1.0, 1.0)), (pick(0.01), (-INF, NAN, 1e300))):
        colour[rows] = value
    return colour, shape, normal, point


def _check(got, want, label):
    got, want = np.ascontiguousarray(got).reshape(-1, 3), np.ascontiguousarray(want).reshape(-1, 3)
    bad = H.differing(got, want)
    assert bad.size == 0, f"{label}: {bad.size} of {len(want)} pixels differ, first {int(bad[0])}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---- 1. the device against the mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_synthetic_hostile_guides_equal_the_mirror_bit_for_bit(demo, W, Hh):
    colour, shape, normal, point = hostile_frame(W, Hh, 100 * W + Hh)
    changed = 0
    for par in parameter_sets():
        want = rb.denoise_host(colour, shape, normal, point, W, Hh, **par)
        got = demo.denoise(colour, shape, normal, point, W, Hh, **par)
        assert got.shape == (Hh, W, 3)
        _check(got, want, f"{W}x{Hh} {par}")
        miss = shape < 0
        if miss.any():  # a miss is copied, whatever it holds
            _check(got.reshape(-1, 3)[miss], colour[miss], f"{W}x{Hh} {par}: the misses")
        changed += int((got.reshape(-1, 3)[~miss] != colour[~miss]).any())
    assert changed or W * Hh == 1  # (the filter did something)


@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_the_guides_of_a_real_hit_frame_equal_the_mirror_bit_for_bit(demo_frames, W, Hh):
    tracer, world, frame, wq = demo_frames(W, Hh)
    rng = np.random.default_rng(W + Hh)
    shape, normal, point = np.asarray(frame.shape_index)[0], np.asarray(frame.normal)[0], np.asarray(frame.point)[0]
    colour = rng.uniform(0.5, 1.5, (Hh, W, 3)) * rng.uniform(0.2, 3.0, 3)
    for par in parameter_sets():
        want = rb.denoise_host(colour, shape, normal, point, W, Hh, **par)
        _check(wq.denoised(colour, frame, **par), want, f"{W}x{Hh} {par}")
    # the same through a ray batch's records and through plain arrays
    batch = wq.ray_intersections(np.asarray(frame.ray_origin).reshape(-1, 3), np.asarray(frame.ray_dir).reshape(-1, 3), channels="point,normal")
    want = rb.denoise_host(colour, batch.shape_index, batch.normal, batch.point, W, Hh)
    _check(wq.denoised(colour, batch), want, "a RayHits")
    _check(wq.denoised(colour, (batch.point, batch.normal, batch.shape_index)), want, "plain arrays")


# ---- 2. entry points, buffers, streams, launch shapes -------------------------------------------------------------------------------
def test_host_form_device_form_out_and_a_stream(dev):
    """``device=True``: the hit frame rendered into a device buffer and a gather of it left in HBM, the filter reading all four inputs
    where they are -- on the default stream into buffers of its own, and on a non-default stream into the caller's, twice: the host
    form's bits."""
    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, DeviceSpan, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh = 70, 33
    m = W * Hh
    flat, cam = S.world("demo")
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    st = Stream()
    try:
        with dev.DeviceScene(flat) as ds:
            hits = DeviceBuffer((abi.hits_bytes(par_f, abi.HIT_ALL),), np.uint8)
            ds.render_hits_into(cam, par_f, abi.HIT_ALL, hits, stream=st)
            frame = HitFrame(hits.numpy(), par_f, abi.HIT_ALL)
            base = hits.data_ptr()
            off = lambda channel, first=0: base + abi.hits_plane_offset(par_f, abi.HIT_ALL, channel, first)  # noqa: E731
            shp_d, pnt_d, nrm_d = base, off(abi.HIT_POINT), off(abi.HIT_NORMAL)
            gathered = ds.gather(pnt_d, nrm_d, 2, 42, None, shp_d, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", device=True, stream=st, n=m)
            col_d = gathered.data_ptr()  # (the three radiance planes come first)
            colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T)
            shape, normal, point = np.asarray(frame.shape_index)[0], np.asarray(frame.normal)[0], np.asarray(frame.point)[0]
            assert (shape >= 0).sum() > m // 2 and len(np.unique(colour, axis=0)) > 10
            planes = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
            for par in (dict(passes=4, wrap_x=True), dict(passes=1), dict(passes=3, sigma_colour=0.5, same_shape=False)):
                want = ds.denoise(colour, shape, normal, point, W, Hh, **par)
                _check(want, rb.denoise_host(colour, shape, normal, point, W, Hh, **par), f"host form {par}")
                fresh = ds.denoise(col_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, **par)  # the default stream, buffers of its own
                _check(planes(fresh), want, f"device form {par}")
                mine = DeviceBuffer((3, m), np.float64)
                work = DeviceBuffer((ds.denoise_workspace_bytes(W, Hh, **par),), np.uint8)
                assert work.nbytes == 24 * m * (2 if par["passes"] > 1 else 1)
                for turn in range(2):  # a non-default stream, the caller's buffers, twice
                    out = ds.denoise(col_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, out=mine, workspace=work, **par)
                    assert out is mine
                    _check(planes(mine), want, f"out= on a stream, turn {turn}, {par}")
                assert gathered.numpy()[: 24 * m].tobytes() == np.ascontiguousarray(colour.T).tobytes()  # (the input is left alone)
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*output too small"):
                ds.denoise(col_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, out=DeviceBuffer((3 * m - 1,), np.float64))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*workspace too small"):
                ds.denoise(col_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, workspace=DeviceBuffer((48 * m - 1,), np.uint8))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*overlaps the colour"):
                ds.denoise(col_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, out=DeviceSpan(gathered, 24 * m, 8))
            with pytest.raises(ValueError, match="device=True"):
                ds.denoise(colour, shape, normal, point, W, Hh, stream=st)
            with pytest.raises(ValueError, match="records"):
                ds.denoise(colour, shape, normal, point, W, Hh + 1)
            assert ds.denoise(np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), 0, 9).shape == (9, 0, 3)  # m = 0
            st.synchronize()
    finally:
        st.close()


LAUNCHES = [dict(PTRACE_DN_TILE="32x8"), dict(PTRACE_DN_TILE="16x16"), dict(PTRACE_DN_TILE="64x4"), dict(PTRACE_DN_VARIANT="direct"),
            dict(PTRACE_DN_VARIANT="lds", PTRACE_DN_BLOCKS="1"), dict(PTRACE_DN_TILE="16x16", PTRACE_DN_BLOCKS="7"),
            dict(PTRACE_DN_VARIANT="direct", PTRACE_DN_BLOCKS="2")]


@pytest.mark.parametrize("env", LAUNCHES, ids=["-".join(d.values()) for d in LAUNCHES])
def test_no_bit_depends_on_the_launch(demo, env):
    """Every legal tile of the LDS variant, the direct variant, and grids far smaller than the work (the grid-stride loops): the
    frame of the default launch -- which the tests above hold against the mirror -- in every bit."""
    W, Hh = 70, 33
    colour, shape, normal, point = hostile_frame(W, Hh, 6)
    assert not any(k in os.environ for k in ("PTRACE_DN_TILE", "PTRACE_DN_VARIANT", "PTRACE_DN_BLOCKS"))
    cases = (dict(passes=4, wrap_x=True, sigma_colour=0.7), dict(passes=5, same_shape=False, sigma_point=INF))
    want = [demo.denoise(colour, shape, normal, point, W, Hh, **par) for par in cases]
    _check(want[0], rb.denoise_host(colour, shape, normal, point, W, Hh, **cases[0]), "default launch")
    os.environ.update(env)
    try:
        got = [demo.denoise(colour, shape, normal, point, W, Hh, **par) for par in cases]
    finally:
        for k in env:
            del os.environ[k]
    for g, w, par in zip(got, want, cases):
        _check(g, w, f"{env} {par}")


# ---- 3. the exact cases of the host tests, on the device ----------------------------------------------------------------------------
def test_the_two_exact_cases_on_the_device(demo):
    W, Hh = 45, 19
    colour, shape, normal, point = coplanar_frame(W, Hh)
    got = demo.denoise(colour, shape, normal, point, W, Hh, passes=1, sigma_point=INF, normal_power_log2=0, sigma_colour=INF)
    assert np.ascontiguousarray(got[2:-2, 2:-2]).tobytes() == b3_blur_interior(colour).tobytes()
    flat = demo.denoise(np.full((Hh, W, 3), 0.75), shape, normal, point, W, Hh, passes=5)
    assert flat.tobytes() == np.full((Hh, W, 3), 0.75).tobytes()
    colour, shape, normal, point = two_shape_frame(W, Hh)
    for wrap in (False, True):
        assert demo.denoise(colour, shape, normal, point, W, Hh, passes=5, wrap_x=wrap).tobytes() == colour.tobytes(), wrap
    bled = demo.denoise(colour, shape, normal, point, W, Hh, passes=1, same_shape=False)
    assert bled.tobytes() != colour.tobytes()


# ---- 4. what it is for --------------------------------------------------------------------------------------------------------------
def test_the_denoised_gather_shader_its_pieces_and_its_error(demo_frames):
    """48 x 36, K = 4, 4 passes (the defaults).  Pieces: the frame is the mirror applied to the same gather and the same materials, bit
    for bit.  Error: its RMS error over the hit pixels against the same shader at K = 1024 unfiltered is LOWER than the unfiltered
    K = 4 frame's -- the asserted bound is the ratio 1.0, because the claim is "it denoises"; the ratio against unfiltered K = 16 is
    printed, not asserted (profiles/denoise_kernel.txt records both)."""
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.shaders import DenoisedGatherShader

    W, Hh, K = 48, 36, 4
    tracer, world, frame, wq = demo_frames(W, Hh)
    bg = hm.Color(0.0, 0.0, 0.0)
    shader = DenoisedGatherShader(world, tracer, samples=K)
    got = shader.shade_hits(frame)
    assert got.shape == (1, Hh, W, 3)
    gathered = wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, bg, 1, "none", init_seq=54)
    assert np.asarray(gathered.radiance).tobytes() == np.asarray(shader.last_gather.radiance).tobytes()
    mat = wq.materials(frame)
    hit = np.asarray(mat.hit)[0]
    assert hit.sum() > W * Hh // 2 and np.array_equal(hit, np.asarray(frame.shape_index)[0] >= 0)
    e = rb.denoise_host(gathered.radiance[0], frame.shape_index[0], frame.normal[0], frame.point[0], W, Hh)
    want = np.where(hit[..., None], np.asarray(mat.emitted)[0] + np.asarray(mat.brdf_color)[0] * e, 0.0)
    _check(got[0], want, "the shader's frame against its pieces")
    # through the tracer: the image holds that frame
    tracer.fire_all_rays(shader)
    assert np.array_equal(np.asarray(tracer.image.array, dtype=np.float64).reshape(Hh, W, 3), got[0])

    def unfiltered(k):
        return DenoisedGatherShader(world, tracer, samples=k, filtered=False).shade_hits(frame)[0]

    noisy = unfiltered(K)
    assert noisy.tobytes() == np.where(hit[..., None], np.asarray(mat.emitted)[0] + np.asarray(mat.brdf_color)[0] * np.asarray(gathered.radiance)[0],
                                       0.0).tobytes()
    reference, noisy16 = unfiltered(1024), unfiltered(16)
    rms = lambda a: float(np.sqrt(np.mean((a[hit] - reference[hit]) ** 2)))  # noqa: E731
    err, err4, err16 = rms(got[0]), rms(noisy), rms(noisy16)
    print(f"demo world {W}x{Hh}, {int(hit.sum())} hit pixels, RMS error against K = 1024 unfiltered: filtered K = {K} {err:.5f}, "
          f"unfiltered K = {K} {err4:.5f} (ratio {err / err4:.3f}), unfiltered K = 16 {err16:.5f} (ratio {err / err16:.3f})")
    for passes in (1, 2, 3, 5):
        other = DenoisedGatherShader(world, tracer, samples=K, passes=passes).shade_hits(frame)[0]
        print(f"    passes = {passes}: {rms(other):.5f} (ratio {rms(other) / err4:.3f})")
    assert err4 > 0.0 and err / err4 < 1.0


def test_the_denoised_light_map_of_a_sphere_and_its_seam(demo_frames):
    tracer, world, frame, wq = demo_frames(48, 36)
    flat = wq.scene.flat
    spheres = [s for s in range(flat.n_shapes) if flat.kind[s] == abi.SHAPE_SPHERE]
    shape, W, Hh, K = spheres[0], 32, 16, 4  # (the demo world's one sphere: what ARRIVES at it does not depend on its own BRDF)
    got = wq.denoised_light_map(shape, W, Hh, K, max_depth=2, passes=3)
    baked = wq.light_map(shape, W, Hh, K, max_depth=2, channels="none")
    points, normals = wq.surface_points(shape, rb.texel_centres(W, Hh))
    index = np.full((Hh, W), shape, np.int32)
    _check(got, rb.denoise_host(baked.radiance, index, normals, points, W, Hh, passes=3, wrap_x=True), "sphere: the wrap is the default")
    _check(wq.denoised_light_map(shape, W, Hh, K, wrap_u=False, max_depth=2, passes=3),
           rb.denoise_host(baked.radiance, index, normals, points, W, Hh, passes=3, wrap_x=False), "wrap_u=False")
    assert got.tobytes() != np.ascontiguousarray(baked.radiance).tobytes() and np.isfinite(got).all()
    # the seam: one perturbed texel in column 0 is read by column W - 1 of its row, and the other way round -- under the wrap alone
    values = np.array(baked.radiance)
    row = Hh // 2
    for col, across in ((0, W - 1), (W - 1, 0)):
        bumped = values.copy()
        bumped[row, col] += 1.0
        for wrap, reads in ((True, True), (False, False)):
            base = wq.denoised(values, (points, normals, shape), passes=1, wrap_x=wrap)
            out = wq.denoised(bumped, (points, normals, shape), passes=1, wrap_x=wrap)
            assert (out[row, across] != base[row, across]).any() == reads, (col, wrap)
            assert (out[row, col] != base[row, col]).all()
