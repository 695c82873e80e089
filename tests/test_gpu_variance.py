"""Variance queries on the device (include/ptrace_variance.h, libptrace_variance.so): the moments, the estimate and the
variance-guided filter against their numpy mirrors (``rays.luminance_moments_host``, ``variance_estimate_host``,
``variance_filter_host``), against themselves across entry points, streams and launch shapes, against the denoise query where the
luminance weight is off, and in what they are for -- ``rays.VarianceAccumulator`` over a sequence of frames and
``shaders.VarianceGuidedGatherShader``.

Expected agreement: bit for bit wherever the expected value is finite; where it is not, NaN where NaN is expected and infinities of
the same sign (``hostile_records.differing``).  The statistical claims are asserted as stated in their tests and no tighter."""
import os

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb
from pytracer_amd import scenes

from . import hostile_records as H
from . import surface_batches as S
from .test_variance_host import FLAGS, hostile_variance_frame, variance_parameter_sets

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
# the denoise tests' frames: narrower than a tile and than the stencil, a step above the frame (passes = 5 at 17 x 5), several tiles
# with partial edges in every sub-lattice (70 x 33; 150 x 12 for the 32-wide tile), PT_VR_WRAP_X across a seam
FRAMES = [(1, 1), (3, 2), (17, 5), (37, 23), (70, 33), (150, 12)]


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
def demo_tracers(dev):
    """(W, H) -> (tracer, world, queries, the demo camera) for the demo world at that size, made once for the module."""
    from pytracer_amd.tracer import GpuImageTracer

    made = {}

    def get(W, Hh):
        if (W, Hh) not in made:
            world, camera = scenes.demo_world()
            tracer = GpuImageTracer(hm.HdrImage(W, Hh), camera, samples_per_side=0)
            made[(W, Hh)] = (tracer, world, tracer.world_queries(world), camera)
        return made[(W, Hh)]

    yield get
    for tracer, _, _, _ in made.values():
        tracer.close()


def frame_of(tracer, world, camera):
    tracer.camera = camera
    return tracer.fire_all_hits(world)


def guides(frame):
    return np.asarray(frame.shape_index)[0], np.asarray(frame.normal)[0], np.asarray(frame.point)[0]


def _check(got, want, label):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    n = got.shape[0] * got.shape[1]
    got, want = got.reshape(n, -1), want.reshape(n, -1)
    bad = H.differing(got, want)
    assert bad.size == 0, f"{label}: {bad.size} of {len(want)} pixels differ, first {int(bad[0])}: got {got[bad[0]]}, want {want[bad[0]]}"


def _check_all_three(ds, colour, variance, shape, normal, point, moments, count, W, Hh, par, label):
    """The three queries' host forms against the mirrors for one parameter set -> the filtered colour."""
    _check(ds.variance_estimate(moments, count, shape, normal, point, W, Hh, **par)[..., None],
           rb.variance_estimate_host(moments, count, shape, normal, point, W, Hh, **par)[..., None], f"{label} estimate")
    got_c, got_v = ds.variance_filter(colour, variance, shape, normal, point, W, Hh, **par)
    want_c, want_v = rb.variance_filter_host(colour, variance, shape, normal, point, W, Hh, **par)
    assert got_c.shape == (Hh, W, 3) and got_v.shape == (Hh, W)
    _check(got_c, want_c, f"{label} filter colour")
    _check(got_v[..., None], want_v[..., None], f"{label} filter variance")
    return got_c, got_v


# ---- 1. the device against the mirrors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_synthetic_hostile_guides_equal_the_mirrors_bit_for_bit(demo, W, Hh):
    colour, variance, shape, normal, point, moments, count = hostile_variance_frame(W, Hh, 100 * W + Hh)
    _check(demo.variance_moments(colour, shape, W, Hh), rb.luminance_moments_host(colour, shape, W, Hh), f"{W}x{Hh} moments")
    changed = 0
    for par in variance_parameter_sets():
        got_c, got_v = _check_all_three(demo, colour, variance, shape, normal, point, moments, count, W, Hh, par, f"{W}x{Hh} {par}")
        miss = shape < 0
        if miss.any():  # a miss is copied, whatever it holds
            assert not H.differing(got_c.reshape(-1, 3)[miss], colour[miss]).size and not H.differing(got_v.reshape(-1, 1)[miss], variance[miss, None]).size
        changed += int((got_c.reshape(-1, 3)[~miss] != colour[~miss]).any())
    assert changed or W * Hh == 1  # (the filter did something)


@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_the_guides_of_a_real_hit_frame_equal_the_mirrors_bit_for_bit(demo_tracers, W, Hh):
    tracer, world, wq, camera = demo_tracers(W, Hh)
    frame = frame_of(tracer, world, camera)
    shape, normal, point = guides(frame)
    rng = np.random.default_rng(W + Hh)
    colour = rng.uniform(0.5, 1.5, (Hh, W, 3)) * rng.uniform(0.2, 3.0, 3)
    variance = rng.uniform(0.0, 0.2, (Hh, W)) ** 2
    lum = rng.uniform(0.5, 1.5, (Hh, W))
    moments = np.stack([lum, lum * lum + rng.uniform(0.0, 0.1, (Hh, W)), np.zeros((Hh, W))], axis=-1)
    count = rng.choice(np.array([0, 1, 2, 3, 4, 9, 2 ** 20], dtype=np.int32), (Hh, W))
    for par in variance_parameter_sets():
        _check_all_three(wq.scene, colour, variance, shape, normal, point, moments, count, W, Hh, par, f"{W}x{Hh} {par}")
    # the single-frame route through the queries: moments, a count of 1, the spatial estimate, the filter
    got_c, got_v = wq.variance_filtered(colour, frame, passes=3)
    var1 = rb.variance_estimate_host(rb.luminance_moments_host(colour, shape, W, Hh), np.ones((Hh, W), np.int32), shape, normal, point, W, Hh)
    want_c, want_v = rb.variance_filter_host(colour, var1, shape, normal, point, W, Hh, passes=3)
    _check(got_c, want_c, "the single-frame route: colour")
    _check(got_v[..., None], want_v[..., None], "the single-frame route: variance")


# ---- 2. entry points, buffers, streams, launch shapes -------------------------------------------------------------------------------
def test_host_forms_device_forms_out_workspace_and_a_stream(dev):
    """``device=True``: the hit frame rendered into a device buffer and a gather of it left in HBM; moments, one accumulation (for a
    count), the estimate and the filter read their inputs where they are -- on the default stream into buffers of their own, and on a
    non-default stream into the caller's, twice: the host forms' bits.  Then the refusals that need real device addresses."""
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
            g = rb.DeviceGuides.of_hit_buffer(hits, par_f, abi.HIT_ALL)
            shp_d, nrm_d, pnt_d = g.addresses()
            gathered = ds.gather(pnt_d, nrm_d, 2, 42, None, shp_d, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", device=True, stream=st, n=m)
            col_d = gathered.data_ptr()  # (the three radiance planes come first)
            colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(Hh, W, 3)
            shape, normal, point = guides(HitFrame(hits.numpy(), par_f, abi.HIT_ALL))
            assert (shape >= 0).sum() > m // 2 and len(np.unique(colour.reshape(-1, 3), axis=0)) > 10
            planes3 = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
            plane1 = lambda b: b.numpy()[:m].reshape(Hh, W)  # noqa: E731
            # moments
            want_mom = ds.variance_moments(colour, shape, W, Hh)
            _check(want_mom, rb.luminance_moments_host(colour, shape, W, Hh), "moments, host form")
            mom_d = ds.variance_moments(col_d, shp_d, W, Hh, device=True)
            _check(planes3(mom_d), want_mom, "moments, device form")
            mine = DeviceBuffer((3, m), np.float64)
            for turn in range(2):
                assert ds.variance_moments(col_d, shp_d, W, Hh, device=True, stream=st, out=mine) is mine
                _check(planes3(mine), want_mom, f"moments, out= on a stream, turn {turn}")
            # a count: one accumulation from an empty history (1 where something was hit)
            nowhere = (abi.CAMERA_PERSPECTIVE, [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0], 1.0, 1.0)  # (an empty history: not read)
            zero = ds.temporal_clear(DeviceBuffer((m,), np.int32), m, st)
            _, cnt_d = ds.temporal(col_d, shp_d, nrm_d, pnt_d, mine, shp_d, nrm_d, pnt_d, zero, nowhere, W, Hh, device=True, stream=st)
            count = cnt_d.numpy().reshape(Hh, W)
            assert np.array_equal(count, (shape >= 0).astype(np.int32))
            # the estimate
            for par in (dict(min_history=4), dict(min_history=1), dict(min_history=2, normal_min=0.99, point_tolerance=0.01, same_shape=False)):
                want_var = ds.variance_estimate(want_mom, count, shape, normal, point, W, Hh, **par)
                _check(want_var[..., None], rb.variance_estimate_host(want_mom, count, shape, normal, point, W, Hh, **par)[..., None], f"estimate {par}")
                var_d = ds.variance_estimate(mom_d, cnt_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, **par)
                _check(plane1(var_d)[..., None], want_var[..., None], f"estimate, device form {par}")
                mine1 = DeviceBuffer((m,), np.float64)
                for turn in range(2):
                    assert ds.variance_estimate(mom_d, cnt_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, out=mine1, **par) is mine1
                    _check(plane1(mine1)[..., None], want_var[..., None], f"estimate, out= on a stream, turn {turn}, {par}")
            assert (want_var > 0).any()
            var_d = ds.variance_estimate(mom_d, cnt_d, shp_d, nrm_d, pnt_d, W, Hh, device=True)
            variance = plane1(var_d)
            # the filter
            for par in (dict(passes=4, wrap_x=True), dict(passes=1), dict(passes=3, sigma_luminance=0.5, same_shape=False), dict(passes=2, sigma_luminance=INF)):
                want_c, want_v = ds.variance_filter(colour, variance, shape, normal, point, W, Hh, **par)
                mirror = rb.variance_filter_host(colour, variance, shape, normal, point, W, Hh, **par)
                _check(want_c, mirror[0], f"filter, host form {par}")
                _check(want_v[..., None], mirror[1][..., None], f"filter variance, host form {par}")
                fresh_c, fresh_v = ds.variance_filter(col_d, var_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, **par)  # the default stream
                _check(planes3(fresh_c), want_c, f"filter, device form {par}")
                _check(plane1(fresh_v)[..., None], want_v[..., None], f"filter variance, device form {par}")
                out_c, out_v = DeviceBuffer((3, m), np.float64), DeviceBuffer((m,), np.float64)
                work = DeviceBuffer((ds.variance_workspace_bytes(W, Hh, **par),), np.uint8)
                assert work.nbytes == m * (64 if par["passes"] > 1 else 32)
                for turn in range(2):  # a non-default stream, the caller's buffers, twice
                    got = ds.variance_filter(col_d, var_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, out=out_c, out_variance=out_v,
                                             workspace=work, **par)
                    assert got[0] is out_c and got[1] is out_v
                    _check(planes3(out_c), want_c, f"filter, out= on a stream, turn {turn}, {par}")
                    _check(plane1(out_v)[..., None], want_v[..., None], f"filter variance, out= on a stream, turn {turn}, {par}")
                assert gathered.numpy()[: 24 * m].tobytes() == np.ascontiguousarray(colour.reshape(-1, 3).T).tobytes()  # (the inputs are left alone)
                assert plane1(var_d).tobytes() == variance.tobytes()
            # refusals, with real device addresses
            call = lambda **kw: ds.variance_filter(col_d, var_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, **kw)  # noqa: E731
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*colour output too small"):
                call(out=DeviceBuffer((3 * m - 1,), np.float64))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*variance output too small"):
                call(out_variance=DeviceBuffer((m - 1,), np.float64))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*workspace too small"):
                call(workspace=DeviceBuffer((64 * m - 1,), np.uint8))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*the colour output overlaps the colour planes"):
                call(out=DeviceSpan(gathered, 24 * m, 8))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*the variance output overlaps the variance plane"):
                call(out_variance=var_d)
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*the colour output overlaps the workspace"):
                call(out=DeviceSpan(work, 24 * m, 0), workspace=work)
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*the variance output overlaps the moments"):
                ds.variance_estimate(mom_d, cnt_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, out=DeviceSpan(mom_d, 8 * m, 16 * m))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*variance output too small"):
                ds.variance_estimate(mom_d, cnt_d, shp_d, nrm_d, pnt_d, W, Hh, device=True, stream=st, out=DeviceBuffer((m - 1,), np.float64))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*the moments output overlaps the colour planes"):
                ds.variance_moments(col_d, shp_d, W, Hh, device=True, stream=st, out=DeviceSpan(gathered, 24 * m, 0))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*moments output too small"):
                ds.variance_moments(col_d, shp_d, W, Hh, device=True, stream=st, out=DeviceBuffer((3 * m - 1,), np.float64))
            with pytest.raises(ValueError, match="device=True"):
                ds.variance_filter(colour, variance, shape, normal, point, W, Hh, stream=st)
            with pytest.raises(ValueError, match="records"):
                ds.variance_filter(colour, variance, shape, normal, point, W, Hh + 1)
            empty3, empty1, emptyi = np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int32)
            out = ds.variance_filter(empty3, empty1, emptyi, empty3, empty3, 0, 9)  # m = 0
            assert out[0].shape == (9, 0, 3) and out[1].shape == (9, 0)
            assert ds.variance_estimate(empty3, emptyi, emptyi, empty3, empty3, 0, 9).shape == (9, 0) and ds.variance_moments(empty3, emptyi, 9, 0).shape == (0, 9, 3)
            st.synchronize()
    finally:
        st.close()


LAUNCHES = [dict(PTRACE_VR_TILE="32x8"), dict(PTRACE_VR_TILE="16x16"), dict(PTRACE_VR_TILE="64x4"), dict(PTRACE_VR_VARIANT="direct"),
            dict(PTRACE_VR_VARIANT="lds", PTRACE_VR_BLOCKS="1"), dict(PTRACE_VR_TILE="16x16", PTRACE_VR_BLOCKS="7"),
            dict(PTRACE_VR_VARIANT="direct", PTRACE_VR_BLOCKS="2"), dict(PTRACE_VR_TILE="64x4", PTRACE_VR_BLOCKS="3")]


@pytest.mark.parametrize("env", LAUNCHES, ids=["-".join(d.values()) for d in LAUNCHES])
def test_no_bit_depends_on_the_launch(demo, env):
    """Every legal tile of the LDS variant, the direct variant, and grids far smaller than the work (the grid-stride loops): the
    outputs of the default launch -- which the tests above hold against the mirrors -- in every bit, for all three queries."""
    W, Hh = 70, 33
    colour, variance, shape, normal, point, moments, count = hostile_variance_frame(W, Hh, 6)
    assert not any(k in os.environ for k in ("PTRACE_VR_TILE", "PTRACE_VR_VARIANT", "PTRACE_VR_BLOCKS"))
    cases = (dict(passes=4, wrap_x=True, sigma_luminance=0.7), dict(passes=5, same_shape=False, sigma_point=INF, min_history=100))

    def run():
        out = [demo.variance_moments(colour, shape, W, Hh)]
        for par in cases:
            out.append(demo.variance_estimate(moments, count, shape, normal, point, W, Hh, **par)[..., None])
            c, v = demo.variance_filter(colour, variance, shape, normal, point, W, Hh, **par)
            out += [c, v[..., None]]
        return out

    want = run()
    _check(want[2], rb.variance_filter_host(colour, variance, shape, normal, point, W, Hh, **cases[0])[0], "default launch")
    os.environ.update(env)
    try:
        got = run()
    finally:
        for k in env:
            del os.environ[k]
    for i, (g, w) in enumerate(zip(got, want)):
        _check(g, w, f"{env} output {i}")


# ---- 3. against the parent's filter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 4, 5])
def test_without_the_luminance_weight_the_colour_is_the_denoise_query_on_the_device(demo, passes):
    for W, Hh in ((17, 5), (70, 33)):
        colour, variance, shape, normal, point, _, _ = hostile_variance_frame(W, Hh, 9 * W + passes)
        colour = np.where(np.isfinite(colour) & (np.abs(colour) < 1e100), colour, 3e99)
        for i, (same, wrap) in enumerate(FLAGS):
            geo = dict(passes=passes, same_shape=same, wrap_x=wrap, normal_power_log2=(0, 5, 10, 5)[i], sigma_point=(0.3, INF, 0.1, 0.2)[i])
            got, _ = demo.variance_filter(colour, variance, shape, normal, point, W, Hh, sigma_luminance=INF, **geo)
            want = demo.denoise(colour, shape, normal, point, W, Hh, sigma_colour=INF, **geo)
            assert got.tobytes() == want.tobytes(), (W, Hh, geo)


def test_the_exact_cases_on_the_device(demo):
    W, Hh = 45, 19
    colour, variance, shape, normal, point, _, _ = hostile_variance_frame(W, Hh, 5)
    flat = np.full((Hh * W, 3), 0.5)
    for same, wrap in FLAGS:
        out, var = demo.variance_filter(flat, np.zeros(Hh * W), shape, normal, point, W, Hh, passes=5, same_shape=same, wrap_x=wrap)
        assert out.tobytes() == flat.tobytes() and var.tobytes() == np.zeros((Hh, W)).tobytes()
        positive = np.where(variance >= 0, variance, 0.25)
        _, var = demo.variance_filter(np.where(np.isfinite(colour), colour, 1.0), positive, shape, normal, point, W, Hh, same_shape=same, wrap_x=wrap)
        assert not (var < 0).any()
    half = rb.luminance_moments_host(flat, shape, W, Hh)
    for min_history in (1, 100):
        var = demo.variance_estimate(half, np.full(W * Hh, 6, np.int32), shape, normal, point, W, Hh, min_history=min_history)
        assert var.tobytes() == np.zeros((Hh, W)).tobytes()


# ---- 4. what it is for --------------------------------------------------------------------------------------------------------------
def test_six_updates_of_the_variance_accumulator_on_the_host_and_in_hbm(dev):
    """48 x 36, the camera stepped 1 degree per frame, 4-sample gathers, 6 frames.  Host mode equals the chain of mirrors --
    ``temporal_host`` twice (colour, moments), then the estimate mirror -- bit for bit; ``device=True`` (hit frames alternating between
    two device buffers, everything in HBM) equals host mode bit for bit; its ``count`` is a plain ``TemporalAccumulator``'s."""
    from pytracer_amd import flatten
    from pytracer_amd.devmem import DeviceBuffer, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh, K, N = 48, 36, 4, 6
    m = W * Hh
    world, camera = scenes.demo_world()
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    params = dict(max_history=4, min_history=3)
    st = Stream()
    try:
        with dev.DeviceScene(S.world("demo")[0]) as ds:
            wq = rb.WorldQueries(ds)
            on_device = rb.VarianceAccumulator(wq, device=True, stream=st, **params)
            on_host = rb.VarianceAccumulator(wq, **params)
            plain = rb.TemporalAccumulator(wq, max_history=4)
            buffers = [DeviceBuffer((abi.hits_bytes(par_f, abi.HIT_ALL),), np.uint8) for _ in range(2)]
            prev_c = prev_m = rb.TemporalHistory.empty(W, Hh)
            prev_camera = camera
            for f in range(N):
                now = scenes.turned_camera(camera, 1.0 * f)
                hits = buffers[f & 1]
                ds.render_hits_into(flatten.flatten_camera(now), par_f, abi.HIT_ALL, hits, stream=st)
                g = rb.DeviceGuides.of_hit_buffer(hits, par_f, abi.HIT_ALL)
                gathered = ds.gather(g.point, g.normal, K, 42, None, g.shape_index, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", init_seq=54 + f * m * K,
                                     device=True, stream=st, n=m)
                out_d, var_d = on_device.update(gathered, g, now, width=W, height=Hh)
                colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(Hh, W, 3)
                shape, normal, point = guides(HitFrame(hits.numpy(), par_f, abi.HIT_ALL))
                # the chain of mirrors
                want_c = rb.temporal_host(colour, shape, normal, point, prev_c.colour, prev_c.shape_index, prev_c.normal, prev_c.point, prev_c.count,
                                          prev_camera, W, Hh, max_history=4)
                want_m = rb.temporal_host(rb.luminance_moments_host(colour, shape, W, Hh), shape, normal, point, prev_m.colour, prev_m.shape_index,
                                          prev_m.normal, prev_m.point, prev_m.count, prev_camera, W, Hh, max_history=4)
                assert np.array_equal(want_c[1], want_m[1])  # (the same taps, the same count)
                want_v = rb.variance_estimate_host(want_m[0], want_m[1], shape, normal, point, W, Hh, min_history=3)
                # host mode
                got_c, got_v = on_host.update(colour, (point, normal, shape), now)
                _check(got_c, want_c[0], f"update {f}: host mode, colour")
                _check(got_v[..., None], want_v[..., None], f"update {f}: host mode, variance")
                assert np.array_equal(on_host.count, want_c[1]) and on_host.frames == f + 1
                # all in HBM
                _check(np.ascontiguousarray(out_d.numpy()[:, :m].T).reshape(Hh, W, 3), got_c, f"update {f}: device mode, colour")
                _check(var_d.numpy()[:m].reshape(Hh, W, 1), got_v[..., None], f"update {f}: device mode, variance")
                assert np.array_equal(on_device.count.numpy()[:m].reshape(Hh, W), on_host.count)
                plain.update(colour, (point, normal, shape), now)
                assert np.array_equal(plain.count, on_host.count)
                assert want_c[1].max() == min(f + 1, 4) and (f < 2 or ((want_v > 0) & (want_c[1] >= 3)).any())
                prev_c = rb.TemporalHistory(want_c[0], shape.copy(), normal.copy(), point.copy(), want_c[1])
                prev_m = rb.TemporalHistory(want_m[0], shape.copy(), normal.copy(), point.copy(), want_m[1])
                prev_camera = now
            st.synchronize()
    finally:
        st.close()


def _shadow_region(frame):
    """The ground-plane pixels (shape 1 of the demo world, the plane z = 0) within two radii of the foot of its one sphere (radius 1,
    foot at the origin): where the contact shadow lies."""
    shape, _, point = guides(frame)
    return (shape == 1) & (np.hypot(point[..., 0], point[..., 1]) <= 2.0)


def quality_figures(demo_tracers, sigmas=(1.0, 2.0, 4.0, 8.0), step=1.0):
    """Demo world, 48 x 36, 8 frames of 4 samples, the camera turning ``step`` degrees per frame; the reference is a 1024-sample
    gather at the last camera.  RMS error of E over the hit pixels and over the shadow region for (a) accumulate + geometry-only
    filter, (b) accumulate + variance-guided filter per ``sigma_luminance``, (c) accumulate alone -> dict."""
    W, Hh, K, N = 48, 36, 4, 8
    tracer, world, wq, camera = demo_tracers(W, Hh)
    bg = hm.Color(0.0, 0.0, 0.0)
    acc = rb.VarianceAccumulator(wq)
    for f in range(N):
        frame = frame_of(tracer, world, scenes.turned_camera(camera, step * f))
        gathered = wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, bg, 1, "none", init_seq=54 + f * W * Hh * K)
        e, variance = acc.update(np.asarray(gathered.radiance)[0], frame, tracer.camera)
    reference = np.asarray(wq.hemisphere_radiance(frame, 1024, 42, None, 1, 10, 3, bg, 1, "none", init_seq=54 + N * W * Hh * K).radiance)[0]
    hit, shadow = guides(frame)[0] >= 0, _shadow_region(frame)
    rms = lambda a, where: float(np.sqrt(np.mean((a[where] - reference[where]) ** 2)))  # noqa: E731
    geometry = wq.denoised(e, frame)
    out = dict(hit=int(hit.sum()), shadow=int(shadow.sum()), a=(rms(geometry, hit), rms(geometry, shadow)), c=(rms(e, hit), rms(e, shadow)), b={},
               mean_history=float(acc.count[hit].mean()))
    for sigma in sigmas:
        guided, _ = wq.variance_filtered(e, frame, variance=variance, sigma_luminance=sigma)
        out["b"][sigma] = (rms(guided, hit), rms(guided, shadow))
    return out


def test_the_variance_guided_filter_is_closer_to_the_converged_frame_than_accumulation_alone(demo_tracers):
    """Asserted, for the default ``sigma_luminance`` over the hit pixels: (b) <= (c), the RMS error of accumulate + variance-guided
    filter against that of accumulation alone -- the claim is "it denoises", so the bound is the ratio 1.0.  And against (a), the
    parent's accumulate + geometry-only filter, in the shadow region, where an illumination edge lies inside one shape: the sequence
    is deterministic, and the recorded ratio (b) / (a) there is 0.278 (profiles/variance_kernel.txt, with the whole sweep); asserted
    with a margin of 10 %.  Printed, not asserted: in the shadow region accumulation ALONE is closer than either filter."""
    from pytracer_amd import _variance_lib

    q = quality_figures(demo_tracers, sigmas=(_variance_lib.DEFAULTS["sigma_luminance"],))
    (b_all, b_shadow), = q["b"].values()
    print(f"demo world 48x36, {q['hit']} hit pixels ({q['shadow']} in the shadow region), mean history {q['mean_history']:.2f}; RMS error of E against "
          f"K = 1024, whole frame / shadow region: (a) geometry-only {q['a'][0]:.5f} / {q['a'][1]:.5f}, (b) variance-guided {b_all:.5f} / "
          f"{b_shadow:.5f}, (c) accumulated alone {q['c'][0]:.5f} / {q['c'][1]:.5f}; (b) / (a) in the shadow region {b_shadow / q['a'][1]:.4f}")
    assert q["shadow"] > 20 and q["c"][0] > 0.0 and b_all <= q["c"][0]
    assert b_shadow / q["a"][1] <= 0.278 * 1.1


def test_the_variance_guided_gather_shader_and_its_pieces(demo_tracers):
    from pytracer_amd.shaders import VarianceGuidedGatherShader

    W, Hh, K = 48, 36, 4
    tracer, world, wq, camera = demo_tracers(W, Hh)
    bg = hm.Color(0.0, 0.0, 0.0)
    shader = VarianceGuidedGatherShader(world, tracer, samples=K, passes=3, sigma_luminance=2.0, max_history=8, min_history=2)
    acc = rb.VarianceAccumulator(wq, max_history=8, min_history=2)
    for f in range(3):
        frame = frame_of(tracer, world, scenes.turned_camera(camera, 1.0 * f))
        got = shader.shade_hits(frame)
        assert got.shape == (1, Hh, W, 3)
        gathered = wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, bg, 1, "none", init_seq=54 + f * W * Hh * K)
        assert np.asarray(gathered.radiance).tobytes() == np.asarray(shader.last_gather.radiance).tobytes()
        e, variance = acc.update(np.asarray(gathered.radiance)[0], frame, tracer.camera)
        assert np.array_equal(variance, shader.last_variance)
        filtered, _ = wq.variance_filtered(e, frame, variance=variance, passes=3, sigma_luminance=2.0)
        mat = wq.materials(frame)
        hit = np.asarray(mat.hit)[0]
        want = np.where(hit[..., None], np.asarray(mat.emitted)[0] + np.asarray(mat.brdf_color)[0] * filtered, 0.0)
        _check(got[0], want, f"frame {f}: the shader's frame against its pieces")
    assert shader.frame_no == 3 and shader.accumulator.count.max() == 3
    # through the tracer: the image holds that frame; without accumulation: the single-frame route, history and frame number left alone
    shader.accumulate = False
    tracer.fire_all_rays(shader)
    alone = np.asarray(tracer.image.array, dtype=np.float64).reshape(Hh, W, 3).copy()
    assert shader.frame_no == 3 and np.isfinite(alone).all() and not np.array_equal(alone, got[0])
    gathered = wq.hemisphere_radiance(frame, K, 42, None, 1, 10, 3, bg, 1, "none", init_seq=54 + 3 * W * Hh * K)
    single, _ = wq.variance_filtered(gathered, frame, passes=3, sigma_luminance=2.0, min_history=2)
    _check(alone, np.where(hit[..., None], np.asarray(mat.emitted)[0] + np.asarray(mat.brdf_color)[0] * single, 0.0), "the single-frame route")
