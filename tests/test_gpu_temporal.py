"""Accumulate queries on the device (include/ptrace_temporal.h, libptrace_temporal.so): the reprojection kernel against its numpy
mirror (``rays.temporal_host``), against itself across entry points, streams and launch shapes, and in what it is for -- a sequence
of gather frames whose mean is carried from frame to frame (``rays.TemporalAccumulator``, ``shaders.TemporalGatherShader``).

Expected agreement: bit for bit wherever the expected value is finite; where it is not, NaN where NaN is expected and infinities of
the same sign (``hostile_records.differing``); the history lengths exactly.  The one statistical claim -- eight accumulated frames are
closer to a converged one than a single frame -- is asserted as that and no tighter: any tighter figure would come from the code
under test."""
import os

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb
from pytracer_amd import scenes

from . import hostile_records as H
from . import surface_batches as S
from .test_temporal_host import cameras, wall_frame

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
# one workgroup takes 256 pixels: 1 x 1 to 37 x 23 are one to four of them with a ragged last one, 70 x 33 is ten
FRAMES = [(1, 1), (3, 2), (17, 5), (37, 23), (70, 33)]
# max_history 1, 2 and 32 x the flag on and off x normal_min -1 and 0.9 x point_tolerance finite and inf
PARAMETERS = [dict(max_history=h, same_shape=s, normal_min=n, point_tolerance=t) for h in (1, 2, 32) for s in (True, False) for n in (-1.0, 0.9)
              for t in (0.05, INF)]


def moved(camera, how):
    """The camera of the frame after ``camera``'s: the same, turned by 1 or 20 degrees about z, or translated."""
    import copy

    if how == "same":
        return camera
    if how == "translated":
        out = copy.copy(camera)
        out.transformation = hm.translation(hm.Vec(0.3, -0.2, 0.1)) * camera.transformation
        return out
    return scenes.turned_camera(camera, {"turned1": 1.0, "turned20": 20.0}[how])


MOVES = ("same", "turned1", "turned20", "translated")
CASES = [(kind, how) for kind in ("perspective", "orthogonal") for how in MOVES]  # eight: every parameter set is used by one of them


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
    """(W, H) -> (tracer, world, queries, the demo camera) for the demo world at that size, made once for the module; a frame of
    another camera is ``frame_of(tracer, world, camera)``."""
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


def hostile(colour, shape, normal, point, seed, counts=False):
    """Copies of a frame's planes with records nobody vouches for sprinkled in: shape indices -1, -2^31, 1000 and 2^31 - 1; normals
    of any length, zero, NaN, infinite and 1e200; points NaN, infinite and 1e300; colours NaN, infinite and 1e300.  ``counts``: also
    -> history lengths of 1 to 40 with 0, negative ones and 2^31 - 1 among them."""
    rng = np.random.default_rng(seed)
    Hh, W = shape.shape
    m = W * Hh
    colour, shape, normal, point = (np.array(a).reshape(m, -1) for a in (colour, shape, normal, point))
    shape = shape.reshape(m)
    normal = normal * np.exp(rng.uniform(-2, 2, (m, 1))) + rng.normal(0, 0.02, (m, 3))
    point = point + rng.normal(0, 0.002, (m, 3))
    pick = lambda share: np.flatnonzero(rng.uniform(0, 1, m) < share)  # noqa: E731
    for rows, value in ((pick(0.06), -1), (pick(0.02), -2 ** 31), (pick(0.03), 1000), (pick(0.02), 2 ** 31 - 1)):
        shape[rows] = value
    for rows, value in ((pick(0.03), (0.0, 0.0, 0.0)), (pick(0.02), (NAN, 0.0, 1.0)), (pick(0.02), (0.0, INF, 1.0)), (pick(0.01), (-INF, INF, NAN)),
                        (pick(0.02), (-1e200, 1e200, 1e200)), (pick(0.02), (-1e-200, 0.0, 1e-200))):
        normal[rows] = value
    for rows, value in ((pick(0.02), (NAN, 0.0, 0.0)), (pick(0.02), (0.0, INF, 0.0)), (pick(0.01), (1e300, -1e300, 1e300)), (pick(0.01), (1e200, 0.0, 0.0))):
        point[rows] = value
    for rows, value in ((pick(0.02), (NAN, 1.0, 1.0)), (pick(0.02), (1.0, INF, 1.0)), (pick(0.02), (1e300, 1.0, 1.0)), (pick(0.01), (-INF, NAN, 1e300))):
        colour[rows] = value
    out = [colour.reshape(Hh, W, 3), shape.reshape(Hh, W), normal.reshape(Hh, W, 3), point.reshape(Hh, W, 3)]
    if counts:
        count = rng.integers(1, 41, m).astype(np.int32)
        for rows, value in ((pick(0.05), 0), (pick(0.03), -1), (pick(0.01), -2 ** 31), (pick(0.03), 2 ** 31 - 1), (pick(0.02), 2 ** 20)):
            count[rows] = value
        out.append(count.reshape(Hh, W))
    return out


def _check(got, want, label):
    (got_c, got_n), (want_c, want_n) = got, want
    got_c, want_c = np.ascontiguousarray(got_c).reshape(-1, 3), np.ascontiguousarray(want_c).reshape(-1, 3)
    bad = H.differing(got_c, want_c)
    assert bad.size == 0, f"{label}: {bad.size} of {len(want_c)} pixels differ, first {int(bad[0])}: got {got_c[bad[0]]}, want {want_c[bad[0]]}"
    got_n, want_n = np.asarray(got_n).reshape(-1), np.asarray(want_n).reshape(-1)
    assert got_n.dtype == want_n.dtype == np.int32
    off = np.flatnonzero(got_n != want_n)
    assert off.size == 0, f"{label}: {off.size} history lengths differ, first {int(off[0])}: got {got_n[off[0]]}, want {want_n[off[0]]}"


# ---- 1. the device against the mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_synthetic_hostile_guides_equal_the_mirror_bit_for_bit(demo, W, Hh):
    reused = blended = 0
    for i, (kind, how) in enumerate(CASES):
        before = cameras(aspect=W / Hh)[kind]
        now = moved(before, how)
        rng = np.random.default_rng(1000 * W + i)
        prev = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *wall_frame(before, W, Hh, split=-1.4)[1:], seed=10 * i + 1, counts=True)
        cur = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *wall_frame(now, W, Hh, split=-1.4)[1:], seed=10 * i + 2)
        for j in range(3):
            par = PARAMETERS[(3 * i + j) % len(PARAMETERS)]
            want = rb.temporal_host(*cur, *prev, before, W, Hh, **par)
            got = demo.temporal(*cur, *prev, before, W, Hh, **par)
            assert got[0].shape == (Hh, W, 3) and got[1].shape == (Hh, W)
            _check(got, want, f"{W}x{Hh} {kind} {how} {par}")
            miss = cur[1] < 0
            if miss.any():  # a miss is copied, whatever it holds, and has no history
                _check((got[0][miss], got[1][miss]), (cur[0][miss], np.zeros(int(miss.sum()), np.int32)), f"{W}x{Hh} {kind} {how} {par}: the misses")
            assert (got[1][~miss] >= 1).all() and (got[1] <= par["max_history"]).all()
            reused += int((got[1] >= 2).sum())
            blended += int(((got[0] != cur[0]).any(axis=-1) & ~miss).sum())
    assert W * Hh < 10 or (reused and blended)  # (the history was used)


@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_the_guides_of_real_hit_frames_equal_the_mirror_bit_for_bit(demo_tracers, W, Hh):
    tracer, world, wq, demo_camera = demo_tracers(W, Hh)
    ortho = hm.OrthogonalCamera(W / Hh, hm.rotation_z(30.0) * hm.translation(hm.Vec(-4.0, 0.0, 1.0)) * hm.scaling(hm.Vec(1.0, 2.0, 2.0)))
    reused = 0
    for i, (before, how) in enumerate((c, how) for c in (demo_camera, ortho) for how in MOVES):
        rng = np.random.default_rng(W + Hh + i)
        last, this = frame_of(tracer, world, before), frame_of(tracer, world, moved(before, how))
        count = rng.integers(-2, 40, (Hh, W)).astype(np.int32)
        prev = rb.TemporalHistory(rng.uniform(0.5, 1.5, (Hh, W, 3)), *guides(last), count)
        colour = rng.uniform(0.5, 1.5, (Hh, W, 3)) * rng.uniform(0.2, 3.0, 3)
        for j in range(3):
            par = PARAMETERS[(3 * i + j) % len(PARAMETERS)]
            want = rb.temporal_host(colour, *guides(this), prev.colour, prev.shape_index, prev.normal, prev.point, prev.count, before, W, Hh, **par)
            got = wq.accumulated(colour, this, prev, before, **par)
            _check((got.colour, got.count), want, f"{W}x{Hh} camera {i} {how} {par}")
            reused += int((got.count >= 2).sum())
    assert reused or W * Hh < 10


# ---- 2. entry points, buffers, streams, launch shapes -------------------------------------------------------------------------------
def test_host_form_device_form_out_and_a_stream(dev):
    """``device=True``: two hit frames rendered into device buffers and a gather of each left in HBM, the accumulation reading all
    nine inputs where they are -- on the default stream into buffers of its own, and on a non-default stream into the caller's,
    twice: the host form's bits, and the inputs untouched."""
    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, DeviceSpan, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh = 70, 33
    m = W * Hh
    world, camera = scenes.demo_world()
    flat, cam_a = S.world("demo")
    from pytracer_amd import flatten

    turned = scenes.turned_camera(camera, 3.0)
    cam_b = flatten.flatten_camera(turned)
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    st = Stream()
    try:
        with dev.DeviceScene(flat) as ds:
            frames = []
            for cam, seq in ((cam_a, 54), (cam_b, 54 + 2 * m)):
                hits = DeviceBuffer((abi.hits_bytes(par_f, abi.HIT_ALL),), np.uint8)
                ds.render_hits_into(cam, par_f, abi.HIT_ALL, hits, stream=st)
                g = rb.DeviceGuides.of_hit_buffer(hits, par_f, abi.HIT_ALL)
                gathered = ds.gather(g.point, g.normal, 2, 42, None, g.shape_index, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", init_seq=seq, device=True,
                                     stream=st, n=m)
                frame = HitFrame(hits.numpy(), par_f, abi.HIT_ALL)
                colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(Hh, W, 3)
                frames.append((g, gathered, hits.numpy().tobytes(), colour) + guides(frame))
            (g0, gat0, hits0, col0, shp0, nrm0, pnt0), (g1, gat1, hits1, col1, shp1, nrm1, pnt1) = frames
            assert (shp1 >= 0).sum() > m // 2 and len(np.unique(col1.reshape(-1, 3), axis=0)) > 10
            planes = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
            # frame 0 from an empty history, on the device: its lengths are the device's own int plane for frame 1
            zero = ds.temporal_clear(DeviceBuffer((m,), np.int32), stream=st)
            assert not zero.numpy().any()
            acc0, cnt0 = ds.temporal(gat0, g0.shape_index, g0.normal, g0.point, gat1, g1.shape_index, g1.normal, g1.point, zero, camera, W, Hh,
                                     device=True, stream=st)
            empty = rb.TemporalHistory.empty(W, Hh)
            want0 = rb.temporal_host(col0, shp0, nrm0, pnt0, empty.colour, empty.shape_index, empty.normal, empty.point, empty.count, camera, W, Hh)
            _check((planes(acc0), cnt0.numpy().reshape(Hh, W)), want0, "the first frame, device form")
            assert np.array_equal(want0[1], (shp0 >= 0).astype(np.int32)) and want0[0].tobytes() == col0.tobytes()
            for par in (dict(), dict(max_history=1), dict(same_shape=False, normal_min=-1.0, point_tolerance=INF)):
                want = ds.temporal(col1, shp1, nrm1, pnt1, want0[0], shp0, nrm0, pnt0, want0[1], camera, W, Hh, **par)
                _check(want, rb.temporal_host(col1, shp1, nrm1, pnt1, want0[0], shp0, nrm0, pnt0, want0[1], camera, W, Hh, **par), f"host form {par}")
                args = (gat1, g1.shape_index, g1.normal, g1.point, acc0, g0.shape_index, g0.normal, g0.point, cnt0, camera, W, Hh)
                fresh = ds.temporal(*args, device=True, **par)  # the default stream, buffers of its own
                _check((planes(fresh[0]), fresh[1].numpy().reshape(Hh, W)), want, f"device form {par}")
                mine, mine_n = DeviceBuffer((3, m), np.float64), DeviceBuffer((m,), np.int32)
                for turn in range(2):  # a non-default stream, the caller's buffers, twice
                    out = ds.temporal(*args, device=True, stream=st, out=mine, out_count=mine_n, **par)
                    assert out[0] is mine and out[1] is mine_n
                    _check((planes(mine), mine_n.numpy().reshape(Hh, W)), want, f"out= on a stream, turn {turn}, {par}")
                # (the inputs are left alone)
                assert gat1.numpy()[: 24 * m].tobytes() == np.ascontiguousarray(col1.reshape(m, 3).T).tobytes()
                assert planes(acc0).tobytes() == want0[0].tobytes() and cnt0.numpy().tobytes() == want0[1].tobytes()
                assert [g.keep.numpy().tobytes() for g in (g0, g1)] == [hits0, hits1]
            if (want[1] >= 2).sum() == 0:
                pytest.fail("a 3 degree step left no history: the test does not test")
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*colour output too small"):
                ds.temporal(*args, device=True, stream=st, out=DeviceBuffer((3 * m - 1,), np.float64))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*count output too small"):
                ds.temporal(*args, device=True, stream=st, out_count=DeviceBuffer((m - 1,), np.int32))
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the previous colour"):
                ds.temporal(*args, device=True, stream=st, out=acc0)
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*count output overlaps the previous counts"):
                ds.temporal(*args, device=True, stream=st, out_count=cnt0)
            with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the colour"):
                ds.temporal(*args, device=True, stream=st, out=DeviceSpan(gat1, 24 * m, 8))
            with pytest.raises(ValueError, match="device=True"):
                ds.temporal(col1, shp1, nrm1, pnt1, want0[0], shp0, nrm0, pnt0, want0[1], camera, W, Hh, stream=st)
            with pytest.raises(ValueError, match="records"):
                ds.temporal(col1, shp1, nrm1, pnt1, want0[0], shp0, nrm0, pnt0, want0[1], camera, W, Hh + 1)
            none3, none1 = np.zeros((0, 3)), np.zeros(0, np.int32)
            out, count = ds.temporal(none3, none1, none3, none3, none3, none1, none3, none3, none1, camera, 0, 9)  # m = 0
            assert out.shape == (9, 0, 3) and count.shape == (9, 0)
            st.synchronize()
    finally:
        st.close()


@pytest.mark.parametrize("blocks", ["1", "2", "7"])
def test_no_bit_depends_on_the_launch(demo, blocks):
    """Grids far smaller than the work (the grid-stride loop; ten workgroups by default): the frame of the default launch -- which the
    tests above hold against the mirror -- in every bit."""
    W, Hh = 70, 33
    before = cameras(aspect=W / Hh)["perspective"]
    rng = np.random.default_rng(6)
    prev = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *wall_frame(before, W, Hh, split=-1.4)[1:], seed=61, counts=True)
    cur = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *wall_frame(moved(before, "turned1"), W, Hh, split=-1.4)[1:], seed=62)
    assert "PTRACE_TA_BLOCKS" not in os.environ
    cases = (dict(), dict(max_history=2, same_shape=False, point_tolerance=INF))
    want = [demo.temporal(*cur, *prev, before, W, Hh, **par) for par in cases]
    _check(want[0], rb.temporal_host(*cur, *prev, before, W, Hh, **cases[0]), "default launch")
    os.environ["PTRACE_TA_BLOCKS"] = blocks
    try:
        got = [demo.temporal(*cur, *prev, before, W, Hh, **par) for par in cases]
    finally:
        del os.environ["PTRACE_TA_BLOCKS"]
    for g, w, par in zip(got, want, cases):
        _check(g, w, f"{blocks} workgroups {par}")


# ---- 3. the exact cases of the host tests, on the device ----------------------------------------------------------------------------
def test_the_exact_cases_on_the_device(demo):
    W, Hh, max_history = 45, 19, 4
    for kind in ("perspective", "orthogonal"):
        camera = cameras(aspect=W / Hh)[kind]
        colour, shape, normal, point = wall_frame(camera, W, Hh, colours=(0.5, 0.5))
        assert (shape >= 0).sum() > W * Hh // 2
        prev = rb.TemporalHistory.empty(W, Hh)
        for frame in range(1, max_history + 3):
            out, count = demo.temporal(colour, shape, normal, point, prev.colour, prev.shape_index, prev.normal, prev.point, prev.count, camera, W, Hh,
                                       max_history=max_history)
            assert out.tobytes() == colour.tobytes() and np.array_equal(count, np.where(shape >= 0, min(frame, max_history), 0)), (kind, frame)
            prev = rb.TemporalHistory(out, shape, normal, point, count)
    camera = cameras(aspect=W / Hh)["perspective"]
    first = wall_frame(camera, W, Hh, split=-1.4)
    colour, shape, normal, point = wall_frame(scenes.turned_camera(camera, 2.0), W, Hh, split=-1.4)
    ones = np.ones((Hh, W), np.int32)
    out, count = demo.temporal(colour, shape, normal, point, *first, ones, camera, W, Hh)
    assert out.tobytes() == colour.tobytes() and (count == 2).sum() > W * Hh // 2
    bled, _ = demo.temporal(colour, shape, normal, point, *first, ones, camera, W, Hh, same_shape=False)
    assert bled.tobytes() != colour.tobytes()


# ---- 4. what it is for --------------------------------------------------------------------------------------------------------------
def test_five_updates_in_hbm_equal_the_mirror_chained_on_the_host(dev):
    """``TemporalAccumulator(device=True)``: the camera turns by a degree per frame; hit frames alternate between two device buffers,
    each frame's gather stays in HBM, the history ping-pongs between the accumulator's buffers.  After every ``update`` the
    downloaded frame and lengths are what five calls of the mirror, each fed the one before, give."""
    from pytracer_amd import flatten
    from pytracer_amd.devmem import DeviceBuffer, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh, K = 37, 23, 2
    m = W * Hh
    world, camera = scenes.demo_world()
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    params = dict(max_history=3)
    st = Stream()
    try:
        with dev.DeviceScene(S.world("demo")[0]) as ds:
            acc = rb.TemporalAccumulator(rb.WorldQueries(ds), device=True, stream=st, **params)
            buffers = [DeviceBuffer((abi.hits_bytes(par_f, abi.HIT_ALL),), np.uint8) for _ in range(2)]
            prev, prev_camera = rb.TemporalHistory.empty(W, Hh), camera
            outs = []
            for f in range(5):
                now = scenes.turned_camera(camera, 1.0 * f)
                hits = buffers[f & 1]
                ds.render_hits_into(flatten.flatten_camera(now), par_f, abi.HIT_ALL, hits, stream=st)
                g = rb.DeviceGuides.of_hit_buffer(hits, par_f, abi.HIT_ALL)
                gathered = ds.gather(g.point, g.normal, K, 42, None, g.shape_index, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", init_seq=54 + f * m * K,
                                     device=True, stream=st, n=m)
                out = acc.update(gathered, g, now, width=W, height=Hh)
                outs.append(out)
                assert acc.frames == f + 1 and (f < 2 or out is outs[f - 2]) and (f < 1 or out is not outs[f - 1])  # (two buffers, ping-ponged)
                colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(Hh, W, 3)
                shape, normal, point = guides(HitFrame(hits.numpy(), par_f, abi.HIT_ALL))
                want = rb.temporal_host(colour, shape, normal, point, prev.colour, prev.shape_index, prev.normal, prev.point, prev.count, prev_camera,
                                        W, Hh, **params)
                got = np.ascontiguousarray(out.numpy()[:, :m].T).reshape(Hh, W, 3), acc.count.numpy().reshape(Hh, W)
                _check(got, want, f"update {f}")
                assert want[1].max() == min(f + 1, 3) and (f == 0 or (want[0] != colour).any())
                prev, prev_camera = rb.TemporalHistory(want[0], shape.copy(), normal.copy(), point.copy(), want[1]), now
            with pytest.raises(ValueError, match="alternate two hit buffers"):
                acc.update(gathered, g, now, width=W, height=Hh)
            acc.reset()
            assert acc.count is None and acc.frames == 0
            st.synchronize()
    finally:
        st.close()


def test_eight_accumulated_frames_are_closer_to_the_converged_frame_than_one(demo_tracers):
    """48 x 36, a static camera, eight frames of K = 4, accumulated and unfiltered, against K = 1024.  Asserted: the accumulated
    frame's RMS error over the hit pixels is below the single K = 4 frame's -- the bound is the ratio 1.0, because the claim is "it
    accumulates" (eight independent frames would give 1 / sqrt(8) = 0.35).  Printed and recorded in profiles/temporal_kernel.txt, not
    asserted: the ratio itself, the ratio under a step of one degree per frame, and the ratio with the filter on."""
    from pytracer_amd.shaders import DenoisedGatherShader, TemporalGatherShader

    W, Hh, K, N = 48, 36, 4, 8
    tracer, world, wq, camera = demo_tracers(W, Hh)

    def sequence(step, filtered):
        shader = TemporalGatherShader(world, tracer, samples=K, filtered=filtered)
        for f in range(N):
            frame = frame_of(tracer, world, scenes.turned_camera(camera, step * f))
            out = shader.shade_hits(frame)[0]
        return out, frame, shader

    def single(k, frame, **kw):
        return DenoisedGatherShader(world, tracer, samples=k, init_seq=54 + (N - 1) * W * Hh * K, **kw).shade_hits(frame)[0]

    report = []
    for step in (0.0, 1.0):
        out, frame, shader = sequence(step, False)
        hit = np.asarray(frame.shape_index)[0] >= 0
        assert hit.sum() > W * Hh // 2
        reference, noisy = single(1024, frame, filtered=False), single(K, frame, filtered=False)
        rms = lambda a: float(np.sqrt(np.mean((a[hit] - reference[hit]) ** 2)))  # noqa: E731
        count = shader.accumulator.count
        assert shader.frame_no == N and count.max() == N and (count[hit] >= 1).all() and not count[~hit].any()
        both, filtered_one = sequence(step, True)[0], single(K, frame, filtered=True)
        report.append((step, rms(out), rms(noisy), rms(both), rms(filtered_one), float(count[hit].mean())))
        print(f"demo world {W}x{Hh}, {int(hit.sum())} hit pixels, {N} frames of K = {K}, {step:g} degree(s) per frame, RMS error against K = 1024 "
              f"unfiltered: accumulated {rms(out):.5f}, one frame {rms(noisy):.5f} (ratio {rms(out) / rms(noisy):.3f}); accumulated and filtered "
              f"{rms(both):.5f} (ratio {rms(both) / rms(noisy):.3f}), one frame filtered {rms(filtered_one):.5f}; mean history {count[hit].mean():.2f}")
        if step == 0.0:  # the last frame's single-frame partner draws the generators the sequence's last frame drew
            last = TemporalGatherShader(world, tracer, samples=K, filtered=False, max_history=1)
            last.frame_no = N - 1
            assert np.abs(last.shade_hits(frame)[0] - noisy).max() <= 1e-15
    _, err, err_one, _, _, _ = report[0]
    assert err_one > 0.0 and err / err_one < 1.0


def test_a_camera_step_keeps_what_was_seen_and_starts_what_comes_into_view(demo_tracers):
    """The demo camera turned by 10 degrees (its screen spans 90): most hit pixels find their history -- a length of 2 -- and the hit
    pixels whose points lay off the previous screen start one: a length of 1, the frame's own colour.  The step was chosen with the
    mirror so that both kinds exist at 48 x 36."""
    W, Hh = 48, 36
    tracer, world, wq, camera = demo_tracers(W, Hh)
    now = scenes.turned_camera(camera, 10.0)
    rng = np.random.default_rng(11)
    acc = rb.TemporalAccumulator(wq)
    first = frame_of(tracer, world, camera)
    acc.update(rng.uniform(0.5, 1.5, (Hh, W, 3)), first, camera)
    assert np.array_equal(acc.count, (np.asarray(first.shape_index)[0] >= 0).astype(np.int32))
    second = frame_of(tracer, world, now)
    colour = rng.uniform(0.5, 1.5, (Hh, W, 3))
    out = acc.update(colour, second, now)
    shape, _, point = guides(second)
    hit = shape >= 0
    _, _, seen = rb.temporal_project_host(camera, point, W, Hh)
    new = hit & ~seen
    print(f"{int(hit.sum())} hit pixels: {int((acc.count >= 2).sum())} with history, {int(new.sum())} newly in view, "
          f"{int((hit & seen & (acc.count == 1)).sum())} seen before but rejected by the guides")
    assert (acc.count[hit & seen] >= 2).sum() > hit.sum() // 2 and new.sum() >= W // 4
    assert (acc.count[new] == 1).all() and out[new].tobytes() == colour[new].tobytes()
    assert (acc.count[~hit] == 0).all() and acc.count.max() == 2
