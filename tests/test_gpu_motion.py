"""Motion accumulate queries on the device (include/ptrace_motion.h, libptrace_motion.so): the kernel against its numpy mirror
(``rays.motion_host``), against the weighted accumulate query it extends (contracts C and D), against itself across entry points,
streams and launch shapes, and in what it is for -- a sequence in which a sphere moves and keeps its history
(``rays.MotionAccumulator``, ``shaders.MovingWorldGatherShader``).

Expected agreement: bit for bit wherever the expected value is finite; where it is not, NaN where NaN is expected and infinities of
the same sign (``hostile_records.differing``); the history lengths exactly."""
import copy
import os

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb
from pytracer_amd import scenes

from . import hostile_records as H
from . import moving_frames as M
from . import surface_batches as S
from .test_gpu_temporal import guides
from .test_gpu_weighted import CASES, FRAMES, PARAMETERS, _check, _to_dev

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


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


# ---- 1. the device against the mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_hostile_records_and_every_table_equal_the_mirror_bit_for_bit(demo, W, Hh):
    reused = blended = carried = followed = outside = 0
    n = 0
    for i, (kind, how) in enumerate(CASES):
        before, args = M.inputs(W, Hh, kind, how, 2000 * W + 10 * i)
        cur, samples, shape = args[0], args[1], args[2]
        for name in M.TABLES:
            par = PARAMETERS[n % len(PARAMETERS)]
            n += 1
            mv, mo = M.table(name)
            want = rb.motion_host(*args, before, mv, mo, W, Hh, **par)
            got = demo.motion(*args, before, mv, mo, W, Hh, **par)
            assert got[0].shape == (Hh, W, 3) and got[1].shape == (Hh, W, 3) and got[2].shape == (Hh, W)
            label = f"{W}x{Hh} {kind} {how} table {name} {par}"
            _check(got, want, label)
            miss = shape < 0
            if miss.any():  # a miss is copied, whatever it holds, and has neither history nor moments
                nothing = np.zeros((int(miss.sum()), 3)), np.zeros(int(miss.sum()), np.int32)
                _check((got[0][miss], got[1][miss], got[2][miss]), (cur[miss], nothing[0], nothing[1]), label + ": the misses")
            assert (got[2] <= par["max_history"]).all() and (got[2][~miss & (samples > 0)] >= 1).all()
            reused += int((got[2] >= 2).sum())
            blended += int(((got[0] != cur).any(axis=-1) & ~miss & (samples > 0)).sum())
            carried += int(((got[0] != cur).any(axis=-1) & ~miss & (samples <= 0)).sum())
            outside += int((shape >= len(mv)).sum())
            if name != "static":  # the table reached the bits: the query on the unmoved records says something else
                plain = rb.weighted_host(*args, before, W, Hh, **par)
                followed += int((H.differing(want[0].reshape(-1, 3), plain[0].reshape(-1, 3)).size > 0) or not np.array_equal(want[2], plain[2]))
    assert W * Hh < 10 or (reused and blended and followed)  # (the history was used, and the tables moved records)
    assert W * Hh < 100 or (carried and outside)  # (and carried where nothing was sampled; indices beyond the table were met)


# ---- 2. and 3. the contracts on the device ----------------------------------------------------------------------------------------------
def test_contract_c_nothing_moved_nothing_changes(demo):
    W, Hh = 70, 33
    reused = 0
    for i, (kind, how) in enumerate((("perspective", "turned1"), ("orthogonal", "translated"))):
        before, args = M.inputs(W, Hh, kind, how, 91 + i)
        for par in (PARAMETERS[i], PARAMETERS[7 + i]):
            plain = demo.weighted(*args, before, W, Hh, **par)
            _check(demo.motion(*args, before, *M.table("static"), W, Hh, **par), plain, f"contract C, a table that is 0 everywhere, {kind} {par}")
            _check(demo.motion(*args, before, None, None, W, Hh, **par), plain, f"contract C, n_shapes = 0 and NULL tables, {kind} {par}")
            reused += int((plain[2] >= 2).sum())
    assert reused  # (there was history to leave alone)


@pytest.mark.parametrize("name", ["translation", "sheared"])
def test_contract_d_it_is_the_weighted_query_on_moved_records(demo, name):
    W, Hh = 70, 33
    changed = 0
    for i, (kind, how) in enumerate((("perspective", "turned1"), ("orthogonal", "same"))):
        before, args = M.inputs(W, Hh, kind, how, 131 + i)
        mv, mo = M.table(name)
        nm, pm = rb.move_records_host(args[2], args[3], args[4], mv, mo)
        for par in (PARAMETERS[2 + i], PARAMETERS[11 + i]):
            on_moved = demo.weighted(*args[:3], nm, pm, *args[5:], before, W, Hh, **par)
            got = demo.motion(*args, before, mv, mo, W, Hh, **par)
            _check(got, on_moved, f"contract D {name} {kind} {par}")
            unmoved = demo.weighted(*args, before, W, Hh, **par)
            changed += int(H.differing(got[0].reshape(-1, 3), unmoved[0].reshape(-1, 3)).size > 0 or not np.array_equal(got[2], unmoved[2]))
    assert changed  # (the motion changed who found a history)


# ---- 4. entry points, buffers, streams, launch shapes -------------------------------------------------------------------------------
def test_host_form_device_form_out_and_a_stream(dev, demo):
    import torch

    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    W, Hh = 70, 33
    m = W * Hh
    before, args = M.inputs(W, Hh, "perspective", "turned1", 31)
    mv, mo = M.table("sheared")
    planar = lambda a: rb.planar(a, 3) if a.ndim == 3 else np.ascontiguousarray(a.reshape(-1))  # noqa: E731
    host_planes = [planar(a) for a in args]
    on_dev = [_to_dev(a) for a in host_planes]
    tables = demo.motion_table(mv, mo)
    torch.cuda.synchronize()
    assert tables[0].dtype == torch.int32 and tables[1].dtype == torch.float64 and tuple(tables[1].shape) == (2, 24)
    assert demo.motion_table(None, None) == (None, None) and demo.motion_table(np.zeros(0, np.int32), np.zeros((0, 24))) == (None, None)
    planes = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
    st = Stream()
    try:
        for par in (dict(), dict(max_history=1, max_weight=0.0), dict(same_shape=False, blend_weight=True, normal_min=-1.0, point_tolerance=INF,
                                                                      max_weight=INF)):
            want = demo.motion(*args, before, mv, mo, W, Hh, **par)
            _check(want, rb.motion_host(*args, before, mv, mo, W, Hh, **par), f"host form {par}")
            fresh = demo.motion(*on_dev, before, *tables, W, Hh, device=True, **par)  # the default stream, buffers of its own
            _check((planes(fresh[0]), planes(fresh[1]), fresh[2].numpy().reshape(Hh, W)), want, f"device form {par}")
            mine = DeviceBuffer((3, m), np.float64), DeviceBuffer((3, m), np.float64), DeviceBuffer((m,), np.int32)
            for turn in range(2):  # a non-default stream, the caller's buffers, twice
                out = demo.motion(*on_dev, before, *tables, W, Hh, device=True, stream=st, out=mine[0], out_moments=mine[1], out_count=mine[2], **par)
                assert all(a is b for a, b in zip(out, mine))
                _check((planes(mine[0]), planes(mine[1]), mine[2].numpy().reshape(Hh, W)), want, f"out= on a stream, turn {turn}, {par}")
            raw = demo.motion(*on_dev, before, int(tables[0].data_ptr()), int(tables[1].data_ptr()), W, Hh, device=True, stream=st, n_shapes=2, **par)
            _check((planes(raw[0]), planes(raw[1]), raw[2].numpy().reshape(Hh, W)), want, f"tables by address {par}")
            none = demo.motion(*on_dev, before, None, None, W, Hh, device=True, stream=st, **par)  # (NULL tables: the weighted query)
            _check((planes(none[0]), planes(none[1]), none[2].numpy().reshape(Hh, W)), rb.weighted_host(*args, before, W, Hh, **par),
                   f"device form without tables {par}")
            st.synchronize()
            for t, a in zip(on_dev, host_planes):  # (the inputs and the tables are left alone)
                assert t.cpu().numpy().tobytes() == a.tobytes()
            assert tables[0].cpu().numpy().tobytes() == mv.tobytes() and tables[1].cpu().numpy().tobytes() == mo.tobytes()
        if (want[2] >= 2).sum() == 0:
            pytest.fail("a 1 degree step left no history: the test does not test")
        dev_args = lambda **kw: demo.motion(*on_dev, before, *tables, W, Hh, device=True, stream=st, **kw)  # noqa: E731
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*colour output too small"):
            dev_args(out=DeviceBuffer((3 * m - 1,), np.float64))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*moments output too small"):
            dev_args(out_moments=DeviceBuffer((3 * m - 1,), np.float64))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*count output too small"):
            dev_args(out_count=DeviceBuffer((m - 1,), np.int32))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the previous colour"):
            dev_args(out=on_dev[5])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*count output overlaps the sample counts"):
            dev_args(out_count=on_dev[1])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the moments output"):
            dev_args(out=mine[0], out_moments=mine[0])
        wide = demo.motion_table(np.ones(m, np.int32), np.zeros((m, 24)))  # (tables as large as the outputs)
        torch.cuda.synchronize()
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the motion table"):
            demo.motion(*on_dev, before, *wide, W, Hh, device=True, stream=st, out=wide[1])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*count output overlaps the moved table"):
            demo.motion(*on_dev, before, *wide, W, Hh, device=True, stream=st, out_count=wide[0])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*n_shapes"):
            dev_args(n_shapes=2 ** 20 + 1)
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*null moved or motion table"):
            demo.motion(*on_dev, before, None, None, W, Hh, device=True, stream=st, n_shapes=2)
        with pytest.raises(ValueError, match="come together"):
            demo.motion(*on_dev, before, tables[0], None, W, Hh, device=True, stream=st)
        with pytest.raises(ValueError, match="device=True"):
            demo.motion(*args, before, mv, mo, W, Hh, stream=st)
        with pytest.raises(ValueError, match="records"):
            demo.motion(*args, before, mv, mo, W, Hh + 1)
        none3, none1 = np.zeros((0, 3)), np.zeros(0, np.int32)
        out, moments, count = demo.motion(none3, none1, none1, none3, none3, none3, none3, none1, none3, none3, none1, before, mv, mo, 0, 9)  # m = 0
        assert out.shape == (9, 0, 3) and moments.shape == (9, 0, 3) and count.shape == (9, 0)
        # an empty history
        filled = _to_dev(np.full(m, 7, np.int32))
        torch.cuda.synchronize()
        assert demo.motion_clear(filled, m, stream=st) is filled
        st.synchronize()
        assert not filled.cpu().numpy().any()
        zero = demo.motion_clear(DeviceBuffer((m,), np.int32), stream=st)
        first = demo.motion(*on_dev[:10], zero, before, *tables, W, Hh, device=True, stream=st)
        empty = rb.WeightedHistory.empty(W, Hh)
        _check((planes(first[0]), planes(first[1]), first[2].numpy().reshape(Hh, W)),
               rb.motion_host(*args[:5], empty.colour, empty.moments, empty.shape_index, empty.normal, empty.point, empty.count, before, mv, mo, W, Hh),
               "the first frame, from lengths the library cleared")
        st.synchronize()
    finally:
        st.close()


@pytest.mark.parametrize("blocks", ["1", "2", "7"])
def test_no_bit_depends_on_the_launch(demo, blocks):
    W, Hh = 70, 33
    before, args = M.inputs(W, Hh, "perspective", "turned1", 61)
    assert "PTRACE_MA_BLOCKS" not in os.environ
    cases = ((dict(), "sheared"), (dict(max_history=2, same_shape=False, blend_weight=True, point_tolerance=INF, max_weight=3.5), "short"))
    want = [demo.motion(*args, before, *M.table(name), W, Hh, **par) for par, name in cases]
    _check(want[0], rb.motion_host(*args, before, *M.table("sheared"), W, Hh), "default launch")
    os.environ["PTRACE_MA_BLOCKS"] = blocks
    try:
        got = [demo.motion(*args, before, *M.table(name), W, Hh, **par) for par, name in cases]
    finally:
        del os.environ["PTRACE_MA_BLOCKS"]
    for g, w, (par, name) in zip(got, want, cases):
        _check(g, w, f"{blocks} workgroups {name} {par}")


# ---- 5. what it is for --------------------------------------------------------------------------------------------------------------
def _moved_demo(f, dy=0.4):
    world, camera = scenes.demo_world()
    sphere = copy.copy(world.shapes[2])
    sphere.transformation = hm.translation(hm.Vec(0.0, dy * f, 0.0)) * sphere.transformation
    world.shapes[2] = sphere
    return world, camera


def test_three_updates_in_hbm_follow_the_sphere_and_equal_the_mirror_chained_on_the_host(dev):
    """``MotionAccumulator(device=True)``: the sphere of the demo world is translated by 0.4 along y per frame and the camera turns by a
    degree; every frame has a fresh ``DeviceScene``, hit frames alternate between two device buffers, the 2-sample gather stays in
    HBM.  After every ``update`` the downloaded colour, moments, lengths and variance are what the mirrors, chained on the host, give;
    after the third, more sphere pixels carry a history than the same sequence on ``WeightedAccumulator`` leaves."""
    import torch

    from pytracer_amd import flatten
    from pytracer_amd.devmem import DeviceBuffer, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh, K = 48, 36, 2
    m = W * Hh
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    params = dict(max_history=8, max_weight=12.0, min_history=2)
    history = {k: v for k, v in params.items() if k != "min_history"}
    st = Stream()
    scenes_open = []
    try:
        acc = plain = None
        buffers = [DeviceBuffer((abi.hits_bytes(par_f, abi.HIT_ALL),), np.uint8) for _ in range(2)]
        prev = plain_prev = rb.WeightedHistory.empty(W, Hh)
        prev_camera = prev_world = None
        seq = 54
        for f in range(3):
            world, camera = _moved_demo(f)
            now = scenes.turned_camera(camera, 1.0 * f)
            ds = dev.DeviceScene(flatten.flatten_world(world))
            scenes_open.append(ds)
            q = rb.WorldQueries(ds)
            if acc is None:
                acc = rb.MotionAccumulator(q, device=True, stream=st, **params)
                plain = rb.WeightedAccumulator(q, device=True, stream=st, **params)
            hits = buffers[f & 1]
            ds.render_hits_into(flatten.flatten_camera(now), par_f, abi.HIT_ALL, hits, stream=st)
            g = rb.DeviceGuides.of_hit_buffer(hits, par_f, abi.HIT_ALL)
            shape, normal, point = guides(HitFrame(hits.numpy(), par_f, abi.HIT_ALL))
            gathered = ds.gather(g.point, g.normal, K, 42, None, g.shape_index, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", init_seq=seq, device=True,
                                 stream=st, n=m)
            seq += m * K
            taken = np.where(shape >= 0, K, 0).astype(np.int32)
            samples = _to_dev(taken.reshape(-1))
            torch.cuda.synchronize()
            out, variance = acc.update(gathered, g, now, samples=samples, world=world, queries=q, width=W, height=Hh)
            plain.queries = q
            plain.update(gathered, g, now, samples=samples, width=W, height=Hh)
            assert acc.frames == f + 1
            colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(Hh, W, 3)
            table = (None, None) if prev_world is None else rb.shape_motion(prev_world, world)
            assert f == 0 or table[0].tolist() == [0, 0, 1]
            want = rb.motion_host(colour, taken, shape, normal, point, prev.colour, prev.moments, prev.shape_index, prev.normal, prev.point,
                                  prev.count, prev_camera if prev_camera is not None else now, *table, W, Hh, **history)
            plane = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
            _check((plane(out), plane(acc.moments), acc.count.numpy().reshape(Hh, W)), want, f"update {f}")
            want_variance = rb.variance_estimate_host(want[1], want[2], shape, normal, point, W, Hh, min_history=2)
            bad = H.differing(variance.numpy()[:m].reshape(-1, 1), want_variance.reshape(-1, 1))
            assert bad.size == 0, f"update {f}: {bad.size} variances differ"
            unfollowed = rb.weighted_host(colour, taken, shape, normal, point, plain_prev.colour, plain_prev.moments, plain_prev.shape_index,
                                          plain_prev.normal, plain_prev.point, plain_prev.count, prev_camera if prev_camera is not None else now, W,
                                          Hh, **history)
            assert np.array_equal(plain.count.numpy().reshape(Hh, W), unfollowed[2])
            prev = rb.WeightedHistory(want[0], shape.copy(), normal.copy(), point.copy(), want[2], want[1])
            plain_prev = rb.WeightedHistory(unfollowed[0], shape.copy(), normal.copy(), point.copy(), unfollowed[2], unfollowed[1])
            prev_camera, prev_world = now, world
        sphere = shape == 2
        with_motion, without = int((want[2][sphere] >= 2).sum()), int((unfollowed[2][sphere] >= 2).sum())
        print(f"{int(sphere.sum())} sphere pixels after frame 2: {with_motion} with a history followed, {without} through the camera only")
        assert sphere.sum() > 20 and with_motion > without
        st.synchronize()
    finally:
        st.close()
        for ds in scenes_open:
            ds.close()


# ---- 6. the shader ------------------------------------------------------------------------------------------------------------------
def test_the_shader_on_a_static_and_on_a_moving_world(dev):
    """``MovingWorldGatherShader`` for three frames at 48 x 36.  On a static world every bit is that of the same shader not following
    (a ``WeightedAccumulator``: contract C through every layer).  On a world whose sphere moves 0.4 per frame the frames are finite
    and the sphere's pixels carry histories longer than 1, which they do not when the motion is not followed."""
    from pytracer_amd.shaders import MovingWorldGatherShader
    from pytracer_amd.tracer import GpuImageTracer

    W, Hh, N = 48, 36, 3

    def run(dy, follow):
        _, camera = scenes.demo_world()
        tracer = GpuImageTracer(hm.HdrImage(W, Hh), camera, samples_per_side=0)
        try:
            shader = MovingWorldGatherShader(_moved_demo(0, dy)[0], tracer, samples=2, max_depth=2, passes=2)
            shader.follow = follow
            frames = []
            for f in range(N):
                tracer.camera = scenes.turned_camera(camera, 1.0 * f)
                shader.world = _moved_demo(f, dy)[0]
                frame = tracer.fire_all_hits(shader.world)
                frames.append(shader.shade_hits(frame))
            return frames, np.asarray(shader.accumulator.count), np.asarray(frame.shape_index)[0], type(shader.accumulator).__name__
        finally:
            tracer.close()

    still, still_count, _, kind = run(0.0, True)
    plain, plain_count, _, plain_kind = run(0.0, False)
    assert (kind, plain_kind) == ("MotionAccumulator", "WeightedAccumulator")
    for a, b in zip(still, plain):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
    assert np.array_equal(still_count, plain_count) and still_count.max() == N
    moving, count, shape, _ = run(0.4, True)
    _, lost, _, _ = run(0.4, False)
    assert all(np.isfinite(f).all() for f in moving)
    sphere = shape == 2
    print(f"{int(sphere.sum())} sphere pixels: {int((count[sphere] >= 2).sum())} with a history followed, {int((lost[sphere] >= 2).sum())} not followed")
    assert sphere.sum() > 20 and (count[sphere] >= 2).sum() > (lost[sphere] >= 2).sum()
