"""Weighted accumulate queries on the device (include/ptrace_weighted.h, libptrace_weighted.so): the kernel against its numpy mirror
(``rays.weighted_host``), against the accumulate and moments queries it replaces (contract A), against itself across entry points,
streams and launch shapes, and in what it is for -- an adaptive sequence whose frames count by the samples they took
(``rays.WeightedAccumulator``, ``shaders.WeightedAdaptiveGatherShader``).

Expected agreement: bit for bit wherever the expected value is finite; where it is not, NaN where NaN is expected and infinities of
the same sign (``hostile_records.differing``); the history lengths exactly."""
import os

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import rays as rb
from pytracer_amd import scenes

from . import hostile_records as H
from . import surface_batches as S
from .test_gpu_temporal import guides, moved
from .test_temporal_host import cameras, wall_frame
from .test_weighted_host import hostile

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
# one workgroup takes 256 pixels: 1 x 1 to 37 x 23 are one to four of them with a ragged last one, 70 x 33 is ten
FRAMES = [(1, 1), (3, 2), (17, 5), (37, 23), (70, 33)]
# both flag bits on and off x max_weight 0, 3.5, 128 and inf, with the accumulate query's parameters turning beside them
PARAMETERS = [dict(same_shape=s, blend_weight=b, max_weight=w, max_history=(1, 2, 32, 5)[i % 4], normal_min=(-1.0, 0.9)[(i // 2) % 2],
                   point_tolerance=(0.05, INF)[(i // 3) % 2])
              for i, (s, b, w) in enumerate((s, b, w) for w in (0.0, 3.5, 128.0, INF) for s in (True, False) for b in (False, True))]
MOVES = ("same", "turned1", "turned20", "translated")
CASES = [(kind, how) for kind in ("perspective", "orthogonal") for how in MOVES]  # eight x two parameter sets: all sixteen are used


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


def hostile_weights(Hh, W, seed):
    """-> (moments [Hh, W, 3] whose S plane holds weights of 0 to 60 with NaN, -1, +-inf, 1e300 and 0 among them and whose M1 and M2
    hold a NaN and an infinity; samples [Hh, W]: 1 to 40 with 0, negatives and 2^31 - 1 among them)."""
    rng = np.random.default_rng(seed)
    m = W * Hh
    moments = rng.uniform(0.0, 2.0, (m, 3)) * np.array([1.0, 1.0, 30.0])
    pick = lambda share: np.flatnonzero(rng.uniform(0, 1, m) < share)  # noqa: E731
    for rows, value in ((pick(0.04), NAN), (pick(0.04), -1.0), (pick(0.04), INF), (pick(0.02), -INF), (pick(0.04), 1e300), (pick(0.04), 0.0)):
        moments[rows, 2] = value
    moments[pick(0.02), 0], moments[pick(0.02), 1] = NAN, INF
    samples = rng.integers(1, 41, m).astype(np.int32)
    for rows, value in ((pick(0.08), 0), (pick(0.03), -1), (pick(0.02), -5), (pick(0.01), -2 ** 31), (pick(0.03), 2 ** 31 - 1)):
        samples[rows] = value
    return moments.reshape(Hh, W, 3), samples.reshape(Hh, W)


def _check(got, want, label):
    for name, g, w in (("colour", got[0], want[0]), ("moments", got[1], want[1])):
        g, w = np.ascontiguousarray(g).reshape(-1, 3), np.ascontiguousarray(w).reshape(-1, 3)
        bad = H.differing(g, w)
        assert bad.size == 0, f"{label}: {bad.size} of {len(w)} pixels differ in {name}, first {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"
    got_n, want_n = np.asarray(got[2]).reshape(-1), np.asarray(want[2]).reshape(-1)
    assert got_n.dtype == want_n.dtype == np.int32
    off = np.flatnonzero(got_n != want_n)
    assert off.size == 0, f"{label}: {off.size} history lengths differ, first {int(off[0])}: got {got_n[off[0]]}, want {want_n[off[0]]}"


def _inputs(W, Hh, kind, how, seed):
    """-> (the camera before, the arguments of ``weighted_host`` / ``DeviceScene.weighted`` up to ``prev_count``)."""
    before = cameras(aspect=W / Hh)[kind]
    rng = np.random.default_rng(seed)
    pcol, pshape, pnormal, ppoint, pcount = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *wall_frame(before, W, Hh, split=-1.4)[1:], seed=seed + 1,
                                                    counts=True)
    col, shape, normal, point = hostile(rng.uniform(0.0, 2.0, (Hh, W, 3)), *wall_frame(moved(before, how), W, Hh, split=-1.4)[1:], seed=seed + 2)
    pmoments, samples = hostile_weights(Hh, W, seed + 3)
    return before, (col, samples, shape, normal, point, pcol, pmoments, pshape, pnormal, ppoint, pcount)


# ---- 1. the device against the mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_hostile_guides_counts_weights_and_samples_equal_the_mirror_bit_for_bit(demo, W, Hh):
    reused = blended = carried = 0
    for i, (kind, how) in enumerate(CASES):
        before, args = _inputs(W, Hh, kind, how, 1000 * W + 10 * i)
        cur, samples, shape = args[0], args[1], args[2]
        for j in range(2):
            par = PARAMETERS[(2 * i + j) % len(PARAMETERS)]
            want = rb.weighted_host(*args, before, W, Hh, **par)
            got = demo.weighted(*args, before, W, Hh, **par)
            assert got[0].shape == (Hh, W, 3) and got[1].shape == (Hh, W, 3) and got[2].shape == (Hh, W)
            _check(got, want, f"{W}x{Hh} {kind} {how} {par}")
            miss = shape < 0
            if miss.any():  # a miss is copied, whatever it holds, and has neither history nor moments
                nothing = np.zeros((int(miss.sum()), 3)), np.zeros(int(miss.sum()), np.int32)
                _check((got[0][miss], got[1][miss], got[2][miss]), (cur[miss], nothing[0], nothing[1]), f"{W}x{Hh} {kind} {how} {par}: the misses")
            assert (got[2] <= par["max_history"]).all() and (got[2][~miss & (samples > 0)] >= 1).all()
            reused += int((got[2] >= 2).sum())
            blended += int(((got[0] != cur).any(axis=-1) & ~miss & (samples > 0)).sum())
            carried += int(((got[0] != cur).any(axis=-1) & ~miss & (samples <= 0)).sum())
        if i == 0:  # samples = None: one sample everywhere
            want = rb.weighted_host(args[0], None, *args[2:], before, W, Hh)
            _check(demo.weighted(args[0], None, *args[2:], before, W, Hh), want, f"{W}x{Hh} {kind} {how}: no samples plane")
    assert W * Hh < 10 or (reused and blended)  # (the history was used)
    assert W * Hh < 100 or carried  # (and carried where nothing was sampled)


# ---- 2. contract A on the device --------------------------------------------------------------------------------------------------------
def test_contract_a_unweighted_it_is_the_accumulate_and_the_moments_query_in_one_launch(demo):
    W, Hh = 70, 33
    for i, (kind, how, max_history) in enumerate((("perspective", "turned1", 32), ("orthogonal", "translated", 2), ("perspective", "same", 1))):
        before, (col, _, shape, normal, point, pcol, pmoments, pshape, pnormal, ppoint, pcount) = _inputs(W, Hh, kind, how, 77 + i)
        pmoments = pmoments.copy()
        pmoments[..., 2] = pcount.astype(np.float64)  # (the premise: the third plane is the history length)
        old = demo.temporal(col, shape, normal, point, pcol, pshape, pnormal, ppoint, pcount, before, W, Hh, max_history=max_history)
        frame = demo.variance_moments(col, shape, W, Hh)
        old_m = demo.temporal(frame, shape, normal, point, pmoments, pshape, pnormal, ppoint, pcount, before, W, Hh, max_history=max_history)
        got = demo.weighted(col, None, shape, normal, point, pcol, pmoments, pshape, pnormal, ppoint, pcount, before, W, Hh, max_history=max_history,
                            max_weight=float(max_history - 1))
        label = f"contract A {kind} {how} max_history {max_history}"
        _check((got[0], np.concatenate([got[1][..., :2], old_m[0][..., 2:]], axis=-1), got[2]), (old[0], old_m[0], old[1]), label)
        assert np.array_equal(old_m[1], old[1]) and np.array_equal(got[1][..., 2], got[2].astype(np.float64)), label  # S == count
        assert max_history == 1 or (got[2] >= 2).sum() > W * Hh // 4


# ---- 3. entry points, buffers, streams, launch shapes -------------------------------------------------------------------------------
def _to_dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()


def test_host_form_device_form_out_and_a_stream(dev, demo):
    """The planes uploaded once, the accumulation reading all eleven inputs where they are -- on the default stream into buffers of its
    own, and on a non-default stream into the caller's, twice: the host form's bits, and the inputs untouched."""
    import torch

    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    W, Hh = 70, 33
    m = W * Hh
    before, args = _inputs(W, Hh, "perspective", "turned1", 31)
    planar = lambda a: rb.planar(a, 3) if a.ndim == 3 else np.ascontiguousarray(a.reshape(-1))  # noqa: E731
    host_planes = [planar(a) for a in args]
    on_dev = [_to_dev(a) for a in host_planes]
    torch.cuda.synchronize()
    planes = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
    st = Stream()
    try:
        for par in (dict(), dict(max_history=1, max_weight=0.0), dict(same_shape=False, blend_weight=True, normal_min=-1.0, point_tolerance=INF,
                                                                      max_weight=INF)):
            want = demo.weighted(*args, before, W, Hh, **par)
            _check(want, rb.weighted_host(*args, before, W, Hh, **par), f"host form {par}")
            fresh = demo.weighted(*on_dev, before, W, Hh, device=True, **par)  # the default stream, buffers of its own
            _check((planes(fresh[0]), planes(fresh[1]), fresh[2].numpy().reshape(Hh, W)), want, f"device form {par}")
            mine = DeviceBuffer((3, m), np.float64), DeviceBuffer((3, m), np.float64), DeviceBuffer((m,), np.int32)
            for turn in range(2):  # a non-default stream, the caller's buffers, twice
                out = demo.weighted(*on_dev, before, W, Hh, device=True, stream=st, out=mine[0], out_moments=mine[1], out_count=mine[2], **par)
                assert all(a is b for a, b in zip(out, mine))
                _check((planes(mine[0]), planes(mine[1]), mine[2].numpy().reshape(Hh, W)), want, f"out= on a stream, turn {turn}, {par}")
            none = demo.weighted(on_dev[0], None, *on_dev[2:], before, W, Hh, device=True, stream=st, **par)  # (a NULL samples plane)
            _check((planes(none[0]), planes(none[1]), none[2].numpy().reshape(Hh, W)), rb.weighted_host(args[0], None, *args[2:], before, W, Hh, **par),
                   f"device form without samples {par}")
            st.synchronize()
            for t, a in zip(on_dev, host_planes):  # (the inputs are left alone)
                assert t.cpu().numpy().tobytes() == a.tobytes()
        if (want[2] >= 2).sum() == 0:
            pytest.fail("a 1 degree step left no history: the test does not test")
        dev_args = lambda **kw: demo.weighted(*on_dev, before, W, Hh, device=True, stream=st, **kw)  # noqa: E731
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*colour output too small"):
            dev_args(out=DeviceBuffer((3 * m - 1,), np.float64))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*moments output too small"):
            dev_args(out_moments=DeviceBuffer((3 * m - 1,), np.float64))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*count output too small"):
            dev_args(out_count=DeviceBuffer((m - 1,), np.int32))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the previous colour"):
            dev_args(out=on_dev[5])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*moments output overlaps the previous moments"):
            dev_args(out_moments=on_dev[6])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*count output overlaps the sample counts"):
            dev_args(out_count=on_dev[1])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the moments output"):
            dev_args(out=mine[0], out_moments=mine[0])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*max_weight"):
            dev_args(max_weight=NAN)
        with pytest.raises(ValueError, match="device=True"):
            demo.weighted(*args, before, W, Hh, stream=st)
        with pytest.raises(ValueError, match="records"):
            demo.weighted(*args, before, W, Hh + 1)
        none3, none1 = np.zeros((0, 3)), np.zeros(0, np.int32)
        out, moments, count = demo.weighted(none3, none1, none1, none3, none3, none3, none3, none1, none3, none3, none1, before, 0, 9)  # m = 0
        assert out.shape == (9, 0, 3) and moments.shape == (9, 0, 3) and count.shape == (9, 0)
        # an empty history
        filled = _to_dev(np.full(m, 7, np.int32))
        torch.cuda.synchronize()
        assert demo.weighted_clear(filled, m, stream=st) is filled
        st.synchronize()
        assert not filled.cpu().numpy().any()
        zero = demo.weighted_clear(DeviceBuffer((m,), np.int32), stream=st)
        first = demo.weighted(*on_dev[:10], zero, before, W, Hh, device=True, stream=st)
        empty = rb.WeightedHistory.empty(W, Hh)
        _check((planes(first[0]), planes(first[1]), first[2].numpy().reshape(Hh, W)),
               rb.weighted_host(*args[:5], empty.colour, empty.moments, empty.shape_index, empty.normal, empty.point, empty.count, before, W, Hh),
               "the first frame, from lengths the library cleared")
        st.synchronize()
    finally:
        st.close()


@pytest.mark.parametrize("blocks", ["1", "2", "7"])
def test_no_bit_depends_on_the_launch(demo, blocks):
    """Grids far smaller than the work (the grid-stride loop; ten workgroups by default): the frame of the default launch -- which the
    tests above hold against the mirror -- in every bit."""
    W, Hh = 70, 33
    before, args = _inputs(W, Hh, "perspective", "turned1", 61)
    assert "PTRACE_WA_BLOCKS" not in os.environ
    cases = (dict(), dict(max_history=2, same_shape=False, blend_weight=True, point_tolerance=INF, max_weight=3.5))
    want = [demo.weighted(*args, before, W, Hh, **par) for par in cases]
    _check(want[0], rb.weighted_host(*args, before, W, Hh, **cases[0]), "default launch")
    os.environ["PTRACE_WA_BLOCKS"] = blocks
    try:
        got = [demo.weighted(*args, before, W, Hh, **par) for par in cases]
    finally:
        del os.environ["PTRACE_WA_BLOCKS"]
    for g, w, par in zip(got, want, cases):
        _check(g, w, f"{blocks} workgroups {par}")


# ---- 4. what it is for --------------------------------------------------------------------------------------------------------------
def test_five_adaptive_updates_in_hbm_equal_the_mirror_chained_on_the_host(dev):
    """``WeightedAccumulator(device=True)``: the camera turns by a degree per frame; hit frames alternate between two device buffers;
    frame 0 is a uniform gather of 2, every later frame a ragged gather with counts from ``sample_counts`` -- all left in HBM, its
    TAKEN plane handed over as ``samples`` by address, under a capacity below the total so that some records take nothing.  After
    every ``update`` the downloaded colour, moments, lengths and variance are what the mirrors, chained on the host, give."""
    import torch

    from pytracer_amd import flatten
    from pytracer_amd.devmem import DeviceBuffer, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh, K = 37, 23, 2
    m = W * Hh
    world, camera = scenes.demo_world()
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    params = dict(max_history=3, max_weight=12.0, min_history=2)
    history = {k: v for k, v in params.items() if k != "min_history"}
    counts_par = dict(min_samples=1, max_samples=8, tolerance=0.05, luminance_floor=0.1)
    bits = rb.adaptive_channels("taken")
    st = Stream()
    try:
        with dev.DeviceScene(S.world("demo")[0]) as ds:
            acc = rb.WeightedAccumulator(rb.WorldQueries(ds), device=True, stream=st, **params)
            buffers = [DeviceBuffer((abi.hits_bytes(par_f, abi.HIT_ALL),), np.uint8) for _ in range(2)]
            prev, prev_camera = rb.WeightedHistory.empty(W, Hh), camera
            outs, variance, seq, starved = [], None, 54, 0
            for f in range(5):
                now = scenes.turned_camera(camera, 1.0 * f)
                hits = buffers[f & 1]
                ds.render_hits_into(flatten.flatten_camera(now), par_f, abi.HIT_ALL, hits, stream=st)
                g = rb.DeviceGuides.of_hit_buffer(hits, par_f, abi.HIT_ALL)
                shape, normal, point = guides(HitFrame(hits.numpy(), par_f, abi.HIT_ALL))
                if f == 0:
                    gathered = ds.gather(g.point, g.normal, K, 42, None, g.shape_index, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", init_seq=seq, device=True,
                                         stream=st, n=m)
                    taken = np.where(shape >= 0, K, 0).astype(np.int32)
                    samples = _to_dev(taken.reshape(-1))
                    torch.cuda.synchronize()
                    seq += m * K
                else:
                    counts = ds.sample_counts(variance, outs[-1], g.shape_index, device=True, stream=st, m=m, **counts_par)
                    offsets = ds.sample_offsets(counts, device=True, stream=st)
                    total = int(offsets.numpy()[-1])
                    capacity = total if f == 1 else (2 * total) // 3  # (the budget runs out on three of the four frames)
                    gathered = ds.gather_ragged(g.point, g.normal, counts, offsets, capacity, 42, None, g.shape_index, 1, 2, 3, (0.0, 0.0, 0.0), 1, bits,
                                                init_seq=seq, device=True, stream=st, n=m)
                    samples = int(gathered.data_ptr()) + rb.adaptive_plane_offset(m, bits, rb.ADAPTIVE_TAKEN)
                    taken = gathered.numpy()[24 * m: 28 * m].view(np.int32).reshape(Hh, W).copy()
                    want_counts = rb.sample_counts_host(prev_variance, prev.colour, shape, **counts_par)
                    assert np.array_equal(counts.numpy().reshape(Hh, W), want_counts)
                    assert np.array_equal(taken.reshape(-1), rb.samples_taken_host(want_counts, rb.sample_offsets_host(want_counts), capacity))
                    starved += int(((taken == 0) & (want_counts > 0)).sum())
                    seq += total
                out, variance = acc.update(gathered, g, now, samples=samples, width=W, height=Hh)
                outs.append(out)
                assert acc.frames == f + 1 and (f < 2 or out is outs[f - 2]) and (f < 1 or out is not outs[f - 1])  # (two buffers, ping-ponged)
                colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(Hh, W, 3)
                want = rb.weighted_host(colour, taken, shape, normal, point, prev.colour, prev.moments, prev.shape_index, prev.normal, prev.point,
                                        prev.count, prev_camera, W, Hh, **history)
                plane = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
                _check((plane(out), plane(acc.moments), acc.count.numpy().reshape(Hh, W)), want, f"update {f}")
                assert acc.weight == int(acc.moments.data_ptr()) + 16 * m
                prev_variance = rb.variance_estimate_host(want[1], want[2], shape, normal, point, W, Hh, min_history=2)
                bad = H.differing(variance.numpy()[:m].reshape(-1, 1), prev_variance.reshape(-1, 1))
                assert bad.size == 0, f"update {f}: {bad.size} variances differ"
                assert want[2].max() == min(f + 1, 3) and want[1][..., 2].max() <= 12.0 + 8
                prev, prev_camera = rb.WeightedHistory(want[0], shape.copy(), normal.copy(), point.copy(), want[2], want[1]), now
            assert starved > 0  # (a budget ran out: some hit records that asked for samples took none)
            with pytest.raises(ValueError, match="alternate two hit buffers"):
                acc.update(gathered, g, now, samples=samples, width=W, height=Hh)
            acc.reset()
            assert acc.count is None and acc.weight is None and acc.frames == 0
            st.synchronize()
    finally:
        st.close()


def test_the_shader_keeps_the_history_of_the_records_a_budget_cut_off(dev):
    """``WeightedAdaptiveGatherShader`` at 48 x 36 for four frames, ``min_samples = 0`` and a budget that truncates: the frame is
    finite, and where the last frame's gather took nothing the accumulated E is the reprojected history (what the mirror carries from
    the frame before), not black."""
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.shaders import WeightedAdaptiveGatherShader
    from pytracer_amd.tracer import GpuImageTracer

    W, Hh, N = 48, 36, 4
    world, camera = scenes.demo_world()
    tracer = GpuImageTracer(hm.HdrImage(W, Hh), camera, samples_per_side=0)
    try:
        shader = WeightedAdaptiveGatherShader(world, tracer, samples=4, filtered=False, min_samples=0, max_samples=16, tolerance=0.01, budget=2000, max_depth=2)
        for f in range(N):
            tracer.camera = scenes.turned_camera(camera, 1.0 * f)
            frame = tracer.fire_all_hits(world)
            if f == N - 1:
                before = shader.accumulator._prev, shader.accumulator._camera
            lit = shader.shade_hits(frame)
        assert np.isfinite(lit).all() and shader.frame_no == N
        taken = np.asarray(shader.last_gather.taken)[0]
        hit = np.asarray(frame.shape_index)[0] >= 0
        cut = hit & (taken == 0) & (np.asarray(shader.last_counts) > 0)
        assert shader.last_total <= 2000 and cut.sum() > W  # (the budget ran out: whole rows took nothing)
        e = shader.accumulator._prev.colour
        prev, prev_camera = before
        black = np.zeros((Hh, W, 3))
        want = rb.weighted_host(black, taken, *guides(frame), prev.colour, prev.moments, prev.shape_index, prev.normal, prev.point, prev.count,
                                prev_camera, W, Hh)
        assert H.differing(e[cut], want[0][cut]).size == 0  # (whatever this frame's colour: it is never read where nothing was taken)
        carried = cut & (want[2] >= 1)
        print(f"{int(cut.sum())} records cut off, {int(carried.sum())} of them with history, {int((e[carried].max(axis=-1) > 0.0).sum())} not black")
        assert carried.sum() > cut.sum() // 2 and (e[carried].max(axis=-1) > 0.0).sum() > carried.sum() // 2  # not black
        assert np.array_equal(shader.accumulator.count[cut], want[2][cut]) and shader.accumulator.count.max() == N
    finally:
        tracer.close()
