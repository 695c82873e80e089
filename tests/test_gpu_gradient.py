"""Gradient accumulate queries on the device (include/ptrace_gradient.h, libptrace_gradient.so): the three kernels against their numpy
mirrors (``rays.gradient_probes_host``, ``gradient_keep_host``, ``gradient_accumulate_host``), against the motion accumulate query
they extend (contracts E and F), through the real gather on an unchanged world (contract G), against themselves across entry points,
streams and launch shapes, and in what they are for -- a sequence in which a sphere moves and the ground under it forgets the
shadow that left (``rays.GradientAccumulator``, ``shaders.GradientGatherShader``).

Expected agreement: bit for bit wherever the expected value is finite; where it is not, NaN where NaN is expected and infinities of
the same sign (``hostile_records.differing``); indices, stream numbers and history lengths exactly."""
import copy
import os

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb
from pytracer_amd import scenes

from . import gradient_frames as G
from . import hostile_records as H
from . import moving_frames as M
from . import surface_batches as S
from .test_gpu_temporal import guides
from .test_gpu_weighted import CASES, FRAMES, PARAMETERS, _check, _to_dev

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
GAINS = (1.0, 4.0, 0.0, 32.0, INF)


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


def _check_probes(got, want, label):
    assert got[0].dtype == want[0].dtype == np.int32 and got[3].dtype == want[3].dtype == np.uint64
    assert np.array_equal(got[0], want[0]), f"{label}: probe indices differ"
    assert np.array_equal(got[3], want[3]), f"{label}: probe stream numbers differ"
    for name, g, w in (("point", got[1], want[1]), ("normal", got[2], want[2])):
        assert g.shape == w.shape, (label, name, g.shape, w.shape)
        bad = H.differing(np.ascontiguousarray(g).reshape(-1, 3), np.ascontiguousarray(w).reshape(-1, 3))
        assert bad.size == 0, f"{label}: {bad.size} probes differ in {name}, first {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"


def _check_keep(got, want, label):
    assert got.shape == want.shape and got.dtype == np.float64
    bad = H.differing(np.ascontiguousarray(got).reshape(-1, 1), np.ascontiguousarray(want).reshape(-1, 1))
    assert bad.size == 0, f"{label}: {bad.size} keep values differ, first {int(bad[0])}: got {got.reshape(-1)[bad[0]]}, want {want.reshape(-1)[bad[0]]}"


# ---- 1. the device against the mirrors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_hostile_records_every_table_stratum_and_radius_equal_the_mirrors_bit_for_bit(demo, W, Hh):
    skipped = carried_back = below = full = shortened = 0
    n = 0
    for i, (kind, how) in enumerate(CASES):
        before, args = M.inputs(W, Hh, kind, how, 3000 * W + 10 * i)
        colour, shape, normal, point = args[0], args[2], args[3], args[4]
        for name in M.TABLES:
            par = PARAMETERS[n % len(PARAMETERS)]
            s, radius, gain = G.STRATA[n % 4], G.RADII[n % 3], GAINS[n % 5]
            K, seq0, phase = 1 + n % 4, (54, 2 ** 64 - 3)[n % 2], (n, 2 ** 64 - 1 - n)[(n // 2) % 2]
            free = bool((n // 3) % 2)
            n += 1
            mv, mo = M.table(name)
            label = f"{W}x{Hh} {kind} {how} table {name} stratum {s} radius {radius} gain {gain}"
            # the probes
            want = rb.gradient_probes_host(shape, normal, point, mv, mo, W, Hh, stratum=s, phase=phase, samples=K, init_seq=seq0)
            got = demo.gradient_probes(shape, normal, point, mv, mo, W, Hh, stratum=s, phase=phase, samples=K, init_seq=seq0)
            _check_probes(got, want, label)
            skipped += int((want[0] < 0).sum())
            unmoved = rb.gradient_probes_host(shape, normal, point, None, None, W, Hh, stratum=s, phase=phase, samples=K, init_seq=seq0)
            carried_back += int(H.differing(want[1], unmoved[1]).size)
            # keep: hostile index planes over the probes' own, old colours that agree at about half of them
            index = G.hostile_index(W, Hh, s, 7 * n, want[0])
            old = G.probe_old(colour, index, 7 * n + 1)
            want_keep = rb.gradient_keep_host(colour, shape, index, old, W, Hh, stratum=s, radius=radius, gain=gain, same_shape_probes=not free)
            got_keep = demo.gradient_keep(colour, shape, index, old, W, Hh, stratum=s, radius=radius, gain=gain, same_shape_probes=not free)
            _check_keep(got_keep, want_keep, label)
            assert (want_keep[shape < 0] == 1.0).all() and (want_keep >= 0.0).all() and (want_keep <= 1.0).all()
            below += int((want_keep < 1.0).sum())
            full += int((want_keep == 1.0).sum())
            # the accumulation: a hostile keep plane, and the plane keep made
            for kp in (G.hostile_keep(W, Hh, 7 * n + 2), want_keep):
                want_acc = rb.gradient_accumulate_host(*args, before, mv, mo, kp, W, Hh, **par)
                got_acc = demo.gradient_accumulate(*args, before, mv, mo, kp, W, Hh, **par)
                assert got_acc[0].shape == (Hh, W, 3) and got_acc[1].shape == (Hh, W, 3) and got_acc[2].shape == (Hh, W)
                _check(got_acc, want_acc, label + f" {par}")
            plain = rb.motion_host(*args, before, mv, mo, W, Hh, **par)
            assert (want_acc[2] <= plain[2]).all()
            shortened += int((want_acc[2] < plain[2]).sum())
    assert W * Hh < 10 or (below and full)  # (keep < 1 and keep == 1 both occurred)
    assert W * Hh < 100 or (skipped and carried_back and shortened)  # (probes on misses were skipped, the tables moved probes, histories shrank)


# ---- 2. the contracts on the device ------------------------------------------------------------------------------------------------
def test_contracts_e_and_f_against_the_motion_query(demo):
    W, Hh = 70, 33
    reused = cut = 0
    for i, (kind, how) in enumerate((("perspective", "turned1"), ("orthogonal", "translated"))):
        before, args = M.inputs(W, Hh, kind, how, 191 + i)
        shape, samples = args[2], args[1]
        took = (shape >= 0) & (samples > 0)
        for par, name in ((PARAMETERS[i], "translation"), (PARAMETERS[5 + i], "sheared"), (PARAMETERS[2 + i], "static")):
            mv, mo = M.table(name)
            plain = demo.motion(*args, before, mv, mo, W, Hh, **par)
            # E: nothing kept back, nothing changes
            _check(demo.gradient_accumulate(*args, before, mv, mo, None, W, Hh, **par), plain, f"contract E, keep NULL, {kind} {name} {par}")
            _check(demo.gradient_accumulate(*args, before, mv, mo, np.ones((Hh, W)), W, Hh, **par), plain, f"contract E, keep 1.0, {kind} {name} {par}")
            reused += int((plain[2] >= 2).sum())
            # F: nothing kept, the history is one frame
            got = demo.gradient_accumulate(*args, before, mv, mo, np.zeros((Hh, W)), W, Hh, **par)
            carried = demo.motion(args[0], np.zeros_like(samples), *args[2:], before, mv, mo, W, Hh, **par)
            tapped, hist = carried[2] >= 1, carried[0]
            assert (got[2][took] == 1).all() and (got[2][(shape >= 0) & (samples <= 0)] == 0).all()
            if np.isfinite(par["max_weight"]):
                with np.errstate(all="ignore"):
                    one_frame = np.where(tapped[..., None], hist + (args[0] - hist) * 1.0, args[0])
                assert H.differing(got[0][took], one_frame[took]).size == 0
                assert np.array_equal(got[1][..., 2][took], samples[took].astype(np.float64))
            cut += int((got[2] < plain[2]).sum())
    assert reused and cut  # (there was history to leave alone, and to cut)


def test_contract_g_through_the_real_gather_a_static_world_keeps_everything(dev, demo):
    """The probes of a 48 x 36 hit frame of the demo world, gathered in the SAME scene with the frame's own streams: the bits of the
    frame's gather at the probes' pixels, keep 1.0 in every bit, and the accumulation is the motion query."""
    from pytracer_amd import flatten

    W, Hh, K, seq0 = 48, 36, 2, 54 + 12345
    m = W * Hh
    _, camera = scenes.demo_world()
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    shape, normal, point = guides(demo.render_hits(flatten.flatten_camera(camera), par_f, abi.HIT_ALL))
    gather = lambda p, n, seqs, active, init_seq: np.array(demo.gather(rb.planar(p, 3), rb.planar(n, 3), K, 42, seqs, active, 1, 2, 3,  # noqa: E731
                                                                       (0.0, 0.0, 0.0), 1, "none", init_seq=init_seq).radiance)
    e = gather(point.reshape(-1, 3), normal.reshape(-1, 3), None, shape.reshape(-1), seq0)
    assert (shape >= 0).sum() > m // 2 and (shape < 0).any() and len(np.unique(e, axis=0)) > 5
    before = rb.WeightedHistory.empty(W, Hh)
    first = demo.motion(e, None, shape, normal, point, before.colour, before.moments, before.shape_index, before.normal, before.point, before.count,
                        camera, None, None, W, Hh)
    for s, radius, gain in ((3, 1, 4.0), (1, 0, INF), (4, 2, 32.0), (16, 4, 1.0)):
        index, pp, nn, seqs = demo.gradient_probes(shape, normal, point, None, None, W, Hh, stratum=s, phase=9, samples=K, init_seq=seq0)
        assert (index >= 0).any() and (index < 0).any()
        old = gather(pp, nn, seqs, index, 0)
        ok = index >= 0
        assert old[ok].tobytes() == e[index[ok]].tobytes() and not old[~ok].any()  # (a gather is a function of world, point, normal, streams)
        keep = demo.gradient_keep(e, shape, index, old, W, Hh, stratum=s, radius=radius, gain=gain)
        assert keep.tobytes() == np.ones((Hh, W)).tobytes(), (s, radius, gain)
        args = (e, None, shape, normal, point, first[0], first[1], shape, normal, point, first[2], camera)
        _check(demo.gradient_accumulate(*args, None, None, keep, W, Hh), demo.motion(*args, None, None, W, Hh), f"contract G, stratum {s}")


# ---- 3. entry points, buffers, streams, launch shapes -------------------------------------------------------------------------------
def test_host_form_device_form_out_and_a_stream(dev, demo):
    import torch

    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    W, Hh, s = 70, 33, 3
    m, ns = W * Hh, 24 * 11
    before, args = M.inputs(W, Hh, "perspective", "turned1", 31)
    colour, shape, normal, point = args[0], args[2], args[3], args[4]
    mv, mo = M.table("sheared")
    planar = lambda a: rb.planar(a, 3) if a.ndim == 3 else np.ascontiguousarray(a.reshape(-1))  # noqa: E731
    host_planes = [planar(a) for a in args]
    on_dev = [_to_dev(a) for a in host_planes]
    tables = demo.motion_table(mv, mo)
    want_probes = rb.gradient_probes_host(shape, normal, point, mv, mo, W, Hh, stratum=s, phase=5, samples=2, init_seq=99)
    index = G.hostile_index(W, Hh, s, 77, want_probes[0])
    old = G.probe_old(colour, index, 78)
    want_keep = rb.gradient_keep_host(colour, shape, index, old, W, Hh, stratum=s, radius=2, gain=2.0)
    kp = G.hostile_keep(W, Hh, 79)
    extra = [_to_dev(a) for a in (index, rb.planar(old, 3), kp.reshape(-1))]
    torch.cuda.synchronize()
    planes = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
    rows = lambda b: np.ascontiguousarray(b.numpy()[:, :ns].T)  # noqa: E731
    st = Stream()
    try:
        # the probes
        _check_probes(demo.gradient_probes(shape, normal, point, mv, mo, W, Hh, stratum=s, phase=5, samples=2, init_seq=99), want_probes, "host form")
        probe_args = (on_dev[2], on_dev[3], on_dev[4], *tables, W, Hh)
        fresh = demo.gradient_probes(*probe_args, stratum=s, phase=5, samples=2, init_seq=99, device=True)
        _check_probes((fresh[0].numpy()[:ns], rows(fresh[1]), rows(fresh[2]), fresh[3].numpy()[:ns]), want_probes, "device form")
        mine = (DeviceBuffer((ns,), np.int32), DeviceBuffer((3, ns), np.float64), DeviceBuffer((3, ns), np.float64), DeviceBuffer((ns,), np.uint64))
        for turn in range(2):
            out = demo.gradient_probes(*probe_args, stratum=s, phase=5, samples=2, init_seq=99, device=True, stream=st, out=mine)
            assert all(a is b for a, b in zip(out, mine))
            _check_probes((mine[0].numpy(), rows(mine[1]), rows(mine[2]), mine[3].numpy()), want_probes, f"probes, out= on a stream, turn {turn}")
        # keep
        _check_keep(demo.gradient_keep(colour, shape, index, old, W, Hh, stratum=s, radius=2, gain=2.0), want_keep, "host form")
        keep_args = (on_dev[0], on_dev[2], extra[0], extra[1], W, Hh)
        fresh = demo.gradient_keep(*keep_args, stratum=s, radius=2, gain=2.0, device=True)
        _check_keep(fresh.numpy()[:m].reshape(Hh, W), want_keep, "device form")
        kept = DeviceBuffer((m,), np.float64)
        for turn in range(2):
            assert demo.gradient_keep(*keep_args, stratum=s, radius=2, gain=2.0, device=True, stream=st, out=kept) is kept
            _check_keep(kept.numpy().reshape(Hh, W), want_keep, f"keep, out= on a stream, turn {turn}")
        # the accumulation
        for par in (dict(), dict(max_history=1, max_weight=0.0), dict(same_shape=False, blend_weight=True, normal_min=-1.0, point_tolerance=INF,
                                                                      max_weight=INF)):
            want = rb.gradient_accumulate_host(*args, before, mv, mo, kp, W, Hh, **par)
            _check(demo.gradient_accumulate(*args, before, mv, mo, kp, W, Hh, **par), want, f"host form {par}")
            fresh = demo.gradient_accumulate(*on_dev, before, *tables, extra[2], W, Hh, device=True, **par)
            _check((planes(fresh[0]), planes(fresh[1]), fresh[2].numpy().reshape(Hh, W)), want, f"device form {par}")
            outs = DeviceBuffer((3, m), np.float64), DeviceBuffer((3, m), np.float64), DeviceBuffer((m,), np.int32)
            for turn in range(2):
                out = demo.gradient_accumulate(*on_dev, before, *tables, extra[2], W, Hh, device=True, stream=st, out=outs[0], out_moments=outs[1],
                                               out_count=outs[2], **par)
                assert all(a is b for a, b in zip(out, outs))
                _check((planes(outs[0]), planes(outs[1]), outs[2].numpy().reshape(Hh, W)), want, f"out= on a stream, turn {turn}, {par}")
            none = demo.gradient_accumulate(*on_dev, before, *tables, None, W, Hh, device=True, stream=st, **par)  # (NULL keep: the motion query)
            _check((planes(none[0]), planes(none[1]), none[2].numpy().reshape(Hh, W)), rb.motion_host(*args, before, mv, mo, W, Hh, **par),
                   f"device form without keep {par}")
            st.synchronize()
        for t, a in zip(on_dev + extra, host_planes + [index, rb.planar(old, 3), kp.reshape(-1)]):  # (the inputs are left alone)
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()
        assert tables[0].cpu().numpy().tobytes() == mv.tobytes() and tables[1].cpu().numpy().tobytes() == mo.tobytes()
        assert (want[2] >= 2).sum() > 0
        # every refusal message
        acc = lambda **kw: demo.gradient_accumulate(*on_dev, before, *tables, extra[2], W, Hh, device=True, stream=st, **kw)  # noqa: E731
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*colour output too small"):
            acc(out=DeviceBuffer((3 * m - 1,), np.float64))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*moments output too small"):
            acc(out_moments=DeviceBuffer((3 * m - 1,), np.float64))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*count output too small"):
            acc(out_count=DeviceBuffer((m - 1,), np.int32))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the previous colour"):
            acc(out=on_dev[5])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the keep plane"):
            demo.gradient_accumulate(*on_dev, before, *tables, outs[0], W, Hh, device=True, stream=st, out=outs[0])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*colour output overlaps the moments output"):
            acc(out=outs[0], out_moments=outs[0])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*n_shapes"):
            acc(n_shapes=2 ** 20 + 1)
        with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE.*keep output too small"):
            demo.gradient_keep(*keep_args, stratum=s, device=True, stream=st, out=DeviceBuffer((m - 1,), np.float64))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*keep output overlaps the colour planes"):
            demo.gradient_keep(*keep_args, stratum=s, device=True, stream=st, out=on_dev[0])
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*radius"):
            demo.gradient_keep(*keep_args, stratum=s, radius=5, device=True, stream=st)
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*gain"):
            demo.gradient_keep(*keep_args, stratum=s, gain=-1.0, device=True, stream=st)
        for k, word in enumerate(("probe index", "probe point", "probe normal", "probe seq")):
            small = list(mine)
            small[k] = DeviceBuffer(((ns - 1,), (3 * ns - 1,), (3 * ns - 1,), (ns - 1,))[k], (np.int32, np.float64, np.float64, np.uint64)[k])
            with pytest.raises(_lib.PtraceError, match=f"PT_ERR_SIZE.*{word} output too small"):
                demo.gradient_probes(*probe_args, stratum=s, device=True, stream=st, out=tuple(small))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*probe point output overlaps the points"):
            demo.gradient_probes(*probe_args, stratum=s, device=True, stream=st, out=(mine[0], on_dev[4], mine[2], mine[3]))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*probe point output overlaps the probe normal output"):
            demo.gradient_probes(*probe_args, stratum=s, device=True, stream=st, out=(mine[0], mine[1], mine[1], mine[3]))
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*stratum"):
            demo.gradient_probes(*probe_args, stratum=17, device=True, stream=st, out=mine)
        with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*samples"):
            demo.gradient_probes(*probe_args, stratum=s, samples=0, device=True, stream=st, out=mine)
        with pytest.raises(ValueError, match="come together"):
            demo.gradient_probes(on_dev[2], on_dev[3], on_dev[4], tables[0], None, W, Hh, device=True, stream=st)
        with pytest.raises(ValueError, match="device=True"):
            demo.gradient_keep(colour, shape, index, old, W, Hh, stream=st)
        with pytest.raises(ValueError, match="records"):
            demo.gradient_accumulate(*args, before, mv, mo, kp, W, Hh + 1)
        with pytest.raises(ValueError, match="probes"):
            demo.gradient_keep(colour, shape, index[:-1], old[:-1], W, Hh, stratum=s)
        # m = 0
        none3, none1 = np.zeros((0, 3)), np.zeros(0, np.int32)
        out, moments, count = demo.gradient_accumulate(none3, none1, none1, none3, none3, none3, none3, none1, none3, none3, none1, before, mv, mo,
                                                       np.zeros(0), 0, 9)
        assert out.shape == (9, 0, 3) and moments.shape == (9, 0, 3) and count.shape == (9, 0)
        assert demo.gradient_keep(none3, none1, none1, none3, 0, 9).shape == (9, 0)
        empty = demo.gradient_probes(none1, none3, none3, mv, mo, 9, 0)
        assert empty[0].shape == (0,) and empty[1].shape == (0, 3) and empty[3].shape == (0,)
        # an empty history
        filled = _to_dev(np.full(m, 7, np.int32))
        torch.cuda.synchronize()
        assert demo.gradient_clear(filled, m, stream=st) is filled
        st.synchronize()
        assert not filled.cpu().numpy().any()
        zero = demo.gradient_clear(DeviceBuffer((m,), np.int32), stream=st)
        first = demo.gradient_accumulate(*on_dev[:10], zero, before, *tables, extra[2], W, Hh, device=True, stream=st)
        nothing = rb.WeightedHistory.empty(W, Hh)
        _check((planes(first[0]), planes(first[1]), first[2].numpy().reshape(Hh, W)),
               rb.gradient_accumulate_host(*args[:5], nothing.colour, nothing.moments, nothing.shape_index, nothing.normal, nothing.point,
                                           nothing.count, before, mv, mo, kp, W, Hh), "the first frame, from lengths the library cleared")
        st.synchronize()
    finally:
        st.close()


@pytest.mark.parametrize("blocks", ["1", "2", "7"])
def test_no_bit_depends_on_the_launch(demo, blocks):
    W, Hh = 70, 33
    before, args = M.inputs(W, Hh, "perspective", "turned1", 61)
    colour, shape, normal, point = args[0], args[2], args[3], args[4]
    assert "PTRACE_GR_BLOCKS" not in os.environ
    mv, mo = M.table("sheared")
    kp = G.hostile_keep(W, Hh, 62)

    def run():
        out = []
        for s, radius in ((1, 1), (3, 2), (4, 4)):
            probes = demo.gradient_probes(shape, normal, point, mv, mo, W, Hh, stratum=s, phase=3, samples=2)
            index = G.hostile_index(W, Hh, s, 63, probes[0])
            out.append((probes, demo.gradient_keep(colour, shape, index, G.probe_old(colour, index, 64), W, Hh, stratum=s, radius=radius, gain=3.0)))
        return out, demo.gradient_accumulate(*args, before, mv, mo, kp, W, Hh, max_history=5)

    want = run()
    _check(want[1], rb.gradient_accumulate_host(*args, before, mv, mo, kp, W, Hh, max_history=5), "default launch")
    os.environ["PTRACE_GR_BLOCKS"] = blocks
    try:
        got = run()
    finally:
        del os.environ["PTRACE_GR_BLOCKS"]
    for (gp, gk), (wp, wk) in zip(got[0], want[0]):
        _check_probes(gp, wp, f"{blocks} workgroups")
        _check_keep(gk, wk, f"{blocks} workgroups")
    _check(got[1], want[1], f"{blocks} workgroups")


# ---- 4. what it is for --------------------------------------------------------------------------------------------------------------
def _moved_demo(f, dy=0.4):
    world, camera = scenes.demo_world()
    sphere = copy.copy(world.shapes[2])
    sphere.transformation = hm.translation(hm.Vec(0.0, dy * f, 0.0)) * sphere.transformation
    world.shapes[2] = sphere
    return world, camera


def test_three_updates_in_hbm_shorten_the_history_under_the_shadow_and_equal_the_mirrors_chained_on_the_host(dev):
    """``GradientAccumulator(device=True)``: the sphere of the demo world is translated by 0.4 along y per frame and the camera turns by
    a degree; every frame has a ``DeviceScene`` of its own (the previous one stays open for the probes' gather), hit frames alternate
    between two device buffers, the 2-sample gather stays in HBM.  After every ``update`` the downloaded keep plane, colour, moments,
    lengths and variance are what the mirrors, chained on the host, give; after the third, a ground pixel within two radii of the
    sphere's foot has keep < 1 and a history shorter than ``MotionAccumulator`` leaves there on the same gathers.  (Confirmed on the
    CPU with the mirrors and the oracle's gather before this ran on a device: 29 of the 35 ground pixels there have keep < 1 after the
    third frame, 28 of them with a shorter history.)"""
    import torch

    from pytracer_amd import flatten
    from pytracer_amd.devmem import DeviceBuffer, Stream
    from pytracer_amd.hits import HitFrame

    W, Hh, K = 48, 36, 2
    m = W * Hh
    par_f = abi.make_params(W, Hh, abi.RENDERER_FLAT, samples_per_side=0)
    params = dict(max_history=8, max_weight=12.0, min_history=2)
    history = {k: v for k, v in params.items() if k != "min_history"}
    spread = dict(stratum=3, radius=1, gain=4.0)
    st = Stream()
    scenes_open = []
    try:
        acc = plain = None
        buffers = [DeviceBuffer((abi.hits_bytes(par_f, abi.HIT_ALL),), np.uint8) for _ in range(2)]
        prev = plain_prev = rb.WeightedHistory.empty(W, Hh)
        prev_camera = prev_world = prev_scene = None
        seq = 54
        for f in range(3):
            world, camera = _moved_demo(f)
            now = scenes.turned_camera(camera, 1.0 * f)
            ds = dev.DeviceScene(flatten.flatten_world(world))
            scenes_open.append(ds)
            q = rb.WorldQueries(ds)
            if acc is None:
                acc = rb.GradientAccumulator(q, device=True, stream=st, **params, **spread)
                plain = rb.MotionAccumulator(q, device=True, stream=st, **params)
            hits = buffers[f & 1]
            ds.render_hits_into(flatten.flatten_camera(now), par_f, abi.HIT_ALL, hits, stream=st)
            g = rb.DeviceGuides.of_hit_buffer(hits, par_f, abi.HIT_ALL)
            shape, normal, point = guides(HitFrame(hits.numpy(), par_f, abi.HIT_ALL))
            gathered = ds.gather(g.point, g.normal, K, 42, None, g.shape_index, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none", init_seq=seq, device=True,
                                 stream=st, n=m)
            taken = np.where(shape >= 0, K, 0).astype(np.int32)
            samples = _to_dev(taken.reshape(-1))
            torch.cuda.synchronize()
            probe = dict(samples=K, init_state=42, init_seq=seq, max_depth=2, russian_roulette_limit=3, background=(0.0, 0.0, 0.0), depth=1)
            out, variance = acc.update(gathered, g, now, samples=samples, world=world, queries=q, probe=probe, width=W, height=Hh)
            plain.update(gathered, g, now, samples=samples, world=world, queries=q, width=W, height=Hh)
            assert acc.frames == f + 1
            colour = np.ascontiguousarray(gathered.numpy()[: 24 * m].view(np.float64).reshape(3, m).T).reshape(Hh, W, 3)
            table = (None, None) if prev_world is None else rb.shape_motion(prev_world, world)
            assert f == 0 or table[0].tolist() == [0, 0, 1]
            keep = None
            if f > 0:  # the chain on the host: probes, the gather on the PREVIOUS scene (host form), keep
                index, pp, nn, seqs = rb.gradient_probes_host(shape, normal, point, *table, W, Hh, stratum=3, phase=f, samples=K, init_seq=seq)
                old = np.array(prev_scene.gather(rb.planar(pp, 3), rb.planar(nn, 3), K, 42, seqs, index, 1, 2, 3, (0.0, 0.0, 0.0), 1, "none").radiance)
                keep = rb.gradient_keep_host(colour, shape, index, old, W, Hh, **spread)
                _check_keep(acc.keep.numpy()[:m].reshape(Hh, W), keep, f"update {f}: keep")
                assert (keep < 1.0).any() and (keep == 1.0).any()
            else:
                assert acc.keep is None
            cam_before = prev_camera if prev_camera is not None else now
            want = rb.gradient_accumulate_host(colour, taken, shape, normal, point, prev.colour, prev.moments, prev.shape_index, prev.normal,
                                               prev.point, prev.count, cam_before, *table, keep, W, Hh, **history)
            plane = lambda b: np.ascontiguousarray(b.numpy()[:, :m].T).reshape(Hh, W, 3)  # noqa: E731
            _check((plane(out), plane(acc.moments), acc.count.numpy().reshape(Hh, W)), want, f"update {f}")
            want_variance = rb.variance_estimate_host(want[1], want[2], shape, normal, point, W, Hh, min_history=2)
            bad = H.differing(variance.numpy()[:m].reshape(-1, 1), want_variance.reshape(-1, 1))
            assert bad.size == 0, f"update {f}: {bad.size} variances differ"
            followed = rb.motion_host(colour, taken, shape, normal, point, plain_prev.colour, plain_prev.moments, plain_prev.shape_index,
                                      plain_prev.normal, plain_prev.point, plain_prev.count, cam_before, *table, W, Hh, **history)
            assert np.array_equal(plain.count.numpy().reshape(Hh, W), followed[2])
            prev = rb.WeightedHistory(want[0], shape.copy(), normal.copy(), point.copy(), want[2], want[1])
            plain_prev = rb.WeightedHistory(followed[0], shape.copy(), normal.copy(), point.copy(), followed[2], followed[1])
            prev_camera, prev_world, prev_scene = now, world, ds
            seq += m * K
        centre = np.array(world.shapes[2].transformation.m)[:3, 3]
        assert abs(centre[2] - 1.0) < 1e-12  # (a unit sphere resting on the ground z = 0)
        ground = (shape >= 0) & (shape != 2) & (np.abs(point[..., 2]) < 1e-9)
        foot = ground & (np.hypot(point[..., 0] - centre[0], point[..., 1] - centre[1]) <= 2.0)
        cut = foot & (keep < 1.0) & (want[2] < followed[2])
        print(f"{int(foot.sum())} ground pixels within two radii of the foot after frame 2: {int((foot & (keep < 1.0)).sum())} with keep < 1, "
              f"{int(cut.sum())} of them with a history shorter than the motion query's")
        assert foot.sum() > 10 and cut.any()
        st.synchronize()
    finally:
        st.close()
        for ds in scenes_open:
            ds.close()


# ---- 5. the shader ------------------------------------------------------------------------------------------------------------------
def test_the_shader_on_a_static_and_on_a_moving_world(dev):
    """``GradientGatherShader`` for three frames at 48 x 36.  On a static world every byte is that of the same shader not following the
    light (``MovingWorldGatherShader``: contract G, then E, through every layer).  On a world whose sphere moves 0.4 per frame the
    frames are finite and some histories are shorter than the parent leaves them."""
    from pytracer_amd.shaders import GradientGatherShader
    from pytracer_amd.tracer import GpuImageTracer

    W, Hh, N = 48, 36, 3

    def run(dy, follow_light):
        _, camera = scenes.demo_world()
        tracer = GpuImageTracer(hm.HdrImage(W, Hh), camera, samples_per_side=0)
        try:
            shader = GradientGatherShader(_moved_demo(0, dy)[0], tracer, samples=2, max_depth=2, passes=2, max_history=8)
            shader.follow_light = follow_light
            frames = []
            for f in range(N):
                tracer.camera = scenes.turned_camera(camera, 1.0 * f)
                shader.world = _moved_demo(f, dy)[0]
                frame = tracer.fire_all_hits(shader.world)
                frames.append(shader.shade_hits(frame))
            return frames, np.asarray(shader.accumulator.count), type(shader.accumulator).__name__, getattr(shader.accumulator, "keep", None)
        finally:
            tracer.close()

    still, still_count, kind, keep = run(0.0, True)
    plain, plain_count, plain_kind, _ = run(0.0, False)
    assert (kind, plain_kind) == ("GradientAccumulator", "MotionAccumulator")
    for a, b in zip(still, plain):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
    assert np.array_equal(still_count, plain_count) and still_count.max() == N and keep.tobytes() == np.ones((Hh, W)).tobytes()
    moving, count, _, keep = run(0.4, True)
    _, parent_count, _, _ = run(0.4, False)
    assert all(np.isfinite(f).all() for f in moving)
    print(f"{int((keep < 1.0).sum())} pixels with keep < 1, {int((count < parent_count).sum())} with a history shorter than the parent's")
    assert (keep < 1.0).any() and (count <= parent_count).all() and (count < parent_count).any()
