"""Scatter queries on the device (include/ptrace_scatter.h, libptrace_scatter.so): the Russian roulette and ``brdf.scatter_ray``
of hit records that carry their generators, against the CPU oracle in its ``x * x`` mode (tests/scatter_batches.py), against the
fused path tracer of libptrace.so, and against themselves across channels, batch sizes and entry points.

Expected agreement.  The records are the oracle's own, fed as host arrays, so everything that involves no libm call is compared
bit for bit: status, the generator's state and increment, origin, tmin, tmax, weight, emitted, the dead rays, and the direction
of every mirror bounce (sqrt and division only).  The direction of a diffuse bounce holds ocml's sin / cos against glibc's: to
``rel=1e-12`` with more than half of the rows bit-identical, the two conditions tests/test_gpu_probes.py applies to this very
function.  Device against device (the shader route against the fused kernel, the chain in HBM against the host route): byte for
byte."""
import numpy as np
import pytest

from pytracer_amd import abi, rays as rb, shaders
from pytracer_amd import hostmodel as hm

from . import scatter_batches as X
from . import surface_batches as S
from . import util

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1001)


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
            open_[name] = dev.DeviceScene((X.world(name) if name in X.WORLDS else S.world(name))[0])
        return open_[name]

    yield get
    for ds in open_.values():
        ds.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)) + 1e-300)


def _scatter(ds, b, k, roulette, channels="all", **kw):
    rec = b["rec"]
    return ds.scatter(rec.shape_index[k], rec.point[k], rec.normal[k], rec.uv[k], b["dirs"][k], b["pcg"][:, k], roulette, channels, **kw)


MIN_FOR_SHARE = 30  # diffuse directions from which on their bit-identical share is asserted (a share of three rows says nothing)


def _compare(got, want, k, label):
    """One scatter batch against rows ``k`` of the helper's expectation: everything but the diffuse directions bit for bit; those
    to 1e-12, every one of them, and more than half bit-identical wherever the batch holds ``MIN_FOR_SHARE`` of them."""
    status, kind = want["status"][k], want["kind"][k]
    assert _bits(got.status, status), f"{label}: status differs in {int((got.status != status).sum())} records"
    assert _bits(got.pcg, want["pcg"][:, k]), f"{label}: generators differ in {int(np.any(got.pcg != want['pcg'][:, k], axis=0).sum())} records"
    rays = want["rays"][:, k]
    for rows, what in ((slice(0, 3), "origin"), (slice(6, 7), "tmin"), (slice(7, 8), "tmax")):
        assert _bits(got.rays[rows], rays[rows]), f"{label}: {what}"
    assert _bits(got.weight, want["weight"][k]) and _bits(got.emitted, want["emitted"][k]), f"{label}: weight / emitted"
    diffuse = (status == 1) & (kind == abi.BRDF_DIFFUSE)
    assert _bits(got.rays[3:6][:, ~diffuse], rays[3:6][:, ~diffuse]), f"{label}: a mirror direction or a dead ray"
    if diffuse.any():
        g, w = got.rays[3:6][:, diffuse].T, rays[3:6][:, diffuse].T
        same = util.bits_equal_rows(g, w)
        den = np.maximum(np.abs(g), np.abs(w))
        worst = float(np.max(np.where(den > 0, np.abs(g - w) / np.where(den > 0, den, 1.0), 0.0)))
        print(f"{label}: {int(diffuse.sum())} diffuse directions, {same.mean():.1%} bit-identical, worst relative difference {worst:.3g}")
        assert _close(g, w, rel=1e-12), f"{label}: a diffuse direction beyond 1e-12 (worst {worst:.3g})"
        if diffuse.sum() >= MIN_FOR_SHARE:
            assert same.mean() > 0.5, f"{label}: only {same.mean():.0%} of the diffuse directions are bit-identical"


# ---- 1. against the oracle, per world ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roulette", [False, True])
@pytest.mark.parametrize("name", X.WORLDS)
def test_scatter_equals_the_oracle(scene_of, orc, name, roulette):
    b = X.batch(orc, name)
    got = _scatter(scene_of(name), b, slice(None), roulette)
    assert got.n == b["rec"].n and got.channels == rb.SCAT_ALL
    _compare(got, b["want"][roulette], slice(None), f"{name} roulette={int(roulette)}")


def test_a_draw_equal_to_q_ends_the_path(scene_of, orc):
    """``draw > q``, not ``>=``: records on the tiny world's black sphere (q = 1.0) whose generators are set to draw exactly 1.0.
    The path ends and the weight stays (0, 0, 0); with ``>=`` it would be 0 * (1 / 0)."""
    b = X.batch(orc, "roulette4")
    rec = b["rec"]
    black = np.flatnonzero(np.asarray(rec.shape_index) == 0)
    assert black.size > 10
    pcg = np.array(b["pcg"])
    pcg[0, black[::2]] = X.state_drawing_one()  # (every other one: aimed and ordinary draws side by side)
    want = X.expected(orc, X.world("roulette4")[0], rec, b["dirs"], pcg, True)
    aimed = black[::2]
    assert np.all(want["status"][aimed] == 0) and not want["weight"][aimed].any() and np.all(want["pcg"][0, aimed] != pcg[0, aimed])
    got = scene_of("roulette4").scatter(rec.shape_index, rec.point, rec.normal, rec.uv, b["dirs"], pcg, True)
    _compare(got, want, slice(None), "roulette4, aimed draws")
    assert np.isfinite(got.weight).all()


# ---- 2. batch sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_around_the_wave_and_the_block(scene_of, orc, n):
    """The last wave and the last block partly idle; an odd n pads the status plane.  Cut from the c2 batch across its boundary
    between primary rays and bounces.  (The cut of ONE record is one diffuse bounce, whose direction is held to 1e-12 like every
    other; a share of bit-identical rows exists from ``MIN_FOR_SHARE`` rows on, which every other cut has -- asserted below.)"""
    b = X.batch(orc, "c2")
    start = b["n_primary"] - n // 2
    k = slice(start, start + n)
    got = _scatter(scene_of("c2"), b, k, True)
    assert got.nbytes == ((n * 4 + 7) // 8 * 8) + 128 * n == got.buffer.nbytes
    want = b["want"][True]
    n_diffuse = int(((want["status"][k] == 1) & (want["kind"][k] == abi.BRDF_DIFFUSE)).sum())
    assert (n_diffuse >= MIN_FOR_SHARE) == (n > 1), (n, n_diffuse)
    _compare(got, want, k, f"c2[{start}:{start + n}]")


# ---- 3. misses -------------------------------------------------------------------------------------------------------------------
def test_misses_only_and_interleaved(scene_of, orc):
    b = X.batch(orc, "c2")
    ds = scene_of("c2")
    rec, n = b["rec"], 1001
    k = slice(0, n)
    dead = np.tile(X.DEAD_RAY[:, None], (1, n))
    for roulette in (False, True):
        none = np.full(n, -1, np.int32)
        got = ds.scatter(none, rec.point[k], rec.normal[k], rec.uv[k], b["dirs"][k], b["pcg"][:, k], roulette)
        assert np.all(got.status == -1) and _bits(got.rays, dead) and _bits(got.pcg, b["pcg"][:, k])  # no hit: nothing is drawn
        assert not got.weight.any() and not got.emitted.any() and not got.scattered.any()
        # every other record a miss (also shape indices beyond the world's): lanes with and without a hit side by side
        some = np.array(rec.shape_index[k])
        some[::2] = -1
        some[4::8] = 10 ** 6
        miss = (some < 0) | (some >= 10 ** 6)
        got = ds.scatter(some, rec.point[k], rec.normal[k], rec.uv[k], b["dirs"][k], b["pcg"][:, k], roulette)
        want = b["want"][roulette]
        assert _bits(got.status, np.where(miss, -1, want["status"][k]).astype(np.int32))
        assert _bits(got.pcg, np.where(miss[None, :], b["pcg"][:, k], want["pcg"][:, k]))
        assert _bits(got.weight, np.where(miss[:, None], 0.0, want["weight"][k])) and _bits(got.emitted, np.where(miss[:, None], 0.0, want["emitted"][k]))
        assert _bits(got.rays[:, miss], dead[:, miss]) and _bits(got.rays[[0, 1, 2, 6, 7]][:, ~miss], want["rays"][[0, 1, 2, 6, 7]][:, k][:, ~miss])


# ---- 4. channels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [0, rb.SCAT_WEIGHT, rb.SCAT_EMITTED, rb.SCAT_ALL])
def test_every_channel_combination_at_the_librarys_offsets(scene_of, orc, channels):
    from pytracer_amd import _scatter_lib

    L = _scatter_lib.lib()
    b = X.batch(orc, "pigments")
    n = 257
    k = slice(0, n)
    want = b["want"][True]
    got = _scatter(scene_of("pigments"), b, k, True, channels)
    assert got.buffer.nbytes == L.pt_rays_scatter_bytes(n, channels) == got.nbytes
    assert _bits(got.buffer[: 4 * n].view(np.int32), want["status"][k])
    plane = lambda sel, comp, dt=np.float64: got.buffer[L.pt_rays_scatter_plane_offset(n, channels, sel, comp):][: 8 * n].view(dt)  # noqa: E731
    for comp in (0, 1, 2, 6, 7):
        assert _bits(plane(rb.SCAT_RAYS, comp), np.ascontiguousarray(want["rays"][comp, k]))
    for comp in (0, 1):
        assert _bits(plane(rb.SCAT_PCG, comp, np.uint64), np.ascontiguousarray(want["pcg"][comp, k]))
    for bit, key in ((rb.SCAT_WEIGHT, "weight"), (rb.SCAT_EMITTED, "emitted")):
        for comp in range(3):
            if channels & bit:
                assert _bits(plane(bit, comp), np.ascontiguousarray(want[key][k, comp]))
            else:
                assert L.pt_rays_scatter_plane_offset(n, channels, bit, comp) < 0 and not got.has(key)


# ---- 5. the dead rays are dead ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["demo", "wide300_lights"])
def test_the_dead_rays_hit_nothing(scene_of, orc, name):
    """``trace_rays`` on a scattered block as it stands: -1 for every record whose status is not 1 -- misses, records the roulette
    ended -- in a small world and in one whose queries walk the grid; and the live records go on hitting things."""
    b = X.batch(orc, name) if name in X.WORLDS else S.batch(orc, name)
    rec = b["rec"]
    ds = scene_of(name)
    if name == "wide300_lights":
        assert S.world(name)[0].n_shapes > 256
    sc = ds.scatter(rec.shape_index, rec.point, rec.normal, rec.uv, b["rays"][:, 3:6], X.streams(rec.n), True)
    dead = sc.status != 1
    assert dead.sum() > 100 and (sc.status == 0).sum() > 50 and (~dead).sum() > 100
    assert _bits(sc.rays[:, dead], np.tile(X.DEAD_RAY[:, None], (1, int(dead.sum()))))
    nxt = ds.trace_rays(sc.rays)
    assert np.all(nxt.shape_index[dead] == -1) and np.all(np.isinf(nxt.t[dead])) and not nxt.point[dead].any()
    assert (nxt.shape_index[~dead] >= 0).sum() > 50
    # ... and a dead record stays dead through the next bounce without anything being compacted
    sc2 = ds.scatter(nxt.shape_index, nxt.point, nxt.normal, nxt.uv, sc.dirs, sc.pcg, True)
    assert np.all(sc2.status[dead] == -1) and _bits(sc2.pcg[:, dead], sc.pcg[:, dead])


# ---- 6. a chain that stays in HBM ------------------------------------------------------------------------------------------------
def test_a_chain_that_stays_in_hbm(dev, orc):
    """trace_rays(device=True) -> scatter(device=True) reading planes by offset -> trace_rays on the output's ray block -> scatter
    again with the output's generator and direction planes; one stream, one download at the end: byte for byte the same chain
    through host arrays."""
    import torch

    from pytracer_amd.devmem import DeviceBuffer, DeviceSpan, Stream

    b = X.batch(orc, "demo")
    flat = X.world("demo")[0]
    n = 1001
    first = b["n_primary"] - n // 2
    block = np.ascontiguousarray(rb.ray_planes(b["rays"][first:first + n]))
    pcg = X.streams(n, first)
    ALL = rb.RAY_CHANNELS
    ds = dev.DeviceScene(flat)
    st = Stream()
    try:
        # the host route
        h1 = ds.trace_rays(block)
        s1 = ds.scatter(h1.shape_index, h1.point, h1.normal, h1.uv, block[3:6].T, pcg, False)
        h2 = ds.trace_rays(s1.rays)
        s2 = ds.scatter(h2.shape_index, h2.point, h2.normal, h2.uv, s1.dirs, s1.pcg, True)
        assert s1.scattered.sum() > 100 and min((s2.status == v).sum() for v in (-1, 0, 1)) >= 10  # (live, ended and dead records all travel)
        # the same on the device
        rays_dev = torch.from_numpy(block).cuda()
        pcg_dev = torch.from_numpy(pcg.view(np.int64)).cuda()
        torch.cuda.synchronize()

        def planes(buf):
            base = buf.data_ptr()
            return [base] + [base + rb.rays_plane_offset(n, ALL, False, ch, 0) for ch in (abi.HIT_POINT, abi.HIT_NORMAL, abi.HIT_UV)]

        soff = lambda sel, comp=0: rb.scatter_plane_offset(n, rb.SCAT_ALL, sel, comp)  # noqa: E731
        r1 = ds.trace_rays(rays_dev, ALL, device=True, stream=st)
        d1 = ds.scatter(*planes(r1), rays_dev.data_ptr() + 3 * n * 8, pcg_dev, False, "all", device=True, stream=st, n=n)
        r2 = ds.trace_rays(DeviceSpan(d1, 64 * n, soff(rb.SCAT_RAYS)), ALL, device=True, stream=st)
        mine = DeviceBuffer((rb.scatter_bytes(n, rb.SCAT_ALL),), np.uint8)
        d2 = ds.scatter(*planes(r2), d1.data_ptr() + soff(rb.SCAT_RAYS, 3), (d1.data_ptr() + soff(rb.SCAT_PCG, 0), d1.data_ptr() + soff(rb.SCAT_PCG, 1)),
                        True, "all", device=True, stream=st, out=mine, n=n)
        assert d2 is mine
        got = mine.numpy()  # (numpy(): behind the stream the chain ran on)
        pad = (4 * n + 7) // 8 * 8  # (n is odd: four bytes behind the status plane belong to nobody)
        for dev_buf, host in ((got, s2), (d1.numpy(), s1)):
            assert dev_buf[: 4 * n].tobytes() == host.buffer[: 4 * n].tobytes(), "the chain in HBM differs from the chain through host arrays"
            assert dev_buf[pad: host.nbytes].tobytes() == host.buffer[pad:].tobytes(), "the chain in HBM differs from the chain through host arrays"
        with pytest.raises(ValueError, match="n="):
            ds.scatter(r2.data_ptr(), 0, 0, 0, 0, pcg_dev, False, device=True)
        with pytest.raises(ValueError, match="device=True"):
            ds.scatter(h1.shape_index, h1.point, h1.normal, h1.uv, block[3:6].T, pcg, False, stream=st)
    finally:
        st.close()
        ds.close()


# ---- 7. end to end, device against device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", [0, 2])
@pytest.mark.parametrize("name,W,H", [("demo", 40, 30), ("c2", 48, 27)])
def test_the_shader_route_equals_the_fused_path_tracer(dev, name, W, H, S_):
    """``PathTracer`` rebuilt from the public pieces -- hit-record frame, then per depth scatter and trace, the sums on the host
    -- against the fused kernels under ``pcg_mode="sample"``, byte for byte: both routes run the same device functions under the
    same flags on the same records."""
    from pytracer_amd.tracer import GpuImageTracer

    world, camera = S.host_world(name)
    assert (W, H) == S.WORLDS[name]
    bg = hm.Color(0.25, 0.5, 0.125)
    fused = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode="sample")
    mine = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode="sample")
    try:
        fused.fire_all_rays(hm.PathTracer(world, bg, hm.PCG(45, 54), num_of_rays=1, max_depth=3, russian_roulette_limit=2))
        mine.fire_all_rays(shaders.PathTracerShader(world, mine, bg, hm.PCG(45, 54), num_of_rays=1, max_depth=3, russian_roulette_limit=2))
        assert fused.last_path == "device" and mine.last_path == "device-hits"
        a, b = np.asarray(fused.image.array), np.asarray(mine.image.array)
        assert a.shape == (H, W, 3) and len(np.unique(a.reshape(-1, 3), axis=0)) > 8
        assert _bits(b, a), f"{int(np.any(a != b, axis=-1).sum())} of {W * H} pixels differ"
    finally:
        fused.close()
        mine.close()
