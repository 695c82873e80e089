"""CPU-only tests of the scatter queries (include/ptrace_scatter.h, libptrace_scatter.so, pytracer_amd.rays / .shaders): the
fourth library builds and loads without a GPU and leaves the other three as they were; its header, the ctypes table and its
dynamic symbols agree; sizes and offsets match their Python mirrors; bad arguments are refused before any HIP call;
``pcg_streams`` is the oracle's generator word for word; the batches the GPU tests compare hold every case they are meant to; and
``PathTracerShader`` -- with every device answer replaced by the oracle's -- is the oracle's ``PathTracer`` bit for bit, which
pins the seeding of the streams, the order of the draws and the unwinding of the recursion without a GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi, flatten, hits, rays as rb, shaders
from pytracer_amd import hostmodel as hm
from pytracer_amd.tracer import GpuImageTracer

from . import ray_batches as B
from . import scatter_batches as X
from . import seed_sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_SIZE = -1, -5  # include/ptrace.h
V11, V12 = (1 << 16) | 1, (1 << 16) | 2
SIZES = [0, 1, 63, 64, 65, 1001, 2 ** 31 - 1]


@pytest.fixture(scope="module")
def libs():
    from pytracer_amd import _lib, _rays_lib, _scatter_lib, _surface_lib, build

    build.build()
    assert os.path.exists(build.SCATTER_LIB) and not build.needs_build()
    return _lib.lib(), _rays_lib.lib(), _surface_lib.lib(), _scatter_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(libs):
    from pytracer_amd import _scatter_lib, build

    _, R, Sf, Sc = libs
    header = open(os.path.join(ROOT, "include", "ptrace_scatter.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_scatter_lib.EXPORTS) and len(declared) == 7
    assert _exported(_scatter_lib.lib_path()) == declared
    # an add-on like the other two: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _scatter_lib.lib_path()], capture_output=True, text=True).stdout
    assert "libptrace" not in needed.replace("libptrace_scatter.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _scatter_lib.lib_path()], capture_output=True, text=True).stdout
    assert not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    # interface 1.2 here, 1.1 in the two halves before it; one argument block for all
    assert Sc.pt_rays_scatter_version() == V12 and R.pt_rays_version() == V11 and Sf.pt_rays_surface_version() == V11
    assert Sc.pt_rays_scatter_args_bytes() == R.pt_rays_args_bytes() == Sf.pt_rays_surface_args_bytes() > 0
    # the only file that includes the new device header is the new translation unit, and the recipe watches the public header
    users = [f for f in os.listdir(build.CSRC) if '"pt_scatter.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_scatter.hip"]
    assert os.path.normpath(os.path.join("..", "..", "include", "ptrace_scatter.h")) in {os.path.normpath(d) for d in build.DEPS}


def test_the_other_three_libraries_are_what_they_were(libs):
    from pytracer_amd import _lib, _rays_lib, _surface_lib, build

    assert _exported(_rays_lib.lib_path()) == set(_rays_lib.EXPORTS) and len(_rays_lib.EXPORTS) == 7
    assert _exported(_surface_lib.lib_path()) == set(_surface_lib.EXPORTS) and len(_surface_lib.EXPORTS) == 11
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert build.code_hash() == json.load(open(os.path.join(ROOT, "profiles", "pmc_c2.json")))["code_hash"]
    for header in ("ptrace_rays.h", "ptrace_surface.h"):
        assert "pt_rays_scatter" not in open(os.path.join(ROOT, "include", header)).read()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_offsets_match_the_python_mirror(libs, n):
    Sc = libs[3]
    pad = (n * 4 + 7) // 8 * 8
    for channels in range(4):
        want = rb.scatter_bytes(n, channels)
        assert Sc.pt_rays_scatter_bytes(n, channels) == want == pad + 80 * n + 24 * n * bin(channels).count("1")
        assert Sc.pt_rays_scatter_plane_offset(n, channels, 0, 0) == 0 and Sc.pt_rays_scatter_plane_offset(n, channels, 0, 1) == ERR_INVALID
        at = pad
        for sel, count in ((rb.SCAT_RAYS, 8), (rb.SCAT_PCG, 2)):  # always there, back to back behind the status plane
            for comp in range(-1, count + 2):
                got = Sc.pt_rays_scatter_plane_offset(n, channels, sel, comp)
                assert got == rb.scatter_plane_offset(n, channels, sel, comp)
                assert got == at + comp * n * 8 if 0 <= comp < count else got < 0
            at += count * n * 8
        for bit in (rb.SCAT_WEIGHT, rb.SCAT_EMITTED):
            for comp in range(-1, 4):
                got = Sc.pt_rays_scatter_plane_offset(n, channels, bit, comp)
                assert got == rb.scatter_plane_offset(n, channels, bit, comp)
                assert got == at + comp * n * 8 if channels & bit and 0 <= comp < 3 else got < 0
            if channels & bit:
                at += 24 * n
        assert at == want
        for bad in (3, 5, 16):  # no such channel
            assert Sc.pt_rays_scatter_plane_offset(n, channels, bad, 0) < 0 and rb.scatter_plane_offset(n, channels, bad, 0) < 0
    for bad in (4, 7, 8, -1, 1 << 20):  # (4 and 8 select planes of plane_offset; they are no channel bits)
        assert Sc.pt_rays_scatter_bytes(n, bad) == 0 and rb.scatter_bytes(n, bad) == 0
        assert Sc.pt_rays_scatter_plane_offset(n, bad, 0, 0) == ERR_INVALID and rb.scatter_plane_offset(n, bad, 0, 0) < 0
    assert Sc.pt_rays_scatter_bytes(-1, 3) == 0 and Sc.pt_rays_scatter_bytes(2 ** 31, 3) == 0 and rb.scatter_bytes(2 ** 31, 3) == 0


def _block(Sc):
    """A block nobody uploaded, with what the checks read: a non-null `cold` (never dereferenced by a refused call), no shapes."""
    nb = int(Sc.pt_rays_scatter_args_bytes())
    block = C.create_string_buffer(nb)
    C.memmove(block, (C.c_uint64 * 1)(0x1000), 8)
    return block, nb


def test_every_refusal_comes_before_a_hip_call(libs):
    """No GPU here: a call that reached the HIP runtime would answer PT_ERR_NODEVICE or PT_ERR_HIP instead."""
    from pytracer_amd import _scatter_lib

    Sc = libs[3]
    block, nb = _block(Sc)
    n = 5
    shape, uv, v3, gen = np.zeros(n, np.int32), np.zeros((2, n)), np.zeros((3, n)), np.zeros((2, n), np.uint64)
    out = np.zeros(rb.scatter_bytes(n, 3), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    slots = C.c_void_p(0x2000)  # (a device address nobody reads in a refused call)
    bad = ERR_INVALID

    def call(device=0, blk=block, nbytes=nb, sl=slots, sh=p(shape), pt=p(v3), nr=p(v3), u=p(uv), d=p(v3), st=p(gen), inc=p(gen[1]), count=n,
             rr=1, ch=3, o=p(out), ob=out.nbytes):
        host = Sc.pt_rays_scatter(device, blk, nbytes, sh, pt, nr, u, d, st, inc, count, rr, ch, o, ob)
        return host, Sc.pt_rays_scatter_device(device, blk, nbytes, sl, sh, pt, nr, u, d, st, inc, count, rr, ch, o, ob, None)

    assert call(count=-1) == (bad, bad) and call(count=2 ** 31) == (bad, bad)          # n out of range
    assert call(nbytes=nb - 8) == (bad, bad) and call(nbytes=nb + 8) == (bad, bad)      # a block of another size
    assert call(blk=None) == (bad, bad) and call(device=-1) == (bad, bad)
    assert call(blk=C.create_string_buffer(nb)) == (bad, bad)                          # a block nobody filled
    for name in ("sh", "pt", "nr", "u", "d", "st", "inc", "o"):                         # every plane is needed, uv too
        assert call(**{name: None}) == (bad, bad), name
    assert call(sl=None)[1] == bad                                                       # (the host form makes the table itself)
    assert call(ob=out.nbytes - 1) == (ERR_SIZE, ERR_SIZE) and "too small" in _scatter_lib.last_error()
    assert call(ob=rb.scatter_bytes(n, 1), ch=1)[1] != ERR_SIZE and call(ob=rb.scatter_bytes(n, 1), ch=3) == (ERR_SIZE, ERR_SIZE)
    for ch in (4, 8, -1, 1 << 20):                                                       # unknown channel bits
        assert call(ch=ch) == (bad, bad)
    for rr in (2, -1, 256):                                                              # roulette outside {0, 1}
        assert call(rr=rr) == (bad, bad) and "roulette" in _scatter_lib.last_error()
    # n = 0: PT_OK, nothing launched (so: no device needed), nothing written
    out[:] = 0xA5
    none = dict(sh=None, pt=None, nr=None, u=None, d=None, st=None, inc=None, o=None, ob=0)
    assert call(count=0) == (0, 0) and call(count=0, **none) == (0, 0) and call(count=0, rr=0, ch=0) == (0, 0)
    assert np.all(out == 0xA5)
    assert call(count=0, rr=2) == (bad, bad) and call(count=0, ch=4) == (bad, bad)  # (but a bad argument stays one)


def test_channels_and_views():
    assert rb.scatter_channels("all") == 3 and rb.scatter_channels("none") == 0 and rb.scatter_channels("emitted") == rb.SCAT_EMITTED
    assert rb.scatter_channels("emitted, weight") == 3 and rb.scatter_channels(1) == rb.SCAT_WEIGHT
    for bad in ("uv", 4, 8, -1):
        with pytest.raises(ValueError):
            rb.scatter_channels(bad)
    n = 5
    buf = np.zeros(rb.scatter_bytes(n, 3), np.uint8)
    sc = rb.ScatteredRays(buf, n)
    sc.status[:] = [1, -1, 0, 1, -1]
    sc.rays[:, 3] = np.arange(8.0)
    sc.pcg_state[3], sc.pcg_inc[3] = 2 ** 64 - 1, 7
    sc.emitted[2] = (1.0, 2.0, 3.0)
    pad = 24
    assert np.array_equal(buf[pad:pad + 64 * n].view(np.float64).reshape(8, n)[:, 3], np.arange(8.0))
    assert np.array_equal(buf[pad + 64 * n:pad + 80 * n].view(np.uint64).reshape(2, n)[:, 3], [2 ** 64 - 1, 7])
    assert np.array_equal(buf[pad + 104 * n:].view(np.float64).reshape(3, n)[:, 2], [1.0, 2.0, 3.0])
    assert np.array_equal(sc.scattered, [True, False, False, True, False]) and np.array_equal(sc.dirs[3], [3.0, 4.0, 5.0])
    assert sorted(sc.planes()) == ["emitted", "pcg_inc", "pcg_state", "rays", "status", "weight"] and sc.pcg.shape == (2, n)
    for view in (sc.rays, sc.pcg, sc.dirs, sc.weight, sc.emitted, sc.status):
        assert np.shares_memory(view, buf)
    assert np.shares_memory(rb.planar(sc.dirs, 3), buf)  # the next step's `dirs`: no copy
    only = rb.ScatteredRays(np.zeros(rb.scatter_bytes(6, 2), np.uint8), 6, "emitted", shape=(1, 2, 3))
    assert only.emitted.shape == (1, 2, 3, 3) and only.status.shape == (1, 2, 3) and only.pcg_state.shape == (1, 2, 3) and not only.has("weight")
    with pytest.raises(KeyError):
        only.weight
    with pytest.raises(ValueError):
        rb.ScatteredRays(np.zeros(8, np.uint8), 6)
    with pytest.raises(ValueError):
        rb.ScatteredRays(buf, n, shape=(2, 2))


@pytest.mark.parametrize("skip", [0, 2])
def test_pcg_streams_are_the_oracles_generators(oracle, skip):
    states = [0, 1, 2 ** 63, 2 ** 64 - 1] + [s for s, _, _ in seed_sweep.PAIRS.values()]
    seqs = [0, 1, 2 ** 63, 2 ** 64 - 1, 54] + [q for _, _, q in seed_sweep.PAIRS.values()] + [b for _, b, _ in seed_sweep.PAIRS.values() if b]
    seqs = [q % 2 ** 64 for q in seqs]
    for s in states:
        got = rb.pcg_streams(s, np.array(seqs, dtype=np.uint64), skip)
        assert got.dtype == np.uint64 and got.shape == (2, len(seqs))
        for j, q in enumerate(seqs):
            g = oracle.Pcg(s, q)
            for _ in range(skip):
                g.random()
            assert (int(got[0, j]), int(got[1, j])) == (g.state, g.inc), (s, q, skip)
    # consecutive sequences wrap at 2^64 as the device's sum does; Python ints and lists are taken as they are
    wrap = rb.pcg_streams(45, np.uint64(2 ** 64 - 2) + np.arange(4, dtype=np.uint64), skip)
    assert np.array_equal(wrap, rb.pcg_streams(45, [2 ** 64 - 2, 2 ** 64 - 1, 0, 1], skip))
    assert np.array_equal(rb.pcg_streams(2 ** 64 + 45, [54], skip), rb.pcg_streams(45, [54], skip))
    h = hm.PCG(45, 54)
    for _ in range(skip):
        h.random()
    assert tuple(int(x) for x in rb.pcg_streams(45, 54, skip)[:, 0]) == (h.state, h.inc)
    with pytest.raises(ValueError):
        rb.pcg_streams(45, [54], -1)


@pytest.mark.parametrize("name", X.WORLDS)
def test_the_batches_hold_every_case(oracle, name):
    """Both outcomes of the roulette in every world, both BRDF kinds where the GPU test compares both, the tiny world's four
    cases: asserted where the batch is built (scatter_batches.check), printed here."""
    b = X.batch(oracle, name)
    counts = X.check(name, b, X.world(name)[0])
    print(name, counts)
    plain, rr = b["want"][False], b["want"][True]
    dead = plain["status"] != 1
    assert np.array_equal(plain["rays"][:, dead], np.tile(X.DEAD_RAY[:, None], (1, int(dead.sum()))))
    live = ~dead
    assert np.all(plain["rays"][7, live] == np.inf) and set(np.unique(plain["rays"][6, live])) <= {1e-3, 1e-5}
    assert np.array_equal(plain["rays"][0:3, live].T, b["rec"].point[live])
    assert np.array_equal(plain["emitted"], rr["emitted"]) and np.isfinite(plain["rays"][:7]).all()


def test_the_aimed_draw_equals_q(oracle):
    """The one draw that separates ``draw > q`` from ``draw >= q``: 1.0 on a black pigment (tests/test_gpu_scatter.py aims it)."""
    g = oracle.Pcg()
    g.st[0], g.st[1] = X.state_drawing_one(), 109
    assert g.random_float() == 1.0
    h = hm.PCG()
    h.state, h.inc = X.state_drawing_one(), 109
    assert h.random() == 0xFFFFFFFF


# ---- PathTracerShader with every device answer replaced by the oracle's ------------------------------------------------------
class OracleQueries:
    """What ``PathTracerShader`` asks of ``WorldQueries``, answered record by record through the oracle."""

    def __init__(self, orc, flat):
        self.orc, self.flat = orc, flat
        self.calls = []

    def scatter(self, hits_, dirs, pcg, roulette=False, channels=rb.SCAT_ALL):
        if dirs is None:
            dirs = hits_.ray_dir
        shape = hits_.shape_index.shape
        n = int(np.prod(shape))

        class Flat:  # the records as a RayHits holds them
            pass

        rec = Flat()
        rec.n, rec.shape_index = n, np.asarray(hits_.shape_index).reshape(n)
        rec.hit = rec.shape_index >= 0
        rec.point, rec.normal, rec.uv = (np.asarray(getattr(hits_, k)).reshape(n, -1) for k in ("point", "normal", "uv"))
        want = X.expected(self.orc, self.flat, rec, np.asarray(dirs).reshape(n, 3), np.asarray(pcg), bool(roulette))
        out = rb.ScatteredRays(np.zeros(rb.scatter_bytes(n, rb.SCAT_ALL), np.uint8), n, rb.SCAT_ALL, shape=shape)
        out.status.reshape(n)[:] = want["status"]
        out.rays[:], out.pcg[:] = want["rays"], want["pcg"]
        out.weight.reshape(n, 3)[:], out.emitted.reshape(n, 3)[:] = want["weight"], want["emitted"]
        self.calls.append(("scatter", bool(roulette), int((want["status"] == 1).sum())))
        return out

    def ray_intersections(self, rays, dirs=None, channels=rb.RAY_CHANNELS, tmin=1e-5, tmax=float("inf")):
        self.calls.append(("trace", rays.shape[0]))
        return B.expected(self.orc, self.flat, np.ascontiguousarray(rays))


class OracleFrameTracer(GpuImageTracer):
    """A tracer whose hit-record frame and world queries come from the oracle (``_render_hit_frame`` is the route's seam)."""

    def __init__(self, orc, flat, cam, *args, **kw):
        super().__init__(*args, **kw)
        self.orc, self.flat, self.cam = orc, flat, cam
        self.queries = OracleQueries(orc, flat)

    def world_queries(self, world):
        return self.queries

    def _render_hit_frame(self, world, channels):
        p = self._hits_params()
        assert p.pcg_mode == abi.PCG_SAMPLE
        frame = hits.HitFrame(None, p, abi.HIT_ALL)
        W, H, S = frame.width, frame.rows, frame.samples_per_side
        frame.shape_index[:] = -1
        frame.t[:] = np.inf
        for row in range(H):
            for col in range(W):
                for k in range(frame.nsamp):
                    up = vp = 0.5
                    if S > 0:
                        g = self.orc.Pcg(p.path_state, (p.path_seq + (row * W + col) * frame.nsamp + k) % 2 ** 64)
                        up = (k % S + g.random_float()) / S
                        vp = (k // S + g.random_float()) / S
                    ray = self.orc.tracer_fire_ray(self.cam, W, H, col, row, up, vp)
                    frame.ray_origin[k, row, col], frame.ray_dir[k, row, col] = ray[0:3], ray[3:6]
                    r = self.orc.world_intersect(self.flat, ray)
                    if r is not None:
                        frame.shape_index[k, row, col] = int(r[9])
                        frame.t[k, row, col], frame.point[k, row, col], frame.normal[k, row, col], frame.uv[k, row, col] = r[0], r[1:4], r[4:7], r[7:9]
        return frame


@pytest.mark.parametrize("S_", [0, 2])
@pytest.mark.parametrize("max_depth,limit", [(3, 2), (0, 3)])
def test_the_shader_on_oracle_answers_is_the_oracles_path_tracer(oracle, max_depth, limit, S_):
    W, H = 24, 18
    world, camera = X.host_world("demo")
    camera = hm.PerspectiveCamera(camera.screen_distance, W / H, camera.transformation)
    flat, cam = flatten.flatten_world(world), flatten.flatten_camera(camera)
    bg = (0.25, 0.5, 0.125)
    seeds = (2 ** 40 + 45, 54)
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        par = abi.make_params(W, H, abi.RENDERER_PATHTRACER, samples_per_side=S_, num_of_rays=1, max_depth=max_depth, rr_limit=limit,
                              pcg_mode=abi.PCG_SAMPLE, path_state=seeds[0], path_seq=seeds[1], background=bg)
        want, n_rays = oracle.render(flat, cam, par, sqr_mode=oracle.SQR_MUL)
        tracer = OracleFrameTracer(oracle, flat, cam, hm.HdrImage(W, H), camera, samples_per_side=S_, pcg=hm.PCG(*seeds), pcg_mode="sample")
        shader = shaders.PathTracerShader(world, tracer, hm.Color(*bg), hm.PCG(*seeds), 1, max_depth, limit)
        tracer.fire_all_rays(shader)
        assert tracer.last_path == "device-hits"
        got = np.asarray(tracer.image.array)
        assert got.shape == want.shape == (H, W, 3) and len(np.unique(want.reshape(-1, 3), axis=0)) >= (9 if max_depth else 3)  # (max_depth 0: emitted, black and the background; deeper: bounces mix the materials)
        assert got.tobytes() == want.tobytes(), f"{int(np.any(got != want, axis=-1).sum())} of {W * H} pixels differ"
        calls = tracer.queries.calls
        scatters = [c for c in calls if c[0] == "scatter"]
        assert len(scatters) == max_depth + 1 and [c[1] for c in scatters] == [d >= limit for d in range(max_depth + 1)]
        assert sum(c[0] == "trace" for c in calls) == max_depth
        # the rays the oracle counted: the primary ones, and one per record that scattered above max_depth
        nsamp = max(S_, 1) ** 2
        assert n_rays == W * H * nsamp + sum(c[2] for c in scatters[:-1])
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def test_the_shaders_scalar_form_is_the_oracles_radiance(oracle):
    """``__call__(ray)``: the same recursion ray by ray, drawing from the shader's own generator, on a world that can intersect."""
    from .test_surface_host import OracleLightWorld

    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        b = X.records(oracle, "demo")
        flat = X.world("demo")[0]
        world = OracleLightWorld(X.host_world("demo")[0], oracle)
        bg = (0.25, 0.5, 0.125)
        par = abi.make_params(8, 8, abi.RENDERER_PATHTRACER, num_of_rays=1, max_depth=3, rr_limit=1, background=bg)
        picks = range(0, b["n_primary"], 7)
        differ = 0
        for i in picks:
            r = b["rays"][i]
            shader = shaders.PathTracerShader(world, None, hm.Color(*bg), hm.PCG(45, 54 + i), 1, 3, 1)
            c = shader(hits.HitRay(hm.Vec(*r[0:3]), hm.Vec(*r[3:6]), float(r[6]), float(r[7])))
            g = oracle.Pcg(45, 54 + i)
            want, _ = oracle.radiance(flat, par, g, r)
            assert (c.r, c.g, c.b) == tuple(want), i
            assert (shader.pcg.state, shader.pcg.inc) == (g.state, g.inc)
            differ += tuple(want) != bg
        assert differ > 20
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
    with pytest.raises(TypeError, match="parameter holder"):
        shaders.PathTracerShader(X.host_world("demo")[0])(hits.HitRay(hm.Vec(0, 0, 0), hm.Vec(1, 0, 0)))
    with pytest.raises(TypeError, match="tracer"):
        shaders.PathTracerShader(X.host_world("demo")[0]).shade_hits(None)


def test_the_shaders_three_refusals():
    world, camera = X.host_world("demo")

    def tracer(mode, S_):
        return GpuImageTracer(hm.HdrImage(8, 6), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode=mode)

    for n_rays in (0, 2, 10):
        with pytest.raises(ValueError, match=r"num_of_rays.*fire_all_rays\(PathTracer"):
            shaders.PathTracerShader(world, tracer("sample", 2), hm.BLACK, hm.PCG(45, 54), n_rays)
    for S_ in (0, 2):
        with pytest.raises(ValueError, match=r'pcg_mode="seq".*fire_all_rays\(PathTracer'):
            shaders.PathTracerShader(world, tracer("seq", S_), hm.BLACK, hm.PCG(45, 54))
    with pytest.raises(ValueError, match=r'pcg_mode="pixel" with 4 samples.*fire_all_rays\(PathTracer'):
        shaders.PathTracerShader(world, tracer("pixel", 2), hm.BLACK, hm.PCG(45, 54))
    # ... and a tracer that changes its mind behind the constructor is caught when the frame is shaded
    t = tracer("sample", 2)
    shader = shaders.PathTracerShader(world, t, hm.BLACK, hm.PCG(45, 54))
    t.pcg_mode = "seq"
    with pytest.raises(ValueError, match="seq"):
        shader.shade_hits(None)
    # what is not refused: a generator per sample, or modes that coincide with it (one sample per pixel)
    for mode, S_ in (("sample", 0), ("sample", 3), ("pixel", 0), ("pixel", 1), ("auto", 0)):
        shaders.PathTracerShader(world, tracer(mode, S_), hm.BLACK, hm.PCG(45, 54))
