"""CPU-only tests of the radiance queries (include/ptrace_radiance.h, libptrace_radiance.so, pytracer_amd.rays / .shaders): the
fifth library builds and loads without a GPU and leaves the other four as they were; its header, the ctypes table and its dynamic
symbols agree; sizes and offsets match their Python mirrors; bad arguments are refused before any HIP call; and
``PathRadianceShader.__call__`` -- the recursion in Python floats, with the loop over ``num_of_rays`` -- is the oracle's
``PathTracer``, which pins the order of the draws and of the additions without a GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi, hits, rays as rb, shaders
from pytracer_amd import hostmodel as hm
from pytracer_amd.tracer import GpuImageTracer

from . import radiance_batches as R
from . import scatter_batches as X
from . import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE = -1, -3, -5  # include/ptrace.h
V13 = (1 << 16) | 3
SIZES = [0, 1, 63, 65, 2 ** 31 - 1]


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _radiance_lib, build

    build.build()
    assert os.path.exists(build.RADIANCE_LIB) and not build.needs_build()
    return _radiance_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _radiance_lib, _rays_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_radiance.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_radiance_lib.EXPORTS) and len(declared) == 8
    assert _exported(_radiance_lib.lib_path()) == declared
    # an add-on like the other three: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _radiance_lib.lib_path()], capture_output=True, text=True).stdout
    assert "libptrace" not in needed.replace("libptrace_radiance.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _radiance_lib.lib_path()], capture_output=True, text=True).stdout
    assert not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    assert lib.pt_rays_radiance_version() == V13
    assert lib.pt_rays_radiance_args_bytes() == _rays_lib.lib().pt_rays_args_bytes() > 0
    # the only file that includes the new device header is the new translation unit, and the recipe watches the public header
    users = [f for f in os.listdir(build.CSRC) if '"pt_radiance.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_radiance.hip"]
    assert os.path.normpath(os.path.join("..", "..", "include", "ptrace_radiance.h")) in {os.path.normpath(d) for d in build.DEPS}
    assert C.sizeof(_radiance_lib.RadianceParams) == 40  # four ints and three doubles: pt_radiance_params


def test_the_other_four_libraries_are_what_they_were(lib):
    from pytracer_amd import _lib, _rays_lib, _scatter_lib, _surface_lib, build

    assert _exported(_rays_lib.lib_path()) == set(_rays_lib.EXPORTS) and len(_rays_lib.EXPORTS) == 7
    assert _exported(_surface_lib.lib_path()) == set(_surface_lib.EXPORTS) and len(_surface_lib.EXPORTS) == 11
    assert _exported(_scatter_lib.lib_path()) == set(_scatter_lib.EXPORTS) and len(_scatter_lib.EXPORTS) == 7
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert build.code_hash() == json.load(open(os.path.join(ROOT, "profiles", "pmc_c2.json")))["code_hash"]
    for header in ("ptrace_rays.h", "ptrace_surface.h", "ptrace_scatter.h"):
        assert "pt_rays_radiance" not in open(os.path.join(ROOT, "include", header)).read()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_offsets_match_the_python_mirror(lib, n):
    for channels in range(4):
        planes = 3 + (2 if channels & rb.RAD_PCG else 0) + (1 if channels & rb.RAD_COUNT else 0)
        assert lib.pt_rays_radiance_bytes(n, channels) == rb.radiance_bytes(n, channels) == 8 * n * planes
        want = {(0, c): 8 * n * c for c in range(3)}
        if channels & rb.RAD_PCG:
            want.update({(rb.RAD_PCG, 0): 24 * n, (rb.RAD_PCG, 1): 32 * n})
        if channels & rb.RAD_COUNT:
            want[(rb.RAD_COUNT, 0)] = 8 * n * (planes - 1)
        for sel in (0, rb.RAD_PCG, rb.RAD_COUNT, 3, 4, -1):
            for comp in (-1, 0, 1, 2, 3):
                got, mirror = lib.pt_rays_radiance_plane_offset(n, channels, sel, comp), rb.radiance_plane_offset(n, channels, sel, comp)
                if (sel, comp) in want:
                    assert got == mirror == want[(sel, comp)], (n, channels, sel, comp)
                else:
                    assert got == ERR_INVALID and mirror == -1, (n, channels, sel, comp)
    for bad in (4, 7, -1, 1 << 20):
        assert lib.pt_rays_radiance_bytes(n, bad) == 0 and rb.radiance_bytes(n, bad) == 0
        assert lib.pt_rays_radiance_plane_offset(n, bad, 0, 0) == ERR_INVALID and rb.radiance_plane_offset(n, bad, 0, 0) == -1
    for bad_n in (-1, 2 ** 31):
        assert lib.pt_rays_radiance_bytes(bad_n, 3) == 0 and rb.radiance_bytes(bad_n, 3) == 0
        assert lib.pt_rays_radiance_plane_offset(bad_n, 3, 0, 0) == ERR_INVALID and rb.radiance_plane_offset(bad_n, 3, 0, 0) == -1


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """No GPU here: whatever is refused with PT_ERR_INVALID / UNSUPPORTED / SIZE was refused by the argument checks (the first HIP
    call would answer PT_ERR_NODEVICE)."""
    from pytracer_amd import _radiance_lib

    nb = int(lib.pt_rays_radiance_args_bytes())
    block = (C.c_char * nb)()
    np.frombuffer(block, dtype=np.uint8)[:] = 1  # (a block whose `cold` pointer is set and whose shape count is positive)
    n = 5
    rays, gen = np.zeros((8, n)), np.zeros((2, n), np.uint64)
    out = np.zeros(rb.radiance_bytes(n, 3), np.uint8)
    ws = np.zeros(64, np.uint8)

    def call(device=0, blk=block, nbytes=nb, r=rays, st=gen[0], inc=gen[1], count=n, N=1, D=3, limit=2, depth=0, ch=3, o=out, ob=None,
             null_par=False):
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        par = None if null_par else C.byref(_radiance_lib.params(N, D, limit, depth, (0, 0, 0)))
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        host = lib.pt_rays_radiance(device, blk, nbytes, p(r), p(st), p(inc), count, par, ch, p(o), ob)
        dev = lib.pt_rays_radiance_device(device, blk, nbytes, None, p(r), p(st), p(inc), count, par, ch, p(ws), ws.nbytes, p(o), ob, None)
        return host, dev

    both = lambda code: (code, code)  # noqa: E731
    assert call(N=0) == both(ERR_INVALID) and "num_of_rays" in _radiance_lib.last_error()
    assert call(D=-1) == both(ERR_INVALID)
    assert call(depth=-1) == both(ERR_INVALID) and "depth" in _radiance_lib.last_error()
    assert call(D=65) == both(ERR_UNSUPPORTED) and "fused renderer" in _radiance_lib.last_error() and "4096" in _radiance_lib.last_error()
    assert call(D=2 ** 31 - 1, depth=2 ** 31 - 66) == both(ERR_UNSUPPORTED)
    assert call(D=2 ** 31 - 1, depth=2 ** 31 - 65)[0] not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # 64 levels: accepted
    assert call(D=3, depth=7)[0] not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # deeper than max_depth: legal (black)
    assert call(count=-1) == both(ERR_INVALID) and call(count=2 ** 31) == both(ERR_INVALID)
    assert call(ch=4) == both(ERR_INVALID) and call(ch=-1) == both(ERR_INVALID)
    assert call(device=-1) == both(ERR_INVALID)
    assert call(blk=None) == both(ERR_INVALID)
    assert call(nbytes=nb - 8) == both(ERR_INVALID) and "one build" in _radiance_lib.last_error()
    assert call(nbytes=nb + 8) == both(ERR_INVALID)
    assert call(null_par=True) == both(ERR_INVALID)
    for missing in ("r", "st", "inc", "o"):
        assert call(**{missing: None}, ob=out.nbytes) == both(ERR_INVALID), missing
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "too small" in _radiance_lib.last_error()
    assert call(ob=rb.radiance_bytes(n, 1), ch=3) == both(ERR_SIZE) and call(ob=rb.radiance_bytes(n, 1), ch=1)[0] != ERR_SIZE
    # n = 0: PT_OK with nothing launched (no device is touched), null planes allowed
    assert call(count=0, r=None, st=None, inc=None, o=None) == both(0)
    # the workspace's size: 0 on refusal, with the reason
    assert lib.pt_rays_radiance_workspace_bytes(0, 10, 1, 65, 0) == 0 and "fused renderer" in _radiance_lib.last_error()
    assert lib.pt_rays_radiance_workspace_bytes(0, 10, 0, 3, 0) == 0 and lib.pt_rays_radiance_workspace_bytes(-1, 10, 1, 3, 0) == 0
    assert lib.pt_rays_radiance_workspace_bytes(0, -1, 1, 3, 0) == 0


def test_channel_names_and_the_views():
    assert rb.radiance_channels("all") == 3 and rb.radiance_channels("none") == 0 and rb.radiance_channels("count") == rb.RAD_COUNT
    assert rb.radiance_channels("count, pcg") == 3 and rb.radiance_channels(1) == rb.RAD_PCG
    for bad in ("weight", 4, -1):
        with pytest.raises(ValueError):
            rb.radiance_channels(bad)
    n = 6
    buf = np.zeros(rb.radiance_bytes(n, 3), np.uint8)
    buf.view(np.float64)[: 3 * n] = np.arange(3 * n)
    buf.view(np.uint64)[3 * n:] = np.arange(100, 100 + 3 * n)
    res = rb.RayRadiance(buf, n, "all", shape=(1, 2, 3))
    assert res.radiance.shape == (1, 2, 3, 3) and np.array_equal(res.radiance[0, 1, 2], [5.0, 11.0, 17.0])
    assert res.pcg.shape == (2, n) and res.pcg_state[0, 0, 1] == 101 and res.pcg_inc[0, 1, 2] == 111 and res.n_rays[0, 1, 0] == 115
    assert np.shares_memory(res.radiance, buf) and np.shares_memory(res.n_rays, buf) and set(res.planes()) == {"radiance", "pcg_state", "pcg_inc", "n_rays"}
    only = rb.RayRadiance(np.zeros(rb.radiance_bytes(n, 2), np.uint8), n, "count")
    only.buffer.view(np.uint64)[3 * n:] = 7
    assert np.all(only.n_rays == 7) and not only.has("pcg") and set(only.planes()) == {"radiance", "n_rays"}
    with pytest.raises(KeyError, match="pcg"):
        only.pcg
    with pytest.raises(ValueError):
        rb.RayRadiance(np.zeros(8, np.uint8), n)
    with pytest.raises(ValueError):
        rb.RayRadiance(buf, n, shape=(2, 2))


# ---- PathRadianceShader.__call__ against the oracle ------------------------------------------------------------------------------
class _SpyWorld:
    """``OracleLightWorld`` that notes whether a diffuse bounce was traced (``DiffuseBRDF.scatter_ray``'s rays start at 1e-3)."""

    def __init__(self, inner):
        self.inner, self.shapes, self.diffuse = inner, inner.shapes, False

    def ray_intersection(self, ray):
        self.diffuse |= ray.tmin == 1.0e-3 and getattr(ray, "depth", 0) > 0
        return self.inner.ray_intersection(ray)


@pytest.mark.parametrize("num_of_rays,max_depth,limit", [(1, 3, 1), (2, 2, 1), (3, 3, 0)])
def test_the_shaders_scalar_form_is_the_oracles_radiance(oracle, num_of_rays, max_depth, limit):
    from .test_surface_host import OracleLightWorld

    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        b = X.records(oracle, "demo")
        flat = X.world("demo")[0]
        inner = OracleLightWorld(X.host_world("demo")[0], oracle)
        bg = R.BACKGROUND
        par = R.params(num_of_rays, max_depth, limit, bg)
        picks = range(0, b["n_primary"], 30)
        assert len(picks) == 40
        exact = bounced = differ = 0
        for i in picks:
            r = b["rays"][i]
            world = _SpyWorld(inner)
            shader = shaders.PathRadianceShader(world, None, hm.Color(*bg), hm.PCG(45, 54 + i), num_of_rays, max_depth, limit)
            c = shader(hits.HitRay(hm.Vec(*r[0:3]), hm.Vec(*r[3:6]), float(r[6]), float(r[7])))
            g = oracle.Pcg(45, 54 + i)
            want, _ = oracle.radiance(flat, par, g, r)
            if not world.diffuse:
                assert (c.r, c.g, c.b) == tuple(want), i
                assert (shader.pcg.state, shader.pcg.inc) == (g.state, g.inc), i
                exact += 1
            else:  # glibc's sin / cos on both sides
                assert np.all(util.rel_err([c.r, c.g, c.b], want) <= 1e-12), (i, (c.r, c.g, c.b), tuple(want))
                bounced += 1
            differ += tuple(want) != bg
        print(f"N={num_of_rays} D={max_depth} limit={limit}: {exact} rays without a diffuse bounce, {bounced} with one")
        assert differ > 10 and exact > 5 and bounced > 5
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


@pytest.mark.parametrize("num_of_rays", [1, 3, 10])
def test_a_hit_at_max_depth_consumes_its_scatter_draws(oracle, num_of_rays):
    """``max_depth = 0``: the primary hit's children are beyond ``max_depth`` -- black without a query -- but ``scatter_ray`` ran for
    each of them: ``2 * num_of_rays`` draws on a diffuse hit with ``lum > 0``, none on a mirror, none on a miss."""
    from .test_surface_host import OracleLightWorld

    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        b = X.records(oracle, "demo")
        flat = X.world("demo")[0]
        world = OracleLightWorld(X.host_world("demo")[0], oracle)
        par = R.params(num_of_rays, 0, 3)
        rec = b["rec"]
        seen = set()
        for i in range(0, b["n_primary"], 23):
            r = b["rays"][i]
            shader = shaders.PathRadianceShader(world, None, hm.Color(*R.BACKGROUND), hm.PCG(45, 54 + i), num_of_rays, 0, 3)
            c = shader(hits.HitRay(hm.Vec(*r[0:3]), hm.Vec(*r[3:6]), float(r[6]), float(r[7])))
            g = oracle.Pcg(45, 54 + i)
            want, n_rays = oracle.radiance(flat, par, g, r)
            assert (c.r, c.g, c.b) == tuple(want) and n_rays == 1 and (shader.pcg.state, shader.pcg.inc) == (g.state, g.inc)
            start = hm.PCG(45, 54 + i)
            draws = 0
            if rec.hit[i]:
                s = int(rec.shape_index[i])
                lum = float(np.max(oracle.pigment(flat, s, False, float(rec.uv[i, 0]), float(rec.uv[i, 1]))))
                if lum > 0.0 and int(flat.brdf_kind[s]) == abi.BRDF_DIFFUSE:
                    draws = 2 * num_of_rays
            assert shader.pcg.state == hm.pcg_advance(start.state, start.inc, draws), (i, draws)
            seen.add(draws)
        assert seen == {0, 2 * num_of_rays}
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def test_the_shaders_refusals_and_what_it_accepts():
    world, camera = X.host_world("demo")

    def tracer(mode, S_):
        return GpuImageTracer(hm.HdrImage(8, 6), camera, samples_per_side=S_, pcg=hm.PCG(45, 54), pcg_mode=mode)

    for n_rays in (1, 2, 10):
        sh = shaders.PathRadianceShader(world, tracer("sample", 2), hm.BLACK, hm.PCG(45, 54), n_rays)
        assert sh.num_of_rays == n_rays and sh.hit_channels == abi.HIT_RAY
    with pytest.raises(ValueError, match="num_of_rays"):
        shaders.PathRadianceShader(world, None, hm.BLACK, hm.PCG(45, 54), 0)
    for S_ in (0, 2):
        with pytest.raises(ValueError, match=r'PathRadianceShader needs a generator per sample, not pcg_mode="seq".*fire_all_rays\(PathTracer'):
            shaders.PathRadianceShader(world, tracer("seq", S_), hm.BLACK, hm.PCG(45, 54), 2)
    with pytest.raises(ValueError, match=r'pcg_mode="auto"'):
        shaders.PathRadianceShader(world, tracer("auto", 2), hm.BLACK, hm.PCG(45, 54), 2)
    with pytest.raises(ValueError, match=r'pcg_mode="pixel" with 4 samples.*share one stream in program order'):
        shaders.PathRadianceShader(world, tracer("pixel", 2), hm.BLACK, hm.PCG(45, 54), 2)
    for mode, S_ in (("pixel", 0), ("pixel", 1), ("auto", 0), ("sample", 3)):
        shaders.PathRadianceShader(world, tracer(mode, S_), hm.BLACK, hm.PCG(45, 54), 10)
    # the wording is PathTracerShader's, word for word behind the class name
    for mode, S_ in (("seq", 0), ("pixel", 2)):
        with pytest.raises(ValueError) as mine:
            shaders.PathRadianceShader(world, tracer(mode, S_), hm.BLACK, hm.PCG(45, 54), 1)
        with pytest.raises(ValueError) as theirs:
            shaders.PathTracerShader(world, tracer(mode, S_), hm.BLACK, hm.PCG(45, 54), 1)
        assert str(mine.value) == str(theirs.value).replace("PathTracerShader", "PathRadianceShader")
    with pytest.raises(TypeError, match="parameter holder"):
        shaders.PathRadianceShader(world)(hits.HitRay(hm.Vec(0, 0, 0), hm.Vec(1, 0, 0)))
    with pytest.raises(TypeError, match="tracer"):
        shaders.PathRadianceShader(world).shade_hits(None)


def test_sample_streams_is_one_function_for_both_shaders():
    world, camera = X.host_world("demo")
    par = abi.make_params(8, 6, abi.RENDERER_PATHTRACER, samples_per_side=2, pcg_mode=abi.PCG_SAMPLE)
    frame = hits.HitFrame(None, par, abi.HIT_RAY)
    old = shaders.PathTracerShader(world, None, hm.BLACK, hm.PCG(2 ** 40 + 45, 54), 1)
    got = shaders.sample_streams(hm.PCG(2 ** 40 + 45, 54), frame)
    assert got.shape == (2, 4 * 48) and np.array_equal(got, old.sample_streams(frame))
    # [nsamp, rows, W] flattened: entry 48 + 5 is sample 1 of pixel 5 -- PCG(S0, Q0 + 5 * 4 + 1), behind its two jitter draws
    assert np.array_equal(got[:, 48 + 5], rb.pcg_streams(2 ** 40 + 45, [54 + 5 * 4 + 1], 2)[:, 0])


def test_the_radiance_command_checks_its_arguments(tmp_path):
    from click.testing import CliRunner

    from pytracer_amd.cli import cli

    run = CliRunner().invoke
    np.save(tmp_path / "bad.npy", np.zeros((4, 7)))
    np.save(tmp_path / "ok.npy", np.zeros((4, 8)))
    r = run(cli, ["radiance", "--input", str(tmp_path / "bad.npy")])
    assert r.exit_code == 2 and "[n, 8]" in r.output
    r = run(cli, ["radiance", "--input", str(tmp_path / "ok.npy"), "--max-depth", "70"])
    assert r.exit_code == 2 and "64 levels" in r.output
    r = run(cli, ["radiance", "--input", str(tmp_path / "ok.npy"), "--num-of-rays", "0"])
    assert r.exit_code == 2
    r = run(cli, ["radiance", "--input", str(tmp_path / "missing.npy")])
    assert r.exit_code == 2
