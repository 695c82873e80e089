"""CPU-only tests of the bake queries (include/ptrace_bake.h, libptrace_bake.so, pytracer_amd.rays / scenes): the seventh library
builds and loads without a GPU and leaves the other six as they were; its header, the ctypes table and its dynamic symbols agree;
sizes and offsets match their Python mirrors up to 2^31 - 1 texels; every refusal of the interface happens before any HIP call;
its translation unit carries no copy of the shared host layer; ``baked_world`` flattens with its maps in ``ImagePigment``'s order;
and the expected maps DEPEND on the order of the sum, so a wrong order cannot pass the GPU's bit tests."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi, rays as rb

from . import bake_maps as M
from . import gather_batches as G
from . import radiance_batches as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE = -1, -3, -5  # include/ptrace.h
V15 = (1 << 16) | 5
SIZES = [0, 1, 63, 65, 2 ** 31 - 1]


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _bake_lib, build

    build.build()
    assert os.path.exists(build.BAKE_LIB) and not build.needs_build()
    return _bake_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _bake_lib, _rays_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_bake.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_bake_lib.EXPORTS) == {s for s, _, _ in _bake_lib._SIGNATURES} and len(declared) == 11
    assert _exported(_bake_lib.lib_path()) == declared
    # an add-on like the other five: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _bake_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_bake.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _bake_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    assert lib.pt_rays_bake_version() == V15
    assert lib.pt_rays_bake_args_bytes() == _rays_lib.lib().pt_rays_args_bytes() > 0
    # the only file that includes the new device header is the new translation unit, which keeps away from the other walks'
    # headers; the recipe builds the library with the add-ons' flags and watches its sources and its public header
    users = [f for f in os.listdir(build.CSRC) if '"pt_bake.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_bake.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_bake.hip")).read() + open(os.path.join(build.CSRC, "pt_bake.h")).read()
    assert '"pt_radiance.h"' not in text and '"pt_gather.h"' not in text
    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_bake.h")), "ptrace_bake.hip", "pt_bake.h"} <= deps
    assert (build.BAKE_FLAGS, build.BAKE_LIB, build.BAKE_SOURCES) == build.ALL_TARGETS[-1] and len(build.ALL_TARGETS) == 7
    assert build.ALL_TARGETS[:6] == build.TARGETS
    assert build.BAKE_FLAGS[:-1] == build.FLAGS[:-1] and build.BAKE_FLAGS[-1] == "-cuid=libptrace_bake"
    assert C.sizeof(_bake_lib.BakeParams) == 96  # fourteen ints, two uint64 and three doubles: pt_bake_params
    # the header states its definitions with their citations
    for cite in ("shapes.py:36-42", "shapes.py:183-185", "transformations.py:58-96", "world.py:66-67", "imagetracer.py:48-58",
                 "materials.py:132-152", "render.py:99-139"):
        assert cite in header, cite


def test_the_other_six_libraries_are_what_they_were(lib):
    from pytracer_amd import _gather_lib, _lib, _radiance_lib, _rays_lib, _scatter_lib, _surface_lib, build

    for module, count in ((_rays_lib, 7), (_surface_lib, 11), (_scatter_lib, 7), (_radiance_lib, 8), (_gather_lib, 8)):
        assert _exported(module.lib_path()) == set(module.EXPORTS) and len(module.EXPORTS) == count
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert build.code_hash() == json.load(open(os.path.join(ROOT, "profiles", "pmc_c2.json")))["code_hash"]
    for header in ("ptrace.h", "ptrace_rays.h", "ptrace_surface.h", "ptrace_scatter.h", "ptrace_radiance.h", "ptrace_gather.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "pt_rays_bake" not in text and "pt_rays_surface_points" not in text
    # the recorded hashes: six rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "bake_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows[:6]] == [os.path.basename(t[1]) for t in build.TARGETS] and all(r[1] == r[2] for r in rows[:6])
    assert [r[2] for r in rows[:6]] == [build.code_hash(t[1]) for t in build.TARGETS]


def test_the_translation_unit_carries_no_copy_of_the_host_layer():
    """tests/test_addon_common.py's checks, for ``bake``."""
    text = open(os.path.join(ROOT, "pytracer_amd", "csrc", "ptrace_bake.hip")).read()
    assert '#include "pt_host_common.h"' in text
    for what in (r"\bg_err\b", r"\bint\s+device_ok\s*\(", r"\bstruct\s+Staged\b", r"\bint\s+fail\s*\(", r"#\s*define\s+HIP_TRY\b",
                 r"\bup8\s*\(size_t", r"\bdim3\s+grid_of\s*\(", r"getenv\s*\(", r"this library's has %zu"):
        assert not re.search(what, text), what
    from pytracer_amd import _bake_lib

    assert _bake_lib.lib_path() == os.environ.get("PTRACE_BAKE_LIB") or _bake_lib.lib_path() == os.path.join(ROOT, "pytracer_amd", "libptrace_bake.so")


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_offsets_match_the_python_mirror(lib, n):
    assert lib.pt_rays_points_bytes(n) == 48 * n
    for channels in range(2):
        planes = 3 + (1 if channels & rb.BAKE_COUNT else 0)
        assert lib.pt_rays_bake_bytes(n, channels) == rb.bake_bytes(n, channels) == 8 * n * planes
        want = {(0, c): 8 * n * c for c in range(3)}
        if channels & rb.BAKE_COUNT:
            want[(rb.BAKE_COUNT, 0)] = 24 * n
        for sel in (0, rb.BAKE_COUNT, 2, 3, -1):
            for comp in (-1, 0, 1, 2, 3):
                got, mirror = lib.pt_rays_bake_plane_offset(n, channels, sel, comp), rb.bake_plane_offset(n, channels, sel, comp)
                if (sel, comp) in want:
                    assert got == mirror == want[(sel, comp)], (n, channels, sel, comp)
                else:
                    assert got == ERR_INVALID and mirror == -1, (n, channels, sel, comp)
    for bad in (2, 3, -1, 1 << 20):
        assert lib.pt_rays_bake_bytes(n, bad) == 0 and rb.bake_bytes(n, bad) == 0
        assert lib.pt_rays_bake_plane_offset(n, bad, 0, 0) == ERR_INVALID and rb.bake_plane_offset(n, bad, 0, 0) == -1
    for bad_n in (-1, 2 ** 31):
        assert lib.pt_rays_points_bytes(bad_n) == 0
        assert lib.pt_rays_bake_bytes(bad_n, 1) == 0 and rb.bake_bytes(bad_n, 1) == 0
        assert lib.pt_rays_bake_plane_offset(bad_n, 1, 0, 0) == ERR_INVALID and rb.bake_plane_offset(bad_n, 1, 0, 0) == -1


ONES = 0x01010101  # what a block of bytes 1 holds in every int: its shape count


def _block(lib):
    """A scene argument block whose ``cold`` pointer is set and whose shape count is positive (``ONES``).  Nothing dereferences
    it: every call below ends before its first HIP call, or at it -- there is no device here."""
    nb = int(lib.pt_rays_bake_args_bytes())
    block = (C.c_char * nb)()
    np.frombuffer(block, dtype=np.uint8)[:] = 1
    return block, nb


def test_every_refusal_happens_before_any_hip_call(lib):
    """No GPU here: whatever is refused with PT_ERR_INVALID / UNSUPPORTED / SIZE was refused by the argument checks (the first HIP
    call would answer PT_ERR_NODEVICE)."""
    from pytracer_amd import _bake_lib

    block, nb = _block(lib)
    out = np.zeros(rb.bake_bytes(35, 1), np.uint8)
    ws = np.zeros(7 * 5 * 3 * 32, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731

    def call(device=0, blk=block, nbytes=nb, shape=1, side=1, W=7, H=5, window=None, jitter=True, K=3, N=1, D=3, limit=2, depth=1, ch=1,
             o=out, ob=None, wsb=ws, wb=None, null_par=False):
        par = None if null_par else C.byref(_bake_lib.params(shape, side, W, H, window, jitter, K, N, D, limit, depth, 42, 54, (0, 0, 0)))
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        host = lib.pt_rays_bake(device, blk, nbytes, par, ch, p(o), ob)
        dev = lib.pt_rays_bake_device(device, blk, nbytes, par, ch, p(wsb), (wsb.nbytes if wsb is not None else 0) if wb is None else wb, p(o), ob,
                                      None)
        return host, dev

    both = lambda code: (code, code)  # noqa: E731
    passed = lambda rc: rc not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # noqa: E731  (got as far as the first HIP call)
    assert all(passed(rc) for rc in call())
    # an unknown side
    for side in (0, 2, -2):
        assert call(side=side) == both(ERR_INVALID) and "side" in _bake_lib.last_error()
    assert all(passed(rc) for rc in call(side=-1))
    # W, H, K, num_of_rays < 1
    for kw, word in ((dict(W=0, window=(0, 0, 1, 1)), "W and H"), (dict(H=-1, window=(0, 0, 1, 1)), "W and H"), (dict(K=0), "samples"),
                     (dict(K=-3), "samples"), (dict(N=0), "num_of_rays")):
        assert call(**kw) == both(ERR_INVALID) and word in _bake_lib.last_error(), kw
    # a rectangle outside the map
    for window in ((0, 0, 8, 5), (0, 0, 7, 6), (1, 0, 7, 5), (0, 1, 7, 5), (-1, 0, 3, 3), (0, -1, 3, 3), (0, 0, 0, 5), (0, 0, 7, 0),
                   (7, 0, 1, 1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)):
        assert call(window=window) == both(ERR_INVALID) and "rectangle" in _bake_lib.last_error(), window
    assert all(passed(rc) for rc in call(window=(6, 4, 1, 1)))
    # a shape out of range (the block says ONES shapes)
    for shape in (-1, ONES, 2 ** 31 - 1):
        assert call(shape=shape) == both(ERR_INVALID) and f"{ONES} shapes" in _bake_lib.last_error(), shape
    assert all(passed(rc) for rc in call(shape=ONES - 1))
    # w * h * K beyond 2^31 - 1
    big = dict(W=2 ** 16, H=2 ** 15, o=out, ob=2 ** 40)
    assert call(K=1, **big) == both(ERR_INVALID) and "2^31 - 1" in _bake_lib.last_error()  # 2^31 texels
    assert call(W=46341, H=46341, K=1, ob=2 ** 40) == both(ERR_INVALID)  # 46341^2 = 2^31 + 4073
    assert call(W=3, H=1, K=715827883, ob=2 ** 40) == both(ERR_INVALID)  # 3 * 715827883 = 2^31 + 1
    assert call(W=2 ** 31 - 1, H=2 ** 31 - 1, K=2 ** 31 - 1, ob=2 ** 40) == both(ERR_INVALID)
    # depths
    assert call(D=-1) == both(ERR_INVALID) and call(depth=-1) == both(ERR_INVALID) and "depth" in _bake_lib.last_error()
    assert call(D=66, depth=1) == both(ERR_UNSUPPORTED) and "64 levels" in _bake_lib.last_error()
    assert call(D=2 ** 31 - 1, depth=2 ** 31 - 66) == both(ERR_UNSUPPORTED)
    assert all(passed(rc) for rc in call(D=65, depth=1))  # 64 levels: accepted
    assert all(passed(rc) for rc in call(D=3, depth=7))  # deeper than max_depth: legal (black)
    # channels, device, block, params
    assert call(ch=2) == both(ERR_INVALID) and call(ch=3) == both(ERR_INVALID) and call(ch=-1) == both(ERR_INVALID)
    assert call(device=-1) == both(ERR_INVALID)
    assert call(blk=None) == both(ERR_INVALID)
    assert call(nbytes=nb - 8) == both(ERR_INVALID) and "one build" in _bake_lib.last_error()
    assert call(null_par=True) == both(ERR_INVALID)
    assert call(o=None, ob=out.nbytes) == both(ERR_INVALID)
    # a short buffer or workspace
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "too small" in _bake_lib.last_error()
    assert call(ob=rb.bake_bytes(35, 0), ch=1) == both(ERR_SIZE) and all(passed(rc) for rc in call(ob=rb.bake_bytes(35, 0), ch=0))
    assert call(wb=35 * 3 * 32 - 1)[1] == ERR_SIZE and "workspace" in _bake_lib.last_error() and passed(call(wb=35 * 3 * 32)[1])
    assert call(wsb=None)[1] == ERR_INVALID and "workspace" in _bake_lib.last_error()
    assert not out.any()
    # the workspace's size: 0 on refusal, with the reason
    size = lambda **kw: lib.pt_rays_bake_workspace_bytes(kw.pop("device", 0), C.byref(_bake_lib.params(  # noqa: E731
        0, kw.pop("side", 1), kw.pop("W", 7), kw.pop("H", 5), kw.pop("window", None), True, kw.pop("K", 3), kw.pop("N", 1), kw.pop("D", 3), 2,
        kw.pop("depth", 1), 42, 54, (0, 0, 0))))
    assert size(D=66) == 0 and "64 levels" in _bake_lib.last_error()
    assert size(K=0) == 0 and size(N=0) == 0 and size(side=0) == 0 and size(window=(0, 0, 8, 5)) == 0 and size(device=-1) == 0
    assert size(W=2 ** 16, H=2 ** 15, K=1) == 0 and lib.pt_rays_bake_workspace_bytes(0, None) == 0


def test_surface_point_refusals_happen_before_any_hip_call(lib):
    from pytracer_amd import _bake_lib

    block, nb = _block(lib)
    n = 5
    shape, uv, side, out = np.zeros(n, np.int32), np.zeros((2, n)), np.ones(n, np.int32), np.zeros((6, n))
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731

    def call(device=0, blk=block, nbytes=nb, s=shape, u=uv, sd=side, count=n, o=out, ob=None):
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        return (lib.pt_rays_surface_points(device, blk, nbytes, p(s), p(u), p(sd), count, p(o), ob),
                lib.pt_rays_surface_points_device(device, blk, nbytes, p(s), p(u), p(sd), count, p(o), ob, None))

    both = lambda code: (code, code)  # noqa: E731
    passed = lambda rc: rc not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # noqa: E731
    assert all(passed(rc) for rc in call()) and all(passed(rc) for rc in call(sd=None))  # side NULL: +1
    assert call(count=-1) == both(ERR_INVALID) and call(count=2 ** 31) == both(ERR_INVALID)
    assert call(device=-1) == both(ERR_INVALID) and call(blk=None) == both(ERR_INVALID) and call(nbytes=nb + 8) == both(ERR_INVALID)
    for missing in ("s", "u", "o"):
        assert call(**{missing: None}, ob=out.nbytes) == both(ERR_INVALID), missing
    assert call(ob=48 * n - 1) == both(ERR_SIZE) and "too small" in _bake_lib.last_error()
    assert call(count=0, s=None, u=None, sd=None, o=None) == both(0)  # n = 0: PT_OK, nothing launched
    assert not out.any()


def test_channel_names_the_views_and_the_parameter_block():
    from pytracer_amd import _bake_lib

    assert rb.bake_channels("all") == 1 and rb.bake_channels("none") == 0 and rb.bake_channels("count") == rb.BAKE_COUNT
    with pytest.raises(ValueError) as e:
        rb.bake_channels("count, bogus,all")
    assert str(e.value) == "a bake batch has the channel count; not bogus, all"
    with pytest.raises(ValueError) as e:
        rb.bake_channels(2)
    assert str(e.value) == "a bake batch has the channel count (1); not 0x2"
    w, h = 3, 2
    buf = np.zeros(rb.bake_bytes(w * h, 1), np.uint8)
    buf.view(np.float64)[: 3 * w * h] = np.arange(3 * w * h)
    buf.view(np.uint64)[3 * w * h:] = np.arange(100, 100 + w * h)
    res = rb.BakedMap(buf, w, h, "all")
    assert res.radiance.shape == (2, 3, 3) and np.array_equal(res.radiance[1, 2], [5.0, 11.0, 17.0])  # texel (row 1, col 2) = index 5
    assert res.n_rays.shape == (2, 3) and res.n_rays[1, 0] == 103
    assert np.shares_memory(res.radiance, buf) and np.shares_memory(res.n_rays, buf) and set(res.planes()) == {"radiance", "n_rays"}
    only = rb.BakedMap(np.zeros(rb.bake_bytes(w * h, 0), np.uint8), w, h, "none")
    assert not only.has("count") and set(only.planes()) == {"radiance"}
    with pytest.raises(KeyError, match="count"):
        only.n_rays
    with pytest.raises(ValueError):
        rb.BakedMap(np.zeros(8, np.uint8), w, h)
    par = _bake_lib.params(2, -1, 7, 5, None, True, 3, 1, 10, 3, 1, -1, 2 ** 64 + 5, (0.5, 0.25, 1))
    assert (par.shape, par.side, par.W, par.H, par.col0, par.row0, par.w, par.h, par.jitter) == (2, -1, 7, 5, 0, 0, 7, 5, 1)
    assert (par.init_state, par.init_seq, par.samples, list(par.background)) == (2 ** 64 - 1, 5, 3, [0.5, 0.25, 1.0])
    par = _bake_lib.params(2, 1, 7, 5, (1, 2, 3, 1), False, 3, 1, 10, 3, 1, 42, 54, (0, 0, 0))
    assert (par.col0, par.row0, par.w, par.h, par.jitter) == (1, 2, 3, 1, 0)
    with pytest.raises(ValueError, match="samples"):
        _bake_lib.params(0, 1, 7, 5, None, True, 2 ** 31, 1, 10, 3, 1, 42, 54, (0, 0, 0))
    # texel centres as the bake forms them
    c = rb.texel_centres(7, 5, (2, 1, 3, 2))
    assert c.shape == (2, 3, 2) and c[1, 2, 0] == (4 + 0.5) * (1.0 / 7) and c[1, 2, 1] == (2 + 0.5) * (1.0 / 5)


def test_what_reaches_the_device_scene_without_a_device():
    """``light_map`` hands ``DeviceScene.bake`` PathTracer's defaults and ``depth=1``; ``surface_points`` broadcasts one shape and one
    side over the records and splits the answer; ``outgoing_map`` composes ``emitted + brdf_color * map`` and refuses a mirror."""
    seen = {}

    class Scene:
        kinds = abi.BRDF_DIFFUSE

        def bake(self, *args):
            seen["bake"] = args
            w, h = args[1], args[2]
            buf = np.zeros(rb.bake_bytes(w * h, rb.bake_channels(args[-1])), np.uint8)
            buf.view(np.float64)[: 3 * w * h] = 2.0
            return rb.BakedMap(buf, w, h, args[-1])

        def surface_points(self, shape, uv, side):
            seen["points"] = (shape, uv, side)
            return np.arange(6.0 * shape.shape[0]).reshape(6, -1)

        def surface(self, shape_index, uv, bits):
            seen["surface"] = (shape_index, uv, bits)
            n = shape_index.size
            buf = np.zeros(rb.surface_bytes(n, bits), np.uint8)
            buf[: 4 * n].view(np.int32)[:] = self.kinds
            buf[rb.surface_plane_offset(n, bits, rb.SURF_BRDF_COLOR):][: 24 * n].view(np.float64)[:] = 0.25
            buf[rb.surface_plane_offset(n, bits, rb.SURF_EMITTED):][: 24 * n].view(np.float64)[:] = 1.0
            return rb.SurfaceColors(buf, n, bits)

    wq = rb.WorldQueries(Scene())
    res = wq.light_map(4, 7, 5, 16)
    assert res.radiance.shape == (5, 7, 3) and res.n_rays.shape == (5, 7)
    assert seen["bake"] == (4, 7, 5, 16, 1, True, None, 42, 54, 1, 10, 3, (0.0, 0.0, 0.0), 1, "all")
    pts, nrm = wq.surface_points(3, np.zeros((2, 4, 2)), side=-1)
    assert pts.shape == nrm.shape == (2, 4, 3) and np.array_equal(pts[1, 2], [6.0, 14.0, 22.0]) and np.array_equal(nrm[0, 0], [24.0, 32.0, 40.0])
    assert seen["points"][0].tolist() == [3] * 8 and seen["points"][2].tolist() == [-1] * 8 and seen["points"][1].shape == (8, 2)
    with pytest.raises(ValueError, match="uv"):
        wq.surface_points(3, np.zeros((4, 3)))
    out = wq.outgoing_map(1, 7, 5, 8, max_depth=3)
    assert out.shape == (5, 7, 3) and np.all(out == 1.0 + 0.25 * 2.0)
    assert seen["surface"][0].shape == (5, 7) and np.all(seen["surface"][0] == 1) and np.array_equal(seen["surface"][1], rb.texel_centres(7, 5))
    assert seen["bake"][:6] == (1, 7, 5, 8, 1, True) and seen["bake"][10] == 3 and seen["bake"][-1] == "none"
    Scene.kinds = abi.BRDF_SPECULAR
    with pytest.raises(ValueError, match="DiffuseBRDF"):
        wq.outgoing_map(1, 7, 5, 8)


def test_baked_world_flattens_with_its_maps_in_the_image_pigments_order():
    from pytracer_amd import flatten, scenes
    from pytracer_amd import hostmodel as hm

    world, _ = R.host_world("demo")
    H, W = 3, 4
    maps = {0: np.arange(H * W * 3, dtype=np.float64).reshape(H, W, 3), 1: 100.0 + np.arange(2 * 5 * 3, dtype=np.float64).reshape(2, 5, 3)}
    before = flatten.flatten_world(world)
    baked = scenes.baked_world(world, maps)
    flat = flatten.flatten_world(baked)
    assert len(world.shapes) == len(baked.shapes) == 3  # (the input is not modified)
    assert type(world.shapes[0].material.emitted_radiance).__name__ == "UniformPigment"
    for i in (0, 1):
        assert flat.brdf_kind[i] == abi.BRDF_DIFFUSE and flat.pig_kind[i] == abi.PIGMENT_UNIFORM and not flat.pig_c1[:, i].any()
        assert flat.emi_kind[i] == abi.PIGMENT_IMAGE and flat.emi_tex[i] == i
        assert isinstance(baked.shapes[i].material.emitted_radiance, hm.ImagePigment)
    assert flat.tex_w.tolist() == [4, 5] and flat.tex_h.tolist() == [3, 2] and flat.tex_offset.tolist() == [0, 36]
    # ImagePigment.get_color reads pixel (col, row) = data[(row * w + col) * 3 ...]: the map's [row, col]
    for i, (w, off) in enumerate(((4, 0), (5, 36))):
        for row, col in ((0, 0), (1, 3), (1, 2)):
            assert np.array_equal(flat.tex_data[off + (row * w + col) * 3: off + (row * w + col) * 3 + 3], maps[i][row, col])
    # everything else stays: the transformations of all shapes, the mirror's material, the light
    assert np.array_equal(flat.m, before.m) and np.array_equal(flat.invm, before.invm) and np.array_equal(flat.kind, before.kind)
    assert flat.brdf_kind[2] == abi.BRDF_SPECULAR and np.array_equal(flat.pig_c1[:, 2], before.pig_c1[:, 2]) and baked.shapes[2] is world.shapes[2]
    assert np.array_equal(flat.light_pos, before.light_pos) and flat.light_pos.shape[1] == 1
    with pytest.raises(ValueError, match="no shape 3"):
        scenes.baked_world(world, {3: maps[0]})
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        scenes.baked_world(world, {0: np.zeros((3, 4))})


def test_the_restated_surface_point_inverts_the_shapes_uv_maps(oracle):
    """On the CPU, with libm: a ray from ``point + normal`` towards ``-normal`` meets the one shape at the (u, v) asked for, and at
    texel centres in the texel asked for -- 1x1, 7x5, 64x64 and 1000x3 maps of a sphere and of a plane.  The other side's point is
    the same and its normal the negative, exactly."""
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        for name, s in (("c2", M.diffuse_shapes("c2")[1]), ("demo", 1)):
            flat = R.world(name)[0]
            for W, H in ((1, 1), (7, 5), (64, 64), (1000, 3)):
                step = max(1, (W * H) // 400)
                for t in range(0, W * H, step):
                    r, c = divmod(t, W)
                    u, v = (c + 0.5) * (1.0 / W), (r + 0.5) * (1.0 / H)
                    p, n = M.surface_point(oracle, flat, s, u, v, 1)
                    hit = oracle.shape_intersect(flat, s, oracle.ray8(p + n, -n))
                    assert hit is not None and int(hit[7] * W) == c and int(hit[8] * H) == r, (name, W, H, t)
                    if 0.05 <= v <= 0.95:
                        assert abs(hit[7] - u) <= 1e-12 and abs(hit[8] - v) <= 1e-12
                    p2, n2 = M.surface_point(oracle, flat, s, u, v, -1)
                    assert np.array_equal(p2, p) and np.array_equal(n2, -n)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def test_the_expected_maps_depend_on_the_order_of_the_sum(oracle):
    """The discriminating power of the GPU's bit tests: on the oracle's composition of a 7 x 5 map at K = 70, adding each texel's
    samples from the last to the first changes the bits of most texels."""
    name, s = "c2", M.diffuse_shapes("c2")[1]
    want = M.expected(oracle, name, s, 70, 1, 2, 0)
    assert want["samples"].shape == (35, 70, 3) and G.same_bits(G.ordered_mean(want["samples"]), want["radiance"]).all()
    changed = ~G.same_bits(G.ordered_mean(want["samples"], reverse=True), want["radiance"])
    print(f"{name} shape {s}, 7x5 at K=70: the reverse order changes {changed.mean():.1%} of the texels")
    assert changed.mean() > 0.5
    assert np.array_equal(want["count"], want["sample_counts"].sum(axis=1)) and want["count"].min() >= 70
    # every sample sits inside its texel, and the samples of a texel are at different points
    cols, rows, _ = M.window_texels(7, 5)
    uv = want["uv"]
    assert np.all((uv[..., 0] * 7).astype(int) == cols[:, None]) and np.all((uv[..., 1] * 5).astype(int) == rows[:, None])
    assert all(len(np.unique(uv[i], axis=0)) == 70 for i in range(35))
