"""CPU-only tests of the denoise query (include/ptrace_denoise.h, libptrace_denoise.so, pytracer_amd.rays.denoise_host): the tenth
library builds and loads without a GPU and leaves the other nine as they were; its header, the ctypes table and its dynamic symbols
agree; every refusal of the interface happens before any HIP call; and the numpy mirror the GPU's bit tests compare with has the
properties of the filter it defines -- an exact B3 kernel that sums to 1, the separable blur where no guide cuts, shapes that do not
bleed, misses that are copied, a wrap that survives frames narrower than the stencil."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import rays as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE = -1, -3, -5  # include/ptrace.h
V18 = (1 << 16) | 8
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _denoise_lib, build

    build.build()
    assert os.path.exists(build.DENOISE_LIB) and not build.needs_build()
    return _denoise_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _denoise_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_denoise.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_denoise_lib.EXPORTS) == {s for s, _, _ in _denoise_lib._SIGNATURES} and len(declared) == 6
    assert all(s.startswith("pt_rays_denoise") for s in declared)
    assert _exported(_denoise_lib.lib_path()) == declared
    assert lib.pt_rays_denoise_version() == V18
    # an add-on like the nine before it: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _denoise_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_denoise.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _denoise_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    # the only file that includes the new device header is the new translation unit; the host layer is the shared one
    users = [f for f in os.listdir(build.CSRC) if '"pt_denoise.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_denoise.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_denoise.hip")).read() + open(os.path.join(build.CSRC, "pt_denoise.h")).read()
    assert '#include "pt_host_common.h"' in text and not re.search(r"\bg_err\b|\bstruct\s+Staged\b|#\s*define\s+HIP_TRY\b", text)
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text) and "exp(" not in text  # (no atomic of any kind is called; rational weights)
    assert "PT_DN_DIRECT" in text
    assert C.sizeof(_denoise_lib.DenoiseParams) == 32  # three ints, their padding and two doubles: pt_denoise_params
    assert (_denoise_lib.DN_SAME_SHAPE, _denoise_lib.DN_WRAP_X) == tuple(int(re.search(rf"#define {n}\s+(\d+)", header).group(1))
                                                                          for n in ("PT_DN_SAME_SHAPE", "PT_DN_WRAP_X"))
    for word in ("dy outer", "9/64", "bit for bit", "NON-FINITE COLOURS", "sigma_colour * 2^-i"):
        assert word in header, word


def test_the_pinned_build_tables_are_unchanged_and_the_new_row_is_in_its_own(lib):
    from pytracer_amd import build

    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_denoise.h")), "ptrace_denoise.hip", "pt_denoise.h"} <= deps
    assert len(build.TARGETS) == 6 and len(build.ALL_TARGETS) == 7 and len(build.EVERY_TARGET) == 8 and len(build.BUILD_TARGETS) == 9
    assert build.BUILD_TARGETS == build.EVERY_TARGET + ((build.LIT_FLAGS, build.LIT_LIB, build.LIT_SOURCES),)
    assert build.DENOISE_TARGETS == ((build.DENOISE_FLAGS, build.DENOISE_LIB, build.DENOISE_SOURCES),)
    assert build.WALK_TARGETS == build.BUILD_TARGETS + build.DENOISE_TARGETS and list(build.DENOISE_ADDONS) == ["denoise"]
    assert build.DENOISE_FLAGS[:-1] == build.FLAGS[:-1] and build.DENOISE_FLAGS[-1] == "-cuid=libptrace_denoise"
    assert "-ffp-contract=off" in build.DENOISE_FLAGS and not any("fast-math" in f and not f.startswith("-fno") for f in build.DENOISE_FLAGS)
    assert build.DENOISE_SOURCES == ["ptrace_denoise.hip"] and os.path.basename(build.DENOISE_LIB) == "libptrace_denoise.so"


def test_the_other_nine_libraries_are_what_they_were(lib):
    from pytracer_amd import _bake_lib, _gather_lib, _lib, _lit_lib, _radiance_lib, _rays_lib, _scatter_lib, _sh_lib, _surface_lib, build

    for module, count in ((_rays_lib, 7), (_surface_lib, 11), (_scatter_lib, 7), (_radiance_lib, 8), (_gather_lib, 8), (_bake_lib, 11), (_sh_lib, 14),
                          (_lit_lib, 9)):
        assert _exported(module.lib_path()) == set(module.EXPORTS) and len(module.EXPORTS) == count
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert _lit_lib.lib().pt_rays_lit_version() == (1 << 16) | 7
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "ptrace_denoise.h":
            assert "pt_rays_denoise" not in open(os.path.join(ROOT, "include", header)).read(), header
    # the recorded hashes: nine rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "denoise_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.BUILD_TARGETS] and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.BUILD_TARGETS]
    # and the eight the lit library recorded are still those
    old = [line.split() for line in open(os.path.join(ROOT, "profiles", "lit_hashes.txt")) if line.startswith("libptrace")]
    assert [r[:3] for r in rows[:8]] == [r[:3] for r in old[:8]]


def test_sizes(lib):
    from pytracer_amd import _denoise_lib

    for m in (0, 1, 63, 65, 2 ** 31 - 1):
        assert lib.pt_rays_denoise_bytes(m) == 24 * m
    assert lib.pt_rays_denoise_bytes(-1) == 0 and lib.pt_rays_denoise_bytes(2 ** 31) == 0
    ws = lambda w, h, **kw: lib.pt_rays_denoise_workspace_bytes(w, h, C.byref(_denoise_lib.params(**kw)))  # noqa: E731
    assert ws(7, 3) == 2 * 24 * 21 and ws(7, 3, passes=1) == 24 * 21 and ws(7, 3, passes=10) == 2 * 24 * 21
    assert ws(2 ** 31 - 1, 1) == 48 * (2 ** 31 - 1) and ws(46340, 46340, passes=1) == 24 * 46340 ** 2 and ws(0, 5) == 0
    assert ws(46341, 46341) == 0 and "2^31 - 1" in _denoise_lib.last_error()
    assert ws(-1, 4) == 0 and ws(4, 4, passes=0) == 0 and ws(4, 4, sigma_point=0.0) == 0
    assert lib.pt_rays_denoise_workspace_bytes(4, 4, None) == 0 and "null pt_denoise_params" in _denoise_lib.last_error()


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
passed = lambda rc: rc not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # noqa: E731  (got as far as the first HIP call)


def test_every_refusal_happens_before_any_hip_call(lib):
    """No GPU here: whatever is refused with PT_ERR_INVALID / SIZE was refused by the argument checks (the first HIP call would
    answer PT_ERR_NODEVICE)."""
    from pytracer_amd import _denoise_lib

    W, H = 5, 3
    m = W * H
    col, nrm, pnt, shp, out = np.zeros((3, m)), np.ones((3, m)), np.zeros((3, m)), np.zeros(m, np.int32), np.zeros((3, m))
    work = np.zeros(2 * 3 * m)

    def call(device=0, w=W, h=H, par=True, c=col, n=nrm, pt=pnt, s=shp, o=out, ob=None, wk=work, wb=None, **kw):
        par = C.byref(_denoise_lib.params(**kw)) if par else None
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        wb = (wk.nbytes if wk is not None else 0) if wb is None else wb
        return (lib.pt_rays_denoise(device, w, h, par, p(c), p(n), p(pt), p(s), p(o), ob),
                lib.pt_rays_denoise_device(device, w, h, par, p(c), p(n), p(pt), p(s), p(o), ob, p(wk), wb, None))

    err = _denoise_lib.last_error
    assert all(passed(rc) for rc in call())
    assert all(passed(rc) for rc in call(sigma_point=INF, sigma_colour=INF, passes=10, normal_power_log2=10, flags=3))
    assert all(passed(rc) for rc in call(passes=1, normal_power_log2=0, flags=0, wb=3 * m * 8))  # (one pass: half the workspace)
    assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
    assert call(w=46341, h=46341, ob=2 ** 40, wb=2 ** 41) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert call(w=2 ** 31 - 1, h=2, ob=2 ** 40, wb=2 ** 41) == both(ERR_INVALID)
    assert call(par=False) == both(ERR_INVALID) and "null pt_denoise_params" in err()
    for passes in (0, 11, -1):
        assert call(passes=passes) == both(ERR_INVALID) and "passes" in err(), passes
    for name in ("sigma_point", "sigma_colour"):
        for bad in (0.0, -1.0, -INF, float("nan")):
            assert call(**{name: bad}) == both(ERR_INVALID) and name in err(), (name, bad)
    for e in (-1, 11):
        assert call(normal_power_log2=e) == both(ERR_INVALID) and "normal_power_log2" in err(), e
    for flags in (4, 8, -1, 1 << 30):
        assert call(flags=flags) == both(ERR_INVALID) and "flag" in err(), flags
    assert call(device=-1) == both(ERR_INVALID)
    for kw in (dict(c=None), dict(n=None), dict(pt=None), dict(s=None)):
        assert call(**kw) == both(ERR_INVALID) and "planes" in err(), kw
    assert call(o=None, ob=out.nbytes) == both(ERR_INVALID) and "null output" in err()
    host, dev = call(wk=None, wb=work.nbytes)  # the workspace is the device form's alone: the host form makes its own
    assert passed(host) and dev == ERR_INVALID and "workspace" in err()
    # `out` overlapping `colour` (wholly, or by one value at either end) or the workspace
    assert call(o=col) == both(ERR_INVALID) and "overlaps the colour" in err()
    big = np.zeros(2 * 3 * m + 3 * m)
    for off in (1, 3 * m - 1):
        assert call(c=big[off:off + 3 * m].reshape(3, m), o=big[:3 * m].reshape(3, m)) == both(ERR_INVALID), off
        assert call(o=big[off:off + 3 * m].reshape(3, m), c=big[:3 * m].reshape(3, m)) == both(ERR_INVALID), off
    assert all(passed(rc) for rc in call(c=big[:3 * m].reshape(3, m), o=big[3 * m:6 * m].reshape(3, m)))  # (adjacent is not overlapping)
    host, dev = call(o=big[:3 * m].reshape(3, m), wk=big[3 * m - 1:])
    assert passed(host) and dev == ERR_INVALID and "overlaps the workspace" in err()
    host, dev = call(o=big[6 * m - 1:9 * m - 1].reshape(3, m), wk=big[:6 * m])  # (the workspace's second half counts)
    assert passed(host) and dev == ERR_INVALID
    assert all(passed(rc) for rc in call(o=big[3 * m:6 * m].reshape(3, m), wk=big[:3 * m], passes=1))  # (one pass: it has no second half)
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "output too small" in err()
    host, dev = call(wb=work.nbytes - 1)
    assert passed(host) and dev == ERR_SIZE and "workspace too small" in err()
    # a launch alternative nobody knows is refused too, before any HIP call
    for name, value in (("PTRACE_DN_TILE", "20x20"), ("PTRACE_DN_VARIANT", "fast"), ("PTRACE_DN_BLOCKS", "0"), ("PTRACE_DN_BLOCKS", "many")):
        os.environ[name] = value
        try:
            assert call() == both(ERR_INVALID) and name in err(), (name, value)
        finally:
            del os.environ[name]
    # m = 0: PT_OK, nothing launched, no buffer needed -- but the parameters are still checked
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert call(w=w, h=h, c=None, n=None, pt=None, s=None, o=None, wk=None) == both(0), (w, h)
    assert call(w=0, h=0, passes=0) == both(ERR_INVALID) and call(w=0, h=0, flags=4) == both(ERR_INVALID)
    assert not out.any() and not work.any()


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def coplanar_frame(W, H, seed=1):
    """One shape, one plane (z = 0, a normal of length 2), points on a lattice, random colours."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    point = np.stack([xx * 0.125, yy * 0.125, np.zeros_like(xx)], axis=-1).astype(np.float64)
    normal = np.zeros((H, W, 3))
    normal[..., 2] = 2.0
    return rng.uniform(0.0, 1.0, (H, W, 3)), np.zeros((H, W), np.int32), normal, point


def two_shape_frame(W, H):
    """Two shapes side by side, coloured 0.5 and 2.0 (powers of two: every weighted mean of equal values is that value)."""
    _, shape, normal, point = coplanar_frame(W, H)
    shape[:, W // 2:] = 1
    return np.where(shape[..., None] == 0, 0.5, 2.0) * np.ones(3), shape, normal, point


def b3_blur_interior(colour):
    """The separable B3 blur of the pixels at least 2 from every edge, in the filter's own order of summation."""
    H, W = colour.shape[:2]
    h = rb.DENOISE_KERNEL
    total, wsum = np.zeros((H - 4, W - 4, 3)), 0.0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = h[dx + 2] * h[dy + 2]
            total, wsum = total + k * colour[2 + dy:H - 2 + dy, 2 + dx:W - 2 + dx], wsum + k
    return total / wsum


def test_the_kernel_is_exact_and_sums_to_one():
    from fractions import Fraction

    h = [Fraction(1, 16), Fraction(1, 4), Fraction(3, 8), Fraction(1, 4), Fraction(1, 16)]
    assert [Fraction(x) for x in rb.DENOISE_KERNEL] == h
    ks = [rb.DENOISE_KERNEL[a] * rb.DENOISE_KERNEL[b] for b in range(5) for a in range(5)]
    assert [Fraction(k) for k in ks] == [h[a] * h[b] for b in range(5) for a in range(5)]  # (all 25 products are exact)
    assert sum(Fraction(k) for k in ks) == 1 and Fraction(ks[12]) == Fraction(9, 64)
    total = 0.0
    for k in ks:  # (and so is their sum in tap order, in fp64)
        total = total + k
    assert total == 1.0
    assert sum(Fraction(k) ** 2 for k in ks) == Fraction(70, 256) ** 2  # the noise a flat region keeps after one pass: 0.273


def test_a_coplanar_shape_without_weights_is_the_separable_b3_blur():
    W, H = 23, 14
    colour, shape, normal, point = coplanar_frame(W, H)
    got = rb.denoise_host(colour, shape, normal, point, W, H, passes=1, sigma_point=INF, normal_power_log2=0, sigma_colour=INF)
    assert got.shape == (H, W, 3) and _same(got[2:-2, 2:-2], b3_blur_interior(colour))
    # a finite sigma_point changes nothing on a plane (dz = 0 exactly), and neither does the power of cos = 1
    again = rb.denoise_host(colour, shape, normal, point, W, H, passes=1, sigma_point=1e-3, normal_power_log2=10)
    assert _same(again, got)
    # at the border the kernel is renormalised over the taps inside: a constant frame stays constant to the last bit
    flat = rb.denoise_host(np.full((H, W, 3), 0.75), shape, normal, point, W, H, passes=4)
    assert _same(flat, np.full((H, W, 3), 0.75))
    # and the second pass is the same blur with the step 2 on the first pass's output
    two = rb.denoise_host(colour, shape, normal, point, W, H, passes=2, sigma_point=INF, normal_power_log2=0)
    h = rb.DENOISE_KERNEL
    y, x = 6, 11
    total = np.zeros(3)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            total = total + (h[dx + 2] * h[dy + 2]) * got[y + 2 * dy, x + 2 * dx]
    assert _same(two[y, x], total / 1.0)


@pytest.mark.parametrize("wrap", [False, True])
def test_two_shapes_do_not_bleed(wrap):
    W, H = 22, 9
    colour, shape, normal, point = two_shape_frame(W, H)
    assert _same(rb.denoise_host(colour, shape, normal, point, W, H, passes=5, wrap_x=wrap), colour)
    # without PT_DN_SAME_SHAPE they do (one plane, one normal: nothing else tells them apart)
    bled = rb.denoise_host(colour, shape, normal, point, W, H, passes=1, same_shape=False)
    assert not _same(bled, colour) and _same(bled[:, :W // 2 - 2], colour[:, :W // 2 - 2])


def test_miss_pixels_are_copied_and_never_read():
    W, H = 19, 11
    colour, shape, normal, point = coplanar_frame(W, H, seed=3)
    rng = np.random.default_rng(4)
    miss = rng.uniform(0, 1, (H, W)) < 0.3
    shape[miss] = rng.integers(-2 ** 31, 0, int(miss.sum()))
    got = rb.denoise_host(colour, shape, normal, point, W, H, passes=3)
    assert _same(got[miss], colour[miss]) and np.isfinite(got).all()
    # whatever a miss holds -- colour, normal, point -- changes no other pixel
    c2, n2, p2 = colour.copy(), normal.copy(), point.copy()
    c2[miss], n2[miss], p2[miss] = np.nan, 0.0, np.inf
    again = rb.denoise_host(c2, shape, n2, p2, W, H, passes=3)
    assert _same(again[~miss], got[~miss]) and np.isnan(again[miss]).all()
    # NaN guides only ever skip taps; a NaN colour stays in its own pixel
    hit = np.flatnonzero(~miss.reshape(-1))
    n3, c3 = normal.copy(), colour.copy()
    n3.reshape(-1, 3)[hit[5]] = np.nan
    c3.reshape(-1, 3)[hit[9]] = np.nan
    out = rb.denoise_host(c3, shape, n3, point, W, H, passes=3).reshape(-1, 3)
    assert np.isnan(out[hit[9]]).all() and np.isfinite(np.delete(out, hit[9], axis=0)).all()
    alone = c3.reshape(-1, 3)[hit[5]]
    for _ in range(3):  # (its own centre tap is all it has, in every pass)
        alone = (0.0 + 0.140625 * alone) / (0.0 + 0.140625)
    assert _same(out[hit[5]], alone)


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (17, 5), (2, 7)])
def test_the_wrap_on_frames_narrower_than_the_stencil(W, H):
    colour, shape, normal, point = coplanar_frame(W, H, seed=W)
    for passes in (1, 5, 10):  # (2 s = 2 .. 1024 columns against W of 1 .. 17)
        got = rb.denoise_host(colour, shape, normal, point, W, H, passes=passes, wrap_x=True, sigma_point=INF)
        assert got.shape == (H, W, 3) and np.isfinite(got).all()
        assert got.min() >= colour.min() - 1e-12 and got.max() <= colour.max() + 1e-12  # (a weighted mean of the input)
        plain = rb.denoise_host(colour, shape, normal, point, W, H, passes=passes, wrap_x=False, sigma_point=INF)
        assert np.isfinite(plain).all()
    # under the wrap a constant column profile is kept: every column sees the same neighbours
    cols = np.broadcast_to(np.linspace(0.0, 1.0, H)[:, None, None], (H, W, 3)).copy()
    out = rb.denoise_host(cols, shape, normal, point * 0.0, W, H, passes=2, wrap_x=True, sigma_point=INF)
    assert np.abs(out - out[:, :1]).max() <= 1e-15


def test_the_mirror_refuses_what_the_library_refuses_and_depends_on_the_tap_order():
    W, H = 9, 6
    colour, shape, normal, point = coplanar_frame(W, H)
    for kw in (dict(passes=0), dict(passes=11), dict(normal_power_log2=-1), dict(normal_power_log2=11), dict(sigma_point=0.0),
               dict(sigma_colour=float("nan")), dict(sigma_point=-INF)):
        with pytest.raises(ValueError):
            rb.denoise_host(colour, shape, normal, point, W, H, **kw)
    assert rb.denoise_host(np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), 0, 4).shape == (4, 0, 3)
    # the discriminating power of the GPU's bit tests: summing the taps from the last to the first changes bits
    got = rb.denoise_host(colour, shape, normal, point, W, H, passes=1, sigma_point=INF, normal_power_log2=0)
    back = rb.denoise_host(colour[::-1, ::-1], shape, normal, point[::-1, ::-1], W, H, passes=1, sigma_point=INF, normal_power_log2=0)[::-1, ::-1]
    changed = (got.view(np.uint64) != np.ascontiguousarray(back).view(np.uint64)).any(axis=-1)
    print(f"{W}x{H}: the reverse tap order changes {changed.mean():.1%} of the pixels")
    assert changed.mean() > 0.2 and np.abs(got - back).max() <= 8 * 2.0 ** -52


def test_what_reaches_the_device_scene_without_a_device():
    """``WorldQueries.denoised`` takes a gather, a bake or an array with a frame, a ray batch or plain guides, and refuses more than
    one sample per pixel; ``denoised_light_map`` composes bake, surface points and filter and picks the wrap by the shape's kind; the
    shader asks its tracer's queries for gather, filter and materials in that order."""
    from types import SimpleNamespace

    from pytracer_amd import abi, shaders
    from pytracer_amd import hostmodel as hm

    seen = []

    class Scene:
        flat = SimpleNamespace(kind=np.array([abi.SHAPE_SPHERE, abi.SHAPE_PLANE], np.int32))

        def denoise(self, colour, shape_index, normal, point, width, height, **params):
            seen.append(("denoise", colour, shape_index, normal, point, width, height, params))
            return np.asarray(colour).reshape(height, width, 3) + 1.0

    wq = rb.WorldQueries(Scene())
    H, W = 3, 4
    frame = SimpleNamespace(shape_index=np.zeros((1, H, W), np.int32), point=np.zeros((1, H, W, 3)), normal=np.ones((1, H, W, 3)))
    values = np.arange(H * W * 3.0).reshape(H, W, 3)
    out = wq.denoised(values, frame, passes=2)
    assert out.shape == (H, W, 3) and np.array_equal(out, values + 1.0)
    assert seen[-1][5:] == (W, H, dict(passes=2)) and seen[-1][2].shape == (H * W,) and seen[-1][3].shape == (H * W, 3)
    gathered = rb.GatheredRadiance(np.zeros(rb.gather_bytes(H * W, 0), np.uint8), H * W, 0, shape=(1, H, W))
    assert wq.denoised(gathered, frame).shape == (H, W, 3) and seen[-1][5:7] == (W, H)
    baked = rb.BakedMap(np.zeros(rb.bake_bytes(H * W, 0), np.uint8), W, H, 0)
    assert wq.denoised(baked, (np.zeros((H, W, 3)), np.ones((H, W, 3)), 1), wrap_x=True).shape == (H, W, 3)
    assert seen[-1][2].tolist() == [1] * (H * W) and seen[-1][7] == dict(wrap_x=True)
    batch = SimpleNamespace(shape_index=np.zeros(H * W, np.int32), point=np.zeros((H * W, 3)), normal=np.ones((H * W, 3)))
    assert wq.denoised(values, batch).shape == (H, W, 3)  # (a ray batch: the frame is the values')
    flat_values = values.reshape(-1, 3)
    assert wq.denoised(flat_values, SimpleNamespace(shape_index=np.zeros((H, W), np.int32), point=batch.point, normal=batch.normal)).shape == (H, W, 3)
    many = SimpleNamespace(shape_index=np.zeros((4, H, W), np.int32), point=np.zeros((4, H, W, 3)), normal=np.ones((4, H, W, 3)))
    with pytest.raises(ValueError, match="samples per pixel"):
        wq.denoised(values, many)
    with pytest.raises(ValueError, match="samples per pixel"):
        wq.denoised(np.zeros((4, H, W, 3)), frame)
    with pytest.raises(ValueError, match="no frame"):
        wq.denoised(flat_values, batch)
    with pytest.raises(ValueError, match="shape indices"):
        wq.denoised(values, SimpleNamespace(shape_index=np.zeros(5, np.int32), point=batch.point, normal=batch.normal))
    # the light map: bake -> surface points at the texel centres -> filter; the wrap follows the shape's kind unless it is given
    calls = []
    wq.light_map = lambda shape, w, h, samples, **kw: calls.append(("bake", shape, w, h, samples, kw)) or baked
    wq.surface_points = lambda shape, uv, side=1: calls.append(("points", shape, uv.shape, side)) or (np.zeros((H, W, 3)), np.ones((H, W, 3)))
    for shape, wrap_u, expect in ((0, None, True), (1, None, False), (0, False, False), (1, True, True)):
        del calls[:]
        out = wq.denoised_light_map(shape, W, H, 16, wrap_u=wrap_u, passes=3, max_depth=2, side=-1)
        assert out.shape == (H, W, 3) and [c[0] for c in calls] == ["bake", "points"]
        assert calls[0][1:5] == (shape, W, H, 16) and calls[0][5] == dict(max_depth=2, side=-1, channels="none") and calls[1][1:] == (shape, (H, W, 2), -1)
        assert seen[-1][7] == dict(wrap_x=expect, passes=3) and seen[-1][2].tolist() == [shape] * (H * W)
    with pytest.raises(ValueError, match="window"):
        wq.denoised_light_map(0, W, H, 16, window=(0, 0, 2, 2))
    # the shader
    world = hm.World()
    order = []

    class Queries:
        def hemisphere_radiance(self, hits, samples, *a, **kw):
            order.append(("gather", samples, a, kw))
            return gathered

        def denoised(self, values, hits, **params):
            order.append(("filter", params))
            return np.full((H, W, 3), 2.0)

        def materials(self, hits):
            order.append(("materials",))
            hit = np.ones((1, H, W), bool)
            hit[0, 0, 0] = False
            return SimpleNamespace(emitted=np.full((1, H, W, 3), 0.5), brdf_color=np.full((1, H, W, 3), 0.25), hit=hit)

    tracer = SimpleNamespace(world_queries=lambda w: Queries() if w is world else None)
    shader = shaders.DenoisedGatherShader(world, tracer, samples=4, background_color=hm.Color(7.0, 8.0, 9.0), passes=2, sigma_point=0.5)
    out = shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "filter", "materials"] and order[0][1] == 4 and order[1][1] == dict(passes=2, sigma_point=0.5)
    assert out.shape == (1, H, W, 3) and out[0, 0, 0].tolist() == [7.0, 8.0, 9.0] and np.all(out[0, 1:] == 0.5 + 0.25 * 2.0)
    shader.filtered = False
    del order[:]
    noisy = shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "materials"] and np.all(noisy[0, 1:] == 0.5)  # (the gather's zeros)
    with pytest.raises(ValueError, match="one record per pixel"):
        shader.shade_hits(many)
    with pytest.raises(TypeError, match="tracer"):
        shaders.DenoisedGatherShader(world).shade_hits(frame)
    with pytest.raises(TypeError, match="ray_intersection"):
        shaders.DenoisedGatherShader(world)(None)
    with pytest.raises(TypeError, match="unknown filter parameter"):
        shaders.DenoisedGatherShader(world, tracer, wrap_x=True)
    with pytest.raises(ValueError, match="samples"):
        shaders.DenoisedGatherShader(world, tracer, samples=0)
