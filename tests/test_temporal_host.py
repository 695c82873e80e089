"""CPU-only tests of the accumulate query (include/ptrace_temporal.h, libptrace_temporal.so, pytracer_amd.rays.temporal_host): the
eleventh library builds and loads without a GPU and leaves the other ten as they were; its header, the ctypes table and its dynamic
symbols agree; every refusal of the interface happens before any HIP call; and the numpy mirror the GPU's bit tests compare with has
the properties of the accumulation it defines -- a projection that inverts the camera, a running mean that is exact on powers of two,
shapes that do not bleed, no history where there is none, misses that are copied, and sums whose order reaches the bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb
from pytracer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_SIZE, ERR_NODEVICE = -1, -5, -6  # include/ptrace.h
V19 = (1 << 16) | 9
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _temporal_lib, build

    build.build()
    assert os.path.exists(build.TEMPORAL_LIB) and not build.needs_build()
    return _temporal_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _temporal_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_temporal.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_temporal_lib.EXPORTS) == {s for s, _, _ in _temporal_lib._SIGNATURES} and len(declared) == 7
    assert all(s.startswith("pt_rays_temporal_") for s in declared)
    assert {"pt_rays_temporal_version", "pt_rays_temporal_last_error", "pt_rays_temporal_bytes", "pt_rays_temporal_count_bytes",
            "pt_rays_temporal_accumulate_device", "pt_rays_temporal_accumulate"} <= declared
    assert _exported(_temporal_lib.lib_path()) == declared
    assert lib.pt_rays_temporal_version() == V19
    # an add-on like the ten before it: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _temporal_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_temporal.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _temporal_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    # the only file that includes the new device header is the new translation unit; the host layer is the shared one
    users = [f for f in os.listdir(build.CSRC) if '"pt_temporal.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_temporal.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_temporal.hip")).read() + open(os.path.join(build.CSRC, "pt_temporal.h")).read()
    assert '#include "pt_host_common.h"' in text and not re.search(r"\bg_err\b|\bstruct\s+Staged\b|#\s*define\s+HIP_TRY\b", text)
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text) and "__shared__" not in text  # (no atomic of any kind is called; no LDS)
    assert text.count("hipLaunchKernelGGL") == 1 and "PTRACE_TA_BLOCKS" in text  # (one launch per call)
    # pt_temporal_params: two ints and two doubles; pt_temporal_camera: an int, its padding and fourteen doubles
    assert C.sizeof(_temporal_lib.TemporalParams) == 24 and C.sizeof(_temporal_lib.TemporalCamera) == 120
    assert _temporal_lib.TA_SAME_SHAPE == int(re.search(r"#define PT_TA_SAME_SHAPE\s+(\d+)", header).group(1))
    assert _temporal_lib.MAX_HISTORY == int(re.search(r"#define PT_TA_MAX_HISTORY\s+(\d+)", header).group(1)) == 2 ** 20
    assert (abi.CAMERA_ORTHOGONAL, abi.CAMERA_PERSPECTIVE) == (0, 1)  # (PT_CAMERA_* of ptrace.h, which the camera struct's kind holds)
    for word in ("bit for bit", "NON-FINITE COLOURS", "(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)", "min(nmax + 1, max_history)",
                 "hist[ch] + (colour[ch] - hist[ch]) * alpha"):
        assert word in header, word


def test_the_pinned_build_tables_are_unchanged_and_the_new_row_is_in_its_own(lib):
    from pytracer_amd import build

    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_temporal.h")), "ptrace_temporal.hip", "pt_temporal.h"} <= deps
    assert [len(t) for t in (build.TARGETS, build.ALL_TARGETS, build.EVERY_TARGET, build.BUILD_TARGETS, build.WALK_TARGETS)] == [6, 7, 8, 9, 10]
    assert build.WALK_TARGETS == build.BUILD_TARGETS + ((build.DENOISE_FLAGS, build.DENOISE_LIB, build.DENOISE_SOURCES),)
    assert list(build.DENOISE_ADDONS) == ["denoise"] and list(build.TEMPORAL_ADDONS) == ["temporal"]
    assert build.TEMPORAL_TARGETS == ((build.TEMPORAL_FLAGS, build.TEMPORAL_LIB, build.TEMPORAL_SOURCES),)
    assert build.FRAME_TARGETS == build.WALK_TARGETS + build.TEMPORAL_TARGETS and len(build.FRAME_TARGETS) == 11
    assert build.TEMPORAL_FLAGS[:-1] == build.FLAGS[:-1] and build.TEMPORAL_FLAGS[-1] == "-cuid=libptrace_temporal"
    assert "-ffp-contract=off" in build.TEMPORAL_FLAGS and not any("fast-math" in f and not f.startswith("-fno") for f in build.TEMPORAL_FLAGS)
    assert build.TEMPORAL_SOURCES == ["ptrace_temporal.hip"] and os.path.basename(build.TEMPORAL_LIB) == "libptrace_temporal.so"
    assert all(os.path.exists(t[1]) for t in build.FRAME_TARGETS)  # build() made all eleven


def test_the_other_ten_libraries_are_what_they_were(lib):
    from pytracer_amd import (_bake_lib, _denoise_lib, _gather_lib, _lib, _lit_lib, _radiance_lib, _rays_lib, _scatter_lib, _sh_lib, _surface_lib,
                              build)

    for module, count in ((_rays_lib, 7), (_surface_lib, 11), (_scatter_lib, 7), (_radiance_lib, 8), (_gather_lib, 8), (_bake_lib, 11), (_sh_lib, 14),
                          (_lit_lib, 9), (_denoise_lib, 6)):
        assert _exported(module.lib_path()) == set(module.EXPORTS) and len(module.EXPORTS) == count
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert _denoise_lib.lib().pt_rays_denoise_version() == (1 << 16) | 8
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "ptrace_temporal.h":
            assert "pt_rays_temporal" not in open(os.path.join(ROOT, "include", header)).read(), header
    # the recorded hashes: ten rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "temporal_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.WALK_TARGETS] and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.WALK_TARGETS]
    # and the nine the denoise library recorded are still those
    old = [line.split() for line in open(os.path.join(ROOT, "profiles", "denoise_hashes.txt")) if line.startswith("libptrace")]
    assert [r[:3] for r in rows[:9]] == [r[:3] for r in old[:9]]


def test_sizes(lib):
    for m in (0, 1, 63, 65, 2 ** 31 - 1):
        assert lib.pt_rays_temporal_bytes(m) == 24 * m and lib.pt_rays_temporal_count_bytes(m) == 4 * m
    for m in (-1, 2 ** 31):
        assert lib.pt_rays_temporal_bytes(m) == 0 and lib.pt_rays_temporal_count_bytes(m) == 0


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
NOWHERE = 2 ** 20  # a device no machine has: a call that passes every argument check ends at the device check, with or without a GPU
IDENTITY12 = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_every_refusal_happens_before_any_hip_call(lib):
    """Every call names a device that does not exist, so nothing is ever launched: a call that passes the argument checks ends at the
    first HIP call, the device check (PT_ERR_NODEVICE without a GPU, "out of range" with one); whatever is refused otherwise was
    refused by the argument checks before it."""
    from pytracer_amd import _temporal_lib

    def passed(rc):
        return rc == ERR_NODEVICE or (rc == ERR_INVALID and "out of range" in _temporal_lib.last_error())

    W, H = 5, 3
    m = W * H
    f3, i1 = (lambda: np.zeros((3, m))), (lambda: np.zeros(m, np.int32))
    names = ("c", "s", "n", "pt", "pc", "ps", "pn", "pp", "pk")
    planes = dict(c=f3(), s=i1(), n=f3() + 1.0, pt=f3(), pc=f3(), ps=i1(), pn=f3() + 1.0, pp=f3(), pk=i1())
    out, cnt = f3(), i1()

    def call(device=NOWHERE, w=W, h=H, par=True, cam=True, kind=abi.CAMERA_PERSPECTIVE, o=out, ob=None, k=cnt, kb=None, **kw):
        a = {name: kw.pop(name, planes[name]) for name in names}
        par = C.byref(_temporal_lib.params(**kw)) if par else None
        cam = C.byref(_temporal_lib.camera((kind, IDENTITY12, 1.0, 1.0))) if cam else None
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        kb = (k.nbytes if k is not None else 0) if kb is None else kb
        args = [device, w, h, par, cam] + [p(a[name]) for name in names] + [p(o), ob, p(k), kb]
        return lib.pt_rays_temporal_accumulate(*args), lib.pt_rays_temporal_accumulate_device(*args, None)

    err = _temporal_lib.last_error
    assert all(passed(rc) for rc in call())
    assert all(passed(rc) for rc in call(max_history=2 ** 20, flags=0, normal_min=-1.0, point_tolerance=INF, kind=abi.CAMERA_ORTHOGONAL))
    assert all(passed(rc) for rc in call(max_history=1, flags=1, normal_min=1.0, point_tolerance=5e-324))
    assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
    assert call(w=46341, h=46341, ob=2 ** 40, kb=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert call(w=2 ** 31 - 1, h=2, ob=2 ** 40, kb=2 ** 40) == both(ERR_INVALID)
    assert call(par=False) == both(ERR_INVALID) and "null pt_temporal_params" in err()
    assert call(cam=False) == both(ERR_INVALID) and "null pt_temporal_camera" in err()
    for max_history in (0, -1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert call(max_history=max_history) == both(ERR_INVALID) and "max_history" in err(), max_history
    for flags in (2, 4, -1, 1 << 30):
        assert call(flags=flags) == both(ERR_INVALID) and "flag" in err(), flags
    for bad in (-1.0000000000000002, 1.0000000000000002, INF, -INF, NAN):
        assert call(normal_min=bad) == both(ERR_INVALID) and "normal_min" in err(), bad
    for bad in (0.0, -0.0, -1.0, -INF, NAN):
        assert call(point_tolerance=bad) == both(ERR_INVALID) and "point_tolerance" in err(), bad
    for kind in (-1, 2, 7):
        assert call(kind=kind) == both(ERR_INVALID) and "camera kind" in err(), kind
    assert call(device=-1) == both(ERR_INVALID)
    for name in names:
        assert call(**{name: None}) == both(ERR_INVALID) and "null" in err() and "planes" in err(), name
    assert call(o=None, ob=out.nbytes) == both(ERR_INVALID) and "null output" in err()
    assert call(k=None, kb=cnt.nbytes) == both(ERR_INVALID) and "null output" in err()
    # either output overlapping `colour` or any plane of the previous frame, wholly or by one value at either end
    big = np.zeros(6 * m + 2)
    whole, ints = big[:3 * m].reshape(3, m), big[:m].view(np.int32)[:m]
    for name in ("c", "pc", "pn", "pp"):
        assert call(o=planes[name]) == both(ERR_INVALID) and "colour output overlaps" in err(), name
        for off in (1, 3 * m - 1):
            assert call(o=big[off:off + 3 * m].reshape(3, m), **{name: whole}) == both(ERR_INVALID), (name, off)
            assert call(o=whole, **{name: big[off:off + 3 * m].reshape(3, m)}) == both(ERR_INVALID), (name, off)
        assert all(passed(rc) for rc in call(o=big[3 * m:6 * m].reshape(3, m), **{name: whole})), name  # (adjacent is not overlapping)
        assert call(k=ints, **{name: whole}) == both(ERR_INVALID) and "count output overlaps" in err(), name
    for name in ("ps", "pk"):
        assert call(k=planes[name]) == both(ERR_INVALID) and "count output overlaps" in err(), name
        half = big.view(np.int32)
        for off in (1, m - 1):
            assert call(k=half[off:off + m], **{name: half[:m]}) == both(ERR_INVALID), (name, off)
        assert all(passed(rc) for rc in call(k=half[m:2 * m], **{name: half[:m]})), name
        assert call(o=whole, **{name: ints}) == both(ERR_INVALID) and "colour output overlaps" in err(), name
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "colour output too small" in err()
    assert call(kb=cnt.nbytes - 1) == both(ERR_SIZE) and "count output too small" in err()
    # a launch alternative nobody knows is refused too, before any HIP call
    for value in ("0", "many", "-3", "2x"):
        os.environ["PTRACE_TA_BLOCKS"] = value
        try:
            assert call() == both(ERR_INVALID) and "PTRACE_TA_BLOCKS" in err(), value
        finally:
            del os.environ["PTRACE_TA_BLOCKS"]
    # m = 0: PT_OK, nothing launched, no buffer needed -- but the structs are still checked
    nothing = {name: None for name in names}
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert call(w=w, h=h, o=None, k=None, **nothing) == both(0), (w, h)
    assert call(w=0, h=0, max_history=0) == both(ERR_INVALID) and call(w=0, h=0, flags=4) == both(ERR_INVALID)
    assert call(w=0, h=0, kind=3) == both(ERR_INVALID) and call(w=0, h=0, par=False) == both(ERR_INVALID)
    assert call(w=0, h=0, normal_min=NAN) == both(ERR_INVALID) and call(w=0, h=0, point_tolerance=0.0) == both(ERR_INVALID)
    # the empty history's own refusals
    clear = lib.pt_rays_temporal_clear_device
    assert clear(NOWHERE, -1, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, 2 ** 31, p(cnt), 2 ** 40, None) == ERR_INVALID
    assert clear(-1, m, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, m, None, cnt.nbytes, None) == ERR_INVALID and "null" in err()
    assert clear(NOWHERE, m, p(cnt), cnt.nbytes - 1, None) == ERR_SIZE and clear(NOWHERE, 0, None, 0, None) == 0
    assert passed(clear(NOWHERE, m, p(cnt), cnt.nbytes, None))
    assert not out.any() and not cnt.any()


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cameras(aspect=1.0):
    """One camera of each kind, neither at the origin nor along an axis."""
    return {"perspective": hm.PerspectiveCamera(1.25, aspect, hm.rotation_z(30.0) * hm.translation(hm.Vec(-4.0, 0.25, 1.0))),
            "orthogonal": hm.OrthogonalCamera(aspect, hm.rotation_z(-15.0) * hm.translation(hm.Vec(-3.0, -0.5, 0.75)) * hm.scaling(hm.Vec(1.0, 2.0, 2.0)))}


def primary_rays(camera, W, H):
    """Origins and directions ``[H, W, 3]`` of the primary rays through the pixel centres: ``GpuImageTracer.fire_ray`` in numpy."""
    from pytracer_amd import flatten

    cam = flatten.flatten_camera(camera)
    m = np.array(list(cam.m)).reshape(3, 4)
    u = ((np.arange(W) + 0.5) / W)[None, :] * np.ones((H, 1))
    v = (1.0 - (np.arange(H) + 0.5) / H)[:, None] * np.ones((1, W))
    one, zero = np.ones((H, W)), np.zeros((H, W))
    if cam.kind == abi.CAMERA_PERSPECTIVE:
        o = np.stack([-cam.screen_distance * one, zero, zero], axis=-1)
        d = np.stack([cam.screen_distance * one, (1.0 - 2 * u) * cam.aspect_ratio, 2 * v - 1], axis=-1)
    else:
        o = np.stack([-one, (1.0 - 2 * u) * cam.aspect_ratio, 2 * v - 1], axis=-1)
        d = np.stack([one, zero, zero], axis=-1)
    return o @ m[:, :3].T + m[:, 3], d @ m[:, :3].T


def wall_frame(camera, W, H, x_wall=3.0, split=None, colours=(0.5, 2.0)):
    """The hit frame of a wall, the plane x = ``x_wall`` with a normal of length 2 towards the camera, seen from ``camera``: shape 0
    where y < ``split`` and shape 1 beyond (``split=None``: one shape), coloured ``colours`` per shape; a miss where the ray
    leaves the wall behind -> (colour, shape, normal, point), ``[H, W, 3]`` and ``[H, W]``."""
    o, d = primary_rays(camera, W, H)
    with np.errstate(all="ignore"):
        t = (x_wall - o[..., 0]) / d[..., 0]
    hit = t > 0.0
    point = np.where(hit[..., None], o + np.where(hit, t, 0.0)[..., None] * d, 0.0)
    point[..., 0] = np.where(hit, x_wall, 0.0)
    shape = np.where(point[..., 1] < (INF if split is None else split), 0, 1).astype(np.int32)
    shape[~hit] = -1
    normal = np.where(hit[..., None], np.array([-2.0, 0.0, 0.0]), 0.0)
    colour = np.where((shape == 1)[..., None], colours[1], colours[0]) * np.ones(3)
    return colour, shape, normal, point


@pytest.mark.parametrize("kind", ["perspective", "orthogonal"])
def test_the_projection_inverts_the_camera(kind):
    """``camera.fire_ray(u, v).at(t)`` projects back onto the pixel it was fired through.

    The tolerance, for the inputs of this test (coordinates below 128, 1 <= t <= 50, aspect ratio >= 1): the point and the three rows
    of ``invm * point`` take at most 8 roundings of values below 128, an absolute error of at most 8 * 128 * 2^-53 = 2^-43 in camera
    space; the perspective scale ``s = d / tn = 1 / t`` is at most 1 and the division by ``a >= 1`` does not grow it, the factor 0.5
    halves it: 2^-44 in ``u`` and ``v``, plus the roundings of the five operations that follow on values near 1, below 2^-50.
    ``fx = u * W - 0.5`` scales that by W: |fx - col| <= W * 2^-43, |fy - row| <= H * 2^-43.  Measured on this mirror: at most
    6 * max(W, H) * 2^-52, an eightieth of the bound."""
    from pytracer_amd.tracer import GpuImageTracer

    rng = np.random.default_rng(7)
    worst = 0.0
    for W, H in ((1, 1), (37, 23), (640, 480), (1280, 720)):
        camera = cameras(aspect=max(1.0, W / H))[kind]
        tracer = GpuImageTracer(hm.HdrImage(W, H), camera)
        pixels = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(40)] + [(0, 0), (W - 1, H - 1), (0, H - 1), (W - 1, 0)]
        points = []
        for col, row in pixels:
            at = tracer.fire_ray(col, row).at(float(rng.uniform(1.0, 50.0)))
            points.append((at.x, at.y, at.z))
        assert np.abs(points).max() < 128.0
        fx, fy, ok = rb.temporal_project_host(camera, np.array(points), W, H)
        want = np.array(pixels, dtype=np.float64)
        assert ok.all()
        ex, ey = np.abs(fx - want[:, 0]).max(), np.abs(fy - want[:, 1]).max()
        worst = max(worst, ex / W, ey / H)
        assert ex <= W * 2.0 ** -43 and ey <= H * 2.0 ** -43, (W, H, ex, ey)
        # the numpy rays of this file are the tracer's
        o, d = primary_rays(camera, W, H)
        ray = tracer.fire_ray(W - 1, H // 2)
        assert np.allclose(o[H // 2, W - 1], (ray.origin.x, ray.origin.y, ray.origin.z), rtol=0, atol=1e-14)
        assert np.allclose(d[H // 2, W - 1], (ray.dir.x, ray.dir.y, ray.dir.z), rtol=0, atol=1e-14)
    print(f"{kind}: worst round-trip error {worst / 2.0 ** -52:.2f} * 2^-52 of the frame's size")


@pytest.mark.parametrize("kind", ["perspective", "orthogonal"])
def test_a_constant_power_of_two_is_kept_exactly_and_the_count_runs_to_max_history(kind):
    W, H, max_history = 23, 14, 5
    camera = cameras(aspect=W / H)[kind]
    colour, shape, normal, point = wall_frame(camera, W, H, colours=(0.5, 0.5))
    assert (shape >= 0).all()
    prev = rb.TemporalHistory.empty(W, H)
    for frame in range(1, max_history + 4):
        out, count = rb.temporal_host(colour, shape, normal, point, prev.colour, prev.shape_index, prev.normal, prev.point, prev.count, camera, W, H,
                                      max_history=max_history)
        assert _same(out, colour), frame  # 0.5 in every bit: (b * 0.5 summed) / (b summed) is 0.5 whatever the weights round to
        assert count.dtype == np.int32 and (count == min(frame, max_history)).all(), frame
        prev = rb.TemporalHistory(out, shape, normal, point, count)


def test_two_shapes_do_not_bleed_across_a_camera_step():
    W, H = 40, 12
    camera = cameras(aspect=W / H)["perspective"]
    moved = scenes.turned_camera(camera, 2.0)
    first = wall_frame(camera, W, H, split=-1.4)
    colour, shape, normal, point = wall_frame(moved, W, H, split=-1.4)
    assert {0, 1} <= set(np.unique(first[1])) and {0, 1} <= set(np.unique(shape))
    ones = np.ones((H, W), np.int32)
    out, count = rb.temporal_host(colour, shape, normal, point, first[0], first[1], first[2], first[3], ones, camera, W, H)
    assert _same(out, colour) and (count == 2).sum() > W * H // 2 and set(np.unique(count)) <= {0, 1, 2}
    # without PT_TA_SAME_SHAPE they do: one plane, one normal -- nothing else tells them apart
    bled, count2 = rb.temporal_host(colour, shape, normal, point, first[0], first[1], first[2], first[3], ones, camera, W, H, same_shape=False)
    changed = (bled != colour).any(axis=-1)
    assert changed.any() and (count2 >= count).all()
    border = np.zeros((H, W), bool)
    border[:, 1:] |= shape[:, 1:] != shape[:, :-1]
    border[:, :-1] |= shape[:, 1:] != shape[:, :-1]
    assert not (changed & ~border).any()  # (a pixel's four taps reach one pixel to either side of its old place)


def test_no_history_gives_the_colour_back_with_a_count_of_one():
    W, H = 16, 9
    camera = cameras(aspect=W / H)["perspective"]
    rng = np.random.default_rng(2)
    _, shape, normal, point = wall_frame(camera, W, H)
    colour, old = rng.uniform(0, 1, (H, W, 3)), rng.uniform(0, 1, (H, W, 3))
    ones = np.ones((H, W), np.int32)
    run = lambda pnt, cnt, cam=camera, **kw: rb.temporal_host(colour, shape, normal, pnt, old, shape, normal, point, cnt, cam, W, H, **kw)  # noqa: E731
    out, count = run(point, ones)
    assert (count == 2).all() and not (out == colour).all(axis=-1).any()  # (the control: with history every pixel is blended)
    # a prev_count of 0 (or below)
    for none in (0, -1, -2 ** 31):
        out, count = run(point, np.full((H, W), none, np.int32))
        assert _same(out, colour) and (count == 1).all(), none
    # a point behind the previous camera: tn = q.x + d is not positive
    behind = point.copy()
    behind[2, 3] = (-7.0, -2.0, 1.0)
    fx, fy, ok = rb.temporal_project_host(camera, behind, W, H)
    assert not ok[2, 3] and ok.sum() == W * H - 1
    out, count = run(behind, ones, point_tolerance=INF)
    assert _same(out[2, 3], colour[2, 3]) and count[2, 3] == 1 and (np.delete(count.reshape(-1), 2 * W + 3) == 2).all()
    # points in front of the previous camera that project off its screen, to either side and above
    away = point.copy()
    away[1, 2], away[1, 3], away[7, 0] = (3.0, 500.0, 0.0), (3.0, -500.0, 0.0), (3.0, 0.0, 500.0)
    fx, fy, ok = rb.temporal_project_host(camera, away, W, H)
    off = np.zeros((H, W), bool)
    off[1, 2], off[1, 3], off[7, 0] = True, True, True
    assert not ok[off].any() and ok[~off].all() and (fx[1, 2] < -1.0 or fx[1, 2] >= W) and (fy[7, 0] < -1.0)
    out, count = run(away, ones, point_tolerance=INF)
    assert _same(out[off], colour[off]) and (count[off] == 1).all() and (count[~off] == 2).all()
    # NaN dies at the screen test
    wild = point.copy()
    wild[4, 5] = (NAN, 0.0, 0.0)
    wild[4, 6] = (INF, 0.0, 0.0)
    out, count = run(wild, ones, point_tolerance=INF)
    assert _same(out[4, 5:7], colour[4, 5:7]) and (count[4, 5:7] == 1).all()


def test_miss_pixels_are_copied_and_never_read_and_nan_guides_only_skip_taps():
    W, H = 19, 11
    camera = cameras(aspect=W / H)["orthogonal"]
    moved = scenes.turned_camera(camera, 1.0)
    rng = np.random.default_rng(3)
    _, pshape, pnormal, ppoint = wall_frame(camera, W, H)
    _, shape, normal, point = wall_frame(moved, W, H)
    colour, old = rng.uniform(0, 1, (H, W, 3)), rng.uniform(0, 1, (H, W, 3))
    counts = rng.integers(1, 9, (H, W)).astype(np.int32)
    miss, pmiss = rng.uniform(0, 1, (H, W)) < 0.25, rng.uniform(0, 1, (H, W)) < 0.25
    shape, pshape = shape.copy(), pshape.copy()
    shape[miss] = rng.integers(-2 ** 31, 0, int(miss.sum()))
    pshape[pmiss] = rng.integers(-2 ** 31, 0, int(pmiss.sum()))
    out, count = rb.temporal_host(colour, shape, normal, point, old, pshape, pnormal, ppoint, counts, camera, W, H)
    assert _same(out[miss], colour[miss]) and (count[miss] == 0).all() and (count[~miss] >= 1).all() and np.isfinite(out).all()
    assert (count[~miss] >= 2).any() and (count[~miss] == 1).any()
    # whatever a miss holds -- in this frame or in the last -- changes no other pixel
    c2, n2, p2, o2, pn2, pp2 = colour.copy(), normal.copy(), point.copy(), old.copy(), pnormal.copy(), ppoint.copy()
    c2[miss], n2[miss], p2[miss] = NAN, 0.0, INF
    o2[pmiss], pn2[pmiss], pp2[pmiss] = NAN, NAN, -INF
    again, count2 = rb.temporal_host(c2, shape, n2, p2, o2, pshape, pn2, pp2, counts, camera, W, H)
    assert _same(again[~miss], out[~miss]) and np.isnan(again[miss]).all() and _same(count2, count)
    # NaN guides only ever skip taps: a pixel whose own normal is NaN keeps its colour with a count of 1, and a NaN normal or point
    # in the history is a tap less for its neighbours, never a NaN in the output
    hit = np.flatnonzero(~miss.reshape(-1))
    n3 = normal.copy()
    n3.reshape(-1, 3)[hit[5]] = NAN
    pn3, pp3 = pnormal.copy(), ppoint.copy()
    pn3[3, 4], pp3[6, 7], pn3[2, 9] = NAN, (0.0, INF, 0.0), 0.0
    out3, count3 = rb.temporal_host(colour, shape, n3, point, old, pshape, pn3, pp3, counts, camera, W, H)
    assert np.isfinite(out3).all() and _same(out3.reshape(-1, 3)[hit[5]], colour.reshape(-1, 3)[hit[5]]) and count3.reshape(-1)[hit[5]] == 1
    assert (count3 <= count).all() and (out3 != out).any()
    # a non-finite colour propagates as the arithmetic says: from the history into the pixels that read it
    o4 = old.copy()
    o4[5, 5] = INF
    out4, _ = rb.temporal_host(colour, shape, normal, point, o4, pshape, pnormal, ppoint, counts, camera, W, H)
    assert (pshape[5, 5] < 0) or not np.isfinite(out4).all()


def test_the_mirror_refuses_what_the_library_refuses_and_depends_on_the_tap_order():
    W, H = 31, 17
    camera = cameras(aspect=W / H)["perspective"]
    moved = scenes.turned_camera(camera, 0.7)
    rng = np.random.default_rng(5)
    _, pshape, pnormal, ppoint = wall_frame(camera, W, H)
    _, shape, normal, point = wall_frame(moved, W, H)
    colour, old = rng.uniform(0, 1, (H, W, 3)), rng.uniform(0, 1, (H, W, 3))
    ones = np.ones((H, W), np.int32)
    run = lambda **kw: rb.temporal_host(colour, shape, normal, point, old, pshape, pnormal, ppoint, ones, camera, W, H, **kw)  # noqa: E731
    for kw in (dict(max_history=0), dict(max_history=2 ** 20 + 1), dict(normal_min=1.5), dict(normal_min=NAN), dict(point_tolerance=0.0),
               dict(point_tolerance=NAN), dict(point_tolerance=-INF)):
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError, match="camera kind"):
        rb.temporal_host(colour, shape, normal, point, old, pshape, pnormal, ppoint, ones, (5, IDENTITY12, 1.0, 1.0), W, H)
    empty = np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3))
    out, count = rb.temporal_host(*empty, *empty, np.zeros(0, np.int32), camera, 0, 4)
    assert out.shape == (4, 0, 3) and count.shape == (4, 0) and count.dtype == np.int32
    # the discriminating power of the GPU's bit tests: summing the four taps from the last to the first changes bits
    got, count = run()
    back, count_back = run(_tap_order=(3, 2, 1, 0))
    four = count == 2
    changed = (got.view(np.uint64) != back.view(np.uint64)).any(axis=-1)
    print(f"{W}x{H}: the reverse tap order changes {changed[four].mean():.1%} of the pixels with history")
    assert _same(count, count_back) and four.mean() > 0.8 and changed[four].mean() > 0.2 and np.abs(got - back).max() <= 8 * 2.0 ** -52
    # max_history = 1 is no accumulation at all (alpha = 1): hist + (colour - hist) is the colour to within a rounding
    alone, one = run(max_history=1)
    assert (one == 1).all() and np.abs(alone - colour).max() <= 2.0 ** -52


def test_what_reaches_the_device_scene_without_a_device():
    """``WorldQueries.accumulated`` hands the frame, the history and the camera to ``DeviceScene.temporal`` and wraps what comes back;
    ``TemporalAccumulator`` starts from lengths of zero, chains the histories and remembers the camera of the frame before; the
    shader asks for gather, accumulation, filter and materials in that order, with fresh generators every frame."""
    from types import SimpleNamespace

    from pytracer_amd import _temporal_lib, shaders

    seen = []
    H, W = 3, 4

    class Scene:
        device = 0

        def temporal(self, colour, shape_index, normal, point, prev_colour, prev_shape, prev_normal, prev_point, prev_count, prev_camera, width,
                     height, **params):
            seen.append(SimpleNamespace(colour=colour, shape=shape_index, normal=normal, point=point, prev_colour=prev_colour, prev_shape=prev_shape,
                                        prev_normal=prev_normal, prev_point=prev_point, prev_count=prev_count, camera=prev_camera,
                                        size=(width, height), params=params))
            return np.asarray(colour).reshape(height, width, 3) + 1.0, np.asarray(prev_count).reshape(height, width) + 1

    wq = rb.WorldQueries(Scene())
    frame = SimpleNamespace(shape_index=np.zeros((1, H, W), np.int32), point=np.zeros((1, H, W, 3)), normal=np.ones((1, H, W, 3)))
    values = np.arange(H * W * 3.0).reshape(H, W, 3)
    cam_a, cam_b = cameras()["perspective"], cameras()["orthogonal"]
    new = wq.accumulated(values, frame, rb.TemporalHistory.empty(W, H), cam_a, max_history=7)
    assert isinstance(new, rb.TemporalHistory) and np.array_equal(new.colour, values + 1.0) and (new.count == 1).all()
    assert new.shape_index.shape == (H, W) and new.normal.shape == (H, W, 3) and new.point.shape == (H, W, 3)
    call = seen[-1]
    assert call.size == (W, H) and call.params == dict(max_history=7) and call.camera is cam_a
    assert call.colour.shape == (H * W, 3) and call.shape.shape == (H * W,) and call.prev_count.shape == (H * W,) and call.prev_colour.shape == (H * W, 3)
    gathered = rb.GatheredRadiance(np.zeros(rb.gather_bytes(H * W, 0), np.uint8), H * W, 0, shape=(1, H, W))
    assert wq.accumulated(gathered, frame, new, cam_b).colour.shape == (H, W, 3) and seen[-1].prev_count.tolist() == [1] * (H * W)
    many = SimpleNamespace(shape_index=np.zeros((4, H, W), np.int32), point=np.zeros((4, H, W, 3)), normal=np.ones((4, H, W, 3)))
    with pytest.raises(ValueError, match="samples per pixel"):
        wq.accumulated(values, many, new, cam_a)
    with pytest.raises(ValueError, match="history"):
        wq.accumulated(values, frame, rb.TemporalHistory.empty(W + 1, H), cam_a)
    # the camera struct of both kinds
    flat = _temporal_lib.camera(cam_a)
    assert flat.kind == abi.CAMERA_PERSPECTIVE and flat.screen_distance == 1.25 and flat.aspect_ratio == 1.0
    assert list(flat.invm) == [x for row in cam_a.transformation.invm[:3] for x in row]
    flat = _temporal_lib.camera(cam_b)
    assert flat.kind == abi.CAMERA_ORTHOGONAL and flat.screen_distance == 1.0 and _temporal_lib.camera(flat) is flat
    # the accumulator
    del seen[:]
    acc = rb.TemporalAccumulator(wq, max_history=3, normal_min=0.5)
    assert acc.count is None and acc.frames == 0
    first = acc.update(values, frame, cam_a)
    assert np.array_equal(first, values + 1.0) and (acc.count == 1).all() and acc.frames == 1
    assert not seen[0].prev_count.any() and seen[0].params == dict(max_history=3, normal_min=0.5)  # (it starts from lengths of zero)
    assert list(seen[0].camera.invm) == list(_temporal_lib.camera(cam_a).invm)  # (nothing of it is read: the frame's own)
    second = acc.update(values * 2.0, frame, cam_b)
    assert np.array_equal(seen[1].prev_colour.reshape(H, W, 3), first) and seen[1].prev_count.tolist() == [1] * (H * W) and (acc.count == 2).all()
    assert seen[1].camera.kind == abi.CAMERA_PERSPECTIVE and np.array_equal(second, values * 2.0 + 1.0)  # (the camera of the frame BEFORE)
    acc.update(values, frame, cam_a)
    assert seen[2].camera.kind == abi.CAMERA_ORTHOGONAL and (acc.count == 3).all()
    acc.reset()
    assert acc.count is None and acc.frames == 0
    acc.update(values, frame, cam_a)
    assert not seen[3].prev_count.any()
    with pytest.raises(TypeError, match="unknown accumulation parameter"):
        rb.TemporalAccumulator(wq, passes=3)
    with pytest.raises(ValueError, match="device=True"):
        rb.TemporalAccumulator(wq, stream=1)
    with pytest.raises(ValueError, match="device=True"):
        acc.update(values, frame, cam_a, width=W, height=H)
    with pytest.raises(ValueError, match="width= and height="):
        rb.TemporalAccumulator(wq, device=True).update(0, rb.DeviceGuides(0, 0, 0), cam_a)
    with pytest.raises(TypeError, match="DeviceGuides"):
        rb.TemporalAccumulator(wq, device=True).update(0, frame, cam_a, width=W, height=H)
    # the shader
    world = hm.World()
    order = []
    scene = Scene()

    class Queries:
        def __init__(self):
            self.scene = scene

        def hemisphere_radiance(self, hits, samples, *a, **kw):
            order.append(("gather", samples, a, kw))
            return gathered

        def accumulated(self, values, hits, prev, prev_camera, **params):
            order.append(("accumulate", params, np.array(prev.count), prev_camera))
            return rb.TemporalHistory(np.asarray(values) + 1.0, hits.shape_index[0], hits.normal[0], hits.point[0], np.asarray(prev.count) + 1)

        def denoised(self, values, hits, **params):
            order.append(("filter", params, np.array(values)))
            return np.asarray(values) * 2.0

        def materials(self, hits):
            order.append(("materials",))
            hit = np.ones((1, H, W), bool)
            hit[0, 0, 0] = False
            return SimpleNamespace(emitted=np.full((1, H, W, 3), 0.5), brdf_color=np.full((1, H, W, 3), 0.25), hit=hit)

    tracer = SimpleNamespace(world_queries=lambda w: Queries() if w is world else None, camera=cam_a)
    shader = shaders.TemporalGatherShader(world, tracer, samples=4, init_seq=54, background_color=hm.Color(7.0, 8.0, 9.0), passes=2, sigma_point=0.5,
                                          max_history=9, history_same_shape=False)
    assert shader.params == dict(passes=2, sigma_point=0.5) and shader.history_params == dict(max_history=9, same_shape=False)
    out = shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "accumulate", "filter", "materials"] and order[0][1] == 4 and order[0][3]["init_seq"] == 54
    assert order[1][1] == dict(max_history=9, same_shape=False) and not order[1][2].any() and order[2][1] == dict(passes=2, sigma_point=0.5)
    assert (order[2][2] == 1.0).all()  # the filter sees the accumulated mean (the gather's zeros + 1)
    assert out.shape == (1, H, W, 3) and out[0, 0, 0].tolist() == [7.0, 8.0, 9.0] and np.all(out[0, 1:] == 0.5 + 0.25 * 2.0)
    assert shader.frame_no == 1 and (shader.accumulator.count == 1).all()
    tracer.camera = cam_b
    del order[:]
    shader.shade_hits(frame)
    assert order[0][3]["init_seq"] == 54 + 1 * (H * W) * 4 and (order[1][2] == 1).all() and order[1][3].kind == abi.CAMERA_PERSPECTIVE
    assert shader.frame_no == 2 and (shader.accumulator.count == 2).all()
    # without accumulation: the same frame number's generators, the history and the frame number left alone
    shader.accumulate, shader.filtered = False, False
    del order[:]
    noisy = shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "materials"] and order[0][3]["init_seq"] == 54 + 2 * (H * W) * 4 and np.all(noisy[0, 1:] == 0.5)
    assert shader.frame_no == 2 and (shader.accumulator.count == 2).all()
    shader.accumulate = True
    del order[:]
    shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "accumulate", "materials"] and order[0][3]["init_seq"] == 54 + 2 * (H * W) * 4
    assert order[1][3].kind == abi.CAMERA_ORTHOGONAL and shader.frame_no == 3
    shader.reset()
    del order[:]
    shader.shade_hits(frame)
    assert shader.frame_no == 1 and order[0][3]["init_seq"] == 54 and not order[1][2].any()
    with pytest.raises(ValueError, match="one record per pixel"):
        shader.shade_hits(many)
    with pytest.raises(TypeError, match="tracer"):
        shaders.TemporalGatherShader(world).shade_hits(frame)
    with pytest.raises(TypeError, match="ray_intersection"):
        shaders.TemporalGatherShader(world)(None)
    for bad in (dict(wrap_x=True), dict(history=3), dict(flags=1)):
        with pytest.raises(TypeError, match="unknown filter or accumulation parameter"):
            shaders.TemporalGatherShader(world, tracer, **bad)
    with pytest.raises(ValueError, match="samples"):
        shaders.TemporalGatherShader(world, tracer, samples=0)
