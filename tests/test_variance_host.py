"""CPU-only tests of the variance queries (include/ptrace_variance.h, libptrace_variance.so, pytracer_amd.rays): the twelfth library
builds and loads without a GPU and leaves the other eleven as they were; its header, the ctypes table and its dynamic symbols agree;
every refusal of the interface happens before any HIP call; each numpy mirror the GPU's bit tests compare with equals a second, plain
scalar-loop implementation written from the header alone, bit for bit, on hostile frames; and the mirrors have the properties of what
they define -- the parent's filter where the luminance weight is off, exact running moments through the unchanged accumulation, an
unbiased variance of Gaussian noise on both branches of the estimate, and a filter that leaves a noiseless constant alone."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import rays as rb

from . import hostile_records as H
from .test_temporal_host import cameras, wall_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_SIZE, ERR_NODEVICE = -1, -5, -6  # include/ptrace.h
V110 = (1 << 16) | 10
INF, NAN = float("inf"), float("nan")
FLAGS = [(True, False), (True, True), (False, False), (False, True)]  # (same_shape, wrap_x)


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _variance_lib, build

    build.build()
    assert os.path.exists(build.VARIANCE_LIB) and not build.needs_build()
    return _variance_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _variance_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_variance.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_variance_lib.EXPORTS) == {s for s, _, _ in _variance_lib._SIGNATURES} and len(declared) == 11
    assert all(s.startswith("pt_rays_variance_") for s in declared)
    assert _exported(_variance_lib.lib_path()) == declared
    assert lib.pt_rays_variance_version() == V110
    # an add-on like the eleven before it: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _variance_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_variance.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _variance_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    # the only file that includes the new device header is the new translation unit; the host layer is the shared one
    users = [f for f in os.listdir(build.CSRC) if '"pt_variance.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_variance.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_variance.hip")).read() + open(os.path.join(build.CSRC, "pt_variance.h")).read()
    assert '#include "pt_host_common.h"' in text and not re.search(r"\bg_err\b|\bstruct\s+Staged\b|#\s*define\s+HIP_TRY\b", text)
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text)  # (no atomic of any kind is called)
    for word in ("PTRACE_VR_TILE", "PTRACE_VR_VARIANT", "PTRACE_VR_BLOCKS"):
        assert word in text, word
    # the header names the two it builds on as files, and none of their symbols (the other headers' tests search for those)
    assert "ptrace_temporal.h" in header and "ptrace_denoise.h" in header
    assert "pt_rays_temporal" not in header and "pt_rays_denoise" not in header
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ptrace_variance.h":
            assert "pt_rays_variance" not in open(os.path.join(ROOT, "include", other)).read(), other
    # pt_variance_params: four ints and five doubles
    assert C.sizeof(_variance_lib.VarianceParams) == 56
    assert [f[0] for f in _variance_lib.VarianceParams._fields_] == re.findall(r"^\s+(?:int|double)\s+(\w+);", header, flags=re.M)
    assert _variance_lib.VR_SAME_SHAPE == int(re.search(r"#define PT_VR_SAME_SHAPE\s+(\d+)", header).group(1)) == 1
    assert _variance_lib.VR_WRAP_X == int(re.search(r"#define PT_VR_WRAP_X\s+(\d+)", header).group(1)) == 2
    assert _variance_lib.MAX_HISTORY == int(re.search(r"#define PT_VR_MAX_HISTORY\s+(\d+)", header).group(1)) == 2 ** 20
    assert _variance_lib.DEFAULTS == dict(passes=4, sigma_point=0.1, normal_power_log2=5, sigma_luminance=1.0, epsilon=1e-10, min_history=4,
                                          normal_min=0.9, point_tolerance=0.05, same_shape=True, wrap_x=False)
    par = _variance_lib.params()
    assert {k: getattr(par, k) for k in ("passes", "sigma_point", "normal_power_log2", "sigma_luminance", "epsilon", "min_history", "normal_min",
                                         "point_tolerance")} == {k: v for k, v in _variance_lib.DEFAULTS.items() if k not in ("same_shape", "wrap_x")}
    assert par.flags == 1
    for word in ("bit for bit", "NON-FINITE COLOURS AND VARIANCES", "lum = (mx + mn) / 2.0", "out = (l, l * l, +0.0)", "v = mu2 - mu1 * mu1",
                 "if (!(v > 0)) v = 0.0", "variance = v / (double)n", "mean = s1 / k;  v = s2 / k - mean * mean", "A CHOICE",
                 "ACCUMULATED MEAN", "left nearly\n * unfiltered", "g = gw > 0 ? gs / gw : 0.0", "den_p = sl2 * g_p + epsilon",
                 "wl = 1.0 / (1.0 + (dl * dl) / den_p)", "w  = ((k * c) * wp) * wl", "vs = vs + (w * w) * var_q",
                 "out_variance = vs / (wsum * wsum)", "24 m (unit normals) + 8 m (g) + 32 m", "No bit depends on the launch shape"):
        assert word in header, word


def test_the_pinned_build_tables_are_unchanged_and_the_new_row_is_in_its_own(lib):
    from pytracer_amd import build

    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_variance.h")), "ptrace_variance.hip", "pt_variance.h"} <= deps
    assert [len(t) for t in (build.TARGETS, build.ALL_TARGETS, build.EVERY_TARGET, build.BUILD_TARGETS, build.WALK_TARGETS, build.FRAME_TARGETS,
                             build.GUIDED_TARGETS)] == [6, 7, 8, 9, 10, 11, 12]
    assert build.FRAME_TARGETS == build.WALK_TARGETS + ((build.TEMPORAL_FLAGS, build.TEMPORAL_LIB, build.TEMPORAL_SOURCES),)
    assert list(build.TEMPORAL_ADDONS) == ["temporal"] and list(build.VARIANCE_ADDONS) == ["variance"]
    assert build.VARIANCE_TARGETS == ((build.VARIANCE_FLAGS, build.VARIANCE_LIB, build.VARIANCE_SOURCES),)
    assert build.GUIDED_TARGETS == build.FRAME_TARGETS + build.VARIANCE_TARGETS
    assert build.VARIANCE_FLAGS[:-1] == build.FLAGS[:-1] and build.VARIANCE_FLAGS[-1] == "-cuid=libptrace_variance"
    assert "-ffp-contract=off" in build.VARIANCE_FLAGS and not any("fast-math" in f and not f.startswith("-fno") for f in build.VARIANCE_FLAGS)
    assert build.VARIANCE_SOURCES == ["ptrace_variance.hip"] and os.path.basename(build.VARIANCE_LIB) == "libptrace_variance.so"
    assert all(os.path.exists(t[1]) for t in build.GUIDED_TARGETS)  # build() made all twelve


def test_the_other_eleven_libraries_are_what_they_were(lib):
    from pytracer_amd import _denoise_lib, _temporal_lib, build

    assert _exported(_temporal_lib.lib_path()) == set(_temporal_lib.EXPORTS) and _exported(_denoise_lib.lib_path()) == set(_denoise_lib.EXPORTS)
    # the recorded hashes: eleven rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "variance_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.FRAME_TARGETS] and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.FRAME_TARGETS]
    # and the ten the temporal library recorded are still those
    old = [line.split() for line in open(os.path.join(ROOT, "profiles", "temporal_hashes.txt")) if line.startswith("libptrace")]
    assert [r[:3] for r in rows[:10]] == [r[:3] for r in old[:10]]
    # none of the other libraries' kernels is compiled into the new one, and none of its into theirs
    text = open(os.path.join(build.CSRC, "ptrace_variance.hip")).read()
    assert set(re.findall(r'#include "(pt_\w+\.h)"', text)) == {"pt_kernels.h", "pt_variance.h", "pt_host_common.h"}


def test_sizes(lib):
    from pytracer_amd import _variance_lib

    for m in (0, 1, 63, 65, 2 ** 31 - 1):
        assert lib.pt_rays_variance_bytes(m) == 24 * m and lib.pt_rays_variance_plane_bytes(m) == 8 * m
    for m in (-1, 2 ** 31):
        assert lib.pt_rays_variance_bytes(m) == 0 and lib.pt_rays_variance_plane_bytes(m) == 0
    ws = lambda w, h, **kw: lib.pt_rays_variance_workspace_bytes(w, h, C.byref(_variance_lib.params(**kw)))  # noqa: E731
    assert ws(7, 5, passes=1) == 32 * 35 and ws(7, 5, passes=2) == 64 * 35 and ws(7, 5, passes=10) == 64 * 35 and ws(0, 5) == 0
    assert ws(7, 5, passes=0) == 0 and "passes" in _variance_lib.last_error()
    assert ws(-1, 5) == 0 and lib.pt_rays_variance_workspace_bytes(7, 5, None) == 0 and "null pt_variance_params" in _variance_lib.last_error()


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
NOWHERE = 2 ** 20  # a device no machine has: a call that passes every argument check ends at the device check, with or without a GPU


def test_every_refusal_happens_before_any_hip_call(lib):
    """Every call names a device that does not exist, so nothing is ever launched: a call that passes the argument checks ends at the
    first HIP call, the device check (PT_ERR_NODEVICE without a GPU, "out of range" with one); whatever is refused otherwise was
    refused by the argument checks before it."""
    from pytracer_amd import _variance_lib

    err = _variance_lib.last_error

    def passed(rc):
        return rc == ERR_NODEVICE or (rc == ERR_INVALID and "out of range" in err())

    W, Hh = 5, 3
    m = W * Hh
    f3, f1, i1 = (lambda: np.zeros((3, m))), (lambda: np.zeros(m)), (lambda: np.zeros(m, np.int32))
    planes = dict(c=f3(), v=f1(), n=f3() + 1.0, pt=f3(), s=i1(), mom=f3(), k=i1() + 1)
    oc, ov, om = f3(), f1(), f3()
    work = np.zeros(8 * m)

    def nbytes(a, given):
        return (a.nbytes if a is not None else 0) if given is None else given

    def filt(device=NOWHERE, w=W, h=Hh, par=True, o=oc, ob=None, o2=ov, o2b=None, ws=work, wsb=None, **kw):
        a = {name: kw.pop(name, planes[name]) for name in ("c", "v", "n", "pt", "s")}
        par = C.byref(_variance_lib.params(**kw)) if par else None
        args = [device, w, h, par] + [p(a[name]) for name in ("c", "v", "n", "pt", "s")] + [p(o), nbytes(o, ob), p(o2), nbytes(o2, o2b)]
        return lib.pt_rays_variance_filter(*args), lib.pt_rays_variance_filter_device(*args, p(ws), nbytes(ws, wsb), None)

    def est(device=NOWHERE, w=W, h=Hh, par=True, o=ov, ob=None, **kw):
        a = {name: kw.pop(name, planes[name]) for name in ("mom", "k", "s", "n", "pt")}
        par = C.byref(_variance_lib.params(**kw)) if par else None
        args = [device, w, h, par] + [p(a[name]) for name in ("mom", "k", "s", "n", "pt")] + [p(o), nbytes(o, ob)]
        return lib.pt_rays_variance_estimate(*args), lib.pt_rays_variance_estimate_device(*args, None)

    def mom(device=NOWHERE, w=W, h=Hh, o=om, ob=None, c=planes["c"], s=planes["s"]):
        args = [device, w, h, p(c), p(s), p(o), nbytes(o, ob)]
        return lib.pt_rays_variance_moments(*args), lib.pt_rays_variance_moments_device(*args, None)

    assert all(passed(rc) for rc in filt()) and all(passed(rc) for rc in est()) and all(passed(rc) for rc in mom())
    legal = (dict(passes=10, normal_power_log2=10, flags=3, min_history=2 ** 20, sigma_point=INF, sigma_luminance=INF, epsilon=1e300,
                  normal_min=-1.0, point_tolerance=INF),
             dict(passes=1, normal_power_log2=0, flags=0, min_history=1, sigma_point=5e-324, sigma_luminance=5e-324, epsilon=5e-324,
                  normal_min=1.0, point_tolerance=5e-324))
    for kw in legal:
        assert all(passed(rc) for rc in filt(**kw)) and all(passed(rc) for rc in est(**kw)), kw
    # a passes = 1 filter needs half the workspace
    assert all(passed(rc) for rc in filt(passes=1, wsb=32 * m)) and filt(passes=2, wsb=64 * m - 1)[1] == ERR_SIZE
    for call in (filt, est, mom):
        assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
        assert call(w=46341, h=46341, ob=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in err()
        assert call(w=2 ** 31 - 1, h=2, ob=2 ** 40) == both(ERR_INVALID)
        assert call(device=-1) == both(ERR_INVALID)
    for call in (filt, est):
        assert call(par=False) == both(ERR_INVALID) and "null pt_variance_params" in err()
        for passes in (0, -1, 11, 2 ** 31 - 1):
            assert call(passes=passes) == both(ERR_INVALID) and "passes" in err(), passes
        for e in (-1, 11):
            assert call(normal_power_log2=e) == both(ERR_INVALID) and "normal_power_log2" in err(), e
        for h in (0, -1, 2 ** 20 + 1, 2 ** 31 - 1):
            assert call(min_history=h) == both(ERR_INVALID) and "min_history" in err(), h
        for name in ("sigma_point", "sigma_luminance", "point_tolerance"):
            for bad in (0.0, -0.0, -1.0, -INF, NAN):
                assert call(**{name: bad}) == both(ERR_INVALID) and name in err(), (name, bad)
        for bad in (0.0, -0.0, -1e-10, INF, -INF, NAN):
            assert call(epsilon=bad) == both(ERR_INVALID) and "epsilon" in err(), bad
        for bad in (-1.0000000000000002, 1.0000000000000002, INF, -INF, NAN):
            assert call(normal_min=bad) == both(ERR_INVALID) and "normal_min" in err(), bad
        for flags in (4, 8, -1, 1 << 30):
            assert call(flags=flags) == both(ERR_INVALID) and "flag" in err(), flags
    # NULL where a buffer is needed
    for name in ("c", "v", "n", "pt", "s"):
        assert filt(**{name: None}) == both(ERR_INVALID) and "null" in err() and "planes" in err(), name
    for name in ("mom", "k", "s", "n", "pt"):
        assert est(**{name: None}) == both(ERR_INVALID) and "null" in err() and "planes" in err(), name
    assert mom(c=None) == both(ERR_INVALID) and mom(s=None) == both(ERR_INVALID) and "null" in err()
    assert filt(o=None, ob=oc.nbytes) == both(ERR_INVALID) and "null output" in err()
    assert filt(o2=None, o2b=ov.nbytes) == both(ERR_INVALID) and "null output" in err()
    assert est(o=None, ob=ov.nbytes) == both(ERR_INVALID) and mom(o=None, ob=om.nbytes) == both(ERR_INVALID) and "null output" in err()
    rc = filt(ws=None, wsb=work.nbytes)
    assert passed(rc[0]) and rc[1] == ERR_INVALID and "null workspace" in err()  # (the host form makes its own)
    # any output overlapping an input, the other output or the workspace: wholly, or by one value at either end
    big = np.zeros(16 * m + 2)
    whole3, whole1, ints = big[:3 * m].reshape(3, m), big[:m], big[:m].view(np.int32)[:m]
    for name in ("c", "n", "pt"):
        assert filt(o=planes[name]) == both(ERR_INVALID) and "the colour output overlaps" in err(), name
        for off in (1, 3 * m - 1):
            assert filt(o=big[off:off + 3 * m].reshape(3, m), **{name: whole3}) == both(ERR_INVALID), (name, off)
        assert all(passed(rc) for rc in filt(o=big[3 * m:6 * m].reshape(3, m), **{name: whole3})), name  # (adjacent is not overlapping)
        assert filt(o2=whole1, **{name: whole3}) == both(ERR_INVALID) and "the variance output overlaps" in err(), name
        assert filt(ws=big[3 * m - 1:11 * m - 1], **{name: whole3})[1] == ERR_INVALID and "the workspace overlaps" in err(), name
    assert filt(o2=planes["v"]) == both(ERR_INVALID) and "the variance output overlaps the variance plane" in err()
    assert filt(o=whole3, v=big[3 * m - 1:4 * m - 1]) == both(ERR_INVALID) and filt(o=whole3, s=ints) == both(ERR_INVALID)
    assert filt(o2=whole1, s=ints) == both(ERR_INVALID) and "the shapes" in err()
    assert filt(o=whole3, o2=big[3 * m - 1:4 * m - 1]) == both(ERR_INVALID) and "the colour output overlaps the variance output" in err()
    assert filt(o=whole3, ws=big[3 * m - 1:11 * m - 1])[1] == ERR_INVALID and "the colour output overlaps the workspace" in err()
    assert filt(o2=big[8 * m - 1:9 * m - 1], ws=big[:8 * m])[1] == ERR_INVALID and "the variance output overlaps the workspace" in err()
    assert all(passed(rc) for rc in filt(o=big[8 * m:11 * m].reshape(3, m), o2=big[11 * m:12 * m], ws=big[:8 * m]))
    for name in ("mom", "n", "pt"):
        assert est(o=whole1, **{name: whole3}) == both(ERR_INVALID) and "the variance output overlaps" in err(), name
        assert est(o=big[3 * m - 1:4 * m - 1], **{name: whole3}) == both(ERR_INVALID), name
        assert all(passed(rc) for rc in est(o=big[3 * m:4 * m], **{name: whole3})), name
    for name in ("k", "s"):
        assert est(o=whole1, **{name: ints}) == both(ERR_INVALID), name
    assert mom(o=planes["c"]) == both(ERR_INVALID) and "the moments output overlaps the colour planes" in err()
    assert mom(o=whole3, s=ints) == both(ERR_INVALID) and mom(o=big[1:3 * m + 1].reshape(3, m), c=whole3) == both(ERR_INVALID)
    # too small
    assert filt(ob=oc.nbytes - 1) == both(ERR_SIZE) and "colour output too small" in err()
    assert filt(o2b=ov.nbytes - 1) == both(ERR_SIZE) and "variance output too small" in err()
    assert filt(wsb=work.nbytes - 1)[1] == ERR_SIZE and "workspace too small" in err()
    assert est(ob=ov.nbytes - 1) == both(ERR_SIZE) and "variance output too small" in err()
    assert mom(ob=om.nbytes - 1) == both(ERR_SIZE) and "moments output too small" in err()
    # a launch alternative nobody knows is refused too, before any HIP call
    for name, values in (("PTRACE_VR_BLOCKS", ("0", "many", "-3", "2x")), ("PTRACE_VR_TILE", ("8x8", "16", "")), ("PTRACE_VR_VARIANT", ("LDS", "fast"))):
        for value in values:
            os.environ[name] = value
            try:
                assert filt() == both(ERR_INVALID) and name in err(), (name, value)
                assert est() == both(ERR_INVALID) and mom() == both(ERR_INVALID)
            finally:
                del os.environ[name]
    # m = 0: PT_OK, nothing launched, no buffer needed -- but the struct is still checked
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert filt(w=w, h=h, o=None, o2=None, ws=None, c=None, v=None, n=None, pt=None, s=None) == both(0), (w, h)
        assert est(w=w, h=h, o=None, mom=None, k=None, s=None, n=None, pt=None) == both(0) and mom(w=w, h=h, o=None, c=None, s=None) == both(0)
    assert filt(w=0, h=0, passes=0) == both(ERR_INVALID) and est(w=0, h=0, epsilon=INF) == both(ERR_INVALID)
    assert filt(w=0, h=0, par=False) == both(ERR_INVALID) and est(w=0, h=0, flags=4) == both(ERR_INVALID)
    assert not oc.any() and not ov.any() and not om.any() and not work.any()


# ---- the mirrors against plain scalar loops written from the header ---------------------------------------------------------------------
def _div(a, b):
    """a / b in IEEE arithmetic (Python raises where the hardware returns inf or NaN)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else NAN  # (NaN compares false)


def _lum(c):
    mx = c[0]
    if c[1] > mx:
        mx = c[1]
    if c[2] > mx:
        mx = c[2]
    mn = c[0]
    if c[1] < mn:
        mn = c[1]
    if c[2] < mn:
        mn = c[2]
    return (mx + mn) / 2.0


def _nh(a):
    length = _sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return (_div(a[0], length), _div(a[1], length), _div(a[2], length))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _lists(W, Hh, *arrays):
    out = []
    for a, width in arrays:
        a = np.asarray(a)
        out.append(a.reshape(Hh * W, width).tolist() if width else a.reshape(Hh * W).tolist())
    return out


def moments_loops(colour, shape, W, Hh):
    colour, shape = _lists(W, Hh, (colour, 3), (shape, 0))
    out = np.zeros((Hh * W, 3))
    for r in range(W * Hh):
        if shape[r] >= 0:
            l = _lum(colour[r])
            out[r] = (l, l * l, 0.0)
    return out.reshape(Hh, W, 3)


def estimate_loops(moments, count, shape, normal, point, W, Hh, min_history=4, normal_min=0.9, point_tolerance=0.05, same_shape=True,
                   wrap_x=False, **_):
    moments, count, shape, normal, point = _lists(W, Hh, (moments, 3), (count, 0), (shape, 0), (normal, 3), (point, 3))
    out = np.zeros(Hh * W)
    for y in range(Hh):
        for x in range(W):
            r = y * W + x
            n = count[r]
            if shape[r] < 0 or n < 1:
                continue
            if n >= min_history:
                v = moments[r][1] - moments[r][0] * moments[r][0]
            else:
                np_ = _nh(normal[r])
                s1, s2, k = 0.0, 0.0, 0.0
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        qx, qy = x + dx, y + dy
                        if wrap_x:
                            qx %= W
                        if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                            continue
                        q = qy * W + qx
                        if dx != 0 or dy != 0:
                            if shape[q] < 0 or (same_shape and shape[q] != shape[r]) or count[q] < 1:
                                continue
                            if not _dot(np_, _nh(normal[q])) >= normal_min:
                                continue
                            if not abs(_dot(np_, _sub(point[q], point[r]))) <= point_tolerance:
                                continue
                        s1, s2, k = s1 + moments[q][0], s2 + moments[q][1], k + 1.0
                mean = _div(s1, k)
                v = _div(s2, k) - mean * mean
            if not v > 0:
                v = 0.0
            out[r] = v / float(n)
    return out.reshape(Hh, W)


H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
G3 = (1 / 4, 1 / 2, 1 / 4)


def filter_loops(colour, variance, shape, normal, point, W, Hh, passes=4, sigma_point=0.1, normal_power_log2=5, sigma_luminance=1.0,
                 epsilon=1e-10, same_shape=True, wrap_x=False, **_):
    cur, var, shape, normal, point = _lists(W, Hh, (colour, 3), (variance, 0), (shape, 0), (normal, 3), (point, 3))
    unit = [_nh(a) for a in normal]
    sl2 = sigma_luminance * sigma_luminance

    def column(qx):
        return qx % W if wrap_x else qx

    for i in range(passes):
        s = 2 ** i
        sps = sigma_point * float(s)
        lum = [_lum(c) for c in cur]
        new, new_var = [list(c) for c in cur], list(var)
        for y in range(Hh):
            for x in range(W):
                r = y * W + x
                if shape[r] < 0:
                    continue
                gs, gw = 0.0, 0.0
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        qx, qy = column(x + dx), y + dy
                        if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                            continue
                        q = qy * W + qx
                        if shape[q] < 0 or (same_shape and shape[q] != shape[r]) or not var[q] >= 0:
                            continue
                        kw = G3[dx + 1] * G3[dy + 1]
                        gs, gw = gs + kw * var[q], gw + kw
                g = gs / gw if gw > 0 else 0.0
                den = sl2 * g + epsilon
                total, wsum, vs = [0.0, 0.0, 0.0], 0.0, 0.0
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        k = H5[dx + 2] * H5[dy + 2]
                        if dx == 0 and dy == 0:
                            w, q = k, r
                        else:
                            qx, qy = column(x + s * dx), y + s * dy
                            if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                                continue
                            q = qy * W + qx
                            if shape[q] < 0 or (same_shape and shape[q] != shape[r]):
                                continue
                            c = _dot(unit[r], unit[q])
                            if not c > 0:
                                c = 0.0
                            for _e in range(normal_power_log2):
                                c = c * c
                            dz = _dot(unit[r], _sub(point[q], point[r]))
                            if sps == INF:
                                wp = 1.0 if abs(dz) < INF else NAN
                            else:
                                t = dz / sps
                                wp = _div(1.0, 1.0 + t * t)
                            dl = lum[q] - lum[r]
                            if sl2 == INF:
                                wl = 1.0 if dl * dl < INF else NAN
                            else:
                                wl = _div(1.0, 1.0 + _div(dl * dl, den))
                            w = ((k * c) * wp) * wl
                            if not w > 0:
                                continue
                        for ch in range(3):
                            total[ch] = total[ch] + w * cur[q][ch]
                        wsum = wsum + w
                        vs = vs + (w * w) * var[q]
                new[r] = [_div(total[ch], wsum) for ch in range(3)]
                new_var[r] = _div(vs, wsum * wsum)
        cur, var = new, new_var
    return np.array(cur, dtype=np.float64).reshape(Hh, W, 3), np.array(var, dtype=np.float64).reshape(Hh, W)


def hostile_variance_frame(W, Hh, seed):
    """Guides and values nobody vouches for: three shapes in patches plus negative and out-of-range indices; normals of any length,
    zero, NaN and infinite; points on a wavy sheet, some NaN and infinite; colours with NaN, inf and 1e300; variances with zero,
    negative, NaN, inf and 1e300; counts of 0, 1, 3, 4, 2^20 and below zero; moments that are sometimes not moments of anything
    -> (colour, variance, shape, normal, point, moments, count), flat in row-major order."""
    rng = np.random.default_rng(seed)
    m = W * Hh
    yy, xx = np.mgrid[0:Hh, 0:W]
    shape = ((xx // 5 + yy // 4) % 3).astype(np.int32).reshape(-1)
    point = np.stack([xx * 0.1, yy * 0.1, 0.05 * np.sin(xx * 0.7) * np.cos(yy * 0.9)], axis=-1).reshape(-1, 3) + rng.normal(0, 0.002, (m, 3))
    normal = (np.array([0.0, 0.0, 1.0]) + rng.normal(0, 0.25, (m, 3))) * np.exp(rng.uniform(-2, 2, (m, 1)))
    colour = rng.uniform(0.0, 2.0, (m, 3))
    variance = rng.uniform(0.0, 0.3, m) ** 2
    lum = rng.uniform(0.0, 2.0, m)
    moments = np.stack([lum, lum * lum + rng.uniform(-0.01, 0.3, m), rng.uniform(0, 1, m)], axis=-1)
    count = rng.choice(np.array([0, 1, 3, 4, 2 ** 20, 1, 3, 2, 7], dtype=np.int32), m)
    pick = lambda share: np.flatnonzero(rng.uniform(0, 1, m) < share)  # noqa: E731
    for rows, value in ((pick(0.08), -1), (pick(0.02), -2 ** 31), (pick(0.04), 1000), (pick(0.02), 2 ** 31 - 1)):
        shape[rows] = value
    for rows, value in ((pick(0.03), (0.0, 0.0, 0.0)), (pick(0.02), (NAN, 0.0, 1.0)), (pick(0.02), (0.0, INF, 1.0)), (pick(0.01), (-INF, INF, NAN)),
                        (pick(0.02), (1e200, 1e200, 1e200)), (pick(0.02), (1e-200, 0.0, 1e-200))):
        normal[rows] = value
    for rows, value in ((pick(0.02), (NAN, 0.0, 0.0)), (pick(0.02), (0.0, INF, 0.0)), (pick(0.01), (1e300, -1e300, 1e300))):
        point[rows] = value
    for rows, value in ((pick(0.02), (NAN, 1.0, 1.0)), (pick(0.02), (1.0, INF, 1.0)), (pick(0.02), (1e300, 1.0, 1.0)), (pick(0.01), (-INF, NAN, 1e300)),
                        (pick(0.02), (1.0, 1.0, NAN)), (pick(0.02), (0.25, 0.5, -1.0))):
        colour[rows] = value
    for rows, value in ((pick(0.1), 0.0), (pick(0.03), -0.5), (pick(0.02), NAN), (pick(0.02), INF), (pick(0.02), 1e300), (pick(0.01), -INF),
                        (pick(0.01), -0.0)):
        variance[rows] = value
    for rows, value in ((pick(0.02), (NAN, 1.0, 0.0)), (pick(0.02), (1.0, INF, 0.0)), (pick(0.02), (1e300, 1.0, NAN)), (pick(0.02), (0.0, 0.0, 0.0)),
                        (pick(0.01), (-INF, NAN, 0.0))):
        moments[rows] = value
    count[pick(0.02)] = -5
    return colour, variance, shape, normal, point, moments, count


def variance_parameter_sets():
    """passes 1 .. 5 x both flags on and off: twenty sets, over which rotate the powers 0, 5 and 10, finite and infinite sigmas, three
    epsilons, and min_history 1, 4 and 100 with two pairs of hard tests."""
    powers, sigmas = (0, 5, 10), ((INF, INF), (0.3, 0.7), (INF, 4.0), (0.2, INF), (0.1, 1.0))  # (sigma_point, sigma_luminance)
    hard = ((0.9, 0.05), (-1.0, INF), (0.5, 0.004))  # (normal_min, point_tolerance)
    out = []
    for i, (passes, (same, wrap)) in enumerate((n, f) for n in range(1, 6) for f in FLAGS):
        sp, sl = sigmas[(3 * i) % 5]
        nm, tol = hard[i % 3]
        out.append(dict(passes=passes, same_shape=same, wrap_x=wrap, normal_power_log2=powers[(7 * i) % 3], sigma_point=sp, sigma_luminance=sl,
                        epsilon=(1e-10, 1e-3, 1.0)[(i // 2) % 3], min_history=(1, 4, 100)[(i // 3) % 3], normal_min=nm, point_tolerance=tol))
    return out


def _check(got, want, label):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    got, want = got.reshape(got.shape[0] * got.shape[1], -1), want.reshape(want.shape[0] * want.shape[1], -1)
    bad = H.differing(got, want)
    assert bad.size == 0, f"{label}: {bad.size} of {len(want)} pixels differ, first {int(bad[0])}: got {got[bad[0]]}, want {want[bad[0]]}"


HOST_FRAMES = [(1, 1), (3, 2), (17, 5), (37, 23)]


@pytest.mark.parametrize("W,Hh", HOST_FRAMES, ids=[f"{w}x{h}" for w, h in HOST_FRAMES])
def test_the_mirrors_equal_plain_scalar_loops_bit_for_bit(W, Hh):
    colour, variance, shape, normal, point, moments, count = hostile_variance_frame(W, Hh, 100 * W + Hh)
    sets = variance_parameter_sets()
    _check(rb.luminance_moments_host(colour, shape, W, Hh), moments_loops(colour, shape, W, Hh), f"{W}x{Hh} moments")
    # the large frame is where the loops cost: there every fourth set (all five pass counts, all four flag pairs among them)
    used = sets if W * Hh < 500 else sets[::3]
    spatial = 0
    for par in used:
        got = rb.variance_estimate_host(moments, count, shape, normal, point, W, Hh, **par)
        _check(got[..., None], estimate_loops(moments, count, shape, normal, point, W, Hh, **par)[..., None], f"{W}x{Hh} estimate {par}")
        spatial += int(((count >= 1) & (count < par["min_history"]) & (shape >= 0)).sum())
        got_c, got_v = rb.variance_filter_host(colour, variance, shape, normal, point, W, Hh, **par)
        want_c, want_v = filter_loops(colour, variance, shape, normal, point, W, Hh, **par)
        _check(got_c, want_c, f"{W}x{Hh} filter colour {par}")
        _check(got_v[..., None], want_v[..., None], f"{W}x{Hh} filter variance {par}")
        miss = shape < 0
        if miss.any():  # a miss is copied, whatever it holds
            assert not H.differing(got_c.reshape(-1, 3)[miss], colour[miss]).size
            assert not H.differing(got_v.reshape(-1, 1)[miss], variance[miss, None]).size
    assert spatial > 0 or W * Hh == 1


@pytest.mark.parametrize("passes", [1, 2, 3, 4, 5])
def test_without_the_luminance_weight_the_colour_is_the_parents_filter_bit_for_bit(passes):
    """Finite colours below 1e100, ``sigma_luminance = +inf`` and ANY variance: the colour output is ``denoise_host(...,
    sigma_colour=inf)`` in every bit, for every flag pair."""
    for W, Hh in ((17, 5), (37, 23)):
        colour, variance, shape, normal, point, _, _ = hostile_variance_frame(W, Hh, 7 * W + passes)
        colour = np.where(np.isfinite(colour) & (np.abs(colour) < 1e100), colour, 3e99)
        for i, (same, wrap) in enumerate(FLAGS):
            geo = dict(passes=passes, same_shape=same, wrap_x=wrap, normal_power_log2=(0, 5, 10, 5)[i], sigma_point=(0.3, INF, 0.1, 0.2)[i])
            got, _ = rb.variance_filter_host(colour, variance, shape, normal, point, W, Hh, sigma_luminance=INF, **geo)
            want = rb.denoise_host(colour, shape, normal, point, W, Hh, sigma_colour=INF, **geo)
            assert got.tobytes() == want.tobytes(), (W, Hh, geo)
            close, _ = rb.variance_filter_host(colour, variance, shape, normal, point, W, Hh, sigma_luminance=0.5, **geo)
            assert close.tobytes() != want.tobytes()  # (the control: the weight does something when it is on)


def test_the_mirrors_refuse_what_the_library_refuses():
    colour, variance, shape, normal, point, moments, count = hostile_variance_frame(5, 3, 1)
    bad = (dict(passes=0), dict(passes=11), dict(normal_power_log2=-1), dict(normal_power_log2=11), dict(min_history=0), dict(min_history=2 ** 20 + 1),
           dict(sigma_point=0.0), dict(sigma_point=NAN), dict(sigma_luminance=-1.0), dict(sigma_luminance=NAN), dict(epsilon=0.0), dict(epsilon=INF),
           dict(epsilon=NAN), dict(normal_min=1.5), dict(normal_min=NAN), dict(point_tolerance=0.0), dict(point_tolerance=NAN))
    for kw in bad:
        with pytest.raises(ValueError):
            rb.variance_filter_host(colour, variance, shape, normal, point, 5, 3, **kw)
        with pytest.raises(ValueError):
            rb.variance_estimate_host(moments, count, shape, normal, point, 5, 3, **kw)
    with pytest.raises(TypeError):
        rb.variance_filter_host(colour, variance, shape, normal, point, 5, 3, sigma_colour=1.0)
    with pytest.raises(ValueError):
        rb.luminance_moments_host(colour, shape, -1, 3)
    out_c, out_v = rb.variance_filter_host(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), 0, 4)
    assert out_c.shape == (4, 0, 3) and out_v.shape == (4, 0)
    assert rb.variance_estimate_host(np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), 4, 0).shape == (0, 4)
    assert rb.luminance_moments_host(np.zeros((0, 3)), np.zeros(0, np.int32), 0, 0).shape == (0, 0, 3)


# ---- moments through the unchanged accumulation -------------------------------------------------------------------------------------
def _accumulate(frames, guides, camera, W, Hh, **kw):
    """``frames`` (``[H, W, 3]`` each) through ``temporal_host`` from an empty history under a static camera -> (last frame, count)."""
    shape, normal, point = guides
    prev = rb.TemporalHistory.empty(W, Hh)
    for frame in frames:
        out, count = rb.temporal_host(frame, shape, normal, point, prev.colour, prev.shape_index, prev.normal, prev.point, prev.count, camera, W, Hh,
                                      **kw)
        prev = rb.TemporalHistory(out, shape, normal, point, count)
    return prev.colour, prev.count


def test_moments_through_the_unchanged_accumulation_are_the_running_means():
    """A static camera, a flat wall, grey frames alternating exactly between 0 and 1: after 4 frames the running means are
    mu1 = mu2 = 1/2 (l * l = l for 0 and 1), to 1e-12 (the reprojection's bilinear weights round); the estimate follows: (1/2 - 1/4) / 4.
    Identical frames of 0.5 give the variance +0.0 exactly: (b * 0.5 summed) / (b summed) is 0.5 and (b * 0.25 summed) / (b summed) is 0.25
    whatever the weights round to, and 0.25 - 0.5 * 0.5 is +0.0."""
    W, Hh = 23, 14
    camera = cameras(aspect=W / Hh)["perspective"]
    _, shape, normal, point = wall_frame(camera, W, Hh)
    assert (shape >= 0).all()
    guides = (shape, normal, point)
    frames = [rb.luminance_moments_host(np.full((Hh, W, 3), float(i % 2)), shape, W, Hh) for i in range(4)]
    assert all(f[..., 2].tobytes() == np.zeros((Hh, W)).tobytes() for f in frames) and (frames[1][..., :2] == 1.0).all()
    mu, count = _accumulate(frames, guides, camera, W, Hh)
    assert (count == 4).all()
    assert np.abs(mu[..., 0] - 0.5).max() <= 1e-12 and np.abs(mu[..., 1] - 0.5).max() <= 1e-12 and not mu[..., 2].any()
    var = rb.variance_estimate_host(mu, count, shape, normal, point, W, Hh, min_history=4)
    want = (mu[..., 1] - mu[..., 0] * mu[..., 0]) / 4.0
    assert var.tobytes() == want.tobytes() and np.abs(var - 0.0625).max() <= 1e-12
    # three frames: 0, 1, 0 -> mu1 = mu2 = 1/3, below min_history the estimate is spatial and, every neighbour holding the same, equal
    mu3, count3 = _accumulate(frames[:3], guides, camera, W, Hh)
    assert (count3 == 3).all() and np.abs(mu3[..., :2] - 1.0 / 3.0).max() <= 1e-12
    var3 = rb.variance_estimate_host(mu3, count3, shape, normal, point, W, Hh, min_history=4, point_tolerance=INF, normal_min=-1.0)
    assert np.abs(var3 - (1.0 / 3.0 - 1.0 / 9.0) / 3.0).max() <= 1e-12
    half = [rb.luminance_moments_host(np.full((Hh, W, 3), 0.5), shape, W, Hh)] * 6
    mu, count = _accumulate(half, guides, camera, W, Hh)
    for min_history in (1, 4, 100):  # (the temporal branch and the spatial one)
        var = rb.variance_estimate_host(mu, count, shape, normal, point, W, Hh, min_history=min_history)
        assert var.tobytes() == np.zeros((Hh, W)).tobytes(), min_history


def test_the_variance_of_gaussian_noise_on_both_branches():
    """Grey Gaussian noise of standard deviation 0.25 around 1.0 on a 64 x 64 one-shape wall, static camera, 8 frames, min_history 4.
    mu2 - mu1^2 of 8 samples is the biased sample variance, expectation sigma^2 * 7/8; its relative standard error per pixel is
    sqrt(2 / 7), over 4096 pixels sqrt(2 / 7) / 64 = 0.8 %: the bound of 5 % is six of them.  With every count forced to 1 the estimate
    is spatial, over the 49 pixels of a whole window: the bound is 5 % around sigma^2 * 48/49, the expectation of a 49-sample variance.
    (The accumulated second moments are means of SQUARES, so what the window sees is the per-frame variance of 8 * 49 samples,
    sigma^2 * 391/392, 1.8 % above that figure; the standard error over the frame's 32768 samples is again 0.8 %.)"""
    W = Hh = 64
    sigma2 = 0.0625
    camera = cameras(aspect=1.0)["perspective"]
    _, shape, normal, point = wall_frame(camera, W, Hh)
    assert (shape >= 0).all()
    rng = np.random.default_rng(11)
    frames = [rb.luminance_moments_host((1.0 + rng.normal(0.0, 0.25, (Hh, W, 1))) * np.ones(3), shape, W, Hh) for _ in range(8)]
    mu, count = _accumulate(frames, (shape, normal, point), camera, W, Hh)
    assert (count == 8).all()
    var = rb.variance_estimate_host(mu, count, shape, normal, point, W, Hh, min_history=4)
    mean = float((var * count).mean())
    print(f"temporal branch: mean of variance * count = {mean:.6f}, expected {sigma2 * 7 / 8:.6f} (ratio {mean / (sigma2 * 7 / 8):.4f})")
    assert abs(mean / (sigma2 * 7 / 8) - 1.0) <= 0.05
    ones = np.ones((Hh, W), np.int32)
    spatial = rb.variance_estimate_host(mu, ones, shape, normal, point, W, Hh, min_history=4, point_tolerance=INF)
    inner = float((spatial * ones)[3:-3, 3:-3].mean())
    print(f"spatial branch: mean of variance * count away from the borders = {inner:.6f}, expected {sigma2 * 48 / 49:.6f} "
          f"(ratio {inner / (sigma2 * 48 / 49):.4f})")
    assert abs(inner / (sigma2 * 48 / 49) - 1.0) <= 0.05


def test_two_properties_of_the_filter():
    W, Hh = 37, 23
    colour, variance, shape, normal, point, _, _ = hostile_variance_frame(W, Hh, 5)
    for same, wrap in FLAGS:
        # every variance 0 and a constant colour (so dl = 0 and wl = 1): the constant is a power of two, so every w * c is exact and
        # every partial sum is that power of two times wsum's, whatever the weights round to: (w * c summed) / (w summed) is c
        flat = np.full((Hh * W, 3), 0.5)
        out, var = rb.variance_filter_host(flat, np.zeros(Hh * W), shape, normal, point, W, Hh, passes=5, same_shape=same, wrap_x=wrap)
        assert out.tobytes() == flat.tobytes() and var.tobytes() == np.zeros((Hh, W)).tobytes()
        # the output variance is never negative for non-negative input: a sum of squares times non-negative numbers
        noisy = np.where(np.isfinite(colour), colour, 1.0)
        positive = np.where(variance >= 0, variance, 0.25)
        _, var = rb.variance_filter_host(noisy, positive, shape, normal, point, W, Hh, passes=4, same_shape=same, wrap_x=wrap)
        assert not (var < 0).any() and not np.isnan(var[np.isfinite(positive).reshape(Hh, W) & (shape.reshape(Hh, W) >= 0)]).all()
    # and a pass never raises a constant variance: the sum of w^2 is at most the square of the sum of w, in every pass (to within the
    # roundings of 25 products and sums, 2^-46 relative over four passes); where neighbours are accepted it lowers it
    _, shape, normal, point = wall_frame(cameras(aspect=W / Hh)["perspective"], W, Hh)
    rng = np.random.default_rng(3)
    noisy = (1.0 + rng.normal(0, 0.1, (Hh, W, 1))) * np.ones(3)
    out, var = rb.variance_filter_host(noisy, np.full((Hh, W), 0.01), shape, normal, point, W, Hh, sigma_point=INF)
    assert (var <= 0.01 * (1.0 + 2.0 ** -46)).all() and var.mean() < 0.01 and out.std() < noisy.std()


def test_what_reaches_the_device_scene_without_a_device():
    """``WorldQueries.variance_filtered`` and ``VarianceAccumulator`` hand the frame to the three queries of a scene in the right order
    with the right parameters; the shader asks for gather, accumulation, filter and materials in that order."""
    from types import SimpleNamespace

    seen = []
    Hh, W = 3, 4

    class Scene:
        device = 0

        def variance_moments(self, colour, shape_index, width, height, **kw):
            seen.append(("moments", np.asarray(colour), kw))
            return rb.luminance_moments_host(colour, shape_index, width, height)

        def variance_estimate(self, moments, count, shape_index, normal, point, width, height, **params):
            seen.append(("estimate", np.asarray(moments), np.asarray(count), params))
            return rb.variance_estimate_host(moments, count, shape_index, normal, point, width, height, **params)

        def variance_filter(self, colour, variance, shape_index, normal, point, width, height, **params):
            seen.append(("filter", np.asarray(variance), params))
            return rb.variance_filter_host(colour, variance, shape_index, normal, point, width, height, **params)

        def temporal(self, colour, shape_index, normal, point, prev_colour, prev_shape, prev_normal, prev_point, prev_count, prev_camera, width,
                     height, **params):
            seen.append(("temporal", np.asarray(colour), params))
            return rb.temporal_host(colour, shape_index, normal, point, prev_colour, prev_shape, prev_normal, prev_point, prev_count, prev_camera,
                                    width, height, **params)

    wq = rb.WorldQueries(Scene())
    camera = cameras(aspect=W / Hh)["perspective"]
    _, shape, normal, point = wall_frame(camera, W, Hh)
    frame = SimpleNamespace(shape_index=shape[None], point=point[None], normal=normal[None])
    rng = np.random.default_rng(1)
    values = rng.uniform(0.5, 1.5, (Hh, W, 3))
    # the single-frame route: moments, a count of 1, the spatial estimate, the filter
    out, var = wq.variance_filtered(values, frame, passes=2, min_history=4, point_tolerance=INF)
    assert [s[0] for s in seen] == ["moments", "estimate", "filter"] and (seen[1][2] == 1).all()
    assert seen[1][3] == seen[2][2] == dict(passes=2, min_history=4, point_tolerance=INF)
    want_var = rb.variance_estimate_host(rb.luminance_moments_host(values, shape, W, Hh), np.ones(W * Hh, np.int32), shape, normal, point, W, Hh,
                                         point_tolerance=INF)
    want = rb.variance_filter_host(values, want_var, shape, normal, point, W, Hh, passes=2, point_tolerance=INF)
    assert out.tobytes() == want[0].tobytes() and var.tobytes() == want[1].tobytes() and out.shape == (Hh, W, 3) and var.shape == (Hh, W)
    # a variance handed in is used as it is
    del seen[:]
    given = rng.uniform(0, 0.1, (Hh, W))
    wq.variance_filtered(values, frame, variance=given)
    assert [s[0] for s in seen] == ["filter"] and np.array_equal(seen[0][1].reshape(Hh, W), given)
    with pytest.raises(ValueError, match="count="):
        wq.variance_filtered(values, frame, variance=given, count=np.ones((Hh, W), np.int32))
    with pytest.raises(ValueError, match="variance of"):
        wq.variance_filtered(values, frame, variance=np.zeros((Hh, W + 1)))
    # the accumulator: per frame moments, two accumulations with the same parameters, the estimate
    del seen[:]
    acc = rb.VarianceAccumulator(wq, max_history=8, min_history=2, normal_min=0.5)
    assert acc.history_params == dict(max_history=8, normal_min=0.5) and acc.estimate_params == dict(min_history=2, normal_min=0.5)
    e1, v1 = acc.update(values, frame, camera)
    assert [s[0] for s in seen] == ["moments", "temporal", "temporal", "estimate"] and seen[1][2] == seen[2][2] == dict(max_history=8, normal_min=0.5)
    assert seen[3][3] == dict(min_history=2, normal_min=0.5) and (acc.count == 1).all() and acc.frames == 1
    assert np.array_equal(e1, values) and v1.shape == (Hh, W)
    e2, v2 = acc.update(values * 0.5, frame, camera)
    assert (acc.count == 2).all() and np.array_equal(acc.count, acc.moments.count) and acc.frames == 2
    mu = acc.moments._prev.colour
    assert v2.tobytes() == rb.variance_estimate_host(mu, acc.count, shape, normal, point, W, Hh, min_history=2, normal_min=0.5).tobytes()
    assert (v2 > 0).all()
    acc.reset()
    assert acc.count is None and acc.frames == 0
    with pytest.raises(TypeError, match="unknown accumulation or estimate parameter"):
        rb.VarianceAccumulator(wq, passes=3)
    with pytest.raises(ValueError, match="device=True"):
        rb.VarianceAccumulator(wq, stream=1)
    with pytest.raises(ValueError, match="device=True"):
        acc.update(values, frame, camera, width=W, height=Hh)
    with pytest.raises(ValueError, match="width= and height="):
        rb.VarianceAccumulator(wq, device=True).update(0, rb.DeviceGuides(0, 0, 0), camera)
    with pytest.raises(TypeError, match="DeviceGuides"):
        rb.VarianceAccumulator(wq, device=True).update(0, frame, camera, width=W, height=Hh)


def test_the_shader_asks_for_gather_accumulation_filter_and_materials_in_that_order():
    """``VarianceGuidedGatherShader`` without a device: its parameters are told apart by name, every frame draws fresh generators,
    ``accumulate=False`` takes the single-frame route and leaves the sequence alone."""
    from types import SimpleNamespace

    from pytracer_amd import hostmodel as hm
    from pytracer_amd import shaders

    Hh, W = 3, 4
    order = []
    camera = cameras(aspect=W / Hh)["perspective"]
    _, shape, normal, point = wall_frame(camera, W, Hh)
    frame = SimpleNamespace(shape_index=shape[None], point=point[None], normal=normal[None])
    gathered = rb.GatheredRadiance(np.zeros(rb.gather_bytes(Hh * W, 0), np.uint8), Hh * W, 0, shape=(1, Hh, W))

    class Scene:
        device = 0

        def variance_moments(self, colour, shape_index, width, height):
            order.append(("moments",))
            return rb.luminance_moments_host(colour, shape_index, width, height)

        def variance_estimate(self, moments, count, shape_index, normal, point, width, height, **params):
            order.append(("estimate", params, np.array(count)))
            return np.full((height, width), 0.25)

        def variance_filter(self, colour, variance, shape_index, normal, point, width, height, **params):
            order.append(("filter", params, np.array(variance)))
            return np.asarray(colour).reshape(height, width, 3) * 2.0, np.asarray(variance).reshape(height, width)

        def temporal(self, colour, shape_index, normal, point, prev_colour, prev_shape, prev_normal, prev_point, prev_count, prev_camera, width,
                     height, **params):
            order.append(("accumulate", params))
            return np.asarray(colour).reshape(height, width, 3) + 1.0, np.asarray(prev_count).reshape(height, width) + 1

    class Queries(rb.WorldQueries):
        def hemisphere_radiance(self, hits, samples, *a, **kw):
            order.append(("gather", samples, kw))
            return gathered

        def materials(self, hits):
            order.append(("materials",))
            hit = np.ones((1, Hh, W), bool)
            hit[0, 0, 0] = False
            return SimpleNamespace(emitted=np.full((1, Hh, W, 3), 0.5), brdf_color=np.full((1, Hh, W, 3), 0.25), hit=hit)

    world, queries = hm.World(), Queries(Scene())
    tracer = SimpleNamespace(world_queries=lambda w: queries if w is world else None, camera=camera)
    shader = shaders.VarianceGuidedGatherShader(world, tracer, samples=4, init_seq=54, background_color=hm.Color(7.0, 8.0, 9.0), passes=2,
                                                sigma_luminance=3.0, max_history=9, min_history=2, history_same_shape=False)
    assert shader.params == dict(passes=2, sigma_luminance=3.0) and shader.history_params == dict(max_history=9, min_history=2, same_shape=False)
    out = shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "moments", "accumulate", "accumulate", "estimate", "filter", "materials"]
    assert order[0][1] == 4 and order[0][2]["init_seq"] == 54 and order[2][1] == order[3][1] == dict(max_history=9, same_shape=False)
    assert order[4][1] == dict(min_history=2, same_shape=False) and (order[4][2] == 1).all()
    assert order[5][1] == dict(passes=2, sigma_luminance=3.0) and (order[5][2] == 0.25).all()
    # the filter sees the accumulated mean (the gather's zeros + 1), doubled by the fake; the first pixel is a miss
    assert out.shape == (1, Hh, W, 3) and out[0, 0, 0].tolist() == [7.0, 8.0, 9.0] and np.all(out[0, 1:] == 0.5 + 0.25 * 2.0)
    assert shader.frame_no == 1 and (shader.accumulator.count == 1).all() and (shader.last_variance == 0.25).all()
    del order[:]
    shader.shade_hits(frame)
    assert order[0][2]["init_seq"] == 54 + 1 * (Hh * W) * 4 and shader.frame_no == 2 and (shader.accumulator.count == 2).all()
    # without accumulation: the single-frame route with the same frame number's generators; history and frame number left alone
    shader.accumulate = False
    del order[:]
    shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "moments", "estimate", "filter", "materials"] and order[0][2]["init_seq"] == 54 + 2 * (Hh * W) * 4
    assert order[2][1] == order[3][1] == dict(passes=2, sigma_luminance=3.0, min_history=2) and (order[2][2] == 1).all()
    assert shader.frame_no == 2 and (shader.accumulator.count == 2).all()
    shader.accumulate, shader.filtered = True, False
    del order[:]
    shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "moments", "accumulate", "accumulate", "estimate", "materials"] and shader.frame_no == 3
    shader.reset()
    assert shader.frame_no == 0 and shader.accumulator.count is None
    many = SimpleNamespace(shape_index=np.zeros((4, Hh, W), np.int32), point=np.zeros((4, Hh, W, 3)), normal=np.ones((4, Hh, W, 3)))
    with pytest.raises(ValueError, match="one record per pixel"):
        shader.shade_hits(many)
    with pytest.raises(TypeError, match="tracer"):
        shaders.VarianceGuidedGatherShader(world).shade_hits(frame)
    for bad in (dict(wrap_x=True), dict(sigma_colour=1.0), dict(flags=1)):
        with pytest.raises(TypeError, match="unknown filter or accumulation parameter"):
            shaders.VarianceGuidedGatherShader(world, tracer, **bad)
    with pytest.raises(ValueError, match="samples"):
        shaders.VarianceGuidedGatherShader(world, tracer, samples=0)
