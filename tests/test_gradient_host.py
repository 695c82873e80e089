"""CPU-only tests of the gradient accumulate query (include/ptrace_gradient.h, libptrace_gradient.so, pytracer_amd.rays.gradient_*_host):
the sixteenth library builds and loads without a GPU and leaves the other fifteen as they were; its header, the ctypes table and its
dynamic symbols agree; every refusal happens before any HIP call; the numpy mirrors keep the header's three contracts in every bit;
and the premise holds against the oracle -- the same records with the same streams, gathered in two worlds, differ only where the
world's change reaches them, and not at all when it did not change."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb

from . import gradient_frames as G
from . import moving_frames as M
from .test_gpu_weighted import PARAMETERS
from .test_temporal_host import cameras
from .test_weighted_host import _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_SIZE, ERR_NODEVICE = -1, -5, -6  # include/ptrace.h
V114 = (1 << 16) | 14
INF, NAN = float("inf"), float("nan")
NAMES = ("version", "last_error", "strata", "keep_bytes", "bytes", "count_bytes", "table_bytes", "clear_device", "probes_device", "probes",
         "keep_device", "keep", "accumulate_device", "accumulate")


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _gradient_lib, build

    build.build()
    assert os.path.exists(build.GRADIENT_LIB) and not build.needs_build()
    return _gradient_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _gradient_lib, _temporal_lib, _weighted_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_gradient.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_gradient_lib.EXPORTS) == {s for s, _, _ in _gradient_lib._SIGNATURES} and len(declared) == 14
    assert declared == {"pt_rays_gradient_" + n for n in NAMES}
    assert _exported(_gradient_lib.lib_path()) == declared
    assert lib.pt_rays_gradient_version() == V114 and (_gradient_lib.ABI_MAJOR, _gradient_lib.ABI_MINOR) == (1, 14)
    needed = subprocess.run(["readelf", "-d", _gradient_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_gradient.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _gradient_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    users = [f for f in os.listdir(build.CSRC) if '"pt_gradient.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_gradient.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_gradient.hip")).read() + open(os.path.join(build.CSRC, "pt_gradient.h")).read()
    assert '#include "pt_host_common.h"' in text and '"pt_motion.h"' not in text and '"pt_weighted.h"' not in text
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text) and not re.search(r"\basm\b", text) and "__shared__" not in text
    assert text.count("hipLaunchKernelGGL") == 3 and "PTRACE_GR_BLOCKS" in text and text.count("__ballot(") == 1  # (one launch per query)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ptrace_gradient.h":
            assert "pt_rays_gradient" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the header names other headers by file name, never their symbols, and includes ptrace.h only
    assert not re.search(r'#include "ptrace_(?!gradient)', header) and '#include "ptrace.h"' in header
    assert set(re.findall(r"\bpt_rays_[a-z]+", header)) == {"pt_rays_gradient"}
    assert not re.search(r"\bpt_(motion|weighted|temporal|variance|gather)_\w+", header) and not re.search(r"\bPT_(MA|WA|TA)_", header)
    # the structs
    assert _gradient_lib.GradientHistory is _weighted_lib.WeightedParams and _gradient_lib.GradientCamera is _temporal_lib.TemporalCamera
    fields = re.search(r"typedef struct pt_gradient_params \{(.*?)\} pt_gradient_params;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:int|double)\s+(\w+);", fields, flags=re.M) == [n for n, _ in _gradient_lib.GradientParams._fields_]
    assert C.sizeof(_gradient_lib.GradientParams) == 24 and _gradient_lib.GradientParams.gain.offset == 16
    fields = re.search(r"typedef struct pt_gradient_history \{(.*?)\} pt_gradient_history;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:int|double)\s+(\w+);", fields, flags=re.M) == [n for n, _ in _gradient_lib.GradientHistory._fields_]
    camera = re.search(r"typedef struct pt_gradient_camera \{(.*?)\} pt_gradient_camera;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:int|double)\s+(\w+)", camera, flags=re.M) == [n for n, _ in _temporal_lib.TemporalCamera._fields_]
    for name, value in (("SAME_SHAPE", _gradient_lib.GR_SAME_SHAPE), ("BLEND_WEIGHT", _gradient_lib.GR_BLEND_WEIGHT),
                        ("MAX_SHAPES", _gradient_lib.MAX_SHAPES), ("MAX_HISTORY", _gradient_lib.MAX_HISTORY), ("RECORD", _gradient_lib.RECORD),
                        ("MAX_STRATUM", _gradient_lib.MAX_STRATUM), ("MAX_RADIUS", _gradient_lib.MAX_RADIUS)):
        assert value == int(re.search(rf"#define PT_GR_{name}\s+(\d+)", header).group(1)), name
    assert (_gradient_lib.GR_SAME_SHAPE, _gradient_lib.GR_BLEND_WEIGHT, _gradient_lib.MAX_STRATUM, _gradient_lib.MAX_RADIUS) == (1, 2, 16, 4)
    defaults = _gradient_lib.params()
    assert (defaults.stratum, defaults.radius, defaults.flags, defaults.gain) == (3, 1, 1, _gradient_lib.KEEP_DEFAULTS["gain"])
    for word in ("bit for bit", "NOTHING KEPT BACK, NOTHING CHANGES", "NOTHING KEPT, THE HISTORY IS ONE FRAME", "A STATIC WORLD KEEPS EVERYTHING",
                 "0x9E3779B97F4A7C15", "0xD1B54A32D192ED03", "0x2545F4914F6CDD1D", "0xD6E8FEB86659FD93", "ROTATES", "sampling noise",
                 "nmax = (int)floor(kp * (double)nmax)", "nobody vouches for", "adaptive and ragged"):
        assert word in header, word


def test_the_pinned_build_tables_are_unchanged_and_the_new_row_is_in_its_own(lib):
    from pytracer_amd import build

    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_gradient.h")), "ptrace_gradient.hip", "pt_gradient.h"} <= deps
    assert [len(t) for t in (build.TARGETS, build.ALL_TARGETS, build.EVERY_TARGET, build.BUILD_TARGETS, build.WALK_TARGETS, build.FRAME_TARGETS,
                             build.GUIDED_TARGETS, build.SAMPLED_TARGETS, build.HISTORY_TARGETS, build.MOVING_TARGETS,
                             build.LIGHT_TARGETS)] == list(range(6, 17))
    assert list(build.MOTION_ADDONS) == ["motion"] and list(build.GRADIENT_ADDONS) == ["gradient"]
    assert build.GRADIENT_TARGETS == ((build.GRADIENT_FLAGS, build.GRADIENT_LIB, build.GRADIENT_SOURCES),)
    assert build.LIGHT_TARGETS == build.MOVING_TARGETS + build.GRADIENT_TARGETS and build.LIGHT_TARGETS[-1] == build.GRADIENT_TARGETS[0]
    assert build.MOVING_TARGETS == build.HISTORY_TARGETS + build.MOTION_TARGETS
    assert build.GRADIENT_FLAGS[:-1] == build.FLAGS[:-1] and build.GRADIENT_FLAGS[-1] == "-cuid=libptrace_gradient"
    assert "-ffp-contract=off" in build.GRADIENT_FLAGS and not any("fast-math" in f and not f.startswith("-fno") for f in build.GRADIENT_FLAGS)
    assert build.GRADIENT_SOURCES == ["ptrace_gradient.hip"] and os.path.basename(build.GRADIENT_LIB) == "libptrace_gradient.so"
    assert all(os.path.exists(t[1]) for t in build.LIGHT_TARGETS)  # build() made all sixteen
    # the recorded hashes: fifteen rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "gradient_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.MOVING_TARGETS] and len(rows) == 15 and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.MOVING_TARGETS]


def test_sizes(lib):
    for m in (0, 1, 63, 65, 2 ** 31 - 1):
        assert lib.pt_rays_gradient_bytes(m) == 24 * m and lib.pt_rays_gradient_count_bytes(m) == 4 * m
        assert lib.pt_rays_gradient_keep_bytes(m) == 8 * m
    for m in (-1, 2 ** 31):
        assert lib.pt_rays_gradient_bytes(m) == 0 and lib.pt_rays_gradient_count_bytes(m) == 0 and lib.pt_rays_gradient_keep_bytes(m) == 0
    for n in (0, 1, 2, 77, 2 ** 20):
        assert lib.pt_rays_gradient_table_bytes(n) == 192 * n
    for n in (-1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert lib.pt_rays_gradient_table_bytes(n) == 0
    from pytracer_amd import _gradient_lib

    for w, h, s, want in ((1, 1, 1, 1), (3, 2, 2, 2), (17, 5, 4, 10), (70, 33, 3, 24 * 11), (70, 33, 16, 15), (1280, 720, 3, 427 * 240),
                          (0, 9, 3, 0), (46340, 46340, 1, 46340 * 46340)):
        assert lib.pt_rays_gradient_strata(w, h, s) == want == _gradient_lib.strata(w, h, s), (w, h, s)
    for w, h, s in ((-1, 4, 2), (4, -1, 2), (4, 4, 0), (4, 4, 17), (4, 4, -3), (46341, 46341, 1)):
        assert lib.pt_rays_gradient_strata(w, h, s) == 0, (w, h, s)
        with pytest.raises(ValueError):
            _gradient_lib.strata(w, h, s)


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
NOWHERE = 2 ** 20  # a device no machine has: a call that passes every argument check ends at the device check, with or without a GPU
IDENTITY12 = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _passed(rc):
    from pytracer_amd import _gradient_lib

    return rc == ERR_NODEVICE or (rc == ERR_INVALID and "out of range" in _gradient_lib.last_error())


def _blocks_refused(call, err):
    for value in ("0", "many", "-3", "2x"):
        os.environ["PTRACE_GR_BLOCKS"] = value
        try:
            assert call() == both(ERR_INVALID) and "PTRACE_GR_BLOCKS" in err(), value
        finally:
            del os.environ["PTRACE_GR_BLOCKS"]


def test_probes_refuse_before_any_hip_call(lib):
    """Every call names a device that does not exist, so nothing is ever launched: a call that passes the argument checks ends at the
    first HIP call, the device check; whatever is refused otherwise was refused by the argument checks before it."""
    from pytracer_amd import _gradient_lib

    W, H, S, s = 5, 3, 4, 2
    m, ns = W * H, 6
    shape, normal, point = np.zeros(m, np.int32), np.ones((3, m)), np.zeros((3, m))
    flags, table = np.ones(S, np.int32), np.zeros((S, 24))
    oi, op, on, os_ = np.zeros(ns, np.int32), np.zeros((3, ns)), np.zeros((3, ns)), np.zeros(ns, np.uint64)

    def call(device=NOWHERE, w=W, h=H, st=s, phase=7, k=2, seq=54, sh=shape, n=normal, pt=point, nsh=S, mv=flags, mo=table, i=oi, ib=None, q=op,
             qb=None, r=on, rb_=None, u=os_, ub=None):
        size = lambda a, b: (a.nbytes if a is not None else 0) if b is None else b  # noqa: E731
        args = [device, w, h, st, phase, k, seq, p(sh), p(n), p(pt), nsh, p(mv), p(mo), p(i), size(i, ib), p(q), size(q, qb), p(r), size(r, rb_),
                p(u), size(u, ub)]
        return lib.pt_rays_gradient_probes(*args), lib.pt_rays_gradient_probes_device(*args, None)

    err = _gradient_lib.last_error
    assert all(_passed(rc) for rc in call())
    assert all(_passed(rc) for rc in call(nsh=0, mv=None, mo=None)) and all(_passed(rc) for rc in call(nsh=0))
    assert all(_passed(rc) for rc in call(st=1, ib=4 * m, i=np.zeros(m, np.int32), q=np.zeros((3, m)), r=np.zeros((3, m)), u=np.zeros(m, np.uint64)))
    assert all(_passed(rc) for rc in call(st=16, phase=2 ** 64 - 1, seq=2 ** 64 - 1, k=2 ** 31 - 1))
    for st in (0, -1, 17, 2 ** 31 - 1):
        assert call(st=st) == both(ERR_INVALID) and "stratum" in err(), st
    for k in (0, -1, -2 ** 31):
        assert call(k=k) == both(ERR_INVALID) and "samples" in err(), k
    for nsh in (-1, 2 ** 20 + 1):
        assert call(nsh=nsh) == both(ERR_INVALID) and "n_shapes" in err(), nsh
    assert call(mv=None) == both(ERR_INVALID) and "null moved or motion table" in err()
    assert call(mo=None) == both(ERR_INVALID) and "null moved or motion table" in err()
    assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
    assert call(w=46341, h=46341) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert call(device=-1) == both(ERR_INVALID)
    for name in ("sh", "n", "pt"):
        assert call(**{name: None}) == both(ERR_INVALID) and "null shape, normal or point" in err(), name
    for name, b in (("i", "ib"), ("q", "qb"), ("r", "rb_"), ("u", "ub")):
        assert call(**{name: None, b: 1000}) == both(ERR_INVALID) and "null output" in err(), name
    assert call(ib=oi.nbytes - 1) == both(ERR_SIZE) and "probe index output too small" in err()
    assert call(qb=op.nbytes - 1) == both(ERR_SIZE) and "probe point output too small" in err()
    assert call(rb_=on.nbytes - 1) == both(ERR_SIZE) and "probe normal output too small" in err()
    assert call(ub=os_.nbytes - 1) == both(ERR_SIZE) and "probe seq output too small" in err()
    # outputs overlapping each other or an input
    big = np.zeros(3 * m + 24 * S)
    assert call(q=point[:, :ns]) == both(ERR_INVALID) and "probe point output overlaps the points" in err()
    assert call(r=normal.reshape(-1)[:3 * ns].reshape(3, ns)) == both(ERR_INVALID) and "probe normal output overlaps the normals" in err()
    assert call(i=shape[:ns]) == both(ERR_INVALID) and "probe index output overlaps the shapes" in err()
    assert call(u=big[:ns].view(np.uint64), mo=big[:24 * S].reshape(S, 24)) == both(ERR_INVALID) and "probe seq output overlaps the motion table" in err()
    assert call(i=big.view(np.int32)[:ns], mv=big.view(np.int32)[ns - 1:ns - 1 + S]) == both(ERR_INVALID) and "index output overlaps the moved" in err()
    assert call(q=op, r=op) == both(ERR_INVALID) and "probe point output overlaps the probe normal output" in err()
    assert call(i=os_.view(np.int32)[:ns]) == both(ERR_INVALID) and "probe index output overlaps the probe seq output" in err()
    assert all(_passed(rc) for rc in call(u=big[:ns].view(np.uint64), mo=big[ns:ns + 24 * S].reshape(S, 24)))  # (adjacent is not overlapping)
    _blocks_refused(call, err)
    nothing = dict(sh=None, n=None, pt=None, mv=None, mo=None, i=None, q=None, r=None, u=None)
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert call(w=w, h=h, **nothing) == both(0), (w, h)
    assert call(w=0, h=0, st=0) == both(ERR_INVALID) and call(w=0, h=0, k=0) == both(ERR_INVALID) and call(w=0, h=0, nsh=-1) == both(ERR_INVALID)
    assert not oi.any() and not op.any() and not os_.any()


def test_keep_refuses_before_any_hip_call(lib):
    from pytracer_amd import _gradient_lib

    W, H, s = 5, 3, 2
    m, ns = W * H, 6
    colour, shape, index, old, keep = np.zeros((3, m)), np.zeros(m, np.int32), np.zeros(ns, np.int32), np.zeros((3, ns)), np.zeros(m)

    def call(device=NOWHERE, w=W, h=H, par=True, c=colour, sh=shape, i=index, o=old, k=keep, kb=None, **kw):
        kw.setdefault("stratum", s)
        par = C.byref(_gradient_lib.params(**kw)) if par else None
        args = [device, w, h, par, p(c), p(sh), p(i), p(o), p(k), (k.nbytes if k is not None else 0) if kb is None else kb]
        return lib.pt_rays_gradient_keep(*args), lib.pt_rays_gradient_keep_device(*args, None)

    err = _gradient_lib.last_error
    assert all(_passed(rc) for rc in call())
    assert all(_passed(rc) for rc in call(radius=0, gain=0.0, flags=0)) and all(_passed(rc) for rc in call(radius=4, gain=INF, same_shape_probes=False))
    assert all(_passed(rc) for rc in call(stratum=16, i=index[:1], o=old[:, :1])) and all(_passed(rc) for rc in call(gain=-0.0))
    assert call(par=False) == both(ERR_INVALID) and "null pt_gradient_params" in err()
    for st in (0, -1, 17):
        assert call(stratum=st) == both(ERR_INVALID) and "stratum" in err(), st
    for r in (-1, 5, 2 ** 31 - 1):
        assert call(radius=r) == both(ERR_INVALID) and "radius" in err(), r
    for bits in (2, 4, -1, 1 << 30):
        assert call(flags=bits) == both(ERR_INVALID) and "flag" in err(), bits
    for bad in (-5e-324, -1.0, -INF, NAN):
        assert call(gain=bad) == both(ERR_INVALID) and "gain" in err(), bad
    assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
    assert call(w=46341, h=46341, kb=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert call(device=-1) == both(ERR_INVALID)
    for name in ("c", "sh", "i", "o"):
        assert call(**{name: None}) == both(ERR_INVALID) and "null colour, shape, probe index or probe_old" in err(), name
    assert call(k=None, kb=keep.nbytes) == both(ERR_INVALID) and "null output" in err()
    assert call(kb=keep.nbytes - 1) == both(ERR_SIZE) and "keep output too small" in err()
    big = np.zeros(4 * m)
    assert call(k=colour.reshape(-1)[:m]) == both(ERR_INVALID) and "keep output overlaps the colour planes" in err()
    assert call(k=big[:m], sh=big.view(np.int32)[2 * m - 1:3 * m - 1]) == both(ERR_INVALID) and "keep output overlaps the shapes" in err()
    assert call(k=big[:m], i=big.view(np.int32)[:ns]) == both(ERR_INVALID) and "keep output overlaps the probe indices" in err()
    assert call(k=big[:m], o=big[m - 1:m - 1 + 3 * ns].reshape(3, ns)) == both(ERR_INVALID) and "keep output overlaps the probes' old colours" in err()
    assert all(_passed(rc) for rc in call(k=big[:m], o=big[m:m + 3 * ns].reshape(3, ns)))
    _blocks_refused(call, err)
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert call(w=w, h=h, c=None, sh=None, i=None, o=None, k=None) == both(0), (w, h)
    assert call(w=0, h=0, radius=5) == both(ERR_INVALID) and call(w=0, h=0, par=False) == both(ERR_INVALID)
    assert call(w=0, h=0, gain=NAN) == both(ERR_INVALID)
    assert not keep.any()


def test_accumulate_refuses_before_any_hip_call(lib):
    from pytracer_amd import _gradient_lib

    W, H, S = 5, 3, 4
    m = W * H
    f3, i1 = (lambda: np.zeros((3, m))), (lambda: np.zeros(m, np.int32))
    names = ("c", "k", "s", "n", "pt", "pc", "pm", "ps", "pn", "pp", "pk")
    planes = dict(c=f3(), k=i1() + 1, s=i1(), n=f3() + 1.0, pt=f3(), pc=f3(), pm=f3(), ps=i1(), pn=f3() + 1.0, pp=f3(), pk=i1())
    flags, table, kept = np.ones(S, np.int32), np.zeros((S, 24)), np.ones(m)
    out, mom, cnt = f3(), f3(), i1()

    def call(device=NOWHERE, w=W, h=H, par=True, cam=True, kind=abi.CAMERA_PERSPECTIVE, o=out, ob=None, q=mom, qb=None, k_out=cnt, kb=None,
             ns=S, mv=flags, mo=table, keep=kept, **kw):
        a = {name: kw.pop(name, planes[name]) for name in names}
        par = C.byref(_gradient_lib.history(**kw)) if par else None
        cam = C.byref(_gradient_lib.camera((kind, IDENTITY12, 1.0, 1.0))) if cam else None
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        qb = (q.nbytes if q is not None else 0) if qb is None else qb
        kb = (k_out.nbytes if k_out is not None else 0) if kb is None else kb
        args = [device, w, h, par, cam] + [p(a[name]) for name in names] + [ns, p(mv), p(mo), p(keep)] + [p(o), ob, p(q), qb, p(k_out), kb]
        return lib.pt_rays_gradient_accumulate(*args), lib.pt_rays_gradient_accumulate_device(*args, None)

    err = _gradient_lib.last_error
    assert all(_passed(rc) for rc in call()) and all(_passed(rc) for rc in call(keep=None))  # (a NULL `keep` is legal)
    assert all(_passed(rc) for rc in call(k=None)) and all(_passed(rc) for rc in call(ns=0, mv=None, mo=None))
    assert all(_passed(rc) for rc in call(max_history=2 ** 20, flags=0, normal_min=-1.0, point_tolerance=INF, max_weight=INF,
                                         kind=abi.CAMERA_ORTHOGONAL))
    # the new refusal: an output overlapping `keep` is refused like any other read
    big = np.zeros(6 * m + 2)
    whole, ints = big[:3 * m].reshape(3, m), big[:m].view(np.int32)[:m]
    assert call(o=whole, keep=big[3 * m - 1:4 * m - 1]) == both(ERR_INVALID) and "colour output overlaps the keep plane" in err()
    assert call(q=whole, keep=big[:m]) == both(ERR_INVALID) and "moments output overlaps the keep plane" in err()
    assert call(k_out=ints, keep=big[:m]) == both(ERR_INVALID) and "count output overlaps the keep plane" in err()
    assert all(_passed(rc) for rc in call(o=whole, keep=big[3 * m:4 * m]))  # (adjacent is not overlapping)
    # all of the motion query's
    for ns in (-1, -2 ** 31, 2 ** 20 + 1, 2 ** 31 - 1):
        assert call(ns=ns) == both(ERR_INVALID) and "n_shapes" in err(), ns
    assert call(mv=None) == both(ERR_INVALID) and "null moved or motion table" in err()
    assert call(mo=None) == both(ERR_INVALID) and "null moved or motion table" in err()
    assert call(o=whole, mo=big[3 * m - 1:3 * m - 1 + 24 * 1].reshape(1, 24), mv=flags[:1], ns=1) == both(ERR_INVALID) and "overlaps the motion table" in err()
    assert call(k_out=ints, mv=big.view(np.int32)[m - 1:m - 1 + S]) == both(ERR_INVALID) and "count output overlaps the moved table" in err()
    assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
    assert call(w=46341, h=46341, ob=2 ** 40, qb=2 ** 40, kb=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert call(par=False) == both(ERR_INVALID) and "null pt_gradient_history" in err()
    assert call(cam=False) == both(ERR_INVALID) and "null pt_gradient_camera" in err()
    for max_history in (0, -1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert call(max_history=max_history) == both(ERR_INVALID) and "max_history" in err(), max_history
    for bits in (4, 8, -1, 1 << 30):
        assert call(flags=bits) == both(ERR_INVALID) and "flag" in err(), bits
    for bad in (-1.0000000000000002, 1.0000000000000002, INF, -INF, NAN):
        assert call(normal_min=bad) == both(ERR_INVALID) and "normal_min" in err(), bad
    for bad in (0.0, -0.0, -1.0, -INF, NAN):
        assert call(point_tolerance=bad) == both(ERR_INVALID) and "point_tolerance" in err(), bad
    for bad in (-5e-324, -1.0, -INF, NAN):
        assert call(max_weight=bad) == both(ERR_INVALID) and "max_weight" in err(), bad
    for kind in (-1, 2, 7):
        assert call(kind=kind) == both(ERR_INVALID) and "camera kind" in err(), kind
    assert call(device=-1) == both(ERR_INVALID)
    for name in names:
        if name != "k":
            assert call(**{name: None}) == both(ERR_INVALID) and "null" in err() and "planes" in err(), name
    assert call(o=None, ob=out.nbytes) == both(ERR_INVALID) and "null output" in err()
    assert call(q=None, qb=mom.nbytes) == both(ERR_INVALID) and "null output" in err()
    assert call(k_out=None, kb=cnt.nbytes) == both(ERR_INVALID) and "null output" in err()
    for name in ("c", "pc", "pm", "pn", "pp"):
        assert call(o=planes[name]) == both(ERR_INVALID) and "colour output overlaps" in err(), name
        assert call(q=planes[name]) == both(ERR_INVALID) and "moments output overlaps" in err(), name
    for name in ("k", "ps", "pk"):
        assert call(k_out=planes[name]) == both(ERR_INVALID) and "count output overlaps" in err(), name
    assert call(q=out) == both(ERR_INVALID) and "colour output overlaps the moments output" in err()
    assert call(o=whole, k_out=ints) == both(ERR_INVALID) and "colour output overlaps the count output" in err()
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "colour output too small" in err()
    assert call(qb=mom.nbytes - 1) == both(ERR_SIZE) and "moments output too small" in err()
    assert call(kb=cnt.nbytes - 1) == both(ERR_SIZE) and "count output too small" in err()
    _blocks_refused(call, err)
    nothing = {name: None for name in names}
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert call(w=w, h=h, o=None, q=None, k_out=None, mv=None, mo=None, keep=None, **nothing) == both(0), (w, h)
    assert call(w=0, h=0, max_history=0) == both(ERR_INVALID) and call(w=0, h=0, ns=-1) == both(ERR_INVALID)
    assert call(w=0, h=0, kind=3) == both(ERR_INVALID) and call(w=0, h=0, par=False) == both(ERR_INVALID)
    clear = lib.pt_rays_gradient_clear_device
    assert clear(NOWHERE, -1, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, 2 ** 31, p(cnt), 2 ** 40, None) == ERR_INVALID
    assert clear(-1, m, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, m, None, cnt.nbytes, None) == ERR_INVALID and "null" in err()
    assert clear(NOWHERE, m, p(cnt), cnt.nbytes - 1, None) == ERR_SIZE and clear(NOWHERE, 0, None, 0, None) == 0
    assert _passed(clear(NOWHERE, m, p(cnt), cnt.nbytes, None))
    assert not out.any() and not mom.any() and not cnt.any()


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------
def _all_same(got, want):
    return all(_same(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("W,Hh", [(1, 1), (3, 2), (17, 5), (70, 33)])
def test_every_probe_lies_in_its_stratum_and_the_hash_is_the_headers(W, Hh):
    m = W * Hh
    rng = np.random.default_rng(W)
    shape = rng.integers(-1, 3, m).astype(np.int32)
    normal, point = rng.normal(0, 1, (m, 3)), rng.normal(0, 1, (m, 3))
    seen = set()
    for s in (1, 2, 3, 4, 16):
        gw, gh = -(-W // s), -(-Hh // s)
        for phase, K, seq0 in ((0, 1, 54), (1, 4, 0), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 64 - 5), (12345678901234567, 3, 54)):
            index, pp, nn, seq = rb.gradient_probes_host(shape, normal, point, None, None, W, Hh, stratum=s, phase=phase, samples=K, init_seq=seq0)
            assert index.shape == (gw * gh,) and index.dtype == np.int32 and seq.dtype == np.uint64 and pp.shape == nn.shape == (gw * gh, 3)
            for j in range(gw * gh):
                x, y = G.scalar_probe(phase, j, W, Hh, s)
                sy, sx = divmod(j, gw)
                assert sx * s <= x < min(W, (sx + 1) * s) and sy * s <= y < min(Hh, (sy + 1) * s), (s, phase, j)
                r = y * W + x
                if shape[r] < 0:
                    assert index[j] == -1 and seq[j] == 0 and not pp[j].any() and not nn[j].any() and not np.signbit(pp[j]).any()
                else:
                    assert index[j] == r and int(seq[j]) == (seq0 + r * K) % 2 ** 64
                    assert _same(pp[j], point[r]) and _same(nn[j], normal[r])  # (nothing moved: the record's bits)
                seen.add((s, j, x % s, y % s))
    assert W * Hh < 100 or len({(a, b) for s, _, a, b in seen if s == 4}) == 16  # (every place of a stratum is taken by some probe)
    with pytest.raises(ValueError, match="stratum"):
        rb.gradient_probes_host(shape, normal, point, None, None, W, Hh, stratum=17)
    with pytest.raises(ValueError, match="samples"):
        rb.gradient_probes_host(shape, normal, point, None, None, W, Hh, samples=0)
    with pytest.raises(ValueError, match="come together"):
        rb.gradient_probes_host(shape, normal, point, np.zeros(2, np.int32), None, W, Hh)


def test_probes_of_a_moved_shape_are_carried_into_the_previous_world():
    W, Hh = 37, 23
    moved = 0
    for name in M.TABLES:
        _, args = M.inputs(W, Hh, "perspective", "turned1", 700)
        shape, normal, point = args[2], args[3], args[4]
        mv, mo = M.table(name)
        nm, pm = rb.move_records_host(shape, normal, point, mv, mo)
        for s in (1, 3):
            index, pp, nn, _ = rb.gradient_probes_host(shape, normal, point, mv, mo, W, Hh, stratum=s, phase=5)
            ok = index >= 0
            assert ((index >= 0) == (shape.reshape(-1)[np.where(ok, index, 0)] >= 0))[ok].all()
            assert _same(pp[ok], pm.reshape(-1, 3)[index[ok]]) and _same(nn[ok], nm.reshape(-1, 3)[index[ok]]), (name, s)
            moved += int(not _same(pp[ok], point.reshape(-1, 3)[index[ok]]))
            if s == 1:  # every pixel is its own stratum: the probes are the frame
                assert np.array_equal(index, np.where(shape.reshape(-1) >= 0, np.arange(W * Hh), -1))
    assert moved >= 4  # (the tables reached the probes)


def test_contracts_e_and_f_of_the_mirror_in_every_bit():
    W, Hh = 37, 23
    shortened = ones = with_taps = 0
    for i, (kind, how) in enumerate((("perspective", "same"), ("perspective", "turned1"), ("orthogonal", "translated"))):
        before, args = M.inputs(W, Hh, kind, how, 900 + i)
        shape, samples = args[2], args[1]
        for j, par in enumerate(PARAMETERS):
            mv, mo = M.table(M.TABLES[(i + j) % 5])
            plain = rb.motion_host(*args, before, mv, mo, W, Hh, **par)
            # E: nothing kept back, nothing changes -- no plane, and a plane of ones
            assert _all_same(rb.gradient_accumulate_host(*args, before, mv, mo, None, W, Hh, **par), plain), (how, par)
            assert _all_same(rb.gradient_accumulate_host(*args, before, mv, mo, np.ones((Hh, W)), W, Hh, **par), plain), (how, par)
            assert _all_same(rb.gradient_accumulate_host(*args, before, mv, mo, np.full((Hh, W), 1.5), W, Hh, **par), plain)  # (clamped)
            assert _all_same(rb.gradient_accumulate_host(*args, before, mv, mo, np.full((Hh, W), INF), W, Hh, **par), plain)
            # F: nothing kept, the history is one frame.  What the taps hold is what the query carries when nothing is sampled.
            carried = rb.gradient_accumulate_host(args[0], np.zeros_like(samples), *args[2:], before, mv, mo, None, W, Hh, **par)
            tapped, hist = carried[2] >= 1, carried[0]
            took = (shape >= 0) & (samples > 0)
            with np.errstate(all="ignore"):
                one_frame = np.where(tapped[..., None], hist + (args[0] - hist) * 1.0, args[0])
            for nothing in (0.0, -0.5, NAN, -INF, -0.0):
                got = rb.gradient_accumulate_host(*args, before, mv, mo, np.full((Hh, W), nothing), W, Hh, **par)
                assert (got[2][took] == 1).all(), (how, par, nothing)
                nowhere = (shape >= 0) & (samples <= 0)
                assert (got[2][nowhere] == 0).all()  # (a carried history has no length left)
                if np.isfinite(par["max_weight"]):  # (a weight of +inf, which max_weight = inf lets through, makes 0 * inf = NaN)
                    assert _same(got[1][..., 2][took], samples[took].astype(np.float64)), (how, par, nothing)
                    assert _same(got[0][took], one_frame[took]), (how, par, nothing)
                    assert not got[1][..., 2][nowhere].any()
                shortened += int((got[2] < plain[2]).sum())
            with_taps += int((tapped & took).sum())
            # in between: the length is floor(kp * nmax) + 1, never longer than the motion query's
            kp = G.hostile_keep(W, Hh, 40 + j)
            got = rb.gradient_accumulate_host(*args, before, mv, mo, kp, W, Hh, **par)
            assert (got[2] <= plain[2]).all()
            keeps_all = ~(kp < 1.0)  # (1, 1.5, +inf -- and NaN and -inf, which keep nothing)
            full = keeps_all & ~np.isnan(kp) & (kp > 0)
            assert _same(got[0][full], plain[0][full]) and np.array_equal(got[2][full], plain[2][full]) and _same(got[1][full], plain[1][full])
            ones += int(full.sum())
    assert shortened > 1000 and ones > 1000 and with_taps > 1000  # (there were histories to cut, and records that kept theirs)
    with pytest.raises(ValueError, match="keep values"):
        rb.gradient_accumulate_host(*args, before, None, None, np.ones(5), W, Hh)


@pytest.mark.parametrize("kind", ["perspective", "orthogonal"])
def test_contract_g_a_static_world_keeps_everything(kind):
    W, Hh = 37, 23
    for i, how in enumerate(("same", "turned1")):
        before, args = M.inputs(W, Hh, kind, how, 1200 + i)
        colour, shape, normal, point = args[0], args[2], args[3], args[4]
        for s in (1, 2, 3, 4, 16):
            index = rb.gradient_probes_host(shape, normal, point, None, None, W, Hh, stratum=s, phase=i)[0]
            old = colour.reshape(-1, 3)[np.where(index >= 0, index, 0)]  # (what gathering the probes in an unchanged world gives)
            for radius in (0, 1, 2, 4):
                for gain in (0.0, 1.0, 32.0, INF):
                    keep = rb.gradient_keep_host(colour, shape, index, old, W, Hh, stratum=s, radius=radius, gain=gain)
                    assert keep.shape == (Hh, W) and keep.tobytes() == np.ones((Hh, W)).tobytes(), (how, s, radius, gain)
            plain = rb.motion_host(*args, before, None, None, W, Hh)
            assert _all_same(rb.gradient_accumulate_host(*args, before, None, None, keep, W, Hh), plain)


def test_a_single_probe_lowers_keep_exactly_in_its_window_and_on_its_shape():
    W, Hh, s = 23, 17, 3
    gw, gh = 8, 6
    camera = cameras(aspect=W / Hh)["perspective"]
    shape, normal, point = M.two_shape_frame(camera, W, Hh, 0.0)
    assert (shape == M.SPHERE).sum() > 10 and (shape == M.GROUND).sum() > 10 and (shape < 0).sum() > 10
    colour = np.random.default_rng(4).uniform(0.5, 1.5, (Hh, W, 3))
    index = rb.gradient_probes_host(shape, normal, point, None, None, W, Hh, stratum=s, phase=2)[0]
    same = colour.reshape(-1, 3)[np.where(index >= 0, index, 0)]
    ys, xs = np.divmod(np.arange(W * Hh), W)
    gx, gy = (xs // s).reshape(Hh, W), (ys // s).reshape(Hh, W)
    tested = 0
    for j in np.flatnonzero(index >= 0)[::5]:
        old = same.copy()
        old[j] = old[j] * 0.5  # (lo != lc: the light at this probe changed by half)
        jy, jx = divmod(int(j), gw)
        on = shape.reshape(-1)[index[j]]
        for radius in (0, 1, 2):
            window = (np.abs(gx - jx) <= radius) & (np.abs(gy - jy) <= radius)
            keep = rb.gradient_keep_host(colour, shape, index, old, W, Hh, stratum=s, radius=radius, gain=1.0)
            assert ((keep < 1.0) == (window & (shape == on))).all(), (j, radius)
            free = rb.gradient_keep_host(colour, shape, index, old, W, Hh, stratum=s, radius=radius, gain=1.0, same_shape_probes=False)
            assert ((free < 1.0) == (window & (shape >= 0))).all(), (j, radius)
            if radius == 0:  # one stratum, one probe: lam = |lc - lo| / max(lc, lo) = 1/2 to the last bit but one
                assert np.abs(keep[keep < 1.0] - 0.5).max() <= 2 ** -50
            assert rb.gradient_keep_host(colour, shape, index, old, W, Hh, stratum=s, radius=radius, gain=0.0).tobytes() == np.ones((Hh, W)).tobytes()
            tested += 1
    assert tested >= 9
    # hostile indices: nothing outside [0, m) is read, and an index from elsewhere is a probe like any other
    hostile = G.hostile_index(W, Hh, s, 8, index)
    keep = rb.gradient_keep_host(colour, shape, hostile, G.probe_old(colour, hostile, 9), W, Hh, stratum=s, radius=1, gain=2.0)
    assert np.isfinite(keep).all() and (keep >= 0).all() and (keep <= 1).all() and (keep < 1).any() and (keep == 1).any()
    assert (keep[shape < 0] == 1.0).all()
    with pytest.raises(ValueError, match="radius"):
        rb.gradient_keep_host(colour, shape, index, same, W, Hh, stratum=s, radius=5)
    with pytest.raises(ValueError, match="gain"):
        rb.gradient_keep_host(colour, shape, index, same, W, Hh, stratum=s, gain=NAN)
    with pytest.raises(ValueError, match="probes"):
        rb.gradient_keep_host(colour, shape, index[:-1], same[:-1], W, Hh, stratum=s)
    assert gh * gw == index.shape[0]


# ---- the premise, against the oracle ------------------------------------------------------------------------------------------------
def _moved_demo(dy):
    world, _ = scenes.demo_world()
    sphere = copy.copy(world.shapes[2])
    sphere.transformation = hm.translation(hm.Vec(0.0, dy, 0.0)) * sphere.transformation
    world.shapes[2] = sphere
    return world


def test_the_oracle_shows_the_gradient_and_a_static_world_shows_none(oracle):
    """156 ground points of the demo world (a 13 x 13 grid over [-3, 3]^2 without the points within 1 of the origin) as a 13 x 12
    frame, strata of 4: a dozen probes.  E and probe_old are composed by the oracle, K = 2, max_depth 2, init_state 42, seq = 54 + i K.
    Unchanged world: keep is 1.0 in every bit.  The sphere moved by 0.4 along y: at least one probe has keep < 1."""
    from . import gather_batches as GB

    grid = np.linspace(-3.0, 3.0, 13)
    point = np.array([(x, y, 0.0) for y in grid for x in grid if x * x + y * y > 1.0])
    W, Hh, s, K, phase = 13, 12, 4, 2, 3
    m = W * Hh
    assert point.shape == (m, 3)
    normal, shape = np.tile([0.0, 0.0, 1.0], (m, 1)), np.zeros(m, np.int32)
    old_world, new_world = _moved_demo(0.0), _moved_demo(0.4)
    table = rb.shape_motion(old_world, new_world)
    assert table[0].tolist() == [0, 0, 1]
    index, pp, nn, seq = rb.gradient_probes_host(shape, normal, point, *table, W, Hh, stratum=s, phase=phase, samples=K, init_seq=54)
    assert index.shape == (12,) and (index >= 0).all() and _same(pp, point[index]) and np.array_equal(seq, (54 + index * K).astype(np.uint64))
    zero = np.zeros((m, 3))

    def gather(world, points, normals, seqs):
        return GB.compose(oracle, flatten.flatten_world(world), points, normals, zero[:len(points)], seqs, K, 1, 2, 3, init_state=42,
                          background=(0.0, 0.0, 0.0))["radiance"]

    mode = oracle.lib().pto_get_sqr_mode()
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        e_new = gather(new_world, point, normal, 54 + np.arange(m) * K)
        in_new, in_old = gather(new_world, pp, nn, seq), gather(old_world, pp, nn, seq)
    finally:
        oracle.set_sqr_mode(mode)
    assert in_new.tobytes() == e_new[index].tobytes()  # (a gather is a function of world, point, normal and streams)
    for radius in (0, 1, 2):
        for gain in (1.0, 4.0, INF):
            assert rb.gradient_keep_host(e_new, shape, index, in_new, W, Hh, stratum=s, radius=radius, gain=gain).tobytes() == np.ones(m).tobytes()
    changed = (in_old != in_new).any(axis=1)
    print(f"{int(changed.sum())} of 12 probes change value when the sphere moves by 0.4")
    assert changed.any() and not changed.all()
    keep = rb.gradient_keep_host(e_new, shape, index, in_old, W, Hh, stratum=s, radius=0, gain=4.0).reshape(-1)
    assert (keep[index[changed]] < 1.0).all() and (keep[index[~changed]] == 1.0).all() and (keep >= 0.0).all()
    wide = rb.gradient_keep_host(e_new, shape, index, in_old, W, Hh, stratum=s, radius=1, gain=4.0)
    assert (wide < 1.0).sum() > (keep < 1.0).sum()


# ---- the layers above, without a device ---------------------------------------------------------------------------------------------
def test_what_reaches_the_device_scene_without_a_device():
    """``GradientAccumulator(device=False)``: without ``probe=``, and on a first frame, it makes the motion accumulator's two calls; from
    the second frame on it asks this frame's scene for probes, the PREVIOUS frame's scene for their gather with this frame's
    parameters, then keep, the accumulation with that plane and the estimate."""
    from types import SimpleNamespace

    from pytracer_amd import shaders

    calls = []
    H, W = 3, 4

    class Scene:
        device = 0

        def __init__(self, name):
            self.name = name

        def motion(self, colour, samples, shape_index, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count,
                   prev_camera, moved, motion, width, height, **params):
            calls.append(SimpleNamespace(what="motion", scene=self.name, moved=moved, params=params))
            return (np.asarray(colour).reshape(height, width, 3) + 1.0, np.asarray(prev_moments).reshape(height, width, 3) + 1.0,
                    np.asarray(prev_count).reshape(height, width) + 1)

        def gradient_probes(self, shape_index, normal, point, moved, motion, width, height, **kw):
            calls.append(SimpleNamespace(what="probes", scene=self.name, moved=moved, kw=kw))
            return np.array([0, -1], np.int32), np.ones((2, 3)), np.ones((2, 3)), np.array([54, 0], np.uint64)

        def gather(self, points, normals, samples, **kw):
            calls.append(SimpleNamespace(what="gather", scene=self.name, points=points, samples=samples, kw=kw))
            return SimpleNamespace(radiance=np.full((2, 3), 0.25))

        def gradient_keep(self, colour, shape_index, probe_index, probe_old, width, height, **kw):
            calls.append(SimpleNamespace(what="keep", scene=self.name, old=probe_old, index=probe_index, kw=kw))
            return np.full((height, width), 0.5)

        def gradient_accumulate(self, colour, samples, shape_index, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point,
                                prev_count, prev_camera, moved, motion, keep, width, height, **params):
            calls.append(SimpleNamespace(what="accumulate", scene=self.name, keep=keep, moved=moved, params=params, camera=prev_camera))
            return (np.asarray(colour).reshape(height, width, 3) + 2.0, np.asarray(prev_moments).reshape(height, width, 3) + 1.0,
                    np.asarray(prev_count).reshape(height, width) + 1)

        def variance_estimate(self, moments, count, shape_index, normal, point, width, height, **params):
            calls.append(SimpleNamespace(what="estimate", scene=self.name, params=params))
            return np.full((height, width), 0.25)

    frame = SimpleNamespace(shape_index=np.zeros((1, H, W), np.int32), point=np.zeros((1, H, W, 3)), normal=np.ones((1, H, W, 3)))
    values = np.arange(H * W * 3.0).reshape(H, W, 3)
    cam_a, cam_b = cameras()["perspective"], cameras()["orthogonal"]
    up = hm.translation(hm.Vec(0.0, 0.0, 1.0))
    world = hm.World()
    world.add_shape(hm.Plane())
    world.add_shape(hm.Sphere(up))
    q0, q1, q2 = (rb.WorldQueries(Scene(n)) for n in ("zero", "one", "two"))
    acc = rb.GradientAccumulator(q0, max_history=3, min_history=2, stratum=2, radius=2, gain=8.0, same_shape_probes=False)
    assert isinstance(acc, rb.MotionAccumulator) and acc.keep is None and acc.frames == 0
    assert acc.keep_params == dict(stratum=2, radius=2, gain=8.0, same_shape_probes=False)
    assert rb.GradientAccumulator(q0).keep_params == dict(stratum=3, radius=1, gain=8.0, same_shape_probes=True)
    probe = dict(samples=2, init_state=7, init_seq=1000, max_depth=2, russian_roulette_limit=1, background=(0.1, 0.2, 0.3))
    e, variance = acc.update(values, frame, cam_a, world=world, queries=q0, probe=probe)
    assert [c.what for c in calls] == ["motion", "estimate"] and acc.keep is None and np.array_equal(e, values + 1.0)  # (a first frame)
    del calls[:]
    world.shapes[1].transformation = hm.translation(hm.Vec(0.0, 0.5, 0.0)) * up
    e, variance = acc.update(values, frame, cam_b, world=world, queries=q1, probe=probe)
    assert [(c.what, c.scene) for c in calls] == [("probes", "one"), ("gather", "zero"), ("keep", "one"), ("accumulate", "one"), ("estimate", "one")]
    probes, gather, keep, accumulate, _ = calls
    assert probes.moved.tolist() == [0, 1] and probes.kw == dict(stratum=2, phase=1, samples=2, init_seq=1000)
    assert gather.samples == 2 and gather.points.shape == (3, 2) and gather.kw["seqs"].tolist() == [54, 0] and gather.kw["active"].tolist() == [0, -1]
    assert {k: gather.kw[k] for k in ("init_state", "max_depth", "russian_roulette_limit", "background", "num_of_rays", "depth", "channels")} == dict(
        init_state=7, max_depth=2, russian_roulette_limit=1, background=(0.1, 0.2, 0.3), num_of_rays=1, depth=0, channels="none")
    assert keep.kw == dict(stratum=2, radius=2, gain=8.0, same_shape_probes=False) and (keep.old == 0.25).all() and keep.index.tolist() == [0, -1]
    assert (accumulate.keep == 0.5).all() and accumulate.moved.tolist() == [0, 1] and accumulate.params == dict(max_history=3)
    assert accumulate.camera.kind == abi.CAMERA_PERSPECTIVE and np.array_equal(e, values + 2.0) and (acc.keep == 0.5).all() and acc.frames == 2
    del calls[:]
    acc.update(values, frame, cam_a, world=world, queries=q2)  # (no probe=: the motion accumulator)
    assert [(c.what, c.scene) for c in calls] == [("motion", "two"), ("estimate", "two")] and acc.keep is None and not calls[0].moved.any()
    del calls[:]
    acc.update(values, frame, cam_a, world=world, probe=dict(probe, queries=q0))  # (a scene of the caller's for the previous world)
    assert [(c.what, c.scene) for c in calls][:2] == [("probes", "two"), ("gather", "zero")] and calls[0].kw["phase"] == 3
    acc.reset()
    del calls[:]
    acc.update(values, frame, cam_a, world=world, probe=probe)
    assert [c.what for c in calls] == ["motion", "estimate"] and acc.frames == 1
    with pytest.raises(TypeError, match="GradientAccumulator: unknown"):
        rb.GradientAccumulator(q0, passes=3)
    with pytest.raises(TypeError, match="probe= takes samples="):
        acc.update(values, frame, cam_a, probe=dict(init_state=4))
    with pytest.raises(TypeError, match="probe= takes samples="):
        acc.update(values, frame, cam_a, probe=dict(samples=2, counts=4))
    with pytest.raises(ValueError, match="not both"):
        acc.update(values, frame, cam_a, world=world, motion=(np.zeros(2, np.int32), np.zeros((2, 24))), probe=probe)
    doc = shaders.GradientGatherShader.__doc__
    assert "follow_light" in doc and "ROTATE" in doc and issubclass(shaders.GradientGatherShader, shaders.MovingWorldGatherShader)
    with pytest.raises(TypeError, match="GradientGatherShader: unknown"):
        shaders.GradientGatherShader(world, None, flags=1)
