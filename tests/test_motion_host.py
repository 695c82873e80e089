"""CPU-only tests of the motion accumulate query (include/ptrace_motion.h, libptrace_motion.so, pytracer_amd.rays.motion_host): the
fifteenth library builds and loads without a GPU and leaves the other fourteen as they were; its header, the ctypes table and its
dynamic symbols agree; every refusal happens before any HIP call; the numpy mirror keeps the header's two contracts against the
weighted query's mirror in every bit; and it does what it is for -- a sphere that moved keeps its history."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from pytracer_amd import rays as rb

from . import moving_frames as M
from .test_gpu_weighted import PARAMETERS
from .test_temporal_host import cameras
from .test_weighted_host import _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_SIZE, ERR_NODEVICE = -1, -5, -6  # include/ptrace.h
V113 = (1 << 16) | 13
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _motion_lib, build

    build.build()
    assert os.path.exists(build.MOTION_LIB) and not build.needs_build()
    return _motion_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _motion_lib, _temporal_lib, _weighted_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_motion.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_motion_lib.EXPORTS) == {s for s, _, _ in _motion_lib._SIGNATURES} and len(declared) == 8
    assert declared == {"pt_rays_motion_" + n for n in ("version", "last_error", "bytes", "count_bytes", "table_bytes", "clear_device",
                                                        "accumulate_device", "accumulate")}
    assert _exported(_motion_lib.lib_path()) == declared
    assert lib.pt_rays_motion_version() == V113 and (_motion_lib.ABI_MAJOR, _motion_lib.ABI_MINOR) == (1, 13)
    needed = subprocess.run(["readelf", "-d", _motion_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_motion.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _motion_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    users = [f for f in os.listdir(build.CSRC) if '"pt_motion.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_motion.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_motion.hip")).read() + open(os.path.join(build.CSRC, "pt_motion.h")).read()
    assert '#include "pt_host_common.h"' in text and '"pt_weighted.h"' not in text
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text) and not re.search(r"\basm\b", text)
    assert text.count("hipLaunchKernelGGL") == 1 and "PTRACE_MA_BLOCKS" in text and "__ballot(" in text  # (one launch, one ballot)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ptrace_motion.h":
            assert "pt_rays_motion" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert not re.search(r'#include "ptrace_(?!motion)', header) and '#include "ptrace.h"' in header
    # the structs have the weighted query's layouts; a record is 192 bytes
    assert _motion_lib.MotionParams is _weighted_lib.WeightedParams and _motion_lib.MotionCamera is _temporal_lib.TemporalCamera
    fields = re.search(r"typedef struct pt_motion_params \{(.*?)\} pt_motion_params;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:int|double)\s+(\w+);", fields, flags=re.M) == [n for n, _ in _motion_lib.MotionParams._fields_]
    camera = re.search(r"typedef struct pt_motion_camera \{(.*?)\} pt_motion_camera;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:int|double)\s+(\w+)", camera, flags=re.M) == [n for n, _ in _temporal_lib.TemporalCamera._fields_]
    assert _motion_lib.MA_SAME_SHAPE == int(re.search(r"#define PT_MA_SAME_SHAPE\s+(\d+)", header).group(1)) == 1
    assert _motion_lib.MA_BLEND_WEIGHT == int(re.search(r"#define PT_MA_BLEND_WEIGHT\s+(\d+)", header).group(1)) == 2
    assert _motion_lib.MAX_SHAPES == int(re.search(r"#define PT_MA_MAX_SHAPES\s+(\d+)", header).group(1)) == 2 ** 20
    assert _motion_lib.RECORD == int(re.search(r"#define PT_MA_RECORD\s+(\d+)", header).group(1)) == 24
    assert _motion_lib.DEFAULTS == _weighted_lib.DEFAULTS
    for word in ("bit for bit", "((a0 * px + a1 * py) + a2 * pz) + a3", "(n0 * nx + n1 * ny) + n2 * nz", "NOTHING MOVED, NOTHING CHANGES",
                 "IT IS THE WEIGHTED QUERY ON MOVED RECORDS", "NON-FINITE TABLE ENTRIES", "ONTO ITSELF", "never read"):
        assert word in header, word


def test_the_pinned_build_tables_are_unchanged_and_the_new_row_is_in_its_own(lib):
    from pytracer_amd import build

    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_motion.h")), "ptrace_motion.hip", "pt_motion.h"} <= deps
    assert [len(t) for t in (build.TARGETS, build.ALL_TARGETS, build.EVERY_TARGET, build.BUILD_TARGETS, build.WALK_TARGETS, build.FRAME_TARGETS,
                             build.GUIDED_TARGETS, build.SAMPLED_TARGETS, build.HISTORY_TARGETS, build.MOVING_TARGETS)] == list(range(6, 16))
    assert list(build.WEIGHTED_ADDONS) == ["weighted"] and list(build.MOTION_ADDONS) == ["motion"]
    assert build.MOTION_TARGETS == ((build.MOTION_FLAGS, build.MOTION_LIB, build.MOTION_SOURCES),)
    assert build.MOVING_TARGETS == build.HISTORY_TARGETS + build.MOTION_TARGETS and build.MOVING_TARGETS[-1] == build.MOTION_TARGETS[0]
    assert build.MOTION_FLAGS[:-1] == build.FLAGS[:-1] and build.MOTION_FLAGS[-1] == "-cuid=libptrace_motion"
    assert "-ffp-contract=off" in build.MOTION_FLAGS and not any("fast-math" in f and not f.startswith("-fno") for f in build.MOTION_FLAGS)
    assert build.MOTION_SOURCES == ["ptrace_motion.hip"] and os.path.basename(build.MOTION_LIB) == "libptrace_motion.so"
    assert all(os.path.exists(t[1]) for t in build.MOVING_TARGETS)  # build() made all fifteen
    # the recorded hashes: fourteen rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "motion_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.HISTORY_TARGETS] and len(rows) == 14 and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.HISTORY_TARGETS]


def test_sizes(lib):
    for m in (0, 1, 63, 65, 2 ** 31 - 1):
        assert lib.pt_rays_motion_bytes(m) == 24 * m and lib.pt_rays_motion_count_bytes(m) == 4 * m
    for m in (-1, 2 ** 31):
        assert lib.pt_rays_motion_bytes(m) == 0 and lib.pt_rays_motion_count_bytes(m) == 0
    for n in (0, 1, 2, 77, 2 ** 20):
        assert lib.pt_rays_motion_table_bytes(n) == 192 * n
    for n in (-1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert lib.pt_rays_motion_table_bytes(n) == 0


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
NOWHERE = 2 ** 20  # a device no machine has: a call that passes every argument check ends at the device check, with or without a GPU
IDENTITY12 = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_every_refusal_happens_before_any_hip_call(lib):
    """Every call names a device that does not exist, so nothing is ever launched: a call that passes the argument checks ends at the
    first HIP call, the device check; whatever is refused otherwise was refused by the argument checks before it."""
    from pytracer_amd import _motion_lib

    def passed(rc):
        return rc == ERR_NODEVICE or (rc == ERR_INVALID and "out of range" in _motion_lib.last_error())

    W, H, S = 5, 3, 4
    m = W * H
    f3, i1 = (lambda: np.zeros((3, m))), (lambda: np.zeros(m, np.int32))
    names = ("c", "k", "s", "n", "pt", "pc", "pm", "ps", "pn", "pp", "pk")
    planes = dict(c=f3(), k=i1() + 1, s=i1(), n=f3() + 1.0, pt=f3(), pc=f3(), pm=f3(), ps=i1(), pn=f3() + 1.0, pp=f3(), pk=i1())
    flags, table = np.ones(S, np.int32), np.zeros((S, 24))
    out, mom, cnt = f3(), f3(), i1()

    def call(device=NOWHERE, w=W, h=H, par=True, cam=True, kind=abi.CAMERA_PERSPECTIVE, o=out, ob=None, q=mom, qb=None, k_out=cnt, kb=None,
             ns=S, mv=flags, mo=table, **kw):
        a = {name: kw.pop(name, planes[name]) for name in names}
        par = C.byref(_motion_lib.params(**kw)) if par else None
        cam = C.byref(_motion_lib.camera((kind, IDENTITY12, 1.0, 1.0))) if cam else None
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        qb = (q.nbytes if q is not None else 0) if qb is None else qb
        kb = (k_out.nbytes if k_out is not None else 0) if kb is None else kb
        args = [device, w, h, par, cam] + [p(a[name]) for name in names] + [ns, p(mv), p(mo)] + [p(o), ob, p(q), qb, p(k_out), kb]
        return lib.pt_rays_motion_accumulate(*args), lib.pt_rays_motion_accumulate_device(*args, None)

    err = _motion_lib.last_error
    assert all(passed(rc) for rc in call())
    assert all(passed(rc) for rc in call(k=None))  # (a NULL `samples` is legal)
    assert all(passed(rc) for rc in call(ns=0, mv=None, mo=None))  # (nothing moved: no tables)
    assert all(passed(rc) for rc in call(ns=0)) and call(w=0, h=0, ns=2 ** 20) == both(0)  # (the largest table is legal)
    assert all(passed(rc) for rc in call(max_history=2 ** 20, flags=0, normal_min=-1.0, point_tolerance=INF, max_weight=INF,
                                         kind=abi.CAMERA_ORTHOGONAL))
    assert all(passed(rc) for rc in call(max_history=1, flags=3, normal_min=1.0, point_tolerance=5e-324, max_weight=0.0))
    # the new refusals
    for ns in (-1, -2 ** 31, 2 ** 20 + 1, 2 ** 31 - 1):
        assert call(ns=ns) == both(ERR_INVALID) and "n_shapes" in err(), ns
    assert call(mv=None) == both(ERR_INVALID) and "null moved or motion table" in err()
    assert call(mo=None) == both(ERR_INVALID) and "null moved or motion table" in err()
    big = np.zeros(6 * m + 2 + 24 * S)
    whole, ints = big[:3 * m].reshape(3, m), big[:m].view(np.int32)[:m]
    assert call(o=whole, mo=big[3 * m - 1:3 * m - 1 + 24 * S].reshape(S, 24)) == both(ERR_INVALID) and "colour output overlaps the motion table" in err()
    assert call(q=whole, mo=big[:24 * S].reshape(S, 24)) == both(ERR_INVALID) and "moments output overlaps the motion table" in err()
    assert call(k_out=ints, mo=big[:24 * S].reshape(S, 24)) == both(ERR_INVALID) and "count output overlaps the motion table" in err()
    assert call(o=whole, mv=big.view(np.int32)[:S]) == both(ERR_INVALID) and "colour output overlaps the moved table" in err()
    assert call(q=whole, mv=big.view(np.int32)[6 * m - 1:6 * m - 1 + S]) == both(ERR_INVALID) and "moments output overlaps the moved table" in err()
    assert call(k_out=ints, mv=big.view(np.int32)[m - 1:m - 1 + S]) == both(ERR_INVALID) and "count output overlaps the moved table" in err()
    assert all(passed(rc) for rc in call(o=whole, mo=big[3 * m:3 * m + 24 * S].reshape(S, 24)))  # (adjacent is not overlapping)
    assert all(passed(rc) for rc in call(o=whole, mo=big[:24 * S].reshape(S, 24), ns=0))  # (a table of no rows overlaps nothing)
    # all of the weighted query's
    assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
    assert call(w=46341, h=46341, ob=2 ** 40, qb=2 ** 40, kb=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert call(par=False) == both(ERR_INVALID) and "null pt_motion_params" in err()
    assert call(cam=False) == both(ERR_INVALID) and "null pt_motion_camera" in err()
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
        assert call(k_out=ints, **{name: whole}) == both(ERR_INVALID) and "count output overlaps" in err(), name
    for name in ("k", "ps", "pk"):
        assert call(k_out=planes[name]) == both(ERR_INVALID) and "count output overlaps" in err(), name
        assert call(o=whole, **{name: ints}) == both(ERR_INVALID) and "colour output overlaps" in err(), name
    assert call(q=out) == both(ERR_INVALID) and "colour output overlaps the moments output" in err()
    assert call(o=whole, k_out=ints) == both(ERR_INVALID) and "colour output overlaps the count output" in err()
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "colour output too small" in err()
    assert call(qb=mom.nbytes - 1) == both(ERR_SIZE) and "moments output too small" in err()
    assert call(kb=cnt.nbytes - 1) == both(ERR_SIZE) and "count output too small" in err()
    for value in ("0", "many", "-3", "2x"):
        os.environ["PTRACE_MA_BLOCKS"] = value
        try:
            assert call() == both(ERR_INVALID) and "PTRACE_MA_BLOCKS" in err(), value
        finally:
            del os.environ["PTRACE_MA_BLOCKS"]
    # m = 0: PT_OK, nothing launched, no buffer needed -- but the structs and n_shapes are still checked
    nothing = {name: None for name in names}
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert call(w=w, h=h, o=None, q=None, k_out=None, mv=None, mo=None, **nothing) == both(0), (w, h)
    assert call(w=0, h=0, max_history=0) == both(ERR_INVALID) and call(w=0, h=0, ns=-1) == both(ERR_INVALID)
    assert call(w=0, h=0, kind=3) == both(ERR_INVALID) and call(w=0, h=0, par=False) == both(ERR_INVALID)
    clear = lib.pt_rays_motion_clear_device
    assert clear(NOWHERE, -1, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, 2 ** 31, p(cnt), 2 ** 40, None) == ERR_INVALID
    assert clear(-1, m, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, m, None, cnt.nbytes, None) == ERR_INVALID and "null" in err()
    assert clear(NOWHERE, m, p(cnt), cnt.nbytes - 1, None) == ERR_SIZE and clear(NOWHERE, 0, None, 0, None) == 0
    assert passed(clear(NOWHERE, m, p(cnt), cnt.nbytes, None))
    assert not out.any() and not mom.any() and not cnt.any()


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def _all_same(got, want):
    return all(_same(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("kind", ["perspective", "orthogonal"])
def test_contracts_c_and_d_of_the_mirror_in_every_bit(kind):
    W, Hh = 37, 23
    changed = movers = 0
    for i, how in enumerate(("same", "turned1", "translated")):
        before, args = M.inputs(W, Hh, kind, how, 500 + i)
        shape, normal, point = args[2], args[3], args[4]
        for j, par in enumerate(PARAMETERS):
            plain = rb.weighted_host(*args, before, W, Hh, **par)
            # C: nothing moved, nothing changes -- no tables, tables of no rows, and a table that is 0 everywhere (whose rows are NaN)
            assert _all_same(rb.motion_host(*args, before, None, None, W, Hh, **par), plain), (how, par)
            assert _all_same(rb.motion_host(*args, before, np.zeros(0, np.int32), np.zeros((0, 24)), W, Hh, **par), plain), (how, par)
            assert _all_same(rb.motion_host(*args, before, *M.table("static"), W, Hh, **par), plain), (how, par)
            # D: it is the weighted query on moved records
            name = M.TABLES[1 + (i + j) % 4]
            mv, mo = M.table(name)
            nm, pm = rb.move_records_host(shape, normal, point, mv, mo)
            got = rb.motion_host(*args, before, mv, mo, W, Hh, **par)
            assert _all_same(got, rb.weighted_host(*args[:3], nm, pm, *args[5:], before, W, Hh, **par)), (how, name, par)
            changed += int(not _all_same(got, plain))
            # step 1 itself: who is moved, and that everybody else keeps every bit
            listed = (shape >= 0) & (shape < len(mv))
            mvd = listed & (mv[np.where(listed, shape, 0)] != 0)
            assert _same(nm[~mvd], normal[~mvd]) and _same(pm[~mvd], point[~mvd]) and nm.shape == normal.shape
            if not mvd.any():  # (the orthogonal camera sees little ground: the one-row table moves nothing it shows)
                continue
            movers += 1
            s = int(shape[mvd][0])
            x = point[mvd][0]
            with np.errstate(all="ignore"):
                row0 = ((mo[s, 0] * x[0] + mo[s, 1] * x[1]) + mo[s, 2] * x[2]) + mo[s, 3]
            assert _same(np.array([pm[mvd][0][0]]), np.array([row0]))
    assert changed > len(PARAMETERS) and movers > len(PARAMETERS)  # (the tables reach the bits)
    with pytest.raises(ValueError, match="come together"):
        rb.motion_host(*args, before, np.zeros(2, np.int32), None, W, Hh)
    with pytest.raises(ValueError, match="24 per shape"):
        rb.motion_host(*args, before, np.zeros(2, np.int32), np.zeros((2, 12)), W, Hh)
    with pytest.raises(ValueError, match="max_weight"):
        rb.motion_host(*args, before, None, None, W, Hh, max_weight=NAN)


def test_a_sphere_that_moved_keeps_its_history():
    """48 x 36, the perspective camera at rest, the sphere 1.0 further along y: through the camera only NO sphere pixel reuses its
    history; carried back by the motion, 90 % or more do (the weighted mirror on moved records: 48 of 48).  Ground whose previous tap
    lay on the sphere restarts at 1 either way."""
    W, Hh = 48, 36
    camera, args, sphere = M.clean_pair("perspective", 1.0)
    plain = rb.weighted_host(*args, camera, W, Hh)
    mv, mo = M.table("translation", 1.0)
    got = rb.motion_host(*args, camera, mv, mo, W, Hh)
    print(f"{int(sphere.sum())} sphere pixels: {int((plain[2][sphere] >= 2).sum())} reuse history unmoved, {int((got[2][sphere] >= 2).sum())} moved")
    assert sphere.sum() >= 40 and (plain[2][sphere] >= 2).sum() == 0
    assert (got[2][sphere] >= 2).sum() >= 0.9 * sphere.sum()
    assert np.abs(got[0][sphere & (got[2] >= 2)] - 1.5).max() < 1e-12  # (half the sphere's old colour 2.0, half this frame's 1.0)
    shape, pshape = args[2], args[7]
    uncovered = (shape == M.GROUND) & (pshape == M.SPHERE)  # (a camera at rest: the previous tap is the pixel itself)
    assert uncovered.sum() > 10 and (plain[2][uncovered] == 1).all() and (got[2][uncovered] == 1).all()
    ground = shape == M.GROUND
    assert _same(got[0][ground], plain[0][ground]) and _same(got[2][ground], plain[2][ground])  # (the ground did not move)


def _world(sphere_t, plane_t=None):
    w = hm.World()
    w.add_shape(hm.Plane(plane_t if plane_t is not None else hm.Transformation()))
    w.add_shape(hm.Sphere(sphere_t))
    return w


def test_shape_motion():
    up = hm.translation(hm.Vec(0.0, 0.0, 1.0))
    a, b = _world(up), _world(up)
    moved, motion = rb.shape_motion(a, b)
    assert moved.dtype == np.int32 and motion.dtype == np.float64 and motion.shape == (2, 24) and not moved.any()
    # a translated sphere: A brings its current points back to the previous ones
    now = _world(hm.translation(hm.Vec(0.2, 0.4, -0.1)) * up)
    moved, motion = rb.shape_motion(a, now)
    assert moved.tolist() == [0, 1]
    rng = np.random.default_rng(3)
    local = rng.normal(0, 1, (50, 3))
    local /= np.linalg.norm(local, axis=1)[:, None]
    cur, prev = local + np.array([0.2, 0.4, 0.9]), local + np.array([0.0, 0.0, 1.0])
    A, N = motion[1, :12].reshape(3, 4), motion[1, 12:21].reshape(3, 3)
    assert np.abs(cur @ A[:, :3].T + A[:, 3] - prev).max() <= 1e-12 and np.abs(N - np.eye(3)).max() <= 1e-12
    # a scale: normals go by the inverse transpose
    grown = _world(up * hm.scaling(hm.Vec(2.0, 1.0, 0.5)))
    _, motion = rb.shape_motion(a, grown)
    assert np.abs(motion[1, 12:21].reshape(3, 3) - np.diag([2.0, 1.0, 0.5])).max() <= 1e-12  # (A = diag(1/2, 1, 2): N = A^-T)
    # static= switches a row off; mismatched worlds raise
    assert rb.shape_motion(a, now, static=(1,))[0].tolist() == [0, 0] and rb.shape_motion(a, now, static=[0])[0].tolist() == [0, 1]
    three = _world(up)
    three.add_shape(hm.Sphere(up))
    with pytest.raises(ValueError, match="2 shapes, this one 3"):
        rb.shape_motion(a, three)
    swapped = hm.World()
    swapped.add_shape(hm.Sphere(up))
    swapped.add_shape(hm.Plane())
    with pytest.raises(ValueError, match="was a Plane and is a Sphere"):
        rb.shape_motion(a, swapped)
    assert "ONTO ITSELF" in rb.shape_motion.__doc__ and "static" in rb.shape_motion.__doc__


def test_a_sphere_spinning_about_its_own_axis_belongs_in_static():
    W, Hh = 48, 36
    camera, args, sphere = M.clean_pair("perspective", 0.0)
    args = list(args)
    cols = np.arange(W)[None, :] * np.ones((Hh, 1))
    args[5] = np.stack([1.0 + cols / W, 0.5 + 0 * cols, 0.25 + 0 * cols], axis=-1)  # (a history that varies across the sphere)
    up = hm.translation(hm.Vec(0.0, 0.0, 1.0))
    before, now = _world(up), _world(up * hm.rotation_z(90.0))
    plain = rb.weighted_host(*args, camera, W, Hh)
    kept = rb.motion_host(*args, camera, *rb.shape_motion(before, now, static=(1,)), W, Hh)
    spun = rb.motion_host(*args, camera, *rb.shape_motion(before, now), W, Hh)
    assert _all_same(kept, plain)  # (the history stays where the light is)
    assert not _same(spun[0][sphere], plain[0][sphere])  # (followed, it is fetched from a quarter turn away, or lost)


def test_what_reaches_the_device_scene_without_a_device():
    """``WorldQueries.accumulated_moving`` hands the frame, the history, the camera and the tables to ``DeviceScene.motion``;
    ``MotionAccumulator(device=False)`` starts from lengths of zero, derives the motion from the world before, makes two calls per
    update and takes a caller's table or a new queries object."""
    from types import SimpleNamespace

    from pytracer_amd import shaders

    seen, estimates = [], []
    H, W = 3, 4

    class Scene:
        device = 0

        def motion(self, colour, samples, shape_index, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count,
                   prev_camera, moved, motion, width, height, **params):
            seen.append(SimpleNamespace(colour=colour, samples=samples, prev_colour=prev_colour, prev_count=prev_count, camera=prev_camera,
                                        moved=moved, motion=motion, size=(width, height), params=params, scene=self))
            moments = np.asarray(prev_moments).reshape(height, width, 3) + 1.0
            return np.asarray(colour).reshape(height, width, 3) + 1.0, moments, np.asarray(prev_count).reshape(height, width) + 1

        def variance_estimate(self, moments, count, shape_index, normal, point, width, height, **params):
            estimates.append(SimpleNamespace(moments=moments, count=count, size=(width, height), params=params, scene=self))
            return np.full((height, width), 0.25)

    wq = rb.WorldQueries(Scene())
    frame = SimpleNamespace(shape_index=np.zeros((1, H, W), np.int32), point=np.zeros((1, H, W, 3)), normal=np.ones((1, H, W, 3)))
    values = np.arange(H * W * 3.0).reshape(H, W, 3)
    cam_a, cam_b = cameras()["perspective"], cameras()["orthogonal"]
    k = np.arange(H * W, dtype=np.int32).reshape(H, W)
    table = (np.array([1], np.int32), np.zeros((1, 24)))
    new = wq.accumulated_moving(values, k, frame, rb.WeightedHistory.empty(W, H), cam_a, table, max_weight=9.0)
    assert isinstance(new, rb.WeightedHistory) and np.array_equal(new.colour, values + 1.0) and (new.count == 1).all()
    assert seen[-1].moved is table[0] and seen[-1].motion is table[1] and seen[-1].params == dict(max_weight=9.0) and seen[-1].camera is cam_a
    assert seen[-1].size == (W, H) and seen[-1].samples.shape == (H * W,)
    assert np.array_equal(new.point, frame.point[0])  # (the guides handed on are this frame's own records, unmoved)
    wq.accumulated_moving(values, None, frame, new, cam_b, None)
    assert seen[-1].moved is None and seen[-1].motion is None and seen[-1].samples is None
    with pytest.raises(ValueError, match="sample counts"):
        wq.accumulated_moving(values, k[:2], frame, new, cam_a, None)
    with pytest.raises(ValueError, match="history"):
        wq.accumulated_moving(values, k, frame, rb.WeightedHistory.empty(W + 1, H), cam_a, None)
    # the accumulator
    del seen[:]
    up = hm.translation(hm.Vec(0.0, 0.0, 1.0))
    world = _world(up)
    acc = rb.MotionAccumulator(wq, max_history=3, max_weight=7.0, min_history=2, normal_min=0.5, static=(0,))
    assert isinstance(acc, rb.WeightedAccumulator) and acc.count is None and acc.frames == 0
    e, variance = acc.update(values, frame, cam_a, samples=k, world=world)
    assert np.array_equal(e, values + 1.0) and (variance == 0.25).all() and acc.frames == 1 and len(seen) == 1 and len(estimates) == 1
    assert seen[0].moved is None and not seen[0].prev_count.any()  # (the first frame has no world before it)
    assert seen[0].params == dict(max_history=3, max_weight=7.0, normal_min=0.5) and estimates[0].params == dict(min_history=2, normal_min=0.5)
    world.shapes[1].transformation = hm.translation(hm.Vec(0.0, 0.5, 0.0)) * up  # (the same World, a shape given a new transformation)
    world.shapes[0].transformation = hm.translation(hm.Vec(0.5, 0.0, 0.0))  # (a plane sliding in its own plane: static)
    acc.update(values, frame, cam_b, world=world)
    assert seen[1].moved.tolist() == [0, 1] and seen[1].motion.shape == (2, 24) and seen[1].motion[1, 7] == -0.5
    assert seen[1].camera.kind == abi.CAMERA_PERSPECTIVE and (acc.count == 2).all() and np.array_equal(seen[1].prev_colour.reshape(H, W, 3), e)
    other = rb.WorldQueries(Scene())
    acc.update(values, frame, cam_a, motion=table, queries=other)  # (a table of the caller's, a scene of this frame's own)
    assert seen[2].moved is table[0] and seen[2].scene is other.scene and estimates[2].scene is other.scene and (acc.count == 3).all()
    acc.update(values, frame, cam_a)
    assert seen[3].moved is None and (acc.count == 4).all()  # (neither: nothing moved)
    with pytest.raises(ValueError, match="not both"):
        acc.update(values, frame, cam_a, world=world, motion=table)
    acc.reset()
    assert acc.count is None and acc.frames == 0
    acc.update(values, frame, cam_a, world=world)
    assert seen[-1].moved is None and not seen[-1].prev_count.any()
    with pytest.raises(TypeError, match="MotionAccumulator: unknown"):
        rb.MotionAccumulator(wq, passes=3)
    with pytest.raises(ValueError, match="device=True"):
        rb.MotionAccumulator(wq, stream=1)
    with pytest.raises(ValueError, match="width= and height="):
        rb.MotionAccumulator(wq, device=True).update(0, rb.DeviceGuides(0, 0, 0), cam_a)
    with pytest.raises(TypeError, match="DeviceGuides"):
        rb.MotionAccumulator(wq, device=True).update(0, frame, cam_a, width=W, height=H)
    with pytest.raises(TypeError, match="MovingWorldGatherShader: unknown"):
        shaders.MovingWorldGatherShader(world, None, flags=1)
    doc = shaders.MovingWorldGatherShader.__doc__
    assert "ADAPTIVE COUNTS STAY OUT" in doc and "sample_counts" in doc and "ONTO THEMSELVES" in doc
