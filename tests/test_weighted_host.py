"""CPU-only tests of the weighted accumulate query (include/ptrace_weighted.h, libptrace_weighted.so, pytracer_amd.rays.weighted_host):
the fourteenth library builds and loads without a GPU and leaves the other thirteen as they were; its header, the ctypes table and its
dynamic symbols agree; every refusal of the interface happens before any HIP call; and the numpy mirror the GPU's bit tests compare
with has the properties the header derives from the arithmetic -- unweighted it is the accumulate query and the moments query in one
(contract A), equal counts change nothing (contract B), it is the exact mean weighted by samples, a record without a sample carries
its history, a hostile weight dies in the clamps -- and does what it is for: it beats the equally weighted mean by what theory says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import rays as rb
from pytracer_amd import scenes

from .test_temporal_host import cameras, wall_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_SIZE, ERR_NODEVICE = -1, -5, -6  # include/ptrace.h
V112 = (1 << 16) | 12
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _weighted_lib, build

    build.build()
    assert os.path.exists(build.WEIGHTED_LIB) and not build.needs_build()
    return _weighted_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _temporal_lib, _weighted_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_weighted.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_weighted_lib.EXPORTS) == {s for s, _, _ in _weighted_lib._SIGNATURES} and len(declared) == 7
    assert declared == {"pt_rays_weighted_" + n for n in ("version", "last_error", "bytes", "count_bytes", "clear_device", "accumulate_device",
                                                          "accumulate")}
    assert _exported(_weighted_lib.lib_path()) == declared
    assert lib.pt_rays_weighted_version() == V112 and (_weighted_lib.ABI_MAJOR, _weighted_lib.ABI_MINOR) == (1, 12)
    # an add-on like the thirteen before it: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _weighted_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_weighted.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _weighted_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    # the only file that includes the new device header is the new translation unit; the host layer is the shared one
    users = [f for f in os.listdir(build.CSRC) if '"pt_weighted.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_weighted.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_weighted.hip")).read() + open(os.path.join(build.CSRC, "pt_weighted.h")).read()
    assert '#include "pt_host_common.h"' in text and not re.search(r"\bg_err\b|\bstruct\s+Staged\b|#\s*define\s+HIP_TRY\b", text)
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text) and "__shared__" not in text and not re.search(r"\basm\b", text)
    assert text.count("hipLaunchKernelGGL") == 1 and "PTRACE_WA_BLOCKS" in text  # (one launch per call)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ptrace_weighted.h":
            assert "pt_rays_weighted" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert not re.search(r'#include "ptrace_(?!weighted)', header) and '#include "ptrace.h"' in header  # (the headers do not include each other)
    # pt_weighted_params: two ints and three doubles, in header order; pt_weighted_camera: the layout of pt_temporal_camera
    assert C.sizeof(_weighted_lib.WeightedParams) == 32 and C.sizeof(_weighted_lib.WeightedCamera) == 120
    fields = re.search(r"typedef struct pt_weighted_params \{(.*?)\} pt_weighted_params;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:int|double)\s+(\w+);", fields, flags=re.M) == [n for n, _ in _weighted_lib.WeightedParams._fields_]
    assert [n for n, _ in _weighted_lib.WeightedParams._fields_] == ["max_history", "flags", "normal_min", "point_tolerance", "max_weight"]
    camera = re.search(r"typedef struct pt_weighted_camera \{(.*?)\} pt_weighted_camera;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(?:int|double)\s+(\w+)", camera, flags=re.M) == [n for n, _ in _temporal_lib.TemporalCamera._fields_]
    assert _weighted_lib.WA_SAME_SHAPE == int(re.search(r"#define PT_WA_SAME_SHAPE\s+(\d+)", header).group(1)) == 1
    assert _weighted_lib.WA_BLEND_WEIGHT == int(re.search(r"#define PT_WA_BLEND_WEIGHT\s+(\d+)", header).group(1)) == 2
    assert _weighted_lib.MAX_HISTORY == int(re.search(r"#define PT_WA_MAX_HISTORY\s+(\d+)", header).group(1)) == 2 ** 20
    assert _weighted_lib.DEFAULTS["max_weight"] == 128.0 and _weighted_lib.DEFAULTS["blend_weight"] is False
    for word in ("bit for bit", "alpha = kd / total", "if (!(Sh > 0.0)) Sh = 0.0;", "if (Sh > max_weight) Sh = max_weight;",
                 "UNWEIGHTED, IT IS THE OLD PATH IN ONE LAUNCH", "EQUAL COUNTS CHANGE NOTHING", "NON-FINITE COLOURS",
                 "(M2 - M1^2) / n", "min(nmax + 1, max_history)", "smax"):
        assert word in header, word


def test_the_pinned_build_tables_are_unchanged_and_the_new_row_is_in_its_own(lib):
    from pytracer_amd import build

    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_weighted.h")), "ptrace_weighted.hip", "pt_weighted.h"} <= deps
    assert [len(t) for t in (build.TARGETS, build.ALL_TARGETS, build.EVERY_TARGET, build.BUILD_TARGETS, build.WALK_TARGETS, build.FRAME_TARGETS,
                             build.GUIDED_TARGETS, build.SAMPLED_TARGETS, build.HISTORY_TARGETS)] == [6, 7, 8, 9, 10, 11, 12, 13, 14]
    assert list(build.ADAPTIVE_ADDONS) == ["adaptive"] and list(build.WEIGHTED_ADDONS) == ["weighted"]
    assert build.WEIGHTED_TARGETS == ((build.WEIGHTED_FLAGS, build.WEIGHTED_LIB, build.WEIGHTED_SOURCES),)
    assert build.HISTORY_TARGETS == build.SAMPLED_TARGETS + build.WEIGHTED_TARGETS and build.HISTORY_TARGETS[-1] == build.WEIGHTED_TARGETS[0]
    assert build.WEIGHTED_FLAGS[:-1] == build.FLAGS[:-1] and build.WEIGHTED_FLAGS[-1] == "-cuid=libptrace_weighted"
    assert "-ffp-contract=off" in build.WEIGHTED_FLAGS and not any("fast-math" in f and not f.startswith("-fno") for f in build.WEIGHTED_FLAGS)
    assert build.WEIGHTED_SOURCES == ["ptrace_weighted.hip"] and os.path.basename(build.WEIGHTED_LIB) == "libptrace_weighted.so"
    assert all(os.path.exists(t[1]) for t in build.HISTORY_TARGETS)  # build() made all fourteen
    # the recorded hashes: thirteen rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "weighted_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.SAMPLED_TARGETS] and len(rows) == 13 and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.SAMPLED_TARGETS]
    assert [int(r[3]) for r in rows[1:]] == [len(_exported(t[1])) for t in build.SAMPLED_TARGETS[1:]]


def test_sizes(lib):
    for m in (0, 1, 63, 65, 2 ** 31 - 1):
        assert lib.pt_rays_weighted_bytes(m) == 24 * m and lib.pt_rays_weighted_count_bytes(m) == 4 * m
    for m in (-1, 2 ** 31):
        assert lib.pt_rays_weighted_bytes(m) == 0 and lib.pt_rays_weighted_count_bytes(m) == 0


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
NOWHERE = 2 ** 20  # a device no machine has: a call that passes every argument check ends at the device check, with or without a GPU
IDENTITY12 = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def test_every_refusal_happens_before_any_hip_call(lib):
    """Every call names a device that does not exist, so nothing is ever launched: a call that passes the argument checks ends at the
    first HIP call, the device check (PT_ERR_NODEVICE without a GPU, "out of range" with one); whatever is refused otherwise was
    refused by the argument checks before it."""
    from pytracer_amd import _weighted_lib

    def passed(rc):
        return rc == ERR_NODEVICE or (rc == ERR_INVALID and "out of range" in _weighted_lib.last_error())

    W, H = 5, 3
    m = W * H
    f3, i1 = (lambda: np.zeros((3, m))), (lambda: np.zeros(m, np.int32))
    names = ("c", "k", "s", "n", "pt", "pc", "pm", "ps", "pn", "pp", "pk")
    planes = dict(c=f3(), k=i1() + 1, s=i1(), n=f3() + 1.0, pt=f3(), pc=f3(), pm=f3(), ps=i1(), pn=f3() + 1.0, pp=f3(), pk=i1())
    out, mom, cnt = f3(), f3(), i1()

    def call(device=NOWHERE, w=W, h=H, par=True, cam=True, kind=abi.CAMERA_PERSPECTIVE, o=out, ob=None, q=mom, qb=None, k_out=cnt, kb=None, **kw):
        a = {name: kw.pop(name, planes[name]) for name in names}
        par = C.byref(_weighted_lib.params(**kw)) if par else None
        cam = C.byref(_weighted_lib.camera((kind, IDENTITY12, 1.0, 1.0))) if cam else None
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        qb = (q.nbytes if q is not None else 0) if qb is None else qb
        kb = (k_out.nbytes if k_out is not None else 0) if kb is None else kb
        args = [device, w, h, par, cam] + [p(a[name]) for name in names] + [p(o), ob, p(q), qb, p(k_out), kb]
        return lib.pt_rays_weighted_accumulate(*args), lib.pt_rays_weighted_accumulate_device(*args, None)

    err = _weighted_lib.last_error
    assert all(passed(rc) for rc in call())
    assert all(passed(rc) for rc in call(k=None))  # (a NULL `samples` is legal)
    assert all(passed(rc) for rc in call(max_history=2 ** 20, flags=0, normal_min=-1.0, point_tolerance=INF, max_weight=INF,
                                         kind=abi.CAMERA_ORTHOGONAL))
    assert all(passed(rc) for rc in call(max_history=1, flags=3, normal_min=1.0, point_tolerance=5e-324, max_weight=0.0))
    assert all(passed(rc) for rc in call(flags=2, max_weight=-0.0))
    assert call(w=-1) == both(ERR_INVALID) and call(h=-2) == both(ERR_INVALID) and "frame" in err()
    assert call(w=46341, h=46341, ob=2 ** 40, qb=2 ** 40, kb=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert call(w=2 ** 31 - 1, h=2, ob=2 ** 40, qb=2 ** 40, kb=2 ** 40) == both(ERR_INVALID)
    assert call(par=False) == both(ERR_INVALID) and "null pt_weighted_params" in err()
    assert call(cam=False) == both(ERR_INVALID) and "null pt_weighted_camera" in err()
    for max_history in (0, -1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert call(max_history=max_history) == both(ERR_INVALID) and "max_history" in err(), max_history
    for flags in (4, 8, -1, 1 << 30):
        assert call(flags=flags) == both(ERR_INVALID) and "flag" in err(), flags
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
    # each output overlapping `colour`, `samples` or any plane of the previous frame, wholly or by one value at either end
    big = np.zeros(6 * m + 2)
    whole, ints = big[:3 * m].reshape(3, m), big[:m].view(np.int32)[:m]
    for name in ("c", "pc", "pm", "pn", "pp"):
        assert call(o=planes[name]) == both(ERR_INVALID) and "colour output overlaps" in err(), name
        assert call(q=planes[name]) == both(ERR_INVALID) and "moments output overlaps" in err(), name
        for off in (1, 3 * m - 1):
            for which in ("o", "q"):
                assert call(**{which: big[off:off + 3 * m].reshape(3, m), name: whole}) == both(ERR_INVALID), (name, off, which)
                assert call(**{which: whole, name: big[off:off + 3 * m].reshape(3, m)}) == both(ERR_INVALID), (name, off, which)
        for which in ("o", "q"):  # (adjacent is not overlapping)
            assert all(passed(rc) for rc in call(**{which: big[3 * m:6 * m].reshape(3, m), name: whole})), (name, which)
        assert call(k_out=ints, **{name: whole}) == both(ERR_INVALID) and "count output overlaps" in err(), name
    for name in ("k", "ps", "pk"):
        assert call(k_out=planes[name]) == both(ERR_INVALID) and "count output overlaps" in err(), name
        half = big.view(np.int32)
        for off in (1, m - 1):
            assert call(k_out=half[off:off + m], **{name: half[:m]}) == both(ERR_INVALID), (name, off)
        assert all(passed(rc) for rc in call(k_out=half[m:2 * m], **{name: half[:m]})), name
        assert call(o=whole, **{name: ints}) == both(ERR_INVALID) and "colour output overlaps" in err(), name
        assert call(q=whole, **{name: ints}) == both(ERR_INVALID) and "moments output overlaps" in err(), name
    # the outputs among themselves
    assert call(q=out) == both(ERR_INVALID) and "colour output overlaps the moments output" in err()
    assert call(o=whole, k_out=ints) == both(ERR_INVALID) and "colour output overlaps the count output" in err()
    assert call(q=whole, k_out=ints) == both(ERR_INVALID) and "moments output overlaps the count output" in err()
    assert call(o=big[1:3 * m + 1].reshape(3, m), q=whole) == both(ERR_INVALID)
    # each output too small, with its own message
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "colour output too small" in err()
    assert call(qb=mom.nbytes - 1) == both(ERR_SIZE) and "moments output too small" in err()
    assert call(kb=cnt.nbytes - 1) == both(ERR_SIZE) and "count output too small" in err()
    # a launch alternative nobody knows is refused too, before any HIP call
    for value in ("0", "many", "-3", "2x"):
        os.environ["PTRACE_WA_BLOCKS"] = value
        try:
            assert call() == both(ERR_INVALID) and "PTRACE_WA_BLOCKS" in err(), value
        finally:
            del os.environ["PTRACE_WA_BLOCKS"]
    # m = 0: PT_OK, nothing launched, no buffer needed -- but the structs are still checked
    nothing = {name: None for name in names}
    for w, h in ((0, 0), (0, 7), (7, 0)):
        assert call(w=w, h=h, o=None, q=None, k_out=None, **nothing) == both(0), (w, h)
    assert call(w=0, h=0, max_history=0) == both(ERR_INVALID) and call(w=0, h=0, flags=4) == both(ERR_INVALID)
    assert call(w=0, h=0, kind=3) == both(ERR_INVALID) and call(w=0, h=0, par=False) == both(ERR_INVALID)
    assert call(w=0, h=0, normal_min=NAN) == both(ERR_INVALID) and call(w=0, h=0, point_tolerance=0.0) == both(ERR_INVALID)
    assert call(w=0, h=0, max_weight=NAN) == both(ERR_INVALID) and call(w=0, h=0, max_weight=-1.0) == both(ERR_INVALID)
    # the empty history's own refusals
    clear = lib.pt_rays_weighted_clear_device
    assert clear(NOWHERE, -1, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, 2 ** 31, p(cnt), 2 ** 40, None) == ERR_INVALID
    assert clear(-1, m, p(cnt), cnt.nbytes, None) == ERR_INVALID and clear(NOWHERE, m, None, cnt.nbytes, None) == ERR_INVALID and "null" in err()
    assert clear(NOWHERE, m, p(cnt), cnt.nbytes - 1, None) == ERR_SIZE and clear(NOWHERE, 0, None, 0, None) == 0
    assert passed(clear(NOWHERE, m, p(cnt), cnt.nbytes, None))
    assert not out.any() and not mom.any() and not cnt.any()


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """Every bit; a NaN for a NaN (numpy does not promise a NaN's sign or payload along two routes)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return a.tobytes() == b.tobytes()
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def hostile(colour, shape, normal, point, seed, counts=False):
    """Copies of a frame's planes with records nobody vouches for sprinkled in: shape indices -1, -2^31, 1000 and 2^31 - 1; normals
    of any length, zero, NaN, infinite and 1e200; points NaN, infinite and 1e300; colours NaN, infinite and 1e300.  ``counts``: also
    -> history lengths of 1 to 40 with 0, negative ones and 2^31 - 1 among them.  (tests/test_gpu_temporal.py's, copied.)"""
    rng = np.random.default_rng(seed)
    Hh, W = shape.shape
    m = W * Hh
    colour, shape, normal, point = (np.array(a).reshape(m, -1) for a in (colour, shape, normal, point))
    shape = shape.reshape(m)
    normal = normal * np.exp(rng.uniform(-2, 2, (m, 1))) + rng.normal(0, 0.02, (m, 3))
    point = point + rng.normal(0, 0.002, (m, 3))
    pick = lambda share: np.flatnonzero(rng.uniform(0, 1, m) < share)  # noqa: E731
    for rows, value in ((pick(0.06), -1), (pick(0.02), -2 ** 31), (pick(0.03), 1000), (pick(0.02), 2 ** 31 - 1)):
        shape[rows] = value
    for rows, value in ((pick(0.03), (0.0, 0.0, 0.0)), (pick(0.02), (NAN, 0.0, 1.0)), (pick(0.02), (0.0, INF, 1.0)), (pick(0.01), (-INF, INF, NAN)),
                        (pick(0.02), (-1e200, 1e200, 1e200)), (pick(0.02), (-1e-200, 0.0, 1e-200))):
        normal[rows] = value
    for rows, value in ((pick(0.02), (NAN, 0.0, 0.0)), (pick(0.02), (0.0, INF, 0.0)), (pick(0.01), (1e300, -1e300, 1e300)), (pick(0.01), (1e200, 0.0, 0.0))):
        point[rows] = value
    for rows, value in ((pick(0.02), (NAN, 1.0, 1.0)), (pick(0.02), (1.0, INF, 1.0)), (pick(0.02), (1e300, 1.0, 1.0)), (pick(0.01), (-INF, NAN, 1e300))):
        colour[rows] = value
    out = [colour.reshape(Hh, W, 3), shape.reshape(Hh, W), normal.reshape(Hh, W, 3), point.reshape(Hh, W, 3)]
    if counts:
        count = rng.integers(1, 41, m).astype(np.int32)
        for rows, value in ((pick(0.05), 0), (pick(0.03), -1), (pick(0.01), -2 ** 31), (pick(0.03), 2 ** 31 - 1), (pick(0.02), 2 ** 20)):
            count[rows] = value
        out.append(count.reshape(Hh, W))
    return out


_sequences = {}


def old_path(kind, max_history, W=37, H=23, frames=5):
    """Five hostile frames of a camera turning 1 degree per frame, and what the UNWEIGHTED path makes of them, chained: per frame
    ``(frame planes, camera before, temporal_host on the colour, temporal_host on the luminance-moments frame)``.  Computed once per
    case and shared; nothing here is modified by a test."""
    key = (kind, max_history, W, H, frames)
    if key not in _sequences:
        base = cameras(aspect=W / H)[kind]
        rng = np.random.default_rng(W * H + max_history)
        colours, moments = rb.TemporalHistory.empty(W, H), rb.TemporalHistory.empty(W, H)
        before, out = base, []
        for f in range(frames):
            now = scenes.turned_camera(base, 1.0 * f)
            cur = hostile(rng.uniform(0.0, 2.0, (H, W, 3)), *wall_frame(now, W, H, split=-1.4)[1:], seed=100 * f + 7)
            col = rb.temporal_host(*cur, colours.colour, colours.shape_index, colours.normal, colours.point, colours.count, before, W, H,
                                   max_history=max_history)
            frame = rb.luminance_moments_host(cur[0], cur[1], W, H)
            mom = rb.temporal_host(frame, *cur[1:], moments.colour, moments.shape_index, moments.normal, moments.point, moments.count, before, W, H,
                                   max_history=max_history)
            out.append((cur, before, col, mom))
            colours, moments = rb.TemporalHistory(col[0], *cur[1:], col[1]), rb.TemporalHistory(mom[0], *cur[1:], mom[1])
            before = now
        _sequences[key] = out
    return _sequences[key]


def chained(sequence, samples, W=37, H=23, **params):
    """``weighted_host`` over ``sequence``'s frames, each fed the one before -> per frame (colour, moments, count)."""
    prev, out = rb.WeightedHistory.empty(W, H), []
    for cur, before, _, _ in sequence:
        k = None if samples is None else np.full((H, W), samples, np.int32)
        got = rb.weighted_host(cur[0], k, *cur[1:], prev.colour, prev.moments, prev.shape_index, prev.normal, prev.point, prev.count, before, W, H,
                               **params)
        out.append(got)
        prev = rb.WeightedHistory(got[0], *cur[1:], got[2], got[1])
    return out


@pytest.mark.parametrize("max_history", [1, 2, 32])
@pytest.mark.parametrize("kind", ["perspective", "orthogonal"])
def test_contract_a_unweighted_it_is_the_old_path_in_one_pass(kind, max_history):
    sequence = old_path(kind, max_history)
    got = chained(sequence, None, max_history=max_history, max_weight=float(max_history - 1))
    reused = 0
    for f, ((cur, _, col, mom), (out, moments, count)) in enumerate(zip(sequence, got)):
        assert _same(out, col[0]) and _same(count, col[1]), f
        assert _same(moments[..., :2], mom[0][..., :2]) and _same(count, mom[1]), f
        assert _same(moments[..., 2], count.astype(np.float64)), f  # S == count
        reused += int((count >= 2).sum())
    assert count.max() == min(5, max_history) and (reused > 0) == (max_history > 1)


@pytest.mark.parametrize("K", [2, 7, 64])
def test_contract_b_equal_counts_change_nothing(K):
    for kind, max_history in (("perspective", 32), ("orthogonal", 2), ("perspective", 1)):
        sequence = old_path(kind, max_history)
        got = chained(sequence, K, max_history=max_history, max_weight=float(K * (max_history - 1)))
        for f, ((cur, _, col, _), (out, moments, count)) in enumerate(zip(sequence, got)):
            assert _same(out, col[0]) and _same(count, col[1]), (kind, max_history, f)
            assert _same(moments[..., 2], K * count.astype(np.float64)), (kind, max_history, f)  # S == K * count


# ---- an exact camera: every hit pixel lands on ONE tap of weight 1 --------------------------------------------------------------------
def exact_frame(W, H, aspect=1.0, x_wall=3.0):
    """An orthogonal camera with the identity transformation, and the hit frame of the wall x = ``x_wall`` whose points are the
    pixel centres -> (camera, shape [H, W], normal, point).  With W and H powers of two and aspect 1 every coordinate is exact and
    the projection gives fx = the column, fy = the row, so ax = ay = 0."""
    cols, rows = np.meshgrid(np.arange(W), np.arange(H))
    u, v = (cols + 0.5) / W, 1.0 - (rows + 0.5) / H
    point = np.stack([np.full((H, W), x_wall), (1.0 - 2.0 * u) * aspect, 2.0 * v - 1.0], axis=-1)
    normal = np.zeros((H, W, 3))
    normal[..., 0] = -2.0
    return (abi.CAMERA_ORTHOGONAL, IDENTITY12, 1.0, aspect), np.zeros((H, W), np.int32), normal, point


def test_the_exact_mean_weighted_by_samples():
    W, H, N = 16, 8, 8
    camera, shape, normal, point = exact_frame(W, H)
    shape = shape.copy()
    shape[2, 3], shape[5, 11] = -1, -7
    hit = shape >= 0
    # the premise: every hit pixel takes exactly one tap, of weight 1
    fx, fy, ok = rb.temporal_project_host(camera, point, W, H)
    cols, rows = np.meshgrid(np.arange(W), np.arange(H))
    assert ok.all() and _same(fx, cols.astype(np.float64)) and _same(fy, rows.astype(np.float64))
    rng = np.random.default_rng(14)
    ks = [1, 31] * (N // 2)
    colours = [rng.uniform(0.0, 2.0, (H, W, 3)) for _ in ks]
    prev = rb.WeightedHistory.empty(W, H)
    for f, (k, c) in enumerate(zip(ks, colours)):
        out, moments, count = rb.weighted_host(c, np.full((H, W), k, np.int32), shape, normal, point, prev.colour, prev.moments, prev.shape_index,
                                               prev.normal, prev.point, prev.count, camera, W, H, max_weight=INF)
        assert (count[hit] == f + 1).all() and not count[~hit].any()  # (the one tap was accepted every time)
        prev = rb.WeightedHistory(out, shape, normal, point, count, moments)
    want = sum(k * c for k, c in zip(ks, colours)) / float(sum(ks))
    lum = [rb._luminance(c) for c in colours]
    want1 = sum(k * l for k, l in zip(ks, lum)) / float(sum(ks))
    want2 = sum(k * l * l for k, l in zip(ks, lum)) / float(sum(ks))
    worst = np.abs(out[hit] / want[hit] - 1.0).max()
    print(f"eight blends, weights 1 and 31: the worst relative error against sum k c / sum k is {worst:.2e}")
    assert worst <= 1e-12
    assert np.abs(moments[hit][:, 0] / want1[hit] - 1.0).max() <= 1e-12 and np.abs(moments[hit][:, 1] / want2[hit] - 1.0).max() <= 1e-12
    assert (moments[hit][:, 2] == 128.0).all() and (count[hit] == 8).all()
    assert _same(out[~hit], colours[-1][~hit]) and not moments[~hit].any()
    # the same frames through the equally weighted query are another mean
    assert sum(ks) == 128 and np.abs(out[hit] - sum(colours)[hit] / N).max() > 0.05


def test_a_record_without_a_sample_carries_its_history():
    W, H = 16, 8
    camera, shape, normal, point = exact_frame(W, H)
    rng = np.random.default_rng(15)
    hit = shape >= 0
    first = rb.weighted_host(rng.uniform(0.0, 2.0, (H, W, 3)), np.full((H, W), 5, np.int32), shape, normal, point,
                             *_empty(W, H), camera, W, H, max_weight=INF)
    prev = rb.WeightedHistory(first[0], shape, normal, point, first[2], first[1])
    assert (first[2] == 1).all() and (first[1][..., 2] == 5.0).all()
    colour = rng.uniform(0.0, 2.0, (H, W, 3))
    none = np.zeros((H, W), bool)
    none[:, ::2] = True  # half the hit records took nothing
    results = []
    for empty in (0, -5, -2 ** 31):
        k = np.where(none, empty, 3).astype(np.int32)
        out, moments, count = rb.weighted_host(colour, k, shape, normal, point, prev.colour, prev.moments, prev.shape_index, prev.normal,
                                               prev.point, prev.count, camera, W, H, max_weight=INF)
        # colour, M1, M2: the reprojected history (one tap of weight 1: the history itself); S and count not grown
        assert _same(out[none], prev.colour[none]) and _same(moments[none], prev.moments[none]) and (count[none] == 1).all(), empty
        assert (count[~none] == 2).all() and (moments[~none][:, 2] == 8.0).all() and (out[~none] != prev.colour[~none]).any(axis=-1).all()
        results.append((out, moments, count))
        # a weight cap still applies to what is carried, and max_history to its length
        capped = rb.weighted_host(colour, k, shape, normal, point, prev.colour, prev.moments, prev.shape_index, prev.normal, prev.point,
                                  np.full((H, W), 9, np.int32), camera, W, H, max_weight=2.0, max_history=4)
        assert (capped[1][none][:, 2] == 2.0).all() and (capped[2][none] == 4).all() and (capped[2][~none] == 4).all()
        # with no history they come out with a count of 0 and nothing in their moments
        fresh = rb.weighted_host(colour, k, shape, normal, point, *_empty(W, H), camera, W, H)
        assert _same(fresh[0], colour) and not fresh[1][none].any() and not fresh[2][none].any() and (fresh[2][~none] == 1).all()
        assert (fresh[1][~none][:, 2] == 3.0).all()
    for other in results[1:]:
        assert all(_same(a, b) for a, b in zip(results[0], other))  # (-5 and -2^31 behave as 0)
    assert hit.all()


def _empty(W, H):
    e = rb.WeightedHistory.empty(W, H)
    return e.colour, e.moments, e.shape_index, e.normal, e.point, e.count


def test_hostile_weights_die_in_the_clamps():
    W, H = 8, 4
    camera, shape, normal, point = exact_frame(W, H)
    rng = np.random.default_rng(16)
    old, colour = rng.uniform(0.0, 2.0, (H, W, 3)), rng.uniform(0.0, 2.0, (H, W, 3))
    values = [NAN, -1.0, INF, 1e300, 0.0, -0.0, -INF, 5.0, 5e-324, 12.5]
    S = np.array([values[i % len(values)] for i in range(W * H)]).reshape(H, W)
    moments = np.stack([rb._luminance(old), rb._luminance(old) ** 2, S], axis=-1)
    ones = np.ones((H, W), np.int32)
    k = np.full((H, W), 3, np.int32)
    lum = rb._luminance(colour)
    for max_weight in (0.0, 10.0, INF):
        for blend in (False, True):  # (one tap of weight 1: its weight is the largest and the blend)
            out, mom, count = rb.weighted_host(colour, k, shape, normal, point, old, moments, shape, normal, point, ones, camera, W, H,
                                               max_weight=max_weight, blend_weight=blend)
            with np.errstate(all="ignore"):
                Sh = np.where(S > 0.0, S, 0.0)  # NaN, -1, -0.0 and -inf become 0
                Sh = np.where(Sh > max_weight, max_weight, Sh)
                total = Sh + 3.0
                alpha = 3.0 / total
                want = old + (colour - old) * alpha[..., None]
                want1 = moments[..., 0] + (lum - moments[..., 0]) * alpha
                want2 = moments[..., 1] + (lum * lum - moments[..., 1]) * alpha
            assert np.isfinite(alpha).all() and (alpha >= 0.0).all() and (alpha <= 1.0).all()  # (NaN never reaches alpha through S)
            assert _same(out, want) and _same(mom[..., 0], want1) and _same(mom[..., 1], want2) and _same(mom[..., 2], total), (max_weight, blend)
            assert np.isfinite(out).all() and (count == 2).all()
            if max_weight == INF:
                assert _same(out[S == INF], old[S == INF]) and (mom[..., 2][S == INF] == INF).all()  # (alpha = 3 / inf = 0)
            if max_weight == 0.0:
                assert (alpha == 1.0).all() and (mom[..., 2] == 3.0).all()
    # several taps: the largest weight, or their blend
    moved = point + np.array([0.0, 0.3 / W, -0.4 / H])
    a = rb.weighted_host(colour, k, shape, normal, moved, old, moments, shape, normal, point, ones, camera, W, H, max_weight=INF, point_tolerance=INF)
    b = rb.weighted_host(colour, k, shape, normal, moved, old, moments, shape, normal, point, ones, camera, W, H, max_weight=INF, point_tolerance=INF,
                         blend_weight=True)
    assert not _same(a[1][..., 2], b[1][..., 2]) and _same(a[2], b[2])
    with pytest.raises(ValueError, match="max_weight"):
        rb.weighted_host(colour, k, shape, normal, point, old, moments, shape, normal, point, ones, camera, W, H, max_weight=NAN)
    with pytest.raises(ValueError, match="max_weight"):
        rb.weighted_host(colour, k, shape, normal, point, old, moments, shape, normal, point, ones, camera, W, H, max_weight=-1.0)
    with pytest.raises(ValueError, match="max_history"):
        rb.weighted_host(colour, k, shape, normal, point, old, moments, shape, normal, point, ones, camera, W, H, max_history=0)
    nothing = rb.weighted_host(*([np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32)] + [np.zeros((0, 3))] * 4
                                 + [np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32)]), camera, 0, 4)
    assert nothing[0].shape == (4, 0, 3) and nothing[1].shape == (4, 0, 3) and nothing[2].shape == (4, 0) and nothing[2].dtype == np.int32


def test_weighting_helps_by_about_what_theory_says():
    """48 x 36, a static camera, eight frames whose colour is the mean of k uniform(0, 2) draws per channel, k = 1, 31, 1, 31, ...: the
    RMS error against 1.0 of the accumulation weighted by k, over that of the equally weighted one on the same frames.  Expected from
    the variances sigma^2 / 128 and sigma^2 (4 + 4 / 31) / 64: 0.348; a numpy simulation of both recurrences gave 0.351.  The bound
    0.5 is the claim "weighting helps by about what theory says" with room for the scatter of 5 184 samples."""
    W, H, N = 48, 36, 8
    camera, shape, normal, point = exact_frame(W, H, aspect=W / H)
    rng = np.random.default_rng(17)
    ks = [1, 31] * (N // 2)
    weighted, plain = rb.WeightedHistory.empty(W, H), rb.TemporalHistory.empty(W, H)
    for k in ks:
        colour = rng.uniform(0.0, 2.0, (k, H, W, 3)).mean(axis=0)
        out, moments, count = rb.weighted_host(colour, np.full((H, W), k, np.int32), shape, normal, point, weighted.colour, weighted.moments,
                                               weighted.shape_index, weighted.normal, weighted.point, weighted.count, camera, W, H, max_weight=INF)
        weighted = rb.WeightedHistory(out, shape, normal, point, count, moments)
        old, old_count = rb.temporal_host(colour, shape, normal, point, plain.colour, plain.shape_index, plain.normal, plain.point, plain.count,
                                          camera, W, H)
        plain = rb.TemporalHistory(old, shape, normal, point, old_count)
    assert (weighted.count == N).all() and (plain.count == N).all() and (weighted.moments[..., 2] == 128.0).all()
    rms = lambda a: float(np.sqrt(np.mean((a - 1.0) ** 2)))  # noqa: E731
    ratio = rms(weighted.colour) / rms(plain.colour)
    print(f"{W}x{H}, eight frames of 1 and 31 samples: RMS error weighted {rms(weighted.colour):.5f}, equally weighted {rms(plain.colour):.5f}, "
          f"ratio {ratio:.3f} (theory 0.348)")
    assert ratio < 0.5


def test_what_reaches_the_device_scene_without_a_device():
    """``WorldQueries.accumulated_weighted`` hands the frame, the samples, the history and the camera to ``DeviceScene.weighted`` and
    wraps what comes back; ``WeightedAccumulator`` starts from lengths of zero, chains the histories, remembers the camera of the
    frame before and makes two calls per update; the shader hands it ``samples`` at the hits on frame 0 and ``taken`` afterwards."""
    from types import SimpleNamespace

    from pytracer_amd import shaders
    from pytracer_amd import hostmodel as hm

    seen, estimates = [], []
    H, W = 3, 4

    class Scene:
        device = 0

        def weighted(self, colour, samples, shape_index, normal, point, prev_colour, prev_moments, prev_shape, prev_normal, prev_point, prev_count,
                     prev_camera, width, height, **params):
            seen.append(SimpleNamespace(colour=colour, samples=samples, prev_colour=prev_colour, prev_moments=prev_moments, prev_count=prev_count,
                                        camera=prev_camera, size=(width, height), params=params))
            k = np.ones(height * width) if samples is None else np.asarray(samples, dtype=np.float64)
            moments = np.asarray(prev_moments).reshape(height, width, 3) + np.stack([k * 0, k * 0, k], axis=-1).reshape(height, width, 3)
            return np.asarray(colour).reshape(height, width, 3) + 1.0, moments, np.asarray(prev_count).reshape(height, width) + 1

        def variance_estimate(self, moments, count, shape_index, normal, point, width, height, **params):
            estimates.append(SimpleNamespace(moments=moments, count=count, size=(width, height), params=params))
            return np.full((height, width), 0.25)

    wq = rb.WorldQueries(Scene())
    frame = SimpleNamespace(shape_index=np.zeros((1, H, W), np.int32), point=np.zeros((1, H, W, 3)), normal=np.ones((1, H, W, 3)))
    frame.shape_index[0, 0, 0] = -1
    values = np.arange(H * W * 3.0).reshape(H, W, 3)
    cam_a, cam_b = cameras()["perspective"], cameras()["orthogonal"]
    k = np.arange(H * W, dtype=np.int32).reshape(H, W)
    new = wq.accumulated_weighted(values, k, frame, rb.WeightedHistory.empty(W, H), cam_a, max_weight=9.0)
    assert isinstance(new, rb.WeightedHistory) and isinstance(new, rb.TemporalHistory) and np.array_equal(new.colour, values + 1.0)
    assert np.array_equal(new.moments[..., 2], k) and (new.count == 1).all() and seen[-1].params == dict(max_weight=9.0)
    assert seen[-1].size == (W, H) and seen[-1].samples.shape == (H * W,) and seen[-1].prev_moments.shape == (H * W, 3) and seen[-1].camera is cam_a
    assert wq.accumulated_weighted(values, None, frame, new, cam_b).count.max() == 2 and seen[-1].samples is None
    with pytest.raises(ValueError, match="sample counts"):
        wq.accumulated_weighted(values, k[:2], frame, new, cam_a)
    with pytest.raises(ValueError, match="history"):
        wq.accumulated_weighted(values, k, frame, rb.WeightedHistory.empty(W + 1, H), cam_a)
    # the accumulator: two calls per update
    del seen[:]
    acc = rb.WeightedAccumulator(wq, max_history=3, max_weight=7.0, blend_weight=True, min_history=2, normal_min=0.5)
    assert acc.count is None and acc.weight is None and acc.frames == 0
    e, variance = acc.update(values, frame, cam_a, samples=k)
    assert np.array_equal(e, values + 1.0) and (variance == 0.25).all() and acc.frames == 1 and len(seen) == 1 and len(estimates) == 1
    assert not seen[0].prev_count.any() and seen[0].params == dict(max_history=3, max_weight=7.0, blend_weight=True, normal_min=0.5)
    assert estimates[0].params == dict(min_history=2, normal_min=0.5) and estimates[0].size == (W, H)
    assert np.array_equal(np.asarray(estimates[0].moments).reshape(H, W, 3), acc.moments) and np.array_equal(acc.weight, k)
    acc.update(values * 2.0, frame, cam_b)
    assert seen[1].samples is None and seen[1].camera.kind == abi.CAMERA_PERSPECTIVE and (acc.count == 2).all()  # (the camera BEFORE)
    assert np.array_equal(seen[1].prev_colour.reshape(H, W, 3), e) and np.array_equal(acc.weight, k + 1)
    acc.reset()
    assert acc.count is None and acc.weight is None and acc.frames == 0
    with pytest.raises(TypeError, match="unknown accumulation or estimate parameter"):
        rb.WeightedAccumulator(wq, passes=3)
    with pytest.raises(ValueError, match="device=True"):
        rb.WeightedAccumulator(wq, stream=1)
    with pytest.raises(ValueError, match="device=True"):
        acc.update(values, frame, cam_a, width=W, height=H)
    with pytest.raises(ValueError, match="width= and height="):
        rb.WeightedAccumulator(wq, device=True).update(0, rb.DeviceGuides(0, 0, 0), cam_a)
    with pytest.raises(TypeError, match="DeviceGuides"):
        rb.WeightedAccumulator(wq, device=True).update(0, frame, cam_a, width=W, height=H)
    # the shader
    world, order = hm.World(), []
    scene = Scene()
    taken = np.arange(H * W, dtype=np.int32).reshape(1, H, W) % 3

    class Queries:
        def __init__(self):
            self.scene = scene

        def hemisphere_radiance(self, hits, samples, *a, **kw):
            order.append(("gather", samples, kw))
            return SimpleNamespace(radiance=np.zeros((1, H, W, 3)))

        def sample_counts(self, values, hits, variance, **params):
            order.append(("counts", params))
            return np.full((H, W), 2, np.int32)

        def hemisphere_radiance_ragged(self, hits, counts, capacity, *a, **kw):
            order.append(("ragged", capacity, kw))
            return SimpleNamespace(radiance=np.zeros((1, H, W, 3)), taken=taken)

        accumulated_weighted = rb.WorldQueries.accumulated_weighted

        def variance_filtered(self, values, hits, variance=None, **params):
            order.append(("filter", params))
            return np.asarray(values), variance

        def materials(self, hits):
            hit = np.asarray(hits.shape_index) >= 0
            return SimpleNamespace(emitted=np.full((1, H, W, 3), 0.5), brdf_color=np.full((1, H, W, 3), 0.25), hit=hit)

    tracer = SimpleNamespace(world_queries=lambda w: Queries() if w is world else None, camera=cam_a)
    shader = shaders.WeightedAdaptiveGatherShader(world, tracer, samples=4, min_samples=0, max_samples=8, budget=11, max_weight=64.0, blend_weight=True,
                                                  max_history=9, passes=2)
    assert shader.count_params["min_samples"] == 0 and shader.history_params == dict(max_history=9, max_weight=64.0, blend_weight=True)
    del seen[:]
    shader.shade_hits(frame)
    assert [o[0] for o in order] == ["gather", "filter"] and isinstance(shader.accumulator, rb.WeightedAccumulator)
    assert np.array_equal(seen[0].samples.reshape(H, W), np.where(frame.shape_index[0] >= 0, 4, 0))  # (`samples` at the hit records)
    assert seen[0].params == dict(max_history=9, max_weight=64.0, blend_weight=True)
    del order[:]
    shader.shade_hits(frame)
    assert [o[0] for o in order] == ["counts", "ragged", "filter"] and order[0][1]["min_samples"] == 0 and order[1][1] == 11
    assert np.array_equal(seen[1].samples.reshape(H, W), taken[0]) and shader.last_total == int(taken.sum()) and shader.frame_no == 2
    with pytest.raises(ValueError, match="min_samples >= 0"):
        shaders.WeightedAdaptiveGatherShader(world, tracer, min_samples=-1)
    with pytest.raises(TypeError, match="WeightedAdaptiveGatherShader: unknown"):
        shaders.WeightedAdaptiveGatherShader(world, tracer, flags=1)
    with pytest.raises(ValueError, match="min_samples >= 1"):
        shaders.AdaptiveGatherShader(world, tracer, min_samples=0)  # (the unweighted shader keeps its rule)
    with pytest.raises(TypeError, match="unknown"):
        shaders.AdaptiveGatherShader(world, tracer, max_weight=3.0)
    assert "OUT OF SCOPE" in shaders.AdaptiveGatherShader.__doc__ and "WeightedAdaptiveGatherShader" in shaders.AdaptiveGatherShader.__doc__
    assert "min_samples = 0" in shaders.WeightedAdaptiveGatherShader.__doc__ and "budget" in shaders.WeightedAdaptiveGatherShader.__doc__
