"""CPU-only tests of the adaptive queries (include/ptrace_adaptive.h, libptrace_adaptive.so, pytracer_amd.rays): the thirteenth library
builds and loads without a GPU and leaves the other twelve as they were; its header, the ctypes table and its dynamic symbols agree;
every refusal of the interface happens before any HIP call; the numpy mirrors the GPU's bit tests compare with do what the header says
on hand-made pixels (each expectation below is worked out by hand or by a scalar loop written from the header alone); and the host-side
arithmetic of the library -- sizes, plane offsets, the checks of values -- runs in a program of its own under the host sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import rays as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE, ERR_NODEVICE = -1, -3, -5, -6  # include/ptrace.h
V111 = (1 << 16) | 11
INF, NAN = float("inf"), float("nan")
NOWHERE = 2 ** 20  # a device no machine has: a call that passes every argument check ends at the device check, with or without a GPU


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _adaptive_lib, build

    build.build()
    assert os.path.exists(build.ADAPTIVE_LIB) and not build.needs_build()
    return _adaptive_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_error_codes_are_the_headers():
    header = open(os.path.join(ROOT, "include", "ptrace.h")).read()
    for name, value in (("PT_ERR_INVALID", ERR_INVALID), ("PT_ERR_UNSUPPORTED", ERR_UNSUPPORTED), ("PT_ERR_SIZE", ERR_SIZE),
                        ("PT_ERR_NODEVICE", ERR_NODEVICE)):
        assert int(re.search(rf"#define {name}\s+\(?(-?\d+)\)?", header).group(1)) == value, name


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _adaptive_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_adaptive.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_adaptive_lib.EXPORTS) == {s for s, _, _ in _adaptive_lib._SIGNATURES} and len(declared) == 14
    assert all(s.startswith("pt_rays_adaptive_") for s in declared)
    assert _exported(_adaptive_lib.lib_path()) == declared
    assert lib.pt_rays_adaptive_version() == V111
    # an add-on like the twelve before it: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _adaptive_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_adaptive.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _adaptive_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    # the only file that includes the new device header is the new translation unit; the host layer is the shared one
    users = [f for f in os.listdir(build.CSRC) if '"pt_adaptive.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_adaptive.hip"]
    unit = open(os.path.join(build.CSRC, "ptrace_adaptive.hip")).read()
    assert set(re.findall(r'#include "(pt_\w+\.h)"', unit)) == {"pt_kernels.h", "pt_adaptive.h", "pt_host_common.h", "pt_adaptive_host.h"}
    text = unit + open(os.path.join(build.CSRC, "pt_adaptive.h")).read() + open(os.path.join(build.CSRC, "pt_adaptive_host.h")).read()
    assert not re.search(r"\bg_err\b|\bstruct\s+Staged\b|#\s*define\s+HIP_TRY\b", text)
    # no atomic of any kind is called, and nothing spins: within a launch no wave waits for another workgroup
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text) and "volatile" not in text.replace('asm volatile', '')
    assert "PTRACE_ADAPTIVE_LANES" in text
    # the other headers do not know this one's symbols
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ptrace_adaptive.h":
            assert "pt_rays_adaptive" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the two structs
    assert C.sizeof(_adaptive_lib.CountParams) == 32 and C.sizeof(_adaptive_lib.AdaptiveParams) == 64
    fields = re.findall(r"^\s+(?:int|double|unsigned long long|long long)\s+(\w+)(?:\[3\])?;", header, flags=re.M)
    assert fields == [f[0] for f in _adaptive_lib.CountParams._fields_] + [f[0] for f in _adaptive_lib.AdaptiveParams._fields_]
    for name, value in (("PT_ADAPTIVE_COUNT", rb.ADAPTIVE_COUNT), ("PT_ADAPTIVE_TAKEN", rb.ADAPTIVE_TAKEN), ("PT_ADAPTIVE_ALL", rb.ADAPTIVE_ALL),
                        ("PT_ADAPTIVE_MAX_SAMPLES", rb.MAX_SAMPLES), ("PT_ADAPTIVE_MAX_LEVELS", 64)):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == value, name
    assert (_adaptive_lib.ADAPTIVE_COUNT, _adaptive_lib.ADAPTIVE_TAKEN, _adaptive_lib.ADAPTIVE_ALL, _adaptive_lib.MAX_SAMPLES) == (1, 2, 3, 2 ** 20)
    par = _adaptive_lib.count_params()
    assert {k: getattr(par, k) for k in _adaptive_lib.DEFAULTS} == _adaptive_lib.DEFAULTS
    for word in ("bit for bit", "BIT FOR BIT", "want = (gain * v) / (tl * tl)", "k = t + ((double)t < want ? 1 : 0)", "(unknown counts as noisy)",
                 "K_i    = min(max(counts[i], 0), max(capacity - offsets[i], 0))", "init_seq + offsets[i]", "STRICTLY in k order",
                 "GARBAGE", "[0, capacity)", "PTRACE_ADAPTIVE_LANES", "OWNER PLANE", "PTRACE_ADAPTIVE_LOOKUP=search", "PADDED to up8(4 n) bytes",
                 "No workgroup waits for another"):
        assert word in header, word
    # pt_adaptive.h says which way a sample finds its record, and why
    assert "FINDING A SAMPLE'S RECORD" in text and "the measurement chose" in text and "PTRACE_ADAPTIVE_LOOKUP" in text


def test_the_pinned_build_tables_are_unchanged_and_the_new_row_is_in_its_own(lib):
    from pytracer_amd import build

    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_adaptive.h")), "ptrace_adaptive.hip", "pt_adaptive.h", "pt_adaptive_host.h"} <= deps
    assert [len(t) for t in (build.TARGETS, build.ALL_TARGETS, build.EVERY_TARGET, build.BUILD_TARGETS, build.WALK_TARGETS, build.FRAME_TARGETS,
                             build.GUIDED_TARGETS, build.SAMPLED_TARGETS)] == [6, 7, 8, 9, 10, 11, 12, 13]
    assert build.GUIDED_TARGETS == build.FRAME_TARGETS + ((build.VARIANCE_FLAGS, build.VARIANCE_LIB, build.VARIANCE_SOURCES),)
    assert list(build.VARIANCE_ADDONS) == ["variance"] and list(build.ADAPTIVE_ADDONS) == ["adaptive"]
    assert build.ADAPTIVE_TARGETS == ((build.ADAPTIVE_FLAGS, build.ADAPTIVE_LIB, build.ADAPTIVE_SOURCES),)
    assert build.SAMPLED_TARGETS == build.GUIDED_TARGETS + build.ADAPTIVE_TARGETS and build.SAMPLED_TARGETS[-1] == build.ADAPTIVE_TARGETS[0]
    assert build.ADAPTIVE_FLAGS[:-1] == build.FLAGS[:-1] and build.ADAPTIVE_FLAGS[-1] == "-cuid=libptrace_adaptive"
    assert "-ffp-contract=off" in build.ADAPTIVE_FLAGS and not any("fast-math" in f and not f.startswith("-fno") for f in build.ADAPTIVE_FLAGS)
    assert build.ADAPTIVE_SOURCES == ["ptrace_adaptive.hip"] and os.path.basename(build.ADAPTIVE_LIB) == "libptrace_adaptive.so"
    assert all(os.path.exists(t[1]) for t in build.SAMPLED_TARGETS)  # build() made all thirteen


def test_the_other_twelve_libraries_are_what_they_were(lib):
    from pytracer_amd import _gather_lib, _variance_lib, build

    assert _exported(_variance_lib.lib_path()) == set(_variance_lib.EXPORTS) and _exported(_gather_lib.lib_path()) == set(_gather_lib.EXPORTS)
    # the recorded hashes: twelve rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "adaptive_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.GUIDED_TARGETS] and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.GUIDED_TARGETS]
    # and the eleven the variance library recorded are still those
    old = [line.split() for line in open(os.path.join(ROOT, "profiles", "variance_hashes.txt")) if line.startswith("libptrace")]
    assert [r[:3] for r in rows[:11]] == [r[:3] for r in old[:11]]


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 130, 2 ** 31 - 1])
def test_sizes_and_offsets_match_the_python_mirror(lib, n):
    up8 = lambda x: (x + 7) // 8 * 8  # noqa: E731
    for channels in range(4):
        size = 24 * n + (8 * n if channels & 1 else 0) + (up8(4 * n) if channels & 2 else 0)
        assert lib.pt_rays_adaptive_bytes(n, channels) == rb.adaptive_bytes(n, channels) == size and size % 8 == 0
        want = {(0, c): 8 * n * c for c in range(3)}
        if channels & 1:
            want[(1, 0)] = 24 * n
        if channels & 2:
            want[(2, 0)] = 24 * n + (8 * n if channels & 1 else 0)
        for sel in (0, 1, 2, 3, 4, -1):
            for comp in (-1, 0, 1, 2, 3):
                got, mirror = lib.pt_rays_adaptive_plane_offset(n, channels, sel, comp), rb.adaptive_plane_offset(n, channels, sel, comp)
                if (sel, comp) in want:
                    assert got == mirror == want[(sel, comp)] and got % 8 == 0, (n, channels, sel, comp)
                else:
                    assert got == ERR_INVALID and mirror == -1, (n, channels, sel, comp)
    for bad in (4, 7, -1, 1 << 20):
        assert lib.pt_rays_adaptive_bytes(n, bad) == 0 and rb.adaptive_bytes(n, bad) == 0
        assert lib.pt_rays_adaptive_plane_offset(n, bad, 0, 0) == ERR_INVALID and rb.adaptive_plane_offset(n, bad, 0, 0) == -1
    assert lib.pt_rays_adaptive_offsets_bytes(n) == 8 * (n + 1)
    assert lib.pt_rays_adaptive_offsets_workspace_bytes(n) == 8 * max((n + 255) // 256, 1)
    for bad_n in (-1, 2 ** 31):
        assert lib.pt_rays_adaptive_bytes(bad_n, 1) == 0 and rb.adaptive_bytes(bad_n, 1) == 0
        assert lib.pt_rays_adaptive_offsets_bytes(bad_n) == 0 and lib.pt_rays_adaptive_offsets_workspace_bytes(bad_n) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731


def test_every_refusal_happens_before_any_hip_call(lib):
    """Every call names a device that does not exist, so nothing is ever launched: a call that passes the argument checks ends at the
    first HIP call, the device check (PT_ERR_NODEVICE without a GPU, "out of range" with one); whatever is refused otherwise was
    refused by the argument checks before it."""
    from pytracer_amd import _adaptive_lib

    err = _adaptive_lib.last_error

    def passed(rc):
        return rc == ERR_NODEVICE or (rc == ERR_INVALID and "out of range" in err())

    m = 15
    var, col, shp, cnt = np.zeros(m), np.zeros((3, m)), np.zeros(m, np.int32), np.zeros(m, np.int32)
    offs, ws8 = np.zeros(m + 1, np.int64), np.zeros(64, np.uint8)

    def nbytes(a, given):
        return (a.nbytes if a is not None else 0) if given is None else given

    def counts(device=NOWHERE, m_=m, par=True, v=var, c=col, s=shp, o=cnt, ob=None, **kw):
        par = C.byref(_adaptive_lib.count_params(**kw)) if par else None
        args = [device, m_, par, p(v), p(c), p(s), p(o), nbytes(o, ob)]
        return lib.pt_rays_adaptive_counts(*args), lib.pt_rays_adaptive_counts_device(*args, None)

    def offsets(device=NOWHERE, n_=m, c=cnt, o=offs, ob=None, ws=ws8, wsb=None):
        args = [device, n_, p(c), p(o), nbytes(o, ob)]
        return lib.pt_rays_adaptive_offsets(*args), lib.pt_rays_adaptive_offsets_device(*args, p(ws), nbytes(ws, wsb), None)

    # 1. counts
    assert all(passed(rc) for rc in counts())
    for kw in (dict(min_samples=0, max_samples=0), dict(min_samples=0, max_samples=2 ** 20), dict(min_samples=2 ** 20, max_samples=2 ** 20),
               dict(tolerance=INF), dict(tolerance=5e-324, luminance_floor=5e-324, gain=5e-324), dict(luminance_floor=1e308, gain=1e308)):
        assert all(passed(rc) for rc in counts(**kw)), kw
    for kw in (dict(min_samples=-1), dict(min_samples=5, max_samples=4), dict(max_samples=2 ** 20 + 1), dict(min_samples=2 ** 31 - 1, max_samples=2 ** 31 - 1)):
        assert counts(**kw) == both(ERR_INVALID) and "min <= max" in err(), kw
    for bad in (0.0, -0.0, -1.0, -INF, NAN):
        assert counts(tolerance=bad) == both(ERR_INVALID) and "tolerance" in err(), bad
    for name in ("luminance_floor", "gain"):
        for bad in (0.0, -0.0, -1.0, INF, -INF, NAN):
            assert counts(**{name: bad}) == both(ERR_INVALID) and name in err(), (name, bad)
    assert counts(par=False) == both(ERR_INVALID) and "null pt_adaptive_count_params" in err()
    assert counts(m_=-1) == both(ERR_INVALID) and counts(m_=2 ** 31, ob=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in err()
    assert counts(device=-1) == both(ERR_INVALID)
    for name in ("v", "c", "s"):
        assert counts(**{name: None}) == both(ERR_INVALID) and "null" in err(), name
    assert counts(o=None, ob=cnt.nbytes) == both(ERR_INVALID) and "null counts output" in err()
    assert counts(ob=4 * m - 1) == both(ERR_SIZE) and "too small" in err()
    assert counts(m_=0, v=None, c=None, s=None, o=None) == both(0)
    assert counts(m_=0, min_samples=-1) == both(ERR_INVALID)  # (the struct is still checked)
    # 2. offsets
    assert all(passed(rc) for rc in offsets())
    assert offsets(n_=-1) == both(ERR_INVALID) and offsets(n_=2 ** 31, ob=2 ** 40) == both(ERR_INVALID) and offsets(device=-1) == both(ERR_INVALID)
    assert offsets(c=None) == both(ERR_INVALID) and offsets(o=None, ob=offs.nbytes) == both(ERR_INVALID) and "null offsets output" in err()
    assert offsets(ob=8 * m) == both(ERR_SIZE) and all(passed(rc) for rc in offsets(ob=8 * m + 8))
    rc = offsets(ws=None, wsb=64)
    assert passed(rc[0]) and rc[1] == ERR_INVALID and "null workspace" in err()  # (the host form makes its own)
    assert offsets(n_=257, ob=2 ** 20, wsb=8)[1] == ERR_SIZE and "workspace" in err() and passed(offsets(n_=257, ob=2 ** 20, wsb=16)[1])
    assert offsets(n_=0, c=None, o=None) == both(0) and not offs.any()
    # 3. the gather
    nb = int(lib.pt_rays_adaptive_args_bytes())
    block = (C.c_char * nb)()
    np.frombuffer(block, dtype=np.uint8)[:] = 1  # (a block whose `cold` pointer is set and whose shape count is positive)
    n = 5
    pts, nrm = np.zeros((3, n)), np.zeros((3, n))
    act, seq = np.zeros(n, np.int32), np.zeros(n, np.uint64)
    kc, ko = np.full(n, 3, np.int32), 3 * np.arange(n + 1, dtype=np.int64)
    out = np.zeros(rb.adaptive_bytes(n, 3), np.uint8)
    ws = np.zeros(4096, np.uint8)

    def gather(device=NOWHERE, blk=block, nbytes_=nb, p_=pts, n_=nrm, a_=act, s_=seq, c_=kc, o_=ko, count=n, N=1, D=3, limit=2, depth=0, cap=15,
               ch=3, o=out, ob=None, wb=None, null_par=False):
        par = None if null_par else C.byref(_adaptive_lib.AdaptiveParams(N, D, limit, depth, 42, 54, (C.c_double * 3)(0, 0, 0), cap))
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        host = lib.pt_rays_adaptive_gather(device, blk, nbytes_, p(p_), p(n_), p(a_), p(s_), p(c_), p(o_), count, par, ch, p(o), ob)
        dev = lib.pt_rays_adaptive_gather_device(device, blk, nbytes_, p(p_), p(n_), p(a_), p(s_), p(c_), p(o_), count, par, ch, p(ws),
                                                 ws.nbytes if wb is None else wb, p(o), ob, None)
        return host, dev

    assert all(passed(rc) for rc in gather())
    assert gather(N=0) == both(ERR_INVALID) and "num_of_rays" in err()
    assert gather(D=-1) == both(ERR_INVALID)
    assert gather(depth=-1) == both(ERR_INVALID) and "depth" in err()
    assert gather(count=-1) == both(ERR_INVALID) and gather(count=2 ** 31) == both(ERR_INVALID)
    assert gather(cap=-1) == both(ERR_INVALID) and "capacity" in err() and gather(cap=2 ** 31) == both(ERR_INVALID) and "capacity" in err()
    assert all(passed(rc) for rc in gather(cap=0)) and passed(gather(cap=2 ** 31 - 1)[0])
    assert gather(D=65) == both(ERR_UNSUPPORTED) and "64 levels" in err()
    assert gather(D=2 ** 31 - 1, depth=2 ** 31 - 66) == both(ERR_UNSUPPORTED)
    assert passed(gather(D=2 ** 31 - 1, depth=2 ** 31 - 65)[0])  # 64 levels: accepted
    assert passed(gather(D=3, depth=7)[0])  # deeper than max_depth: legal (black)
    assert gather(ch=4) == both(ERR_INVALID) and gather(ch=-1) == both(ERR_INVALID) and "channel bits" in err()
    assert gather(device=-1) == both(ERR_INVALID)
    assert gather(blk=None) == both(ERR_INVALID)
    assert gather(nbytes_=nb - 8) == both(ERR_INVALID) and "one build" in err()
    assert gather(nbytes_=nb + 8) == both(ERR_INVALID)
    assert gather(null_par=True) == both(ERR_INVALID) and "null pt_adaptive_params" in err()
    for missing in ("p_", "n_", "o"):
        assert gather(**{missing: None}, ob=out.nbytes) == both(ERR_INVALID), missing
    for missing in ("c_", "o_"):
        assert gather(**{missing: None}) == both(ERR_INVALID) and "null counts or offsets" in err(), missing
    for optional in ("a_", "s_"):  # NULL: every record is active / seq_i = init_seq + offsets[i]
        assert all(passed(rc) for rc in gather(**{optional: None})), optional
    assert gather(ob=out.nbytes - 1) == both(ERR_SIZE) and "too small" in err()
    assert gather(ob=rb.adaptive_bytes(n, 1), ch=3) == both(ERR_SIZE) and passed(gather(ob=rb.adaptive_bytes(n, 1), ch=1)[0])
    # a workspace that cannot even hold the sample planes (4 x 8 bytes per sample of capacity): refused without asking a device
    assert gather(wb=15 * 32 - 1)[1] == ERR_SIZE and "workspace" in err() and passed(gather(wb=15 * 32)[1])
    assert gather(wb=0, cap=0)[1] != ERR_SIZE
    assert lib.pt_rays_adaptive_gather_device(NOWHERE, block, nb, p(pts), p(nrm), None, None, p(kc), p(ko), n,
                                              C.byref(_adaptive_lib.params(1, 3, 2, 0, 42, 54, (0, 0, 0), 15)), 3, None, 0, p(out), out.nbytes,
                                              None) == ERR_INVALID and "workspace" in err()
    # n = 0: PT_OK with nothing launched (no device is touched), null planes allowed
    assert gather(count=0, p_=None, n_=None, a_=None, s_=None, c_=None, o_=None, o=None) == both(0)
    assert not out.any()
    # the workspace's size: 0 on refusal, with the reason
    assert lib.pt_rays_adaptive_workspace_bytes(0, 10, 30, 1, 65, 0) == 0 and "64 levels" in err()
    assert lib.pt_rays_adaptive_workspace_bytes(0, 10, -1, 1, 3, 0) == 0 and "capacity" in err()
    assert lib.pt_rays_adaptive_workspace_bytes(0, 10, 2 ** 31, 1, 3, 0) == 0 and lib.pt_rays_adaptive_workspace_bytes(0, 10, 30, 0, 3, 0) == 0
    assert lib.pt_rays_adaptive_workspace_bytes(-1, 10, 30, 1, 3, 0) == 0 and lib.pt_rays_adaptive_workspace_bytes(0, -1, 30, 1, 3, 0) == 0


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------------------
def _counts_by_the_header(variance, colour, shape, min_samples, max_samples, tolerance, luminance_floor, gain):
    """The rule of include/ptrace_adaptive.h, one pixel at a time in Python floats (IEEE fp64, one rounding per operation)."""
    out = []
    for v, c, s in zip(variance, colour, shape):
        if s < 0:
            out.append(0)
            continue
        c = [float(x) for x in c]
        mx, mn = c[0], c[0]
        if c[1] > mx: mx = c[1]  # noqa: E701
        if c[2] > mx: mx = c[2]  # noqa: E701
        if c[1] < mn: mn = c[1]  # noqa: E701
        if c[2] < mn: mn = c[2]  # noqa: E701
        l = (mx + mn) / 2.0
        if not l > luminance_floor:
            l = luminance_floor
        tl = tolerance * l
        v = float(v)
        try:
            want = (gain * v) / (tl * tl)
        except (ZeroDivisionError, OverflowError):
            want = NAN if gain * v == 0.0 or math.isnan(v) else math.copysign(INF, v)
        if not v >= 0.0 or not want < float(max_samples):
            out.append(max_samples)
            continue
        t = int(want)
        k = t + (1 if float(t) < want else 0)
        out.append(max(k, min_samples))
    return np.array(out, dtype=np.int32)


def test_sample_counts_on_hand_made_pixels():
    # tolerance 0.5 and luminance 2 (grey 2): tl = 1, so want = gain * v exactly
    par = dict(min_samples=2, max_samples=32, tolerance=0.5, luminance_floor=0.25, gain=1.0)
    grey2 = [2.0, 2.0, 2.0]
    above = np.nextafter(7.0, INF)  # one ulp above an integer
    pixels = [(7.0, grey2, 0, 7),            # want exactly an integer: no rounding up
              (above, grey2, 0, 8),          # one ulp above it: the next integer
              (np.nextafter(7.0, 0.0), grey2, 0, 7),
              (0.0, grey2, 0, 2),            # no variance: min_samples
              (-0.0, grey2, 0, 2),           # (-0.0 >= 0)
              (-1e-300, grey2, 0, 32),       # negative: unknown counts as noisy
              (NAN, grey2, 0, 32),
              (INF, grey2, 0, 32),
              (-INF, grey2, 0, 32),
              (31.5, grey2, 0, 32),          # the last count below the cap
              (32.0, grey2, 0, 32),          # !(want < max)
              (1e300, grey2, 0, 32),
              (0.5, grey2, 0, 2),            # ceil gives 1, raised to min_samples
              (1.0, [0.1, 0.1, 0.1], 0, 32),   # l below the floor: l = 0.25, tl = 0.125, want = 64
              (0.25, [0.1, 0.1, 0.1], 0, 16),  # want = 0.25 / 0.015625 = 16
              (0.25, [NAN, NAN, NAN], 0, 16),  # a NaN luminance is "not above the floor"
              (0.25, [0.0, 1.0, 4.0], 0, 2),   # lum = (4 + 0) / 2 = 2: want 0.25 -> 1 -> min
              (5.0, grey2, -1, 0),           # no record: no samples
              (NAN, grey2, -7, 0)]
    v, c, s, want = (np.array([px[i] for px in pixels]) for i in range(4))
    got = rb.sample_counts_host(v, c, s, **par)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert got.tolist() == _counts_by_the_header(v, c, s, **par).tolist()
    # min = 0: a converged pixel gets nothing; min = max: every record gets that, whatever its variance
    zero_min = rb.sample_counts_host(v, c, s, **dict(par, min_samples=0))
    assert zero_min.tolist() == _counts_by_the_header(v, c, s, **dict(par, min_samples=0)).tolist()
    assert zero_min[3] == 0 and zero_min[4] == 0 and zero_min[12] == 1 and zero_min[16] == 1 and zero_min[0] == 7
    flat = rb.sample_counts_host(v, c, s, **dict(par, min_samples=9, max_samples=9))
    assert flat.tolist() == [0 if x < 0 else 9 for x in s]
    # the result is shaped like the variance
    assert rb.sample_counts_host(v[:18].reshape(3, 6), c[:18].reshape(3, 6, 3), s[:18].reshape(3, 6), **par).shape == (3, 6)
    # random pixels against the scalar loop
    rng = np.random.default_rng(11)
    v = np.abs(rng.standard_normal(500)) * 10.0 ** rng.integers(-6, 3, 500)
    c = np.abs(rng.standard_normal((500, 3)))
    s = rng.integers(-1, 4, 500).astype(np.int32)
    for kw in (dict(), dict(tolerance=0.01, gain=3.0, max_samples=2 ** 20), dict(tolerance=INF), dict(luminance_floor=5.0, min_samples=0, gain=1e-3)):
        full = dict(dict(min_samples=1, max_samples=32, tolerance=0.05, luminance_floor=1.0, gain=1.0), **kw)
        assert rb.sample_counts_host(v, c, s, **kw).tolist() == _counts_by_the_header(v, c, s, **full).tolist(), kw
    for bad in (dict(min_samples=-1), dict(max_samples=2 ** 20 + 1), dict(min_samples=3, max_samples=2), dict(tolerance=0.0), dict(tolerance=NAN),
                dict(luminance_floor=INF), dict(gain=0.0), dict(gain=INF)):
        with pytest.raises(ValueError):
            rb.sample_counts_host(v, c, s, **bad)


def test_sample_offsets_and_the_truncation_rule():
    counts = np.array([3, 0, -5, 2, 1, -1, 4], np.int32)
    off = rb.sample_offsets_host(counts)
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 3, 3, 5, 6, 6, 10]
    assert rb.sample_offsets_host(np.zeros(0, np.int32)).tolist() == [0]
    # sums beyond 2^31, and beyond 2^32: int64 all the way
    big = np.full(5000, 2 ** 20, np.int32)
    big[::7] = -2 ** 31
    want = np.concatenate([[0], np.cumsum(np.maximum(big.astype(object), 0))])
    got = rb.sample_offsets_host(big)
    assert got.tolist() == [int(x) for x in want] and got[-1] > 2 ** 32
    assert rb.sample_offsets_host(np.full(3, 2 ** 31 - 1, np.int32)).tolist() == [0, 2 ** 31 - 1, 2 ** 32 - 2, 3 * (2 ** 31 - 1)]
    # K_i = min(max(counts[i], 0), max(capacity - offsets[i], 0))
    total = int(off[-1])
    assert rb.samples_taken_host(counts, off, total).tolist() == [3, 0, 0, 2, 1, 0, 4] == rb.samples_taken_host(counts, off, total + 100).tolist()
    assert rb.samples_taken_host(counts, off, 0).tolist() == [0] * 7
    assert rb.samples_taken_host(counts, off, 4).tolist() == [3, 0, 0, 1, 0, 0, 0]   # in the middle of record 3
    assert rb.samples_taken_host(counts, off, 5).tolist() == [3, 0, 0, 2, 0, 0, 0]   # at a record's boundary
    assert rb.samples_taken_host(counts, off, 8).tolist() == [3, 0, 0, 2, 1, 0, 2]
    for cap in range(total + 2):
        taken = rb.samples_taken_host(counts, off, cap)
        assert taken.sum() == min(cap, total) and all(0 <= off[i] + k < cap for i in range(7) for k in range(taken[i]))
    with pytest.raises(ValueError):
        rb.samples_taken_host(counts, off[:-1], 5)


def test_gain_for_budget_is_the_largest_gain_within_the_budget():
    rng = np.random.default_rng(5)
    m = 400
    v = np.abs(rng.standard_normal(m)) * 1e-3
    c = 0.2 + np.abs(rng.standard_normal((m, 3)))
    s = rng.integers(-1, 3, m).astype(np.int32)
    par = dict(min_samples=1, max_samples=32, tolerance=0.05, luminance_floor=0.05)
    total = lambda g: int(rb.sample_counts_host(v, c, s, gain=g, **par).astype(np.int64).sum())  # noqa: E731
    hit = int((s >= 0).sum())
    for budget in (hit, hit + 1, 4 * hit, 17 * hit + 3, 32 * hit - 1):
        g = rb.gain_for_budget(v, c, s, budget, **par)
        assert g > 0 and math.isfinite(g) and total(g) <= budget < total(float(np.nextafter(g, INF))), budget
    # a budget nothing exceeds: every count is at max_samples (all variances here are positive)
    g = rb.gain_for_budget(v + 1e-9, c, s, 32 * hit, **par)
    assert total(g) == 32 * hit and set(rb.sample_counts_host(v + 1e-9, c, s, gain=g, **par)[s >= 0].tolist()) == {32}
    with pytest.raises(ValueError, match="least"):
        rb.gain_for_budget(v, c, s, hit - 1, **par)
    with pytest.raises(TypeError):
        rb.gain_for_budget(v, c, s, 4 * hit, gain=2.0, **par)
    # the total is monotone in the gain (what the bisection rests on)
    totals = [total(g) for g in 10.0 ** np.arange(-6.0, 7.0)]
    assert totals == sorted(totals) and totals[0] == hit and totals[-1] > 20 * hit


def test_channel_names_the_views_and_the_parameter_blocks():
    from pytracer_amd import _adaptive_lib

    assert rb.adaptive_channels("all") == 3 and rb.adaptive_channels("none") == 0 and rb.adaptive_channels("count") == 1
    assert rb.adaptive_channels("taken") == 2 and rb.adaptive_channels("taken, count") == 3 and rb.adaptive_channels(2) == 2
    for bad in ("pcg", 4, -1):
        with pytest.raises(ValueError):
            rb.adaptive_channels(bad)
    n = 5  # (odd: the taken plane is padded)
    buf = np.zeros(rb.adaptive_bytes(n, 3), np.uint8)
    assert buf.nbytes == 24 * n + 8 * n + 24
    buf[: 24 * n].view(np.float64)[:] = np.arange(3 * n)
    buf[24 * n: 32 * n].view(np.uint64)[:] = np.arange(100, 100 + n)
    buf[32 * n: 32 * n + 4 * n].view(np.int32)[:] = np.arange(7, 7 + n)
    res = rb.RaggedRadiance(buf, n, "all", shape=(1, 5))
    assert res.radiance.shape == (1, 5, 3) and np.array_equal(res.radiance[0, 2], [2.0, 7.0, 12.0])
    assert res.n_rays[0, 3] == 103 and res.taken.dtype == np.int32 and res.taken[0].tolist() == [7, 8, 9, 10, 11]
    assert np.shares_memory(res.taken, buf) and set(res.planes()) == {"radiance", "n_rays", "taken"}
    only = rb.RaggedRadiance(np.zeros(rb.adaptive_bytes(n, 2), np.uint8), n, "taken")
    assert not only.has("count") and only.has("taken") and only.taken.shape == (5,) and set(only.planes()) == {"radiance", "taken"}
    with pytest.raises(KeyError, match="count"):
        only.n_rays
    with pytest.raises(KeyError, match="taken"):
        rb.RaggedRadiance(np.zeros(rb.adaptive_bytes(n, 1), np.uint8), n, "count").taken
    with pytest.raises(ValueError):
        rb.RaggedRadiance(np.zeros(8, np.uint8), n)
    par = _adaptive_lib.params(1, 10, 3, 0, -1, 2 ** 64 + 5, (0.5, 0.25, 1), 77)
    assert (par.init_state, par.init_seq, par.capacity, list(par.background)) == (2 ** 64 - 1, 5, 77, [0.5, 0.25, 1.0])
    with pytest.raises(ValueError, match="capacity"):
        _adaptive_lib.params(1, 10, 3, 0, 42, 54, (0, 0, 0), 2 ** 63)


def test_the_ragged_query_hands_over_counts_offsets_and_the_total():
    """What reaches ``DeviceScene``, without a device: the offsets come from ``sample_offsets``; ``capacity=None`` is their last value;
    a records object hands over its ``shape_index`` as ``active``; the result is shaped like the records."""
    seen = {}

    class Scene:
        def sample_offsets(self, counts):
            seen["offsets_of"] = counts
            return rb.sample_offsets_host(counts)

        def gather_ragged(self, points, normals, counts, offsets, capacity, init_state, seqs, active, *rest, **kw):
            seen.update(points=points, counts=counts, offsets=offsets, capacity=capacity, init_state=init_state, seqs=seqs, active=active, rest=rest, kw=kw)
            bits = rest[5]
            return rb.RaggedRadiance(np.zeros(rb.adaptive_bytes(points.shape[1], bits), np.uint8), points.shape[1], bits)

        def sample_counts(self, variance, colour, shape_index, **params):
            seen.update(variance=variance, colour=colour, shape_index=shape_index, params=params)
            return rb.sample_counts_host(variance, colour, shape_index, **params)

    class Frame:
        shape_index = np.array([[0, -1, 2], [3, 4, -1]], np.int32)
        point = np.arange(18.0).reshape(2, 3, 3)
        normal = -np.arange(18.0).reshape(2, 3, 3)

    wq = rb.WorldQueries(Scene())
    counts = np.array([[2, 0, 1], [5, -1, 3]], np.int32)
    res = wq.hemisphere_radiance_ragged(Frame, counts)
    assert res.radiance.shape == (2, 3, 3) and res.n_rays.shape == (2, 3) and res.taken.shape == (2, 3)
    assert seen["counts"].tolist() == [2, 0, 1, 5, -1, 3] and seen["counts"].dtype == np.int32 and seen["offsets"].tolist() == [0, 2, 2, 3, 8, 8, 11]
    assert seen["capacity"] == 11 and seen["active"] is Frame.shape_index and (seen["init_state"], seen["seqs"]) == (42, None)
    assert seen["rest"] == (1, 10, 3, (0.0, 0.0, 0.0), 0, 3) and seen["kw"] == {"init_seq": 54}  # PathTracer's defaults
    wq.hemisphere_radiance_ragged(np.zeros((6, 3)), counts, 7, normals=np.ones((6, 3)), channels="taken")
    assert seen["capacity"] == 7 and seen["active"] is None and seen["rest"][5] == 2
    with pytest.raises(ValueError, match="normals="):
        wq.hemisphere_radiance_ragged(np.zeros((6, 3)), counts)
    got = wq.sample_counts(np.ones((2, 3, 3)), Frame, np.full((2, 3), 0.01), tolerance=0.1, max_samples=8)
    assert got.shape == (2, 3) and got.tolist() == [[1, 0, 1], [1, 1, 0]] and seen["params"] == dict(tolerance=0.1, max_samples=8)
    with pytest.raises(ValueError, match="variance"):
        wq.sample_counts(np.ones((2, 3, 3)), Frame, np.zeros(5))


def test_the_adaptive_shader_checks_its_parameters():
    from pytracer_amd.shaders import AdaptiveGatherShader, VarianceGuidedGatherShader

    sh = AdaptiveGatherShader(None, None, 4, tolerance=0.1, max_samples=16, sigma_luminance=2.0, max_history=8, budget=1000)
    assert isinstance(sh, VarianceGuidedGatherShader) and sh.budget == 1000
    assert sh.count_params == dict(min_samples=1, max_samples=16, tolerance=0.1, luminance_floor=1.0, gain=1.0)
    assert sh.params == {"sigma_luminance": 2.0} and sh.history_params == {"max_history": 8}
    with pytest.raises(ValueError, match="min_samples"):
        AdaptiveGatherShader(None, None, 4, min_samples=0)
    with pytest.raises(TypeError, match="AdaptiveGatherShader"):
        AdaptiveGatherShader(None, None, 4, sigma_colour=1.0)
    with pytest.raises(TypeError, match="tracer"):
        sh.shade_hits(None)
    assert "OUT OF SCOPE" in AdaptiveGatherShader.__doc__ and "equally" in AdaptiveGatherShader.__doc__


# ---- the host-side arithmetic under the sanitizers, in a program of its own ------------------------------------------------------------------
def test_the_host_side_checks_run_clean_under_the_host_sanitizers(tmp_path):
    """tests/adaptive_checks/adaptive_checks.cpp has its own main, makes no HIP call and is not loaded into Python: sizes, plane offsets
    and the value checks of csrc/pt_adaptive_host.h, compiled with the host AddressSanitizer and UndefinedBehaviorSanitizer."""
    from pytracer_amd import build

    source = os.path.join(ROOT, "tests", "adaptive_checks", "adaptive_checks.cpp")
    exe = str(tmp_path / "adaptive_checks")
    flags = ["-x", "hip", "--offload-host-only", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
             "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([build._hipcc()] + flags + ["-o", exe, source], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.strip().endswith("adaptive checks: ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
