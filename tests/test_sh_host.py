"""CPU-only tests of the probe queries (include/ptrace_sh.h, libptrace_sh.so, pytracer_amd.rays): the eighth library builds and
loads without a GPU and leaves the other seven as they were; its header, the ctypes table and its dynamic symbols agree; sizes and
offsets match their Python mirrors up to 2^31 - 1 probes; every refusal of the interface happens before any HIP call; its
translation unit carries no copy of the shared host layer; the basis' literals, the direction, the band factors and the host
classes are what the header says; and the expected coefficients DEPEND on the order of the sum and survive a one-ulp change of
every direction, so the GPU's bit tests discriminate and its oracle test's outlier cap means something."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import rays as rb

from . import probe_sets as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE = -1, -3, -5  # include/ptrace.h
V16 = (1 << 16) | 6
SIZES = [0, 1, 63, 65, 2 ** 31 - 1]


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _sh_lib, build

    build.build()
    assert os.path.exists(build.SH_LIB) and not build.needs_build()
    return _sh_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _rays_lib, _sh_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_sh.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_sh_lib.EXPORTS) == {s for s, _, _ in _sh_lib._SIGNATURES} and len(declared) == 14
    assert all(s.startswith("pt_rays_sh_") for s in declared)
    assert _exported(_sh_lib.lib_path()) == declared
    # an add-on like the other six: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _sh_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_sh.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _sh_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    assert lib.pt_rays_sh_version() == V16
    assert lib.pt_rays_sh_args_bytes() == _rays_lib.lib().pt_rays_args_bytes() > 0
    # the only file that includes the new device header is the new translation unit, which keeps away from the other walks' headers
    users = [f for f in os.listdir(build.CSRC) if '"pt_sh.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_sh.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_sh.hip")).read() + open(os.path.join(build.CSRC, "pt_sh.h")).read()
    assert '"pt_radiance.h"' not in text and '"pt_gather.h"' not in text and '"pt_bake.h"' not in text
    # the recipe: the pinned tables stay, the new row is in a further one, built with the add-ons' flags and watched
    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_sh.h")), "ptrace_sh.hip", "pt_sh.h"} <= deps
    assert len(build.TARGETS) == 6 and len(build.ALL_TARGETS) == 7 and build.ALL_TARGETS[:6] == build.TARGETS
    assert build.EVERY_TARGET == build.ALL_TARGETS + ((build.SH_FLAGS, build.SH_LIB, build.SH_SOURCES),)
    assert build.SH_FLAGS[:-1] == build.FLAGS[:-1] and build.SH_FLAGS[-1] == "-cuid=libptrace_sh" and "-ffp-contract=off" in build.SH_FLAGS
    assert build.SH_SOURCES == ["ptrace_sh.hip"] and os.path.basename(build.SH_LIB) == "libptrace_sh.so"
    assert C.sizeof(_sh_lib.ShParams) == 64  # five ints (and their padding), two uint64 and three doubles: pt_sh_params
    # the header states its definitions with their citations
    for cite in ("pcg.py:60-62", "pcg.py:25-41", "ray.py", "render.py:99-139", "render.py:128-139", "materials.py:132-152"):
        assert cite in header, cite
    for literal in ("0.28209479177387814", "0.4886025119029199", "1.0925484305920792", "0.31539156525252005", "0.5462742152960396"):
        assert literal in header and literal in text, literal


def test_the_other_seven_libraries_are_what_they_were(lib):
    from pytracer_amd import _bake_lib, _gather_lib, _lib, _radiance_lib, _rays_lib, _scatter_lib, _surface_lib, build

    for module, count in ((_rays_lib, 7), (_surface_lib, 11), (_scatter_lib, 7), (_radiance_lib, 8), (_gather_lib, 8), (_bake_lib, 11)):
        assert _exported(module.lib_path()) == set(module.EXPORTS) and len(module.EXPORTS) == count
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert build.code_hash() == json.load(open(os.path.join(ROOT, "profiles", "pmc_c2.json")))["code_hash"]
    for header in ("ptrace.h", "ptrace_rays.h", "ptrace_surface.h", "ptrace_scatter.h", "ptrace_radiance.h", "ptrace_gather.h", "ptrace_bake.h"):
        assert "pt_rays_sh_" not in open(os.path.join(ROOT, "include", header)).read()
    # the recorded hashes: seven rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "sh_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows[:7]] == [os.path.basename(t[1]) for t in build.ALL_TARGETS] and all(r[1] == r[2] for r in rows[:7])
    assert [r[2] for r in rows[:7]] == [build.code_hash(t[1]) for t in build.ALL_TARGETS]


def test_the_translation_unit_carries_no_copy_of_the_host_layer():
    """tests/test_addon_common.py's checks, for ``sh``."""
    text = open(os.path.join(ROOT, "pytracer_amd", "csrc", "ptrace_sh.hip")).read()
    assert '#include "pt_host_common.h"' in text
    for what in (r"\bg_err\b", r"\bint\s+device_ok\s*\(", r"\bstruct\s+Staged\b", r"\bint\s+fail\s*\(", r"#\s*define\s+HIP_TRY\b",
                 r"\bup8\s*\(size_t", r"\bdim3\s+grid_of\s*\(", r"getenv\s*\(", r"this library's has %zu"):
        assert not re.search(what, text), what
    from pytracer_amd import _sh_lib

    assert _sh_lib.lib_path() == os.environ.get("PTRACE_SH_LIB") or _sh_lib.lib_path() == os.path.join(ROOT, "pytracer_amd", "libptrace_sh.so")


def test_a_missing_library_is_an_import_error_and_nothing_loads_before_the_first_call(tmp_path):
    """The loader follows ``_bake_lib``: ``PTRACE_SH_LIB`` overrides the file, loading is lazy, the text is ``_addon``'s."""
    import sys

    missing = str(tmp_path / "libptrace_sh.so")
    code = ("from pytracer_amd import _sh_lib\nprint('PATH', _sh_lib.lib_path())\n"
            "try:\n    _sh_lib.lib()\nexcept ImportError as e:\n    print('IMPORTERROR', e)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PTRACE_SH_LIB=missing))
    assert r.returncode == 0, r.stderr
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert out["PATH"] == missing and out["IMPORTERROR"].startswith(f"{missing} is missing: the HIP extension has not been built.")
    assert "no CPU fallback" in out["IMPORTERROR"]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_offsets_match_the_python_mirror(lib, n):
    assert lib.pt_rays_sh_eval_bytes(n) == 24 * n
    for channels in range(2):
        planes = 27 + (1 if channels & rb.SH_COUNT else 0)
        assert lib.pt_rays_sh_bytes(n, channels) == rb.sh_bytes(n, channels) == 8 * n * planes
        want = {(0, c): 8 * n * c for c in range(27)}
        if channels & rb.SH_COUNT:
            want[(rb.SH_COUNT, 0)] = 216 * n
        for sel in (0, rb.SH_COUNT, 2, 3, -1):
            for comp in (-1, 0, 1, 2, 3, 26, 27, 28):
                got, mirror = lib.pt_rays_sh_plane_offset(n, channels, sel, comp), rb.sh_plane_offset(n, channels, sel, comp)
                if (sel, comp) in want:
                    assert got == mirror == want[(sel, comp)], (n, channels, sel, comp)
                else:
                    assert got == ERR_INVALID and mirror == -1, (n, channels, sel, comp)
    for bad in (2, 3, -1, 1 << 20):
        assert lib.pt_rays_sh_bytes(n, bad) == 0 and rb.sh_bytes(n, bad) == 0
        assert lib.pt_rays_sh_plane_offset(n, bad, 0, 0) == ERR_INVALID and rb.sh_plane_offset(n, bad, 0, 0) == -1
    for bad_n in (-1, 2 ** 31):
        assert lib.pt_rays_sh_eval_bytes(bad_n) == 0
        assert lib.pt_rays_sh_bytes(bad_n, 1) == 0 and rb.sh_bytes(bad_n, 1) == 0
        assert lib.pt_rays_sh_plane_offset(bad_n, 1, 0, 0) == ERR_INVALID and rb.sh_plane_offset(bad_n, 1, 0, 0) == -1
        assert lib.pt_rays_sh_dirs_bytes(bad_n, 1) == 0 and rb.sh_dirs_bytes(bad_n, 1) == 0
    # the directions: 24 n K, refused beyond 2^31 - 1 samples
    for K in (1, 3, 70):
        ok = n * K <= 2 ** 31 - 1
        assert lib.pt_rays_sh_dirs_bytes(n, K) == rb.sh_dirs_bytes(n, K) == (24 * n * K if ok else 0)
    assert lib.pt_rays_sh_dirs_bytes(n, 0) == 0 and rb.sh_dirs_bytes(n, 0) == 0 and lib.pt_rays_sh_dirs_bytes(n, -2) == 0


def _block(lib):
    """A scene argument block whose ``cold`` pointer is set and whose shape count is positive.  Nothing dereferences it: every
    call below ends before its first HIP call, or at it -- there is no device here."""
    nb = int(lib.pt_rays_sh_args_bytes())
    block = (C.c_char * nb)()
    np.frombuffer(block, dtype=np.uint8)[:] = 1
    return block, nb


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
passed = lambda rc: rc not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # noqa: E731  (got as far as the first HIP call)


def test_every_projection_refusal_happens_before_any_hip_call(lib):
    """No GPU here: whatever is refused with PT_ERR_INVALID / UNSUPPORTED / SIZE was refused by the argument checks (the first HIP
    call would answer PT_ERR_NODEVICE)."""
    from pytracer_amd import _sh_lib

    block, nb = _block(lib)
    n = 5
    pts, act, seq = np.zeros((3, n)), np.zeros(n, np.int32), np.zeros(n, np.uint64)
    out = np.zeros(rb.sh_bytes(n, 1), np.uint8)
    ws = np.zeros(n * 3 * 56, np.uint8)

    def call(device=0, blk=block, nbytes=nb, pt=pts, a=act, s=seq, count=n, K=3, N=1, D=3, limit=2, depth=1, ch=1, o=out, ob=None, wsb=ws,
             wb=None, null_par=False):
        par = None if null_par else C.byref(_sh_lib.params(K, N, D, limit, depth, 42, 54, (0, 0, 0)))
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        host = lib.pt_rays_sh_project(device, blk, nbytes, p(pt), p(a), p(s), count, par, ch, p(o), ob)
        dev = lib.pt_rays_sh_project_device(device, blk, nbytes, p(pt), p(a), p(s), count, par, ch, p(wsb),
                                            (wsb.nbytes if wsb is not None else 0) if wb is None else wb, p(o), ob, None)
        return host, dev

    assert all(passed(rc) for rc in call()) and all(passed(rc) for rc in call(a=None, s=None))  # the optional planes
    # K, num_of_rays < 1
    for kw, word in ((dict(K=0), "samples"), (dict(K=-3), "samples"), (dict(N=0), "num_of_rays"), (dict(N=-1), "num_of_rays")):
        assert call(**kw) == both(ERR_INVALID) and word in _sh_lib.last_error(), kw
    # n out of range; n K beyond 2^31 - 1
    assert call(count=-1) == both(ERR_INVALID) and "probe count" in _sh_lib.last_error()
    assert call(count=2 ** 31, ob=2 ** 40) == both(ERR_INVALID)
    assert call(count=2 ** 31 - 1, K=2, ob=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in _sh_lib.last_error()
    assert call(count=3, K=715827883, ob=2 ** 40) == both(ERR_INVALID)  # 3 * 715827883 = 2^31 + 1
    assert call(count=46341, K=46341, ob=2 ** 40) == both(ERR_INVALID)  # 46341^2 = 2^31 + 4073
    # depths
    assert call(D=-1) == both(ERR_INVALID) and "max_depth" in _sh_lib.last_error()
    assert call(depth=-1) == both(ERR_INVALID) and "depth" in _sh_lib.last_error()
    assert call(D=66, depth=1) == both(ERR_UNSUPPORTED) and "64 levels" in _sh_lib.last_error()
    assert call(D=2 ** 31 - 1, depth=2 ** 31 - 66) == both(ERR_UNSUPPORTED)
    assert all(passed(rc) for rc in call(D=65, depth=1))  # 64 levels: accepted
    assert all(passed(rc) for rc in call(D=3, depth=7))  # deeper than max_depth: legal (black)
    # channels, device, block, params, buffers
    for ch in (2, 3, -1):
        assert call(ch=ch) == both(ERR_INVALID) and "channel" in _sh_lib.last_error(), ch
    assert call(device=-1) == both(ERR_INVALID)
    assert call(blk=None) == both(ERR_INVALID) and "null scene" in _sh_lib.last_error()
    assert call(nbytes=nb - 8) == both(ERR_INVALID) and "one build" in _sh_lib.last_error()
    assert call(null_par=True) == both(ERR_INVALID) and "null pt_sh_params" in _sh_lib.last_error()
    assert call(pt=None) == both(ERR_INVALID) and "null points" in _sh_lib.last_error()
    assert call(o=None, ob=out.nbytes) == both(ERR_INVALID) and "null output" in _sh_lib.last_error()
    # a short buffer or workspace
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "too small" in _sh_lib.last_error()
    assert call(ob=rb.sh_bytes(n, 0), ch=1) == both(ERR_SIZE) and all(passed(rc) for rc in call(ob=rb.sh_bytes(n, 0), ch=0))
    assert call(wb=n * 3 * 56 - 1)[1] == ERR_SIZE and "workspace" in _sh_lib.last_error() and passed(call(wb=n * 3 * 56)[1])
    assert call(wsb=None)[1] == ERR_INVALID and "workspace" in _sh_lib.last_error()
    # n = 0: PT_OK, nothing launched, no buffer needed
    assert call(count=0, pt=None, a=None, s=None, o=None, wsb=None) == both(0)
    assert not out.any()
    # the workspace's size: 0 on refusal, with the reason
    size = lambda count=n, device=0, **kw: lib.pt_rays_sh_workspace_bytes(device, count, C.byref(_sh_lib.params(  # noqa: E731
        kw.pop("K", 3), kw.pop("N", 1), kw.pop("D", 3), 2, kw.pop("depth", 1), 42, 54, (0, 0, 0))))
    assert size(D=66) == 0 and "64 levels" in _sh_lib.last_error()
    assert size(K=0) == 0 and size(N=0) == 0 and size(device=-1) == 0 and size(count=-1) == 0 and size(count=2 ** 31 - 1, K=2) == 0
    assert lib.pt_rays_sh_workspace_bytes(0, n, None) == 0


def test_every_direction_and_evaluation_refusal_happens_before_any_hip_call(lib):
    from pytracer_amd import _sh_lib

    n, m, K = 5, 4, 3
    seq, dirs_out = np.zeros(n, np.uint64), np.zeros((3, n * K))

    def directions(device=0, s=seq, count=n, samples=K, N=1, D=3, depth=1, o=dirs_out, ob=None, null_par=False):
        par = None if null_par else C.byref(_sh_lib.params(samples, N, D, 2, depth, 42, 54, (0, 0, 0)))
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        return (lib.pt_rays_sh_directions(device, p(s), count, par, p(o), ob),
                lib.pt_rays_sh_directions_device(device, p(s), count, par, p(o), ob, None))

    assert all(passed(rc) for rc in directions()) and all(passed(rc) for rc in directions(s=None))
    assert directions(samples=0) == both(ERR_INVALID) and "samples" in _sh_lib.last_error()
    assert directions(count=-1) == both(ERR_INVALID) and directions(count=2 ** 31, ob=2 ** 40) == both(ERR_INVALID)
    assert directions(count=2 ** 30, samples=2, ob=2 ** 40) == both(ERR_INVALID) and "2^31 - 1" in _sh_lib.last_error()
    assert directions(N=0) == both(ERR_INVALID) and directions(D=-1) == both(ERR_INVALID) and directions(D=66) == both(ERR_UNSUPPORTED)
    assert directions(device=-1) == both(ERR_INVALID) and directions(null_par=True) == both(ERR_INVALID)
    assert directions(o=None, ob=dirs_out.nbytes) == both(ERR_INVALID) and "null output" in _sh_lib.last_error()
    assert directions(ob=dirs_out.nbytes - 1) == both(ERR_SIZE) and "too small" in _sh_lib.last_error()
    assert directions(count=0, s=None, o=None) == both(0)

    coeffs, index, dirs, out = np.zeros((27, n)), np.zeros(m, np.int32), np.zeros((3, m)), np.zeros((3, m))

    def evaluate(device=0, c=coeffs, probes=n, idx=index, d=dirs, records=m, kind=1, o=out, ob=None):
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        return (lib.pt_rays_sh_eval(device, p(c), probes, p(idx), p(d), records, kind, p(o), ob),
                lib.pt_rays_sh_eval_device(device, p(c), probes, p(idx), p(d), records, kind, p(o), ob, None))

    assert all(passed(rc) for rc in evaluate()) and all(passed(rc) for rc in evaluate(idx=None)) and all(passed(rc) for rc in evaluate(kind=0))
    for kind in (2, -1, 3):
        assert evaluate(kind=kind) == both(ERR_INVALID) and "kind" in _sh_lib.last_error(), kind
    assert evaluate(probes=-1) == both(ERR_INVALID) and "probe count" in _sh_lib.last_error()
    assert evaluate(probes=2 ** 31) == both(ERR_INVALID)
    assert evaluate(records=-1) == both(ERR_INVALID) and "record count" in _sh_lib.last_error()
    assert evaluate(records=2 ** 31, ob=2 ** 40) == both(ERR_INVALID)
    assert evaluate(probes=m - 1, idx=None) == both(ERR_INVALID) and "index" in _sh_lib.last_error()  # m > n with a NULL index
    assert all(passed(rc) for rc in evaluate(probes=m, idx=None)) and all(passed(rc) for rc in evaluate(probes=1))  # (with an index: any n)
    assert evaluate(device=-1) == both(ERR_INVALID)
    assert evaluate(c=None) == both(ERR_INVALID) and "coefficient" in _sh_lib.last_error()
    assert evaluate(d=None) == both(ERR_INVALID) and "directions" in _sh_lib.last_error()
    assert evaluate(o=None, ob=out.nbytes) == both(ERR_INVALID)
    assert evaluate(ob=out.nbytes - 1) == both(ERR_SIZE) and "too small" in _sh_lib.last_error()
    assert evaluate(records=0, idx=None, d=None, o=None, c=None, probes=0) == both(0)  # m = 0: PT_OK, nothing launched
    assert not out.any() and not dirs_out.any()


def test_each_basis_literal_is_within_one_ulp_of_its_expression():
    pi = math.pi
    for literal, value in ((rb.SH_K0, math.sqrt(1.0 / (4.0 * pi))), (rb.SH_K1, math.sqrt(3.0 / (4.0 * pi))), (rb.SH_K2, math.sqrt(15.0 / (4.0 * pi))),
                           (rb.SH_K3, math.sqrt(5.0 / (16.0 * pi))), (rb.SH_K4, math.sqrt(15.0 / (16.0 * pi)))):
        assert abs(literal - value) <= math.ulp(value), (literal, value)
    assert rb.SH_BAND_FACTORS == (1.0, 2.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0, 0.25, 0.25, 0.25, 0.25, 0.25)
    # the basis as the header orders it: y, z, x; xy, yz, 3 z^2 - 1, xz, x^2 - y^2
    d = np.array([0.3, -0.5, 0.7])
    y = rb.sh_basis(d)
    assert y.tolist() == [rb.SH_K0, rb.SH_K1 * -0.5, rb.SH_K1 * 0.7, rb.SH_K1 * 0.3, rb.SH_K2 * (0.3 * -0.5), rb.SH_K2 * (-0.5 * 0.7),
                          rb.SH_K3 * (3.0 * (0.7 * 0.7) - 1.0), rb.SH_K2 * (0.3 * 0.7), rb.SH_K4 * (0.3 * 0.3 - -0.5 * -0.5)]
    # orthonormal over the sphere: a 64 x 128 Gauss / midpoint grid integrates these polynomials exactly, so what is left is the
    # rounding of a sum of 64 * 128 terms of magnitude <= 1 -- at most one eps each
    x, w = np.polynomial.legendre.leggauss(64)
    phi = (np.arange(128) + 0.5) * (2.0 * pi / 128)
    s = np.sqrt(1.0 - x * x)
    grid = np.stack([s[:, None] * np.cos(phi), s[:, None] * np.sin(phi), np.broadcast_to(x[:, None], (64, 128))], axis=-1)
    yy = rb.sh_basis(grid)
    gram = np.einsum("tpi,tpj,t->ij", yy, yy, w) * (2.0 * pi / 128)
    assert np.abs(gram - np.eye(9)).max() <= 64 * 128 * P.EPS


def test_the_direction_is_a_unit_vector_with_z_in_range(oracle):
    g = oracle.Pcg(P.S0, 12345)
    u = np.array([g.random_float() for _ in range(100000)]).reshape(-1, 2)
    u[0], u[1], u[2] = (0.0, 0.0), (1.0, 1.0), (0.5, 0.25)  # the ends of the draws' range
    d = P.directions_np(u)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 4 * P.EPS
    assert d[:, 2].min() >= -1.0 and d[:, 2].max() <= 1.0 and np.isfinite(d).all()
    assert d[0].tolist() == [0.0, 0.0, 1.0] and d[1, 2] == -1.0 and d[2, 2] == 0.0
    # uniform: the mean of every basis function but the first is 0 within six sigma (sigma^2 = 1 / (4 pi n))
    y = rb.sh_basis(d[3:])
    assert np.abs(y[:, 1:].mean(axis=0)).max() <= 6.0 * math.sqrt(1.0 / (4.0 * math.pi * (d.shape[0] - 3)))
    # the scalar restatement with libm agrees with the numpy one to a few ulp
    one = np.array([P.direction(a, b) for a, b in u[:500]])
    assert np.abs(one - d[:500]).max() <= 4 * P.EPS


NORMALS = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.6, 0.0, 0.8), (-0.48, 0.6, 0.64), (0.0, -1.0, 0.0))


def test_the_band_factors_give_the_cosine_weighted_hemisphere_mean():
    """For a band-limited field the numpy mirror of PT_SH_HEMISPHERE on the exact coefficients is the closed form, and the closed
    form is the integral: a quadrature that is itself checked on two cases with known answers."""
    one = lambda d: np.ones(d.shape[:-1])  # noqa: E731
    assert abs(P.hemisphere_quadrature(one, np.array([0.0, 0.0, 1.0])) - 1.0) <= 1e-12  # (1 / pi) * integral of cos = 1
    assert abs(P.hemisphere_quadrature(lambda d: d[..., 2], np.array([0.0, 0.0, 1.0])) - 2.0 / 3.0) <= 1e-12
    assert abs(P.hemisphere_quadrature(lambda d: d[..., 2] ** 2, np.array([0.6, 0.0, 0.8])) - (0.25 + 0.25 * 0.64)) <= 1e-12
    coeffs = np.repeat(P.field_coefficients()[:, None], 3, axis=1)  # [9, 3]: the same field in every channel
    for n in NORMALS:
        n = np.array(n)
        closed = P.field_hemisphere(n)
        mirror = rb.sh_evaluate(coeffs, n, rb.SH_HEMISPHERE)
        assert np.abs(mirror - closed).max() <= 1e-14, (n, mirror, closed)
        assert abs(P.hemisphere_quadrature(P.field, n) - closed) <= 1e-6, n
        assert np.abs(rb.sh_evaluate(coeffs, n, rb.SH_RADIANCE) - P.field(n)).max() <= 1e-14
    with pytest.raises(ValueError, match="kind"):
        rb.sh_evaluate(coeffs, np.array(NORMALS[0]), 2)


def test_channel_names_the_views_and_the_parameter_block():
    from pytracer_amd import _sh_lib

    assert rb.sh_channels("all") == 1 and rb.sh_channels("none") == 0 and rb.sh_channels("count") == rb.SH_COUNT
    with pytest.raises(ValueError) as e:
        rb.sh_channels("count, bogus,all")
    assert str(e.value) == "a probe batch has the channel count; not bogus, all"
    with pytest.raises(ValueError) as e:
        rb.sh_channels(2)
    assert str(e.value) == "a probe batch has the channel count (1); not 0x2"
    n = 6
    buf = np.zeros(rb.sh_bytes(n, 1), np.uint8)
    buf.view(np.float64)[: 27 * n] = np.arange(27 * n)
    buf.view(np.uint64)[27 * n:] = np.arange(100, 100 + n)
    res = rb.ProbeSet(buf, n, "all", shape=(2, 3))
    assert res.coefficients.shape == (2, 3, 9, 3) and res.block.shape == (27, n) and res.n_rays.shape == (2, 3)
    assert res.coefficients[1, 2, 4, 1] == (3 * 4 + 1) * n + 5 and res.n_rays[1, 0] == 103  # plane 3 j + ch, probe 5
    assert np.shares_memory(res.coefficients, buf) and np.shares_memory(res.block, buf) and np.shares_memory(res.n_rays, buf)
    res.coefficients[0, 1, 8, 2] = -7.0
    assert buf.view(np.float64)[26 * n + 1] == -7.0
    assert set(res.planes()) == {"coefficients", "n_rays"}
    only = rb.ProbeSet(np.zeros(rb.sh_bytes(n, 0), np.uint8), n, "none")
    assert only.coefficients.shape == (n, 9, 3) and not only.has("count") and set(only.planes()) == {"coefficients"}
    with pytest.raises(KeyError, match="count"):
        only.n_rays
    with pytest.raises(ValueError):
        rb.ProbeSet(np.zeros(8, np.uint8), n)
    with pytest.raises(ValueError, match="evaluator"):
        only.hemisphere_mean(np.zeros((n, 3)))
    par = _sh_lib.params(3, 2, 10, 4, 1, -1, 2 ** 64 + 5, (0.5, 0.25, 1))
    assert (par.samples, par.num_of_rays, par.max_depth, par.rr_limit, par.depth0) == (3, 2, 10, 4, 1)
    assert (par.init_state, par.init_seq, list(par.background)) == (2 ** 64 - 1, 5, [0.5, 0.25, 1.0])
    with pytest.raises(ValueError, match="samples"):
        _sh_lib.params(2 ** 31)


def test_what_reaches_the_device_scene_without_a_device():
    """``radiance_probes`` hands ``DeviceScene.sh_project`` PathTracer's defaults and ``depth=1``; the views evaluate through the
    scene's ``sh_eval``; ``probe_map`` asks for the hemisphere mean at the texel centres' normals; ``outgoing_probe_map`` composes
    ``emitted + brdf_color * map`` and refuses a mirror."""
    from pytracer_amd import abi

    seen = {}

    class Scene:
        kinds = abi.BRDF_DIFFUSE

        def sh_project(self, points, *args):
            seen["project"] = (points,) + args
            n = points.shape[1]
            buf = np.zeros(rb.sh_bytes(n, args[-1]), np.uint8)
            buf.view(np.float64)[: 27 * n] = 1.0
            return rb.ProbeSet(buf, n, args[-1])

        def sh_directions(self, n, samples, *args):
            seen["directions"] = (n, samples) + args
            return np.arange(3.0 * n * samples).reshape(3, n * samples)

        def sh_eval(self, block, dirs, index, kind):
            seen["eval"] = (block, dirs, index, kind)
            return np.full((3, dirs.shape[1]), 2.0)

        def surface_points(self, shape, uv, side):
            seen["points"] = (shape, uv, side)
            out = np.zeros((6, shape.shape[0]))
            out[5] = 1.0
            return out

        def surface(self, shape_index, uv, bits):
            n = shape_index.size
            buf = np.zeros(rb.surface_bytes(n, bits), np.uint8)
            buf[: 4 * n].view(np.int32)[:] = self.kinds
            buf[rb.surface_plane_offset(n, bits, rb.SURF_BRDF_COLOR):][: 24 * n].view(np.float64)[:] = 0.25
            buf[rb.surface_plane_offset(n, bits, rb.SURF_EMITTED):][: 24 * n].view(np.float64)[:] = 1.0
            return rb.SurfaceColors(buf, n, bits)

    wq = rb.WorldQueries(Scene())
    pts = np.arange(24.0).reshape(2, 4, 3)
    res = wq.radiance_probes(pts, 16)
    assert res.coefficients.shape == (2, 4, 9, 3) and res.n_rays.shape == (2, 4)
    assert np.array_equal(seen["project"][0], rb.planar(pts, 3)) and seen["project"][1:] == (16, 42, 54, None, None, 1, 10, 3, (0.0, 0.0, 0.0), 1, 1)
    d = wq.probe_directions(2, 3, seqs=[5, 6])
    assert d.shape == (2, 3, 3) and d[1, 2].tolist() == [5.0, 11.0, 17.0] and seen["directions"] == (2, 3, 42, 54, [5, 6])
    # the views evaluate on the scene: planar directions, one probe index per record, the kind
    got = res.hemisphere_mean(np.ones((5, 2, 3)), index=3)
    assert got.shape == (5, 2, 3) and np.all(got == 2.0)
    assert seen["eval"][0] is res.block and seen["eval"][1].shape == (3, 10) and seen["eval"][2].tolist() == [3] * 10 and seen["eval"][3] == rb.SH_HEMISPHERE
    res.radiance(np.ones((8, 3)))
    assert seen["eval"][2] is None and seen["eval"][3] == rb.SH_RADIANCE
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        res.radiance(np.ones((8, 2)))
    m = wq.probe_map(1, 7, 5, res, probe=2, side=-1)
    assert m.shape == (5, 7, 3) and seen["points"][0].tolist() == [1] * 35 and seen["points"][2].tolist() == [-1] * 35
    assert np.array_equal(seen["points"][1], rb.texel_centres(7, 5).reshape(35, 2)) and seen["eval"][2].tolist() == [2] * 35
    assert np.array_equal(seen["eval"][1], np.array([[0.0] * 35, [0.0] * 35, [1.0] * 35]))  # the normals of surface_points
    out = wq.outgoing_probe_map(1, 7, 5, res)
    assert out.shape == (5, 7, 3) and np.all(out == 1.0 + 0.25 * 2.0) and seen["eval"][2].tolist() == [0] * 35
    Scene.kinds = abi.BRDF_SPECULAR
    with pytest.raises(ValueError, match="DiffuseBRDF"):
        wq.outgoing_probe_map(1, 7, 5, res)
    with pytest.raises(ValueError, match="points"):
        wq.radiance_probes(np.zeros((4, 2)), 16)


def test_the_probe_grid_places_its_points_and_blends_them():
    grid = rb.ProbeGrid((1.0, -2.0, 0.5), (0.5, 1.0, 2.0), (3, 2, 4))
    pts = grid.points()
    assert grid.n == 24 and pts.shape == (24, 3)
    assert pts[0].tolist() == [1.0, -2.0, 0.5] and pts[1].tolist() == [1.5, -2.0, 0.5] and pts[3].tolist() == [1.0, -1.0, 0.5]
    assert pts[(2 * 2 + 1) * 3 + 2].tolist() == [2.0, -1.0, 4.5]  # (ix, iy, iz) = (2, 1, 2)
    rng = np.random.default_rng(5)
    buf = np.zeros(rb.sh_bytes(24, 0), np.uint8)
    probes = rb.ProbeSet(buf, 24, 0)
    probes.block[:] = rng.standard_normal((27, 24))
    # at a corner: that corner's coefficients, exactly
    at = grid.blend(probes, pts)
    assert at.n == 24 and at.block.tobytes() == probes.block.tobytes()
    # between two corners along every axis: linear
    for axis, (a, b) in ((0, (0, 1)), (1, (1, 4)), (2, (5, 11))):
        for f in (0.25, 0.5, 0.875):
            x = pts[a] + f * (pts[b] - pts[a])
            got = grid.blend(probes, x[None, :]).block[:, 0]
            want = (1.0 - f) * probes.block[:, a] + f * probes.block[:, b]
            assert np.abs(got - want).max() <= 4 * P.EPS * np.abs(probes.block).max(), (axis, f)
    # the weights of any point are eight non-negative numbers that sum to 1; outside the lattice the border is held
    index, weight = grid.corners(rng.uniform(-5, 8, (50, 3)))
    assert index.shape == weight.shape == (50, 8) and index.min() >= 0 and index.max() < 24 and weight.min() >= 0.0
    assert np.abs(weight.sum(axis=1) - 1.0).max() <= 4 * P.EPS
    assert grid.blend(probes, np.array([[-9.0, -9.0, -9.0]])).block[:, 0].tobytes() == probes.block[:, 0].tobytes()
    shaped = grid.blend(probes, np.zeros((2, 5, 3)))
    assert shaped.coefficients.shape == (2, 5, 9, 3) and shaped.evaluator is probes.evaluator
    flat = rb.ProbeGrid((0, 0, 0), 1.0, (2, 2, 1))  # one layer: the third axis has nothing to blend
    assert flat.points().shape == (4, 3) and np.abs(flat.corners(np.array([[0.5, 0.5, 3.0]]))[1].sum() - 1.0) <= 4 * P.EPS
    with pytest.raises(ValueError, match="dims"):
        rb.ProbeGrid((0, 0, 0), 1.0, (2, 0, 1))
    with pytest.raises(ValueError, match="step"):
        rb.ProbeGrid((0, 0, 0), 0.0, (2, 2, 1))
    with pytest.raises(ValueError, match="lattice"):
        grid.blend(rb.ProbeSet(np.zeros(rb.sh_bytes(3, 0), np.uint8), 3, 0), pts)


def test_the_expected_coefficients_depend_on_the_order_of_the_sum(oracle):
    """The discriminating power of the GPU's bit tests: on the oracle's composition for c2's seven probes at K = 70, adding each
    probe's samples from the last to the first changes the bits of most coefficients."""
    want = P.expected(oracle, "c2", 70, 1, 3, 2)
    assert want["samples"].shape == (7, 70, 3) and P.same_bits(P.project(want["dirs"], want["samples"]), want["coefficients"])
    back = P.project(want["dirs"], want["samples"], reverse=True)
    changed = back.view(np.uint64) != want["coefficients"].view(np.uint64)
    print(f"c2, 7 probes at K=70: the reverse order changes {changed.mean():.1%} of the coefficients")
    assert changed.mean() > 0.5
    assert np.array_equal(want["count"], want["sample_counts"].sum(axis=1)) and want["count"].min() >= 70
    # every sample has a direction of its own, and the probes see different things
    assert len(np.unique(want["dirs"].reshape(-1, 3), axis=0)) == 7 * 70 and len(np.unique(want["coefficients"][:, 0, :], axis=0)) == 7


@pytest.mark.parametrize("K,N,D,limit", P.ORACLE_CASES)
@pytest.mark.parametrize("name", P.WORLDS)
def test_the_outlier_cap_is_meaningful(oracle, name, K, N, D, limit):
    """Every direction of the case moved by one ``nextafter`` in each component -- what another sin / cos might give -- and the
    case recomposed: the probes that then differ beyond the bar number at most ``MAX_OUTLIERS``.  The GPU test holds the device
    to the same cap on the same cases."""
    want = P.expected(oracle, name, K, N, D, limit)
    moved = P.expected(oracle, name, K, N, D, limit, nudge=True)
    assert not P.same_bits(moved["dirs"], want["dirs"]) and np.abs(moved["dirs"] - want["dirs"]).max() <= 2 * P.EPS
    bad, worst = P.outliers(moved["coefficients"], moved["count"], want)
    print(f"{name} K={K} N={N} D={D} limit={limit}: {int(bad.sum())} of 7 probes beyond the bar, worst |difference| / bar {worst:.3g}")
    assert bad.sum() <= P.MAX_OUTLIERS
    assert want["count"].min() >= K and (want["bar"] > 0).any()


def test_the_furnace_bounds_hold_on_the_oracles_composition(oracle):
    """The seeds of the GPU's furnace test, before a GPU sees them: band 0 to 1e-13, bands 1 and 2 within six sigma."""
    want = P.furnace_expected(oracle)
    assert len(np.unique(want["samples"].reshape(-1, 3), axis=0)) == 1  # every sample brings the same bits
    assert np.abs(want["samples"] - P.furnace_radiance()).max() <= 4 * P.EPS * P.furnace_radiance().max() and np.all(want["count"] == P.FURNACE_K * (P.FURNACE_D - P.FURNACE_DEPTH + 1))
    rel0, bound0, rest, bound = P.furnace_bounds(want["coefficients"])
    print(f"furnace at K={P.FURNACE_K}: band 0 off by {rel0.max():.3g} (bound {bound0:.3g}, 2 K eps = {2 * P.FURNACE_K * P.EPS:.3g}); "
          f"|c_j| / L at most {rest.max():.3g} (bound {bound:.3g})")
    assert rel0.max() <= bound0 <= 2 * P.FURNACE_K * P.EPS and rest.max() <= bound
