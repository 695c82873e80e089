"""CPU-only tests of the lit queries (include/ptrace_lit.h, libptrace_lit.so, pytracer_amd.rays): the ninth library builds and loads
without a GPU and leaves the other eight as they were; its header, the ctypes table and its dynamic symbols agree; sizes match their
Python mirrors up to 2^31 - 1 records; every refusal of the interface happens before any HIP call; and the numpy mirror the GPU's
bit tests compare with has the properties of a trilinear blend -- weights that sum to 1, a lattice point that is its probe, a one-probe
lattice that is ``sh_evaluate`` -- and DEPENDS on the order of the corners, so those bit tests discriminate."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import rays as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE = -1, -3, -5  # include/ptrace.h
V17 = (1 << 16) | 7
SIZES = [0, 1, 63, 65, 2 ** 31 - 1]
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _lit_lib, build

    build.build()
    assert os.path.exists(build.LIT_LIB) and not build.needs_build()
    return _lit_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _lit_lib, _rays_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_lit.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lit_lib.EXPORTS) == {s for s, _, _ in _lit_lib._SIGNATURES} and len(declared) == 9
    assert all(s.startswith("pt_rays_lit_") for s in declared)
    assert _exported(_lit_lib.lib_path()) == declared
    # an add-on like the seven before it: no link dependency on any of the eight libraries, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _lit_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_lit.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _lit_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    assert lib.pt_rays_lit_version() == V17
    assert lib.pt_rays_lit_args_bytes() == _rays_lib.lib().pt_rays_args_bytes() > 0
    # the only file that includes the new device header is the new translation unit, which restates what it needs of the others'
    users = [f for f in os.listdir(build.CSRC) if '"pt_lit.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_lit.hip"]
    text = open(os.path.join(build.CSRC, "ptrace_lit.hip")).read() + open(os.path.join(build.CSRC, "pt_lit.h")).read()
    assert '"pt_sh.h"' not in text and '"pt_surface.h"' not in text and '"pt_scatter.h"' not in text
    assert '#include "pt_host_common.h"' in text and not re.search(r"\bg_err\b|\bstruct\s+Staged\b|#\s*define\s+HIP_TRY\b|getenv\s*\(", text)
    # the recipe: the pinned tables stay, the new row is in a further one, built with the add-ons' flags and watched
    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_lit.h")), "ptrace_lit.hip", "pt_lit.h"} <= deps
    assert len(build.TARGETS) == 6 and len(build.ALL_TARGETS) == 7 and len(build.EVERY_TARGET) == 8
    assert build.BUILD_TARGETS == build.EVERY_TARGET + ((build.LIT_FLAGS, build.LIT_LIB, build.LIT_SOURCES),)
    assert build.LIT_FLAGS[:-1] == build.FLAGS[:-1] and build.LIT_FLAGS[-1] == "-cuid=libptrace_lit" and "-ffp-contract=off" in build.LIT_FLAGS
    assert build.LIT_SOURCES == ["ptrace_lit.hip"] and os.path.basename(build.LIT_LIB) == "libptrace_lit.so"
    assert C.sizeof(_lit_lib.LitGrid) == 64  # six doubles, three ints and their padding: pt_lit_grid
    # the header states its definitions with their sources, and the basis' literals are the probe library's
    for cite in ("ProbeGrid.corners", "ProbeGrid.blend", "materials.py:186-192", "shapes.py:126, 181", "(4 * 2^-52)"):
        assert cite in header, cite
    sh_header = open(os.path.join(ROOT, "include", "ptrace_sh.h")).read()
    for literal in ("0.28209479177387814", "0.4886025119029199", "1.0925484305920792", "0.31539156525252005", "0.5462742152960396"):
        assert literal in header and literal in text and literal in sh_header, literal


def test_the_other_eight_libraries_are_what_they_were(lib):
    from pytracer_amd import _bake_lib, _gather_lib, _lib, _radiance_lib, _rays_lib, _scatter_lib, _sh_lib, _surface_lib, build

    for module, count in ((_rays_lib, 7), (_surface_lib, 11), (_scatter_lib, 7), (_radiance_lib, 8), (_gather_lib, 8), (_bake_lib, 11), (_sh_lib, 14)):
        assert _exported(module.lib_path()) == set(module.EXPORTS) and len(module.EXPORTS) == count
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert _sh_lib.lib().pt_rays_sh_version() == (1 << 16) | 6
    assert build.code_hash() == json.load(open(os.path.join(ROOT, "profiles", "pmc_c2.json")))["code_hash"]
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "ptrace_lit.h":
            assert "pt_rays_lit_" not in open(os.path.join(ROOT, "include", header)).read(), header
    # the recorded hashes: eight rows, parent and this change equal, and equal to what this build made
    rows = [line.split() for line in open(os.path.join(ROOT, "profiles", "lit_hashes.txt")) if line.startswith("libptrace")]
    assert [r[0] for r in rows] == [os.path.basename(t[1]) for t in build.EVERY_TARGET] and all(r[1] == r[2] for r in rows)
    assert [r[2] for r in rows] == [build.code_hash(t[1]) for t in build.EVERY_TARGET]
    # and the seven the probe library recorded are still those
    old = [line.split() for line in open(os.path.join(ROOT, "profiles", "sh_hashes.txt")) if line.startswith("libptrace")]
    assert [r[:3] for r in rows[:7]] == [r[:3] for r in old[:7]]


def test_a_missing_library_is_an_import_error_and_nothing_loads_before_the_first_call(tmp_path):
    import sys

    missing = str(tmp_path / "libptrace_lit.so")
    code = ("from pytracer_amd import _lit_lib\nprint('PATH', _lit_lib.lib_path())\n"
            "try:\n    _lit_lib.lib()\nexcept ImportError as e:\n    print('IMPORTERROR', e)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PTRACE_LIT_LIB=missing))
    assert r.returncode == 0, r.stderr
    out = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert out["PATH"] == missing and out["IMPORTERROR"].startswith(f"{missing} is missing: the HIP extension has not been built.")
    assert "no CPU fallback" in out["IMPORTERROR"]


@pytest.mark.parametrize("m", SIZES)
def test_sizes_match_the_python_mirror(lib, m):
    from pytracer_amd import _lit_lib

    assert lib.pt_rays_lit_bytes(m) == 24 * m
    for bad in (-1, 2 ** 31):
        assert lib.pt_rays_lit_bytes(bad) == 0
    # the coefficient block of a lattice: the probe library's 216 n, through its own mirror
    for dims in ((1, 1, 1), (3, 2, 4), (16, 16, 16), (2 ** 31 - 1, 1, 1), (1, 46340, 46340), (max(m, 1), 1, 1)):
        n = dims[0] * dims[1] * dims[2]
        g = _lit_lib.grid((0, 0, 0), (1, 1, 1), dims)
        assert lib.pt_rays_lit_coeffs_bytes(C.byref(g)) == rb.sh_bytes(n, 0) == 216 * n, dims
    for dims in ((2 ** 31 - 1, 2, 1), (46341, 46341, 1), (2 ** 16, 2 ** 16, 2 ** 16), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.pt_rays_lit_coeffs_bytes(C.byref(_lit_lib.grid((0, 0, 0), (1, 1, 1), dims))) == 0 and "2^31 - 1" in _lit_lib.last_error()
    assert lib.pt_rays_lit_coeffs_bytes(None) == 0


def _block(lib):
    """A scene argument block whose ``cold`` pointer is set and whose shape count is positive.  Nothing dereferences it: every
    call below ends before its first HIP call, or at it -- there is no device here."""
    nb = int(lib.pt_rays_lit_args_bytes())
    block = (C.c_char * nb)()
    np.frombuffer(block, dtype=np.uint8)[:] = 1
    return block, nb


p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
both = lambda code: (code, code)  # noqa: E731
passed = lambda rc: rc not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # noqa: E731  (got as far as the first HIP call)
BAD_GRIDS = (("dims", dict(dims=(0, 2, 2))), ("dims", dict(dims=(2, -1, 2))), ("dims", dict(dims=(2, 2, 0))),
             ("step", dict(step=(0.0, 1.0, 1.0))), ("step", dict(step=(1.0, -1.0, 1.0))), ("step", dict(step=(1.0, 1.0, np.inf))),
             ("step", dict(step=(np.nan, 1.0, 1.0))), ("origin", dict(origin=(np.nan, 0.0, 0.0))), ("origin", dict(origin=(0.0, np.inf, 0.0))),
             ("origin", dict(origin=(0.0, 0.0, -np.inf))), ("2^31 - 1", dict(dims=(2 ** 16, 2 ** 15, 1))), ("2^31 - 1", dict(dims=(2 ** 20, 2 ** 20, 2 ** 20))))


def test_every_lit_query_refusal_happens_before_any_hip_call(lib):
    """No GPU here: whatever is refused with PT_ERR_INVALID / SIZE was refused by the argument checks (the first HIP call would
    answer PT_ERR_NODEVICE)."""
    from pytracer_amd import _lit_lib

    m, dims = 5, (3, 2, 4)
    n = 24
    coeffs, pts, dirs, act, out = np.zeros((27, n)), np.zeros((3, m)), np.zeros((3, m)), np.zeros(m, np.int32), np.zeros((3, m))

    def call(device=0, grid=True, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), dims=dims, c=coeffs, cb=None, pt=pts, d=dirs, a=act, records=m,
             kind=1, o=out, ob=None):
        g = C.byref(_lit_lib.grid(origin, step, dims)) if grid else None
        cb = (c.nbytes if c is not None else 0) if cb is None else cb
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        return (lib.pt_rays_lit_eval(device, g, p(c), cb, p(pt), p(d), p(a), records, kind, p(o), ob),
                lib.pt_rays_lit_eval_device(device, g, p(c), cb, p(pt), p(d), p(a), records, kind, p(o), ob, None))

    assert all(passed(rc) for rc in call()) and all(passed(rc) for rc in call(a=None)) and all(passed(rc) for rc in call(kind=0))
    for word, kw in BAD_GRIDS:
        assert call(**kw) == both(ERR_INVALID) and word in _lit_lib.last_error(), kw
    assert call(grid=False) == both(ERR_INVALID) and "null pt_lit_grid" in _lit_lib.last_error()
    for kind in (2, -1, 3):
        assert call(kind=kind) == both(ERR_INVALID) and "kind" in _lit_lib.last_error(), kind
    assert call(records=-1) == both(ERR_INVALID) and "record count" in _lit_lib.last_error()
    assert call(records=2 ** 31, ob=2 ** 40) == both(ERR_INVALID)
    assert call(device=-1) == both(ERR_INVALID)
    assert call(c=None, cb=coeffs.nbytes) == both(ERR_INVALID) and "coefficient" in _lit_lib.last_error()
    assert call(pt=None) == both(ERR_INVALID) and "points" in _lit_lib.last_error()
    assert call(d=None) == both(ERR_INVALID) and "directions" in _lit_lib.last_error()
    assert call(o=None, ob=out.nbytes) == both(ERR_INVALID) and "null output" in _lit_lib.last_error()
    assert call(cb=coeffs.nbytes - 1) == both(ERR_SIZE) and "coefficient block too small" in _lit_lib.last_error()
    assert call(dims=(3, 2, 5)) == both(ERR_SIZE)  # a lattice of 30 probes, a block of 24
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "output too small" in _lit_lib.last_error()
    assert all(passed(rc) for rc in call(dims=(2 ** 31 - 1, 1, 1), cb=2 ** 40))  # (the largest lattice: accepted)
    # m = 0: PT_OK, nothing launched, no buffer needed -- but the lattice and the kind are still checked
    assert call(records=0, c=None, pt=None, d=None, a=None, o=None) == both(0)
    assert call(records=0, dims=(0, 1, 1)) == both(ERR_INVALID) and call(records=0, kind=7) == both(ERR_INVALID)
    assert not out.any()


def test_every_shade_query_refusal_happens_before_any_hip_call(lib):
    from pytracer_amd import _lit_lib

    block, nb = _block(lib)
    n_shapes = int(np.frombuffer(block, dtype=np.uint8)[0]) * 0x01010101  # (every byte is 1: whatever int the block holds is this)
    m, dims, n = 5, (3, 2, 4), 24
    coeffs, shape, v3, uv, out = np.zeros((27, n)), np.zeros(m, np.int32), np.zeros((3, m)), np.zeros((2, m)), np.zeros((3, m))
    slots = np.zeros(n_shapes + 2, np.int32)
    bg = (C.c_double * 3)(0.0, 0.0, 0.0)

    def call(device=0, blk=block, nbytes=nb, sl=slots, sb=None, grid=True, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), dims=dims, c=coeffs, cb=None,
             sh=shape, pt=v3, nr=v3, u=uv, d=v3, records=m, background=bg, o=out, ob=None):
        g = C.byref(_lit_lib.grid(origin, step, dims)) if grid else None
        cb = (c.nbytes if c is not None else 0) if cb is None else cb
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        sb = (sl.nbytes if sl is not None else 0) if sb is None else sb
        return (lib.pt_rays_lit_shade(device, blk, nbytes, g, p(c), cb, p(sh), p(pt), p(nr), p(u), p(d), records, background, p(o), ob),
                lib.pt_rays_lit_shade_device(device, blk, nbytes, p(sl), sb, g, p(c), cb, p(sh), p(pt), p(nr), p(u), p(d), records, background,
                                             p(o), ob, None))

    assert all(passed(rc) for rc in call())
    for word, kw in BAD_GRIDS:
        assert call(**kw) == both(ERR_INVALID) and word in _lit_lib.last_error(), kw
    assert call(grid=False) == both(ERR_INVALID) and "null pt_lit_grid" in _lit_lib.last_error()
    assert call(records=-1) == both(ERR_INVALID) and call(records=2 ** 31, ob=2 ** 40) == both(ERR_INVALID)
    assert call(device=-1) == both(ERR_INVALID)
    assert call(blk=None) == both(ERR_INVALID) and "null scene" in _lit_lib.last_error()
    assert call(nbytes=nb - 8) == both(ERR_INVALID) and "one build" in _lit_lib.last_error()
    assert call(background=None) == both(ERR_INVALID) and "background" in _lit_lib.last_error()
    assert call(c=None, cb=coeffs.nbytes) == both(ERR_INVALID) and "coefficient" in _lit_lib.last_error()
    for kw in (dict(sh=None), dict(pt=None), dict(nr=None), dict(u=None), dict(d=None)):
        assert call(**kw) == both(ERR_INVALID) and "planes" in _lit_lib.last_error(), kw
    assert call(o=None, ob=out.nbytes) == both(ERR_INVALID) and "null output" in _lit_lib.last_error()
    assert call(cb=coeffs.nbytes - 1) == both(ERR_SIZE) and "coefficient block too small" in _lit_lib.last_error()
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "output too small" in _lit_lib.last_error()
    # the slot table is the device form's alone: the host form makes its own
    host, dev = call(sl=None)
    assert passed(host) and dev == ERR_INVALID and "slot table" in _lit_lib.last_error()
    host, dev = call(sb=4 * n_shapes - 1)
    assert passed(host) and dev == ERR_SIZE and "slot table too small" in _lit_lib.last_error()
    assert call(records=0, c=None, sh=None, pt=None, nr=None, u=None, d=None, o=None, sl=None) == both(0)
    assert call(records=0, step=(0.0, 1.0, 1.0)) == both(ERR_INVALID)
    assert not out.any()


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def _probes(n, seed):
    rng = np.random.default_rng(seed)
    probes = rb.ProbeSet(np.zeros(rb.sh_bytes(n, 0), np.uint8), n, 0)
    probes.block[:] = rng.standard_normal((27, n)) * np.exp(rng.uniform(-3, 3, (27, 1)))
    return probes


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


GRIDS = (((1.0, -2.0, 0.5), (0.5, 1.0, 2.0), (3, 2, 4)), ((0.0, 0.0, 0.0), 1.0, (1, 1, 1)), ((-1.0, 0.0, 3.0), 0.25, (5, 1, 1)),
         ((0.0, 0.0, 0.0), (1.0, 3.0, 1.0), (2, 2, 1)))


@pytest.mark.parametrize("origin,step,dims", GRIDS)
def test_the_weights_sum_to_one_and_a_lattice_point_is_its_probe(origin, step, dims):
    grid = rb.ProbeGrid(origin, step, dims)
    rng = np.random.default_rng(7)
    index, weight = grid.corners(rng.uniform(-5, 8, (400, 3)))
    assert index.min() >= 0 and index.max() < grid.n and weight.min() >= 0.0
    assert np.abs(weight.sum(axis=1) - 1.0).max() <= 4 * EPS
    probes = _probes(grid.n, 11)
    dirs = rng.standard_normal((grid.n, 3))
    pts = grid.points()
    for kind in (rb.SH_RADIANCE, rb.SH_HEMISPHERE):
        want = rb.sh_evaluate(probes.coefficients, dirs, kind)
        assert _same(rb.lit_eval_host(grid, probes, pts, dirs, kind), want)
        # one ulp either side of the lattice point: the snap puts the record ON it
        for side in (-np.inf, np.inf):
            assert _same(rb.lit_eval_host(grid, probes, np.nextafter(pts, side), dirs, kind), want), (kind, side)
        # far outside on every face: the border's probe
        for axis in range(3):
            for sign, border in ((-1.0, 0), (1.0, dims[axis] - 1)):
                far = pts.copy()
                far[:, axis] = origin[axis] + sign * 1.0e6
                held = pts.copy()
                held[:, axis] = grid.origin[axis] + border * grid.step[axis]
                assert _same(rb.lit_eval_host(grid, probes, far, dirs, kind), rb.lit_eval_host(grid, probes, held, dirs, kind)), (axis, sign)


def test_a_lattice_of_one_probe_is_sh_evaluate_and_the_rules_for_nan_and_active():
    grid = rb.ProbeGrid((0.5, 0.5, 0.5), 2.0, (1, 1, 1))
    probes = _probes(1, 3)
    rng = np.random.default_rng(5)
    # on the probe or beyond it along every axis (f = 0 or 1: one corner has the weight 1.0, the others 0.0): every bit
    pts = np.where(rng.uniform(0, 1, (50, 3)) < 0.5, rng.uniform(-9, 0.5, (50, 3)), rng.uniform(2.5, 9, (50, 3)))
    dirs = rng.standard_normal((50, 3))
    pts[3], pts[4], pts[5], pts[6] = (np.inf, -np.inf, 1e300), (-1e300, 0.0, np.inf), (1.7e308, -1.7e308, 0.0), (0.5, 0.5, 0.5)
    inside = rng.uniform(0.5, 2.5, (50, 3))  # eight weights that sum to 1 within 4 eps, all on the one probe
    for kind in (rb.SH_RADIANCE, rb.SH_HEMISPHERE):
        want = rb.sh_evaluate(probes.coefficients[0], dirs, kind)
        assert _same(rb.lit_eval_host(grid, probes, pts, dirs, kind), want)
        # (the blend: 8 products and additions on weights that sum to 1 within 4 eps -- 16 eps of each coefficient at most)
        a = np.array(rb.SH_BAND_FACTORS) if kind == rb.SH_HEMISPHERE else np.ones(9)
        scale = (np.abs(rb.sh_basis(dirs)) * a)[:, :, None] * np.abs(probes.coefficients[0])[None]
        assert np.all(np.abs(rb.lit_eval_host(grid, probes, inside, dirs, kind) - want) <= 32 * EPS * scale.sum(axis=1))
    hostile = pts.copy()
    hostile[7], hostile[8], hostile[9] = (np.nan, 0.0, 0.0), (0.0, np.nan, 0.0), (np.nan, np.nan, np.nan)
    active = np.zeros(50, np.int32)
    active[20], active[21] = -1, -2 ** 31
    got = rb.lit_eval_host(grid, probes, hostile, dirs, rb.SH_HEMISPHERE, active)
    want = rb.sh_evaluate(probes.coefficients[0], dirs, rb.SH_HEMISPHERE)
    zero = np.zeros(50, bool)
    zero[[7, 8, 9, 20, 21]] = True
    assert not got[zero].any() and not np.signbit(got[zero]).any() and _same(got[~zero], want[~zero])
    with pytest.raises(ValueError, match="lattice"):
        rb.lit_eval_host(rb.ProbeGrid((0, 0, 0), 1.0, (2, 1, 1)), probes, pts, dirs)


def test_the_expected_values_depend_on_the_order_of_the_corners():
    """The discriminating power of the GPU's bit tests: blending the corners from the last to the first changes the bits of a good
    share of the records."""
    grid = rb.ProbeGrid((1.0, -2.0, 0.5), (0.5, 1.0, 2.0), (3, 2, 4))
    probes = _probes(grid.n, 21)
    rng = np.random.default_rng(22)
    pts = grid.origin + rng.uniform(0.0, 1.0, (500, 3)) * (np.asarray(grid.dims) - 1) * grid.step
    dirs = rng.standard_normal((500, 3))
    index, weight = grid.corners(pts)
    back = np.zeros((27, 500))
    for c in range(7, -1, -1):
        back = back + weight[:, c][None, :] * probes.block[:, index[:, c]]
    reverse = rb.sh_evaluate(np.moveaxis(back.reshape(9, 3, 500), 2, 0), dirs, rb.SH_HEMISPHERE)
    want = rb.lit_eval_host(grid, probes, pts, dirs, rb.SH_HEMISPHERE)
    changed = (reverse.view(np.uint64) != want.view(np.uint64)).any(axis=1)
    print(f"500 records in a (3, 2, 4) lattice: the reverse corner order changes {changed.mean():.1%} of them")
    assert changed.mean() > 0.25 and np.abs(reverse - want).max() <= 64 * EPS * np.abs(want).max()


def test_the_mirror_direction_and_the_shade_mirror():
    """``mirror_directions`` is ``shaders.scatter_ray``'s specular branch per row; ``lit_shade_host`` composes background, emitted and
    colour as the header says, leaves records without a hit unevaluated, and normalises a normal that is not unit length."""
    from pytracer_amd import abi, shaders
    from pytracer_amd import hostmodel as hm

    rng = np.random.default_rng(2)
    d, nrm = rng.standard_normal((40, 3)), rng.standard_normal((40, 3)) * 3.0
    got = rb.mirror_directions(d, nrm)
    brdf = hm.SpecularBRDF(hm.UniformPigment(hm.Color(1, 1, 1)))
    for i in range(40):
        _, want, _ = shaders.scatter_ray(brdf, None, tuple(d[i]), (0.0, 0.0, 0.0), tuple(nrm[i]))
        assert tuple(got[i]) == want, i
    grid = rb.ProbeGrid((0.0, 0.0, 0.0), 1.0, (2, 2, 2))
    probes = _probes(8, 4)
    m = 12
    kinds = np.array([abi.BRDF_DIFFUSE, abi.BRDF_SPECULAR, -1] * 4, dtype=np.int32)
    buf = np.zeros(rb.surface_bytes(m, rb.SURF_ALL), np.uint8)
    mat = rb.SurfaceColors(buf, m, rb.SURF_ALL)
    mat.brdf_kind[:] = kinds
    mat.brdf_color[:] = rng.uniform(0, 1, (m, 3))
    mat.emitted[:] = rng.uniform(0, 1, (m, 3))
    pts = rng.uniform(0, 1, (m, 3))
    pts[2] = np.nan  # (a record without a hit may hold anything)
    pts[3] = (np.nan, 0.5, 0.5)
    out = rb.lit_shade_host(grid, probes, mat, pts, nrm[:m], d[:m], (0.25, 0.5, 0.75))
    assert np.all(out[kinds < 0] == (0.25, 0.5, 0.75))
    unit = nrm[:m] / np.sqrt(nrm[:m, 0] * nrm[:m, 0] + nrm[:m, 1] * nrm[:m, 1] + nrm[:m, 2] * nrm[:m, 2])[:, None]
    e_dif = rb.lit_eval_host(grid, probes, pts, unit, rb.SH_HEMISPHERE)
    e_spec = rb.lit_eval_host(grid, probes, pts, got[:m], rb.SH_RADIANCE)
    for r in range(m):
        if kinds[r] >= 0:
            e = e_dif[r] if kinds[r] == abi.BRDF_DIFFUSE else e_spec[r]
            assert _same(out[r], np.asarray(mat.emitted)[r] + np.asarray(mat.brdf_color)[r] * e), r
    assert _same(out[3], np.asarray(mat.emitted)[3] + np.asarray(mat.brdf_color)[3] * 0.0)  # a NaN point: E = +0.0
    shaped = rb.lit_shade_host(grid, probes, rb.SurfaceColors(buf, m, rb.SURF_ALL, shape=(3, 4)), pts.reshape(3, 4, 3), nrm[:m].reshape(3, 4, 3),
                               d[:m].reshape(3, 4, 3), hm.Color(0.25, 0.5, 0.75))
    assert shaped.shape == (3, 4, 3) and _same(shaped.reshape(m, 3), out)


def test_what_reaches_the_device_scene_without_a_device():
    """``ProbeGrid.evaluate`` goes to ``lit_eval`` of the scene behind ``probes.evaluator`` with planar arrays;
    ``probe_lit_radiance`` hands ``lit_shade`` the planes of a frame, of a ray batch with ``dirs=`` or of plain arrays; the shader
    asks its tracer's queries and refuses a probe count that is not the lattice's."""
    from types import SimpleNamespace

    from pytracer_amd import shaders
    from pytracer_amd import hostmodel as hm

    seen = {}

    class Scene:
        def sh_eval(self, *a):  # pragma: no cover  (only its owner is asked for)
            raise AssertionError

        def lit_eval(self, grid, block, points, dirs, active, kind):
            seen["eval"] = (grid, block, points, dirs, active, kind)
            return np.arange(3.0 * points.shape[1]).reshape(3, -1)

        def lit_shade(self, grid, block, index, point, normal, uv, dirs, background):
            seen["shade"] = (grid, block, index, point, normal, uv, dirs, background)
            return np.full((index.size, 3), 2.0)

    scene = Scene()
    grid = rb.ProbeGrid((0, 0, 0), 1.0, (2, 2, 1))
    probes = rb.ProbeSet(np.zeros(rb.sh_bytes(4, 0), np.uint8), 4, 0, evaluator=scene.sh_eval)
    pts, dirs = np.arange(30.0).reshape(2, 5, 3), np.ones((2, 5, 3))
    got = grid.evaluate(probes, pts, dirs, rb.SH_HEMISPHERE)
    assert got.shape == (2, 5, 3) and got[1, 4].tolist() == [9.0, 19.0, 29.0]
    assert seen["eval"][0] is grid and seen["eval"][1] is probes.block and np.array_equal(seen["eval"][2], rb.planar(pts, 3)) and seen["eval"][4:] == (None, 1)
    with pytest.raises(ValueError, match="lattice"):
        rb.ProbeGrid((0, 0, 0), 1.0, (2, 2, 2)).evaluate(probes, pts, dirs)
    with pytest.raises(ValueError, match="device scene"):
        grid.evaluate(rb.ProbeSet(probes.buffer, 4, 0), pts, dirs)
    with pytest.raises(ValueError, match="directions"):
        grid.evaluate(probes, pts, dirs[:1])
    wq = rb.WorldQueries(scene)
    frame = SimpleNamespace(shape_index=np.zeros((1, 3, 4), np.int32), point=np.zeros((1, 3, 4, 3)), normal=np.ones((1, 3, 4, 3)),
                            uv=np.zeros((1, 3, 4, 2)), ray_dir=np.full((1, 3, 4, 3), 5.0))
    out = wq.probe_lit_radiance(grid, probes, frame, background=(1, 2, 3))
    assert out.shape == (1, 3, 4, 3) and np.all(out == 2.0) and seen["shade"][6] is frame.ray_dir and seen["shade"][7] == (1, 2, 3)
    batch = SimpleNamespace(shape_index=np.zeros(6, np.int32), point=np.zeros((6, 3)), normal=np.ones((6, 3)), uv=np.zeros((6, 2)))
    with pytest.raises(ValueError, match="dirs="):
        wq.probe_lit_radiance(grid, probes, batch)
    assert wq.probe_lit_radiance(grid, probes, batch, dirs=np.ones((6, 3))).shape == (6, 3)
    plain = wq.probe_lit_radiance(grid, probes, dict(shape_index=[0, -1], point=np.zeros((2, 3)), normal=np.ones((2, 3)), uv=np.zeros((2, 2))),
                                  dirs=np.ones((2, 3)))
    assert plain.shape == (2, 3) and seen["shade"][2].tolist() == [0, -1]
    with pytest.raises(ValueError, match="lattice"):
        wq.probe_lit_radiance(rb.ProbeGrid((0, 0, 0), 1.0, (3, 1, 1)), probes, batch, dirs=np.ones((6, 3)))
    world = hm.World()
    tracer = SimpleNamespace(world_queries=lambda w: wq if w is world else None)
    shader = shaders.ProbeLitShader(world, grid, probes, tracer, hm.Color(1, 2, 3))
    assert shader.shade_hits(frame).shape == (1, 3, 4, 3) and seen["shade"][0] is grid and seen["shade"][7] is shader.background_color
    with pytest.raises(TypeError, match="tracer"):
        shaders.ProbeLitShader(world, grid, probes).shade_hits(frame)
    with pytest.raises(TypeError, match="ray_intersection"):
        shaders.ProbeLitShader(world, grid, probes)(None)
    with pytest.raises(ValueError, match="lattice"):
        shaders.ProbeLitShader(world, rb.ProbeGrid((0, 0, 0), 1.0, (3, 1, 1)), probes)


def test_the_shader_ray_by_ray_is_the_mirror():
    """``ProbeLitShader.__call__`` on a world that answers ``ray_intersection`` with a prepared record: the arithmetic of
    ``lit_shade_host`` for one record, for both BRDFs and a miss."""
    from types import SimpleNamespace

    from pytracer_amd import abi, shaders
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.hits import HitRay, HitRecord, Vec2d

    grid = rb.ProbeGrid((0.0, 0.0, 0.0), 0.5, (3, 3, 3))
    probes = _probes(27, 8)
    materials = [hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(0.5, 0.25, 0.125))), hm.UniformPigment(hm.Color(0.1, 0.2, 0.3))),
                 hm.Material(hm.SpecularBRDF(hm.CheckeredPigment(hm.Color(1.0, 0.5, 0.0), hm.Color(0.0, 0.5, 1.0), 4)), hm.UniformPigment(hm.Color(0, 0, 0)))]
    records = {}

    class World:
        shapes = [SimpleNamespace(material=m) for m in materials]

        def ray_intersection(self, ray):
            return records[id(ray)]

    shader = shaders.ProbeLitShader(World(), grid, probes, None, hm.Color(0.5, 0.5, 0.25))
    rng = np.random.default_rng(3)
    for i in range(6):
        wp, nrm, d, uv = rng.uniform(0, 1, 3), rng.standard_normal(3) * 2.0, rng.standard_normal(3), rng.uniform(0, 1, 2)
        ray = HitRay(hm.Vec(0, 0, 0), hm.Vec(*d))
        records[id(ray)] = HitRecord(hm.Vec(*wp), hm.Vec(*nrm), Vec2d(*uv), 1.0, ray, i % 2)
        got = shader(ray)
        mat = SimpleNamespace(brdf_kind=np.array([abi.BRDF_DIFFUSE if i % 2 == 0 else abi.BRDF_SPECULAR], np.int32),
                              brdf_color=np.array([[getattr(shaders.pigment_color(materials[i % 2].brdf.pigment, Vec2d(*uv)), c) for c in "rgb"]]),
                              emitted=np.array([[getattr(shaders.pigment_color(materials[i % 2].emitted_radiance, Vec2d(*uv)), c) for c in "rgb"]]))
        want = rb.lit_shade_host(grid, probes, mat, wp[None], nrm[None], d[None])[0]
        assert (got.r, got.g, got.b) == tuple(want), i
    miss = HitRay(hm.Vec(0, 0, 0), hm.Vec(0, 0, 1))
    records[id(miss)] = None
    assert shader(miss) is shader.background_color
