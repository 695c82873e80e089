"""CPU-only tests of the gather queries (include/ptrace_gather.h, libptrace_gather.so, pytracer_amd.rays): the sixth library builds
and loads without a GPU and leaves the other five as they were; its header, the ctypes table and its dynamic symbols agree; sizes
and offsets match their Python mirrors; bad arguments are refused before any HIP call; and the expected values the GPU tests
compare bit for bit DEPEND on the order of the sum, so a wrong order cannot pass there."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import rays as rb

from . import gather_batches as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE = -1, -3, -5  # include/ptrace.h
V14 = (1 << 16) | 4
SIZES = [0, 1, 63, 65, 2 ** 31 - 1]


@pytest.fixture(scope="module")
def lib():
    from pytracer_amd import _gather_lib, build

    build.build()
    assert os.path.exists(build.GATHER_LIB) and not build.needs_build()
    return _gather_lib.lib()


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(lib):
    from pytracer_amd import _gather_lib, _rays_lib, build

    header = open(os.path.join(ROOT, "include", "ptrace_gather.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_gather_lib.EXPORTS) and len(declared) == 8
    assert _exported(_gather_lib.lib_path()) == declared
    # an add-on like the other four: no link dependency on any of them, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _gather_lib.lib_path()], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libptrace" not in needed.replace("libptrace_gather.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _gather_lib.lib_path()], capture_output=True, text=True).stdout
    assert "hipLaunchKernel" in undefined and not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    assert lib.pt_rays_gather_version() == V14
    assert lib.pt_rays_gather_args_bytes() == _rays_lib.lib().pt_rays_args_bytes() > 0
    # the only file that includes the new device header is the new translation unit, which keeps away from the radiance walk's
    # header; the recipe builds the library like the other add-ons and watches its sources and its public header
    users = [f for f in os.listdir(build.CSRC) if '"pt_gather.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_gather.hip"]
    assert '"pt_radiance.h"' not in open(os.path.join(build.CSRC, "ptrace_gather.hip")).read() + open(os.path.join(build.CSRC, "pt_gather.h")).read()
    deps = {os.path.normpath(d) for d in build.DEPS}
    assert {os.path.normpath(os.path.join("..", "..", "include", "ptrace_gather.h")), "ptrace_gather.hip", "pt_gather.h"} <= deps
    assert (build.GATHER_FLAGS, build.GATHER_LIB, build.GATHER_SOURCES) == build.TARGETS[-1] and len(build.TARGETS) == 6
    assert build.GATHER_FLAGS[:-1] == build.FLAGS[:-1] and build.GATHER_FLAGS[-1] == "-cuid=libptrace_gather"
    assert C.sizeof(_gather_lib.GatherParams) == 64  # five ints (and padding), two uint64 and three doubles: pt_gather_params


def test_the_other_five_libraries_are_what_they_were(lib):
    from pytracer_amd import _lib, _radiance_lib, _rays_lib, _scatter_lib, _surface_lib, build

    assert _exported(_rays_lib.lib_path()) == set(_rays_lib.EXPORTS) and len(_rays_lib.EXPORTS) == 7
    assert _exported(_surface_lib.lib_path()) == set(_surface_lib.EXPORTS) and len(_surface_lib.EXPORTS) == 11
    assert _exported(_scatter_lib.lib_path()) == set(_scatter_lib.EXPORTS) and len(_scatter_lib.EXPORTS) == 7
    assert _exported(_radiance_lib.lib_path()) == set(_radiance_lib.EXPORTS) and len(_radiance_lib.EXPORTS) == 8
    assert _exported(_lib.lib_path()) == set(_lib.EXPORTS) | set(_lib.DEBUG_EXPORTS)
    assert build.code_hash() == json.load(open(os.path.join(ROOT, "profiles", "pmc_c2.json")))["code_hash"]
    for header in ("ptrace.h", "ptrace_rays.h", "ptrace_surface.h", "ptrace_scatter.h", "ptrace_radiance.h"):
        assert "pt_rays_gather" not in open(os.path.join(ROOT, "include", header)).read()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_offsets_match_the_python_mirror(lib, n):
    for channels in range(2):
        planes = 3 + (1 if channels & rb.GATHER_COUNT else 0)
        assert lib.pt_rays_gather_bytes(n, channels) == rb.gather_bytes(n, channels) == 8 * n * planes
        want = {(0, c): 8 * n * c for c in range(3)}
        if channels & rb.GATHER_COUNT:
            want[(rb.GATHER_COUNT, 0)] = 24 * n
        for sel in (0, rb.GATHER_COUNT, 2, 3, -1):
            for comp in (-1, 0, 1, 2, 3):
                got, mirror = lib.pt_rays_gather_plane_offset(n, channels, sel, comp), rb.gather_plane_offset(n, channels, sel, comp)
                if (sel, comp) in want:
                    assert got == mirror == want[(sel, comp)], (n, channels, sel, comp)
                else:
                    assert got == ERR_INVALID and mirror == -1, (n, channels, sel, comp)
    for bad in (2, 3, -1, 1 << 20):
        assert lib.pt_rays_gather_bytes(n, bad) == 0 and rb.gather_bytes(n, bad) == 0
        assert lib.pt_rays_gather_plane_offset(n, bad, 0, 0) == ERR_INVALID and rb.gather_plane_offset(n, bad, 0, 0) == -1
    for bad_n in (-1, 2 ** 31):
        assert lib.pt_rays_gather_bytes(bad_n, 1) == 0 and rb.gather_bytes(bad_n, 1) == 0
        assert lib.pt_rays_gather_plane_offset(bad_n, 1, 0, 0) == ERR_INVALID and rb.gather_plane_offset(bad_n, 1, 0, 0) == -1


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """No GPU here: whatever is refused with PT_ERR_INVALID / UNSUPPORTED / SIZE was refused by the argument checks (the first HIP
    call would answer PT_ERR_NODEVICE)."""
    from pytracer_amd import _gather_lib

    nb = int(lib.pt_rays_gather_args_bytes())
    block = (C.c_char * nb)()
    np.frombuffer(block, dtype=np.uint8)[:] = 1  # (a block whose `cold` pointer is set and whose shape count is positive)
    n = 5
    pts, nrm = np.zeros((3, n)), np.zeros((3, n))
    act, seq = np.zeros(n, np.int32), np.zeros(n, np.uint64)
    out = np.zeros(rb.gather_bytes(n, 1), np.uint8)
    ws = np.zeros(4096, np.uint8)

    def call(device=0, blk=block, nbytes=nb, p_=pts, n_=nrm, a_=act, s_=seq, count=n, K=3, N=1, D=3, limit=2, depth=0, ch=1, o=out, ob=None,
             wb=None, null_par=False):
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        par = None if null_par else C.byref(_gather_lib.params(K, N, D, limit, depth, 42, 54, (0, 0, 0)))
        ob = (o.nbytes if o is not None else 0) if ob is None else ob
        host = lib.pt_rays_gather(device, blk, nbytes, p(p_), p(n_), p(a_), p(s_), count, par, ch, p(o), ob)
        dev = lib.pt_rays_gather_device(device, blk, nbytes, p(p_), p(n_), p(a_), p(s_), count, par, ch, p(ws), ws.nbytes if wb is None else wb,
                                        p(o), ob, None)
        return host, dev

    both = lambda code: (code, code)  # noqa: E731
    passed = lambda rc: rc not in (ERR_INVALID, ERR_UNSUPPORTED, ERR_SIZE)  # noqa: E731  (got as far as the first HIP call)
    assert call(K=0) == both(ERR_INVALID) and "samples" in _gather_lib.last_error()
    assert call(K=-3) == both(ERR_INVALID)
    assert call(N=0) == both(ERR_INVALID) and "num_of_rays" in _gather_lib.last_error()
    assert call(D=-1) == both(ERR_INVALID)
    assert call(depth=-1) == both(ERR_INVALID) and "depth" in _gather_lib.last_error()
    assert call(count=-1) == both(ERR_INVALID) and call(count=2 ** 31) == both(ERR_INVALID)
    # n * samples beyond 2^31 - 1
    assert call(count=2 ** 30, K=2) == both(ERR_INVALID) and "2^31 - 1" in _gather_lib.last_error()
    assert call(count=5, K=2 ** 31 - 1) == both(ERR_INVALID)
    assert call(count=3, K=715827883) == both(ERR_INVALID)  # 3 * 715827883 = 2^31 + 1
    assert call(D=65) == both(ERR_UNSUPPORTED) and "64 levels" in _gather_lib.last_error()
    assert call(D=2 ** 31 - 1, depth=2 ** 31 - 66) == both(ERR_UNSUPPORTED)
    assert passed(call(D=2 ** 31 - 1, depth=2 ** 31 - 65)[0])  # 64 levels: accepted
    assert passed(call(D=3, depth=7)[0])  # deeper than max_depth: legal (black)
    assert call(ch=2) == both(ERR_INVALID) and call(ch=3) == both(ERR_INVALID) and call(ch=-1) == both(ERR_INVALID)
    assert call(device=-1) == both(ERR_INVALID)
    assert call(blk=None) == both(ERR_INVALID)
    assert call(nbytes=nb - 8) == both(ERR_INVALID) and "one build" in _gather_lib.last_error()
    assert call(nbytes=nb + 8) == both(ERR_INVALID)
    assert call(null_par=True) == both(ERR_INVALID)
    for missing in ("p_", "n_", "o"):
        assert call(**{missing: None}, ob=out.nbytes) == both(ERR_INVALID), missing
    for optional in ("a_", "s_"):  # NULL: every record is active / seq_i = init_seq + i K
        assert all(passed(rc) for rc in call(**{optional: None})), optional
    assert call(ob=out.nbytes - 1) == both(ERR_SIZE) and "too small" in _gather_lib.last_error()
    assert call(ob=rb.gather_bytes(n, 0), ch=1) == both(ERR_SIZE) and passed(call(ob=rb.gather_bytes(n, 0), ch=0)[0])
    # a workspace that cannot even hold the sample planes (4 x 8 bytes per sample): refused without asking a device
    assert call(wb=n * 3 * 32 - 1)[1] == ERR_SIZE and "workspace" in _gather_lib.last_error() and passed(call(wb=n * 3 * 32)[1])
    assert lib.pt_rays_gather_device(0, block, nb, pts.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), None, None, n,
                                     C.byref(_gather_lib.params(3, 1, 3, 2, 0, 42, 54, (0, 0, 0))), 1, None, 0,
                                     out.ctypes.data_as(C.c_void_p), out.nbytes, None) == ERR_INVALID and "workspace" in _gather_lib.last_error()
    # n = 0: PT_OK with nothing launched (no device is touched), null planes allowed
    assert call(count=0, p_=None, n_=None, a_=None, s_=None, o=None) == both(0)
    assert not out.any()
    # the workspace's size: 0 on refusal, with the reason
    assert lib.pt_rays_gather_workspace_bytes(0, 10, 3, 1, 65, 0) == 0 and "64 levels" in _gather_lib.last_error()
    assert lib.pt_rays_gather_workspace_bytes(0, 10, 0, 1, 3, 0) == 0 and lib.pt_rays_gather_workspace_bytes(0, 10, 3, 0, 3, 0) == 0
    assert lib.pt_rays_gather_workspace_bytes(-1, 10, 3, 1, 3, 0) == 0 and lib.pt_rays_gather_workspace_bytes(0, -1, 3, 1, 3, 0) == 0
    assert lib.pt_rays_gather_workspace_bytes(0, 2 ** 30, 2, 1, 3, 0) == 0


def test_channel_names_the_views_and_the_parameter_block():
    from pytracer_amd import _gather_lib

    assert rb.gather_channels("all") == 1 and rb.gather_channels("none") == 0 and rb.gather_channels("count") == rb.GATHER_COUNT
    assert rb.gather_channels(0) == 0 and rb.gather_channels(1) == 1
    for bad in ("pcg", 2, -1):
        with pytest.raises(ValueError):
            rb.gather_channels(bad)
    n = 6
    buf = np.zeros(rb.gather_bytes(n, 1), np.uint8)
    buf.view(np.float64)[: 3 * n] = np.arange(3 * n)
    buf.view(np.uint64)[3 * n:] = np.arange(100, 100 + n)
    res = rb.GatheredRadiance(buf, n, "all", shape=(1, 2, 3))
    assert res.radiance.shape == (1, 2, 3, 3) and np.array_equal(res.radiance[0, 1, 2], [5.0, 11.0, 17.0])
    assert res.n_rays.shape == (1, 2, 3) and res.n_rays[0, 1, 0] == 103
    assert np.shares_memory(res.radiance, buf) and np.shares_memory(res.n_rays, buf) and set(res.planes()) == {"radiance", "n_rays"}
    only = rb.GatheredRadiance(np.zeros(rb.gather_bytes(n, 0), np.uint8), n, "none")
    assert not only.has("count") and set(only.planes()) == {"radiance"}
    with pytest.raises(KeyError, match="count"):
        only.n_rays
    with pytest.raises(ValueError):
        rb.GatheredRadiance(np.zeros(8, np.uint8), n)
    with pytest.raises(ValueError):
        rb.GatheredRadiance(buf, n, shape=(2, 2))
    # stream numbers and seeds wrap into 64 bits as pcg_streams wraps them
    assert rb.stream_numbers([2 ** 64 + 3, -1]).tolist() == [3, 2 ** 64 - 1] and rb.stream_numbers(np.array([-2], np.int64)).tolist() == [2 ** 64 - 2]
    par = _gather_lib.params(3, 1, 10, 3, 0, -1, 2 ** 64 + 5, (0.5, 0.25, 1))
    assert (par.init_state, par.init_seq, par.samples, list(par.background)) == (2 ** 64 - 1, 5, 3, [0.5, 0.25, 1.0])
    with pytest.raises(ValueError, match="samples"):
        _gather_lib.params(2 ** 31, 1, 10, 3, 0, 42, 54, (0, 0, 0))


def test_hemisphere_radiance_takes_records_or_plain_arrays():
    """What reaches ``DeviceScene.gather``, without a device: a records object hands over its ``shape_index`` as ``active``; plain
    ``points`` with ``normals=`` hand over none; the result is shaped like the records."""
    seen = {}

    class Scene:
        def gather(self, points, normals, samples, init_state, seqs, active, *rest, **kw):
            seen.update(points=points, normals=normals, samples=samples, init_state=init_state, seqs=seqs, active=active, rest=rest, kw=kw)
            return rb.GatheredRadiance(np.zeros(rb.gather_bytes(points.shape[1], 1), np.uint8), points.shape[1], 1)

    class Frame:
        shape_index = np.array([[0, -1, 2], [3, 4, -1]], np.int32)
        point = np.arange(18.0).reshape(2, 3, 3)
        normal = -np.arange(18.0).reshape(2, 3, 3)

    wq = rb.WorldQueries(Scene())
    res = wq.hemisphere_radiance(Frame, 7)
    assert res.radiance.shape == (2, 3, 3) and res.n_rays.shape == (2, 3)
    assert seen["points"].shape == (3, 6) and np.array_equal(seen["points"][:, 4], [12.0, 13.0, 14.0]) and seen["active"] is Frame.shape_index
    assert (seen["samples"], seen["init_state"], seen["seqs"]) == (7, 42, None)
    assert seen["rest"] == (1, 10, 3, (0.0, 0.0, 0.0), 0, 1) and seen["kw"] == {"init_seq": 54}  # PathTracer's defaults
    res = wq.hemisphere_radiance(np.zeros((5, 3)), 2, 45, [1, 2, 3, 4, 5], normals=np.ones((5, 3)), channels="none")
    assert res.radiance.shape == (5, 3) and seen["active"] is None and seen["seqs"] == [1, 2, 3, 4, 5] and seen["normals"].shape == (3, 5)
    with pytest.raises(ValueError, match="normals="):
        wq.hemisphere_radiance(np.zeros((5, 3)), 2)


def test_the_expected_values_depend_on_the_order_of_the_sum(oracle):
    """The discriminating power of the GPU's bit test: on the ``mirrors`` expected values at K = 70, adding each record's samples
    from the last to the first changes the bits of at least 10 % of the records."""
    K, N, D, limit = G.CASES[3]
    assert (K, N) == (70, 1)
    want = G.expected(oracle, "mirrors", K, N, D, limit)
    assert want["samples"].shape == (130, 70, 3) and G.same_bits(G.ordered_mean(want["samples"]), want["radiance"]).all()
    changed = ~G.same_bits(G.ordered_mean(want["samples"], reverse=True), want["radiance"])
    print(f"mirrors K=70: the reverse order changes {changed.mean():.1%} of the records")
    assert changed.mean() >= 0.10
    # the samples take several values per record (uniform pigments, depth 2: a handful of paths; a sum of 70 equal values would
    # not tell orders apart) and the counts are the samples' sum
    assert np.median([len(np.unique(want["samples"][i], axis=0)) for i in range(130)]) >= 3
    assert np.array_equal(want["count"], want["sample_counts"].sum(axis=1)) and want["count"].min() >= K


def test_the_oracles_composition_is_the_contract(oracle):
    """One record by hand: the generator of sample k is PCG(init_state, seq + k), the hemisphere ray starts at the point with
    tmin 1e-3 and an infinite tmax after two draws, and the mean is the ordered sum times 1.0 / K."""
    r = G.records(oracle, "demo")
    want = G.expected(oracle, "demo", 3, 2, 2, 1)
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        from pytracer_amd import abi
        from pytracer_amd import hostmodel as hm

        from . import radiance_batches as R

        i = 7
        acc = np.zeros(3)
        for k in range(3):
            g = oracle.Pcg(G.S0, int(r["seq"][i]) + k)
            start = hm.PCG(G.S0, int(r["seq"][i]) + k)
            assert (g.state, g.inc) == (start.state, start.inc)
            ray = oracle.scatter(abi.BRDF_DIFFUSE, g, r["in_dir"][i], r["point"][i], r["normal"][i], 0)
            assert np.array_equal(ray[0:3], r["point"][i]) and ray[6] == 1.0e-3 and ray[7] == np.inf
            assert g.state == hm.pcg_advance(start.state, start.inc, 2)
            L, _ = oracle.radiance(R.world("demo")[0], R.params(2, 2, 1), g, ray, 0)
            acc = acc + L
        assert np.array_equal(acc * (1.0 / 3), want["radiance"][i])
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
