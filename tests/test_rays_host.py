"""CPU-only tests of the ray-batch add-on (include/ptrace_rays.h, libptrace_rays.so, pytracer_amd.rays): both libraries
build and load without a GPU, the header, the ctypes table and the library's dynamic symbols agree, sizes and offsets match
their Python mirror, bad arguments are refused before any HIP call, and the host-side ray construction of
``is_point_visible`` is the reference's.  Also: the batches the GPU tests compare are not vacuous."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi, rays as rb

from . import ray_batches as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = rb.RAY_CHANNELS
ERR_INVALID, ERR_SIZE = -1, -5  # include/ptrace.h


@pytest.fixture(scope="module")
def libs():
    from pytracer_amd import _lib, _rays_lib, build

    build.build()
    assert os.path.exists(build.LIB) and os.path.exists(build.RAYS_LIB) and not build.needs_build()
    return _lib.lib(), _rays_lib.lib()


def test_both_libraries_load_and_the_header_the_table_and_the_symbols_agree(libs):
    from pytracer_amd import _lib, _rays_lib

    L, R = libs
    header = open(os.path.join(ROOT, "include", "ptrace_rays.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_rays_lib.EXPORTS) and len(declared) == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _rays_lib.lib_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))
    assert exported == declared, exported ^ declared
    # no link dependency between the two, and nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _rays_lib.lib_path()], capture_output=True, text=True).stdout
    assert "libptrace.so" not in needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _rays_lib.lib_path()], capture_output=True, text=True).stdout
    assert not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    assert R.pt_rays_version() >> 16 == 1
    assert L.pt_version() >> 16 == 1 and (L.pt_version() & 0xFFFF) >= 7 and "pt_scene_kernel_args" in _lib.EXPORTS
    assert R.pt_rays_args_bytes() > 0 and R.pt_rays_args_bytes() % 8 == 0


def test_libptrace_device_code_is_the_profiled_one():
    """Every profiles/pmc_*.json prices bench.py's roofline only for the device code it names: the add-on must not change it."""
    import glob
    import json

    from pytracer_amd import build

    build.build()
    have = build.code_hash()
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "pmc_*.json")))
    assert files
    for f in files:
        assert json.load(open(f)).get("code_hash") == have, f


@pytest.mark.parametrize("anyhit", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_sizes_and_offsets_match_the_python_mirror(libs, n, anyhit):
    _, R = libs
    for channels in range(16):
        ok = not (anyhit and channels)
        want = rb.rays_bytes(n, channels, bool(anyhit))
        assert R.pt_rays_bytes(n, channels, anyhit) == want
        planes = sum(k for bit, k in rb._PLANES.items() if channels & bit)
        assert want == ((((n * 4 + 7) // 8) * 8 + n * 8 * planes) if ok else 0)
        assert R.pt_rays_plane_offset(n, channels, anyhit, 0, 0) == (0 if ok else ERR_INVALID)
        at = (n * 4 + 7) // 8 * 8
        for bit, k in rb._PLANES.items():
            for comp in range(-1, k + 1):
                got = R.pt_rays_plane_offset(n, channels, anyhit, bit, comp)
                assert got == rb.rays_plane_offset(n, channels, bool(anyhit), bit, comp)
                if ok and channels & bit and 0 <= comp < k:
                    assert got == at + comp * n * 8  # planes in bit order, back to back
                else:
                    assert got < 0
            if ok and channels & bit:
                at += k * n * 8
        assert at == want or not ok
    if n:
        h = rb.RayHits(np.zeros(rb.rays_bytes(n, abi.HIT_T | abi.HIT_UV), np.uint8), n, "t,uv")
        assert h.has("uv") and not h.has("point") and sorted(h.planes()) == ["shape_index", "t", "uv"] and h.uv.shape == (n, 2)
        with pytest.raises(KeyError):
            h.normal


def test_invalid_channels_and_counts(libs):
    _, R = libs
    for bad in (abi.HIT_RAY, abi.HIT_RAY | abi.HIT_T, 32, 64 | abi.HIT_T, -1, 1 << 20):
        assert R.pt_rays_bytes(10, bad, 0) == 0 and rb.rays_bytes(10, bad) == 0
        assert R.pt_rays_plane_offset(10, bad, 0, 0, 0) == ERR_INVALID
    assert R.pt_rays_bytes(10, abi.HIT_T, 1) == 0 and R.pt_rays_bytes(10, 0, 1) == 40 and R.pt_rays_bytes(10, 0, 2) == 0
    assert R.pt_rays_bytes(-1, 0, 0) == 0 and R.pt_rays_bytes(2 ** 31, 0, 0) == 0
    assert R.pt_rays_bytes(2 ** 31 - 1, ALL, 0) == rb.rays_bytes(2 ** 31 - 1, ALL) > 2 ** 37  # (no 32-bit arithmetic)
    assert R.pt_rays_plane_offset(2 ** 31 - 1, ALL, 0, abi.HIT_UV, 1) == rb.rays_plane_offset(2 ** 31 - 1, ALL, False, abi.HIT_UV, 1)
    with pytest.raises(ValueError):
        rb.ray_channels("ray")
    assert rb.ray_channels("all") == ALL and rb.ray_channels("normal,t") == abi.HIT_NORMAL | abi.HIT_T


def test_trace_calls_refuse_bad_arguments_before_any_hip_call(libs):
    """No GPU here: a call that reached the HIP runtime would answer PT_ERR_NODEVICE or PT_ERR_HIP instead."""
    from pytracer_amd import _rays_lib

    _, R = libs
    nb = int(R.pt_rays_args_bytes())
    block = C.create_string_buffer(nb)
    C.memmove(block, (C.c_uint64 * 1)(0x1000), 8)  # (a non-null `cold`: never dereferenced by a refused call)
    n = 4
    rays = np.zeros((8, n))
    out = np.zeros(rb.rays_bytes(n, ALL), np.uint8)
    pr, po = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def both(*a):
        host = R.pt_rays_trace(*a)
        return host, R.pt_rays_trace_device(*a, None), _rays_lib.last_error()

    bad = ERR_INVALID
    assert both(0, block, nb - 8, pr, n, ALL, 0, po, out.nbytes)[:2] == (bad, bad)       # wrong scene_args_bytes
    assert both(0, block, nb + 8, pr, n, ALL, 0, po, out.nbytes)[:2] == (bad, bad)
    assert both(0, None, nb, pr, n, ALL, 0, po, out.nbytes)[:2] == (bad, bad)
    assert both(0, block, nb, pr, -1, ALL, 0, po, out.nbytes)[:2] == (bad, bad)          # negative n
    assert both(0, block, nb, pr, 2 ** 31, ALL, 0, po, out.nbytes)[:2] == (bad, bad)
    assert both(0, block, nb, pr, n, abi.HIT_T, 1, po, out.nbytes)[:2] == (bad, bad)     # channels with any-hit
    assert both(0, block, nb, pr, n, abi.HIT_RAY, 0, po, out.nbytes)[:2] == (bad, bad)
    assert both(0, block, nb, pr, n, 32, 0, po, out.nbytes)[:2] == (bad, bad)
    assert both(0, block, nb, None, n, ALL, 0, po, out.nbytes)[:2] == (bad, bad)
    assert both(-1, block, nb, pr, n, ALL, 0, po, out.nbytes)[:2] == (bad, bad)
    r = both(0, block, nb, pr, n, ALL, 0, po, out.nbytes - 1)                              # output too small
    assert r[:2] == (ERR_SIZE, ERR_SIZE) and "too small" in r[2]
    zero = C.create_string_buffer(nb)                                                      # a block nobody filled
    assert both(0, zero, nb, pr, n, ALL, 0, po, out.nbytes)[:2] == (bad, bad)
    # n = 0: PT_OK, nothing launched (so: no device needed), nothing written
    out[:] = 0xA5
    assert both(0, block, nb, pr, 0, ALL, 0, po, out.nbytes)[:2] == (0, 0) and both(0, block, nb, None, 0, 0, 1, None, 0)[:2] == (0, 0)
    assert np.all(out == 0xA5)
    # pt_scene_kernel_args of libptrace.so refuses a null handle before touching a device too
    L, _ = libs
    assert L.pt_scene_kernel_args(None, block, nb) == bad


def test_ray_planes_and_visibility_rays():
    o = np.arange(12.0).reshape(4, 3)
    d = -o + 0.5
    blk = rb.ray_planes(o, d)
    assert blk.shape == (8, 4) and blk.flags.c_contiguous
    assert np.array_equal(blk[0:3].T, o) and np.array_equal(blk[3:6].T, d) and np.all(blk[6] == 1e-5) and np.all(np.isposinf(blk[7]))
    rows = np.hstack([o, d, np.full((4, 1), -2.0), np.arange(4.0)[:, None]])
    assert np.array_equal(rb.ray_planes(rows), rows.T) and rb.ray_planes(rows).flags.c_contiguous
    assert np.array_equal(rb.ray_planes(o, d, tmin=np.arange(4.0), tmax=7.0)[6:], [np.arange(4.0), np.full(4, 7.0)])
    with pytest.raises(ValueError):
        rb.ray_planes(o)
    with pytest.raises(ValueError):
        rb.ray_planes(o, d[:3])
    v = rb.visibility_rays(o, (1.0, 2.0, 3.5))
    assert v.shape == (8, 4) and np.array_equal(v[0:3].T, np.tile([1.0, 2.0, 3.5], (4, 1))) and np.all(v[7] == 1.0)
    import math

    for i in range(4):  # world.py:72-75 in Python floats: point - observer, then 1e-2 / sqrt(x*x + y*y + z*z)
        dx, dy, dz = float(o[i, 0]) - 1.0, float(o[i, 1]) - 2.0, float(o[i, 2]) - 3.5
        assert (v[3, i], v[4, i], v[5, i]) == (dx, dy, dz)
        assert v[6, i] == 1e-2 / math.sqrt(dx * dx + dy * dy + dz * dz)


@pytest.mark.parametrize("name", list(B.WORLDS))
def test_visibility_rays_are_the_oracles_and_no_batch_is_vacuous(oracle, name):
    """``visibility_rays`` then ``shape_quick_intersect`` over all shapes IS ``is_point_visible`` (world.py:71-80): pins the
    host-side ray construction.  And the shares the GPU comparisons rest on: blocked and free, hit and miss."""
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        b = B.batches(oracle, name)
        flat, _ = B.world(name)
        seg, vis = b["shadow"]["rays"], b["visible"]
        m = seg.shape[0]
        assert m == b["points"].shape[0] == b["bounce"]["rays"].shape[0] and m > 100
        step = max(1, m // 60)  # (every shape for every segment is the CPU's slow way: a spread of ~60 segments per world)
        for i in range(0, m, step):
            blocked = any(oracle.shape_quick_intersect(flat, s, seg[i]) for s in range(flat.n_shapes))
            assert blocked == (not vis[i]), (name, i)
        # "closest hit within tmax exists" is the same verdict (what the any-hit kernel is compared with on the device)
        assert np.array_equal(b["shadow"]["want"].hit, ~vis)
        free, hits = float(vis.mean()), float(b["bounce"]["want"].hit.mean())
        print(f"{name}: {int(b['bounce']['want'].hit.sum())} of {m} bounce rays hit, {int(vis.sum())} of {m} points visible")
        if name in B.FRAME_WORLDS:
            assert 0.1 <= free <= 0.9, f"{name}: {free:.0%} of the points are visible"
        else:
            assert 0 < vis.sum() < m
        if name == "demo":
            assert 0.1 <= hits <= 0.9
        counts = {"demo": (391, 778, 920), "c2p": (1296, 1036, 1296), "wide300": (1296, 1073, 1296), "wide1500": (576, 477, 576)}
        if name in counts:
            assert (int(b["bounce"]["want"].hit.sum()), int(vis.sum()), m) == counts[name]
        prim = b["primary"]["want"]
        assert prim.hit.sum() >= m and len(np.unique(prim.shape_index)) >= 3
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def test_rays_command_refuses_bad_input_before_any_gpu_work(tmp_path):
    from click.testing import CliRunner

    from pytracer_amd.cli import cli

    np.save(tmp_path / "bad.npy", np.zeros((5, 7)))
    r = CliRunner().invoke(cli, ["rays", "--input", str(tmp_path / "bad.npy"), "builtin:c2"])
    assert r.exit_code == 2 and "[n, 8]" in r.output
    np.save(tmp_path / "ok.npy", np.zeros((5, 8)))
    r = CliRunner().invoke(cli, ["rays", "--input", str(tmp_path / "ok.npy"), "--channels", "ray", "builtin:c2"])
    assert r.exit_code == 2 and "--channels" in r.output
    r = CliRunner().invoke(cli, ["rays", "--input", str(tmp_path / "none.npy"), "builtin:c2"])
    assert r.exit_code == 2
