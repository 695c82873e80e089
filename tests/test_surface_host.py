"""CPU-only tests of the surface queries (include/ptrace_surface.h, libptrace_surface.so, pytracer_amd.rays / .shaders): the
library builds and loads without a GPU, its header, the ctypes table and its dynamic symbols agree, sizes and offsets match
their Python mirrors, bad arguments are refused before any HIP call, ``PointLightShader``'s scalar form is the oracle's
``PointLightRenderer``, and the batches the GPU tests compare bit for bit are fit for that: no acos decides a branch by
rounding, and no batch is vacuous."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pytracer_amd import abi, hits, rays as rb, shaders
from pytracer_amd import hostmodel as hm

from . import surface_batches as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_SIZE = -1, -5  # include/ptrace.h
V11 = (1 << 16) | 1


@pytest.fixture(scope="module")
def libs():
    from pytracer_amd import _lib, _rays_lib, _surface_lib, build

    build.build()
    assert os.path.exists(build.SURFACE_LIB) and not build.needs_build()
    return _lib.lib(), _rays_lib.lib(), _surface_lib.lib()


def test_the_library_loads_and_the_header_the_table_and_the_symbols_agree(libs):
    from pytracer_amd import _surface_lib, build

    _, R, Sf = libs
    header = open(os.path.join(ROOT, "include", "ptrace_surface.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|long long)\s+(pt_rays_[a-z_]+)\s*\(", header, flags=re.M))
    assert declared == set(_surface_lib.EXPORTS) and len(declared) == 11
    nm = subprocess.run(["nm", "-D", "--defined-only", _surface_lib.lib_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pt_[a-z_0-9]+)$", nm, flags=re.M))
    assert exported == declared, exported ^ declared
    # an add-on like libptrace_rays.so: no link dependency on either of the others, nothing that loads a library
    needed = subprocess.run(["readelf", "-d", _surface_lib.lib_path()], capture_output=True, text=True).stdout
    assert "libptrace" not in needed.replace("libptrace_surface.so", "")
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _surface_lib.lib_path()], capture_output=True, text=True).stdout
    assert not re.search(r"\b(dlopen|dlsym|dlmopen)\b", undefined)
    # interface 1.1 in both halves; one argument block for all
    assert R.pt_rays_version() == V11 and Sf.pt_rays_surface_version() == V11
    assert Sf.pt_rays_surface_args_bytes() == R.pt_rays_args_bytes() > 0
    assert '#include "ptrace_surface.h"' in open(os.path.join(ROOT, "include", "ptrace_rays.h")).read()
    # the only file that includes the new device header is the new translation unit
    users = [f for f in os.listdir(build.CSRC) if '"pt_surface.h"' in open(os.path.join(build.CSRC, f)).read()]
    assert users == ["ptrace_surface.hip"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1001, 2 ** 31 - 1])
def test_sizes_and_offsets_match_the_python_mirror(libs, n):
    Sf = libs[2]
    pad = (n * 4 + 7) // 8 * 8
    for channels in range(4):
        want = rb.surface_bytes(n, channels)
        assert Sf.pt_rays_surface_bytes(n, channels) == want == pad + 24 * n * bin(channels).count("1")
        assert Sf.pt_rays_surface_plane_offset(n, channels, 0, 0) == 0 and Sf.pt_rays_surface_plane_offset(n, channels, 0, 1) == ERR_INVALID
        at = pad
        for bit in (rb.SURF_BRDF_COLOR, rb.SURF_EMITTED):
            for comp in range(-1, 4):
                got = Sf.pt_rays_surface_plane_offset(n, channels, bit, comp)
                assert got == rb.surface_plane_offset(n, channels, bit, comp)
                if channels & bit and 0 <= comp < 3:
                    assert got == at + comp * n * 8  # planes in bit order, back to back
                else:
                    assert got < 0
            if channels & bit:
                at += 24 * n
        assert at == want
        for bad in (3, 4, 8):  # no such channel
            assert Sf.pt_rays_surface_plane_offset(n, channels, bad, 0) < 0 and rb.surface_plane_offset(n, channels, bad, 0) < 0
    for bad in (4, 7, -1, 1 << 20):
        assert Sf.pt_rays_surface_bytes(n, bad) == 0 and rb.surface_bytes(n, bad) == 0
        assert Sf.pt_rays_surface_plane_offset(n, bad, 0, 0) == ERR_INVALID and rb.surface_plane_offset(n, bad, 0, 0) < 0
    assert Sf.pt_rays_surface_bytes(-1, 3) == 0 and Sf.pt_rays_surface_bytes(2 ** 31, 3) == 0 and rb.surface_bytes(2 ** 31, 3) == 0


def _block(Sf):
    """A block nobody uploaded, with what the checks read: a non-null `cold` (never dereferenced by a refused call), no shapes."""
    nb = int(Sf.pt_rays_surface_args_bytes())
    block = C.create_string_buffer(nb)
    C.memmove(block, (C.c_uint64 * 1)(0x1000), 8)
    return block, nb


def test_every_refusal_comes_before_a_hip_call(libs):
    """No GPU here: a call that reached the HIP runtime would answer PT_ERR_NODEVICE or PT_ERR_HIP instead."""
    from pytracer_amd import _surface_lib

    Sf = libs[2]
    block, nb = _block(Sf)
    n = 4
    shape, uv, v3 = np.zeros(n, np.int32), np.zeros((2, n)), np.zeros((3, n))
    out = np.zeros(rb.surface_bytes(n, 3), np.uint8)
    col = np.zeros((3, n))
    amb, bg = (C.c_double * 3)(0.1, 0.1, 0.1), (C.c_double * 3)()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    slots = C.c_void_p(0x2000)  # (a device address nobody reads in a refused call)
    bad = ERR_INVALID

    def surface(device=0, blk=block, nbytes=nb, sl=slots, sh=p(shape), u=p(uv), count=n, ch=3, o=p(out), ob=out.nbytes):
        host = Sf.pt_rays_surface(device, blk, nbytes, sh, u, count, ch, o, ob)
        return host, Sf.pt_rays_surface_device(device, blk, nbytes, sl, sh, u, count, ch, o, ob, None)

    def lights(device=0, blk=block, nbytes=nb, sl=slots, sh=p(shape), pt=p(v3), nr=p(v3), u=p(uv), d=p(v3), count=n, a=amb, b=bg, o=p(col),
               ob=col.nbytes):
        host = Sf.pt_rays_shade_lights(device, blk, nbytes, sh, pt, nr, u, d, count, a, b, o, ob)
        return host, Sf.pt_rays_shade_lights_device(device, blk, nbytes, sl, sh, pt, nr, u, d, count, a, b, o, ob, None)

    for call in (surface, lights):
        assert call(count=-1) == (bad, bad) and call(count=2 ** 31) == (bad, bad)          # bad n
        assert call(nbytes=nb - 8) == (bad, bad) and call(nbytes=nb + 8) == (bad, bad)      # a block of another size
        assert call(blk=None) == (bad, bad) and call(device=-1) == (bad, bad)
        assert call(blk=C.create_string_buffer(nb)) == (bad, bad)                          # a block nobody filled
        assert call(sh=None) == (bad, bad) and call(o=None) == (bad, bad)                    # a NULL plane that is needed
        assert call(sl=None)[1] == bad                                                       # (the host forms make the table themselves)
        assert call(ob=call.__defaults__[-1] - 1) == (ERR_SIZE, ERR_SIZE) and "too small" in _surface_lib.last_error()
    assert surface(ch=4) == (bad, bad) and surface(ch=-1) == (bad, bad) and surface(ch=1 << 20) == (bad, bad)  # unknown channel bits
    assert surface(u=None) == (bad, bad) and surface(u=None, ch=1) == (bad, bad) and "uv" in _surface_lib.last_error()
    for name in ("pt", "nr", "u", "d", "a", "b"):
        assert lights(**{name: None}) == (bad, bad), name
    # the slot table: a refused block gives 0 bytes; a short table, a null one and a bad device are refused
    assert Sf.pt_rays_slots_bytes(block, nb - 8) == 0 and Sf.pt_rays_slots_bytes(None, nb) == 0
    assert Sf.pt_rays_slots_bytes(C.create_string_buffer(nb), nb) == 0
    assert Sf.pt_rays_slots_device(0, block, nb - 8, slots, 64, None) == bad and Sf.pt_rays_slots_device(-1, block, nb, slots, 64, None) == bad
    assert Sf.pt_rays_slots_device(0, None, nb, slots, 64, None) == bad
    # n = 0: PT_OK, nothing launched (so: no device needed), nothing written; uv may be null without a colour
    out[:] = 0xA5
    assert surface(count=0) == (0, 0) and surface(count=0, sh=None, u=None, o=None, ob=0) == (0, 0) and lights(count=0) == (0, 0)
    assert np.all(out == 0xA5)


def test_a_short_slot_table_is_refused_before_a_hip_call(libs):
    """A block with shapes in it comes from an upload, which needs a GPU.  Here the count is planted into an empty block, at the
    one int32 whose value pt_rays_slots_bytes follows."""
    Sf = libs[2]
    block, nb = _block(Sf)
    assert Sf.pt_rays_slots_bytes(block, nb) == 0  # (zero shapes)
    found = None
    for off in range(8, nb - 3, 4):  # find n_shapes: the one int32 whose value pt_rays_slots_bytes follows
        probe = C.create_string_buffer(block.raw, nb)
        C.memmove(C.byref(probe, off), (C.c_int32 * 1)(5), 4)
        if Sf.pt_rays_slots_bytes(probe, nb) == 24:
            found = (off, probe)
            break
    assert found is not None
    off, probe = found
    C.memmove(C.byref(probe, off), (C.c_int32 * 1)(1001), 4)
    assert Sf.pt_rays_slots_bytes(probe, nb) == 4008  # 4 * 1001 rounded up to 8
    slots = C.c_void_p(0x2000)
    assert Sf.pt_rays_slots_device(0, probe, nb, slots, 4007, None) == ERR_SIZE
    assert Sf.pt_rays_slots_device(0, probe, nb, slots, 0, None) == ERR_SIZE
    assert Sf.pt_rays_slots_device(0, probe, nb, None, 4008, None) == ERR_INVALID
    C.memmove(C.byref(probe, off), (C.c_int32 * 1)(-3), 4)
    assert Sf.pt_rays_slots_bytes(probe, nb) == 0 and Sf.pt_rays_slots_device(0, probe, nb, slots, 4008, None) == ERR_INVALID


def test_channels_views_and_planes():
    assert rb.surface_channels("all") == 3 and rb.surface_channels("none") == 0 and rb.surface_channels("emitted") == rb.SURF_EMITTED
    assert rb.surface_channels("emitted, brdf_color") == 3 and rb.surface_channels(1) == rb.SURF_BRDF_COLOR
    for bad in ("uv", 4, -1):
        with pytest.raises(ValueError):
            rb.surface_channels(bad)
    n = 5
    buf = np.zeros(rb.surface_bytes(n, 3), np.uint8)
    sc = rb.SurfaceColors(buf, n)
    sc.brdf_kind[:] = [0, -1, 1, 0, -1]
    sc.emitted[2] = (1.0, 2.0, 3.0)
    pad = 24
    assert np.array_equal(buf[pad + 24 * n:].view(np.float64).reshape(3, n)[:, 2], [1.0, 2.0, 3.0])  # planar: component-major
    assert np.array_equal(sc.hit, [True, False, True, True, False]) and sorted(sc.planes()) == ["brdf_color", "brdf_kind", "emitted"]
    assert np.shares_memory(sc.emitted, buf) and np.shares_memory(sc.brdf_color, buf) and sc.brdf_color.shape == (n, 3)
    only = rb.SurfaceColors(np.zeros(rb.surface_bytes(6, 2), np.uint8), 6, "emitted", shape=(1, 2, 3))
    assert only.emitted.shape == (1, 2, 3, 3) and only.brdf_kind.shape == (1, 2, 3) and not only.has("brdf_color")
    with pytest.raises(KeyError):
        only.brdf_color
    with pytest.raises(ValueError):
        rb.SurfaceColors(np.zeros(8, np.uint8), 6)
    with pytest.raises(ValueError):
        rb.SurfaceColors(buf, n, shape=(2, 2))
    # planar(): the strided views of a RayHits and of a hit frame are planes seen from the other side -- no copy
    h = rb.RayHits(np.zeros(rb.rays_bytes(7, rb.RAY_CHANNELS), np.uint8), 7)
    assert np.shares_memory(rb.planar(h.point, 3), h.buffer) and np.shares_memory(rb.planar(h.uv, 2), h.buffer)
    frame = hits.HitFrame(None, abi.make_params(4, 3, abi.RENDERER_FLAT, samples_per_side=2), abi.HIT_ALL)
    assert np.shares_memory(rb.planar(frame.ray_dir, 3), frame.buffer) and rb.planar(frame.normal, 3).shape == (3, 48)
    rows = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(rb.planar(rows, 3), rows.T) and rb.planar(rows, 3).flags.c_contiguous
    with pytest.raises(ValueError):
        rb.planar(rows, 2)


# ---- the scalar form of the shader against the oracle ---------------------------------------------------------------------------
class OracleLightWorld(hm.World):
    """A world that can answer both questions of ``PointLightRenderer`` -- by asking the oracle (test infrastructure)."""

    def __init__(self, world, orc):
        from pytracer_amd import flatten

        super().__init__()
        self.shapes, self.point_lights = world.shapes, world.point_lights
        self.flat, self.orc = flatten.flatten_world(world), orc

    def ray_intersection(self, ray):
        o, d = ray.origin, ray.dir
        r = self.orc.world_intersect(self.flat, self.orc.ray8([o.x, o.y, o.z], [d.x, d.y, d.z], ray.tmin, ray.tmax))
        if r is None:
            return None
        return hits.HitRecord(world_point=hm.Vec(*r[1:4]), normal=hm.Vec(*r[4:7]), surface_point=hits.Vec2d(r[7], r[8]), t=float(r[0]),
                              ray=ray, shape_index=int(r[9]))

    def is_point_visible(self, point, observer_pos):
        return self.orc.is_point_visible(self.flat, [point.x, point.y, point.z], [observer_pos.x, observer_pos.y, observer_pos.z])


@pytest.mark.parametrize("name", ["demo", "c2_lights", "pigments", "lights"])
def test_the_shaders_scalar_form_is_the_oracles_point_light_renderer(oracle, name):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        b = S.batch(oracle, name)
        world = OracleLightWorld(S.host_world(name)[0], oracle)
        shader = shaders.PointLightShader(world, None, hm.Color(*S.BACKGROUND), hm.Color(*S.AMBIENT))
        n = b["rec"].n
        picks = sorted(set(range(0, n, max(1, n // 150))) | set(range(b["n_primary"], n, max(1, n // 150))))
        seen_miss = False
        for i in picks:
            r = b["rays"][i]
            ray = hits.HitRay(hm.Vec(*r[0:3]), hm.Vec(*r[3:6]), float(r[6]), float(r[7]))
            c = shader(ray)
            assert (c.r, c.g, c.b) == tuple(b["colors"][i]), (name, i)
            seen_miss |= not b["rec"].hit[i]
        assert len(np.unique(b["colors"][picks], axis=0)) > 20 and (seen_miss or name != "demo")
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
    with pytest.raises(TypeError, match="parameter holder"):
        shaders.PointLightShader(S.host_world("demo")[0])(hits.HitRay(hm.Vec(0, 0, 0), hm.Vec(1, 0, 0)))
    with pytest.raises(TypeError, match="tracer"):
        shaders.PointLightShader(world).shade_hits(None)


# ---- the batches the GPU tests compare -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.WORLDS))
def test_no_specular_pair_is_near_the_threshold_and_no_batch_is_vacuous(oracle, name):
    """The one libm call of the lights kernel is the acos pair in ``|th_in - th_out| < threshold``: it decides a branch and
    never enters a value.  No visible (specular record, light) pair of any batch lies within 1e-9 rad of its threshold -- ocml's
    acos and glibc's differ by a few ulp, 1e-15 -- so the bit-for-bit comparisons of the GPU tests leave no record out."""
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        b = S.batch(oracle, name)
        flat = S.world(name)[0]
        margins = S.specular_margins(oracle, name)
        print(f"{name}: {b['rec'].n} records, {int(b['rec'].hit.sum())} hits, {flat.n_lights} lights, {len(margins)} visible specular-light pairs, "
              f"closest {min(map(abs, margins)) if margins else float('nan'):.3g} rad from the threshold, {sum(m < 0 for m in margins)} inside it")
        assert all(abs(m) > 1e-9 for m in margins)
        rec, mat = b["rec"], b["materials"]
        assert rec.n > 1000 and rec.hit.sum() > 1000 and len(np.unique(rec.shape_index)) >= 3
        assert set(np.unique(mat["brdf_kind"][rec.hit])) == {abi.BRDF_DIFFUSE, abi.BRDF_SPECULAR}
        assert len(np.unique(mat["brdf_color"], axis=0)) >= 3 and len(np.unique(mat["emitted"], axis=0)) >= 2
        if name == "demo":
            assert (~rec.hit).sum() > 100 and np.all(b["colors"][~rec.hit] == S.BACKGROUND) and len(margins) >= 1
        if name == "c2":
            assert flat.n_lights == 0 and np.array_equal(b["colors"], np.asarray(S.AMBIENT) + mat["emitted"])
        else:
            assert flat.n_lights >= 1 and len(np.unique(b["colors"], axis=0)) > 400
            lit = np.any(b["colors"] != np.asarray(S.AMBIENT) + mat["emitted"], axis=1)
            assert 0.1 < lit[rec.hit].mean() < 0.95, "shadowed and lit records"
        if name == "pigments":
            kinds = set(np.asarray(flat.pig_kind)[np.unique(rec.shape_index[rec.hit])])
            assert {abi.PIGMENT_CHECKERED, abi.PIGMENT_IMAGE} <= kinds
        if name == "lights":
            assert flat.n_lights >= 4 and sum(m < 0 for m in margins) >= 1  # (the specular branch IS taken here: thresholds up to pi)
        if name == "wide300_lights":
            assert flat.n_shapes > 256
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def test_the_aimed_specular_cases_straddle_the_threshold(oracle):
    """e = thr / 2 and thr - 1e-6 are lit (about 1e-4 to 5e-4 a channel), e = thr + 1e-6 is not, at both radii; and 1e-6 rad
    is far outside what two acos implementations can differ by."""
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        base = np.asarray(S.AMBIENT) + (0.01, 0.02, 0.03)
        for e, radius in S.AIMED:
            flat, ray = S.aimed_case(e, radius)
            rec = S.B.expected(oracle, flat, ray)
            assert rec.hit[0] and np.abs(rec.point[0]).max() < 1e-12
            gap = S._angle_gap(rec.point[0] - np.asarray(flat.light_pos).reshape(3), rec.normal[0], -ray[0, 3:6])
            assert abs(gap - e) < 1e-12 and abs(gap - S.THRESHOLD) > 9e-7
            added = S.expected_colors(oracle, flat, ray)[0] - base
            if e < S.THRESHOLD:
                assert np.all(added > 5e-5) and np.all(added < 6e-4), (e, radius, added)
            else:
                assert np.all(np.abs(added) < 1e-16), (e, radius, added)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
