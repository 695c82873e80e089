"""Hit-record frames on the device (pt_render_hits, csrc/pt_hits.h) against the oracle, against the device's own unculled
probe, against the renderers, and through the Python layers above.

What must hold, and why these bounds:
* Against the oracle in its x*x mode (``set_sqr_mode(SQR_MUL)``: the device multiplies where the reference calls pow, SURVEY.md
  H2) hit / miss and the shape index are equal on EVERY sample, and t, the point, the normal and the ray are bit-identical:
  none of them involves a transcendental function, and the kernel runs the same operations in the same order as the Flat
  kernels whose full-size frames are bit-identical to the oracle.  (u, v) of a sphere goes through ocml's atan2 / acos
  against glibc's: relative 1e-11, this project's existing bound for exactly that (tests/test_gpu_probes.py:65); a
  plane's (u, v) uses floor only and is bit-identical.  No sample is excluded.
* Against ``pt_debug_hit_probe`` -- the same device code with no culling, no tiles and caller-supplied rays -- everything is
  bit-identical, (u, v) included.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from pytracer_amd import _lib, abi, flatten, scenes, shaders
from pytracer_amd import hostmodel as hm
from pytracer_amd.hits import HitFrame

from . import util
from .util import oracle_frame  # noqa: F401  (shared with tests/test_gpu_families.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    return device


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o

    o.build()
    o.set_sqr_mode(o.SQR_MUL)
    yield o
    o.set_sqr_mode(o.SQR_POW)


@pytest.fixture()
def tuning(dev):
    saved = {}

    def set_(name, value):
        saved.setdefault(name, dev.get_tuning(name))
        dev.set_tuning(name, value)

    yield set_
    for name, value in saved.items():
        dev.set_tuning(name, value)


_flat = {}


def flat_of(name):
    if name not in _flat:
        if name == "demo":
            world = scenes.demo_world()[0]
        elif name == "c2p":
            world = scenes.synthetic_world(32, with_plane=True)
        elif name == "open":  # C2 + plane without its sky sphere: rays over the horizon hit nothing
            world = scenes.synthetic_world(32, with_plane=True)
            del world.shapes[0]
        elif name == "big":
            world = scenes.synthetic_world(300, wide=True)
        else:
            raise KeyError(name)
        _flat[name] = flatten.flatten_world(world)
    return _flat[name]


def camera_of(name, w, h, ortho=False):
    if ortho:
        return flatten.flatten_camera(hm.OrthogonalCamera(w / h, hm.translation(hm.Vec(-1.0, 0.0, 1.5)) * hm.scaling(hm.Vec(1.0, 3.0, 1.7))))
    if name == "demo":
        return flatten.flatten_camera(scenes.demo_world()[1])
    return flatten.flatten_camera(scenes.synthetic_camera(w, h))


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


CASES = [
    # S, pcg_mode, orthogonal camera, partition
    (0, abi.PCG_SEQ, False, {}),
    (2, abi.PCG_SEQ, False, {}),
    (2, abi.PCG_PIXEL, False, {}),
    (2, abi.PCG_SAMPLE, False, {}),
    (0, abi.PCG_PIXEL, True, {}),
    (2, abi.PCG_SEQ, True, dict(row_block=8, n_ranks=3, rank=1)),
    (2, abi.PCG_PIXEL, False, dict(row_block=5, n_ranks=3, rank=2)),
]


@pytest.mark.parametrize("S,mode,ortho,part", CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("scene", ["demo", "c2p", "open"])
def test_small_frames_equal_the_oracle(dev, orc, scene, S, mode, ortho, part):
    W, H = 161, 97  # not multiples of 8: edge tiles in both directions
    flat, cam = flat_of(scene), camera_of(scene, W, H, ortho)
    p = abi.make_params(W, H, abi.RENDERER_POINTLIGHT, samples_per_side=S, pcg_mode=mode, jitter_state=45, jitter_seq=54,
                        path_state=1234, path_seq=77, out_format=abi.OUT_F32, **part)  # (renderer, out_format: ignored)
    with dev.DeviceScene(flat) as ds:
        got = ds.render_hits(cam, p, abi.HIT_ALL)
        st = ds.stats()
    exp = oracle_frame(orc, flat, cam, p)
    n = got.shape_index.size
    assert st.kernel == abi.KERNEL_HITS and st.n_pixels * got.nsamp == st.n_rays == n and st.n_rays_resolved == 0
    assert np.array_equal(got.shape_index, exp.shape_index), "hit / miss or the winning shape differs on some sample"
    hit = exp.hit
    assert hit.any() and (scene != "open" or ortho or not hit.all())
    assert _bits(got.ray_origin, exp.ray_origin) and _bits(got.ray_dir, exp.ray_dir)
    assert _bits(got.t, exp.t) and np.all(np.isposinf(got.t[~hit]))
    assert _bits(got.point, exp.point) and _bits(got.normal, exp.normal)
    plane = hit & (flat.kind[np.where(hit, exp.shape_index, 0)] == abi.SHAPE_PLANE)
    assert _bits(got.uv[plane], exp.uv[plane]) and _bits(got.uv[~hit], exp.uv[~hit])  # floor only / zeros
    a, b = got.uv[hit & ~plane], exp.uv[hit & ~plane]
    err = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    print(f"{scene} S={S} mode={mode} ortho={ortho}: {int(hit.sum())} hits of {n}, sphere uv max rel err {err.max() if err.size else 0:.3g}")
    assert np.all(np.abs(a - b) <= 1e-11 * np.maximum(np.abs(a), np.abs(b)) + 1e-300)


def _probe_fields(frame):
    """The 11 fields of pt_debug_hit_probe (hit, t, point, normal, u, v, index) as the frame holds them; the probe leaves
    zeros in every field of a miss, the frame +inf in t and -1 in the index (include/ptrace.h)."""
    hit = frame.hit.reshape(-1)
    out = np.zeros((hit.size, 11))
    out[:, 0] = hit
    out[:, 1] = np.where(hit, frame.t.reshape(-1), 0.0)
    out[:, 2:5] = frame.point.reshape(-1, 3)
    out[:, 5:8] = frame.normal.reshape(-1, 3)
    out[:, 8:10] = frame.uv.reshape(-1, 2)
    out[:, 10] = np.where(hit, frame.shape_index.reshape(-1), 0)
    return out


@pytest.mark.parametrize("W,H,S", [(1280, 720, 0), (640, 360, 2)])
def test_frame_size_equals_the_unculled_probe_on_its_own_rays(dev, W, H, S):
    flat, cam = flat_of("c2p"), camera_of("c2p", W, H)
    p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=S, pcg_mode=abi.PCG_PIXEL)
    with dev.DeviceScene(flat) as ds:
        frame = ds.render_hits(cam, p, abi.HIT_ALL, pinned=True)
        assert dev.plan_hits(flat, cam, p).main_kernel == "pt_hits_kernel"
        n = frame.shape_index.size
        rays = np.empty((n, 8))
        rays[:, 0:3], rays[:, 3:6] = frame.ray_origin.reshape(-1, 3), frame.ray_dir.reshape(-1, 3)
        rays[:, 6], rays[:, 7] = 1e-5, np.inf
        probe = ds.hit_probe(rays, -1)
    mine = _probe_fields(frame)
    assert 0.3 * n < mine[:, 0].sum() <= n and len(np.unique(frame.shape_index)) > 20
    same = util.bits_equal_rows(mine, probe[:, :11])
    assert same.all(), f"{int((~same).sum())} of {n} samples differ, first at {int(np.argmin(same))}"


def test_culling_is_invisible(dev, tuning):
    for scene, W, H, S, names in (("c2p", 640, 360, 0, ["pt_hits_kernel"]), ("open", 161, 97, 2, ["pt_hits_kernel"]),
                                  ("big", 320, 180, 0, ["pt_cell_kernel", "pt_hits_kernel<HIER>"])):
        flat, cam = flat_of(scene), camera_of(scene, W, H)
        p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=S, pcg_mode=abi.PCG_SAMPLE)
        with dev.DeviceScene(flat) as ds:
            tuning("cull", 1)
            assert dev.plan_hits(flat, cam, p).kernels == names
            culled = ds.render_hits(cam, p, abi.HIT_ALL)
            tuning("cull", 0)
            assert dev.plan_hits(flat, cam, p).kernels == ["pt_hits_kernel<noCULL>"]
            plain = ds.render_hits(cam, p, abi.HIT_ALL)
            tuning("cull", 1)
        assert culled.hit.any()
        for name, a in culled.planes().items():
            b = plain.planes()[name]
            assert a.tobytes() == b.tobytes(), (scene, name)
    # the beam of an orthogonal camera
    flat, cam = flat_of("c2p"), camera_of("c2p", 161, 97, ortho=True)
    p = abi.make_params(161, 97, abi.RENDERER_FLAT, samples_per_side=2)
    with dev.DeviceScene(flat) as ds:
        culled = ds.render_hits(cam, p, abi.HIT_ALL)
        tuning("cull", 0)
        plain = ds.render_hits(cam, p, abi.HIT_ALL)
        tuning("cull", 1)
    assert all(a.tobytes() == plain.planes()[k].tobytes() for k, a in culled.planes().items())


def test_channel_selection_sizes_and_guard(dev):
    import torch

    W, H, S = 161, 97, 2
    flat, cam = flat_of("c2p"), camera_of("c2p", W, H)
    p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=S, pcg_mode=abi.PCG_SEQ)
    with dev.DeviceScene(flat) as ds:
        full = ds.render_hits(cam, p, abi.HIT_ALL).planes()
        for channels in (0, abi.HIT_T, abi.HIT_UV, abi.HIT_NORMAL | abi.HIT_UV, abi.HIT_POINT | abi.HIT_RAY, abi.HIT_T | abi.HIT_NORMAL,
                         abi.HIT_ALL & ~abi.HIT_UV):
            need = abi.hits_bytes(p, channels)
            guard = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
            # one byte short: refused, nothing written
            with pytest.raises(_lib.PtraceError) as e:
                ds.render_hits_into(cam, p, channels, guard.data_ptr(), need - 1, None)
            assert e.value.code == -5  # PT_ERR_SIZE
            assert bool((guard == 0xA5).all())
            ds.render_hits_into(cam, p, channels, guard.data_ptr(), need, None)
            host = guard.cpu().numpy()
            assert np.all(host[need:] == 0xA5), "the kernel wrote beyond pt_hits_bytes"
            part = HitFrame(host[:need], p, channels).planes()
            assert set(part) <= set(full) and len(part) == 1 + sum(1 for b in (1, 2, 4, 8) if channels & b) + 2 * bool(channels & 16)
            for name, a in part.items():
                assert a.tobytes() == full[name].tobytes(), (channels, name)
        with pytest.raises(_lib.PtraceError) as e:
            _lib.check(_lib.lib().pt_render_hits_device(ds._h, C.byref(cam), C.byref(p), 64, C.c_void_p(guard.data_ptr()), guard.numel(), None))
        assert e.value.code == -1  # PT_ERR_INVALID: unknown channel bits


def test_flat_frame_recomputed_from_the_hit_frame(dev, orc):
    """render.py:65-74 in numpy from the planes: pigment(shape_index, uv) + emitted, via oracle.pigment == pt_render's Flat
    frame, bit for bit (checkered pigments on spheres and on the plane; pixel centres and a jittered frame)."""
    world = scenes.synthetic_world(12, with_plane=True)
    for i, shape in enumerate(world.shapes[1:8]):
        shape.material = hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.9, 0.1 * i, 0.2), hm.Color(0.1, 0.3, 0.1 * i), 6 + i)),
                                     hm.CheckeredPigment(hm.Color(0.0, 0.0, 0.5), hm.Color(0.25, 0.0, 0.0), 3) if i % 2 else hm.UniformPigment(hm.BLACK))
    flat = flatten.flatten_world(world)
    W, H = 80, 45
    cam = camera_of("c2p", W, H)
    for S in (0, 2):
        p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=S, pcg_mode=abi.PCG_SEQ, background=(0.125, 0.25, 0.5))
        with dev.DeviceScene(flat) as ds:
            image = ds.render(cam, p)
            frame = ds.render_hits(cam, p, abi.HIT_UV)
        vals = np.empty(frame.shape_index.shape + (3,))
        vals[...] = (0.125, 0.25, 0.5)
        for k, r, c in np.argwhere(frame.hit):
            i, (u, v) = int(frame.shape_index[k, r, c]), frame.uv[k, r, c]
            vals[k, r, c] = orc.pigment(flat, i, False, u, v) + orc.pigment(flat, i, True, u, v)
        if S > 0:  # imagetracer.py:83-101
            cum = np.zeros((H, W, 3))
            for k in range(frame.nsamp):
                cum = cum + vals[k]
            vals = cum * (1 / S ** 2)
        else:
            vals = vals[0]
        assert len(np.unique(image.reshape(-1, 3), axis=0)) > 12
        assert util.bits_equal(image, vals), S


def test_hit_shaders_end_to_end(dev, orc):
    """fire_all_rays(shader) on the device == the image the CPU test builds from the oracle's frame."""
    from pytracer_amd.tracer import GpuImageTracer

    from .test_hits_host import OracleWorld, SeamTracer

    demo, camera = scenes.demo_world()
    world = OracleWorld(demo, orc)
    W, H = 24, 16
    for S in (0, 2):
        for shader in (shaders.NormalShader(world, hm.Color(0.25, 0.5, 0.125)), shaders.DepthShader(world, 1.0, 12.0)):
            gpu = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=S, pcg=hm.PCG(45, 54))
            gpu.fire_all_rays(shader)
            cpu = SeamTracer(hm.HdrImage(W, H), camera, samples_per_side=S, pcg=hm.PCG(45, 54), orc=orc)
            cpu.fire_all_rays(shader)
            assert gpu.last_path == "device-hits" and gpu.last_stats.kernel == abi.KERNEL_HITS
            assert util.bits_equal(gpu.image.array, cpu.image.array), (type(shader).__name__, S)
            assert gpu.pcg.state == cpu.pcg.state
            gpu.close()
    # fire_all_hits: the frame itself, and records for scalar shading
    t = GpuImageTracer(hm.HdrImage(W, H), camera, samples_per_side=2, pcg=hm.PCG(45, 54))
    frame = t.fire_all_hits(demo, "normal,t,uv")
    assert frame.channels == abi.HIT_NORMAL | abi.HIT_T | abi.HIT_UV and t.pcg.state == cpu.pcg.state
    rec = frame.record(12, 15, 3)
    ref = SeamTracer(hm.HdrImage(W, H), camera, samples_per_side=2, pcg=hm.PCG(45, 54), orc=orc)._render_hit_frame(world, abi.HIT_ALL)
    want = ref.record(12, 15, 3)
    assert rec is not None and rec.shape_index == want.shape_index and rec.t == want.t and rec.normal == want.normal and rec.ray is None
    assert shaders.NormalShader(world).shade_record(rec) == shaders.NormalShader(world).shade_record(want)
    t.close()


def test_hits_command_writes_the_frame_without_torch(dev, tmp_path):
    W, H = 96, 40
    out = str(tmp_path / "frame.npz")
    code = ("import sys; sys.modules['torch'] = None\n"
            "from pytracer_amd.cli import cli\n"
            "try:\n"
            "    cli(sys.argv[1:], standalone_mode=False)\n"
            "finally:\n"
            "    maps = open('/proc/self/maps').read()\n"
            "    assert 'libptrace.so' in maps and 'site-packages/torch' not in maps and 'libtorch' not in maps\n"
            "    print('no torch in this process')\n")
    args = ["hits", "--width", str(W), "--height", str(H), "--channels", "normal,t,uv", "--samples-per-pixel", "4", "--output", out, "builtin:c2"]
    r = subprocess.run([sys.executable, "-c", code] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "no torch in this process" in r.stdout, r.stdout + r.stderr
    got = np.load(out)
    flat, cam = flat_of("c2p"), camera_of("c2p", W, H)
    p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=2, pcg_mode=abi.PCG_SEQ, jitter_state=42, jitter_seq=54)
    with dev.DeviceScene(flat) as ds:
        want = ds.render_hits(cam, p, "normal,t,uv").planes()
    assert sorted(got.files) == sorted(want) == ["normal", "shape_index", "t", "uv"]
    for name in want:
        assert got[name].shape == want[name].shape and got[name].tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
    # a bad channel name is a usage error before any GPU work
    from click.testing import CliRunner

    from pytracer_amd.cli import cli

    r = CliRunner().invoke(cli, ["hits", "--channels", "colour", "builtin:c2"])
    assert r.exit_code == 2 and "colour" in r.output


def test_two_clones_on_two_streams_download_complete_frames(dev):
    """Two handles of one scene render hit frames concurrently on two streams; DeviceBuffer.numpy() with no stream given
    orders its copy behind the stream the buffer was rendered on, so the frames are complete without an explicit wait."""
    from pytracer_amd.devmem import DeviceBuffer, Stream

    W, H = 1280, 720
    flat, cam = flat_of("c2p"), camera_of("c2p", W, H)
    ps = [abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=0), abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=1, pcg_mode=abi.PCG_SAMPLE)]
    with dev.DeviceScene(flat) as a:
        want = [a.render_hits(cam, p, abi.HIT_ALL) for p in ps]
        b = a.clone()
        streams = [Stream(), Stream()]
        bufs = [DeviceBuffer((abi.hits_bytes(p, abi.HIT_ALL),), np.uint8) for p in ps]
        for _ in range(3):  # (several frames deep: the last one is still in flight when numpy() is called)
            for ds, p, buf, st in zip((a, b), ps, bufs, streams):
                ds.render_hits_into(cam, p, abi.HIT_ALL, buf, stream=st)
        got = [HitFrame(buf.numpy(), p, abi.HIT_ALL) for buf, p in zip(bufs, ps)]
        for g, w in zip(got, want):
            for name, plane in w.planes().items():
                assert g.planes()[name].tobytes() == plane.tobytes(), name
        assert not np.array_equal(got[0].ray_dir, got[1].ray_dir)
        for st in streams:
            st.synchronize()
        for buf in bufs:
            buf.free()
        b.close()
        for st in streams:
            st.close()
