"""The scene families of tests/scene_families.py on the device (run with ``-m gpu``): mirrored and sheared shapes, scaled and
mirrored cameras at screen distances of 0.02 to 50, patterned pigments on every shape, many lights.

* Frames against the oracle's ``x*x`` mode under the bars of ``test_random_scenes_match_oracle`` (tests/test_gpu_parity.py):
  bit-identical frames and equal ray counts where no libm function is involved, else 1e-5 relative per channel, with at
  most one outlier pixel for the path tracer.
* Where the oracle cannot demand bits (patterned spheres go through atan2 / acos) the device is held to itself: every frame
  must be byte-equal with culling on and off, with the dome shortcut on and off, and rendered whole or as three ranks' shares
  of 8-row blocks reassembled.  A sphere culled wrongly under a scaled camera, or lost to the diag path, fails there exactly.
* Hit-record frames against ``util.oracle_frame``: index, t, point, normal, ray and a plane's (u, v) bit-identical, a
  sphere's (u, v) within 1e-11 (tests/test_gpu_probes.py), no sample excluded.
* Texel and checker boundaries by construction: dyadic pixel centres over a textured plane, rays at a sphere's seam and poles.

``PT_FAMILY_SEEDS`` (default 6) seeds a family; tests/test_scene_families.py checks on the CPU that these very frames are not
vacuous.
"""
import os

import numpy as np
import pytest

from pytracer_amd import abi, flatten
from pytracer_amd import hostmodel as hm
from tests import scene_families as sf
from tests import util
from tests.test_gpu_parity import TOL, _uses_libm
from tests.test_scene_families import CULLING, flat_of, frames_of

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("PT_FAMILY_SEEDS", "6")))
UV_TOL = 1e-11  # (tests/test_gpu_probes.py:65, tests/test_gpu_hits.py)


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


@pytest.fixture()
def mul_oracle(oracle):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    yield oracle
    oracle.set_sqr_mode(oracle.SQR_POW)


def _whole_from_shares(ds, cam, par):
    out = np.empty((par.height, par.width, 3), dtype=np.float64)
    for rank in range(3):
        share = abi.copy_params(par, row_block=8, n_ranks=3, rank=rank)
        rows = abi.rows_for_rank(par.height, 8, 3, rank)
        if not rows:  # (a frame of fewer than 17 rows has no third block)
            continue
        part = ds.render(cam, share)
        assert part.shape[0] == len(rows)
        out[rows] = part
    return out


def check_scene(dev, oracle, tag, flat, cam, W, H, frames):
    """One DeviceScene: every frame against the oracle, then against the device's own unculled, shortcut-free and partitioned
    renderings."""
    assert dev.get_tuning("cull") == 1
    with dev.DeviceScene(flat) as ds:
        for renderer, kw in frames:
            par = abi.make_params(W, H, renderer, **kw)
            info = dev.plan(flat, cam, par, n_cu=dev.device_info(0)[0])
            assert any(name.startswith(CULLING) for name in info.kernels), (tag, renderer, info.kernels)
            ora, n_rays = oracle.render(flat, cam, par, sqr_mode=oracle.SQR_MUL)
            out = ds.render(cam, par)
            n_dev = int(ds.stats().n_rays)
            err = util.rel_err(out, ora)
            bad = int((err > TOL).any(axis=-1).sum())
            libm = _uses_libm(flat, par)
            print(f"[families] {tag} renderer {renderer} S={par.samples_per_side} N={par.num_of_rays} mode={par.pcg_mode} {'+'.join(info.kernels)}: "
                  f"{'libm' if libm else 'bits'}, max rel {err.max():.3e}, outliers {bad}/{W * H}, rays {n_dev} vs {n_rays}")
            if renderer == abi.RENDERER_PATHTRACER:
                assert bad <= 1, f"{tag}: {bad} pixels off, max rel {err.max():.3e}"
            elif libm:
                assert np.all(err <= TOL), f"{tag} renderer {renderer}: {bad} pixels beyond {TOL}, max rel {err.max():.3e}"
            else:
                assert util.bits_equal(out, ora), f"{tag} renderer {renderer} S={par.samples_per_side}: max rel {err.max()}"
                assert n_dev == n_rays
            # the device against itself: byte for byte
            dev.set_tuning("cull", 0)
            try:
                assert not any(name.startswith(CULLING) for name in dev.plan(flat, cam, par).kernels)
                plain = ds.render(cam, par)
            finally:
                dev.set_tuning("cull", 1)
            assert out.tobytes() == plain.tobytes(), \
                f"{tag} renderer {renderer}: culling changes {int((out != plain).any(axis=-1).sum())} pixels"
            ds.set_dome_shortcut(False)
            try:
                every_ray = ds.render(cam, par)
            finally:
                ds.set_dome_shortcut(True)
            assert out.tobytes() == every_ray.tobytes(), \
                f"{tag} renderer {renderer}: the dome shortcut changes {int((out != every_ray).any(axis=-1).sum())} pixels"
            shares = _whole_from_shares(ds, cam, par)
            assert out.tobytes() == shares.tobytes(), \
                f"{tag} renderer {renderer}: the 3-rank partition changes {int((out != shares).any(axis=-1).sum())} pixels"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("family", sf.FAMILIES)
def test_family_frames_match_the_oracle_and_the_device_itself(dev, mul_oracle, family, seed):
    flat, cam, W, H = flat_of(family, seed)
    check_scene(dev, mul_oracle, f"{family}-{seed}", flat, cam, W, H, frames_of(seed))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("family", sf.HIT_FAMILIES)
def test_family_hit_frames_equal_the_oracle(dev, mul_oracle, family, seed):
    flat, cam, W, H = flat_of(family, seed)
    S, mode = (0, abi.PCG_PIXEL) if seed % 3 == 0 else (2, abi.PCG_PIXEL if seed % 2 else abi.PCG_SAMPLE)
    p = abi.make_params(W, H, abi.RENDERER_FLAT, samples_per_side=S, pcg_mode=mode, path_state=1234 + seed, path_seq=77)
    names = dev.plan_hits(flat, cam, p).kernels
    assert names and names[-1].startswith("pt_hits_kernel") and "noCULL" not in names[-1], names
    with dev.DeviceScene(flat) as ds:
        got = ds.render_hits(cam, p, abi.HIT_ALL)
    exp = util.oracle_frame(mul_oracle, flat, cam, p)
    bits = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))  # noqa: E731
    assert np.array_equal(got.shape_index, exp.shape_index), \
        f"hit / miss or the winning shape differs on {int((got.shape_index != exp.shape_index).sum())} samples"
    hit = exp.hit
    assert hit.mean() > 0.25
    assert bits(got.ray_origin, exp.ray_origin) and bits(got.ray_dir, exp.ray_dir)
    assert bits(got.t, exp.t) and bits(got.point, exp.point) and bits(got.normal, exp.normal)
    plane = hit & (flat.kind[np.where(hit, exp.shape_index, 0)] == abi.SHAPE_PLANE)
    assert bits(got.uv[plane], exp.uv[plane]) and bits(got.uv[~hit], exp.uv[~hit])
    a, b = got.uv[hit & ~plane], exp.uv[hit & ~plane]
    err = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    print(f"[families] hits {family}-{seed} S={S} {names}: {int(hit.sum())} hits of {hit.size}, {int(plane.sum())} on planes, "
          f"sphere uv max rel err {err.max() if err.size else 0:.3g}")
    assert np.all(np.abs(a - b) <= UV_TOL * np.maximum(np.abs(a), np.abs(b)) + 1e-300)


# ---- texel and checker edges by construction ---------------------------------------------------------------------------------
def _exact(m3, t3):
    """A Transformation from an exact 3x3 block of 0 / +-1 / powers of two and a translation (no sin / cos anywhere)."""
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = m3, t3
    inv = np.eye(4)
    inv[:3, :3] = np.linalg.inv(np.array(m3, dtype=np.float64))
    inv[:3, 3] = -inv[:3, :3] @ np.array(t3, dtype=np.float64)
    assert np.array_equal(inv @ m, np.eye(4))
    return hm.Transformation(m.tolist(), inv.tolist())


def _texture(w, h):
    img = hm.HdrImage(w, h)
    img.pixels = [hm.Color(*c) for c in sf.texture_pixels(w, h, 3)]
    return img


@pytest.mark.parametrize("mirror", [1.0, -1.0], ids=["plain", "mirrored"])
@pytest.mark.parametrize("tex", [(1, 1), (1, 8), (8, 1), (4, 2)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_pixel_centres_on_texel_and_checker_boundaries(dev, mul_oracle, tex, mirror):
    """An orthogonal camera straight above a plane, 16 x 16 pixels whose centres are odd multiples of 1/8: with the plane
    scaled by 1/2 (and shifted by 1/8, 3/8 in the second world) every hp.x, hp.y is an exact odd multiple of 1/4 (a multiple
    of 1/2), so u * w, v * h and u * steps are exact integers on many pixels: texel and checker boundaries, decided by floor
    alone."""
    W = H = 16
    on_texels = on_checkers = 0
    colours = set()
    # camera x -> world -z, y -> y, z -> x, both screen axes doubled; 5 above the plane
    camera = hm.OrthogonalCamera(1.0, _exact([[0.0, 0.0, 2.0], [0.0, 2.0, 0.0], [-1.0, 0.0, 0.0]], [0.0, 0.0, 4.0]))
    cam = flatten.flatten_camera(camera)
    for shift in ((0.0, 0.0), (0.125, 0.375)):
        for steps in (1, 2, 200):
            world = hm.World()
            world.add_shape(hm.Plane(hm.translation(hm.Vec(shift[0], shift[1], 0.0)) * hm.scaling(hm.Vec(0.5 * mirror, 0.5, 1.0)),
                                     hm.Material(hm.DiffuseBRDF(hm.ImagePigment(_texture(*tex))),
                                                 hm.CheckeredPigment(hm.Color(0.25, 0.0, 0.5), hm.Color(0.0, 0.125, 0.0), steps))))
            for k in range(4):  # (small spheres beside the view: four shapes and more get the tile kernels)
                world.add_shape(hm.Sphere(hm.translation(hm.Vec(3.0 + k, 3.0, 1.0)) * hm.scaling(hm.Vec(0.25, 0.25, 0.25))))
            world.add_light(hm.PointLight(hm.Vec(0.5, -0.25, 3.0), hm.Color(1.0, 0.5, 0.25), 0.0))
            world.add_light(hm.PointLight(hm.Vec(-1.0, 1.0, 2.0), hm.Color(0.5, 0.5, 1.0), 2.0))
            flat = flatten.flatten_world(world)
            frame = util.oracle_frame(mul_oracle, flat, cam, abi.make_params(W, H, abi.RENDERER_FLAT))
            u, v = frame.uv[0, ..., 0], frame.uv[0, ..., 1]
            assert np.all(frame.shape_index == 0) and np.all(u * 4 == np.floor(u * 4)) and np.all(v * 4 == np.floor(v * 4))
            on_texel = (u * tex[0] == np.floor(u * tex[0])) & (v * tex[1] == np.floor(v * tex[1]))
            on_checker = (u * steps == np.floor(u * steps)) | (v * steps == np.floor(v * steps))
            on_texels += int(on_texel.sum())
            on_checkers += int(on_checker.sum())
            with dev.DeviceScene(flat) as ds:
                for renderer in (abi.RENDERER_FLAT, abi.RENDERER_POINTLIGHT):
                    par = abi.make_params(W, H, renderer, background=(0.5, 0.25, 0.125))
                    assert dev.plan(flat, cam, par).main_kernel.startswith("pt_tile_kernel") and "ORTHO" in dev.plan(flat, cam, par).main_kernel
                    assert not _uses_libm(flat, par)
                    ora, n_rays = mul_oracle.render(flat, cam, par, sqr_mode=mul_oracle.SQR_MUL)
                    out = ds.render(cam, par)
                    colours |= {tuple(c) for c in np.unique(ora.reshape(-1, 3), axis=0).tolist()}
                    assert util.bits_equal(out, ora), (tex, mirror, shift, steps, renderer, int((out != ora).any(axis=-1).sum()))
                    assert int(ds.stats().n_rays) == n_rays

    assert on_texels >= W * H // 4 * 3 and on_checkers >= W * H // 4 and len(colours) >= 4, (on_texels, on_checkers, len(colours))


def test_rays_at_the_seam_and_the_poles_of_a_textured_sphere(dev, mul_oracle):
    """u = uu + 1.0 == 1.0 for a tiny negative atan2, v == 1.0 at the south pole: (u, v) stays inside [0, 1], the texel is
    the clamped last column / row, and the Flat colour of a 1 x 1 frame whose only ray is that ray is the oracle's pigment
    at the device's own (u, v)."""
    rays = {  # name: (origin, direction), expected (u, v) of the reference's formulas
        "seam, y = -0.0": ((3.0, -0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.5)),
        "seam, y tiny negative": ((3.0, -1e-20, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.5)),
        "seam, y tiny positive": ((3.0, 1e-20, 0.0), (-1.0, 0.0, 0.0), None),  # (u = 1.6e-21)
        "far side, x < 0, y = +0.0": ((-3.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 0.5)),
        "far side, x < 0, y = -0.0": ((-3.0, -0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 0.5)),
        "north pole": ((0.0, 0.0, 3.0), (0.0, 0.0, -1.0), (0.0, 0.0)),
        "south pole": ((0.0, 0.0, -3.0), (0.0, 0.0, 1.0), (0.0, 1.0)),
    }
    for mirror in (1.0, -1.0):
        for tw, th in ((5, 3), (1, 1), (64, 64)):
            world = hm.World()
            world.add_shape(hm.Sphere(hm.scaling(hm.Vec(1.0, mirror, 1.0)),
                                      hm.Material(hm.DiffuseBRDF(hm.ImagePigment(_texture(tw, th))),
                                                  hm.CheckeredPigment(hm.Color(0.25, 0.0, 0.5), hm.Color(0.0, 0.125, 0.0), 7))))
            flat = flatten.flatten_world(world)
            with dev.DeviceScene(flat) as ds:
                for name, (o, d, want) in rays.items():
                    o = (o[0], o[1] * mirror, o[2])  # (object-space y keeps its sign under the mirror)
                    # an orthogonal camera whose central (only) ray is this one: M * (-1, 0, 0) = o, M * (1, 0, 0) = d
                    others = [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]] if d[0] else [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]
                    m3 = [[d[k]] + others[k] for k in range(3)]
                    cam = flatten.flatten_camera(hm.OrthogonalCamera(1.0, _exact(m3, [o[k] + d[k] for k in range(3)])))
                    par = abi.make_params(1, 1, abi.RENDERER_FLAT)
                    assert dev.plan(flat, cam, par).main_kernel.startswith("pt_simple_kernel<FLAT")
                    ray = np.array(list(o) + list(d) + [1e-5, np.inf])
                    assert np.array_equal(dev.camera_probe(cam, 1, 1, [[0, 0, 0.5, 0.5]])[0, :6], ray[:6]), name
                    rec = ds.hit_probe(ray[None, :], 0)[0]
                    u, v = rec[8], rec[9]
                    exp = mul_oracle.world_intersect(flat, ray)
                    print(f"[families] {name} mirror {mirror:+.0f} {tw}x{th}: device (u, v) = ({u!r}, {v!r}), oracle ({exp[7]!r}, {exp[8]!r})")
                    assert rec[0] == 1.0 and 0.0 <= u <= 1.0 and 0.0 <= v <= 1.0
                    if want is not None:  # (atan2 / acos at +-0, +-1 and an angle far below one ulp of 1: exact values)
                        assert (u, v) == want == (exp[7], exp[8]), name
                    assert abs(u - exp[7]) <= UV_TOL * abs(exp[7]) and abs(v - exp[8]) <= UV_TOL * abs(exp[8]), name
                    pixel = ds.render(cam, par)[0, 0]
                    colour = mul_oracle.pigment(flat, 0, False, u, v) + mul_oracle.pigment(flat, 0, True, u, v)
                    assert util.bits_equal(pixel, colour), name
                    col, row = min(int(u * tw), tw - 1), min(int(v * th), th - 1)
                    texel = flat.tex_data[3 * (row * tw + col): 3 * (row * tw + col) + 3]
                    assert util.bits_equal(mul_oracle.pigment(flat, 0, False, u, v), texel), name
