"""The scene families (tests/scene_families.py) do what they claim: checked on the oracle and on the host-side planner
(``pt_debug_plan``), without a GPU, for every seed tests/test_gpu_families.py renders.

These are conditions, not measurements: a family that misses one gets other generator constants, not another threshold.
A "dome" here is a sphere that contains the origin of the central pixel's ray.
"""
import functools
import os

import numpy as np
import pytest

from pytracer_amd import abi, flatten
from tests import scene_families as sf
from tests import util

SEEDS = range(int(os.environ.get("PT_FAMILY_SEEDS", "6")))
OFF_DIAGONAL = [1, 2, 4, 6, 8, 9]
CULLING = ("pt_tile_kernel", "pt_tile4_kernel", "pt_path_regions_kernel", "pt_path_tree_kernel")


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    yield oracle
    oracle.set_sqr_mode(oracle.SQR_POW)


def frames_of(seed):
    """(renderer, keywords) of every frame tests/test_gpu_families.py renders of a seed's scene."""
    path = dict(samples_per_side=2, path_state=45 + seed, path_seq=54, **sf.path_params(seed))
    return [(abi.RENDERER_ONOFF, {}), (abi.RENDERER_FLAT, {}), (abi.RENDERER_FLAT, dict(samples_per_side=2)),
            (abi.RENDERER_POINTLIGHT, {}), (abi.RENDERER_PATHTRACER, dict(path, pcg_mode=abi.PCG_PIXEL)),
            (abi.RENDERER_PATHTRACER, dict(path, pcg_mode=abi.PCG_SAMPLE))]


@functools.lru_cache(maxsize=None)
def flat_of(family, seed):
    world, camera, W, H = sf.family_world(family, seed)
    return flatten.flatten_world(world), flatten.flatten_camera(camera), W, H


_frames = {}


def primary(orc, family, seed):
    """The oracle's hit-record frame of the pixel centres, and which shapes are domes."""
    key = (family, seed)
    if key not in _frames:
        flat, cam, W, H = flat_of(family, seed)
        frame = util.oracle_frame(orc, flat, cam, abi.make_params(W, H, abi.RENDERER_FLAT))
        o = frame.ray_origin[0, H // 2, W // 2]
        dome = np.zeros(flat.n_shapes, bool)
        for i in np.flatnonzero(flat.kind == abi.SHAPE_SPHERE):
            m = flat.invm[:, i].reshape(3, 4)
            q = m[:, :3] @ o + m[:, 3]
            dome[i] = q @ q < 1.0
        _frames[key] = (frame, dome)
    return _frames[key]


def determinants(flat):
    return np.array([np.linalg.det(flat.m[:, i].reshape(3, 4)[:, :3]) for i in range(flat.n_shapes)])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("family", sf.FAMILIES)
def test_frames_are_not_vacuous_and_culling_is_in_play(orc, family, seed):
    from pytracer_amd import device

    flat, cam, W, H = flat_of(family, seed)
    assert W <= 128 and H <= 104 and (W % 8 or H % 8) and 24 <= flat.n_shapes <= 64
    assert np.all(np.isfinite(flat.m)) and np.all(np.isfinite(flat.invm)) and np.all(np.abs(determinants(flat)) > 1e-9)
    frame, dome = primary(orc, family, seed)
    idx = frame.shape_index[0]
    hit = idx >= 0
    beyond_dome = hit & ~dome[np.where(hit, idx, 0)]
    winners = np.unique(idx[hit])
    print(f"{family} seed {seed}: {W}x{H}, {flat.n_shapes} shapes, {flat.n_lights} lights, {beyond_dome.mean():.2f} of the rays hit a "
          f"shape that is no dome, {len(winners)} shapes win a pixel")
    assert beyond_dome.mean() >= 0.25
    assert len(winners) >= 8
    for renderer, kw in frames_of(seed):
        info = device.plan(flat, cam, abi.make_params(W, H, renderer, **kw))
        assert any(name.startswith(CULLING) for name in info.kernels), (renderer, info.kernels)


@pytest.mark.parametrize("seed", SEEDS)
def test_mirrored_shapes_win_pixels_on_the_diag_path_too(orc, seed):
    from pytracer_amd import device

    flat, cam, W, H = flat_of("mirrored", seed)
    frame, _ = primary(orc, "mirrored", seed)
    winners = np.unique(frame.shape_index[0][frame.shape_index[0] >= 0])
    det = determinants(flat)
    is_diag = (flat.kind == abi.SHAPE_SPHERE) & ~np.any(flat.invm[OFF_DIAGONAL, :] != 0.0, axis=0)
    info = device.plan(flat, cam, abi.make_params(W, H, abi.RENDERER_FLAT))
    assert info.n_diag == int(is_diag.sum()), "the library's scale+translate records are not the spheres with a diagonal invm"
    flipped = [i for i in winners if det[i] < 0]
    flipped_diag = [i for i in flipped if is_diag[i]]
    assert all(min(flat.invm[k, i] for k in (0, 5, 10)) < 0 for i in flipped_diag)
    planes = [i for i in flipped if flat.kind[i] == abi.SHAPE_PLANE]
    print(f"mirrored seed {seed}: {len(flipped)} shapes of negative determinant win pixels, {len(flipped_diag)} of them diag records, "
          f"{len(planes)} planes")
    assert len(flipped) >= 5 and len(flipped_diag) >= 2


def test_sheared_shapes_are_not_orthogonal(orc):
    for seed in SEEDS:
        flat = flat_of("sheared", seed)[0]
        worst = 0.0
        for i in range(flat.n_shapes):
            sv = np.linalg.svd(flat.m[:, i].reshape(3, 4)[:, :3], compute_uv=False)
            worst = max(worst, sv[0] / sv[-1])
        a = flat.m.reshape(3, 4, -1)[:, :3, :]
        gram_off = max(abs(float(a[:, 0, i] @ a[:, 1, i])) / np.sqrt(float(a[:, 0, i] @ a[:, 0, i]) * float(a[:, 1, i] @ a[:, 1, i]))
                       for i in range(flat.n_shapes))
        assert 5.0 < worst <= 50.0 and gram_off > 0.3, (seed, worst, gram_off)


def test_every_texture_is_sampled_and_the_clamped_texel_taken(orc):
    clamped = 0
    for seed in SEEDS:
        flat, cam, W, H = flat_of("pigments", seed)
        assert sorted(zip(flat.tex_w.tolist(), flat.tex_h.tolist())) == sorted(sf.TEXTURE_SIZES)
        assert np.all(flat.pig_kind != abi.PIGMENT_UNIFORM) and 0.3 < np.mean(flat.emi_kind != abi.PIGMENT_UNIFORM) < 0.7
        steps = np.concatenate([flat.pig_steps[flat.pig_kind == abi.PIGMENT_CHECKERED], flat.emi_steps[flat.emi_kind == abi.PIGMENT_CHECKERED]])
        assert steps.min() >= 1 and steps.max() <= 200
        frame, _ = primary(orc, "pigments", seed)
        idx, uv = frame.shape_index[0], frame.uv[0]
        sampled = set()
        for kind, tex in ((flat.pig_kind, flat.pig_tex), (flat.emi_kind, flat.emi_tex)):
            for r, c in np.argwhere(idx >= 0):
                i = idx[r, c]
                if kind[i] == abi.PIGMENT_IMAGE:
                    t = int(tex[i])
                    sampled.add(t)
                    u, v = uv[r, c]
                    clamped += int(u * flat.tex_w[t]) >= flat.tex_w[t] or int(v * flat.tex_h[t]) >= flat.tex_h[t]
        assert sampled == set(range(flat.n_textures)), (seed, sampled)
    print(f"pigments: the clamped last column or row is the texel of {clamped} samples")
    assert clamped >= 1
    assert max(flat_of("pigments", s)[0].pig_steps.max() for s in SEEDS) > 50


def test_camera_family_reaches_the_extreme_screen_distances():
    cams = [flat_of("camera", seed)[1:] for seed in SEEDS]
    persp = [c for c, _, _ in cams if c.kind == abi.CAMERA_PERSPECTIVE]
    assert sum(c.screen_distance <= 0.05 for c in persp) >= 2 and sum(c.screen_distance >= 20.0 for c in persp) >= 2
    aspects = [W / H for _, W, H in cams]
    assert min(aspects) <= 1 / 8 and max(aspects) >= 8
    mirrored = mirrored_ortho = 0
    for c, _, _ in cams:
        m = np.array(list(c.m)).reshape(3, 4)[:, :3]
        sv = np.linalg.svd(m, compute_uv=False)
        assert 0.19 <= sv[-1] and sv[0] <= 5.01 and np.abs(sv - 1.0).max() > 0.1  # (factors of 0.2 to 5, not rigid)
        mirrored += np.linalg.det(m) < 0
        mirrored_ortho += c.kind == abi.CAMERA_ORTHOGONAL and np.linalg.det(m) < 0
    assert mirrored >= 2 and mirrored_ortho >= 1


def test_cameras_sit_inside_small_spheres(orc):
    small = 0
    for seed in SEEDS:
        flat = flat_of("camera", seed)[0]
        _, dome = primary(orc, "camera", seed)
        for i in np.flatnonzero(dome):
            small += np.linalg.svd(flat.m[:, i].reshape(3, 4)[:, :3], compute_uv=False)[0] < 5.0
    assert small >= 2


def test_shadow_rays_are_blocked_and_not_in_frames_of_many_lights(orc):
    blocked = free = frames = 0
    placed = set()
    for seed in SEEDS:
        flat, cam, W, H = flat_of("lights", seed)
        assert 0 <= flat.n_lights <= 6
        if flat.n_lights < 3:
            continue
        frames += 1
        frame, _ = primary(orc, "lights", seed)
        for r, c in np.argwhere(frame.shape_index[0] >= 0)[::7]:
            for l in range(flat.n_lights):
                seen = orc.is_point_visible(flat, flat.light_pos[:, l], frame.point[0, r, c])
                free += seen
                blocked += not seen
        placed |= {"far" if np.abs(flat.light_pos[:, l]).max() > 500 else "near" for l in range(flat.n_lights)}
        placed |= {"radius" if flat.light_radius[l] > 0 else "no radius" for l in range(flat.n_lights)}
    counts = [flat_of("lights", seed)[0].n_lights for seed in SEEDS]
    print(f"lights: {counts} lights a seed; {blocked} shadow rays blocked, {free} not, in {frames} frames of 3 or more lights")
    assert frames >= 1 and blocked > 100 and free > 100
    assert placed == {"far", "near", "radius", "no radius"}
    thresholds = np.concatenate([flat_of("lights", s)[0].brdf_param[flat_of("lights", s)[0].brdf_kind == abi.BRDF_SPECULAR] for s in SEEDS])
    assert thresholds.min() == 0.0 and thresholds.max() >= 3.0


def test_the_families_cover_the_kernels_they_are_meant_to():
    """16x16 tiles, the orthogonal camera's tile kernel, and a second pass with several rays per hit."""
    from pytracer_amd import device

    names = set()
    for family in sf.FAMILIES:
        for seed in SEEDS:
            flat, cam, W, H = flat_of(family, seed)
            for renderer, kw in frames_of(seed):
                par = abi.make_params(W, H, renderer, **kw)
                info = device.plan(flat, cam, par)
                names |= set(info.kernels)
                if renderer == abi.RENDERER_PATHTRACER and par.num_of_rays > 1:
                    names.add("second pass, N > 1: " + info.main_kernel.split("<")[0])
    print(sorted(names))
    assert any(n.startswith("pt_tile4_kernel<FLAT") for n in names) and any(n.startswith("pt_tile4_kernel<ONOFF") for n in names)
    assert {"pt_tile_kernel<FLAT, ORTHO>", "pt_tile_kernel<POINTLIGHT, ORTHO>", "pt_tile_kernel<PATHTRACER, ORTHO>"} <= names
    assert "second pass, N > 1: pt_path_tree_kernel" in names
    assert any(n.startswith("pt_path_regions_kernel") for n in names)


def test_the_recipe_is_deterministic():
    for family in sf.FAMILIES:
        a = flatten.flatten_world(sf.family_world(family, 2)[0])
        b = flatten.flatten_world(sf.family_world(family, 2)[0])
        assert a.same_bits(b) and not a.same_bits(flat_of(family, 3)[0])
