"""The plane-heavy worlds (tests/plane_worlds.py) plan the kernels they were chosen for and give them real work: checked on
the host-side planner (``pt_debug_plan`` / ``pt_debug_plan_hits``) and on the oracle's hit-record frames, without a GPU, for
every case tests/test_gpu_plane_worlds.py renders.

The conditions on the worlds are conditions, not measurements: a world that misses one gets other generator constants.
"""
import functools

import numpy as np
import pytest

from pytracer_amd import abi, flatten
from tests import plane_worlds as pw
from tests import util


@pytest.fixture(autouse=True)
def default_switches():
    """Every switch of the planner's table at its default from the header for the test, then the values it had: the table is
    process-wide, and whatever the environment or an earlier test left in it must not reach a case (tests/variant_catalog.py)."""
    from pytracer_amd import device
    from tests import variant_catalog as vc

    defaults = vc.tuning_defaults()
    saved = {name: device.get_tuning(name) for name in defaults}
    try:
        for name, value in defaults.items():
            device.set_tuning(name, value)
        yield
    finally:
        for name, value in saved.items():
            device.set_tuning(name, value)


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    yield oracle
    oracle.set_sqr_mode(oracle.SQR_POW)


@functools.lru_cache(maxsize=None)
def flat_of(case_id):
    """-> (FlatScene, info) of a case, or of the constructed world ("coincident", "coincident-plain")."""
    if case_id.startswith("coincident"):
        world, info = pw.constructed_world(plain=case_id.endswith("plain"))
    else:
        world, info = pw.case_world(pw.BY_ID[case_id])
    return flatten.flatten_world(world), info


@functools.lru_cache(maxsize=None)
def cams_of(case_id, size):
    """-> {"perspective": Camera, "orthogonal": Camera}"""
    pair = pw.constructed_cameras(size) if case_id.startswith("coincident") else pw.case_cameras(pw.BY_ID[case_id], size)
    return dict(zip(("perspective", "orthogonal"), (flatten.flatten_camera(c) for c in pair)))


def frame_of(case, frame, **more):
    """-> (Camera, Params) of one of a case's frames."""
    par = pw.frame_params(frame, case.size, **more)
    return cams_of(case.id, (par.width, par.height))[pw.FRAMES[frame][0]], par


_primary = {}


def primary(orc, case_id, size, camera="perspective"):
    """The oracle's hit-record frame of the pixel centres."""
    key = (case_id, size, camera)
    if key not in _primary:
        _primary[key] = util.oracle_frame(orc, flat_of(case_id)[0], cams_of(case_id, size)[camera], abi.make_params(size[0], size[1], abi.RENDERER_FLAT))
    return _primary[key]


def slot_of_planes(flat):
    """The slot of each plane in the library's tables: [scale+translate spheres | other spheres | planes], each in list order."""
    planes = np.flatnonzero(flat.kind == abi.SHAPE_PLANE)
    return planes, int((flat.kind == abi.SHAPE_SPHERE).sum()) + np.arange(len(planes))


def names(info):
    return (info.pre_kernel, info.first_kernel, info.main_kernel, info.alt_kernel)


# ---- the plan -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pw.CASES, ids=lambda c: c.id)
def test_case_plans_the_kernels_it_lists(case):
    from pytracer_amd import device

    flat, info = flat_of(case.id)
    assert flat.n_shapes == case.n_shapes
    assert int((flat.kind == abi.SHAPE_PLANE).sum()) == case.n_planes
    assert flat.n_lights == case.n_lights
    W, H = case.size
    assert 40 <= W <= 104
    assert 24 <= H <= 60
    assert W % 8
    assert H % 8
    assert ("cli" in case.kernels) == (case.n_shapes <= pw.CLI_MAX_SHAPES)
    for frame in pw.frames_of(case):
        cam, par = frame_of(case, frame)
        plan = device.plan(flat, cam, par)
        assert names(plan) == case.kernels[frame], (case.id, frame)
        assert (plan.n_spheres, plan.ball_levels, plan.has_grid) == (case.n_spheres, case.ball_levels, case.has_grid), (case.id, frame)
        assert plan.n_diag == (case.n_spheres + 2) // 3 + (case.n_spheres + 1) // 3  # (two thirds are scale+translate only)
    cam, par = frame_of(case, "flat-s2")
    assert names(device.plan_hits(flat, cam, par)) == case.kernels["hits"]
    # planes are not last in the list, so a record's index is not its slot
    if case.n_spheres and case.n_planes:
        assert max(info["sphere_at"]) > min(info["plane_at"])


def test_the_cases_cover_every_kind_of_kernel_with_planes_present():
    got = {n for c in pw.CASES for k in c.kernels.values() for n in k if n}
    print(sorted(got))
    for r in ("ONOFF", "FLAT", "POINTLIGHT"):  # (pixel-centre OnOff frames of 4 .. 256 shapes take the 16x16 tiles: no plain 8x8 form here)
        assert {f"pt_simple_kernel<{r}, HOIST>", f"pt_tile_kernel<{r}, HIER>"} <= got
        assert (r == "ONOFF" or f"pt_tile_kernel<{r}>" in got)
    assert {"pt_simple_kernel<FLAT, noHOIST>", "pt_tile_kernel<FLAT, ORTHO>", "pt_tile_kernel<POINTLIGHT, ORTHO>",
            "pt_tile4_kernel<FLAT, LDS>", "pt_tile4_kernel<FLAT, noLDS>", "pt_tile4_kernel<ONOFF, noLDS>", "pt_cell_kernel",
            "pt_tile_kernel<PATHTRACER>", "pt_tile_kernel<PATHTRACER, BLOCKS>", "pt_tile_kernel<PATHTRACER, HIER>",
            "pt_tile_kernel<PATHTRACER, ORTHO>", "pt_path_regions_kernel<LDS, SCENE, LEAN>", "pt_path_regions_kernel<LDS, NOGRID>",
            "pt_path_regions_kernel<LDS>", "pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>",
            "pt_hits_kernel", "pt_hits_kernel<HIER>", "pt_hits_kernel<noCULL>"} <= got
    # the pairs the issue names, and the classes of world the kernels tell apart
    pairs = {(c.n_spheres, c.n_planes) for c in pw.CASES}
    assert {(0, 3), (0, 4), (1, 3), (0, 64), (0, 65), (60, 5), (63, 2), (64, 1), (0, 256), (0, 257), (1, 256), (100, 200),
            (128, 10), (127, 130), (128, 129)} <= pairs and any(c.has_grid for c in pw.CASES)
    assert {c.flavour for c in pw.CASES} == set(pw.FLAVOURS)
    for case_id, frames in pw.STRICT_PATH.items():
        assert pw.BY_ID[case_id].flavour == "plain"
        assert all(f in pw.BY_ID[case_id].kernels for f in frames)
    strict = {n.split("<")[0] for case_id, frames in pw.STRICT_PATH.items() for f in frames for n in pw.BY_ID[case_id].kernels[f] if n}
    assert {"pt_path_regions_kernel", "pt_path_tree_kernel", "pt_path_flagged_kernel", "pt_cell_kernel", "pt_tile_kernel"} <= strict


# ---- the worlds give those kernels work ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pw.CASES, ids=lambda c: c.id)
def test_planes_and_spheres_are_seen_and_lights_both_reach_and_miss(orc, case):
    flat, info = flat_of(case.id)
    frame = primary(orc, case.id, case.size)
    idx = frame.shape_index[0]
    hit = idx >= 0
    winners = set(np.unique(idx[hit]).tolist())
    planes, slots = slot_of_planes(flat)
    assert planes.tolist() == sorted(info["plane_at"])
    seen = np.array([p in winners for p in planes])
    spheres_seen = sum(1 for p in info["sphere_at"] if p in winners)
    print(f"{case.id}: {int(seen.sum())} of {case.n_planes} planes and {spheres_seen} of {case.n_spheres} spheres are the first hit of a pixel, "
          f"{(~hit).mean():.2f} of the pixels see the sky")
    assert 2 * seen.sum() >= case.n_planes
    assert spheres_seen >= min(case.n_spheres, 1)
    assert 2 * spheres_seen >= min(case.n_spheres, 120)
    if case.flavour in ("fan", "horizon"):
        assert 0.03 < (~hit).mean() < 0.6  # OnOff is neither white nor black
    elif case.n_planes >= 4:
        assert hit.all()                   # closed: every primary ray hits something
    if case.id in pw.PASS_BOUNDARY:
        for p in sorted(set((slots // 64).tolist())):
            assert seen[slots // 64 == p].any(), f"no plane of pass {p} is visible"
    # lights: per hit point and light, is the point on the side the normal points to, and does the shadow ray get through?
    pts = np.argwhere(hit)
    facing = np.zeros((len(pts), flat.n_lights), bool)
    visible = np.zeros((len(pts), flat.n_lights), bool)
    for n, (r, c) in enumerate(pts):
        for l in range(flat.n_lights):
            facing[n, l] = (flat.light_pos[:, l] - frame.point[0, r, c]) @ frame.normal[0, r, c] > 0.0
            visible[n, l] = orc.is_point_visible(flat, flat.light_pos[:, l], frame.point[0, r, c])
    reach = facing & visible
    lit, dark = reach.any(axis=1), ~reach.all(axis=1)
    print(f"    lights: reach {reach.sum(axis=0).tolist()} of {len(pts)} points; facing but blocked {(facing & ~visible).sum(axis=0).tolist()}")
    assert lit.sum() > len(pts) // 10
    assert dark.sum() > len(pts) // 10
    # one light reaches no point of the picture -- and not because every surface turns its back on it: its shadow rays from
    # points that face it are blocked, every one
    shadowed = [l for l in range(flat.n_lights) if not reach[:, l].any()]
    assert shadowed, "no light is shadowed for every point of the picture"
    assert max((facing[:, l] & ~visible[:, l]).sum() for l in shadowed) >= 100
    assert (reach.sum(axis=0) > 0).sum() >= 2
    radii = flat.light_radius
    assert (radii == 0.0).any()
    assert (radii > 0.0).any()


def test_the_constructed_world_shows_the_pair_and_never_the_plane_through_the_origin(orc):
    flat, info = flat_of("coincident")
    i, j = info["pair"]
    assert flat.kind[i] == flat.kind[j] == abi.SHAPE_PLANE
    assert np.array_equal(flat.m[:, i], flat.m[:, j])
    assert np.array_equal(flat.invm[:, i], flat.invm[:, j])
    assert not np.array_equal(flat.pig_c1[:, i], flat.pig_c1[:, j])
    between = flat.kind[i + 1:j]
    assert (between == abi.SHAPE_SPHERE).sum() >= 2
    assert (between == abi.SHAPE_PLANE).sum() >= 2
    for size in ((75, 45), (41, 27)):
        for camera in ("perspective", "orthogonal"):
            frame = primary(orc, "coincident", size, camera)
            idx = frame.shape_index[0]
            assert (idx == i).sum() >= 20
            assert not (idx == j).any()
            assert camera == "orthogonal" or not (idx == info["through_origin"]).any()
            W, H = size
            # the central ray is (1, 0, 0) exactly: parallel to the wall (d'.z == 0), starting on the plane through the origin
            assert frame.ray_dir[0, H // 2, W // 2].tolist() == [1.0, 0.0, 0.0] or camera == "perspective"
            if camera == "perspective":
                d = frame.ray_dir[0, H // 2, W // 2]
                assert d[1] == 0.0
                assert d[2] == 0.0
                assert not frame.ray_origin[0].any()
                assert flat.invm[8:11, info["parallel"]] @ d == 0.0
                assert (idx == info["parallel"]).sum() >= 20


def test_light_worlds_hold_the_lights_they_are_asked_for():
    for n_spheres, n_planes in pw.LIGHT_WORLDS:
        for n_lights in pw.LIGHT_COUNTS:
            for flavour in ("plain", "closed"):
                flat = flatten.flatten_world(pw.light_world(n_spheres, n_planes, n_lights, flavour)[0])
                assert (flat.n_shapes, flat.n_lights) == (n_spheres + n_planes, n_lights)
                assert bool(np.any(flat.brdf_kind == abi.BRDF_SPECULAR)) == (flavour == "closed")
    assert set(pw.LIGHT_COUNTS) >= {1, 8, 33, 64, 65}


def test_sheared_planes_are_sheared_and_the_recipe_is_deterministic():
    flat, _ = flat_of("s1-p256")
    worst, scaled = 0.0, 0
    for i in np.flatnonzero(flat.kind == abi.SHAPE_PLANE):
        m = flat.m[:, i].reshape(3, 4)[:, :3]
        sv = np.linalg.svd(m, compute_uv=False)
        worst = max(worst, sv[0] / sv[-1])
        scaled += abs(np.linalg.norm(flat.invm[8:11, i]) - 1.0) > 1e-2  # (row 2 of invm: what plane_keeps normalises by)
    assert worst > 10.0
    assert scaled > 200
    a = flatten.flatten_world(pw.case_world(pw.BY_ID["s60-p5"])[0])
    assert a.same_bits(flat_of("s60-p5")[0])
    assert not a.same_bits(flat_of("s63-p2")[0])
