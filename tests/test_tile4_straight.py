"""The worlds of tests/tile4_straight.py hold what they are named for (CPU: the oracle's own rays and hit records), so that
tests/test_gpu_tile4_straight.py cannot pass vacuously; and the three instantiations of pt_tile4_kernel keep their registers."""
import os
import sys

import numpy as np
import pytest

from pytracer_amd import abi, device
from tests import tile4_straight as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_hits = {}


def _records(oracle, name, W, H):
    """Per pixel: the world's hit record (or None) and every shape's own, computed once per (world, frame)."""
    key = (name, W, H)
    if key not in _hits:
        scene, _ = ts.scene(name)
        cam = ts.camera(W, H)
        rows = []
        for row in range(H):
            for col in range(W):
                ray = oracle.tracer_fire_ray(cam, W, H, col, row)
                rows.append((col, row, ray, oracle.world_intersect(scene, ray)))
        _hits[key] = rows
    return _hits[key]


def _winner(rec):
    return -1 if rec is None else int(rec[9])


@pytest.mark.parametrize("W,H", ts.FRAMES)
def test_a_kept_sphere_that_no_ray_meets_beside_one_that_some_lanes_meet(oracle, W, H):
    scene, roles = ts.scene("never-hit")
    rows = _records(oracle, "never-hit", W, H)
    assert not any(oracle.shape_intersect(scene, roles["tiny"], ray) is not None for _, _, ray, _ in rows)
    # ... though it lies inside the frame: between the rays of the four pixels around the frame's centre
    first_tile = [_winner(rec) == roles["some"] for col, row, _, rec in rows if col < 16 and row < 16]
    assert any(first_tile) and not all(first_tile)


@pytest.mark.parametrize("W,H", ts.FRAMES)
def test_the_eye_is_inside_a_sphere_whose_first_root_is_computed(oracle, W, H):
    scene, roles = ts.scene("inside")
    i = roles["near"]
    o = oracle.xform(scene.invm[:, i], 0, ts.EYE)
    c = (o[0] * o[0] + o[1] * o[1] + o[2] * o[2]) - 1.0
    assert -0.5 < c < 0.0
    rows = _records(oracle, "inside", W, H)
    won = [rec for _, _, _, rec in rows if _winner(rec) == i]
    assert won and all(rec[0] > 1e-5 for rec in won)  # (the second root: the first is behind the eye)
    assert any(_winner(rec) not in (i, -1) for _, _, _, rec in rows)


@pytest.mark.parametrize("name", ("ties", "ties-swapped"))
@pytest.mark.parametrize("W,H", ts.FRAMES)
def test_coincident_shapes_tie_exactly_and_the_first_wins(oracle, name, W, H):
    scene, roles = ts.scene(name)
    rows = _records(oracle, name, W, H)
    for first, second in (("first_sphere", "second_sphere"), ("first_plane", "second_plane")):
        a, b = roles[first], roles[second]
        ties = wins = 0
        for _, _, ray, rec in rows:
            ha, hb = oracle.shape_intersect(scene, a, ray), oracle.shape_intersect(scene, b, ray)
            assert (ha is None) == (hb is None)
            if ha is not None:
                assert ha[0].tobytes() == hb[0].tobytes()
                ties += 1
                assert _winner(rec) != b
                wins += _winner(rec) == a
        assert ties > 0 and wins > 0, (first, ties, wins)
    # a tile with a tie: the first tile holds pixels of both pairs
    first_tile = {_winner(rec) for col, row, _, rec in rows if col < 16 and row < 16}
    assert {roles["first_sphere"], roles["first_plane"]} <= first_tile


@pytest.mark.parametrize("W,H", ts.FRAMES)
def test_a_plane_edge_on_and_a_plane_behind_the_eye(oracle, W, H):
    scene, roles = ts.scene("planes")
    rows = _records(oracle, "planes", W, H)
    assert not any(oracle.shape_intersect(scene, roles["behind"], ray) is not None for _, _, ray, _ in rows)
    edge_rows = {row for _, row, _, rec in rows if _winner(rec) == roles["edge"]}
    assert edge_rows and min(edge_rows) > (H - 1) // 2  # only the rows that look down
    flat_rows = {row for _, row, ray, _ in rows if ray[5] == 0.0}
    if H % 2:
        # the middle row's rays have d.z exactly 0: |dz| < 1e-5 for these lanes, and the tile's wave is not `fast`
        assert flat_rows == {H // 2}
        assert not any(oracle.shape_intersect(scene, roles["edge"], ray) is not None for _, row, ray, _ in rows if row == H // 2)
    else:
        assert not flat_rows


@pytest.mark.parametrize("W,H", ts.FRAMES)
def test_the_checkered_sphere_is_seen(oracle, W, H):
    _, roles = ts.scene("checkered")
    assert any(_winner(rec) == roles["ball"] for _, _, _, rec in _records(oracle, "checkered", W, H))


@pytest.mark.parametrize("name", ("n65", "n130"))
def test_the_shapes_of_the_later_passes_are_seen(oracle, name):
    scene, roles = ts.scene(name)
    W, H = ts.FRAMES[1]
    assert scene.n_shapes == int(name[1:])
    winners = {_winner(rec) for _, _, _, rec in _records(oracle, name, W, H)}
    assert set(roles.values()) <= winners
    assert device.plan(scene, ts.camera(W, H), ts.params(W, H)).main_kernel == "pt_tile4_kernel<FLAT, noLDS>"


@pytest.mark.parametrize("name", ts.WORLDS)
def test_the_plan_sends_every_world_to_the_16x16_tiles(name):
    scene, _ = ts.scene(name)
    staged = scene.n_shapes <= 64
    saved = device.get_tuning("tile4_lds")
    try:
        device.set_tuning("tile4_lds", 1)
        for W, H in ts.FRAMES:
            assert device.plan(scene, ts.camera(W, H), ts.params(W, H)).main_kernel == \
                ("pt_tile4_kernel<FLAT, LDS>" if staged else "pt_tile4_kernel<FLAT, noLDS>")
            assert device.plan(scene, ts.camera(W, H), ts.params(W, H, abi.RENDERER_ONOFF)).main_kernel == "pt_tile4_kernel<ONOFF, noLDS>"
    finally:
        device.set_tuning("tile4_lds", saved)


def test_the_three_instantiations_keep_their_registers_and_use_no_scratch():
    from pytracer_amd import build

    build.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kres
    finally:
        sys.path.pop(0)
    res = {k: v for k, v in kres.kernel_resources(build.LIB).items() if k.startswith("void pt_tile4_kernel<")}
    assert sorted(res) == ["void pt_tile4_kernel<0, false>(PtKArgs)", "void pt_tile4_kernel<1, false>(PtKArgs)", "void pt_tile4_kernel<1, true>(PtKArgs)"]
    assert all(r["scratch"] == 0 for r in res.values()), res
    assert res["void pt_tile4_kernel<1, true>(PtKArgs)"]["vgpr"] <= 96 and res["void pt_tile4_kernel<1, false>(PtKArgs)"]["vgpr"] <= 96
    assert res["void pt_tile4_kernel<0, false>(PtKArgs)"]["vgpr"] <= 78
