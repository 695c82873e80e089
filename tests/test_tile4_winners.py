"""The worlds of tests/tile4_winners.py really show what they are for (from the oracle's hit records, no GPU), and the three
pt_tile4_kernel instantiations keep their resources: no scratch, at most 128 VGPRs (four waves per SIMD).

A world that fails its own condition here is a bug of the test world, never a reason to skip.
"""
import os
import sys

import numpy as np
import pytest

from pytracer_amd import abi
from tests import tile4_winners as tw
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_records = {}


def _hits(oracle, name, w, h):
    """(scene, shape index [h, w], uv [h, w, 2]) of a world's frame, computed once."""
    key = (name, w, h)
    if key not in _records:
        scene, cam = tw.scene_and_camera(name, w, h)
        fr = util.oracle_frame(oracle, scene, cam, tw.params(w, h))
        _records[key] = (scene, fr.shape_index[0].copy(), fr.uv[0].copy())
    return _records[key]


def _lane_pixels(idx16):
    """The named tile's winners as the kernel's lanes hold them: [64 lanes, 4 pixels] (lane l: pixel (l & 7, l >> 3) of each
    8x8 quadrant); pixels off the frame are -2."""
    full = np.full((16, 16), -2, dtype=np.int64)
    full[:idx16.shape[0], :idx16.shape[1]] = idx16
    return np.stack([full[:8, :8].reshape(64), full[:8, 8:].reshape(64), full[8:, :8].reshape(64), full[8:, 8:].reshape(64)], axis=1)


def _winners(idx16):
    return sorted(set(int(i) for i in np.unique(idx16) if i >= 0))


def _both_checker_colours(scene, idx, uv, kind_field, steps_field):
    """For every shape on screen whose pigment of that field is checkered: are both of its colours on screen?"""
    found = 0
    for s in _winners(idx):
        if int(getattr(scene, kind_field)[s]) != abi.PIGMENT_CHECKERED:
            continue
        n = float(getattr(scene, steps_field)[s])
        u, v = uv[..., 0][idx == s], uv[..., 1][idx == s]
        first = (np.floor(u * n) % 2) == (np.floor(v * n) % 2)
        assert first.any() and (~first).any(), f"shape {s}: one colour of its {kind_field[:3]} checker only"
        found += 1
    return found


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_winner(oracle, size):
    scene, idx, uv = _hits(oracle, "one_winner", *size)
    ground = scene.n_shapes - 1
    assert (idx == ground).all(), "the ground must fill the frame"
    assert _winners(tw.tile_of(idx, *size)) == [ground]
    assert _both_checker_colours(scene, tw.tile_of(idx, *size), tw.tile_of(uv, *size), "pig_kind", "pig_steps") == 1


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_horizon(oracle, size):
    scene, idx, uv = _hits(oracle, "horizon", *size)
    tile = tw.tile_of(idx, *size)
    assert len(_winners(tile)) == 2 and (idx >= 0).all()
    lanes = _lane_pixels(tile)
    both = sum(1 for l in lanes if len(set(int(i) for i in l if i >= 0)) == 2)
    assert both > 0, "no lane holds both winners"
    assert _both_checker_colours(scene, tile, tw.tile_of(uv, *size), "pig_kind", "pig_steps") == 1


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_many_winners(oracle, size):
    scene, idx, uv = _hits(oracle, "many_winners", *size)
    tile, tuv = tw.tile_of(idx, *size), tw.tile_of(uv, *size)
    won = _winners(tile)
    assert len(won) >= 5, won
    kinds_p, kinds_e = np.asarray(scene.pig_kind)[won], np.asarray(scene.emi_kind)[won]
    assert ((kinds_p == abi.PIGMENT_UNIFORM) & (kinds_e == abi.PIGMENT_UNIFORM)).sum() >= 3, "small uniform spheres"
    wall = [s for s in won if scene.pig_kind[s] == abi.PIGMENT_CHECKERED and scene.emi_kind[s] == abi.PIGMENT_CHECKERED]
    assert len(wall) == 1 and scene.pig_steps[wall[0]] != scene.emi_steps[wall[0]]
    assert _both_checker_colours(scene, tile, tuv, "pig_kind", "pig_steps") == 2  # the ground and the wall
    assert _both_checker_colours(scene, tile, tuv, "emi_kind", "emi_steps") == 1


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_remainder(oracle, size):
    scene, idx, uv = _hits(oracle, "remainder", *size)
    tile, tuv = tw.tile_of(idx, *size), tw.tile_of(uv, *size)
    won = _winners(tile)
    kp, ke = np.asarray(scene.pig_kind), np.asarray(scene.emi_kind)
    image_planes = [s for s in won if kp[s] == abi.PIGMENT_IMAGE]
    mixed_planes = [s for s in won if kp[s] == abi.PIGMENT_CHECKERED and ke[s] == abi.PIGMENT_IMAGE]
    uniform = [s for s in won if kp[s] == abi.PIGMENT_UNIFORM and ke[s] == abi.PIGMENT_UNIFORM]
    assert len(image_planes) == 1 and len(mixed_planes) == 1 and len(uniform) >= 2, won
    for s in image_planes + mixed_planes:  # at least one pixel per texel row (pigment_color: row = int(v * h))
        rows = set(np.minimum((tuv[..., 1][tile == s] * tw.TEX_H).astype(np.int64), tw.TEX_H - 1).tolist())
        assert rows == set(range(tw.TEX_H)), (s, rows)
    assert _both_checker_colours(scene, tile, tuv, "pig_kind", "pig_steps") == 1


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_miss(oracle, size):
    scene, idx, _ = _hits(oracle, "miss", *size)
    tile = tw.tile_of(idx, *size)
    assert (tile < 0).any() and len(_winners(tile)) >= 3
    lanes = _lane_pixels(tile)
    assert any((l >= 0).any() and (l == -1).any() for l in lanes), "no lane holds a hit and a miss"
    if size == (48, 40):  # (the smaller frames have no tile above the horizon that the spheres stay out of)
        assert (idx[:16, :16] < 0).all(), "tile (0, 0) must hit nothing"


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_patterned_sphere(oracle, size):
    scene, idx, _ = _hits(oracle, "patterned_sphere", *size)
    won = _winners(tw.tile_of(idx, *size))
    patterned = [s for s in won if scene.kind[s] == abi.SHAPE_SPHERE and scene.pig_kind[s] == abi.PIGMENT_CHECKERED]
    assert len(patterned) == 1 and len(won) >= 3


def test_tile4_kernels_fit_four_waves_without_scratch():
    """The resources of the three instantiations, read from the built library's metadata as tools/kres.py reads them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kres
    from pytracer_amd import _lib, build

    build.build()
    rows = {k: v for k, v in kres.kernel_resources(_lib.lib_path()).items() if "pt_tile4_kernel<" in k}
    assert len(rows) == 3, sorted(rows)
    for name, r in rows.items():
        print(f"{name}: {r}")
        assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch"
        assert r["vgpr"] + r["agpr"] <= 128, f"{name}: {r['vgpr']} VGPRs + {r['agpr']} AGPRs"
