"""The worlds of tests/tile4_front.py really show what they are named for (from the oracle's hit records, no GPU), and the three
pt_tile4_kernel instantiations keep their resources: no scratch, at most 128 VGPRs.

A world that fails its own condition here is a bug of the test world, never a reason to skip.
"""
import os
import sys

import numpy as np
import pytest

from pytracer_amd import abi
from tests import tile4_front as tf
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_records = {}


def _hits(oracle, name, w, h):
    """(scene, shape index [h, w]) of a world's frame, computed once."""
    key = (name, w, h)
    if key not in _records:
        scene, cam = tf.scene_and_camera(name, w, h)
        fr = util.oracle_frame(oracle, scene, cam, tf.params(w, h), channels=abi.HIT_ALL)
        _records[key] = (scene, fr.shape_index[0].copy())
    return _records[key]


def _winners(idx):
    return sorted(set(int(i) for i in np.unique(idx) if i >= 0))


@pytest.mark.parametrize("size", tf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_empty_beside_full(oracle, size):
    scene, idx = _hits(oracle, "empty_beside_full", *size)
    tile = tf.tile_of(idx, *size)
    assert len(_winners(tile)) >= 6 and (tile < 0).any(), "hits and misses in the named tile"
    if size == (48, 40):
        assert (idx[:16, :16] < 0).all() and (idx[32:, 32:] < 0).all(), "tiles away from the spheres must hit nothing"


@pytest.mark.parametrize("size", tf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_survivor(oracle, size):
    scene, idx = _hits(oracle, "one_survivor", *size)
    assert _winners(idx) == [0], "the sphere around the camera wins every pixel"


@pytest.mark.parametrize("size", tf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twelve_mixed(oracle, size):
    scene, idx = _hits(oracle, "twelve_mixed", *size)
    won = _winners(tf.tile_of(idx, *size))
    # one-tile frames: the second row of spheres may fall off the 16 or 17 rows only if the grid says so (it does not)
    assert len(won) >= 12, won
    inv = np.asarray(scene.invm, dtype=np.float64)  # [12, n]: rows of the 3 x 4 inverse matrices
    off = np.abs(inv[[1, 2, 4, 6, 8, 9], :]).max(axis=0)  # the off-diagonal entries: zero for scale + translate
    turned = [s for s in won if off[s] > 0.0]
    plain = [s for s in won if s >= 1 and off[s] == 0.0]  # (shape 0 is the sphere around the camera)
    assert len(turned) >= 5 and len(plain) >= 5, won


@pytest.mark.parametrize("size", tf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planes_only(oracle, size):
    scene, idx = _hits(oracle, "planes_only", *size)
    assert scene.n_shapes == 4 and all(int(k) == abi.SHAPE_PLANE for k in scene.kind)
    assert (idx >= 0).all() and len(_winners(idx)) >= 3, _winners(idx)
    assert int(scene.kind[scene.n_shapes - 1]) == abi.SHAPE_PLANE


@pytest.mark.parametrize("n", tf.COUNTS)
def test_counted(oracle, n):
    scene, idx = _hits(oracle, f"counted_{n}", 33, 17)
    assert scene.n_shapes == n and (idx >= 0).all()
    if n > 1:
        assert len(_winners(idx)) >= 2


@pytest.mark.parametrize("size", tf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_inside_two(oracle, size):
    scene, idx = _hits(oracle, "inside_two", *size)
    cam = tf.scene_and_camera("inside_two", *size)[1]
    m = np.asarray(list(cam.m), dtype=np.float64).reshape(3, 4)
    origin = m[:, :3] @ np.array([-float(cam.screen_distance), 0.0, 0.0]) + m[:, 3]
    cs = []
    for s in range(scene.n_shapes):
        inv = np.asarray(scene.invm, dtype=np.float64)[:, s].reshape(3, 4)
        o = inv[:, :3] @ origin + inv[:, 3]
        cs.append(float(o @ o - 1.0))
    inside = sorted(c for c in cs if c < 0.0)
    assert len(inside) == 2 and inside[0] < -0.5 < inside[1], cs
    assert _winners(idx) == [1], "the nearer wall wins every pixel: the sky and the small spheres lie behind it"


def test_the_odd_frame_has_a_column_with_zero_dy():
    """(f) 33 columns: the middle pixel centre has u = 0.5 exactly, so d.y = (1 - 2u) * aspect = 0 and its wave is not `fast`."""
    w = 33
    assert (1.0 - 2.0 * ((16 + 0.5) / w)) == 0.0


def test_partial_tiles_have_idle_lanes():
    """(h) Every frame but 16x16 has tiles that stick out of it: to the right and below, the 48x40 frame below only."""
    for w, h in tf.FRAMES[1:]:
        assert w % 16 != 0 or h % 16 != 0
    assert sum(1 for w, h in tf.FRAMES if w % 16 and h % 16) >= 2


def test_tile4_kernels_keep_their_resources():
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
