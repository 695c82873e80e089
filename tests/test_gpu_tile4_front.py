"""pt_tile4_kernel's front end: the wave's shared u / v quotients, cone, cull and the walk over a tile's survivors.

The worlds come from tests/tile4_front.py (tests/test_tile4_front.py shows on the CPU that each holds what it is named for).
Frames are S = 0 and, but for one, perspective.  Each frame is compared bit for bit with the oracle in its ``x*x`` mode, in fp64
and fp32, with the dome shortcut on and off, and -- where the plan names the staged 16x16 kernel -- bit for bit with the same
frame under ``tile4_lds = 0``.  A world the planner gives to another kernel (one shape; an orthogonal camera) is still held to
the oracle: its frame must not depend on which kernel renders it.
"""
import numpy as np
import pytest

from pytracer_amd import abi
from tests import tile4_front as tf

pytestmark = pytest.mark.gpu

STAGED, UNSTAGED, ONOFF = "pt_tile4_kernel<FLAT, LDS>", "pt_tile4_kernel<FLAT, noLDS>", "pt_tile4_kernel<ONOFF, noLDS>"

_wanted = {}


def _oracle(oracle, key, scene, cam, par):
    """The oracle's frame in its x*x mode, computed once per key and left unchanged."""
    if key not in _wanted:
        try:
            _wanted[key] = oracle.render(scene, cam, par, sqr_mode=oracle.SQR_MUL)[0]
        finally:
            oracle.set_sqr_mode(oracle.SQR_POW)
        _wanted[key].setflags(write=False)
    return _wanted[key]


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


def _check(dev, oracle, key, scene, cam, make_par, formats=(abi.OUT_F64, abi.OUT_F32), tile4=True):
    """Every format, the dome shortcut on and off: frame == oracle; with ``tile4`` the plan must name a 16x16 kernel, and the
    staged kernel's frame == the unstaged one's."""
    saved = dev.get_tuning("tile4_lds")
    try:
        with dev.DeviceScene(scene) as ds:
            for fmt in formats:
                par = make_par(fmt)
                want = _oracle(oracle, key + (fmt,), scene, cam, par)
                for dome in (True, False):
                    ds.set_dome_shortcut(dome)
                    dev.set_tuning("tile4_lds", 1)
                    kernel = dev.plan(scene, cam, par).main_kernel
                    if tile4:
                        assert kernel in (STAGED, UNSTAGED, ONOFF), kernel
                    got = ds.render(cam, par)
                    assert got.dtype == want.dtype and got.shape == want.shape
                    assert got.tobytes() == want.tobytes(), \
                        f"{key} fmt {fmt} dome {dome} ({kernel}): {int((got != want).any(axis=-1).sum())} pixels != oracle"
                    if kernel == STAGED:
                        dev.set_tuning("tile4_lds", 0)
                        assert dev.plan(scene, cam, par).main_kernel == UNSTAGED
                        plain = ds.render(cam, par)
                        assert got.tobytes() == plain.tobytes(), f"{key} fmt {fmt} dome {dome}: staged frame != unstaged frame"
            ds.set_dome_shortcut(True)
    finally:
        dev.set_tuning("tile4_lds", saved)


NAMED = ("empty_beside_full", "one_survivor", "twelve_mixed", "planes_only", "inside_two", "horizon")


@pytest.mark.parametrize("size", tf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", NAMED)
def test_flat_frames(dev, oracle, name, size):
    w, h = size
    scene, cam = tf.scene_and_camera(name, w, h)
    _check(dev, oracle, (name, w, h), scene, cam, lambda fmt: tf.params(w, h, fmt))


@pytest.mark.parametrize("size", tf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ("twelve_mixed", "empty_beside_full", "planes_only"))
def test_onoff_frames(dev, oracle, name, size):
    w, h = size
    scene, cam = tf.scene_and_camera(name, w, h)
    _check(dev, oracle, (name, w, h, "onoff"), scene, cam, lambda fmt: tf.params(w, h, fmt, renderer=abi.RENDERER_ONOFF))


@pytest.mark.parametrize("n", tf.COUNTS)
def test_counted_worlds(dev, oracle, n):
    """1, 63, 64, 65 and 130 shapes at 33x17 (the middle column's wave is not `fast`): the lane clamp of the first pass, the pass
    boundary, and a world past the 64 shapes that are staged.  One shape is below what the planner tiles."""
    w, h = 33, 17
    scene, cam = tf.scene_and_camera(f"counted_{n}", w, h)
    _check(dev, oracle, (f"counted_{n}", w, h), scene, cam, lambda fmt: tf.params(w, h, fmt), tile4=n >= 4)


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("name", ("twelve_mixed", "horizon"))
def test_share_of_two_ranks(dev, oracle, name, rank):
    """Row blocks of 16 of the 40-row frame: rank 0 has image rows 0..15 and 32..39 (a partial tile whose global row is not
    its local one: the shared v-quotients must be the global rows'), rank 1 the rows 16..31."""
    w, h = 48, 40
    assert abi.rows_for_rank(h, 16, 2, 0) == list(range(16)) + list(range(32, 40))
    scene, cam = tf.scene_and_camera(name, w, h)
    _check(dev, oracle, (name, w, h, "rank", rank), scene, cam,
           lambda fmt: tf.params(w, h, fmt, row_block=16, n_ranks=2, rank=rank))


def test_three_frames_with_the_camera_moved(dev, oracle):
    """Three frames on one handle, another camera each time: nothing of a frame's rays or culling outlives it."""
    w, h = 48, 40
    scene, _ = tf.scene_and_camera("twelve_mixed", w, h)
    par = tf.params(w, h)
    with dev.DeviceScene(scene) as ds:
        for k in (0, 1, 2):
            cam = tf.moved_camera(w, h, k)
            assert dev.plan(scene, cam, par).main_kernel == STAGED
            got = ds.render(cam, par)
            want = _oracle(oracle, ("twelve_mixed", w, h, "moved", k), scene, cam, par)
            assert got.tobytes() == want.tobytes(), f"frame {k} != oracle"
    assert not np.array_equal(_wanted[("twelve_mixed", w, h, "moved", 0)], _wanted[("twelve_mixed", w, h, "moved", 1)])


def test_orthogonal_camera(dev, oracle):
    w, h = 17, 17
    scene, cam = tf.scene_and_camera("ortho", w, h)
    _check(dev, oracle, ("ortho", w, h), scene, cam, lambda fmt: tf.params(w, h, fmt), tile4=False)
