"""pt_tile4_kernel on frames of one full tile and of partial tiles (16x16, 17x17, 33x17: idle lanes to the right and below), over
the worlds of tests/tile4_straight.py: a kept sphere no ray meets, the eye inside a sphere whose first root is computed, exact
ties between coincident spheres and planes in both orders, a plane edge-on (an image row with d.z = 0: that wave is not `fast`)
and one behind the eye, a checkered sphere (the per-pixel remainder), 65 and 130 shapes (passes 1 and 2 of the cull).
tests/test_tile4_straight.py shows on the CPU that each frame holds what its world is named for.

Flat in fp64 and fp32 and OnOff, dome shortcut on and off, ``tile4_lds`` 1 and 0: every frame bit for bit the oracle's (its
``x*x`` mode) and bit for bit the other variant's; the checkered sphere goes through atan2 / acos and is held to the oracle
within the 1e-5 relative per channel of tests/test_gpu_tile4_winners.py, and bit for bit between the variants.
"""
import numpy as np
import pytest

from pytracer_amd import abi
from tests import tile4_straight as ts
from tests import util

pytestmark = pytest.mark.gpu

LIBM_TOL = 1e-5  # tests/test_gpu_parity.py: TOL, the bar of frames that depend on atan2 / acos

_wanted = {}


def _oracle(oracle, key, scene, cam, par):
    """The oracle's frame in its x*x mode, computed once per (world, frame, renderer, format) and left unchanged."""
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


@pytest.mark.parametrize("name", ts.WORLDS)
def test_frames_against_the_oracle_and_the_other_variant(dev, oracle, name):
    scene, _ = ts.scene(name)
    saved = dev.get_tuning("tile4_lds")
    try:
        with dev.DeviceScene(scene) as ds:
            for W, H in ts.FRAMES:
                cam = ts.camera(W, H)
                for renderer, fmt in ((abi.RENDERER_FLAT, abi.OUT_F64), (abi.RENDERER_FLAT, abi.OUT_F32), (abi.RENDERER_ONOFF, abi.OUT_F64)):
                    par = ts.params(W, H, renderer, fmt)
                    want = _oracle(oracle, (name, W, H, renderer, fmt), scene, cam, par)
                    for dome in (True, False):
                        ds.set_dome_shortcut(dome)
                        frames = []
                        for lds in (1, 0):
                            dev.set_tuning("tile4_lds", lds)
                            assert dev.plan(scene, cam, par).main_kernel.startswith("pt_tile4_kernel<")
                            frames.append(ds.render(cam, par))
                            assert ds.stats().kernel == abi.KERNEL_TILE4
                        got, plain = frames
                        where = f"{name} {W}x{H} renderer {renderer} fmt {fmt} dome {dome}"
                        assert got.dtype == want.dtype and got.shape == want.shape, where
                        if name == "checkered" and renderer == abi.RENDERER_FLAT:
                            err = util.rel_err(got, want)
                            assert np.all(err <= LIBM_TOL), f"{where}: max rel {err.max():.3e}"
                        else:
                            assert got.tobytes() == want.tobytes(), f"{where}: {int((got != want).any(axis=-1).sum())} pixels != oracle"
                        assert got.tobytes() == plain.tobytes(), f"{where}: differs from the frame under tile4_lds = 0"
            ds.set_dome_shortcut(True)
    finally:
        dev.set_tuning("tile4_lds", saved)
