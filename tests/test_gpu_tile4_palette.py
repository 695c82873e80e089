"""pt_tile4_kernel<FLAT, *>: step (a) of the shading reads the Flat palette (pt_layout.h: PtFlatPal) -- the staged variant from
the copy every wave makes in its own slice of LDS, with no workgroup barrier; the unstaged variant from the table behind aux[].

The worlds come from tests/tile4_palette.py (tests/test_tile4_palette_worlds.py shows on the CPU that each holds what it is for):
48x40 frames, 3x3 tiles with the right and lower workgroups partly outside the frame, a wave settled by the dome shortcut beside
three that shade, every sphere with a pigment and an emitted colour of its own, a checkered plane, an image-pigment plane (the
per-pixel remainder, which reads global memory in both variants).  Shape counts of the staged variant: 4 (nearly all lanes copy
padding, and the four waves share one slice), 32 and 33 (the last entry of the palette's first chunk, the first of its second),
63, 64 (both chunks full); of the unstaged variant: 65, 100, 256.

Each frame, fp64 and fp32, dome shortcut on and off, rays counted (the barrier inside the ray count is the kernel's only one),
is bit for bit the oracle's in its ``x*x`` mode and bit for bit the same under ``tile4_lds = 0``; the plan names the expected
kernel.  The worlds with a checkered SPHERE go through atan2 / acos: bit for bit between the variants, and the oracle within the
1e-5 relative per channel of tests/test_gpu_tile4_winners.py.
"""
import numpy as np
import pytest

from pytracer_amd import abi
from tests import tile4_palette as tp
from tests import util

pytestmark = pytest.mark.gpu

STAGED, UNSTAGED = "pt_tile4_kernel<FLAT, LDS>", "pt_tile4_kernel<FLAT, noLDS>"
LIBM_TOL = 1e-5  # tests/test_gpu_parity.py: TOL, the bar of frames that depend on atan2 / acos

_wanted = {}


def _oracle(oracle, key, scene, cam, par):
    """The oracle's frame in its x*x mode, computed once per (world, format) and left unchanged."""
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


def _frames(dev, oracle, n, checkered_ball=False):
    scene, cam = tp.scene_and_camera(n, checkered_ball)
    default_kernel = STAGED if n <= 64 else UNSTAGED
    saved = dev.get_tuning("tile4_lds")
    try:
        with dev.DeviceScene(scene) as ds:
            ds.set_count_rays(True)
            for fmt in (abi.OUT_F64, abi.OUT_F32):
                par = tp.params(fmt)
                want = _oracle(oracle, (n, checkered_ball, fmt), scene, cam, par)
                for dome in (True, False):
                    ds.set_dome_shortcut(dome)
                    frames = []
                    for lds, kernel in ((1, default_kernel), (0, UNSTAGED)):
                        dev.set_tuning("tile4_lds", lds)
                        assert dev.plan(scene, cam, par).main_kernel == kernel
                        frames.append(ds.render(cam, par))
                        st = ds.stats()
                        assert st.kernel == abi.KERNEL_TILE4 and st.lds_bytes == (384 * n if kernel == STAGED else 0)
                        # every pixel's ray counted once; whole tiles (the top left one sees the sky alone) settled by the shortcut
                        assert st.n_rays == tp.W * tp.H, st.n_rays
                        assert (0 < st.n_rays_resolved < st.n_rays and st.n_rays_resolved % 256 == 0) if dome else st.n_rays_resolved == 0, \
                            st.n_rays_resolved
                    got, plain = frames
                    assert got.dtype == want.dtype and got.shape == want.shape
                    where = f"{n} shapes fmt {fmt} dome {dome}"
                    if checkered_ball:
                        err = util.rel_err(got, want)
                        print(f"\n[tile4 palette] {where}: max rel err {err.max():.3e}")
                        assert np.all(err <= LIBM_TOL), f"{where}: max rel {err.max():.3e}"
                    else:
                        assert got.tobytes() == want.tobytes(), f"{where}: {int((got != want).any(axis=-1).sum())} pixels != oracle"
                    assert got.tobytes() == plain.tobytes(), f"{where}: {default_kernel} != the frame under tile4_lds = 0"
            ds.set_dome_shortcut(True)
    finally:
        dev.set_tuning("tile4_lds", saved)


@pytest.mark.parametrize("n", tp.STAGED_COUNTS)
def test_staged_palette_against_the_oracle_and_the_unstaged_kernel(dev, oracle, n):
    _frames(dev, oracle, n)


@pytest.mark.parametrize("n", tp.UNSTAGED_COUNTS)
def test_unstaged_palette_against_the_oracle(dev, oracle, n):
    _frames(dev, oracle, n)


@pytest.mark.parametrize("n", (33, 100))
def test_checkered_sphere_beside_the_palette(dev, oracle, n):
    _frames(dev, oracle, n, checkered_ball=True)
