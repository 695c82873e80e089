"""The worlds of tests/tile4_palette.py show what they are for (CPU, the oracle): every small sphere wins a pixel with a colour
nobody else has, the planes are seen, the plan sends each shape count to the kernel variant the GPU test expects, and the top
left tile sees the sky alone."""
import numpy as np
import pytest

from pytracer_amd import abi, device
from tests import tile4_palette as tp


@pytest.mark.parametrize("n", tp.STAGED_COUNTS + tp.UNSTAGED_COUNTS)
def test_every_small_sphere_wins_a_pixel(oracle, n):
    scene, cam = tp.scene_and_camera(n)
    assert scene.n_shapes == n
    try:
        img = oracle.render(scene, cam, tp.params(), sqr_mode=oracle.SQR_MUL)[0]
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
    colours = {tuple(p) for p in img.reshape(-1, 3)}
    # the sky, n - 3 small spheres, at least two colours of the ground and two of the wall's image
    assert len(colours) >= 1 + (n - 3) + 4, (n, len(colours))
    # the small spheres' colours: pigment + emitted, as FlatRenderer adds them
    for i in (0, n - 4):
        pig = (0.1 + 0.003 * i, 0.9 - 0.0031 * i, 0.3 + 0.0017 * (i % 97))
        emi = (0.01 + 0.0007 * i, 0.02 + 0.0003 * (i % 31), 0.2 - 0.00071 * i)
        assert tuple(p + e for p, e in zip(pig, emi)) in colours, (n, i)
    sky = tuple(img[0, 0])
    assert sky == (0.05 + 0.7, 0.1 + 0.5, 0.15 + 1.0) and np.all(img[:16, :16] == np.array(sky))


@pytest.mark.parametrize("n", tp.STAGED_COUNTS + tp.UNSTAGED_COUNTS)
def test_the_plan_names_the_variant(n):
    """(The switch is set here and put back: it is one value for the whole process, and whatever ran before may have left it.)"""
    scene, cam = tp.scene_and_camera(n)
    staged = n in tp.STAGED_COUNTS
    saved = device.get_tuning("tile4_lds")
    try:
        device.set_tuning("tile4_lds", 1)
        pl = device.plan(scene, cam, tp.params())
        assert pl.main_kernel == ("pt_tile4_kernel<FLAT, LDS>" if staged else "pt_tile4_kernel<FLAT, noLDS>")
        assert pl.lds_main == (384 * n if staged else 0)
        device.set_tuning("tile4_lds", 0)
        pl = device.plan(scene, cam, tp.params())
        assert pl.main_kernel == "pt_tile4_kernel<FLAT, noLDS>" and pl.lds_main == 0
    finally:
        device.set_tuning("tile4_lds", saved)


def test_the_checkered_sphere_is_seen(oracle):
    for n in (33, 100):
        scene, cam = tp.scene_and_camera(n, checkered_ball=True)
        try:
            img = oracle.render(scene, cam, tp.params(), sqr_mode=oracle.SQR_MUL)[0]
        finally:
            oracle.set_sqr_mode(oracle.SQR_POW)
        colours = {tuple(p) for p in img.reshape(-1, 3)}
        assert (0.8 + 0.05, 0.7 + 0.05, 0.1 + 0.05) in colours and (0.1 + 0.05, 0.1 + 0.05, 0.6 + 0.05) in colours
