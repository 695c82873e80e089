"""Worlds for the Flat palette of pt_tile4_kernel<FLAT, *> (tests/test_gpu_tile4_palette.py): ``n`` shapes in a 48x40 frame.

A world is the sphere around the camera, a checkered ground plane, a wall with an image pigment (the per-pixel remainder) and
``n - 3`` small spheres, each with a BRDF pigment AND an emitted colour of its own: a palette entry read from the wrong place,
or not there, changes a pixel.  Every small sphere sits on the ray through a pixel centre, 0.9 pixels in angular radius on a
grid of two pixels, so each wins at least that pixel and none hides another; the first ones stand nearest the frame's centre.
The top left 16x16 tile is left empty and looks away from both planes: its wave is settled by the dome shortcut, beside three
waves that shade, and the 48x40 frame leaves the right and lower workgroups partly outside.

``checkered_ball`` swaps the first small sphere for a larger checkered one (atan2 / acos: the remainder, held within the libm
tolerance).  Slots are spheres first, planes last (pt_scene_build.h): with 33 shapes the planes are the last entry of the
palette's first 1 KiB chunk and the first of its second.
"""
from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm
from tests import tile4_winners as tw

W, H = 48, 40
STAGED_COUNTS = (4, 32, 33, 63, 64)
UNSTAGED_COUNTS = (65, 100, 256)
DIST = 0.75  # along the pixel's ray (direction (1, dy, dz) from the rays' origin (-2, 0, 1)): above the ground for every row


def _spots():
    """(x, y, z, radius) of every grid position, nearest the frame's centre first, none near the top left tile."""
    out = []
    for row in range(1, H, 2):
        for col in range(1, W, 2):
            if col < 21 and row < 21:  # (the tile's cone is circular: it reaches 3.3 pixels past the middle of the tile's edges)
                continue
            dy, dz = (1.0 - 2.0 * (col + 0.5) / W) * (W / H), 1.0 - 2.0 * (row + 0.5) / H  # imagetracer.py:48-58, camera.py:103-124
            key = (col - W // 2) ** 2 + (row - H // 2) ** 2
            out.append((key, row, col, (-2.0 + DIST, DIST * dy, 1.0 + DIST * dz, 0.9 * DIST * 2.0 / H)))
    return [s[3] for s in sorted(out)]


def _ball(i, x, y, z, rad) -> hm.Sphere:
    """Small sphere ``i``: no two share a pigment or an emitted colour, and most sums of the two are inexact in fp64."""
    pig = hm.Color(0.1 + 0.003 * i, 0.9 - 0.0031 * i, 0.3 + 0.0017 * (i % 97))
    emi = hm.Color(0.01 + 0.0007 * i, 0.02 + 0.0003 * (i % 31), 0.2 - 0.00071 * i)
    return hm.Sphere(hm.translation(hm.Vec(x, y, z)) * hm.scaling(hm.Vec(rad, rad, rad)),
                     hm.Material(hm.DiffuseBRDF(hm.UniformPigment(pig)), hm.UniformPigment(emi)))


def world(n: int, checkered_ball: bool = False) -> hm.World:
    assert 4 <= n <= 256
    sky = hm.Sphere(hm.scaling(hm.Vec(50.0, 50.0, 50.0)),
                    hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(0.05, 0.1, 0.15))), hm.UniformPigment(hm.Color(0.7, 0.5, 1.0))))
    ground = hm.Plane(hm.Transformation(),
                      hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.3, 0.5, 0.1), hm.Color(0.1, 0.2, 0.5), 4)),
                                  hm.UniformPigment(hm.Color(0.01, 0.02, 0.03))))
    wall = hm.Plane(hm.translation(hm.Vec(0.13, -6.0, 0.29)) * hm.rotation_x(90.0),  # the plane y = -6, right of the camera
                    hm.Material(hm.DiffuseBRDF(hm.ImagePigment(tw.texture())), hm.UniformPigment(hm.Color(0.02, 0.0, 0.01))))
    w = hm.World()
    w.add_shape(sky)
    spots = _spots()
    assert len(spots) >= n - 3
    for i, (x, y, z, rad) in enumerate(spots[:n - 3]):
        if checkered_ball and i == 0:
            check = hm.CheckeredPigment(hm.Color(0.8, 0.7, 0.1), hm.Color(0.1, 0.1, 0.6), 6)
            w.add_shape(hm.Sphere(hm.translation(hm.Vec(x, y, z)) * hm.scaling(hm.Vec(3.0 * rad, 3.0 * rad, 3.0 * rad)),
                                  hm.Material(hm.DiffuseBRDF(check), hm.UniformPigment(hm.Color(0.05, 0.05, 0.05)))))
        else:
            w.add_shape(_ball(i, x, y, z, rad))
    w.add_shape(ground)
    w.add_shape(wall)
    assert len(w.shapes) == n
    return w


_built = {}


def scene_and_camera(n: int, checkered_ball: bool = False):
    """(FlatScene, abi.Camera), built once."""
    key = (n, checkered_ball)
    if key not in _built:
        _built[key] = (flatten.flatten_world(world(n, checkered_ball)), flatten.flatten_camera(scenes.synthetic_camera(W, H)))
    return _built[key]


def params(fmt=abi.OUT_F64) -> abi.Params:
    return abi.make_params(W, H, abi.RENDERER_FLAT, out_format=fmt)
