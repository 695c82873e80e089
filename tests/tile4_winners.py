"""Worlds for the shading of pt_tile4_kernel<FLAT, *>: a loop over the wave's winning shapes, a per-pixel remainder behind it.

The loop shades shapes with two uniform pigments and planes whose pigments are uniform or checkered; a plane with an image
pigment and a patterned sphere go to the remainder.  Each builder below puts one of those mixtures into ONE 16x16 tile (one
wave) of every frame in ``FRAMES``; ``named_tile`` says which tile that is.  tests/test_tile4_winners.py asserts from the oracle's
hit records that each world shows what it is for, tests/test_gpu_tile4_winners.py renders them.

Every world has at least four shapes (the planner tiles from four on) and, but for ``patterned_sphere``, no patterned sphere: a
plane's (u, v) is x - floor(x), so its frames can be demanded bit for bit.
"""
from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm

# one tile; lanes off the frame in three of four tiles; three tiles across; two workgroups each way, the edge ones partly outside
FRAMES = ((16, 16), (17, 17), (33, 17), (48, 40))
TEX_W, TEX_H = 8, 4


def named_tile(w: int, h: int):
    """(tx, ty) of the 16x16 tile the worlds are built around: the middle one of the 48x40 frame, else the first."""
    return (1, 1) if (w, h) == (48, 40) else (0, 0)


def tile_of(a, w: int, h: int):
    """The named tile's part of a (rows, width, ...) array."""
    tx, ty = named_tile(w, h)
    return a[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]


def texture() -> hm.HdrImage:
    tex = hm.HdrImage(TEX_W, TEX_H)
    tex.array[...] = [[[0.1 + 0.1 * x, 0.9 - 0.2 * y, 0.3 + 0.05 * (x + y)] for x in range(TEX_W)] for y in range(TEX_H)]
    return tex


def _uniform(r, g, b) -> hm.Material:
    return hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(r, g, b))), hm.UniformPigment(hm.BLACK))


def _ball(x, y, z, rad, colour) -> hm.Sphere:
    return hm.Sphere(hm.translation(hm.Vec(x, y, z)) * hm.scaling(hm.Vec(rad, rad, rad)), _uniform(*colour))


def _sky() -> hm.Sphere:
    return hm.Sphere(hm.scaling(hm.Vec(50.0, 50.0, 50.0)),
                     hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.BLACK)), hm.UniformPigment(hm.Color(0.7, 0.5, 1.0))))


def _ground(steps=4, emitted=None) -> hm.Plane:
    check = hm.CheckeredPigment(hm.Color(0.3, 0.5, 0.1), hm.Color(0.1, 0.2, 0.5), steps)
    return hm.Plane(hm.Transformation(), hm.Material(hm.DiffuseBRDF(check), emitted or hm.UniformPigment(hm.BLACK)))


def _behind():
    """Three small spheres behind the camera: they make a world of four shapes and win no pixel."""
    return [_ball(-6.0 - i, 0.5 * i, 1.0, 0.2, (0.2, 0.3 + 0.1 * i, 0.4)) for i in range(3)]


def _world(shapes) -> hm.World:
    w = hm.World()
    for s in shapes:
        w.add_shape(s)
    assert len(w.shapes) >= 4
    return w


def _spots(w: int, h: int, n: int):
    """``n`` (x, y, z, radius) for spheres four units in front of synthetic_camera that show in the named tile above the
    horizon: centred on the rays through the pixel centres of columns 2, 5, 8, ... of the tile, three rows above the horizon,
    one pixel in angular radius (so each covers at least its own pixel centre, and neighbours do not touch)."""
    tx, _ = named_tile(w, h)
    row = h // 2 - 3
    out = []
    for k in range(n):
        col = tx * 16 + 2 + 3 * k
        dy, dz = (1.0 - 2.0 * (col + 0.5) / w) * (w / h), 1.0 - 2.0 * (row + 0.5) / h  # imagetracer.py:48-58, camera.py:103-124
        out.append((3.0, 4.0 * dy, 1.0 + 4.0 * dz, 4.0 * 2.0 / h))
    return out


def one_winner(w, h):
    """The camera looks down at the checkered ground: every pixel of every tile has the same winner, a plane."""
    cam = hm.PerspectiveCamera(1.0, w / h, hm.translation(hm.Vec(-1.0, 0.0, 2.0)) * hm.rotation_y(60.0))
    return _world(_behind() + [_ground()]), cam


def horizon(w, h):
    """The ground below the sphere around the camera: the named tile holds the horizon, so its wave has two winners and the
    lanes whose upper pixels are above it hold both."""
    return _world([_sky()] + _behind()[:2] + [_ground()]), scenes.synthetic_camera(w, h)


def many_winners(w, h):
    """Five small uniform spheres in front of a wall whose brdf pigment and emitted pigment are checkered with different
    steps, above the checkered ground: seven winners in the named tile."""
    wall = hm.Plane(hm.translation(hm.Vec(9.0, 0.37, 0.21)) * hm.rotation_y(90.0),  # (off the dyadic grid of the pixel centres)
                    hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.6, 0.1, 0.2), hm.Color(0.2, 0.6, 0.7), 2)),
                                hm.CheckeredPigment(hm.Color(0.05, 0.1, 0.3), hm.Color(0.3, 0.05, 0.1), 3)))
    balls = [_ball(x, y, z, r, (0.1 + 0.15 * i, 0.9 - 0.15 * i, 0.5)) for i, (x, y, z, r) in enumerate(_spots(w, h, 5))]
    return _world(balls + [_ground(), wall]), scenes.synthetic_camera(w, h)


def remainder(w, h):
    """A ceiling with an image pigment, a ground with a checkered pigment and an image as emitted radiance (both go to the
    per-pixel remainder) and uniform spheres between them (shaded in the loop), all in the named tile."""
    image = hm.ImagePigment(texture())
    ceiling = hm.Plane(hm.translation(hm.Vec(0.0, 0.0, 3.0)), hm.Material(hm.DiffuseBRDF(image), hm.UniformPigment(hm.BLACK)))
    balls = [_ball(x, y, z, r, (0.2 + 0.3 * i, 0.4, 0.8 - 0.3 * i)) for i, (x, y, z, r) in enumerate(_spots(w, h, 3))]
    return _world(balls + [_ground(emitted=image), ceiling]), scenes.synthetic_camera(w, h)


def miss(w, h):
    """No sphere around the camera: above the horizon a pixel hits one of three small spheres or nothing (the background)."""
    balls = [_ball(x, y, z, r, (0.9 - 0.3 * i, 0.4, 0.2 + 0.3 * i)) for i, (x, y, z, r) in enumerate(_spots(w, h, 3))]
    return _world(balls + [_ground()]), scenes.synthetic_camera(w, h)


def patterned_sphere(w, h):
    """A checkered sphere (its (u, v) goes through atan2 / acos: the remainder) on the checkered ground under the sky."""
    check = hm.CheckeredPigment(hm.Color(0.8, 0.7, 0.1), hm.Color(0.1, 0.1, 0.6), 6)
    ball = hm.Sphere(hm.translation(hm.Vec(2.0, 0.0, 0.9)) * hm.scaling(hm.Vec(0.8, 0.8, 0.8)),
                     hm.Material(hm.DiffuseBRDF(check), hm.UniformPigment(hm.Color(0.05, 0.05, 0.05))))
    return _world([_sky(), ball] + _behind()[:1] + [_ground()]), scenes.synthetic_camera(w, h)


BIT_EXACT = {"one_winner": one_winner, "horizon": horizon, "many_winners": many_winners, "remainder": remainder, "miss": miss}

_built = {}


def scene_and_camera(name: str, w: int, h: int):
    """(FlatScene, abi.Camera) of a world at a frame size (the small spheres follow the named tile), built once."""
    if (name, w, h) not in _built:
        world, cam = (patterned_sphere if name == "patterned_sphere" else BIT_EXACT[name])(w, h)
        _built[(name, w, h)] = (flatten.flatten_world(world), flatten.flatten_camera(cam))
    return _built[(name, w, h)]


def params(w: int, h: int, fmt=abi.OUT_F64, **kw) -> abi.Params:
    return abi.make_params(w, h, abi.RENDERER_FLAT, out_format=fmt, **kw)
