"""Worlds for the front end of pt_tile4_kernel: prologue, primary rays, cone, cull and the walk over a tile's survivors.

The four primary rays of a lane are made from quotients that the wave shares: one fp64 division per lane gives the sixteen
u = (column + 0.5) / W and the sixteen v-quotients of the tile, and every lane fetches its four.  What can go wrong there shows
at tiles that stick out of the frame (clamped columns and rows), at shares of a frame (a tile's global row is not its local
one) and wherever a tile's survivors are few, many or of mixed kinds.  Each builder returns (World, camera) for a frame size;
tests/test_tile4_front.py asserts from the oracle's hit records that a world shows what it is named for,
tests/test_gpu_tile4_front.py renders them.

No world has a patterned sphere: a plane's (u, v) is x - floor(x), so every frame can be demanded bit for bit.
"""
from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm
from tests import tile4_winners as tw

# one tile; lanes off the frame in three of four tiles; three tiles across, the middle column with d.y = 0 (a wave that is not
# `fast`); two workgroups each way whose right and lower tiles are partial (idle lanes stand on clamped pixels)
FRAMES = tw.FRAMES
named_tile, tile_of = tw.named_tile, tw.tile_of
COUNTS = (1, 63, 64, 65, 130)  # shapes: the lane clamp, one pass exactly, the pass boundary, a world too large to stage


def _uniform(r, g, b, emit=0.0) -> hm.Material:
    return hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(r, g, b))), hm.UniformPigment(hm.Color(emit, emit, emit)))


def _ball(x, y, z, rad, colour, turn=None) -> hm.Sphere:
    """A sphere of radius ``rad``; with ``turn`` (degrees) an ellipsoid turned about z, so that its inverse matrix is no
    scale + translate and it is queried through the full product."""
    t = hm.translation(hm.Vec(x, y, z))
    if turn is None:
        return hm.Sphere(t * hm.scaling(hm.Vec(rad, rad, rad)), _uniform(*colour))
    return hm.Sphere(t * hm.rotation_z(turn) * hm.scaling(hm.Vec(rad, 0.8 * rad, rad)), _uniform(*colour))


def _world(shapes) -> hm.World:
    w = hm.World()
    for s in shapes:
        w.add_shape(s)
    return w


def _grid(w: int, h: int, cols: int, rows: int):
    """(x, y, z, radius) of cols x rows small spheres four units in front of synthetic_camera, centred on the rays through
    pixel centres of the named tile: columns 1, 3, 5, ..., rows 1, 4, ... of the tile (above the horizon in every frame of
    FRAMES but for the one-tile frames, where the lower rows fall below it: no ground in these worlds), 0.8 pixel in
    angular radius."""
    tx, ty = named_tile(w, h)
    out = []
    for r in range(rows):
        for c in range(cols):
            col, row = tx * 16 + 1 + 2 * c, ty * 16 + 1 + 3 * r
            if col >= w or row >= h:
                continue
            dy, dz = (1.0 - 2.0 * (col + 0.5) / w) * (w / h), 1.0 - 2.0 * (row + 0.5) / h  # imagetracer.py:48-58, camera.py:103-124
            out.append((3.0, 4.0 * dy, 1.0 + 4.0 * dz, 4.0 * 1.6 / h))
    return out


def empty_beside_full(w, h):
    """(a) Twelve small spheres in the named tile and nothing else: tiles away from them have no survivor at all."""
    balls = [_ball(x, y, z, r, (0.1 + 0.07 * i, 0.9 - 0.07 * i, 0.4)) for i, (x, y, z, r) in enumerate(_grid(w, h, 6, 2))]
    return _world(balls + tw._behind()), scenes.synthetic_camera(w, h)


def one_survivor(w, h):
    """(b) The sphere around the camera and three spheres behind it: every tile has exactly one survivor, every pixel one winner."""
    return _world([tw._sky()] + tw._behind()), scenes.synthetic_camera(w, h)


def twelve_mixed(w, h):
    """(c) Twelve small spheres in the named tile, every other one a turned ellipsoid: both record forms among one tile's
    survivors, under the sphere around the camera."""
    balls = [_ball(x, y, z, r, (0.1 + 0.07 * i, 0.3, 0.9 - 0.07 * i), turn=(25.0 + 10.0 * i) if i % 2 else None)
             for i, (x, y, z, r) in enumerate(_grid(w, h, 6, 2))]
    return _world([tw._sky()] + balls), scenes.synthetic_camera(w, h)


def planes_only(w, h):
    """(d) Four planes and no sphere: ground, ceiling with a checker of its own, and two walls; the last slot is a plane."""
    ceiling = hm.Plane(hm.translation(hm.Vec(0.0, 0.0, 3.0)),
                       hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.9, 0.8, 0.1), hm.Color(0.1, 0.1, 0.7), 3)),
                                   hm.UniformPigment(hm.BLACK)))
    left = hm.Plane(hm.translation(hm.Vec(0.0, 4.13, 0.0)) * hm.rotation_x(90.0), _uniform(0.7, 0.2, 0.2))
    far = hm.Plane(hm.translation(hm.Vec(9.0, 0.37, 0.21)) * hm.rotation_y(90.0), _uniform(0.2, 0.7, 0.3, emit=0.1))
    return _world([tw._ground(), ceiling, left, far]), scenes.synthetic_camera(w, h)


def counted(n: int):
    """(e) builder of a world with exactly ``n`` shapes: the generator's spheres (the first is the one around the camera)."""
    def build(w, h):
        world = scenes.synthetic_world(n)
        assert len(world.shapes) == n, len(world.shapes)
        return world, scenes.synthetic_camera(w, h)
    build.__name__ = f"counted_{n}"
    return build


def inside_two(w, h):
    """(g) The camera inside two spheres: deep inside the large one (hoisted c = |o'|^2 - 1 near -1, below -0.5: no first-root
    division) and close to the wall of a smaller one (the rays start at (-2, 0, 1), 1.6 radii of 2 from its centre:
    c = -0.36, both roots); the small spheres lie behind that wall and are queried without winning."""
    cam = scenes.synthetic_camera(w, h)
    near_wall = hm.Sphere(hm.translation(hm.Vec(-0.4, 0.0, 1.0)) * hm.scaling(hm.Vec(2.0, 2.0, 2.0)), _uniform(0.3, 0.6, 0.9, emit=0.2))
    balls = [_ball(x, y, z, r, (0.8, 0.2 + 0.1 * i, 0.1)) for i, (x, y, z, r) in enumerate(_grid(w, h, 3, 1))]
    return _world([tw._sky(), near_wall] + balls), cam


def ortho(w, h):
    """An orthogonal camera over the ground and a few spheres (the planner decides which kernel renders it)."""
    cam = hm.OrthogonalCamera(w / h, hm.translation(hm.Vec(-1.0, 0.0, 1.0)))
    balls = [_ball(2.0, -0.6 + 0.6 * i, 0.5 + 0.3 * i, 0.25, (0.2 + 0.3 * i, 0.5, 0.7)) for i in range(3)]
    return _world(balls + [tw._ground()]), cam


WORLDS = {"empty_beside_full": empty_beside_full, "one_survivor": one_survivor, "twelve_mixed": twelve_mixed,
          "planes_only": planes_only, "inside_two": inside_two, "horizon": tw.horizon}
WORLDS.update({f"counted_{n}": counted(n) for n in COUNTS})

_built = {}


def scene_and_camera(name: str, w: int, h: int):
    """(FlatScene, abi.Camera) of a world at a frame size, built once."""
    if (name, w, h) not in _built:
        world, cam = (ortho if name == "ortho" else WORLDS[name])(w, h)
        _built[(name, w, h)] = (flatten.flatten_world(world), flatten.flatten_camera(cam))
    return _built[(name, w, h)]


def moved_camera(w: int, h: int, k: int) -> abi.Camera:
    """synthetic_camera moved and turned a little, differently for every k (k = 0: the camera itself)."""
    if k == 0:
        return flatten.flatten_camera(scenes.synthetic_camera(w, h))
    t = hm.translation(hm.Vec(-1.0 + 0.3 * k, 0.2 * k, 1.0 + 0.1 * k)) * hm.rotation_z(7.0 * k)
    return flatten.flatten_camera(hm.PerspectiveCamera(1.0, w / h, t))


def params(w: int, h: int, fmt=abi.OUT_F64, renderer=abi.RENDERER_FLAT, **kw) -> abi.Params:
    return abi.make_params(w, h, renderer, out_format=fmt, **kw)
