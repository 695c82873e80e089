"""Worlds for the survivor loop and the stores of pt_tile4_kernel (tests/test_gpu_tile4_straight.py), seen through
``scenes.synthetic_camera`` (the rays start at (-2, 0, 1) and run towards +x) in frames of 16x16 (one full tile), 17x17 and 33x17
pixels (partial tiles with idle lanes to the right and below).

Every world is the sphere around the camera (hoisted ``c`` far below -0.5), a ground plane, and what it is named for:

``never-hit``   a sphere of radius 0.01 near the frame's centre, 0.03 from the nearest pixel's ray in all three frames: the
                tile's cone keeps it and no ray meets it; beside it a sphere that only some lanes of a tile meet.
``inside``      a second sphere around the camera whose hoisted ``c`` lies in (-0.5, 0): its first root is computed and rejected
                by every lane, the second taken.
``ties``        two coincident spheres and two coincident planes; ``ties-swapped`` lists each pair the other way round.  The
                first of a pair in ``World.shapes`` must win every pixel the pair wins (world.py:62, a strict <).
``planes``      a plane 1e-4 below the camera's eye, seen edge-on (``|dz|`` of its object-space ray is below 1e-5 for the lanes
                of one image row and above for the others), and a plane behind the camera (every t negative).
``checkered``   a checkered sphere: the per-pixel remainder behind the shading loop (libm: held to a tolerance).
``n65``, ``n130``  65 and 130 shapes (the unstaged variant, passes 1 and 2 of the cull): slot 64 and slot 128 hold the spheres
                that are seen, the slots in front of them hold spheres behind the camera.

tests/test_tile4_straight.py shows on the CPU, from the oracle's hit records, that each frame holds what its world is for.
"""
from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm

FRAMES = ((16, 16), (17, 17), (33, 17))
WORLDS = ("never-hit", "inside", "ties", "ties-swapped", "planes", "checkered", "n65", "n130")
EYE = (-2.0, 0.0, 1.0)  # where scenes.synthetic_camera's rays start


def _uniform(r, g, b, emit=0.5):
    return hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(r, g, b))), hm.UniformPigment(hm.Color(emit * r, emit * g, emit * b)))


def _ball(x, y, z, rad, mat):
    return hm.Sphere(hm.translation(hm.Vec(x, y, z)) * hm.scaling(hm.Vec(rad, rad, rad)), mat)


def _sky():
    return hm.Sphere(hm.scaling(hm.Vec(50.0, 50.0, 50.0)), _uniform(0.05, 0.1, 0.15, 2.0))


def _ground():
    return hm.Plane(hm.Transformation(), hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.3, 0.5, 0.1), hm.Color(0.1, 0.2, 0.5), 4)),
                                                      hm.UniformPigment(hm.Color(0.01, 0.02, 0.03))))


# names of the shapes the CPU test asks about -> index in World.shapes
def shapes(name: str):
    """(list of shapes in World.shapes order, {role: index})."""
    sky, ground = _sky(), _ground()
    if name == "never-hit":
        tiny = _ball(-1.0, 0.031, 1.047, 0.01, _uniform(0.9, 0.1, 0.1))
        some = _ball(-0.5, 0.45, 1.3, 0.25, _uniform(0.2, 0.8, 0.3))
        return [sky, tiny, some, ground], {"tiny": 1, "some": 2}
    if name == "inside":
        # about the world's origin, the eye at distance sqrt(5): c = 5 / 2.6^2 - 1 = -0.26
        near = hm.Sphere(hm.scaling(hm.Vec(2.6, 2.6, 2.6)), _uniform(0.6, 0.5, 0.9))
        return [sky, near, _ball(-1.0, 0.1, 1.1, 0.1, _uniform(0.8, 0.3, 0.2)), ground], {"near": 1}
    if name in ("ties", "ties-swapped"):
        a, b = _ball(0.0, 0.3, 1.2, 0.5, _uniform(0.9, 0.2, 0.1)), _ball(0.0, 0.3, 1.2, 0.5, _uniform(0.1, 0.2, 0.9))
        pa = hm.Plane(hm.Transformation(), _uniform(0.3, 0.6, 0.2))
        pb = hm.Plane(hm.Transformation(), _uniform(0.6, 0.3, 0.7))
        if name == "ties-swapped":
            a, b, pa, pb = b, a, pb, pa
        return [sky, a, b, pa, pb], {"first_sphere": 1, "second_sphere": 2, "first_plane": 3, "second_plane": 4}
    if name == "planes":
        # the plane z = 1 - 1e-4 passes just below the eye: the image row whose rays have d.z = 0 (odd heights) sees it edge-on,
        # the rows that look down meet it in front of everything else
        edge = hm.Plane(hm.translation(hm.Vec(0.0, 0.0, 1.0 - 1e-4)), _uniform(0.7, 0.7, 0.1))
        # the plane x = -3, behind the eye
        behind = hm.Plane(hm.translation(hm.Vec(-3.0, 0.0, 0.0)) * hm.rotation_y(90.0), _uniform(0.1, 0.7, 0.7))
        return [sky, _ball(-0.5, -0.3, 1.4, 0.2, _uniform(0.8, 0.3, 0.2)), edge, behind, ground], {"edge": 2, "behind": 3}
    if name == "checkered":
        check = hm.Material(hm.DiffuseBRDF(hm.CheckeredPigment(hm.Color(0.8, 0.7, 0.1), hm.Color(0.1, 0.1, 0.6), 6)),
                            hm.UniformPigment(hm.Color(0.05, 0.05, 0.05)))
        return [sky, _ball(-0.6, 0.1, 1.1, 0.45, check), _ball(-1.0, -0.5, 0.7, 0.1, _uniform(0.8, 0.3, 0.2)), ground], {"ball": 1}
    n = {"n65": 65, "n130": 130}[name]

    def fillers(k):  # behind the eye: culled by every tile's cone
        return [_ball(-6.0 - 0.01 * i, 0.02 * (i % 7), 1.0, 0.05, _uniform(0.5, 0.5, 0.5)) for i in range(k)]

    out = [sky] + fillers(63) + [_ball(-0.8, 0.2, 1.2, 0.3, _uniform(0.9, 0.4, 0.1))]  # slot 64: the first of pass 1
    roles = {"seen64": 64}
    if n == 130:
        out += fillers(63) + [_ball(-0.9, -0.3, 0.8, 0.2, _uniform(0.2, 0.9, 0.4)), ground]  # slot 128: the first of pass 2
        roles["seen128"] = 128
    assert len(out) == n
    return out, roles


_built = {}


def scene(name: str):
    """(FlatScene, {role: index}), built once."""
    if name not in _built:
        w = hm.World()
        sh, roles = shapes(name)
        for s in sh:
            w.add_shape(s)
        _built[name] = (flatten.flatten_world(w), roles)
    return _built[name]


def camera(W: int, H: int):
    return flatten.flatten_camera(scenes.synthetic_camera(W, H))


def params(W: int, H: int, renderer=abi.RENDERER_FLAT, fmt=abi.OUT_F64) -> abi.Params:
    return abi.make_params(W, H, renderer, out_format=fmt)
