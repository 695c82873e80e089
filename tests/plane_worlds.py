"""A third scene source: worlds whose shapes are mostly PLANES, and worlds with dozens of lights.

The planner (csrc/pt_plan.h) decides from ``n_shapes``; the kernels split the same tables by ``n_spheres`` (``slot >=
a.n_spheres`` is a plane: ``plane_keeps`` instead of ``cone_keeps``, no bounding ball, never in the grid).  Every other
generator of the suite draws ``n_shapes ~ n_spheres`` and at most seven lights.  ``plane_world`` varies the mix:

* the base world is a convex room around the camera: plane k is ``R_k * translation(0, 0, -d_k)`` (times an in-plane shear in
  the "sheared" flavour), its normal side towards the camera, ``d_k`` within ``ROOM * (1 + 0.5 / n)`` of each other so that
  nearly every plane is a facet; the normals of all planes but the closing four pass through the cells of a grid over the
  screen, so that the facets are IN the picture;
* flavours:

  - ``closed``: four planes of a tetrahedron first, so every ray hits something; plane 1 emits: the sky;
  - ``fan``: planes below and in front only: sky pixels;
  - ``horizon``: planes whose normals are nearly square to the view axis, all around it: the sky is a polygon in the middle
    of the picture, each edge the horizon of a plane at another angle, so that tiles straddle a horizon with one, two or
    three corners on the plane's side;
  - ``sheared``: closed; ``scaling * rotation_z * scaling`` on every plane, z scaled too: row 2 of ``invm`` is no unit vector;
  - ``plain``: closed; uniform pigments, no specular surface: nothing on a primary or shadow ray's way needs libm, and a
    path has no checker cell a last-bit difference could flip;
* spheres go inside the room, by thirds scale+translate only (uniform), scale+translate only (three factors) and rotated
  ellipsoids: all three record groups ``[scale+translate spheres | other spheres | planes]`` are populated; the list order
  interleaves spheres and planes evenly, so planes are not last and ``recs[].index != slot``;
* the room's centre (and with it the perspective camera's origin) is the world's origin, or ``centre``: with the room away from
  the origin ``invm[11]`` of a plane is no longer its distance from the camera and takes either sign;
* lights: the first inside the room, the second exactly ON a plane, the third outside the room (beyond two planes: shadowed
  for every point of the picture), the others inside; ``linear_radius`` alternately 0 and positive.

``constructed_world`` holds what chance does not give: two coincident planes with different materials at list positions
``i < j`` with spheres and planes between them (world.py's strict ``<``: position i wins every pixel), a plane through the
camera's origin and a plane parallel to the view axis.

Everything is drawn from ``hostmodel.PCG(9000 + seed, 301 + index of the flavour)`` in one fixed order through a *kit* of
constructors (tests/scene_families.py): ``HOST`` here, the reference's own classes in tests/golden/make_golden.py.

``CASES`` are ``(n_spheres, n_planes)`` pairs read off the planner's rules, each with the kernels every frame of it must plan
(tests/test_plane_worlds.py checks them on the CPU; tests/test_gpu_plane_worlds.py renders them).

A plain helper module: no fixtures, no hooks.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Tuple

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from tests.scene_families import HOST

FLAVOURS = ("closed", "fan", "sheared", "plain", "horizon")
SCREEN_DISTANCE = 0.6   # a wide view: +-70 degrees by +-59
ASPECT = 1.7            # the screen the facets are spread over (the frames' own aspect ratios are 1.6 to 1.8)


def _unit(v):
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / n, v[1] / n, v[2] / n)


def _apply(m, p, w=1.0):
    return tuple(m[i][0] * p[0] + m[i][1] * p[1] + m[i][2] * p[2] + m[i][3] * w for i in range(3))


CENTRE = (12.0, -7.0, 5.0)  # the room's centre of the cases that are not built around the world's origin


def view_rotation(seed, kit=None):
    """The cameras' rotation: camera space -> world (both cameras of a seed look the same way)."""
    K = kit or HOST
    g = hm.PCG(9000 + seed, 300)
    return K.rotation_z(30.0 * (g.random_float() - 0.5)) * K.rotation_y(14.0 * (g.random_float() - 0.5))


def cameras(seed, size, kit=None, centre=(0.0, 0.0, 0.0)):
    """-> (perspective, orthogonal).  The perspective camera's rays start at ``centre`` (at the world's origin exactly:
    M * (-d, 0, 0) with M = R * translation(d, 0, 0)); the orthogonal camera's start within 2.3 of it: inside every room
    (ROOM >= 3)."""
    K = kit or HOST
    rot = view_rotation(seed, K)
    if any(centre):
        rot = K.translation(K.Vec(*centre)) * rot
    W, H = size
    return (K.PerspectiveCamera(SCREEN_DISTANCE, W / H, rot * K.translation(K.Vec(SCREEN_DISTANCE, 0.0, 0.0))),
            K.OrthogonalCamera(W / H, rot))


def _towards(K, rot, n_c, spin):
    """The rotation that takes the plane's outward direction (0, 0, -1) to ``rot * n_c`` (``n_c``: a unit vector in camera
    space), after a turn of ``spin`` degrees in the plane."""
    az = math.degrees(math.atan2(n_c[1], n_c[0]))
    lat = math.atan2(n_c[2], math.hypot(n_c[0], n_c[1]))
    el = math.degrees(math.atan2(-math.cos(lat), -math.sin(lat)))  # rotation_y(el) * (0, 0, -1) = (cos lat, 0, sin lat)
    return rot * K.rotation_z(az) * K.rotation_y(el) * K.rotation_z(spin)


def plane_world(n_spheres, n_planes, n_lights, seed, flavour, kit=None, centre=(0.0, 0.0, 0.0)):
    """-> (world, info); info: ``plane_at`` / ``sphere_at`` list positions, ``room`` the least plane distance."""
    K = kit or HOST
    fi = FLAVOURS.index(flavour)
    g = hm.PCG(9000 + seed, 301 + fi)
    r = g.random_float
    V = K.Vec
    rot = view_rotation(seed, K)
    if any(centre):  # (camera space -> world: everything below is placed through this one transformation)
        rot = K.translation(V(*centre)) * rot
    plain, fan, sheared, horizon = flavour == "plain", flavour == "fan", flavour == "sheared", flavour == "horizon"
    room = 3.0 + r()
    black = K.Color(0.0, 0.0, 0.0)

    def colour(lo=0.05, hi=0.95):
        return K.Color(lo + (hi - lo) * r(), lo + (hi - lo) * r(), lo + (hi - lo) * r())

    def at(p_c, w=1.0):
        return _apply(rot.m, p_c, w)

    def material(patterned, sky=False):
        if sky:  # black BRDF pigment: a sample that ends here spawns nothing (the first pass settles such pixels)
            return K.Material(K.DiffuseBRDF(K.UniformPigment(black)), K.UniformPigment(colour(0.5, 1.0)))
        if patterned and not plain and r() < 0.5:
            pig = K.CheckeredPigment(colour(), colour(), 1 + int(11.999 * r()))
        else:
            pig = K.UniformPigment(colour())
        emit = K.UniformPigment(colour(0.0, 0.5) if r() < 0.25 else black)
        if not plain and r() < 0.2:
            return K.Material(K.SpecularBRDF(pig), emit)
        return K.Material(K.DiffuseBRDF(pig), emit)

    # ---- planes -------------------------------------------------------------------------------------------------------------
    n_closing = 0 if fan or horizon else min(4, n_planes)
    n_grid = n_planes - n_closing
    cols = max(1, int(math.ceil(math.sqrt(n_grid * ASPECT))))
    rows = max(1, (n_grid + cols - 1) // cols)
    spread = 0.5 / max(1, n_planes)  # d_k / room - 1: small against the squared angle between neighbouring normals
    phi0 = 360.0 * r()
    planes, normals, dists, transforms = [], [], [], []
    for k in range(n_planes):
        if k < n_closing:  # a tetrahedron: one face behind the camera, three around the view
            if k == 0:
                n_c = (-1.0, 0.0, 0.0)
            else:
                a = math.radians(phi0 + 120.0 * k)
                n_c = (1.0 / 3.0, math.sqrt(8.0) / 3.0 * math.cos(a), math.sqrt(8.0) / 3.0 * math.sin(a))
        else:
            j = k - n_closing
            sy = ASPECT * 0.95 * (2.0 * (j % cols + r()) / cols - 1.0)
            sz = 0.95 * (2.0 * (j // cols + r()) / rows - 1.0)
            if horizon:  # the horizon n . v = 0 crosses the picture 0.36 screen units from its middle, at the angle phi
                a = math.radians(phi0 + 360.0 * (j + 0.5 * r()) / n_planes)
                n_c = _unit((-SCREEN_DISTANCE, math.cos(a), math.sin(a)))
            elif fan:  # below and in front only: the upper rows of the picture see the sky
                n_c = _unit((SCREEN_DISTANCE, sy, -0.35 - 0.65 * abs(sz) - 0.5))
            else:
                n_c = _unit((SCREEN_DISTANCE, sy, sz))
        d = room * (1.0 + spread * r())
        t = _towards(K, rot, n_c, 360.0 * r()) * K.translation(V(0.0, 0.0, -d))
        if sheared:  # the plane z = 0 stays where it is; (u, v) are sheared, row 2 of invm is scaled
            t = t * K.scaling(V(0.4 + 2.0 * r(), 0.4 + 2.0 * r(), 1.0)) * K.rotation_z(360.0 * r()) * \
                K.scaling(V(0.3 + 1.2 * r(), 1.0 + 2.0 * r(), 0.25 + 3.0 * r() * r()))
        planes.append(K.Plane(t, material(True, sky=(k == 1 and n_closing == 4))))
        normals.append(_apply(rot.m, n_c, 0.0))
        dists.append(d)
        transforms.append(t)

    # ---- spheres: inside the ball of radius 0.8 room, in front of the camera ------------------------------------------------
    cover = min(0.12, math.sqrt(0.8 / (math.pi * max(1, n_spheres))))
    spheres = []
    for i in range(n_spheres):
        sy, sz = ASPECT * 0.9 * (2.0 * r() - 1.0), 0.9 * (2.0 * r() - 1.0)
        rho = 1.0 + (0.8 * room - 1.0) * r()
        u = _unit((SCREEN_DISTANCE, sy, sz))
        where = at((rho * u[0], rho * u[1], rho * u[2]))
        rad = rho * cover * (0.6 + 0.8 * r())
        t = K.translation(V(*where))
        if i % 3 == 0:
            t = t * K.scaling(V(rad, rad, rad))
        elif i % 3 == 1:
            t = t * K.scaling(V(rad, rad * (0.5 + 0.5 * r()), rad * (0.5 + 0.5 * r())))
        else:
            t = t * K.rotation_z(360.0 * r()) * K.rotation_y(360.0 * r()) * K.rotation_x(360.0 * r()) * \
                K.scaling(V(rad, rad * (0.4 + 0.6 * r()), rad * (0.4 + 0.6 * r())))
        spheres.append(K.Sphere(t, material(False)))

    # ---- the list: spheres and planes interleaved evenly --------------------------------------------------------------------
    keyed = sorted([((k + 0.5) / n_planes, 0, k) for k in range(n_planes)] + [((i + 0.5) / n_spheres, 1, i) for i in range(n_spheres)])
    world = K.World()
    plane_at, sphere_at = [0] * n_planes, [0] * n_spheres
    for pos, (_, is_sphere, k) in enumerate(keyed):
        world.add_shape(spheres[k] if is_sphere else planes[k])
        (sphere_at if is_sphere else plane_at)[k] = pos

    # ---- lights ---------------------------------------------------------------------------------------------------------------
    for k in range(n_lights):
        radius = 0.0 if k % 2 == 0 else 0.5 + 2.0 * r()
        if k == 1 and n_planes > 0:    # exactly on a plane, within its facet: the image of a point of z = 0
            reach = (0.25 if sheared else 1.0) * min(0.5, 1.5 / math.sqrt(n_planes))
            p = _apply(transforms[min(n_planes - 1, 4)].m, (reach * (r() - 0.5), reach * (r() - 0.5), 0.0))
        elif k == 2 and n_planes > 1:  # outside: beyond planes 0 and 1, so that a point ON one of them still has the other in the way
            s = _unit((normals[0][0] + normals[1][0], normals[0][1] + normals[1][1], normals[0][2] + normals[1][2]))
            p = (centre[0] + 4.0 * room * s[0], centre[1] + 4.0 * room * s[1], centre[2] + 4.0 * room * s[2])
        elif k == 2 and n_spheres > 0:  # (a single plane shadows no point of its own: the centre of the first sphere instead)
            p = _apply(spheres[0].transformation.m, (0.0, 0.0, 0.0))
        else:                          # inside
            u = _unit((0.2 + r(), 2.0 * (r() - 0.5), 1.6 * (r() - 0.3)))
            rho = room * (0.25 + 0.45 * r())
            p = at((rho * u[0], rho * u[1], rho * u[2]))
        world.add_light(K.PointLight(K.Point(*p), colour(0.2, 1.0), radius))
    return world, dict(plane_at=plane_at, sphere_at=sphere_at, room=room)


def constructed_world(kit=None, plain=False):
    """-> (world, info): an open room seen by ``cameras(CONSTRUCTED_SEED, ...)`` turned back to the axes (``info['cameras']``).

    list position  shape
    0              the floor, checkered
    1              the coincident pair's FIRST plane: a wall across the view, red, diffuse
    2, 3           a sphere, a rotated ellipsoid
    4              a plane THROUGH the camera's origin (o'.z == 0 exactly: t = -0 / d'.z is never beyond tmin)
    5              a sphere
    6              a wall PARALLEL to the view axis (d'.z == 0 exactly for the central column's rays at mid height)
    7              the pair's SECOND plane: the same transformation object, green, emitting
    8              the ceiling
    9              a scale+translate sphere in front of the pair
    """
    K = kit or HOST
    V, C = K.Vec, K.Color
    black = K.UniformPigment(C(0.0, 0.0, 0.0))

    def diffuse(pig, emit=None):
        return K.Material(K.DiffuseBRDF(pig), emit or black)

    pair_t = K.rotation_z(10.0) * K.rotation_y(-80.0) * K.translation(V(0.0, 0.0, -4.0))
    floor_pig = K.UniformPigment(C(0.3, 0.5, 0.1)) if plain else K.CheckeredPigment(C(0.3, 0.5, 0.1), C(0.1, 0.2, 0.5), 4)
    world = K.World()
    world.add_shape(K.Plane(K.translation(V(0.0, 0.0, -1.0)), diffuse(floor_pig)))
    world.add_shape(K.Plane(pair_t, diffuse(K.UniformPigment(C(0.9, 0.1, 0.1)))))
    world.add_shape(K.Sphere(K.translation(V(2.0, 1.0, -0.5)) * K.scaling(V(0.5, 0.5, 0.5)), diffuse(K.UniformPigment(C(0.2, 0.6, 0.9)))))
    world.add_shape(K.Sphere(K.translation(V(2.5, -1.2, 0.3)) * K.rotation_z(30.0) * K.rotation_x(20.0) * K.scaling(V(0.6, 0.3, 0.4)),
                             diffuse(K.UniformPigment(C(0.8, 0.7, 0.2)))))
    world.add_shape(K.Plane(K.rotation_x(75.0) * K.rotation_y(20.0), diffuse(K.UniformPigment(C(0.5, 0.5, 0.5)))))
    world.add_shape(K.Sphere(K.translation(V(1.5, 0.2, 0.6)) * K.scaling(V(0.2, 0.25, 0.2)),
                             diffuse(K.UniformPigment(C(0.1, 0.1, 0.1)), K.UniformPigment(C(0.4, 0.3, 0.1)))))
    world.add_shape(K.Plane(K.rotation_x(90.0) * K.translation(V(0.0, 0.0, -2.5)),
                            diffuse(K.UniformPigment(C(0.6, 0.6, 0.3)) if plain else K.CheckeredPigment(C(0.6, 0.6, 0.3), C(0.2, 0.1, 0.4), 3))))
    world.add_shape(K.Plane(pair_t, diffuse(K.UniformPigment(C(0.1, 0.9, 0.1)), K.UniformPigment(C(0.0, 0.5, 0.0)))))
    world.add_shape(K.Plane(K.rotation_x(180.0) * K.translation(V(0.0, 0.0, -2.0)),
                            diffuse(K.UniformPigment(C(0.0, 0.0, 0.0)), K.UniformPigment(C(0.6, 0.7, 1.0)))))
    world.add_shape(K.Sphere(K.translation(V(3.0, 0.3, 0.2)) * K.scaling(V(0.4, 0.4, 0.4)),
                             diffuse(K.UniformPigment(C(0.7, 0.3, 0.6))) if plain else
                             K.Material(K.SpecularBRDF(K.UniformPigment(C(0.7, 0.7, 0.6))), black)))
    world.add_light(K.PointLight(K.Point(1.0, -1.0, 1.5), C(1.0, 0.9, 0.8), 0.0))
    world.add_light(K.PointLight(K.Point(2.0, 2.0, 0.5), C(0.3, 0.4, 0.9), 1.5))
    return world, dict(pair=(1, 7), through_origin=4, parallel=6)


def constructed_cameras(size, kit=None):
    """Unturned cameras at the origin looking along x: the central ray of an odd-sized frame is (1, 0, 0) exactly."""
    K = kit or HOST
    W, H = size
    return (K.PerspectiveCamera(SCREEN_DISTANCE, W / H, K.translation(K.Vec(SCREEN_DISTANCE, 0.0, 0.0))),
            K.OrthogonalCamera(W / H, K.scaling(K.Vec(1.0, 1.0, 1.0))))


# ---- the frames of a case ---------------------------------------------------------------------------------------------------
ON, FL, PT, PL = abi.RENDERER_ONOFF, abi.RENDERER_FLAT, abi.RENDERER_PATHTRACER, abi.RENDERER_POINTLIGHT
C3 = dict(renderer=PT, samples_per_side=2, num_of_rays=1, max_depth=3, rr_limit=3, path_state=45, path_seq=54, pcg_mode=abi.PCG_PIXEL)
CLI = dict(C3, samples_per_side=1, num_of_rays=10)
CLI_SIZE = (40, 24)
CLI_MAX_SHAPES = 70
# frame -> (camera, abi.make_params keywords); "cli" is rendered at CLI_SIZE and only of worlds of at most CLI_MAX_SHAPES shapes
FRAMES = {
    "onoff": ("perspective", dict(renderer=ON)),
    "flat": ("perspective", dict(renderer=FL)),
    "flat-s2": ("perspective", dict(renderer=FL, samples_per_side=2, pcg_mode=abi.PCG_PIXEL, path_state=7, path_seq=11)),
    "pointlight": ("perspective", dict(renderer=PL)),
    "c3": ("perspective", C3),
    "cli": ("perspective", CLI),
    "ortho-flat": ("orthogonal", dict(renderer=FL)),
    "ortho-pointlight": ("orthogonal", dict(renderer=PL, samples_per_side=2, pcg_mode=abi.PCG_SAMPLE, path_state=3, path_seq=5)),
    "ortho-c3": ("orthogonal", dict(C3, samples_per_side=1, pcg_mode=abi.PCG_SAMPLE)),
}

# what the planner's rules give (csrc/pt_plan.h), spelled out once per class of world; (pre, first, main, alt) kernels
_S = lambda r, h: ("", "", f"pt_simple_kernel<{r}, {h}>", "")  # noqa: E731
_T = lambda r, tm="": ("", "", f"pt_tile_kernel<{r}{tm}>", "")  # noqa: E731
_H = lambda r: ("pt_cell_kernel", "", f"pt_tile_kernel<{r}, HIER>", "")  # noqa: E731
_T4 = lambda r, lds: ("", "", f"pt_tile4_kernel<{r}, {lds}>", "")  # noqa: E731
_LEAN = "pt_path_regions_kernel<LDS, SCENE, LEAN>"
_NOGRID = "pt_path_regions_kernel<LDS, NOGRID>"
_TREE = ("pt_path_tree_kernel<LEAN, SCENE>", "pt_path_flagged_kernel<LEAN, LDS>")


def _ortho(n_shapes, second):
    if n_shapes < 4:
        return {"ortho-flat": _S("FLAT", "noHOIST"), "ortho-pointlight": _S("POINTLIGHT", "noHOIST"),
                "ortho-c3": ("", "pt_tile_kernel<PATHTRACER, ORTHO>", second, "")}
    return {"ortho-flat": _T("FLAT", ", ORTHO"), "ortho-pointlight": _T("POINTLIGHT", ", ORTHO"),
            "ortho-c3": ("", "pt_tile_kernel<PATHTRACER, ORTHO>", second, "")}


def _fewer_than_four():
    """n_shapes < 4: one lane per pixel for the primary-ray renderers; the path tracer's passes need only a shape."""
    return dict({"onoff": _S("ONOFF", "HOIST"), "flat": _S("FLAT", "HOIST"), "flat-s2": _S("FLAT", "HOIST"),
                 "pointlight": _S("POINTLIGHT", "HOIST"), "c3": ("", "pt_tile_kernel<PATHTRACER>", _LEAN, ""),
                 "cli": ("", "pt_tile_kernel<PATHTRACER>") + _TREE, "hits": ("", "", "pt_hits_kernel<noCULL>", "")}, **_ortho(3, _LEAN))


def _one_pass(n_shapes=4):
    """4 .. 64 shapes: 16x16 tiles for pixel-centre OnOff / Flat (the records staged: 64 x 384 B = 24 KB at most), 8x8 tiles
    otherwise; one 64-slot pass; the second pass stages the scene."""
    return dict({"onoff": _T4("ONOFF", "noLDS"), "flat": _T4("FLAT", "LDS"), "flat-s2": _T("FLAT"), "pointlight": _T("POINTLIGHT"),
                 "c3": ("", "pt_tile_kernel<PATHTRACER>", _LEAN, ""), "cli": ("", "pt_tile_kernel<PATHTRACER>") + _TREE,
                 "hits": ("", "", "pt_hits_kernel", "")}, **_ortho(n_shapes, _LEAN))


def _two_passes():
    """65 shapes: two 64-slot passes (the first pass by BLOCKS at these frame sizes), 65 x 384 B no longer staged for tile4."""
    return dict(_one_pass(65), flat=_T4("FLAT", "noLDS"), c3=("", "pt_tile_kernel<PATHTRACER, BLOCKS>", _LEAN, ""),
                cli=("", "pt_tile_kernel<PATHTRACER, BLOCKS>") + _TREE)


def _up_to_256(n_shapes):
    """117 .. 256 shapes: still 16x16 tiles, the scene's records no longer fit behind the second pass's frames."""
    d = dict(_two_passes(), c3=("", "pt_tile_kernel<PATHTRACER, BLOCKS>", _NOGRID, ""), **_ortho(n_shapes, _NOGRID))
    del d["cli"]
    return d


def _cell_lists(second=_NOGRID):
    """More than hier_min = 256 shapes: pt_cell_kernel, then HIER tiles (never with an orthogonal camera, never tile4)."""
    return dict({"onoff": _H("ONOFF"), "flat": _H("FLAT"), "flat-s2": _H("FLAT"), "pointlight": _H("POINTLIGHT"),
                 "c3": ("pt_cell_kernel", "pt_tile_kernel<PATHTRACER, HIER>", second, ""),
                 "hits": ("pt_cell_kernel", "", "pt_hits_kernel<HIER>", "")}, **_ortho(257, second))


@dataclass(frozen=True)
class Case:
    id: str
    n_spheres: int
    n_planes: int
    flavour: str
    size: Tuple[int, int]
    kernels: Dict[str, Tuple[str, str, str, str]]  # frame (FRAMES' keys, "hits") -> (pre, first, main, alt) kernel
    n_lights: int = 4
    seed: int = 0
    ball_levels: int = 0  # the ball hierarchy is consulted (n_spheres >= 128)
    has_grid: int = 0
    centre: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    @property
    def n_shapes(self):
        return self.n_spheres + self.n_planes


CASES = [
    # ---- the 4-shape threshold ----------------------------------------------------------------------------------------------
    Case("s0-p3", 0, 3, "closed", (43, 27), _fewer_than_four(), seed=1),
    Case("s0-p4", 0, 4, "closed", (45, 25), _one_pass(), seed=2),
    Case("s1-p3", 1, 3, "plain", (41, 27), _one_pass(), seed=3),
    # ---- the boundaries of a 64-slot pass: all planes, planes only in the second pass, a pass that straddles the groups ----
    Case("s0-p64", 0, 64, "closed", (75, 45), _one_pass(64), seed=4),
    Case("s0-p65", 0, 65, "closed", (101, 57), _two_passes(), seed=5, centre=CENTRE),
    Case("s60-p5", 60, 5, "fan", (99, 59), _two_passes(), n_lights=9, seed=6, centre=CENTRE),
    Case("s63-p2", 63, 2, "fan", (97, 55), _two_passes(), seed=7),
    Case("s64-p1", 64, 1, "fan", (93, 53), _two_passes(), seed=8),
    # ---- horizons at many angles across the picture: tiles with one, two, three corners on a plane's side ---------------
    Case("s2-p7", 2, 7, "horizon", (101, 59), _one_pass(9), seed=17),
    # ---- the tile4 limit and hier_min ---------------------------------------------------------------------------------------
    Case("s0-p256", 0, 256, "plain", (101, 57), _up_to_256(256), seed=9),
    Case("s0-p257", 0, 257, "closed", (103, 59), _cell_lists(), seed=10, centre=CENTRE),
    Case("s1-p256", 1, 256, "sheared", (99, 57), _cell_lists(), seed=11),
    Case("s100-p200", 100, 200, "closed", (102, 58), _cell_lists(), seed=12, centre=CENTRE),  # (HIER without the ball hierarchy)
    # ---- the ball hierarchy (n_spheres >= 128) without and with HIER ------------------------------------------------------
    Case("s128-p10", 128, 10, "sheared", (101, 57), _up_to_256(138), seed=13, ball_levels=1),
    Case("s127-p130", 127, 130, "closed", (97, 59), _cell_lists(), seed=14),
    Case("s128-p129", 128, 129, "plain", (103, 57), _cell_lists(), seed=15, ball_levels=1),
    # ---- the uniform grid (>= 1024 ordinary spheres) --------------------------------------------------------------------------
    Case("s1100-p40", 1100, 40, "closed", (95, 53), _cell_lists("pt_path_regions_kernel<LDS>"), seed=16, ball_levels=1, has_grid=1, centre=CENTRE),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
PASS_BOUNDARY = ("s0-p64", "s0-p65", "s60-p5", "s63-p2", "s64-p1")
HIT_CASES = ("s0-p65", "s0-p257", "s60-p5")
QUERY_CASES = ("s0-p65", "s100-p200", "s1100-p40")
# path-traced frames that must have NO outlier: uniform pigments only ("plain"), rr_limit > max_depth; one per kernel family
# (regions with the scene staged, regions without, HIER first pass, tree + flagged)
STRICT_PATH = {"s1-p3": ("c3", "cli"), "s0-p256": ("c3",), "s128-p129": ("c3",)}
STRICT = dict(rr_limit=4)

# the three worlds the reference itself rendered into tests/golden/g13_planes_<name>.npz
GOLDEN = {"closed": "s0-p65", "fan": "s60-p5", "coincident": None}
GOLDEN_SIZE = (24, 16)

LIGHT_COUNTS = (1, 8, 33, 64, 65)
LIGHT_WORLDS = ((0, 6), (20, 6))
LIGHT_SIZE = (43, 27)


def case_world(case, kit=None):
    return plane_world(case.n_spheres, case.n_planes, case.n_lights, case.seed, case.flavour, kit, case.centre)


def case_cameras(case, size, kit=None):
    return cameras(case.seed, size, kit, case.centre)


def light_world(n_spheres, n_planes, n_lights, flavour, kit=None):
    """The lights worlds: "plain" (no specular surface: PointLight frames are bit-exact) or "closed" (specular ``eval``)."""
    return plane_world(n_spheres, n_planes, n_lights, 40 + n_spheres, flavour, kit)


def frame_params(frame, size, **more):
    kw = dict(FRAMES[frame][1], **more)
    W, H = CLI_SIZE if frame == "cli" else size
    return abi.make_params(W, H, kw.pop("renderer"), **kw)


def frames_of(case):
    return [f for f in FRAMES if f in case.kernels]
