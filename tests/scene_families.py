"""A second scene source: small mixed scenes that each open ONE axis the other generators never draw.

``scenes.synthetic_world``, ``scenes.demo_world``, the variant catalogue's gallery and ``_random_world`` of
tests/test_gpu_parity.py only ever scale shapes by positive factors under ``translation * rotation * scaling``, only ever
give a perspective camera a rigid transformation and a screen distance of order one, give random spheres uniform pigments
and a world one or two lights.  The reference accepts much more, and the kernels' fast paths (the scale+translate sphere
records, the hoisted origins, the culling cones and radii, ``plane_keeps``, the texel clamp) see those inputs as
arguments nobody has fed them.  ``family_world(family, seed)`` draws them:

=========  =====================================================================================================
mirrored   spheres and planes scaled by one, two or three negative factors; the spheres by thirds scale+translate only
           (the diag fast path), ``translation * rotation * scaling`` and ``translation * scaling * rotation``
sheared    ``scaling * rotation * scaling`` on spheres and planes (condition numbers up to about 50), with checkered and
           image pigments on them, so that (u, v) and the normals both matter
camera     perspective cameras under ``translation * rotation * scaling(a, b, c)``, factors of 0.2 to 5 of either sign,
           screen distances of 0.02 to 50, aspect ratios of 1:8 to 8:1, cameras inside a small sphere; orthogonal cameras
           with mirrored scalings
pigments   every shape with a checkered or image BRDF pigment, half of them with a checkered or image emitted pigment
           too; steps of 1 to 200; six textures a world (1x1, 1x7, 6x1, 2x2, 5x3, 64x64)
lights     zero to six lights: inside spheres, behind planes, 1e4 away; ``linear_radius`` zero or positive; specular
           shapes with thresholds of 0 to pi
mixed      all of the above at once
=========  =====================================================================================================

The scene is a few dozen spheres, one to three planes and sometimes a dome; frames are at most 123 x 104 and off the 8 / 16
grid of the tiles, so the oracle renders one in a second or two.

What the generator avoids, because the reference itself cannot render it and there is nothing to be faithful to: singular
matrices (every scale factor is at least 0.1 in magnitude, so ``scaling`` never divides by zero and every composite is
invertible), a light placed exactly on a surface (lights inside a sphere sit within 0.05 radii of its centre, lights behind
a plane a whole unit off it: ``is_point_visible`` of a point ON a surface is decided by rounding alone), and non-finite
values (the largest coordinate is 1e4).

Everything is drawn from ``hostmodel.PCG(7000 + seed, 101 + index of the family)`` in one fixed order, and the objects are
built through a *kit* of constructors: ``HOST`` (pytracer_amd.hostmodel, the default) here, the reference's own classes in
tests/golden/make_golden.py -- one recipe, two sets of classes, the same flattened scene bit for bit.

A plain helper module: no fixtures, no hooks.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

from pytracer_amd import hostmodel as hm

FAMILIES = ("mirrored", "sheared", "camera", "pigments", "lights", "mixed")
HIT_FAMILIES = ("mirrored", "sheared", "camera")  # (families whose hit-record frames the GPU suite compares)
# the seed of each family whose frames the reference itself rendered into tests/golden/g12_family_<family>.npz
GOLDEN_SEEDS = {"mirrored": 0, "sheared": 1, "camera": 3, "pigments": 1, "lights": 3, "mixed": 4}
GOLDEN_SIZE = (32, 20)

SIZES = [(123, 77), (97, 61), (75, 45), (109, 67), (51, 77), (117, 29)]
# the camera families: a tiny frame whose tiles span almost a half space at screen distance 0.02, 8:1, 1:8
WILD_SIZES = [(24, 15), (123, 15), (97, 61), (13, 104), (75, 45), (61, 37)]
TEXTURE_SIZES = [(1, 1), (1, 7), (6, 1), (2, 2), (5, 3), (64, 64)]


def _host_image(w, h, rgb):
    img = hm.HdrImage(w, h)
    img.pixels = [hm.Color(*c) for c in rgb]
    return img


HOST = SimpleNamespace(
    Vec=hm.Vec, Point=hm.Point, Color=hm.Color, translation=hm.translation, scaling=hm.scaling, rotation_x=hm.rotation_x,
    rotation_y=hm.rotation_y, rotation_z=hm.rotation_z, UniformPigment=hm.UniformPigment, CheckeredPigment=hm.CheckeredPigment,
    ImagePigment=hm.ImagePigment, DiffuseBRDF=hm.DiffuseBRDF, SpecularBRDF=hm.SpecularBRDF, Material=hm.Material,
    Sphere=hm.Sphere, Plane=hm.Plane, PointLight=hm.PointLight, World=hm.World, PerspectiveCamera=hm.PerspectiveCamera,
    OrthogonalCamera=hm.OrthogonalCamera, image=_host_image)


def texture_pixels(w, h, k):
    """Texel colours by formula (a few dozen distinct values: the fixtures that carry them stay small)."""
    return [(((5 * x + 3 * y + k) % 17) / 16.0, ((x + 2 * y + 3 * k) % 11) / 10.0, ((3 * x + y + k) % 7) / 6.0)
            for y in range(h) for x in range(w)]


def family_world(family, seed, kit=None):
    """-> (world, camera, W, H), built from the constructors of ``kit``."""
    K = kit or HOST
    fi = FAMILIES.index(family)
    g = hm.PCG(7000 + seed, 101 + fi)
    r = g.random_float
    V = K.Vec
    mixed = family == "mixed"
    mirrored, sheared = family == "mirrored" or mixed, family == "sheared" or mixed
    wild = family == "camera" or mixed
    patterned = family in ("pigments", "sheared") or mixed
    many_lights = family == "lights" or mixed

    def sign():
        return -1.0 if r() < 0.5 else 1.0

    def rot():
        return K.rotation_z(360.0 * r()) * K.rotation_y(360.0 * r()) * K.rotation_x(360.0 * r())

    def signs3():
        """One, two or three negative factors."""
        s = [1.0, 1.0, 1.0]
        n_neg = 1 + int(2.999 * r())
        first = int(2.999 * r())
        for k in range(n_neg):
            s[(first + k) % 3] = -1.0
        return s

    # ---- the camera: where it is decides where the shapes go ------------------------------------------------------------
    case = seed % 6
    enclosed = seam = ortho = False
    if not wild:
        W, H = SIZES[(seed + fi) % len(SIZES)]
        pos = (-1.0 - 2.0 * r(), r() - 0.5, 0.5 + r())
        cam_t = K.translation(V(*pos)) * K.rotation_z(40.0 * (r() - 0.5)) * K.rotation_y(24.0 * (r() - 0.3))
        seam = family == "pigments" and seed % 3 == 1
        if seam:  # (an unturned camera in the plane y = 0: the central ray runs along x exactly, see the seam sphere below)
            pos = (pos[0], 0.0, pos[2])
            cam_t = K.translation(V(*pos))
        camera = K.PerspectiveCamera(0.6 + 1.4 * r(), W / H, cam_t)
        origin = pos
    else:
        W, H = WILD_SIZES[case]
        pos = (2.0 * (r() - 0.5), 2.0 * (r() - 0.5), 1.0 + r())
        ortho = case in (2, 5)
        enclosed = case in (1, 5)
        if ortho:
            dist = 1.0
            s = signs3()
            if s[0] * s[1] * s[2] > 0.0:  # (mirrored: an odd number of negative factors)
                s[0] = -s[0]
            a, b, c = s[0] * (0.5 + 1.5 * r()), s[1] * (2.0 + 3.0 * r()) * H / max(W, H), s[2] * (2.0 + 3.0 * r())
        else:
            if mixed:
                dist = 0.02 * math.pow(2500.0, r())
            else:
                dist = (0.02, 50.0, 0.0, 0.05 * (0.4 + 0.6 * r()), 20.0 + 30.0 * r(), 0.0)[case]
            if case == 0:  # a very wide view: the directions of one tile span almost a half space
                a, b, c = sign() * (0.5 + 1.5 * r()), sign() * (0.5 + 1.5 * r()), sign() * (0.5 + 1.5 * r())
            else:          # factors that bring the view back to tan(half angle) of 0.5 .. 2
                a = min(5.0, max(0.2, (0.3 + 1.2 * r()) / dist))
                b = sign() * min(5.0, max(0.2, a * dist * (0.5 + 1.5 * r()) * min(1.0, H / W)))
                c = sign() * min(5.0, max(0.2, a * dist * (0.5 + 1.5 * r()) * min(1.0, H / W)))
                a *= sign()
        cam_t = K.translation(V(*pos)) * rot() * K.scaling(V(a, b, c))
        camera = K.OrthogonalCamera(W / H, cam_t) if ortho else K.PerspectiveCamera(dist, W / H, cam_t)
        # the point the rays (of the central pixel) start from: M * (-dist, 0, 0)
        m = cam_t.m
        origin = tuple(m[i][0] * -dist + m[i][3] for i in range(3))

    world = K.World()

    # ---- pigments and materials -------------------------------------------------------------------------------------------
    textures = []
    if patterned:
        for k, (tw, th) in enumerate(TEXTURE_SIZES):
            textures.append(K.image(tw, th, texture_pixels(tw, th, k + seed)))
    n_tex = [0]

    def colour(lo=0.05, hi=0.95):
        return K.Color(lo + (hi - lo) * r(), lo + (hi - lo) * r(), lo + (hi - lo) * r())

    def pattern(dim=1.0):
        if r() < 0.5:
            c1, c2 = colour(0.05 * dim, 0.95 * dim), colour(0.05 * dim, 0.95 * dim)
            return K.CheckeredPigment(c1, c2, 1 + int(199.999 * r() * r() * r()))
        n_tex[0] += 1
        return K.ImagePigment(textures[(n_tex[0] - 1) % len(textures)])

    def material():
        if patterned:
            pig = pattern()
            emit = pattern(0.5) if r() < 0.5 else K.UniformPigment(K.Color(0.0, 0.0, 0.0))
        else:
            pig = K.UniformPigment(colour())
            emit = K.UniformPigment(colour(0.0, 0.5) if r() < 0.3 else K.Color(0.0, 0.0, 0.0))
        if r() < 0.25:
            if many_lights:
                threshold = (0.0, math.pi, math.pi * r(), 0.3 * r())[int(3.999 * r())]
                return K.Material(K.SpecularBRDF(pig, threshold), emit)
            return K.Material(K.SpecularBRDF(pig), emit)
        return K.Material(K.DiffuseBRDF(pig), emit)

    # ---- a dome, sometimes; around a camera "inside a small sphere" always, and small ----------------------------------
    reach = 1.0
    if enclosed:
        rad = 1.0 + 0.5 * r() if ortho else 2.0 + 1.5 * r()  # (orthogonal: around the origins of the central pixels only)
        reach = 1.0 if ortho else rad / 6.5                   # (perspective: the spheres below move inside it)
        dome_t = K.translation(V(origin[0] + 0.2 * rad * (r() - 0.5), origin[1] + 0.2 * rad * (r() - 0.5), origin[2])) * \
            K.scaling(V(rad * sign(), rad * (0.8 + 0.4 * r()), rad))
        world.add_shape(K.Sphere(dome_t, material()))
    elif r() < 0.5:
        rad = 30.0 + 40.0 * r()
        dome_t = K.translation(V(4.0 * (r() - 0.5), 4.0 * (r() - 0.5), 2.0 * (r() - 0.5))) * \
            K.scaling(V(rad, rad * (0.7 + 0.6 * r()), rad * (sign() if mirrored else 1.0)))
        world.add_shape(K.Sphere(dome_t, material() if family == "pigments" else
                                 K.Material(K.DiffuseBRDF(K.UniformPigment(K.Color(0.0, 0.0, 0.0))), K.UniformPigment(colour(0.3, 1.0)))))

    # ---- spheres ----------------------------------------------------------------------------------------------------------
    def sphere_transform(i, centre, rad):
        t = K.translation(V(*centre))
        kinds = []
        if mirrored:
            kinds += ["m-diag", "m-trs", "m-tsr"]
        if sheared:
            kinds += ["srs"]
        if not kinds:
            kinds = ["diag", "diag", "trs"]
        kind = kinds[i % len(kinds)] if not mixed else kinds[int(len(kinds) * 0.999 * r())]
        if kind == "diag":
            return t * K.scaling(V(rad, rad, rad))
        if kind == "trs":
            return t * rot() * K.scaling(V(rad, rad * (0.4 + 1.2 * r()), rad * (0.4 + 1.2 * r())))
        if kind.startswith("m-"):
            s = signs3()
            sc = K.scaling(V(s[0] * rad * (0.5 + r()), s[1] * rad * (0.5 + r()), s[2] * rad * (0.5 + r())))
            if kind == "m-diag":
                return t * sc
            return t * rot() * sc if kind == "m-trs" else t * sc * rot()
        # scaling * rotation * scaling: singular values between rad / 7 and rad, condition number up to 7 x 7
        s1 = K.scaling(V(rad * (1.0 - 0.85 * r()), rad * (1.0 - 0.85 * r()), rad))
        s2 = K.scaling(V(1.0, 1.0 - 0.85 * r(), 1.0 - 0.85 * r()))
        return t * s1 * rot() * s2

    n_spheres = (28 if wild else 24) + int(16.0 * r())
    centres = []
    for i in range(n_spheres):
        if wild:  # on the ray through a point of the screen (or a little beside it), whatever way the camera looks, however wide
            sy, sz = 1.1 * (W / H) * (2.0 * r() - 1.0), 1.1 * (2.0 * r() - 1.0)
            m = cam_t.m
            start = (-1.0, sy, sz) if ortho else (-dist, 0.0, 0.0)
            along = (1.0, 0.0, 0.0) if ortho else (dist, sy, sz)
            o3 = [m[k][0] * start[0] + m[k][1] * start[1] + m[k][2] * start[2] + m[k][3] for k in range(3)]
            d3 = [m[k][0] * along[0] + m[k][1] * along[1] + m[k][2] * along[2] for k in range(3)]
            d = (1.5 + 4.0 * r()) * reach
            t = d / math.sqrt(d3[0] * d3[0] + d3[1] * d3[1] + d3[2] * d3[2])
            centre = (o3[0] + t * d3[0], o3[1] + t * d3[1], o3[2] + t * d3[2])
            rad = d * (0.06 + 0.12 * r())
        else:     # in front of it
            x = 1.0 + 7.0 * r()
            centre = (x, (0.5 * x + 0.5) * 2.0 * (r() - 0.5), -0.3 + 2.8 * r())
            rad = 0.2 + 0.5 * r()
        centres.append((centre, rad))
        world.add_shape(K.Sphere(sphere_transform(i, centre, rad), material()))

    if not wild and seam:
        # The texel clamp on purpose: a mirrored sphere a hair off the central ray (widths and heights of SIZES are odd, so
        # there is one), which meets it at object-space (1, -4e-20, 0): atan2 gives a tiny negative angle, u = uu + 1.0 == 1.0,
        # and column int(u * 5) == 5 of the 5x3 texture is clamped to 4 (materials.py:74-75).
        world.add_shape(K.Sphere(K.translation(V(pos[0] + 0.75, 1e-20, pos[2])) * K.scaling(V(-0.25, 0.25, 0.25)),
                                 K.Material(K.DiffuseBRDF(K.ImagePigment(textures[4])), K.UniformPigment(K.Color(0.0, 0.0, 0.0)))))

    # ---- one to three planes: a ground, a ceiling, a wall ---------------------------------------------------------------
    def plane_transform(t, tilt):
        if mirrored and (not mixed or r() < 0.5):
            s = signs3()
            return t * K.rotation_z(360.0 * r()) * tilt * K.scaling(V(s[0] * (0.3 + 2.7 * r()), s[1] * (0.3 + 2.7 * r()), s[2] * (0.3 + 2.7 * r())))
        if sheared:
            s1 = K.scaling(V(1.0 + 4.0 * r(), 1.0, 1.0 + r()))
            s2 = K.scaling(V(0.5 + 0.5 * r(), 1.0 + 2.0 * r(), 0.7 + 0.6 * r()))
            return t * tilt * s1 * K.rotation_z(360.0 * r()) * s2
        return t * tilt

    ground_z = origin[2] - (1.0 + 0.5 * r()) * (reach if enclosed else 1.0)
    n_planes = 2 + int(1.999 * r()) if wild else 1 + int(2.999 * r())
    plane_z = [ground_z]
    world.add_shape(K.Plane(plane_transform(K.translation(V(0.0, 0.0, ground_z)),
                                            K.rotation_x(8.0 * (r() - 0.5)) * K.rotation_y(8.0 * (r() - 0.5))), material()))
    if n_planes >= 2:
        ceil_z = origin[2] + (2.5 + r()) * (reach if enclosed else 1.0)
        world.add_shape(K.Plane(plane_transform(K.translation(V(0.0, 0.0, ceil_z)),
                                                K.rotation_x(180.0 + 8.0 * (r() - 0.5)) * K.rotation_y(8.0 * (r() - 0.5))), material()))
    if n_planes >= 3:
        wall_x = origin[0] + (9.0 + 2.0 * r()) * (reach if enclosed else 1.0)
        world.add_shape(K.Plane(plane_transform(K.translation(V(wall_x, 0.0, 0.0)),
                                                K.rotation_y(90.0 + 10.0 * (r() - 0.5)) * K.rotation_x(10.0 * (r() - 0.5))), material()))

    # ---- lights -------------------------------------------------------------------------------------------------------------
    def light(p, radius):
        world.add_light(K.PointLight(K.Point(*p), colour(0.2, 1.0), radius))

    if many_lights:
        for k in range(int(6.999 * r())):
            where = int(3.999 * r())
            radius = 0.0 if r() < 0.5 else 0.5 + 3.0 * r()
            if where == 0:    # inside a sphere, well off its surface
                (cx, cy, cz), rad = centres[int(len(centres) * 0.999 * r())]
                light((cx + 0.05 * rad * (r() - 0.5), cy + 0.05 * rad * (r() - 0.5), cz + 0.05 * rad * (r() - 0.5)), radius)
            elif where == 1:  # behind the ground plane
                light((origin[0] + 6.0 * (r() - 0.5), origin[1] + 6.0 * (r() - 0.5), plane_z[0] - 1.0 - r()), radius)
            elif where == 2:  # far away
                light((1e4 * (r() - 0.5), 1e4 * (r() - 0.5), 1e4 * (0.2 + 0.3 * r())), radius * 1e3)
            else:             # above the scene
                light((origin[0] + 4.0 * r(), origin[1] + 6.0 * (r() - 0.5), origin[2] + 0.5 + 1.5 * r()), radius)
    else:
        light((origin[0] - 1.0 + 4.0 * r(), origin[1] + 6.0 * (r() - 0.5), origin[2] + 1.0 + r()), 0.0 if r() < 0.5 else 2.0 + r())
    return world, camera, W, H


def path_params(seed):
    """The path tracer's parameters of a seed, as tests/test_gpu_parity.py's fuzz draws them."""
    return dict(num_of_rays=1 + seed % 3, max_depth=1 + seed % 4, rr_limit=seed % 3)
