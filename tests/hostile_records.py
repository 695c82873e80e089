"""Hit records nobody vouches for, and what the surface and scatter queries must answer for them (tests/test_hostile_records.py,
tests/test_gpu_hostile_records.py).

include/ptrace_surface.h and include/ptrace_scatter.h promise: "a record is the caller's: nothing about it is assumed".  The
oracle cannot say what follows from that -- its ``pigment_color`` casts ``u * w`` and ``floor(u * steps)`` to ``int64_t``, which is
undefined for NaN, infinity and beyond 2^63, and it shades rays, not records -- so the references here are plain Python floats,
one record at a time (no numpy vector arithmetic: nothing is contracted or reordered):

* :func:`texel` -- the headers' clamp; :func:`pigment` -- materials.py:50-100 with Python's exact integers for the checkered
  parity, and the library's definition where ``u * steps`` is not finite (NaN counts as odd, +-inf as even);
* :func:`shade_record` -- ``PointLightRenderer.__call__`` (render.py:157-193) for a record and a direction, with
  ``oracle.is_point_visible`` for the shadow rays, Python's ``max`` order and IEEE division (:func:`div`);
* :func:`scatter_record` -- ``scatter_batches.expected`` with this module's :func:`pigment`; ``oracle.scatter`` stays the
  reference for the ray (it has no integer casts: defined for any normal and direction).

tests/test_hostile_records.py pins all three to the oracle, bit for bit, on the oracle's own records.

The records.  Per world (``hostile``: this module's own small world; ``wide300_lights``: more than 256 shapes, grid on) the
oracle's genuine records -- primary rays and their mirror bounces -- and from them the CLASSES: a genuine record with ONE field
replaced (the generator class also moves a record onto a chosen texel where it says so).  :func:`batch` interleaves the hostile
records with ordinary ones and misses, so every wave holds all three, ends in a partly idle wave that holds a NaN point (where
the batch has the point class), an ordinary record and a miss, and asserts the preconditions the GPU tests rely on.

Computed once per process and shared; nothing here is modified by a test."""
import math
from contextlib import contextmanager

import numpy as np

from pytracer_amd import abi, flatten
from pytracer_amd import hostmodel as hm

from . import ray_batches as B
from . import scatter_batches as X
from . import surface_batches as S

NAN, INF = float("nan"), float("inf")
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -(2 ** 31)
U64_MAX = 2 ** 64 - 1
AMBIENT, BACKGROUND = S.AMBIENT, S.BACKGROUND
WORLD, SIZE = "hostile", (24, 18)
WORLDS = (WORLD, "wide300_lights")
CLASSES = ("ordinary", "miss", "uv", "shape", "normal", "point", "dir", "generator")
HOSTILE = CLASSES[2:]
MARGIN = 1e-6  # rad: how far every aimed specular record stays from its shape's threshold (as surface_batches.AIMED_E)
AIM_OFFSET = 2e-6

_worlds, _records, _batches, _wants = {}, {}, {}, {}


# ---- the references: plain Python floats ---------------------------------------------------------------------------------------
def div(a: float, b: float) -> float:
    """IEEE ``a / b`` where Python raises: x / 0 is +-inf, 0 / 0 and NaN / 0 are NaN."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def acos(x: float) -> float:
    """C's ``acos``: NaN outside [-1, 1] (and for NaN), where ``math.acos`` raises."""
    try:
        return math.acos(x)
    except ValueError:
        return NAN


def texel(x: float, w: int) -> int:
    """The headers' contract for an image pigment's column (row): ``f = x * w``; not ``f >= 0`` -> 0; ``f >= w`` -> ``w - 1``; else
    ``int(f)``."""
    f = x * float(w)
    if not f >= 0.0:
        return 0
    if f >= float(w):
        return w - 1
    return int(f)


def parity(t: float) -> int:
    """``int(floor(t)) % 2`` with Python's exact integers (materials.py:96-100) -- defined beyond 2^63, non-negative for negative
    cells.  Where ``t`` is not finite the reference raises; the library's definition (include/ptrace_surface.h): NaN is odd,
    +-inf is even."""
    if t != t:
        return 1
    if t in (INF, -INF):
        return 0
    return int(math.floor(t)) % 2


def pigment(flat, shape: int, emitted: bool, u: float, v: float) -> np.ndarray:
    """materials.py:50-100 for any (u, v) -> ``[3]``."""
    pre = "emi" if emitted else "pig"
    kind = int(getattr(flat, pre + "_kind")[shape])
    c1, c2 = getattr(flat, pre + "_c1"), getattr(flat, pre + "_c2")
    if kind == abi.PIGMENT_IMAGE:
        t = int(getattr(flat, pre + "_tex")[shape])
        w, h = int(flat.tex_w[t]), int(flat.tex_h[t])
        at = int(flat.tex_offset[t]) + (texel(v, h) * w + texel(u, w)) * 3
        return np.array(flat.tex_data[at: at + 3], dtype=np.float64)
    if kind == abi.PIGMENT_CHECKERED:
        steps = float(getattr(flat, pre + "_steps")[shape])
        c = c1 if parity(u * steps) == parity(v * steps) else c2
        return np.array(c[:, shape], dtype=np.float64)
    return np.array(c1[:, shape], dtype=np.float64)


def _normalize(a):
    n = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return (div(a[0], n), div(a[1], n), div(a[2], n))


def _ndot(a, b) -> float:  # geometry.py:265-276
    a, b = _normalize(a), _normalize(b)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _lights(flat):
    pos, col = np.asarray(flat.light_pos, dtype=np.float64), np.asarray(flat.light_color, dtype=np.float64)
    return [(tuple(float(x) for x in pos[:, j]), tuple(float(x) for x in col[:, j]), float(flat.light_radius[j])) for j in range(pos.shape[1])]


def light_terms(orc, flat, shape: int, point, normal, uv, d) -> list:
    """Per light of the scene, for a record on a shape of the world: None where the light does not see the point, else
    {"cos_theta", "df", "bc", "gap"} (``gap``: ``|th_in - th_out|`` of a specular shape, else None) -- render.py:166-190."""
    p = tuple(float(x) for x in point)
    nrm = tuple(float(x) for x in normal)
    out_dir = (-float(d[0]), -float(d[1]), -float(d[2]))
    diffuse = int(flat.brdf_kind[shape]) == abi.BRDF_DIFFUSE
    pc = pigment(flat, shape, False, float(uv[0]), float(uv[1]))
    terms = []
    for lp, _, lr in _lights(flat):
        if not orc.is_point_visible(flat, lp, p):
            terms.append(None)
            continue
        dv = (p[0] - lp[0], p[1] - lp[1], p[2] - lp[2])
        dist = math.sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2])
        inv = div(1.0, dist)
        in_dir = (inv * dv[0], inv * dv[1], inv * dv[2])
        neg_in = (-in_dir[0], -in_dir[1], -in_dir[2])
        c = _ndot(neg_in, nrm)
        cos_theta = max(0.0, c)  # Python's order: 0.0 where c is NaN
        q = div(lr, dist)
        df = q * q if lr > 0 else 1.0
        gap = None
        if diffuse:  # materials.py:129-130
            k = 1.0 / math.pi
            bc = (float(pc[0]) * k, float(pc[1]) * k, float(pc[2]) * k)
        else:  # materials.py:164-173
            gap = abs(acos(_ndot(nrm, in_dir)) - acos(_ndot(nrm, out_dir)))
            bc = tuple(float(x) for x in pc) if gap < float(flat.brdf_param[shape]) else (0.0, 0.0, 0.0)
        terms.append({"cos_theta": cos_theta, "df": df, "bc": bc, "gap": gap})
    return terms


def shade_record(orc, flat, shape: int, point, normal, uv, d, ambient=AMBIENT, background=BACKGROUND) -> tuple:
    """``PointLightRenderer.__call__`` (render.py:157-193) for a ray of direction ``d`` whose HitRecord is the given one."""
    if not 0 <= shape < flat.n_shapes:
        return tuple(float(x) for x in background)
    em = pigment(flat, shape, True, float(uv[0]), float(uv[1]))
    res = [float(ambient[k]) + float(em[k]) for k in range(3)]
    for (_, lc, _), t in zip(_lights(flat), light_terms(orc, flat, shape, point, normal, uv, d)):
        if t is not None:
            res = [res[k] + t["bc"][k] * lc[k] * t["cos_theta"] * t["df"] for k in range(3)]
    return tuple(res)


def scatter_record(orc, flat, rec, dirs, pcg, roulette: bool) -> dict:
    """render.py:107-134 for one child of every record: ``scatter_batches.expected`` with this module's :func:`pigment`."""
    return X.expected(orc, flat, rec, dirs, pcg, roulette, pigment=pigment)


@contextmanager
def mul_mode(orc):
    """The oracle in its ``x * x`` mode (the device multiplies where the reference writes ``x**2``)."""
    old = orc.lib().pto_get_sqr_mode()
    orc.set_sqr_mode(orc.SQR_MUL)
    try:
        yield
    finally:
        orc.set_sqr_mode(old)


# ---- generator states with a chosen next draw (pcg.py:43-58) ---------------------------------------------------------------------
def state_drawing_zero() -> int:
    """A non-zero generator state whose next ``random()`` is 0, i.e. whose next ``random_float()`` is exactly 0.0: solved like
    ``scatter_batches.state_drawing_one`` -- rotation 0 (the top five bits clear) and bits 27 .. 58 of ``(state >> 18) ^ state``
    all CLEAR, from the top down; the low 27 bits do not reach the output and are set."""
    old = (1 << 27) - 1
    for b in range(58, 26, -1):
        if (old >> (b + 18)) & 1:
            old |= 1 << b
    return old


# ---- the small world -------------------------------------------------------------------------------------------------------------
NONFINITE_TEXELS = ((NAN, 0.5, 0.5), (0.5, NAN, 0.5), (0.5, 0.5, NAN), (INF, 0.2, 0.2), (-1.0, -2.0, -3.0), (0.0, 0.0, 0.0))
TEXTURE_SIZES = ((3, 2), (1, 1), (7, 5), (len(NONFINITE_TEXELS), 1))  # in tex_data order: the 1x1 texture neither first nor last
NONFINITE_SHAPE, BLACK_SHAPE, MID_SHAPE = 5, 8, 6
LIGHTS = (((0.0, 0.0, 3.5), (1.0, 0.875, 0.75), 0.0), ((-1.0, 2.5, 1.0), (0.25, 0.375, 0.875), 2.0))


def texel_colour(tex: int, row: int, col: int) -> tuple:
    """Texture, row and column in the colour: every texel of every finite texture is distinct, so a wrong column, row or texture
    offset, or a read outside one texture, is a wrong value.  Binary fractions in (0, 1): ``lum`` is the red component."""
    code = (1 + tex * 64 + row * 8 + col) / 256.0
    return (code, code / 2, code / 4)


def _texture(tex: int) -> hm.HdrImage:
    w, h = TEXTURE_SIZES[tex]
    img = hm.HdrImage(w, h)
    if tex == 3:
        img.set_array(np.array(NONFINITE_TEXELS, dtype=np.float64).reshape(1, w, 3))
    else:
        img.set_array(np.array([[texel_colour(tex, row, col) for col in range(w)] for row in range(h)], dtype=np.float64))
    return img


def small_world():
    """-> (hostmodel World, camera): nine spheres in a 3 x 3 array in front of the default camera over one plane.  Diffuse and
    specular BRDFs; uniform, checkered (steps 1, 2 and 7) and image pigments, each as BRDF pigment and as emitted radiance; two
    lights, one without and one with a linear radius."""
    t32, t11, t75, tnf = (_texture(k) for k in range(4))
    uni = lambda r, g, b: hm.UniformPigment(hm.Color(r, g, b))  # noqa: E731
    chk = lambda steps: hm.CheckeredPigment(hm.Color(0.75, 0.5, 0.25), hm.Color(0.125, 0.25, 0.625), steps)  # noqa: E731
    glow = lambda steps: hm.CheckeredPigment(hm.Color(0.0625, 0.03125, 0.0), hm.Color(0.0, 0.015625, 0.125), steps)  # noqa: E731
    img = hm.ImagePigment
    mats = [hm.Material(hm.DiffuseBRDF(img(t32)), uni(0.03125, 0.0625, 0.015625)),   # 0
            hm.Material(hm.DiffuseBRDF(img(t11)), glow(2)),                           # 1
            hm.Material(hm.SpecularBRDF(img(t75)), uni(0.0, 0.0, 0.0)),               # 2
            hm.Material(hm.DiffuseBRDF(chk(7)), img(t32)),                            # 3
            hm.Material(hm.SpecularBRDF(chk(1)), img(t75)),                           # 4
            hm.Material(hm.DiffuseBRDF(img(tnf)), uni(0.25, 0.125, 0.0625)),          # 5  NONFINITE_SHAPE
            hm.Material(hm.DiffuseBRDF(uni(0.5, 0.75, 0.25)), img(t11)),              # 6  MID_SHAPE: lum 0.75, q 0.25
            hm.Material(hm.SpecularBRDF(uni(0.75, 0.5, 0.625)), uni(0.0, 0.0, 0.0)),  # 7
            hm.Material(hm.DiffuseBRDF(uni(0.0, 0.0, 0.0)), glow(2))]                 # 8  BLACK_SHAPE: lum 0, q 1
    world = hm.World()
    spots = [(y, z) for z in (1.3, 0.0, -1.3) for y in (1.3, 0.0, -1.3)]
    for (y, z), m in zip(spots, mats):
        world.add_shape(hm.Sphere(hm.translation(hm.Vec(1.0, y, z)) * hm.scaling(hm.Vec(0.6, 0.6, 0.6)), m))
    world.add_shape(hm.Plane(hm.translation(hm.Vec(0.0, 0.0, -2.5)), hm.Material(hm.DiffuseBRDF(chk(2)), uni(0.015625, 0.0, 0.03125))))  # 9
    for pos, col, radius in LIGHTS:
        world.add_light(hm.PointLight(hm.Vec(*pos), hm.Color(*col), radius))
    return world, hm.PerspectiveCamera(screen_distance=1.0, aspect_ratio=SIZE[0] / SIZE[1])


def world(name):
    """-> (FlatScene, Camera)"""
    if name != WORLD:
        return S.world(name)
    if name not in _worlds:
        wd, cam = small_world()
        _worlds[name] = (flatten.flatten_world(wd), flatten.flatten_camera(cam))
    return _worlds[name]


def records(orc, name) -> dict:
    """-> {"rays": [n, 8], "rec": RayHits}: the oracle's genuine records, ``surface_batches.batch``'s construction."""
    if name != WORLD:
        return S.batch(orc, name)
    if name not in _records:
        with mul_mode(orc):
            flat, cam = world(name)
            w, h = SIZE
            first = np.array([orc.tracer_fire_ray(cam, w, h, col, row) for row in range(h) for col in range(w)])
            rays = np.vstack([first, S.mirror_bounces(first, B.expected(orc, flat, first))])
            rec = B.expected(orc, flat, rays)
        rays.setflags(write=False)
        rec.buffer.setflags(write=False)
        _records[name] = {"rays": rays, "rec": rec}
    return _records[name]


# ---- a batch of records ----------------------------------------------------------------------------------------------------------
class Records:
    """The planes of a batch as the queries take them (``shape_index``, ``point``, ``normal``, ``uv``: the attributes of a
    ``RayHits``), the directions and generators, and per record its class (an index into ``CLASSES``) and a label."""

    def __init__(self, rows, n_shapes: int):
        self.n = len(rows)
        self.n_shapes = n_shapes
        self.shape_index = np.array([r["shape"] for r in rows], dtype=np.int64).astype(np.int32)
        self.point = np.array([r["point"] for r in rows], dtype=np.float64).reshape(-1, 3)
        self.normal = np.array([r["normal"] for r in rows], dtype=np.float64).reshape(-1, 3)
        self.uv = np.array([r["uv"] for r in rows], dtype=np.float64).reshape(-1, 2)
        self.dirs = np.array([r["dir"] for r in rows], dtype=np.float64).reshape(-1, 3)
        own = X.streams(self.n)
        self.pcg = np.array([[int(own[k, i]) if r["pcg"][k] is None else r["pcg"][k] for i, r in enumerate(rows)] for k in range(2)],
                            dtype=np.uint64).reshape(2, -1)
        self.cls = np.array([CLASSES.index(r["cls"]) for r in rows], dtype=np.int32)
        self.label = [r["label"] for r in rows]
        for a in (self.shape_index, self.point, self.normal, self.uv, self.dirs, self.pcg, self.cls):
            a.setflags(write=False)

    @property
    def hit(self) -> np.ndarray:
        return (self.shape_index >= 0) & (self.shape_index < self.n_shapes)

    def of(self, cls: str) -> np.ndarray:
        return self.cls == CLASSES.index(cls)

    def name(self, i: int) -> str:
        return f"record {i}, class {CLASSES[self.cls[i]]!r}: {self.label[i]}"

    def subset(self, keep) -> "Records":
        """The records ``keep`` (indices) as a batch of their own -- generators and all."""
        out = Records.__new__(Records)
        out.n, out.n_shapes = len(keep), self.n_shapes
        for key in ("shape_index", "point", "normal", "uv", "dirs", "cls"):
            setattr(out, key, np.ascontiguousarray(getattr(self, key)[keep]))
        out.pcg = np.ascontiguousarray(self.pcg[:, keep])
        out.label = [self.label[i] for i in keep]
        return out


UV_SPECIAL = (0.0, -0.0, -5e-324, -1e-320, -0.25, -1.0, -1e300, -INF, math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), 1e300,
              INF, NAN)
CELLS_NEGATIVE = (-3.0, -2.0, -1.0)
CELLS_HUGE = (float(2 ** 53 - 1), float(2 ** 53), float(2 ** 53 + 2), float(2 ** 62), float(2 ** 63), float(2 ** 64), 1e300)
F32_1E17 = float(np.float32(1e17))
POINT_1E17 = (float(np.nextafter(np.float32(1e17), np.float32(0.0))), F32_1E17, float(np.nextafter(np.float32(1e17), np.float32(np.inf))))


def _pigments(flat, s):
    """[(kind, steps, tex)] of the shape's BRDF pigment and emitted radiance."""
    return [(int(flat.pig_kind[s]), float(flat.pig_steps[s]), int(flat.pig_tex[s])), (int(flat.emi_kind[s]), float(flat.emi_steps[s]), int(flat.emi_tex[s]))]


def _uv_values(flat, s) -> list:
    """[(label, u or None, v or None)] for shape ``s`` (None: the genuine record's coordinate stays)."""
    out = []
    for k, x in enumerate(UV_SPECIAL):
        out += [(f"u={x!r}", x, None), (f"v={x!r}", None, x), (f"u=v={x!r}", x, x)]
        if k % 3 == 0:
            y = UV_SPECIAL[(k + 5) % len(UV_SPECIAL)]
            out.append((f"u={x!r} v={y!r}", x, y))
    for kind, steps, tex in _pigments(flat, s):
        if kind == abi.PIGMENT_IMAGE:
            w, h = int(flat.tex_w[tex]), int(flat.tex_h[tex])
            for col in range(w):
                for row in range(h):  # every texel through its middle
                    out.append((f"texture {tex} texel ({col}, {row})", (col + 0.5) / w, (row + 0.5) / h))
            for k in range(w + 1):  # every k / w with its two neighbours, the row going round
                for x in (math.nextafter(k / w, -INF), k / w, math.nextafter(k / w, INF)):
                    out.append((f"texture {tex} u={x!r} ({k}/{w})", x, ((k % h) + 0.5) / h))
            for k in range(h + 1):
                for x in (math.nextafter(k / h, -INF), k / h, math.nextafter(k / h, INF)):
                    out.append((f"texture {tex} v={x!r} ({k}/{h})", ((k % w) + 0.5) / w, x))
        elif kind == abi.PIGMENT_CHECKERED:
            at = [(f"cell {c!r}", (c + 0.5) / steps) for c in CELLS_NEGATIVE] + [("cell -0.5 / steps", -0.5 / steps)] + \
                 [(f"cell {c!r}", c / steps) for c in CELLS_HUGE]
            for label, x in at:
                out += [(f"steps {steps:g} {label} in u", x, None), (f"steps {steps:g} {label} in v", None, x), (f"steps {steps:g} {label} in both", x, x)]
    return out


def _perpendicular(n):
    """A direction whose dot product with ``n`` is exactly 0.0 (two commuting products of opposite sign)."""
    return (-n[1], n[0], 0.0) if (n[0] != 0.0 or n[1] != 0.0) else (1.0, 0.0, 0.0)


def _aimed(p, n, lp, e):
    """The direction of a ray whose reflection at ``p`` (normal ``n``) leaves ``e`` rad off the mirror direction of the light at
    ``lp``: ``out_dir`` is ``in_dir`` turned by ``e`` in the plane of ``n`` and ``in_dir`` -> d = -out_dir."""
    i = np.asarray(_normalize(tuple(p[k] - lp[k] for k in range(3))))
    k = np.cross(np.asarray(n, dtype=np.float64), i)
    assert np.linalg.norm(k) > 1e-3, "normal and light direction are parallel: nothing to turn about"
    k = k / np.linalg.norm(k)
    out = i * math.cos(e) + np.cross(k, i) * math.sin(e)
    return tuple(float(-x) for x in out)


def _rows(orc, name, classes) -> list:
    """The hostile rows of the requested classes, class by class."""
    flat = world(name)[0]
    g = records(orc, name)
    rec, rays = g["rec"], g["rays"]
    shape = np.asarray(rec.shape_index)
    n_shapes = int(flat.n_shapes)
    by_shape = {int(s): np.flatnonzero(shape == s) for s in np.unique(shape[shape >= 0])}
    turn = {s: 0 for s in by_shape}

    def base(s):
        """The next genuine record on shape ``s`` as a row."""
        i = int(by_shape[s][turn[s] % by_shape[s].size])
        turn[s] += 1
        return {"shape": s, "point": tuple(rec.point[i].tolist()), "normal": tuple(rec.normal[i].tolist()), "uv": tuple(rec.uv[i].tolist()),
                "dir": tuple(rays[i, 3:6].tolist()), "pcg": (None, None), "cls": "ordinary", "label": f"genuine record {i} on shape {s}", "genuine": i}

    def changed(s, cls, label, r=None, **fields):
        r = base(s) if r is None else r
        r.update(fields)
        r["cls"], r["label"] = cls, f"{label} (shape {s}, from genuine record {r['genuine']})"
        return r

    seen = sorted(by_shape, key=lambda s: -by_shape[s].size)
    textured = [s for s in seen if any(k != abi.PIGMENT_UNIFORM for k, _, _ in _pigments(flat, s))]
    diffuse = [s for s in seen if int(flat.brdf_kind[s]) == abi.BRDF_DIFFUSE]
    specular = [s for s in seen if int(flat.brdf_kind[s]) == abi.BRDF_SPECULAR]
    assert diffuse and specular and textured, (name, diffuse, specular, textured)
    planes = [s for s in seen if int(flat.kind[s]) == abi.SHAPE_PLANE]
    a_few = [diffuse[0], specular[0]] + planes[:1]
    rng = np.random.default_rng(20)
    rows = []
    if "uv" in classes:
        for s in sorted(set(textured + a_few)):
            for label, u, v in _uv_values(flat, s):
                r = base(s)
                r["uv"] = (r["uv"][0] if u is None else u, r["uv"][1] if v is None else v)
                r["cls"], r["label"] = "uv", f"{label} (shape {s}, from genuine record {r['genuine']})"
                rows.append(r)
    if "shape" in classes:
        for value in (n_shapes - 1, n_shapes, n_shapes + 1, INT32_MAX, INT32_MIN, -2):
            for s in a_few:
                rows.append(changed(s, "shape", f"shape index {value}", shape=value))
    if "normal" in classes:
        for s in a_few:
            for f in (1e-3, 1e3, 1e-170, 1e170):
                r = base(s)
                rows.append(changed(s, "normal", f"normal scaled by {f:g}", r, normal=tuple(x * f for x in r["normal"])))
            for label, fn in (("the zero vector", lambda n: (0.0, 0.0, 0.0)), ("NaN in x", lambda n: (NAN, n[1], n[2])), ("NaN in z", lambda n: (n[0], n[1], NAN)),
                              ("+inf in y", lambda n: (n[0], INF, n[2])), ("-inf in z", lambda n: (n[0], n[1], -INF)), ("n.z = 0.0", lambda n: (n[0], n[1], 0.0)),
                              ("n.z = -0.0", lambda n: (n[0], n[1], -0.0)), ("n.z = 1.0", lambda n: (n[0], n[1], 1.0)), ("n.z = -1.0", lambda n: (n[0], n[1], -1.0)),
                              ("n = (0, 0, -1)", lambda n: (0.0, 0.0, -1.0)), ("n = (1, 0, 0)", lambda n: (1.0, 0.0, 0.0))):
                r = base(s)
                rows.append(changed(s, "normal", f"normal: {label}", r, normal=fn(r["normal"])))
    if "point" in classes:
        centre = next(tuple(float(flat.m[k][s]) for k in (3, 7, 11)) for s in range(1, n_shapes) if int(flat.kind[s]) == abi.SHAPE_SPHERE)
        for s in a_few[:2]:
            for j, (lp, _, _) in enumerate(_lights(flat)):
                rows.append(changed(s, "point", f"point exactly at light {j}", point=lp))
                rows.append(changed(s, "point", f"point at light {j} plus 1e-300", point=tuple(x + 1e-300 for x in lp)))
            for k in range(3):
                r = base(s)
                rows.append(changed(s, "point", f"point: NaN in component {k}", r, point=tuple(NAN if q == k else x for q, x in enumerate(r["point"]))))
                r = base(s)
                rows.append(changed(s, "point", f"point: +inf in component {k}", r, point=tuple(INF if q == k else x for q, x in enumerate(r["point"]))))
            rows.append(changed(s, "point", "point at (1e200, 1e200, 1e200)", point=(1e200, 1e200, 1e200)))
            r = base(s)
            rows.append(changed(s, "point", "point: 1e200 in x", r, point=(1e200,) + r["point"][1:]))
            for k, x in enumerate(POINT_1E17):
                r = base(s)
                rows.append(changed(s, "point", f"point: largest coordinate {x!r} (float32(1e17) and its neighbours)", r,
                                    point=tuple(x if q == k else c for q, c in enumerate(r["point"]))))
            rows.append(changed(s, "point", f"point inside a sphere, at its centre {centre}", point=centre))
            free = tuple(0.5 * (a + b) for a, b in zip(_lights(flat)[0][0], _lights(flat)[1][0]))
            rows.append(changed(s, "point", f"point in free space, midway between the lights {free}", point=free))
    if "dir" in classes:
        for s in specular[:2]:
            for _ in range(4):
                f = 10.0 ** rng.uniform(-3.0, 3.0)
                r = base(s)
                rows.append(changed(s, "dir", f"direction scaled by {f!r}", r, dir=tuple(x * f for x in r["dir"])))
            rows.append(changed(s, "dir", "direction: the zero vector", dir=(0.0, 0.0, 0.0)))
            r = base(s)
            rows.append(changed(s, "dir", "direction: NaN in y", r, dir=(r["dir"][0], NAN, r["dir"][2])))
            r = base(s)
            rows.append(changed(s, "dir", "direction exactly perpendicular to the normal", r, dir=_perpendicular(r["normal"])))
        # the mirror direction of a light the point sees, and around the shape's threshold: the first records that see one
        aimed = 0
        for s in specular:
            thr = float(flat.brdf_param[s])
            for _ in range(by_shape[s].size):
                r = base(s)
                lit = [(j, lp) for j, (lp, _, _) in enumerate(_lights(flat)) if orc.is_point_visible(flat, lp, r["point"])]
                if not lit:
                    continue
                j, lp = lit[aimed % len(lit)]
                for e in (0.0, thr - AIM_OFFSET, -(thr - AIM_OFFSET), thr + AIM_OFFSET, -(thr + AIM_OFFSET)):
                    q = dict(r)
                    q["dir"] = _aimed(r["point"], r["normal"], lp, e)
                    q["cls"], q["label"] = "dir", f"direction {e!r} rad off the mirror direction of light {j} (shape {s}, from genuine record {r['genuine']})"
                    rows.append(q)
                aimed += 1
                if aimed % 2 == 0:
                    break
            if aimed >= 4:
                break
        assert aimed >= 2, f"{name}: {aimed} records on specular shapes see a light"
    if "generator" in classes:
        one, zero = X.state_drawing_one(), state_drawing_zero()
        words = [(st, inc) for st in (0, U64_MAX, one, zero) for inc in (None, 0, 1, U64_MAX)] + [(None, 0), (None, 1), (None, U64_MAX)]
        shapes = [diffuse[0], specular[0]] + [s for s in (MID_SHAPE, BLACK_SHAPE) if name == WORLD]
        for s in shapes:
            for st, inc in words:
                rows.append(changed(s, "generator", f"state {st} inc {inc}" + (" (lum 0: q = 1.0)" if name == WORLD and s == BLACK_SHAPE else ""), pcg=(st, inc)))
        if name == WORLD:  # ... and on the nonfinite texture's texels: the generator class's two-field records
            for col, tx in enumerate(NONFINITE_TEXELS):
                for st in (one, zero):
                    rows.append(changed(NONFINITE_SHAPE, "generator", f"state {st} on texel {tx}", pcg=(st, None), uv=((col + 0.5) / len(NONFINITE_TEXELS), 0.5)))
    return rows


def batch(orc, name, classes=HOSTILE) -> Records:
    """The hostile records of ``classes`` in ``name``, every two of them followed by an ordinary record and every three by a
    miss; then a tail that leaves the last wave partly idle with a NaN point (point class), an ordinary record and a miss in it."""
    key = (name, tuple(classes))
    if key in _batches:
        return _batches[key]
    with mul_mode(orc):
        flat = world(name)[0]
        hostile = _rows(orc, name, classes)
        g = records(orc, name)
        rec, rays = g["rec"], g["rays"]
        hits = np.flatnonzero(rec.hit)
        assert hits.size > 50
        turn = [0]

        def ordinary(miss=False):
            i = int(hits[(turn[0] * 7) % hits.size])
            turn[0] += 1
            return {"shape": -1 if miss else int(rec.shape_index[i]), "point": tuple(rec.point[i].tolist()), "normal": tuple(rec.normal[i].tolist()),
                    "uv": tuple(rec.uv[i].tolist()), "dir": tuple(rays[i, 3:6].tolist()), "pcg": (None, None), "cls": "miss" if miss else "ordinary",
                    "label": f"genuine record {i}" + (" with shape index -1" if miss else "")}

        rows = []
        for k, r in enumerate(hostile):
            rows.append(r)
            if k % 2 == 1:
                rows.append(ordinary())
            if k % 3 == 2:
                rows.append(ordinary(miss=True))
        tail = [ordinary(), ordinary(miss=True), ordinary()]
        if "point" in classes:
            nan_point = next(r for r in hostile if r["cls"] == "point" and "NaN" in r["label"])
            tail.insert(1, dict(nan_point))
        # the whole tail in the last, partly idle wave, and an odd n (the int32 planes end in padding)
        while (len(rows) + len(tail)) % 64 < len(tail) or (len(rows) + len(tail)) % 2 == 0:
            rows.append(ordinary())
        rows += tail
        b = Records(rows, int(flat.n_shapes))
        _check(orc, name, flat, b, classes)
    _batches[key] = b
    return b


def _check(orc, name, flat, b, classes):
    """What the GPU tests rely on."""
    assert b.n % 2 == 1 and b.n % 64 != 0, b.n
    for c in ("ordinary", "miss") + tuple(classes):
        assert b.of(c).any(), f"{name}: class {c!r} is empty"
    last = np.arange(b.n - b.n % 64, b.n)
    assert b.of("ordinary")[last].any() and b.of("miss")[last].any()
    if "point" in classes:
        assert np.isnan(b.point[last]).any(axis=1)[b.hit[last]].any(), "no NaN point in the partly idle wave"
    waves = [np.arange(w, min(w + 64, b.n)) for w in range(0, b.n, 64)]
    mixed = [w for w in waves if b.of("ordinary")[w].any() and b.of("miss")[w].any() and (~b.of("ordinary") & ~b.of("miss"))[w].any()]
    assert len(mixed) >= len(waves) - 1, f"{name}: {len(waves) - len(mixed)} waves without ordinary, hostile and missing records side by side"
    if "uv" in classes:  # the texel classes reach every texel of every texture
        reached = {t: set() for t in range(len(flat.tex_w))}
        for i in np.flatnonzero(b.of("uv") & b.hit):
            for kind, _, t in _pigments(flat, int(b.shape_index[i])):
                if kind == abi.PIGMENT_IMAGE:
                    reached[t].add((texel(float(b.uv[i, 0]), int(flat.tex_w[t])), texel(float(b.uv[i, 1]), int(flat.tex_h[t]))))
        for t, cells in reached.items():
            assert len(cells) == int(flat.tex_w[t]) * int(flat.tex_h[t]), f"{name}: texture {t}: only {len(cells)} texels reached"
    if "dir" in classes:
        margins = dir_margins(orc, flat, b)
        assert margins and min(margins) >= MARGIN, f"{name}: a specular record of the dir class within {min(margins):.3g} rad of its threshold"


def dir_margins(orc, flat, b, every: bool = False) -> list:
    """``| |th_in - th_out| - threshold |`` over every (specular record of the dir class, light it sees) pair whose angles are
    numbers: the one quantity whose sign a libm call (acos) decides in the lights kernel.  ``every``: over all classes."""
    out = []
    for i in np.flatnonzero(b.hit if every else b.of("dir") & b.hit):
        s = int(b.shape_index[i])
        if int(flat.brdf_kind[s]) != abi.BRDF_SPECULAR:
            continue
        for t in light_terms(orc, flat, s, b.point[i], b.normal[i], b.uv[i], b.dirs[i]):
            if t is not None and t["gap"] == t["gap"]:
                out.append(abs(t["gap"] - float(flat.brdf_param[s])))
    return out


def lone_nan_points(orc, name) -> Records:
    """Three waves of ordinary records and misses and a partly idle fourth; the ONLY NaN points are lane 0 of the first wave and
    lane 63 of the second (one lane sends its whole wave through the exhaustive query)."""
    key = (name, "lone")
    if key not in _batches:
        full = batch(orc, name, ("point",))
        plain = np.flatnonzero(full.of("ordinary") | full.of("miss"))
        nan = np.flatnonzero(full.of("point") & np.isnan(full.point).any(axis=1))
        assert plain.size >= 16 and nan.size >= 2
        keep = [int(plain[k % plain.size]) for k in range(64 * 3 + 21)]
        keep[0], keep[127] = int(nan[0]), int(nan[1])
        b = full.subset(keep)
        where = np.flatnonzero(np.isnan(b.point).any(axis=1) & b.hit)
        assert where.tolist() == [0, 127] and b.n % 64 != 0 and b.n % 2 == 1
        _batches[key] = b
    return _batches[key]


# ---- expectations ----------------------------------------------------------------------------------------------------------------
def want_surface(flat, b) -> dict:
    kind = np.full(b.n, -1, np.int32)
    pc, em = np.zeros((b.n, 3)), np.zeros((b.n, 3))
    for i in np.flatnonzero(b.hit):
        s = int(b.shape_index[i])
        kind[i] = int(flat.brdf_kind[s])
        pc[i], em[i] = pigment(flat, s, False, float(b.uv[i, 0]), float(b.uv[i, 1])), pigment(flat, s, True, float(b.uv[i, 0]), float(b.uv[i, 1]))
    return {"brdf_kind": kind, "brdf_color": pc, "emitted": em}


def want_lights(orc, flat, b) -> np.ndarray:
    with mul_mode(orc):
        return np.array([shade_record(orc, flat, int(b.shape_index[i]), b.point[i], b.normal[i], b.uv[i], b.dirs[i]) for i in range(b.n)]).reshape(-1, 3)


def want_scatter(orc, flat, b, roulette: bool) -> dict:
    with mul_mode(orc):
        return scatter_record(orc, flat, b, b.dirs, b.pcg, roulette)


def wanted(orc, name, classes, what, roulette=False):
    """The expectation ``what`` ("surface", "lights", "scatter") of ``batch(orc, name, classes)``, computed once."""
    key = (name, tuple(classes), what, bool(roulette))
    if key not in _wants:
        flat, b = world(name)[0], batch(orc, name, classes)
        w = want_surface(flat, b) if what == "surface" else want_lights(orc, flat, b) if what == "lights" else want_scatter(orc, flat, b, roulette)
        for a in (w.values() if isinstance(w, dict) else [w]):
            a.setflags(write=False)
        _wants[key] = w
    return _wants[key]


# ---- the comparison: NaN where NaN is expected, every other value bit for bit ------------------------------------------------------
def differing(got, want) -> np.ndarray:
    """Indices of the records (first axis) in which ``got`` is not ``want``: the positions of NaN must be equal and every other
    value bit-identical; a NaN's sign and payload are not pinned."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        ok = (gn == wn) & (gn | (got.view(np.uint64) == want.view(np.uint64)))
    else:
        ok = got == want
    return np.flatnonzero(~ok.reshape(got.shape[0], -1).all(axis=1))


def explain(b, what, got, want) -> str:
    """'' when equal, else the message of the first differing record with its class."""
    bad = differing(got, want)
    if bad.size == 0:
        return ""
    i = int(bad[0])
    classes = sorted({CLASSES[c] for c in b.cls[bad]})
    return f"{what}: {bad.size} of {b.n} records differ (classes {classes}); first: {b.name(i)}: got {np.asarray(got)[i]!r}, want {np.asarray(want)[i]!r}"
