"""CPU-only tests of tests/hostile_records.py, the reference for hit records nobody vouches for (include/ptrace_surface.h,
include/ptrace_scatter.h: "a record is the caller's: nothing about it is assumed").

The reference is plain Python; what makes it one: on the oracle's own records -- where the oracle IS defined -- ``pigment``,
``shade_record`` and ``scatter_record`` are the existing expectations of tests/surface_batches.py and tests/scatter_batches.py
bit for bit; ``texel`` and the checkered parity are hand-written tables; the Python semantics the expectations lean on are
asserted literally; and the batches the GPU tests run hold every class they are meant to (the helper's own asserts, run here)."""
import math

import numpy as np
import pytest

from pytracer_amd import abi

from . import hostile_records as H
from . import scatter_batches as X
from . import surface_batches as S

NAN, INF = H.NAN, H.INF
PINNED = ("demo", "c2_lights", "pigments", "lights")


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    yield oracle
    oracle.set_sqr_mode(oracle.SQR_POW)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the new reference is the oracle wherever the oracle is defined ---------------------------------------------------------
@pytest.mark.parametrize("name", PINNED)
def test_pigment_and_shade_record_are_the_oracles_on_its_own_records(orc, name):
    b = S.batch(orc, name)
    flat, rec, rays = S.world(name)[0], b["rec"], b["rays"]
    mats = b["materials"]
    uv = np.array(rec.uv)
    wrong = []
    for i in range(rec.n):
        s = int(rec.shape_index[i])
        got = H.shade_record(orc, flat, s, rec.point[i], rec.normal[i], uv[i], rays[i, 3:6])
        if not _bits(got, b["colors"][i]):
            wrong.append(("colour", i))
        if s >= 0 and not (_bits(H.pigment(flat, s, False, float(uv[i, 0]), float(uv[i, 1])), mats["brdf_color"][i])
                           and _bits(H.pigment(flat, s, True, float(uv[i, 0]), float(uv[i, 1])), mats["emitted"][i])):
            wrong.append(("pigment", i))
    assert not wrong, f"{name}: {len(wrong)} of {rec.n} records differ from the oracle, first {wrong[:5]}"
    assert rec.n > 500
    want = H.want_surface(flat, _as_records(rec, rays, flat))
    for key in ("brdf_kind", "brdf_color", "emitted"):
        assert want[key].tobytes() == np.ascontiguousarray(mats[key]).tobytes(), (name, key)


def _as_records(rec, rays, flat):
    rows = [{"shape": int(rec.shape_index[i]), "point": rec.point[i], "normal": rec.normal[i], "uv": rec.uv[i], "dir": rays[i, 3:6], "pcg": (None, None),
             "cls": "ordinary", "label": ""} for i in range(rec.n)]
    return H.Records(rows, int(flat.n_shapes))


@pytest.mark.parametrize("name", PINNED)
def test_scatter_record_is_the_oracles_on_its_own_records(orc, name):
    """``scatter_batches.expected`` with the oracle's pigment (its default: the batches of tests/scatter_batches.py, where the
    world has one) against the same with this module's."""
    if name in X.WORLDS:
        b = X.batch(orc, name)
        rec, dirs, pcg, wants = b["rec"], b["dirs"], b["pcg"], b["want"]
    else:
        b = S.batch(orc, name)
        rec, dirs, pcg = b["rec"], np.ascontiguousarray(b["rays"][:, 3:6]), X.streams(b["rec"].n)
        wants = {True: X.expected(orc, S.world(name)[0], rec, dirs, pcg, True)}
    flat = S.world(name)[0]
    for roulette, want in wants.items():
        got = H.scatter_record(orc, flat, rec, dirs, pcg, roulette)
        assert set(got) == set(want)
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), (name, roulette, key)
        assert (got["status"] == 1).sum() > 100 and (not roulette or (got["status"] == 0).sum() > 10)


# ---- 2. texel and parity, by hand -----------------------------------------------------------------------------------------------
TEXEL = [  # (x, w, column)
    (0.0, 7, 0), (-0.0, 7, 0), (-5e-324, 7, 0), (-1e-320, 7, 0), (-0.25, 7, 0), (-1.0, 7, 0), (-1e300, 7, 0), (-INF, 7, 0), (NAN, 7, 0),
    (math.nextafter(1.0, 0.0), 7, 6), (1.0, 7, 6), (math.nextafter(1.0, 2.0), 7, 6), (1e300, 7, 6), (INF, 7, 6),
    (0.5, 1, 0), (1.0, 1, 0), (-1.0, 1, 0), (INF, 1, 0), (NAN, 1, 0),
    (1 / 3, 3, 1), (math.nextafter(1 / 3, 0.0), 3, 0), (math.nextafter(1 / 3, 1.0), 3, 1), (2 / 3, 3, 2), (math.nextafter(2 / 3, 0.0), 3, 1),
    (0.5, 2, 1), (math.nextafter(0.5, 0.0), 2, 0), (0.2, 5, 1), (0.4, 5, 2), (0.6, 5, 3), (0.8, 5, 4), (math.nextafter(0.8, 0.0), 5, 3),
    (1 / 7, 7, 1), (2 / 7, 7, 2), (3 / 7, 7, 3), (4 / 7, 7, 4), (5 / 7, 7, 5), (6 / 7, 7, 6), (math.nextafter(6 / 7, 0.0), 7, 5),
]


def test_texel_against_a_table():
    for x, w, col in TEXEL:
        assert H.texel(x, w) == col, (x, w, H.texel(x, w), col)
    # 1/3 * 3 and 2/3 * 3 round to whole numbers, 3/7 * 7 and 6/7 * 7 too: the table above has the column the PRODUCT lands in
    assert (1 / 3) * 3.0 == 1.0 and (3 / 7) * 7.0 == 3.0 and (6 / 7) * 7.0 == 6.0


PARITY = [  # (t = u * steps, parity of int(floor(t)))
    (0.0, 0), (-0.0, 0), (0.5, 0), (1.0, 1), (1.5, 1), (2.0, 0), (-0.5, 1), (-1.0, 1), (-1.5, 0), (-2.0, 0), (-2.5, 1), (-3.0, 1), (-5e-324, 1),
    (float(2 ** 53 - 1), 1), (float(2 ** 53), 0), (float(2 ** 53 + 2), 0), (float(2 ** 62), 0), (float(2 ** 63), 0), (float(2 ** 64), 0), (1e300, 0),
    (-float(2 ** 63), 0), (-float(2 ** 53 - 1), 1),
    (NAN, 1), (INF, 0), (-INF, 0),  # the library's definition (include/ptrace_surface.h): the reference raises here
]


def test_checkered_parity_against_a_table(orc):
    for t, odd in PARITY:
        assert H.parity(t) == odd, (t, H.parity(t), odd)
    # ... and through pigment(): steps 1, 2 and 7 of the small world, one of the pigment's two colours and never anything else
    flat = H.world(H.WORLD)[0]
    s = next(s for s in range(flat.n_shapes) if int(flat.pig_kind[s]) == abi.PIGMENT_CHECKERED and float(flat.pig_steps[s]) == 1.0)
    c1, c2 = flat.pig_c1[:, s], flat.pig_c2[:, s]
    for t, odd in PARITY:
        assert _bits(H.pigment(flat, s, False, t, 0.5), c2 if odd else c1), t      # against an even cell
        assert _bits(H.pigment(flat, s, False, 1.5, t), c1 if odd else c2), t      # against an odd one
    assert _bits(H.pigment(flat, s, False, NAN, NAN), c1) and _bits(H.pigment(flat, s, False, INF, -INF), c1)
    assert {float(flat.pig_steps[k]) for k in range(flat.n_shapes) if int(flat.pig_kind[k]) == abi.PIGMENT_CHECKERED} == {1.0, 2.0, 7.0}
    # where the oracle is defined it agrees (finite cells inside int64)
    for t, _ in PARITY:
        if math.isfinite(t) and abs(t) < 2.0 ** 62:
            assert _bits(H.pigment(flat, s, False, t, 0.5), orc.pigment(flat, s, False, t, 0.5)), t


def test_the_python_semantics_the_expectations_depend_on():
    assert max(0.0, NAN) == 0.0
    assert math.isnan(max(NAN, 0.5))
    assert max(max(NAN, 0.5), 0.5) != max(max(0.5, NAN), 0.5) and max(max(0.5, NAN), 0.5) == 0.5  # lum of (NaN, .5, .5) and of (.5, NaN, .5)
    assert -3 % 2 == 1
    assert int(-0.5) == 0
    assert int(math.floor(-0.5)) % 2 == 1
    assert H.div(1.0, 0.0) == INF and H.div(-1.0, 0.0) == -INF and H.div(1.0, -0.0) == -INF and math.isnan(H.div(0.0, 0.0)) and math.isnan(H.div(NAN, 0.0))
    assert H.div(1.0, INF) == 0.0 and math.isnan(H.div(INF, INF)) and H.div(3.0, 2.0) == 1.5
    assert math.isnan(H.acos(NAN)) and math.isnan(H.acos(math.nextafter(1.0, 2.0))) and H.acos(1.0) == 0.0
    assert math.sqrt(INF) == INF and math.isnan(math.sqrt(NAN)) and 1e200 * 1e200 == INF


def test_generator_states_with_a_chosen_draw(orc):
    for state, draw in ((X.state_drawing_one(), 1.0), (H.state_drawing_zero(), 0.0), (0, 0.0)):
        for inc in (0, 1, H.U64_MAX, 109):
            g = orc.Pcg()
            g.st[0], g.st[1] = state, inc
            assert g.random_float() == draw, (state, inc)
    assert H.state_drawing_zero() != 0


# ---- 3. the small world and the batches the GPU tests run ---------------------------------------------------------------------
def test_the_small_world_is_what_the_classes_need():
    flat = H.world(H.WORLD)[0]
    assert [(int(w), int(h)) for w, h in zip(flat.tex_w, flat.tex_h)] == list(H.TEXTURE_SIZES)  # the 1x1 texture neither first nor last
    texels = np.asarray(flat.tex_data).reshape(-1, 3)
    finite = texels[: -len(H.NONFINITE_TEXELS)]
    assert len({tuple(t) for t in finite}) == len(finite) == 3 * 2 + 1 + 7 * 5 and np.isfinite(finite).all()
    assert np.isnan(texels[-6:-3]).sum() == 3 and texels[-3, 0] == INF and tuple(texels[-2]) == (-1.0, -2.0, -3.0) and not texels[-1].any()
    for kinds in (flat.pig_kind, flat.emi_kind):
        assert {abi.PIGMENT_UNIFORM, abi.PIGMENT_CHECKERED, abi.PIGMENT_IMAGE} <= set(int(k) for k in kinds)
    assert {abi.BRDF_DIFFUSE, abi.BRDF_SPECULAR} == set(int(k) for k in flat.brdf_kind)
    assert (np.asarray(flat.kind) == abi.SHAPE_PLANE).sum() == 1 and flat.n_shapes == 10
    assert sorted(float(r) for r in flat.light_radius) == [0.0, 2.0]
    assert S.world("wide300_lights")[0].n_shapes > 256


@pytest.mark.parametrize("name", H.WORLDS)
def test_the_batches_hold_every_class(orc, name):
    """``batch`` asserts its own preconditions (every class non-empty, every texel reached, the aimed directions' margin, the
    mixed last wave); here, besides, what each class must contain."""
    classes = H.HOSTILE if name == H.WORLD else H.HOSTILE[:-1]  # (wide300_lights: shade_lights only -- no generators)
    b = H.batch(orc, name, classes)
    flat = H.world(name)[0]
    assert b.n <= 2000 and b.n % 64 != 0 and b.n % 2 == 1
    counts = {c: int(b.of(c).sum()) for c in H.CLASSES}
    print(name, b.n, counts)
    u = b.uv[b.of("uv")]
    for x in H.UV_SPECIAL:
        for axis in (0, 1):
            col, negative = u[:, axis], math.copysign(1.0, x) < 0
            assert (np.isnan(col).any() if x != x else ((col == x) & (np.signbit(col) == negative)).any()), (name, x, axis)
    assert set(b.shape_index[b.of("shape")].tolist()) == {flat.n_shapes - 1, flat.n_shapes, flat.n_shapes + 1, H.INT32_MAX, H.INT32_MIN, -2}
    nrm = b.normal[b.of("normal")]
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (nrm * nrm).sum(axis=1)
    assert (sq == 0.0).sum() >= 4 and np.isinf(sq).any() and np.isnan(sq).any()  # zero vector and underflow; overflow and inf; NaN
    pts = b.point[b.of("point")]
    lp = np.asarray(flat.light_pos).T
    for j in range(lp.shape[0]):
        assert (pts == lp[j]).all(axis=1).any(), f"no point exactly at light {j}"
    assert np.isnan(pts).any() and (pts == INF).any() and (pts == 1e200).any()
    for x in H.POINT_1E17:
        assert (pts == x).any()
    assert H.POINT_1E17[0] < 1e17 < H.POINT_1E17[2] and np.float32(H.POINT_1E17[1]) == np.float32(1e17)
    d = b.dirs[b.of("dir")]
    assert (~d.any(axis=1)).any() and np.isnan(d).any()
    perp = [i for i in np.flatnonzero(b.of("dir")) if "perpendicular" in b.label[i]]
    dot = lambda a, c: float(a[0]) * float(c[0]) + float(a[1]) * float(c[1]) + float(a[2]) * float(c[2])  # noqa: E731 (the device's order)
    assert perp and all(dot(b.normal[i], b.dirs[i]) == 0.0 for i in perp)
    margins = H.dir_margins(orc, flat, b)
    assert min(margins) >= H.MARGIN
    # ... and no other specular record of the batch sits where the last bits of an acos could decide (they are not aimed: 1e-9 rad)
    assert min(H.dir_margins(orc, flat, b, every=True)) >= 1e-9
    # aimed on both sides of the threshold: with a light's term and without
    gaps = [t["gap"] - float(flat.brdf_param[int(b.shape_index[i])]) for i in np.flatnonzero(b.of("dir")) if "mirror" in b.label[i]
            for t in H.light_terms(orc, flat, int(b.shape_index[i]), b.point[i], b.normal[i], b.uv[i], b.dirs[i]) if t is not None]
    assert min(gaps) < -H.MARGIN and max(gaps) > H.MARGIN and any(-2.5e-6 < g < -H.MARGIN for g in gaps) and any(H.MARGIN < g < 2.5e-6 for g in gaps)
    if name == H.WORLD:
        st, inc = b.pcg[0][b.of("generator")], b.pcg[1][b.of("generator")]
        assert {0, H.U64_MAX, X.state_drawing_one(), H.state_drawing_zero()} <= set(int(x) for x in st)
        assert {0, 1, H.U64_MAX} <= set(int(x) for x in inc)
    lone = H.lone_nan_points(orc, name)
    assert np.flatnonzero(np.isnan(lone.point).any(axis=1)).tolist() == [0, 127]


def test_the_expectations_hold_the_cases_the_headers_name(orc):
    """What the reference says about the cases the GPU tests single out -- so that an expectation cannot be right for a wrong
    reason."""
    b = H.batch(orc, H.WORLD, H.HOSTILE)
    flat = H.world(H.WORLD)[0]
    lights = H.wanted(orc, H.WORLD, H.HOSTILE, "lights")
    # the record exactly at the radius-0 light with a finite normal: cos_theta = max(0.0, NaN) = 0.0 and the colour is finite
    at0 = [i for i in np.flatnonzero(b.of("point")) if "exactly at light 0" in b.label[i] and int(flat.brdf_kind[b.shape_index[i]]) == abi.BRDF_DIFFUSE]
    assert at0
    for i in at0:
        t = H.light_terms(orc, flat, int(b.shape_index[i]), b.point[i], b.normal[i], b.uv[i], b.dirs[i])[0]
        assert t is not None and t["cos_theta"] == 0.0 and t["df"] == 1.0 and np.isfinite(lights[i]).all(), b.name(i)
    assert np.isnan(lights).any() and np.array_equal(lights[~b.hit], np.tile(np.asarray(H.BACKGROUND), (int((~b.hit).sum()), 1)))
    # the nonfinite texture: lum by Python's max order; (-1, -2, -3) ends every path behind the roulette's one draw
    plain, rr = (H.wanted(orc, H.WORLD, H.HOSTILE, "scatter", flag) for flag in (False, True))
    on = lambda col: [i for i in np.flatnonzero(b.hit & (b.shape_index == H.NONFINITE_SHAPE))  # noqa: E731
                      if H.texel(float(b.uv[i, 0]), 6) == col]
    assert all(on(col) for col in range(6))
    assert all(plain["status"][i] == 0 for i in on(0)) and all(plain["status"][i] == 1 for i in on(1))  # lum NaN: not > 0; lum 0.5
    assert all(plain["status"][i] == 1 for i in on(2)) and all(plain["status"][i] == 1 for i in on(3))  # lum 0.5; lum inf
    for i in on(4):
        assert plain["status"][i] == 0 and rr["status"][i] == 0 and rr["pcg"][0, i] != b.pcg[0, i], b.name(i)  # lum -1, q 2
        g = orc.Pcg()
        g.st[0], g.st[1] = int(b.pcg[0, i]), int(b.pcg[1, i])
        g.random()
        assert g.state == int(rr["pcg"][0, i])
    assert all(plain["status"][i] == 0 and rr["status"][i] == 0 for i in on(5))
    for w in (plain, rr):
        miss = ~b.hit
        assert np.all(w["status"][miss] == -1) and np.array_equal(w["pcg"][:, miss], b.pcg[:, miss]) and np.all(w["status"][~miss] >= 0)
    # the draws aimed at the roulette and at the diffuse bounce's first draw
    one, zero = X.state_drawing_one(), H.state_drawing_zero()
    gen = np.flatnonzero(b.of("generator") & (b.shape_index == H.MID_SHAPE))
    assert all(rr["status"][i] == 1 for i in gen if int(b.pcg[0, i]) == one) and all(rr["status"][i] == 0 for i in gen if int(b.pcg[0, i]) in (zero, 0))
    black = np.flatnonzero(b.of("generator") & (b.shape_index == H.BLACK_SHAPE))
    assert black.size and all(rr["status"][i] == 0 and not rr["weight"][i].any() for i in black)  # a draw EQUAL to q = 1.0 ends the path
    for i in gen:
        if int(b.pcg[0, i]) in (one, zero):  # cos_theta 1: the normal itself (ct = 1, st = 0 only scales e1, e2 by 1 and n by 0); cos_theta 0
            assert plain["status"][i] == 1 and np.isfinite(plain["rays"][3:6, i]).all()
