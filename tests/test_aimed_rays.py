"""The aimed rays of tests/aimed_rays.py do what they say -- on the CPU, so that the GPU tests built on them
(tests/test_gpu_aimed_rays.py, and through ``_stress_rays`` tests/test_gpu_probes.py and tests/test_gpu_rays.py) cannot
silently stop aiming: ``_stress_rays`` once read the planar ``FlatScene.m`` as if it were ``[n, 3, 4]`` and sent every ray
at a scramble of matrix elements, and no test noticed.

The caps below are conditions on the INPUTS of the GPU tests: surface origins on the true surface in long double, grazing
rays that the oracle's exact test of the TARGET hits about half the time (a hit or a miss by rounding), inside rays that hit
their own sphere, segment ends that flip the any-hit verdict.  Measured, 1280 rays per world: classes 0 / 1 / 4 hit their
target in 34-55 % of the rays (class 1 the least: from up to 1e5 spans away the discriminant is all cancellation), class 3 in
80-87 %, every segment end flips, the surface origins are within 7e-14 of |q| = 1.

Structures: every ``*1500`` world gets the grid (``has_grid`` 1), line1500 included: pt_build_grid refuses a grid only when a
cell collects more than 255 spheres or the cells more than 2^23 entries, and the line's grid (capped at 64 cells along the
line, about 64 x 4 x 4 for its 60 x 0.5 x 0.5 box) holds a few dozen spheres per cell."""
import numpy as np
import pytest

from pytracer_amd import abi, device, flatten, scenes

from . import aimed_rays as A

WORLDS = list(A.WORLDS)


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    yield oracle
    oracle.set_sqr_mode(oracle.SQR_POW)


def _own(flat):
    """World.shapes index -> (L, T) of that sphere."""
    L, T = A.sphere_transforms(flat)
    return {int(s): (L[j], T[j]) for j, s in enumerate(A.sphere_indices(flat))}


def test_sphere_transforms_reads_the_planar_layout():
    flat = A.world("shear300")
    L, T = A.sphere_transforms(flat)
    idx = A.sphere_indices(flat)
    assert L.shape == (300, 3, 3) and T.shape == (300, 3) and len(idx) == 300 and flat.n_shapes == 301
    assert flat.kind[300] == abi.SHAPE_PLANE and 300 not in idx
    m, invm = np.asarray(flat.m), np.asarray(flat.invm)
    for j in (0, 7, 299):
        i = int(idx[j])
        for r in range(3):
            for c in range(3):
                assert L[j, r, c] == m[r * 4 + c, i]
            assert T[j, r] == m[r * 4 + 3, i]
        # ... and it IS the forward transform: invm undoes it
        inv = invm[:, i].reshape(3, 4)
        assert np.allclose(inv[:, :3] @ L[j], np.eye(3), atol=1e-9) and np.allclose(inv[:, :3] @ T[j] + inv[:, 3], 0.0, atol=1e-6)
    assert (np.abs(L[:, 0, 1]) > 0).mean() > 0.5  # (sheared: most blocks are full)


@pytest.mark.parametrize("name", WORLDS)
def test_the_same_seed_gives_the_same_bytes(name):
    flat = A.world(name)
    a = A.aimed(flat, 200, 5, A.span_of(flat))
    b = A.aimed(flat, 200, 5, A.span_of(flat))
    c = A.aimed(flat, 200, 6, A.span_of(flat))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].tobytes() != c[0].tobytes()
    assert np.array_equal(a[2], np.arange(200) % 5) and np.isfinite(a[0][:, :7]).all() and np.all(np.isposinf(a[0][:, 7]))
    assert set(np.unique(a[0][a[2] == 2, 6])) == {0.0, 1e-5, 1e-3} and np.all(a[0][a[2] != 2, 6] == 1e-5)
    assert np.all(np.asarray(flat.kind)[a[1]] == abi.SHAPE_SPHERE)
    few = A.aimed(flat, 1280, 5, A.span_of(flat), targets=64)[1]
    assert len(np.unique(few)) == min(64, len(A.sphere_indices(flat)))
    # the world itself: built twice, the same bytes
    A._worlds.pop(name)
    assert A.world(name).same_bits(flat)


@pytest.mark.parametrize("name", WORLDS)
def test_the_rays_are_aimed(orc, name):
    flat = A.world(name)
    b = A.batch(orc, name)
    rays, target, cls = b["rays"], b["target"], b["cls"]
    assert rays.shape == (A.N_RAYS, 8)
    own = _own(flat)
    # class 2: ON the true surface, in long double
    worst = 0.0
    for i in np.nonzero(cls == 2)[0]:
        L, T = own[int(target[i])]
        q = A.object_point(L, T, rays[i, :3])
        qn = np.sqrt((q * q).sum())
        grad = A.inv3(L).T @ (q / qn)  # d|q| / d(origin): the distance to the surface is (|q| - 1) / |grad| to first order
        dist = abs(qn - 1) / np.sqrt((grad * grad).sum())
        size = np.linalg.norm(L @ np.asarray(q / qn, dtype=np.float64))
        worst = max(worst, float(dist / size))
        assert dist <= 1e-12 * size, (i, float(dist), size)
    # the exact test of the TARGET
    hit_own = np.array([orc.shape_intersect(flat, int(target[i]), rays[i]) is not None for i in range(len(rays))])
    share = [float(hit_own[cls == c].mean()) for c in range(5)]
    print(f"{name}: the target is hit by {[f'{s:.0%}' for s in share]} of the classes; surface origins within {worst:.2e} size")
    for c in (0, 1, 4):
        assert 0.25 <= share[c] <= 0.75, (A.CLASSES[c], share[c])
    assert 0.25 <= float(hit_own[np.isin(cls, (0, 1, 4))].mean()) <= 0.75
    assert share[3] >= 0.70
    # class 4: exact zeros in the direction, one component left
    assert np.all((rays[cls == 4, 3:6] != 0).sum(axis=1) == 1)
    # class 1 straddles grid_far_eo (100 x the world's largest coordinate)
    far = np.abs(rays[cls == 1, :3]).max(axis=1) / A.span_of(flat)
    assert (far < 100).sum() > 20 and (far > 100).sum() > 20
    # segment ends: the verdict flips between tmax = t* and the next double
    want, seg, sw = b["want"], b["seg"], b["seg_want"].hit
    m = len(b["seg_of"])
    assert m == int(want.hit.sum()) > A.N_RAYS // 2 and seg.shape == (4 * m, 8)
    t = want.t[b["seg_of"]]
    assert np.array_equal(seg[:m, 7], t) and np.array_equal(seg[m: 2 * m, 7], np.nextafter(t, np.inf))
    assert np.array_equal(seg[2 * m: 3 * m, 7], t * (1.0 - 1e-6)) and np.array_equal(seg[3 * m:, 7], t * (1.0 + 1e-6))
    flips = sw[:m] != sw[m: 2 * m]
    assert flips.mean() >= 0.5 and sw[m: 2 * m].all(), float(flips.mean())
    assert np.array_equal(b["seg_want"].t[m: 2 * m], t)  # (with the end just behind it, the same hit)
    # the world's winners are not only the targets: other shapes get in the way, the plane among them
    assert (want.shape_index[want.hit] != target[want.hit]).any()


@pytest.mark.parametrize("name", WORLDS)
def test_each_world_opens_its_structure(name):
    flat = A.world(name)
    n = A.WORLDS[name][0]
    cam = flatten.flatten_camera(scenes.synthetic_camera(64, 36))
    p = device.plan(flat, cam, abi.make_params(64, 36, abi.RENDERER_PATHTRACER))
    assert p.n_spheres == n == len(A.sphere_indices(flat)) and flat.n_shapes == n + 1
    assert p.ball_levels == (0 if n < 128 else 1)
    assert p.has_grid == (1 if n >= 1024 else 0)
    if name.startswith("shear"):
        assert 0.6 < 1.0 - p.n_diag / n < 0.8  # 70 % sheared
    else:
        assert p.n_diag == n


def test_stress_rays_aim_at_the_true_spheres():
    """tests/test_gpu_probes.py::_stress_rays for the (40, 0, 10.0, 0.05, 2.0) world: kind 1 leaves from the ball of radius
    scale[k] about the TRUE centre of sphere k, kind 2 passes that ball's rim."""
    from tests.test_gpu_probes import _stress_rays, _stress_world

    scene, rays, aim = _stress_rays(_stress_world(40, 0, 10.0, 0.05, 2.0), 3072, 0, 10.0, targets=True)
    assert _stress_rays(_stress_world(40, 0, 10.0, 0.05, 2.0), 3072, 0, 10.0)[1].tobytes() == rays.tobytes()
    assert np.all(np.asarray(scene.kind)[aim] == abi.SHAPE_SPHERE) and len(np.unique(aim)) == 41  # (40 and the dome)
    own = _own(scene)
    kind = np.arange(3072) % 6
    L = np.array([own[int(k)][0] for k in aim])
    c = np.array([own[int(k)][1] for k in aim])
    scale = np.linalg.norm(L, axis=(1, 2)) / np.sqrt(3.0)
    plain = L[:, 0, 1] == 0
    assert np.allclose(scale[plain], L[plain, 0, 0])  # (an unrotated sphere: its radius)
    k1 = kind == 1
    off = np.abs(np.linalg.norm(rays[k1, :3] - c[k1], axis=1) - scale[k1])
    assert off.max() <= 1e-9, float(off.max())
    k2 = kind == 2
    o, d = rays[k2, :3], rays[k2, 3:6]
    oc = c[k2] - o
    along = (oc * d).sum(axis=1) / (d * d).sum(axis=1)
    gap = np.abs(np.linalg.norm(oc - along[:, None] * d, axis=1) - scale[k2]) / scale[k2]
    print(f"kind 1: at most {off.max():.2e} off the ball; kind 2: {float((gap <= 1e-3).mean()):.0%} within 1e-3 radii of the rim")
    assert (gap <= 1e-3).mean() >= 0.25
