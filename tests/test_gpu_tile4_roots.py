"""Primary rays against a sphere that encloses the camera: no first-root division (csrc/pt_query.h: PT_SPHERE_ROOTS_IN), and
an orthogonal-camera frame for the cone's beam.

The tile kernels take the shorter form for a sphere whose hoisted ``c = |o'|^2 - 1`` is ``<= -0.5``; the frame must stay bit
for bit what shapes.py:103-121 gives.  The worlds below are the smallest the planner tiles (four shapes on): three small
uniform spheres in front of the camera and, around camera and spheres, the enclosing sphere(s) of the case.  Which form every
shape runs is asserted on the CPU from the oracle's own ray origin and the flattened inverse matrices, together with what the
frame shows, so a world that stopped showing its case fails here and not silently.

Flat frames are compared three ways as in tests/test_gpu_tile4_staging.py (oracle in its ``x*x`` mode in fp64 and fp32, the same
frame under ``tile4_lds = 0``, the plan's kernel); OnOff, jittered and point-light frames (``world_query_tile``) with the oracle.
Everything is uniform and diffuse: no libm, every frame bit-exact.
"""
import numpy as np
import pytest

from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm
from tests import util

FRAME = (48, 40)  # 3 x 3 tiles of 16 x 16, the right and the lower ones partly outside
ODD = (33, 17)    # the middle column's direction has d.y = 0: its tile's wave is not `fast` and keeps the old code
INSIDE, OLD = "inside", "old"
STAGED, UNSTAGED = "pt_tile4_kernel<FLAT, LDS>", "pt_tile4_kernel<FLAT, noLDS>"


def _uniform(r, g, b, emit=0.0):
    return hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(r, g, b))), hm.UniformPigment(hm.Color(emit * r, emit * g, emit * b)))


def _small():
    """Three small spheres in front of the camera of scenes.synthetic_camera (its rays start at (-2, 0, 1) and run towards +x), all
    within 1.6 of the world's origin: inside every enclosing sphere below."""
    return [hm.Sphere(hm.translation(hm.Vec(0.3, 0.2, 0.9)) * hm.scaling(hm.Vec(0.2, 0.2, 0.2)), _uniform(0.8, 0.3, 0.2, 0.5)),
            hm.Sphere(hm.translation(hm.Vec(0.5, -0.4, 1.2)) * hm.scaling(hm.Vec(0.15, 0.15, 0.15)), _uniform(0.2, 0.7, 0.3, 0.25)),
            hm.Sphere(hm.translation(hm.Vec(0.2, 0.0, 0.5)) * hm.rotation_x(20.0) * hm.scaling(hm.Vec(0.1, 0.12, 0.1)), _uniform(0.1, 0.2, 0.9, 1.0))]


def _ball(radius):
    """A sphere about the world's origin: the rays start at (-2, 0, 1), so its hoisted c is 5 / radius^2 - 1."""
    return hm.Sphere(hm.scaling(hm.Vec(radius, radius, radius)), _uniform(0.6, 0.5, 0.9, 1.0))


# case -> (the enclosing shapes in front of the three small ones, the form each of them must run)
CASES = {
    "one": ([_ball(50.0)], [INSIDE]),
    "nested": ([_ball(50.0), hm.Sphere(hm.translation(hm.Vec(1.0, 0.0, 0.5)) * hm.scaling(hm.Vec(20.0, 20.0, 20.0)), _uniform(0.3, 0.3, 0.4, 1.0))],
               [INSIDE, INSIDE]),
    "scale-translate": ([hm.Sphere(hm.translation(hm.Vec(2.0, -1.0, 0.5)) * hm.scaling(hm.Vec(9.0, 12.0, 7.0)), _uniform(0.5, 0.4, 0.3, 1.0))], [INSIDE]),
    "rotated": ([hm.Sphere(hm.rotation_z(30.0) * hm.rotation_y(10.0) * hm.scaling(hm.Vec(30.0, 40.0, 50.0)), _uniform(0.2, 0.6, 0.6, 1.0))], [INSIDE]),
    "just-below": ([_ball(3.16244)], [INSIDE]),  # radius^2 = 10 (1 + 1e-4): c = -0.50005
    "just-above": ([_ball(3.16212)], [OLD]),     # radius^2 = 10 (1 - 1e-4): c = -0.49995
    "between": ([_ball(2.6)], [OLD]),            # c = -0.26
    # nobody encloses the camera: a large sphere far ahead for the small ones to stand against
    "outside": ([hm.Sphere(hm.translation(hm.Vec(6.0, 0.0, 1.0)) * hm.scaling(hm.Vec(2.0, 2.0, 2.0)), _uniform(0.4, 0.4, 0.4, 1.0))], [OLD]),
}

_flat = {}


def _scene(case: str) -> abi.FlatScene:
    if case not in _flat:
        w = hm.World()
        for s in CASES[case][0] + _small():
            w.add_shape(s)
        w.add_light(hm.PointLight(hm.Vec(-0.8, 0.6, 1.6), hm.Color(1.0, 0.9, 0.8)))
        _flat[case] = flatten.flatten_world(w)
        assert 4 <= _flat[case].n_shapes <= 6
    return _flat[case]


def _camera(w, h):
    return flatten.flatten_camera(scenes.synthetic_camera(w, h))


def _params(w, h, fmt=abi.OUT_F64, renderer=abi.RENDERER_FLAT, **kw):
    return abi.make_params(w, h, renderer, out_format=fmt, **kw)


def _hoisted_c(scene, origin):
    """c = |invm * o|^2 - 1 of every shape, the full product added left to right (transformations.py:58-86)."""
    m, (x, y, z) = scene.invm, (float(v) for v in origin)
    o = [((x * m[4 * r] + y * m[4 * r + 1]) + z * m[4 * r + 2]) + m[4 * r + 3] for r in range(3)]
    return (o[0] * o[0] + o[1] * o[1] + o[2] * o[2]) - 1.0


_frames = {}


def _hits(oracle, case, size=FRAME):
    if (case, size) not in _frames:
        _frames[case, size] = util.oracle_frame(oracle, _scene(case), _camera(*size), _params(*size))
    return _frames[case, size]


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


# ---- without a device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_case_geometry(oracle, case):
    """Every enclosing shape is on the side of c = -0.5 its case names, every small sphere has the camera outside (c > 0), and
    the frame shows the enclosing shape(s) and the small spheres."""
    scene, frame = _scene(case), _hits(oracle, case)
    c = _hoisted_c(scene, frame.ray_origin[0, 0, 0])
    forms = CASES[case][1]
    for i, form in enumerate(forms):
        assert (c[i] <= -0.5) == (form == INSIDE), f"{case}: shape {i} has c = {c[i]!r}"
    assert (c[len(forms):] > 0.0).all()
    if case == "just-below":
        assert -0.5002 < c[0] <= -0.5
    if case == "just-above":
        assert -0.5 < c[0] < -0.4998
    if case == "between":
        assert -0.5 < c[0] < 0.0
    idx = frame.shape_index[0]
    shown = set(np.unique(idx).tolist())
    assert set(range(len(forms), scene.n_shapes)) <= shown, f"{case}: a small sphere is hidden"
    if case == "nested":
        assert 1 in shown and 0 not in shown  # the inner sphere hides the outer one; both go through the roots
    else:
        assert 0 in shown
    assert (idx >= 0).all() == (case != "outside")  # an enclosing sphere leaves no pixel without a hit


def test_plans():
    """Which kernel runs what: 16 x 16 tiles for pixel-centre rays, the 8 x 8 tile kernel (world_query_tile) otherwise."""
    from pytracer_amd import device

    scene, cam = _scene("one"), _camera(*FRAME)
    name = lambda **kw: device.plan(scene, cam, _params(*FRAME, **kw)).main_kernel  # noqa: E731
    assert name() == STAGED
    assert name(renderer=abi.RENDERER_ONOFF) == "pt_tile4_kernel<ONOFF, noLDS>"
    assert name(samples_per_side=2, pcg_mode=abi.PCG_SAMPLE) == "pt_tile_kernel<FLAT>"
    assert name(renderer=abi.RENDERER_POINTLIGHT) == "pt_tile_kernel<POINTLIGHT>"
    ortho = flatten.flatten_camera(hm.OrthogonalCamera(1.0, hm.translation(hm.Vec(-1.0, 0.0, 1.0))))
    assert device.plan(scene, ortho, _params(17, 17)).main_kernel == "pt_tile_kernel<FLAT, ORTHO>"


def test_the_odd_frame_has_a_wave_that_is_not_fast(oracle):
    d = _hits(oracle, "one", ODD).ray_dir[0]
    assert (d[:, 16, 1] == 0.0).all() and (d[:, :16, 1] != 0.0).all() and (d[:, 17:, 1] != 0.0).all()


# ---- on the device ----------------------------------------------------------------------------------------------------------
def _mul_oracle(oracle, scene, cam, par):
    try:
        return oracle.render(scene, cam, par, sqr_mode=oracle.SQR_MUL)[0]
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def _three_ways(dev, oracle, scene, cam, make_par):
    """fp64 and fp32 frames: staged == oracle == shaded from global memory, bit for bit; the plan names each kernel."""
    saved = dev.get_tuning("tile4_lds")
    try:
        with dev.DeviceScene(scene) as ds:
            for fmt in (abi.OUT_F64, abi.OUT_F32):
                par = make_par(fmt)
                want = _mul_oracle(oracle, scene, cam, par)
                dev.set_tuning("tile4_lds", 1)
                assert dev.plan(scene, cam, par).main_kernel == STAGED
                got = ds.render(cam, par)
                assert ds.stats().kernel == abi.KERNEL_TILE4 and ds.stats().lds_bytes == 384 * scene.n_shapes
                dev.set_tuning("tile4_lds", 0)
                assert dev.plan(scene, cam, par).main_kernel == UNSTAGED
                plain = ds.render(cam, par)
                assert ds.stats().lds_bytes == 0
                assert got.dtype == want.dtype and got.shape == want.shape
                assert got.tobytes() == want.tobytes(), f"fmt {fmt}: staged frame != oracle"
                assert got.tobytes() == plain.tobytes(), f"fmt {fmt}: staged frame != frame shaded from global memory"
    finally:
        dev.set_tuning("tile4_lds", saved)


def _against_oracle(dev, oracle, scene, cam, par, kernel):
    assert dev.plan(scene, cam, par).main_kernel == kernel
    with dev.DeviceScene(scene) as ds:
        got = ds.render(cam, par)
    want = _mul_oracle(oracle, scene, cam, par)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), f"{kernel}: {int((got != want).any(axis=-1).sum())} pixels differ from the oracle"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_flat_frames(dev, oracle, case):
    w, h = FRAME
    _three_ways(dev, oracle, _scene(case), _camera(w, h), lambda fmt: _params(w, h, fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "rotated", "just-below"])
def test_flat_frames_with_every_ray_traced(dev, oracle, case):
    """The dome shortcut off: the tiles that see nothing but the enclosing sphere run its roots too (bench.py's headline)."""
    w, h = FRAME
    scene, cam, par = _scene(case), _camera(w, h), _params(w, h)
    with dev.DeviceScene(scene) as ds:
        ds.set_count_rays(True)
        frames = {}
        for on in (True, False):
            ds.set_dome_shortcut(on)
            frames[on] = ds.render(cam, par)
            assert ds.stats().n_rays == w * h and (ds.stats().n_rays_resolved == 0) == (not on)
        ds.set_dome_shortcut(True)
    want = _mul_oracle(oracle, scene, cam, par)
    assert frames[False].tobytes() == want.tobytes() and frames[True].tobytes() == want.tobytes()


@pytest.mark.gpu
def test_flat_frame_with_a_wave_that_is_not_fast(dev, oracle):
    w, h = ODD
    _three_ways(dev, oracle, _scene("one"), _camera(w, h), lambda fmt: _params(w, h, fmt))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_onoff_frames(dev, oracle, case):
    w, h = FRAME
    out = _against_oracle(dev, oracle, _scene(case), _camera(w, h), _params(w, h, renderer=abi.RENDERER_ONOFF), "pt_tile4_kernel<ONOFF, noLDS>")
    assert out.all() == (case != "outside") and out.any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nested", "rotated", "just-above"])
def test_jittered_frames(dev, oracle, case):
    """S = 2: the 8 x 8 tile kernel, whose world_query_tile replays the survivors for every sample."""
    w, h = FRAME
    par = _params(w, h, samples_per_side=2, pcg_mode=abi.PCG_SAMPLE)
    _against_oracle(dev, oracle, _scene(case), _camera(w, h), par, "pt_tile_kernel<FLAT>")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nested", "rotated", "just-below"])
def test_point_light_frames(dev, oracle, case):
    """Primary rays through world_query_tile with the skip, shadow rays (a per-ray c) through the old code."""
    w, h = FRAME
    out = _against_oracle(dev, oracle, _scene(case), _camera(w, h), _params(w, h, renderer=abi.RENDERER_POINTLIGHT), "pt_tile_kernel<POINTLIGHT>")
    assert len(np.unique(out.reshape(-1, 3), axis=0)) > 20  # (lit and shaded surfaces, not one flat colour)


@pytest.mark.gpu
def test_orthogonal_camera_17x17(dev, oracle):
    """Parallel rays: the cone is a beam whose radius is a quad reduction of its own (rbeam); nothing is hoisted, every
    sphere takes the old roots.  3 x 3 tiles of 8 x 8, the right and the lower ones one pixel wide."""
    cam = flatten.flatten_camera(hm.OrthogonalCamera(1.0, hm.translation(hm.Vec(-1.0, 0.0, 1.0))))
    for case in ("one", "outside"):
        out = _against_oracle(dev, oracle, _scene(case), cam, _params(17, 17), "pt_tile_kernel<FLAT, ORTHO>")
        assert len(np.unique(out.reshape(-1, 3), axis=0)) >= 3
