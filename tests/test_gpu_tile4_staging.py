"""pt_tile4_kernel<FLAT, LDS>: the asynchronous staging copy and the one barrier in front of the shading.

The kernel copies the scene image (records, then aux: 384 bytes per shape) into LDS with 16-byte global -> LDS loads: one
wave-instruction covers 1 024 bytes, a round of the workgroup's four waves 4 096, the plan stages at most six rounds.  Every
wave of a workgroup -- with a tile outside the frame, settled by the dome shortcut, or tracing -- meets the others at one
barrier before anybody reads the image.  The worlds below put the image's end and the records / aux boundary on every side of
those granules, the frames put every kind of wave into one workgroup.

Each frame is compared three ways: bit for bit with the oracle in its ``x*x`` mode (fp64 and fp32 output), bit for bit with
the same frame under ``tile4_lds = 0`` (shading reads global memory), and the plan must name the staged kernel.

Bit-exactness needs worlds without libm: the checkered and the image pigment sit on PLANES (a plane's (u, v) is x - floor(x);
a sphere's goes through atan2 / acos), all spheres are uniform.  The one-shape world is a plane that carries both: a checkered
pigment and an image as its emitted radiance.
"""
import numpy as np
import pytest

from pytracer_amd import abi, flatten, scenes
from pytracer_amd import hostmodel as hm
from tests import util

STAGED, UNSTAGED = "pt_tile4_kernel<FLAT, LDS>", "pt_tile4_kernel<FLAT, noLDS>"
# The planner culls by tiles from four shapes on (pt_plan.h: smaller worlds go to pt_simple_kernel, which stages nothing), so
# the worlds of 1, 2 and 3 shapes cannot reach the staged kernel: they are rendered and compared all the same, their plan is
# asserted to be the simple kernel's, and 4, 5 and 6 shapes put the same edges in front of the staged one.
TILED_FROM, SIMPLE = 4, "pt_simple_kernel<FLAT, HOIST>"
# shapes per world against the copy's granules (384 n bytes; records end at 128 n):
#   1: 384 B, three waves issue nothing            2, 3: into a second chunk, the boundary inside chunk 0
#   4, 5: 1 536 / 1 920 B, a partial second chunk, two waves issue nothing, the boundary inside chunk 0
#   6: 2 304 B, into a third chunk
#   8: exactly three chunks, records exactly one   10, 11: the first lane of a second round
#   32: exactly three rounds                       33 (C2's count), 63
#   64: exactly six rounds, the largest image the plan stages
WORLD_SIZES = (1, 2, 3, 4, 5, 6, 8, 10, 11, 32, 33, 63, 64)
WORLD_FRAME = (48, 40)  # 3 x 3 tiles: two workgroups across and down, the right and the lower ones partly outside


def _texture() -> hm.HdrImage:
    tex = hm.HdrImage(8, 4)
    tex.array[...] = [[[0.1 + 0.1 * x, 0.9 - 0.2 * y, 0.3 + 0.05 * (x + y)] for x in range(8)] for y in range(4)]
    return tex


def _world(n: int) -> hm.World:
    """``n`` shapes: a checkered ground (z = 0) and a ceiling with an image pigment (z = 3) around the first ``n - 2`` shapes
    of the synthetic world (its sky sphere and uniform spheres); ``n = 1``: one ground plane with both pigments."""
    check = hm.CheckeredPigment(hm.Color(0.3, 0.5, 0.1), hm.Color(0.1, 0.2, 0.5), 4)
    image = hm.ImagePigment(_texture())
    w = hm.World()
    if n == 1:
        w.add_shape(hm.Plane(hm.Transformation(), hm.Material(hm.DiffuseBRDF(check), image)))
        return w
    for s in scenes.synthetic_world(max(n - 2, 1)).shapes[:n - 2]:
        w.add_shape(s)
    w.add_shape(hm.Plane(hm.Transformation(), hm.Material(hm.DiffuseBRDF(check), hm.UniformPigment(hm.BLACK))))
    w.add_shape(hm.Plane(hm.translation(hm.Vec(0.0, 0.0, 3.0)), hm.Material(hm.DiffuseBRDF(image), hm.UniformPigment(hm.BLACK))))
    assert len(w.shapes) == n
    return w


_flat = {}


def _scene(n: int) -> abi.FlatScene:
    if n not in _flat:
        _flat[n] = flatten.flatten_world(_world(n))
    return _flat[n]


def _camera(w: int, h: int) -> abi.Camera:
    return flatten.flatten_camera(scenes.synthetic_camera(w, h))


def _params(w: int, h: int, fmt=abi.OUT_F64, **kw) -> abi.Params:
    return abi.make_params(w, h, abi.RENDERER_FLAT, out_format=fmt, **kw)


_wanted = {}


def _oracle(oracle, key, scene, cam, par):
    """The oracle's frame in its x*x mode, computed once per (world, frame, format)."""
    if key not in _wanted:
        try:
            _wanted[key] = oracle.render(scene, cam, par, sqr_mode=oracle.SQR_MUL)[0]
        finally:
            oracle.set_sqr_mode(oracle.SQR_POW)
        _wanted[key].setflags(write=False)
    return _wanted[key]


_seen = {}


def _pigments_on_screen(oracle, n: int):
    """From the oracle's hit records of the world frame: how many pixels show a checkered, an image, a uniform shape."""
    if n not in _seen:
        scene = _scene(n)
        hits = util.oracle_frame(oracle, scene, _camera(*WORLD_FRAME), _params(*WORLD_FRAME))
        idx = hits.shape_index[0]
        hit = idx >= 0
        kinds_p, kinds_e = np.asarray(scene.pig_kind)[idx[hit]], np.asarray(scene.emi_kind)[idx[hit]]
        _seen[n] = (int(((kinds_p == abi.PIGMENT_CHECKERED) | (kinds_e == abi.PIGMENT_CHECKERED)).sum()),
                    int(((kinds_p == abi.PIGMENT_IMAGE) | (kinds_e == abi.PIGMENT_IMAGE)).sum()),
                    int(((kinds_p == abi.PIGMENT_UNIFORM) & (kinds_e == abi.PIGMENT_UNIFORM)).sum()))
    return _seen[n]


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


def _three_ways(dev, oracle, key, scene, cam, make_par):
    """fp64 and fp32 frames: staged == oracle == unstaged, bit for bit; the plan names the staged kernel."""
    saved = dev.get_tuning("tile4_lds")
    try:
        with dev.DeviceScene(scene) as ds:
            for fmt in (abi.OUT_F64, abi.OUT_F32):
                par = make_par(fmt)
                want = _oracle(oracle, key + (fmt,), scene, cam, par)
                tiled = scene.n_shapes >= TILED_FROM
                dev.set_tuning("tile4_lds", 1)
                assert dev.plan(scene, cam, par).main_kernel == (STAGED if tiled else SIMPLE)
                got = ds.render(cam, par)
                if tiled:
                    assert ds.stats().kernel == abi.KERNEL_TILE4 and ds.stats().lds_bytes == 384 * scene.n_shapes
                dev.set_tuning("tile4_lds", 0)
                assert dev.plan(scene, cam, par).main_kernel == (UNSTAGED if tiled else SIMPLE)
                plain = ds.render(cam, par)
                assert ds.stats().lds_bytes == 0
                assert got.dtype == want.dtype and got.shape == want.shape
                assert got.tobytes() == want.tobytes(), f"{key} fmt {fmt}: staged frame != oracle"
                assert got.tobytes() == plain.tobytes(), f"{key} fmt {fmt}: staged frame != frame shaded from global memory"
    finally:
        dev.set_tuning("tile4_lds", saved)


# ---- without a device -------------------------------------------------------------------------------------------------------
def test_plan_stages_up_to_64_shapes():
    """384 n <= 24 KB is staged; n = 65 (24 960 B) is not: the kernel's copy has six unrolled rounds and no more."""
    from pytracer_amd import device

    cam, par = _camera(*WORLD_FRAME), _params(*WORLD_FRAME)
    for n, name in ((64, STAGED), (65, UNSTAGED)):
        info = device.plan(_scene(n), cam, par)
        assert info.main_kernel == name and info.lds_main == (384 * n if name == STAGED else 0)


@pytest.mark.parametrize("n", WORLD_SIZES)
def test_worlds_show_every_pigment(oracle, n):
    """The staged records, aux colours, steps and texture fields are all really read: the oracle's hit records show
    checkered, image and (from three shapes on) uniform pixels in every world's frame."""
    checkered, image, uniform = _pigments_on_screen(oracle, n)
    assert checkered > 0 and image > 0
    assert uniform > 0 or n < 3


# ---- on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", WORLD_SIZES)
def test_world_sizes_against_the_copy_granules(dev, oracle, n):
    checkered, image, _ = _pigments_on_screen(oracle, n)
    assert checkered > 0 and image > 0
    w, h = WORLD_FRAME
    _three_ways(dev, oracle, ("world", n), _scene(n), _camera(w, h), lambda fmt: _params(w, h, fmt))


# frames against the workgroup's 2 x 2 tiles: one pixel; one valid wave and three that only reach the barrier; four valid
# waves, three of them partial; a second workgroup with one valid wave; 3 x 3 tiles
@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 17), (33, 16), (48, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_against_the_workgroup_tiles(dev, oracle, size):
    w, h = size
    _three_ways(dev, oracle, ("frame", w, h), _scene(33), _camera(w, h), lambda fmt: _params(w, h, fmt))


@pytest.mark.gpu
def test_share_of_two_ranks(dev, oracle):
    """Rank 0 of two with row blocks of 16 in a 40-row frame: local rows 0..15 are image rows 0..15, local rows 16..23 are
    image rows 32..39 (a partial tile whose global row is not its local one)."""
    w, h = 33, 40
    assert abi.rows_for_rank(h, 16, 2, 0) == list(range(16)) + list(range(32, 40))
    _three_ways(dev, oracle, ("share", w, h), _scene(33), _camera(w, h), lambda fmt: _params(w, h, fmt, row_block=16, n_ranks=2, rank=0))


def _dome_case():
    """C2's world in ONE workgroup (32 x 32), seen from above its spheres with the camera tilted upwards: the two upper tiles
    see nothing but the surrounding sphere, the two lower ones the spheres and the ground."""
    scene = flatten.flatten_world(scenes.synthetic_world(32, with_plane=True))
    cam = flatten.flatten_camera(hm.PerspectiveCamera(1.0, 1.0, hm.translation(hm.Vec(-1.0, 0.0, 4.0)) * hm.rotation_y(-15.0)))
    return scene, cam


def test_dome_case_geometry(oracle):
    scene, cam = _dome_case()
    idx = util.oracle_frame(oracle, scene, cam, _params(32, 32)).shape_index[0]
    assert (idx[:16] == 0).all(), "the upper tiles must see the surrounding sphere only"
    assert (idx[16:] != 0).any() and (idx[16:, :16] != 0).any() and (idx[16:, 16:] != 0).any()


@pytest.mark.gpu
def test_dome_shortcut_waves_meet_the_others_at_the_barrier(dev, oracle):
    """Waves that took the shortcut and waves that traced sit in one workgroup: some tiles resolved, not all."""
    scene, cam = _dome_case()
    assert scene.n_shapes == 33
    frames = {}
    with dev.DeviceScene(scene) as ds:
        ds.set_count_rays(True)
        for fmt in (abi.OUT_F64, abi.OUT_F32):
            par = _params(32, 32, fmt)
            assert dev.plan(scene, cam, par).main_kernel == STAGED
            want = _oracle(oracle, ("dome", fmt), scene, cam, par)
            for on in (True, False):
                ds.set_dome_shortcut(on)
                got = ds.render(cam, par)
                st = ds.stats()
                print(f"\n[tile4 staging] dome shortcut {on}: rays {st.n_rays} resolved {st.n_rays_resolved}")
                assert st.n_rays == 1024
                if on:
                    assert 0 < st.n_rays_resolved < 1024 and st.n_rays_resolved % 256 == 0
                else:
                    assert st.n_rays_resolved == 0
                assert got.tobytes() == want.tobytes(), f"dome shortcut {on}, fmt {fmt}: frame != oracle"
                frames[(fmt, on)] = got
        ds.set_dome_shortcut(True)
    saved = dev.get_tuning("tile4_lds")
    try:
        dev.set_tuning("tile4_lds", 0)
        with dev.DeviceScene(scene) as ds:
            for fmt in (abi.OUT_F64, abi.OUT_F32):
                assert dev.plan(scene, cam, _params(32, 32, fmt)).main_kernel == UNSTAGED
                assert ds.render(cam, _params(32, 32, fmt)).tobytes() == frames[(fmt, True)].tobytes()
    finally:
        dev.set_tuning("tile4_lds", saved)


@pytest.mark.gpu
def test_three_frames_in_a_row_on_one_handle(dev, oracle):
    """Back to back on one handle into alternating buffers: no frame reads what an earlier one staged or left in flight."""
    import torch

    w, h = WORLD_FRAME
    scene, cam, par = _scene(33), _camera(w, h), _params(w, h)
    want = _oracle(oracle, ("world", 33, abi.OUT_F64), scene, cam, par)
    bufs = [torch.full((h, w, 3), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    outs = []
    with dev.DeviceScene(scene) as ds:
        assert dev.plan(scene, cam, par).main_kernel == STAGED
        for k in range(3):
            ds.render_into(cam, par, bufs[k % 2].data_ptr(), bufs[k % 2].numel() * 8, None)
            outs.append(bufs[k % 2].cpu().numpy().copy())
    for k, o in enumerate(outs):
        assert o.tobytes() == want.tobytes(), f"frame {k} != oracle"
