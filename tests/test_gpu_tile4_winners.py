"""pt_tile4_kernel<FLAT, *>: shading once per winning shape of the wave, the per-pixel remainder behind the loop.

The worlds come from tests/tile4_winners.py (tests/test_tile4_winners.py shows on the CPU that each holds what it is named
for): one winner, two winners with lanes that hold both, seven winners in one tile with a plane whose two checkers differ,
image pigments (the remainder) beside uniform spheres (the loop), misses beside hits.  Frames are Flat, S = 0, perspective.

Each frame is compared bit for bit with the oracle in its ``x*x`` mode, in fp64 and fp32, with the dome shortcut on and off,
and bit for bit with the same frame under ``tile4_lds = 0`` (the remainder then reads global memory); the plan must name the
staged kernel.  The world with a checkered SPHERE goes through atan2 / acos: it is held bit for bit to ``tile4_lds = 0`` and to
the oracle within the 1e-5 relative per channel of the family tests (tests/test_gpu_families.py, tests/test_gpu_parity.py).
"""
import numpy as np
import pytest

from pytracer_amd import abi
from tests import tile4_winners as tw
from tests import util

pytestmark = pytest.mark.gpu

STAGED, UNSTAGED = "pt_tile4_kernel<FLAT, LDS>", "pt_tile4_kernel<FLAT, noLDS>"
LIBM_TOL = 1e-5  # tests/test_gpu_parity.py: TOL, the bar of frames that depend on atan2 / acos

_wanted = {}


def _oracle(oracle, key, scene, cam, par):
    """The oracle's frame in its x*x mode, computed once per (world, frame, share, format) and left unchanged."""
    if key not in _wanted:
        try:
            _wanted[key] = oracle.render(scene, cam, par, sqr_mode=oracle.SQR_MUL)[0]
        finally:
            oracle.set_sqr_mode(oracle.SQR_POW)
        _wanted[key].setflags(write=False)
    return _wanted[key]


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


def _three_ways(dev, oracle, key, scene, cam, make_par, bits=True):
    """fp64 and fp32 frames, the dome shortcut on and off: staged == oracle == unstaged, bit for bit (``bits`` False: the
    oracle within LIBM_TOL, the two variants still bit for bit); the plan names the staged kernel."""
    saved = dev.get_tuning("tile4_lds")
    try:
        with dev.DeviceScene(scene) as ds:
            for fmt in (abi.OUT_F64, abi.OUT_F32):
                par = make_par(fmt)
                want = _oracle(oracle, key + (fmt,), scene, cam, par)
                for dome in (True, False):
                    ds.set_dome_shortcut(dome)
                    dev.set_tuning("tile4_lds", 1)
                    assert dev.plan(scene, cam, par).main_kernel == STAGED
                    got = ds.render(cam, par)
                    assert ds.stats().kernel == abi.KERNEL_TILE4 and ds.stats().lds_bytes == 384 * scene.n_shapes
                    dev.set_tuning("tile4_lds", 0)
                    assert dev.plan(scene, cam, par).main_kernel == UNSTAGED
                    plain = ds.render(cam, par)
                    assert ds.stats().lds_bytes == 0
                    assert got.dtype == want.dtype and got.shape == want.shape
                    if bits:
                        assert got.tobytes() == want.tobytes(), \
                            f"{key} fmt {fmt} dome {dome}: {int((got != want).any(axis=-1).sum())} pixels != oracle"
                    else:
                        err = util.rel_err(got, want)
                        print(f"\n[tile4 winners] {key} fmt {fmt} dome {dome}: max rel err {err.max():.3e}")
                        assert np.all(err <= LIBM_TOL), f"{key} fmt {fmt}: max rel {err.max():.3e}"
                    assert got.tobytes() == plain.tobytes(), f"{key} fmt {fmt} dome {dome}: staged frame != frame shaded from global memory"
            ds.set_dome_shortcut(True)
    finally:
        dev.set_tuning("tile4_lds", saved)


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(tw.BIT_EXACT))
def test_worlds_against_the_oracle_and_the_unstaged_kernel(dev, oracle, name, size):
    w, h = size
    scene, cam = tw.scene_and_camera(name, w, h)
    _three_ways(dev, oracle, (name, w, h), scene, cam, lambda fmt: tw.params(w, h, fmt))


@pytest.mark.parametrize("size", tw.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_patterned_sphere_goes_through_the_remainder(dev, oracle, size):
    w, h = size
    scene, cam = tw.scene_and_camera("patterned_sphere", w, h)
    _three_ways(dev, oracle, ("patterned_sphere", w, h), scene, cam, lambda fmt: tw.params(w, h, fmt), bits=False)


@pytest.mark.parametrize("rank", (0, 1))
@pytest.mark.parametrize("name", ("many_winners", "remainder"))
def test_share_of_two_ranks(dev, oracle, name, rank):
    """Row blocks of 16 of the 40-row frame: rank 0 has image rows 0..15 and 32..39 (a partial tile whose global row is not
    its local one), rank 1 the rows 16..31 with the named tile."""
    w, h = 48, 40
    assert abi.rows_for_rank(h, 16, 2, 0) == list(range(16)) + list(range(32, 40)) and abi.rows_for_rank(h, 16, 2, 1) == list(range(16, 32))
    scene, cam = tw.scene_and_camera(name, w, h)
    _three_ways(dev, oracle, (name, w, h, "rank", rank), scene, cam,
                lambda fmt: tw.params(w, h, fmt, row_block=16, n_ranks=2, rank=rank))


def test_three_frames_in_a_row_on_one_handle(dev, oracle):
    """Back to back on one handle into alternating buffers: a frame's loop leaves nothing behind for the next."""
    import torch

    w, h = 48, 40
    scene, cam = tw.scene_and_camera("many_winners", w, h)
    par = tw.params(w, h)
    want = _oracle(oracle, ("many_winners", w, h, abi.OUT_F64), scene, cam, par)
    bufs = [torch.full((h, w, 3), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    outs = []
    with dev.DeviceScene(scene) as ds:
        assert dev.plan(scene, cam, par).main_kernel == STAGED
        for k in range(3):
            ds.render_into(cam, par, bufs[k % 2].data_ptr(), bufs[k % 2].numel() * 8, None)
            outs.append(bufs[k % 2].cpu().numpy().copy())
    for k, o in enumerate(outs):
        assert o.tobytes() == want.tobytes(), f"frame {k} != oracle"
