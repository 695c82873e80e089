"""Frames whose pixel and sample indices leave 32 bits (tests/frame_geometry.py) on the device (run with ``-m gpu``).

tests/test_frame_geometry.py (CPU) holds the conditions under which a strip equal to the oracle's means something: the
oracle's strips are derived a second way there, and differ from the strips a 32-bit index would give.

* Against the oracle, each case's block of rows at the bars of tests/test_gpu_variants.py and tests/test_gpu_seeds.py (imported,
  not restated): bit for bit with equal ray counts where no libm value enters (OnOff, Flat) and for the "plain" path strips (``PLAIN``), else <= 1e-5 relative per channel
  with one outlier pixel allowed; the path tracer's ray count within ``_path_check``'s margin, exactly the oracle's behind a
  hand-over.  An index error is not subtle: every pixel behind the crossing that draws a number changes.
* Against the device itself, byte for byte: culling off, the dome shortcut off, 8x8 instead of 16x16 tiles, a 16-row block as
  its two 8-row halves.  An index error survives all four (the same wrong generator either way); a cone that lost a shape to
  the fp32 model of the primary rays at these coordinates does not.
* Hit-record frames under PIXEL, SAMPLE and SEQ at 2^32, compared as tests/test_gpu_hits.py compares them at the pixels of
  ``frame_geometry.window`` (either side of the crossing, both ends of every row), and whole against the unculled kernel.
  The RAY planes are bit-identical: they show a pixel coordinate that went through fp32.
* ``pt_output_bytes``, ``pt_hits_bytes`` and ``pt_rows_for_rank`` against Python-integer arithmetic, up to 2^40 pixels and
  2^31 - 1 rows.
* A frame of 2^40 pixels renders; one of 2^40 + 2^20 is refused, as is a SEQ frame of more than 2^63 draws.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from pytracer_amd import _lib, abi
from tests import frame_geometry as fg
from tests import util
from tests import variant_catalog as vc
from tests.test_gpu_fullsize import _path_check
from tests.test_gpu_hits import _bits
from tests.test_gpu_parity import _uses_libm
from tests.test_gpu_variants import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


# "plain" path worlds -- uniform pigments, ``rr_limit > max_depth`` -- are held to the oracle bit for bit with equal ray counts
PLAIN = [c.id for c in fg.CASES if fg.params(c).renderer == abi.RENDERER_PATHTRACER and fg.params(c).rr_limit > fg.params(c).max_depth
         and not _uses_libm(fg.scene(c), abi.copy_params(fg.params(c), renderer=abi.RENDERER_FLAT))]
assert PLAIN == ["regions-plain-31", "regions-plain-32"]


def _oracle_strip(oracle, c):
    try:
        return oracle.render(fg.scene(c), fg.camera(c), fg.oracle_params(c), sqr_mode=oracle.SQR_MUL)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


def _switched(c, **switches):
    return dataclasses.replace(c.case, tuning=dict(c.case.tuning, **switches))


def _same(tag, what, out, other):
    assert other.dtype == out.dtype and other.shape == out.shape
    assert out.tobytes() == other.tobytes(), f"{tag}: {what} changes {int((out != other).any(axis=-1).sum())} of {out.shape[0] * out.shape[1]} pixels"


@pytest.mark.parametrize("cid", [c.id for c in fg.CASES])
def test_strip_matches_oracle_and_the_device_itself(dev, oracle, cid):
    c = fg.BY_ID[cid]
    case = c.case
    tag = f"[geometry] {cid}"
    scene, cam, par = fg.scene(c), fg.camera(c), fg.params(c)
    n_cu = dev.device_info(0)[0]
    ds = dev.DeviceScene(scene)
    try:
        with vc.tuned(case):
            info = dev.plan(scene, cam, par, n_cu=n_cu)
            names = vc.plan_names(info)
            ds.set_count_rays(True)
            out = ds.render(cam, par)
            st = ds.stats()
            handed = ds.handed_over()[0] if case.kernels[3] else None
            ds.set_count_rays(False)
            ds.set_dome_shortcut(False)
            try:
                every_ray = ds.render(cam, par)
            finally:
                ds.set_dome_shortcut(True)
            halves = None
            if c.geo.row_block == 16:
                blk = par.rank
                halves = [ds.render(cam, abi.copy_params(par, row_block=8, n_ranks=-(-par.height // 8), rank=2 * blk + k)) for k in (0, 1)]
        unculled = small_tiles = None
        if case.tuning.get("cull", 1) != 0:
            with vc.tuned(_switched(c, cull=0)):
                # (worlds of fewer than four shapes are never culled: the same kernel, run once more)
                assert vc.plan_names(dev.plan(scene, cam, par, n_cu=n_cu)) != names or "pt_simple_kernel" in names[2]
                unculled = ds.render(cam, par)
        if "pt_tile4_kernel" in case.kernels[2]:
            with vc.tuned(_switched(c, tile4=0)):
                assert "pt_tile_kernel" in dev.plan(scene, cam, par, n_cu=n_cu).main_kernel
                small_tiles = ds.render(cam, par)
    finally:
        ds.close()
    W, H = case.size
    print(f"\n{tag}: {W} x {H}, rows {fg.rows(c)[0]}.., crossing (row, col) {c.crossing}, mode {par.pcg_mode} S {par.samples_per_side}: "
          f"plan {list(names)} stats.kernel {st.kernel} handed_over {handed} rays {st.n_rays}")
    assert names == case.kernels
    assert st.kernel == (case.worker if case.worker is not None else info.kernel)
    if case.handover is True:
        assert handed > 0, f"{tag}: no pixel was handed to the tree kernel"
    elif case.handover is False:
        assert handed == 0, f"{tag}: {handed} pixels handed over"

    # ---- against the oracle ----------------------------------------------------------------------------------------------
    ora, n = _oracle_strip(oracle, c)
    assert out.dtype == ora.dtype and out.shape == ora.shape == (c.geo.row_block, W, 3)
    npix = out.shape[0] * out.shape[1]
    err = util.rel_err(out, ora)
    bad = (err > TOL).any(axis=-1)
    differ = (np.ascontiguousarray(out).view(np.uint8).reshape(npix, -1) != np.ascontiguousarray(ora).view(np.uint8).reshape(npix, -1)).any(axis=1)
    at = fg.crossing_gpix(c) - fg.rows(c)[0] * W
    print(f"{tag}: max rel {err.max():.3e}, outliers {int(bad.sum())}/{npix}, pixels not bit-identical {int(differ.sum())} "
          f"({int(differ[:at].sum())} before the crossing, {int(differ[at:].sum())} from it on), rays {int(st.n_rays)} vs {n} ({int(st.n_rays) - n:+d})")
    if not _uses_libm(scene, par) or cid in PLAIN:
        assert not differ.any(), f"{tag}: device != oracle in {int(differ.sum())} pixels, the first at local index {int(np.flatnonzero(differ)[0])} (crossing at {at})"
        assert int(st.n_rays) == n
    elif par.renderer != abi.RENDERER_PATHTRACER:
        assert int(bad.sum()) <= 1, f"{tag}: {int(bad.sum())} pixels beyond {TOL}"
        assert int(st.n_rays) == n
    else:
        _path_check(tag, out, ora, st.n_rays, n, 1, npix)
        if case.handover:
            assert int(st.n_rays) == n  # (the tree kernel goes on from the record: the ray count is the oracle's)

    # ---- against the device itself ---------------------------------------------------------------------------------------
    _same(tag, "the dome shortcut off", out, every_ray)
    if unculled is not None:
        _same(tag, "culling off", out, unculled)
    if small_tiles is not None:
        _same(tag, "8x8 instead of 16x16 tiles", out, small_tiles)
    if halves is not None:
        assert halves[0].shape[0] == halves[1].shape[0] == 8
        _same(tag, "the block as its two 8-row halves", out, np.concatenate(halves, axis=0))
    print(f"{tag}: PASS")


# ---- hit-record frames -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fg.HIT_CASES, ids=lambda c: c.id)
def test_hit_frames_equal_the_oracle(dev, oracle, c):
    """As tests/test_gpu_hits.py::test_small_frames_equal_the_oracle compares: hit / miss and the shape equal on every sample;
    rays, t, point and normal bit for bit; a plane's (u, v) bit for bit, a sphere's within 1e-11 (ocml's atan2 / acos against
    glibc's).  The whole frame, byte for byte, against the kernel without culling."""
    flat, cam, p = fg.scene(c), fg.camera(c), fg.params(c)
    with vc.tuned(c.case):
        with dev.DeviceScene(flat) as ds:
            got = ds.render_hits(cam, p, abi.HIT_ALL)
            st = ds.stats()
            with vc.tuned(_switched(c, cull=0)):
                plain = ds.render_hits(cam, p, abi.HIT_ALL)
    n = got.shape_index.size
    assert st.kernel == abi.KERNEL_HITS and st.n_pixels * got.nsamp == st.n_rays == n == fg.nsamp(p) * 8 * p.width
    assert all(a.tobytes() == plain.planes()[k].tobytes() for k, a in got.planes().items()), "culling changes the hit frame"
    pixels = fg.window(c)
    lrow, col = np.array([r for r, _ in pixels]), np.array([q for _, q in pixels])
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        exp = fg.oracle_hits(oracle, c, pixels)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)

    def at(plane):
        return np.ascontiguousarray(plane[:, lrow, col])

    assert _bits(at(got.ray_origin), exp["ray_origin"]) and _bits(at(got.ray_dir), exp["ray_dir"]), \
        "the primary rays differ: the index did not arrive whole, or the pixel's coordinates did not"
    assert np.array_equal(at(got.shape_index), exp["shape_index"]), "hit / miss or the winning shape differs on some sample"
    hit = exp["shape_index"] >= 0
    assert hit.any()
    t = at(got.t)
    assert _bits(t, exp["t"]) and np.all(np.isposinf(t[~hit]))
    assert _bits(at(got.point), exp["point"]) and _bits(at(got.normal), exp["normal"])
    plane = hit & (flat.kind[np.where(hit, exp["shape_index"], 0)] == abi.SHAPE_PLANE)
    uv = at(got.uv)
    assert _bits(uv[plane], exp["uv"][plane]) and _bits(uv[~hit], exp["uv"][~hit])
    a, b = uv[hit & ~plane], exp["uv"][hit & ~plane]
    assert np.all(np.abs(a - b) <= 1e-11 * np.maximum(np.abs(a), np.abs(b)) + 1e-300)
    print(f"\n[geometry] {c.id}: {len(pixels)} pixels x {got.nsamp} samples equal the oracle's, {int(hit.sum())} of them hits; culled == unculled on {n} samples")


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
def _rows(height, row_block, n_ranks, rank):
    """A direct count in Python integers: the rank's blocks ``rank, rank + n_ranks, ...`` one by one, each cut at the frame's
    last row (no closed form: the library's is what is being checked).  One rank owns every row."""
    if n_ranks == 1:
        return height if rank == 0 else 0
    nb = -(-height // row_block)
    return sum(min(row_block, height - b * row_block) for b in range(rank, nb, n_ranks)) if 0 <= rank < n_ranks else 0


SIZES = [fg.params(c) for c in fg.CASES + fg.HIT_CASES] + [
    abi.make_params(2**20, 2**20, abi.RENDERER_FLAT),                                       # 2^40 pixels, one rank
    abi.make_params(2**20, 2**20, abi.RENDERER_FLAT, samples_per_side=12, out_format=abi.OUT_F32, row_block=16, n_ranks=3, rank=2),
    abi.make_params(512, 2**31 - 1, abi.RENDERER_FLAT, samples_per_side=2),                # the tallest frame an int holds
    abi.make_params(512, 2**31 - 1, abi.RENDERER_FLAT, row_block=8, n_ranks=2**28, rank=2**28 - 1),  # ... its last, short block
    abi.make_params(512, 2**31 - 1, abi.RENDERER_FLAT, row_block=1000, n_ranks=7, rank=3),
    abi.make_params(2**31 - 1, 512, abi.RENDERER_FLAT, samples_per_side=1, row_block=5, n_ranks=3, rank=1),
]


def test_sizes_equal_python_integer_arithmetic():
    lib = _lib.lib()
    lib.pt_output_bytes.restype = C.c_size_t
    for p in SIZES:
        rows = _rows(p.height, max(p.row_block, 1), max(p.n_ranks, 1), p.rank)
        if p.height <= 2**27:
            assert rows == len(abi.rows_for_rank(p.height, p.row_block, p.n_ranks, p.rank))
        tag = f"{p.width} x {p.height} rb {p.row_block} ranks {p.n_ranks} rank {p.rank}"
        assert int(lib.pt_rows_for_rank(C.byref(p))) == rows, tag
        assert int(lib.pt_output_bytes(C.byref(p))) == rows * p.width * 3 * (4 if p.out_format == abi.OUT_F32 else 8), tag
        values = fg.nsamp(p) * rows * p.width
        for channels, planes in ((abi.HIT_ALL, 15), (abi.HIT_T, 1), (abi.HIT_RAY | abi.HIT_UV, 8), (0, 0)):
            assert int(lib.pt_hits_bytes(C.byref(p), channels)) == ((values * 4 + 7) & ~7) + values * 8 * planes, (tag, channels)
    assert any(p.width * p.height == 2**40 for p in SIZES) and any(p.height == 2**31 - 1 for p in SIZES)


# ---- the largest frame, and the refusals ----------------------------------------------------------------------------------------
def _one_row(width, height, row, **kw):
    return abi.make_params(width, height, abi.RENDERER_FLAT, row_block=1, n_ranks=height, rank=row, path_state=45, path_seq=54, **kw)


def test_a_frame_of_2_40_pixels_renders(dev, oracle):
    """2^20 x 2^20: one row half-way down (pixel indices from 2^39 on) and the last one (up to 2^40 - 1), jittered per sample."""
    case = vc.BY_ID["tile-flat-share-rb8"]
    scene, cam = vc.scene(case), fg.camera_of("perspective")
    with dev.DeviceScene(scene) as ds:
        for row in (2**19, 2**20 - 1):
            p = _one_row(2**20, 2**20, row, samples_per_side=2, pcg_mode=abi.PCG_SAMPLE)
            ds.set_count_rays(True)
            out = ds.render(cam, p)
            n_dev = int(ds.stats().n_rays)
            try:
                ora, n = oracle.render(scene, cam, p, sqr_mode=oracle.SQR_MUL)
            finally:
                oracle.set_sqr_mode(oracle.SQR_POW)
            assert out.shape == (1, 2**20, 3) and util.bits_equal(out, ora) and n_dev == n == 4 * 2**20, row
        assert len(np.unique(out.reshape(-1, 3), axis=0)) > 3


def test_oversized_frames_are_refused_and_render_nothing(dev):
    case = vc.BY_ID["tile-flat-share-rb8"]
    scene, cam = vc.scene(case), fg.camera_of("perspective")
    lib = _lib.lib()
    # 2^40 + 1 = 257 x 4 278 255 361 has no two ``int`` sides: the smallest step over the limit at this width is one more
    # column, 2^20 more pixels.  That the limit itself is accepted (``>``, not ``>=``) is test_a_frame_of_2_40_pixels_renders.
    too_many_pixels = _one_row(2**20 + 1, 2**20, 2**19)
    assert too_many_pixels.width * too_many_pixels.height == 2**40 + 2**20
    # (1024 samples a side, the most accepted, draw 2^61 numbers in 2^40 pixels: a frame beyond 2^63 draws is beyond 2^40
    # pixels too, and the message tells which check refused it -- the draw count is checked first)
    too_many_draws = _one_row(2**21 + 1, 2**21 + 1, 2**20, samples_per_side=1024, pcg_mode=abi.PCG_SEQ)
    assert 2 * 1024**2 * too_many_draws.width * too_many_draws.height > 2**63
    just_enough_draws = _one_row(2**20, 2**20, 2**19, samples_per_side=1024, pcg_mode=abi.PCG_SEQ)
    assert 2 * 1024**2 * 2**40 <= 2**63
    with dev.DeviceScene(scene) as ds:
        for p, words in ((too_many_pixels, "too large"), (too_many_draws, "2^63")):
            out = np.full((1, p.width, 3), -7.0)
            rc = lib.pt_render(ds._h, C.byref(cam), C.byref(p), out.ctypes.data_as(C.c_void_p), out.nbytes)
            assert rc == -1 and abi.ERROR_NAMES[rc] == "PT_ERR_INVALID" and words in _lib.last_error(), (rc, _lib.last_error())
            assert np.all(out == -7.0), "a refused frame wrote pixels"
            hits = np.full(int(abi.hits_bytes(abi.copy_params(p, samples_per_side=0), abi.HIT_T)), 0x5A, dtype=np.uint8)
            rc = lib.pt_render_hits(ds._h, C.byref(cam), C.byref(p), abi.HIT_T, hits.ctypes.data_as(C.c_void_p), hits.nbytes)
            assert rc == -1 and np.all(hits == 0x5A), (rc, _lib.last_error())
        # (the SEQ bound itself is met by no frame of 2^40 pixels: 1024 samples a side draw 2^61 numbers there)
        assert dev.plan(scene, cam, just_enough_draws).rows == 1
