"""The seed sweep (tests/seed_sweep.py) on the device, against the oracle (run with ``-m gpu``): every swept case under seed
pairs whose per-pixel / per-sample sum crosses 2^32, 2^63 and 2^64 inside the frame, and the SEQ alignment with seeds up
to 2^64 - 1.  tests/test_seed_sweep.py (CPU) holds the conditions under which a frame equal to the oracle's means that all
64 bits of both seeds arrived: the oracle's frames are checked against an independent derivation there, and differ on
both sides of the crossing from the frames truncated or shifted seeds give.

Each case runs exactly as tests/test_gpu_variants.py runs it, with that file's bars (imported, not restated): bit for bit
where no libm transcendental is involved, else <= 1e-5 relative per channel with one outlier pixel allowed, the ray count
within ``_path_check``'s margin, and exactly the oracle's for the non-path and the hand-over cases.  A seeding error is not
subtle: every pixel past the crossing that draws a number changes, and the bit-identical share printed here collapses.

The SEQ rows x63 and x64 have ``jitter_seq`` 2^63 - 1 and 2^64 - 1 and states beyond 2^63.  include/ptrace.h used to say
"< 2^63" of the jitter seeds; nothing in csrc/ptrace.hip enforced or needed that (``pcg_seed`` and ``pcg_advance64`` are
64-bit throughout), these rows equal the serial oracle, and the clause is gone from the header's comment.
"""
import numpy as np
import pytest

from pytracer_amd import abi
from tests import seed_sweep as ss
from tests import util
from tests import variant_catalog as vc
from tests.test_gpu_fullsize import _path_check
from tests.test_gpu_hits import _bits, camera_of, flat_of
from tests.test_gpu_parity import _uses_libm
from tests.test_gpu_variants import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


@pytest.mark.parametrize("cid,name,mode", ss.SWEEP, ids=[ss.sweep_id(*s) for s in ss.SWEEP])
def test_swept_case_matches_oracle(dev, oracle, cid, name, mode):
    case = vc.BY_ID[cid]
    tag = f"[seeds] {ss.sweep_id(cid, name, mode)}"
    scene, cam, par = vc.scene(case), vc.camera(case), ss.params(case, name, mode)
    n_cu = dev.device_info(0)[0]
    with vc.tuned(case):
        ds = dev.DeviceScene(scene)
        try:
            info = dev.plan(scene, cam, par, n_cu=n_cu)
            names = vc.plan_names(info)
            ds.set_count_rays(True)
            out = ds.render(cam, par)
            st = ds.stats()
            handed = ds.handed_over()[0] if case.kernels[3] else None
        finally:
            ds.close()
    print(f"\n{tag}: state {par.path_state:#x} seq {par.path_seq:#x} jitter {par.jitter_state:#x} {par.jitter_seq:#x} mode {par.pcg_mode}: "
          f"plan {list(names)} stats.kernel {st.kernel} handed_over {handed} rays {st.n_rays}")
    assert names == case.kernels
    assert st.kernel == (case.worker if case.worker is not None else info.kernel)
    if case.handover is True:
        assert handed > 0, f"{tag}: no pixel was handed to the tree kernel"
    elif case.handover is False:
        assert handed == 0, f"{tag}: {handed} pixels handed over"
    try:
        ora, n = oracle.render(scene, cam, par, sqr_mode=oracle.SQR_MUL)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
    assert out.dtype == ora.dtype and out.shape == ora.shape
    npix = out.shape[0] * out.shape[1]
    if not _uses_libm(scene, par):
        assert util.bits_equal(out, ora), f"{tag}: device != oracle"
        assert out.tobytes() == ora.tobytes()
        assert int(st.n_rays) == n
    elif par.renderer != abi.RENDERER_PATHTRACER:
        err = util.rel_err(out, ora)
        bad = int((err > TOL).any(axis=-1).sum())
        exact = int((np.ascontiguousarray(out, dtype=np.float64).view(np.uint64) ==
                     np.ascontiguousarray(ora, dtype=np.float64).view(np.uint64)).all(axis=-1).sum())
        print(f"{tag}: max rel {err.max():.3e}, outliers {bad}/{npix}, bit-identical pixels {exact}/{npix}")
        assert bad <= 1, f"{tag}: {bad} pixels beyond {TOL}"
        assert int(st.n_rays) == n
    else:
        _path_check(tag, out, ora, st.n_rays, n, 1, npix)
        if case.handover:
            assert int(st.n_rays) == n  # (the tree kernel goes on from the record: the ray count is the oracle's)
    print(f"{tag}: PASS vs oracle")


@pytest.mark.parametrize("cid", ["tile-flat-hier-jitter-share", "tree-lean-scene-share-rb5"])
def test_shares_equal_the_whole_frame_across_the_crossing(dev, cid):
    """x64: the sequence numbers wrap through 2^64 in the middle of a rank's rows.  The three shares of five-row blocks,
    scattered to their rows, are the whole frame bit for bit (the seeds follow the GLOBAL pixel index)."""
    case = vc.BY_ID[cid]
    scene, cam, swept = vc.scene(case), vc.camera(case), ss.params(case, "x64")
    row, _ = ss.crossing_pixel(case)
    assert (row // 5) % 3 != 0, "the crossing is in the share that holds row 0"
    with vc.tuned(case):
        ds = dev.DeviceScene(scene)
        try:
            whole = ds.render(cam, abi.copy_params(swept, n_ranks=1, rank=0))
            H = whole.shape[0]
            assert H == swept.height
            built = np.zeros_like(whole)
            seen = np.zeros(H, dtype=int)
            for rank in range(3):
                p = abi.copy_params(swept, n_ranks=3, rank=rank, row_block=5)
                rows = abi.rows_for_rank(p.height, p.row_block, p.n_ranks, p.rank)
                part = ds.render(cam, p)
                assert part.shape[0] == len(rows)
                built[rows] = part
                seen[rows] += 1
        finally:
            ds.close()
    assert (seen == 1).all()
    same = util.bits_equal_rows(built, whole)
    assert same.all(), f"{cid}: rows {np.flatnonzero(~same).tolist()} of the shares differ from the whole frame"
    assert len(np.unique(whole.reshape(-1, 3), axis=0)) > 20


# ---- hit frames ------------------------------------------------------------------------------------------------------------
HIT_W, HIT_H, HIT_S = 161, 97, 2
HIT_CROSSING = (HIT_H // 2, HIT_W // 2)


def _hit_params(mode, name):
    base = abi.make_params(HIT_W, HIT_H, abi.RENDERER_POINTLIGHT, samples_per_side=HIT_S, pcg_mode=mode, out_format=abi.OUT_F32)
    state, boundary, seq_seq = ss.PAIRS[name]
    if mode == abi.PCG_SEQ:
        return ss.with_seeds(base, state, seq_seq)
    c = ss.crossing_index(base, *HIT_CROSSING)
    return ss.with_seeds(base, state, (boundary - c) & ss.M64)


@pytest.mark.parametrize("name", ss.CROSSING_NAMES)
@pytest.mark.parametrize("mode", [abi.PCG_PIXEL, abi.PCG_SAMPLE, abi.PCG_SEQ], ids=["pixel", "sample", "seq"])
def test_hit_frames_equal_the_oracle(dev, oracle, mode, name):
    """pt_hits.h's seeding, compared as tests/test_gpu_hits.py::test_small_frames_equal_the_oracle compares: hit / miss and
    the shape equal on every sample; rays, t, point and normal bit for bit; a plane's (u, v) bit for bit, a sphere's within
    1e-11 (ocml's atan2 / acos against glibc's)."""
    flat, cam = flat_of("c2p"), camera_of("c2p", HIT_W, HIT_H)
    p = _hit_params(mode, name)
    with dev.DeviceScene(flat) as ds:
        got = ds.render_hits(cam, p, abi.HIT_ALL)
        st = ds.stats()
    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        exp = util.oracle_frame(oracle, flat, cam, p)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
    n = got.shape_index.size
    assert st.kernel == abi.KERNEL_HITS and st.n_pixels * got.nsamp == st.n_rays == n
    assert _bits(got.ray_origin, exp.ray_origin) and _bits(got.ray_dir, exp.ray_dir), "the jitter differs: the seeds did not arrive whole"
    assert np.array_equal(got.shape_index, exp.shape_index), "hit / miss or the winning shape differs on some sample"
    hit = exp.hit
    assert hit.any()
    assert _bits(got.t, exp.t) and np.all(np.isposinf(got.t[~hit]))
    assert _bits(got.point, exp.point) and _bits(got.normal, exp.normal)
    plane = hit & (flat.kind[np.where(hit, exp.shape_index, 0)] == abi.SHAPE_PLANE)
    assert _bits(got.uv[plane], exp.uv[plane]) and _bits(got.uv[~hit], exp.uv[~hit])
    a, b = got.uv[hit & ~plane], exp.uv[hit & ~plane]
    assert np.all(np.abs(a - b) <= 1e-11 * np.maximum(np.abs(a), np.abs(b)) + 1e-300)
