"""Every case of the variant catalogue (tests/variant_catalog.py) on the device, against the oracle (run with ``-m gpu``).

Each case sets its switches (the upload ones before the scene is uploaded), asserts its plan again in this process, renders
through the C-ABI with ray counting on (``pt_stats.kernel`` follows the device's choice between the tree kernel and the
one-queue kernel only when the frame is counted or timed), asserts which kernel did the work and whether pixels were handed
over, and compares frame and ray count with the oracle's ``x*x`` mode.  Bars as in tests/test_gpu_parity.py: bit for bit
where no libm transcendental is involved, else <= 1e-5 relative per channel with one outlier pixel allowed.
"""
import numpy as np
import pytest

from pytracer_amd import abi
from tests import util
from tests import variant_catalog as vc
from tests.test_gpu_fullsize import _path_check
from tests.test_gpu_parity import _uses_libm

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


@pytest.mark.parametrize("cid", [pytest.param(c.id, marks=pytest.mark.slow) if c.slow else c.id for c in vc.CASES])
def test_variant_matches_oracle(dev, oracle, cid):
    case = vc.BY_ID[cid]
    scene, cam, par = vc.scene(case), vc.camera(case), vc.params(case)
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
    print(f"\n[variant] {cid}: plan {list(names)} stats.kernel {st.kernel} handed_over {handed} rays {st.n_rays}")
    assert names == case.kernels
    assert st.kernel == (case.worker if case.worker is not None else info.kernel)
    if case.handover is True:
        assert handed > 0, f"{cid}: no pixel was handed to the tree kernel"
    elif case.handover is False:
        assert handed == 0, f"{cid}: {handed} pixels handed over"
    try:
        ora, n = oracle.render(scene, cam, par, sqr_mode=oracle.SQR_MUL)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)
    assert out.dtype == ora.dtype and out.shape == ora.shape
    npix = out.shape[0] * out.shape[1]
    if case.zero:
        assert not out.any() and int(st.n_rays) == 0 == n
    elif not _uses_libm(scene, par):
        assert util.bits_equal(out, ora), f"{cid}: device != oracle"
        assert out.tobytes() == ora.tobytes()
        assert int(st.n_rays) == n
    elif par.renderer != abi.RENDERER_PATHTRACER:
        err = util.rel_err(out, ora)
        bad = int((err > TOL).any(axis=-1).sum())
        print(f"[variant] {cid}: max rel {err.max():.3e}, outliers {bad}/{npix}")
        assert bad <= 1, f"{cid}: {bad} pixels beyond {TOL}"
        assert int(st.n_rays) == n
    else:
        _path_check(f"[variant] {cid}", out, ora, st.n_rays, n, 1, npix)
        if case.handover:
            assert int(st.n_rays) == n  # (the tree kernel goes on from the record: the ray count is the oracle's)
    print(f"[variant] {cid}: PASS vs oracle")
