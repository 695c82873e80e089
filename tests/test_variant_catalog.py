"""The variant catalogue (tests/variant_catalog.py) on the CPU: every case plans the kernels it names, the catalogue names every
kernel ``pt_plan_kernel_name`` can return and sets every switch of PT_TUNING_TABLE, and every frame gives its kernels real
work on the oracle.  tests/test_gpu_variants.py renders the same cases on the device."""
import numpy as np
import pytest

from pytracer_amd import abi, device
from tests import variant_catalog as vc

CASE_IDS = [c.id for c in vc.CASES]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_plans_exactly_its_kernels(cid):
    case = vc.BY_ID[cid]
    got = vc.plan(case)
    assert vc.plan_names(got) == case.kernels
    if case.worker is not None:
        assert case.kernels[3], "a case that names the kernel doing the work must have an alternative kernel"
    if case.kernels[3]:
        assert case.worker in (vc.PATH, vc.TREE), f"{cid}: which of the two second-pass kernels works is not stated"
    if case.handover is not None:
        assert case.worker is not None
    # a switch case changes what runs: the kernels, a field of the plan it lists, or a place it names where the plan cannot see
    if cid.startswith("sw-"):
        with vc.tuned(vc.Case("base", case.world, case.size, case.params, case.kernels, camera=case.camera)):
            base = device.plan(vc.scene(case), vc.camera(case), vc.params(case))
        differs = vc.plan_names(base) != vc.plan_names(got) or any(getattr(base, f) != getattr(got, f) for f in case.changes)
        assert differs or case.why_not_in_plan, f"{cid}: its switches change nothing the plan reports, and no reason is given"
        assert not (case.changes and not any(getattr(base, f) != getattr(got, f) for f in case.changes)), \
            f"{cid}: {case.changes} unchanged by {case.tuning}"


def test_catalogue_names_every_kernel_the_planner_can_name():
    plannable = vc.plannable_names()
    assert len(plannable) == 37, sorted(plannable)  # (pt_plan.h as of this catalogue: a new name needs a case)
    assert vc.catalogue_names() == plannable, (sorted(plannable - vc.catalogue_names()), sorted(vc.catalogue_names() - plannable))


def test_catalogue_sets_every_switch():
    table = vc.tuning_switches()
    covered = set().union(*(vc.switches(c) for c in vc.CASES if c.id.startswith("sw-")))
    assert covered | set(vc.EXEMPT_SWITCHES) == table, (sorted(table - covered - set(vc.EXEMPT_SWITCHES)),
                                                       sorted((covered | set(vc.EXEMPT_SWITCHES)) - table))
    assert not covered & set(vc.EXEMPT_SWITCHES)
    assert all(vc.EXEMPT_SWITCHES.values())
    defaults = vc.tuning_defaults()
    assert len(defaults) == len(table) and defaults["grid_density"] == 4
    for c in vc.CASES:
        for name, value in c.tuning.items():
            assert value != defaults[name], f"{c.id}: {name}={value} is the default"


def test_alternative_kernels_are_seen_doing_the_work_and_handing_over():
    """For each one-queue kernel: a case where it does all the work, one where it hands pixels to the tree kernel; for each
    tree kernel planned behind one, a case where the tree kernel does the work."""
    alts = {c.kernels[3] for c in vc.CASES if c.kernels[3]}
    for alt in alts:
        mine = [c for c in vc.CASES if c.kernels[3] == alt]
        assert any(c.worker == vc.PATH and c.handover is False for c in mine), alt
        assert any(c.worker == vc.PATH and c.handover is True for c in mine), alt
    for main in {c.kernels[2] for c in vc.CASES if c.kernels[3]}:
        assert any(c.kernels[2] == main and c.worker == vc.TREE for c in vc.CASES), main


def test_frames_cover_the_edges():
    sizes = [c.size for c in vc.CASES]
    assert sum(w % 8 != 0 and h % 8 != 0 for w, h in sizes) >= len(sizes) - 2
    ps = [vc.params(c) for c in vc.CASES]
    assert any(p.samples_per_side == 0 for p in ps) and any(p.samples_per_side > 0 for p in ps)
    path = [p for p in ps if p.renderer == abi.RENDERER_PATHTRACER and p.max_depth >= 0]
    assert {p.pcg_mode for p in path} >= {abi.PCG_PIXEL, abi.PCG_SAMPLE}
    assert {p.samples_per_side == 0 for p in path} == {True, False}
    shares = [p for p in ps if p.n_ranks > 1]
    assert any(p.row_block % 16 == 0 for p in shares) and any(p.row_block % 16 != 0 for p in shares)
    assert any(p.out_format == abi.OUT_F32 for p in ps)
    assert {c.camera for c in vc.CASES} == {"perspective", "orthogonal"}


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_does_real_work_on_the_oracle(oracle, cid):
    case = vc.BY_ID[cid]
    scene, cam, par = vc.scene(case), vc.camera(case), vc.params(case)
    ora, n = oracle.render(scene, cam, par, sqr_mode=oracle.SQR_MUL)
    oracle.set_sqr_mode(oracle.SQR_POW)
    rows = vc.rows(case)
    npix = len(rows) * par.width
    assert ora.shape[:2] == (len(rows), par.width) and npix > 0
    if case.zero:
        assert not ora.any() and n == 0
        return
    # no frame is all one colour (all sky, all background)
    flat = np.ascontiguousarray(ora, dtype=np.float64).reshape(-1, 3)
    _, counts = np.unique(flat, axis=0, return_counts=True)
    assert counts.max() <= 0.98 * npix, f"{cid}: {counts.max()} of {npix} pixels share one colour"
    nsamp = max(par.samples_per_side, 1) ** 2
    if par.renderer != abi.RENDERER_PATHTRACER:
        return
    assert n > npix * nsamp, f"{cid}: {n} rays for {npix} pixels x {nsamp} samples: nothing scattered"
    info = vc.plan(case)
    if case.kernels[3]:
        # pixels the first pass flags (their primary ray hit a shape that scatters): a flagged pixel traces at most
        # N + N^2 + ... + N^D rays per sample beyond its primary one
        tree = nsamp * sum(par.num_of_rays ** d for d in range(1, max(par.max_depth, 1) + 1))
        flagged_min = -(-(n - npix * nsamp) // tree)
        assert flagged_min >= 1
        if case.worker == vc.TREE:
            assert info.q_min_flagged < 0 or npix < info.q_min_flagged, f"{cid}: the one-queue kernel could take the frame"
        else:
            assert 0 <= info.q_min_flagged <= flagged_min, f"{cid}: the tree kernel could keep the frame"
        if case.handover:
            # a pixel is handed over once it has traced the budget's rays: some pixel must trace more
            assert n - npix * nsamp > 16 * par.num_of_rays
