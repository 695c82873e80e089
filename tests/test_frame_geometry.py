"""The frame-geometry catalogue (tests/frame_geometry.py) on the CPU: the conditions under which a device strip equal to the
oracle's (tests/test_gpu_geometry.py) means that the kernels formed ``gpix``, ``gpix * nsamp + k`` and ``2 * nsamp * gpix`` in 64
bits and the primary rays from exact pixel coordinates.  All of them are conditions on the reference side:

1. every case plans exactly the kernels it names;
2. the crossing pixel lies strictly inside the rendered rows and strictly inside its row, and the index reaches the boundary
   exactly there;
3. every strip shows the sky and the shapes that stand on the horizon (three at least where the world has them), path cases
   have scattering pixels on both sides of the crossing, and the oracle renders the strip in a second or two;
4. the oracle's strip differs from the strips an index kept in an ``unsigned`` or an ``int`` temporary would give -- on both
   sides of the crossing wherever the narrowed index differs there (``MIN_DIFFERING`` states how many pixels at least);
5. pixels on either side of every crossing are derived a second way: the index summed in Python, one ``radiance`` call per
   sample;
6. the oracle's ``tracer_fire_ray`` at these (col, row, W, H) equals the reference's ``ImageTracer.fire_ray`` bit for bit
   (tests/golden/g16_geometry_rays.npz).
"""
import time

import numpy as np
import pytest

from pytracer_amd import abi
from pytracer_amd import hostmodel as hm
from tests import frame_geometry as fg
from tests import util
from tests import variant_catalog as vc

CASE_IDS = [c.id for c in fg.CASES]
JITTERED = [c.id for c in fg.CASES if fg.params(c).samples_per_side > 0 or fg.params(c).renderer == abi.RENDERER_PATHTRACER]

# Condition 4, the least number of pixels of a side that must differ from the strip a narrowed index gives there.
# PathTracer, and PointLight on the gallery's diffuse spheres: every pixel whose primary ray meets a scattering (a lit) surface
# changes with its scattering draws (its jitter).  Asked for: a tenth of the side's pixels that see a shape, their share
# estimated from the sampled hit records of condition 3.
# OnOff, Flat, and PointLight on the three-shape gallery (a mirror and the emitting dome: nothing lit): jitter moves a pixel's
# value only where a silhouette crosses the pixel, and a strip of 8 rows at one elevation has a few dozen such pixels at the
# most.  Asked for: one pixel.  The device's strip is compared with the oracle's bit for bit, so one pixel is what it takes.
MIN_DIFFERING_SHARE = 0.1


# ---- 1, 2: plans, crossings ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_plans_exactly_its_kernels(cid):
    c = fg.BY_ID[cid]
    info = fg.plan(c)
    assert vc.plan_names(info) == c.case.kernels
    p = fg.params(c)
    assert info.rows == len(fg.rows(c)) == c.geo.row_block and info.npix == c.geo.row_block * p.width


@pytest.mark.parametrize("c", fg.CASES + fg.HIT_CASES, ids=lambda c: c.id)
def test_crossing_lies_inside_the_share(c):
    p = fg.params(c)
    W, H = c.case.size
    assert (p.width, p.height) == (W, H) and W % 8 and H % 8 and W % 2 and H % 2, "a frame on the 8 / 16 grid"
    assert W * H <= 2**40
    row, col = c.crossing
    r = fg.rows(c)
    assert r == list(range(r[0], r[0] + c.geo.row_block)) and r[0] % c.geo.row_block == 0 and r[-1] < H
    assert r[0] < row < r[-1] and 0 < col < W - 1
    at, n, bound = fg.crossing_gpix(c), fg.nsamp(p), 1 << c.bits
    assert fg.index_of(p, at) >= bound > fg.index_of(p, at - 1) and fg.index_of(p, fg.before_end(c), n - 1) < bound
    assert at - fg.before_end(c) in (1, 2)
    # small seeds: the index alone carries the high bits, and the ones that play no part are set apart
    seeds = (p.jitter_state, p.jitter_seq) if p.pcg_mode == abi.PCG_SEQ else (p.path_state, p.path_seq)
    assert seeds == fg.SEEDS
    # the catalogue case's own params but for the frame, the share, the alignment and what the entry changes
    base = vc.params(vc.BY_ID[c.geo.base])
    changed = {"width", "height", "row_block", "n_ranks", "rank", "pcg_mode", "jitter_state", "jitter_seq", "path_state", "path_seq"}
    changed |= set(c.geo.params)
    for name, _ in abi.Params._fields_:
        if name not in changed and not name.startswith("_"):
            a, b = getattr(p, name), getattr(base, name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name


def test_every_seeding_site_crosses_both_boundaries():
    """The table in tests/frame_geometry.py's docstring, held to the catalogue: per kernel family and alignment, a case at
    2^31 and one at 2^32 (SEQ: 2^33 as well), and the factor ``nsamp`` greater than one wherever a site multiplies by it."""
    def have(main, mode, nsamp_min=1, first=None):
        return {c.bits for c in fg.CASES if main in c.case.kernels[2] and c.mode == mode and fg.nsamp(fg.params(c)) >= nsamp_min
                and fg.params(c).samples_per_side > (0 if fg.params(c).renderer != abi.RENDERER_PATHTRACER else -1)
                and (first is None or first in c.case.kernels[0] + c.case.kernels[1])}

    for main in ("pt_simple_kernel", "pt_tile_kernel<ONOFF", "pt_tile_kernel<FLAT", "pt_path_kernel", "pt_path_regions_kernel", "pt_path_tree_kernel"):
        assert have(main, fg.P) >= {31, 32}, main
    for main in ("pt_simple_kernel", "pt_tile_kernel<", "pt_path_kernel", "pt_path_regions_kernel", "pt_path_tree_kernel"):
        assert have(main, fg.S, 4) >= {31, 32}, main
    for main in ("pt_simple_kernel", "pt_tile_kernel<ONOFF", "pt_tile_kernel<FLAT>", "pt_tile_kernel<POINTLIGHT", "pt_tile_kernel<FLAT, ORTHO>"):
        assert have(main, fg.Q) >= {32, 33}, main
    assert have("HIER", fg.P, first="pt_cell_kernel") >= {31, 32} and have("ORTHO", fg.P) >= {31, 32} and have("ORTHO", fg.S, 4) >= {31, 32}
    for main in ("pt_tile4_kernel<FLAT, LDS>", "pt_tile4_kernel<FLAT, noLDS>", "pt_tile4_kernel<ONOFF, noLDS>"):
        assert {c.bits for c in fg.CASES if c.case.kernels[2] == main} >= {31, 32}, main
    # the one-queue kernel with and without a hand-over, in both alignments between them; the tree kernel behind it
    queue = [c for c in fg.CASES if c.case.worker == vc.PATH]
    assert {(c.case.handover, c.bits) for c in queue} >= {(True, 31), (True, 32), (False, 31), (False, 32)}
    assert {c.mode for c in queue if c.case.handover} == {fg.P, fg.S}
    # rows beyond 2^24 and columns beyond 2^18; 81 and 144 samples per pixel; an fp32 frame
    assert any(c.crossing[0] > 2**24 for c in fg.CASES) and any(c.crossing[1] > 2**17 and c.case.size[0] > 2**18 for c in fg.CASES)
    assert {fg.nsamp(fg.params(c)) for c in fg.CASES if c.mode == fg.S} >= {1, 4, 81, 144}
    assert any(fg.params(c).out_format == abi.OUT_F32 and c.case.size[0] > 2**18 for c in fg.CASES)
    assert {(c.mode, c.crossing[0] > 2**24) for c in fg.HIT_CASES} >= {(fg.P, True), (fg.S, False), (fg.Q, False)}


# ---- the oracle's strips, rendered once ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strips(oracle):
    """``strips(case, delta)`` -> (the oracle's strip of the case with every index ``delta`` larger, its ray count, seconds)."""
    cache = {}

    def strip(c, delta=0):
        key = (c.id, delta)
        if key not in cache:
            t = time.perf_counter()
            try:
                out, n = oracle.render(fg.scene(c), fg.camera(c), fg.shifted(fg.params(c), delta), sqr_mode=oracle.SQR_MUL)
            finally:
                oracle.set_sqr_mode(oracle.SQR_POW)
            cache[key] = (out, n, time.perf_counter() - t)
        return cache[key]

    yield strip
    cache.clear()


def _first_hits(oracle, c, n_columns=1500):
    """First-hit shape (-1: none) at the pixel centres of ``n_columns`` columns of the crossing row, evenly spread."""
    W, H = c.case.size
    cols = np.unique(np.linspace(0, W - 1, min(n_columns, W)).astype(int))
    scene, cam = fg.scene(c), fg.camera(c)
    shapes = []
    for col in cols:
        rec = oracle.world_intersect(scene, oracle.tracer_fire_ray(cam, W, H, int(col), c.crossing[0]))
        shapes.append(-1 if rec is None else int(rec[9]))
    return cols, np.array(shapes)


def _flagged_pixels(oracle, c, npix):
    """Pixels of the strip that trace more rays than their primary ones (the oracle's per-pixel ray counts): what the first
    pass flags, whose number decides between the tree kernel and the one-queue kernel."""
    return int(_scattering(oracle, c, npix).sum())


def _scattering(oracle, c, npix):
    """Per pixel of the strip (row-major): does it trace more rays than its primary ones?"""
    import ctypes as C

    counts = np.zeros(npix, dtype=np.uint32)
    L = oracle.lib()
    L.pto_set_ray_image.argtypes = [C.c_void_p]
    L.pto_set_ray_image(counts.ctypes.data_as(C.c_void_p))
    try:
        oracle.render(fg.scene(c), fg.camera(c), fg.oracle_params(c), sqr_mode=oracle.SQR_MUL)
    finally:
        L.pto_set_ray_image(None)
        oracle.set_sqr_mode(oracle.SQR_POW)
    return counts > fg.nsamp(fg.params(c))


def _dome_and_planes(c):
    """(index of the sky sphere or None, indices of the planes) of the case's world."""
    key = c.case.world
    has_dome = ((key[0] == "synthetic" and (len(key) <= 4 or key[4])) or key[0] == "rotated"
                or (key[0] == "gallery" and (len(key) < 3 or key[2])))
    dome = 0 if has_dome else None
    kinds = fg.scene(c).kind
    return dome, [i for i in range(len(kinds)) if kinds[i] == abi.SHAPE_PLANE]


# ---- 3: the strips show the world, cheaply -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_strip_shows_sky_and_shapes(oracle, strips, cid):
    c = fg.BY_ID[cid]
    p = fg.params(c)
    out, n, seconds = strips(c)
    npix = len(fg.rows(c)) * p.width
    assert out.shape == (len(fg.rows(c)), p.width, 3)
    print(f"\n[geometry] {cid}: {p.width} x {p.height}, {npix} pixels, {n} rays, oracle {seconds:.2f} s")
    # "a second or two" on 16 cores (the catalogue's convention): the work is bounded by count -- the slowest strips, 8.9 M
    # rays at 144 samples per pixel and the serial SEQ strips of 1.9 M, take 1.5 s to 2.5 s -- and the clock with room for a
    # machine that is busy with other work
    assert n <= 10_000_000 and seconds < 5.0, "the oracle's strip is meant to take a second or two"
    dome, planes = _dome_and_planes(c)
    cols, shapes = _first_hits(oracle, c)
    sky = shapes == (dome if dome is not None else -1)
    others = set(shapes[~sky].tolist()) - {-1}
    standing = len(fg.scene(c).kind) - (dome is not None) - len(planes)  # (no ray along the horizon reaches a ground plane)
    print(f"[geometry] {cid}: sky at {int(sky.sum())} of {len(cols)} sampled columns, first-hit shapes {sorted(others)}")
    assert sky.any(), "no sky in the strip"
    assert len(others) >= min(3, standing), f"{sorted(others)}: fewer than three shapes (of {standing} standing ones) in the strip"
    if p.renderer == abi.RENDERER_PATHTRACER:
        # every shape but the sky scatters (BRDF pigments are not black): these are the pixels the first pass flags.  Sides
        # are taken in row-major order: whole rows lie before and behind the crossing row (test_crossing_lies_inside_the_share),
        # and all rows of a strip show what this one shows; test_pixels_across_the_crossing_a_second_way finds three a side
        assert (~sky).any(), "no scattering pixel in the strip"
        nsamp = fg.nsamp(p)
        assert n > npix * nsamp, "nothing scattered"
        if c.case.kernels[3]:
            info = fg.plan(c)
            tree = nsamp * sum(p.num_of_rays ** d for d in range(1, max(p.max_depth, 1) + 1))
            flagged_min = -(-(n - npix * nsamp) // tree)
            flagged = _flagged_pixels(oracle, c, npix)
            print(f"[geometry] {cid}: {flagged} pixels trace beyond their primary rays, q_min_flagged {info.q_min_flagged}")
            assert flagged >= flagged_min
            if c.case.worker == vc.TREE:
                assert info.q_min_flagged < 0 or flagged < info.q_min_flagged, "the one-queue kernel would take the strip"
            else:
                assert 0 <= info.q_min_flagged <= flagged_min, "the tree kernel could keep the strip"
            if c.case.handover:
                assert n - npix * nsamp > 16 * p.num_of_rays
    some = np.ascontiguousarray(out, dtype=np.float64).reshape(-1, 3)[::max(1, npix // 200_000)]
    _, counts = np.unique(some, axis=0, return_counts=True)
    assert counts.max() <= 0.98 * len(some)


# ---- 4: a 32-bit index gives another strip -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", JITTERED)
def test_strip_depends_on_the_high_bits_of_the_index(oracle, strips, cid):
    """``low32``: the index reduced mod 2^32 (an ``unsigned`` temporary, a ``(unsigned)`` cast); ``sext32``: the same, sign-
    extended (an ``int`` temporary).  On each side of the crossing the narrowed index is the true one plus a multiple of
    2^32 (tests/frame_geometry.py: ``narrowed``): the strip it gives there is the oracle's with every index that much larger.
    Where that multiple is not zero the two strips must differ: in 2^31 frames behind the crossing under ``sext32``; in 2^32
    frames behind it under ``low32`` and on BOTH sides under ``sext32``; in 2^33 frames on both sides under both."""
    c = fg.BY_ID[cid]
    p = fg.params(c)
    W = p.width
    own = np.ascontiguousarray(strips(c)[0]).reshape(-1, 3)
    at = fg.crossing_gpix(c) - fg.rows(c)[0] * W
    end = fg.before_end(c) - fg.rows(c)[0] * W
    cols, shapes = _first_hits(oracle, c)
    dome, _ = _dome_and_planes(c)
    seen = shapes != (dome if dome is not None else -1)
    seen &= shapes != -1
    checked = 0
    for narrow in (fg.low32, fg.sext32):
        for side, delta in zip(("before", "behind"), fg.narrowed(c, narrow)):
            if delta == 0:
                continue
            other = np.ascontiguousarray(strips(c, delta)[0]).reshape(-1, 3)
            sl = slice(0, end + 1) if side == "before" else slice(at, None)
            differs = int((own[sl].view(np.uint8) != other[sl].view(np.uint8)).any(axis=1).sum())
            npix = own[sl].shape[0]
            if p.renderer == abi.RENDERER_PATHTRACER or (p.renderer == abi.RENDERER_POINTLIGHT and c.case.world == ("gallery", 6)):
                least = max(1, int(MIN_DIFFERING_SHARE * float(seen.mean()) * npix))  # (every row shows what the sampled one shows)
            else:
                least = 1
            print(f"\n[geometry] {cid}: {narrow.__name__} {side} the crossing (index {delta:+d}): {differs} of {npix} pixels differ (at least {least})")
            assert differs >= least, f"{cid}: {narrow.__name__} {side} the crossing changes {differs} pixels"
            checked += 1
    assert checked >= {31: 1, 32: 3, 33: 4}[c.bits]


# ---- 5: pixels on either side of the crossing, a second way ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_pixels_across_the_crossing_a_second_way(oracle, strips, cid):
    """Three pixels before and three from the crossing pixel on -- for the path tracer: three that scatter (more than one ray
    per sample) on either side --: the index taken in Python (``frame_geometry.index_of``), generators seeded with the
    sum (PIXEL, SAMPLE) or advanced by it (SEQ, ``hostmodel.pcg_advance``), two jitter draws and ONE ``radiance`` call per
    sample, summed in sample order times 1 / S^2 (imagetracer.py:83-101) == the strip's pixel."""
    c = fg.BY_ID[cid]
    p, cam, scene = fg.params(c), fg.camera(c), fg.scene(c)
    sps, W, H, n = p.samples_per_side, p.width, p.height, fg.nsamp(p)
    image = strips(c)[0]
    first = fg.rows(c)[0]
    at = fg.crossing_gpix(c)
    path = p.renderer == abi.RENDERER_PATHTRACER

    def pixel(gpix):
        r, col = divmod(gpix, W)
        cum, rays, g = np.zeros(3), [], None
        for k in range(n):
            if p.pcg_mode == abi.PCG_SEQ:
                g = oracle.Pcg(p.jitter_state, p.jitter_seq)
                g.st[0] = hm.pcg_advance(g.state, g.inc, fg.index_of(p, gpix, k))
            elif g is None or (p.pcg_mode == abi.PCG_SAMPLE and sps > 0):
                g = oracle.Pcg(p.path_state, (p.path_seq + fg.index_of(p, gpix, k)) & fg.M64)
                h = hm.PCG(p.path_state, (p.path_seq + fg.index_of(p, gpix, k)) & fg.M64)
                assert (g.state, g.inc) == (h.state, h.inc)
            up = vp = 0.5
            if sps > 0:
                up = (k % sps + g.random_float()) / sps
                vp = (k // sps + g.random_float()) / sps
            value, traced = oracle.radiance(scene, p, g, oracle.tracer_fire_ray(cam, W, H, col, r, up, vp))
            cum = cum + value
            rays.append(traced)
        value = cum * (1 / sps ** 2) if sps > 0 else cum
        if p.out_format == abi.OUT_F32:
            value = value.astype(np.float32)
        return value, min(rays), image[r - first, col]

    oracle.set_sqr_mode(oracle.SQR_MUL)
    try:
        if path:
            # the three scattering pixels nearest the crossing on either side, named by the oracle's per-pixel ray counts (a
            # walk over the sky pixels between them would cost a ``radiance`` call each)
            lit = np.flatnonzero(_scattering(oracle, c, image.shape[0] * W)) + first * W
            oracle.set_sqr_mode(oracle.SQR_MUL)
            sides = (lit[lit < at][-3:], lit[lit >= at][:3])
        else:
            sides = (range(at - 3, at), range(at, at + 3))
        for side in sides:
            assert len(side) == 3, f"{cid}: fewer than three scattering pixels on one side of the crossing"
            for gpix in side:
                value, fewest, want = pixel(int(gpix))
                assert not path or fewest >= 1
                assert util.bits_equal(value, want), (gpix, value, want)
    finally:
        oracle.set_sqr_mode(oracle.SQR_POW)


# ---- 6: the primary rays of these frames against the reference's ----------------------------------------------------------------
def test_oracle_rays_equal_the_references(oracle):
    """tests/golden/g16_geometry_rays.npz: ``ImageTracer.fire_ray`` of the reference at the crossing pixels and the corners
    of the frames here -- columns to 262 160, rows to 65 572 020 -- with pixel offsets at and between 0 and 1."""
    g = util.load("g16_geometry_rays")
    want_at = np.array(fg.ray_points(), dtype=np.int64)
    assert g["at"].dtype == np.int64 and np.array_equal(g["at"], want_at), "the fixture's points are not the catalogue's: regenerate it"
    assert g["at"][:, 0].max() > 2**18 and g["at"][:, 1].max() > 2**25
    for j, kind in enumerate(("perspective", "orthogonal")):
        cam = fg.camera_of(kind)
        for i, (col, row, W, H) in enumerate(g["at"].tolist()):
            for k, (up, vp) in enumerate(g["offsets"].tolist()):
                ray = oracle.tracer_fire_ray(cam, W, H, col, row, up, vp)
                assert util.bits_equal(ray[0:6], g["rays"][j, i, k]), (kind, col, row, W, H, up, vp)
