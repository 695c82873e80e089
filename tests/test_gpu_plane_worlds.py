"""The plane-heavy and light-heavy worlds of tests/plane_worlds.py on the device (run with ``-m gpu``).

* Every frame of every case against the oracle's ``x*x`` mode under the bars of ``test_random_scenes_match_oracle``
  (tests/test_gpu_parity.py): bit-identical frames and equal ray counts where no libm function is on the way, else at most
  one pixel beyond 1e-5 relative; the path-traced frames of the "plain" worlds with ``rr_limit > max_depth`` (no roulette
  decision, no checker cell a last-bit ``sin`` / ``cos`` difference could flip) must have NO outlier.
* The device against itself, byte for byte: culling off, the dome shortcut off, three ranks' shares of 5-row blocks
  reassembled, cell lists off (``hier_min = -1``) above 256 shapes, 8x8 instead of 16x16 tiles at 256.
* Hit-record frames against ``util.oracle_frame``, every channel bit for bit (there are no patterned spheres), culled equal
  to unculled.
* Two coincident planes: the one that comes first in the list wins every pixel under every tile mode.
* 1 to 65 lights under the one-lane-per-pixel and the tile kernel.
* ``lanes_probe`` (the scattered and shadow rays' query) against ``hit_probe`` (every shape) for rays that start on planes,
  run parallel to planes, or cross the room.

tests/test_plane_worlds.py checks on the CPU that these very frames plan the kernels listed and are not vacuous.
"""
import contextlib

import numpy as np
import pytest

from pytracer_amd import abi
from tests import plane_worlds as pw
from tests import util
from tests.test_gpu_parity import TOL, _uses_libm
from tests.test_plane_worlds import cams_of, flat_of, frame_of, names

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    assert device.device_count() >= 1, "no HIP device visible"
    return device


@pytest.fixture(autouse=True)
def default_switches():
    """Every switch of the planner's table at its default from the header for the test, then the values it had: the table is
    process-wide, and whatever the environment or an earlier test left in it must not reach a case (tests/variant_catalog.py)."""
    from pytracer_amd import device
    from tests import variant_catalog as vc

    defaults = vc.tuning_defaults()
    saved = {name: device.get_tuning(name) for name in defaults}
    try:
        for name, value in defaults.items():
            device.set_tuning(name, value)
        yield
    finally:
        for name, value in saved.items():
            device.set_tuning(name, value)


@pytest.fixture()
def mul_oracle(oracle):
    oracle.set_sqr_mode(oracle.SQR_MUL)
    yield oracle
    oracle.set_sqr_mode(oracle.SQR_POW)


@contextlib.contextmanager
def tuned(dev, **switches):
    saved = {name: dev.get_tuning(name) for name in switches}
    try:
        for name, value in switches.items():
            dev.set_tuning(name, value)
        yield
    finally:
        for name, value in saved.items():
            dev.set_tuning(name, value)


def _whole_from_shares(ds, cam, par, row_block=5):
    out = np.empty((par.height, par.width, 3), dtype=np.float64)
    for rank in range(3):
        share = abi.copy_params(par, row_block=row_block, n_ranks=3, rank=rank)
        rows = abi.rows_for_rank(par.height, row_block, 3, rank)
        part = ds.render(cam, share)
        assert part.shape[0] == len(rows) > 0
        out[rows] = part
    return out


def against_oracle(tag, ds, oracle, flat, cam, par, kernels, strict=False):
    """One frame under the fuzz test's bars -> the device's frame."""
    ora, n_rays = oracle.render(flat, cam, par, sqr_mode=oracle.SQR_MUL)
    out = ds.render(cam, par)
    n_dev = int(ds.stats().n_rays)
    err = util.rel_err(out, ora)
    bad = int((err > TOL).any(axis=-1).sum())
    libm = _uses_libm(flat, par)
    print(f"[planes] {tag} renderer {par.renderer} S={par.samples_per_side} N={par.num_of_rays} {'+'.join(k for k in kernels if k)}: "
          f"{'libm' if libm else 'bits'}{', strict' if strict else ''}, max rel {err.max():.3e}, outliers {bad}/{par.width * par.height}, "
          f"rays {n_dev} vs {n_rays}")
    if not libm:
        assert util.bits_equal(out, ora), f"{tag}: {int((out != ora).any(axis=-1).sum())} pixels differ, max rel {err.max():.3e}"
        assert n_dev == n_rays
    else:
        assert bad <= (0 if strict else 1), f"{tag}: {bad} pixels beyond {TOL}, max rel {err.max():.3e}"
    return out


def against_itself(tag, dev, ds, flat, cam, par, out, **switches):
    """Each of ``switches`` (culling off, ...) plans other kernels; they, the dome shortcut off and a 3-rank partition give
    the same bytes."""
    base = names(dev.plan(flat, cam, par))
    for name, value in switches.items():
        with tuned(dev, **{name: value}):
            assert names(dev.plan(flat, cam, par)) != base, (tag, name)
            other = ds.render(cam, par)
        assert out.tobytes() == other.tobytes(), f"{tag}: {name} = {value} changes {int((out != other).any(axis=-1).sum())} pixels"
    ds.set_dome_shortcut(False)
    try:
        every_ray = ds.render(cam, par)
    finally:
        ds.set_dome_shortcut(True)
    assert out.tobytes() == every_ray.tobytes(), f"{tag}: the dome shortcut changes {int((out != every_ray).any(axis=-1).sum())} pixels"
    shares = _whole_from_shares(ds, cam, par)
    assert out.tobytes() == shares.tobytes(), f"{tag}: the 3-rank partition changes {int((out != shares).any(axis=-1).sum())} pixels"


# ---- every case, every frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pw.CASES, ids=lambda c: c.id)
def test_case_frames_match_the_oracle_and_the_device_itself(dev, mul_oracle, case):
    flat, _ = flat_of(case.id)
    assert dev.get_tuning("cull") == 1
    with dev.DeviceScene(flat) as ds:
        for frame in pw.frames_of(case):
            cam, par = frame_of(case, frame)
            assert names(dev.plan(flat, cam, par)) == case.kernels[frame]
            out = against_oracle(f"{case.id} {frame}", ds, mul_oracle, flat, cam, par, case.kernels[frame])
            more = {}
            if case.kernels[frame][0] == "pt_cell_kernel":
                more["hier_min"] = -1
            if case.id == "s0-p256" and frame in ("onoff", "flat"):
                more["tile4"] = 0
            culled = case.n_shapes >= 4 or par.renderer == abi.RENDERER_PATHTRACER  # (else one lane per pixel already)
            against_itself(f"{case.id} {frame}", dev, ds, flat, cam, par, out, **(dict(cull=0, **more) if culled else {}))
            if frame == "flat":
                f32 = ds.render(cam, abi.copy_params(par, out_format=abi.OUT_F32))
                assert f32.dtype == np.float32
                assert np.array_equal(f32, out.astype(np.float32))
        for frame in pw.STRICT_PATH.get(case.id, ()):
            cam, par = frame_of(case, frame, **pw.STRICT)
            assert par.rr_limit > par.max_depth
            assert np.all(flat.pig_kind == abi.PIGMENT_UNIFORM)
            assert np.all(flat.emi_kind == abi.PIGMENT_UNIFORM)
            assert names(dev.plan(flat, cam, par)) == case.kernels[frame]
            against_oracle(f"{case.id} {frame} rr_limit {par.rr_limit}", ds, mul_oracle, flat, cam, par, case.kernels[frame], strict=True)


# ---- hit-record frames ----------------------------------------------------------------------------------------------------------
def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


UV_TOL = 1e-11  # (a sphere's (u, v) goes through atan2 / acos: tests/test_gpu_probes.py, tests/test_gpu_families.py)


def _hit_frames_equal(got, exp, flat=None):
    """Every channel bit for bit; with ``flat`` (device against oracle) a sphere's (u, v) within UV_TOL instead."""
    assert np.array_equal(got.shape_index, exp.shape_index), \
        f"hit / miss or the winning shape differs on {int((got.shape_index != exp.shape_index).sum())} samples"
    for channel in ("t", "ray_origin", "ray_dir", "point", "normal"):
        assert _bits(getattr(got, channel), getattr(exp, channel)), channel
    sphere = np.zeros(exp.shape_index.shape, bool)
    if flat is not None:
        sphere = exp.hit & (flat.kind[np.where(exp.hit, exp.shape_index, 0)] == abi.SHAPE_SPHERE)
    assert _bits(got.uv[~sphere], exp.uv[~sphere]), "uv"
    a, b = got.uv[sphere], exp.uv[sphere]
    assert np.all(np.abs(a - b) <= UV_TOL * np.maximum(np.abs(a), np.abs(b)) + 1e-300), "uv of spheres"


@pytest.mark.parametrize("case_id", pw.HIT_CASES + ("coincident",))
def test_hit_frames_equal_the_oracle_culled_and_unculled(dev, mul_oracle, case_id):
    flat, info = flat_of(case_id)
    size = (75, 45) if case_id == "coincident" else pw.BY_ID[case_id].size
    assert not np.any((flat.kind == abi.SHAPE_SPHERE) & ((flat.pig_kind != abi.PIGMENT_UNIFORM) | (flat.emi_kind != abi.PIGMENT_UNIFORM)))
    with dev.DeviceScene(flat) as ds:
        for camera, S, mode in (("perspective", 0, abi.PCG_PIXEL), ("perspective", 2, abi.PCG_SAMPLE), ("orthogonal", 0, abi.PCG_PIXEL)):
            cam = cams_of(case_id, size)[camera]
            p = abi.make_params(size[0], size[1], abi.RENDERER_FLAT, samples_per_side=S, pcg_mode=mode, path_state=1234, path_seq=77)
            kernels = names(dev.plan_hits(flat, cam, p))
            if case_id != "coincident" and camera == "perspective":
                assert kernels == pw.BY_ID[case_id].kernels["hits"]
            assert "noCULL" not in kernels[2]
            got = ds.render_hits(cam, p, abi.HIT_ALL)
            exp = util.oracle_frame(mul_oracle, flat, cam, p)
            _hit_frames_equal(got, exp, flat)
            with tuned(dev, cull=0):
                assert "noCULL" in dev.plan_hits(flat, cam, p).main_kernel
                plain = ds.render_hits(cam, p, abi.HIT_ALL)
            _hit_frames_equal(plain, got)
            hit = exp.hit
            plane = hit & (flat.kind[np.where(hit, exp.shape_index, 0)] == abi.SHAPE_PLANE)
            # object-space (x, y) of the hit points on planes: both signs, so u = x - floor(x) is taken of negative numbers too
            neg = 0
            for i in np.unique(exp.shape_index[plane]):
                m = flat.invm[:, i].reshape(3, 4)
                q = exp.point[plane & (exp.shape_index == i)] @ m[:2, :3].T + m[:2, 3]
                neg += int((q < 0.0).any(axis=-1).sum())
            print(f"[planes] hits {case_id} {camera} S={S} {kernels}: {int(hit.sum())} hits of {hit.size}, {int(plane.sum())} on planes, "
                  f"{neg} of them at negative object-space x or y")
            assert plane.sum() > hit.size // 20
            assert neg > plane.sum() // 10
            assert np.all((exp.uv[plane] >= 0.0) & (exp.uv[plane] < 1.0))


# ---- the coincident pair ----------------------------------------------------------------------------------------------------------
MODES = {"default": {}, "tile4=0": dict(tile4=0), "hier_min=0": dict(tile4=0, hier_min=0), "cull=0": dict(cull=0)}


@pytest.mark.parametrize("mode", list(MODES))
def test_the_first_of_two_coincident_planes_wins_every_pixel(dev, mul_oracle, mode):
    flat, info = flat_of("coincident")
    i, j = info["pair"]
    switches = MODES[mode]
    main = {"default": "pt_tile4_kernel<FLAT, LDS>", "tile4=0": "pt_tile_kernel<FLAT>", "hier_min=0": "pt_tile_kernel<FLAT, HIER>",
            "cull=0": "pt_simple_kernel<FLAT, HOIST>"}[mode]
    red = flat.pig_c1[:, i] + flat.emi_c1[:, i]
    assert red.tolist() == [0.9, 0.1, 0.1]
    with dev.DeviceScene(flat) as ds, tuned(dev, **switches):
        for size in ((75, 45), (41, 27)):
            for camera in ("perspective", "orthogonal"):
                cam = cams_of("coincident", size)[camera]
                par = abi.make_params(size[0], size[1], abi.RENDERER_FLAT)
                if camera == "perspective":
                    assert dev.plan(flat, cam, par).main_kernel == main
                exp = util.oracle_frame(mul_oracle, flat, cam, par)
                pair = (exp.shape_index[0] == i)
                assert pair.sum() >= 20
                assert not (exp.shape_index == j).any()
                got = ds.render_hits(cam, par, abi.HIT_ALL)
                assert np.array_equal(got.shape_index, exp.shape_index)
                assert _bits(got.t, exp.t)
                out = ds.render(cam, par)
                ora, _ = mul_oracle.render(flat, cam, par, sqr_mode=mul_oracle.SQR_MUL)
                assert util.bits_equal(out, ora)
                assert np.all(out[pair] == red), f"{mode} {camera}: {int((out[pair] != red).any(axis=-1).sum())} pixels of the pair are not the first plane's"
                for renderer, kw in ((abi.RENDERER_POINTLIGHT, {}), (abi.RENDERER_PATHTRACER, pw.C3)):
                    kw = {k: v for k, v in kw.items() if k != "renderer"}
                    par2 = abi.make_params(size[0], size[1], renderer, **kw)
                    against_oracle(f"coincident {mode} {camera}", ds, mul_oracle, flat, cam, par2, names(dev.plan(flat, cam, par2)))


# ---- many lights ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["plain", "closed"])
@pytest.mark.parametrize("n_lights", pw.LIGHT_COUNTS)
@pytest.mark.parametrize("mix", pw.LIGHT_WORLDS, ids=lambda m: f"s{m[0]}-p{m[1]}")
def test_one_to_65_lights_under_the_simple_and_the_tile_kernel(dev, mul_oracle, mix, n_lights, flavour):
    from pytracer_amd import flatten

    flat = flatten.flatten_world(pw.light_world(mix[0], mix[1], n_lights, flavour)[0])
    W, H = pw.LIGHT_SIZE
    with dev.DeviceScene(flat) as ds:
        for camera, S in (("perspective", 0), ("orthogonal", 2)):
            cam = flatten.flatten_camera(pw.cameras(40 + mix[0], pw.LIGHT_SIZE)[camera == "orthogonal"])
            par = abi.make_params(W, H, abi.RENDERER_POINTLIGHT, samples_per_side=S, pcg_mode=abi.PCG_SAMPLE, path_state=9, path_seq=4)
            assert _uses_libm(flat, par) == (flavour == "closed")
            kernels = names(dev.plan(flat, cam, par))
            assert kernels[2] == f"pt_tile_kernel<POINTLIGHT{', ORTHO' if camera == 'orthogonal' else ''}>"
            tag = f"lights s{mix[0]}-p{mix[1]} x{n_lights} {flavour} {camera}"
            out = against_oracle(tag, ds, mul_oracle, flat, cam, par, kernels)
            assert len(np.unique(out.reshape(-1, 3), axis=0)) > 20
            with tuned(dev, cull=0):
                kernels = names(dev.plan(flat, cam, par))
                assert kernels[2].startswith("pt_simple_kernel<POINTLIGHT")
                simple = against_oracle(tag, ds, mul_oracle, flat, cam, par, kernels)
            assert out.tobytes() == simple.tobytes()


# ---- queries without a camera ---------------------------------------------------------------------------------------------------
def query_rays(case, flat, info, pts, nrm):
    """-> ([3 x 1024, 8] rays, the index of the first ray of each group): from surface points ``pts`` with normals ``nrm`` into
    the room and (every fourth) through the surface; parallel to a plane (the image of an object-space (x, y, 0) direction)
    from inside the room; across the room.  The origins of the last two groups lie in a box of half width 1.5 around the
    room's centre: within 2.6 of it, and no plane is nearer than ``info['room']`` >= 3."""
    rng = np.random.default_rng(case.seed)
    planes = np.flatnonzero(flat.kind == abi.SHAPE_PLANE)
    centre = np.array(case.centre)
    rays = []
    for p, n in zip(pts, nrm):
        d = rng.normal(size=3)
        if (d @ n < 0) != (len(rays) % 4 == 3):
            d = -d
        rays.append(list(p) + list(d) + [1e-5, np.inf])
    first = [0, len(rays)]
    for k in range(1024):
        m = flat.m[:, planes[k % len(planes)]].reshape(3, 4)[:, :3]
        d = m @ np.array([rng.normal(), rng.normal(), 0.0])
        rays.append(list(centre + rng.uniform(-1.5, 1.5, size=3)) + list(d) + [1e-5, np.inf])
    first.append(len(rays))
    for k in range(1024):
        rays.append(list(centre + rng.uniform(-1.5, 1.5, size=3)) + list(rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3)) +
                    [1e-5, np.inf if k % 2 else 10.0 ** rng.uniform(-1, 1)])
    rays = np.array(rays)
    inside = np.linalg.norm(rays[first[1]:, :3] - centre, axis=1) < info["room"]
    assert inside.all(), f"{int((~inside).sum())} origins lie outside the room"
    return rays, first


@pytest.mark.parametrize("case_id", pw.QUERY_CASES)
def test_filtered_query_agrees_with_the_exhaustive_one_among_planes(dev, case_id):
    """tests/test_gpu_probes.py's comparison for worlds of planes: rays that start ON a plane (as scattered rays do), rays
    parallel to a plane (d'.z == 0 or a rounding away from it), rays across the room.  Same closest shape, same t to the bit,
    same shadow verdict."""
    case = pw.BY_ID[case_id]
    flat, info = flat_of(case_id)
    cam, par = frame_of(case, "flat")
    with dev.DeviceScene(flat) as ds:
        frame = ds.render_hits(cam, par, abi.HIT_ALL)
        on = np.argwhere(frame.shape_index[0] >= 0)
        on = on[np.random.default_rng(case.seed).permutation(len(on))[:1024]]
        pts, nrm, who = frame.point[0][on[:, 0], on[:, 1]], frame.normal[0][on[:, 0], on[:, 1]], frame.shape_index[0][on[:, 0], on[:, 1]]
        assert (flat.kind[who] == abi.SHAPE_PLANE).sum() > 300
        rays, first = query_rays(case, flat, info, pts, nrm)
        exact = ds.hit_probe(rays, -1)
        lanes = ds.lanes_probe(rays, anyhit=False)
        assert np.array_equal(lanes[:, 0], exact[:, 0]), f"{int((lanes[:, 0] != exact[:, 0]).sum())} rays differ in hit / miss"
        hit = exact[:, 0] != 0
        on_planes = hit & (flat.kind[np.where(hit, exact[:, 10], 0).astype(int)] == abi.SHAPE_PLANE)
        on_spheres = hit & ~on_planes
        per_group = [(int(on_planes[a:b].sum()), int(on_spheres[a:b].sum())) for a, b in zip(first, first[1:] + [len(rays)])]
        print(f"[planes] query {case_id}: {int(hit.sum())} of {len(rays)} rays hit; (planes, spheres) hit from the surface, parallel to a "
              f"plane, across the room: {per_group}")
        # the spheres cover about 0.8 sr by construction (plane_worlds: ``cover``), 6 % of all directions: some 60 of 1024 rays,
        # fewer where half the rays are cut to segments; half of that is asked for
        for n_planes_hit, n_spheres_hit in per_group:
            assert n_planes_hit > 256
        if case.n_spheres:
            assert per_group[1][1] >= 30, "too few rays parallel to a plane meet a sphere"
            assert per_group[2][1] >= 30, "too few rays across the room meet a sphere"
        assert np.array_equal(lanes[hit, 1].view(np.uint64), exact[hit, 1].view(np.uint64))
        assert np.array_equal(lanes[hit, 2], exact[hit, 10])
        # shadow rays: from the surface points towards every light (tmax = 1), and the rays above cut to segments
        seg = rays.copy()
        seg[:, 7] = np.where(np.isfinite(seg[:, 7]), seg[:, 7], 1.0)
        towards = [list(p) + list(flat.light_pos[:, l] - p) + [1e-5, 1.0] for p in pts[:256] for l in range(flat.n_lights)]
        seg = np.concatenate([seg, np.array(towards)])
        blocked = ds.lanes_probe(seg, anyhit=True)[:, 0]
        assert np.array_equal(blocked, ds.hit_probe(seg, -1)[:, 0])
        assert 0 < blocked[len(rays):].sum() < len(towards)
