"""Probe queries on the device (include/ptrace_sh.h, libptrace_sh.so): directions, SH projection and evaluation -- against a numpy
restatement and the CPU oracle in its ``x * x`` mode (tests/probe_sets.py), against the libraries there already were (the device's
own directions, the radiance query, then the host's ordered projection), and against itself across launch shapes and entry points.

Expected agreement.  Directions against libm: 64 eps per component (ocml's sin / cos against glibc's: a few ulp each, one product),
and ``z`` bit for bit.  Against the oracle's composition the entry ray itself holds ocml's sin / cos against glibc's: a probe whose
count differs, or with a coefficient beyond ``TOL * (4 pi / K) * sum_k |Y_j(d_k)| |L_k[ch]|``, is an outlier, of which a case may hold
ONE -- the cap tests/test_sh_host.py vetted on the same cases.  Device against device, and the evaluation against its numpy mirror:
bit for bit, no cap and no tolerance."""
import math

import numpy as np
import pytest

from pytracer_amd import rays as rb

from . import probe_sets as P
from . import radiance_batches as R

pytestmark = pytest.mark.gpu

BG = P.BACKGROUND


@pytest.fixture(scope="module")
def dev():
    from pytracer_amd import device

    if device.device_count() < 1:
        pytest.skip("no HIP device")
    return device


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o

    o.build()
    o.set_sqr_mode(o.SQR_MUL)
    yield o
    o.set_sqr_mode(o.SQR_POW)


@pytest.fixture(scope="module")
def scene_of(dev):
    """name -> the world's DeviceScene, uploaded once for the module."""
    open_ = {}

    def get(name):
        if name not in open_:
            open_[name] = dev.DeviceScene(R.world(name)[0])
        return open_[name]

    yield get
    for ds in open_.values():
        ds.close()


def _probes(ds, pts, K, N, D, limit, seqs=None, active=None, depth=1, channels="all", init_seq=P.SEQ0):
    return rb.WorldQueries(ds).radiance_probes(pts, K, P.S0, init_seq, seqs, active, N, D, limit, BG, depth, channels)


def _chain(ds, pts, seq, K, N, D, limit, depth=1):
    """The libraries there already were: the device's directions, the radiance query on the ``n K`` rays with the generators two
    draws in, the host's ordered projection -> (coefficients [n, 9, 3], count uint64 [n])."""
    wq = rb.WorldQueries(ds)
    n = len(pts)
    dirs = wq.probe_directions(n, K, P.S0, seqs=seq)
    origins = np.repeat(np.asarray(pts, dtype=np.float64), K, axis=0)
    pcg = rb.pcg_streams(P.S0, [(int(q) + k) & P.MASK for q in seq for k in range(K)], skip=2)
    rad = wq.path_radiance(origins, pcg, dirs=dirs.reshape(n * K, 3), num_of_rays=N, max_depth=D, russian_roulette_limit=limit, background=BG,
                           depth=depth, channels="count")
    count = np.asarray(rad.n_rays).reshape(n, K).sum(axis=1, dtype=np.uint64)
    return P.project(dirs, np.asarray(rad.radiance).reshape(n, K, 3)), count


def _same(got, coefficients, count, label):
    c = np.ascontiguousarray(got.coefficients).reshape(-1, 9, 3)
    want = np.ascontiguousarray(coefficients).reshape(-1, 9, 3)
    bad = (c.view(np.uint64) != want.view(np.uint64)).any(axis=(1, 2))
    assert not bad.any(), f"{label}: coefficients differ in {int(bad.sum())} of {c.shape[0]} probes (first: {int(np.flatnonzero(bad)[0])})"
    assert P.same_bits(np.asarray(got.n_rays).reshape(-1), np.asarray(count, dtype=np.uint64).reshape(-1)), f"{label}: counts differ"


# ---- 1. directions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(1, 1), (65, 70)])
def test_directions_against_the_numpy_restatement(scene_of, orc, n, K):
    seq = P.seqs(n)
    got = rb.WorldQueries(scene_of("demo")).probe_directions(n, K, P.S0, seqs=seq)
    u = P.draws(orc, P.S0, seq, K)
    want = P.directions_np(u)
    assert got.shape == (n, K, 3)
    err = np.abs(got - want)
    print(f"directions n={n} K={K}: worst |device - numpy| = {err.max() / P.EPS:.2f} eps")
    assert err.max() <= 64 * P.EPS
    assert P.same_bits(got[..., 2], want[..., 2])  # 1.0 - 2.0 * u1 has no function call in it
    assert np.abs(np.sqrt((got * got).sum(axis=-1)) - 1.0).max() <= 4 * P.EPS
    # without a seqs plane: probe i starts at init_seq + i K
    plain = rb.WorldQueries(scene_of("demo")).probe_directions(n, K, P.S0, init_seq=P.SEQ0)
    again = rb.WorldQueries(scene_of("demo")).probe_directions(n, K, P.S0, seqs=[P.SEQ0 + i * K for i in range(n)])
    assert P.same_bits(plain, again) and P.same_bits(plain[0], got[0])


# ---- 2. bit for bit against the device chain ---------------------------------------------------------------------------------------
NK = ((1, 1), (3, 63), (5, 64), (65, 65), (2, 70), (1, 300))
NDL = ((1, 3, 2), (2, 2, 1), (10, 2, 3))
CHAIN_CASES = [(P.WORLDS[i % 4], NK[i], NDL[i % 3]) for i in range(6)]


@pytest.mark.parametrize("name,nk,ndl", CHAIN_CASES, ids=[f"{w}-n{nk[0]}K{nk[1]}-N{ndl[0]}D{ndl[1]}L{ndl[2]}" for w, nk, ndl in CHAIN_CASES])
def test_the_projection_equals_the_device_chain_bit_for_bit(scene_of, orc, name, nk, ndl):
    (n, K), (N, D, limit) = nk, ndl
    ds = scene_of(name)
    pts, seq = P.many_points(orc, name, n), P.seqs(n)
    want, count = _chain(ds, pts, seq, K, N, D, limit)
    got = _probes(ds, pts, K, N, D, limit, seqs=seq)
    assert got.coefficients.shape == (n, 9, 3) and count.min() >= K
    _same(got, want, count, f"{name} n={n} K={K} N={N} D={D} limit={limit}")


@pytest.mark.parametrize("depth", [0, 1])
def test_the_chain_at_both_entry_depths_with_far_streams_and_skipped_probes(scene_of, orc, depth):
    """``depth0`` 0 and 1; a ``seqs`` plane with values beyond 2^63 (the sums wrap); an ``active`` plane: a skipped probe is zeros
    and count 0, and its neighbours are what they are without it."""
    name, n, K, N, D, limit = "pigments", 9, 5, 2, 2, 1
    ds = scene_of(name)
    pts = P.many_points(orc, name, n)
    seq = rb.stream_numbers([2 ** 63 + 12345 * i for i in range(n - 2)] + [2 ** 64 - 3, 2 ** 64 - 1])  # (the last two wrap inside their K)
    want, count = _chain(ds, pts, seq, K, N, D, limit, depth)
    got = _probes(ds, pts, K, N, D, limit, seqs=seq, depth=depth)
    _same(got, want, count, f"depth0={depth}")
    active = np.array([0, -1, 3, -7, 0, 0, -1, 5, 0], np.int32)
    part = _probes(ds, pts, K, N, D, limit, seqs=seq, active=active, depth=depth)
    skipped = active < 0
    assert not part.coefficients[skipped].any() and not np.signbit(part.coefficients[skipped]).any() and not part.n_rays[skipped].any()
    assert P.same_bits(part.coefficients[~skipped], got.coefficients[~skipped]) and P.same_bits(part.n_rays[~skipped], got.n_rays[~skipped])
    # the default stream numbers are init_seq + i K
    plain = _probes(ds, pts, K, N, D, limit, depth=depth, init_seq=1000)
    listed = _probes(ds, pts, K, N, D, limit, seqs=[1000 + i * K for i in range(n)], depth=depth)
    assert plain.buffer.tobytes() == listed.buffer.tobytes()


# ---- 3. against the oracle's composition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,D,limit", P.ORACLE_CASES)
@pytest.mark.parametrize("name", P.WORLDS)
def test_the_projection_equals_the_oracles_composition(scene_of, orc, name, K, N, D, limit):
    want = P.expected(orc, name, K, N, D, limit)
    pts = P.points(orc, name)
    got = _probes(scene_of(name), pts, K, N, D, limit, seqs=P.seqs(len(pts)))
    bad, worst = P.outliers(got.coefficients, got.n_rays, want)
    same = (np.ascontiguousarray(got.coefficients).view(np.uint64) == want["coefficients"].view(np.uint64)).mean()
    print(f"probes {name} K={K} N={N} D={D} limit={limit}: {int(want['count'].sum())} traced, outliers {int(bad.sum())} of {len(pts)}, "
          f"worst |difference| / bar {worst:.3g} (bar: TOL = {P.TOL:g} of the sum of magnitudes), bit-identical coefficients {same:.1%}")
    assert bad.sum() <= P.MAX_OUTLIERS, f"{int(bad.sum())} outlier probes ({np.flatnonzero(bad).tolist()}), worst {worst:.3g}"


# ---- 4. the shape of the launch ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2_set(scene_of, orc):
    """130 probes of c2 at K = 10, N = 2: 1300 samples -- six workgroups of the walk, three of the projection"""
    n, K = 130, 10
    pts, seq = P.many_points(orc, "c2", n), P.seqs(n)
    full = _probes(scene_of("c2"), pts, K, 2, 2, 1, seqs=seq)
    assert len(np.unique(full.coefficients.reshape(n, 27), axis=0)) > 100 and full.n_rays.min() >= K
    return pts, seq, K, full


def test_sub_batches_give_the_same_bits(scene_of, c2_set):
    pts, seq, K, full = c2_set
    ds = scene_of("c2")
    for a, b in ((0, 1), (1, 64), (64, 65), (65, 130)):
        part = _probes(ds, pts[a:b], K, 2, 2, 1, seqs=seq[a:b])
        _same(part, full.coefficients[a:b], full.n_rays[a:b], f"probes [{a}, {b})")


def test_a_launch_capped_at_one_workgroup_gives_the_same_bits(scene_of, c2_set, monkeypatch):
    pts, seq, K, full = c2_set
    ds = scene_of("c2")
    planes = 130 * K * 56
    assert ds.sh_workspace_bytes(130, K, 2, 2, 1) == 1536 * 20 * 1 * 8 + planes  # 1300 samples: six workgroups of 256
    monkeypatch.setenv("PTRACE_SH_LANES", "256")
    assert ds.sh_workspace_bytes(130, K, 2, 2, 1) == 256 * 20 * 1 * 8 + planes
    assert ds.sh_workspace_bytes(7, 3, 1, 4, 1) == 256 * 6 * 3 * 8 + 7 * 3 * 56
    capped = _probes(ds, pts, K, 2, 2, 1, seqs=seq)
    monkeypatch.delenv("PTRACE_SH_LANES")
    assert capped.buffer.tobytes() == full.buffer.tobytes()


def test_probes_that_stay_in_hbm_and_the_count_channel(dev, scene_of, c2_set):
    """``sh_project(device=True)`` on device tensors with a caller-owned workspace, output buffer and stream, twice into the same
    buffers: byte for byte the host form.  Without PT_SH_COUNT the buffer has 27 planes, and they are the same."""
    import torch

    from pytracer_amd import _lib, _sh_lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    pts, seq, K, full = c2_set
    n = len(pts)
    ds = scene_of("c2")
    L = _sh_lib.lib()
    st = Stream()
    try:
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        pts_d, seq_d = to_dev(rb.planar(pts, 3)), to_dev(seq.view(np.int64))
        torch.cuda.synchronize()
        need = ds.sh_workspace_bytes(n, K, 2, 2, 1)
        ws = DeviceBuffer((need,), np.uint8)
        mine = DeviceBuffer((rb.sh_bytes(n, rb.SH_ALL),), np.uint8)
        args = (K, P.S0, P.SEQ0, seq_d, None, 2, 2, 1, BG, 1)
        for turn in range(2):
            out = ds.sh_project(pts_d, *args, "all", device=True, stream=st, out=mine, workspace=ws)
            assert out is mine
            assert mine.numpy().tobytes() == full.buffer.tobytes(), f"turn {turn}: the probes in HBM differ from the probes through the host form"
        bare = _probes(ds, pts, K, 2, 2, 1, seqs=seq, channels="none")
        assert bare.buffer.nbytes == L.pt_rays_sh_bytes(n, 0) == 216 * n and full.buffer.nbytes == L.pt_rays_sh_bytes(n, 1) == 224 * n
        assert bare.buffer.tobytes() == full.buffer[: 216 * n].tobytes() and not bare.has("count")
        assert L.pt_rays_sh_plane_offset(n, 0, rb.SH_COUNT, 0) < 0 and L.pt_rays_sh_plane_offset(n, 1, rb.SH_COUNT, 0) == 216 * n
        small = ds.sh_project(pts_d.data_ptr(), *args, "none", device=True, stream=st, n=n)  # a raw address, the library's own workspace
        assert small.numpy()[: 216 * n].tobytes() == bare.buffer.tobytes()
        # the evaluation in HBM: the coefficient planes where the projection left them
        normals = np.tile(np.array([[0.0, 0.6, 0.8]]), (n, 1))
        nrm_d = to_dev(rb.planar(normals, 3))
        torch.cuda.synchronize()
        ev = ds.sh_eval(mine, nrm_d, None, rb.SH_HEMISPHERE, n=n, device=True, stream=st)
        assert P.same_bits(ev.numpy()[:, :n], ds.sh_eval(full.block, rb.planar(normals, 3), None, rb.SH_HEMISPHERE))
        for kw in (dict(workspace=DeviceBuffer((need - 8,), np.uint8), out=mine), dict(workspace=DeviceBuffer((n * K * 56 - 8,), np.uint8), out=mine),
                   dict(workspace=ws, out=DeviceBuffer((mine.nbytes - 8,), np.uint8))):
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE"):
                ds.sh_project(pts_d, *args, "all", device=True, stream=st, **kw)
        with pytest.raises(ValueError, match="n="):
            ds.sh_project(pts_d.data_ptr(), *args, "all", device=True)
        with pytest.raises(ValueError, match="device=True"):
            ds.sh_project(rb.planar(pts, 3), *args, "all", stream=st)
    finally:
        st.close()


# ---- 5. depths ---------------------------------------------------------------------------------------------------------------------
def test_depths_at_and_beyond_max_depth(scene_of, orc):
    from pytracer_amd import _lib

    name, K, N, D, limit = "pigments", 3, 2, 2, 1
    ds = scene_of(name)
    pts, seq = P.points(orc, name), P.seqs(7)
    deep = _probes(ds, pts, K, N, D, limit, seqs=seq, depth=D + 1)
    assert not deep.buffer.any()  # all zeros, count 0: no ray, and no draw beyond the direction's two
    want, count = _chain(ds, pts, seq, K, N, D, limit, depth=D)
    got = _probes(ds, pts, K, N, D, limit, seqs=seq, depth=D)
    assert np.all(count == K)
    _same(got, want, count, "depth0 == max_depth")
    with pytest.raises(_lib.PtraceError, match="PT_ERR_UNSUPPORTED.*64 levels"):
        _probes(ds, pts, K, N, 66, limit, depth=1)
    assert _probes(ds, pts[:2], 1, 1, 65, 3, depth=1).coefficients.shape == (2, 9, 3)  # 64 levels
    with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*samples"):
        _probes(ds, pts, 0, N, D, limit)
    empty = _probes(ds, np.zeros((0, 3)), K, N, D, limit)
    assert empty.coefficients.shape == (0, 9, 3) and empty.n_rays.shape == (0,)


# ---- 6. hostile points -------------------------------------------------------------------------------------------------------------
def test_hostile_points_beside_ordinary_ones(scene_of, orc):
    """Points of NaN, +-inf and 1e300 among ordinary ones: the call returns (the walk ends by integer counters), and the ordinary
    probes' bits are those of a batch without the hostile ones."""
    name, K, N, D, limit = "pigments", 6, 2, 3, 1
    ds = scene_of(name)
    n = 70
    pts, seq = P.many_points(orc, name, n).copy(), P.seqs(n)
    rows = np.arange(2, n, 5)
    hostile = [(np.nan, 0.0, 0.0), (np.inf, 1.0, 2.0), (0.0, -np.inf, 0.0), (1.0e300, -1.0e300, 1.0e300), (np.nan, np.nan, np.nan),
               (np.inf, -np.inf, np.inf), (0.5, 0.5, 1.7e308)]
    for i, row in enumerate(rows):
        pts[row] = hostile[i % len(hostile)]
    others = np.setdiff1d(np.arange(n), rows)
    got = _probes(ds, pts, K, N, D, limit, seqs=seq)
    clean = _probes(ds, pts[others], K, N, D, limit, seqs=seq[others])
    assert rows.size >= 2 * len(hostile) - 1 and np.isfinite(clean.coefficients).all()
    assert P.same_bits(got.coefficients[others], clean.coefficients) and P.same_bits(got.n_rays[others], clean.n_rays)
    assert np.all(got.n_rays[rows] >= K)  # every sample's entry ray was handed to a query, whatever it met
    for other in ("mirrors", "c2"):  # (a world of mirrors and one of diffuse spheres over a plane: the same batch ends there too)
        assert _probes(scene_of(other), pts, 2, 1, 4, 2, seqs=seq).n_rays.shape == (n,)


# ---- 7. evaluation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 65, 1000])
def test_the_evaluation_equals_its_numpy_mirror_bit_for_bit(scene_of, m):
    ds = scene_of("demo")
    rng = np.random.default_rng(1000 + m)
    n = 37
    block = rng.standard_normal((27, n)) * np.exp(rng.uniform(-3, 3, (27, 1)))
    coeffs = np.moveaxis(block.reshape(9, 3, n), 2, 0)  # [n, 9, 3]
    dirs = rng.standard_normal((m, 3))
    dirs[::3] /= np.linalg.norm(dirs[::3], axis=1, keepdims=True)  # a third of them unit vectors, the rest of any length
    index = rng.integers(0, n, m).astype(np.int32)
    index[::7] = index[0]  # repeated
    for kind in (rb.SH_RADIANCE, rb.SH_HEMISPHERE):
        got = ds.sh_eval(block, rb.planar(dirs, 3), index, kind)
        want = rb.sh_evaluate(coeffs[index], dirs, kind)
        assert got.shape == (3, m) and P.same_bits(got.T, want), (m, kind)
        # out of range: zeros, and the neighbours are unchanged
        wild = index.copy()
        wild[::5] = (-1, n, 2 ** 31 - 1, -2 ** 31)[m % 4]
        some = ds.sh_eval(block, rb.planar(dirs, 3), wild, kind)
        assert not some[:, ::5].any() and not np.signbit(some[:, ::5]).any()
        keep = np.ones(m, bool)
        keep[::5] = False
        assert P.same_bits(some[:, keep], got[:, keep])
        # a NULL index: record r reads probe r
        k = min(m, n)
        plain = ds.sh_eval(block, rb.planar(dirs[:k], 3), None, kind)
        assert P.same_bits(plain.T, rb.sh_evaluate(coeffs[:k], dirs[:k], kind))
    from pytracer_amd import _lib

    with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*index"):
        ds.sh_eval(block, np.zeros((3, n + 1)), None, 0)
    with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID.*kind"):
        ds.sh_eval(block, rb.planar(dirs, 3), index, 2)
    assert ds.sh_eval(block, np.zeros((3, 0)), None, 0).shape == (3, 0)


def test_the_evaluation_of_a_band_limited_field(scene_of):
    """The field of tests/test_sh_host.py through the views: the radiance and the hemisphere mean to 1e-14 of their closed forms."""
    ds = scene_of("demo")
    n = 5
    buf = np.zeros(rb.sh_bytes(n, 0), np.uint8)
    probes = rb.ProbeSet(buf, n, 0, evaluator=ds.sh_eval)
    probes.coefficients[2] = P.field_coefficients()[:, None]
    rng = np.random.default_rng(9)
    d = rng.standard_normal((200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rad, hem = probes.radiance(d, index=2), probes.hemisphere_mean(d, index=2)
    assert np.abs(rad - P.field(d)[:, None]).max() <= 1e-14 and np.abs(hem - P.field_hemisphere(d)[:, None]).max() <= 1e-14
    assert not probes.radiance(d, index=1).any()  # (another probe: zeros)
    # a blend between two probes of a lattice, evaluated with a NULL index
    grid = rb.ProbeGrid((0.0, 0.0, 0.0), 1.0, (5, 1, 1))
    mid = grid.blend(probes, np.array([[1.5, 0.0, 0.0], [2.0, 0.0, 0.0], [2.25, 0.0, 0.0]]))
    got = mid.hemisphere_mean(np.tile(d[:1], (3, 1)))
    assert np.abs(got[:, 0] - np.array([0.5, 1.0, 0.75]) * P.field_hemisphere(d[0])).max() <= 1e-14


# ---- 8. furnace --------------------------------------------------------------------------------------------------------------------
def test_a_furnace_seen_from_inside(dev, orc):
    """A unit sphere seen from inside, uniform emission Le and diffuse albedo rho < 1, no roulette: every ray from every point inside
    brings ``L = Le * sum rho^d``.  Band 0 is that constant to 1e-13; bands 1 and 2 are noise within six sigma of 0; the hemisphere
    mean for any normal is L within what those two imply."""
    from pytracer_amd import flatten

    K, D, depth = P.FURNACE_K, P.FURNACE_D, P.FURNACE_DEPTH
    pts = np.array(P.FURNACE_POINTS)
    with dev.DeviceScene(flatten.flatten_world(P.furnace_world())) as ds:
        got = rb.WorldQueries(ds).radiance_probes(pts, K, P.S0, seqs=P.seqs(len(pts)), num_of_rays=1, max_depth=D, russian_roulette_limit=D + 5,
                                                  background=BG, depth=depth)
        rng = np.random.default_rng(4)
        normals = rng.standard_normal((100, 3))
        normals /= np.linalg.norm(normals, axis=1, keepdims=True)
        means = np.stack([got.hemisphere_mean(normals, index=i) for i in range(len(pts))])  # [3, 100, 3]
    L = P.furnace_radiance()
    rel0, bound0, rest, bound = P.furnace_bounds(got.coefficients)
    print(f"furnace at K={K}: band 0 off by {rel0.max():.3g} (bound {bound0:.3g}, 2 K eps = {2 * K * P.EPS:.3g}); |c_j| / L at most {rest.max():.3g} "
          f"(bound {bound:.3g}); hemisphere means off by at most {np.abs(means / L - 1.0).max():.3g}")
    assert rel0.max() <= bound0 and rest.max() <= bound
    assert np.all(got.n_rays == K * (D - depth + 1))
    # |mean / L - 1| <= band 0's bound + sum_j A_j |Y_j(n)| * the bound on |c_j| / L (+ the nine products' and additions' roundings)
    y = np.abs(rb.sh_basis(normals)) * np.array(rb.SH_BAND_FACTORS)
    allowed = bound0 + y[:, 1:].sum(axis=1) * bound + 32 * P.EPS
    assert np.all(np.abs(means / L - 1.0) <= allowed[None, :, None])
    # the same seeds on the oracle's composition: the host test held them to these bounds before a GPU saw them
    want = P.furnace_expected(orc)
    bad, worst = P.outliers(got.coefficients, got.n_rays, want)
    assert bad.sum() <= P.MAX_OUTLIERS, (int(bad.sum()), worst)


# ---- 9. what it is for: a shape the baked world does not know, lit by a probe ----------------------------------------------------------
def test_the_flat_frame_of_a_world_lit_by_a_probe(dev, orc):
    """One probe inside the furnace; a small diffuse sphere placed at that point gets its map from the probe
    (``outgoing_probe_map``), ``baked_world`` takes the map, and ``FlatRenderer`` at 48 x 36 through ``GpuImageTracer`` is the oracle's
    frame of that world bit for bit -- every pixel on the small sphere the texel under it, which is ``emitted + colour * L`` within the
    furnace's bounds."""
    from pytracer_amd import flatten, scenes
    from pytracer_amd import hostmodel as hm
    from pytracer_amd.tracer import GpuImageTracer

    K, D, depth = P.FURNACE_K, P.FURNACE_D, P.FURNACE_DEPTH
    at, radius, colour, glow = (0.3, 0.1, -0.05), 0.25, (0.6, 0.3, 0.9), (0.0, 0.05, 0.0)
    with dev.DeviceScene(flatten.flatten_world(P.furnace_world())) as ds:
        probes = rb.WorldQueries(ds).radiance_probes(np.array([at]), K, P.S0, num_of_rays=1, max_depth=D, russian_roulette_limit=D + 5,
                                                     background=BG, depth=depth)
        world = P.furnace_world()
        world.add_shape(hm.Sphere(hm.translation(hm.Vec(*at)) * hm.scaling(hm.Vec(radius, radius, radius)),
                                  hm.Material(hm.DiffuseBRDF(hm.UniformPigment(hm.Color(*colour))), hm.UniformPigment(hm.Color(*glow)))))
        with dev.DeviceScene(flatten.flatten_world(world)) as both:
            lit = rb.WorldQueries(both).outgoing_probe_map(1, 16, 8, probes)
    L = P.furnace_radiance()
    want_map = np.array(glow) + np.array(colour) * L
    slack = np.array(colour) * L * (1e-13 + 6.0 * math.sqrt(4.0 * math.pi / K) * (3 * (2.0 / 3.0) * rb.SH_K1 + 5 * 0.25 * rb.SH_K2) + 32 * P.EPS)
    assert lit.shape == (8, 16, 3) and np.all(np.abs(lit - want_map) <= slack) and len(np.unique(lit.reshape(-1, 3), axis=0)) > 60
    baked = scenes.baked_world(world, {1: lit})
    camera = hm.PerspectiveCamera(screen_distance=1.0, aspect_ratio=48 / 36, transformation=hm.translation(hm.Vec(0.4, 0.0, 0.0)))
    W, H = 48, 36
    image = hm.HdrImage(W, H)
    tracer = GpuImageTracer(image, camera, samples_per_side=0)
    try:
        tracer.fire_all_rays(hm.FlatRenderer(baked))
    finally:
        tracer.close()
    flat, cam = flatten.flatten_world(baked), flatten.flatten_camera(camera)
    par = flatten.renderer_params(hm.FlatRenderer(baked), W, H, samples_per_side=0)
    want, _ = orc.render(flat, cam, par, sqr_mode=orc.SQR_MUL)
    got = np.asarray(image.array)
    assert got.tobytes() == np.ascontiguousarray(want, dtype=np.float64).tobytes()
    seen = 0
    for row in range(H):
        for col in range(W):
            hit = orc.world_intersect(flat, orc.tracer_fire_ray(cam, W, H, col, row))
            if hit is None or int(hit[9]) != 1:
                continue
            assert np.array_equal(got[row, col], lit[min(int(hit[8] * 8), 7), min(int(hit[7] * 16), 15)]), (row, col, hit)
            seen += 1
    assert seen > 40  # (a disc of about five pixels' radius)
