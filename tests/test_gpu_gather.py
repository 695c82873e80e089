"""Gather queries on the device (include/ptrace_gather.h, libptrace_gather.so): the mean radiance over the hemisphere of batches of
surface points, against the CPU oracle in its ``x * x`` mode (tests/gather_batches.py), against the library's own scatter and
radiance queries summed on the host, and against itself across batch sizes, launch shapes, channels and entry points.

Expected agreement.  Against the oracle a diffuse bounce holds ocml's sin / cos against glibc's: radiance to ``TOL = 1e-5`` relative
per channel, and a record beyond it, or not finite, or with another count (a last-ulp difference may flip a silhouette, checker or
roulette decision behind a bounce), is an outlier, of which a case may hold ONE -- tests/test_gpu_radiance.py's cap and tolerance.
Device against device -- the scatter query followed by the radiance query, summed on the host in sample order; other batch sizes
and launch shapes; the two entry points -- bit for bit, no cap and no tolerance: the order of the sum is part of the interface
(tests/test_gather_host.py shows that the expected values tell the orders apart)."""
import numpy as np
import pytest

from pytracer_amd import abi, rays as rb

from . import gather_batches as G
from . import radiance_batches as R

pytestmark = pytest.mark.gpu

BG = G.BACKGROUND
MAX_OUTLIERS = 1
MASK = 2 ** 64 - 1


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


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _gather(ds, r, K, N, D, limit, depth=0, channels="all", rows=slice(None), active=None, seqs="own", init_state=G.S0, **kw):
    """the records ``rows`` of ``r`` (``point``, ``normal``, ``seq``), every record with its own stream number"""
    seq = r["seq"][rows] if isinstance(seqs, str) else seqs
    return ds.gather(rb.planar(r["point"][rows], 3), rb.planar(r["normal"][rows], 3), K, init_state, seq, active, N, D, limit, BG, depth,
                     channels, **kw)


def _same(got, want_radiance, want_count, label, rows=slice(None)):
    """radiance and count of the records ``rows`` of ``got`` bit for bit"""
    rad, cnt = np.asarray(got.radiance)[rows], np.asarray(got.n_rays)[rows]
    bad = ~G.same_bits(rad, want_radiance)
    assert not bad.any(), f"{label}: radiance differs in {int(bad.sum())} of {rad.shape[0]} records (first: {int(np.flatnonzero(bad)[0])})"
    assert _bits(cnt, np.asarray(want_count, dtype=np.uint64)), f"{label}: counts differ in {int((cnt != want_count).sum())} records"


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,D,limit", G.CASES)
@pytest.mark.parametrize("name", G.WORLDS)
def test_gather_equals_the_oracle(scene_of, orc, name, K, N, D, limit):
    r = G.records(orc, name)
    want = G.expected(orc, name, K, N, D, limit)
    got = _gather(scene_of(name), r, K, N, D, limit)
    assert got.n == 130 and want["count"].min() >= K
    bad, worst = G.outliers(got, want)
    same = G.same_bits(got.radiance, want["radiance"])
    print(f"gather {name} K={K} N={N} D={D} limit={limit}: {got.n} records, {int(want['count'].sum())} traced, outliers {int(bad.sum())}, "
          f"worst relative error {worst:.3g}, bit-identical {same.mean():.1%}")
    assert bad.sum() <= MAX_OUTLIERS, f"{name} K={K} N={N} D={D} limit={limit}: {int(bad.sum())} outliers (records {np.flatnonzero(bad)[:8].tolist()}), worst {worst:.3g}"


def test_mirrors_at_70_samples_equal_the_oracles_ordered_sum_bit_for_bit(scene_of, orc):
    """No libm call decides anything behind the hemisphere's ray in the world of mirrors: whatever differs from the oracle differs
    by that ray's sin / cos, which one record at most may show as another path.  With tests/test_gather_host.py's assertion (the
    reverse order changes the bits of most records) this pins the order of the sum."""
    K, N, D, limit = G.CASES[3]
    want = G.expected(orc, "mirrors", K, N, D, limit)
    got = _gather(scene_of("mirrors"), G.records(orc, "mirrors"), K, N, D, limit)
    same = G.same_bits(got.radiance, want["radiance"]) & (np.asarray(got.n_rays) == want["count"])
    reverse = G.same_bits(got.radiance, G.ordered_mean(want["samples"], reverse=True))
    print(f"gather mirrors K={K}: {int((~same).sum())} of {got.n} records differ from the oracle's ordered sum; {int(reverse.sum())} equal the reverse sum")
    assert (~same).sum() <= 1, np.flatnonzero(~same)[:8].tolist()
    assert reverse.mean() < 0.5


# ---- 2. bit for bit against the library itself: scatter, then path_radiance, summed on the host in k order --------------------------
_diffuse = {}


def _diffuse_records(orc, ds, name, limit_n=130) -> dict:
    """The world's hit records that lie on shapes with a DiffuseBRDF whose pigment is not black there (the scatter query goes on:
    status 1) -> {"point", "normal", "shape", "uv", "in_dir", "seq"}"""
    if name not in _diffuse:
        b = R.records(orc, name)
        rec, flat = b["rec"], R.world(name)[0]
        shape = np.asarray(rec.shape_index)
        rows = np.flatnonzero((shape >= 0) & (np.asarray(flat.brdf_kind)[np.maximum(shape, 0)] == abi.BRDF_DIFFUSE))
        probe = ds.scatter(shape[rows], rec.point[rows], rec.normal[rows], rec.uv[rows], b["rays"][rows, 3:6], rb.pcg_streams(1, np.arange(rows.size)),
                           False, "none")
        rows = rows[np.asarray(probe.status) == 1]
        assert rows.size >= limit_n, (name, rows.size)
        rows = rows[np.linspace(0, rows.size - 1, limit_n).astype(np.int64)]
        _diffuse[name] = {"point": np.array(rec.point[rows]), "normal": np.array(rec.normal[rows]), "shape": np.array(shape[rows], dtype=np.int32),
                          "uv": np.array(rec.uv[rows]), "in_dir": np.array(b["rays"][rows, 3:6]),
                          "seq": (G.SEQ0 + G.STRIDE * np.arange(rows.size)).astype(np.uint64)}
    return _diffuse[name]


def _route(ds, r, K, N, D, limit, depth=0, rows=slice(None), seqs=None, init_state=G.S0):
    """What a caller does today: per sample ``scatter`` (no roulette) with the generator ``pcg_streams(init_state, seq_i + k)``, then
    ``radiance`` of those rays with the generators behind their two draws, then the sum in k order on the host
    -> (radiance [n, 3], count uint64 [n])"""
    seq = [int(x) for x in (r["seq"][rows] if seqs is None else seqs)]
    m = len(seq)
    rep = lambda a: np.repeat(a[rows], K, axis=0)  # noqa: E731  (record-major: sample j = i K + k)
    pcg = rb.pcg_streams(init_state, [(s + k) & MASK for s in seq for k in range(K)])
    sc = ds.scatter(rep(r["shape"]), rep(r["point"]), rep(r["normal"]), rep(r["uv"]), rep(r["in_dir"]), pcg, False, "none")
    assert np.all(sc.status == 1) and np.all(sc.rays[6] == 1.0e-3) and np.all(sc.rays[7] == np.inf)
    rad = ds.radiance(np.ascontiguousarray(sc.rays), np.ascontiguousarray(sc.pcg), N, D, limit, BG, depth, "count")
    with np.errstate(over="ignore"):
        count = np.asarray(rad.n_rays).reshape(m, K).sum(axis=1, dtype=np.uint64)
    return G.ordered_mean(np.asarray(rad.radiance).reshape(m, K, 3)), count


@pytest.mark.parametrize("K,N,D,limit,depth", [(1, 1, 3, 2, 0), (3, 2, 3, 1, 1), (64, 2, 2, 1, 0), (70, 1, 3, 0, 0)])
@pytest.mark.parametrize("name", ["c2", "demo"])
def test_gather_equals_scatter_then_path_radiance_bit_for_bit(scene_of, orc, name, K, N, D, limit, depth):
    ds = scene_of(name)
    r = _diffuse_records(orc, ds, name)
    want, count = _route(ds, r, K, N, D, limit, depth)
    got = _gather(ds, r, K, N, D, limit, depth)
    assert got.n == 130 and len(np.unique(want, axis=0)) > 2 and count.max() > K
    _same(got, want, count, f"{name} K={K} N={N} D={D} limit={limit} depth={depth}")


# ---- 3. batch sizes and launch shapes --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2_many(orc):
    """257 hit records of c2 (primary hits and bounces), every record with a stream number of its own"""
    rec = R.records(orc, "c2")["rec"]
    hit = np.flatnonzero(np.asarray(rec.hit))
    rows = hit[np.linspace(0, hit.size - 1, 257).astype(np.int64)]
    return {"point": np.array(rec.point[rows]), "normal": np.array(rec.normal[rows]), "seq": (G.SEQ0 + G.STRIDE * np.arange(257)).astype(np.uint64)}


@pytest.fixture(scope="module")
def c2_full(scene_of, c2_many):
    return _gather(scene_of("c2"), c2_many, 3, 2, 2, 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_around_the_wave_and_the_block(scene_of, c2_many, c2_full, n):
    start = (257 - n) // 2
    k = slice(start, start + n)
    got = _gather(scene_of("c2"), c2_many, 3, 2, 2, 1, rows=k)
    assert got.nbytes == 32 * n == got.buffer.nbytes and len(np.unique(c2_full.radiance, axis=0)) > 20
    _same(got, c2_full.radiance[k], c2_full.n_rays[k], f"n={n}")


def test_a_record_that_spans_four_waves(scene_of, c2_many, monkeypatch):
    """n = 5 at K = 200: 1000 samples, record i on lanes 200 i .. 200 i + 199 -- across four waves, and across the workgroups'
    boundaries.  Each record alone (another launch shape: its samples start at lane 0) and the launch capped at one workgroup give
    the same bits."""
    ds = scene_of("c2")
    rows = slice(100, 105)
    full = _gather(ds, c2_many, 200, 1, 3, 2, rows=rows)
    assert full.n == 5 and full.n_rays.min() >= 200 and len(np.unique(full.radiance, axis=0)) > 1
    for i in range(5):
        one = _gather(ds, c2_many, 200, 1, 3, 2, rows=slice(100 + i, 101 + i))
        _same(one, full.radiance[i: i + 1], full.n_rays[i: i + 1], f"record {i} alone")
    monkeypatch.setenv("PTRACE_GATHER_LANES", "256")
    capped = _gather(ds, c2_many, 200, 1, 3, 2, rows=rows)
    assert capped.buffer.tobytes() == full.buffer.tobytes()


def test_a_batch_larger_than_the_resident_lanes(scene_of, c2_many, monkeypatch):
    """PTRACE_GATHER_LANES caps the lanes of a launch (include/ptrace_gather.h): at 256 every wave of the one workgroup walks four
    sets of 64 samples one after the other (the last one partly idle), on one workgroup's worth of node stacks.  n K = 1000."""
    ds = scene_of("c2")
    rows = slice(0, 125)
    full = _gather(ds, c2_many, 8, 2, 2, 1, rows=rows)
    planes = 1000 * 4 * 8
    assert ds.gather_workspace_bytes(125, 8, 2, 2) == 1024 * 20 * 2 * 8 + planes
    monkeypatch.setenv("PTRACE_GATHER_LANES", "300")  # (rounded down to 256)
    assert ds.gather_workspace_bytes(125, 8, 2, 2) == 256 * 20 * 2 * 8 + planes and ds.gather_workspace_bytes(125, 8, 1, 3) == 256 * 6 * 3 * 8 + planes
    got = _gather(ds, c2_many, 8, 2, 2, 1, rows=rows)
    monkeypatch.delenv("PTRACE_GATHER_LANES")
    assert got.buffer.tobytes() == full.buffer.tobytes() and len(np.unique(full.radiance, axis=0)) > 20


# ---- 4. active, streams, depths, channels ----------------------------------------------------------------------------------------
def test_skipped_records_are_black_and_leave_their_neighbours_alone(scene_of, orc, c2_many, c2_full):
    ds = scene_of("c2")
    active = np.arange(257, dtype=np.int32) % 7 - 2  # (-2, -1: skipped; 0 .. 4: active -- a shape_index plane looks like this)
    got = _gather(ds, c2_many, 3, 2, 2, 1, active=active)
    off, on = active < 0, active >= 0
    assert off.sum() > 70 and not got.radiance[off].any() and not np.signbit(got.radiance[off]).any() and not got.n_rays[off].any()
    _same(got, c2_full.radiance[on], c2_full.n_rays[on], "active records beside skipped ones", rows=on)
    none = _gather(ds, c2_many, 3, 2, 2, 1, active=np.full(257, -1, np.int32))
    assert not none.buffer.any()
    # a RayHits goes in as it is: its shape_index is the `active` plane
    rec = R.records(orc, "c2")["rec"]
    wq = rb.WorldQueries(ds)
    res = wq.hemisphere_radiance(rec, 2, G.S0, num_of_rays=1, max_depth=2, russian_roulette_limit=1, background=BG)
    miss = ~np.asarray(rec.hit)
    assert res.radiance.shape == (rec.n, 3) and not res.radiance[miss].any() and not res.n_rays[miss].any() and np.all(res.n_rays[~miss] >= 2)
    plain = wq.hemisphere_radiance(np.asarray(rec.point), 2, G.S0, normals=np.asarray(rec.normal), active=np.asarray(rec.shape_index),
                                   num_of_rays=1, max_depth=2, russian_roulette_limit=1, background=BG)
    assert plain.buffer.tobytes() == res.buffer.tobytes()


def test_stream_numbers(scene_of, orc):
    """``seqs=None`` is ``init_seq + i K``; stream numbers near 2^64 wrap as ``pcg_streams`` wraps them."""
    ds = scene_of("c2")
    r = _diffuse_records(orc, ds, "c2")
    K = 5
    implicit = _gather(ds, r, K, 1, 3, 2, seqs=None, init_seq=1000)
    explicit = _gather(ds, r, K, 1, 3, 2, seqs=(1000 + K * np.arange(130)).astype(np.uint64))
    assert implicit.buffer.tobytes() == explicit.buffer.tobytes() and len(np.unique(implicit.radiance, axis=0)) > 10
    # the last streams of the 64-bit range and the first: record i's samples are seq_i, seq_i + 1, ... modulo 2^64
    rows = slice(0, 8)
    seqs = [2 ** 64 - 3, 2 ** 64 - 1, 2 ** 64 - K, 2 ** 64 - 2, 0, 2 ** 63 - 2, 2 ** 64 + 7, -1]
    want, count = _route(ds, r, K, 1, 3, 2, rows=rows, seqs=seqs, init_state=2 ** 64 - 1)
    got = _gather(ds, r, K, 1, 3, 2, rows=rows, seqs=seqs, init_state=2 ** 64 - 1)
    _same(got, want, count, "streams around 2^64")
    # implicit numbering wraps too: init_seq = 2^64 - 7 with K = 5 gives record 0 streams -7 .. -3, record 1 streams -2 .. 2
    wrapped = _gather(ds, r, K, 1, 3, 2, rows=slice(0, 2), seqs=None, init_seq=2 ** 64 - 7)
    want, count = _route(ds, r, K, 1, 3, 2, rows=slice(0, 2), seqs=[2 ** 64 - 7, 2 ** 64 - 2])
    _same(wrapped, want, count, "implicit streams across 2^64")


@pytest.mark.parametrize("name", ["demo", "mirrors"])
def test_depths_at_and_beyond_max_depth(scene_of, orc, name):
    """``depth0 > max_depth``: black and 0 for every record.  ``depth0 = max_depth``: one query per sample; a hit with ``lum > 0``
    scatters children that are black without a query -- as the oracle has it."""
    K, N, D, limit = 3, 2, 2, 1
    ds, r = scene_of(name), G.records(orc, name)
    deep = _gather(ds, r, K, N, D, limit, depth=D + 1)
    assert not deep.buffer.any()
    want = G.expected(orc, name, K, N, D, limit, depth0=D)
    got = _gather(ds, r, K, N, D, limit, depth=D)
    assert np.all(want["count"] == K) and _bits(got.n_rays, want["count"]) and len(np.unique(want["radiance"], axis=0)) > 2
    bad, worst = G.outliers(got, want)
    assert bad.sum() <= MAX_OUTLIERS, (name, int(bad.sum()), worst)


def test_the_radiance_is_the_same_without_the_count_channel(scene_of, orc):
    from pytracer_amd import _gather_lib

    L = _gather_lib.lib()
    ds, r = scene_of("pigments"), G.records(orc, "pigments")
    full = _gather(ds, r, 3, 2, 2, 1)
    bare = _gather(ds, r, 3, 2, 2, 1, channels="none")
    assert bare.buffer.nbytes == L.pt_rays_gather_bytes(130, 0) == 24 * 130 and full.buffer.nbytes == L.pt_rays_gather_bytes(130, 1) == 32 * 130
    assert bare.buffer.tobytes() == full.buffer[: 24 * 130].tobytes() and not bare.has("count")
    assert L.pt_rays_gather_plane_offset(130, 0, rb.GATHER_COUNT, 0) < 0 and L.pt_rays_gather_plane_offset(130, 1, rb.GATHER_COUNT, 0) == 24 * 130
    assert _bits(full.buffer[24 * 130:].view(np.uint64), full.n_rays) and full.n_rays.min() >= 3


# ---- 5. the query that stays in HBM ----------------------------------------------------------------------------------------------
def test_a_gather_that_stays_in_hbm(dev, orc, c2_many):
    """``gather(device=True)`` on device tensors with a caller-owned workspace, output buffer and stream, twice into the same buffers:
    byte for byte the host route.  An undersized workspace or output: PT_ERR_SIZE before anything runs."""
    import torch

    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    K, N, D, limit = 6, 2, 2, 1
    n = 257
    active = (np.arange(n, dtype=np.int32) % 5) - 1
    ds = dev.DeviceScene(R.world("c2")[0])
    st = Stream()
    try:
        host = _gather(ds, c2_many, K, N, D, limit, active=active)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        pts, nrm = to_dev(rb.planar(c2_many["point"], 3)), to_dev(rb.planar(c2_many["normal"], 3))
        seq, act = to_dev(c2_many["seq"].view(np.int64)), to_dev(active)
        torch.cuda.synchronize()
        need = ds.gather_workspace_bytes(n, K, N, D)
        assert need > n * K * 32 and (need - n * K * 32) % (256 * 20 * 2 * 8) == 0
        ws = DeviceBuffer((need,), np.uint8)
        mine = DeviceBuffer((rb.gather_bytes(n, rb.GATHER_ALL),), np.uint8)
        for turn in range(2):
            out = ds.gather(pts, nrm, K, G.S0, seq, act, N, D, limit, BG, 0, "all", device=True, stream=st, out=mine, workspace=ws)
            assert out is mine
            assert mine.numpy().tobytes() == host.buffer.tobytes(), f"turn {turn}: the gather in HBM differs from the gather through host arrays"
        # raw addresses, no optional planes, the radiance alone, the library's own workspace
        some = ds.gather(pts.data_ptr(), nrm.data_ptr(), K, G.S0, None, None, N, D, limit, BG, 0, "none", init_seq=77, device=True, stream=st, n=n)
        want = ds.gather(rb.planar(c2_many["point"], 3), rb.planar(c2_many["normal"], 3), K, G.S0, None, None, N, D, limit, BG, 0, "none", init_seq=77)
        assert some.numpy()[: want.nbytes].tobytes() == want.buffer.tobytes()
        for kw in (dict(workspace=DeviceBuffer((need - 8,), np.uint8), out=mine), dict(workspace=DeviceBuffer((n * K * 32 - 8,), np.uint8), out=mine),
                   dict(workspace=ws, out=DeviceBuffer((mine.nbytes - 8,), np.uint8))):
            with pytest.raises(_lib.PtraceError, match="PT_ERR_SIZE"):
                ds.gather(pts, nrm, K, G.S0, seq, act, N, D, limit, BG, device=True, stream=st, **kw)
        with pytest.raises(ValueError, match="n="):
            ds.gather(pts.data_ptr(), nrm, K, device=True)
        with pytest.raises(ValueError, match="device=True"):
            ds.gather(rb.planar(c2_many["point"], 3), rb.planar(c2_many["normal"], 3), K, stream=st)
    finally:
        st.close()
        ds.close()


# ---- 6. records nobody vouches for -----------------------------------------------------------------------------------------------
def _unvouched(r):
    """Every fourth record replaced, in turn, by a NaN point, an infinite point, a zero normal, a NaN normal, a point of huge
    coordinates, an infinite normal and a huge normal -> (point, normal, rows, {kind: rows}); every value is legal input."""
    point, normal = np.array(r["point"]), np.array(r["normal"])
    rows = np.arange(1, point.shape[0], 4)
    kinds = {k: rows[i::7] for i, k in enumerate(("nan_point", "inf_point", "zero_normal", "nan_normal", "huge_point", "inf_normal", "huge_normal"))}
    point[kinds["nan_point"]] = np.nan
    point[kinds["inf_point"], 1] = -np.inf
    normal[kinds["zero_normal"]] = 0.0
    normal[kinds["nan_normal"], 2] = np.nan
    point[kinds["huge_point"]] = [1.0e300, -1.0e305, 1.7e308]
    normal[kinds["inf_normal"], 0] = np.inf
    normal[kinds["huge_normal"]] *= 1.0e200
    return point, normal, rows, kinds


@pytest.mark.parametrize("name,K,N,D,limit", [("c2", 5, 2, 2, 1), ("pigments", 3, 3, 2, 0), ("mirrors", 70, 1, 3, 1)])
def test_records_nobody_vouches_for(scene_of, orc, name, K, N, D, limit):
    ds, r = scene_of(name), G.records(orc, name)
    clean = _gather(ds, r, K, N, D, limit)
    point, normal, rows, kinds = _unvouched(r)
    got = _gather(ds, {"point": point, "normal": normal, "seq": r["seq"]}, K, N, D, limit)  # (the call returns: the walk ends by its counters)
    others = np.setdiff1d(np.arange(130), rows)
    assert rows.size >= 30 and all(k.size >= 4 for k in kinds.values())
    assert _bits(got.radiance[others], clean.radiance[others]) and _bits(got.n_rays[others], clean.n_rays[others])
    assert np.all(got.n_rays >= K) and np.all(got.n_rays <= K * sum(N ** d for d in range(D + 1)))
    # a sample whose ray is NaN hits nothing and returns the background: K queries, and the ordered mean of K backgrounds
    bg_mean = G.ordered_mean(np.tile(np.array(BG), (1, K, 1)))[0]
    for kind in ("nan_point", "nan_normal"):
        k = kinds[kind]
        assert np.all(got.n_rays[k] == K) and np.all(got.radiance[k] == bg_mean), kind
    assert len(np.unique(clean.radiance[others], axis=0)) > 5


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(scene_of, c2_many):
    from pytracer_amd import _lib

    ds = scene_of("c2")
    rows = slice(0, 65)
    for kw, code, word in ((dict(K=0), "PT_ERR_INVALID", "samples"), (dict(N=0), "PT_ERR_INVALID", "num_of_rays"),
                           (dict(D=65), "PT_ERR_UNSUPPORTED", "64 levels"), (dict(D=70, depth=5), "PT_ERR_UNSUPPORTED", "64 levels"),
                           (dict(depth=-1), "PT_ERR_INVALID", "depth"), (dict(D=-1), "PT_ERR_INVALID", "max_depth"),
                           (dict(K=2 ** 31 - 1), "PT_ERR_INVALID", "2\\^31 - 1")):
        args = dict(K=3, N=2, D=2, limit=1, depth=0)
        args.update(kw)
        with pytest.raises(_lib.PtraceError, match=f"{code}.*{word}"):
            _gather(ds, c2_many, args["K"], args["N"], args["D"], args["limit"], args["depth"], rows=rows)
    assert _gather(ds, c2_many, 2, 1, 64, 60, rows=rows).n == 65 and _gather(ds, c2_many, 2, 1, 70, 3, depth=6, rows=rows).n == 65  # 64 levels
    with pytest.raises(ValueError, match="channel"):
        _gather(ds, c2_many, 3, 2, 2, 1, channels=2, rows=rows)
    with pytest.raises(ValueError, match="seqs"):
        _gather(ds, c2_many, 3, 2, 2, 1, seqs=[1, 2, 3], rows=rows)
    with pytest.raises(ValueError, match="active"):
        _gather(ds, c2_many, 3, 2, 2, 1, active=np.zeros(3, np.int32), rows=rows)
    with pytest.raises(ValueError, match="planar"):
        ds.gather(c2_many["point"], c2_many["normal"], 3)
    empty = ds.gather(np.zeros((3, 0)), np.zeros((3, 0)), 3)
    assert empty.n == 0 and empty.buffer.nbytes == 0
