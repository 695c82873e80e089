"""Adaptive queries on the device (include/ptrace_adaptive.h, libptrace_adaptive.so): sample counts against their numpy mirror,
offsets against ``np.cumsum``, and the ragged gather against the gather query of include/ptrace_gather.h -- for every record bit for
bit what ``DeviceScene.gather`` returns for that record with ``samples = K_i`` and its stream number, with no cap and no tolerance --
and, in one case, against the CPU oracle in its ``x * x`` mode (tests/gather_batches.py) with tests/test_gpu_gather.py's tolerance,
outlier definition and cap of one outlier record."""
import numpy as np
import pytest

from pytracer_amd import rays as rb

from . import gather_batches as G
from . import radiance_batches as R

pytestmark = pytest.mark.gpu

BG = G.BACKGROUND
MAX_OUTLIERS = 1  # tests/test_gpu_gather.py's
INF, NAN = float("inf"), float("nan")
CYCLE = (0, 1, 2, 63, 64, 65, 7, -3, 300, 17)  # records that straddle 64- and 256-sample boundaries, one longer than a workgroup


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


def _to_dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared records are read-only)


def _cycle(n=130, shift=0):
    return np.array([CYCLE[(i + shift) % len(CYCLE)] for i in range(n)], dtype=np.int32)


def _ragged(ds, r, counts, N, D, limit, capacity=None, depth=0, channels="all", active=None, seqs="own", init_state=G.S0, **kw):
    """the records of ``r`` with ``counts`` samples each (offsets from the mirror; ``capacity=None``: the total)"""
    counts = np.asarray(counts, dtype=np.int32)
    off = rb.sample_offsets_host(counts)
    seq = r["seq"] if isinstance(seqs, str) else seqs
    return ds.gather_ragged(rb.planar(r["point"], 3), rb.planar(r["normal"], 3), counts, off, int(off[-1]) if capacity is None else capacity,
                            init_state, seq, active, N, D, limit, BG, depth, channels, **kw)


def _equals_the_uniform_gather(ds, r, got, taken, seq, N, D, limit, label, depth=0):
    """For each distinct K > 0: the rows of ``got`` that took K samples are ``ds.gather`` of those rows with ``samples = K`` and their
    ``seq``, radiance and count bit for bit; rows with K = 0 are black with count 0."""
    taken = np.asarray(taken)
    assert np.array_equal(np.asarray(got.taken), taken), f"{label}: taken {np.asarray(got.taken)[:12].tolist()} is not the rule's {taken[:12].tolist()}"
    rad, cnt = np.asarray(got.radiance), np.asarray(got.n_rays)
    none = taken == 0
    assert not rad[none].any() and not np.signbit(rad[none]).any() and not cnt[none].any(), f"{label}: a record without samples is not black"
    for K in sorted(set(taken[taken > 0].tolist())):
        rows = np.flatnonzero(taken == K)
        want = ds.gather(rb.planar(r["point"][rows], 3), rb.planar(r["normal"][rows], 3), K, G.S0, np.asarray(seq)[rows], None, N, D, limit, BG, depth, "all")
        bad = ~G.same_bits(rad[rows], want.radiance)
        assert not bad.any(), f"{label}: K={K}: radiance differs from the uniform gather in {int(bad.sum())} of {rows.size} records (first: {int(rows[np.flatnonzero(bad)[0]])})"
        assert np.array_equal(cnt[rows], np.asarray(want.n_rays)), f"{label}: K={K}: counts differ"
        assert np.asarray(want.n_rays).min() >= K or depth > D


# ---- 1. counts against the mirror -------------------------------------------------------------------------------------------------------
def test_counts_equal_the_mirror_bit_for_bit(dev, scene_of):
    W, H = 48, 36
    m = W * H
    rng = np.random.default_rng(3)
    var = np.abs(rng.standard_normal(m)) * 10.0 ** rng.integers(-7, 1, m)
    col = np.abs(rng.standard_normal((m, 3))) * 10.0 ** rng.integers(-3, 1, (m, 1))
    shape = rng.integers(-1, 5, m).astype(np.int32)
    # the hostile values: integers and their neighbours (tolerance 0.5 on grey 2: want = v), zeros, negatives, NaN, infinities, dark pixels
    hostile = [7.0, np.nextafter(7.0, INF), np.nextafter(7.0, 0.0), 0.0, -0.0, -1e-300, -1.0, NAN, INF, -INF, 31.5, 32.0, 1e300, 5e-324, 0.5]
    for i, v in enumerate(hostile):
        var[100 + i], col[100 + i], shape[100 + i] = v, 2.0, 3
    col[200:210], var[200:210] = 0.0, np.linspace(0.0, 0.05, 10)      # below the floor
    col[210:214] = [[NAN, 1, 1], [INF, 1, 1], [-INF, 1, 1], [NAN, NAN, NAN]]
    shape[220:225], var[220:225] = -1, [1.0, NAN, INF, -1.0, 0.0]
    ds = scene_of("demo")
    for par in (dict(min_samples=2, max_samples=32, tolerance=0.5, luminance_floor=0.25, gain=1.0), dict(), dict(min_samples=0, max_samples=2 ** 20, tolerance=0.01),
                dict(min_samples=9, max_samples=9), dict(tolerance=INF), dict(gain=5e-324)):
        want = rb.sample_counts_host(var, col, shape, **par)
        host = ds.sample_counts(var, col, shape, **par)
        assert host.dtype == np.int32 and np.array_equal(host, want), (par, np.flatnonzero(host != want)[:8].tolist())
        on_dev = ds.sample_counts(_to_dev(var), _to_dev(rb.planar(col, 3)), _to_dev(shape), device=True, **par).numpy()
        assert np.array_equal(on_dev[:m], want), (par, np.flatnonzero(on_dev[:m] != want)[:8].tolist())
    first = rb.sample_counts_host(var, col, shape, min_samples=2, max_samples=32, tolerance=0.5, luminance_floor=0.25, gain=1.0)
    assert first[100:115].tolist() == [7, 8, 7, 2, 2, 32, 32, 32, 32, 32, 32, 32, 32, 2, 2] and not first[220:225].any() and len(set(first.tolist())) > 10
    wq = rb.WorldQueries(ds)
    frame = (np.zeros((m, 3)), np.zeros((m, 3)), shape.reshape(H, W))
    assert np.array_equal(wq.sample_counts(col.reshape(H, W, 3), frame, var.reshape(H, W)), rb.sample_counts_host(var, col, shape).reshape(H, W))


# ---- 2. offsets against np.cumsum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_offsets_equal_the_cumulative_sum(dev, scene_of, n):
    ds = scene_of("demo")
    rng = np.random.default_rng(n)
    counts = rng.integers(-5, 40, n).astype(np.int32)
    cases = [counts]
    if n == 65537:  # a total beyond 2^31 (and beyond 2^32), negatives in between
        big = rng.integers(-2 ** 31, 2 ** 20, n).astype(np.int64)
        big[big < 0] //= 2 ** 11  # (half of them negative, of every size)
        big[::3] = 2 ** 20
        cases.append(big.astype(np.int32))
    for c in cases:
        want = np.concatenate([[0], np.cumsum(np.maximum(c.astype(np.int64), 0))])
        assert np.array_equal(rb.sample_offsets_host(c), want)
        host = ds.sample_offsets(c)
        assert host.dtype == np.int64 and np.array_equal(host, want), np.flatnonzero(host != want)[:8].tolist()
        on_dev = ds.sample_offsets(_to_dev(c), device=True).numpy()
        assert np.array_equal(on_dev, want), np.flatnonzero(on_dev != want)[:8].tolist()
    if n == 65537:
        assert want[-1] > 2 ** 32 and (cases[1] < 0).sum() > 1000
    else:
        assert (counts < 0).any() or n == 1


# ---- 3. all counts equal to one value -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,D,limit", [("c2", 1, 3, 2), ("demo", 2, 2, 1)])
def test_equal_counts_are_the_uniform_gather(scene_of, orc, name, N, D, limit):
    ds, r = scene_of(name), G.records(orc, name)
    got = _ragged(ds, r, np.full(130, 5, np.int32), N, D, limit)
    want = ds.gather(rb.planar(r["point"], 3), rb.planar(r["normal"], 3), 5, G.S0, r["seq"], None, N, D, limit, BG, 0, "all")
    assert G.same_bits(got.radiance, want.radiance).all() and np.array_equal(got.n_rays, want.n_rays) and np.all(np.asarray(got.taken) == 5)
    assert got.buffer[: 32 * 130].tobytes() == want.buffer.tobytes() and len(np.unique(got.radiance, axis=0)) > 10 and got.n_rays.min() >= 5


# ---- 4. a ragged plane ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookup", ["search", "owner"])
@pytest.mark.parametrize("N,D,limit", [(1, 3, 2), (3, 2, 1)])
@pytest.mark.parametrize("name", ["c2", "pigments"])
def test_a_ragged_plane_equals_the_uniform_gather_per_count(scene_of, orc, monkeypatch, name, N, D, limit, lookup):
    monkeypatch.setenv("PTRACE_ADAPTIVE_LOOKUP", lookup)  # (both ways a sample finds its record; one of them is the default)
    ds, r = scene_of(name), G.records(orc, name)
    counts = _cycle()
    got = _ragged(ds, r, counts, N, D, limit)
    assert int(np.maximum(counts, 0).sum()) == 13 * 519 and (counts == 300).sum() == 13
    _equals_the_uniform_gather(ds, r, got, np.maximum(counts, 0), r["seq"], N, D, limit, f"{name} N={N}")
    assert len(np.unique(np.asarray(got.radiance)[counts > 0], axis=0)) > 10


# ---- 5. one case against the oracle ---------------------------------------------------------------------------------------------------------
def test_a_ragged_plane_equals_the_oracle(scene_of, orc):
    """Stream ``seq_i + k`` does not depend on K, so record i's expectation is the oracle's ordered mean over the first K_i of its 70
    samples.  The cap of ONE outlier record is a condition (the oracle against itself has none): tests/test_gpu_gather.py's."""
    name = "c2"
    K, N, D, limit = max(G.CASES)  # the largest K: (70, 1, 2, 0)
    assert K == 70
    want = G.expected(orc, name, K, N, D, limit)
    counts = np.array([(70, 1, 0, 33, 64, 65, 7, -2, 16, 69)[i % 10] for i in range(130)], dtype=np.int32)
    taken = np.maximum(counts, 0)
    radiance, count = np.zeros((130, 3)), np.zeros(130, np.uint64)
    for k in sorted(set(taken[taken > 0].tolist())):
        rows = np.flatnonzero(taken == k)
        radiance[rows] = G.ordered_mean(want["samples"][rows, :k])
        count[rows] = want["sample_counts"][rows, :k].sum(axis=1, dtype=np.uint64)
    full = taken == 70
    assert G.same_bits(radiance[full], want["radiance"][full]).all() and np.array_equal(count[full], want["count"][full])
    got = _ragged(scene_of(name), G.records(orc, name), counts, N, D, limit)
    bad, worst = G.outliers(got, {"radiance": radiance, "count": count})
    same = G.same_bits(got.radiance, radiance)
    print(f"ragged gather {name} K<=70 N={N} D={D} limit={limit}: outliers {int(bad.sum())}, worst relative error {worst:.3g}, bit-identical {same.mean():.1%}")
    assert np.array_equal(got.taken, taken)
    assert bad.sum() <= MAX_OUTLIERS, f"{int(bad.sum())} outliers (records {np.flatnonzero(bad)[:8].tolist()}), worst {worst:.3g}"


# ---- 6. seq = NULL ---------------------------------------------------------------------------------------------------------------------------
def test_without_stream_numbers_a_record_starts_at_its_offset(scene_of, orc):
    ds, r = scene_of("c2"), G.records(orc, "c2")
    counts = _cycle(shift=3)
    off = rb.sample_offsets_host(counts)
    implicit = _ragged(ds, r, counts, 1, 3, 2, seqs=None, init_seq=1000)
    explicit = _ragged(ds, r, counts, 1, 3, 2, seqs=(1000 + off[:-1]).astype(np.uint64))
    assert implicit.buffer.tobytes() == explicit.buffer.tobytes() and len(np.unique(implicit.radiance, axis=0)) > 10
    # it wraps: init_seq near 2^64
    wrapped = _ragged(ds, r, counts, 1, 3, 2, seqs=None, init_seq=2 ** 64 - 100)
    numbers = [(2 ** 64 - 100 + int(o)) % 2 ** 64 for o in off[:-1]]
    assert wrapped.buffer.tobytes() == _ragged(ds, r, counts, 1, 3, 2, seqs=numbers).buffer.tobytes()


# ---- 7. capacity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookup", ["search", "owner"])
def test_a_capacity_truncates_in_record_order(scene_of, orc, monkeypatch, lookup):
    monkeypatch.setenv("PTRACE_ADAPTIVE_LOOKUP", lookup)
    ds, r = scene_of("c2"), G.records(orc, "c2")
    counts = _cycle()
    off = rb.sample_offsets_host(counts)
    total = int(off[-1])
    whole = _ragged(ds, r, counts, 1, 3, 2)
    inside = int(off[28]) + 100   # record 28 has 300 samples: 100 of them
    boundary = int(off[44])       # records 0 .. 43 whole, nothing of record 44 (64 samples)
    assert counts[28] == 300 and counts[44] == 64
    for cap in (0, inside, boundary, total, total + 1000):
        taken = rb.samples_taken_host(counts, off, cap)
        got = _ragged(ds, r, counts, 1, 3, 2, capacity=cap)
        assert np.array_equal(got.taken, taken) and int(taken.sum()) == min(cap, total), cap
        front = taken == np.maximum(counts, 0)  # the records in front of the cut (and those that never had samples)
        assert G.same_bits(np.asarray(got.radiance)[front], np.asarray(whole.radiance)[front]).all(), cap
        assert np.array_equal(np.asarray(got.n_rays)[front], np.asarray(whole.n_rays)[front]), cap
        behind = (taken == 0) & (counts > 0)
        assert not np.asarray(got.radiance)[behind].any() and not np.asarray(got.n_rays)[behind].any(), cap
        _equals_the_uniform_gather(ds, r, got, taken, r["seq"], 1, 3, 2, f"capacity {cap}")
        if cap == inside:
            assert taken[28] == 100 and not taken[29:].any() and front[:28].all()
        if cap == boundary:
            assert not taken[44:].any() and front[:44].all()
        if cap == 0:
            assert not got.buffer.any()
        if cap >= total:
            assert got.buffer.tobytes() == whole.buffer.tobytes()


# ---- 8. launch shape and entry points -----------------------------------------------------------------------------------------------------
def test_the_launch_shape_and_the_entry_points_change_no_bit(dev, scene_of, orc, monkeypatch):
    from pytracer_amd import _lib
    from pytracer_amd.devmem import DeviceBuffer, Stream

    ds, r = scene_of("c2"), G.records(orc, "c2")
    n, N, D, limit = 130, 2, 2, 1
    counts = _cycle(shift=5)
    off = rb.sample_offsets_host(counts)
    total = int(off[-1])
    active = (np.arange(n, dtype=np.int32) % 6) - 1  # (-1: skipped)
    host = _ragged(ds, r, counts, N, D, limit, active=active)
    skipped = active < 0
    assert not np.asarray(host.radiance)[skipped].any() and not np.asarray(host.n_rays)[skipped].any() and not np.asarray(host.taken)[skipped].any()
    _equals_the_uniform_gather(ds, r, host, np.where(skipped, 0, np.maximum(counts, 0)), r["seq"], N, D, limit, "beside skipped records")
    # the two look-ups (one of them is the default) and a launch of one workgroup: the same bits; the owner plane is 4 bytes a sample
    for lookup, plane in (("search", 0), ("owner", (4 * total + 7) // 8 * 8)):
        monkeypatch.setenv("PTRACE_ADAPTIVE_LOOKUP", lookup)
        stacks = ds.adaptive_workspace_bytes(n, total, N, D) - total * 32 - plane
        assert stacks > 0 and stacks % (256 * 20 * 2 * 8) == 0, lookup
        assert _ragged(ds, r, counts, N, D, limit, active=active).buffer.tobytes() == host.buffer.tobytes(), lookup
        monkeypatch.setenv("PTRACE_ADAPTIVE_LANES", "300")  # (rounded down to 256: every wave walks its 64 samples 27 times over)
        assert ds.adaptive_workspace_bytes(n, total, N, D) == 256 * 20 * 2 * 8 + total * 32 + plane
        capped = _ragged(ds, r, counts, N, D, limit, active=active)
        monkeypatch.delenv("PTRACE_ADAPTIVE_LANES")
        assert capped.buffer.tobytes() == host.buffer.tobytes(), lookup
    monkeypatch.setenv("PTRACE_ADAPTIVE_LOOKUP", "table")
    with pytest.raises(_lib.PtraceError, match="PT_ERR_INVALID"):
        _ragged(ds, r, counts, N, D, limit)
    monkeypatch.delenv("PTRACE_ADAPTIVE_LOOKUP")
    # the device form, offsets from the device's own scan, a caller's stream, workspace and output -- twice into the same buffers
    st = Stream()
    try:
        pts, nrm = _to_dev(rb.planar(r["point"], 3)), _to_dev(rb.planar(r["normal"], 3))
        seq, act, cnt = _to_dev(r["seq"].view(np.int64)), _to_dev(active), _to_dev(counts)
        import torch

        torch.cuda.synchronize()
        ws = DeviceBuffer((ds.adaptive_workspace_bytes(n, total, N, D),), np.uint8)
        mine = DeviceBuffer((rb.adaptive_bytes(n, rb.ADAPTIVE_ALL),), np.uint8)
        for turn in range(2):
            offsets = ds.sample_offsets(cnt, device=True, stream=st)
            out = ds.gather_ragged(pts, nrm, cnt, offsets, total, G.S0, seq, act, N, D, limit, BG, 0, "all", device=True, stream=st, out=mine, workspace=ws)
            assert out is mine and mine.numpy().tobytes() == host.buffer.tobytes(), f"turn {turn}: the ragged gather in HBM differs from the one through host arrays"
        # channels = 0: the radiance alone, and not a byte behind it is touched
        filled = _to_dev(np.full(rb.adaptive_bytes(n, rb.ADAPTIVE_ALL), 0xAB, np.uint8))
        torch.cuda.synchronize()
        ds.gather_ragged(pts, nrm, cnt, offsets, total, G.S0, seq, act, N, D, limit, BG, 0, "none", device=True, stream=st, out=filled, workspace=ws)
        st.synchronize()
        back = filled.cpu().numpy()
        assert back[: 24 * n].tobytes() == host.buffer[: 24 * n].tobytes() and np.all(back[24 * n:] == 0xAB)
        bare = _ragged(ds, r, counts, N, D, limit, active=active, channels="none")
        assert bare.buffer.nbytes == 24 * n and bare.buffer.tobytes() == host.buffer[: 24 * n].tobytes()
        only_taken = _ragged(ds, r, counts, N, D, limit, active=active, channels="taken")
        assert only_taken.buffer.nbytes == 24 * n + 4 * n and np.array_equal(only_taken.taken, host.taken)
        # the query of WorldQueries: offsets and gather, the total read back
        res = rb.WorldQueries(ds).hemisphere_radiance_ragged(r["point"], counts, None, G.S0, r["seq"], N, D, limit, BG, normals=r["normal"], active=active)
        assert res.buffer.tobytes() == host.buffer.tobytes()
    finally:
        st.close()


# ---- 9. records of NaN and infinity ---------------------------------------------------------------------------------------------------------
def test_records_of_nan_and_infinity_return_what_the_gather_returns(scene_of, orc):
    """Every value in points and normals is legal (include/ptrace_gather.h): the walk ends by integer counters alone."""
    ds = scene_of("c2")
    base = G.records(orc, "c2")
    point, normal = np.array(base["point"][:40]), np.array(base["normal"][:40])
    values = (NAN, INF, -INF, 1e308, -1e308, 5e-324, 0.0, -0.0)
    for i, v in enumerate(values):
        point[i, i % 3] = v
        normal[8 + i, i % 3] = v
        point[16 + i], normal[16 + i] = v, v
    normal[24:28] = 0.0
    point[28:32] = [[NAN, INF, -INF]] * 4
    r = {"point": point, "normal": normal, "seq": base["seq"][:40]}
    counts = _cycle(40, shift=2)  # (record 16, all NaN, has 300 samples)
    for N, D, limit in ((1, 3, 2), (2, 2, 0)):
        got = _ragged(ds, r, counts, N, D, limit)
        _equals_the_uniform_gather(ds, r, got, np.maximum(counts, 0), r["seq"], N, D, limit, f"hostile records N={N}")
        # a sample whose ray is NaN hits nothing: the background, one ray per sample
        lost = np.flatnonzero((counts > 0) & np.isnan(point).all(axis=1))
        assert lost.size >= 1 and np.array_equal(np.asarray(got.n_rays)[lost], counts[lost].astype(np.uint64))
        assert np.allclose(np.asarray(got.radiance)[lost], BG, rtol=1e-12)
