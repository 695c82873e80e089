"""Probe planes, hostile index planes and hostile keep planes for the tests of the gradient accumulate query
(include/ptrace_gradient.h), on the frames of tests/moving_frames.py.  Nothing here needs a GPU, and nothing here is modified by a
test."""
import numpy as np

from pytracer_amd import _gradient_lib
from pytracer_amd import rays as rb

from . import moving_frames as M

NAN, INF = float("nan"), float("inf")
STRATA = (1, 2, 3, 4)
RADII = (0, 1, 2)

_planes = {}


def probe_planes(W, Hh, kind, how, seed, stratum, table="translation", phase=0, samples=3, init_seq=54):
    """The probes of the current frame of ``moving_frames.inputs(W, Hh, kind, how, seed)`` as the mirror gives them -> (index, point,
    normal, seq)."""
    _, args = M.inputs(W, Hh, kind, how, seed)
    return rb.gradient_probes_host(args[2], args[3], args[4], *M.table(table), W, Hh, stratum=stratum, phase=phase, samples=samples,
                                   init_seq=init_seq)


def hostile_index(W, Hh, stratum, seed, index=None):
    """-> probe_index int32[ns]: the indices ``index`` (default: a pixel of every stratum, drawn at random) with -1, -2^31, m and
    2^31 - 1 laid over about a quarter of them, and a few indices that point into another stratum."""
    m, ns = W * Hh, _gradient_lib.strata(W, Hh, stratum)
    rng = np.random.default_rng(seed)
    out = rng.integers(0, max(m, 1), ns).astype(np.int32) if index is None else np.array(index, dtype=np.int32)
    pick = lambda share: np.flatnonzero(rng.uniform(0, 1, ns) < share)  # noqa: E731
    for rows, value in ((pick(0.08), -1), (pick(0.05), -2 ** 31), (pick(0.06), m), (pick(0.05), 2 ** 31 - 1), (pick(0.03), m + 1)):
        out[rows] = value
    far = pick(0.1)
    out[far] = rng.integers(0, max(m, 1), far.size)
    return out


def probe_old(colour, index, seed, share=0.5):
    """-> probe_old [ns, 3]: for about ``share`` of the probes the bits of ``colour`` at the probe's pixel (nothing changed there),
    for the others another colour; a NaN, an infinity and a negative colour among them."""
    col = np.asarray(colour, dtype=np.float64).reshape(-1, 3)
    index = np.asarray(index).astype(np.int64)
    rng = np.random.default_rng(seed)
    ns, m = index.shape[0], col.shape[0]
    old = rng.uniform(0.0, 2.0, (ns, 3))
    ok = (index >= 0) & (index < m)
    same = ok & (rng.uniform(0, 1, ns) < share)
    old[same] = col[index[same]]
    pick = lambda p: np.flatnonzero(rng.uniform(0, 1, ns) < p)  # noqa: E731
    old[pick(0.03), 0], old[pick(0.03), 1], old[pick(0.03)] = NAN, INF, -1.5
    return old


def hostile_keep(W, Hh, seed):
    """-> keep [Hh, W]: values in [0, 1] with 0, 1, NaN, +-inf, -0.5, 1.5 and -0.0 among them."""
    rng = np.random.default_rng(seed)
    m = W * Hh
    keep = rng.uniform(0.0, 1.0, m)
    pick = lambda share: np.flatnonzero(rng.uniform(0, 1, m) < share)  # noqa: E731
    for rows, value in ((pick(0.1), 0.0), (pick(0.15), 1.0), (pick(0.04), NAN), (pick(0.03), INF), (pick(0.03), -INF), (pick(0.04), -0.5),
                        (pick(0.04), 1.5), (pick(0.02), -0.0)):
        keep[rows] = value
    return keep.reshape(Hh, W)


def scalar_probe(phase, j, W, Hh, s):
    """The hash of the header restated in Python integers -> (x, y) of stratum ``j``'s probe."""
    mask = 2 ** 64 - 1
    gw = (W + s - 1) // s
    sy, sx = divmod(j, gw)
    sw, sh = min(s, W - sx * s), min(s, Hh - sy * s)
    x = (phase * 0x9E3779B97F4A7C15 + j * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & mask
    for _ in range(2):
        x ^= x >> 32
        x = (x * 0xD6E8FEB86659FD93) & mask
    x ^= x >> 32
    return sx * s + (x & 0xffff) % sw, sy * s + ((x >> 16) & 0xffff) % sh
