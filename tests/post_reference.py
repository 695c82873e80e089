"""A plain reference for the HdrImage post-processing kernels (csrc/pt_post.h), independent of the C oracle and of the device.

Not a test module and no fixtures: helpers for tests/test_postprocess.py (which pins them to the oracle and to the g10
goldens on the CPU) and tests/test_gpu_postprocess.py (which judges the kernels with them).  numpy, ``math.fsum`` and, where
installed, ``mpmath`` for the values fp64 cannot decide.

  pfm_payload        hdrimages.py:113-118   float32 payload, bottom row first
  luminosity         hdrimages.py:120-128   10^(mean(log10(delta + (max+min)/2))), the sum exact
  tonemap            hdrimages.py:130-146   x * scale, then x / (1 + x)
  ldr_bytes          hdrimages.py:160-166   int(255 * x**(1/gamma)), saturated to a byte
"""
import math

import numpy as np

try:
    import mpmath
except ImportError:  # the device tests then run on fsum and libm alone; only the mpmath cross-checks skip
    mpmath = None

U = 2.0 ** -53  # unit roundoff of fp64

# the kernels' constants (csrc/pt_post.h, ptrace.hip post_grid): the test sizes are chosen from these
POST_CHUNK = 8192            # pixels per block of pt_post_loglum_kernel
POST_THREADS = 256
POST_MAX_BLOCKS = 4096       # post_grid(): 4096 * 256 = 1 048 576 threads per grid-stride trip
GRID_THREADS = POST_MAX_BLOCKS * POST_THREADS


def pfm_payload(img, big_endian: bool) -> bytes:
    with np.errstate(over="ignore"):  # (a double beyond FLT_MAX + ulp/2 becomes inf: that is the expected payload)
        return np.asarray(img).astype(">f4" if big_endian else "<f4")[::-1].tobytes()


# ---- luminosity ---------------------------------------------------------------------------------------------------------
def luminosity_terms(img, delta: float = 1e-10) -> np.ndarray:
    """log10(delta + (max + min) / 2) per pixel, fp64.  Evaluated in extended precision where numpy has it (x86: 64-bit
    mantissa) and rounded once, so a term is within 1 ulp of the exact value (test_reference_terms_against_mpmath)."""
    a = np.asarray(img, dtype=np.float64).reshape(-1, 3)
    lum = delta + (a.max(axis=1) + a.min(axis=1)) / 2  # (these three operations are exact IEEE ones on the device too)
    with np.errstate(divide="ignore"):
        return np.log10(lum.astype(np.longdouble)).astype(np.float64)


def luminosity(img, delta: float = 1e-10) -> float:
    t = luminosity_terms(img, delta)
    return 10.0 ** (math.fsum(t) / t.size)


def sum_depth(npix: int) -> int:
    """The longest chain of additions a term goes through in pt_post_loglum_kernel + pt_post_sum_kernel."""
    nblocks = -(-npix // POST_CHUNK)
    per_thread = -(-min(npix, POST_CHUNK) // POST_THREADS)  # <= 32 terms in sequence
    return per_thread + 8 + -(-nblocks // POST_THREADS) + 8  # + block tree + partials in sequence + second tree


def luminosity_bound(terms: np.ndarray, depth: int, l_units: float, p_ulp: float) -> float:
    """Relative bound on |lum - luminosity()| for a sum of the terms whose additions nest `depth` deep and whose log10 is
    within `l_units` * U * |t| of the reference's terms; both sides end in libm's pow(10, .), within `p_ulp` ulp each.

      |S - S_ref| <= (depth + L) * U * T,  T = sum |t|       (first order; the reference's sum is exact: fsum)
      mean: that over n, plus the rounding of the division on either side, U * |mean| each
      result: relative ln(10) * (error of the mean), plus pow's own p_ulp ulp (1 ulp <= 2 U relative) on either side"""
    n = terms.size
    big_t = math.fsum(np.abs(terms))
    mean = abs(math.fsum(terms)) / n
    return math.log(10.0) * ((depth + l_units) * U * big_t / n + 2 * U * mean) + 2 * p_ulp * 2 * U


# ---- tone map -----------------------------------------------------------------------------------------------------------
def tonemap_f64(img, scale: float, clamp: bool) -> np.ndarray:
    """The kernel's value BEFORE it is rounded to the image's type: fp64(x) * scale, then x / (1 + x)."""
    x = np.asarray(img).astype(np.float64) * np.float64(scale)
    if clamp:
        with np.errstate(invalid="ignore"):  # (inf / inf: NaN, as on the device)
            x = x / (1 + x)
    return x


def tonemap(img, scale: float, clamp: bool, fmt=None) -> np.ndarray:
    """The written-back image in `fmt` (default: the type of `img`): for float32, float32(the fp64 result of float64(x))."""
    fmt = np.dtype(fmt if fmt is not None else np.asarray(img).dtype)
    with np.errstate(over="ignore"):
        return tonemap_f64(img, scale, clamp).astype(fmt)


# ---- LDR bytes ----------------------------------------------------------------------------------------------------------
def _saturate(v: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.where(v >= 255.0, 255.0, np.where(v > 0.0, np.floor(v), 0.0)).astype(np.uint8)  # NaN fails both: 0


def ldr_bytes(x, gamma: float, k_ulp: float):
    """-> (want, other, ambiguous): floor(255 * x**(1/gamma)) saturated to [0, 255] (NaN -> 0), the second byte that is
    accepted (== want wherever there is no doubt), and the mask of the values whose fp64 product lies within `k_ulp` ulp of
    an integer: there a pow that is `k_ulp - 1` ulp off may truncate to either side.  For those alone the exact product is
    taken from mpmath (50 digits): beyond `k_ulp` ulp from the integer it decides (other == want), otherwise -- or without
    mpmath -- the integer's two neighbours are both accepted.
    gamma 1.0: pow(x, 1.0) is x and the product one IEEE multiplication: nothing is ambiguous.
    x of 0, 1, inf and NaN are exact cases of pow, not roundings: never ambiguous."""
    x = np.asarray(x, dtype=np.float64)
    inv = 1.0 / gamma
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = 255 * (x if gamma == 1.0 else np.power(x, inv))
    want = _saturate(v)
    other = want.copy()
    ambiguous = np.zeros(x.shape, dtype=bool)
    if gamma == 1.0:
        return want, other, ambiguous
    with np.errstate(invalid="ignore"):
        m = np.rint(v)
        rounded = np.isfinite(v) & (x != 0.0) & (x != 1.0) & (v < 256.0)
        ambiguous = rounded & (np.abs(v - m) <= k_ulp * np.spacing(np.where(rounded, v, 1.0)))
    for idx in zip(*np.nonzero(ambiguous)):
        mi, tol = float(m[idx]), k_ulp * float(np.spacing(v[idx]))
        lo, hi = _saturate(np.array([mi - 1.0, mi]))
        other[idx] = lo if want[idx] == hi else hi  # (`want` stays the fp64 product's own verdict)
        if mpmath is not None:
            with mpmath.workprec(170):  # (50 digits)
                e = 255 * mpmath.power(mpmath.mpf(float(x[idx])), mpmath.mpf(inv))
                if abs(e - mi) > tol:
                    want[idx] = other[idx] = _saturate(np.array([float(mpmath.floor(e))]))[0]
    return want, other, ambiguous


def ldr_mismatches(got, want, other) -> np.ndarray:
    """Mask of the bytes that are neither of the accepted two."""
    got = np.asarray(got)
    return (got != want) & (got != other)


# ---- distance of a libm to the reference and to the exact value --------------------------------------------------------------
def distance(got, ref_ld):
    """max |got - ref| in ulp of the fp64 reference and in units of U * |ref|; `ref_ld` in extended precision (log10 or pow
    evaluated on np.longdouble: good to 2^-11 fp64 ulp on x86), so the figures are those against the exact value."""
    got, ref_ld = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref_ld, dtype=np.longdouble).reshape(-1)
    keep = ref_ld != 0
    assert np.all(got[~keep] == 0.0)
    err = np.abs(got[keep].astype(np.longdouble) - ref_ld[keep])
    ref = np.abs(ref_ld[keep])
    return float((err / np.spacing(ref.astype(np.float64))).max()), float((err / (ref * U)).max())


def exact_distance(fn_name: str, got, *args):
    """max over the sample of |got - exact| in ulp of the exact value and in units of U * |exact| (what the luminosity
    bound needs), the exact value from mpmath at 50 digits.  fn_name: 'log10' (one argument) or 'pow' (two)."""
    worst_ulp = worst_units = 0.0
    with mpmath.workprec(170):
        for i, g in enumerate(np.asarray(got, dtype=np.float64).reshape(-1)):
            a = [mpmath.mpf(float(np.asarray(arg).reshape(-1)[i])) for arg in args]
            e = mpmath.log10(a[0]) if fn_name == "log10" else mpmath.power(a[0], a[1])
            if e == 0:
                assert g == 0.0
                continue
            err = abs(mpmath.mpf(float(g)) - e)
            worst_ulp = max(worst_ulp, float(err / mpmath.mpf(float(np.spacing(abs(float(e)))))))
            worst_units = max(worst_units, float(err / (abs(e) * U)))
    return worst_ulp, worst_units
