/* Check by enumeration for csrc/pt_query.h: PT_SPHERE_ROOTS_IN with INSIDE.
 *
 * shapes.py:103-121 tries t1 = (-b - sqrt(delta)) / (2a) first and t2 = (-b + sqrt(delta)) / (2a) only when t1 is outside
 * (tmin, tmax).  For a sphere whose hoisted c = |o'|^2 - 1 is <= -0.5 (the common origin of the primary rays lies well inside
 * it) the kernels leave the first quotient out: it can never exceed tmin >= 0 (the argument is in pt_query.h).  This program
 * restates both forms and compares verdict and accepted t, bit for bit, over 1e8 inputs:
 *   - geometric ones: o' inside the ball |o'|^2 <= 0.5, d' = d * s with every component of d at or between the ends of
 *     wave_guard's range [1e-100, 1e100] and scales that take aa and bb through the whole exponent range;
 *   - c within a few ulp of -0.5 on either side (the guard itself decides which form runs, as in the kernels);
 *   - d' so small that bb*bb and aa are subnormal or zero (delta near 0), and so large that they overflow;
 *   - raw (bb, aa, cc) triples the geometry cannot produce: every exponent, infinities and NaNs, and |bb| = sd exactly
 *     (4 aa |cc| far below one ulp of bb*bb).
 * Build with -ffp-contract=off.  tests/test_sphere_inside_roots.py builds and runs it (a few seconds). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

typedef struct {
  int ok;
  double t;
} Verdict;

/* PT_SPHERE_ROOTS_IN, given bb: `inside` leaves the first quotient out */
static Verdict roots(double bb, double aa, double cc, double tmin, double tmax, int inside) {
  Verdict v = {0, 0.0};
  const double delta = bb * bb - 4.0 * aa * cc;
  if (delta > 0.0) {
    const double sd = sqrt(delta);
    const double den = 2.0 * aa;
    double t = 0.0;
    int ok = 0;
    if (!inside) {
      t = (-bb - sd) / den;
      ok = (t > tmin) && (t < tmax);
    }
    if (!ok) {
      t = (-bb + sd) / den;
      ok = (t > tmin) && (t < tmax);
    }
    v.ok = ok;
    v.t = ok ? t : 0.0;
  }
  return v;
}

static int origin_inside(double c) { return c <= -0.5; } /* pt_origin_inside */

static uint64_t next(uint64_t *s) { /* splitmix64 */
  uint64_t z = (*s += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static double unit(uint64_t *s) { return (double)(next(s) >> 11) * 0x1p-53; }
static double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}
static uint64_t to_bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}
/* random sign and mantissa, the exponent FIELD uniform in [elo, ehi] (0: subnormal or zero, 2047: infinity or NaN) */
static double any_double(uint64_t *s, int elo, int ehi) {
  const uint64_t r = next(s);
  const uint64_t e = (uint64_t)elo + next(s) % (uint64_t)(ehi - elo + 1);
  uint64_t m = r & 0xFFFFFFFFFFFFFULL;
  if ((r >> 60) == 0) m = 0; /* powers of two, true zeros and infinities now and then */
  return from_bits((r & 0x8000000000000000ULL) | (e << 52) | m);
}
static double guard_clamped(double d) { /* wave_guard: 1e-100 <= |d.c| <= 1e100; the ends themselves often */
  const double a = fabs(d);
  return copysign(a < 1e-100 ? 1e-100 : (a > 1e100 ? 1e100 : a), d);
}

int main(void) {
  const long long N = 100000000LL;
  long long bad = 0, n_inside = 0, n_outside = 0, n_delta = 0, n_hit = 0, n_first_would = 0, n_equal_sd = 0;
#pragma omp parallel for reduction(+ : bad, n_inside, n_outside, n_delta, n_hit, n_first_would, n_equal_sd) schedule(static)
  for (long long i = 0; i < N; ++i) {
    uint64_t s = 0x243F6A8885A308D3ULL ^ ((uint64_t)i * 0xD1342543DE82EF95ULL);
    const int family = (int)(i & 7);
    const double tmin = (i & 8) ? 0.0 : 1e-5, tmax = INFINITY;
    double bb, aa, cc;
    if (family <= 4) {
      /* o': a random direction at radius^2 in [0, 0.5] */
      double ox = 2.0 * unit(&s) - 1.0, oy = 2.0 * unit(&s) - 1.0, oz = 2.0 * unit(&s) - 1.0;
      double r2 = 0.5 * unit(&s);
      if (family == 2) r2 = 0.5; /* c at -0.5, then nudged by ulps below */
      const double k = sqrt(r2 / (ox * ox + oy * oy + oz * oz));
      ox *= k;
      oy *= k;
      oz *= k;
      if (family == 2) {
        const int ulps = (int)(next(&s) % 17) - 8;
        ox = from_bits(to_bits(ox) + (uint64_t)(int64_t)ulps);
      }
      cc = (ox * ox + oy * oy + oz * oz) - 1.0; /* pt_prep_hoist's order */
      /* d' = d * s: d inside the guard's range, ends included */
      int elo = 1023 - 340, ehi = 1023 + 340, slo = 1023 - 300, shi = 1023 + 300;
      if (family == 3) slo = 1, shi = 1023 - 200;    /* |d'| down to the subnormals: bb*bb and aa underflow */
      if (family == 4) slo = 1023 + 200, shi = 2046; /* ... and up to overflow */
      const double dx = guard_clamped(any_double(&s, elo, ehi)) * any_double(&s, slo, shi);
      const double dy = guard_clamped(any_double(&s, elo, ehi)) * any_double(&s, slo, shi);
      const double dz = guard_clamped(any_double(&s, elo, ehi)) * any_double(&s, slo, shi);
      aa = dx * dx + dy * dy + dz * dz;
      bb = 2.0 * (ox * dx + oy * dy + oz * dz);
    } else if (family <= 6) {
      /* raw triples: every exponent, infinities and NaNs; cc <= -0.5 by construction (NaN: the guard says no) */
      bb = any_double(&s, 0, 2047);
      aa = fabs(any_double(&s, 0, 2047));
      cc = -fabs(any_double(&s, 1022, 2047));
    } else {
      /* 4 aa |cc| = bb^2 * 2^-k: sd = |bb| exactly for k beyond the precision, one ulp above for smaller k */
      bb = any_double(&s, 1023 - 400, 1023 + 400);
      cc = -fabs(any_double(&s, 1022, 1030));
      const int k = 40 + (int)(next(&s) % 90);
      aa = ldexp(bb * bb, -k) / (4.0 * fabs(cc));
    }
    const int inside = origin_inside(cc);
    const Verdict want = roots(bb, aa, cc, tmin, tmax, 0), got = roots(bb, aa, cc, tmin, tmax, inside);
    if (got.ok != want.ok || to_bits(got.t) != to_bits(want.t)) ++bad;
    if (inside) {
      ++n_inside;
      const double delta = bb * bb - 4.0 * aa * cc;
      if (delta > 0.0) {
        ++n_delta;
        const double sd = sqrt(delta), t1 = (-bb - sd) / (2.0 * aa);
        if (t1 > tmin && t1 < tmax) ++n_first_would;
        if (sd == fabs(bb)) ++n_equal_sd;
      }
      if (want.ok) ++n_hit;
    } else {
      ++n_outside;
    }
  }
  printf("inputs: %lld; guard says inside: %lld, not inside: %lld; delta > 0: %lld; second root accepted: %lld; sd == |bb|: %lld\n", N,
         n_inside, n_outside, n_delta, n_hit, n_equal_sd);
  printf("first root acceptable under the guard: %lld; differences between the two forms: %lld\n", n_first_would, bad);
  return bad != 0 || n_first_would != 0;
}
