// pt_gradient.h -- the three kernels of include/ptrace_gradient.h: probes, keep and the accumulation.  Every kernel walks a
// grid-stride loop with one item (a stratum, a pixel) per lane, so no bit depends on the launch shape.  Included by
// ptrace_gradient.hip only, behind pt_kernels.h's query parts (PT_DEV, V3): nothing here is part of the other fifteen libraries, and
// none of their kernels is compiled into this one (the motion step, the projection, the unit normal, the luminance and the three tap
// batches of pt_motion.h are restated, as that header belongs to its unit).
//
// PROBES   a lane's chain is: the hash (integers only) -> shape[r] -> moved[s] -> the 21 doubles of the table.  The record's point
//          and normal do not depend on the shape, so they are issued with shape[r]; the table entry follows under the lane's
//          predicate.  There is one lane per STRATUM, a ninth of the frame at s = 3: no ballot is worth its trip here.
// KEEP     a lane's chain is probe_index[j] -> shape[q] -> colour[q], with probe_old[j] beside it.  The window is (2 radius + 1)^2
//          strata; the kernel is compiled once per radius (0..4) so that every loop over the window is unrolled and nothing is
//          indexed at run time.  Each ROW of the window is three batches -- the row's indices, then the shapes at them, then the
//          six doubles of every stratum still accepted -- each batch issued whole before its first value is used; the rows are
//          unrolled too, so the compiler is free to start a row's loads under the row before it as far as registers allow.  A whole
//          window in flight at once is 54 doubles at radius 1 (what the row form gives there as well, the rows being independent)
//          and 486 at radius 4, which no lane has registers for: there the rows bound what is in flight.  Neighbouring pixels
//          share their strata; the caches serve them (no LDS: not measured to pay).
// ACCUMULATE  pt_motion.h's chain with one more word: keep[r] is issued with the record and used after the taps.
// No atomics, no LDS, no array indexed at run time, nothing that depends on blockIdx but the item.
#pragma once

#define PT_GR_FLAG_SAME_SHAPE 1
#define PT_GR_FLAG_BLEND_WEIGHT 2
#define PT_GR_RECORD_DOUBLES 24
#define PT_GR_RADIUS_MAX 4

// ---- shared pieces ------------------------------------------------------------------------------------------------------------------
// nh(a) of the header: three divisions by one rounded length
PT_DEV V3 gr_unit(V3 a) {
  const double len = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x / len, a.y / len, a.z / len};
}

// lum(c) of the header: Color.luminosity with comparisons
PT_DEV double gr_lum(double c0, double c1, double c2) {
  double mx = c0, mn = c0;
  if (c1 > mx) mx = c1;
  if (c2 > mx) mx = c2;
  if (c1 < mn) mn = c1;
  if (c2 < mn) mn = c2;
  return (mx + mn) / 2.0;
}

// step 1 of ptrace_motion.h for a lane whose shape moved: the 21 doubles all in flight before the first is used
PT_DEV void gr_move(const double *__restrict__ rec, V3 &pp, V3 &nn) {
  double t[21];
#pragma unroll
  for (int i = 0; i < 21; i++) t[i] = rec[i];
  const V3 q = pp, g = nn;
  pp = {((t[0] * q.x + t[1] * q.y) + t[2] * q.z) + t[3], ((t[4] * q.x + t[5] * q.y) + t[6] * q.z) + t[7],
        ((t[8] * q.x + t[9] * q.y) + t[10] * q.z) + t[11]};
  nn = {(t[12] * g.x + t[13] * g.y) + t[14] * g.z, (t[15] * g.x + t[16] * g.y) + t[17] * g.z, (t[18] * g.x + t[19] * g.y) + t[20] * g.z};
}

// ---- 1. probes ----------------------------------------------------------------------------------------------------------------------
struct PtGrProbeK {
  int W, H, s;       // the frame and the stratum's side
  int gw;            // strata per row: ceil(W / s)
  int n_shapes;      // rows of the two tables (0: none is read)
  long long m, ns;   // W * H, and the number of strata
  unsigned long long phase, K, init_seq;
};

__global__ __launch_bounds__(PT_BLOCK) void pt_gr_probes_kernel(PtGrProbeK K, const int *__restrict__ shape, const double *__restrict__ normal,
                                                               const double *__restrict__ point, const int *__restrict__ moved,
                                                               const double *__restrict__ motion, int *__restrict__ probe_index,
                                                               double *__restrict__ probe_point, double *__restrict__ probe_normal,
                                                               unsigned long long *__restrict__ probe_seq) {
  const long long m = K.m, ns = K.ns;
  for (long long j = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; j < ns; j += (long long)gridDim.x * PT_BLOCK) {
    const int sy = (int)(j / K.gw), sx = (int)(j - (long long)sy * K.gw);
    const int left = K.W - sx * K.s, below = K.H - sy * K.s;
    const unsigned long long sw = (unsigned long long)(left < K.s ? left : K.s), sh = (unsigned long long)(below < K.s ? below : K.s);
    unsigned long long x = K.phase * 0x9E3779B97F4A7C15ULL + (unsigned long long)j * 0xD1B54A32D192ED03ULL + 0x2545F4914F6CDD1DULL;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ULL;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ULL;
    x ^= x >> 32;
    const int ox = (int)((x & 0xffffULL) % sw), oy = (int)(((x >> 16) & 0xffffULL) % sh);
    const long long r = (long long)(sy * K.s + oy) * K.W + (sx * K.s + ox);  // (inside the stratum, hence inside the frame)
    // the record, issued whole; the table depends on `sp`
    const int sp = shape[r];
    V3 pp = {point[r], point[m + r], point[2 * m + r]};
    V3 nn = {normal[r], normal[m + r], normal[2 * m + r]};
    const bool listed = sp >= 0 && sp < K.n_shapes;
    if (listed && moved[sp] != 0) gr_move(motion + (long long)sp * PT_GR_RECORD_DOUBLES, pp, nn);
    int at = -1;
    unsigned long long seq = 0;
    if (sp >= 0) {
      at = (int)r;
      seq = K.init_seq + (unsigned long long)r * K.K;
    } else {
      pp = nn = {0.0, 0.0, 0.0};
    }
    probe_index[j] = at;
    probe_point[j] = pp.x;
    probe_point[ns + j] = pp.y;
    probe_point[2 * ns + j] = pp.z;
    probe_normal[j] = nn.x;
    probe_normal[ns + j] = nn.y;
    probe_normal[2 * ns + j] = nn.z;
    probe_seq[j] = seq;
  }
}

// ---- 2. keep ------------------------------------------------------------------------------------------------------------------------
struct PtGrKeepK {
  int W, H, s;      // the frame and the stratum's side
  int gw, gh;       // the grid of strata
  int flags;        // PT_GR_SAME_SHAPE
  long long m, ns;  // W * H, gw * gh
  double gain;
};

template <int R>
__global__ __launch_bounds__(PT_BLOCK) void pt_gr_keep_kernel(PtGrKeepK K, const double *__restrict__ colour, const int *__restrict__ shape,
                                                             const int *__restrict__ probe_index, const double *__restrict__ probe_old,
                                                             double *__restrict__ keep) {
  constexpr int N = 2 * R + 1;
  const long long m = K.m, ns = K.ns;
  const bool same = K.flags & PT_GR_FLAG_SAME_SHAPE;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    const int sp = shape[r];
    double kp = 1.0;
    if (sp >= 0) {
      const int y = (int)(r / K.W), x = (int)(r - (long long)y * K.W);
      const int gx = x / K.s, gy = y / K.s;
      double num = 0.0, den = 0.0;
#pragma unroll
      for (int iy = 0; iy < N; iy++) {
        const int ty = gy + iy - R;
        const bool row = ty >= 0 && ty < K.gh;
        // batch a: the row's probe indices (a stratum outside the grid reads nothing)
        bool live[N];
        long long j[N], q[N];
#pragma unroll
        for (int ix = 0; ix < N; ix++) {
          const int tx = gx + ix - R;
          live[ix] = row && tx >= 0 && tx < K.gw;
          j[ix] = live[ix] ? (long long)ty * K.gw + tx : 0;
          q[ix] = live[ix] ? (long long)probe_index[j[ix]] : -1;
        }
        // batch b: the shapes at the indices somebody vouches for (no read at any other)
        int sq[N];
#pragma unroll
        for (int ix = 0; ix < N; ix++) {
          live[ix] = live[ix] && q[ix] >= 0 && q[ix] < m;
          sq[ix] = (live[ix] && same) ? shape[q[ix]] : sp;
        }
        // batch c: six doubles per stratum still accepted, all in flight before the first is used
        V3 cq[N], co[N];
#pragma unroll
        for (int ix = 0; ix < N; ix++) {
          live[ix] = live[ix] && sq[ix] == sp;
          cq[ix] = co[ix] = {0.0, 0.0, 0.0};
          if (live[ix]) {
            cq[ix] = {colour[q[ix]], colour[m + q[ix]], colour[2 * m + q[ix]]};
            co[ix] = {probe_old[j[ix]], probe_old[ns + j[ix]], probe_old[2 * ns + j[ix]]};
          }
        }
#pragma unroll
        for (int ix = 0; ix < N; ix++) {
          if (!live[ix]) continue;
          const double lc = gr_lum(cq[ix].x, cq[ix].y, cq[ix].z), lo = gr_lum(co[ix].x, co[ix].y, co[ix].z);
          double d = lc - lo;
          if (d < 0.0) d = 0.0 - d;
          const double mx = lc > lo ? lc : lo;
          num = num + d;
          den = den + mx;
        }
      }
      double lam = K.gain * (num / den);
      if (!(lam > 0.0)) lam = 0.0;
      if (lam > 1.0) lam = 1.0;
      kp = 1.0 - lam;
    }
    keep[r] = kp;
  }
}

// ---- 3. the accumulation: pt_motion.h's kernel, and `keep` ---------------------------------------------------------------------------
struct PtGrK {
  int W, H;        // the frame
  int max_history; // 1 .. 2^20
  int flags;       // PT_GR_* bits
  int persp;       // the previous camera is a PerspectiveCamera
  int n_shapes;    // rows of the two tables (0: none is read)
  long long m;     // W * H
  double normal_min, point_tolerance, max_weight;
  double invm[12]; // the previous camera's world -> camera rows
  double d, a;     // its screen_distance and aspect_ratio
};

// Steps 2 - 5 of ptrace_temporal.h: where `p` was on the previous screen, in pixels.  false: no history (behind the camera, off
// screen, NaN).
PT_DEV bool gr_project(const PtGrK &K, V3 p, double &fx, double &fy) {
  const double *m = K.invm;
  const double qx = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
  const double qy = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
  const double qz = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
  double u, v;
  if (K.persp) {
    const double tn = qx + K.d;
    if (!(tn > 0.0)) return false;
    const double s = K.d / tn;
    u = (1.0 - (qy * s) / K.a) * 0.5;
    v = (1.0 + qz * s) * 0.5;
  } else {
    const double tn = qx + 1.0;
    if (!(tn > 0.0)) return false;
    u = (1.0 - qy / K.a) * 0.5;
    v = (1.0 + qz) * 0.5;
  }
  fx = u * (double)K.W - 0.5;
  fy = (1.0 - v) * (double)K.H - 0.5;
  return fx > -1.0 && fx < (double)K.W && fy > -1.0 && fy < (double)K.H;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_gr_accumulate_kernel(PtGrK K, const double *__restrict__ colour, const int *__restrict__ samples,
                                                                   const int *__restrict__ shape, const double *__restrict__ normal,
                                                                   const double *__restrict__ point, const double *__restrict__ prev_colour,
                                                                   const double *__restrict__ prev_moments, const int *__restrict__ prev_shape,
                                                                   const double *__restrict__ prev_normal, const double *__restrict__ prev_point,
                                                                   const int *__restrict__ prev_count, const int *__restrict__ moved,
                                                                   const double *__restrict__ motion, const double *__restrict__ keep,
                                                                   double *__restrict__ out_colour, double *__restrict__ out_moments,
                                                                   int *__restrict__ out_count) {
  const long long m = K.m;
  const bool same = K.flags & PT_GR_FLAG_SAME_SHAPE, blend = K.flags & PT_GR_FLAG_BLEND_WEIGHT;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    // the record, keep[r] with it: everything is issued before the table, which depends on `sp`
    const int sp = shape[r];
    const int k = samples ? samples[r] : 1;
    const V3 cp = {colour[r], colour[m + r], colour[2 * m + r]};
    V3 pp = {point[r], point[m + r], point[2 * m + r]};
    V3 nn = {normal[r], normal[m + r], normal[2 * m + r]};
    double kp = keep ? keep[r] : 1.0;
    // 0a: the shape's word (an index outside the table is a static shape and reads nothing)
    const bool listed = sp >= 0 && sp < K.n_shapes;
    const bool mv = listed && moved[sp] != 0;
    // 0b: one ballot, then the 21 doubles of the lanes that moved
    if (__ballot(mv) != 0) {
      if (mv) gr_move(motion + (long long)sp * PT_GR_RECORD_DOUBLES, pp, nn);
    }
    V3 o = cp, mo = {0.0, 0.0, 0.0};
    int n = 0;
    if (sp >= 0) {
      const double kd = (double)k;
      const double l = gr_lum(cp.x, cp.y, cp.z);
      const double l2 = l * l;
      if (k > 0) {  // (step 4 until a tap is accepted)
        mo = {l, l2, kd};
        n = 1;
      }
      const V3 np = gr_unit(nn);
      double fx, fy;
      if (gr_project(K, pp, fx, fy)) {
        const double x0f = floor(fx), y0f = floor(fy);
        const double ax = fx - x0f, ay = fy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;  // (-1 .. W - 1, -1 .. H - 1: step 5 has passed)
        const double bx[2] = {1.0 - ax, ax}, by[2] = {1.0 - ay, ay};
        // batch 1: shape and count of the four taps
        bool live[4];
        long long at[4];
        int sq[4], nq[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const int x = x0 + (t & 1), y = y0 + (t >> 1);
          live[t] = x >= 0 && x < K.W && y >= 0 && y < K.H;
          at[t] = live[t] ? (long long)y * K.W + x : r;  // (a tap outside the frame reads nothing; `r` keeps the address legal)
          sq[t] = live[t] ? prev_shape[at[t]] : -1;
          nq[t] = live[t] ? prev_count[at[t]] : 0;
        }
        double b[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          b[t] = bx[t & 1] * by[t >> 1];
          live[t] = live[t] && nq[t] > 0 && sq[t] >= 0 && !(same && sq[t] != sp) && b[t] > 0.0;
        }
        // batch 2: normal and point of the taps still alive, all in flight before the first is used
        V3 nr[4], pr[4], cr[4], mr[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          nr[t] = pr[t] = cr[t] = mr[t] = {0.0, 0.0, 0.0};
          if (live[t]) {
            const long long q = at[t];
            nr[t] = {prev_normal[q], prev_normal[m + q], prev_normal[2 * m + q]};
            pr[t] = {prev_point[q], prev_point[m + q], prev_point[2 * m + q]};
          }
        }
        // the geometry tests against the MOVED record, then batch 3: colour and moments of the taps that passed them
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (!live[t]) continue;
          const V3 nu = gr_unit(nr[t]);
          const double c = np.x * nu.x + np.y * nu.y + np.z * nu.z;
          const double dz = np.x * (pr[t].x - pp.x) + np.y * (pr[t].y - pp.y) + np.z * (pr[t].z - pp.z);
          live[t] = (c >= K.normal_min) && (fabs(dz) <= K.point_tolerance);
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (live[t]) {
            const long long q = at[t];
            cr[t] = {prev_colour[q], prev_colour[m + q], prev_colour[2 * m + q]};
            mr[t] = {prev_moments[q], prev_moments[m + q], prev_moments[2 * m + q]};
          }
        }
        double h0 = 0.0, h1 = 0.0, h2 = 0.0, g1 = 0.0, g2 = 0.0, gS = 0.0, ws = 0.0, smax = 0.0;
        int nmax = 0;
        bool any = false;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (!live[t]) continue;
          h0 = h0 + b[t] * cr[t].x;
          h1 = h1 + b[t] * cr[t].y;
          h2 = h2 + b[t] * cr[t].z;
          g1 = g1 + b[t] * mr[t].x;
          g2 = g2 + b[t] * mr[t].y;
          gS = gS + b[t] * mr[t].z;
          ws = ws + b[t];
          nmax = nq[t] > nmax ? nq[t] : nmax;
          if (mr[t].z > smax) smax = mr[t].z;
          any = true;
        }
        if (any) {
          const double e0 = h0 / ws, e1 = h1 / ws, e2 = h2 / ws;
          const double m1 = g1 / ws, m2 = g2 / ws;
          double Sh = blend ? gS / ws : smax;
          if (!(Sh > 0.0)) Sh = 0.0;
          if (Sh > K.max_weight) Sh = K.max_weight;
          if (keep) {  // the insertion: the history's weight and length shrink where the light changed
            if (!(kp >= 0.0)) kp = 0.0;
            if (kp > 1.0) kp = 1.0;
            Sh = kp * Sh;
            nmax = (int)floor(kp * (double)nmax);
          }
          if (k > 0) {
            const double total = Sh + kd;
            const double alpha = kd / total;
            o = {e0 + (cp.x - e0) * alpha, e1 + (cp.y - e1) * alpha, e2 + (cp.z - e2) * alpha};
            mo = {m1 + (l - m1) * alpha, m2 + (l2 - m2) * alpha, total};
            n = nmax >= K.max_history ? K.max_history : nmax + 1;  // min(nmax + 1, max_history) without leaving an int
          } else {  // nothing was sampled here: the history is carried, this frame's colour never enters it
            o = {e0, e1, e2};
            mo = {m1, m2, Sh};
            n = nmax > K.max_history ? K.max_history : nmax;
          }
        }
      }
    }
    out_colour[r] = o.x;
    out_colour[m + r] = o.y;
    out_colour[2 * m + r] = o.z;
    out_moments[r] = mo.x;
    out_moments[m + r] = mo.y;
    out_moments[2 * m + r] = mo.z;
    out_count[r] = n;
  }
}
