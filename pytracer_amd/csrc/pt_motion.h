// pt_motion.h -- the accumulation of include/ptrace_motion.h: one kernel, one pixel per lane in frame order inside a grid-stride
// loop, so no bit depends on the launch shape.  Included by ptrace_motion.hip only, behind pt_kernels.h's query parts (PT_DEV, V3):
// nothing here is part of the other fourteen libraries, and none of their kernels is compiled into this one (the projection, the
// unit normal, the luminance and the three tap batches of pt_weighted.h are restated, as that header belongs to its unit).
//
// A lane's chain is pt_weighted.h's with one more link in front.  The table entry depends on shape[r]; `point`, `normal`, `colour`
// and `samples` do not, so all of the record is issued together and the table follows:
//     0a. moved[s], one word under the predicate 0 <= s < n_shapes (a table of a few shapes: it stays in the caches), issued as soon
//         as shape[r] is there, while the rest of the record is still in flight;
//     0b. ONE ballot: a wave in which no lane's shape moved skips the table batch altogether, so a frame of a static world costs the
//         one word above on top of the weighted kernel;  otherwise the 21 doubles of A_s and N_s under the lane's predicate, all in
//         flight before the first is used (12 + 9 named values, nothing indexed at run time);
//     1 - 3. the three tap batches of pt_weighted.h, on pm and nm.
// The word of 0a has to come back before the ballot can be taken: reading it TOGETHER with the 21 doubles would save that trip
// for a wave that moves and cost every static wave 21 loads it never uses -- the static frame is the common one.
// No atomics, no LDS, no array indexed at run time (every loop over the taps and over the table is unrolled), nothing that depends
// on blockIdx but the pixel.
#pragma once

#define PT_MA_FLAG_SAME_SHAPE 1
#define PT_MA_FLAG_BLEND_WEIGHT 2
#define PT_MA_RECORD_DOUBLES 24

struct PtMaK {
  int W, H;        // the frame
  int max_history; // 1 .. 2^20
  int flags;       // PT_MA_* bits
  int persp;       // the previous camera is a PerspectiveCamera
  int n_shapes;    // rows of the two tables (0: none is read)
  long long m;     // W * H
  double normal_min, point_tolerance, max_weight;
  double invm[12]; // the previous camera's world -> camera rows
  double d, a;     // its screen_distance and aspect_ratio
};

// nh(a) of the header: three divisions by one rounded length
PT_DEV V3 ma_unit(V3 a) {
  const double len = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x / len, a.y / len, a.z / len};
}

// lum(c) of the header: Color.luminosity with comparisons
PT_DEV double ma_lum(double c0, double c1, double c2) {
  double mx = c0, mn = c0;
  if (c1 > mx) mx = c1;
  if (c2 > mx) mx = c2;
  if (c1 < mn) mn = c1;
  if (c2 < mn) mn = c2;
  return (mx + mn) / 2.0;
}

// Steps 2 - 5 of ptrace_temporal.h: where `p` was on the previous screen, in pixels.  false: no history (behind the camera, off
// screen, NaN).
PT_DEV bool ma_project(const PtMaK &K, V3 p, double &fx, double &fy) {
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

__global__ __launch_bounds__(PT_BLOCK) void pt_ma_accumulate_kernel(PtMaK K, const double *__restrict__ colour, const int *__restrict__ samples,
                                                                   const int *__restrict__ shape, const double *__restrict__ normal,
                                                                   const double *__restrict__ point, const double *__restrict__ prev_colour,
                                                                   const double *__restrict__ prev_moments, const int *__restrict__ prev_shape,
                                                                   const double *__restrict__ prev_normal, const double *__restrict__ prev_point,
                                                                   const int *__restrict__ prev_count, const int *__restrict__ moved,
                                                                   const double *__restrict__ motion, double *__restrict__ out_colour,
                                                                   double *__restrict__ out_moments, int *__restrict__ out_count) {
  const long long m = K.m;
  const bool same = K.flags & PT_MA_FLAG_SAME_SHAPE, blend = K.flags & PT_MA_FLAG_BLEND_WEIGHT;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    // the record: everything is issued before the table, which depends on `sp`
    const int sp = shape[r];
    const int k = samples ? samples[r] : 1;
    const V3 cp = {colour[r], colour[m + r], colour[2 * m + r]};
    V3 pp = {point[r], point[m + r], point[2 * m + r]};
    V3 nn = {normal[r], normal[m + r], normal[2 * m + r]};
    // 0a: the shape's word (an index outside the table is a static shape and reads nothing)
    const bool listed = sp >= 0 && sp < K.n_shapes;
    const bool mv = listed && moved[sp] != 0;
    // 0b: one ballot, then the 21 doubles of the lanes that moved
    if (__ballot(mv) != 0) {
      if (mv) {
        const double *rec = motion + (long long)sp * PT_MA_RECORD_DOUBLES;
        double t[21];
#pragma unroll
        for (int i = 0; i < 21; i++) t[i] = rec[i];
        const V3 q = pp, g = nn;
        pp = {((t[0] * q.x + t[1] * q.y) + t[2] * q.z) + t[3], ((t[4] * q.x + t[5] * q.y) + t[6] * q.z) + t[7],
              ((t[8] * q.x + t[9] * q.y) + t[10] * q.z) + t[11]};
        nn = {(t[12] * g.x + t[13] * g.y) + t[14] * g.z, (t[15] * g.x + t[16] * g.y) + t[17] * g.z, (t[18] * g.x + t[19] * g.y) + t[20] * g.z};
      }
    }
    V3 o = cp, mo = {0.0, 0.0, 0.0};
    int n = 0;
    if (sp >= 0) {
      const double kd = (double)k;
      const double l = ma_lum(cp.x, cp.y, cp.z);
      const double l2 = l * l;
      if (k > 0) {  // (step 4 until a tap is accepted)
        mo = {l, l2, kd};
        n = 1;
      }
      const V3 np = ma_unit(nn);
      double fx, fy;
      if (ma_project(K, pp, fx, fy)) {
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
          const V3 nu = ma_unit(nr[t]);
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
