// pt_temporal.h -- the accumulation of include/ptrace_temporal.h: one kernel, one pixel per lane in frame order inside a grid-stride
// loop, so no bit depends on the launch shape.  Included by ptrace_temporal.hip only, behind pt_kernels.h's query parts (PT_DEV,
// V3): nothing here is part of the other ten libraries.
//
// A lane's chain: its own record (shape, colour, point, normal), two divisions to the previous screen, then four taps at addresses
// that depend on them.  The kernel is expected to be bound by that latency and not by arithmetic, so the taps are read in two
// batches that each leave all their loads in flight before the first use:
//     1. prev_shape and prev_count of the four taps (8 words): every test that needs no fp64 record is made on these, so a tap
//        that is rejected here costs two words;
//     2. prev_normal, prev_point and prev_colour of the taps still alive (4 x 9 doubles), each tap under its own predicate, all
//        issued before the loop that consumes them.
// No atomics, no LDS (neighbouring lanes' taps overlap, but only in L2-resident lines: nothing measured pays for staging them), no
// array indexed at run time (every loop over the taps is unrolled), nothing that depends on blockIdx but the pixel.
#pragma once

#define PT_TA_FLAG_SAME_SHAPE 1

struct PtTaK {
  int W, H;        // the frame
  int max_history; // 1 .. 2^20
  int flags;       // PT_TA_* bits
  int persp;       // the previous camera is a PerspectiveCamera
  long long m;     // W * H
  double normal_min, point_tolerance;
  double invm[12]; // the previous camera's world -> camera rows
  double d, a;     // its screen_distance and aspect_ratio
};

// nh(a) of the header: three divisions by one rounded length
PT_DEV V3 ta_unit(V3 a) {
  const double len = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x / len, a.y / len, a.z / len};
}

// Steps 2 - 5: where `p` was on the previous screen, in pixels.  false: no history (behind the camera, off screen, NaN).
PT_DEV bool ta_project(const PtTaK &K, V3 p, double &fx, double &fy) {
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

__global__ __launch_bounds__(PT_BLOCK) void pt_ta_accumulate_kernel(PtTaK K, const double *__restrict__ colour, const int *__restrict__ shape,
                                                                   const double *__restrict__ normal, const double *__restrict__ point,
                                                                   const double *__restrict__ prev_colour, const int *__restrict__ prev_shape,
                                                                   const double *__restrict__ prev_normal, const double *__restrict__ prev_point,
                                                                   const int *__restrict__ prev_count, double *__restrict__ out_colour,
                                                                   int *__restrict__ out_count) {
  const long long m = K.m;
  const bool same = K.flags & PT_TA_FLAG_SAME_SHAPE;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    const int sp = shape[r];
    const V3 cp = {colour[r], colour[m + r], colour[2 * m + r]};
    V3 o = cp;
    int n = sp < 0 ? 0 : 1;
    if (sp >= 0) {
      const V3 pp = {point[r], point[m + r], point[2 * m + r]};
      const V3 np = ta_unit({normal[r], normal[m + r], normal[2 * m + r]});
      double fx, fy;
      if (ta_project(K, pp, fx, fy)) {
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
        // batch 2: the records of the taps still alive, all in flight before the first is used
        V3 nr[4], pr[4], cr[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          nr[t] = pr[t] = cr[t] = {0.0, 0.0, 0.0};
          if (live[t]) {
            const long long q = at[t];
            nr[t] = {prev_normal[q], prev_normal[m + q], prev_normal[2 * m + q]};
            pr[t] = {prev_point[q], prev_point[m + q], prev_point[2 * m + q]};
            cr[t] = {prev_colour[q], prev_colour[m + q], prev_colour[2 * m + q]};
          }
        }
        double h0 = 0.0, h1 = 0.0, h2 = 0.0, ws = 0.0;
        int nmax = 0;
        bool any = false;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (!live[t]) continue;
          const V3 nu = ta_unit(nr[t]);
          const double c = np.x * nu.x + np.y * nu.y + np.z * nu.z;
          const double dz = np.x * (pr[t].x - pp.x) + np.y * (pr[t].y - pp.y) + np.z * (pr[t].z - pp.z);
          if (!(c >= K.normal_min) || !(fabs(dz) <= K.point_tolerance)) continue;
          h0 = h0 + b[t] * cr[t].x;
          h1 = h1 + b[t] * cr[t].y;
          h2 = h2 + b[t] * cr[t].z;
          ws = ws + b[t];
          nmax = nq[t] > nmax ? nq[t] : nmax;
          any = true;
        }
        if (any) {
          n = nmax >= K.max_history ? K.max_history : nmax + 1;  // min(nmax + 1, max_history) without leaving an int
          const double alpha = 1.0 / (double)n;
          const double g0 = h0 / ws, g1 = h1 / ws, g2 = h2 / ws;
          o = {g0 + (cp.x - g0) * alpha, g1 + (cp.y - g1) * alpha, g2 + (cp.z - g2) * alpha};
        }
      }
    }
    out_colour[r] = o.x;
    out_colour[m + r] = o.y;
    out_colour[2 * m + r] = o.z;
    out_count[r] = n;
  }
}
