// pt_variance.h -- the kernels of include/ptrace_variance.h: luminance moments, the variance estimate, and the variance-guided
// a-trous filter (the unit-normal pre-pass, the prefiltered-variance plane and one pass of the 5x5 dilated stencil, in two variants
// that share every arithmetic operation: vr_tap).  Included by ptrace_variance.hip only, behind pt_kernels.h's query parts (PT_DEV,
// V3): nothing here is part of the other eleven libraries, and none of their kernels is compiled into this one.
//
// The filter starts from the denoise query's design.  LDS variant (pt_vr_lds_kernel<TW, TH>, TW * TH = 256): a workgroup takes one
// residue of the step and a TW x TH tile of that sub-lattice and stages its (TW + 4) x (TH + 4) records -- unit normal, point,
// colour, variance, luminance, shape: 92 bytes a slot, 36.8 KB for the 16 x 16 tile -- in LDS.  The luminance is formed ONCE per
// staged record instead of once per tap.  Slots outside the frame hold shape -1; under PT_VR_WRAP_X the staging address is wrapped.
//
// The prefiltered variance g needs the step-1 neighbours, which are not in a sub-lattice tile once s >= 2: a small pre-pass per pass
// (pt_vr_prefilter_kernel) writes g as a plane, at every step, and a pass reads ONE g per pixel from it.
//
// Direct variant (pt_vr_direct_kernel): one pixel per lane in frame order, every tap a global load, no LDS -- the A/B partner.
//
// The estimate (pt_vr_estimate_kernel) is direct: only short-history pixels walk the 7x7 window.
//
// All walk grid-stride loops over their work items, so no bit depends on the launch shape.  No atomics; nothing is indexed at run
// time but the planes themselves.
#pragma once

#define PT_VR_FLAG_SAME_SHAPE 1
#define PT_VR_FLAG_WRAP_X 2

struct PtVrK {
  int W, H;              // the frame
  int s;                 // the step of this pass, 2^i
  int flags, e;          // PT_VR_* bits; normal_power_log2
  int rxn, ryn;          // residues that have pixels: min(s, W), min(s, H)
  int tiles_x, tiles_y;  // tiles of one sub-lattice (LDS variant)
  int sp_inf, sl_inf;    // sigma_point * s / sigma_luminance^2 is +inf: the weight is 1.0 where its argument is finite
  int min_history;       // (the estimate)
  long long m;           // W * H
  long long nblocks;     // work items: tiles of all residues (LDS variant), ceil(m / 256) (the others)
  double sps;            // sigma_point * (double)s
  double sl2, epsilon;   // sigma_luminance^2; den = sl2 * g + epsilon
  double normal_min, point_tolerance;  // (the estimate)
};

struct VrSums {
  double c0, c1, c2, w, v;
};

// Color.luminosity with comparisons
PT_DEV double vr_lum(double c0, double c1, double c2) {
  double mx = c0, mn = c0;
  if (c1 > mx) mx = c1;
  if (c2 > mx) mx = c2;
  if (c1 < mn) mn = c1;
  if (c2 < mn) mn = c2;
  return (mx + mn) / 2.0;
}

// One tap that is not the centre and whose shape passed: the weights of include/ptrace_variance.h, operation for operation.  A
// division by an infinite sigma is not performed (as in dn_tap).
PT_DEV void vr_tap(const PtVrK &K, double k, double den, V3 np, V3 pp, double lp, V3 nq, V3 pq, V3 cq, double lq, double vq, VrSums &a) {
  double c = np.x * nq.x + np.y * nq.y + np.z * nq.z;
  if (!(c > 0.0)) c = 0.0;
  for (int j = 0; j < K.e; j++) c = c * c;
  const double dz = np.x * (pq.x - pp.x) + np.y * (pq.y - pp.y) + np.z * (pq.z - pp.z);
  double wp;
  if (K.sp_inf) {
    wp = (fabs(dz) < __builtin_inf()) ? 1.0 : __builtin_nan("");
  } else {
    const double t = dz / K.sps;
    wp = 1.0 / (1.0 + t * t);
  }
  const double dl = lq - lp;
  const double dl2 = dl * dl;
  double wl;
  if (K.sl_inf) {
    wl = (dl2 < __builtin_inf()) ? 1.0 : __builtin_nan("");
  } else {
    wl = 1.0 / (1.0 + dl2 / den);
  }
  const double w = ((k * c) * wp) * wl;
  if (w > 0.0) {
    a.c0 = a.c0 + w * cq.x;
    a.c1 = a.c1 + w * cq.y;
    a.c2 = a.c2 + w * cq.z;
    a.w = a.w + w;
    a.v = a.v + (w * w) * vq;
  }
}

PT_DEV void vr_centre(double k, V3 cp, double vp, VrSums &a) {
  a.c0 = a.c0 + k * cp.x;
  a.c1 = a.c1 + k * cp.y;
  a.c2 = a.c2 + k * cp.z;
  a.w = a.w + k;
  a.v = a.v + (k * k) * vp;
}

// h[d + 2] of the 5x5 stencil: (1/16, 1/4, 3/8, 1/4, 1/16), ptrace_denoise.h's; every product of two is exact
PT_DEV constexpr double vr_h(int d) { return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625; }

// the prefilter's (1/4, 1/2, 1/4): every product of two is exact
PT_DEV constexpr double vr_g(int d) { return d == 0 ? 0.5 : 0.25; }

// ---- 1. moments --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_vr_moments_kernel(const double *__restrict__ colour, const int *__restrict__ shape, long long m,
                                                                double *__restrict__ out) {
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    double l = 0.0, l2 = 0.0;
    if (shape[r] >= 0) {
      l = vr_lum(colour[r], colour[m + r], colour[2 * m + r]);
      l2 = l * l;
    }
    out[r] = l;
    out[m + r] = l2;
    out[2 * m + r] = 0.0;
  }
}

// ---- 2. the estimate ---------------------------------------------------------------------------------------------------------------
PT_DEV V3 vr_unit(const double *__restrict__ normal, long long m, long long r) {
  const double x = normal[r], y = normal[m + r], z = normal[2 * m + r];
  const double len = sqrt(x * x + y * y + z * z);
  return V3{x / len, y / len, z / len};
}

__global__ __launch_bounds__(PT_BLOCK) void pt_vr_estimate_kernel(PtVrK K, const double *__restrict__ moments, const int *__restrict__ count,
                                                                 const int *__restrict__ shape, const double *__restrict__ normal,
                                                                 const double *__restrict__ point, double *__restrict__ out) {
  const long long m = K.m;
  const bool same = K.flags & PT_VR_FLAG_SAME_SHAPE, wrap = K.flags & PT_VR_FLAG_WRAP_X;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    const int sp = shape[r], n = count[r];
    if (sp < 0 || n < 1) {
      out[r] = 0.0;
      continue;
    }
    double v;
    if (n >= K.min_history) {
      const double mu1 = moments[r], mu2 = moments[m + r];
      v = mu2 - mu1 * mu1;
    } else {
      const long long x = r % K.W, y = r / K.W;
      const V3 np = vr_unit(normal, m, r), pp = {point[r], point[m + r], point[2 * m + r]};
      double s1 = 0.0, s2 = 0.0, k = 0.0;
      for (int dy = -3; dy <= 3; dy++) {
        const long long qy = y + dy;
        if (qy < 0 || qy >= K.H) continue;
        for (int dx = -3; dx <= 3; dx++) {
          long long qx = x + dx;
          if (wrap) {
            qx %= K.W;
            if (qx < 0) qx += K.W;
          }
          if (qx < 0 || qx >= K.W) continue;
          const long long q = qy * K.W + qx;
          if (dx != 0 || dy != 0) {
            const int sq = shape[q];
            if (sq < 0 || (same && sq != sp)) continue;
            if (count[q] < 1) continue;
            const V3 nq = vr_unit(normal, m, q);
            const double c = np.x * nq.x + np.y * nq.y + np.z * nq.z;
            if (!(c >= K.normal_min)) continue;
            const double dz = np.x * (point[q] - pp.x) + np.y * (point[m + q] - pp.y) + np.z * (point[2 * m + q] - pp.z);
            if (!(fabs(dz) <= K.point_tolerance)) continue;
          }
          s1 = s1 + moments[q];
          s2 = s2 + moments[m + q];
          k = k + 1.0;
        }
      }
      const double mean = s1 / k;
      v = s2 / k - mean * mean;
    }
    if (!(v > 0.0)) v = 0.0;
    out[r] = v / (double)n;
  }
}

// ---- 3. the filter: the unit normals (once) and the prefiltered variance (per pass) ----------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_vr_unit_kernel(const double *__restrict__ normal, long long m, double *__restrict__ unit) {
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    const V3 u = vr_unit(normal, m, r);
    unit[r] = u.x;
    unit[m + r] = u.y;
    unit[2 * m + r] = u.z;
  }
}

__global__ __launch_bounds__(PT_BLOCK) void pt_vr_prefilter_kernel(PtVrK K, const double *__restrict__ var, const int *__restrict__ shape,
                                                                  double *__restrict__ g) {
  const bool same = K.flags & PT_VR_FLAG_SAME_SHAPE, wrap = K.flags & PT_VR_FLAG_WRAP_X;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < K.m; r += (long long)gridDim.x * PT_BLOCK) {
    const long long x = r % K.W, y = r / K.W;
    const int sp = shape[r];
    double gs = 0.0, gw = 0.0;
    if (sp >= 0) {
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          const double kw = vr_g(dx) * vr_g(dy);
          long long qx = x + dx;
          const long long qy = y + dy;
          if (wrap) {
            qx %= K.W;
            if (qx < 0) qx += K.W;
          }
          if (qx < 0 || qx >= K.W || qy < 0 || qy >= K.H) continue;
          const long long q = qy * K.W + qx;
          const int sq = shape[q];
          if (sq < 0 || (same && sq != sp)) continue;
          const double vq = var[q];
          if (!(vq >= 0.0)) continue;
          gs = gs + kw * vq;
          gw = gw + kw;
        }
      }
    }
    g[r] = gw > 0.0 ? gs / gw : 0.0;
  }
}

// ---- one pass, LDS variant ---------------------------------------------------------------------------------------------------------
template <int TW, int TH>
__global__ __launch_bounds__(PT_BLOCK) void pt_vr_lds_kernel(PtVrK K, const double *__restrict__ colour, const double *__restrict__ var,
                                                            const double *__restrict__ g, const double *__restrict__ unit,
                                                            const double *__restrict__ point, const int *__restrict__ shape,
                                                            double *__restrict__ out, double *__restrict__ out_var) {
  static_assert(TW * TH == PT_BLOCK, "one pixel per lane");
  constexpr int LW = TW + 4, LH = TH + 4, NS = LW * LH;
  __shared__ double s_v[11][NS];  // unit normal xyz, point xyz, colour xyz, variance, luminance
  __shared__ int s_shape[NS];
  const int tid = threadIdx.x, lx = tid % TW, ly = tid / TW;
  const long long m = K.m;
  const bool same = K.flags & PT_VR_FLAG_SAME_SHAPE, wrap = K.flags & PT_VR_FLAG_WRAP_X;
  for (long long b = blockIdx.x; b < K.nblocks; b += gridDim.x) {  // (uniform per workgroup: the barriers below are reached by all)
    long long t = b;
    const long long u0 = (t % K.tiles_x) * TW;
    t /= K.tiles_x;
    const int rx = (int)(t % K.rxn);
    t /= K.rxn;
    const long long v0 = (t % K.tiles_y) * TH;
    const int ry = (int)(t / K.tiles_y);
    // stage the tile and its halo of 2: slot (ui, vi) is sub-lattice pixel (u0 - 2 + ui, v0 - 2 + vi)
    for (int i = tid; i < NS; i += PT_BLOCK) {
      const int ui = i % LW, vi = i / LW;
      long long x = rx + (u0 - 2 + ui) * K.s;
      const long long y = ry + (v0 - 2 + vi) * K.s;
      if (wrap) {
        x %= K.W;
        if (x < 0) x += K.W;
      }
      int sh = -1;
      double v[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (x >= 0 && x < K.W && y >= 0 && y < K.H) {
        const long long r = y * K.W + x;
        sh = shape[r];
        if (sh >= 0) {
#pragma unroll
          for (int j = 0; j < 3; j++) {
            v[j] = unit[j * m + r];
            v[3 + j] = point[j * m + r];
            v[6 + j] = colour[j * m + r];
          }
          v[9] = var[r];
          v[10] = vr_lum(v[6], v[7], v[8]);
        }
      }
      s_shape[i] = sh;
#pragma unroll
      for (int j = 0; j < 11; j++) s_v[j][i] = v[j];
    }
    __syncthreads();
    const long long x = rx + (u0 + lx) * K.s, y = ry + (v0 + ly) * K.s;
    if (x < K.W && y < K.H) {
      const long long r = y * K.W + x;
      const int c = (ly + 2) * LW + lx + 2;
      const int sp = s_shape[c];
      if (sp < 0) {
        out[r] = colour[r];
        out[m + r] = colour[m + r];
        out[2 * m + r] = colour[2 * m + r];
        out_var[r] = var[r];
      } else {
        const V3 np = {s_v[0][c], s_v[1][c], s_v[2][c]}, pp = {s_v[3][c], s_v[4][c], s_v[5][c]}, cp = {s_v[6][c], s_v[7][c], s_v[8][c]};
        const double lp = s_v[10][c];
        const double den = K.sl2 * g[r] + K.epsilon;
        VrSums a = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
          for (int dx = -2; dx <= 2; dx++) {
            const double k = vr_h(dx) * vr_h(dy);
            if (dx == 0 && dy == 0) {
              vr_centre(k, cp, s_v[9][c], a);
              continue;
            }
            const int q = c + dy * LW + dx;
            const int sq = s_shape[q];
            if (sq < 0 || (same && sq != sp)) continue;
            const V3 nq = {s_v[0][q], s_v[1][q], s_v[2][q]}, pq = {s_v[3][q], s_v[4][q], s_v[5][q]}, cq = {s_v[6][q], s_v[7][q], s_v[8][q]};
            vr_tap(K, k, den, np, pp, lp, nq, pq, cq, s_v[10][q], s_v[9][q], a);
          }
        }
        out[r] = a.c0 / a.w;
        out[m + r] = a.c1 / a.w;
        out[2 * m + r] = a.c2 / a.w;
        out_var[r] = a.v / (a.w * a.w);
      }
    }
    __syncthreads();  // (the next tile's staging overwrites what this one read)
  }
}

// ---- one pass, direct variant: every tap a global load ----------------------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_vr_direct_kernel(PtVrK K, const double *__restrict__ colour, const double *__restrict__ var,
                                                               const double *__restrict__ g, const double *__restrict__ unit,
                                                               const double *__restrict__ point, const int *__restrict__ shape,
                                                               double *__restrict__ out, double *__restrict__ out_var) {
  const long long m = K.m;
  const bool same = K.flags & PT_VR_FLAG_SAME_SHAPE, wrap = K.flags & PT_VR_FLAG_WRAP_X;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    const long long x = r % K.W, y = r / K.W;
    const int sp = shape[r];
    const V3 cp = {colour[r], colour[m + r], colour[2 * m + r]};
    const double vp = var[r];
    if (sp < 0) {
      out[r] = cp.x;
      out[m + r] = cp.y;
      out[2 * m + r] = cp.z;
      out_var[r] = vp;
      continue;
    }
    const V3 np = {unit[r], unit[m + r], unit[2 * m + r]}, pp = {point[r], point[m + r], point[2 * m + r]};
    const double lp = vr_lum(cp.x, cp.y, cp.z);
    const double den = K.sl2 * g[r] + K.epsilon;
    VrSums a = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const double k = vr_h(dx) * vr_h(dy);
        if (dx == 0 && dy == 0) {
          vr_centre(k, cp, vp, a);
          continue;
        }
        long long qx = x + (long long)K.s * dx;
        const long long qy = y + (long long)K.s * dy;
        if (wrap) {
          qx %= K.W;
          if (qx < 0) qx += K.W;
        }
        if (qx < 0 || qx >= K.W || qy < 0 || qy >= K.H) continue;
        const long long q = qy * K.W + qx;
        const int sq = shape[q];
        if (sq < 0 || (same && sq != sp)) continue;
        const V3 nq = {unit[q], unit[m + q], unit[2 * m + q]}, pq = {point[q], point[m + q], point[2 * m + q]},
                 cq = {colour[q], colour[m + q], colour[2 * m + q]};
        vr_tap(K, k, den, np, pp, lp, nq, pq, cq, vr_lum(cq.x, cq.y, cq.z), var[q], a);
      }
    }
    out[r] = a.c0 / a.w;
    out[m + r] = a.c1 / a.w;
    out[2 * m + r] = a.c2 / a.w;
    out_var[r] = a.v / (a.w * a.w);
  }
}
