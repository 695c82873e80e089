// pt_denoise.h -- the edge-avoiding a-trous filter of include/ptrace_denoise.h: the unit-normal pre-pass and one pass of the 5x5
// dilated stencil, in two variants that share every arithmetic operation (dn_tap).  Included by ptrace_denoise.hip only, behind
// pt_kernels.h's query parts (PT_DEV, V3): nothing here is part of the other nine libraries.
//
// The first kernel of this tree in which a lane reads its NEIGHBOURS' records.
//
// LDS variant (pt_dn_lds_kernel<TW, TH>, TW * TH = 256).  A pass of step s splits the frame into s^2 independent sub-lattices, the
// pixels congruent (rx, ry) modulo s, and within one sub-lattice the stencil is a DENSE 5x5.  So a workgroup takes one residue and a
// TW x TH tile of that sub-lattice and stages its (TW + 4) x (TH + 4) records -- unit normal, point, colour, shape: 76 bytes -- in
// LDS, whatever s is (a tile of the full frame would need a halo of 2 s).  Slots outside the frame hold shape -1, which is what skips
// a tap anyway; under PT_DN_WRAP_X the staging address is wrapped, so the stencil never thinks about the seam.  Planes are per
// component (structure of arrays, ds_read_b64).  The price of the sub-lattice tiling is strided global reads at s >= 2.
//
// The tile.  By the LDS bank rule a half-wave of a 32 x 8 tile reads 32 CONSECUTIVE doubles of one row -- every one of the 64 banks
// once, for every tap and any row pitch -- where a half-wave of a 16 x 16 tile reads two rows of 16, conflict-free only at a pitch of
// 16 mod 32 doubles (48 for a staged row of 20).  Measured (tools/denoisebench.py, profiles/denoise_kernel.txt) it is the other way
// round: 16 x 16 is the fastest at every step and 25 % ahead over four passes, 32 x 8 and 64 x 4 losing most at s = 8, where a wider
// tile stages longer strided rows.  So 16 x 16 (pitch 20) is the default and the other two are launch alternatives.
//
// Direct variant (pt_dn_direct_kernel): one pixel per lane in frame order, every tap a global load, no LDS -- the A/B partner.
//
// Both walk a grid-stride loop over their work items, so no bit depends on the launch shape.  No atomics; nothing is indexed at
// run time but the planes themselves.
#pragma once

#define PT_DN_FLAG_SAME_SHAPE 1
#define PT_DN_FLAG_WRAP_X 2

struct PtDnK {
  int W, H;          // the frame
  int s;             // the step of this pass, 2^i
  int flags, e;      // PT_DN_* bits; normal_power_log2
  int rxn, ryn;      // residues that have pixels: min(s, W), min(s, H)
  int tiles_x, tiles_y;  // tiles of one sub-lattice (LDS variant)
  int sp_inf, sc_inf;    // sigma_point * s / (sigma_colour * 2^-i)^2 is +inf: the weight is 1.0 where its argument is finite
  long long m;       // W * H
  long long nblocks; // work items: tiles of all residues (LDS variant), ceil(m / 256) (direct variant)
  double sps;        // sigma_point * (double)s
  double sc2;        // sc * sc, sc = sigma_colour * 2^-i
};

struct DnSums {
  double c0, c1, c2, w;
};

// One tap that is not the centre and whose shape passed: the weights of include/ptrace_denoise.h, operation for operation.
// A division by an infinite sigma is not performed: x / inf is +-0.0 for a finite x and NaN otherwise, so 1 / (1 + (x / inf)^2) is
// exactly 1.0 or NaN -- the same bits, two fp64 divisions less per tap with the default sigma_colour.
PT_DEV void dn_tap(const PtDnK &K, double k, V3 np, V3 pp, V3 cp, V3 nq, V3 pq, V3 cq, DnSums &a) {
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
  const double d0 = cq.x - cp.x, d1 = cq.y - cp.y, d2c = cq.z - cp.z;
  const double d2 = (d0 * d0 + d1 * d1) + d2c * d2c;
  double wc;
  if (K.sc_inf) {
    wc = (d2 < __builtin_inf()) ? 1.0 : __builtin_nan("");
  } else {
    wc = 1.0 / (1.0 + d2 / K.sc2);
  }
  const double w = ((k * c) * wp) * wc;
  if (w > 0.0) {
    a.c0 = a.c0 + w * cq.x;
    a.c1 = a.c1 + w * cq.y;
    a.c2 = a.c2 + w * cq.z;
    a.w = a.w + w;
  }
}

PT_DEV void dn_centre(double k, V3 cp, DnSums &a) {
  a.c0 = a.c0 + k * cp.x;
  a.c1 = a.c1 + k * cp.y;
  a.c2 = a.c2 + k * cp.z;
  a.w = a.w + k;
}

// h[d + 2]: (1/16, 1/4, 3/8, 1/4, 1/16); every product of two is exact
PT_DEV constexpr double dn_h(int d) { return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625; }

// ---- the pre-pass: nh(normal) for every record, into the workspace ---------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_dn_unit_kernel(const double *__restrict__ normal, long long m, double *__restrict__ unit) {
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    const double x = normal[r], y = normal[m + r], z = normal[2 * m + r];
    const double len = sqrt(x * x + y * y + z * z);
    unit[r] = x / len;
    unit[m + r] = y / len;
    unit[2 * m + r] = z / len;
  }
}

// ---- one pass, LDS variant ---------------------------------------------------------------------------------------------------------
template <int TW, int TH>
__global__ __launch_bounds__(PT_BLOCK) void pt_dn_lds_kernel(PtDnK K, const double *__restrict__ colour, const double *__restrict__ unit,
                                                            const double *__restrict__ point, const int *__restrict__ shape,
                                                            double *__restrict__ out) {
  static_assert(TW * TH == PT_BLOCK, "one pixel per lane");
  constexpr int LW = TW + 4, LH = TH + 4, NS = LW * LH;
  __shared__ double s_v[9][NS];  // unit normal xyz, point xyz, colour xyz
  __shared__ int s_shape[NS];
  const int tid = threadIdx.x, lx = tid % TW, ly = tid / TW;
  const long long m = K.m;
  const bool same = K.flags & PT_DN_FLAG_SAME_SHAPE, wrap = K.flags & PT_DN_FLAG_WRAP_X;
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
      double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
        }
      }
      s_shape[i] = sh;
#pragma unroll
      for (int j = 0; j < 9; j++) s_v[j][i] = v[j];
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
      } else {
        const V3 np = {s_v[0][c], s_v[1][c], s_v[2][c]}, pp = {s_v[3][c], s_v[4][c], s_v[5][c]}, cp = {s_v[6][c], s_v[7][c], s_v[8][c]};
        DnSums a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
          for (int dx = -2; dx <= 2; dx++) {
            const double k = dn_h(dx) * dn_h(dy);
            if (dx == 0 && dy == 0) {
              dn_centre(k, cp, a);
              continue;
            }
            const int q = c + dy * LW + dx;
            const int sq = s_shape[q];
            if (sq < 0 || (same && sq != sp)) continue;
            const V3 nq = {s_v[0][q], s_v[1][q], s_v[2][q]}, pq = {s_v[3][q], s_v[4][q], s_v[5][q]}, cq = {s_v[6][q], s_v[7][q], s_v[8][q]};
            dn_tap(K, k, np, pp, cp, nq, pq, cq, a);
          }
        }
        out[r] = a.c0 / a.w;
        out[m + r] = a.c1 / a.w;
        out[2 * m + r] = a.c2 / a.w;
      }
    }
    __syncthreads();  // (the next tile's staging overwrites what this one read)
  }
}

// ---- one pass, direct variant: every tap a global load ----------------------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_dn_direct_kernel(PtDnK K, const double *__restrict__ colour, const double *__restrict__ unit,
                                                               const double *__restrict__ point, const int *__restrict__ shape,
                                                               double *__restrict__ out) {
  const long long m = K.m;
  const bool same = K.flags & PT_DN_FLAG_SAME_SHAPE, wrap = K.flags & PT_DN_FLAG_WRAP_X;
  for (long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * PT_BLOCK) {
    const long long x = r % K.W, y = r / K.W;
    const int sp = shape[r];
    const V3 cp = {colour[r], colour[m + r], colour[2 * m + r]};
    if (sp < 0) {
      out[r] = cp.x;
      out[m + r] = cp.y;
      out[2 * m + r] = cp.z;
      continue;
    }
    const V3 np = {unit[r], unit[m + r], unit[2 * m + r]}, pp = {point[r], point[m + r], point[2 * m + r]};
    DnSums a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const double k = dn_h(dx) * dn_h(dy);
        if (dx == 0 && dy == 0) {
          dn_centre(k, cp, a);
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
        dn_tap(K, k, np, pp, cp, nq, pq, cq, a);
      }
    }
    out[r] = a.c0 / a.w;
    out[m + r] = a.c1 / a.w;
    out[2 * m + r] = a.c2 / a.w;
  }
}
