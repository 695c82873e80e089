// pt_lit.h -- hit records shaded from a lattice of SH probes: corners, blend, evaluation and the material (include/ptrace_lit.h).
// Included by ptrace_lit.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h, pt_shade.h): nothing here is part of
// the other eight libraries.
//
// What it restates: ProbeGrid.corners and ProbeGrid.blend (pytracer_amd/rays.py) and the evaluation of include/ptrace_sh.h, operation
// for operation, per record instead of per batch; for the shade query also the mirror direction of scatter_ray (pt_shade.h, used as
// it is) and the look-up of a record nobody vouches for (slot table, texel clamp) -- pt_surface.h's, and the SH basis -- pt_sh.h's,
// both restated under names of their own: those headers belong to their one translation unit each.
//
// One record per lane, planar 8-byte loads and stores (512 consecutive bytes per wave), as pt_surface_kernel.  The coefficient block
// is read where the projection wrote it, [27][n]: per lane 27 planes x 8 corners = 216 gathered 8-byte loads, of which the two ix
// neighbours are adjacent words and which the coherent pixels of a wave share with their cell.  The blend of plane q = 3 j + ch is
// consumed at once by the evaluation's term j of channel ch, so what lives across the 27 planes is three sums, eight weights, eight
// row numbers and nine basis weights: nothing is indexed at run time (every loop below is unrolled over compile-time bounds), and
// nothing of size 27 is kept.  The order ACROSS planes is the evaluation's (j ascending per channel); the order WITHIN a plane is
// the blend's, corner 0 .. 7 from 0.0.
#pragma once

struct PtLitK {
  double origin[3], step[3];
  int dims[3];
  long long n;  // nx ny nz <= 2^31 - 1: rows of a coefficient plane
};

// ---- Y_0 .. Y_8 of include/ptrace_sh.h: each constant ONE literal, the products in the header's order ----------------------------
struct LitBasis {
  double y0, y1, y2, y3, y4, y5, y6, y7, y8;
};
PT_DEV LitBasis lit_basis(double x, double y, double z) {
  LitBasis b;
  b.y0 = 0.28209479177387814;
  b.y1 = 0.4886025119029199 * y;
  b.y2 = 0.4886025119029199 * z;
  b.y3 = 0.4886025119029199 * x;
  b.y4 = 1.0925484305920792 * (x * y);
  b.y5 = 1.0925484305920792 * (y * z);
  b.y6 = 0.31539156525252005 * (3.0 * (z * z) - 1.0);
  b.y7 = 1.0925484305920792 * (x * z);
  b.y8 = 0.5462742152960396 * (x * x - y * y);
  return b;
}

// materials.py:70-82 for a (u, v) that may be negative, huge or NaN: not >= 0 -> 0, >= w -> w - 1, else int()'s truncation.
PT_DEV long long lit_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}

template <typename CP>
PT_DEV V3 lit_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = lit_texel(u, w), row = lit_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}

// World.shapes index -> grouped slot, or -1: an index outside [0, n_shapes) is "no hit", and so is a table entry that does
// not name a record (the table is the caller's memory).
PT_DEV int lit_slot(const PtKArgs &a, const int *__restrict__ slots, int index) {
  if ((unsigned)index >= (unsigned)a.n_shapes) return -1;
  const int s = slots[index];
  return ((unsigned)s < (unsigned)a.n_shapes) ? s : -1;
}

// the host form's own slot table: slots[recs[s].index] = s (`index` is a permutation of 0 .. n_shapes - 1)
__global__ __launch_bounds__(PT_BLOCK) void pt_lit_slots_kernel(const PtKArgs a, int *__restrict__ slots) {
  const int s = blockIdx.x * PT_BLOCK + threadIdx.x;
  if (s >= a.n_shapes) return;
  const int index = a.recs[s].index;
  if ((unsigned)index < (unsigned)a.n_shapes) slots[index] = s;
}

// ---- CORNERS of include/ptrace_lit.h ---------------------------------------------------------------------------------------------
// numpy's clip is minimum(maximum(x, lo), hi) with the second operand taken where the comparison fails; a NaN never reaches it
// here (the record is answered with zeros), but whatever g is, i0 and i1 are rows of the lattice: lo when `x > lo` fails.
struct LitAxis {
  int i0, i1;
  double f;
};
PT_DEV LitAxis lit_axis(double p, double origin, double step, int dim) {
  double g = (p - origin) / step;
  const double near = rint(g);
  if (fabs(g - near) <= (4.0 * 0x1p-52) * max2(fabs(g), 1.0)) g = near;
  const double top = (double)(dim >= 2 ? dim - 2 : 0);
  double lo = floor(g);
  lo = (lo > 0.0) ? lo : 0.0;
  lo = (lo < top) ? lo : top;
  LitAxis r;
  r.i0 = (int)lo;  // 0 <= lo <= top < 2^31
  double f = g - (double)r.i0;
  f = (f > 0.0) ? f : 0.0;
  f = (f < 1.0) ? f : 1.0;
  r.f = f;
  r.i1 = (r.i0 + 1 < dim - 1) ? r.i0 + 1 : dim - 1;
  return r;
}

struct LitCell {
  long long row[8];  // each in [0, n)
  double w[8];
};
PT_DEV LitCell lit_cell(const PtLitK &K, V3 p) {
  const LitAxis ax = lit_axis(p.x, K.origin[0], K.step[0], K.dims[0]);
  const LitAxis ay = lit_axis(p.y, K.origin[1], K.step[1], K.dims[1]);
  const LitAxis az = lit_axis(p.z, K.origin[2], K.step[2], K.dims[2]);
  const double gx = 1.0 - ax.f, gy = 1.0 - ay.f, gz = 1.0 - az.f;
  LitCell c;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int ix = (k & 1) ? ax.i1 : ax.i0, iy = (k & 2) ? ay.i1 : ay.i0, iz = (k & 4) ? az.i1 : az.i0;
    c.row[k] = ((long long)iz * K.dims[1] + iy) * K.dims[0] + ix;
    c.w[k] = (((k & 1) ? ax.f : gx) * ((k & 2) ? ay.f : gy)) * ((k & 4) ? az.f : gz);
  }
  return c;
}

// ---- BLEND and EVALUATION: E[ch] = sum over j of (A_j * Y_j(d)) * b[3 j + ch], b[q] = sum over corners from 0.0 ------------------------
PT_DEV V3 lit_blend_eval(const double *__restrict__ coeffs, long long n, const LitCell &c, V3 d, int kind) {
  const LitBasis b = lit_basis(d.x, d.y, d.z);
  const double a1 = kind == PT_LIT_HEMISPHERE ? 2.0 / 3.0 : 1.0, a2 = kind == PT_LIT_HEMISPHERE ? 0.25 : 1.0;
  const double w[9] = {1.0 * b.y0, a1 * b.y1, a1 * b.y2, a1 * b.y3, a2 * b.y4, a2 * b.y5, a2 * b.y6, a2 * b.y7, a2 * b.y8};
  double o[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 9; j++) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const double *plane = coeffs + (size_t)(3 * j + ch) * (size_t)n;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 8; k++) s = s + c.w[k] * plane[c.row[k]];
      o[ch] = o[ch] + w[j] * s;
    }
  }
  V3 r = {o[0], o[1], o[2]};
  return r;
}

PT_DEV bool lit_is_nan(V3 p) { return p.x != p.x || p.y != p.y || p.z != p.z; }

// ---- the lit query: no scene ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_lit_eval_kernel(const PtLitK K, const double *__restrict__ coeffs, const double *__restrict__ points,
                                                               const double *__restrict__ dirs, const int *__restrict__ act, long long m, int kind,
                                                               double *__restrict__ out) {
  const long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (r >= m) return;
  V3 e = {0.0, 0.0, 0.0};
  if (act == nullptr || act[r] >= 0) {
    const V3 p = {points[r], points[m + r], points[2 * m + r]};
    const V3 d = {dirs[r], dirs[m + r], dirs[2 * m + r]};
    if (!lit_is_nan(p)) e = lit_blend_eval(coeffs, K.n, lit_cell(K, p), d, kind);
  }
  out[r] = e.x;
  out[m + r] = e.y;
  out[2 * m + r] = e.z;
}

// ---- the shade query: emitted + brdf_color * E, or the background ------------------------------------------------------------------
// A lane without a hit reads its shape index and nothing else.  The two BRDFs differ in the direction and the band factors alone, so
// a mixed wave runs the 216 loads once.
__global__ __launch_bounds__(PT_BLOCK) void pt_lit_shade_kernel(const PtKArgs a, const int *__restrict__ slots, const PtLitK K,
                                                                const double *__restrict__ coeffs, const int *__restrict__ shape,
                                                                const double *__restrict__ point, const double *__restrict__ normal,
                                                                const double *__restrict__ uv, const double *__restrict__ dir, long long m, V3 bg,
                                                                double *__restrict__ out) {
  const long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (r >= m) return;
  const int slot = lit_slot(a, slots, shape[r]);
  V3 res = bg;
  if (slot >= 0) {
    // (every plane of the record is requested here, in front of the arithmetic: one round trip to memory)
    const double u = uv[r], v = uv[m + r];
    const V3 wp = {point[r], point[m + r], point[2 * m + r]};
    const V3 nrm = {normal[r], normal[m + r], normal[2 * m + r]};
    const V3 in = {dir[r], dir[m + r], dir[2 * m + r]};
    const PtShapeAux *ax = a.aux + slot;
    const V3 pc = lit_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, u, v);
    const V3 em = lit_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, u, v);
    const bool diffuse = ax->brdf_kind == PT_BRDF_DIFFUSE;
    const V3 nn = normalize3(nrm);
    V3 d = nn;
    if (!diffuse) {  // materials.py:186-192 as scatter_ray (pt_shade.h) forms it
      const V3 rd = normalize3(in);
      const double dp = dot3(nn, rd);
      d.x = rd.x - dp * (2.0 * nn.x);
      d.y = rd.y - dp * (2.0 * nn.y);
      d.z = rd.z - dp * (2.0 * nn.z);
    }
    V3 e = {0.0, 0.0, 0.0};
    if (!lit_is_nan(wp)) e = lit_blend_eval(coeffs, K.n, lit_cell(K, wp), d, diffuse ? PT_LIT_HEMISPHERE : PT_LIT_RADIANCE);
    res.x = em.x + pc.x * e.x;
    res.y = em.y + pc.y * e.y;
    res.z = em.z + pc.z * e.z;
  }
  out[r] = res.x;
  out[m + r] = res.y;
  out[2 * m + r] = res.z;
}
