// pt_scene_build.h — what pt_scene_upload computes on the HOST before anything is uploaded: the records in slot order, the
// culling bounds, the ball hierarchy, the uniform grid.  A pure host function: no HIP call, no handle, no global but the
// PtTuning passed in.
//
//   pt_build_scene(description, tuning) -> PtSceneHost          ptrace.hip: pt_scene_upload = build + upload
//
// pt_debug_plan runs it for a scene DESCRIPTION on any machine, and tests/scene_build/scene_digest.cpp is a program of its
// own over it: every conservative margin the culling and the grid walk rely on is in this file, and
// tests/test_scene_build.py pins every table and scalar it produces, bit for bit, on a CPU (also under the host sanitizers).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/ptrace.h"
#include "pt_layout.h"
#include "pt_plan.h"

// every scalar of the analysis: what the kernels' argument block and the plan read beside the tables
struct PtSceneScalars {
  int n_shapes = 0, n_spheres = 0, n_diag = 0, n_lights = 0, n_textures = 0;
  int bs_stride = 0, gs_stride = 0, cs_stride = 0, bs_levels = 0;
  float bs_rmax[3] = {0.0f, 0.0f, 0.0f};
  int grid_n_always = 0, grid_n_cells = 0, grid_res[3] = {0, 0, 0};
  float grid_far_eo = INFINITY;  // rays with 1e-6 * max|origin component| above this do not walk the grid (see world_query_lanes)
  float grid_min[3] = {0, 0, 0}, grid_max[3] = {0, 0, 0}, grid_cell[3] = {0, 0, 0}, grid_inv[3] = {0, 0, 0};
};

struct PtDomeCand {
  int slot;
  double invm[12];
};

struct PtSceneHost {
  PtSceneScalars sc;
  std::vector<PtShapeRec> recs;
  std::vector<PtShapeAux> aux;
  std::vector<PtFlatPal> flat_pal;  // [n_shapes]; the upload pads it to whole chunks behind aux[] (pt_layout.h)
  std::vector<PtDiagRec> diag;
  std::vector<float4> bounds;
  std::vector<float> bsoa;
  std::vector<PtLight> lights;
  std::vector<PtTex> tex;
  std::vector<double> tex_data;
  bool has_grid = false;
  std::vector<unsigned> grid_cells, grid_occ;
  std::vector<unsigned short> grid_slots;
  std::vector<float4> grid_balls;
  std::vector<int> grid_always;
  std::vector<PtDomeCand> dome_cands;  // spheres that may serve as "the dome" of a view: uniform pigments, sane scale
};

static inline PtSceneFacts pt_scene_facts(const PtSceneScalars &s, int n_cu, bool dome_shortcut) {
  PtSceneFacts f;
  f.n_shapes = s.n_shapes;
  f.n_spheres = s.n_spheres;
  f.n_diag = s.n_diag;
  f.n_lights = s.n_lights;
  f.bs_levels = s.bs_levels;
  f.has_grid = s.grid_n_cells > 0 ? 1 : 0;
  f.grid_n_cells = s.grid_n_cells;
  f.n_cu = n_cu;
  f.dome_shortcut = dome_shortcut ? 1 : 0;
  return f;
}

static inline int pt_desc_error(char *msg, size_t cap, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, cap, fmt, ap);
  va_end(ap);
  return PT_ERR_INVALID;
}

// PT_OK, or PT_ERR_INVALID with the reason in msg[cap]
static inline int pt_check_desc(const pt_scene_desc *d, char *msg, size_t cap) {
  if (!d) return pt_desc_error(msg, cap, "null scene descriptor");
  if (d->n_shapes < 0 || d->n_lights < 0 || d->n_textures < 0)
    return pt_desc_error(msg, cap, "negative count in scene descriptor");
  if (d->n_shapes > 0 &&
      (!d->kind || !d->invm || !d->m || !d->brdf_kind || !d->brdf_param || !d->pig_kind ||
       !d->pig_c1 || !d->pig_c2 || !d->pig_steps || !d->pig_tex || !d->emi_kind || !d->emi_c1 ||
       !d->emi_c2 || !d->emi_steps || !d->emi_tex))
    return pt_desc_error(msg, cap, "null array in scene descriptor");
  if (d->n_lights > 0 && (!d->light_pos || !d->light_color || !d->light_radius))
    return pt_desc_error(msg, cap, "null light array in scene descriptor");
  if (d->n_textures > 0 && (!d->tex_w || !d->tex_h || !d->tex_offset || !d->tex_data))
    return pt_desc_error(msg, cap, "null texture array in scene descriptor");
  for (int i = 0; i < d->n_shapes; ++i) {
    if (d->kind[i] != PT_SHAPE_SPHERE && d->kind[i] != PT_SHAPE_PLANE)
      return pt_desc_error(msg, cap, "shape %d: unknown kind %d", i, d->kind[i]);
    if (d->brdf_kind[i] != PT_BRDF_DIFFUSE && d->brdf_kind[i] != PT_BRDF_SPECULAR)
      return pt_desc_error(msg, cap, "shape %d: unknown BRDF kind %d", i, d->brdf_kind[i]);
    const int pk[2] = {d->pig_kind[i], d->emi_kind[i]};
    const int pt[2] = {d->pig_tex[i], d->emi_tex[i]};
    for (int k = 0; k < 2; ++k) {
      if (pk[k] < PT_PIGMENT_UNIFORM || pk[k] > PT_PIGMENT_IMAGE)
        return pt_desc_error(msg, cap, "shape %d: unknown pigment kind %d", i, pk[k]);
      if (pk[k] == PT_PIGMENT_IMAGE && (pt[k] < 0 || pt[k] >= d->n_textures))
        return pt_desc_error(msg, cap, "shape %d: texture index %d out of range", i, pt[k]);
    }
  }
  for (int t = 0; t < d->n_textures; ++t)
    if (d->tex_w[t] <= 0 || d->tex_h[t] <= 0 || d->tex_offset[t] < 0)
      return pt_desc_error(msg, cap, "texture %d: bad size/offset", t);
  return PT_OK;
}

// A ball of the scattered-ray filter as the kernels want it: r'^2 / (1 - 8e-6) rounded up; where there is no usable bound
// (r' not finite or >= 1e17, a centre that is not finite or beyond 1e17) the centre 0 and r'^2 = 1e38, which the filter's
// arithmetic never rejects and never overflows on (pt_query.h: world_query_lanes).
static inline void pt_ball_square(float *x, float *y, float *z, float *r, bool *ordinary) {
  const bool ok = std::isfinite(*r) && *r >= 0.0f && *r < 1e17f && std::isfinite(*x) && std::isfinite(*y) && std::isfinite(*z) &&
                  std::fabs(*x) < 1e17f && std::fabs(*y) < 1e17f && std::fabs(*z) < 1e17f;
  *ordinary = ok;
  if (ok) {
    *r = std::nextafter((float)((double)*r * (double)*r * (1.0 + 8.1e-6)), INFINITY);
  } else {
    *x = *y = *z = 0.0f;
    *r = 1e38f;
  }
}

// slot -> World.shapes index; sets n_diag, n_spheres and bs_levels
static inline std::vector<int> pt_slot_order(const pt_scene_desc *d, PtSceneScalars &s) {
  const int n = d->n_shapes;
  // group the records: scale+translate spheres, other spheres, planes — each group in World.shapes order
  auto is_diag = [&](int i) {
    if (d->kind[i] != PT_SHAPE_SPHERE) return false;
    const int off[6] = {1, 2, 4, 6, 8, 9};
    for (int k : off)
      if (d->invm[(size_t)k * n + i] != 0.0) return false;
    const int dia[3] = {0, 5, 10};
    for (int k : dia) {
      const double v = std::fabs(d->invm[(size_t)k * n + i]);
      if (!(v >= 1e-100 && v <= 1e100)) return false;
    }
    for (int k : {3, 7, 11})
      if (!std::isfinite(d->invm[(size_t)k * n + i])) return false;
    return true;
  };
  std::vector<int> order;
  order.reserve(n);
  for (int i = 0; i < n; ++i)
    if (is_diag(i)) order.push_back(i);
  s.n_diag = (int)order.size();
  for (int i = 0; i < n; ++i)
    if (d->kind[i] == PT_SHAPE_SPHERE && !is_diag(i)) order.push_back(i);
  s.n_spheres = (int)order.size();
  for (int i = 0; i < n; ++i)
    if (d->kind[i] != PT_SHAPE_SPHERE) order.push_back(i);
  // Large scenes: within each sphere group the slots follow a Morton curve through the centres (the few
  // spheres much larger than the rest first), so that 8 and 64 consecutive slots are close in space and
  // a ball around them is tight (per-ray prefilter of scattered and shadow rays, world_query_lanes).
  // Any slot order gives the same image: ties in t go to the lower World.shapes index (r.index).
  s.bs_levels = s.n_spheres >= 128 ? 1 : 0;
  if (s.bs_levels) {
    auto centre = [&](int i, int k) { return d->m[(size_t)(3 + 4 * k) * n + i]; };
    auto radius2 = [&](int i) {  // squared Frobenius norm of M's 3x3 block: a size, not a bound
      double v = 0.0;
      for (int r_ = 0; r_ < 3; ++r_)
        for (int c_ = 0; c_ < 3; ++c_) v += d->m[(size_t)(r_ * 4 + c_) * n + i] * d->m[(size_t)(r_ * 4 + c_) * n + i];
      return v;
    };
    std::vector<double> sizes;
    for (int k = 0; k < s.n_spheres; ++k) sizes.push_back(radius2(order[k]));
    std::vector<double> sorted_sizes = sizes;
    std::nth_element(sorted_sizes.begin(), sorted_sizes.begin() + sorted_sizes.size() / 2, sorted_sizes.end());
    const double big = 64.0 * sorted_sizes[sorted_sizes.size() / 2];  // 8x the median radius
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < s.n_spheres; ++k) {
      if (!(sizes[k] <= big)) continue;
      for (int c_ = 0; c_ < 3; ++c_) {
        const double v = centre(order[k], c_);
        if (std::isfinite(v)) {
          lo[c_] = std::min(lo[c_], v);
          hi[c_] = std::max(hi[c_], v);
        }
      }
    }
    auto morton = [&](int i) {
      uint64_t code = 0;
      uint32_t q[3];
      for (int c_ = 0; c_ < 3; ++c_) {
        const double v = centre(i, c_), span = hi[c_] - lo[c_];
        double u = (span > 0.0 && std::isfinite(v)) ? (v - lo[c_]) / span : 0.0;
        u = std::min(1.0, std::max(0.0, u));
        q[c_] = (uint32_t)(u * 2097151.0);  // 21 bits
      }
      for (int b = 20; b >= 0; --b)
        for (int c_ = 0; c_ < 3; ++c_) code = (code << 1) | ((q[c_] >> b) & 1u);
      return code;
    };
    auto sort_range = [&](int a0, int a1) {
      std::vector<std::pair<std::pair<int, uint64_t>, int>> keyed;  // ((small?, code), shape)
      for (int k = a0; k < a1; ++k) {
        const bool small_ = sizes[k] <= big;
        // large spheres first, largest leading; then the Morton order of the rest
        const uint64_t code = small_ ? morton(order[k]) : (uint64_t)(k - a0);
        keyed.push_back({{small_ ? 1 : 0, code}, order[k]});
      }
      std::stable_sort(keyed.begin(), keyed.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
      for (int k = a0; k < a1; ++k) order[k] = keyed[k - a0].second;
    };
    sort_range(0, s.n_diag);
    sort_range(s.n_diag, s.n_spheres);
  }
  return order;
}

static inline void pt_pack_records(const pt_scene_desc *d, const std::vector<int> &order, PtSceneHost &h) {
  const PtSceneScalars &s = h.sc;
  const int n = d->n_shapes;
  std::vector<PtShapeRec> recs(n);
  std::vector<PtShapeAux> aux(n);
  for (int slot = 0; slot < n; ++slot) {
    const int i = order[slot];
    PtShapeRec &r = recs[slot];
    PtShapeAux &x = aux[slot];
    memset(&r, 0, sizeof r);
    memset(&x, 0, sizeof x);
    for (int k = 0; k < 12; ++k) {
      r.invm[k] = d->invm[(size_t)k * n + i];
      x.m[k] = d->m[(size_t)k * n + i];
    }
    r.kind = d->kind[i];
    for (int k = 0; k < 3; ++k) {
      x.pig_c1[k] = d->pig_c1[(size_t)k * n + i];
      x.pig_c2[k] = d->pig_c2[(size_t)k * n + i];
      x.emi_c1[k] = d->emi_c1[(size_t)k * n + i];
      x.emi_c2[k] = d->emi_c2[(size_t)k * n + i];
    }
    x.pig_steps = d->pig_steps[i];
    x.emi_steps = d->emi_steps[i];
    x.brdf_param = d->brdf_param[i];
    x.brdf_kind = d->brdf_kind[i];
    x.pig_kind = d->pig_kind[i];
    x.emi_kind = d->emi_kind[i];
    x.pig_tex = d->pig_tex[i];
    x.emi_tex = d->emi_tex[i];
    x.needs_uv = (d->pig_kind[i] != PT_PIGMENT_UNIFORM || d->emi_kind[i] != PT_PIGMENT_UNIFORM) ? 1 : 0;
    // both pigments uniform: color2 of the (uniform) BRDF pigment is never read, and the slot carries what FlatRenderer
    // returns for the shape, pigment + emitted (render.py:65-74; the same fp64 addition the kernel would do per pixel)
    if (!x.needs_uv)
      for (int k = 0; k < 3; ++k) x.pig_c2[k] = x.pig_c1[k] + x.emi_c1[k];
    r.index = i;
    // |invm|_F^2 for the "camera inside this sphere" shortcut of the tile kernel; +inf disables it unless
    // every singular value of invm's 3x3 block is within 1e-6 .. 1e6 (Gershgorin bounds of invm^T invm)
    r.fro2 = INFINITY;
    if (r.kind == PT_SHAPE_SPHERE) {
      double A[3][3], fro2 = 0.0;
      for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
          A[p][q] = 0.0;
          for (int k = 0; k < 3; ++k) A[p][q] += r.invm[k * 4 + p] * r.invm[k * 4 + q];
        }
      double lmin = INFINITY, lmax = 0.0;
      for (int p = 0; p < 3; ++p) {
        double off = 0.0;
        for (int q = 0; q < 3; ++q)
          if (q != p) off += std::fabs(A[p][q]);
        lmin = std::min(lmin, A[p][p] - off);
        lmax = std::max(lmax, A[p][p] + off);
        fro2 += A[p][p];
      }
      if (std::isfinite(fro2) && lmin >= 1e-12 && lmax <= 1e12) r.fro2 = fro2 * (1.0 + 1e-9);
    }
  }
  std::vector<PtLight> lights(d->n_lights);
  for (int l = 0; l < d->n_lights; ++l) {
    memset(&lights[l], 0, sizeof(PtLight));
    for (int k = 0; k < 3; ++k) {
      lights[l].pos[k] = d->light_pos[(size_t)k * d->n_lights + l];
      lights[l].color[k] = d->light_color[(size_t)k * d->n_lights + l];
    }
    lights[l].radius = d->light_radius[l];
  }
  std::vector<PtTex> tex(d->n_textures);
  size_t tex_doubles = 0;
  for (int t = 0; t < d->n_textures; ++t) {
    tex[t].w = d->tex_w[t];
    tex[t].h = d->tex_h[t];
    tex[t].offset = d->tex_offset[t];
    tex_doubles = std::max(tex_doubles, (size_t)d->tex_offset[t] + (size_t)d->tex_w[t] * d->tex_h[t] * 3);
  }
  std::vector<double> tex_data(d->tex_data, d->tex_data + tex_doubles);

  std::vector<PtDiagRec> diag(s.n_diag);
  for (int slot = 0; slot < s.n_diag; ++slot) {
    PtDiagRec &g = diag[slot];
    memset(&g, 0, sizeof g);
    const double *im = recs[slot].invm;
    g.s[0] = im[0];
    g.s[1] = im[5];
    g.s[2] = im[10];
    g.t[0] = im[3];
    g.t[1] = im[7];
    g.t[2] = im[11];
    g.tnz = (im[3] != 0.0 ? 1 : 0) | (im[7] != 0.0 ? 2 : 0) | (im[11] != 0.0 ? 4 : 0);
  }
  h.recs = recs;
  h.diag = diag;
  h.aux = aux;
  h.lights = lights;
  h.tex = tex;
  h.tex_data = tex_data;
}

// the Flat palette (pt_layout.h: PtFlatPal), from the packed aux[]: pt_pack_records has already put pigment + emitted into
// pig_c2 of every shape with two uniform pigments
static inline void pt_flat_palette(PtSceneHost &h) {
  std::vector<PtFlatPal> pal(h.aux.size());
  for (size_t slot = 0; slot < pal.size(); ++slot) {
    PtFlatPal &e = pal[slot];
    memset(&e, 0, sizeof e);
    e.needs_uv = h.aux[slot].needs_uv;
    if (!e.needs_uv)
      for (int k = 0; k < 3; ++k) e.c[k] = h.aux[slot].pig_c2[k];
  }
  h.flat_pal = pal;
}

// what the upload puts into ONE allocation: aux[], and directly behind it the palette in whole zero-filled chunks
// (pt_flat_pal_chunks: a wave of pt_tile4_kernel<FLAT, LDS> reads every chunk to its end)
static inline std::vector<unsigned char> pt_aux_image(const PtSceneHost &h) {
  const size_t n = h.aux.size(), aux_bytes = n * sizeof(PtShapeAux);
  std::vector<unsigned char> img(aux_bytes + (size_t)pt_flat_pal_chunks((int)n) * PT_FLAT_PAL_CHUNK, 0);
  if (n) {
    memcpy(img.data(), h.aux.data(), aux_bytes);
    memcpy(img.data() + aux_bytes, h.flat_pal.data(), n * sizeof(PtFlatPal));
  }
  return img;
}

static inline void pt_cull_bounds(PtSceneHost &h) {
  const std::vector<PtShapeRec> &recs = h.recs;
  const std::vector<PtShapeAux> &aux = h.aux;
  const int n = h.sc.n_shapes;
  // bounding spheres for tile culling: radius = a rigorous upper bound of the spectral norm of M's 3x3 block
  struct Bound64 {
    double cx, cy, cz, r;
  };
  std::vector<float4> bounds(n);
  for (int slot = 0; slot < n; ++slot) {
    Bound64 b;
    const double *m = aux[slot].m;
    b.cx = m[3];
    b.cy = m[7];
    b.cz = m[11];
    b.r = -1.0;
    if (recs[slot].kind == PT_SHAPE_SPHERE) {
      double A[3][3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          A[i][j] = 0.0;
          for (int k = 0; k < 3; ++k) A[i][j] += m[k * 4 + i] * m[k * 4 + j];
        }
      // Gershgorin: lambda_max(M^T M) <= max_i sum_j |(M^T M)_ij|  (exact for scale/rotation blocks)
      double lam = 0.0;
      for (int i = 0; i < 3; ++i)
        lam = std::max(lam, std::fabs(A[i][0]) + std::fabs(A[i][1]) + std::fabs(A[i][2]));
      // The exact test uses invm, the bound uses m: check that m really inverts invm (the reference
      // stores both, transformations.py:48-56) and widen the radius by the residual; else never cull.
      const double *im = recs[slot].invm;
      double resid = 0.0;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
          double e = (i == j) ? -1.0 : 0.0;
          for (int k = 0; k < 3; ++k) e += im[i * 4 + k] * m[k * 4 + j];
          resid = std::max(resid, std::fabs(e));
        }
        double e = im[i * 4 + 3];
        for (int k = 0; k < 3; ++k) e += im[i * 4 + k] * m[k * 4 + 3];
        resid = std::max(resid, std::fabs(e));
      }
      const double r = std::sqrt(lam) * (1.0 + 1e-9 + 16.0 * resid);
      const bool finite = std::isfinite(r) && std::isfinite(b.cx) && std::isfinite(b.cy) &&
                          std::isfinite(b.cz) && resid < 1e-6;
      b.r = finite ? r : -1.0;
    }
    // to fp32: widen r by the rounding of the centre (<= 2^-24 relative per component) and of r itself
    float4 f;
    f.x = (float)b.cx;
    f.y = (float)b.cy;
    f.z = (float)b.cz;
    const double cabs = std::max(std::fabs(b.cx), std::max(std::fabs(b.cy), std::fabs(b.cz)));
    const double rw = b.r * (1.0 + 1e-6) + 2e-7 * cabs;
    f.w = (b.r >= 0.0 && std::isfinite(rw) && rw < 1e37 && cabs < 1e37) ? (float)rw * (1.0f + 1e-6f) : -1.0f;
    if (recs[slot].kind == PT_SHAPE_PLANE) {
      // planes have no bounding sphere; their slot carries what plane_keeps() needs instead: the z row of
      // invm (object-space d.z = row . d, o.z = row . o + invm[11]) rounded to fp32
      const double *im = recs[slot].invm;
      f.x = (float)im[8];
      f.y = (float)im[9];
      f.z = (float)im[10];
      f.w = (float)im[11];
    }
    bounds[slot] = f;
  }
  h.bounds = bounds;
}

static inline void pt_ball_tables(PtSceneHost &h) {
  PtSceneScalars &s = h.sc;
  const std::vector<float4> &bounds = h.bounds;
  const int n = s.n_shapes;
  // ... and as structure-of-arrays for the per-ray prefilter of scattered rays (world_query_lanes): two
  // neighbouring spheres per packed fp32 instruction.  r' = r*(1 + 1e-5) + 1e-6*max|c| rounded up;
  // +inf where there is no bound (the test then always keeps the shape).
  s.bs_stride = (n + 8 + 7) / 8 * 8;  // 8 floats of slack: the prefilter reads eight at a time, 32-byte aligned
  const int n_groups = (s.n_spheres + 7) / 8, n_chunks = (s.n_spheres + 63) / 64;
  s.gs_stride = (n_chunks * 8 + 8 + 7) / 8 * 8;  // eight groups per chunk, read eight at a time
  s.cs_stride = (n_chunks + 8 + 7) / 8 * 8;
  std::vector<float> bsoa((size_t)4 * (s.bs_stride + s.gs_stride + s.cs_stride), 0.0f);
  for (int slot = 0; slot < s.bs_stride; ++slot) {
    float rk = INFINITY;
    if (slot < n) {
      const float4 f = bounds[slot];
      bsoa[slot] = f.x;
      bsoa[(size_t)s.bs_stride + slot] = f.y;
      bsoa[(size_t)2 * s.bs_stride + slot] = f.z;
      if (slot < s.n_spheres && f.w >= 0.0f) {
        const double cabs = std::max(std::fabs((double)f.x), std::max(std::fabs((double)f.y), std::fabs((double)f.z)));
        const double v = (double)f.w * (1.0 + 1e-5) + 1e-6 * cabs;
        rk = std::nextafter((float)v, INFINITY);
      }
    }
    bsoa[(size_t)3 * s.bs_stride + slot] = rk;
  }
  // a ball around the (already inflated) balls of slots [a0, a1): centre = middle of the centres' box,
  // radius = max_i(|c_i - centre| + r'_i), rounded up; +inf as soon as one member has no bound
  auto ball_around = [&](int a0, int a1, float *out4) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bounded = a1 > a0;
    for (int k = a0; k < a1; ++k) {
      bounded = bounded && std::isfinite(bsoa[(size_t)3 * s.bs_stride + k]);
      for (int c_ = 0; c_ < 3; ++c_) {
        const double v = bsoa[(size_t)c_ * s.bs_stride + k];
        lo[c_] = std::min(lo[c_], v);
        hi[c_] = std::max(hi[c_], v);
      }
    }
    out4[0] = out4[1] = out4[2] = 0.0f;
    out4[3] = INFINITY;
    if (!bounded) return;
    float c[3];
    for (int c_ = 0; c_ < 3; ++c_) c[c_] = (float)(0.5 * (lo[c_] + hi[c_]));
    double rad = 0.0;
    for (int k = a0; k < a1; ++k) {
      double d2 = 0.0;
      for (int c_ = 0; c_ < 3; ++c_) {
        const double dv = (double)bsoa[(size_t)c_ * s.bs_stride + k] - (double)c[c_];
        d2 += dv * dv;
      }
      rad = std::max(rad, std::sqrt(d2) * (1.0 + 1e-12) + (double)bsoa[(size_t)3 * s.bs_stride + k]);
    }
    const double cabs = std::max(std::fabs((double)c[0]), std::max(std::fabs((double)c[1]), std::fabs((double)c[2])));
    const double v = rad * (1.0 + 1e-5) + 1e-6 * cabs;
    if (!std::isfinite(v) || v > 1e37) return;
    out4[0] = c[0];
    out4[1] = c[1];
    out4[2] = c[2];
    out4[3] = std::nextafter((float)v, INFINITY);
  };
  {
    float *gs = bsoa.data() + (size_t)4 * s.bs_stride, *cs = gs + (size_t)4 * s.gs_stride;
    for (int k = 0; k < s.gs_stride; ++k) {
      float b4[4] = {0.0f, 0.0f, 0.0f, INFINITY};
      if (k < n_groups) ball_around(k * 8, std::min(k * 8 + 8, s.n_spheres), b4);
      for (int c_ = 0; c_ < 4; ++c_) gs[(size_t)c_ * s.gs_stride + k] = b4[c_];
    }
    for (int k = 0; k < s.cs_stride; ++k) {
      float b4[4] = {0.0f, 0.0f, 0.0f, INFINITY};
      if (k < n_chunks) ball_around(k * 64, std::min(k * 64 + 64, s.n_spheres), b4);
      for (int c_ = 0; c_ < 4; ++c_) cs[(size_t)c_ * s.cs_stride + k] = b4[c_];
    }
  }
  h.bsoa = bsoa;
}

static inline void pt_build_grid(const PtTuning &tn, PtSceneHost &h) {
  PtSceneScalars &s = h.sc;
  const std::vector<float> &bsoa = h.bsoa;
  // ---- uniform grid over the ordinary spheres (scenes of >= 128 spheres) ----
  // A sphere is entered into every cell that the box around its ball (the r' of the per-ray prefilter, already
  // inflated) overlaps after widening it by eps = 2e-3 cell + 1e-4 max|coordinate|.  The walk (world_query_lanes)
  // runs a 3D-DDA in fp32 on the fp32 copy of the ray: that copy stays within ~1e-7 |coordinate| x a few of the
  // true ray, and the accumulated rounding of the DDA's crossing parameters (<= 200 steps x 2^-24) can make it
  // enter a face or skip a corner cell up to ~1.2e-5 x the grid's extent early or late; eps (>= 3e-5 extent, since
  // a cell is >= 1/64 of it) covers both, so a point where the true ray meets a sphere always lies within eps of a
  // visited cell, i.e. in a cell the sphere is entered in.  Spheres much larger than the rest (8x the median
  // radius: a dome would be in every cell) or without a bound go to the "always" list.
  if (tn.grid && s.bs_levels && s.n_spheres <= 65535) {
    auto ball = [&](int k, int q) { return bsoa[(size_t)q * s.bs_stride + k]; };  // q: 0..2 centre, 3 radius r'
    std::vector<float> radii;
    for (int k = 0; k < s.n_spheres; ++k)
      if (std::isfinite(ball(k, 3))) radii.push_back(ball(k, 3));
    std::vector<int> always, inside;
    float big = INFINITY;
    if (!radii.empty()) {
      std::nth_element(radii.begin(), radii.begin() + radii.size() / 2, radii.end());
      big = 8.0f * radii[radii.size() / 2];
    }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, cmax = 0.0;
    for (int k = 0; k < s.n_spheres; ++k) {
      const float r = ball(k, 3);
      if (!std::isfinite(r) || r > big) {
        always.push_back(k);
        continue;
      }
      inside.push_back(k);
      for (int q = 0; q < 3; ++q) {
        lo[q] = std::min(lo[q], (double)ball(k, q) - r);
        hi[q] = std::max(hi[q], (double)ball(k, q) + r);
      }
    }
    // (below ~1000 spheres the exhaustive packed prefilter and the cell walk cost the same -- measured on C4's 256 --
    //  and the prefilter has the sparse path for the deep stragglers; the grid wins 2.5-3.3x at 10 000)
    if ((int)inside.size() >= std::max(64, (int)tn.grid_min)) {
      double ext[3], vol = 1.0;
      for (int q = 0; q < 3; ++q) {
        const double pad = 1e-3 * (hi[q] - lo[q]) + 1e-4 * (1.0 + std::max(std::fabs(lo[q]), std::fabs(hi[q])));
        lo[q] -= pad;
        hi[q] += pad;
        ext[q] = hi[q] - lo[q];
        vol *= ext[q];
        cmax = std::max(cmax, std::max(std::fabs(lo[q]), std::fabs(hi[q])));
      }
      const double target = std::min<double>(32768.0, std::max<double>(64.0, tn.grid_density * (double)inside.size()));  // (cells per sphere)
      const double side = std::cbrt(vol / target);
      long long ncell = 1;
      for (int q = 0; q < 3; ++q) {
        s.grid_res[q] = (int)std::min(64.0, std::max(1.0, std::ceil(ext[q] / side)));
        s.grid_min[q] = (float)lo[q];
        s.grid_max[q] = (float)hi[q];
        s.grid_cell[q] = (float)(ext[q] / s.grid_res[q]);
        s.grid_inv[q] = (float)(s.grid_res[q] / ext[q]);
        ncell *= s.grid_res[q];
      }
      std::vector<std::vector<unsigned short>> cells((size_t)ncell);
      size_t items = 0;
      bool ok = std::isfinite(vol) && vol > 0.0 && ncell <= 65535;  // (cell ids travel in 16 bits)
      for (int k : inside) {
        if (!ok) break;
        int c0[3], c1[3];
        for (int q = 0; q < 3; ++q) {
          const double eps = 2e-3 * s.grid_cell[q] + 1e-4 * cmax, c = ball(k, q), r = ball(k, 3);
          c0[q] = std::max(0, std::min(s.grid_res[q] - 1, (int)std::floor((c - r - eps - lo[q]) * s.grid_res[q] / ext[q])));
          c1[q] = std::max(0, std::min(s.grid_res[q] - 1, (int)std::floor((c + r + eps - lo[q]) * s.grid_res[q] / ext[q])));
        }
        for (int z = c0[2]; z <= c1[2]; ++z)
          for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
              auto &cell = cells[((size_t)z * s.grid_res[1] + y) * s.grid_res[0] + x];
              cell.push_back((unsigned short)k);
              ++items;
              ok = ok && cell.size() <= 255 && items <= ((size_t)1 << 23);
            }
      }
      if (ok) {
        std::vector<unsigned> words((size_t)ncell), occ((size_t)(ncell + 31) / 32 + 1, 0u);
        std::vector<unsigned short> slots;
        std::vector<float4> balls;
        for (size_t cidx = 0; cidx < (size_t)ncell; ++cidx) {
          words[cidx] = ((unsigned)slots.size() << 8) | (unsigned)cells[cidx].size();
          if (!cells[cidx].empty()) occ[cidx >> 5] |= 1u << (cidx & 31);
          for (unsigned short k : cells[cidx]) {
            slots.push_back(k);
            float4 b;
            b.x = ball(k, 0);
            b.y = ball(k, 1);
            b.z = ball(k, 2);
            b.w = ball(k, 3);
            bool ordinary;
            pt_ball_square(&b.x, &b.y, &b.z, &b.w, &ordinary);
            balls.push_back(b);
          }
        }
        h.grid_cells = words;
        h.grid_occ = occ;
        h.grid_slots = slots;
        h.grid_balls = balls;
        h.grid_always = always;
        h.has_grid = true;
        s.grid_n_always = (int)always.size();
        // the margin a sphere is entered with, >= 1e-4 * cmax, covers the fp32 copy of a ray whose origin lies within
        // ~100 x the grid's coordinates (1.2e-7 |o| <= a quarter of the margin); a ray from farther away takes the
        // exhaustive filter instead of the walk
        s.grid_far_eo = (float)(1e-4 * cmax);
        s.grid_n_cells = (int)ncell;
      }
    }
  }
}

static inline void pt_square_radii(PtSceneHost &h) {
  PtSceneScalars &s = h.sc;
  std::vector<float> &bsoa = h.bsoa;
  // the filter compares squares (world_query_lanes): r' -> r'^2 rounded up, in all three tables
  {
    float *tab[3] = {bsoa.data(), bsoa.data() + (size_t)4 * s.bs_stride, bsoa.data() + (size_t)4 * (s.bs_stride + s.gs_stride)};
    const int stride[3] = {s.bs_stride, s.gs_stride, s.cs_stride};
    for (int lv = 0; lv < 3; ++lv) {
      float rmax = 0.0f;
      for (int k = 0; k < stride[lv]; ++k) {
        float *x = tab[lv] + k, *y = x + stride[lv], *z = y + stride[lv], *r = z + stride[lv];
        const float rp = *r;
        bool ordinary;
        pt_ball_square(x, y, z, r, &ordinary);
        if (ordinary) rmax = std::max(rmax, rp);
      }
      s.bs_rmax[lv] = rmax;
    }
  }
}

static inline void pt_dome_candidates(PtSceneHost &h) {
  const PtSceneScalars &s = h.sc;
  const std::vector<PtShapeRec> &recs = h.recs;
  const std::vector<PtShapeAux> &aux = h.aux;
  for (int slot = 0; slot < s.n_spheres; ++slot)
    if (aux[slot].needs_uv == 0 && std::isfinite(recs[slot].fro2)) {
      PtDomeCand dc;
      dc.slot = slot;
      memcpy(dc.invm, recs[slot].invm, sizeof dc.invm);
      h.dome_cands.push_back(dc);
    }
}

// `h`: a fresh PtSceneHost; `d` has passed pt_check_desc
static inline void pt_build_scene(const pt_scene_desc *d, const PtTuning &tn, PtSceneHost &h) {
  h.sc.n_shapes = d->n_shapes;
  h.sc.n_lights = d->n_lights;
  h.sc.n_textures = d->n_textures;
  pt_pack_records(d, pt_slot_order(d, h.sc), h);
  pt_flat_palette(h);
  pt_cull_bounds(h);
  pt_ball_tables(h);
  pt_build_grid(tn, h);
  pt_square_radii(h);  // (after the grid: its cells are cut from the unsquared r')
  pt_dome_candidates(h);
}
