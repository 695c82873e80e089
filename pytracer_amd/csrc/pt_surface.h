// pt_surface.h -- materials and point-light shading for a CALLER's hit records (include/ptrace_surface.h).
// Included by ptrace_surface.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h, pt_shade.h): nothing here is
// part of libptrace.so or libptrace_rays.so.
//
// What it restates: the pigment look-up of materials.py:50-100 and PointLightRenderer.__call__ (render.py:157-193) exactly as
// pt_simple.h's pointlight_shade has them -- the same operations in the same order -- for records that arrive in planes
// instead of coming out of hit_details.  What is new is what a caller's record needs and the library's own never did: a
// shape index may be anything, (u, v) may be anything, a shadow ray's tmin may be NaN.
#pragma once

// materials.py:70-82 for a (u, v) nobody vouches for.  pigment_color (pt_shade.h) clamps column and row from above only, which
// is all hit_details' (u, v) in [0, 1] need; a caller's may be negative, huge or NaN, so the clamp is made on the product
// while it is still a double: not >= 0 (negative, NaN) -> 0, >= w -> w - 1, else the truncation the reference's int() makes.
// For (u, v) in [0, 1) the texel is pigment_color's.
PT_DEV long long surf_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}

template <typename CP>
PT_DEV V3 surf_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = surf_texel(u, w), row = surf_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}
PT_DEV V3 surf_brdf_pigment(const PtKArgs &a, const PtShapeAux *ax, double u, double v) {
  return surf_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, u, v);
}
PT_DEV V3 surf_emitted_pigment(const PtKArgs &a, const PtShapeAux *ax, double u, double v) {
  return surf_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, u, v);
}

// World.shapes index -> grouped slot, or -1: an index outside [0, n_shapes) is "no hit", and so is a table entry that does
// not name a record (the table is the caller's memory).
PT_DEV int surf_slot(const PtKArgs &a, const int *__restrict__ slots, int index) {
  if ((unsigned)index >= (unsigned)a.n_shapes) return -1;
  const int s = slots[index];
  return ((unsigned)s < (unsigned)a.n_shapes) ? s : -1;
}

// slots[recs[s].index] = s: `index` is a permutation of 0 .. n_shapes - 1 (pt_scene_build.h), every entry is written once.
__global__ __launch_bounds__(PT_BLOCK) void pt_slots_kernel(const PtKArgs a, int *__restrict__ slots) {
  const int s = blockIdx.x * PT_BLOCK + threadIdx.x;
  if (s >= a.n_shapes) return;
  const int index = a.recs[s].index;
  if ((unsigned)index < (unsigned)a.n_shapes) slots[index] = s;
}

// One record per lane; a plane is read and written 8 bytes per lane, 512 consecutive bytes per wave (the int32 planes: 256).
// `channels` is wave-uniform: a colour that is not selected costs neither its pigment nor its stores, and without a colour
// uv is not read (it may be null).
__global__ __launch_bounds__(PT_BLOCK) void pt_surface_kernel(const PtKArgs a, const int *__restrict__ slots, const int *__restrict__ shape,
                                                              const double *__restrict__ uv, long long n, int channels,
                                                              void *__restrict__ out) {
  const long long i = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int slot = surf_slot(a, slots, shape[i]);
  int kind = -1;
  V3 pc = {0.0, 0.0, 0.0}, em = {0.0, 0.0, 0.0};
  if (slot >= 0) {
    const PtShapeAux *ax = a.aux + slot;
    kind = ax->brdf_kind;
    if (channels != 0) {
      const double u = uv[i], v = uv[n + i];
      if (channels & PT_SURF_BRDF_COLOR) pc = surf_brdf_pigment(a, ax, u, v);
      if (channels & PT_SURF_EMITTED) em = surf_emitted_pigment(a, ax, u, v);
    }
  }
  ((int *)out)[i] = kind;
  double *o = (double *)((char *)out + ((n * 4 + 7) & ~7LL)) + i;
  if (channels & PT_SURF_BRDF_COLOR) {
    o[0] = pc.x;
    o[n] = pc.y;
    o[2 * n] = pc.z;
    o += 3 * n;
  }
  if (channels & PT_SURF_EMITTED) {
    o[0] = em.x;
    o[n] = em.y;
    o[2 * n] = em.z;
  }
}

// PointLightRenderer.__call__ per record: pointlight_shade (pt_simple.h) with wp, n, (u, v) and the ray's direction from the
// planes.  Kept from there on purpose: the second normalize3 of a normal that arrives normalised (render.py:175 calls
// normalized_dot), the BRDF's pigment taken once per hit in front of the light loop, ambient + emitted as the sum's start.
// The light loop is wave-uniform and EVERY lane enters world_query_lanes for every light (it ballots): the idle lanes of the
// last wave stand on record 0, they and the lanes without a hit enter with active = false.  A shadow ray's tmin is
// 1e-2 / |light - point| >= 0 for every finite record; one that is not (a NaN point) takes the exhaustive world_query, which
// the whole wave enters only when some lane needs it -- pt_rays_kernel's rule for the same filter.
// Three waves per SIMD, as the fused point-light kernel asks for (pt_simple.h): left to itself the compiler takes 187 VGPRs
// (two waves, no scratch); held to 168 it spills 48 B -- five stores in front of the light loop, three reloads inside it -- and
// the kernel is still a fifth faster on the C2 frame (profiles/surface_kernel.txt): its time is the latency of the query.
__global__ __launch_bounds__(PT_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 8))) void pt_shade_lights_kernel(
    const PtKArgs a, const int *__restrict__ slots, const int *__restrict__ shape, const double *__restrict__ point,
    const double *__restrict__ normal, const double *__restrict__ uv, const double *__restrict__ dir, long long n, V3 ambient, V3 bg,
    double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  const bool active = i < n;
  const long long j = active ? i : 0;
  const int slot = active ? surf_slot(a, slots, shape[j]) : -1;
  const bool lit = slot >= 0;
  Hit h;
  h.wp = {point[j], point[n + j], point[2 * n + j]};
  h.n = {normal[j], normal[n + j], normal[2 * n + j]};
  h.u = uv[j];
  h.v = uv[n + j];
  const V3 rd = {dir[j], dir[n + j], dir[2 * n + j]};
  pt_kargs ca = cold_args(a);
  const PtShapeAux *ax = ca->aux + (lit ? slot : 0);
  V3 res = bg;
  V3 pc = {0.0, 0.0, 0.0};
  bool diffuse = true;
  double spec_threshold = 0.0;
  if (lit) {
    const V3 em = surf_emitted_pigment(a, ax, h.u, h.v);
    res.x = ambient.x + em.x;
    res.y = ambient.y + em.y;
    res.z = ambient.z + em.z;
    pc = surf_brdf_pigment(a, ax, h.u, h.v);
    diffuse = ax->brdf_kind == PT_BRDF_DIFFUSE;
    spec_threshold = ax->brdf_param;
  }
  const int n_lights = ca->n_lights;
  const PtLight *lights = ca->lights;
  for (int l = 0; l < n_lights; ++l) {
    pt_kdouble L = PT_KD(&lights[l]);
    const V3 lp = {L[0], L[1], L[2]};
    // world.py:71-80: shadow ray from the hit point towards the light, any-hit in (1e-2/|d|, 1)
    Ray sh;
    sh.o = lit ? h.wp : lp;
    sh.d.x = lp.x - sh.o.x;
    sh.d.y = lp.y - sh.o.y;
    sh.d.z = lp.z - sh.o.z;
    const double dn = sqrt(sh.d.x * sh.d.x + sh.d.y * sh.d.y + sh.d.z * sh.d.z);
    sh.tmin = 1e-2 / dn;
    const bool exhaustive = lit && !(sh.tmin >= 0.0);
    double tlim;
    int blocked = world_query_lanes<true>(a, sh, 1.0, tlim, lit && !exhaustive, -1);
    if (__ballot(exhaustive) != 0ULL) {
      double t_all;
      const int blocked_all = world_query<true, false>(a, sh, 1.0, t_all, exhaustive);
      if (exhaustive) blocked = blocked_all;
    }
    if (lit && blocked < 0) {
      const V3 dv = {h.wp.x - lp.x, h.wp.y - lp.y, h.wp.z - lp.z};
      const double dist = sqrt(dv.x * dv.x + dv.y * dv.y + dv.z * dv.z);
      const double inv = 1.0 / dist;
      const V3 in_dir = {inv * dv.x, inv * dv.y, inv * dv.z};
      const V3 neg_in = {-in_dir.x, -in_dir.y, -in_dir.z};
      const double cos_theta = max2(0.0, dot3(normalize3(neg_in), normalize3(h.n)));
      const double lr = L[6];
      const double q = lr / dist;
      const double df = (lr > 0) ? q * q : 1.0;
      V3 bc = {0.0, 0.0, 0.0};
      if (diffuse) {  // materials.py:129-130
        const double k = 1.0 / PT_PI;
        bc.x = pc.x * k;
        bc.y = pc.y * k;
        bc.z = pc.z * k;
      } else {  // materials.py:164-173
        const V3 out_dir = {-rd.x, -rd.y, -rd.z};
        const double th_in = pt_acos(dot3(normalize3(h.n), normalize3(in_dir)));
        const double th_out = pt_acos(dot3(normalize3(h.n), normalize3(out_dir)));
        if (fabs(th_in - th_out) < spec_threshold) bc = pc;
      }
      res.x = res.x + bc.x * L[3] * cos_theta * df;
      res.y = res.y + bc.y * L[4] * cos_theta * df;
      res.z = res.z + bc.z * L[5] * cos_theta * df;
    }
  }
  if (!active) return;
  out[i] = res.x;
  out[n + i] = res.y;
  out[2 * n + i] = res.z;
}
