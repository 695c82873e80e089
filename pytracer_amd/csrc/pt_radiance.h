// pt_radiance.h -- PathTracer.__call__(ray) for a CALLER's rays, each with its own generator (include/ptrace_radiance.h).
// Included by ptrace_radiance.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h, pt_shade.h): nothing here is
// part of the other four libraries.
//
// What it restates: the recursion of render.py:99-139 as a loop over an explicit node stack, one ray per lane, depth-first in
// the reference's order of draws.  The queries are world_query_lanes (and, for an entry ray with tmin < 0, world_query), the
// record is hit_details<true>, the bounce scatter_ray<true>, the draws pcg_float -- the device functions of the fused path
// tracer, included as they are.  The arithmetic of a node is the oracle's pathtracer(), operation for operation:
//     cum = cum + hc * rad per child, in child order;  emitted + cum * (1.0 / num_of_rays) at the end;
//     emitted alone where the roulette ends the path;  the background on a miss;  black beyond max_depth without a query.
// A hit AT max_depth with lum > 0 still scatters num_of_rays times (2 draws each on a diffuse BRDF, none on a mirror): the
// generator jumps over those draws (nobody reads them), and the children's sum is 0.0 + hc * 0.0 once -- N additions of
// hc * 0 to a zero give that same zero, or that same NaN.
//
// The walk ends by integer counters alone: a node is pushed only while sp < levels (= max_depth - depth0 <= 64), every node
// spawns its `left` children and no more, and a wave's outer loop advances its ray index by the launch's lane count.  No
// floating-point value decides whether a lane loops again; a ray of NaNs hits nothing and returns the background.
//
// The node stack lives in the caller's workspace in HBM, planar [level][field][lane]: a wave's access to one field of one
// level is 512 consecutive bytes.  Fields: 0..2 hc (after the roulette's compensation), 3..5 emitted; MANY (num_of_rays > 1)
// only: 6..8 cum, 9 children still to spawn (an integer in the 8 bytes), 10..12 world point, 13..15 normal, 16..18 incoming
// direction, 19 BRDF kind (an integer).  Nothing of it is indexed at run time in registers or in a local array.
#pragma once

#define PT_RAD_FIELDS_ONE 6
#define PT_RAD_FIELDS_MANY 20

struct PtRadK {
  int N;       // num_of_rays >= 1
  int levels;  // max_depth - depth0: 0 .. 64, or < 0: every entry ray is deeper than max_depth
  int rr_rel;  // russian_roulette_limit - depth0, clamped into [-1, 65]: the roulette runs where sp >= rr_rel
  int channels;
  double bg[3];
  double invN;           // 1.0 / num_of_rays
  unsigned long long lanes;  // threads of the launch = lanes of the workspace
};

// materials.py:70-82 for a (u, v) nobody vouches for: an entry ray with an infinite direction and tmin < 0 reaches a plane at
// t = -0 with NaN surface coordinates.  Not >= 0 -> 0, >= w -> w - 1, else int()'s truncation: pigment_color's texel for every
// (u, v) in [0, 1], and an address inside the texture for every other.
PT_DEV long long rad_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}
template <typename CP>
PT_DEV V3 rad_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = rad_texel(u, w), row = rad_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}

struct RadStack {
  double *p;  // this lane's word of field 0, level 0
  size_t lanes;
  int fields;
  __device__ __forceinline__ double get(int slot, int field) const { return p[((size_t)slot * fields + field) * lanes]; }
  __device__ __forceinline__ void put(int slot, int field, double v) const { p[((size_t)slot * fields + field) * lanes] = v; }
  __device__ __forceinline__ int geti(int slot, int field) const { return (int)__double_as_longlong(get(slot, field)); }
  __device__ __forceinline__ void puti(int slot, int field, int v) const { put(slot, field, __longlong_as_double((long long)v)); }
};

// A wave takes rays [base, base + 64) and, when all of them are done, the next 64 that no other wave of the launch takes:
// base += lanes.  Every lane of the wave enters the queries (they ballot); lanes without a ray to query pass active = false.
template <bool MANY>
__global__ __launch_bounds__(PT_BLOCK) void pt_radiance_kernel(const PtKArgs a, const double *__restrict__ rays,
                                                               const unsigned long long *__restrict__ pcg_state,
                                                               const unsigned long long *__restrict__ pcg_inc, long long n, const PtRadK K,
                                                               double *__restrict__ ws, void *__restrict__ out) {
  const size_t gtid = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  RadStack st;
  st.p = ws + gtid;
  st.lanes = (size_t)K.lanes;
  st.fields = MANY ? PT_RAD_FIELDS_MANY : PT_RAD_FIELDS_ONE;
  const long long first_base = (long long)(gtid & ~(size_t)63);
  for (long long base = first_base; base < n; base += (long long)K.lanes) {
    const long long i = base + (long long)(threadIdx.x & 63);
    const bool active = i < n;
    const double *rp = rays + (active ? i : 0);
    Ray ray;
    ray.o = {rp[0], rp[n], rp[2 * n]};
    ray.d = {rp[3 * n], rp[4 * n], rp[5 * n]};
    ray.tmin = rp[6 * n];
    double tmax = rp[7 * n];
    Pcg g;
    g.state = pcg_state[active ? i : 0];
    g.inc = pcg_inc[active ? i : 0];
    g.n = 0;
    unsigned long long count = 0ULL;
    V3 ret = {0.0, 0.0, 0.0};
    int sp = 0;                              // nodes on this lane's stack = depth of `ray` below the entry ray
    bool query = active && K.levels >= 0;    // `ray` waits for its world query (render.py:100-101: deeper than max_depth -> black)
    bool done = active && !query;            // `ret` is the entry ray's radiance
    // pt_rays_kernel's way for an ENTRY ray that looks backwards (tmin < 0, or NaN): the filtered query drops roots <= 0, so such
    // a lane takes the exhaustive one, entered by the wave only when a ballot says some lane needs it.  Scattered rays: tmin > 0.
    bool behind = query && !(ray.tmin >= 0.0);
    bool entry = true;  // wave-uniform
    while (__ballot(query) != 0ULL) {
      double t;
      int hit = world_query_lanes<false>(a, ray, tmax, t, query && !behind, -1);
      if (entry && __ballot(behind) != 0ULL) {
        double t_all;
        const int hit_all = world_query<false, false>(a, ray, tmax, t_all, behind);
        if (behind) {
          hit = hit_all;
          t = t_all;
        }
      }
      entry = false;
      behind = false;
      // ---- render.py:103-134 for the ray that was queried, at depth sp ----
      bool returned = false, spawn = false;
      V3 f_wp = {0.0, 0.0, 0.0}, f_n = {0.0, 0.0, 1.0}, f_in = {0.0, 0.0, 1.0};
      int f_brdf = PT_BRDF_SPECULAR;
      if (query) {
        count++;
        query = false;
        returned = true;
        if (hit < 0) {
          ret.x = K.bg[0];
          ret.y = K.bg[1];
          ret.z = K.bg[2];
        } else {
          const PtShapeRec *rec = a.recs + hit;
          const PtShapeAux *ax = a.aux + hit;
          Hit h;
          hit_details<true>(rec, ax, ray, t, h, ax->needs_uv != 0);
          V3 hc = rad_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, h.u, h.v);
          const V3 em = rad_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, h.u, h.v);
          const double lum = max2(max2(hc.x, hc.y), hc.z);
          bool ended = false;
          if (sp >= K.rr_rel) {  // render.py:116-123
            const double q = max2(0.05, 1.0 - lum);
            if (pcg_float(g) > q) {
              const double k = 1.0 / (1.0 - q);
              hc.x = hc.x * k;
              hc.y = hc.y * k;
              hc.z = hc.z * k;
            } else {
              ret = em;
              ended = true;
            }
          }
          if (!ended) {
            if (!(lum > 0.0)) {  // render.py:139 with cum_radiance = 0
              ret.x = em.x + 0.0 * K.invN;
              ret.y = em.y + 0.0 * K.invN;
              ret.z = em.z + 0.0 * K.invN;
            } else if (sp >= K.levels) {
              // a hit AT max_depth: scatter_ray runs num_of_rays times, its draws are consumed, every child is black without a query
              if (ax->brdf_kind == PT_BRDF_DIFFUSE) g.state = pcg_advance(g.state, g.inc, 2u * (unsigned)K.N);
              const V3 fc = {0.0 + hc.x * 0.0, 0.0 + hc.y * 0.0, 0.0 + hc.z * 0.0};
              ret.x = em.x + fc.x * K.invN;
              ret.y = em.y + fc.y * K.invN;
              ret.z = em.z + fc.z * K.invN;
            } else {  // render.py:126-137: push the node, child 0 is scattered below
              st.put(sp, 0, hc.x);
              st.put(sp, 1, hc.y);
              st.put(sp, 2, hc.z);
              st.put(sp, 3, em.x);
              st.put(sp, 4, em.y);
              st.put(sp, 5, em.z);
              if (MANY) {
                st.put(sp, 6, 0.0);
                st.put(sp, 7, 0.0);
                st.put(sp, 8, 0.0);
                st.puti(sp, 9, K.N - 1);
                st.put(sp, 10, h.wp.x);
                st.put(sp, 11, h.wp.y);
                st.put(sp, 12, h.wp.z);
                st.put(sp, 13, h.n.x);
                st.put(sp, 14, h.n.y);
                st.put(sp, 15, h.n.z);
                st.put(sp, 16, ray.d.x);
                st.put(sp, 17, ray.d.y);
                st.put(sp, 18, ray.d.z);
                st.puti(sp, 19, ax->brdf_kind);
              }
              f_wp = h.wp;
              f_n = h.n;
              f_in = ray.d;
              f_brdf = ax->brdf_kind;
              sp++;
              spawn = true;
              returned = false;
            }
          }
        }
      }
      // ---- a call returned `ret`: hand it to the node above, which spawns its next child or returns in turn ----
      // (at most `levels` turns: sp falls by one in every turn in which the lane stays in the loop)
      while (__ballot(returned && sp > 0) != 0ULL) {
        if (returned && sp > 0) {
          const int slot = sp - 1;
          const V3 hc = {st.get(slot, 0), st.get(slot, 1), st.get(slot, 2)};
          V3 cum = {0.0, 0.0, 0.0};
          int left = 0;
          if (MANY) {
            cum = {st.get(slot, 6), st.get(slot, 7), st.get(slot, 8)};
            left = st.geti(slot, 9);
          }
          cum.x = cum.x + hc.x * ret.x;  // render.py:135-137
          cum.y = cum.y + hc.y * ret.y;
          cum.z = cum.z + hc.z * ret.z;
          if (MANY && left > 0) {
            st.put(slot, 6, cum.x);
            st.put(slot, 7, cum.y);
            st.put(slot, 8, cum.z);
            st.puti(slot, 9, left - 1);
            f_wp = {st.get(slot, 10), st.get(slot, 11), st.get(slot, 12)};
            f_n = {st.get(slot, 13), st.get(slot, 14), st.get(slot, 15)};
            f_in = {st.get(slot, 16), st.get(slot, 17), st.get(slot, 18)};
            f_brdf = st.geti(slot, 19);
            spawn = true;
            returned = false;
          } else {
            const V3 em = {st.get(slot, 3), st.get(slot, 4), st.get(slot, 5)};
            ret.x = em.x + cum.x * K.invN;  // render.py:139
            ret.y = em.y + cum.y * K.invN;
            ret.z = em.z + cum.z * K.invN;
            sp = slot;
          }
        }
      }
      if (returned) done = true;  // (sp == 0: the entry ray's own call returned)
      if (spawn) {                // brdf.scatter_ray for the next child of the node at sp - 1, at depth sp
        ray = scatter_ray<true>(f_brdf, g, f_in, f_wp, f_n);
        tmax = INFINITY;
        query = true;
      }
    }
    if (done) {
      double *o = (double *)out + i;
      o[0] = ret.x;
      o[n] = ret.y;
      o[2 * n] = ret.z;
      unsigned long long *u = (unsigned long long *)(o + 3 * n);
      if (K.channels & PT_RAD_PCG) {
        u[0] = g.state;
        u[n] = g.inc;
        u += 2 * n;
      }
      if (K.channels & PT_RAD_COUNT) u[0] = count;
    }
  }
}
