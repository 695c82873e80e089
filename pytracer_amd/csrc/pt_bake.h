// pt_bake.h -- surface points from (shape, u, v), and light maps over a shape's (u, v) grid (include/ptrace_bake.h).
// Included by ptrace_bake.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h, pt_shade.h): nothing here is
// part of the other six libraries.
//
// What it restates: the INVERSE of the shapes' (u, v) maps (shapes.py:36-42, 183-185) with the point and normal transforms of
// transformations.py:58-96 (bake_surface_point: the one __device__ function both kernels call, so both give the same bits); per
// sample j = t_local * K + k of a texel PCG(init_state, init_seq + t K + k) (pcg_seed), the two jitter draws, the surface point,
// DiffuseBRDF.scatter_ray there (scatter_ray<true>), then the recursion of render.py:99-139 for that ray as a loop over an
// explicit node stack -- the walk of pt_gather.h, restated here on purpose (that header belongs to its one translation unit).
// The arithmetic of a node is the oracle's pathtracer(), operation for operation:
//     cum = cum + hc * rad per child, in child order;  emitted + cum * (1.0 / num_of_rays) at the end;
//     emitted alone where the roulette ends the path;  the background on a miss.
// A hit AT max_depth with lum > 0 still scatters num_of_rays times: the generator jumps over those draws, and the children's
// sum is 0.0 + hc * 0.0 once.
//
// The front end (bake_front) replaces the gather's loads of a point and a normal: two draws, the shape's record, two sincos and
// the two transforms with the normalisation.  It is inlined: what it computes on the way is dead before the walk starts, and the
// compiler does not spill for it (234 / 236 VGPRs against the gather's 232, no scratch, the same two waves per SIMD; behind a
// call it cost 80 B of scratch for the values handed back).
//
// The walk ends by integer counters alone: a node is pushed only while sp < levels (= max_depth - depth0 <= 64), every node
// spawns its `left` children and no more, and a wave's outer loop advances its sample index by the launch's lane count.  No
// floating-point value decides whether a lane loops again; a ray of NaNs hits nothing and returns the background.
//
// Work layout: the gather's.  A wave takes samples [base, base + 64) -- one texel's samples are neighbours -- and then the next
// 64 that no other wave of the launch takes: base += lanes.  The node stack lives in the caller's workspace in HBM, planar
// [level][field][lane]; behind it the sample planes [4][w h K]: L_tk r, g, b and the sample's count.
//
// The mean: pt_bake_mean_kernel, a second launch on the same stream, one lane per texel, adds the texel's K values in k order
// (staged through LDS as pt_gather_mean_kernel stages them).  No atomics, nothing that depends on scheduling or launch shape.
#pragma once

#define PT_BAKE_FIELDS_ONE 6
#define PT_BAKE_FIELDS_MANY 20
#define PT_BAKE_SAMPLE_PLANES 4

struct PtBakeK {
  int samples;  // K >= 1
  int N;        // num_of_rays >= 1
  int levels;   // max_depth - depth0: 0 .. 64, or < 0: every sample's ray is deeper than max_depth
  int rr_rel;   // russian_roulette_limit - depth0, clamped into [-1, 65]: the roulette runs where sp >= rr_rel
  int channels;
  int shape;    // World.shapes index (inside [0, n_shapes): the host checked)
  int side;     // +1 or -1
  int jitter;
  int W, col0, row0, w;  // the map's width, the rectangle's corner and width (texel t_local = r * w + c)
  double invW, invH;     // 1.0 / W, 1.0 / H
  double bg[3];
  double invN;  // 1.0 / num_of_rays
  double invK;  // 1.0 / samples
  unsigned long long init_state, init_seq;
  unsigned long long lanes;  // threads of the walk's launch = lanes of the node stacks
};

// materials.py:70-82 for a (u, v) nobody vouches for: an address inside the texture for every (u, v) (as pt_gather.h has it).
PT_DEV long long bake_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}
template <typename CP>
PT_DEV V3 bake_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = bake_texel(u, w), row = bake_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}

// World.shapes index -> grouped slot, or -1.  `index` is a permutation of 0 .. n_shapes - 1 (pt_scene_build.h): a scan of the
// records' index fields, fewer loads than ONE ray's world query makes (the loop index is wave-uniform: scalar loads).
PT_DEV int bake_slot(const PtKArgs &a, int shape) {
  int slot = -1;
  if ((unsigned)shape >= (unsigned)a.n_shapes) return slot;
  for (int s = 0; s < a.n_shapes; s++)
    if (a.recs[s].index == shape) slot = s;
  return slot;
}

// S(shape, u, v, side) of include/ptrace_bake.h for the record (rec, ax).  sincos inline: both callers have registers to spare
// (a kernel of its own; the front of a walk whose registers are not live yet), and the values are ocml's either way.
struct BakePoint {
  V3 wp, wn;
};
PT_DEV BakePoint bake_surface_point(const PtShapeRec *rec, const PtShapeAux *ax, double u, double v, double side) {
  V3 p, nl;
  if (rec->kind == PT_SHAPE_SPHERE) {
    const double th = v * PT_PI, ph = (2.0 * PT_PI) * u;
    double st, ct, sp, cp;
    sincos(th, &st, &ct);
    sincos(ph, &sp, &cp);
    p.x = st * cp;
    p.y = st * sp;
    p.z = ct;
    nl.x = side * p.x;
    nl.y = side * p.y;
    nl.z = side * p.z;
  } else {
    p.x = u;
    p.y = v;
    p.z = 0.0;
    nl.x = 0.0;
    nl.y = 0.0;
    nl.z = side;
  }
  double fm[12], im[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) fm[k] = ax->m[k];
#pragma unroll
  for (int k = 0; k < 12; ++k) im[k] = rec->invm[k];
  BakePoint r;
  r.wp = xf_point(fm, p);
  r.wn = normalize3(xf_normal(im, nl));
  return r;
}

// One record per lane.  Out: planar [6, n], point then normal; a record whose shape names no record: zeros.
__global__ __launch_bounds__(PT_BLOCK) void pt_surface_points_kernel(const PtKArgs a, const int *__restrict__ shape, const double *__restrict__ uv,
                                                                     const int *__restrict__ side, long long n, double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int slot = bake_slot(a, shape[i]);
  BakePoint b = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (slot >= 0) b = bake_surface_point(a.recs + slot, a.aux + slot, uv[i], uv[n + i], (side != nullptr && side[i] < 0) ? -1.0 : 1.0);
  double *o = out + i;
  o[0] = b.wp.x;
  o[n] = b.wp.y;
  o[2 * n] = b.wp.z;
  o[3 * n] = b.wn.x;
  o[4 * n] = b.wn.y;
  o[5 * n] = b.wn.z;
}

// The bake's front end for the sample that draws from stream `seq` at texel (col, row): the generator, the jitter draws, the
// surface point.  Everything goes in and comes out by value: nothing of the kernel's argument blocks has its address taken.
struct BakeFront {
  Pcg g;
  BakePoint b;
};
PT_DEV BakeFront bake_front(const PtShapeRec *rec, const PtShapeAux *ax, double col, double row, unsigned long long init_state,
                                 unsigned long long seq, int jitter, double invW, double invH, double side) {
  BakeFront f;
  pcg_seed(f.g, init_state, seq);
  double ju = 0.5, jv = 0.5;
  if (jitter) {
    ju = pcg_float(f.g);
    jv = pcg_float(f.g);
  }
  const double u = (col + ju) * invW, v = (row + jv) * invH;
  f.b = bake_surface_point(rec, ax, u, v, side);
  return f;
}

struct BakeStack {
  double *p;  // this lane's word of field 0, level 0
  size_t lanes;
  int fields;
  __device__ __forceinline__ double get(int slot, int field) const { return p[((size_t)slot * fields + field) * lanes]; }
  __device__ __forceinline__ void put(int slot, int field, double v) const { p[((size_t)slot * fields + field) * lanes] = v; }
  __device__ __forceinline__ int geti(int slot, int field) const { return (int)__double_as_longlong(get(slot, field)); }
  __device__ __forceinline__ void puti(int slot, int field, int v) const { put(slot, field, __longlong_as_double((long long)v)); }
};

// `total` = w * h * K <= 2^31 - 1.  Every lane of a wave enters the query (it ballots); lanes without a sample pass active = false.
template <bool MANY>
__global__ __launch_bounds__(PT_BLOCK) void pt_bake_kernel(const PtKArgs a, long long total, const PtBakeK K, double *__restrict__ ws,
                                                           double *__restrict__ samples) {
  const size_t gtid = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  BakeStack st;
  st.p = ws + gtid;
  st.lanes = (size_t)K.lanes;
  st.fields = MANY ? PT_BAKE_FIELDS_MANY : PT_BAKE_FIELDS_ONE;
  const int shape_slot = bake_slot(a, K.shape);  // (uniform)
  const long long first_base = (long long)(gtid & ~(size_t)63);
  for (long long base = first_base; base < total; base += (long long)K.lanes) {
    const long long j = base + (long long)(threadIdx.x & 63);
    const bool inside = j < total;
    const unsigned tl = inside ? (unsigned)j / (unsigned)K.samples : 0u;  // (j < 2^31: a 32-bit division)
    const unsigned long long k = inside ? (unsigned long long)((unsigned)j - tl * (unsigned)K.samples) : 0ULL;
    const bool active = inside && shape_slot >= 0;
    V3 f_wp = {0.0, 0.0, 0.0};
    V3 f_n = {0.0, 0.0, 1.0};
    V3 f_in = {0.0, 0.0, 1.0};  // (a DiffuseBRDF does not look at the incoming direction)
    int f_brdf = PT_BRDF_DIFFUSE;
    Pcg g;
    g.state = 0ULL;
    g.inc = 1ULL;
    g.n = 0;
    if (active) {
      const unsigned r = tl / (unsigned)K.w, c = tl - r * (unsigned)K.w;
      const long long col = (long long)K.col0 + c, row = (long long)K.row0 + r;  // (exact as doubles: below 2^32)
      const unsigned long long t = (unsigned long long)row * (unsigned long long)K.W + (unsigned long long)col;  // the GLOBAL texel
      const BakeFront f = bake_front(a.recs + shape_slot, a.aux + shape_slot, (double)col, (double)row, K.init_state,
                                     K.init_seq + t * (unsigned long long)K.samples + k, K.jitter, K.invW, K.invH, (double)K.side);
      g = f.g;
      f_wp = f.b.wp;
      f_n = f.b.wn;
    }
    unsigned long long count = 0ULL;
    V3 ret = {0.0, 0.0, 0.0};
    Ray ray;
    ray.o = {0.0, 0.0, 0.0};
    ray.d = {0.0, 0.0, 1.0};
    ray.tmin = 1.0e-3;
    int sp = 0;                              // nodes on this lane's stack = depth of `ray` below the entry ray
    bool spawn = active && K.levels >= 0;    // a scatter_ray is due: the entry ray first (deeper than max_depth -> black, no draw seen)
    while (__ballot(spawn) != 0ULL) {
      // ---- brdf.scatter_ray: the entry ray at the surface point, or the next child of the node at sp - 1; always at depth sp ----
      const bool query = spawn;
      if (spawn) ray = scatter_ray<true>(f_brdf, g, f_in, f_wp, f_n);
      spawn = false;
      double t;
      const int hit = world_query_lanes<false>(a, ray, INFINITY, t, query, -1);
      // ---- render.py:103-134 for the ray that was queried, at depth sp ----
      bool returned = false;
      if (query) {
        count++;
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
          V3 hc = bake_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, h.u, h.v);
          const V3 em = bake_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, h.u, h.v);
          const double lum = max2(max2(hc.x, hc.y), hc.z);
          bool ended = false;
          if (sp >= K.rr_rel) {  // render.py:116-123
            const double q = max2(0.05, 1.0 - lum);
            if (pcg_float(g) > q) {
              const double kk = 1.0 / (1.0 - q);
              hc.x = hc.x * kk;
              hc.y = hc.y * kk;
              hc.z = hc.z * kk;
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
            } else {  // render.py:126-137: push the node, child 0 is scattered at the top of the loop
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
    }
    if (inside) {  // (levels < 0, or no record for the shape: black and 0, as initialised)
      double *o = samples + j;
      o[0] = ret.x;
      o[total] = ret.y;
      o[2 * total] = ret.z;
      if (K.channels & PT_BAKE_COUNT) ((unsigned long long *)o)[3 * total] = count;
    }
  }
}

// The mean.  One texel per lane: out_t = (((0 + L_t0) + L_t1) + ... + L_t,K-1) * (1.0 / K) per channel, the counts added in the
// same order.  A workgroup stages the values of its 256 texels through LDS, PT_BAKE_TILE samples of a plane at a time: 16
// consecutive lanes load one texel's 128 consecutive bytes, the tile is written as [texel][sample] with a row of 17 words (a
// lane's row starts on its own banks), and behind a barrier every lane adds its row in k order.  The trip counts depend on K
// alone, so every wave of a workgroup reaches every barrier; nobody waits for another workgroup.
#define PT_BAKE_TILE 16
#define PT_BAKE_ROW (PT_BAKE_TILE + 1)

template <bool AS_DOUBLE>
__device__ __forceinline__ void bake_stage_and_add(const unsigned long long *__restrict__ plane, unsigned long long *tile, long long rec0,
                                                   long long n, int samples, int k0, double &acc, unsigned long long &cnt) {
  // load: element e = lane + 256 m of the tile is (texel e / 16, sample e % 16)
#pragma unroll
  for (int m = 0; m < PT_BAKE_TILE; m++) {
    const int e = (int)threadIdx.x + PT_BLOCK * m;
    const int r = e / PT_BAKE_TILE, kk = e % PT_BAKE_TILE;
    const long long rec = rec0 + r;
    const int k = k0 + kk;
    unsigned long long v = 0ULL;
    if (rec < n && k < samples) v = plane[rec * samples + k];
    tile[r * PT_BAKE_ROW + kk] = v;
  }
  __syncthreads();
  const int left = samples - k0 < PT_BAKE_TILE ? samples - k0 : PT_BAKE_TILE;  // (uniform)
  const unsigned long long *row = tile + threadIdx.x * PT_BAKE_ROW;
  for (int kk = 0; kk < left; kk++) {
    if (AS_DOUBLE)
      acc = acc + __longlong_as_double((long long)row[kk]);
    else
      cnt += row[kk];
  }
  __syncthreads();
}

// `n` = w * h texels, `total` = n * K
__global__ __launch_bounds__(PT_BLOCK) void pt_bake_mean_kernel(const double *__restrict__ samples, long long n, long long total, const PtBakeK K,
                                                                void *__restrict__ out) {
  __shared__ unsigned long long tile[PT_BLOCK * PT_BAKE_ROW];
  const long long rec0 = (long long)blockIdx.x * PT_BLOCK;
  const long long i = rec0 + threadIdx.x;
  const unsigned long long *planes = (const unsigned long long *)samples;
  const bool counted = (K.channels & PT_BAKE_COUNT) != 0;
  double sx = 0.0, sy = 0.0, sz = 0.0, unused = 0.0;
  unsigned long long count = 0ULL, none = 0ULL;
  for (int k0 = 0; k0 < K.samples; k0 += PT_BAKE_TILE) {  // (K <= 2^31 - 1, and k0 stops at the last tile: no overflow below)
    bake_stage_and_add<true>(planes, tile, rec0, n, K.samples, k0, sx, none);
    bake_stage_and_add<true>(planes + total, tile, rec0, n, K.samples, k0, sy, none);
    bake_stage_and_add<true>(planes + 2 * total, tile, rec0, n, K.samples, k0, sz, none);
    if (counted) bake_stage_and_add<false>(planes + 3 * total, tile, rec0, n, K.samples, k0, unused, count);
    if (K.samples - k0 <= PT_BAKE_TILE) break;
  }
  if (i >= n) return;
  double *o = (double *)out + i;
  o[0] = sx * K.invK;
  o[n] = sy * K.invK;
  o[2 * n] = sz * K.invK;
  if (counted) ((unsigned long long *)o)[3 * n] = count;
}
