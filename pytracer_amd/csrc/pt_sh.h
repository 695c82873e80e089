// pt_sh.h -- SH radiance probes at free points: directions, the walk, the projection and the evaluation (include/ptrace_sh.h).
// Included by ptrace_sh.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h, pt_shade.h): nothing here is part of
// the other seven libraries.
//
// What it restates: per sample j = i * K + k of probe i, PCG(init_state, seq_i + k) (pcg_seed), the uniform direction D(g) of
// include/ptrace_sh.h (sh_direction: the one __device__ function the walk and the directions query call, so both give the same
// bits), the ray Ray(x_i, d, tmin = 1e-5, tmax = inf) (ray.py's defaults), then the recursion of render.py:99-139 for that ray as a
// loop over an explicit node stack -- the walk of pt_radiance.h with a GIVEN entry ray, restated here on purpose (that header
// belongs to its one translation unit).  The arithmetic of a node is the oracle's pathtracer(), operation for operation:
//     cum = cum + hc * rad per child, in child order;  emitted + cum * (1.0 / num_of_rays) at the end;
//     emitted alone where the roulette ends the path;  the background on a miss;  black beyond max_depth without a query.
// A hit AT max_depth with lum > 0 still scatters num_of_rays times: the generator jumps over those draws, and the children's
// sum is 0.0 + hc * 0.0 once.
//
// The front end (seed, two draws, one sqrt, one sincos) is inlined and dead before the walk starts: what stays live is the ray and
// the generator, as in the radiance query.  The direction goes to three sample planes at once; the projection reads it from there.
// The entry ray's tmin is 1e-5 > 0, so the filtered query serves it: the exhaustive backward-looking query of the radiance kernel
// is not here.
//
// The walk ends by integer counters alone: a node is pushed only while sp < levels (= max_depth - depth0 <= 64), every node
// spawns its `left` children and no more, and a wave's outer loop advances its sample index by the launch's lane count.  No
// floating-point value decides whether a lane loops again; a ray of NaNs hits nothing and returns the background.
//
// Work layout: the gather's.  A wave takes samples [base, base + 64) -- one probe's samples are neighbours -- and then the next
// 64 that no other wave of the launch takes: base += lanes.  The node stack lives in the caller's workspace in HBM, planar
// [level][field][lane]; behind it the sample planes [7][n K]: L_ik r, g, b, the sample's count, d_ik x, y, z.
//
// The projection: pt_sh_project_kernel, a second launch on the same stream, one lane per probe, 27 accumulators in registers,
// adds Y_j(d_ik) * L_ik[ch] in k order (the planes staged through LDS as pt_gather_mean_kernel stages them).  No atomics, nothing
// that depends on scheduling or launch shape.
#pragma once

#define PT_SHP_FIELDS_ONE 6
#define PT_SHP_FIELDS_MANY 20
#define PT_SHP_SAMPLE_PLANES 7

struct PtShK {
  int samples;  // K >= 1
  int N;        // num_of_rays >= 1
  int levels;   // max_depth - depth0: 0 .. 64, or < 0: every sample's ray is deeper than max_depth
  int rr_rel;   // russian_roulette_limit - depth0, clamped into [-1, 65]: the roulette runs where sp >= rr_rel
  int channels;
  double bg[3];
  double invN;   // 1.0 / num_of_rays
  double scale;  // (4.0 * pi) * (1.0 / samples)
  unsigned long long init_state, init_seq;
  unsigned long long lanes;  // threads of the walk's launch = lanes of the node stacks
};

// ---- D(g) of include/ptrace_sh.h: two draws, uniform on the sphere ---------------------------------------------------------------
PT_DEV V3 sh_direction(Pcg &g) {
  const double u1 = pcg_float(g);
  const double u2 = pcg_float(g);
  const double z = 1.0 - 2.0 * u1;
  const double r = sqrt(1.0 - z * z);
  const double ph = (2.0 * PT_PI) * u2;
  double sp, cp;
  sincos(ph, &sp, &cp);
  V3 d;
  d.x = r * cp;
  d.y = r * sp;
  d.z = z;
  return d;
}

// stream number of probe i (seq == nullptr: init_seq + i K, the gather's default)
PT_DEV unsigned long long sh_seq(const unsigned long long *__restrict__ seq, const PtShK &K, long long i) {
  return seq ? seq[i] : K.init_seq + (unsigned long long)i * (unsigned long long)K.samples;
}

// ---- Y_0 .. Y_8 of include/ptrace_sh.h: each constant ONE literal, the products in the header's order ----------------------------
#define PT_SH_Y0(x, y, z) (0.28209479177387814)
#define PT_SH_Y1(x, y, z) (0.4886025119029199 * (y))
#define PT_SH_Y2(x, y, z) (0.4886025119029199 * (z))
#define PT_SH_Y3(x, y, z) (0.4886025119029199 * (x))
#define PT_SH_Y4(x, y, z) (1.0925484305920792 * ((x) * (y)))
#define PT_SH_Y5(x, y, z) (1.0925484305920792 * ((y) * (z)))
#define PT_SH_Y6(x, y, z) (0.31539156525252005 * (3.0 * ((z) * (z)) - 1.0))
#define PT_SH_Y7(x, y, z) (1.0925484305920792 * ((x) * (z)))
#define PT_SH_Y8(x, y, z) (0.5462742152960396 * ((x) * (x) - (y) * (y)))

struct ShBasis {
  double y0, y1, y2, y3, y4, y5, y6, y7, y8;
};
PT_DEV ShBasis sh_basis(double x, double y, double z) {
  ShBasis b;
  b.y0 = PT_SH_Y0(x, y, z);
  b.y1 = PT_SH_Y1(x, y, z);
  b.y2 = PT_SH_Y2(x, y, z);
  b.y3 = PT_SH_Y3(x, y, z);
  b.y4 = PT_SH_Y4(x, y, z);
  b.y5 = PT_SH_Y5(x, y, z);
  b.y6 = PT_SH_Y6(x, y, z);
  b.y7 = PT_SH_Y7(x, y, z);
  b.y8 = PT_SH_Y8(x, y, z);
  return b;
}

// materials.py:70-82 for a (u, v) nobody vouches for: an address inside the texture for every (u, v) (as pt_radiance.h has it).
PT_DEV long long sh_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}
template <typename CP>
PT_DEV V3 sh_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = sh_texel(u, w), row = sh_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}

// ---- the directions alone: one sample per lane, planar [3][n K] ------------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_sh_directions_kernel(const unsigned long long *__restrict__ seq, long long total, const PtShK K,
                                                                    double *__restrict__ out) {
  const long long j = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (j >= total) return;
  const long long i = (long long)((unsigned)j / (unsigned)K.samples);  // (j < 2^31: a 32-bit division)
  const unsigned long long k = (unsigned long long)(j - i * K.samples);
  Pcg g;
  pcg_seed(g, K.init_state, sh_seq(seq, K, i) + k);
  const V3 d = sh_direction(g);
  double *o = out + j;
  o[0] = d.x;
  o[total] = d.y;
  o[2 * total] = d.z;
}

struct ShStack {
  double *p;  // this lane's word of field 0, level 0
  size_t lanes;
  int fields;
  __device__ __forceinline__ double get(int slot, int field) const { return p[((size_t)slot * fields + field) * lanes]; }
  __device__ __forceinline__ void put(int slot, int field, double v) const { p[((size_t)slot * fields + field) * lanes] = v; }
  __device__ __forceinline__ int geti(int slot, int field) const { return (int)__double_as_longlong(get(slot, field)); }
  __device__ __forceinline__ void puti(int slot, int field, int v) const { put(slot, field, __longlong_as_double((long long)v)); }
};

// ---- the walk ------------------------------------------------------------------------------------------------------------------
// `total` = n * K <= 2^31 - 1.  Every lane of a wave enters the query (it ballots); lanes without a ray pass active = false.
// A sample of a skipped probe writes nothing: the projection does not add it.
template <bool MANY>
__global__ __launch_bounds__(PT_BLOCK) void pt_sh_kernel(const PtKArgs a, const double *__restrict__ points, const int *__restrict__ act,
                                                         const unsigned long long *__restrict__ seq, long long n, long long total, const PtShK K,
                                                         double *__restrict__ ws, double *__restrict__ samples) {
  const size_t gtid = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  ShStack st;
  st.p = ws + gtid;
  st.lanes = (size_t)K.lanes;
  st.fields = MANY ? PT_SHP_FIELDS_MANY : PT_SHP_FIELDS_ONE;
  const long long first_base = (long long)(gtid & ~(size_t)63);
  for (long long base = first_base; base < total; base += (long long)K.lanes) {
    const long long j = base + (long long)(threadIdx.x & 63);
    const bool inside = j < total;
    const long long i = inside ? (long long)((unsigned)j / (unsigned)K.samples) : 0;  // (j < 2^31: a 32-bit division)
    const unsigned long long k = (unsigned long long)(inside ? j - i * K.samples : 0);
    const bool active = inside && (act == nullptr || act[i] >= 0);
    // the front end: the probe's point, the generator, the direction (on its way to the planes at once)
    Ray ray;
    ray.o = {points[i], points[n + i], points[2 * n + i]};
    ray.tmin = 1.0e-5;
    Pcg g;
    pcg_seed(g, K.init_state, sh_seq(seq, K, i) + k);
    ray.d = sh_direction(g);
#ifndef PT_SH_RECOMPUTE_DIRS
    if (active) {
      double *o = samples + j;
      o[4 * total] = ray.d.x;
      o[5 * total] = ray.d.y;
      o[6 * total] = ray.d.z;
    }
#endif
    unsigned long long count = 0ULL;
    V3 ret = {0.0, 0.0, 0.0};
    int sp = 0;                            // nodes on this lane's stack = depth of `ray` below the entry ray
    bool query = active && K.levels >= 0;  // `ray` waits for its world query (render.py:100-101: deeper than max_depth -> black)
    while (__ballot(query) != 0ULL) {
      double t;
      const int hit = world_query_lanes<false>(a, ray, INFINITY, t, query, -1);
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
          V3 hc = sh_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, h.u, h.v);
          const V3 em = sh_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, h.u, h.v);
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
      if (spawn) {  // brdf.scatter_ray for the next child of the node at sp - 1, at depth sp
        ray = scatter_ray<true>(f_brdf, g, f_in, f_wp, f_n);
        query = true;
      }
    }
    if (active) {  // (levels < 0: black and 0, as initialised)
      double *o = samples + j;
      o[0] = ret.x;
      o[total] = ret.y;
      o[2 * total] = ret.z;
      if (K.channels & PT_SH_COUNT) ((unsigned long long *)o)[3 * total] = count;
    }
  }
}

// ---- the projection ------------------------------------------------------------------------------------------------------------
// One probe per lane: c_i[j][ch] = ((((0 + Y_j(d_i0) * L_i0[ch]) + Y_j(d_i1) * L_i1[ch]) + ...) * scale, the counts added in the
// same order.  A lane's K values are consecutive in a sample plane, so lanes that read them directly stand K * 8 bytes apart and
// every load of a wave touches 64 lines (the gather's mean measured what that costs).  So the planes are staged through LDS as
// pt_gather_mean_kernel stages them, PT_SHP_TILE samples at a time: 16 consecutive lanes load one probe's 128 consecutive bytes,
// a tile is written as [probe][sample] with a row of 17 words (a lane's row starts on its own banks), and behind a barrier every
// lane walks its row in k order.  Unlike a mean, a projection needs a sample's direction and its radiance TOGETHER, so all seven
// planes of a tile are staged at once; to fit them, a workgroup is ONE wave of 64 probes (7 x 64 x 17 x 8 B = 60928 B of LDS).  The
// accumulators are 27 named doubles: nothing is indexed at run time.  Every line of the planes is fetched once.  The trip counts
// depend on K alone, so the wave reaches every barrier; nobody waits for another workgroup.  A skipped probe's samples were never
// written: they are loaded like the others (inside the planes), and the lane's result is replaced by zeros.
// -DPT_SH_RECOMPUTE_DIRS builds the alternative that was measured against this one (DESIGN item 31): no direction planes; the
// lane makes d_ik again from PCG(init_state, seq_i + k) with sh_direction -- the same bits, K serial sincos per lane.
#define PT_SHP_BLOCK 64
#define PT_SHP_TILE 16
#define PT_SHP_ROW (PT_SHP_TILE + 1)
#define PT_SHP_TILE_WORDS (PT_SHP_BLOCK * PT_SHP_ROW)

struct ShAcc {
  double c0, c1, c2, c3, c4, c5, c6, c7, c8;
};

__device__ __forceinline__ void sh_add(ShAcc &c, const ShBasis &b, double L) {
  c.c0 = c.c0 + b.y0 * L;
  c.c1 = c.c1 + b.y1 * L;
  c.c2 = c.c2 + b.y2 * L;
  c.c3 = c.c3 + b.y3 * L;
  c.c4 = c.c4 + b.y4 * L;
  c.c5 = c.c5 + b.y5 * L;
  c.c6 = c.c6 + b.y6 * L;
  c.c7 = c.c7 + b.y7 * L;
  c.c8 = c.c8 + b.y8 * L;
}

// plane 3 j + ch of the output
__device__ __forceinline__ void sh_store(double *o, long long n, int ch, const ShAcc &c, double scale) {
  o[(0 + ch) * n] = c.c0 * scale;
  o[(3 + ch) * n] = c.c1 * scale;
  o[(6 + ch) * n] = c.c2 * scale;
  o[(9 + ch) * n] = c.c3 * scale;
  o[(12 + ch) * n] = c.c4 * scale;
  o[(15 + ch) * n] = c.c5 * scale;
  o[(18 + ch) * n] = c.c6 * scale;
  o[(21 + ch) * n] = c.c7 * scale;
  o[(24 + ch) * n] = c.c8 * scale;
}

// `n` probes, `total` = n * K; launched with PT_SHP_BLOCK threads per workgroup
__global__ __launch_bounds__(PT_SHP_BLOCK) void pt_sh_project_kernel(const double *__restrict__ samples, const int *__restrict__ act,
                                                                     const unsigned long long *__restrict__ seq, long long n, long long total,
                                                                     const PtShK K, void *__restrict__ out) {
  __shared__ unsigned long long tile[PT_SHP_SAMPLE_PLANES * PT_SHP_TILE_WORDS];
  const long long rec0 = (long long)blockIdx.x * PT_SHP_BLOCK;
  const long long i = rec0 + threadIdx.x;
  const unsigned long long *planes = (const unsigned long long *)samples;
  const bool counted = (K.channels & PT_SH_COUNT) != 0;
  const ShAcc zero = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ShAcc cr = zero, cg = zero, cb = zero;
  unsigned long long count = 0ULL;
#ifdef PT_SH_RECOMPUTE_DIRS
  const unsigned long long seq_i = sh_seq(seq, K, i < n ? i : 0);
#endif
  for (int k0 = 0; k0 < K.samples; k0 += PT_SHP_TILE) {  // (K <= 2^31 - 1, and k0 stops at the last tile: no overflow below)
    // load: element e = lane + 64 m of a tile is (probe e / 16, sample e % 16)
#pragma unroll
    for (int m = 0; m < PT_SHP_TILE; m++) {
      const int e = (int)threadIdx.x + PT_SHP_BLOCK * m;
      const int r = e / PT_SHP_TILE, kk = e % PT_SHP_TILE;
      const long long rec = rec0 + r;
      const int k = k0 + kk;
      const bool have = rec < n && k < K.samples;
      const unsigned long long *src = planes + (have ? rec * K.samples + k : 0);
      unsigned long long *dst = tile + r * PT_SHP_ROW + kk;
#pragma unroll
      for (int pl = 0; pl < PT_SHP_SAMPLE_PLANES; pl++) {
        unsigned long long v = 0ULL;
#ifdef PT_SH_RECOMPUTE_DIRS
        if (pl > 3) continue;
#endif
        if (have && (pl != 3 || counted)) v = src[pl * total];  // (the count plane is not written without its channel)
        dst[pl * PT_SHP_TILE_WORDS] = v;
      }
    }
    __syncthreads();
    const int left = K.samples - k0 < PT_SHP_TILE ? K.samples - k0 : PT_SHP_TILE;  // (uniform)
    const unsigned long long *row = tile + threadIdx.x * PT_SHP_ROW;
    for (int kk = 0; kk < left; kk++) {
#ifdef PT_SH_RECOMPUTE_DIRS
      Pcg g;
      pcg_seed(g, K.init_state, seq_i + (unsigned long long)(k0 + kk));
      const V3 d = sh_direction(g);
      const ShBasis b = sh_basis(d.x, d.y, d.z);
#else
      const ShBasis b = sh_basis(__longlong_as_double((long long)row[4 * PT_SHP_TILE_WORDS + kk]),
                                 __longlong_as_double((long long)row[5 * PT_SHP_TILE_WORDS + kk]),
                                 __longlong_as_double((long long)row[6 * PT_SHP_TILE_WORDS + kk]));
#endif
      sh_add(cr, b, __longlong_as_double((long long)row[kk]));
      sh_add(cg, b, __longlong_as_double((long long)row[PT_SHP_TILE_WORDS + kk]));
      sh_add(cb, b, __longlong_as_double((long long)row[2 * PT_SHP_TILE_WORDS + kk]));
      count += row[3 * PT_SHP_TILE_WORDS + kk];
    }
    __syncthreads();
    if (K.samples - k0 <= PT_SHP_TILE) break;
  }
  if (i >= n) return;
  double scale = K.scale;
  if (!(act == nullptr || act[i] >= 0)) {  // skipped: zeros and 0, whatever the planes held
    cr = zero;
    cg = zero;
    cb = zero;
    scale = 0.0;
    count = 0ULL;
  }
  double *o = (double *)out + i;
  sh_store(o, n, 0, cr, scale);
  sh_store(o, n, 1, cg, scale);
  sh_store(o, n, 2, cb, scale);
  if (counted) ((unsigned long long *)o)[27 * n] = count;
}

// ---- the evaluation: one record per lane; no scene, no ray ---------------------------------------------------------------------
// out_r[ch] = (((0 + (A_0 * Y_0(n_r)) * c_p[0][ch]) + (A_1 * Y_1(n_r)) * c_p[1][ch]) + ... ); an index outside [0, n): zeros.
__global__ __launch_bounds__(PT_BLOCK) void pt_sh_eval_kernel(const double *__restrict__ coeffs, long long n, const int *__restrict__ index,
                                                              const double *__restrict__ dirs, long long m, int kind, double *__restrict__ out) {
  const long long r = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (r >= m) return;
  const long long p = index ? (long long)index[r] : r;
  double o0 = 0.0, o1 = 0.0, o2 = 0.0;
  if (p >= 0 && p < n) {
    const ShBasis b = sh_basis(dirs[r], dirs[m + r], dirs[2 * m + r]);
    const double a1 = kind == PT_SH_HEMISPHERE ? 2.0 / 3.0 : 1.0, a2 = kind == PT_SH_HEMISPHERE ? 0.25 : 1.0;
    const double w[9] = {1.0 * b.y0, a1 * b.y1, a1 * b.y2, a1 * b.y3, a2 * b.y4, a2 * b.y5, a2 * b.y6, a2 * b.y7, a2 * b.y8};
    const double *c = coeffs + p;
#pragma unroll
    for (int j = 0; j < 9; j++) {
      o0 = o0 + w[j] * c[(3 * j + 0) * n];
      o1 = o1 + w[j] * c[(3 * j + 1) * n];
      o2 = o2 + w[j] * c[(3 * j + 2) * n];
    }
  }
  out[r] = o0;
  out[m + r] = o1;
  out[2 * m + r] = o2;
}
