// pt_gather.h -- the mean radiance over the hemisphere of a CALLER's surface points (include/ptrace_gather.h).
// Included by ptrace_gather.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h, pt_shade.h): nothing here is
// part of the other five libraries.
//
// What it restates: per sample j = i * K + k of record i, PCG(init_state, seq_i + k) (pcg_seed), DiffuseBRDF.scatter_ray at
// (p_i, n_i) (scatter_ray<true>, as pt_scatter.h calls it for a record), then the recursion of render.py:99-139 for that ray
// as a loop over an explicit node stack, depth-first in the reference's order of draws -- the walk of pt_radiance.h, restated
// here on purpose (that header belongs to its one translation unit).  The arithmetic of a node is the oracle's pathtracer(),
// operation for operation:
//     cum = cum + hc * rad per child, in child order;  emitted + cum * (1.0 / num_of_rays) at the end;
//     emitted alone where the roulette ends the path;  the background on a miss.
// A hit AT max_depth with lum > 0 still scatters num_of_rays times: the generator jumps over those draws, and the children's
// sum is 0.0 + hc * 0.0 once.
//
// What is simpler than pt_radiance.h's walk: EVERY ray that is queried comes out of scatter_ray -- the entry ray too -- so
// tmin > 0 always, tmax is always infinite, and the exhaustive query for entry rays that look backwards is not needed.  The
// entry ray is "child 0 of a node that is not on the stack": the loop starts with a spawn pending, and there is ONE scatter
// site and ONE query site in the kernel.
//
// The walk ends by integer counters alone: a node is pushed only while sp < levels (= max_depth - depth0 <= 64), every node
// spawns its `left` children and no more, and a wave's outer loop advances its sample index by the launch's lane count.  No
// floating-point value decides whether a lane loops again; a ray of NaNs hits nothing and returns the background.
//
// Work layout: a wave takes samples [base, base + 64) -- one record's samples are neighbours, so its lanes mostly share an
// origin, and with num_of_rays = 1 their walks are of similar length -- and then the next 64 that no other wave of the launch
// takes: base += lanes.  The node stack lives in the caller's workspace in HBM, planar [level][field][lane] (fields as in
// pt_radiance.h); behind it the sample planes [4][n * K]: L_ik r, g, b and the sample's count, written by this kernel 8 bytes
// per lane, 512 consecutive bytes per wave.
//
// The mean: pt_gather_mean_kernel, a second launch on the same stream, one lane per record, adds the record's K values in k
// order (staged through LDS, so that the sample planes are read a whole line at a time).  A one-launch design would have to hand partial sums from wave to wave where a record straddles waves or workgroups;
// keeping the order would then make one wave wait for another, which this library never does.  The order is part of the
// interface: no atomics, nothing that depends on scheduling, on n, on K or on the launch's shape.
#pragma once

#define PT_GAT_FIELDS_ONE 6
#define PT_GAT_FIELDS_MANY 20
#define PT_GAT_SAMPLE_PLANES 4

struct PtGatK {
  int samples;  // K >= 1
  int N;        // num_of_rays >= 1
  int levels;   // max_depth - depth0: 0 .. 64, or < 0: every sample's ray is deeper than max_depth
  int rr_rel;   // russian_roulette_limit - depth0, clamped into [-1, 65]: the roulette runs where sp >= rr_rel
  int channels;
  double bg[3];
  double invN;  // 1.0 / num_of_rays
  double invK;  // 1.0 / samples
  unsigned long long init_state, init_seq;
  unsigned long long lanes;  // threads of the walk's launch = lanes of the node stacks
};

// materials.py:70-82 for a (u, v) nobody vouches for (a record's normal may be anything, so may the rays and what they hit):
// not >= 0 -> 0, >= w -> w - 1, else int()'s truncation -- an address inside the texture for every (u, v).
PT_DEV long long gat_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}
template <typename CP>
PT_DEV V3 gat_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = gat_texel(u, w), row = gat_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}

struct GatStack {
  double *p;  // this lane's word of field 0, level 0
  size_t lanes;
  int fields;
  __device__ __forceinline__ double get(int slot, int field) const { return p[((size_t)slot * fields + field) * lanes]; }
  __device__ __forceinline__ void put(int slot, int field, double v) const { p[((size_t)slot * fields + field) * lanes] = v; }
  __device__ __forceinline__ int geti(int slot, int field) const { return (int)__double_as_longlong(get(slot, field)); }
  __device__ __forceinline__ void puti(int slot, int field, int v) const { put(slot, field, __longlong_as_double((long long)v)); }
};

// `total` = n * K <= 2^31 - 1.  Every lane of a wave enters the query (it ballots); lanes without a ray pass active = false.
// A sample of a skipped record writes nothing: the mean does not read it.
template <bool MANY>
__global__ __launch_bounds__(PT_BLOCK) void pt_gather_kernel(const PtKArgs a, const double *__restrict__ points,
                                                             const double *__restrict__ normals, const int *__restrict__ act,
                                                             const unsigned long long *__restrict__ seq, long long n, long long total,
                                                             const PtGatK K, double *__restrict__ ws, double *__restrict__ samples) {
  const size_t gtid = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  GatStack st;
  st.p = ws + gtid;
  st.lanes = (size_t)K.lanes;
  st.fields = MANY ? PT_GAT_FIELDS_MANY : PT_GAT_FIELDS_ONE;
  const long long first_base = (long long)(gtid & ~(size_t)63);
  for (long long base = first_base; base < total; base += (long long)K.lanes) {
    const long long j = base + (long long)(threadIdx.x & 63);
    const bool inside = j < total;
    const long long i = inside ? (long long)((unsigned)j / (unsigned)K.samples) : 0;  // (j < 2^31: a 32-bit division)
    const unsigned long long k = (unsigned long long)(inside ? j - i * K.samples : 0);
    const bool active = inside && (act == nullptr || act[i] >= 0);
    // the record, as the scatter query reads one: requested in front of the arithmetic, one round trip to memory
    V3 f_wp = {points[i], points[n + i], points[2 * n + i]};
    V3 f_n = {normals[i], normals[n + i], normals[2 * n + i]};
    V3 f_in = {0.0, 0.0, 1.0};  // (a DiffuseBRDF does not look at the incoming direction)
    int f_brdf = PT_BRDF_DIFFUSE;
    const unsigned long long seq_i = seq ? seq[i] : K.init_seq + (unsigned long long)i * (unsigned long long)K.samples;
    Pcg g;
    pcg_seed(g, K.init_state, seq_i + k);
    unsigned long long count = 0ULL;
    V3 ret = {0.0, 0.0, 0.0};
    Ray ray;
    ray.o = {0.0, 0.0, 0.0};
    ray.d = {0.0, 0.0, 1.0};
    ray.tmin = 1.0e-3;
    int sp = 0;                              // nodes on this lane's stack = depth of `ray` below the entry ray
    bool spawn = active && K.levels >= 0;    // a scatter_ray is due: the entry ray first (deeper than max_depth -> black, no draw seen)
    while (__ballot(spawn) != 0ULL) {
      // ---- brdf.scatter_ray: the entry ray at (p_i, n_i), or the next child of the node at sp - 1; always at depth sp ----
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
          V3 hc = gat_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, h.u, h.v);
          const V3 em = gat_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, h.u, h.v);
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
    if (active) {  // (levels < 0: black and 0, as initialised)
      double *o = samples + j;
      o[0] = ret.x;
      o[total] = ret.y;
      o[2 * total] = ret.z;
      if (K.channels & PT_GATHER_COUNT) ((unsigned long long *)o)[3 * total] = count;
    }
  }
}

// The mean.  One record per lane: out_i = (((0 + L_i0) + L_i1) + ... + L_i,K-1) * (1.0 / K) per channel, the counts added in the
// same order.  A lane's K values are consecutive in a sample plane, so lanes that read them directly stand K * 8 bytes apart: every
// load of a wave touches 64 lines, and the lines are evicted before the lane comes back for its next value (measured at K = 16:
// 16 times the planes' bytes through the L2, profiles/gather_kernel.txt).  So a workgroup stages the values of its 256
// records through LDS, PT_GAT_TILE samples of a plane at a time: 16 consecutive lanes load one record's 128 consecutive bytes, the
// tile is written as [record][sample] with a row of 17 words (a lane's row starts on its own banks), and behind a barrier every
// lane adds its row in k order.  Every line of the planes is fetched once.  The trip counts depend on K alone, so every wave of a
// workgroup reaches every barrier; nobody waits for another workgroup.  A skipped record's samples were never written: they are
// loaded like the others (inside the planes) and not added.
#define PT_GAT_TILE 16
#define PT_GAT_ROW (PT_GAT_TILE + 1)

template <bool AS_DOUBLE>
__device__ __forceinline__ void gat_stage_and_add(const unsigned long long *__restrict__ plane, unsigned long long *tile, long long rec0,
                                                  long long n, int samples, int k0, double &acc, unsigned long long &cnt) {
  // load: element e = lane + 256 m of the tile is (record e / 16, sample e % 16)
#pragma unroll
  for (int m = 0; m < PT_GAT_TILE; m++) {
    const int e = (int)threadIdx.x + PT_BLOCK * m;
    const int r = e / PT_GAT_TILE, kk = e % PT_GAT_TILE;
    const long long rec = rec0 + r;
    const int k = k0 + kk;
    unsigned long long v = 0ULL;
    if (rec < n && k < samples) v = plane[rec * samples + k];
    tile[r * PT_GAT_ROW + kk] = v;
  }
  __syncthreads();
  const int left = samples - k0 < PT_GAT_TILE ? samples - k0 : PT_GAT_TILE;  // (uniform)
  const unsigned long long *row = tile + threadIdx.x * PT_GAT_ROW;
  for (int kk = 0; kk < left; kk++) {
    if (AS_DOUBLE)
      acc = acc + __longlong_as_double((long long)row[kk]);
    else
      cnt += row[kk];
  }
  __syncthreads();
}

__global__ __launch_bounds__(PT_BLOCK) void pt_gather_mean_kernel(const double *__restrict__ samples, const int *__restrict__ act, long long n,
                                                                  long long total, const PtGatK K, void *__restrict__ out) {
  __shared__ unsigned long long tile[PT_BLOCK * PT_GAT_ROW];
  const long long rec0 = (long long)blockIdx.x * PT_BLOCK;
  const long long i = rec0 + threadIdx.x;
  const unsigned long long *planes = (const unsigned long long *)samples;
  const bool counted = (K.channels & PT_GATHER_COUNT) != 0;
  double sx = 0.0, sy = 0.0, sz = 0.0, unused = 0.0;
  unsigned long long count = 0ULL, none = 0ULL;
  for (int k0 = 0; k0 < K.samples; k0 += PT_GAT_TILE) {  // (K <= 2^31 - 1, and k0 stops at the last tile: no overflow below)
    gat_stage_and_add<true>(planes, tile, rec0, n, K.samples, k0, sx, none);
    gat_stage_and_add<true>(planes + total, tile, rec0, n, K.samples, k0, sy, none);
    gat_stage_and_add<true>(planes + 2 * total, tile, rec0, n, K.samples, k0, sz, none);
    if (counted) gat_stage_and_add<false>(planes + 3 * total, tile, rec0, n, K.samples, k0, unused, count);
    if (K.samples - k0 <= PT_GAT_TILE) break;
  }
  if (i >= n) return;
  if (act == nullptr || act[i] >= 0) {
    sx = sx * K.invK;
    sy = sy * K.invK;
    sz = sz * K.invK;
  } else {
    sx = sy = sz = 0.0;
    count = 0ULL;
  }
  double *o = (double *)out + i;
  o[0] = sx;
  o[n] = sy;
  o[2 * n] = sz;
  if (counted) ((unsigned long long *)o)[3 * n] = count;
}
