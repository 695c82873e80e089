// pt_adaptive.h -- the kernels of include/ptrace_adaptive.h: sample counts from a variance plane, their prefix sum, and the gather
// whose sample count is a plane.  Included by ptrace_adaptive.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h,
// pt_shade.h): nothing here is part of the other twelve libraries.
//
// What it restates: the walk of a sample is the walk of the gather query's device header, operation for operation -- PCG(init_state,
// seq_i + k) (pcg_seed), DiffuseBRDF.scatter_ray at (p_i, n_i) (scatter_ray<true>), then the recursion of render.py:99-139 as a loop
// over an explicit node stack, depth-first in the reference's order of draws -- restated here on purpose, as that header restates
// pt_radiance.h's (each belongs to its one translation unit).  What differs is where a lane's (record, sample) comes from and how
// long a record's row of samples is; L_ik is the same function of (p_i, n_i, generator) in every bit.
//
// The walk ends by integer counters alone: a node is pushed only while sp < levels (<= 64), every node spawns its `left` children
// and no more, a wave's outer loop advances its sample index by the launch's lane count, and both searches below halve or
// 64-th an integer span.  No floating-point value decides whether a lane loops again.
//
// FINDING A SAMPLE'S RECORD.  Sample j belongs to the record i with offsets[i] <= j < offsets[i + 1].  Two ways were on the table: an
// expand launch that writes owner[j] into the workspace first, or a search of `offsets` for the upper bound by the lane that
// walks j.  BOTH are built on one search (ad_find), and the measurement chose: the owner plane is the default, the search inside
// the walk its A/B partner (PTRACE_ADAPTIVE_LOOKUP; profiles/adaptive_kernel.txt, profiles/DROPPED_VARIANTS.md).  What was weighed
// beforehand.  (1) The owner plane costs 4 bytes per sample written and 4 read -- a quarter of what the sample planes themselves
// move -- a launch, and an expand kernel that either runs the same search per j (built) or lets one lane write a whole record's
// row (up to 2^20 uncoalesced stores behind one lane; not built).  (2) The search need not be the
// naive one of log2(n) dependent loads per lane (20 at n = 921 600, each an L2 round trip of some 200 cycles): a wave's 64
// samples are CONSECUTIVE, so the wave searches together.  ad_wave_bounds finds the records of the wave's first and last sample
// by a 64-ary search -- lane l probes offsets[lo + (l + 1) step], one ballot narrows the span 64 times, 4 trips at n = 921 600,
// the two chains in flight together -- and every lane then halves only the span between those two records (2 trips at 16
// samples per record, 6 at one; the probes of a wave fall into a few neighbouring lines).  The probes are per-lane vector loads on
// purpose: they differ per lane, so the scalar cache has nothing to share, and the spans and ballots are wave-uniform by
// value without the compiler having to prove it.  No LDS is needed: the window between the two records is not bounded (zeros
// and negatives take no samples), so a fixed LDS window would need the global fallback anyway.  (3) The search is a chain of
// some eight dependent round trips either way; in the walk it is paid by two waves per SIMD, in the expand kernel (a few
// registers) by eight, and on the MI355X that was worth 1 % of the gather.  Most of what the ragged gather costs beyond the
// uniform one is this chain, in whichever launch it sits (tools/adaptivebench.py times the launches apart).
//
// Work layout: the gather's.  A wave takes samples [base, base + 64) and then the next 64 no other wave of the launch takes.
// The node stack lives in the caller's workspace, planar [level][field][lane]; behind it the sample planes [4][capacity].
//
// The mean: pt_adaptive_mean_kernel, a second launch on the same stream, one record per lane, rows of unequal length staged
// through LDS a tile of 16 samples at a time.  The trip count is the workgroup's largest K_i, which every wave works out for
// itself from the workgroup's 256 counts (four loads per lane and a butterfly) BEFORE the first barrier: it is uniform, every
// wave reaches every barrier, nobody waits for another workgroup.  A lane adds only its own K_i values, in k order.
#pragma once

#define PT_AD_FIELDS_ONE 6
#define PT_AD_FIELDS_MANY 20
#define PT_AD_SAMPLE_PLANES 4
#define PT_AD_SCAN 256  // counts per workgroup of the scan (= PT_BLOCK)

struct PtAdK {
  int N;        // num_of_rays >= 1
  int levels;   // max_depth - depth0: 0 .. 64, or < 0: every sample's ray is deeper than max_depth
  int rr_rel;   // russian_roulette_limit - depth0, clamped into [-1, 65]: the roulette runs where sp >= rr_rel
  int channels;
  double bg[3];
  double invN;  // 1.0 / num_of_rays
  unsigned long long init_state, init_seq;
  unsigned long long lanes;  // threads of the walk's launch = lanes of the node stacks
  long long capacity;        // samples a plane holds = the planes' stride
};

struct PtAdC {
  int min_samples, max_samples;
  double tolerance, luminance_floor, gain;
};

// ---- 1. counts ------------------------------------------------------------------------------------------------------------------
// Color.luminosity with comparisons (lum of include/ptrace_variance.h)
PT_DEV double ad_lum(double c0, double c1, double c2) {
  double mx = c0, mn = c0;
  if (c1 > mx) mx = c1;
  if (c2 > mx) mx = c2;
  if (c1 < mn) mn = c1;
  if (c2 < mn) mn = c2;
  return (mx + mn) / 2.0;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_adaptive_counts_kernel(const double *__restrict__ variance, const double *__restrict__ colour,
                                                                      const int *__restrict__ shape, long long m, const PtAdC C,
                                                                      int *__restrict__ counts) {
  const long long p = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (p >= m) return;
  int out = 0;
  if (shape[p] >= 0) {
    const double v = variance[p];
    double l = ad_lum(colour[p], colour[m + p], colour[2 * m + p]);
    if (!(l > C.luminance_floor)) l = C.luminance_floor;
    const double tl = C.tolerance * l;
    const double want = (C.gain * v) / (tl * tl);
    if (!(v >= 0.0)) {
      out = C.max_samples;
    } else if (!(want < (double)C.max_samples)) {
      out = C.max_samples;
    } else {
      const long long t = (long long)want;  // (0 <= want < 2^20)
      long long k = t + ((double)t < want ? 1 : 0);
      if (k < C.min_samples) k = C.min_samples;
      out = (int)k;
    }
  }
  counts[p] = out;
}

// ---- 2. offsets: reduce, then scan ------------------------------------------------------------------------------------------------
// The exclusive scan of one value per thread over a workgroup of 256, in LDS (two buffers of 256, eight doubling steps); `total` is
// the workgroup's sum.  Every thread of the workgroup calls it.
PT_DEV long long ad_block_scan(long long v, long long *lds, long long &total) {
  const int t = (int)threadIdx.x;
  int cur = 0;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < PT_AD_SCAN; d <<= 1) {
    long long x = lds[cur * PT_AD_SCAN + t];
    if (t >= d) x += lds[cur * PT_AD_SCAN + t - d];
    lds[(cur ^ 1) * PT_AD_SCAN + t] = x;
    __syncthreads();
    cur ^= 1;
  }
  const long long incl = lds[cur * PT_AD_SCAN + t];
  total = lds[cur * PT_AD_SCAN + PT_AD_SCAN - 1];
  __syncthreads();  // (the buffers are free again)
  return incl - v;
}

PT_DEV long long ad_count_at(const int *__restrict__ counts, long long n, long long i) {
  if (i >= n) return 0;
  const int c = counts[i];
  return c > 0 ? (long long)c : 0;
}

// launch 1: sums[b] = the sum of workgroup b's 256 counts
__global__ __launch_bounds__(PT_BLOCK) void pt_adaptive_sums_kernel(const int *__restrict__ counts, long long n, long long *__restrict__ sums) {
  __shared__ long long lds[2 * PT_AD_SCAN];
  long long total;
  ad_block_scan(ad_count_at(counts, n, (long long)blockIdx.x * PT_AD_SCAN + threadIdx.x), lds, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// launch 2, ONE workgroup: sums becomes its own exclusive scan, 256 at a time with a carry (the trip count is nb's alone)
__global__ __launch_bounds__(PT_BLOCK) void pt_adaptive_scan_sums_kernel(long long *__restrict__ sums, long long nb) {
  __shared__ long long lds[2 * PT_AD_SCAN];
  long long carry = 0;
  for (long long c = 0; c < nb; c += PT_AD_SCAN) {
    const long long b = c + threadIdx.x;
    long long total;
    const long long ex = ad_block_scan(b < nb ? sums[b] : 0, lds, total);
    if (b < nb) sums[b] = carry + ex;
    carry += total;
  }
}

// launch 3: offsets[i] = sums[workgroup] + the exclusive scan inside the workgroup; the last record's thread writes the total
__global__ __launch_bounds__(PT_BLOCK) void pt_adaptive_offsets_kernel(const int *__restrict__ counts, long long n, const long long *__restrict__ sums,
                                                                       long long *__restrict__ offsets) {
  __shared__ long long lds[2 * PT_AD_SCAN];
  const long long i = (long long)blockIdx.x * PT_AD_SCAN + threadIdx.x;
  const long long v = ad_count_at(counts, n, i);
  long long total;
  const long long ex = ad_block_scan(v, lds, total);
  if (i >= n) return;
  const long long at = sums[blockIdx.x] + ex;
  offsets[i] = at;
  if (i == n - 1) offsets[n] = at + v;
}

// ---- 3. the ragged gather -----------------------------------------------------------------------------------------------------------
// materials.py:70-82 for a (u, v) nobody vouches for: not >= 0 -> 0, >= w -> w - 1, else int()'s truncation
PT_DEV long long ad_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}
template <typename CP>
PT_DEV V3 ad_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = ad_texel(u, w), row = ad_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}

struct AdStack {
  double *p;  // this lane's word of field 0, level 0
  size_t lanes;
  int fields;
  __device__ __forceinline__ double get(int slot, int field) const { return p[((size_t)slot * fields + field) * lanes]; }
  __device__ __forceinline__ void put(int slot, int field, double v) const { p[((size_t)slot * fields + field) * lanes] = v; }
  __device__ __forceinline__ int geti(int slot, int field) const { return (int)__double_as_longlong(get(slot, field)); }
  __device__ __forceinline__ void puti(int slot, int field, int v) const { put(slot, field, __longlong_as_double((long long)v)); }
};

// K_i of the header, from values nobody vouches for: 0 where the offset is not inside [0, capacity]
PT_DEV int ad_taken(int count, long long offset, long long capacity) {
  if (offset < 0 || offset > capacity) return 0;
  const long long room = capacity - offset, c = count > 0 ? count : 0;
  return (int)(c < room ? c : room);
}

// The largest i in [0, n) with off[i] <= t, for t = ta and for t = tb at once (off[0] <= ta <= tb is the caller's; n >= 1).  ALL 64
// lanes of the wave call it with the same arguments.  A span [lo, hi) holds the answer; lane l probes lo + (l + 1) step with step
// = ceil(span / 64); the number of probes that are <= t says which 64th the answer is in.  A span of s becomes one of at most
// ceil(s / 64) < s: integers alone end the loop, whatever the plane holds.
PT_DEV void ad_wave_bounds(const long long *__restrict__ off, long long n, long long ta, long long tb, int lane, long long &ia, long long &ib) {
  long long lo_a = 0, hi_a = n, lo_b = 0, hi_b = n;
  while (hi_a - lo_a > 1 || hi_b - lo_b > 1) {
    const long long step_a = (hi_a - lo_a + 63) >> 6, step_b = (hi_b - lo_b + 63) >> 6;
    const long long pa = lo_a + (lane + 1) * step_a, pb = lo_b + (lane + 1) * step_b;
    const bool in_a = pa < hi_a, in_b = pb < hi_b;
    const long long va = in_a ? off[pa] : 0, vb = in_b ? off[pb] : 0;  // (both loads in flight together)
    const int ca = __popcll(__ballot(in_a && va <= ta)), cb = __popcll(__ballot(in_b && vb <= tb));
    lo_a += ca * step_a;
    lo_b += cb * step_b;
    if (lo_a + step_a < hi_a) hi_a = lo_a + step_a;
    if (lo_b + step_b < hi_b) hi_b = lo_b + step_b;
  }
  ia = lo_a;
  ib = lo_b;
}

// The record of sample j, for the wave whose samples are [base, last] (j = base + lane, or `last` on the lanes behind it): the wave's
// first and last record together, then this lane's between them.  ALL 64 lanes of the wave call it.  -> i in [0, n)
PT_DEV long long ad_find(const long long *__restrict__ off, long long n, long long base, long long last, int lane, long long j) {
  long long lo, hi;
  ad_wave_bounds(off, n, base, last, lane, lo, hi);
  hi = hi + 1;
  while (hi - lo > 1) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The expand launch of the OWNER variant (PTRACE_ADAPTIVE_LOOKUP=owner): owner[j] = the record of sample j, for every j below
// min(offsets[n], capacity), found as the walk finds it -- but by a kernel of a few registers whose many resident waves hide the
// search's round trips, which the walk's two waves per SIMD cannot.
__global__ __launch_bounds__(PT_BLOCK) void pt_adaptive_owner_kernel(const long long *__restrict__ off, long long n, long long capacity,
                                                                     int *__restrict__ owner) {
  const size_t gtid = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  long long total = off[n];
  if (total > capacity) total = capacity;
  const long long stride = (long long)gridDim.x * PT_BLOCK;
  for (long long base = (long long)(gtid & ~(size_t)63); base < total; base += stride) {
    const long long last = base + 63 < total ? base + 63 : total - 1;
    const bool inside = base + lane <= last;
    const long long j = inside ? base + lane : last;
    const long long i = ad_find(off, n, base, last, lane, j);
    if (inside) owner[j] = (int)i;
  }
}

// Every lane of a wave enters the search and the query (they ballot); lanes without a sample pass active = false.  A sample of a
// skipped record writes nothing: the mean does not read it.  OWNER: the record comes from the plane the expand launch wrote.
template <bool MANY, bool OWNER>
__global__ __launch_bounds__(PT_BLOCK) void pt_adaptive_walk_kernel(const PtKArgs a, const double *__restrict__ points,
                                                                    const double *__restrict__ normals, const int *__restrict__ act,
                                                                    const unsigned long long *__restrict__ seq, const int *__restrict__ counts,
                                                                    const long long *__restrict__ off, long long n, const PtAdK K,
                                                                    double *__restrict__ ws, double *__restrict__ samples,
                                                                    const int *__restrict__ owner) {
  const size_t gtid = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  AdStack st;
  st.p = ws + gtid;
  st.lanes = (size_t)K.lanes;
  st.fields = MANY ? PT_AD_FIELDS_MANY : PT_AD_FIELDS_ONE;
  // the samples there are: the total the scan wrote, never more than the planes hold
  long long total = off[n];
  if (total > K.capacity) total = K.capacity;
  const long long first_base = (long long)(gtid & ~(size_t)63);
  // OWNER: the record of this lane's sample of the wave's NEXT turn is requested a turn ahead -- the one load nothing depends
  // on until then -- so that a turn begins with the record's loads, one round trip to memory as in the gather query
  int owner_ahead = 0;
  if (OWNER && first_base + lane < total) owner_ahead = owner[first_base + lane];
  for (long long base = first_base; base < total; base += (long long)K.lanes) {
    const long long last = base + 63 < total ? base + 63 : total - 1;
    const bool inside = base + lane <= last;
    const long long j = inside ? base + lane : last;
    // (i, k) of sample j; i in [0, n) whatever the planes hold
    long long i;
    if (OWNER) {
      i = (long long)owner_ahead;
      i = i < 0 ? 0 : (i < n ? i : n - 1);
      const long long ahead = base + (long long)K.lanes + lane;
      owner_ahead = ahead < total ? owner[ahead] : 0;
    } else {
      i = ad_find(off, n, base, last, lane, j);
    }
    const long long at = off[i];
    const long long kk = j - at;
    const bool mine = inside && kk >= 0 && kk < (long long)ad_taken(counts[i], at, K.capacity);
    const unsigned long long k = (unsigned long long)(mine ? kk : 0);
    const bool active = mine && (act == nullptr || act[i] >= 0);
    // the record, as the scatter query reads one: requested in front of the arithmetic, one round trip to memory
    V3 f_wp = {points[i], points[n + i], points[2 * n + i]};
    V3 f_n = {normals[i], normals[n + i], normals[2 * n + i]};
    V3 f_in = {0.0, 0.0, 1.0};  // (a DiffuseBRDF does not look at the incoming direction)
    int f_brdf = PT_BRDF_DIFFUSE;
    const unsigned long long seq_i = seq ? seq[i] : K.init_seq + (unsigned long long)at;
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
          V3 hc = ad_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, h.u, h.v);
          const V3 em = ad_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, h.u, h.v);
          const double lum = max2(max2(hc.x, hc.y), hc.z);
          bool ended = false;
          if (sp >= K.rr_rel) {  // render.py:116-123
            const double q = max2(0.05, 1.0 - lum);
            if (pcg_float(g) > q) {
              const double kq = 1.0 / (1.0 - q);
              hc.x = hc.x * kq;
              hc.y = hc.y * kq;
              hc.z = hc.z * kq;
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
    if (active) {  // (levels < 0: black and 0, as initialised); j < total <= capacity
      double *o = samples + j;
      o[0] = ret.x;
      o[K.capacity] = ret.y;
      o[2 * K.capacity] = ret.z;
      if (K.channels & PT_ADAPTIVE_COUNT) ((unsigned long long *)o)[3 * K.capacity] = count;
    }
  }
}

// The mean over rows of unequal length.  One record per lane; a workgroup stages the rows of its 256 records through LDS,
// PT_AD_TILE samples of a plane at a time, as the gather's mean does and for its reason (a lane that read its row directly would
// touch a line per load and lose it before its next value): 16 consecutive lanes load 16 consecutive samples of one record, the
// tile is [record][sample] with a row of 17 words, and behind a barrier every lane adds ITS first min(K_i - k0, 16) words in k
// order.  A word with k >= K_r is not loaded (its address may lie outside the planes) and never added.
#define PT_AD_TILE 16
#define PT_AD_ROW (PT_AD_TILE + 1)

template <bool AS_DOUBLE>
__device__ __forceinline__ void ad_stage_and_add(const unsigned long long *__restrict__ plane, unsigned long long *tile, const long long *s_off,
                                                 const int *s_k, long long k0, int mine, double &acc, unsigned long long &cnt) {
  // load: element e = lane + 256 m of the tile is (record e / 16, sample e % 16)
#pragma unroll
  for (int m = 0; m < PT_AD_TILE; m++) {
    const int e = (int)threadIdx.x + PT_BLOCK * m;
    const int r = e / PT_AD_TILE, kk = e % PT_AD_TILE;
    const long long k = k0 + kk;
    unsigned long long v = 0ULL;
    if (k < (long long)s_k[r]) v = plane[s_off[r] + k];  // 0 <= s_off[r], s_off[r] + k < s_off[r] + K_r <= capacity
    tile[r * PT_AD_ROW + kk] = v;
  }
  __syncthreads();
  const long long rest = (long long)mine - k0;
  const int left = rest < PT_AD_TILE ? (int)rest : PT_AD_TILE;  // (<= 0: this lane's row has ended)
  const unsigned long long *row = tile + threadIdx.x * PT_AD_ROW;
  for (int kk = 0; kk < left; kk++) {
    if (AS_DOUBLE)
      acc = acc + __longlong_as_double((long long)row[kk]);
    else
      cnt += row[kk];
  }
  __syncthreads();
}

__global__ __launch_bounds__(PT_BLOCK) void pt_adaptive_mean_kernel(const double *__restrict__ samples, const int *__restrict__ act,
                                                                    const int *__restrict__ counts, const long long *__restrict__ off, long long n,
                                                                    const PtAdK K, void *__restrict__ out) {
  __shared__ unsigned long long tile[PT_BLOCK * PT_AD_ROW];
  __shared__ long long s_off[PT_BLOCK];
  __shared__ int s_k[PT_BLOCK];
  const long long rec0 = (long long)blockIdx.x * PT_BLOCK;
  const long long i = rec0 + threadIdx.x;
  // the trip count: the largest K of the workgroup's records, worked out by every wave for itself -- uniform without a barrier
  int most = 0;
#pragma unroll
  for (int w = 0; w < PT_BLOCK / 64; w++) {
    const long long r = rec0 + (threadIdx.x & 63) + 64 * w;
    const int kr = r < n ? ad_taken(counts[r], off[r], K.capacity) : 0;
    most = kr > most ? kr : most;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int other = __shfl_xor(most, d, 64);
    most = other > most ? other : most;
  }
  const long long at = i < n ? off[i] : 0;
  const int mine = i < n ? ad_taken(counts[i], at, K.capacity) : 0;
  s_off[threadIdx.x] = mine > 0 ? at : 0;
  s_k[threadIdx.x] = mine;
  __syncthreads();
  const unsigned long long *planes = (const unsigned long long *)samples;
  const bool counted = (K.channels & PT_ADAPTIVE_COUNT) != 0;
  double sx = 0.0, sy = 0.0, sz = 0.0, unused = 0.0;
  unsigned long long count = 0ULL, none = 0ULL;
  for (long long k0 = 0; k0 < (long long)most; k0 += PT_AD_TILE) {
    ad_stage_and_add<true>(planes, tile, s_off, s_k, k0, mine, sx, none);
    ad_stage_and_add<true>(planes + K.capacity, tile, s_off, s_k, k0, mine, sy, none);
    ad_stage_and_add<true>(planes + 2 * K.capacity, tile, s_off, s_k, k0, mine, sz, none);
    if (counted) ad_stage_and_add<false>(planes + 3 * K.capacity, tile, s_off, s_k, k0, mine, unused, count);
  }
  if (i >= n) return;
  int taken = mine;
  if ((act == nullptr || act[i] >= 0) && mine > 0) {
    const double invK = 1.0 / (double)mine;
    sx = sx * invK;
    sy = sy * invK;
    sz = sz * invK;
  } else {
    sx = sy = sz = 0.0;
    count = 0ULL;
    if (mine > 0) taken = 0;  // (a skipped record)
  }
  double *o = (double *)out + i;
  o[0] = sx;
  o[n] = sy;
  o[2 * n] = sz;
  char *behind = (char *)out + (size_t)n * 24;
  if (counted) {
    ((unsigned long long *)behind)[i] = count;
    behind += (size_t)n * 8;
  }
  if (K.channels & PT_ADAPTIVE_TAKEN) ((int *)behind)[i] = taken;
}
