// pt_scatter.h -- BRDF.scatter_ray and the Russian roulette for a CALLER's hit records (include/ptrace_scatter.h).
// Included by ptrace_scatter.hip only, behind pt_kernels.h's query parts (pt_math.h, pt_query.h, pt_shade.h): nothing here is
// part of the other three libraries.
//
// What it restates: render.py:107-134 for one child of a hit, exactly as pt_path.h's path_shade_hit and path_trace have it --
// pigments, lum = max2(max2(r, g), b), the roulette's one draw, scatter_ray<true> (the inlined sincos of the fused second
// pass) -- for records that arrive in planes and a generator that arrives with them.  The look-up of a record nobody vouches
// for (slot table, texel clamp) is pt_surface.h's, restated under names of its own: that header belongs to its one
// translation unit.
#pragma once

// materials.py:70-82 for a (u, v) that may be negative, huge or NaN: not >= 0 -> 0, >= w -> w - 1, else int()'s truncation.
PT_DEV long long scat_texel(double x, int w) {
  const double f = x * (double)w;
  if (!(f >= 0.0)) return 0;
  if (f >= (double)w) return (long long)w - 1;
  return (long long)f;
}

template <typename CP>
PT_DEV V3 scat_pigment_color(const PtKArgs &a, int kind, CP c1, CP c2, double steps, int tex, double u, double v) {
  if (kind == PT_PIGMENT_IMAGE) {
    pt_kargs ca = cold_args(a);
    const PtTex *tx = ca->tex + tex;
    const int w = tx->w, hh = tx->h;
    const long long col = scat_texel(u, w), row = scat_texel(v, hh);
    const double *c = ca->tex_data + tx->offset + (row * w + col) * 3;
    V3 r = {c[0], c[1], c[2]};
    return r;
  }
  return pigment_color(a, kind, c1, c2, steps, tex, u, v);  // uniform, checkered: no address is formed from (u, v)
}

// World.shapes index -> grouped slot, or -1: an index outside [0, n_shapes) is "no hit", and so is a table entry that does
// not name a record (the table is the caller's memory).
PT_DEV int scat_slot(const PtKArgs &a, const int *__restrict__ slots, int index) {
  if ((unsigned)index >= (unsigned)a.n_shapes) return -1;
  const int s = slots[index];
  return ((unsigned)s < (unsigned)a.n_shapes) ? s : -1;
}

// the host form's own slot table: slots[recs[s].index] = s (`index` is a permutation of 0 .. n_shapes - 1)
__global__ __launch_bounds__(PT_BLOCK) void pt_scatter_slots_kernel(const PtKArgs a, int *__restrict__ slots) {
  const int s = blockIdx.x * PT_BLOCK + threadIdx.x;
  if (s >= a.n_shapes) return;
  const int index = a.recs[s].index;
  if ((unsigned)index < (unsigned)a.n_shapes) slots[index] = s;
}

// One record per lane; a plane is read and written 8 bytes per lane, 512 consecutive bytes per wave (the int32 planes: 256).
// A streaming kernel: 112 B in (the slot table's entry included), 84 B + 24 B per selected channel out, and between them two
// pigments, at most three draws, two square roots and one sincos.  `roulette` and `channels` are wave-uniform.  A lane without
// a hit reads its shape index and its generator and nothing else; the two BRDF branches are scatter_ray's own, so a mixed wave
// runs each of them once.
__global__ __launch_bounds__(PT_BLOCK) void pt_scatter_kernel(const PtKArgs a, const int *__restrict__ slots, const int *__restrict__ shape,
                                                              const double *__restrict__ point, const double *__restrict__ normal,
                                                              const double *__restrict__ uv, const double *__restrict__ dir,
                                                              const unsigned long long *__restrict__ pcg_state,
                                                              const unsigned long long *__restrict__ pcg_inc, long long n, int roulette,
                                                              int channels, void *__restrict__ out) {
  const long long i = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int slot = scat_slot(a, slots, shape[i]);
  Pcg g;
  g.state = pcg_state[i];
  g.inc = pcg_inc[i];
  g.n = 0;
  int status = -1;
  // the dead ray (include/ptrace_scatter.h): finite, ordinary, and its interval (0, 0) holds no root
  Ray r;
  r.o = {0.0, 0.0, 0.0};
  r.d = {0.0, 0.0, 1.0};
  r.tmin = 0.0;
  double tmax = 0.0;
  V3 hc = {0.0, 0.0, 0.0}, em = {0.0, 0.0, 0.0};
  if (slot >= 0) {
    // (every plane of the record is requested here, in front of the arithmetic: one round trip to memory, not three)
    const double u = uv[i], v = uv[n + i];
    const V3 wp = {point[i], point[n + i], point[2 * n + i]};
    const V3 nrm = {normal[i], normal[n + i], normal[2 * n + i]};
    const V3 in = {dir[i], dir[n + i], dir[2 * n + i]};
    const PtShapeAux *ax = a.aux + slot;
    hc = scat_pigment_color(a, ax->pig_kind, &ax->pig_c1[0], &ax->pig_c2[0], ax->pig_steps, ax->pig_tex, u, v);  // render.py:107-109
    em = scat_pigment_color(a, ax->emi_kind, &ax->emi_c1[0], &ax->emi_c2[0], ax->emi_steps, ax->emi_tex, u, v);
    const double lum = max2(max2(hc.x, hc.y), hc.z);
    bool alive = true;
    if (roulette) {  // render.py:116-123
      const double q = max2(0.05, 1.0 - lum);
      if (pcg_float(g) > q) {
        const double k = 1.0 / (1.0 - q);
        hc.x = hc.x * k;
        hc.y = hc.y * k;
        hc.z = hc.z * k;
      } else {
        alive = false;
      }
    }
    status = 0;
    if (alive && lum > 0.0) {  // render.py:126-134, one child
      r = scatter_ray<true>(ax->brdf_kind, g, in, wp, nrm);
      tmax = INFINITY;
      status = 1;
    }
  }
  ((int *)out)[i] = status;
  double *o = (double *)((char *)out + ((n * 4 + 7) & ~7LL)) + i;
  o[0] = r.o.x;
  o[n] = r.o.y;
  o[2 * n] = r.o.z;
  o[3 * n] = r.d.x;
  o[4 * n] = r.d.y;
  o[5 * n] = r.d.z;
  o[6 * n] = r.tmin;
  o[7 * n] = tmax;
  unsigned long long *po = (unsigned long long *)(o + 8 * n);
  po[0] = g.state;
  po[n] = g.inc;
  o += 10 * n;
  if (channels & PT_SCAT_WEIGHT) {
    o[0] = hc.x;
    o[n] = hc.y;
    o[2 * n] = hc.z;
    o += 3 * n;
  }
  if (channels & PT_SCAT_EMITTED) {
    o[0] = em.x;
    o[n] = em.y;
    o[2 * n] = em.z;
  }
}
