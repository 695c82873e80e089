// pt_hits.h -- hit-record frames: World.ray_intersection for every primary ray of a frame, written out as planes.
// A part of pt_kernels.h (which includes the parts in order: each relies on the ones before it); not a header of its own.
//
// What it restates: the loop of ImageTracer.fire_all_rays (imagetracer.py:60-110) with `func` cut off after its first
// line -- `hit = self.world.ray_intersection(ray)` (world.py:51-69; render.py:52, 65, 103, 158 all start there) -- and
// the HitRecord (hitrecord.py:27-46) stored instead of a colour: include/ptrace.h, pt_render_hits.
//
// Built from the pieces pt_tile_kernel is built from, and from nothing else: 8x8 tiles, one wave per tile; tile_cone /
// cone_keeps / plane_keeps into this wave's LDS survivor masks; world_query_tile<false, HIER, !ORTHO> (closest hit);
// primary_ray; hit_details for the winner.  So every value comes from the same operations in the same order as the
// renderers' (a Flat frame recomputed from these planes equals pt_render's, tests/test_gpu_hits.py), and culling is
// invisible for the same reason it is there.  What is NOT here: the dome shortcut (a record needs its point, so every
// ray is traced) and the path tracer's flagging.
//   HIER   worlds of more than 256 shapes: the tile culls its 32x32 cell's list (pt_cell_kernel runs first)
//   ORTHO  orthogonal camera: a beam instead of a cone, nothing hoisted
//   CULL   false (the switch cull = 0, and worlds of fewer than four shapes): every shape goes through world_query --
//          the same tiles and stores, which makes it the on-device A/B for "culling is invisible"
// Stores: planes are [sample][local row][column], so the 8 lanes of a tile row write 8 consecutive values of a plane
// (64 B runs of fp64, 32 B of the int32 shape plane), one plain vector store per selected component and sample.  A
// channel that is not selected costs nothing: `channels` is wave-uniform, its tests are scalar branches, and
// hit_details is told need_uv only with PT_HIT_UV (pt_atan2 / pt_acos stay behind their calls either way).
template <bool HIER, bool ORTHO, bool CULL>
__global__ __launch_bounds__(PT_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 8))) void pt_hits_kernel(const PtKArgs a, int channels) {
  int S, W, rows_local, npass;
  {
    pt_kargs c = cold_args(a);
    S = c->S;
    W = c->W;
    rows_local = c->rows_local;
    npass = c->npass;
  }
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int mbase = wib * npass;  // this wave's slice of pt_lds_masks
  const int nsamp = S > 0 ? S * S : 1;
  const int tiles_x = (W + 7) >> 3, tiles_y = (rows_local + 7) >> 3;
  const int ntiles = tiles_x * tiles_y;
  // the buffer: int32 shape plane (padded to 8 bytes), then the selected fp64 planes in bit order (include/ptrace.h)
  const long long plane = (long long)nsamp * rows_local * W;  // values per plane
  int *const shape_out = (int *)a.out;
  double *const planes = (double *)((char *)a.out + ((plane * 4 + 7) & ~7LL));
  const bool need_uv = (channels & PT_HIT_UV) != 0;
  unsigned long long nrays = 0;
  for (int tile = blockIdx.x * (PT_BLOCK / 64) + wib; tile < ntiles; tile += gridDim.x * (PT_BLOCK / 64)) {
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int col = tx * 8 + (lane & 7), lrow = ty * 8 + (lane >> 3);
    const bool active = col < W && lrow < rows_local;
    // clamp so that idle lanes of edge tiles stand on a real pixel (they only widen nothing)
    const int pcol = col < W ? col : W - 1, clrow = lrow < rows_local ? lrow : rows_local - 1;
    const int grow = global_row(a, clrow);
    int tpass = npass;
    const unsigned int *list = nullptr;
    if (CULL) {
      // ---- cull: one bounding sphere per lane per pass -> ballot -> LDS (as pt_tile_kernel) ----
      const int gr0 = global_row(a, ty * 8);
      const int gr1 = global_row(a, (ty * 8 + 7 < rows_local) ? ty * 8 + 7 : rows_local - 1);
      const TileCone tc = tile_cone(a, tx * 8, (tx * 8 + 8 < W) ? tx * 8 + 8 : W, gr0, gr1);
      if (HIER) {
        // the tile's 8 rows are consecutive global rows starting at a multiple of 8 (the plan checks row_block % 8 == 0)
        const int cell = __builtin_amdgcn_readfirstlane((gr0 / PT_CELL) * a.cells_x + (tx * 8) / PT_CELL);
        const int cnt = PT_KI(a.cell_count)[cell];
        list = a.cell_list + (size_t)cell * a.cell_stride;
        tpass = (cnt + 63) >> 6;
        for (int p = 0; p < tpass; ++p) {
          const int idx = p * 64 + lane;
          bool keep = false;
          int slot = 0;
          float4 b = {0.0f, 0.0f, 0.0f, -1.0f};
          if (idx < cnt) {
            slot = (int)list[idx];
            b = a.bounds[slot];
          }
          const bool isplane = idx < cnt && slot >= a.n_spheres;
          if (idx < cnt && !isplane) keep = cone_keeps(tc, b);
          if (__any(isplane)) {
            const bool pk = plane_keeps(tc, b, isplane);
            if (isplane) keep = pk;
          }
          const unsigned long long m = __ballot(keep);
          if (lane == 0) pt_lds_masks[mbase + p] = m;
        }
      } else {
        for (int p = 0; p < npass; ++p) {
          const int slot = p * 64 + lane;
          bool keep = false;
          float4 b = {0.0f, 0.0f, 0.0f, -1.0f};
          if (slot < a.n_shapes) b = a.bounds[slot];  // 16 B per lane, coalesced
          const bool isplane = slot >= a.n_spheres && slot < a.n_shapes;
          if (slot < a.n_spheres) keep = cone_keeps(tc, b);
          if (__any(isplane)) {
            const bool pk = plane_keeps(tc, b, isplane);
            if (isplane) keep = pk;
          }
          const unsigned long long m = __ballot(keep);
          if (lane == 0) pt_lds_masks[mbase + p] = m;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    Pcg pcg;
    unsigned long long gpix = 0;
    if (S > 0) {
      pt_kargs c = cold_args(a);
      gpix = (unsigned long long)grow * c->W + pcol;
      pcg_seed_pixel(pcg, c->pcg_mode, c->s0, c->q0, gpix, nsamp);
    }
    for (int s = 0; s < nsamp; ++s) {
      double up = 0.5, vp = 0.5;
      if (S > 0) {  // imagetracer.py:86-93: u drawn first, then v; sub_row outer, sub_col inner
        pt_kargs c = cold_args(a);
        if (c->pcg_mode == PT_PCG_SAMPLE) pcg_seed(pcg, c->s0, c->q0 + gpix * (unsigned)nsamp + (unsigned)s);
        const int sr = s / S, sc = s - sr * S;
        up = ((double)sc + pcg_float(pcg)) / (double)S;
        vp = ((double)sr + pcg_float(pcg)) / (double)S;
      }
      const Ray ray = primary_ray(a, pcol, grow, up, vp);
      double best_t;
      int hit;
      if (CULL)
        hit = world_query_tile<false, HIER, !ORTHO>(a, ray, mbase, tpass, best_t, active, list);
      else
        hit = world_query<false, !ORTHO>(a, ray, INFINITY, best_t, active);
      // world.py:51-69: None -> shape -1, t = +inf, zeros; else the winner's record, its normal normalised
      Hit h;
      h.wp = {0.0, 0.0, 0.0};
      h.n = {0.0, 0.0, 0.0};
      h.u = 0.0;
      h.v = 0.0;
      int index = -1;
      if (hit >= 0) {
        hit_details(a.recs + hit, cold_args(a)->aux + hit, ray, best_t, h, need_uv);
        index = a.recs[hit].index;
      }
      if (active) {
        nrays++;
        const long long at = ((long long)s * rows_local + lrow) * W + col;
        shape_out[at] = index;
        double *o = planes + at;
        if (channels & PT_HIT_T) {
          o[0] = best_t;  // (world_query* leave +inf where nothing was hit)
          o += plane;
        }
        if (channels & PT_HIT_POINT) {
          o[0] = h.wp.x;
          o[plane] = h.wp.y;
          o[2 * plane] = h.wp.z;
          o += 3 * plane;
        }
        if (channels & PT_HIT_NORMAL) {
          o[0] = h.n.x;
          o[plane] = h.n.y;
          o[2 * plane] = h.n.z;
          o += 3 * plane;
        }
        if (channels & PT_HIT_UV) {
          o[0] = h.u;
          o[plane] = h.v;
          o += 2 * plane;
        }
        if (channels & PT_HIT_RAY) {
          o[0] = ray.o.x;
          o[plane] = ray.o.y;
          o[2 * plane] = ray.o.z;
          o[3 * plane] = ray.d.x;
          o[4 * plane] = ray.d.y;
          o[5 * plane] = ray.d.z;
        }
      }
    }
    if (CULL) __builtin_amdgcn_wave_barrier();  // the next tile overwrites this wave's mask slice
  }
  add_ray_count(a, nrays);
}
