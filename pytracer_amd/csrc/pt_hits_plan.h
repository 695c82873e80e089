// pt_hits_plan.h -- what a hit-record frame (pt_render_hits, include/ptrace.h) WILL launch: a pure host function like
// pt_make_plan (pt_plan.h), and the names of its kernels.  pt_debug_plan_hits (include/ptrace_debug.h) runs it for a
// scene DESCRIPTION on any machine.
//
// The hit-record kernel is pt_tile_kernel's 8x8-tile machinery with records stored instead of colours (pt_hits.h), so its
// culling mode is chosen from the same scene facts by the same function: the plan of a Flat frame that may not take the
// 16x16 tiles (four pixels per lane suit one colour per pixel, not fifteen planes per sample).  No switch of its own: it
// reads cull, levels_min, hier_min, tile_wg_per_cu and the grid switches like every other frame.
#pragma once
#include "pt_plan.h"

static inline void pt_make_hits_plan(const PtSceneFacts &s, const pt_camera *cam, const pt_params *p, const PtTuning &t, PtPlan &pl,
                                     bool &cull) {
  pt_params q = *p;
  q.renderer = PT_RENDERER_FLAT;
  q.out_format = PT_OUT_F64;
  PtTuning tt = t;
  tt.tile4 = 0;
  pt_make_plan(s, cam, &q, tt, pl);
  cull = pl.tile;  // (worlds of at least four shapes unless cull = 0; then plain / HIER / ORTHO as pl.tile_mode says)
  if (pl.npix == 0) return;
  if (!cull) {  // the same tiles, every shape through world_query: no masks in LDS, no cell lists
    const long long cap = t.tile_wg_per_cu > 0 ? (long long)s.n_cu * t.tile_wg_per_cu : (long long)s.n_cu * 8;
    const long long wave_tiles = (long long)((p->width + 7) / 8) * ((pl.rows + 7) / 8);
    pl.grid = (int)std::max<long long>(1, std::min<long long>((wave_tiles + 3) / 4, cap));
    pl.nthreads = pl.grid * PT_PLAN_BLOCK;
    pl.lds_main = 0;
  }
  pl.kernel = PT_KERNEL_HITS;
}

// which: 0 = pre-pass (pt_cell_kernel), 2 = the render kernel; the variant spelled out as pt_plan_kernel_name does
static inline const char *pt_hits_kernel_name(const PtPlan &pl, bool cull, int which, char *buf, size_t n) {
  buf[0] = 0;
  if (pl.npix == 0) return buf;
  if (which == 0) {
    if (cull && pl.hier) snprintf(buf, n, "pt_cell_kernel");
  } else if (which == 2) {
    if (!cull)
      snprintf(buf, n, "pt_hits_kernel<%snoCULL>", pl.ortho ? "ORTHO, " : "");
    else if (pl.tile_mode == PT_TILE_HIER)
      snprintf(buf, n, "pt_hits_kernel<HIER>");
    else if (pl.tile_mode == PT_TILE_ORTHO)
      snprintf(buf, n, "pt_hits_kernel<ORTHO>");
    else
      snprintf(buf, n, "pt_hits_kernel");
  }
  return buf;
}
