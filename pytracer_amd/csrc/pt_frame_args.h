// pt_frame_args.h — the kernels' argument block (PtKArgs, pt_layout.h) as far as it is made of HOST values: the scene's
// scalars, the camera, the frame's parameters and what the plan decided.  Pure host functions like pt_plan.h's (no HIP call,
// no environment, no global; every function static inline), so what a frame hands its kernels can be read off on any machine:
// tests/frame_args/frame_args_probe.cpp prints the blocks, tests/test_frame_args.py checks them against the formulas below.
// Pointers (tables, workspace, output) and the queue parity are the handle's and stay with ptrace.hip.
#pragma once
#include <cstring>
#include <vector>

#include "../../include/ptrace.h"
#include "pt_layout.h"
#include "pt_plan.h"
#include "pt_scene_build.h"

// ---- the scene -----------------------------------------------------------------------------------------------------------
// how many records the shapes' tables hold: [scale+translate spheres | other spheres | planes]
static inline void pt_fill_shape_counts(PtKArgs &a, const PtSceneScalars &sc) {
  a.n_shapes = sc.n_shapes;
  a.n_spheres = sc.n_spheres;
  a.n_diag = sc.n_diag;
}

// every scalar the kernels read of the analysis (the tables' pointers: fill_scene_args of ptrace.hip)
static inline void pt_fill_scene_scalars(PtKArgs &a, const PtSceneScalars &sc, const PtTuning &tn) {
  a.bs_stride = sc.bs_stride;
  for (int q = 0; q < 3; ++q) a.bs_rmax[q] = sc.bs_rmax[q];
  a.gs_stride = sc.gs_stride;
  a.cs_stride = sc.cs_stride;
  a.bs_levels = sc.bs_levels && sc.n_spheres >= tn.levels_min;
  a.grid_n_always = sc.grid_n_always;
  a.grid_far_eo = sc.grid_far_eo;
  a.grid_occ_lds = -1;
  a.scene_lds = -1;
  for (int q = 0; q < 3; ++q) {
    a.grid_res[q] = sc.grid_res[q];
    a.grid_min[q] = sc.grid_min[q];
    a.grid_max[q] = sc.grid_max[q];
    a.grid_cell[q] = sc.grid_cell[q];
    a.grid_inv[q] = sc.grid_inv[q];
  }
  pt_fill_shape_counts(a, sc);
  a.n_lights = sc.n_lights;
}

// ---- the camera ----------------------------------------------------------------------------------------------------------
// camera.py, as primary_ray reads it, and the image it is aimed through
static inline void pt_fill_camera(PtKArgs &a, const pt_camera *cam, int width, int height) {
  a.cam_kind = cam->kind;
  memcpy(a.cam_m, cam->m, sizeof a.cam_m);
  a.cam_dist = cam->screen_distance;
  a.cam_aspect = cam->aspect_ratio;
  a.W = width;
  a.H = height;
}

// The fp32 model of the primary rays that the culling cones are built from (tile_cone, pixel_cone):
// camera.py:116-124 + imagetracer.py:56-58 folded into d(x, y) = d0 + x * dx + y * dy (perspective: directions,
// common origin in `apex`; orthogonal, camera.py:59-78: the same affine model describes the ORIGINS and the
// "apex" slot carries the common direction).
static inline void fill_cone_model(PtKArgs &a, const pt_camera *cam, int width, int height) {
  const double *m = cam->m, dist = cam->screen_distance, asp = cam->aspect_ratio;
  for (int r = 0; r < 3; ++r) {
    a.cone_d0[r] = (float)(m[r * 4 + 0] * dist + m[r * 4 + 1] * asp + m[r * 4 + 2]);
    a.cone_dx[r] = (float)(m[r * 4 + 1] * (-2.0 * asp / width));
    a.cone_dy[r] = (float)(m[r * 4 + 2] * (-2.0 / height));
    a.cone_apex[r] = (float)(m[r * 4 + 0] * -dist + m[r * 4 + 3]);
    if (cam->kind != PT_CAMERA_PERSPECTIVE) {
      a.cone_d0[r] = (float)(-m[r * 4 + 0] + m[r * 4 + 1] * asp + m[r * 4 + 2] + m[r * 4 + 3]);
      a.cone_apex[r] = (float)m[r * 4 + 0];
    }
  }
  a.cam_kind = cam->kind;
}

// camera.py:116-124: origin (-d, 0, 0) through the camera transformation, reference order -- what pt_prep_hoist builds the
// per-shape constants of the primary rays from, bit for bit (the zero products stay: they decide signed zeros and NaNs)
static inline void pt_hoist_origin(const pt_camera *cam, double w[3]) {
  const struct { double x, y, z; } o = {-cam->screen_distance, 0.0, 0.0};
  w[0] = o.x * cam->m[0] + o.y * cam->m[1] + o.z * cam->m[2] + cam->m[3];
  w[1] = o.x * cam->m[4] + o.y * cam->m[5] + o.z * cam->m[6] + cam->m[7];
  w[2] = o.x * cam->m[8] + o.y * cam->m[9] + o.z * cam->m[10] + cam->m[11];
}

// The sphere the camera is deepest inside (object-space |o'|^2 - 1 most negative, and below -0.5), or -1: the first pass
// settles, per pixel, what can only hit that sphere (pt_tile_kernel re-checks every condition from the exact hoisted
// constants; this only names the candidate).
static inline int pt_dome_slot(const std::vector<PtDomeCand> &dome_cands, const pt_camera *cam, const PtPlan &pl, const PtTuning &tn) {
  int slot = -1;
  if (!pl.ortho && tn.pixel_dome) {
    const double ox = -cam->screen_distance * cam->m[0] + cam->m[3], oy = -cam->screen_distance * cam->m[4] + cam->m[7],
                 oz = -cam->screen_distance * cam->m[8] + cam->m[11];
    double best = -0.5;
    for (const auto &dc : dome_cands) {
      const double *m = dc.invm;
      const double px = ox * m[0] + oy * m[1] + oz * m[2] + m[3], py = ox * m[4] + oy * m[5] + oz * m[6] + m[7],
                   pz = ox * m[8] + oy * m[9] + oz * m[10] + m[11];
      const double c = px * px + py * py + pz * pz - 1.0;
      if (c < best) {
        best = c;
        slot = dc.slot;
      }
    }
  }
  return slot;
}

// ---- the frame -----------------------------------------------------------------------------------------------------------
// Every host value of a frame's block, over a block that holds the scene (fill_scene_args): the camera, pt_params as the
// kernels take them, and what the plan decided, copied (nothing is decided here: pt_plan.h).  A frame that launches nothing
// (pl.npix == 0, pl.zero_frame) gets the same block; nobody reads it.
static inline void pt_fill_frame_args(PtKArgs &a, const pt_camera *cam, const pt_params *p, const PtPlan &pl, const PtTuning &tn,
                                      bool dome_shortcut, const std::vector<PtDomeCand> &dome_cands) {
  a.dome_shortcut = dome_shortcut ? 1 : 0;
  pt_fill_camera(a, cam, p->width, p->height);
  fill_cone_model(a, cam, p->width, p->height);
  a.S = p->samples_per_side;
  a.N = p->num_of_rays;
  a.D = p->max_depth;
  a.rr = p->rr_limit;
  a.pcg_mode = p->pcg_mode;
  a.s0 = p->path_state;
  a.q0 = p->path_seq;
  if (p->pcg_mode == PT_PCG_SEQ) {  // (OnOff / Flat / PointLight only: check_params)
    if (p->samples_per_side > 0) {  // the jitter stream of the reference's ImageTracer, entered by jump-ahead per pixel
      a.s0 = p->jitter_state;
      a.q0 = p->jitter_seq;
    } else {
      a.pcg_mode = PT_PCG_PIXEL;  // pixel-centre rays: no random number is drawn, the alignments coincide
    }
  }
  a.row_block = p->row_block > 0 ? p->row_block : 1;
  a.n_ranks = p->n_ranks > 0 ? p->n_ranks : 1;
  a.rank = p->rank;
  a.out_f32 = p->out_format == PT_OUT_F32;
  for (int k = 0; k < 3; ++k) {
    a.bg[k] = p->background[k];
    a.onoff[k] = p->onoff_color[k];
    a.ambient[k] = p->ambient[k];
  }
  a.bs_levels = pl.bs_levels;
  a.rows_local = pl.rows;
  a.npass = pl.npass;
  a.npix = pl.npix;
  a.frame_doubles = pl.frame_doubles;
  a.diag_lds = pl.diag_lds;
  a.grid_occ_lds = pl.grid_occ_lds;
  a.scene_lds = pl.scene_lds;
  a.nthreads = pl.nthreads;
  a.block_h = pl.block_h;
  if (p->renderer == PT_RENDERER_PATHTRACER) {
    a.p_max_path = pl.p_max_path;
    a.s_min_path = pl.s_min_path;
  }
  if (pl.path_tiled) {
    a.spec_draws = pl.spec_draws;
    a.tree_jump_lds = pl.tree_jump_lds;
    a.handover_cap = pl.q_alt ? pl.handover_cap : 0;
    a.q_budget = a.q_tail_budget = a.q_few_lanes = 0;  // (the one-queue kernel's block carries these)
    a.dbg_trace_unit = (int)tn.trace_unit;
    a.dome_slot = pt_dome_slot(dome_cands, cam, pl, tn);
  }
  if (pl.hier) {  // large scenes: two-level culling (cells of PT_CELL x PT_CELL global pixels, then 8x8 tiles)
    a.cells_x = pl.cells_x;
    a.cell_stride = pl.cell_stride;
  }
}

// num_of_rays > 1: the one-queue kernel IN FRONT of the tree kernel has an argument block of its own (a lane per pixel: 20
// doubles per depth and lane, its own grid, its own slots for the ray counts, nothing of the scene staged in LDS but the
// scale+translate records).  `cold` is the caller's to set.
static inline PtKArgs pt_one_queue_args(const PtKArgs &a, const PtPlan &pl) {
  PtKArgs aq = a;
  aq.nthreads = pl.grid_q * PT_PLAN_BLOCK;
  aq.frame_doubles = 20;
  aq.p_max_path = pl.q_p_max_path;
  aq.s_min_path = pl.q_s_min_path;
  aq.count_base = pl.grid + pl.grid_first;
  aq.q_budget = pl.q_budget;
  aq.q_tail_budget = pl.q_tail_budget;
  aq.q_few_lanes = pl.q_few_lanes;
  aq.scene_lds = -1;
  aq.grid_occ_lds = -1;
  aq.diag_lds = pl.q_diag_lds;
  return aq;
}
