// frame_args_probe.cpp — a stand-alone host program over csrc/pt_frame_args.h: for a fixed list of cases it builds a scene
// description, runs pt_build_scene, pt_scene_facts, the planner and the functions that fill a frame's argument block, and
// prints every non-pointer field of the block (and of the one-queue kernel's block where the plan has one), one per line:
//
//     <case> <key> <value>            floats and doubles as bit patterns (hex), integers in decimal
//
// plus what the expectations need: the plan's fields (plan.*), the scene's facts (facts.*), the dome candidates and the origin
// handed to pt_prep_hoist.  tests/test_frame_args.py builds it (plain, and with the host sanitizers), runs it and checks the
// lines against what it computes itself from the documented formulas.  No HIP call, no device: it runs on any machine.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pytracer_amd/csrc/pt_scene_build.h"
#include "../../pytracer_amd/csrc/pt_plan.h"
#include "../../pytracer_amd/csrc/pt_hits_plan.h"
#include "../../pytracer_amd/csrc/pt_frame_args.h"

static const char *g_case = "";

static void put_int(const char *pre, const char *key, long long v) { printf("%s %s%s %lld\n", g_case, pre, key, v); }
static void put_u64(const char *pre, const char *key, unsigned long long v) { printf("%s %s%s %llu\n", g_case, pre, key, v); }
static void put_f32(const char *pre, const char *key, const float *v, int n) {
  for (int k = 0; k < n; ++k) {
    uint32_t bits;
    memcpy(&bits, v + k, 4);
    printf("%s %s%s[%d] %08x\n", g_case, pre, key, k, bits);
  }
}
static void put_f64(const char *pre, const char *key, const double *v, int n) {
  for (int k = 0; k < n; ++k) {
    uint64_t bits;
    memcpy(&bits, v + k, 8);
    printf("%s %s%s[%d] %016llx\n", g_case, pre, key, k, (unsigned long long)bits);
  }
}

// every field of PtKArgs (pt_layout.h) that is no pointer, in the order of the struct
static void print_block(const char *pre, const PtKArgs &a) {
#define I(f) put_int(pre, #f, a.f)
#define I3(f) \
  for (int k = 0; k < 3; ++k) printf("%s %s%s[%d] %d\n", g_case, pre, #f, k, a.f[k])
#define F3(f) put_f32(pre, #f, a.f, 3)
#define D3(f) put_f64(pre, #f, a.f, 3)
  I(bs_stride); I(gs_stride); I(cs_stride); I(bs_levels); F3(bs_rmax);
  put_f32(pre, "grid_far_eo", &a.grid_far_eo, 1);
  I(grid_n_always); I(grid_occ_lds); I3(grid_res); F3(grid_min); F3(grid_max); F3(grid_cell); F3(grid_inv);
  I(scene_lds); I(diag_lds); I(block_h); I(qpar); I(dome_slot); I(dome_shortcut); I(handover_cap);
  I(q_budget); I(q_tail_budget); I(q_few_lanes); I(tree_jump_lds); I(dbg_trace_unit); I(spec_draws);
  I(cells_x); I(cell_stride); I(p_max_path); I(s_min_path); I(count_base); I(npix);
  I(n_shapes); I(n_lights); I(n_spheres); I(n_diag); I(nthreads); I(frame_doubles); I(rows_local); I(npass);
  I(cam_kind); put_f64(pre, "cam_m", a.cam_m, 12); put_f64(pre, "cam_dist", &a.cam_dist, 1); put_f64(pre, "cam_aspect", &a.cam_aspect, 1);
  F3(cone_d0); F3(cone_dx); F3(cone_dy); F3(cone_apex);
  I(W); I(H); I(S); I(N); I(D); I(rr); I(pcg_mode);
  put_u64(pre, "s0", a.s0); put_u64(pre, "q0", a.q0);
  I(row_block); I(n_ranks); I(rank); I(out_f32); D3(bg); D3(onoff); D3(ambient);
#undef I
#undef I3
#undef F3
#undef D3
}

static void print_plan(const PtPlan &pl) {
#define P(f) put_int("plan.", #f, (long long)pl.f)
  P(rows); P(npix); P(npass); P(bs_levels); P(frame_doubles); P(diag_lds); P(grid_occ_lds); P(scene_lds); P(nthreads); P(block_h);
  P(p_max_path); P(s_min_path); P(spec_draws); P(tree_jump_lds); P(cells_x); P(cell_stride); P(handover_cap);
  P(path_tiled); P(hier); P(q_alt); P(tile4); P(ortho); P(hoist); P(kernel);
  P(grid); P(grid_first); P(grid_q); P(q_p_max_path); P(q_s_min_path); P(q_budget); P(q_tail_budget); P(q_few_lanes); P(q_diag_lds);
#undef P
}

// ---- scene descriptions: spheres (translation * scaling, uniform or checkered pigment) and planes z = const -----------------
struct Shape {
  int kind;
  double scale, c[3];
  int pig_kind;
};
static Shape sphere(double r, double x, double y, double z, int pig_kind = PT_PIGMENT_UNIFORM) { return {PT_SHAPE_SPHERE, r, {x, y, z}, pig_kind}; }
static Shape plane(double z) { return {PT_SHAPE_PLANE, 1.0, {0.0, 0.0, z}, PT_PIGMENT_UNIFORM}; }

// the structure-of-arrays form of include/ptrace.h; the arrays live as long as this object
struct Flat {
  std::vector<int32_t> kind, brdf_kind, pig_kind, tex;
  std::vector<double> invm, m, zero, pig_c1, pig_c2, steps;
  pt_scene_desc d;
  explicit Flat(const std::vector<Shape> &shapes) {
    const size_t n = shapes.size();
    invm.assign(12 * n, 0.0);
    m.assign(12 * n, 0.0);
    zero.assign(3 * n, 0.0);
    pig_c1.assign(3 * n, 0.5);
    pig_c2.assign(3 * n, 0.25);
    steps.assign(n, 4.0);
    tex.assign(n, -1);
    brdf_kind.assign(n, PT_BRDF_DIFFUSE);
    for (size_t i = 0; i < n; ++i) {
      const Shape &s = shapes[i];
      kind.push_back(s.kind);
      pig_kind.push_back(s.pig_kind);
      for (int r = 0; r < 3; ++r) {
        m[(r * 4 + r) * n + i] = s.scale;
        m[(r * 4 + 3) * n + i] = s.c[r];
        invm[(r * 4 + r) * n + i] = 1.0 / s.scale;
        invm[(r * 4 + 3) * n + i] = -s.c[r] / s.scale;
      }
    }
    memset(&d, 0, sizeof d);
    d.n_shapes = (int32_t)n;
    d.kind = kind.data();
    d.invm = invm.data();
    d.m = m.data();
    d.brdf_kind = brdf_kind.data();
    d.brdf_param = zero.data();
    d.pig_kind = pig_kind.data();
    d.pig_c1 = pig_c1.data();
    d.pig_c2 = pig_c2.data();
    d.pig_steps = steps.data();
    d.pig_tex = tex.data();
    d.emi_kind = brdf_kind.data();  // (PT_PIGMENT_UNIFORM: asserted below)
    d.emi_c1 = zero.data();
    d.emi_c2 = zero.data();
    d.emi_steps = steps.data();
    d.emi_tex = tex.data();
  }
};
static_assert(PT_PIGMENT_UNIFORM == PT_BRDF_DIFFUSE, "Flat reuses one array of zeros for both kinds");

// `n` spheres of radius 0.4 on a line in front of the camera, a plane below them when asked for
static std::vector<Shape> row_of_spheres(int n, bool with_plane) {
  std::vector<Shape> v;
  for (int k = 0; k < n; ++k) v.push_back(sphere(0.4, 3.0 + 0.01 * k, -8.0 + 0.5 * k, 0.25));
  if (with_plane) v.push_back(plane(-1.0));
  return v;
}

static pt_camera camera(int kind, bool moved, double dist, double aspect) {
  pt_camera c;
  memset(&c, 0, sizeof c);
  c.kind = kind;
  c.screen_distance = dist;
  c.aspect_ratio = aspect;
  // identity, or a rotation about z by the 3-4-5 angle behind a translation
  const double id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, mv[12] = {0.6, -0.8, 0, 1.5, 0.8, 0.6, 0, -2.0, 0, 0, 1, 0.25};
  memcpy(c.m, moved ? mv : id, sizeof c.m);
  return c;
}

static pt_params params(int w, int h, int renderer) {
  pt_params p;
  memset(&p, 0, sizeof p);
  p.width = w;
  p.height = h;
  p.renderer = renderer;
  p.num_of_rays = 1;
  p.max_depth = 3;
  p.rr_limit = 3;
  p.pcg_mode = PT_PCG_PIXEL;
  p.jitter_state = 42;
  p.jitter_seq = 54;
  p.path_state = 45;
  p.path_seq = 59;
  p.row_block = 1;
  p.n_ranks = 1;
  const double bg[3] = {0.125, 0.25, 0.5}, on[3] = {1.0, 0.75, 0.5}, am[3] = {0.0625, 0.03125, 0.015625};
  memcpy(p.background, bg, sizeof bg);
  memcpy(p.onoff_color, on, sizeof on);
  memcpy(p.ambient, am, sizeof am);
  return p;
}

// what launch() (csrc/ptrace.hip) does with host values, in its order; hits: a hit-record frame's plan
static void run(const char *name, const std::vector<Shape> &shapes, const pt_camera &cam, const pt_params &p, const PtTuning &tn,
                bool hits = false) {
  g_case = name;
  Flat flat(shapes);
  char msg[256] = "";
  if (pt_check_desc(&flat.d, msg, sizeof msg)) {
    printf("%s refused %s\n", g_case, msg);
    return;
  }
  PtSceneHost h;
  pt_build_scene(&flat.d, tn, h);
  const PtSceneFacts facts = pt_scene_facts(h.sc, 256, true);
  put_int("facts.", "n_shapes", facts.n_shapes);
  put_int("facts.", "n_spheres", facts.n_spheres);
  put_int("facts.", "n_diag", facts.n_diag);
  put_int("facts.", "bs_levels", facts.bs_levels);
  put_int("facts.", "has_grid", facts.has_grid);
  PtPlan pl;
  bool cull = false;
  if (hits)
    pt_make_hits_plan(facts, &cam, &p, tn, pl, cull);
  else
    pt_make_plan(facts, &cam, &p, tn, pl);
  print_plan(pl);
  for (size_t k = 0; k < h.dome_cands.size(); ++k) printf("%s dome_cand[%d] %d\n", g_case, h.recs[h.dome_cands[k].slot].index, h.dome_cands[k].slot);
  PtKArgs a;
  memset(&a, 0, sizeof a);
  pt_fill_scene_scalars(a, h.sc, tn);
  pt_fill_frame_args(a, &cam, &p, pl, tn, true, h.dome_cands);
  print_block("", a);
  double o[3];
  pt_hoist_origin(&cam, o);
  put_f64("", "hoist_origin", o, 3);
  if (pl.q_alt) print_block("aq.", pt_one_queue_args(a, pl));
}

int main() {
  const PtTuning dflt;  // (the defaults of the table, whatever the environment holds)
  const std::vector<Shape> none, few = row_of_spheres(3, false);
  // ---- the cone model: identity and moved cameras, perspective and orthogonal, 4 x 2 pixels
  for (int moved = 0; moved < 2; ++moved)
    for (int ortho = 0; ortho < 2; ++ortho) {
      char name[32];
      snprintf(name, sizeof name, "cone_%s_%s", moved ? "moved" : "identity", ortho ? "ortho" : "persp");
      run(name, few, camera(ortho ? PT_CAMERA_ORTHOGONAL : PT_CAMERA_PERSPECTIVE, moved, 1.5, 2.0), params(4, 2, PT_RENDERER_FLAT), dflt);
    }
  // ---- the generator's mode, and the defaults of the partition
  const pt_camera cam = camera(PT_CAMERA_PERSPECTIVE, false, 1.0, 2.0);
  {
    pt_params p = params(4, 2, PT_RENDERER_FLAT);
    p.pcg_mode = PT_PCG_SEQ;
    run("pcg_seq_centre", few, cam, p, dflt);
    p.samples_per_side = 2;
    run("pcg_seq_jitter", few, cam, p, dflt);
    p.pcg_mode = PT_PCG_PIXEL;
    run("pcg_pixel", few, cam, p, dflt);
    p.pcg_mode = PT_PCG_SAMPLE;
    run("pcg_sample", few, cam, p, dflt);
    p.row_block = 0;
    p.n_ranks = 0;
    p.out_format = PT_OUT_F32;
    run("defaults_f32", few, cam, p, dflt);
    p.row_block = 2;
    p.n_ranks = 3;
    p.rank = 1;
    p.height = 16;
    p.out_format = PT_OUT_F64;
    run("partition_f64", few, cam, p, dflt);
  }
  // ---- the dome candidate: a path-tracer frame (tiled first pass), the camera's origin at (-1, 0, 0)
  {
    const pt_params p = params(16, 8, PT_RENDERER_PATHTRACER);
    // shape 0 does not hold the camera; 1: |o'|^2 - 1 = -0.9375; 2: -1 (the deepest); 3 has a pattern: no candidate
    const std::vector<Shape> nested = {sphere(0.5, 3.0, 0.0, 0.0), sphere(4.0, 0.0, 0.0, 0.0), sphere(10.0, -1.0, 0.0, 0.0),
                                       sphere(20.0, -1.0, 0.0, 0.0, PT_PIGMENT_CHECKERED)};
    run("dome_nested", nested, cam, p, dflt);
    run("dome_ortho", nested, camera(PT_CAMERA_ORTHOGONAL, false, 1.0, 2.0), p, dflt);
    PtTuning off = dflt;
    off.pixel_dome = 0;
    run("dome_switched_off", nested, cam, p, off);
    // |o'|^2 - 1 = 0.775^2 - 1 = -0.399...: inside, but not by the -0.5 a dome needs
    run("dome_shallow", {sphere(0.5, 3.0, 0.0, 0.0), sphere(1.0, -0.225, 0.0, 0.0)}, cam, p, dflt);
    run("dome_no_candidates", {plane(-1.0), sphere(10.0, -1.0, 0.0, 0.0, PT_PIGMENT_CHECKERED)}, cam, p, dflt);
  }
  // ---- what the plan decided, copied: num_of_rays = 10 (tree kernel + one-queue alternative), the 16x16 Flat tiles, cell lists
  {
    pt_params p = params(1280, 720, PT_RENDERER_PATHTRACER);
    p.samples_per_side = 1;
    p.num_of_rays = 10;
    const pt_camera wide = camera(PT_CAMERA_PERSPECTIVE, false, 1.0, 1280.0 / 720.0);
    run("plan_tree_q_alt", row_of_spheres(32, false), wide, p, dflt);
    run("plan_tile4_flat", row_of_spheres(32, true), wide, params(1280, 720, PT_RENDERER_FLAT), dflt);
    run("plan_hier_flat", row_of_spheres(257, false), wide, params(320, 180, PT_RENDERER_FLAT), dflt);
    run("plan_hits", row_of_spheres(32, true), wide, params(64, 32, PT_RENDERER_ONOFF), dflt, true);
    p.max_depth = -1;
    run("plan_zero_frame", row_of_spheres(32, false), wide, p, dflt);
    run("plan_no_rows", none, wide, params(64, 0, PT_RENDERER_FLAT), dflt);
  }
  return 0;
}
