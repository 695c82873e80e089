// scene_digest.cpp — a stand-alone host program over csrc/pt_scene_build.h: it generates scene descriptions deterministically,
// runs pt_build_scene on each and prints one 64-bit digest (FNV-1a) per table and every scalar, one per line:
//
//     <scene> <key> <value>
//
// tests/test_scene_build.py builds it (plain, and with the host sanitizers), runs it and compares the output line by line
// with tests/golden/g14_scene_build_digests.txt.  No HIP call, no device: it runs on any machine.
//
// The scenes are the smallest at which each branch of the analysis runs (the empty world, planes only, the general case, the
// 127 / 128 border of the ball hierarchy, a grid with an "always" list, the grid switched off, a small grid, every kind of
// "no bound", the fallback of pt_ball_square, a grid abandoned for its crowded cells).  No libm function but the ones the
// analysis itself calls: rotations come from the 3-4-5 triangle.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../pytracer_amd/csrc/pt_scene_build.h"

// ---- digests --------------------------------------------------------------------------------------------------------------
static uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ULL) {
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ULL;
  return h;
}

static const char *g_scene = "";

static void put(const char *key, uint64_t v) { printf("%s %s %016llx\n", g_scene, key, (unsigned long long)v); }
static void put_int(const char *key, long long v) { printf("%s %s %lld\n", g_scene, key, v); }
static void put_f32(const char *key, const float *v, int n) {
  for (int k = 0; k < n; ++k) {
    uint32_t bits;
    memcpy(&bits, v + k, 4);
    printf("%s %s[%d] %08x\n", g_scene, key, k, bits);
  }
}
template <typename T>
static void put_table(const char *key, const std::vector<T> &v) {
  const uint64_t n = v.size();
  put(key, fnv(v.data(), v.size() * sizeof(T), fnv(&n, sizeof n)));
}

static void print_digests(const PtSceneHost &h) {
  const PtSceneScalars &s = h.sc;
  put_int("n_shapes", s.n_shapes);
  put_int("n_spheres", s.n_spheres);
  put_int("n_diag", s.n_diag);
  put_int("n_lights", s.n_lights);
  put_int("n_textures", s.n_textures);
  put_int("bs_levels", s.bs_levels);
  put_int("bs_stride", s.bs_stride);
  put_int("gs_stride", s.gs_stride);
  put_int("cs_stride", s.cs_stride);
  put_f32("bs_rmax", s.bs_rmax, 3);
  put_int("grid_n_always", s.grid_n_always);
  put_int("grid_n_cells", s.grid_n_cells);
  for (int q = 0; q < 3; ++q) printf("%s grid_res[%d] %d\n", g_scene, q, s.grid_res[q]);
  put_f32("grid_far_eo", &s.grid_far_eo, 1);
  put_f32("grid_min", s.grid_min, 3);
  put_f32("grid_max", s.grid_max, 3);
  put_f32("grid_cell", s.grid_cell, 3);
  put_f32("grid_inv", s.grid_inv, 3);
  put_int("has_grid", h.has_grid ? 1 : 0);
  put_table("recs", h.recs);
  put_table("aux", h.aux);
  put_table("diag", h.diag);
  put_table("bounds", h.bounds);
  put_table("bsoa", h.bsoa);
  put_table("lights", h.lights);
  put_table("tex", h.tex);
  put_table("tex_data", h.tex_data);
  put_table("grid_cells", h.grid_cells);
  put_table("grid_occ", h.grid_occ);
  put_table("grid_slots", h.grid_slots);
  put_table("grid_balls", h.grid_balls);
  put_table("grid_always", h.grid_always);
  uint64_t dc = fnv("dome", 4);  // (slot and matrix separately: the struct has padding between them)
  for (const auto &c : h.dome_cands) dc = fnv(c.invm, sizeof c.invm, fnv(&c.slot, sizeof c.slot, dc));
  put_int("dome_cands_n", (long long)h.dome_cands.size());
  put("dome_cands", dc);
}

// ---- scene descriptions ---------------------------------------------------------------------------------------------------
struct Rng {  // splitmix64
  uint64_t x;
  uint64_t next() {
    uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
  double range(double a, double b) { return a + (b - a) * uni(); }
};

struct Shape {
  int kind = PT_SHAPE_SPHERE;
  double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, invm[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  int brdf_kind = PT_BRDF_DIFFUSE;
  double brdf_param = 0.0;
  int pig_kind = PT_PIGMENT_UNIFORM, emi_kind = PT_PIGMENT_UNIFORM, pig_tex = -1, emi_tex = -1;
  double pig_c1[3] = {0.5, 0.25, 0.125}, pig_c2[3] = {0, 0, 0}, emi_c1[3] = {0, 0, 0}, emi_c2[3] = {0, 0, 0};
  double pig_steps = 0.0, emi_steps = 0.0;
};

// m = [A | t] (row-major 3x4), invm = [A^-1 | -A^-1 t] by cofactors
static void set_affine(Shape &s, const double A[9], const double t[3]) {
  const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
  const double I[9] = {(A[4] * A[8] - A[5] * A[7]) / det, (A[2] * A[7] - A[1] * A[8]) / det, (A[1] * A[5] - A[2] * A[4]) / det,
                       (A[5] * A[6] - A[3] * A[8]) / det, (A[0] * A[8] - A[2] * A[6]) / det, (A[2] * A[3] - A[0] * A[5]) / det,
                       (A[3] * A[7] - A[4] * A[6]) / det, (A[1] * A[6] - A[0] * A[7]) / det, (A[0] * A[4] - A[1] * A[3]) / det};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      s.m[r * 4 + c] = A[r * 3 + c];
      s.invm[r * 4 + c] = I[r * 3 + c];
    }
    s.m[r * 4 + 3] = t[r];
    s.invm[r * 4 + 3] = -(I[r * 3] * t[0] + I[r * 3 + 1] * t[1] + I[r * 3 + 2] * t[2]);
  }
}

// translation * scaling: the 3x3 block of invm is diagonal with exact zeros beside it
static Shape scaled_sphere(double sx, double sy, double sz, double tx, double ty, double tz) {
  Shape s;
  const double sc[3] = {sx, sy, sz}, t[3] = {tx, ty, tz};
  for (int r = 0; r < 3; ++r) {
    s.m[r * 4 + r] = sc[r];
    s.m[r * 4 + 3] = t[r];
    s.invm[r * 4 + r] = 1.0 / sc[r];
    s.invm[r * 4 + 3] = -t[r] / sc[r];
  }
  return s;
}

static Shape rotated_sphere(double scale, double shear, double tx, double ty, double tz) {
  Shape s;
  // rotation about z by the 3-4-5 angle, times a scaling, plus a shear of x by y
  const double A[9] = {0.6 * scale, -0.8 * scale + shear, 0.0, 0.8 * scale, 0.6 * scale, 0.0, 0.0, 0.0, scale * 1.25};
  const double t[3] = {tx, ty, tz};
  set_affine(s, A, t);
  return s;
}

static Shape plane(double tz, bool tilted) {
  Shape s;
  s.kind = PT_SHAPE_PLANE;
  const double flat[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tilt[9] = {1, 0, 0, 0, 0.6, -0.8, 0, 0.8, 0.6};
  const double t[3] = {0.0, 0.0, tz};
  set_affine(s, tilted ? tilt : flat, t);
  return s;
}

struct Scene {
  std::vector<Shape> shapes;
  std::vector<double> light_pos, light_color, light_radius;  // per light: xyz, rgb, radius
  std::vector<int32_t> tex_w, tex_h;
  std::vector<int64_t> tex_offset;
  std::vector<double> tex_data;

  void add_light(double x, double y, double z, double r, double g, double b, double radius) {
    for (double v : {x, y, z}) light_pos.push_back(v);
    for (double v : {r, g, b}) light_color.push_back(v);
    light_radius.push_back(radius);
  }
  void add_texture(int w, int h, Rng &rng) {
    tex_w.push_back(w);
    tex_h.push_back(h);
    tex_offset.push_back((int64_t)tex_data.size());
    for (int k = 0; k < w * h * 3; ++k) tex_data.push_back(rng.uni());
  }
};

// the structure-of-arrays form of include/ptrace.h; the arrays live as long as this object
struct Flat {
  std::vector<int32_t> kind, brdf_kind, pig_kind, pig_tex, emi_kind, emi_tex;
  std::vector<double> invm, m, brdf_param, pig_c1, pig_c2, pig_steps, emi_c1, emi_c2, emi_steps, light_pos, light_color;
  pt_scene_desc d;

  explicit Flat(const Scene &sc) {
    const size_t n = sc.shapes.size(), nl = sc.light_radius.size();
    invm.resize(12 * n);
    m.resize(12 * n);
    pig_c1.resize(3 * n);
    pig_c2.resize(3 * n);
    emi_c1.resize(3 * n);
    emi_c2.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const Shape &s = sc.shapes[i];
      kind.push_back(s.kind);
      brdf_kind.push_back(s.brdf_kind);
      brdf_param.push_back(s.brdf_param);
      pig_kind.push_back(s.pig_kind);
      pig_tex.push_back(s.pig_tex);
      pig_steps.push_back(s.pig_steps);
      emi_kind.push_back(s.emi_kind);
      emi_tex.push_back(s.emi_tex);
      emi_steps.push_back(s.emi_steps);
      for (int k = 0; k < 12; ++k) {
        invm[k * n + i] = s.invm[k];
        m[k * n + i] = s.m[k];
      }
      for (int k = 0; k < 3; ++k) {
        pig_c1[k * n + i] = s.pig_c1[k];
        pig_c2[k * n + i] = s.pig_c2[k];
        emi_c1[k * n + i] = s.emi_c1[k];
        emi_c2[k * n + i] = s.emi_c2[k];
      }
    }
    light_pos.resize(3 * nl);
    light_color.resize(3 * nl);
    for (size_t l = 0; l < nl; ++l)
      for (int k = 0; k < 3; ++k) {
        light_pos[k * nl + l] = sc.light_pos[l * 3 + k];
        light_color[k * nl + l] = sc.light_color[l * 3 + k];
      }
    memset(&d, 0, sizeof d);
    d.n_shapes = (int32_t)n;
    d.kind = kind.data();
    d.invm = invm.data();
    d.m = m.data();
    d.brdf_kind = brdf_kind.data();
    d.brdf_param = brdf_param.data();
    d.pig_kind = pig_kind.data();
    d.pig_c1 = pig_c1.data();
    d.pig_c2 = pig_c2.data();
    d.pig_steps = pig_steps.data();
    d.pig_tex = pig_tex.data();
    d.emi_kind = emi_kind.data();
    d.emi_c1 = emi_c1.data();
    d.emi_c2 = emi_c2.data();
    d.emi_steps = emi_steps.data();
    d.emi_tex = emi_tex.data();
    d.n_lights = (int32_t)nl;
    d.light_pos = light_pos.data();
    d.light_color = light_color.data();
    d.light_radius = sc.light_radius.data();
    d.n_textures = (int32_t)sc.tex_w.size();
    d.tex_w = sc.tex_w.data();
    d.tex_h = sc.tex_h.data();
    d.tex_offset = sc.tex_offset.data();
    d.tex_data = sc.tex_data.data();
  }
};

// `count` scale+translate spheres of radius 0.2 .. 0.6 with centres in [-spread, spread]^3, every seventh one rotated
static void add_cloud(Scene &sc, int count, double spread, Rng &rng) {
  for (int k = 0; k < count; ++k) {
    const double r = rng.range(0.2, 0.6), x = rng.range(-spread, spread), y = rng.range(-spread, spread), z = rng.range(-spread, spread);
    Shape s = k % 7 == 3 ? rotated_sphere(r, 0.0, x, y, z) : scaled_sphere(r, r * rng.range(0.8, 1.2), r, x, y, z);
    for (int c = 0; c < 3; ++c) s.pig_c1[c] = rng.uni();
    if (k % 11 == 5) s.emi_c1[0] = s.emi_c1[1] = s.emi_c1[2] = 1.0;
    if (k % 13 == 2) {
      s.brdf_kind = PT_BRDF_SPECULAR;
      s.brdf_param = 0.001;
    }
    sc.shapes.push_back(s);
  }
}

static Scene general_scene() {
  Rng rng{11};
  Scene sc;
  sc.add_texture(3, 2, rng);
  sc.add_texture(2, 4, rng);
  sc.add_light(5.0, 4.0, 10.0, 1.0, 0.9, 0.8, 0.0);
  sc.add_light(-3.0, 2.0, 6.0, 0.2, 0.3, 0.4, 1.5);
  sc.shapes.push_back(plane(-1.0, false));
  sc.shapes.push_back(scaled_sphere(0.5, 0.5, 0.5, 1.0, 0.0, 0.0));
  sc.shapes.push_back(rotated_sphere(0.7, 0.0, -1.0, 2.0, 0.5));
  sc.shapes.push_back(scaled_sphere(1.0, 2.0, 0.25, 0.0, -3.0, 1.0));
  sc.shapes.push_back(rotated_sphere(0.4, 0.3, 2.0, 2.0, 2.0));  // sheared
  sc.shapes.push_back(plane(4.0, true));
  sc.shapes.push_back(scaled_sphere(50.0, 50.0, 50.0, 0.0, 0.0, 0.0));  // a dome
  sc.shapes.push_back(scaled_sphere(0.3, 0.3, 0.3, 0.0, 0.0, 0.0));    // zero translation: tnz = 0
  sc.shapes[0].pig_kind = PT_PIGMENT_CHECKERED;
  sc.shapes[0].pig_steps = 4.0;
  sc.shapes[0].pig_c2[1] = 0.75;
  sc.shapes[1].pig_kind = PT_PIGMENT_IMAGE;
  sc.shapes[1].pig_tex = 1;
  sc.shapes[2].emi_kind = PT_PIGMENT_IMAGE;
  sc.shapes[2].emi_tex = 0;
  sc.shapes[3].brdf_kind = PT_BRDF_SPECULAR;
  sc.shapes[3].brdf_param = 0.0017;
  sc.shapes[6].emi_c1[0] = sc.shapes[6].emi_c1[1] = sc.shapes[6].emi_c1[2] = 1.0;
  return sc;
}

static Scene cloud_scene(int count, double spread, uint64_t seed) {
  Rng rng{seed};
  Scene sc;
  add_cloud(sc, count, spread, rng);
  return sc;
}

static void run(const char *name, const Scene &sc, const PtTuning &tn) {
  g_scene = name;
  Flat flat(sc);
  char msg[256] = "";
  const int rc = pt_check_desc(&flat.d, msg, sizeof msg);
  put_int("check_desc", rc);
  if (rc) {
    printf("%s message %s\n", g_scene, msg);
    return;
  }
  PtSceneHost h;
  pt_build_scene(&flat.d, tn, h);
  print_digests(h);
}

int main() {
  const PtTuning dflt;  // (the defaults of the table, whatever the environment holds)
  run("empty", Scene(), dflt);
  {
    Scene sc;
    sc.shapes.push_back(plane(-2.0, true));
    run("plane_only", sc, dflt);
  }
  run("general", general_scene(), dflt);
  run("spheres_127", cloud_scene(127, 8.0, 127), dflt);
  run("spheres_128", cloud_scene(128, 8.0, 128), dflt);
  {
    // 1 100 spheres spread wide and one of 100x the median radius: a grid with an "always" list
    Scene sc = cloud_scene(1100, 40.0, 1100);
    sc.shapes.push_back(scaled_sphere(40.0, 40.0, 40.0, 1.0, 2.0, 3.0));
    sc.shapes.push_back(plane(-45.0, false));
    run("grid_1100", sc, dflt);
    PtTuning off = dflt;
    off.grid = 0;
    run("grid_1100_off", sc, off);
    PtTuning dense = dflt;
    dense.grid_density = 9.0;
    run("grid_1100_density9", sc, dense);
  }
  {
    PtTuning small = dflt;
    small.grid_min = 64;
    run("grid_130_min64", cloud_scene(130, 10.0, 130), small);
    run("grid_130_default", cloud_scene(130, 10.0, 130), dflt);
  }
  {
    Scene sc = cloud_scene(140, 10.0, 140);
    sc.shapes[5].m[3] = std::numeric_limits<double>::quiet_NaN();
    sc.shapes[17].m[7] = std::numeric_limits<double>::infinity();
    PtTuning small = dflt;
    small.grid_min = 64;
    run("nonfinite_centre", sc, small);
    Scene few = general_scene();
    few.shapes[1].m[11] = -std::numeric_limits<double>::infinity();
    few.shapes[3].invm[7] = std::numeric_limits<double>::quiet_NaN();
    run("nonfinite_centre_few", few, dflt);
  }
  {
    // m does not invert invm: residuals of 1e-3 (no bound), 1e-6 (the border: no bound) and 1e-8 (a widened bound)
    Scene sc = general_scene();
    sc.shapes[1].m[0] *= 1.0 + 1e-3;
    sc.shapes[2].m[3] += 1e-6 * 4.0;
    sc.shapes[3].m[5] *= 1.0 + 1e-8;
    run("m_not_inverse", sc, dflt);
  }
  {
    Scene sc = general_scene();
    sc.shapes.push_back(scaled_sphere(1e120, 1.0, 1.0, 0.0, 1.0, 0.0));   // invm[0] = 1e-120: not in the diag group
    sc.shapes.push_back(scaled_sphere(1.0, 1e-120, 1.0, 0.0, 1.0, 0.0));  // invm[5] = 1e120
    sc.shapes.push_back(scaled_sphere(1e-7, 1e-7, 1e-7, 0.0, 1.0, 0.0));  // diag, but fro2 = +inf
    run("singular_scale", sc, dflt);
  }
  {
    Scene sc = general_scene();
    sc.shapes.push_back(scaled_sphere(1e17, 1e17, 1e17, 0.0, 0.0, 0.0));
    sc.shapes.push_back(scaled_sphere(3e18, 3e18, 3e18, 1.0, 0.0, 0.0));
    sc.shapes.push_back(scaled_sphere(1e38, 1e38, 1e38, 1.0, 0.0, 0.0));
    sc.shapes.push_back(scaled_sphere(1.0, 1.0, 1.0, 2e17, 0.0, 0.0));
    run("huge_radius", sc, dflt);
    Scene many = cloud_scene(150, 10.0, 150);
    many.shapes.push_back(scaled_sphere(1e17, 1e17, 1e17, 0.0, 0.0, 0.0));
    many.shapes.push_back(scaled_sphere(1.0, 1.0, 1.0, 2e17, 0.0, 0.0));
    PtTuning small = dflt;
    small.grid_min = 64;
    run("huge_radius_grid", many, small);
  }
  {
    // 1 100 spheres of radius ~0.5 within 0.02 of one point: every cell would hold them all, the grid is abandoned
    Rng rng{255};
    Scene sc;
    for (int k = 0; k < 1100; ++k) {
      const double r = rng.range(0.45, 0.55);
      sc.shapes.push_back(scaled_sphere(r, r, r, rng.range(-0.02, 0.02), rng.range(-0.02, 0.02), rng.range(-0.02, 0.02)));
    }
    run("crowded_cells", sc, dflt);
  }
  {
    // what pt_check_desc refuses, with its message
    Scene sc = general_scene();
    sc.shapes[2].kind = 7;
    run("bad_kind", sc, dflt);
    Scene tx = general_scene();
    tx.shapes[1].pig_tex = 2;
    run("bad_texture", tx, dflt);
  }
  return 0;
}
