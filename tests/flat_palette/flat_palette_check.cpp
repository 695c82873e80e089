// flat_palette_check.cpp — a stand-alone host program over csrc/pt_scene_build.h: the Flat palette (pt_layout.h: PtFlatPal)
// of generated scenes against the aux[] records it is made from, and the image the upload puts behind aux[].
//
//     <shapes> ok <entries checked> <uniform entries> <chunks>          one line per scene, or
//     <shapes> FAIL <what>                                              and exit status 1
//
// tests/test_flat_palette.py builds it (plain, and with the host sanitizers) and runs it.  No HIP call, no device.
//
// Every scene mixes the pigment kinds (uniform / checkered / image, for the BRDF pigment and the emitted one independently),
// spheres and planes, so that slots are reordered; colours are random doubles, whose fp64 sum is inexact for nearly every
// pair, beside a few sums that are exact.  The expected colour is computed HERE from the description, not read back from aux.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pytracer_amd/csrc/pt_scene_build.h"

struct Rng {  // splitmix64
  uint64_t x;
  uint64_t next() {
    uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
};

// structure-of-arrays scene of n shapes (include/ptrace.h); shape i is a unit sphere or the plane z = 0, moved to (i, 0, 0)
struct Flat {
  std::vector<int32_t> kind, brdf_kind, pig_kind, pig_tex, emi_kind, emi_tex;
  std::vector<double> invm, m, brdf_param, pig_c1, pig_c2, pig_steps, emi_c1, emi_c2, emi_steps, tex_data;
  std::vector<int32_t> tex_w, tex_h;
  std::vector<int64_t> tex_offset;
  pt_scene_desc d;

  Flat(int n, uint64_t seed) {
    Rng rng{seed};
    const size_t N = (size_t)n;
    invm.assign(12 * N, 0.0);
    m.assign(12 * N, 0.0);
    pig_c1.resize(3 * N);
    pig_c2.resize(3 * N);
    emi_c1.resize(3 * N);
    emi_c2.resize(3 * N);
    tex_w = {2};
    tex_h = {2};
    tex_offset = {0};
    for (int k = 0; k < 12; ++k) tex_data.push_back(rng.uni());
    const int kinds[3] = {PT_PIGMENT_UNIFORM, PT_PIGMENT_CHECKERED, PT_PIGMENT_IMAGE};
    for (size_t i = 0; i < N; ++i) {
      kind.push_back(i % 5 == 2 ? PT_SHAPE_PLANE : PT_SHAPE_SPHERE);
      brdf_kind.push_back(PT_BRDF_DIFFUSE);
      brdf_param.push_back(0.0);
      // two of three shapes uniform in both pigments; the rest runs through every other pair of kinds
      const int pk = i % 3 == 1 ? kinds[(i / 3) % 3] : PT_PIGMENT_UNIFORM;
      const int ek = i % 3 == 1 ? kinds[(i / 9 + (pk == PT_PIGMENT_UNIFORM ? 1 : 0)) % 3] : PT_PIGMENT_UNIFORM;
      pig_kind.push_back(pk);
      emi_kind.push_back(ek);
      pig_tex.push_back(pk == PT_PIGMENT_IMAGE ? 0 : -1);
      emi_tex.push_back(ek == PT_PIGMENT_IMAGE ? 0 : -1);
      pig_steps.push_back(4.0);
      emi_steps.push_back(3.0);
      for (int k = 0; k < 3; ++k) {
        pig_c1[k * N + i] = rng.uni();
        pig_c2[k * N + i] = rng.uni();
        emi_c1[k * N + i] = i % 7 == 0 ? 0.25 * (double)k : rng.uni() * 1e-3;  // (a few exact sums among the inexact)
        emi_c2[k * N + i] = rng.uni();
      }
      for (int r = 0; r < 3; ++r) m[(size_t)(r * 4 + r) * N + i] = invm[(size_t)(r * 4 + r) * N + i] = 1.0;
      m[3 * N + i] = (double)i;
      invm[3 * N + i] = -(double)i;
    }
    memset(&d, 0, sizeof d);
    d.n_shapes = n;
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
    d.n_textures = 1;
    d.tex_w = tex_w.data();
    d.tex_h = tex_h.data();
    d.tex_offset = tex_offset.data();
    d.tex_data = tex_data.data();
  }
};

static int g_shapes = 0;
static bool fail(const char *what, long long at) {
  printf("%d FAIL %s at %lld\n", g_shapes, what, at);
  return false;
}

static bool check(int n) {
  g_shapes = n;
  Flat flat(n, 1000 + (uint64_t)n);
  char msg[256] = "";
  if (pt_check_desc(&flat.d, msg, sizeof msg)) return fail(msg, -1);
  PtSceneHost h;
  pt_build_scene(&flat.d, PtTuning(), h);
  const size_t N = (size_t)n;
  if (h.aux.size() != N || h.recs.size() != N || h.flat_pal.size() != N) return fail("table sizes", (long long)h.flat_pal.size());
  int uniform = 0, inexact = 0;
  for (size_t slot = 0; slot < N; ++slot) {
    const PtShapeAux &x = h.aux[slot];
    const PtFlatPal &e = h.flat_pal[slot];
    const size_t i = (size_t)h.recs[slot].index;
    const bool both = flat.pig_kind[i] == PT_PIGMENT_UNIFORM && flat.emi_kind[i] == PT_PIGMENT_UNIFORM;
    if (e.needs_uv != x.needs_uv || e.needs_uv != (both ? 0 : 1)) return fail("needs_uv", (long long)slot);
    if (e._pad != 0) return fail("record padding", (long long)slot);
    double want[3] = {0.0, 0.0, 0.0};
    if (both)
      for (int k = 0; k < 3; ++k) {
        const volatile double p = flat.pig_c1[k * N + i], q = flat.emi_c1[k * N + i];
        want[k] = p + q;  // render.py:65-74, the fp64 addition
        if ((want[k] - p) != q) ++inexact;
      }
    if (memcmp(e.c, want, sizeof want) != 0) return fail("colour", (long long)slot);
    if (both && memcmp(e.c, x.pig_c2, sizeof want) != 0) return fail("colour != aux.pig_c2", (long long)slot);
    uniform += both ? 1 : 0;
  }
  if (n >= 63 && (inexact == 0 || uniform == n || uniform == 0)) return fail("the scene does not show what it is for", inexact);
  // the image of the upload: aux[] byte for byte, the palette behind it, zeros to the end of the last chunk
  const std::vector<unsigned char> img = pt_aux_image(h);
  const int chunks = pt_flat_pal_chunks(n);
  if (chunks != (n * 32 + 1023) / 1024) return fail("chunk count", chunks);
  if (img.size() != N * sizeof(PtShapeAux) + (size_t)chunks * PT_FLAT_PAL_CHUNK) return fail("image size", (long long)img.size());
  if (N && memcmp(img.data(), h.aux.data(), N * sizeof(PtShapeAux)) != 0) return fail("aux part of the image", 0);
  const unsigned char *pal = img.data() + N * sizeof(PtShapeAux);
  if (N && memcmp(pal, h.flat_pal.data(), N * sizeof(PtFlatPal)) != 0) return fail("palette part of the image", 0);
  for (size_t b = N * sizeof(PtFlatPal); b < (size_t)chunks * PT_FLAT_PAL_CHUNK; ++b)
    if (pal[b] != 0) return fail("chunk padding", (long long)b);
  // the four wave slices of the staged kernel lie inside the LDS block the plan reserves for it (worlds of 4 .. 64 shapes)
  if (n >= 4 && n <= 64) {
    const long long end = 3LL * pt_flat_pal_slice(n) + (long long)chunks * PT_FLAT_PAL_CHUNK;
    if (end > (long long)n * (PT_PLAN_REC_BYTES + PT_PLAN_AUX_BYTES) || pt_flat_pal_slice(n) % 16 != 0) return fail("slices", end);
  }
  printf("%d ok %d %d %d\n", n, n, uniform, chunks);
  return true;
}

int main() {
  bool ok = true;
  for (int n : {0, 1, 63, 64, 65, 256}) ok = check(n) && ok;
  // (every count the staged kernel can meet, for the slice arithmetic)
  for (int n = 4; n <= 64; ++n) {
    const long long end = 3LL * pt_flat_pal_slice(n) + (long long)pt_flat_pal_chunks(n) * PT_FLAT_PAL_CHUNK;
    if (end > (long long)n * (PT_PLAN_REC_BYTES + PT_PLAN_AUX_BYTES) || pt_flat_pal_chunks(n) > 2) {
      printf("%d FAIL slices end at %lld\n", n, end);
      ok = false;
    }
  }
  return ok ? 0 : 1;
}
