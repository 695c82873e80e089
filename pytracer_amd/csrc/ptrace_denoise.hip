// ptrace_denoise.hip — libptrace_denoise.so: the C-ABI of include/ptrace_denoise.h, an edge-avoiding filter for noisy radiance frames.
//
// The kernels are pt_denoise.h's.  Why a tenth translation unit and a tenth shared object: libptrace.so's device code is pinned by
// build.code_hash, and the exported symbols of the nine libraries beside it are pinned to their interfaces'.  So this library stands
// beside them: no link dependency, nothing is loaded from here, and no scene is read.
//
// Launch alternatives, for A/B runs and for the tests that no bit depends on them (all read per call):
//     PTRACE_DN_VARIANT = lds | direct   which kernel filters (default: lds; a build with -DPT_DN_DIRECT makes direct the default)
//     PTRACE_DN_TILE    = 16x16 | 32x8 | 64x4   the LDS variant's tile of a sub-lattice (default 16x16: the fastest measured)
//     PTRACE_DN_BLOCKS  = N              at most N workgroups per launch (the kernels walk grid-stride loops)
// Any other value is refused with PT_ERR_INVALID.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ptrace_denoise.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_denoise.h"
#include "pt_host_common.h"

#define PT_DN_VERSION ((1 << 16) | 8)
#define PT_DN_MAX_M 2147483647LL
#define PT_DN_MAX_GRID 2147483647LL

static_assert(PT_DN_FLAG_SAME_SHAPE == PT_DN_SAME_SHAPE && PT_DN_FLAG_WRAP_X == PT_DN_WRAP_X, "the kernels' flag bits are the header's");

extern "C" int pt_rays_denoise_version(void) { return PT_DN_VERSION; }

extern "C" int pt_rays_denoise_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes and checks: every argument, before any HIP call ---------------------------------------------------------------------
extern "C" size_t pt_rays_denoise_bytes(long long m) { return (m >= 0 && m <= PT_DN_MAX_M) ? (size_t)m * 24 : 0; }

static int check_frame(int width, int height, const pt_denoise_params *p, long long &m) {
  m = 0;
  if (width < 0 || height < 0) return fail(PT_ERR_INVALID, "frame of %d x %d records", width, height);
  if ((long long)width * height > PT_DN_MAX_M) return fail(PT_ERR_INVALID, "record count %d x %d outside [0, 2^31 - 1]", width, height);
  if (!p) return fail(PT_ERR_INVALID, "null pt_denoise_params");
  if (p->passes < 1 || p->passes > 10) return fail(PT_ERR_INVALID, "passes = %d: 1 to 10", p->passes);
  if (!(p->sigma_point > 0.0)) return fail(PT_ERR_INVALID, "sigma_point = %g: a sigma is positive (or +inf)", p->sigma_point);
  if (!(p->sigma_colour > 0.0)) return fail(PT_ERR_INVALID, "sigma_colour = %g: a sigma is positive (or +inf)", p->sigma_colour);
  if (p->normal_power_log2 < 0 || p->normal_power_log2 > 10) return fail(PT_ERR_INVALID, "normal_power_log2 = %d: 0 to 10", p->normal_power_log2);
  if (p->flags & ~(PT_DN_SAME_SHAPE | PT_DN_WRAP_X)) return fail(PT_ERR_INVALID, "unknown flag bits in 0x%x", (unsigned)p->flags);
  m = (long long)width * height;
  return PT_OK;
}

static size_t workspace_need(long long m, const pt_denoise_params *p) { return (size_t)m * 24 * (p->passes > 1 ? 2 : 1); }

extern "C" size_t pt_rays_denoise_workspace_bytes(int width, int height, const pt_denoise_params *params) {
  long long m;
  return check_frame(width, height, params, m) ? 0 : workspace_need(m, params);
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// `workspace` null is allowed where the host form makes it itself (need_ws = false)
static int check_all(int device, int width, int height, const pt_denoise_params *p, const void *colour, const void *normal, const void *point,
                     const void *shape, const void *out, size_t out_bytes, bool need_ws, const void *ws, size_t ws_bytes, long long &m) {
  if (int rc = check_frame(width, height, p, m)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!colour || !normal || !point || !shape) return fail(PT_ERR_INVALID, "null colour, normal, point or shape planes");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  const size_t need = (size_t)m * 24;
  if (overlap(out, need, colour, need)) return fail(PT_ERR_INVALID, "the output overlaps the colour planes: a pass reads its neighbours' input");
  if (need_ws) {
    if (!ws) return fail(PT_ERR_INVALID, "null workspace (pt_rays_denoise_workspace_bytes sizes it)");
    if (overlap(out, need, ws, workspace_need(m, p))) return fail(PT_ERR_INVALID, "the output overlaps the workspace");
  }
  if (out_bytes < need) return fail(PT_ERR_SIZE, "denoise output too small: %zu < %zu bytes", out_bytes, need);
  if (need_ws && ws_bytes < workspace_need(m, p)) return fail(PT_ERR_SIZE, "workspace too small: %zu < %zu bytes", ws_bytes, workspace_need(m, p));
  return PT_OK;
}

// ---- launch alternatives --------------------------------------------------------------------------------------------------------
struct DnLaunch {
  bool direct;
  int tw, th;
  long long max_blocks;
};

static int launch_choice(DnLaunch &L) {
#ifdef PT_DN_DIRECT
  L.direct = true;
#else
  L.direct = false;
#endif
  L.tw = 16, L.th = 16, L.max_blocks = PT_DN_MAX_GRID;
  if (const char *v = getenv("PTRACE_DN_VARIANT")) {
    if (!strcmp(v, "lds")) L.direct = false;
    else if (!strcmp(v, "direct")) L.direct = true;
    else return fail(PT_ERR_INVALID, "PTRACE_DN_VARIANT=%s: lds or direct", v);
  }
  if (const char *v = getenv("PTRACE_DN_TILE")) {
    if (!strcmp(v, "32x8")) L.tw = 32, L.th = 8;
    else if (!strcmp(v, "16x16")) L.tw = 16, L.th = 16;
    else if (!strcmp(v, "64x4")) L.tw = 64, L.th = 4;
    else return fail(PT_ERR_INVALID, "PTRACE_DN_TILE=%s: 16x16, 32x8 or 64x4", v);
  }
  if (const char *v = getenv("PTRACE_DN_BLOCKS")) {
    char *end = nullptr;
    const long long n = strtoll(v, &end, 10);
    if (end == v || *end || n < 1) return fail(PT_ERR_INVALID, "PTRACE_DN_BLOCKS=%s: a positive count of workgroups", v);
    L.max_blocks = std::min(n, PT_DN_MAX_GRID);
  }
  return PT_OK;
}

// the pre-pass and the passes; `unit` and `other` are the workspace's halves (`other` unused when passes == 1)
static int enqueue(const DnLaunch &L, int width, int height, const pt_denoise_params &p, long long m, const double *colour, const double *normal,
                   const double *point, const int *shape, double *out, double *unit, double *other, hipStream_t st) {
  const long long flat = (m + PT_BLOCK - 1) / PT_BLOCK;
  hipLaunchKernelGGL(pt_dn_unit_kernel, dim3((unsigned)std::min(flat, L.max_blocks)), dim3(PT_BLOCK), 0, st, normal, m, unit);
  HIP_TRY(hipGetLastError());
  const double *src = colour;
  for (int i = 0; i < p.passes; i++) {
    double *dst = ((p.passes - 1 - i) % 2 == 0) ? out : other;  // (the last pass lands in `out`)
    PtDnK K;
    K.W = width, K.H = height, K.s = 1 << i, K.flags = p.flags, K.e = p.normal_power_log2, K.m = m;
    K.rxn = std::min(K.s, width), K.ryn = std::min(K.s, height);
    K.sps = p.sigma_point * (double)K.s;
    const double sc = p.sigma_colour * (1.0 / (double)K.s);  // (2^-i: exact)
    K.sc2 = sc * sc;
    K.sp_inf = std::isinf(K.sps), K.sc_inf = std::isinf(K.sc2);
    const long long sw = ((long long)width + K.s - 1) / K.s, sh = ((long long)height + K.s - 1) / K.s;  // the widest, tallest sub-lattice
    K.tiles_x = (int)((sw + L.tw - 1) / L.tw), K.tiles_y = (int)((sh + L.th - 1) / L.th);
    K.nblocks = L.direct ? flat : (long long)K.tiles_x * K.rxn * ((long long)K.tiles_y * K.ryn);
    const dim3 grid((unsigned)std::min(K.nblocks, L.max_blocks));
    if (L.direct) hipLaunchKernelGGL(pt_dn_direct_kernel, grid, dim3(PT_BLOCK), 0, st, K, src, (const double *)unit, point, shape, dst);
    else if (L.tw == 32) hipLaunchKernelGGL((pt_dn_lds_kernel<32, 8>), grid, dim3(PT_BLOCK), 0, st, K, src, (const double *)unit, point, shape, dst);
    else if (L.tw == 16) hipLaunchKernelGGL((pt_dn_lds_kernel<16, 16>), grid, dim3(PT_BLOCK), 0, st, K, src, (const double *)unit, point, shape, dst);
    else hipLaunchKernelGGL((pt_dn_lds_kernel<64, 4>), grid, dim3(PT_BLOCK), 0, st, K, src, (const double *)unit, point, shape, dst);
    HIP_TRY(hipGetLastError());
    src = dst;
  }
  return PT_OK;
}

// ---- the device form ------------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_denoise_device(int device, int width, int height, const pt_denoise_params *params, const double *colour_dev,
                                      const double *normal_dev, const double *point_dev, const int *shape_dev, void *out_dev, size_t out_bytes,
                                      void *workspace_dev, size_t workspace_bytes, void *stream) {
  long long m;
  DnLaunch L;
  int rc = check_all(device, width, height, params, colour_dev, normal_dev, point_dev, shape_dev, out_dev, out_bytes, true, workspace_dev,
                     workspace_bytes, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  double *unit = (double *)workspace_dev;
  if ((rc = enqueue(L, width, height, *params, m, colour_dev, normal_dev, point_dev, shape_dev, (double *)out_dev, unit, unit + 3 * m,
                    (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- the host form: one device allocation holds the inputs, the workspace and the output -----------------------------------------
extern "C" int pt_rays_denoise(int device, int width, int height, const pt_denoise_params *params, const double *colour_host,
                               const double *normal_host, const double *point_host, const int *shape_host, void *out_host, size_t out_bytes) {
  long long m;
  DnLaunch L;
  int rc = check_all(device, width, height, params, colour_host, normal_host, point_host, shape_host, out_host, out_bytes, false, nullptr, 0, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t plane3 = (size_t)m * 24, shape_b = up8((size_t)m * 4), ws_b = workspace_need(m, params);
  Staged s;
  if ((rc = s.alloc(4 * plane3 + shape_b + ws_b))) return rc;
  char *col_d = s.dev, *nrm_d = col_d + plane3, *pnt_d = nrm_d + plane3, *out_d = pnt_d + plane3, *ws_d = out_d + plane3, *shape_d = ws_d + ws_b;
  HIP_TRY(hipMemcpy(col_d, colour_host, plane3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(nrm_d, normal_host, plane3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(pnt_d, point_host, plane3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue(L, width, height, *params, m, (const double *)col_d, (const double *)nrm_d, (const double *)pnt_d, (const int *)shape_d,
                    (double *)out_d, (double *)ws_d, (double *)ws_d + 3 * m, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, plane3, hipMemcpyDeviceToHost));  // (the null stream: behind the kernels)
  return PT_OK;
}
