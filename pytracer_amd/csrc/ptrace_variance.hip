// ptrace_variance.hip — libptrace_variance.so: the C-ABI of include/ptrace_variance.h, luminance moments, a per-pixel variance and a
// variance-guided filter.
//
// The kernels are pt_variance.h's.  Why a twelfth translation unit and a twelfth shared object: libptrace.so's device code is pinned
// by build.code_hash, and the exported symbols of the eleven libraries beside it are pinned to their interfaces'.  So this library
// stands beside them: no link dependency, nothing is loaded from here, and no scene is read.
//
// Launch alternatives, for A/B runs and for the tests that no bit depends on them (all read per call):
//     PTRACE_VR_VARIANT = lds | direct   which kernel filters (default: lds)
//     PTRACE_VR_TILE    = 16x16 | 32x8 | 64x4   the LDS variant's tile of a sub-lattice (default 16x16)
//     PTRACE_VR_BLOCKS  = N              at most N workgroups per launch (the kernels walk grid-stride loops)
// Any other value is refused with PT_ERR_INVALID.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ptrace_variance.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_variance.h"
#include "pt_host_common.h"

#define PT_VR_VERSION ((1 << 16) | 10)
#define PT_VR_MAX_M 2147483647LL
#define PT_VR_MAX_GRID 2147483647LL

static_assert(PT_VR_FLAG_SAME_SHAPE == PT_VR_SAME_SHAPE && PT_VR_FLAG_WRAP_X == PT_VR_WRAP_X, "the kernels' flag bits are the header's");
static_assert(sizeof(pt_variance_params) == 56, "the struct of the header");

extern "C" int pt_rays_variance_version(void) { return PT_VR_VERSION; }

extern "C" int pt_rays_variance_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes and checks: every argument, before any HIP call ---------------------------------------------------------------------
extern "C" size_t pt_rays_variance_bytes(long long m) { return (m >= 0 && m <= PT_VR_MAX_M) ? (size_t)m * 24 : 0; }

extern "C" size_t pt_rays_variance_plane_bytes(long long m) { return (m >= 0 && m <= PT_VR_MAX_M) ? (size_t)m * 8 : 0; }

static int check_size(int width, int height, long long &m) {
  m = 0;
  if (width < 0 || height < 0) return fail(PT_ERR_INVALID, "frame of %d x %d records", width, height);
  if ((long long)width * height > PT_VR_MAX_M) return fail(PT_ERR_INVALID, "record count %d x %d outside [0, 2^31 - 1]", width, height);
  m = (long long)width * height;
  return PT_OK;
}

static int check_frame(int width, int height, const pt_variance_params *p, long long &m) {
  long long n;
  m = 0;
  if (int rc = check_size(width, height, n)) return rc;
  if (!p) return fail(PT_ERR_INVALID, "null pt_variance_params");
  if (p->passes < 1 || p->passes > 10) return fail(PT_ERR_INVALID, "passes = %d: 1 to 10", p->passes);
  if (p->normal_power_log2 < 0 || p->normal_power_log2 > 10) return fail(PT_ERR_INVALID, "normal_power_log2 = %d: 0 to 10", p->normal_power_log2);
  if (p->flags & ~(PT_VR_SAME_SHAPE | PT_VR_WRAP_X)) return fail(PT_ERR_INVALID, "unknown flag bits in 0x%x", (unsigned)p->flags);
  if (p->min_history < 1 || p->min_history > PT_VR_MAX_HISTORY) return fail(PT_ERR_INVALID, "min_history = %d: 1 to 2^20", p->min_history);
  if (!(p->sigma_point > 0.0)) return fail(PT_ERR_INVALID, "sigma_point = %g: a sigma is positive (or +inf)", p->sigma_point);
  if (!(p->sigma_luminance > 0.0)) return fail(PT_ERR_INVALID, "sigma_luminance = %g: a sigma is positive (or +inf)", p->sigma_luminance);
  if (!(p->epsilon > 0.0 && p->epsilon < __builtin_inf())) return fail(PT_ERR_INVALID, "epsilon = %g: positive and finite", p->epsilon);
  if (!(p->normal_min >= -1.0 && p->normal_min <= 1.0)) return fail(PT_ERR_INVALID, "normal_min = %g: a cosine, -1 to 1", p->normal_min);
  if (!(p->point_tolerance > 0.0)) return fail(PT_ERR_INVALID, "point_tolerance = %g: positive (or +inf)", p->point_tolerance);
  m = n;
  return PT_OK;
}

// 24 m (unit normals) + 8 m (g) + 32 m (the other colour and variance; only when passes > 1)
static size_t workspace_need(long long m, const pt_variance_params *p) { return (size_t)m * (p->passes > 1 ? 64 : 32); }

extern "C" size_t pt_rays_variance_workspace_bytes(int width, int height, const pt_variance_params *params) {
  long long m;
  return check_frame(width, height, params, m) ? 0 : workspace_need(m, params);
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

struct VrSpan {
  const void *at;
  size_t bytes;
  const char *name;
};

// every output against every input and against the outputs after it
static int check_overlaps(const VrSpan *outs, int n_outs, const VrSpan *reads, int n_reads) {
  for (int i = 0; i < n_outs; i++) {
    for (int j = 0; j < n_reads; j++)
      if (overlap(outs[i].at, outs[i].bytes, reads[j].at, reads[j].bytes))
        return fail(PT_ERR_INVALID, "%s overlaps %s", outs[i].name, reads[j].name);
    for (int j = i + 1; j < n_outs; j++)
      if (overlap(outs[i].at, outs[i].bytes, outs[j].at, outs[j].bytes))
        return fail(PT_ERR_INVALID, "%s overlaps %s", outs[i].name, outs[j].name);
  }
  return PT_OK;
}

static int check_moments(int device, int width, int height, const void *colour, const void *shape, const void *out, size_t out_bytes, long long &m) {
  if (int rc = check_size(width, height, m)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!colour || !shape) return fail(PT_ERR_INVALID, "null colour or shape planes");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  const size_t b3 = (size_t)m * 24, b1 = (size_t)m * 4;
  const VrSpan outs[1] = {{out, b3, "the moments output"}}, reads[2] = {{colour, b3, "the colour planes"}, {shape, b1, "the shapes"}};
  if (int rc = check_overlaps(outs, 1, reads, 2)) return rc;
  if (out_bytes < b3) return fail(PT_ERR_SIZE, "moments output too small: %zu < %zu bytes", out_bytes, b3);
  return PT_OK;
}

static int check_estimate(int device, int width, int height, const pt_variance_params *p, const void *moments, const void *count, const void *shape,
                          const void *normal, const void *point, const void *out, size_t out_bytes, long long &m) {
  if (int rc = check_frame(width, height, p, m)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!moments || !count || !shape || !normal || !point) return fail(PT_ERR_INVALID, "null moments, count, shape, normal or point planes");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  const size_t b3 = (size_t)m * 24, b2 = (size_t)m * 8, b1 = (size_t)m * 4;
  const VrSpan outs[1] = {{out, b2, "the variance output"}},
               reads[5] = {{moments, b3, "the moments"}, {count, b1, "the counts"}, {shape, b1, "the shapes"}, {normal, b3, "the normals"},
                           {point, b3, "the points"}};
  if (int rc = check_overlaps(outs, 1, reads, 5)) return rc;
  if (out_bytes < b2) return fail(PT_ERR_SIZE, "variance output too small: %zu < %zu bytes", out_bytes, b2);
  return PT_OK;
}

// `workspace` null is allowed where the host form makes it itself (need_ws = false)
static int check_filter(int device, int width, int height, const pt_variance_params *p, const void *colour, const void *variance, const void *normal,
                        const void *point, const void *shape, const void *out_colour, size_t out_colour_bytes, const void *out_variance,
                        size_t out_variance_bytes, bool need_ws, const void *ws, size_t ws_bytes, long long &m) {
  if (int rc = check_frame(width, height, p, m)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!colour || !variance || !normal || !point || !shape) return fail(PT_ERR_INVALID, "null colour, variance, normal, point or shape planes");
  if (!out_colour || !out_variance) return fail(PT_ERR_INVALID, "null output buffer");
  if (need_ws && !ws) return fail(PT_ERR_INVALID, "null workspace (pt_rays_variance_workspace_bytes sizes it)");
  const size_t b3 = (size_t)m * 24, b2 = (size_t)m * 8, b1 = (size_t)m * 4, wsb = workspace_need(m, p);
  const VrSpan outs[3] = {{out_colour, b3, "the colour output"}, {out_variance, b2, "the variance output"}, {ws, wsb, "the workspace"}},
               reads[5] = {{colour, b3, "the colour planes"}, {variance, b2, "the variance plane"}, {normal, b3, "the normals"},
                           {point, b3, "the points"}, {shape, b1, "the shapes"}};
  if (int rc = check_overlaps(outs, need_ws ? 3 : 2, reads, 5)) return rc;
  if (out_colour_bytes < b3) return fail(PT_ERR_SIZE, "colour output too small: %zu < %zu bytes", out_colour_bytes, b3);
  if (out_variance_bytes < b2) return fail(PT_ERR_SIZE, "variance output too small: %zu < %zu bytes", out_variance_bytes, b2);
  if (need_ws && ws_bytes < wsb) return fail(PT_ERR_SIZE, "workspace too small: %zu < %zu bytes", ws_bytes, wsb);
  return PT_OK;
}

// ---- launch alternatives --------------------------------------------------------------------------------------------------------
struct VrLaunch {
  bool direct;
  int tw, th;
  long long max_blocks;
};

static int launch_choice(VrLaunch &L) {
  L.direct = false;
  L.tw = 16, L.th = 16, L.max_blocks = PT_VR_MAX_GRID;
  if (const char *v = getenv("PTRACE_VR_VARIANT")) {
    if (!strcmp(v, "lds")) L.direct = false;
    else if (!strcmp(v, "direct")) L.direct = true;
    else return fail(PT_ERR_INVALID, "PTRACE_VR_VARIANT=%s: lds or direct", v);
  }
  if (const char *v = getenv("PTRACE_VR_TILE")) {
    if (!strcmp(v, "32x8")) L.tw = 32, L.th = 8;
    else if (!strcmp(v, "16x16")) L.tw = 16, L.th = 16;
    else if (!strcmp(v, "64x4")) L.tw = 64, L.th = 4;
    else return fail(PT_ERR_INVALID, "PTRACE_VR_TILE=%s: 16x16, 32x8 or 64x4", v);
  }
  if (const char *v = getenv("PTRACE_VR_BLOCKS")) {
    char *end = nullptr;
    const long long n = strtoll(v, &end, 10);
    if (end == v || *end || n < 1) return fail(PT_ERR_INVALID, "PTRACE_VR_BLOCKS=%s: a positive count of workgroups", v);
    L.max_blocks = std::min(n, PT_VR_MAX_GRID);
  }
  return PT_OK;
}

static PtVrK base_args(int width, int height, const pt_variance_params &p, long long m) {
  PtVrK K = {};
  K.W = width, K.H = height, K.s = 1, K.flags = p.flags, K.e = p.normal_power_log2, K.m = m;
  K.min_history = p.min_history, K.normal_min = p.normal_min, K.point_tolerance = p.point_tolerance;
  K.sl2 = p.sigma_luminance * p.sigma_luminance, K.epsilon = p.epsilon;
  K.sl_inf = std::isinf(K.sl2);
  K.nblocks = (m + PT_BLOCK - 1) / PT_BLOCK;
  return K;
}

static dim3 flat_grid(const VrLaunch &L, long long m) { return dim3((unsigned)std::min((m + PT_BLOCK - 1) / PT_BLOCK, L.max_blocks)); }

static int enqueue_moments(const VrLaunch &L, long long m, const double *colour, const int *shape, double *out, hipStream_t st) {
  hipLaunchKernelGGL(pt_vr_moments_kernel, flat_grid(L, m), dim3(PT_BLOCK), 0, st, colour, shape, m, out);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_estimate(const VrLaunch &L, int width, int height, const pt_variance_params &p, long long m, const double *moments,
                            const int *count, const int *shape, const double *normal, const double *point, double *out, hipStream_t st) {
  const PtVrK K = base_args(width, height, p, m);
  hipLaunchKernelGGL(pt_vr_estimate_kernel, flat_grid(L, m), dim3(PT_BLOCK), 0, st, K, moments, count, shape, normal, point, out);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// the pre-pass and the passes; the workspace is `unit` [3, m], `g` [m] and, when passes > 1, `other` [3, m] and `other_var` [m]
static int enqueue_filter(const VrLaunch &L, int width, int height, const pt_variance_params &p, long long m, const double *colour,
                          const double *variance, const double *normal, const double *point, const int *shape, double *out, double *out_var,
                          double *ws, hipStream_t st) {
  double *unit = ws, *g = ws + 3 * m, *other = ws + 4 * m, *other_var = ws + 7 * m;
  const dim3 flat = flat_grid(L, m);
  hipLaunchKernelGGL(pt_vr_unit_kernel, flat, dim3(PT_BLOCK), 0, st, normal, m, unit);
  HIP_TRY(hipGetLastError());
  const double *src = colour, *src_var = variance;
  for (int i = 0; i < p.passes; i++) {
    const bool last = (p.passes - 1 - i) % 2 == 0;  // (the last pass lands in the outputs)
    double *dst = last ? out : other, *dst_var = last ? out_var : other_var;
    PtVrK K = base_args(width, height, p, m);
    K.s = 1 << i;
    K.rxn = std::min(K.s, width), K.ryn = std::min(K.s, height);
    K.sps = p.sigma_point * (double)K.s;
    K.sp_inf = std::isinf(K.sps);
    hipLaunchKernelGGL(pt_vr_prefilter_kernel, flat, dim3(PT_BLOCK), 0, st, K, src_var, shape, g);
    HIP_TRY(hipGetLastError());
    const long long sw = ((long long)width + K.s - 1) / K.s, sh = ((long long)height + K.s - 1) / K.s;  // the widest, tallest sub-lattice
    K.tiles_x = (int)((sw + L.tw - 1) / L.tw), K.tiles_y = (int)((sh + L.th - 1) / L.th);
    if (!L.direct) K.nblocks = (long long)K.tiles_x * K.rxn * ((long long)K.tiles_y * K.ryn);
    const dim3 grid((unsigned)std::min(K.nblocks, L.max_blocks));
    const double *cg = g, *cu = unit;
    if (L.direct) hipLaunchKernelGGL(pt_vr_direct_kernel, grid, dim3(PT_BLOCK), 0, st, K, src, src_var, cg, cu, point, shape, dst, dst_var);
    else if (L.tw == 32) hipLaunchKernelGGL((pt_vr_lds_kernel<32, 8>), grid, dim3(PT_BLOCK), 0, st, K, src, src_var, cg, cu, point, shape, dst, dst_var);
    else if (L.tw == 16) hipLaunchKernelGGL((pt_vr_lds_kernel<16, 16>), grid, dim3(PT_BLOCK), 0, st, K, src, src_var, cg, cu, point, shape, dst, dst_var);
    else hipLaunchKernelGGL((pt_vr_lds_kernel<64, 4>), grid, dim3(PT_BLOCK), 0, st, K, src, src_var, cg, cu, point, shape, dst, dst_var);
    HIP_TRY(hipGetLastError());
    src = dst, src_var = dst_var;
  }
  return PT_OK;
}

// ---- the device forms -----------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_variance_moments_device(int device, int width, int height, const double *colour_dev, const int *shape_dev, void *out_dev,
                                               size_t out_bytes, void *stream) {
  long long m;
  VrLaunch L;
  int rc = check_moments(device, width, height, colour_dev, shape_dev, out_dev, out_bytes, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_moments(L, m, colour_dev, shape_dev, (double *)out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_variance_estimate_device(int device, int width, int height, const pt_variance_params *params, const double *moments_dev,
                                                const int *count_dev, const int *shape_dev, const double *normal_dev, const double *point_dev,
                                                void *out_dev, size_t out_bytes, void *stream) {
  long long m;
  VrLaunch L;
  int rc = check_estimate(device, width, height, params, moments_dev, count_dev, shape_dev, normal_dev, point_dev, out_dev, out_bytes, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_estimate(L, width, height, *params, m, moments_dev, count_dev, shape_dev, normal_dev, point_dev, (double *)out_dev,
                             (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_variance_filter_device(int device, int width, int height, const pt_variance_params *params, const double *colour_dev,
                                              const double *variance_dev, const double *normal_dev, const double *point_dev, const int *shape_dev,
                                              void *out_colour_dev, size_t out_colour_bytes, void *out_variance_dev, size_t out_variance_bytes,
                                              void *workspace_dev, size_t workspace_bytes, void *stream) {
  long long m;
  VrLaunch L;
  int rc = check_filter(device, width, height, params, colour_dev, variance_dev, normal_dev, point_dev, shape_dev, out_colour_dev, out_colour_bytes,
                        out_variance_dev, out_variance_bytes, true, workspace_dev, workspace_bytes, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_filter(L, width, height, *params, m, colour_dev, variance_dev, normal_dev, point_dev, shape_dev, (double *)out_colour_dev,
                           (double *)out_variance_dev, (double *)workspace_dev, (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- the host forms: one device allocation holds the inputs, the workspace and the outputs -------------------------------------------
extern "C" int pt_rays_variance_moments(int device, int width, int height, const double *colour_host, const int *shape_host, void *out_host,
                                        size_t out_bytes) {
  long long m;
  VrLaunch L;
  int rc = check_moments(device, width, height, colour_host, shape_host, out_host, out_bytes, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b3 = (size_t)m * 24, b1 = up8((size_t)m * 4);
  Staged s;
  if ((rc = s.alloc(2 * b3 + b1))) return rc;
  char *col_d = s.dev, *out_d = col_d + b3, *shape_d = out_d + b3;
  HIP_TRY(hipMemcpy(col_d, colour_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_moments(L, m, (const double *)col_d, (const int *)shape_d, (double *)out_d, nullptr))) return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, b3, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}

extern "C" int pt_rays_variance_estimate(int device, int width, int height, const pt_variance_params *params, const double *moments_host,
                                         const int *count_host, const int *shape_host, const double *normal_host, const double *point_host,
                                         void *out_host, size_t out_bytes) {
  long long m;
  VrLaunch L;
  int rc = check_estimate(device, width, height, params, moments_host, count_host, shape_host, normal_host, point_host, out_host, out_bytes, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b3 = (size_t)m * 24, b2 = (size_t)m * 8, b1 = up8((size_t)m * 4);
  Staged s;
  if ((rc = s.alloc(3 * b3 + b2 + 2 * b1))) return rc;
  char *mom_d = s.dev, *nrm_d = mom_d + b3, *pnt_d = nrm_d + b3, *out_d = pnt_d + b3, *cnt_d = out_d + b2, *shape_d = cnt_d + b1;
  HIP_TRY(hipMemcpy(mom_d, moments_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(nrm_d, normal_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(pnt_d, point_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(cnt_d, count_host, (size_t)m * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_estimate(L, width, height, *params, m, (const double *)mom_d, (const int *)cnt_d, (const int *)shape_d, (const double *)nrm_d,
                             (const double *)pnt_d, (double *)out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, b2, hipMemcpyDeviceToHost));
  return PT_OK;
}

extern "C" int pt_rays_variance_filter(int device, int width, int height, const pt_variance_params *params, const double *colour_host,
                                       const double *variance_host, const double *normal_host, const double *point_host, const int *shape_host,
                                       void *out_colour_host, size_t out_colour_bytes, void *out_variance_host, size_t out_variance_bytes) {
  long long m;
  VrLaunch L;
  int rc = check_filter(device, width, height, params, colour_host, variance_host, normal_host, point_host, shape_host, out_colour_host,
                        out_colour_bytes, out_variance_host, out_variance_bytes, false, nullptr, 0, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b3 = (size_t)m * 24, b2 = (size_t)m * 8, b1 = up8((size_t)m * 4), ws_b = workspace_need(m, params);
  Staged s;
  if ((rc = s.alloc(4 * b3 + 2 * b2 + ws_b + b1))) return rc;
  char *col_d = s.dev, *nrm_d = col_d + b3, *pnt_d = nrm_d + b3, *out_d = pnt_d + b3, *var_d = out_d + b3, *ovar_d = var_d + b2, *ws_d = ovar_d + b2,
       *shape_d = ws_d + ws_b;
  HIP_TRY(hipMemcpy(col_d, colour_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(nrm_d, normal_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(pnt_d, point_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(var_d, variance_host, b2, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_filter(L, width, height, *params, m, (const double *)col_d, (const double *)var_d, (const double *)nrm_d, (const double *)pnt_d,
                           (const int *)shape_d, (double *)out_d, (double *)ovar_d, (double *)ws_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_colour_host, out_d, b3, hipMemcpyDeviceToHost));  // (the null stream: behind the kernels)
  HIP_TRY(hipMemcpy(out_variance_host, ovar_d, b2, hipMemcpyDeviceToHost));
  return PT_OK;
}
