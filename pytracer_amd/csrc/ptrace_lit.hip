// ptrace_lit.hip — libptrace_lit.so: the C-ABI of include/ptrace_lit.h, hit records shaded from a lattice of SH radiance probes.
//
// What it restates: ProbeGrid.corners and ProbeGrid.blend (pytracer_amd/rays.py), the evaluation of include/ptrace_sh.h, the pigment
// look-up (materials.py:50-100) and the mirror direction of materials.py:186-192.  The kernels are pt_lit.h's; the pigments and the
// vector arithmetic are pt_shade.h's and pt_math.h's, included here as they are.
//
// Why a ninth translation unit and a ninth shared object: libptrace.so's device code is pinned by build.code_hash (every
// profiles/pmc_*.json names it), and the exported symbols of the seven add-ons beside it are pinned to their interfaces'.
// So this library stands beside them: the scene arrives as the argument block pt_scene_kernel_args (ptrace.h, ABI 1.7) hands
// out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ptrace_lit.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_lit.h"
#include "pt_host_common.h"

#define PT_LIT_VERSION ((1 << 16) | 7)
#define PT_LIT_MAX_N 2147483647LL  // the grid is m / 256 blocks in x

extern "C" int pt_rays_lit_version(void) { return PT_LIT_VERSION; }

extern "C" size_t pt_rays_lit_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_lit_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static bool count_ok(long long n) { return n >= 0 && n <= PT_LIT_MAX_N; }

extern "C" size_t pt_rays_lit_bytes(long long m) { return count_ok(m) ? (size_t)m * 24 : 0; }

// the lattice: every field, and n = nx ny nz without overflow
static int check_grid(const pt_lit_grid *g, long long &n) {
  n = 0;
  if (!g) return fail(PT_ERR_INVALID, "null pt_lit_grid");
  for (int a = 0; a < 3; a++) {
    if (g->dims[a] < 1) return fail(PT_ERR_INVALID, "dims[%d] = %d: a lattice has at least one probe along every axis", a, g->dims[a]);
    if (!(g->step[a] > 0.0) || !std::isfinite(g->step[a])) return fail(PT_ERR_INVALID, "step[%d] = %g: a step is positive and finite", a, g->step[a]);
    if (!std::isfinite(g->origin[a])) return fail(PT_ERR_INVALID, "origin[%d] = %g: the origin is finite", a, g->origin[a]);
  }
  long long rows = (long long)g->dims[0] * g->dims[1];  // (< 2^62)
  if (rows > PT_LIT_MAX_N || rows * g->dims[2] > PT_LIT_MAX_N)
    return fail(PT_ERR_INVALID, "probe count %d x %d x %d outside [0, 2^31 - 1]", g->dims[0], g->dims[1], g->dims[2]);
  n = rows * g->dims[2];
  return PT_OK;
}

extern "C" size_t pt_rays_lit_coeffs_bytes(const pt_lit_grid *grid) {
  long long n;
  return check_grid(grid, n) ? 0 : (size_t)n * 8 * PT_LIT_COEFFS;
}

static size_t slots_need(const void *scene_args) { return up8((size_t)((const PtKArgs *)scene_args)->n_shapes * 4); }

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
static int check_batch(int device, const pt_lit_grid *grid, const void *coeffs, size_t coeffs_bytes, long long m, const void *out, size_t out_bytes,
                       long long &n, size_t &need) {
  need = 0;
  if (int rc = check_grid(grid, n)) return rc;
  if (!count_ok(m)) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", m);
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  need = pt_rays_lit_bytes(m);
  if (m == 0) return PT_OK;
  if (!coeffs) return fail(PT_ERR_INVALID, "null coefficient block");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (coeffs_bytes < (size_t)n * 8 * PT_LIT_COEFFS)
    return fail(PT_ERR_SIZE, "coefficient block too small: %zu < %zu bytes (27 planes of %lld probes)", coeffs_bytes, (size_t)n * 8 * PT_LIT_COEFFS, n);
  if (out_bytes < need) return fail(PT_ERR_SIZE, "lit output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

static int check_eval(int device, const pt_lit_grid *grid, const void *coeffs, size_t coeffs_bytes, const double *points, const double *dirs, long long m,
                      int kind, const void *out, size_t out_bytes, long long &n, size_t &need) {
  need = 0;
  if (kind != PT_LIT_RADIANCE && kind != PT_LIT_HEMISPHERE)
    return fail(PT_ERR_INVALID, "kind %d: an evaluation is PT_LIT_RADIANCE or PT_LIT_HEMISPHERE", kind);
  if (int rc = check_batch(device, grid, coeffs, coeffs_bytes, m, out, out_bytes, n, need)) return rc;
  if (m == 0) return PT_OK;
  if (!points) return fail(PT_ERR_INVALID, "null points planes");
  if (!dirs) return fail(PT_ERR_INVALID, "null directions planes");
  return PT_OK;
}

// `slots` null is allowed where the host form makes the table itself (need_slots = false)
static int check_shade(int device, const void *scene_args, size_t scene_args_bytes, bool need_slots, const void *slots, size_t slots_bytes,
                       const pt_lit_grid *grid, const void *coeffs, size_t coeffs_bytes, const int *shape, const double *point, const double *normal,
                       const double *uv, const double *dir, long long m, const double *background, const void *out, size_t out_bytes, long long &n,
                       size_t &need) {
  need = 0;
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  if (!background) return fail(PT_ERR_INVALID, "null background colour");
  if (int rc = check_batch(device, grid, coeffs, coeffs_bytes, m, out, out_bytes, n, need)) return rc;
  if (m == 0) return PT_OK;
  if (!shape || !point || !normal || !uv || !dir) return fail(PT_ERR_INVALID, "null shape, point, normal, uv or dir planes");
  if (need_slots) {
    if (!slots) return fail(PT_ERR_INVALID, "null slot table (pt_rays_slots_device makes it)");
    if (slots_bytes < slots_need(scene_args)) return fail(PT_ERR_SIZE, "slot table too small: %zu < %zu bytes", slots_bytes, slots_need(scene_args));
  }
  return PT_OK;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
static PtLitK kernel_grid(const pt_lit_grid &g, long long n) {
  PtLitK K;
  for (int a = 0; a < 3; a++) {
    K.origin[a] = g.origin[a];
    K.step[a] = g.step[a];
    K.dims[a] = g.dims[a];
  }
  K.n = n;
  return K;
}

static int enqueue_slots(const void *scene_args, void *slots_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  if (a.n_shapes == 0) return PT_OK;
  hipLaunchKernelGGL(pt_lit_slots_kernel, grid_of(a.n_shapes), dim3(PT_BLOCK), 0, st, a, (int *)slots_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_eval(const pt_lit_grid &grid, long long n, const double *coeffs_dev, const double *points_dev, const double *dirs_dev,
                        const int *active_dev, long long m, int kind, void *out_dev, hipStream_t st) {
  hipLaunchKernelGGL(pt_lit_eval_kernel, grid_of(m), dim3(PT_BLOCK), 0, st, kernel_grid(grid, n), coeffs_dev, points_dev, dirs_dev, active_dev, m, kind,
                     (double *)out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_shade(const void *scene_args, const void *slots_dev, const pt_lit_grid &grid, long long n, const double *coeffs_dev,
                         const int *shape_dev, const double *point_dev, const double *normal_dev, const double *uv_dev, const double *dir_dev,
                         long long m, const double *background, void *out_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  const V3 bg = {background[0], background[1], background[2]};
  hipLaunchKernelGGL(pt_lit_shade_kernel, grid_of(m), dim3(PT_BLOCK), 0, st, a, (const int *)slots_dev, kernel_grid(grid, n), coeffs_dev, shape_dev,
                     point_dev, normal_dev, uv_dev, dir_dev, m, bg, (double *)out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device forms -----------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_lit_eval_device(int device, const pt_lit_grid *grid, const double *coeffs_dev, size_t coeffs_bytes, const double *points_dev,
                                       const double *dirs_dev, const int *active_dev, long long m, int kind, void *out_dev, size_t out_bytes,
                                       void *stream) {
  long long n;
  size_t need;
  int rc = check_eval(device, grid, coeffs_dev, coeffs_bytes, points_dev, dirs_dev, m, kind, out_dev, out_bytes, n, need);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_eval(*grid, n, coeffs_dev, points_dev, dirs_dev, active_dev, m, kind, out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_lit_shade_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev, size_t slots_bytes,
                                        const pt_lit_grid *grid, const double *coeffs_dev, size_t coeffs_bytes, const int *shape_dev,
                                        const double *point_dev, const double *normal_dev, const double *uv_dev, const double *dir_dev, long long m,
                                        const double *background, void *out_dev, size_t out_bytes, void *stream) {
  long long n;
  size_t need;
  int rc = check_shade(device, scene_args, scene_args_bytes, true, slots_dev, slots_bytes, grid, coeffs_dev, coeffs_bytes, shape_dev, point_dev,
                       normal_dev, uv_dev, dir_dev, m, background, out_dev, out_bytes, n, need);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_shade(scene_args, slots_dev, *grid, n, coeffs_dev, shape_dev, point_dev, normal_dev, uv_dev, dir_dev, m, background, out_dev,
                          (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host forms: one device allocation holds the tables, the input planes and the output -----------------------------------------
extern "C" int pt_rays_lit_eval(int device, const pt_lit_grid *grid, const double *coeffs_host, size_t coeffs_bytes, const double *points_host,
                                const double *dirs_host, const int *active_host, long long m, int kind, void *out_host, size_t out_bytes) {
  long long n;
  size_t need;
  int rc = check_eval(device, grid, coeffs_host, coeffs_bytes, points_host, dirs_host, m, kind, out_host, out_bytes, n, need);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t co_b = (size_t)n * 8 * PT_LIT_COEFFS, plane3 = (size_t)m * 24, act_b = up8((size_t)m * 4);
  Staged s;
  if ((rc = s.alloc(co_b + 2 * plane3 + act_b + need))) return rc;
  char *co_d = s.dev, *pts_d = co_d + co_b, *dir_d = pts_d + plane3, *act_d = dir_d + plane3, *out_d = act_d + act_b;
  HIP_TRY(hipMemcpy(co_d, coeffs_host, co_b, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(pts_d, points_host, plane3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dir_d, dirs_host, plane3, hipMemcpyHostToDevice));
  if (active_host) HIP_TRY(hipMemcpy(act_d, active_host, (size_t)m * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_eval(*grid, n, (const double *)co_d, (const double *)pts_d, (const double *)dir_d, active_host ? (const int *)act_d : nullptr, m,
                         kind, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}

extern "C" int pt_rays_lit_shade(int device, const void *scene_args, size_t scene_args_bytes, const pt_lit_grid *grid, const double *coeffs_host,
                                 size_t coeffs_bytes, const int *shape_host, const double *point_host, const double *normal_host,
                                 const double *uv_host, const double *dir_host, long long m, const double *background, void *out_host,
                                 size_t out_bytes) {
  long long n;
  size_t need;
  int rc = check_shade(device, scene_args, scene_args_bytes, false, nullptr, 0, grid, coeffs_host, coeffs_bytes, shape_host, point_host, normal_host,
                       uv_host, dir_host, m, background, out_host, out_bytes, n, need);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t slots_b = std::max<size_t>(slots_need(scene_args), 8), co_b = (size_t)n * 8 * PT_LIT_COEFFS, shape_b = up8((size_t)m * 4),
               plane = (size_t)m * 8;
  Staged s;
  if ((rc = s.alloc(slots_b + co_b + shape_b + 11 * plane + need))) return rc;
  char *slots_d = s.dev, *co_d = slots_d + slots_b, *shape_d = co_d + co_b, *point_d = shape_d + shape_b, *normal_d = point_d + 3 * plane,
       *uv_d = normal_d + 3 * plane, *dir_d = uv_d + 2 * plane, *out_d = dir_d + 3 * plane;
  HIP_TRY(hipMemcpy(co_d, coeffs_host, co_b, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(point_d, point_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(normal_d, normal_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(uv_d, uv_host, 2 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dir_d, dir_host, 3 * plane, hipMemcpyHostToDevice));
  if ((rc = enqueue_slots(scene_args, slots_d, nullptr))) return rc;
  if ((rc = enqueue_shade(scene_args, slots_d, *grid, n, (const double *)co_d, (const int *)shape_d, (const double *)point_d,
                          (const double *)normal_d, (const double *)uv_d, (const double *)dir_d, m, background, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernels)
  return PT_OK;
}
