// ptrace_scatter.hip — libptrace_scatter.so: the C-ABI of include/ptrace_scatter.h, BRDF.scatter_ray and the roulette for hit records.
//
// What it restates: render.py:107-134 for one child of a hit (pigments, Russian roulette, brdf.scatter_ray) for records the
// CALLER supplies, as planes, each with its own generator.  The kernel is pt_scatter.h's; the draws are pt_math.h's pcg_float,
// the bounce is pt_shade.h's scatter_ray, included here as they are.
//
// Why a fourth translation unit and a fourth shared object: libptrace.so's device code is pinned by build.code_hash (every
// profiles/pmc_*.json names it), libptrace_rays.so's exported symbols are pinned to the seven of its interface 1.0 and
// libptrace_surface.so's to its eleven.  So this library stands beside them: the scene arrives as the argument block
// pt_scene_kernel_args (ptrace.h, ABI 1.7) hands out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_scatter.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_scatter.h"
#include "pt_host_common.h"

#define PT_SCAT_VERSION ((1 << 16) | 2)
#define PT_SCAT_MAX_N 2147483647LL  // the grid is n / 256 blocks in x

extern "C" int pt_rays_scatter_version(void) { return PT_SCAT_VERSION; }

extern "C" size_t pt_rays_scatter_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_scatter_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static bool shape_ok(long long n, int channels) { return n >= 0 && n <= PT_SCAT_MAX_N && channels >= 0 && !(channels & ~PT_SCAT_ALL); }

static long long pad_of(long long n) { return (n * 4 + 7) & ~7LL; }

extern "C" size_t pt_rays_scatter_bytes(long long n, int channels) {
  if (!shape_ok(n, channels)) return 0;
  const int colours = ((channels & PT_SCAT_WEIGHT) ? 1 : 0) + ((channels & PT_SCAT_EMITTED) ? 1 : 0);
  return (size_t)pad_of(n) + (size_t)n * 8 * (size_t)(10 + 3 * colours);
}

extern "C" long long pt_rays_scatter_plane_offset(long long n, int channels, int channel, int component) {
  if (!shape_ok(n, channels)) return PT_ERR_INVALID;
  if (channel == 0) return component == 0 ? 0 : PT_ERR_INVALID;
  if (component < 0) return PT_ERR_INVALID;
  if (channel == PT_SCAT_RAYS) return component < 8 ? pad_of(n) + n * 8 * component : PT_ERR_INVALID;
  if (channel == PT_SCAT_PCG) return component < 2 ? pad_of(n) + n * 8 * (8 + component) : PT_ERR_INVALID;
  if ((channel != PT_SCAT_WEIGHT && channel != PT_SCAT_EMITTED) || !(channels & channel) || component >= 3) return PT_ERR_INVALID;
  const long long before = (channel == PT_SCAT_EMITTED && (channels & PT_SCAT_WEIGHT)) ? 3 : 0;
  return pad_of(n) + n * 8 * (10 + before + component);
}

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
// `slots` null is allowed where the host form makes the table itself (need_slots = false)
static int check_args(int device, const void *scene_args, size_t scene_args_bytes, bool need_slots, const void *slots, const int *shape,
                      const double *point, const double *normal, const double *uv, const double *dir, const unsigned long long *pcg_state,
                      const unsigned long long *pcg_inc, long long n, int roulette, int channels, const void *out, size_t out_bytes,
                      size_t &need) {
  need = 0;
  if (n < 0 || n > PT_SCAT_MAX_N) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", n);
  if (roulette != 0 && roulette != 1) return fail(PT_ERR_INVALID, "roulette must be 0 or 1, not %d", roulette);
  if (channels < 0 || (channels & ~PT_SCAT_ALL))
    return fail(PT_ERR_INVALID, "channel bits %#x: a scatter batch has PT_SCAT_WEIGHT | PT_SCAT_EMITTED", channels);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  need = pt_rays_scatter_bytes(n, channels);
  if (n == 0) return PT_OK;
  if (need_slots && !slots) return fail(PT_ERR_INVALID, "null slot table (pt_rays_slots_device makes it)");
  if (!shape || !point || !normal || !uv || !dir) return fail(PT_ERR_INVALID, "null shape, point, normal, uv or dir planes");
  if (!pcg_state || !pcg_inc) return fail(PT_ERR_INVALID, "null generator planes (state, inc)");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "scatter output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
static int enqueue_slots(const void *scene_args, void *slots_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  if (a.n_shapes == 0) return PT_OK;
  hipLaunchKernelGGL(pt_scatter_slots_kernel, grid_of(a.n_shapes), dim3(PT_BLOCK), 0, st, a, (int *)slots_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_scatter(const void *scene_args, const void *slots_dev, const int *shape_dev, const double *point_dev, const double *normal_dev,
                           const double *uv_dev, const double *dir_dev, const unsigned long long *state_dev, const unsigned long long *inc_dev,
                           long long n, int roulette, int channels, void *out_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  hipLaunchKernelGGL(pt_scatter_kernel, grid_of(n), dim3(PT_BLOCK), 0, st, a, (const int *)slots_dev, shape_dev, point_dev, normal_dev, uv_dev,
                     dir_dev, state_dev, inc_dev, n, roulette, channels, out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device form ------------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_scatter_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev, const int *shape_dev,
                                      const double *point_dev, const double *normal_dev, const double *uv_dev, const double *dir_dev,
                                      const unsigned long long *pcg_state_dev, const unsigned long long *pcg_inc_dev, long long n,
                                      int roulette, int channels, void *out_dev, size_t out_bytes, void *stream) {
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, true, slots_dev, shape_dev, point_dev, normal_dev, uv_dev, dir_dev, pcg_state_dev,
                      pcg_inc_dev, n, roulette, channels, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_scatter(scene_args, slots_dev, shape_dev, point_dev, normal_dev, uv_dev, dir_dev, pcg_state_dev, pcg_inc_dev, n, roulette,
                            channels, out_dev, (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host form: one device allocation holds the slot table, the input planes and the output -------------------------------------
extern "C" int pt_rays_scatter(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host, const double *point_host,
                               const double *normal_host, const double *uv_host, const double *dir_host,
                               const unsigned long long *pcg_state_host, const unsigned long long *pcg_inc_host, long long n, int roulette,
                               int channels, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, false, nullptr, shape_host, point_host, normal_host, uv_host, dir_host,
                      pcg_state_host, pcg_inc_host, n, roulette, channels, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t slots_b = std::max<size_t>(up8((size_t)((const PtKArgs *)scene_args)->n_shapes * 4), 8), shape_b = up8((size_t)n * 4),
               plane = (size_t)n * 8;
  const size_t total = slots_b + shape_b + 13 * plane + need;
  Staged s;
  if ((rc = s.alloc(total))) return rc;
  char *slots_d = s.dev, *shape_d = slots_d + slots_b, *point_d = shape_d + shape_b, *normal_d = point_d + 3 * plane, *uv_d = normal_d + 3 * plane,
       *dir_d = uv_d + 2 * plane, *state_d = dir_d + 3 * plane, *inc_d = state_d + plane, *out_d = inc_d + plane;
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(point_d, point_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(normal_d, normal_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(uv_d, uv_host, 2 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dir_d, dir_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(state_d, pcg_state_host, plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(inc_d, pcg_inc_host, plane, hipMemcpyHostToDevice));
  if ((rc = enqueue_slots(scene_args, slots_d, nullptr))) return rc;
  if ((rc = enqueue_scatter(scene_args, slots_d, (const int *)shape_d, (const double *)point_d, (const double *)normal_d, (const double *)uv_d,
                            (const double *)dir_d, (const unsigned long long *)state_d, (const unsigned long long *)inc_d, n, roulette, channels,
                            out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernels)
  return PT_OK;
}
