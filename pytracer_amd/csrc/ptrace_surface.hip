// ptrace_surface.hip — libptrace_surface.so: the C-ABI of include/ptrace_surface.h, materials and point-light shading of hit records.
//
// What it restates: the pigment look-up (materials.py:50-100) and PointLightRenderer.__call__ (render.py:157-193) for records
// the CALLER supplies, as planes.  The kernels are pt_surface.h's; the shadow rays go through pt_query.h's world_query_lanes
// and the pigments through pt_shade.h's pigment_color, included here as they are.
//
// Why a third translation unit and a third shared object: libptrace.so's device code is pinned by build.code_hash (every
// profiles/pmc_*.json names it), and libptrace_rays.so's exported symbols are pinned to the seven of its interface 1.0.  So
// this library stands beside them the way libptrace_rays.so stands beside libptrace.so: the scene arrives as the argument
// block pt_scene_kernel_args (ptrace.h, ABI 1.7) hands out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_surface.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_surface.h"
#include "pt_host_common.h"

#define PT_SURF_VERSION ((1 << 16) | 1)
#define PT_SURF_MAX_N 2147483647LL  // the grid is n / 256 blocks in x

extern "C" int pt_rays_surface_version(void) { return PT_SURF_VERSION; }

extern "C" size_t pt_rays_surface_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_surface_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static bool block_ok(const void *scene_args, size_t scene_args_bytes) {
  return scene_args && scene_args_bytes == sizeof(PtKArgs) && ((const PtKArgs *)scene_args)->cold && ((const PtKArgs *)scene_args)->n_shapes >= 0;
}

static size_t slots_need(const void *scene_args) { return ((size_t)((const PtKArgs *)scene_args)->n_shapes * 4 + 7) & ~(size_t)7; }

extern "C" size_t pt_rays_slots_bytes(const void *scene_args, size_t scene_args_bytes) {
  return block_ok(scene_args, scene_args_bytes) ? slots_need(scene_args) : 0;
}

static bool shape_ok(long long n, int channels) { return n >= 0 && n <= PT_SURF_MAX_N && channels >= 0 && !(channels & ~PT_SURF_ALL); }

extern "C" size_t pt_rays_surface_bytes(long long n, int channels) {
  if (!shape_ok(n, channels)) return 0;
  const int colours = ((channels & PT_SURF_BRDF_COLOR) ? 1 : 0) + ((channels & PT_SURF_EMITTED) ? 1 : 0);
  return (size_t)((n * 4 + 7) & ~7LL) + (size_t)n * 8 * 3 * (size_t)colours;
}

extern "C" long long pt_rays_surface_plane_offset(long long n, int channels, int channel, int component) {
  if (!shape_ok(n, channels)) return PT_ERR_INVALID;
  if (channel == 0) return component == 0 ? 0 : PT_ERR_INVALID;
  if ((channel != PT_SURF_BRDF_COLOR && channel != PT_SURF_EMITTED) || !(channels & channel) || component < 0 || component >= 3) return PT_ERR_INVALID;
  const long long before = (channel == PT_SURF_EMITTED && (channels & PT_SURF_BRDF_COLOR)) ? 3 : 0;
  return ((n * 4 + 7) & ~7LL) + n * 8 * (before + component);
}

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
static int check_block(int device, const void *scene_args, size_t scene_args_bytes) {
  return check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES | PT_BLOCK_LIGHTS);
}

static int check_count(long long n) {
  if (n < 0 || n > PT_SURF_MAX_N) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", n);
  return PT_OK;
}

// `slots` null is allowed where the host forms make the table themselves (need_slots = false)
static int check_surface(int device, const void *scene_args, size_t scene_args_bytes, bool need_slots, const void *slots, const int *shape,
                         const double *uv, long long n, int channels, const void *out, size_t out_bytes, size_t &need) {
  need = 0;
  int rc = check_count(n);
  if (rc) return rc;
  if (channels < 0 || (channels & ~PT_SURF_ALL))
    return fail(PT_ERR_INVALID, "channel bits %#x: a surface batch has PT_SURF_BRDF_COLOR | PT_SURF_EMITTED", channels);
  if ((rc = check_block(device, scene_args, scene_args_bytes))) return rc;
  need = pt_rays_surface_bytes(n, channels);
  if (n == 0) return PT_OK;
  if (need_slots && !slots) return fail(PT_ERR_INVALID, "null slot table (pt_rays_slots_device makes it)");
  if (!shape || !out) return fail(PT_ERR_INVALID, "null shape plane or output buffer");
  if (channels != 0 && !uv) return fail(PT_ERR_INVALID, "null uv planes: a colour channel is selected");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "surface output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

static int check_lights(int device, const void *scene_args, size_t scene_args_bytes, bool need_slots, const void *slots, const int *shape,
                        const double *point, const double *normal, const double *uv, const double *dir, long long n, const double *ambient,
                        const double *background, const void *out, size_t out_bytes, size_t &need) {
  need = 0;
  int rc = check_count(n);
  if (rc) return rc;
  if ((rc = check_block(device, scene_args, scene_args_bytes))) return rc;
  if (!ambient || !background) return fail(PT_ERR_INVALID, "null ambient or background colour");
  need = (size_t)n * 24;
  if (n == 0) return PT_OK;
  if (need_slots && !slots) return fail(PT_ERR_INVALID, "null slot table (pt_rays_slots_device makes it)");
  if (!shape || !point || !normal || !uv || !dir || !out) return fail(PT_ERR_INVALID, "null shape, point, normal, uv or dir planes, or null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "shading output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
static int enqueue_slots(const void *scene_args, void *slots_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  if (a.n_shapes == 0) return PT_OK;
  hipLaunchKernelGGL(pt_slots_kernel, grid_of(a.n_shapes), dim3(PT_BLOCK), 0, st, a, (int *)slots_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_surface(const void *scene_args, const void *slots_dev, const int *shape_dev, const double *uv_dev, long long n, int channels,
                           void *out_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  hipLaunchKernelGGL(pt_surface_kernel, grid_of(n), dim3(PT_BLOCK), 0, st, a, (const int *)slots_dev, shape_dev, uv_dev, n, channels, out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_lights(const void *scene_args, const void *slots_dev, const int *shape_dev, const double *point_dev, const double *normal_dev,
                          const double *uv_dev, const double *dir_dev, long long n, const double *ambient, const double *background,
                          void *out_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  const V3 amb = {ambient[0], ambient[1], ambient[2]}, bg = {background[0], background[1], background[2]};
  hipLaunchKernelGGL(pt_shade_lights_kernel, grid_of(n), dim3(PT_BLOCK), 0, st, a, (const int *)slots_dev, shape_dev, point_dev, normal_dev, uv_dev,
                     dir_dev, n, amb, bg, (double *)out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device forms -----------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_slots_device(int device, const void *scene_args, size_t scene_args_bytes, void *slots_dev, size_t slots_bytes,
                                    void *stream) {
  int rc = check_block(device, scene_args, scene_args_bytes);
  if (rc) return rc;
  const size_t need = slots_need(scene_args);
  if (need == 0) return PT_OK;  // a scene without shapes: nothing to write
  if (!slots_dev) return fail(PT_ERR_INVALID, "null slot table");
  if (slots_bytes < need) return fail(PT_ERR_SIZE, "slot table too small: %zu < %zu bytes", slots_bytes, need);
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_slots(scene_args, slots_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_surface_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev, const int *shape_dev,
                                      const double *uv_dev, long long n, int channels, void *out_dev, size_t out_bytes, void *stream) {
  size_t need;
  int rc = check_surface(device, scene_args, scene_args_bytes, true, slots_dev, shape_dev, uv_dev, n, channels, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_surface(scene_args, slots_dev, shape_dev, uv_dev, n, channels, out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_shade_lights_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev, const int *shape_dev,
                                           const double *point_dev, const double *normal_dev, const double *uv_dev, const double *dir_dev,
                                           long long n, const double *ambient, const double *background, void *out_dev, size_t out_bytes,
                                           void *stream) {
  size_t need;
  int rc = check_lights(device, scene_args, scene_args_bytes, true, slots_dev, shape_dev, point_dev, normal_dev, uv_dev, dir_dev, n, ambient,
                        background, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_lights(scene_args, slots_dev, shape_dev, point_dev, normal_dev, uv_dev, dir_dev, n, ambient, background, out_dev,
                           (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host forms: one device allocation holds the slot table, the input planes and the output -------------------------------------
extern "C" int pt_rays_surface(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host, const double *uv_host,
                               long long n, int channels, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_surface(device, scene_args, scene_args_bytes, false, nullptr, shape_host, uv_host, n, channels, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t slots_b = std::max<size_t>(slots_need(scene_args), 8), shape_b = up8((size_t)n * 4), uv_b = channels ? (size_t)n * 16 : 0;
  Staged s;
  if ((rc = s.alloc(slots_b + shape_b + uv_b + need))) return rc;
  char *slots_d = s.dev, *shape_d = slots_d + slots_b, *uv_d = shape_d + shape_b, *out_d = uv_d + uv_b;
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)n * 4, hipMemcpyHostToDevice));
  if (uv_b) HIP_TRY(hipMemcpy(uv_d, uv_host, uv_b, hipMemcpyHostToDevice));
  if ((rc = enqueue_slots(scene_args, slots_d, nullptr))) return rc;
  if ((rc = enqueue_surface(scene_args, slots_d, (const int *)shape_d, uv_b ? (const double *)uv_d : nullptr, n, channels, out_d, nullptr))) return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernels)
  return PT_OK;
}

extern "C" int pt_rays_shade_lights(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host, const double *point_host,
                                    const double *normal_host, const double *uv_host, const double *dir_host, long long n, const double *ambient,
                                    const double *background, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_lights(device, scene_args, scene_args_bytes, false, nullptr, shape_host, point_host, normal_host, uv_host, dir_host, n, ambient,
                        background, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t slots_b = std::max<size_t>(slots_need(scene_args), 8), shape_b = up8((size_t)n * 4), plane = (size_t)n * 8;
  const size_t total = slots_b + shape_b + 11 * plane + need;
  Staged s;
  if ((rc = s.alloc(total))) return rc;
  char *slots_d = s.dev, *shape_d = slots_d + slots_b, *point_d = shape_d + shape_b, *normal_d = point_d + 3 * plane, *uv_d = normal_d + 3 * plane,
       *dir_d = uv_d + 2 * plane, *out_d = dir_d + 3 * plane;
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(point_d, point_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(normal_d, normal_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(uv_d, uv_host, 2 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dir_d, dir_host, 3 * plane, hipMemcpyHostToDevice));
  if ((rc = enqueue_slots(scene_args, slots_d, nullptr))) return rc;
  if ((rc = enqueue_lights(scene_args, slots_d, (const int *)shape_d, (const double *)point_d, (const double *)normal_d, (const double *)uv_d,
                           (const double *)dir_d, n, ambient, background, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernels)
  return PT_OK;
}
