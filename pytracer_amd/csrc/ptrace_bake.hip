// ptrace_bake.hip — libptrace_bake.so: the C-ABI of include/ptrace_bake.h, surface points from (shape, u, v) and light maps over
// a shape's (u, v) grid.
//
// What it restates: the inverse of the shapes' (u, v) maps (shapes.py:36-42, 183-185) with Transformation.__mul__
// (transformations.py:58-96); per texel and sample PCG(init_state, init_seq + t K + k) (pcg.py:25-41), the jitter of
// imagetracer.py:48-58, DiffuseBRDF.scatter_ray (materials.py:132-152) and PathTracer.__call__ (render.py:99-139), then the mean in
// k order.  The kernels are pt_bake.h's; the queries are pt_query.h's, the record and the bounce pt_shade.h's, the draws
// pt_math.h's, included here as they are.
//
// Why a seventh translation unit and a seventh shared object: libptrace.so's device code is pinned by build.code_hash (every
// profiles/pmc_*.json names it), and the exported symbols of the five add-ons before this one are pinned to their interfaces'.
// So this library stands beside them: the scene arrives as the argument block pt_scene_kernel_args (ptrace.h, ABI 1.7) hands
// out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_bake.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_bake.h"
#include "pt_host_common.h"

#define PT_BAKE_VERSION ((1 << 16) | 5)
#define PT_BAKE_MAX_N 2147483647LL

extern "C" int pt_rays_bake_version(void) { return PT_BAKE_VERSION; }

extern "C" size_t pt_rays_bake_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_bake_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static bool shape_ok(long long n, int channels) { return n >= 0 && n <= PT_BAKE_MAX_N && channels >= 0 && !(channels & ~PT_BAKE_ALL); }

extern "C" size_t pt_rays_points_bytes(long long n) { return shape_ok(n, 0) ? (size_t)n * 48 : 0; }

extern "C" size_t pt_rays_bake_bytes(long long texels, int channels) {
  if (!shape_ok(texels, channels)) return 0;
  return (size_t)texels * 8 * (size_t)(3 + ((channels & PT_BAKE_COUNT) ? 1 : 0));
}

extern "C" long long pt_rays_bake_plane_offset(long long texels, int channels, int channel, int component) {
  if (!shape_ok(texels, channels) || component < 0) return PT_ERR_INVALID;
  if (channel == 0) return component < 3 ? texels * 8 * component : PT_ERR_INVALID;
  if (channel == PT_BAKE_COUNT && (channels & PT_BAKE_COUNT)) return component < 1 ? texels * 8 * 3 : PT_ERR_INVALID;
  return PT_ERR_INVALID;
}

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
static int check_params(const pt_bake_params *p) {
  if (!p) return fail(PT_ERR_INVALID, "null pt_bake_params");
  if (p->side != 1 && p->side != -1) return fail(PT_ERR_INVALID, "side must be +1 or -1, not %d", p->side);
  if (p->W < 1 || p->H < 1) return fail(PT_ERR_INVALID, "a map of %d x %d texels: W and H must be at least 1", p->W, p->H);
  if (p->w < 1 || p->h < 1 || p->col0 < 0 || p->row0 < 0 || (long long)p->col0 + p->w > p->W || (long long)p->row0 + p->h > p->H)
    return fail(PT_ERR_INVALID, "rectangle [%d, %d + %d) x [%d, %d + %d) is not a non-empty part of the %d x %d map", p->col0, p->col0, p->w,
                p->row0, p->row0, p->h, p->W, p->H);
  if (p->samples < 1) return fail(PT_ERR_INVALID, "samples must be at least 1, not %d", p->samples);
  const long long texels = (long long)p->w * p->h;
  if (texels > PT_BAKE_MAX_N / p->samples)
    return fail(PT_ERR_INVALID, "%lld texels x %d samples: a bake takes at most 2^31 - 1 hemisphere rays (bake the map in windows)", texels,
                p->samples);
  if (p->num_of_rays < 1) return fail(PT_ERR_INVALID, "num_of_rays must be at least 1, not %d", p->num_of_rays);
  if (p->max_depth < 0) return fail(PT_ERR_INVALID, "max_depth must not be negative, not %d", p->max_depth);
  if (p->depth0 < 0) return fail(PT_ERR_INVALID, "depth (the hemisphere rays' Ray.depth) must not be negative, not %d", p->depth0);
  if ((long long)p->max_depth - p->depth0 > PT_BAKE_MAX_LEVELS)
    return fail(PT_ERR_UNSUPPORTED, "max_depth - depth = %lld: a bake walks at most %d levels below its hemisphere rays",
                (long long)p->max_depth - p->depth0, PT_BAKE_MAX_LEVELS);
  return PT_OK;
}

static int check_bake(int device, const void *scene_args, size_t scene_args_bytes, const pt_bake_params *p, int channels, const void *out,
                      size_t out_bytes, size_t &need) {
  need = 0;
  if (int rc = check_params(p)) return rc;
  if (channels < 0 || (channels & ~PT_BAKE_ALL)) return fail(PT_ERR_INVALID, "channel bits %#x: a bake has PT_BAKE_COUNT", channels);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  const int n_shapes = ((const PtKArgs *)scene_args)->n_shapes;
  if (p->shape < 0 || p->shape >= n_shapes) return fail(PT_ERR_INVALID, "shape %d: the scene has %d shapes", p->shape, n_shapes);
  need = pt_rays_bake_bytes((long long)p->w * p->h, channels);
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "bake output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

static int check_points(int device, const void *scene_args, size_t scene_args_bytes, const int *shape, const double *uv, long long n,
                        const void *out, size_t out_bytes, size_t &need) {
  need = 0;
  if (n < 0 || n > PT_BAKE_MAX_N) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", n);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  need = pt_rays_points_bytes(n);
  if (n == 0) return PT_OK;
  if (!shape || !uv) return fail(PT_ERR_INVALID, "null record planes (shape, uv)");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "surface-point output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

// ---- the launch's shape -------------------------------------------------------------------------------------------------------
static long long total_of(const pt_bake_params &p) { return (long long)p.w * p.h * p.samples; }

// lanes the walk's launch keeps resident: no more than the w h K samples need, no more than PTRACE_BAKE_LANES allows
static int lanes_of(int device, long long total, bool many, unsigned long long &lanes) {
  const void *kernel = many ? (const void *)pt_bake_kernel<true> : (const void *)pt_bake_kernel<false>;
  return resident_lanes(device, total, kernel, "PTRACE_BAKE_LANES", lanes);
}

static size_t stacks_of(unsigned long long lanes, const pt_bake_params &p) {
  const long long levels = std::max<long long>((long long)p.max_depth - p.depth0, 1);
  return (size_t)lanes * (size_t)levels * (size_t)(p.num_of_rays > 1 ? PT_BAKE_FIELDS_MANY : PT_BAKE_FIELDS_ONE) * sizeof(double);
}

static size_t planes_of(const pt_bake_params &p) { return (size_t)total_of(p) * PT_BAKE_SAMPLE_PLANES * sizeof(double); }

static size_t workspace_of(unsigned long long lanes, const pt_bake_params &p) { return stacks_of(lanes, p) + planes_of(p); }

extern "C" size_t pt_rays_bake_workspace_bytes(int device, const pt_bake_params *params) {
  if (check_params(params)) return 0;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device), 0;
  if (device_ok(device)) return 0;
  if (hipSetDevice(device) != hipSuccess) return fail(PT_ERR_HIP, "hipSetDevice(%d) failed", device), 0;
  unsigned long long lanes;
  if (lanes_of(device, total_of(*params), params->num_of_rays > 1, lanes)) return 0;
  return workspace_of(lanes, *params);
}

static int enqueue_bake(const void *scene_args, const pt_bake_params &p, int channels, unsigned long long lanes, void *ws_dev, void *out_dev,
                        hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  PtBakeK K;
  K.samples = p.samples;
  K.N = p.num_of_rays;
  const long long levels = (long long)p.max_depth - p.depth0;
  K.levels = levels < 0 ? -1 : (int)levels;
  K.rr_rel = (int)std::min<long long>(std::max<long long>((long long)p.rr_limit - p.depth0, -1), PT_BAKE_MAX_LEVELS + 1);
  K.channels = channels;
  K.shape = p.shape;
  K.side = p.side;
  K.jitter = p.jitter != 0;
  K.W = p.W;
  K.col0 = p.col0;
  K.row0 = p.row0;
  K.w = p.w;
  K.invW = 1.0 / p.W;
  K.invH = 1.0 / p.H;
  K.bg[0] = p.background[0];
  K.bg[1] = p.background[1];
  K.bg[2] = p.background[2];
  K.invN = 1.0 / p.num_of_rays;
  K.invK = 1.0 / p.samples;
  K.init_state = p.init_state;
  K.init_seq = p.init_seq;
  K.lanes = lanes;
  const long long texels = (long long)p.w * p.h, total = total_of(p);
  double *stacks = (double *)ws_dev;
  double *samples = (double *)((char *)ws_dev + stacks_of(lanes, p));
  const dim3 grid((unsigned)(lanes / PT_BLOCK));
  if (p.num_of_rays > 1)
    hipLaunchKernelGGL(pt_bake_kernel<true>, grid, dim3(PT_BLOCK), 0, st, a, total, K, stacks, samples);
  else
    hipLaunchKernelGGL(pt_bake_kernel<false>, grid, dim3(PT_BLOCK), 0, st, a, total, K, stacks, samples);
  HIP_TRY(hipGetLastError());
  // the mean: behind the walk on the same stream, one lane per texel
  hipLaunchKernelGGL(pt_bake_mean_kernel, grid_of(texels), dim3(PT_BLOCK), 0, st, (const double *)samples, texels, total, K, out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_points(const void *scene_args, const int *shape_dev, const double *uv_dev, const int *side_dev, long long n, void *out_dev,
                          hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  hipLaunchKernelGGL(pt_surface_points_kernel, grid_of(n), dim3(PT_BLOCK), 0, st, a, shape_dev, uv_dev, side_dev, n, (double *)out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device forms -----------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_surface_points_device(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_dev,
                                             const double *uv_dev, const int *side_dev, long long n, void *out_dev, size_t out_bytes,
                                             void *stream) {
  size_t need;
  int rc = check_points(device, scene_args, scene_args_bytes, shape_dev, uv_dev, n, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_points(scene_args, shape_dev, uv_dev, side_dev, n, out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_bake_device(int device, const void *scene_args, size_t scene_args_bytes, const pt_bake_params *params, int channels,
                                   void *workspace_dev, size_t workspace_bytes, void *out_dev, size_t out_bytes, void *stream) {
  size_t need;
  int rc = check_bake(device, scene_args, scene_args_bytes, params, channels, out_dev, out_bytes, need);
  if (rc) return rc;
  if (!workspace_dev) return fail(PT_ERR_INVALID, "null workspace (pt_rays_bake_workspace_bytes says how large)");
  // (whatever the resident lanes turn out to be, the sample planes alone need this much: refused before any HIP call)
  if (workspace_bytes < planes_of(*params))
    return fail(PT_ERR_SIZE, "bake workspace too small: %zu bytes do not hold the sample planes (%zu)", workspace_bytes, planes_of(*params));
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, total_of(*params), params->num_of_rays > 1, lanes))) return rc;
  const size_t ws_need = workspace_of(lanes, *params);
  if (workspace_bytes < ws_need) return fail(PT_ERR_SIZE, "bake workspace too small: %zu < %zu bytes", workspace_bytes, ws_need);
  if ((rc = enqueue_bake(scene_args, *params, channels, lanes, workspace_dev, out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host forms: one device allocation holds the inputs, the workspace and the output -------------------------------------------
extern "C" int pt_rays_surface_points(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host, const double *uv_host,
                                      const int *side_host, long long n, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_points(device, scene_args, scene_args_bytes, shape_host, uv_host, n, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t int_b = up8((size_t)n * 4), uv_b = (size_t)n * 16;
  Staged s;
  if ((rc = s.alloc(2 * int_b + uv_b + need))) return rc;
  char *shape_d = s.dev, *side_d = shape_d + int_b, *uv_d = side_d + int_b, *out_d = uv_d + uv_b;
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)n * 4, hipMemcpyHostToDevice));
  if (side_host) HIP_TRY(hipMemcpy(side_d, side_host, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(uv_d, uv_host, uv_b, hipMemcpyHostToDevice));
  if ((rc = enqueue_points(scene_args, (const int *)shape_d, (const double *)uv_d, side_host ? (const int *)side_d : nullptr, n, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}

extern "C" int pt_rays_bake(int device, const void *scene_args, size_t scene_args_bytes, const pt_bake_params *params, int channels,
                            void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_bake(device, scene_args, scene_args_bytes, params, channels, out_host, out_bytes, need);
  if (rc) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, total_of(*params), params->num_of_rays > 1, lanes))) return rc;
  const size_t ws_b = workspace_of(lanes, *params);
  Staged s;
  if ((rc = s.alloc(ws_b + need))) return rc;
  char *ws_d = s.dev, *out_d = ws_d + ws_b;
  if ((rc = enqueue_bake(scene_args, *params, channels, lanes, ws_d, out_d, nullptr))) return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind both kernels)
  return PT_OK;
}
