// ptrace_radiance.hip — libptrace_radiance.so: the C-ABI of include/ptrace_radiance.h, PathTracer.__call__(ray) for ray batches.
//
// What it restates: render.py:99-139, the whole recursion, for rays the CALLER supplies, each with its own generator.  The
// kernel is pt_radiance.h's; the queries are pt_query.h's, the record and the bounce pt_shade.h's, the draws pt_math.h's,
// included here as they are.
//
// Why a fifth translation unit and a fifth shared object: libptrace.so's device code is pinned by build.code_hash (every
// profiles/pmc_*.json names it), and the exported symbols of libptrace_rays.so, libptrace_surface.so and libptrace_scatter.so
// are pinned to the seven, eleven and seven of their interfaces.  So this library stands beside them: the scene arrives as
// the argument block pt_scene_kernel_args (ptrace.h, ABI 1.7) hands out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_radiance.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_radiance.h"
#include "pt_host_common.h"

#define PT_RAD_VERSION ((1 << 16) | 3)
#define PT_RAD_MAX_N 2147483647LL

extern "C" int pt_rays_radiance_version(void) { return PT_RAD_VERSION; }

extern "C" size_t pt_rays_radiance_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_radiance_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static bool shape_ok(long long n, int channels) { return n >= 0 && n <= PT_RAD_MAX_N && channels >= 0 && !(channels & ~PT_RAD_ALL); }

extern "C" size_t pt_rays_radiance_bytes(long long n, int channels) {
  if (!shape_ok(n, channels)) return 0;
  return (size_t)n * 8 * (size_t)(3 + ((channels & PT_RAD_PCG) ? 2 : 0) + ((channels & PT_RAD_COUNT) ? 1 : 0));
}

extern "C" long long pt_rays_radiance_plane_offset(long long n, int channels, int channel, int component) {
  if (!shape_ok(n, channels) || component < 0) return PT_ERR_INVALID;
  if (channel == 0) return component < 3 ? n * 8 * component : PT_ERR_INVALID;
  if (channel == PT_RAD_PCG && (channels & PT_RAD_PCG)) return component < 2 ? n * 8 * (3 + component) : PT_ERR_INVALID;
  if (channel == PT_RAD_COUNT && (channels & PT_RAD_COUNT)) return component < 1 ? n * 8 * (3 + ((channels & PT_RAD_PCG) ? 2 : 0)) : PT_ERR_INVALID;
  return PT_ERR_INVALID;
}

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
static int check_params(long long n, int num_of_rays, int max_depth, int depth0) {
  if (n < 0 || n > PT_RAD_MAX_N) return fail(PT_ERR_INVALID, "ray count %lld outside [0, 2^31 - 1]", n);
  if (num_of_rays < 1) return fail(PT_ERR_INVALID, "num_of_rays must be at least 1, not %d", num_of_rays);
  if (max_depth < 0) return fail(PT_ERR_INVALID, "max_depth must not be negative, not %d", max_depth);
  if (depth0 < 0) return fail(PT_ERR_INVALID, "depth (the entry rays' Ray.depth) must not be negative, not %d", depth0);
  if ((long long)max_depth - depth0 > PT_RAD_MAX_LEVELS)
    return fail(PT_ERR_UNSUPPORTED,
                "max_depth - depth = %lld: a radiance query walks at most %d levels below its entry rays (the fused renderer, pt_render with "
                "PT_RENDERER_PATHTRACER, takes max_depth up to 4096)",
                (long long)max_depth - depth0, PT_RAD_MAX_LEVELS);
  return PT_OK;
}

static int check_args(int device, const void *scene_args, size_t scene_args_bytes, const double *rays, const unsigned long long *pcg_state,
                      const unsigned long long *pcg_inc, long long n, const pt_radiance_params *p, int channels, const void *out,
                      size_t out_bytes, size_t &need) {
  need = 0;
  if (!p) return fail(PT_ERR_INVALID, "null pt_radiance_params");
  if (int rc = check_params(n, p->num_of_rays, p->max_depth, p->depth0)) return rc;
  if (channels < 0 || (channels & ~PT_RAD_ALL))
    return fail(PT_ERR_INVALID, "channel bits %#x: a radiance batch has PT_RAD_PCG | PT_RAD_COUNT", channels);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  need = pt_rays_radiance_bytes(n, channels);
  if (n == 0) return PT_OK;
  if (!rays) return fail(PT_ERR_INVALID, "null ray planes");
  if (!pcg_state || !pcg_inc) return fail(PT_ERR_INVALID, "null generator planes (state, inc)");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "radiance output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

// ---- the launch's shape -------------------------------------------------------------------------------------------------------
// lanes one launch keeps resident: no more than the batch needs, no more than PTRACE_RADIANCE_LANES allows
static int lanes_of(int device, long long n, bool many, unsigned long long &lanes) {
  const void *kernel = many ? (const void *)pt_radiance_kernel<true> : (const void *)pt_radiance_kernel<false>;
  return resident_lanes(device, n, kernel, "PTRACE_RADIANCE_LANES", lanes);
}

static size_t workspace_of(unsigned long long lanes, const pt_radiance_params &p) {
  const long long levels = std::max<long long>((long long)p.max_depth - p.depth0, 1);
  return (size_t)lanes * (size_t)levels * (size_t)(p.num_of_rays > 1 ? PT_RAD_FIELDS_MANY : PT_RAD_FIELDS_ONE) * sizeof(double);
}

extern "C" size_t pt_rays_radiance_workspace_bytes(int device, long long n, int num_of_rays, int max_depth, int depth0) {
  if (check_params(n, num_of_rays, max_depth, depth0)) return 0;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device), 0;
  if (device_ok(device)) return 0;
  if (hipSetDevice(device) != hipSuccess) return fail(PT_ERR_HIP, "hipSetDevice(%d) failed", device), 0;
  unsigned long long lanes;
  if (lanes_of(device, n, num_of_rays > 1, lanes)) return 0;
  pt_radiance_params p = {num_of_rays, max_depth, 0, depth0, {0.0, 0.0, 0.0}};
  return workspace_of(lanes, p);
}

static int enqueue(const void *scene_args, const double *rays_dev, const unsigned long long *state_dev, const unsigned long long *inc_dev,
                   long long n, const pt_radiance_params &p, int channels, unsigned long long lanes, void *ws_dev, void *out_dev,
                   hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  PtRadK K;
  K.N = p.num_of_rays;
  const long long levels = (long long)p.max_depth - p.depth0;
  K.levels = levels < 0 ? -1 : (int)levels;
  K.rr_rel = (int)std::min<long long>(std::max<long long>((long long)p.rr_limit - p.depth0, -1), PT_RAD_MAX_LEVELS + 1);
  K.channels = channels;
  K.bg[0] = p.background[0];
  K.bg[1] = p.background[1];
  K.bg[2] = p.background[2];
  K.invN = 1.0 / p.num_of_rays;
  K.lanes = lanes;
  const dim3 grid((unsigned)(lanes / PT_BLOCK));
  if (p.num_of_rays > 1)
    hipLaunchKernelGGL(pt_radiance_kernel<true>, grid, dim3(PT_BLOCK), 0, st, a, rays_dev, state_dev, inc_dev, n, K, (double *)ws_dev, out_dev);
  else
    hipLaunchKernelGGL(pt_radiance_kernel<false>, grid, dim3(PT_BLOCK), 0, st, a, rays_dev, state_dev, inc_dev, n, K, (double *)ws_dev, out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device form ------------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_radiance_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev,
                                       const double *rays_dev, const unsigned long long *pcg_state_dev,
                                       const unsigned long long *pcg_inc_dev, long long n, const pt_radiance_params *params, int channels,
                                       void *workspace_dev, size_t workspace_bytes, void *out_dev, size_t out_bytes, void *stream) {
  (void)slots_dev;  // (the walk's slots are its own queries': include/ptrace_radiance.h)
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, rays_dev, pcg_state_dev, pcg_inc_dev, n, params, channels, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if (!workspace_dev) return fail(PT_ERR_INVALID, "null workspace (pt_rays_radiance_workspace_bytes says how large)");
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, n, params->num_of_rays > 1, lanes))) return rc;
  const size_t ws_need = workspace_of(lanes, *params);
  if (workspace_bytes < ws_need) return fail(PT_ERR_SIZE, "radiance workspace too small: %zu < %zu bytes", workspace_bytes, ws_need);
  if ((rc = enqueue(scene_args, rays_dev, pcg_state_dev, pcg_inc_dev, n, *params, channels, lanes, workspace_dev, out_dev, (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host form: one device allocation holds the input planes, the workspace and the output -------------------------------------
extern "C" int pt_rays_radiance(int device, const void *scene_args, size_t scene_args_bytes, const double *rays_host,
                                const unsigned long long *pcg_state_host, const unsigned long long *pcg_inc_host, long long n,
                                const pt_radiance_params *params, int channels, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, rays_host, pcg_state_host, pcg_inc_host, n, params, channels, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, n, params->num_of_rays > 1, lanes))) return rc;
  const size_t plane = (size_t)n * 8, ws_b = workspace_of(lanes, *params);
  const size_t total = 10 * plane + ws_b + need;
  Staged s;
  if ((rc = s.alloc(total))) return rc;
  char *rays_d = s.dev, *state_d = rays_d + 8 * plane, *inc_d = state_d + plane, *ws_d = inc_d + plane, *out_d = ws_d + ws_b;
  HIP_TRY(hipMemcpy(rays_d, rays_host, 8 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(state_d, pcg_state_host, plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(inc_d, pcg_inc_host, plane, hipMemcpyHostToDevice));
  if ((rc = enqueue(scene_args, (const double *)rays_d, (const unsigned long long *)state_d, (const unsigned long long *)inc_d, n, *params,
                    channels, lanes, ws_d, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}
