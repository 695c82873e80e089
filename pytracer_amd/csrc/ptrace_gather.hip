// ptrace_gather.hip — libptrace_gather.so: the C-ABI of include/ptrace_gather.h, hemisphere radiance for batches of surface points.
//
// What it restates: per record and sample PCG(init_state, seq + k) (pcg.py:25-41), DiffuseBRDF.scatter_ray (materials.py:132-152)
// and PathTracer.__call__ (render.py:99-139), then the mean in k order.  The kernels are pt_gather.h's; the queries are
// pt_query.h's, the record and the bounce pt_shade.h's, the draws pt_math.h's, included here as they are.
//
// Why a sixth translation unit and a sixth shared object: libptrace.so's device code is pinned by build.code_hash (every
// profiles/pmc_*.json names it), and the exported symbols of the four add-ons before this one are pinned to their interfaces'.
// So this library stands beside them: the scene arrives as the argument block pt_scene_kernel_args (ptrace.h, ABI 1.7) hands
// out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_gather.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_gather.h"
#include "pt_host_common.h"

#define PT_GAT_VERSION ((1 << 16) | 4)
#define PT_GAT_MAX_N 2147483647LL

extern "C" int pt_rays_gather_version(void) { return PT_GAT_VERSION; }

extern "C" size_t pt_rays_gather_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_gather_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static bool shape_ok(long long n, int channels) { return n >= 0 && n <= PT_GAT_MAX_N && channels >= 0 && !(channels & ~PT_GATHER_ALL); }

extern "C" size_t pt_rays_gather_bytes(long long n, int channels) {
  if (!shape_ok(n, channels)) return 0;
  return (size_t)n * 8 * (size_t)(3 + ((channels & PT_GATHER_COUNT) ? 1 : 0));
}

extern "C" long long pt_rays_gather_plane_offset(long long n, int channels, int channel, int component) {
  if (!shape_ok(n, channels) || component < 0) return PT_ERR_INVALID;
  if (channel == 0) return component < 3 ? n * 8 * component : PT_ERR_INVALID;
  if (channel == PT_GATHER_COUNT && (channels & PT_GATHER_COUNT)) return component < 1 ? n * 8 * 3 : PT_ERR_INVALID;
  return PT_ERR_INVALID;
}

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
static int check_params(long long n, int samples, int num_of_rays, int max_depth, int depth0) {
  if (n < 0 || n > PT_GAT_MAX_N) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", n);
  if (samples < 1) return fail(PT_ERR_INVALID, "samples must be at least 1, not %d", samples);
  if (n * (long long)samples > PT_GAT_MAX_N)
    return fail(PT_ERR_INVALID, "%lld records x %d samples = %lld hemisphere rays: a gather takes at most 2^31 - 1 (split the batch)", n, samples,
                n * (long long)samples);
  if (num_of_rays < 1) return fail(PT_ERR_INVALID, "num_of_rays must be at least 1, not %d", num_of_rays);
  if (max_depth < 0) return fail(PT_ERR_INVALID, "max_depth must not be negative, not %d", max_depth);
  if (depth0 < 0) return fail(PT_ERR_INVALID, "depth (the hemisphere rays' Ray.depth) must not be negative, not %d", depth0);
  if ((long long)max_depth - depth0 > PT_GATHER_MAX_LEVELS)
    return fail(PT_ERR_UNSUPPORTED, "max_depth - depth = %lld: a gather query walks at most %d levels below its hemisphere rays",
                (long long)max_depth - depth0, PT_GATHER_MAX_LEVELS);
  return PT_OK;
}

static int check_args(int device, const void *scene_args, size_t scene_args_bytes, const double *points, const double *normals, long long n,
                      const pt_gather_params *p, int channels, const void *out, size_t out_bytes, size_t &need) {
  need = 0;
  if (!p) return fail(PT_ERR_INVALID, "null pt_gather_params");
  if (int rc = check_params(n, p->samples, p->num_of_rays, p->max_depth, p->depth0)) return rc;
  if (channels < 0 || (channels & ~PT_GATHER_ALL)) return fail(PT_ERR_INVALID, "channel bits %#x: a gather batch has PT_GATHER_COUNT", channels);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  need = pt_rays_gather_bytes(n, channels);
  if (n == 0) return PT_OK;
  if (!points || !normals) return fail(PT_ERR_INVALID, "null record planes (points, normals)");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "gather output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

// ---- the launch's shape -------------------------------------------------------------------------------------------------------
// lanes the walk's launch keeps resident: no more than the n * K samples need, no more than PTRACE_GATHER_LANES allows
static int lanes_of(int device, long long total, bool many, unsigned long long &lanes) {
  const void *kernel = many ? (const void *)pt_gather_kernel<true> : (const void *)pt_gather_kernel<false>;
  return resident_lanes(device, total, kernel, "PTRACE_GATHER_LANES", lanes);
}

static size_t stacks_of(unsigned long long lanes, const pt_gather_params &p) {
  const long long levels = std::max<long long>((long long)p.max_depth - p.depth0, 1);
  return (size_t)lanes * (size_t)levels * (size_t)(p.num_of_rays > 1 ? PT_GAT_FIELDS_MANY : PT_GAT_FIELDS_ONE) * sizeof(double);
}

static size_t workspace_of(unsigned long long lanes, long long n, const pt_gather_params &p) {
  return stacks_of(lanes, p) + (size_t)n * (size_t)p.samples * PT_GAT_SAMPLE_PLANES * sizeof(double);
}

extern "C" size_t pt_rays_gather_workspace_bytes(int device, long long n, int samples, int num_of_rays, int max_depth, int depth0) {
  if (check_params(n, samples, num_of_rays, max_depth, depth0)) return 0;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device), 0;
  if (device_ok(device)) return 0;
  if (hipSetDevice(device) != hipSuccess) return fail(PT_ERR_HIP, "hipSetDevice(%d) failed", device), 0;
  unsigned long long lanes;
  if (lanes_of(device, n * (long long)samples, num_of_rays > 1, lanes)) return 0;
  pt_gather_params p = {samples, num_of_rays, max_depth, 0, depth0, 0ULL, 0ULL, {0.0, 0.0, 0.0}};
  return workspace_of(lanes, n, p);
}

static int enqueue(const void *scene_args, const double *points_dev, const double *normals_dev, const int *active_dev,
                   const unsigned long long *seq_dev, long long n, const pt_gather_params &p, int channels, unsigned long long lanes,
                   void *ws_dev, void *out_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  PtGatK K;
  K.samples = p.samples;
  K.N = p.num_of_rays;
  const long long levels = (long long)p.max_depth - p.depth0;
  K.levels = levels < 0 ? -1 : (int)levels;
  K.rr_rel = (int)std::min<long long>(std::max<long long>((long long)p.rr_limit - p.depth0, -1), PT_GATHER_MAX_LEVELS + 1);
  K.channels = channels;
  K.bg[0] = p.background[0];
  K.bg[1] = p.background[1];
  K.bg[2] = p.background[2];
  K.invN = 1.0 / p.num_of_rays;
  K.invK = 1.0 / p.samples;
  K.init_state = p.init_state;
  K.init_seq = p.init_seq;
  K.lanes = lanes;
  const long long total = n * (long long)p.samples;
  double *stacks = (double *)ws_dev;
  double *samples = (double *)((char *)ws_dev + stacks_of(lanes, p));
  const dim3 grid((unsigned)(lanes / PT_BLOCK));
  if (p.num_of_rays > 1)
    hipLaunchKernelGGL(pt_gather_kernel<true>, grid, dim3(PT_BLOCK), 0, st, a, points_dev, normals_dev, active_dev, seq_dev, n, total, K, stacks,
                       samples);
  else
    hipLaunchKernelGGL(pt_gather_kernel<false>, grid, dim3(PT_BLOCK), 0, st, a, points_dev, normals_dev, active_dev, seq_dev, n, total, K, stacks,
                       samples);
  HIP_TRY(hipGetLastError());
  // the mean: behind the walk on the same stream, one lane per record
  hipLaunchKernelGGL(pt_gather_mean_kernel, grid_of(n), dim3(PT_BLOCK), 0, st, (const double *)samples, active_dev, n, total, K, out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device form ------------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_gather_device(int device, const void *scene_args, size_t scene_args_bytes, const double *points_dev,
                                     const double *normals_dev, const int *active_dev, const unsigned long long *seq_dev, long long n,
                                     const pt_gather_params *params, int channels, void *workspace_dev, size_t workspace_bytes, void *out_dev,
                                     size_t out_bytes, void *stream) {
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, points_dev, normals_dev, n, params, channels, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if (!workspace_dev) return fail(PT_ERR_INVALID, "null workspace (pt_rays_gather_workspace_bytes says how large)");
  // (whatever the resident lanes turn out to be, the sample planes alone need this much: refused before any HIP call)
  const size_t planes = (size_t)n * (size_t)params->samples * PT_GAT_SAMPLE_PLANES * sizeof(double);
  if (workspace_bytes < planes) return fail(PT_ERR_SIZE, "gather workspace too small: %zu bytes do not hold the sample planes (%zu)", workspace_bytes, planes);
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, n * (long long)params->samples, params->num_of_rays > 1, lanes))) return rc;
  const size_t ws_need = workspace_of(lanes, n, *params);
  if (workspace_bytes < ws_need) return fail(PT_ERR_SIZE, "gather workspace too small: %zu < %zu bytes", workspace_bytes, ws_need);
  if ((rc = enqueue(scene_args, points_dev, normals_dev, active_dev, seq_dev, n, *params, channels, lanes, workspace_dev, out_dev,
                    (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host form: one device allocation holds the input planes, the workspace and the output -------------------------------------
extern "C" int pt_rays_gather(int device, const void *scene_args, size_t scene_args_bytes, const double *points_host, const double *normals_host,
                              const int *active_host, const unsigned long long *seq_host, long long n, const pt_gather_params *params,
                              int channels, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, points_host, normals_host, n, params, channels, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, n * (long long)params->samples, params->num_of_rays > 1, lanes))) return rc;
  const size_t plane = (size_t)n * 8, ws_b = workspace_of(lanes, n, *params);
  const size_t total = 8 * plane + ws_b + need;  // points 3, normals 3, seq 1, active 1 (int32, padded)
  Staged s;
  if ((rc = s.alloc(total))) return rc;
  char *points_d = s.dev, *normals_d = points_d + 3 * plane, *seq_d = normals_d + 3 * plane, *act_d = seq_d + plane, *ws_d = act_d + plane,
       *out_d = ws_d + ws_b;
  HIP_TRY(hipMemcpy(points_d, points_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(normals_d, normals_host, 3 * plane, hipMemcpyHostToDevice));
  if (seq_host) HIP_TRY(hipMemcpy(seq_d, seq_host, plane, hipMemcpyHostToDevice));
  if (active_host) HIP_TRY(hipMemcpy(act_d, active_host, (size_t)n * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue(scene_args, (const double *)points_d, (const double *)normals_d, active_host ? (const int *)act_d : nullptr,
                    seq_host ? (const unsigned long long *)seq_d : nullptr, n, *params, channels, lanes, ws_d, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind both kernels)
  return PT_OK;
}
