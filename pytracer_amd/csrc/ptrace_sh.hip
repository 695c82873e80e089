// ptrace_sh.hip — libptrace_sh.so: the C-ABI of include/ptrace_sh.h, order-2 spherical-harmonic radiance probes at free points.
//
// What it restates: per probe and sample PCG(init_state, seq_i + k) (pcg.py:25-41), a uniform direction on the sphere from two
// draws, Ray's defaults (ray.py) and PathTracer.__call__ (render.py:99-139), then the projection onto the nine real SH functions of
// bands 0 - 2 in k order, and their evaluation.  The kernels are pt_sh.h's; the queries are pt_query.h's, the record and the bounce
// pt_shade.h's, the draws pt_math.h's, included here as they are.
//
// Why an eighth translation unit and an eighth shared object: libptrace.so's device code is pinned by build.code_hash (every
// profiles/pmc_*.json names it), and the exported symbols of the six add-ons before this one are pinned to their interfaces'.
// So this library stands beside them: the scene arrives as the argument block pt_scene_kernel_args (ptrace.h, ABI 1.7) hands
// out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_sh.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_sh.h"
#include "pt_host_common.h"

#define PT_SHP_VERSION ((1 << 16) | 6)
#define PT_SHP_MAX_N 2147483647LL

extern "C" int pt_rays_sh_version(void) { return PT_SHP_VERSION; }

extern "C" size_t pt_rays_sh_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_sh_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static bool count_ok(long long n) { return n >= 0 && n <= PT_SHP_MAX_N; }

static bool shape_ok(long long n, int channels) { return count_ok(n) && channels >= 0 && !(channels & ~PT_SH_ALL); }

extern "C" size_t pt_rays_sh_dirs_bytes(long long n, int samples) {
  if (!count_ok(n) || samples < 1 || n > PT_SHP_MAX_N / samples) return 0;
  return (size_t)n * (size_t)samples * 24;
}

extern "C" size_t pt_rays_sh_bytes(long long n, int channels) {
  if (!shape_ok(n, channels)) return 0;
  return (size_t)n * 8 * (size_t)(PT_SH_COEFFS + ((channels & PT_SH_COUNT) ? 1 : 0));
}

extern "C" long long pt_rays_sh_plane_offset(long long n, int channels, int channel, int component) {
  if (!shape_ok(n, channels) || component < 0) return PT_ERR_INVALID;
  if (channel == 0) return component < PT_SH_COEFFS ? n * 8 * component : PT_ERR_INVALID;
  if (channel == PT_SH_COUNT && (channels & PT_SH_COUNT)) return component < 1 ? n * 8 * PT_SH_COEFFS : PT_ERR_INVALID;
  return PT_ERR_INVALID;
}

extern "C" size_t pt_rays_sh_eval_bytes(long long m) { return count_ok(m) ? (size_t)m * 24 : 0; }

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
static int check_params(long long n, const pt_sh_params *p) {
  if (!p) return fail(PT_ERR_INVALID, "null pt_sh_params");
  if (!count_ok(n)) return fail(PT_ERR_INVALID, "probe count %lld outside [0, 2^31 - 1]", n);
  if (p->samples < 1) return fail(PT_ERR_INVALID, "samples must be at least 1, not %d", p->samples);
  if (n > PT_SHP_MAX_N / p->samples)
    return fail(PT_ERR_INVALID, "%lld probes x %d samples: a call takes at most 2^31 - 1 rays (split the probes into batches)", n, p->samples);
  if (p->num_of_rays < 1) return fail(PT_ERR_INVALID, "num_of_rays must be at least 1, not %d", p->num_of_rays);
  if (p->max_depth < 0) return fail(PT_ERR_INVALID, "max_depth must not be negative, not %d", p->max_depth);
  if (p->depth0 < 0) return fail(PT_ERR_INVALID, "depth (the probe rays' Ray.depth) must not be negative, not %d", p->depth0);
  if ((long long)p->max_depth - p->depth0 > PT_SH_MAX_LEVELS)
    return fail(PT_ERR_UNSUPPORTED, "max_depth - depth = %lld: a probe walks at most %d levels below its rays",
                (long long)p->max_depth - p->depth0, PT_SH_MAX_LEVELS);
  return PT_OK;
}

static int check_project(int device, const void *scene_args, size_t scene_args_bytes, const double *points, long long n, const pt_sh_params *p,
                         int channels, const void *out, size_t out_bytes, size_t &need) {
  need = 0;
  if (int rc = check_params(n, p)) return rc;
  if (channels < 0 || (channels & ~PT_SH_ALL)) return fail(PT_ERR_INVALID, "channel bits %#x: a probe batch has PT_SH_COUNT", channels);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  need = pt_rays_sh_bytes(n, channels);
  if (n == 0) return PT_OK;
  if (!points) return fail(PT_ERR_INVALID, "null points plane");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "probe output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

static int check_directions(int device, long long n, const pt_sh_params *p, const void *out, size_t out_bytes, size_t &need) {
  need = 0;
  if (int rc = check_params(n, p)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  need = pt_rays_sh_dirs_bytes(n, p->samples);
  if (n == 0) return PT_OK;
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "directions output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

static int check_eval(int device, const double *coeffs, long long n, const int *index, const double *dirs, long long m, int kind, const void *out,
                      size_t out_bytes, size_t &need) {
  need = 0;
  if (!count_ok(n)) return fail(PT_ERR_INVALID, "probe count %lld outside [0, 2^31 - 1]", n);
  if (!count_ok(m)) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", m);
  if (kind != PT_SH_RADIANCE && kind != PT_SH_HEMISPHERE)
    return fail(PT_ERR_INVALID, "kind %d: an evaluation is PT_SH_RADIANCE or PT_SH_HEMISPHERE", kind);
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (!index && m > n) return fail(PT_ERR_INVALID, "%lld records without an index plane, but %lld probes: record r reads probe r", m, n);
  need = pt_rays_sh_eval_bytes(m);
  if (m == 0) return PT_OK;
  if (!dirs) return fail(PT_ERR_INVALID, "null directions plane");
  if (n > 0 && !coeffs) return fail(PT_ERR_INVALID, "null coefficient block");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "evaluation output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

// ---- the launch's shape -------------------------------------------------------------------------------------------------------
static long long total_of(long long n, const pt_sh_params &p) { return n * p.samples; }

// lanes the walk's launch keeps resident: no more than the n K samples need, no more than PTRACE_SH_LANES allows
static int lanes_of(int device, long long total, bool many, unsigned long long &lanes) {
  const void *kernel = many ? (const void *)pt_sh_kernel<true> : (const void *)pt_sh_kernel<false>;
  return resident_lanes(device, total, kernel, "PTRACE_SH_LANES", lanes);
}

static size_t stacks_of(unsigned long long lanes, const pt_sh_params &p) {
  const long long levels = std::max<long long>((long long)p.max_depth - p.depth0, 1);
  return (size_t)lanes * (size_t)levels * (size_t)(p.num_of_rays > 1 ? PT_SHP_FIELDS_MANY : PT_SHP_FIELDS_ONE) * sizeof(double);
}

static size_t planes_of(long long n, const pt_sh_params &p) { return (size_t)total_of(n, p) * PT_SHP_SAMPLE_PLANES * sizeof(double); }

static size_t workspace_of(unsigned long long lanes, long long n, const pt_sh_params &p) { return stacks_of(lanes, p) + planes_of(n, p); }

extern "C" size_t pt_rays_sh_workspace_bytes(int device, long long n, const pt_sh_params *params) {
  if (check_params(n, params)) return 0;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device), 0;
  if (device_ok(device)) return 0;
  if (hipSetDevice(device) != hipSuccess) return fail(PT_ERR_HIP, "hipSetDevice(%d) failed", device), 0;
  unsigned long long lanes;
  if (lanes_of(device, total_of(n, *params), params->num_of_rays > 1, lanes)) return 0;
  return workspace_of(lanes, n, *params);
}

static PtShK kernel_params(const pt_sh_params &p, int channels, unsigned long long lanes) {
  PtShK K;
  K.samples = p.samples;
  K.N = p.num_of_rays;
  const long long levels = (long long)p.max_depth - p.depth0;
  K.levels = levels < 0 ? -1 : (int)levels;
  K.rr_rel = (int)std::min<long long>(std::max<long long>((long long)p.rr_limit - p.depth0, -1), PT_SH_MAX_LEVELS + 1);
  K.channels = channels;
  K.bg[0] = p.background[0];
  K.bg[1] = p.background[1];
  K.bg[2] = p.background[2];
  K.invN = 1.0 / p.num_of_rays;
  K.scale = (4.0 * PT_PI) * (1.0 / p.samples);
  K.init_state = p.init_state;
  K.init_seq = p.init_seq;
  K.lanes = lanes;
  return K;
}

static int enqueue_project(const void *scene_args, const double *points_dev, const int *active_dev, const unsigned long long *seqs_dev, long long n,
                           const pt_sh_params &p, int channels, unsigned long long lanes, void *ws_dev, void *out_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  const PtShK K = kernel_params(p, channels, lanes);
  const long long total = total_of(n, p);
  double *stacks = (double *)ws_dev;
  double *samples = (double *)((char *)ws_dev + stacks_of(lanes, p));
  const dim3 grid((unsigned)(lanes / PT_BLOCK));
  if (p.num_of_rays > 1)
    hipLaunchKernelGGL(pt_sh_kernel<true>, grid, dim3(PT_BLOCK), 0, st, a, points_dev, active_dev, seqs_dev, n, total, K, stacks, samples);
  else
    hipLaunchKernelGGL(pt_sh_kernel<false>, grid, dim3(PT_BLOCK), 0, st, a, points_dev, active_dev, seqs_dev, n, total, K, stacks, samples);
  HIP_TRY(hipGetLastError());
  // the projection: behind the walk on the same stream, one lane per probe
  hipLaunchKernelGGL(pt_sh_project_kernel, dim3((unsigned)((n + PT_SHP_BLOCK - 1) / PT_SHP_BLOCK)), dim3(PT_SHP_BLOCK), 0, st, (const double *)samples, active_dev, seqs_dev, n, total, K, out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_directions(const unsigned long long *seqs_dev, long long n, const pt_sh_params &p, void *out_dev, hipStream_t st) {
  const PtShK K = kernel_params(p, 0, 0ULL);
  const long long total = total_of(n, p);
  hipLaunchKernelGGL(pt_sh_directions_kernel, grid_of(total), dim3(PT_BLOCK), 0, st, seqs_dev, total, K, (double *)out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_eval(const double *coeffs_dev, long long n, const int *index_dev, const double *dirs_dev, long long m, int kind, void *out_dev,
                        hipStream_t st) {
  hipLaunchKernelGGL(pt_sh_eval_kernel, grid_of(m), dim3(PT_BLOCK), 0, st, coeffs_dev, n, index_dev, dirs_dev, m, kind, (double *)out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device forms -----------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_sh_directions_device(int device, const unsigned long long *seqs_dev, long long n, const pt_sh_params *params,
                                            void *out_dev, size_t out_bytes, void *stream) {
  size_t need;
  int rc = check_directions(device, n, params, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_directions(seqs_dev, n, *params, out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_sh_project_device(int device, const void *scene_args, size_t scene_args_bytes, const double *points_dev,
                                         const int *active_dev, const unsigned long long *seqs_dev, long long n, const pt_sh_params *params,
                                         int channels, void *workspace_dev, size_t workspace_bytes, void *out_dev, size_t out_bytes,
                                         void *stream) {
  size_t need;
  int rc = check_project(device, scene_args, scene_args_bytes, points_dev, n, params, channels, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if (!workspace_dev) return fail(PT_ERR_INVALID, "null workspace (pt_rays_sh_workspace_bytes says how large)");
  // (whatever the resident lanes turn out to be, the sample planes alone need this much: refused before any HIP call)
  if (workspace_bytes < planes_of(n, *params))
    return fail(PT_ERR_SIZE, "probe workspace too small: %zu bytes do not hold the sample planes (%zu)", workspace_bytes, planes_of(n, *params));
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, total_of(n, *params), params->num_of_rays > 1, lanes))) return rc;
  const size_t ws_need = workspace_of(lanes, n, *params);
  if (workspace_bytes < ws_need) return fail(PT_ERR_SIZE, "probe workspace too small: %zu < %zu bytes", workspace_bytes, ws_need);
  if ((rc = enqueue_project(scene_args, points_dev, active_dev, seqs_dev, n, *params, channels, lanes, workspace_dev, out_dev, (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_sh_eval_device(int device, const double *coeffs_dev, long long n, const int *index_dev, const double *dirs_dev, long long m,
                                      int kind, void *out_dev, size_t out_bytes, void *stream) {
  size_t need;
  int rc = check_eval(device, coeffs_dev, n, index_dev, dirs_dev, m, kind, out_dev, out_bytes, need);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_eval(coeffs_dev, n, index_dev, dirs_dev, m, kind, out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host forms: one device allocation holds the inputs, the workspace and the output -------------------------------------------
extern "C" int pt_rays_sh_directions(int device, const unsigned long long *seqs_host, long long n, const pt_sh_params *params, void *out_host,
                                     size_t out_bytes) {
  size_t need;
  int rc = check_directions(device, n, params, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t seq_b = (size_t)n * 8;
  Staged s;
  if ((rc = s.alloc(seq_b + need))) return rc;
  char *seq_d = s.dev, *out_d = seq_d + seq_b;
  if (seqs_host) HIP_TRY(hipMemcpy(seq_d, seqs_host, seq_b, hipMemcpyHostToDevice));
  if ((rc = enqueue_directions(seqs_host ? (const unsigned long long *)seq_d : nullptr, n, *params, out_d, nullptr))) return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}

extern "C" int pt_rays_sh_project(int device, const void *scene_args, size_t scene_args_bytes, const double *points_host, const int *active_host,
                                  const unsigned long long *seqs_host, long long n, const pt_sh_params *params, int channels, void *out_host,
                                  size_t out_bytes) {
  size_t need;
  int rc = check_project(device, scene_args, scene_args_bytes, points_host, n, params, channels, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, total_of(n, *params), params->num_of_rays > 1, lanes))) return rc;
  const size_t pts_b = (size_t)n * 24, act_b = up8((size_t)n * 4), seq_b = (size_t)n * 8, ws_b = workspace_of(lanes, n, *params);
  Staged s;
  if ((rc = s.alloc(pts_b + act_b + seq_b + ws_b + need))) return rc;
  char *pts_d = s.dev, *act_d = pts_d + pts_b, *seq_d = act_d + act_b, *ws_d = seq_d + seq_b, *out_d = ws_d + ws_b;
  HIP_TRY(hipMemcpy(pts_d, points_host, pts_b, hipMemcpyHostToDevice));
  if (active_host) HIP_TRY(hipMemcpy(act_d, active_host, (size_t)n * 4, hipMemcpyHostToDevice));
  if (seqs_host) HIP_TRY(hipMemcpy(seq_d, seqs_host, seq_b, hipMemcpyHostToDevice));
  if ((rc = enqueue_project(scene_args, (const double *)pts_d, active_host ? (const int *)act_d : nullptr,
                            seqs_host ? (const unsigned long long *)seq_d : nullptr, n, *params, channels, lanes, ws_d, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind both kernels)
  return PT_OK;
}

extern "C" int pt_rays_sh_eval(int device, const double *coeffs_host, long long n, const int *index_host, const double *dirs_host, long long m,
                               int kind, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_eval(device, coeffs_host, n, index_host, dirs_host, m, kind, out_host, out_bytes, need);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t co_b = (size_t)n * 8 * PT_SH_COEFFS, idx_b = up8((size_t)m * 4), dir_b = (size_t)m * 24;
  Staged s;
  if ((rc = s.alloc(co_b + idx_b + dir_b + need))) return rc;
  char *co_d = s.dev, *idx_d = co_d + co_b, *dir_d = idx_d + idx_b, *out_d = dir_d + dir_b;
  if (n > 0) HIP_TRY(hipMemcpy(co_d, coeffs_host, co_b, hipMemcpyHostToDevice));
  if (index_host) HIP_TRY(hipMemcpy(idx_d, index_host, (size_t)m * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dir_d, dirs_host, dir_b, hipMemcpyHostToDevice));
  if ((rc = enqueue_eval((const double *)co_d, n, index_host ? (const int *)idx_d : nullptr, (const double *)dir_d, m, kind, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}
