// ptrace_adaptive.hip — libptrace_adaptive.so: the C-ABI of include/ptrace_adaptive.h, sample counts from a variance plane, their
// prefix sum, and a gather whose sample count is a plane.
//
// The kernels are pt_adaptive.h's; the queries are pt_query.h's, the record and the bounce pt_shade.h's, the draws pt_math.h's,
// included here as they are; the sizes and the checks of values are pt_adaptive_host.h's.  Why a thirteenth translation unit and a
// thirteenth shared object: libptrace.so's device code is pinned by build.code_hash, and the exported symbols of the twelve
// libraries beside it are pinned to their interfaces'.  So this library stands beside them: the scene arrives as the argument block
// pt_scene_kernel_args (ptrace.h, ABI 1.7) hands out, there is no link dependency, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_adaptive.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_adaptive.h"
#include "pt_host_common.h"
#include "pt_adaptive_host.h"

#define PT_AD_VERSION ((1 << 16) | 11)
#define PT_AD_DEFAULT_OWNER true       // how a sample finds its record unless PTRACE_ADAPTIVE_LOOKUP says otherwise (the faster, as measured)
#define PT_AD_OWNER_MAX_BLOCKS 65536LL  // the expand launch walks a grid-stride loop

static_assert(PT_AD_SCAN == PT_BLOCK && PT_AD_SCAN_BLOCK == PT_AD_SCAN && PT_AD_PLANES == PT_AD_SAMPLE_PLANES, "the host header's sizes are the kernels'");
static_assert(sizeof(pt_adaptive_count_params) == 32 && sizeof(pt_adaptive_params) == 64, "the structs of the header");

extern "C" int pt_rays_adaptive_version(void) { return PT_AD_VERSION; }

extern "C" size_t pt_rays_adaptive_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_adaptive_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes ------------------------------------------------------------------------------------------------------------------
extern "C" size_t pt_rays_adaptive_bytes(long long n, int channels) { return ad_bytes(n, channels); }

extern "C" long long pt_rays_adaptive_plane_offset(long long n, int channels, int channel, int component) {
  return ad_plane_offset(n, channels, channel, component);
}

extern "C" size_t pt_rays_adaptive_offsets_bytes(long long n) { return ad_offsets_bytes(n); }

extern "C" size_t pt_rays_adaptive_offsets_workspace_bytes(long long n) { return ad_offsets_workspace_bytes(n); }

// ---- launch alternatives, for A/B runs and for the tests that no bit depends on them (read per call) ---------------------------------
//     PTRACE_ADAPTIVE_LOOKUP = search | owner     how a sample finds its record: the walk searches `offsets` itself, or an expand
//                                                 launch writes an owner plane into the workspace first (pt_adaptive.h)
//     PTRACE_ADAPTIVE_PART   = both | walk | mean which of the gather's launches are enqueued (tools/adaptivebench.py times them
//                                                 apart; `mean` alone averages whatever the sample planes hold; `walk` includes the
//                                                 expand launch)
// Any other value is refused with PT_ERR_INVALID.
enum { PT_AD_PART_BOTH = 0, PT_AD_PART_WALK = 1, PT_AD_PART_MEAN = 2 };

struct AdLaunch {
  int part;
  bool owner;
};

static int launch_choice(AdLaunch &L) {
  L.part = PT_AD_PART_BOTH;
  L.owner = PT_AD_DEFAULT_OWNER;
  if (const char *v = getenv("PTRACE_ADAPTIVE_LOOKUP")) {
    if (!strcmp(v, "search")) L.owner = false;
    else if (!strcmp(v, "owner")) L.owner = true;
    else return fail(PT_ERR_INVALID, "PTRACE_ADAPTIVE_LOOKUP=%s: search or owner", v);
  }
  if (const char *v = getenv("PTRACE_ADAPTIVE_PART")) {
    if (!strcmp(v, "both")) L.part = PT_AD_PART_BOTH;
    else if (!strcmp(v, "walk")) L.part = PT_AD_PART_WALK;
    else if (!strcmp(v, "mean")) L.part = PT_AD_PART_MEAN;
    else return fail(PT_ERR_INVALID, "PTRACE_ADAPTIVE_PART=%s: both, walk or mean", v);
  }
  return PT_OK;
}

// ---- the launch's shape -------------------------------------------------------------------------------------------------------
// lanes the walk's launch keeps resident: no more than `capacity` samples need, no more than PTRACE_ADAPTIVE_LANES allows
static int lanes_of(int device, long long capacity, bool many, bool owner, unsigned long long &lanes) {
  const void *kernel = many ? (owner ? (const void *)pt_adaptive_walk_kernel<true, true> : (const void *)pt_adaptive_walk_kernel<true, false>)
                            : (owner ? (const void *)pt_adaptive_walk_kernel<false, true> : (const void *)pt_adaptive_walk_kernel<false, false>);
  return resident_lanes(device, capacity, kernel, "PTRACE_ADAPTIVE_LANES", lanes);
}

static size_t stacks_of(unsigned long long lanes, const pt_adaptive_params &p) {
  return ad_stacks_bytes(lanes, p.num_of_rays, p.max_depth, p.depth0, PT_AD_FIELDS_ONE, PT_AD_FIELDS_MANY);
}

static size_t workspace_of(unsigned long long lanes, const pt_adaptive_params &p, bool owner) {
  return stacks_of(lanes, p) + ad_planes_bytes(p.capacity) + (owner ? ad_owner_bytes(p.capacity) : 0);
}

extern "C" size_t pt_rays_adaptive_workspace_bytes(int device, long long n, long long capacity, int num_of_rays, int max_depth, int depth0) {
  AdLaunch L;
  if (ad_check_walk(n, capacity, num_of_rays, max_depth, depth0) || launch_choice(L)) return 0;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device), 0;
  if (device_ok(device)) return 0;
  if (hipSetDevice(device) != hipSuccess) return fail(PT_ERR_HIP, "hipSetDevice(%d) failed", device), 0;
  unsigned long long lanes;
  if (lanes_of(device, capacity, num_of_rays > 1, L.owner, lanes)) return 0;
  pt_adaptive_params p = {num_of_rays, max_depth, 0, depth0, 0ULL, 0ULL, {0.0, 0.0, 0.0}, capacity};
  return workspace_of(lanes, p, L.owner);
}

// ---- checks: every argument, before any HIP call ------------------------------------------------------------------------------
static int check_counts(int device, long long m, const pt_adaptive_count_params *p, const void *variance, const void *colour, const void *shape,
                        const void *counts, size_t counts_bytes) {
  if (int rc = ad_check_counts(m, p)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!variance || !colour || !shape) return fail(PT_ERR_INVALID, "null variance, colour or shape planes");
  if (!counts) return fail(PT_ERR_INVALID, "null counts output");
  if (counts_bytes < (size_t)m * 4) return fail(PT_ERR_SIZE, "counts output too small: %zu < %zu bytes", counts_bytes, (size_t)m * 4);
  return PT_OK;
}

static int check_offsets(int device, long long n, const void *counts, const void *offsets, size_t offsets_bytes) {
  if (n < 0 || n > PT_AD_MAX_N) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", n);
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (n == 0) return PT_OK;
  if (!counts) return fail(PT_ERR_INVALID, "null counts plane");
  if (!offsets) return fail(PT_ERR_INVALID, "null offsets output");
  if (offsets_bytes < ad_offsets_bytes(n)) return fail(PT_ERR_SIZE, "offsets output too small: %zu < %zu bytes", offsets_bytes, ad_offsets_bytes(n));
  return PT_OK;
}

static int check_gather(int device, const void *scene_args, size_t scene_args_bytes, const double *points, const double *normals, const int *counts,
                        const long long *offsets, long long n, const pt_adaptive_params *p, int channels, const void *out, size_t out_bytes,
                        size_t &need) {
  need = 0;
  if (!p) return fail(PT_ERR_INVALID, "null pt_adaptive_params");
  if (int rc = ad_check_walk(n, p->capacity, p->num_of_rays, p->max_depth, p->depth0)) return rc;
  if (channels < 0 || (channels & ~PT_ADAPTIVE_ALL))
    return fail(PT_ERR_INVALID, "channel bits %#x: an adaptive batch has PT_ADAPTIVE_COUNT and PT_ADAPTIVE_TAKEN", channels);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, PT_BLOCK_SHAPES)) return rc;
  need = ad_bytes(n, channels);
  if (n == 0) return PT_OK;
  if (!points || !normals) return fail(PT_ERR_INVALID, "null record planes (points, normals)");
  if (!counts || !offsets) return fail(PT_ERR_INVALID, "null counts or offsets plane");
  if (!out) return fail(PT_ERR_INVALID, "null output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "adaptive output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

// ---- the launches -----------------------------------------------------------------------------------------------------------------
static int enqueue_counts(long long m, const pt_adaptive_count_params &p, const double *variance, const double *colour, const int *shape, int *counts,
                          hipStream_t st) {
  const PtAdC C = {p.min_samples, p.max_samples, p.tolerance, p.luminance_floor, p.gain};
  hipLaunchKernelGGL(pt_adaptive_counts_kernel, grid_of(m), dim3(PT_BLOCK), 0, st, variance, colour, shape, m, C, counts);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_offsets(long long n, const int *counts, long long *offsets, long long *sums, hipStream_t st) {
  const long long nb = ad_scan_blocks(n);
  hipLaunchKernelGGL(pt_adaptive_sums_kernel, dim3((unsigned)nb), dim3(PT_BLOCK), 0, st, counts, n, sums);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(pt_adaptive_scan_sums_kernel, dim3(1), dim3(PT_BLOCK), 0, st, sums, nb);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(pt_adaptive_offsets_kernel, dim3((unsigned)nb), dim3(PT_BLOCK), 0, st, counts, n, (const long long *)sums, offsets);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

static int enqueue_gather(const void *scene_args, const double *points_dev, const double *normals_dev, const int *active_dev,
                          const unsigned long long *seq_dev, const int *counts_dev, const long long *offsets_dev, long long n,
                          const pt_adaptive_params &p, int channels, const AdLaunch &L, unsigned long long lanes, void *ws_dev, void *out_dev,
                          hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  PtAdK K;
  K.N = p.num_of_rays;
  const long long levels = (long long)p.max_depth - p.depth0;
  K.levels = levels < 0 ? -1 : (int)levels;
  K.rr_rel = (int)std::min<long long>(std::max<long long>((long long)p.rr_limit - p.depth0, -1), PT_ADAPTIVE_MAX_LEVELS + 1);
  K.channels = channels;
  K.bg[0] = p.background[0];
  K.bg[1] = p.background[1];
  K.bg[2] = p.background[2];
  K.invN = 1.0 / p.num_of_rays;
  K.init_state = p.init_state;
  K.init_seq = p.init_seq;
  K.lanes = lanes;
  K.capacity = p.capacity;
  double *stacks = (double *)ws_dev;
  double *samples = (double *)((char *)ws_dev + stacks_of(lanes, p));
  int *owner = (int *)((char *)samples + ad_planes_bytes(p.capacity));  // (behind the sample planes; there only if L.owner)
  if (p.capacity > 0 && L.part != PT_AD_PART_MEAN) {  // (capacity 0: no plane holds a sample, nothing to walk, every record is black)
    const dim3 grid((unsigned)(lanes / PT_BLOCK));
    const int *co = owner;
    if (L.owner) {
      const long long blocks = std::min<long long>((p.capacity + PT_BLOCK - 1) / PT_BLOCK, PT_AD_OWNER_MAX_BLOCKS);
      hipLaunchKernelGGL(pt_adaptive_owner_kernel, dim3((unsigned)blocks), dim3(PT_BLOCK), 0, st, offsets_dev, n, p.capacity, owner);
      HIP_TRY(hipGetLastError());
    }
#define PT_AD_WALK(MANY, OWNER)                                                                                                                 \
  hipLaunchKernelGGL((pt_adaptive_walk_kernel<MANY, OWNER>), grid, dim3(PT_BLOCK), 0, st, a, points_dev, normals_dev, active_dev, seq_dev, counts_dev, \
                     offsets_dev, n, K, stacks, samples, co)
    if (p.num_of_rays > 1) {
      if (L.owner) PT_AD_WALK(true, true);
      else PT_AD_WALK(true, false);
    } else {
      if (L.owner) PT_AD_WALK(false, true);
      else PT_AD_WALK(false, false);
    }
#undef PT_AD_WALK
    HIP_TRY(hipGetLastError());
  }
  if (L.part == PT_AD_PART_WALK) return PT_OK;
  // the mean: behind the walk on the same stream, one lane per record
  hipLaunchKernelGGL(pt_adaptive_mean_kernel, grid_of(n), dim3(PT_BLOCK), 0, st, (const double *)samples, active_dev, counts_dev, offsets_dev, n, K,
                     out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- device forms -----------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_adaptive_counts_device(int device, long long m, const pt_adaptive_count_params *params, const double *variance_dev,
                                              const double *colour_dev, const int *shape_dev, int *counts_dev, size_t counts_bytes, void *stream) {
  int rc = check_counts(device, m, params, variance_dev, colour_dev, shape_dev, counts_dev, counts_bytes);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_counts(m, *params, variance_dev, colour_dev, shape_dev, counts_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_adaptive_offsets_device(int device, long long n, const int *counts_dev, long long *offsets_dev, size_t offsets_bytes,
                                               void *workspace_dev, size_t workspace_bytes, void *stream) {
  int rc = check_offsets(device, n, counts_dev, offsets_dev, offsets_bytes);
  if (rc || n == 0) return rc;
  if (!workspace_dev) return fail(PT_ERR_INVALID, "null workspace (pt_rays_adaptive_offsets_workspace_bytes says how large)");
  if (workspace_bytes < ad_offsets_workspace_bytes(n))
    return fail(PT_ERR_SIZE, "offsets workspace too small: %zu < %zu bytes", workspace_bytes, ad_offsets_workspace_bytes(n));
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_offsets(n, counts_dev, offsets_dev, (long long *)workspace_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_adaptive_gather_device(int device, const void *scene_args, size_t scene_args_bytes, const double *points_dev,
                                              const double *normals_dev, const int *active_dev, const unsigned long long *seq_dev,
                                              const int *counts_dev, const long long *offsets_dev, long long n, const pt_adaptive_params *params,
                                              int channels, void *workspace_dev, size_t workspace_bytes, void *out_dev, size_t out_bytes,
                                              void *stream) {
  size_t need;
  int rc = check_gather(device, scene_args, scene_args_bytes, points_dev, normals_dev, counts_dev, offsets_dev, n, params, channels, out_dev, out_bytes,
                        need);
  if (rc || n == 0) return rc;
  AdLaunch L;
  if ((rc = launch_choice(L))) return rc;
  if (!workspace_dev) return fail(PT_ERR_INVALID, "null workspace (pt_rays_adaptive_workspace_bytes says how large)");
  // (whatever the resident lanes turn out to be, the sample planes alone need this much: refused before any HIP call)
  const size_t planes = ad_planes_bytes(params->capacity);
  if (workspace_bytes < planes)
    return fail(PT_ERR_SIZE, "adaptive workspace too small: %zu bytes do not hold the sample planes (%zu)", workspace_bytes, planes);
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, params->capacity, params->num_of_rays > 1, L.owner, lanes))) return rc;
  const size_t ws_need = workspace_of(lanes, *params, L.owner);
  if (workspace_bytes < ws_need) return fail(PT_ERR_SIZE, "adaptive workspace too small: %zu < %zu bytes", workspace_bytes, ws_need);
  if ((rc = enqueue_gather(scene_args, points_dev, normals_dev, active_dev, seq_dev, counts_dev, offsets_dev, n, *params, channels, L, lanes,
                           workspace_dev, out_dev, (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ---- host forms: one device allocation holds the inputs, the workspace and the output ----------------------------------------------
extern "C" int pt_rays_adaptive_counts(int device, long long m, const pt_adaptive_count_params *params, const double *variance_host,
                                       const double *colour_host, const int *shape_host, int *counts_host, size_t counts_bytes) {
  int rc = check_counts(device, m, params, variance_host, colour_host, shape_host, counts_host, counts_bytes);
  if (rc || m == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b3 = (size_t)m * 24, b2 = (size_t)m * 8, b1 = up8((size_t)m * 4);
  Staged s;
  if ((rc = s.alloc(b3 + b2 + 2 * b1))) return rc;
  char *col_d = s.dev, *var_d = col_d + b3, *shape_d = var_d + b2, *out_d = shape_d + b1;
  HIP_TRY(hipMemcpy(col_d, colour_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(var_d, variance_host, b2, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(shape_d, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_counts(m, *params, (const double *)var_d, (const double *)col_d, (const int *)shape_d, (int *)out_d, nullptr))) return rc;
  HIP_TRY(hipMemcpy(counts_host, out_d, (size_t)m * 4, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}

extern "C" int pt_rays_adaptive_offsets(int device, long long n, const int *counts_host, long long *offsets_host, size_t offsets_bytes) {
  int rc = check_offsets(device, n, counts_host, offsets_host, offsets_bytes);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b1 = up8((size_t)n * 4), off_b = ad_offsets_bytes(n), ws_b = ad_offsets_workspace_bytes(n);
  Staged s;
  if ((rc = s.alloc(off_b + ws_b + b1))) return rc;
  char *off_d = s.dev, *ws_d = off_d + off_b, *cnt_d = ws_d + ws_b;
  HIP_TRY(hipMemcpy(cnt_d, counts_host, (size_t)n * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_offsets(n, (const int *)cnt_d, (long long *)off_d, (long long *)ws_d, nullptr))) return rc;
  HIP_TRY(hipMemcpy(offsets_host, off_d, off_b, hipMemcpyDeviceToHost));
  return PT_OK;
}

extern "C" int pt_rays_adaptive_gather(int device, const void *scene_args, size_t scene_args_bytes, const double *points_host,
                                       const double *normals_host, const int *active_host, const unsigned long long *seq_host,
                                       const int *counts_host, const long long *offsets_host, long long n, const pt_adaptive_params *params,
                                       int channels, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_gather(device, scene_args, scene_args_bytes, points_host, normals_host, counts_host, offsets_host, n, params, channels, out_host,
                        out_bytes, need);
  if (rc || n == 0) return rc;
  AdLaunch L;
  if ((rc = launch_choice(L))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  unsigned long long lanes;
  if ((rc = lanes_of(device, params->capacity, params->num_of_rays > 1, L.owner, lanes))) return rc;
  const size_t plane = (size_t)n * 8, ws_b = workspace_of(lanes, *params, L.owner), need8 = up8(need);
  // points 3, normals 3, seq 1, offsets 1 (+ 8), active and counts 1 each (int32, padded)
  const size_t total = 10 * plane + 8 + ws_b + need8;
  Staged s;
  if ((rc = s.alloc(total))) return rc;
  char *points_d = s.dev, *normals_d = points_d + 3 * plane, *seq_d = normals_d + 3 * plane, *off_d = seq_d + plane, *ws_d = off_d + plane + 8,
       *out_d = ws_d + ws_b, *act_d = out_d + need8, *cnt_d = act_d + plane;
  HIP_TRY(hipMemcpy(points_d, points_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(normals_d, normals_host, 3 * plane, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(off_d, offsets_host, plane + 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(cnt_d, counts_host, (size_t)n * 4, hipMemcpyHostToDevice));
  if (seq_host) HIP_TRY(hipMemcpy(seq_d, seq_host, plane, hipMemcpyHostToDevice));
  if (active_host) HIP_TRY(hipMemcpy(act_d, active_host, (size_t)n * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_gather(scene_args, (const double *)points_d, (const double *)normals_d, active_host ? (const int *)act_d : nullptr,
                           seq_host ? (const unsigned long long *)seq_d : nullptr, (const int *)cnt_d, (const long long *)off_d, n, *params,
                           channels, L, lanes, ws_d, out_d, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost));  // (the null stream: behind both kernels)
  return PT_OK;
}
