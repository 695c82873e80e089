// ptrace_gradient.hip — libptrace_gradient.so: the C-ABI of include/ptrace_gradient.h, temporal gradients for the accumulation over
// frames: probes of this frame to be gathered in the previous world, the share of its history every pixel keeps, and the motion
// accumulation with that share applied.
//
// The kernels are pt_gradient.h's.  Why a sixteenth translation unit and a sixteenth shared object: libptrace.so's device code is
// pinned by build.code_hash, and the exported symbols of the fifteen libraries beside it are pinned to their interfaces'.  So this
// library stands beside them: no link dependency, nothing is loaded from here, and no scene is read.
//
// A launch alternative, for the tests that no bit depends on it (read per call):
//     PTRACE_GR_BLOCKS = N              at most N workgroups (every kernel walks a grid-stride loop)
// Any other value is refused with PT_ERR_INVALID.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ptrace_gradient.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_gradient.h"
#include "pt_host_common.h"

#define PT_GR_VERSION ((1 << 16) | 14)
#define PT_GR_MAX_M 2147483647LL
#define PT_GR_MAX_GRID 2147483647LL

static_assert(PT_GR_FLAG_SAME_SHAPE == PT_GR_SAME_SHAPE && PT_GR_FLAG_BLEND_WEIGHT == PT_GR_BLEND_WEIGHT, "the kernels' flag bits are the header's");
static_assert(sizeof(pt_gradient_params) == 24 && sizeof(pt_gradient_history) == 32 && sizeof(pt_gradient_camera) == 120, "the structs of the header");
static_assert(PT_GR_RECORD_DOUBLES == PT_GR_RECORD && PT_GR_RECORD * sizeof(double) == 192, "a table record of the header: 192 bytes");
static_assert(PT_GR_RADIUS_MAX == PT_GR_MAX_RADIUS, "one keep kernel per radius of the header");

extern "C" int pt_rays_gradient_version(void) { return PT_GR_VERSION; }

extern "C" int pt_rays_gradient_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes and checks: every argument, before any HIP call ---------------------------------------------------------------------
extern "C" long long pt_rays_gradient_strata(int width, int height, int stratum) {
  if (width < 0 || height < 0 || (long long)width * height > PT_GR_MAX_M || stratum < 1 || stratum > PT_GR_MAX_STRATUM) return 0;
  return (long long)((width + stratum - 1) / stratum) * ((height + stratum - 1) / stratum);
}

extern "C" size_t pt_rays_gradient_keep_bytes(long long m) { return (m >= 0 && m <= PT_GR_MAX_M) ? (size_t)m * 8 : 0; }

extern "C" size_t pt_rays_gradient_bytes(long long m) { return (m >= 0 && m <= PT_GR_MAX_M) ? (size_t)m * 24 : 0; }

extern "C" size_t pt_rays_gradient_count_bytes(long long m) { return (m >= 0 && m <= PT_GR_MAX_M) ? (size_t)m * 4 : 0; }

extern "C" size_t pt_rays_gradient_table_bytes(int n_shapes) { return (n_shapes >= 0 && n_shapes <= PT_GR_MAX_SHAPES) ? (size_t)n_shapes * 192 : 0; }

static int check_size(int width, int height, long long &m) {
  m = 0;
  if (width < 0 || height < 0) return fail(PT_ERR_INVALID, "frame of %d x %d records", width, height);
  if ((long long)width * height > PT_GR_MAX_M) return fail(PT_ERR_INVALID, "record count %d x %d outside [0, 2^31 - 1]", width, height);
  m = (long long)width * height;
  return PT_OK;
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

struct Span {
  const void *at;
  size_t bytes;
  const char *name;
};

// no output may overlap anything the call reads, or another output
static int check_overlaps(const Span *outs, int n_outs, const Span *reads, int n_reads, const char *why) {
  for (int i = 0; i < n_outs; i++)
    for (int j = 0; j < n_reads; j++)
      if (reads[j].bytes && reads[j].at && overlap(outs[i].at, outs[i].bytes, reads[j].at, reads[j].bytes))
        return fail(PT_ERR_INVALID, "the %s output overlaps %s%s", outs[i].name, reads[j].name, why);
  for (int i = 0; i < n_outs; i++)
    for (int j = i + 1; j < n_outs; j++)
      if (overlap(outs[i].at, outs[i].bytes, outs[j].at, outs[j].bytes))
        return fail(PT_ERR_INVALID, "the %s output overlaps the %s output", outs[i].name, outs[j].name);
  return PT_OK;
}

// ---- the launch alternative -----------------------------------------------------------------------------------------------------
static int launch_choice(long long &max_blocks) {
  max_blocks = PT_GR_MAX_GRID;
  if (const char *v = getenv("PTRACE_GR_BLOCKS")) {
    char *end = nullptr;
    const long long n = strtoll(v, &end, 10);
    if (end == v || *end || n < 1) return fail(PT_ERR_INVALID, "PTRACE_GR_BLOCKS=%s: a positive count of workgroups", v);
    max_blocks = std::min(n, PT_GR_MAX_GRID);
  }
  return PT_OK;
}

static dim3 blocks_for(long long items, long long max_blocks) { return dim3((unsigned)std::min((items + PT_BLOCK - 1) / PT_BLOCK, max_blocks)); }

// ---- an empty history -------------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_gradient_clear_device(int device, long long m, void *count_dev, size_t count_bytes, void *stream) {
  if (m < 0 || m > PT_GR_MAX_M) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", m);
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!count_dev) return fail(PT_ERR_INVALID, "null count buffer");
  if (count_bytes < (size_t)m * 4) return fail(PT_ERR_SIZE, "count buffer too small: %zu < %zu bytes", count_bytes, (size_t)m * 4);
  if (int rc = device_ok(device)) return rc;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemsetAsync(count_dev, 0, (size_t)m * 4, (hipStream_t)stream));
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// ==== 1. probes ======================================================================================================================
struct ProbeIn {
  const int *shape;
  const double *normal, *point;
  int n_shapes;
  const int *moved;  // (both may be NULL with n_shapes = 0)
  const double *motion;
};

struct ProbeOut {
  void *index;
  size_t index_bytes;
  void *point;
  size_t point_bytes;
  void *normal;
  size_t normal_bytes;
  void *seq;
  size_t seq_bytes;
};

static int check_probes(int device, int width, int height, int stratum, int samples, const ProbeIn &in, const ProbeOut &out, long long &m,
                        long long &ns) {
  ns = 0;
  if (int rc = check_size(width, height, m)) return rc;
  if (stratum < 1 || stratum > PT_GR_MAX_STRATUM) return fail(PT_ERR_INVALID, "stratum = %d: 1 to 16", stratum);
  if (samples < 1) return fail(PT_ERR_INVALID, "samples = %d: at least 1", samples);
  if (in.n_shapes < 0 || in.n_shapes > PT_GR_MAX_SHAPES) return fail(PT_ERR_INVALID, "n_shapes = %d: 0 to 2^20", in.n_shapes);
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  ns = pt_rays_gradient_strata(width, height, stratum);
  if (!in.shape || !in.normal || !in.point) return fail(PT_ERR_INVALID, "null shape, normal or point planes");
  if (in.n_shapes > 0 && (!in.moved || !in.motion)) return fail(PT_ERR_INVALID, "null moved or motion table for %d shapes", in.n_shapes);
  if (!out.index || !out.point || !out.normal || !out.seq) return fail(PT_ERR_INVALID, "null output buffer");
  const size_t b3 = (size_t)m * 24, b1 = (size_t)m * 4, n3 = (size_t)ns * 24, n1 = (size_t)ns * 4, n2 = (size_t)ns * 8;
  const Span outs[4] = {{out.index, n1, "probe index"}, {out.point, n3, "probe point"}, {out.normal, n3, "probe normal"}, {out.seq, n2, "probe seq"}};
  const Span reads[5] = {{in.shape, b1, "the shapes"},
                         {in.normal, b3, "the normals"},
                         {in.point, b3, "the points"},
                         {in.moved, (size_t)in.n_shapes * 4, "the moved table"},
                         {in.motion, (size_t)in.n_shapes * 192, "the motion table"}};
  if (int rc = check_overlaps(outs, 4, reads, 5, "")) return rc;
  if (out.index_bytes < n1) return fail(PT_ERR_SIZE, "probe index output too small: %zu < %zu bytes", out.index_bytes, n1);
  if (out.point_bytes < n3) return fail(PT_ERR_SIZE, "probe point output too small: %zu < %zu bytes", out.point_bytes, n3);
  if (out.normal_bytes < n3) return fail(PT_ERR_SIZE, "probe normal output too small: %zu < %zu bytes", out.normal_bytes, n3);
  if (out.seq_bytes < n2) return fail(PT_ERR_SIZE, "probe seq output too small: %zu < %zu bytes", out.seq_bytes, n2);
  return PT_OK;
}

static int enqueue_probes(long long max_blocks, int width, int height, int stratum, unsigned long long phase, int samples, unsigned long long init_seq,
                          long long m, long long ns, const ProbeIn &in, int *index, double *point, double *normal, unsigned long long *seq,
                          hipStream_t st) {
  PtGrProbeK K;
  K.W = width, K.H = height, K.s = stratum, K.gw = (width + stratum - 1) / stratum;
  K.n_shapes = (in.moved && in.motion) ? in.n_shapes : 0;
  K.m = m, K.ns = ns, K.phase = phase, K.K = (unsigned long long)samples, K.init_seq = init_seq;
  hipLaunchKernelGGL(pt_gr_probes_kernel, blocks_for(ns, max_blocks), dim3(PT_BLOCK), 0, st, K, in.shape, in.normal, in.point, in.moved, in.motion,
                     index, point, normal, seq);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

extern "C" int pt_rays_gradient_probes_device(int device, int width, int height, int stratum, unsigned long long phase, int samples,
                                              unsigned long long init_seq, const int *shape_dev, const double *normal_dev, const double *point_dev,
                                              int n_shapes, const int *moved_dev, const double *motion_dev, void *probe_index_dev,
                                              size_t probe_index_bytes, void *probe_point_dev, size_t probe_point_bytes, void *probe_normal_dev,
                                              size_t probe_normal_bytes, void *probe_seq_dev, size_t probe_seq_bytes, void *stream) {
  long long m, ns, max_blocks;
  const ProbeIn in = {shape_dev, normal_dev, point_dev, n_shapes, moved_dev, motion_dev};
  const ProbeOut out = {probe_index_dev, probe_index_bytes, probe_point_dev, probe_point_bytes, probe_normal_dev, probe_normal_bytes,
                        probe_seq_dev,   probe_seq_bytes};
  int rc = check_probes(device, width, height, stratum, samples, in, out, m, ns);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(max_blocks))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_probes(max_blocks, width, height, stratum, phase, samples, init_seq, m, ns, in, (int *)probe_index_dev, (double *)probe_point_dev,
                           (double *)probe_normal_dev, (unsigned long long *)probe_seq_dev, (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_gradient_probes(int device, int width, int height, int stratum, unsigned long long phase, int samples,
                                       unsigned long long init_seq, const int *shape_host, const double *normal_host, const double *point_host,
                                       int n_shapes, const int *moved_host, const double *motion_host, void *probe_index_host,
                                       size_t probe_index_bytes, void *probe_point_host, size_t probe_point_bytes, void *probe_normal_host,
                                       size_t probe_normal_bytes, void *probe_seq_host, size_t probe_seq_bytes) {
  long long m, ns, max_blocks;
  const ProbeIn in = {shape_host, normal_host, point_host, n_shapes, moved_host, motion_host};
  const ProbeOut out = {probe_index_host, probe_index_bytes, probe_point_host, probe_point_bytes, probe_normal_host, probe_normal_bytes,
                        probe_seq_host,   probe_seq_bytes};
  int rc = check_probes(device, width, height, stratum, samples, in, out, m, ns);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(max_blocks))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  // the motion table first (its records on 64-byte boundaries), the moved words, the frame's planes, then the four outputs
  const size_t b3 = (size_t)m * 24, b1 = up8((size_t)m * 4), tb = (size_t)n_shapes * 192, fb = up8((size_t)n_shapes * 4);
  const size_t n3 = (size_t)ns * 24, n2 = (size_t)ns * 8, n1 = up8((size_t)ns * 4);
  Staged s;
  if ((rc = s.alloc(tb + fb + 2 * b3 + b1 + 2 * n3 + n2 + n1))) return rc;
  char *dt = s.dev, *df = dt + tb, *dn = df + fb, *dp = dn + b3, *dsh = dp + b3, *op = dsh + b1, *on = op + n3, *os = on + n3, *oi = os + n2;
  if (n_shapes > 0) {
    HIP_TRY(hipMemcpy(dt, motion_host, tb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(df, moved_host, (size_t)n_shapes * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(dn, normal_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dp, point_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dsh, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  const ProbeIn dev = {(const int *)dsh, (const double *)dn, (const double *)dp, n_shapes, n_shapes > 0 ? (const int *)df : nullptr,
                       n_shapes > 0 ? (const double *)dt : nullptr};
  if ((rc = enqueue_probes(max_blocks, width, height, stratum, phase, samples, init_seq, m, ns, dev, (int *)oi, (double *)op, (double *)on,
                           (unsigned long long *)os, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(probe_index_host, oi, (size_t)ns * 4, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  HIP_TRY(hipMemcpy(probe_point_host, op, n3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(probe_normal_host, on, n3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(probe_seq_host, os, n2, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ==== 2. keep ========================================================================================================================
static int check_keep(int device, int width, int height, const pt_gradient_params *p, const double *colour, const int *shape, const int *probe_index,
                      const double *probe_old, const void *keep, size_t keep_bytes, long long &m, long long &ns) {
  ns = 0;
  if (int rc = check_size(width, height, m)) return rc;
  if (!p) return fail(PT_ERR_INVALID, "null pt_gradient_params");
  if (p->stratum < 1 || p->stratum > PT_GR_MAX_STRATUM) return fail(PT_ERR_INVALID, "stratum = %d: 1 to 16", p->stratum);
  if (p->radius < 0 || p->radius > PT_GR_MAX_RADIUS) return fail(PT_ERR_INVALID, "radius = %d: 0 to 4", p->radius);
  if (p->flags & ~PT_GR_SAME_SHAPE) return fail(PT_ERR_INVALID, "unknown flag bits in 0x%x", (unsigned)p->flags);
  if (!(p->gain >= 0.0)) return fail(PT_ERR_INVALID, "gain = %g: not negative (or +inf)", p->gain);
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  ns = pt_rays_gradient_strata(width, height, p->stratum);
  if (!colour || !shape || !probe_index || !probe_old) return fail(PT_ERR_INVALID, "null colour, shape, probe index or probe_old planes");
  if (!keep) return fail(PT_ERR_INVALID, "null output buffer");
  const Span outs[1] = {{keep, (size_t)m * 8, "keep"}};
  const Span reads[4] = {{colour, (size_t)m * 24, "the colour planes"},
                         {shape, (size_t)m * 4, "the shapes"},
                         {probe_index, (size_t)ns * 4, "the probe indices"},
                         {probe_old, (size_t)ns * 24, "the probes' old colours"}};
  if (int rc = check_overlaps(outs, 1, reads, 4, "")) return rc;
  if (keep_bytes < (size_t)m * 8) return fail(PT_ERR_SIZE, "keep output too small: %zu < %zu bytes", keep_bytes, (size_t)m * 8);
  return PT_OK;
}

static int enqueue_keep(long long max_blocks, int width, int height, const pt_gradient_params &p, long long m, long long ns, const double *colour,
                        const int *shape, const int *probe_index, const double *probe_old, double *keep, hipStream_t st) {
  PtGrKeepK K;
  K.W = width, K.H = height, K.s = p.stratum, K.gw = (width + p.stratum - 1) / p.stratum, K.gh = (height + p.stratum - 1) / p.stratum;
  K.flags = p.flags, K.m = m, K.ns = ns, K.gain = p.gain;
  const dim3 grid = blocks_for(m, max_blocks);
  // one kernel per radius, so that every loop over the window is unrolled
  void (*const kernels[PT_GR_RADIUS_MAX + 1])(PtGrKeepK, const double *, const int *, const int *, const double *, double *) = {
      pt_gr_keep_kernel<0>, pt_gr_keep_kernel<1>, pt_gr_keep_kernel<2>, pt_gr_keep_kernel<3>, pt_gr_keep_kernel<4>};
  hipLaunchKernelGGL(kernels[p.radius], grid, dim3(PT_BLOCK), 0, st, K, colour, shape, probe_index, probe_old, keep);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

extern "C" int pt_rays_gradient_keep_device(int device, int width, int height, const pt_gradient_params *params, const double *colour_dev,
                                            const int *shape_dev, const int *probe_index_dev, const double *probe_old_dev, void *keep_dev,
                                            size_t keep_bytes, void *stream) {
  long long m, ns, max_blocks;
  int rc = check_keep(device, width, height, params, colour_dev, shape_dev, probe_index_dev, probe_old_dev, keep_dev, keep_bytes, m, ns);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(max_blocks))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue_keep(max_blocks, width, height, *params, m, ns, colour_dev, shape_dev, probe_index_dev, probe_old_dev, (double *)keep_dev,
                         (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_gradient_keep(int device, int width, int height, const pt_gradient_params *params, const double *colour_host,
                                     const int *shape_host, const int *probe_index_host, const double *probe_old_host, void *keep_host,
                                     size_t keep_bytes) {
  long long m, ns, max_blocks;
  int rc = check_keep(device, width, height, params, colour_host, shape_host, probe_index_host, probe_old_host, keep_host, keep_bytes, m, ns);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(max_blocks))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b3 = (size_t)m * 24, b2 = (size_t)m * 8, b1 = up8((size_t)m * 4), n3 = (size_t)ns * 24, n1 = up8((size_t)ns * 4);
  Staged s;
  if ((rc = s.alloc(b3 + b2 + n3 + b1 + n1))) return rc;
  char *dc = s.dev, *dk = dc + b3, *dold = dk + b2, *dsh = dold + n3, *di = dsh + b1;
  HIP_TRY(hipMemcpy(dc, colour_host, b3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dold, probe_old_host, n3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dsh, shape_host, (size_t)m * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(di, probe_index_host, (size_t)ns * 4, hipMemcpyHostToDevice));
  if ((rc = enqueue_keep(max_blocks, width, height, *params, m, ns, (const double *)dc, (const int *)dsh, (const int *)di, (const double *)dold,
                         (double *)dk, nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(keep_host, dk, b2, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  return PT_OK;
}

// ==== 3. the accumulation ============================================================================================================
static int check_frame(int width, int height, const pt_gradient_history *p, const pt_gradient_camera *cam, int n_shapes, long long &m) {
  if (int rc = check_size(width, height, m)) return rc;
  const long long records = m;
  m = 0;
  if (!p) return fail(PT_ERR_INVALID, "null pt_gradient_history");
  if (!cam) return fail(PT_ERR_INVALID, "null pt_gradient_camera");
  if (p->max_history < 1 || p->max_history > PT_GR_MAX_HISTORY) return fail(PT_ERR_INVALID, "max_history = %d: 1 to 2^20", p->max_history);
  if (p->flags & ~(PT_GR_SAME_SHAPE | PT_GR_BLEND_WEIGHT)) return fail(PT_ERR_INVALID, "unknown flag bits in 0x%x", (unsigned)p->flags);
  if (!(p->normal_min >= -1.0 && p->normal_min <= 1.0)) return fail(PT_ERR_INVALID, "normal_min = %g: a cosine, -1 to 1", p->normal_min);
  if (!(p->point_tolerance > 0.0)) return fail(PT_ERR_INVALID, "point_tolerance = %g: positive (or +inf)", p->point_tolerance);
  if (!(p->max_weight >= 0.0)) return fail(PT_ERR_INVALID, "max_weight = %g: not negative (or +inf)", p->max_weight);
  if (cam->kind != PT_CAMERA_ORTHOGONAL && cam->kind != PT_CAMERA_PERSPECTIVE) return fail(PT_ERR_INVALID, "unknown camera kind %d", cam->kind);
  if (n_shapes < 0 || n_shapes > PT_GR_MAX_SHAPES) return fail(PT_ERR_INVALID, "n_shapes = %d: 0 to 2^20", n_shapes);
  m = records;
  return PT_OK;
}

struct GrPlanes {
  const double *colour;
  const int *samples;  // (may be NULL: one sample everywhere)
  const int *shape;
  const double *normal, *point, *prev_colour, *prev_moments;
  const int *prev_shape;
  const double *prev_normal, *prev_point;
  const int *prev_count;
  int n_shapes;
  const int *moved;      // (both may be NULL with n_shapes = 0)
  const double *motion;
  const double *keep;    // (may be NULL: everything is kept)
};

struct GrOuts {
  void *colour;
  size_t colour_bytes;
  void *moments;
  size_t moments_bytes;
  void *count;
  size_t count_bytes;
};

static int check_all(int device, int width, int height, const pt_gradient_history *p, const pt_gradient_camera *cam, const GrPlanes &in,
                     const GrOuts &out, long long &m) {
  if (int rc = check_frame(width, height, p, cam, in.n_shapes, m)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!in.colour || !in.shape || !in.normal || !in.point) return fail(PT_ERR_INVALID, "null colour, shape, normal or point planes");
  if (!in.prev_colour || !in.prev_moments || !in.prev_shape || !in.prev_normal || !in.prev_point || !in.prev_count)
    return fail(PT_ERR_INVALID, "null previous colour, moments, shape, normal, point or count planes");
  if (in.n_shapes > 0 && (!in.moved || !in.motion)) return fail(PT_ERR_INVALID, "null moved or motion table for %d shapes", in.n_shapes);
  if (!out.colour || !out.moments || !out.count) return fail(PT_ERR_INVALID, "null output buffer");
  const size_t b3 = (size_t)m * 24, b1 = (size_t)m * 4;
  const Span outs[3] = {{out.colour, b3, "colour"}, {out.moments, b3, "moments"}, {out.count, b1, "count"}};
  const Span reads[11] = {{in.colour, b3, "the colour planes"},
                          {in.samples, in.samples ? b1 : 0, "the sample counts"},
                          {in.prev_colour, b3, "the previous colour planes"},
                          {in.prev_moments, b3, "the previous moments"},
                          {in.prev_shape, b1, "the previous shapes"},
                          {in.prev_normal, b3, "the previous normals"},
                          {in.prev_point, b3, "the previous points"},
                          {in.prev_count, b1, "the previous counts"},
                          {in.moved, (size_t)in.n_shapes * 4, "the moved table"},
                          {in.motion, (size_t)in.n_shapes * 192, "the motion table"},
                          {in.keep, in.keep ? (size_t)m * 8 : 0, "the keep plane"}};
  if (int rc = check_overlaps(outs, 3, reads, 11, ": a tap reads its neighbours' history (ping-pong two buffers)")) return rc;
  if (out.colour_bytes < b3) return fail(PT_ERR_SIZE, "colour output too small: %zu < %zu bytes", out.colour_bytes, b3);
  if (out.moments_bytes < b3) return fail(PT_ERR_SIZE, "moments output too small: %zu < %zu bytes", out.moments_bytes, b3);
  if (out.count_bytes < b1) return fail(PT_ERR_SIZE, "count output too small: %zu < %zu bytes", out.count_bytes, b1);
  return PT_OK;
}

static int enqueue(long long max_blocks, int width, int height, const pt_gradient_history &p, const pt_gradient_camera &cam, long long m,
                   const GrPlanes &in, double *out_colour, double *out_moments, int *out_count, hipStream_t st) {
  PtGrK K;
  K.W = width, K.H = height, K.m = m, K.max_history = p.max_history, K.flags = p.flags;
  K.persp = cam.kind == PT_CAMERA_PERSPECTIVE;
  K.n_shapes = (in.moved && in.motion) ? in.n_shapes : 0;
  K.normal_min = p.normal_min, K.point_tolerance = p.point_tolerance, K.max_weight = p.max_weight;
  for (int i = 0; i < 12; i++) K.invm[i] = cam.invm[i];
  K.d = cam.screen_distance, K.a = cam.aspect_ratio;
  hipLaunchKernelGGL(pt_gr_accumulate_kernel, blocks_for(m, max_blocks), dim3(PT_BLOCK), 0, st, K, in.colour, in.samples, in.shape, in.normal, in.point,
                     in.prev_colour, in.prev_moments, in.prev_shape, in.prev_normal, in.prev_point, in.prev_count, in.moved, in.motion, in.keep,
                     out_colour, out_moments, out_count);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

extern "C" int pt_rays_gradient_accumulate_device(int device, int width, int height, const pt_gradient_history *params,
                                                  const pt_gradient_camera *prev_camera, const double *colour_dev, const int *samples_dev,
                                                  const int *shape_dev, const double *normal_dev, const double *point_dev,
                                                  const double *prev_colour_dev, const double *prev_moments_dev, const int *prev_shape_dev,
                                                  const double *prev_normal_dev, const double *prev_point_dev, const int *prev_count_dev,
                                                  int n_shapes, const int *moved_dev, const double *motion_dev, const double *keep_dev,
                                                  void *out_colour_dev, size_t out_colour_bytes, void *out_moments_dev, size_t out_moments_bytes,
                                                  void *out_count_dev, size_t out_count_bytes, void *stream) {
  long long m, max_blocks;
  const GrPlanes in = {colour_dev,     samples_dev,     shape_dev,      normal_dev,     point_dev, prev_colour_dev, prev_moments_dev, prev_shape_dev,
                       prev_normal_dev, prev_point_dev, prev_count_dev, n_shapes,       moved_dev, motion_dev,      keep_dev};
  const GrOuts out = {out_colour_dev, out_colour_bytes, out_moments_dev, out_moments_bytes, out_count_dev, out_count_bytes};
  int rc = check_all(device, width, height, params, prev_camera, in, out, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(max_blocks))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue(max_blocks, width, height, *params, *prev_camera, m, in, (double *)out_colour_dev, (double *)out_moments_dev,
                    (int *)out_count_dev, (hipStream_t)stream)))
    return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

// the host form: one device allocation holds the tables, the inputs and the outputs
extern "C" int pt_rays_gradient_accumulate(int device, int width, int height, const pt_gradient_history *params, const pt_gradient_camera *prev_camera,
                                           const double *colour_host, const int *samples_host, const int *shape_host, const double *normal_host,
                                           const double *point_host, const double *prev_colour_host, const double *prev_moments_host,
                                           const int *prev_shape_host, const double *prev_normal_host, const double *prev_point_host,
                                           const int *prev_count_host, int n_shapes, const int *moved_host, const double *motion_host,
                                           const double *keep_host, void *out_colour_host, size_t out_colour_bytes, void *out_moments_host,
                                           size_t out_moments_bytes, void *out_count_host, size_t out_count_bytes) {
  long long m, max_blocks;
  const GrPlanes in = {colour_host,      samples_host,    shape_host,      normal_host, point_host, prev_colour_host, prev_moments_host, prev_shape_host,
                       prev_normal_host, prev_point_host, prev_count_host, n_shapes,    moved_host, motion_host,      keep_host};
  const GrOuts out = {out_colour_host, out_colour_bytes, out_moments_host, out_moments_bytes, out_count_host, out_count_bytes};
  int rc = check_all(device, width, height, params, prev_camera, in, out, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(max_blocks))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b3 = (size_t)m * 24, b2 = (size_t)m * 8, b1 = up8((size_t)m * 4);
  const size_t tb = (size_t)n_shapes * 192, fb = up8((size_t)n_shapes * 4);
  Staged s;
  if ((rc = s.alloc(tb + fb + 9 * b3 + b2 + 5 * b1))) return rc;
  // the motion table first (its records on 64-byte boundaries), the moved words, then nine [3, m] planes (the last two are
  // outputs), the keep plane and five int planes (the last is the output; the fourth holds `samples`)
  char *dt = s.dev, *df = s.dev + tb, *base = s.dev + tb + fb;
  char *d3[9], *d1[5];
  for (int i = 0; i < 9; i++) d3[i] = base + i * b3;
  char *dk = base + 9 * b3;
  for (int i = 0; i < 5; i++) d1[i] = dk + b2 + i * b1;
  const double *h3[7] = {colour_host, normal_host, point_host, prev_colour_host, prev_moments_host, prev_normal_host, prev_point_host};
  const int *h1[4] = {shape_host, prev_shape_host, prev_count_host, samples_host};
  if (n_shapes > 0) {
    HIP_TRY(hipMemcpy(dt, motion_host, tb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(df, moved_host, (size_t)n_shapes * 4, hipMemcpyHostToDevice));
  }
  for (int i = 0; i < 7; i++) HIP_TRY(hipMemcpy(d3[i], h3[i], b3, hipMemcpyHostToDevice));
  if (keep_host) HIP_TRY(hipMemcpy(dk, keep_host, b2, hipMemcpyHostToDevice));
  for (int i = 0; i < 4; i++)
    if (h1[i]) HIP_TRY(hipMemcpy(d1[i], h1[i], (size_t)m * 4, hipMemcpyHostToDevice));
  const GrPlanes dev = {(const double *)d3[0], samples_host ? (const int *)d1[3] : nullptr,
                        (const int *)d1[0],    (const double *)d3[1],
                        (const double *)d3[2], (const double *)d3[3],
                        (const double *)d3[4], (const int *)d1[1],
                        (const double *)d3[5], (const double *)d3[6],
                        (const int *)d1[2],    n_shapes,
                        n_shapes > 0 ? (const int *)df : nullptr, n_shapes > 0 ? (const double *)dt : nullptr,
                        keep_host ? (const double *)dk : nullptr};
  if ((rc = enqueue(max_blocks, width, height, *params, *prev_camera, m, dev, (double *)d3[7], (double *)d3[8], (int *)d1[4], nullptr))) return rc;
  HIP_TRY(hipMemcpy(out_colour_host, d3[7], b3, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  HIP_TRY(hipMemcpy(out_moments_host, d3[8], b3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_count_host, d1[4], (size_t)m * 4, hipMemcpyDeviceToHost));
  return PT_OK;
}
