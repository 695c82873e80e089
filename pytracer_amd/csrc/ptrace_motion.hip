// ptrace_motion.hip — libptrace_motion.so: the C-ABI of include/ptrace_motion.h, the weighted accumulation over frames with a motion
// per shape: a record whose shape moved is carried into the previous frame's world before it is projected and tested.
//
// The kernel is pt_motion.h's.  Why a fifteenth translation unit and a fifteenth shared object: libptrace.so's device code is
// pinned by build.code_hash, and the exported symbols of the fourteen libraries beside it are pinned to their interfaces'.  So this
// library stands beside them: no link dependency, nothing is loaded from here, and no scene is read.
//
// A launch alternative, for the tests that no bit depends on it (read per call):
//     PTRACE_MA_BLOCKS = N              at most N workgroups (the kernel walks a grid-stride loop)
// Any other value is refused with PT_ERR_INVALID.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ptrace_motion.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_motion.h"
#include "pt_host_common.h"

#define PT_MA_VERSION ((1 << 16) | 13)
#define PT_MA_MAX_M 2147483647LL
#define PT_MA_MAX_GRID 2147483647LL

static_assert(PT_MA_FLAG_SAME_SHAPE == PT_MA_SAME_SHAPE && PT_MA_FLAG_BLEND_WEIGHT == PT_MA_BLEND_WEIGHT, "the kernel's flag bits are the header's");
static_assert(sizeof(pt_motion_params) == 32 && sizeof(pt_motion_camera) == 120, "the structs of the header");
static_assert(PT_MA_RECORD_DOUBLES == PT_MA_RECORD && PT_MA_RECORD * sizeof(double) == 192, "a table record of the header: 192 bytes");

extern "C" int pt_rays_motion_version(void) { return PT_MA_VERSION; }

extern "C" int pt_rays_motion_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

// ---- sizes and checks: every argument, before any HIP call ---------------------------------------------------------------------
extern "C" size_t pt_rays_motion_bytes(long long m) { return (m >= 0 && m <= PT_MA_MAX_M) ? (size_t)m * 24 : 0; }

extern "C" size_t pt_rays_motion_count_bytes(long long m) { return (m >= 0 && m <= PT_MA_MAX_M) ? (size_t)m * 4 : 0; }

extern "C" size_t pt_rays_motion_table_bytes(int n_shapes) { return (n_shapes >= 0 && n_shapes <= PT_MA_MAX_SHAPES) ? (size_t)n_shapes * 192 : 0; }

static int check_frame(int width, int height, const pt_motion_params *p, const pt_motion_camera *cam, int n_shapes, long long &m) {
  m = 0;
  if (width < 0 || height < 0) return fail(PT_ERR_INVALID, "frame of %d x %d records", width, height);
  if ((long long)width * height > PT_MA_MAX_M) return fail(PT_ERR_INVALID, "record count %d x %d outside [0, 2^31 - 1]", width, height);
  if (!p) return fail(PT_ERR_INVALID, "null pt_motion_params");
  if (!cam) return fail(PT_ERR_INVALID, "null pt_motion_camera");
  if (p->max_history < 1 || p->max_history > PT_MA_MAX_HISTORY) return fail(PT_ERR_INVALID, "max_history = %d: 1 to 2^20", p->max_history);
  if (p->flags & ~(PT_MA_SAME_SHAPE | PT_MA_BLEND_WEIGHT)) return fail(PT_ERR_INVALID, "unknown flag bits in 0x%x", (unsigned)p->flags);
  if (!(p->normal_min >= -1.0 && p->normal_min <= 1.0)) return fail(PT_ERR_INVALID, "normal_min = %g: a cosine, -1 to 1", p->normal_min);
  if (!(p->point_tolerance > 0.0)) return fail(PT_ERR_INVALID, "point_tolerance = %g: positive (or +inf)", p->point_tolerance);
  if (!(p->max_weight >= 0.0)) return fail(PT_ERR_INVALID, "max_weight = %g: not negative (or +inf)", p->max_weight);
  if (cam->kind != PT_CAMERA_ORTHOGONAL && cam->kind != PT_CAMERA_PERSPECTIVE) return fail(PT_ERR_INVALID, "unknown camera kind %d", cam->kind);
  if (n_shapes < 0 || n_shapes > PT_MA_MAX_SHAPES) return fail(PT_ERR_INVALID, "n_shapes = %d: 0 to 2^20", n_shapes);
  m = (long long)width * height;
  return PT_OK;
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

struct MaPlanes {
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
};

struct MaOuts {
  void *colour;
  size_t colour_bytes;
  void *moments;
  size_t moments_bytes;
  void *count;
  size_t count_bytes;
};

static int check_all(int device, int width, int height, const pt_motion_params *p, const pt_motion_camera *cam, const MaPlanes &in,
                     const MaOuts &out, long long &m) {
  if (int rc = check_frame(width, height, p, cam, in.n_shapes, m)) return rc;
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (m == 0) return PT_OK;
  if (!in.colour || !in.shape || !in.normal || !in.point) return fail(PT_ERR_INVALID, "null colour, shape, normal or point planes");
  if (!in.prev_colour || !in.prev_moments || !in.prev_shape || !in.prev_normal || !in.prev_point || !in.prev_count)
    return fail(PT_ERR_INVALID, "null previous colour, moments, shape, normal, point or count planes");
  if (in.n_shapes > 0 && (!in.moved || !in.motion)) return fail(PT_ERR_INVALID, "null moved or motion table for %d shapes", in.n_shapes);
  if (!out.colour || !out.moments || !out.count) return fail(PT_ERR_INVALID, "null output buffer");
  const size_t b3 = (size_t)m * 24, b1 = (size_t)m * 4;
  const struct {
    const void *at;
    size_t bytes;
    const char *name;
  } outs[3] = {{out.colour, b3, "colour"}, {out.moments, b3, "moments"}, {out.count, b1, "count"}},
    reads[10] = {{in.colour, b3, "the colour planes"},
                 {in.samples, in.samples ? b1 : 0, "the sample counts"},
                 {in.prev_colour, b3, "the previous colour planes"},
                 {in.prev_moments, b3, "the previous moments"},
                 {in.prev_shape, b1, "the previous shapes"},
                 {in.prev_normal, b3, "the previous normals"},
                 {in.prev_point, b3, "the previous points"},
                 {in.prev_count, b1, "the previous counts"},
                 {in.moved, (size_t)in.n_shapes * 4, "the moved table"},
                 {in.motion, (size_t)in.n_shapes * 192, "the motion table"}};
  for (const auto &o : outs)
    for (const auto &r : reads)
      if (r.bytes && overlap(o.at, o.bytes, r.at, r.bytes))
        return fail(PT_ERR_INVALID, "the %s output overlaps %s: a tap reads its neighbours' history (ping-pong two buffers)", o.name, r.name);
  for (int i = 0; i < 3; i++)
    for (int j = i + 1; j < 3; j++)
      if (overlap(outs[i].at, outs[i].bytes, outs[j].at, outs[j].bytes))
        return fail(PT_ERR_INVALID, "the %s output overlaps the %s output", outs[i].name, outs[j].name);
  if (out.colour_bytes < b3) return fail(PT_ERR_SIZE, "colour output too small: %zu < %zu bytes", out.colour_bytes, b3);
  if (out.moments_bytes < b3) return fail(PT_ERR_SIZE, "moments output too small: %zu < %zu bytes", out.moments_bytes, b3);
  if (out.count_bytes < b1) return fail(PT_ERR_SIZE, "count output too small: %zu < %zu bytes", out.count_bytes, b1);
  return PT_OK;
}

// ---- the launch alternative -----------------------------------------------------------------------------------------------------
static int launch_choice(long long &max_blocks) {
  max_blocks = PT_MA_MAX_GRID;
  if (const char *v = getenv("PTRACE_MA_BLOCKS")) {
    char *end = nullptr;
    const long long n = strtoll(v, &end, 10);
    if (end == v || *end || n < 1) return fail(PT_ERR_INVALID, "PTRACE_MA_BLOCKS=%s: a positive count of workgroups", v);
    max_blocks = std::min(n, PT_MA_MAX_GRID);
  }
  return PT_OK;
}

static int enqueue(long long max_blocks, int width, int height, const pt_motion_params &p, const pt_motion_camera &cam, long long m,
                   const MaPlanes &in, double *out_colour, double *out_moments, int *out_count, hipStream_t st) {
  PtMaK K;
  K.W = width, K.H = height, K.m = m, K.max_history = p.max_history, K.flags = p.flags;
  K.persp = cam.kind == PT_CAMERA_PERSPECTIVE;
  K.n_shapes = (in.moved && in.motion) ? in.n_shapes : 0;
  K.normal_min = p.normal_min, K.point_tolerance = p.point_tolerance, K.max_weight = p.max_weight;
  for (int i = 0; i < 12; i++) K.invm[i] = cam.invm[i];
  K.d = cam.screen_distance, K.a = cam.aspect_ratio;
  const long long flat = (m + PT_BLOCK - 1) / PT_BLOCK;
  hipLaunchKernelGGL(pt_ma_accumulate_kernel, dim3((unsigned)std::min(flat, max_blocks)), dim3(PT_BLOCK), 0, st, K, in.colour, in.samples, in.shape,
                     in.normal, in.point, in.prev_colour, in.prev_moments, in.prev_shape, in.prev_normal, in.prev_point, in.prev_count, in.moved,
                     in.motion, out_colour, out_moments, out_count);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

// ---- an empty history -------------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_motion_clear_device(int device, long long m, void *count_dev, size_t count_bytes, void *stream) {
  if (m < 0 || m > PT_MA_MAX_M) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", m);
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

// ---- the device form ------------------------------------------------------------------------------------------------------------
extern "C" int pt_rays_motion_accumulate_device(int device, int width, int height, const pt_motion_params *params,
                                                const pt_motion_camera *prev_camera, const double *colour_dev, const int *samples_dev,
                                                const int *shape_dev, const double *normal_dev, const double *point_dev,
                                                const double *prev_colour_dev, const double *prev_moments_dev, const int *prev_shape_dev,
                                                const double *prev_normal_dev, const double *prev_point_dev, const int *prev_count_dev,
                                                int n_shapes, const int *moved_dev, const double *motion_dev, void *out_colour_dev,
                                                size_t out_colour_bytes, void *out_moments_dev, size_t out_moments_bytes, void *out_count_dev,
                                                size_t out_count_bytes, void *stream) {
  long long m, max_blocks;
  const MaPlanes in = {colour_dev,     samples_dev,     shape_dev,      normal_dev,     point_dev, prev_colour_dev, prev_moments_dev,
                       prev_shape_dev, prev_normal_dev, prev_point_dev, prev_count_dev, n_shapes,  moved_dev,       motion_dev};
  const MaOuts out = {out_colour_dev, out_colour_bytes, out_moments_dev, out_moments_bytes, out_count_dev, out_count_bytes};
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

// ---- the host form: one device allocation holds the tables, the inputs and the outputs --------------------------------------------
extern "C" int pt_rays_motion_accumulate(int device, int width, int height, const pt_motion_params *params, const pt_motion_camera *prev_camera,
                                         const double *colour_host, const int *samples_host, const int *shape_host, const double *normal_host,
                                         const double *point_host, const double *prev_colour_host, const double *prev_moments_host,
                                         const int *prev_shape_host, const double *prev_normal_host, const double *prev_point_host,
                                         const int *prev_count_host, int n_shapes, const int *moved_host, const double *motion_host,
                                         void *out_colour_host, size_t out_colour_bytes, void *out_moments_host, size_t out_moments_bytes,
                                         void *out_count_host, size_t out_count_bytes) {
  long long m, max_blocks;
  const MaPlanes in = {colour_host,     samples_host,     shape_host,      normal_host,     point_host, prev_colour_host, prev_moments_host,
                       prev_shape_host, prev_normal_host, prev_point_host, prev_count_host, n_shapes,   moved_host,       motion_host};
  const MaOuts out = {out_colour_host, out_colour_bytes, out_moments_host, out_moments_bytes, out_count_host, out_count_bytes};
  int rc = check_all(device, width, height, params, prev_camera, in, out, m);
  if (rc || m == 0) return rc;
  if ((rc = launch_choice(max_blocks))) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t b3 = (size_t)m * 24, b1 = up8((size_t)m * 4);
  const size_t tb = (size_t)n_shapes * 192, fb = up8((size_t)n_shapes * 4);
  Staged s;
  if ((rc = s.alloc(tb + fb + 9 * b3 + 5 * b1))) return rc;
  // the motion table first (its records on 64-byte boundaries), the moved words, then nine [3, m] planes (the last two are
  // outputs) and five int planes (the last is the output; the fourth holds `samples`)
  char *dt = s.dev, *df = s.dev + tb, *base = s.dev + tb + fb;
  char *d3[9], *d1[5];
  for (int i = 0; i < 9; i++) d3[i] = base + i * b3;
  for (int i = 0; i < 5; i++) d1[i] = base + 9 * b3 + i * b1;
  const double *h3[7] = {colour_host, normal_host, point_host, prev_colour_host, prev_moments_host, prev_normal_host, prev_point_host};
  const int *h1[4] = {shape_host, prev_shape_host, prev_count_host, samples_host};
  if (n_shapes > 0) {
    HIP_TRY(hipMemcpy(dt, motion_host, tb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(df, moved_host, (size_t)n_shapes * 4, hipMemcpyHostToDevice));
  }
  for (int i = 0; i < 7; i++) HIP_TRY(hipMemcpy(d3[i], h3[i], b3, hipMemcpyHostToDevice));
  for (int i = 0; i < 4; i++)
    if (h1[i]) HIP_TRY(hipMemcpy(d1[i], h1[i], (size_t)m * 4, hipMemcpyHostToDevice));
  const MaPlanes dev = {(const double *)d3[0], samples_host ? (const int *)d1[3] : nullptr, (const int *)d1[0],    (const double *)d3[1],
                        (const double *)d3[2], (const double *)d3[3],                       (const double *)d3[4], (const int *)d1[1],
                        (const double *)d3[5], (const double *)d3[6],                       (const int *)d1[2],    n_shapes,
                        n_shapes > 0 ? (const int *)df : nullptr,                           n_shapes > 0 ? (const double *)dt : nullptr};
  if ((rc = enqueue(max_blocks, width, height, *params, *prev_camera, m, dev, (double *)d3[7], (double *)d3[8], (int *)d1[4], nullptr))) return rc;
  HIP_TRY(hipMemcpy(out_colour_host, d3[7], b3, hipMemcpyDeviceToHost));  // (the null stream: behind the kernel)
  HIP_TRY(hipMemcpy(out_moments_host, d3[8], b3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_count_host, d1[4], (size_t)m * 4, hipMemcpyDeviceToHost));
  return PT_OK;
}
