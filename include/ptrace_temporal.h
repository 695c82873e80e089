/* ptrace_temporal.h — C-ABI of libptrace_temporal.so: last frame's radiance reprojected onto this frame's hits, on the device.
 *
 * Interface 1.9 of the ray library, its eleventh step: an ACCUMULATE QUERY, the companion of the tenth (accumulate, then filter).
 * Where the filter of ptrace_denoise.h trades rays for space, this step trades them for time.  What is carried from frame to frame
 * is the DEMODULATED signal (E of the gather and bake queries: the diffuse hemisphere mean at a surface point), which does not
 * depend on the viewer, so reprojection adds no view-dependent error.
 *
 * Only + - * / sqrt floor and comparisons occur, in fp64, every operation rounded on its own (no contraction), so that
 * pytracer_amd.rays.temporal_host matches the device bit for bit.  The literals and the order below define the bits.
 *
 * FRAMES   W x H records, row-major: record r = y * W + x, m = W * H; the current and the previous frame have this size.
 *     current:   `colour` [3, m] fp64 (this frame's noisy E), `shape` int32[m] (negative = no record), `normal` [3, m] (NOT unit
 *                length), `point` [3, m]
 *     previous:  `prev_colour`, `prev_shape`, `prev_normal`, `prev_point` (the same planes) and `prev_count` int32[m], the history
 *                length (<= 0: nothing to reuse)
 *     outputs:   `out_colour` [3, m] fp64, `out_count` int32[m]
 *
 * PIXEL p = (x, y), with nh(a) = a / sqrt(a.x * a.x + a.y * a.y + a.z * a.z) and every dot product summed from x to z:
 *   1. shape[p] < 0:  out = colour[p] bit for bit, out_count = 0.
 *   2. q = invm * point_p, each row as ((m0 * px + m1 * py) + m2 * pz) + m3        (the PREVIOUS camera's frame)
 *   3. onto the previous screen; "not tn > 0" means NO HISTORY:
 *        perspective:  tn = q.x + d;    s = d / tn;  u = (1.0 - (q.y * s) / a) * 0.5;  v = (1.0 + q.z * s) * 0.5
 *        orthogonal:   tn = q.x + 1.0;               u = (1.0 - q.y / a) * 0.5;        v = (1.0 + q.z) * 0.5
 *      (d = screen_distance, a = aspect_ratio)
 *   4. fx = u * (double)W - 0.5;  fy = (1.0 - v) * (double)H - 0.5               (the inverse of a primary ray at a pixel centre)
 *   5. unless fx > -1 && fx < W && fy > -1 && fy < H:  NO HISTORY                (this is where NaN dies)
 *   6. x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0
 *   7. four taps in the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with the weights
 *        b = (1 - ax) * (1 - ay),  ax * (1 - ay),  (1 - ax) * ay,  ax * ay
 *   8. a tap r is SKIPPED if it lies outside the frame; if prev_count[r] <= 0; if prev_shape[r] < 0; under PT_TA_SAME_SHAPE if
 *      prev_shape[r] != shape[p]; unless c >= normal_min, c = nh(n_p) . nh(prev_n_r); unless fabs(dz) <= point_tolerance,
 *      dz = nh(n_p) . (prev_point_r - point_p); unless b > 0
 *   9. sums from +0.0 in tap order:  hs[ch] = hs[ch] + b * prev_colour_r[ch],  ws = ws + b;  nmax = the largest prev_count of
 *      the accepted taps
 *  10. no tap accepted, or NO HISTORY:  out = colour[p] bit for bit, out_count = 1
 *  11. else  hist = hs / ws;  n = min(nmax + 1, max_history);  alpha = 1.0 / (double)n;
 *            out[ch] = hist[ch] + (colour[ch] - hist[ch]) * alpha;  out_count = n
 * A running mean until max_history, an exponential average from then on.
 *
 * NON-FINITE COLOURS are not an error and propagate as the arithmetic says.  Non-finite guides only ever skip taps.
 *
 * AN ELEVENTH shared object, for the reasons the ten before it give.  It links to none of the others, loads nothing and reads no
 * scene.
 *
 * LAUNCHES  pt_rays_temporal_accumulate_device allocates nothing, makes ONE launch and is asynchronous on the caller's stream (a
 * hipStream_t; NULL: the default stream, and the call returns when the work is done).  No bit depends on the launch shape.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never throws,
 * and checks every argument before its first HIP call:
 *     width or height < 0; width * height > 2^31 - 1; a NULL struct; max_history outside 1 .. 2^20; unknown flag bits;
 *     normal_min outside [-1, 1] (NaN included); a point_tolerance that is not > 0 (+inf is legal and switches the test off); an
 *     unknown camera kind; NULL where a buffer is needed; either output overlapping the other, any previous plane or `colour`
 *     (a tap reads its neighbours' history: the history ping-pongs)                                        PT_ERR_INVALID
 *     an output that is too small                                                                          PT_ERR_SIZE
 * m = 0 is PT_OK with nothing launched (the structs are still checked).  pt_rays_temporal_accumulate takes host buffers, stages
 * them through device memory it allocates and frees, and is synchronous.
 */
#ifndef PTRACE_TEMPORAL_H
#define PTRACE_TEMPORAL_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_*, PT_CAMERA_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_TA_SAME_SHAPE 1 /* a tap on another shape is skipped (default: on) */

#define PT_TA_MAX_HISTORY 1048576 /* 2^20 */

typedef struct pt_temporal_params {
  int max_history;        /* 1 .. 2^20 (default 32): the running mean becomes an exponential average there      */
  int flags;              /* PT_TA_* bits                                                                       */
  double normal_min;      /* in [-1, 1] (default 0.9): the least cosine between the unit normals                */
  double point_tolerance; /* > 0 or +inf (default 0.05): the largest distance from the pixel's tangent plane    */
} pt_temporal_params;

/* The camera the PREVIOUS frame was seen from. */
typedef struct pt_temporal_camera {
  int kind;               /* PT_CAMERA_* of ptrace.h                                  */
  double invm[12];        /* rows 0..2 of camera.transformation.invm (world -> camera) */
  double screen_distance; /* perspective only                                         */
  double aspect_ratio;
} pt_temporal_camera;

/* (major << 16) | minor of the ray library's interface this library implements: 1.9. */
int pt_rays_temporal_version(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_temporal_last_error(char *buf, size_t n);

/* Bytes of an accumulated frame of m records: 24 m (0 on refusal). */
size_t pt_rays_temporal_bytes(long long m);
/* Bytes of its history lengths: 4 m (0 on refusal). */
size_t pt_rays_temporal_count_bytes(long long m);

/* A history that holds nothing: the m lengths at count_dev become 0, on the caller's stream (the start of a sequence, whose first
 * frame then takes the path of every other; the library has no other way to write a plane it does not compute).  Refuses m outside
 * [0, 2^31 - 1] and a NULL buffer (PT_ERR_INVALID) and a buffer below 4 m bytes (PT_ERR_SIZE); m = 0 is PT_OK. */
int pt_rays_temporal_clear_device(int device, long long m, void *count_dev, size_t count_bytes, void *stream);

int pt_rays_temporal_accumulate_device(int device, int width, int height, const pt_temporal_params *params,
                                       const pt_temporal_camera *prev_camera, const double *colour_dev, const int *shape_dev,
                                       const double *normal_dev, const double *point_dev, const double *prev_colour_dev,
                                       const int *prev_shape_dev, const double *prev_normal_dev, const double *prev_point_dev,
                                       const int *prev_count_dev, void *out_colour_dev, size_t out_colour_bytes, void *out_count_dev,
                                       size_t out_count_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_temporal_accumulate(int device, int width, int height, const pt_temporal_params *params, const pt_temporal_camera *prev_camera,
                                const double *colour_host, const int *shape_host, const double *normal_host, const double *point_host,
                                const double *prev_colour_host, const int *prev_shape_host, const double *prev_normal_host,
                                const double *prev_point_host, const int *prev_count_host, void *out_colour_host, size_t out_colour_bytes,
                                void *out_count_host, size_t out_count_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_TEMPORAL_H */
