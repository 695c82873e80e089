/* ptrace_gradient.h — C-ABI of libptrace_gradient.so: temporal gradients for the accumulation of ptrace_motion.h, so that a history
 * shortens where the LIGHT changed, on the device.
 *
 * Interface 1.14 of the ray library, its sixteenth step: a GRADIENT ACCUMULATE QUERY, in the spirit of A-SVGF's temporal gradients.
 * Steps eleven to fifteen reuse last frame's E wherever the geometry tests let a tap through; none asks whether the light at that
 * place is still the same.  A shadow that moved, or a reflection of a shape that did, averages up to max_history frames of a world
 * that no longer exists.  This step measures, at a sparse set of this frame's pixels (PROBES, one per stratum of s x s pixels), how
 * much E changed because the WORLD changed, free of sampling noise, and cuts the history's weight where it did (KEEP, ACCUMULATE).
 * It can be exact because a gather is a pure function of (world, point, normal, stream numbers): the same record with the same PCG
 * streams, gathered in the PREVIOUS world, differs from this frame's value only by what moved; in a static world every bit of the
 * difference is zero.
 *
 * THE CHAIN of a frame, every plane [3, m] or [m] over the frame's m = width * height records in frame order:
 *     this frame's hit records and its gather E (uniform: K samples per record, seq_i = init_seq + i * K)
 *  1. PROBES     -> probe_index int32[ns], probe_point [3, ns], probe_normal [3, ns], probe_seq uint64[ns]
 *     the caller gathers those four planes (points, normals, active = index >= 0, seq) IN THE PREVIOUS FRAME'S SCENE with this
 *     frame's K, init_state and path parameters (the gather query of ptrace_gather.h, which this library does not call)
 *                -> probe_old [3, ns]
 *  2. KEEP       -> keep double[m], in [0, 1]: 1 where nothing changed
 *  3. ACCUMULATE -> the three outputs of ptrace_motion.h, the history's weight and length multiplied by keep.
 *
 * 1. PROBES.  The frame is cut into ns = ceil(W / s) * ceil(H / s) strata, row-major; stratum j at (sx, sy) = (j % gw, j / gw):
 *     sw = min(s, W - sx * s),  sh = min(s, H - sy * s)
 *     in uint64 arithmetic mod 2^64:
 *       x = phase * 0x9E3779B97F4A7C15 + j * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D
 *       x ^= x >> 32;  x *= 0xD6E8FEB86659FD93;  x ^= x >> 32;  x *= 0xD6E8FEB86659FD93;  x ^= x >> 32
 *       ox = (x & 0xffff) % sw,  oy = ((x >> 16) & 0xffff) % sh
 *     r = (sy * s + oy) * W + sx * s + ox
 *     shape[r] < 0:  probe_index = -1, the point, the normal and the seq are +0.0 / 0
 *     otherwise:     probe_index = r,  probe_seq = init_seq + r * K (mod 2^64),  and the point and the normal are the record's carried
 *                    into the previous world by step 1 of ptrace_motion.h (pm, nm: each row as ((a0 * px + a1 * py) + a2 * pz) + a3
 *                    and (n0 * nx + n1 * ny) + n2 * nz); for a shape that did not move, or that lies outside the table, they are
 *                    the record's bits unchanged and NO table entry is read.
 *    The tables n_shapes, moved int32[n_shapes] and motion double[n_shapes][24] are those of ptrace_motion.h (NULL / 0: nothing moved).
 *
 * 2. KEEP.  Pixel p = (x, y):
 *     shape[p] < 0:  keep = 1.0
 *     otherwise num and den are summed from +0.0 over the strata (x / s + dx, y / s + dy), dy then dx from -radius to radius in that
 *     order.  A stratum outside the grid is skipped.  A stratum with q = probe_index[j] outside [0, m) is skipped and NO read happens
 *     at such an index: these are records nobody vouches for.  Under PT_GR_SAME_SHAPE a stratum with shape[q] != shape[p] is skipped.
 *     For the others
 *       lc = lum(colour[q]),  lo = lum(probe_old[j])      lum(c) = (max(c0, c1, c2) + min(c0, c1, c2)) / 2.0, with comparisons
 *       d = lc - lo;  if (d < 0.0) d = 0.0 - d;
 *       mx = lc > lo ? lc : lo
 *       num = num + d;  den = den + mx
 *     lam = gain * (num / den);  if (!(lam > 0.0)) lam = 0.0;  if (lam > 1.0) lam = 1.0;  keep = 1.0 - lam
 *    0 / 0, NaN and no accepted stratum all end in keep = 1.0.
 *
 * 3. ACCUMULATE.  Steps 0 to 5 of ptrace_motion.h and ptrace_weighted.h EXACTLY, with one insertion in step 5 after the two clamps
 *    of Sh, and only when `keep` is not NULL:
 *       kp = keep[p];  if (!(kp >= 0.0)) kp = 0.0;  if (kp > 1.0) kp = 1.0;  Sh = kp * Sh;  nmax = (int)floor(kp * (double)nmax);
 *    Both the k > 0 branch and the k <= 0 branch then use these.  The text of those two headers is the specification of all that
 *    is not restated here.
 *
 * Only + - * / sqrt floor, comparisons and integer arithmetic occur, in fp64, every operation rounded on its own (no contraction),
 * in the order above, so that pytracer_amd.rays.gradient_probes_host, gradient_keep_host and gradient_accumulate_host match the
 * device bit for bit.
 *
 * THREE CONTRACTS that come from the arithmetic:
 *   E. NOTHING KEPT BACK, NOTHING CHANGES.  With `keep` NULL, or 1.0 everywhere, all three outputs are bit for bit those of the motion
 *      accumulate query, since 1.0 * Sh and floor(1.0 * n) are exact.  Contracts A to D of the earlier headers therefore hold here too.
 *   F. NOTHING KEPT, THE HISTORY IS ONE FRAME.  With `keep` 0.0 everywhere, every record that has k > 0 and an accepted tap has
 *      out_count == 1, S == kd and the colour hist + (c - hist) * 1.0.  (A history weight of +inf, which max_weight = +inf lets
 *      through, makes 0 * inf = NaN of S and the colour; the length is 1 all the same.)
 *   G. A STATIC WORLD KEEPS EVERYTHING.  If probe_old holds, for every probe, the bits of `colour` at that probe's pixel, keep is 1.0
 *      everywhere; gathering the probes in an unchanged world gives exactly those bits.  So through E the whole chain is the motion
 *      query, for any gain, stratum and radius.
 *
 * WHAT IT DOES NOT COVER.  A probe's streams need seq = init_seq + r * K: adaptive and ragged sample counts stay out.  A shape that
 * ROTATES gives its probes a turned normal and hence other sample directions: that gradient contains sampling noise.  Translations
 * leave the normal's bits alone and are exact.
 *
 * A SIXTEENTH shared object, for the reasons the fifteen before it give.  It links to none of the others, loads nothing and reads
 * no scene.
 *
 * LAUNCHES  every _device entry point allocates nothing, makes ONE launch and is asynchronous on the caller's stream (a hipStream_t;
 * NULL: the default stream, and the call returns when the work is done).  No bit depends on the launch shape.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never throws,
 * and checks every argument before its first HIP call.  Refused with PT_ERR_INVALID: a negative width or height, more than
 * 2^31 - 1 records, a negative device, a NULL struct or plane, n_shapes outside [0, 2^20], n_shapes > 0 with a NULL table, a stratum
 * outside 1..16, a radius outside 0..4, K < 1, unknown flag bits, a gain that is negative or NaN, the parameters ptrace_motion.h
 * refuses, and an output that overlaps another output or anything the call reads.  An output too small: PT_ERR_SIZE, each with its
 * own message.  m = 0 is PT_OK with nothing launched (the structs and scalars are still checked).  The forms without _device take
 * host buffers, stage them through device memory they allocate and free, and are synchronous.
 */
#ifndef PTRACE_GRADIENT_H
#define PTRACE_GRADIENT_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_*, PT_CAMERA_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_GR_SAME_SHAPE 1   /* keep: a probe on another shape is skipped; accumulate: a tap on another shape is skipped (default: on) */
#define PT_GR_BLEND_WEIGHT 2 /* accumulate only: the history's weight is the taps' blend hS / ws, not their largest (smax)            */

#define PT_GR_MAX_HISTORY 1048576 /* 2^20 */
#define PT_GR_MAX_SHAPES 1048576  /* 2^20 */
#define PT_GR_RECORD 24           /* doubles per shape in `motion`: 192 bytes */
#define PT_GR_MAX_STRATUM 16
#define PT_GR_MAX_RADIUS 4

typedef struct pt_gradient_params {
  int stratum; /* 1 .. 16 (default 3): the side of a stratum, in pixels                              */
  int radius;  /* 0 .. 4 (default 1): the window of KEEP is (2 radius + 1)^2 strata                  */
  int flags;   /* PT_GR_SAME_SHAPE                                                                   */
  double gain; /* >= 0 or +inf (default 8): how much of the history a relative change of 1 takes away */
} pt_gradient_params;

/* The layout of the params struct of ptrace_motion.h. */
typedef struct pt_gradient_history {
  int max_history;        /* 1 .. 2^20 (default 32): the cap of the history LENGTH out_count                     */
  int flags;              /* PT_GR_* bits                                                                       */
  double normal_min;      /* in [-1, 1] (default 0.9): the least cosine between the unit normals                */
  double point_tolerance; /* > 0 or +inf (default 0.05): the largest distance from the pixel's tangent plane    */
  double max_weight;      /* >= 0 or +inf (default 128): the cap of the history's WEIGHT before this frame's is added */
} pt_gradient_history;

/* The camera the PREVIOUS frame was seen from: the layout of the camera struct of ptrace_motion.h. */
typedef struct pt_gradient_camera {
  int kind;               /* PT_CAMERA_* of ptrace.h                                  */
  double invm[12];        /* rows 0..2 of camera.transformation.invm (world -> camera) */
  double screen_distance; /* perspective only                                         */
  double aspect_ratio;
} pt_gradient_camera;

/* (major << 16) | minor of the ray library's interface this library implements: 1.14. */
int pt_rays_gradient_version(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_gradient_last_error(char *buf, size_t n);

/* The number of strata, hence of probes, of a frame: ceil(width / stratum) * ceil(height / stratum) (0 on refusal, and for an empty frame). */
long long pt_rays_gradient_strata(int width, int height, int stratum);
/* Bytes of the keep plane of m records: 8 m (0 on refusal). */
size_t pt_rays_gradient_keep_bytes(long long m);
/* Bytes of an accumulated frame of m records, and of its moments frame: 24 m (0 on refusal). */
size_t pt_rays_gradient_bytes(long long m);
/* Bytes of its history lengths: 4 m (0 on refusal). */
size_t pt_rays_gradient_count_bytes(long long m);
/* Bytes of the `motion` table of n_shapes shapes: 192 n_shapes (0 on refusal: n_shapes outside [0, 2^20]). */
size_t pt_rays_gradient_table_bytes(int n_shapes);

/* A history that holds nothing: the m lengths at count_dev become 0, on the caller's stream.  Refuses m outside [0, 2^31 - 1] and
 * a NULL buffer (PT_ERR_INVALID) and a buffer below 4 m bytes (PT_ERR_SIZE); m = 0 is PT_OK. */
int pt_rays_gradient_clear_device(int device, long long m, void *count_dev, size_t count_bytes, void *stream);

/* 1. The probes of a frame.  Outputs: 4 ns, 24 ns, 24 ns and 8 ns bytes. */
int pt_rays_gradient_probes_device(int device, int width, int height, int stratum, unsigned long long phase, int samples,
                                   unsigned long long init_seq, const int *shape_dev, const double *normal_dev, const double *point_dev,
                                   int n_shapes, const int *moved_dev, const double *motion_dev, void *probe_index_dev, size_t probe_index_bytes,
                                   void *probe_point_dev, size_t probe_point_bytes, void *probe_normal_dev, size_t probe_normal_bytes,
                                   void *probe_seq_dev, size_t probe_seq_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_gradient_probes(int device, int width, int height, int stratum, unsigned long long phase, int samples, unsigned long long init_seq,
                            const int *shape_host, const double *normal_host, const double *point_host, int n_shapes, const int *moved_host,
                            const double *motion_host, void *probe_index_host, size_t probe_index_bytes, void *probe_point_host,
                            size_t probe_point_bytes, void *probe_normal_host, size_t probe_normal_bytes, void *probe_seq_host,
                            size_t probe_seq_bytes);

/* 2. How much of the history every pixel keeps.  Output: 8 m bytes. */
int pt_rays_gradient_keep_device(int device, int width, int height, const pt_gradient_params *params, const double *colour_dev,
                                 const int *shape_dev, const int *probe_index_dev, const double *probe_old_dev, void *keep_dev, size_t keep_bytes,
                                 void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_gradient_keep(int device, int width, int height, const pt_gradient_params *params, const double *colour_host, const int *shape_host,
                          const int *probe_index_host, const double *probe_old_host, void *keep_host, size_t keep_bytes);

/* 3. The accumulation of ptrace_motion.h with one more plane, `keep` double[m], or NULL. */
int pt_rays_gradient_accumulate_device(int device, int width, int height, const pt_gradient_history *params, const pt_gradient_camera *prev_camera,
                                       const double *colour_dev, const int *samples_dev, const int *shape_dev, const double *normal_dev,
                                       const double *point_dev, const double *prev_colour_dev, const double *prev_moments_dev,
                                       const int *prev_shape_dev, const double *prev_normal_dev, const double *prev_point_dev,
                                       const int *prev_count_dev, int n_shapes, const int *moved_dev, const double *motion_dev,
                                       const double *keep_dev, void *out_colour_dev, size_t out_colour_bytes, void *out_moments_dev,
                                       size_t out_moments_bytes, void *out_count_dev, size_t out_count_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_gradient_accumulate(int device, int width, int height, const pt_gradient_history *params, const pt_gradient_camera *prev_camera,
                                const double *colour_host, const int *samples_host, const int *shape_host, const double *normal_host,
                                const double *point_host, const double *prev_colour_host, const double *prev_moments_host,
                                const int *prev_shape_host, const double *prev_normal_host, const double *prev_point_host,
                                const int *prev_count_host, int n_shapes, const int *moved_host, const double *motion_host,
                                const double *keep_host, void *out_colour_host, size_t out_colour_bytes, void *out_moments_host,
                                size_t out_moments_bytes, void *out_count_host, size_t out_count_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_GRADIENT_H */
