/* ptrace_weighted.h — C-ABI of libptrace_weighted.so: the accumulation of ptrace_temporal.h with every frame weighted by the samples
 * it took, for the colour and for its luminance moments in one pass over the taps, on the device.
 *
 * Interface 1.12 of the ray library, its fourteenth step: a WEIGHTED ACCUMULATE QUERY.  The accumulate query (ptrace_temporal.h)
 * blends with alpha = 1 / n: a pixel's 31-sample frame counts as much as its 1-sample frame, a record the ragged gather of
 * ptrace_adaptive.h cut off (taken = 0, radiance 0) is blended in as black, and the variance path finds the same four taps twice
 * (once for the colour, once for the moments) after a launch that makes the moments.  This query is ONE kernel that does, per pixel
 * and in one pass over the four taps, what the accumulate query does for the colour, what it does for the luminance moments, and
 * what the moments query of ptrace_variance.h does -- with every frame weighted by its sample count, and the weight sum S carried
 * beside them.
 *
 * Only + - * / sqrt floor and comparisons occur, in fp64, every operation rounded on its own (no contraction), so that
 * pytracer_amd.rays.weighted_host matches the device bit for bit.  The literals and the order below define the bits.
 * lum(c) is that of ptrace_variance.h: mx = the largest, mn = the smallest of the three channels by comparisons, (mx + mn) / 2.0.
 * nh(a) = a / sqrt(a.x * a.x + a.y * a.y + a.z * a.z) and every dot product summed from x to z, as in ptrace_temporal.h.
 *
 * FRAMES   W x H records, row-major: record r = y * W + x, m = W * H; the current and the previous frame have this size.
 *     current:   `colour` [3, m] fp64 (this frame's noisy E), `samples` int32[m] or NULL (NULL: k = 1 everywhere; it may point
 *                straight at the PT_ADAPTIVE_TAKEN plane of a ragged gather in HBM), `shape` int32[m] (negative = no record),
 *                `normal` [3, m] (NOT unit length), `point` [3, m]
 *     previous:  `prev_colour` [3, m], `prev_moments` [3, m] = (M1, M2, S), `prev_shape`, `prev_normal`, `prev_point` and
 *                `prev_count` int32[m], the history length (<= 0: nothing to reuse)
 *     outputs:   `out_colour` [3, m] fp64, `out_moments` [3, m] fp64 = (M1, M2, S), `out_count` int32[m]
 * S is the accumulated weight.  The moments frame has the layout the variance estimate of ptrace_variance.h reads (planes 0 and 1,
 * the third "not read"), so the estimate query of that header takes `out_moments` and `out_count` unchanged; the third plane,
 * which the unweighted path fills with zeros, carries S.
 *
 * PIXEL p, with k = samples ? samples[p] : 1, kd = (double)k and l = lum(colour_p):
 *   1. shape[p] < 0:  out_colour = colour_p bit for bit, out_moments = (+0.0, +0.0, +0.0), out_count = 0.
 *   2. steps 2 to 8 of ptrace_temporal.h EXACTLY: the projection onto the previous screen, "NO HISTORY", the four taps in the
 *      order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), their weights b, and every skip rule (PT_WA_SAME_SHAPE in
 *      the place of PT_TA_SAME_SHAPE).
 *   3. sums from +0.0 in tap order over the accepted taps r:
 *        hs[ch] = hs[ch] + b * prev_colour_r[ch],  h1 = h1 + b * M1_r,  h2 = h2 + b * M2_r,  hS = hS + b * S_r,  ws = ws + b;
 *        nmax = the largest prev_count of the accepted taps;  smax from +0.0 with  if (S_r > smax) smax = S_r
 *   4. no tap accepted, or NO HISTORY:
 *        k > 0:   out_colour = colour_p bit for bit, out_moments = (l, l * l, kd), out_count = 1
 *        k <= 0:  out_colour = colour_p bit for bit, out_moments = (+0.0, +0.0, +0.0), out_count = 0   (nothing to reuse)
 *   5. else  hist[ch] = hs[ch] / ws,  m1 = h1 / ws,  m2 = h2 / ws;
 *            Sh = smax, or under PT_WA_BLEND_WEIGHT Sh = hS / ws;
 *            if (!(Sh > 0.0)) Sh = 0.0;  if (Sh > max_weight) Sh = max_weight;     (in this order: NaN and negative weights
 *                                                                                   die in the first clamp)
 *        k > 0:   total = Sh + kd;  alpha = kd / total;
 *                 out[ch] = hist[ch] + (colour_p[ch] - hist[ch]) * alpha;
 *                 M1 = m1 + (l - m1) * alpha;  M2 = m2 + (l * l - m2) * alpha;  S = total;
 *                 out_count = min(nmax + 1, max_history), formed without leaving an int
 *        k <= 0:  out_colour = hist, out_moments = (m1, m2, Sh), out_count = min(nmax, max_history): the history is carried and
 *                 this frame's colour is never read into it.
 * A mean weighted by samples until the weight reaches max_weight, an exponential average from then on.
 *
 * THE VARIANCE ESTIMATE NEEDS NO CHANGE.  With weights k_i, S (M2 - M1^2) estimates sum k_i (l_i - lbar)^2, about n sigma^2 (sigma^2
 * the variance of one sample, n = out_count frames), and the accumulated mean has the variance sigma^2 / S.  So (M2 - M1^2) / n
 * remains the variance of the accumulated mean: the formula of ptrace_variance.h step 2, which reads out_moments and out_count.
 *
 * TWO CONTRACTS that come from the arithmetic:
 *   A. UNWEIGHTED, IT IS THE OLD PATH IN ONE LAUNCH.  With samples = NULL, max_weight = (double)(max_history - 1),
 *      PT_WA_BLEND_WEIGHT off and a prev_moments whose third plane is (double)prev_count: out_colour and out_count are bit for bit
 *      those of the accumulate query (ptrace_temporal.h); planes 0 and 1 of out_moments are bit for bit the accumulate query
 *      applied to the frame of the moments query; and out_moments[2] == (double)out_count.  (total = min(nmax, max_history - 1)
 *      + 1.0 = n exactly, and 1.0 / total is the old alpha.)
 *   B. EQUAL COUNTS CHANGE NOTHING.  With a samples plane that is K everywhere, max_weight = K * (max_history - 1) and S planes
 *      that are K * count, the colour bits are those under A.  (K / (K * n) and 1.0 / n are both the correctly rounded 1 / n.)
 *
 * NON-FINITE COLOURS are not an error and propagate as the arithmetic says.  Non-finite guides only ever skip taps.
 *
 * A FOURTEENTH shared object, for the reasons the thirteen before it give.  It links to none of the others, loads nothing and reads
 * no scene.
 *
 * LAUNCHES  pt_rays_weighted_accumulate_device allocates nothing, makes ONE launch and is asynchronous on the caller's stream (a
 * hipStream_t; NULL: the default stream, and the call returns when the work is done).  No bit depends on the launch shape.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never throws,
 * and checks every argument before its first HIP call:
 *     width or height < 0; width * height > 2^31 - 1; a NULL struct; max_history outside 1 .. 2^20; unknown flag bits;
 *     normal_min outside [-1, 1] (NaN included); a point_tolerance that is not > 0 (+inf is legal and switches the test off); a
 *     max_weight that is not >= 0 (NaN included; +inf is legal and means never cap); an unknown camera kind; NULL where a buffer
 *     is needed (a NULL `samples` is legal); any of the three outputs overlapping another output, any previous plane, `colour`
 *     or `samples` (a tap reads its neighbours' history: the history ping-pongs)                              PT_ERR_INVALID
 *     an output that is too small (each with its own message)                                                PT_ERR_SIZE
 * m = 0 is PT_OK with nothing launched (the structs are still checked).  pt_rays_weighted_accumulate takes host buffers, stages
 * them through device memory it allocates and frees, and is synchronous.
 */
#ifndef PTRACE_WEIGHTED_H
#define PTRACE_WEIGHTED_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_*, PT_CAMERA_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_WA_SAME_SHAPE 1   /* a tap on another shape is skipped (default: on)                             */
#define PT_WA_BLEND_WEIGHT 2 /* the history's weight is the taps' blend hS / ws, not their largest (smax)   */

#define PT_WA_MAX_HISTORY 1048576 /* 2^20 */

typedef struct pt_weighted_params {
  int max_history;        /* 1 .. 2^20 (default 32): the cap of the history LENGTH out_count                     */
  int flags;              /* PT_WA_* bits                                                                       */
  double normal_min;      /* in [-1, 1] (default 0.9): the least cosine between the unit normals                */
  double point_tolerance; /* > 0 or +inf (default 0.05): the largest distance from the pixel's tangent plane    */
  double max_weight;      /* >= 0 or +inf (default 128): the cap of the history's WEIGHT before this frame's is added */
} pt_weighted_params;

/* The camera the PREVIOUS frame was seen from: the layout of pt_temporal_camera. */
typedef struct pt_weighted_camera {
  int kind;               /* PT_CAMERA_* of ptrace.h                                  */
  double invm[12];        /* rows 0..2 of camera.transformation.invm (world -> camera) */
  double screen_distance; /* perspective only                                         */
  double aspect_ratio;
} pt_weighted_camera;

/* (major << 16) | minor of the ray library's interface this library implements: 1.12. */
int pt_rays_weighted_version(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_weighted_last_error(char *buf, size_t n);

/* Bytes of an accumulated frame of m records, and of its moments frame: 24 m (0 on refusal). */
size_t pt_rays_weighted_bytes(long long m);
/* Bytes of its history lengths: 4 m (0 on refusal). */
size_t pt_rays_weighted_count_bytes(long long m);

/* A history that holds nothing: the m lengths at count_dev become 0, on the caller's stream (the start of a sequence; with lengths
 * of 0 no colour, moment or weight of the history is ever read).  Refuses m outside [0, 2^31 - 1] and a NULL buffer
 * (PT_ERR_INVALID) and a buffer below 4 m bytes (PT_ERR_SIZE); m = 0 is PT_OK. */
int pt_rays_weighted_clear_device(int device, long long m, void *count_dev, size_t count_bytes, void *stream);

int pt_rays_weighted_accumulate_device(int device, int width, int height, const pt_weighted_params *params,
                                       const pt_weighted_camera *prev_camera, const double *colour_dev, const int *samples_dev,
                                       const int *shape_dev, const double *normal_dev, const double *point_dev,
                                       const double *prev_colour_dev, const double *prev_moments_dev, const int *prev_shape_dev,
                                       const double *prev_normal_dev, const double *prev_point_dev, const int *prev_count_dev,
                                       void *out_colour_dev, size_t out_colour_bytes, void *out_moments_dev, size_t out_moments_bytes,
                                       void *out_count_dev, size_t out_count_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_weighted_accumulate(int device, int width, int height, const pt_weighted_params *params, const pt_weighted_camera *prev_camera,
                                const double *colour_host, const int *samples_host, const int *shape_host, const double *normal_host,
                                const double *point_host, const double *prev_colour_host, const double *prev_moments_host,
                                const int *prev_shape_host, const double *prev_normal_host, const double *prev_point_host,
                                const int *prev_count_host, void *out_colour_host, size_t out_colour_bytes, void *out_moments_host,
                                size_t out_moments_bytes, void *out_count_host, size_t out_count_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_WEIGHTED_H */
