/* ptrace_variance.h — C-ABI of libptrace_variance.so: luminance moments, a per-pixel variance and a variance-guided filter, on the device.
 *
 * Interface 1.10 of the ray library, its twelfth step: a VARIANCE QUERY, the piece that joins the tenth step (ptrace_denoise.h, rays
 * for space) and the eleventh (ptrace_temporal.h, rays for time): how noisy a pixel still is.  Three queries:
 *     MOMENTS   a frame (l, l * l, 0) of the luminance of a noisy frame, which the accumulate query of ptrace_temporal.h carries from
 *               frame to frame UNCHANGED (its kernel is generic in its three channels): running first and second moments with the
 *               taps, the alpha and the count of the colour
 *     ESTIMATE  the variance of the accumulated mean from those moments, with a spatial fallback where the history is short
 *     FILTER    the a-trous filter of ptrace_denoise.h with its colour weight replaced by a luminance weight scaled by the variance,
 *               and which filters the variance along with the colour (SVGF's filter)
 *
 * Only + - * / sqrt and comparisons occur, in fp64, every operation rounded on its own (no contraction), so that
 * pytracer_amd.rays.luminance_moments_host, variance_estimate_host and variance_filter_host match the device bit for bit.  The
 * literals and the order below define the bits.
 *
 * FRAME    W x H records, row-major: record r = y * W + x, m = W * H.  Planar fp64 `colour` [3, m], `normal` [3, m] (NOT unit
 * length), `point` [3, m]; `shape` int32[m], negative = no record here; `variance` fp64 [m]; `moments` fp64 [3, m]; `count`
 * int32[m], the accumulate query's history length.
 *
 * lum(c)   mx = c0; if (c1 > mx) mx = c1; if (c2 > mx) mx = c2;  mn = c0; if (c1 < mn) mn = c1; if (c2 < mn) mn = c2;
 *          lum = (mx + mn) / 2.0                                    (Color.luminosity, with comparisons: NaN behaves the same everywhere)
 * nh(a)    a / sqrt(a.x * a.x + a.y * a.y + a.z * a.z); every dot product is summed from x to z.
 *
 * 1. MOMENTS, per record r:   shape[r] < 0:  out = (+0.0, +0.0, +0.0);   else  l = lum(colour_r):  out = (l, l * l, +0.0)
 *
 * 2. ESTIMATE, per pixel p = (x, y), with n = count[p], mu1 = moments[0][p], mu2 = moments[1][p]:
 *     shape[p] < 0 or n < 1:   variance = +0.0
 *     n >= min_history:        v = mu2 - mu1 * mu1;  if (!(v > 0)) v = 0.0;  variance = v / (double)n          (the temporal estimate)
 *     else the spatial estimate over the 7x7 window: dy outer -3 .. 3, dx inner -3 .. 3, at q = (x + dx, y + dy):
 *         PT_VR_WRAP_X: qx is taken modulo W into [0, W); otherwise qx outside the frame skips the tap
 *         qy outside the frame always skips the tap
 *         the centre is always taken; any other tap q is skipped if shape[q] < 0; under PT_VR_SAME_SHAPE if shape[q] != shape[p];
 *         if count[q] < 1; unless nh(n_p) . nh(n_q) >= normal_min; unless fabs(nh(n_p) . (point_q - point_p)) <= point_tolerance
 *         sums from +0.0 in tap order:  s1 = s1 + moments[0][q],  s2 = s2 + moments[1][q],  k = k + 1.0
 *         mean = s1 / k;  v = s2 / k - mean * mean;  if (!(v > 0)) v = 0.0;  variance = v / (double)n
 * A CHOICE: dividing by n makes this the variance of the ACCUMULATED MEAN, which is the signal the filter sees; SVGF hands its
 * filter the per-frame variance instead.  A pixel with no accepted neighbour and n = 1 gets the variance 0 and is left nearly
 * unfiltered (its luminance weight is 1 / (1 + dl^2 / epsilon)).
 *
 * 3. FILTER.  Pass i = 0 .. passes - 1 has the step s = 2^i and reads the colour AND the variance pass i - 1 wrote (pass 0: the
 * inputs).  The guides never change.  Per pixel p of one pass:
 *     shape[p] < 0:  both outputs equal the inputs, bit for bit.
 *     the prefiltered variance g_p: a 3x3 stencil at step 1 (NOT dilated) with the weights (1/4, 1/2, 1/4) squared (all exact),
 *         dy outer -1 .. 1, dx inner -1 .. 1, over this pass's input variance; a tap, THE CENTRE INCLUDED, is skipped when it lies
 *         outside the frame (PT_VR_WRAP_X applies to qx), when shape[q] < 0, when shape[q] != shape[p] under PT_VR_SAME_SHAPE, or
 *         unless var_q >= 0 (negative and NaN variances die here); sums from +0.0:  gs = gs + kw * var_q,  gw = gw + kw;
 *         g = gw > 0 ? gs / gw : 0.0
 *     den_p = sl2 * g_p + epsilon,  sl2 = sigma_luminance * sigma_luminance (formed once, on the host)
 *     the 25 taps, their order, k, c (with normal_power_log2), wp (with sigma_point * (double)s) and the treatment of an infinite
 *     sigma_point are EXACTLY those of ptrace_denoise.h; in place of its wc:
 *         dl = lum(colour_q) - lum(colour_p) of THIS pass's input
 *         wl = 1.0 / (1.0 + (dl * dl) / den_p);   sigma_luminance = +inf:  wl = 1.0 where dl * dl < inf, else NaN (no division)
 *         w  = ((k * c) * wp) * wl;  skipped unless w > 0
 *     the centre tap has w = 9/64
 *     sums from +0.0 in tap order:  sum[ch] = sum[ch] + w * colour_q[ch],  wsum = wsum + w,  vs = vs + (w * w) * var_q
 *     out_colour[ch] = sum[ch] / wsum;   out_variance = vs / (wsum * wsum)
 *
 * NON-FINITE COLOURS AND VARIANCES are not an error and propagate as the arithmetic says.  Non-finite guides only ever skip taps.
 *
 * A TWELFTH shared object, for the reasons the eleven before it give.  It links to none of the others, loads nothing and reads no
 * scene.
 *
 * LAUNCHES  The device forms allocate nothing and are asynchronous on the caller's stream (a hipStream_t; NULL: the default stream,
 * and the call returns when the work is done).  Moments and estimate: one launch each.  Filter: one pre-pass that writes nh(normal)
 * into the workspace, then per pass one launch that writes g as a plane and one that filters, colour and variance ping-ponging
 * between the outputs and the workspace so that the last pass lands in `out_colour` and `out_variance`.  Workspace:
 *     pt_rays_variance_workspace_bytes = 24 m (unit normals) + 8 m (g) + 32 m (the other colour and variance; only when passes > 1).
 * No bit depends on the launch shape.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never throws,
 * and checks every argument before its first HIP call:
 *     width or height < 0; width * height > 2^31 - 1; a NULL struct; passes outside 1 .. 10; normal_power_log2 outside 0 .. 10;
 *     min_history outside 1 .. 2^20; a sigma_point, sigma_luminance or point_tolerance that is not > 0 (NaN included; +inf is
 *     legal); an epsilon that is not finite and > 0; normal_min outside [-1, 1]; unknown flag bits; NULL where a buffer is needed;
 *     any output overlapping an input, the other output or the workspace                                     PT_ERR_INVALID
 *     an output or a workspace that is too small                                                           PT_ERR_SIZE
 * m = 0 is PT_OK with nothing launched (the struct is still checked).  The forms without `_device` take host buffers, stage them
 * through device memory they allocate and free (workspace included) and are synchronous.
 */
#ifndef PTRACE_VARIANCE_H
#define PTRACE_VARIANCE_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_VR_SAME_SHAPE 1 /* a tap on another shape is skipped (default: on) */
#define PT_VR_WRAP_X     2 /* columns wrap: the u seam of a sphere's (u, v) map */

#define PT_VR_MAX_HISTORY 1048576 /* 2^20 */

typedef struct pt_variance_params {
  int passes;             /* 1 .. 10 (default 4): pass i has the step 2^i                                        */
  int normal_power_log2;  /* e in 0 .. 10 (default 5: cos^32)                                                    */
  int flags;              /* PT_VR_* bits                                                                        */
  int min_history;        /* 1 .. 2^20 (default 4): below it the estimate is spatial                             */
  double sigma_point;     /* > 0 or +inf: plane distance at which wp = 1/2, per step                             */
  double sigma_luminance; /* > 0 or +inf (default 1.0; +inf: the luminance weight is off)                        */
  double epsilon;         /* finite, > 0 (default 1e-10): what keeps den_p from 0                                */
  double normal_min;      /* in [-1, 1] (default 0.9): the spatial estimate's least cosine between unit normals  */
  double point_tolerance; /* > 0 or +inf (default 0.05): its largest distance from the pixel's tangent plane     */
} pt_variance_params;

/* (major << 16) | minor of the ray library's interface this library implements: 1.10. */
int pt_rays_variance_version(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_variance_last_error(char *buf, size_t n);

/* Bytes of a [3, m] frame (moments, filtered colour): 24 m (0 on refusal). */
size_t pt_rays_variance_bytes(long long m);
/* Bytes of a variance plane: 8 m (0 on refusal). */
size_t pt_rays_variance_plane_bytes(long long m);
/* Bytes of the workspace of pt_rays_variance_filter_device (0 on refusal, the reason in pt_rays_variance_last_error; 0 for m = 0). */
size_t pt_rays_variance_workspace_bytes(int width, int height, const pt_variance_params *params);

int pt_rays_variance_moments_device(int device, int width, int height, const double *colour_dev, const int *shape_dev, void *out_dev,
                                    size_t out_bytes, void *stream);
int pt_rays_variance_estimate_device(int device, int width, int height, const pt_variance_params *params, const double *moments_dev,
                                     const int *count_dev, const int *shape_dev, const double *normal_dev, const double *point_dev,
                                     void *out_dev, size_t out_bytes, void *stream);
int pt_rays_variance_filter_device(int device, int width, int height, const pt_variance_params *params, const double *colour_dev,
                                   const double *variance_dev, const double *normal_dev, const double *point_dev, const int *shape_dev,
                                   void *out_colour_dev, size_t out_colour_bytes, void *out_variance_dev, size_t out_variance_bytes,
                                   void *workspace_dev, size_t workspace_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_variance_moments(int device, int width, int height, const double *colour_host, const int *shape_host, void *out_host,
                             size_t out_bytes);
int pt_rays_variance_estimate(int device, int width, int height, const pt_variance_params *params, const double *moments_host,
                              const int *count_host, const int *shape_host, const double *normal_host, const double *point_host,
                              void *out_host, size_t out_bytes);
int pt_rays_variance_filter(int device, int width, int height, const pt_variance_params *params, const double *colour_host,
                            const double *variance_host, const double *normal_host, const double *point_host, const int *shape_host,
                            void *out_colour_host, size_t out_colour_bytes, void *out_variance_host, size_t out_variance_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_VARIANCE_H */
