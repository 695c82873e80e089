/* ptrace_denoise.h — C-ABI of libptrace_denoise.so: an edge-avoiding filter for noisy radiance frames, on the device.
 *
 * Interface 1.8 of the ray library, its tenth step: a DENOISE QUERY.  Every step from the radiance query on hands back Monte-Carlo
 * estimates; this step trades rays for a guided filter: an a-trous (dilated) 5x5 B3 stencil whose tap weights are cut by the
 * guides the library already makes -- `shape`, `point` and `normal` of a hit frame, or of surface points over a texel grid.  What
 * is filtered is the DEMODULATED signal (E of the gather and bake queries, before emitted + brdf_color * E), so pigments stay sharp.
 *
 * Only + - * / sqrt and comparisons occur, in fp64, every operation rounded on its own (no contraction): the weights are rational,
 * not exp, so that pytracer_amd.rays.denoise_host matches the device bit for bit.  The literals and the order below define the bits.
 *
 * FRAME    W x H records, row-major: record r = y * W + x, m = W * H.  Planar fp64 `colour` [3, m] (the noisy signal), `normal`
 * [3, m] (NOT unit length, as a HitRecord.normal is not), `point` [3, m]; `shape` int32[m], negative = no record here.
 *
 * PASSES   pass i = 0 .. passes - 1 has the step s = 2^i and reads the colour pass i - 1 wrote (pass 0: the input).  The guides
 * never change.
 *
 * PIXEL p = (x, y) of one pass:
 *     shape[p] < 0:  out = in, bit for bit.
 *     else, with nh(a) = a / sqrt(a.x * a.x + a.y * a.y + a.z * a.z) and every dot product summed from x to z:
 *     h = (1/16, 1/4, 3/8, 1/4, 1/16),  k(dx, dy) = h[dx + 2] * h[dy + 2]                (all 25 products are exact)
 *     taps: dy outer -2 .. 2, dx inner -2 .. 2, at q = (x + s * dx, y + s * dy):
 *         PT_DN_WRAP_X: qx is taken modulo W into [0, W); otherwise qx outside the frame skips the tap
 *         qy outside the frame always skips the tap
 *     the centre tap (dx = dy = 0):  w = k(0, 0) = 9/64
 *     every other tap:  skipped if shape[q] < 0;  under PT_DN_SAME_SHAPE skipped if shape[q] != shape[p];  else
 *         c  = nh(n_p) . nh(n_q);  if not c > 0: c = 0.0;  then normal_power_log2 times c = c * c
 *         dz = nh(n_p) . (point_q - point_p)
 *         t  = dz / (sigma_point * (double)s)
 *         wp = 1.0 / (1.0 + t * t)
 *         d2 = (dc0 * dc0 + dc1 * dc1) + dc2 * dc2,  dc = colour_q - colour_p of THIS pass's input
 *         sc = sigma_colour * 2^-i
 *         wc = 1.0 / (1.0 + d2 / (sc * sc))
 *         w  = ((k * c) * wp) * wc
 *         skipped unless w > 0                                   (this is where NaN guides die)
 *     sums from +0.0 in tap order:  sum[ch] = sum[ch] + w * colour_q[ch],  wsum = wsum + w;   out[ch] = sum[ch] / wsum
 * The centre tap makes wsum >= 9/64: no division by zero.
 *
 * NON-FINITE COLOURS are not an error and propagate as the arithmetic says: a NaN or infinite colour (or one whose square leaves
 * fp64, 1e300) at p makes every d2 of p NaN or infinite, so p keeps k(0, 0) * colour_p / k(0, 0) -- NaN stays NaN, inf stays inf --
 * and as a neighbour q of a finite pixel it has w = NaN or 0 and is skipped.  Non-finite guides only ever skip taps.
 *
 * A TENTH shared object, for the reasons the nine before it give.  It links to none of the others, loads nothing and reads no
 * scene (like the lit library's evaluation query).
 *
 * LAUNCHES  pt_rays_denoise_device allocates nothing and is asynchronous on the caller's stream (a hipStream_t; NULL: the default
 * stream, and the call returns when the work is done): one pre-pass that writes nh(normal) into the workspace, then one launch
 * per pass, ping-ponging between `out` and the workspace so that the last pass lands in `out`.  Workspace:
 *     pt_rays_denoise_workspace_bytes = 24 m (unit normals) + 24 m (the other colour buffer; only when passes > 1).
 * No bit depends on the launch shape.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never throws,
 * and checks every argument before its first HIP call:
 *     width or height < 0; width * height > 2^31 - 1; passes outside 1 .. 10; a sigma that is not > 0 (NaN included; +inf is
 *     legal and switches the weight off); normal_power_log2 outside 0 .. 10; unknown flag bits; NULL where a buffer is needed;
 *     `out` overlapping `colour` or the workspace                                                          PT_ERR_INVALID
 *     an output or a workspace that is too small                                                           PT_ERR_SIZE
 * m = 0 is PT_OK with nothing launched.  pt_rays_denoise takes host buffers, stages them through device memory it allocates and
 * frees (workspace included) and is synchronous.
 */
#ifndef PTRACE_DENOISE_H
#define PTRACE_DENOISE_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_DN_SAME_SHAPE 1 /* a tap on another shape is skipped (default: on) */
#define PT_DN_WRAP_X     2 /* columns wrap: the u seam of a sphere's (u, v) map */

typedef struct pt_denoise_params {
  int passes;            /* 1 .. 10 (default 4): pass i has the step 2^i            */
  int normal_power_log2; /* e in 0 .. 10 (default 5: cos^32)                        */
  int flags;             /* PT_DN_* bits                                            */
  double sigma_point;    /* > 0 or +inf: plane distance at which wp = 1/2, per step */
  double sigma_colour;   /* > 0 or +inf (default +inf: the colour weight is off)    */
} pt_denoise_params;

/* (major << 16) | minor of the ray library's interface this library implements: 1.8. */
int pt_rays_denoise_version(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_denoise_last_error(char *buf, size_t n);

/* Bytes of a filtered frame of m records: 24 m (0 on refusal). */
size_t pt_rays_denoise_bytes(long long m);
/* Bytes of the workspace of pt_rays_denoise_device (0 on refusal, the reason in pt_rays_denoise_last_error; and 0 for m = 0). */
size_t pt_rays_denoise_workspace_bytes(int width, int height, const pt_denoise_params *params);

int pt_rays_denoise_device(int device, int width, int height, const pt_denoise_params *params, const double *colour_dev,
                           const double *normal_dev, const double *point_dev, const int *shape_dev, void *out_dev, size_t out_bytes,
                           void *workspace_dev, size_t workspace_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_denoise(int device, int width, int height, const pt_denoise_params *params, const double *colour_host,
                    const double *normal_host, const double *point_host, const int *shape_host, void *out_host, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_DENOISE_H */
