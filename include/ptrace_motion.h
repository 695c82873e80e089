/* ptrace_motion.h — C-ABI of libptrace_motion.so: the accumulation of ptrace_weighted.h with a motion per shape, so that the history
 * of a shape that moved between two frames is fetched where that surface point WAS, on the device.
 *
 * Interface 1.13 of the ray library, its fifteenth step: a MOTION ACCUMULATE QUERY.  Steps eleven to fourteen (ptrace_temporal.h,
 * ptrace_variance.h, ptrace_adaptive.h, ptrace_weighted.h) reproject this frame's hit point through the previous CAMERA only: the
 * world is taken to be the same in both frames.  A shape that moved breaks that twice over.  The point it shows at a pixel was
 * somewhere else on the previous screen, so the taps found at the unmoved point fail the tangent-plane test and the shape restarts
 * at one frame of history on every frame it moves; and where the test does pass, the tap belongs to another surface point of the
 * same shape.  This query is the weighted accumulate query with one more step in front: a record whose shape moved is carried into
 * the PREVIOUS frame's world before it is projected and tested.  Everything else -- params, previous camera, the eleven planes, the
 * three outputs, the stream -- is ptrace_weighted.h's, and that header's text is the specification of all that is not restated here.
 *
 * TABLES   `n_shapes` (an int), `moved` int32[n_shapes] and `motion` double[n_shapes][24], one record of 192 bytes per shape so that
 *          every record starts on a 64-byte boundary of a table that does:
 *     motion[s][0 .. 11]   rows 0..2 of the affine map A_s, which takes a point of shape s in THIS frame's world to where that surface
 *                          point was in the PREVIOUS frame's world (prev.transformation * cur.transformation^-1)
 *     motion[s][12 .. 20]  the 3 x 3 N_s, row-major, which carries a normal the same way: the transpose of the linear part of A_s^-1
 *     motion[s][21 .. 23]  never read
 *
 * PIXEL p, with s = shape[p]:
 *   0. s < 0:  step 1 of ptrace_weighted.h.
 *   1. if 0 <= s < n_shapes and moved[s] != 0:
 *          pm = A_s * point_p,   each row as  ((a0 * px + a1 * py) + a2 * pz) + a3
 *          nm = N_s * normal_p,  each row as  (n0 * nx + n1 * ny) + n2 * nz
 *      otherwise pm = point_p and nm = normal_p, bit for bit, and NO table entry is read.  An index at or beyond n_shapes is a
 *      static shape and not an error, so that records nobody vouches for keep every address legal.
 *   2. steps 2 to 5 of ptrace_weighted.h EXACTLY, with pm wherever they read point_p and nm wherever they read n_p: the projection
 *      onto the previous screen, the cosine c, the tangent-plane distance dz and the unit normal nh(nm).  The outputs and their
 *      layouts are unchanged.
 * The kernel writes no guides: next frame's history guides are this frame's own records, unmoved.
 *
 * Only + - * / sqrt floor and comparisons occur, in fp64, every operation rounded on its own (no contraction), in the order above, so
 * that pytracer_amd.rays.motion_host matches the device bit for bit.  NON-FINITE TABLE ENTRIES are not an error: they end in
 * "NO HISTORY" or in skipped taps.
 *
 * TWO CONTRACTS that come from the arithmetic:
 *   C. NOTHING MOVED, NOTHING CHANGES.  With n_shapes = 0, NULL tables or a `moved` that is 0 everywhere, all three outputs are bit
 *      for bit those of the weighted accumulate query.  Contracts A and B of ptrace_weighted.h therefore hold here too.
 *   D. IT IS THE WEIGHTED QUERY ON MOVED RECORDS.  For any table, the outputs are bit for bit those of the weighted accumulate
 *      query on records whose `point` and `normal` were replaced by pm and nm on the host.
 *
 * WHAT MOVES AND WHAT DOES NOT.  E is light arriving at a PLACE.  A shape that moves ONTO ITSELF -- a sphere spinning about an axis
 * through its centre, a plane sliding in its own plane -- carries no light with it: its `moved` entry belongs at 0, and the
 * history then stays where the light is.
 *
 * A FIFTEENTH shared object, for the reasons the fourteen before it give.  It links to none of the others, loads nothing and reads
 * no scene.
 *
 * LAUNCHES  pt_rays_motion_accumulate_device allocates nothing, makes ONE launch and is asynchronous on the caller's stream (a
 * hipStream_t; NULL: the default stream, and the call returns when the work is done).  No bit depends on the launch shape.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never throws,
 * and checks every argument before its first HIP call.  The refusals are all of ptrace_weighted.h's, and in addition:
 *     n_shapes < 0 or above 2^20; n_shapes > 0 with a NULL `moved` or `motion`; any of the three outputs overlapping either
 *     table                                                                                                  PT_ERR_INVALID
 * m = 0 is PT_OK with nothing launched (the structs and n_shapes are still checked).  pt_rays_motion_accumulate takes host buffers,
 * stages them through device memory it allocates and frees, and is synchronous.
 */
#ifndef PTRACE_MOTION_H
#define PTRACE_MOTION_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_*, PT_CAMERA_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_MA_SAME_SHAPE 1   /* a tap on another shape is skipped (default: on)                             */
#define PT_MA_BLEND_WEIGHT 2 /* the history's weight is the taps' blend hS / ws, not their largest (smax)   */

#define PT_MA_MAX_HISTORY 1048576 /* 2^20 */
#define PT_MA_MAX_SHAPES 1048576  /* 2^20 */
#define PT_MA_RECORD 24           /* doubles per shape in `motion`: 192 bytes */

/* The layout of pt_weighted_params. */
typedef struct pt_motion_params {
  int max_history;        /* 1 .. 2^20 (default 32): the cap of the history LENGTH out_count                     */
  int flags;              /* PT_MA_* bits                                                                       */
  double normal_min;      /* in [-1, 1] (default 0.9): the least cosine between the unit normals                */
  double point_tolerance; /* > 0 or +inf (default 0.05): the largest distance from the pixel's tangent plane    */
  double max_weight;      /* >= 0 or +inf (default 128): the cap of the history's WEIGHT before this frame's is added */
} pt_motion_params;

/* The camera the PREVIOUS frame was seen from: the layout of pt_temporal_camera. */
typedef struct pt_motion_camera {
  int kind;               /* PT_CAMERA_* of ptrace.h                                  */
  double invm[12];        /* rows 0..2 of camera.transformation.invm (world -> camera) */
  double screen_distance; /* perspective only                                         */
  double aspect_ratio;
} pt_motion_camera;

/* (major << 16) | minor of the ray library's interface this library implements: 1.13. */
int pt_rays_motion_version(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_motion_last_error(char *buf, size_t n);

/* Bytes of an accumulated frame of m records, and of its moments frame: 24 m (0 on refusal). */
size_t pt_rays_motion_bytes(long long m);
/* Bytes of its history lengths: 4 m (0 on refusal). */
size_t pt_rays_motion_count_bytes(long long m);
/* Bytes of the `motion` table of n_shapes shapes: 192 n_shapes (0 on refusal: n_shapes outside [0, 2^20]). */
size_t pt_rays_motion_table_bytes(int n_shapes);

/* A history that holds nothing: the m lengths at count_dev become 0, on the caller's stream.  Refuses m outside [0, 2^31 - 1] and
 * a NULL buffer (PT_ERR_INVALID) and a buffer below 4 m bytes (PT_ERR_SIZE); m = 0 is PT_OK. */
int pt_rays_motion_clear_device(int device, long long m, void *count_dev, size_t count_bytes, void *stream);

int pt_rays_motion_accumulate_device(int device, int width, int height, const pt_motion_params *params, const pt_motion_camera *prev_camera,
                                     const double *colour_dev, const int *samples_dev, const int *shape_dev, const double *normal_dev,
                                     const double *point_dev, const double *prev_colour_dev, const double *prev_moments_dev,
                                     const int *prev_shape_dev, const double *prev_normal_dev, const double *prev_point_dev,
                                     const int *prev_count_dev, int n_shapes, const int *moved_dev, const double *motion_dev,
                                     void *out_colour_dev, size_t out_colour_bytes, void *out_moments_dev, size_t out_moments_bytes,
                                     void *out_count_dev, size_t out_count_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_motion_accumulate(int device, int width, int height, const pt_motion_params *params, const pt_motion_camera *prev_camera,
                              const double *colour_host, const int *samples_host, const int *shape_host, const double *normal_host,
                              const double *point_host, const double *prev_colour_host, const double *prev_moments_host,
                              const int *prev_shape_host, const double *prev_normal_host, const double *prev_point_host,
                              const int *prev_count_host, int n_shapes, const int *moved_host, const double *motion_host,
                              void *out_colour_host, size_t out_colour_bytes, void *out_moments_host, size_t out_moments_bytes,
                              void *out_count_host, size_t out_count_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_MOTION_H */
