/* ptrace_rays.h — C-ABI of libptrace_rays.so: World.ray_intersection and World.is_point_visible for a CALLER's rays.
 *
 * libptrace.so (ptrace.h) traces the primary rays of a frame.  A renderer built on its hit-record frames asks a second
 * question per hit -- a shadow ray to a light, a mirror bounce, an ambient-occlusion probe -- which the reference answers with
 *     World.ray_intersection(ray)             src/pytracer/world.py:51-69    closest hit over all shapes
 *     World.is_point_visible(point, observer) src/pytracer/world.py:71-80    "does any shape block the segment?"
 * one ray at a time.  This library answers both for a batch of rays with the query the path tracer's own scattered and
 * shadow rays go through (csrc/pt_query.h: per-lane candidate lists from a conservative fp32 filter or a grid walk, then
 * the reference's arithmetic on every candidate), so every value is the one the reference computes: shape, t, point and
 * normal bit for bit, a sphere's (u, v) to the few ulp ROCm's atan2 / acos differ from glibc's.
 *
 * It is an add-on: a second shared object with no link dependency on libptrace.so, which loads nothing itself.  The scene
 * comes from the caller, in two calls:
 *     char block[...];                                       // pt_rays_args_bytes() bytes
 *     pt_scene_kernel_args(scene, block, sizeof block);      // libptrace.so (ptrace.h, ABI 1.7)
 *     pt_rays_trace_device(device, block, sizeof block, rays_dev, n, channels, 0, out_dev, out_bytes, stream);
 * Both libraries must come from the same build of the tree (the block's layout is csrc/pt_layout.h's); a block of another
 * size is refused.  The block stays valid until the scene handle it came from is freed.  The scene's tables are immutable
 * after the upload: batches may run on any stream, concurrently with each other and with frames of the same scene.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h, never throws, and checks every argument
 * before its first HIP call (so a bad call fails the same way on a machine without a GPU).
 *
 * Input: PLANAR, eight planes of n doubles -- origin x, y, z; direction x, y, z; tmin; tmax -- the fields of the
 * reference's Ray (ray.py:29-50).  tmax may be +inf.  A ray's tmin has no special meaning: negative values are ordinary.
 *
 * Output, closest hit (anyhit = 0): planar like a hit-record frame (ptrace.h, pt_render_hits) with n values per plane:
 * the int32 shape plane (index into World.shapes, -1 = no hit), padded to a multiple of 8 bytes, then the fp64 planes
 * selected by `channels`, an OR of PT_HIT_T | PT_HIT_POINT | PT_HIT_NORMAL | PT_HIT_UV, in bit order, components
 * x, y, z (u, v).  On a miss t is +inf and every other selected value 0.0.  A channel that is not selected costs no
 * stores (and UV, for spheres, no atan2 / acos).  PT_HIT_RAY (the caller has the rays) and unknown bits: PT_ERR_INVALID.
 *
 * Output, any hit (anyhit = 1; `channels` must be 0): the int32 plane alone, 1 = blocked (some shape has a root in
 * (tmin, tmax): Shape.quick_ray_intersection, shapes.py:133-151, 191-199), 0 = free.
 *
 * n = 0: PT_OK, nothing launched, nothing written.  n < 0 or n > 2^31 - 1: PT_ERR_INVALID.
 *
 * Interface 1.1 adds the question a renderer asks next -- the hit's material, and its shading under the scene's point
 * lights -- as ptrace_surface.h (included below), served by libptrace_surface.so from the same argument block.  The seven
 * entry points of this library are those of 1.0, unchanged.
 */
#ifndef PTRACE_RAYS_H
#define PTRACE_RAYS_H

#include <stddef.h>

#include "ptrace.h" /* PT_HIT_*, PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* (major << 16) | minor of THIS library's interface; this header describes 1.1. */
int pt_rays_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_args_bytes(void);
/* Bytes of the output of a batch; 0 for arguments the trace calls refuse (and for n = 0). */
size_t pt_rays_bytes(long long n, int channels, int anyhit);
/* Byte offset of a plane in that buffer: `channel` one of PT_HIT_* (0: the int32 plane), `component` 0 .. planes - 1.
 * < 0: the channel is not selected (or no such channel / component / bad arguments). */
long long pt_rays_plane_offset(long long n, int channels, int anyhit, int channel, int component);
/* rays_dev and out_dev in the HBM of `device`; asynchronous on `stream` (a hipStream_t; NULL: the default stream, and the
 * call returns when the batch is done).  Allocates nothing.  out_bytes < pt_rays_bytes: PT_ERR_SIZE. */
int pt_rays_trace_device(int device, const void *scene_args, size_t scene_args_bytes, const double *rays_dev,
                         long long n, int channels, int anyhit, void *out_dev, size_t out_bytes, void *stream);
/* The same for host buffers: stages through device memory it allocates and frees.  Synchronous. */
int pt_rays_trace(int device, const void *scene_args, size_t scene_args_bytes, const double *rays_host,
                  long long n, int channels, int anyhit, void *out_host, size_t out_bytes);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_last_error(char *buf, size_t n);

#ifdef __cplusplus
}
#endif

#include "ptrace_surface.h" /* 1.1: materials and point-light shading of the records (libptrace_surface.so) */

#endif /* PTRACE_RAYS_H */
