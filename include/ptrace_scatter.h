/* ptrace_scatter.h — C-ABI of libptrace_scatter.so: BRDF.scatter_ray and the Russian roulette for hit records, in batches.
 *
 * Interface 1.2 of the ray library, its fourth step: trace (ptrace.h / ptrace_rays.h) -> material (ptrace_surface.h) ->
 * SCATTER -> trace.  What the reference's PathTracer does between two calls of world.ray_intersection (render.py:107-134) for
 * ONE child of a hit, here for n records at once, each record carrying its own generator from one bounce to the next:
 *     1. hit_color = brdf.pigment.get_color(uv), emitted = emitted_radiance.get_color(uv), lum = max(r, g, b) of hit_color
 *     2. roulette (the caller says whether ray.depth >= russian_roulette_limit holds for this batch):
 *        q = max(0.05, 1 - lum), ONE draw; draw > q: hit_color *= 1.0 / (1.0 - q); otherwise the record is terminated
 *     3. lum > 0.0 and not terminated: brdf.scatter_ray (materials.py:132-196) -- TWO draws and a cosine-weighted direction for
 *        a DiffuseBRDF, no draw and the mirror direction for a SpecularBRDF
 * with the device functions of the fused path tracer (pcg_float, scatter_ray with its inlined sincos: csrc/pt_math.h,
 * pt_shade.h), so every value is the one the fused kernel computes for that record, bit for bit.
 *
 * A FOURTH shared object, for the reasons the third one gives: libptrace_surface.so's exported symbols are pinned to its 11,
 * libptrace_rays.so's to its seven, libptrace.so's device code by every profiles/pmc_*.json.  ptrace_rays.h and
 * ptrace_surface.h stay as they are (they report interface 1.1); a caller of this step includes this header as well.  Like the
 * others the library links to none of them, loads nothing, and gets the scene from its caller as the argument block of
 * pt_scene_kernel_args (ptrace.h, ABI 1.7); all four must come from one build of the tree, a block of another size is refused.
 * The slot table is the one pt_rays_slots_device (ptrace_surface.h) makes.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never
 * throws, and checks every argument before its first HIP call.  n = 0: PT_OK, nothing launched, nothing written.  n < 0 or
 * n > 2^31 - 1: PT_ERR_INVALID.  The *_device form is asynchronous on the caller's stream (a hipStream_t; NULL: the default
 * stream, and the call returns when the work is done) and allocates nothing.
 *
 * Input: PLANAR, n values per plane, as a hit-record frame or a closest-hit batch holds them -- a plane pointer into either
 * buffer is passed as it is:
 *     shape   n int32   index into World.shapes, or anything outside [0, n_shapes) (-1) for "no hit"
 *     point   3 planes  HitRecord.world_point            normal  3 planes  HitRecord.normal
 *     uv      2 planes  HitRecord.surface_point          dir     3 planes  the direction of the ray that was traced
 *     state, inc   n uint64 each: the record's generator (PCG-XSH-RR 64/32, pcg.py: `state` and `inc` as the class keeps them)
 * uv is ALWAYS required (a scene whose pigments are all uniform would not read it, but the library does not ask the scene).
 * A record is the caller's: nothing about it is assumed (non-finite values give the reference's non-finite results; an image
 * pigment's column and row are clamped into the texture, NaN to 0, as in ptrace_surface.h; a checkered pigment whose
 * u * steps or v * steps is not finite -- the reference raises -- answers one of its two colours by that header's definition:
 * a NaN cell counts as odd, an infinite one as even).  The generator's words are the caller's too: every value of state and
 * inc is legal input, an even inc included.
 *
 * Output: one buffer of pt_rays_scatter_bytes(n, channels) bytes, planar, n values per plane:
 *     status  n int32, padded to a multiple of 8 bytes:  -1 no hit (the caller's value: its background)
 *                                                          0 terminated, by the roulette or by lum <= 0 (value: emitted)
 *                                                          1 scattered
 *     rays    8 fp64 planes in the layout pt_rays_trace_device reads (origin xyz, direction xyz, tmin, tmax): the block can be
 *             traced as it stands, and its direction planes are the next step's `dir`.
 *             status 1: the reference's ray -- origin = point, tmin 1e-3 (diffuse) or 1e-5 (mirror), tmax +inf.
 *             status != 1: the DEAD RAY origin (0, 0, 0), direction (0, 0, 1), tmin 0, tmax 0.  Every number is finite and
 *             ordinary, and no root lies in the empty interval (0, 0): by the reference's own test tmin < t < tmax such a ray
 *             hits nothing, so a dead record answers -1 at every later step and nothing needs compacting.  In the ray library's
 *             query (csrc/pt_query.h) tmin = 0 keeps the lane on the filtered path, whose filter and grid walk do not read
 *             tmax for a closest-hit query: the lane walks the cells along +z from the origin (at most res_x + res_y + res_z + 3
 *             steps, its `guard`), every candidate's roots fail `t > 0 && t < 0`, and so does every plane's.  A terminating miss.
 *     pcg     2 uint64 planes: the generator after the record's draws (inc copied) -- pass them back in as they are.
 *             A record with status -1 draws nothing.
 *     then the fp64 planes selected by `channels`, an OR of PT_SCAT_WEIGHT | PT_SCAT_EMITTED, 3 planes each, in bit order;
 *     no hit: zeros.  A plane that is not selected costs no stores.  Unknown bits: PT_ERR_INVALID (pt_rays_scatter_bytes: 0).
 */
#ifndef PTRACE_SCATTER_H
#define PTRACE_SCATTER_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_SCAT_WEIGHT  1 /* 3 planes: hit_color after the roulette's compensation (what multiplies the child's radiance) */
#define PT_SCAT_EMITTED 2 /* 3 planes: material.emitted_radiance.get_color(uv)                                             */
#define PT_SCAT_ALL     3
/* selectors of pt_rays_scatter_plane_offset for the planes that are always written (NOT bits of `channels`) */
#define PT_SCAT_RAYS    4 /* component 0 .. 7: origin xyz, direction xyz, tmin, tmax */
#define PT_SCAT_PCG     8 /* component 0: state, 1: inc                               */

/* (major << 16) | minor of the ray library's interface this library implements: 1.2. */
int pt_rays_scatter_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_scatter_args_bytes(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_scatter_last_error(char *buf, size_t n);

/* Bytes of the output: 4 n rounded up to 8, + 80 n (rays, generator), + 24 n per selected channel. */
size_t pt_rays_scatter_bytes(long long n, int channels);
/* Byte offset of a plane in that buffer: `channel` 0 (the status plane), PT_SCAT_RAYS, PT_SCAT_PCG, PT_SCAT_WEIGHT or
 * PT_SCAT_EMITTED.  < 0: the channel is not selected (or no such channel / component / bad arguments). */
long long pt_rays_scatter_plane_offset(long long n, int channels, int channel, int component);

/* `roulette`: 0 or 1, for the whole batch. */
int pt_rays_scatter_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev, const int *shape_dev,
                           const double *point_dev, const double *normal_dev, const double *uv_dev, const double *dir_dev,
                           const unsigned long long *pcg_state_dev, const unsigned long long *pcg_inc_dev, long long n, int roulette,
                           int channels, void *out_dev, size_t out_bytes, void *stream);
/* The same for host buffers: stages through device memory it allocates and frees, builds the slot table itself.  Synchronous. */
int pt_rays_scatter(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host, const double *point_host,
                    const double *normal_host, const double *uv_host, const double *dir_host,
                    const unsigned long long *pcg_state_host, const unsigned long long *pcg_inc_host, long long n, int roulette,
                    int channels, void *out_host, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_SCATTER_H */
