/* ptrace_surface.h — C-ABI of libptrace_surface.so: the material and the point-light shading of a HitRecord, in batches.
 *
 * The second half of interface 1.1 of the ray library (ptrace_rays.h includes this header).  A renderer built on hit records
 * -- a hit-record frame of libptrace.so (pt_render_hits) or a closest-hit batch of libptrace_rays.so (pt_rays_trace) -- next
 * reads the hit's material and lights it.  The reference does that one Python object at a time:
 *     material.brdf.pigment.get_color(uv), material.emitted_radiance.get_color(uv)     materials.py:50-100
 *     PointLightRenderer.__call__                                                        render.py:157-193
 * Here both are answered for n records at once, with the arithmetic of the fused point-light renderer (csrc/pt_simple.h)
 * restated operation for operation: every value is the one the reference computes, bit for bit, for the record it is given.
 *
 * A THIRD shared object, not new symbols of libptrace_rays.so: that library's exported symbols are pinned to the seven of
 * interface 1.0, and libptrace.so's device code is pinned by every profiles/pmc_*.json.  Like libptrace_rays.so it links to
 * neither of the others, loads nothing, and gets the scene from its caller as the argument block of pt_scene_kernel_args
 * (ptrace.h, ABI 1.7); all three must come from one build of the tree, and a block of another size is refused.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never
 * throws, and checks every argument before its first HIP call.  n = 0: PT_OK, nothing launched, nothing written.  n < 0 or
 * n > 2^31 - 1: PT_ERR_INVALID.  The *_device forms are asynchronous on the caller's stream (a hipStream_t; NULL: the default
 * stream, and the call returns when the work is done) and allocate nothing.
 *
 * Layout: PLANAR, n values per plane, components x, y, z (u, v; r, g, b) one plane after the other -- the layout of both a
 * closest-hit batch and a hit-record frame, so a plane pointer into either buffer is passed as it is:
 *     shape   n int32   index into World.shapes, or anything outside [0, n_shapes) (-1) for "no hit"
 *     point   3 planes  HitRecord.world_point            normal  3 planes  HitRecord.normal
 *     uv      2 planes  HitRecord.surface_point          dir     3 planes  the direction of the ray that was traced
 * A record is the caller's: nothing about it is assumed (non-finite values give the reference's non-finite results; an image
 * pigment's column and row are clamped into the texture, NaN to 0).  One case the reference does not define -- it raises: a
 * checkered pigment whose u * steps (v * steps) is not finite.  The library's definition: such a cell counts as ODD where the
 * product is NaN and as EVEN where it is +-inf, so the answer is one of the pigment's two colours, never anything else (NaN
 * against a finite even cell: color2; NaN against NaN, +inf against -inf: color1).  Finite products of any size, negative ones
 * included, take the parity of Python's exact int(floor(.)) % 2.  tests/test_gpu_hostile_records.py pins all of this.
 *
 * Slot table.  The scene's records are grouped spheres-first; the shape plane holds World.shapes indices.  The table maps an
 * index to its record and is the caller's to keep: make it once per scene handle, it stays valid as long as the handle.
 */
#ifndef PTRACE_SURFACE_H
#define PTRACE_SURFACE_H

#include <stddef.h>

#include "ptrace.h" /* PT_BRDF_*, PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_SURF_BRDF_COLOR 1 /* 3 planes: material.brdf.pigment.get_color(uv)       */
#define PT_SURF_EMITTED    2 /* 3 planes: material.emitted_radiance.get_color(uv)   */
#define PT_SURF_ALL        3

/* (major << 16) | minor of the ray library's interface this library implements: 1.1, as pt_rays_version. */
int pt_rays_surface_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_surface_args_bytes(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_surface_last_error(char *buf, size_t n);

/* Bytes of the slot table of a scene: 4 * n_shapes rounded up to 8; 0 on a block the calls below refuse. */
size_t pt_rays_slots_bytes(const void *scene_args, size_t scene_args_bytes);
/* Fill it (one small kernel: slots[recs[s].index] = s).  slots_bytes < pt_rays_slots_bytes: PT_ERR_SIZE. */
int pt_rays_slots_device(int device, const void *scene_args, size_t scene_args_bytes, void *slots_dev, size_t slots_bytes,
                         void *stream);

/* Materials.  Output: an int32 plane of PT_BRDF_* kinds (-1: no hit), padded to a multiple of 8 bytes, then the fp64 planes
 * selected by `channels`, an OR of PT_SURF_*, in bit order.  No hit: zeros.  A plane that is not selected costs no stores;
 * channels = 0: uv_dev may be NULL.  Unknown bits: PT_ERR_INVALID (pt_rays_surface_bytes: 0). */
size_t pt_rays_surface_bytes(long long n, int channels);
/* Byte offset of a plane in that buffer: `channel` one of PT_SURF_* (0: the int32 plane), `component` 0 .. 2.
 * < 0: the channel is not selected (or no such channel / component / bad arguments). */
long long pt_rays_surface_plane_offset(long long n, int channels, int channel, int component);
int pt_rays_surface_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev,
                           const int *shape_dev, const double *uv_dev, long long n, int channels, void *out_dev,
                           size_t out_bytes, void *stream);
/* The same for host buffers: stages through device memory it allocates and frees, builds the slot table itself.  Synchronous. */
int pt_rays_surface(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host, const double *uv_host,
                    long long n, int channels, void *out_host, size_t out_bytes);

/* Lights.  Output: three fp64 planes (24 n bytes), PointLightRenderer.__call__ (render.py:157-193) for a ray of direction
 * `dir` whose HitRecord is the given one: no hit -> `background`; else `ambient` + emitted, then one addition per light that
 * World.is_point_visible (world.py:71-80) sees from the hit point, in the scene's light order.  `ambient` and `background`
 * are three doubles each, on the host, read before the call returns. */
int pt_rays_shade_lights_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev,
                                const int *shape_dev, const double *point_dev, const double *normal_dev, const double *uv_dev,
                                const double *dir_dev, long long n, const double *ambient, const double *background,
                                void *out_dev, size_t out_bytes, void *stream);
int pt_rays_shade_lights(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host,
                         const double *point_host, const double *normal_host, const double *uv_host, const double *dir_host,
                         long long n, const double *ambient, const double *background, void *out_host, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_SURFACE_H */
