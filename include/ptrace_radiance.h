/* ptrace_radiance.h — C-ABI of libptrace_radiance.so: PathTracer.__call__(ray) for batches of a caller's own rays.
 *
 * Interface 1.3 of the ray library, its fifth step: a RADIANCE QUERY.  The steps before it -- trace (ptrace_rays.h), material
 * (ptrace_surface.h), scatter (ptrace_scatter.h) -- give one bounce of the reference's PathTracer; this one gives the whole
 * recursion (render.py:99-139): for n rays, each with a generator of its own,
 *     out[i] = PathTracer(world, background, pcg_i, num_of_rays, max_depth, russian_roulette_limit)(ray_i)
 * with ray_i.depth = depth0.  Every ray is walked depth-first on the device, in the reference's order of draws, and nothing
 * returns to the host in between.  The device functions are the fused path tracer's (world_query_lanes, hit_details,
 * scatter_ray with its inlined sincos, pcg_float: csrc/pt_query.h, pt_shade.h, pt_math.h), so every value is the one the fused
 * kernels compute for that ray and that generator, bit for bit.  Per node, as the reference orders it:
 *     no hit: background.  hit_color, emitted, lum = max(r, g, b) of hit_color.
 *     depth >= russian_roulette_limit: q = max(0.05, 1 - lum), ONE draw; draw > q: hit_color *= 1.0 / (1.0 - q); else: emitted.
 *     lum > 0: num_of_rays times brdf.scatter_ray (TWO draws on a DiffuseBRDF, none on a SpecularBRDF), the child's radiance,
 *              cum = cum + hit_color * child, in child order.
 *     emitted + cum * (1.0 / num_of_rays).
 * Three cases spelled out:
 *   - depth0 > max_depth: every result is black (0, 0, 0); no query is made, no draw is taken, the count is 0.
 *   - a hit at exactly max_depth with lum > 0 still calls scatter_ray num_of_rays times: the draws are consumed (the generator
 *     returned for that ray shows them), the children are black without a query and are not counted.
 *   - an entry ray with tmin < 0 (or NaN tmin) is answered by the exhaustive query of ptrace_rays.h (roots at t <= 0 count, as
 *     the reference's test tmin < t < tmax has it); scattered rays never need it.
 * The walk ends by integer counters alone (depth, children left): a ray of NaNs hits nothing and returns the background.
 *
 * A FIFTH shared object, for the reasons the fourth one gives: the other four libraries' exported symbols and libptrace.so's
 * device code are pinned.  Like them it links to none of the others, loads nothing, and gets the scene from its caller as the
 * argument block of pt_scene_kernel_args (ptrace.h, ABI 1.7); all five must come from one build of the tree, a block of another
 * size is refused.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never
 * throws, and checks every argument before its first HIP call.  n = 0: PT_OK, nothing launched, nothing written.  n < 0 or
 * n > 2^31 - 1: PT_ERR_INVALID.  max_depth - depth0 > 64: PT_ERR_UNSUPPORTED (the fused renderer, pt_render of ptrace.h, takes
 * max_depth up to 4096).  The *_device form is asynchronous on the caller's stream (a hipStream_t; NULL: the default stream,
 * and the call returns when the work is done) and allocates nothing.
 *
 * Input: the PLANAR [8, n] block pt_rays_trace_device reads (origin xyz, direction xyz, tmin, tmax; n doubles per plane) and two
 * planes of n uint64: state and inc of every ray's generator (PCG-XSH-RR 64/32, pcg.py: `state` and `inc` as the class keeps
 * them).  Every value is legal, in the rays (non-finite ones included) and in the generators (an even inc included).
 *
 * Workspace: the node stacks, pt_rays_radiance_workspace_bytes(device, n, num_of_rays, max_depth, depth0) bytes of device
 * memory, planar [level][field][lane].  It is sized by the lanes one launch keeps resident, not by n: a launch of at most L
 * lanes walks all n rays, a wave taking its next 64 rays when its 64 are done.  L is what the device holds of the kernel
 * (compute units x resident workgroups x 256), lowered to PTRACE_RADIANCE_LANES where that environment variable names a
 * smaller number (rounded down to a multiple of 256, at least 256; read at every call).  The contents are scratch: nothing is
 * expected in it, nothing of use is left in it, and two calls that may overlap need a workspace each.
 *
 * Output: one buffer of pt_rays_radiance_bytes(n, channels) bytes, planar, 8-byte planes of n values, in this order:
 *     radiance      3 fp64 planes (r, g, b), always written
 *     PT_RAD_PCG    2 uint64 planes: the generator's state after the ray's draws; inc, copied
 *     PT_RAD_COUNT  1 uint64 plane: the rays handed to a world query for this ray (the entry ray and every scattered ray at
 *                   depth <= max_depth) -- what the reference's renderers count as rays traced.  It wraps.
 * `channels` is an OR of PT_RAD_PCG | PT_RAD_COUNT.  A plane that is not selected costs no stores.  Unknown bits:
 * PT_ERR_INVALID (pt_rays_radiance_bytes: 0).
 */
#ifndef PTRACE_RADIANCE_H
#define PTRACE_RADIANCE_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_RAD_PCG   1 /* 2 planes: state, inc          */
#define PT_RAD_COUNT 2 /* 1 plane: rays traced (uint64) */
#define PT_RAD_ALL   3

#define PT_RAD_MAX_LEVELS 64 /* max_depth - depth0 at most */

typedef struct pt_radiance_params {
  int num_of_rays;      /* >= 1                                                                     */
  int max_depth;        /* >= 0                                                                     */
  int rr_limit;         /* russian_roulette_limit: any value (<= depth0: the roulette at every hit) */
  int depth0;           /* Ray.depth of the entry rays, one value for the batch, >= 0               */
  double background[3]; /* the renderer's background_color                                          */
} pt_radiance_params;

/* (major << 16) | minor of the ray library's interface this library implements: 1.3. */
int pt_rays_radiance_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_radiance_args_bytes(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_radiance_last_error(char *buf, size_t n);

/* Bytes of the output: 24 n, + 16 n with PT_RAD_PCG, + 8 n with PT_RAD_COUNT. */
size_t pt_rays_radiance_bytes(long long n, int channels);
/* Byte offset of a plane in that buffer: `channel` 0 (radiance; component 0 .. 2), PT_RAD_PCG (0: state, 1: inc) or
 * PT_RAD_COUNT (0).  < 0: the channel is not selected (or no such channel / component / bad arguments). */
long long pt_rays_radiance_plane_offset(long long n, int channels, int channel, int component);
/* Bytes of the workspace a batch of n rays needs on `device` (never 0 for arguments the library accepts; 0 on refusal, with
 * the reason in pt_rays_radiance_last_error). */
size_t pt_rays_radiance_workspace_bytes(int device, long long n, int num_of_rays, int max_depth, int depth0);

/* `slots_dev`: the slot table of pt_rays_slots_device (ptrace_surface.h), for symmetry with the other steps' device forms.
 * The walk gets its record slots from its own queries and does not read the table: NULL is accepted. */
int pt_rays_radiance_device(int device, const void *scene_args, size_t scene_args_bytes, const void *slots_dev, const double *rays_dev,
                            const unsigned long long *pcg_state_dev, const unsigned long long *pcg_inc_dev, long long n,
                            const pt_radiance_params *params, int channels, void *workspace_dev, size_t workspace_bytes, void *out_dev,
                            size_t out_bytes, void *stream);
/* The same for host buffers: stages through device memory it allocates and frees, the workspace included.  Synchronous. */
int pt_rays_radiance(int device, const void *scene_args, size_t scene_args_bytes, const double *rays_host,
                     const unsigned long long *pcg_state_host, const unsigned long long *pcg_inc_host, long long n,
                     const pt_radiance_params *params, int channels, void *out_host, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_RADIANCE_H */
