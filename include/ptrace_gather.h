/* ptrace_gather.h — C-ABI of libptrace_gather.so: the mean radiance arriving over the hemisphere of batches of surface points.
 *
 * Interface 1.4 of the ray library, its sixth step: a GATHER QUERY.  The steps before it -- trace (ptrace_rays.h), material
 * (ptrace_surface.h), scatter (ptrace_scatter.h), radiance (ptrace_radiance.h) -- leave the caller of an irradiance probe or a
 * light-map texel to build n * K rays and n * K generators on the host and to average on the host.  This one takes n records
 * (a world point p_i and a normal n_i) and K = `samples` and returns, per record,
 *     g_ik   = PCG(init_state, seq_i + k)                                        (pcg.py:25-41; 64-bit wrap)
 *     ray_ik = DiffuseBRDF.scatter_ray(g_ik, ., p_i, n_i, depth0)                (materials.py:132-152: two draws, tmin 1e-3, tmax inf)
 *     L_ik   = PathTracer(world, background, g_ik, num_of_rays, max_depth, russian_roulette_limit)(ray_ik)    (render.py:99-139)
 *     out_i  = (((0 + L_i0) + L_i1) + ... + L_i,K-1) * (1.0 / K)                 per channel, STRICTLY in k order
 *     count_i = sum over k of the rays handed to a world query for sample k      (uint64; it wraps)
 * Every sample runs on a lane of its own (sample j = i * K + k; a wave takes 64 consecutive j, which mostly share an origin), with
 * the fused path tracer's device functions (pcg_seed, scatter_ray with its inlined sincos, world_query_lanes, hit_details,
 * pcg_float), so L_ik is what ptrace_scatter.h followed by ptrace_radiance.h return for that record and that generator, bit for
 * bit.  The mean is taken on the device by a second launch on the same stream, one lane per record adding its K values in k
 * order: the result is a pure function of the inputs -- no floating-point atomics, no order that depends on scheduling, on n,
 * on K or on the launch's shape.  Nothing of size n * K crosses the host link or is supplied by the caller.
 *
 * Cases spelled out:
 *   - the normal is used exactly as ptrace_scatter.h uses a record's `normal`: nothing is normalised, flipped or checked.
 *   - depth0 > max_depth: every result is black (0, 0, 0) and every count is 0.
 *   - `active` (int32 per record, or NULL: every record is active): a record with a NEGATIVE value is skipped -- radiance 0,
 *     count 0 -- so the shape_index plane of a ray batch or of a hit frame can be passed as it is.
 *   - `seq` (uint64 per record, or NULL): the stream number of the record's sample 0.  NULL: seq_i = init_seq + i * K, which
 *     keeps all n * K streams disjoint.
 *   - every value in points and normals is legal, NaN and infinity included: the walk ends by integer counters alone, and a
 *     sample whose ray is NaN hits nothing and returns the background.
 *
 * A SIXTH shared object, for the reasons the fifth one gives: the other libraries' exported symbols and libptrace.so's device
 * code are pinned.  Like them it links to none of the others, loads nothing, and gets the scene from its caller as the argument
 * block of pt_scene_kernel_args (ptrace.h, ABI 1.7); all six must come from one build of the tree, a block of another size is
 * refused.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never
 * throws, and checks every argument before its first HIP call.  n = 0: PT_OK, nothing launched, nothing written.  samples < 1,
 * num_of_rays < 1, n < 0, n * samples > 2^31 - 1, max_depth < 0, depth0 < 0, unknown channel bits: PT_ERR_INVALID.
 * max_depth - depth0 > 64: PT_ERR_UNSUPPORTED.  An output or a workspace that is too small: PT_ERR_SIZE.  The *_device form is
 * asynchronous on the caller's stream (a hipStream_t; NULL: the default stream, and the call returns when the work is done) and
 * allocates nothing.
 *
 * Input: PLANAR points [3, n] and normals [3, n] (n doubles per plane), the optional planes `active` (n int32) and `seq`
 * (n uint64).
 *
 * Workspace: pt_rays_gather_workspace_bytes(device, n, samples, num_of_rays, max_depth, depth0) bytes of device memory, in two
 * parts.  The node stacks, planar [level][field][lane], sized by the lanes one launch keeps resident and not by n * K (compute
 * units x resident workgroups x 256, lowered to PTRACE_GATHER_LANES where that environment variable names a smaller number;
 * rounded down to a multiple of 256, at least 256; read at every call): a wave takes its next 64 samples when its 64 are done.
 * Behind them the sample planes, [4][n * K] of 8 bytes (L_ik r, g, b and the sample's count): the walk writes them coalesced,
 * the mean reads them.  The contents are scratch; two calls that may overlap need a workspace each.
 *
 * Output: one buffer of pt_rays_gather_bytes(n, channels) bytes, planar, 8-byte planes of n values, in this order:
 *     radiance         3 fp64 planes (r, g, b), always written
 *     PT_GATHER_COUNT  1 uint64 plane: count_i
 * `channels` is 0 or PT_GATHER_COUNT.  A plane that is not selected costs no stores.  Unknown bits: PT_ERR_INVALID
 * (pt_rays_gather_bytes: 0).
 */
#ifndef PTRACE_GATHER_H
#define PTRACE_GATHER_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_GATHER_COUNT 1 /* 1 plane: rays traced per record (uint64) */
#define PT_GATHER_ALL   1

#define PT_GATHER_MAX_LEVELS 64 /* max_depth - depth0 at most */

typedef struct pt_gather_params {
  int samples;                   /* K >= 1: samples per record                                               */
  int num_of_rays;               /* >= 1                                                                     */
  int max_depth;                 /* >= 0                                                                     */
  int rr_limit;                  /* russian_roulette_limit: any value (<= depth0: the roulette at every hit) */
  int depth0;                    /* Ray.depth of the hemisphere's rays, one value for the batch, >= 0        */
  unsigned long long init_state; /* PCG(init_state, .)                                                       */
  unsigned long long init_seq;   /* with seq = NULL: record i's sample k draws from stream init_seq + i K + k */
  double background[3];          /* the renderer's background_color                                          */
} pt_gather_params;

/* (major << 16) | minor of the ray library's interface this library implements: 1.4. */
int pt_rays_gather_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_gather_args_bytes(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_gather_last_error(char *buf, size_t n);

/* Bytes of the output: 24 n, + 8 n with PT_GATHER_COUNT. */
size_t pt_rays_gather_bytes(long long n, int channels);
/* Byte offset of a plane in that buffer: `channel` 0 (radiance; component 0 .. 2) or PT_GATHER_COUNT (0).  < 0: the channel is
 * not selected (or no such channel / component / bad arguments). */
long long pt_rays_gather_plane_offset(long long n, int channels, int channel, int component);
/* Bytes of the workspace a batch of n records needs on `device` (never 0 for arguments the library accepts; 0 on refusal, with
 * the reason in pt_rays_gather_last_error). */
size_t pt_rays_gather_workspace_bytes(int device, long long n, int samples, int num_of_rays, int max_depth, int depth0);

int pt_rays_gather_device(int device, const void *scene_args, size_t scene_args_bytes, const double *points_dev, const double *normals_dev,
                          const int *active_dev, const unsigned long long *seq_dev, long long n, const pt_gather_params *params,
                          int channels, void *workspace_dev, size_t workspace_bytes, void *out_dev, size_t out_bytes, void *stream);
/* The same for host buffers: stages through device memory it allocates and frees, the workspace included.  Synchronous. */
int pt_rays_gather(int device, const void *scene_args, size_t scene_args_bytes, const double *points_host, const double *normals_host,
                   const int *active_host, const unsigned long long *seq_host, long long n, const pt_gather_params *params, int channels,
                   void *out_host, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_GATHER_H */
