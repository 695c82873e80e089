/* ptrace_adaptive.h — C-ABI of libptrace_adaptive.so: sample counts from a variance plane, their prefix sum, and a gather whose
 * sample count is a plane -- on the device.
 *
 * Interface 1.11 of the ray library, its thirteenth step: an ADAPTIVE QUERY.  The twelfth step (ptrace_variance.h) measures, per
 * pixel, how noisy the accumulated estimate still is; the sixth (ptrace_gather.h) takes ONE `samples` for a whole batch.  This
 * step lets the measurement decide where the rays go.  Three queries:
 *     COUNTS   a variance plane, the estimate whose variance it is and a tolerance -> a sample-count plane
 *     OFFSETS  the exclusive prefix sum of a count plane: where every record's samples start, and the total
 *     GATHER   the gather query of ptrace_gather.h with `samples` replaced by those two planes: a RAGGED gather
 *
 * 1. COUNTS, per pixel p of m.  fp64, only + - * / and comparisons, every operation rounded on its own (no contraction), so that
 * pytracer_amd.rays.sample_counts_host matches the device bit for bit.  lum(c) is ptrace_variance.h's:
 *     lum(c)   mx = c0; if (c1 > mx) mx = c1; if (c2 > mx) mx = c2;  mn = c0; if (c1 < mn) mn = c1; if (c2 < mn) mn = c2;
 *              lum = (mx + mn) / 2.0
 *     shape[p] < 0:                       counts = 0
 *     v = variance[p];  l = lum(colour_p);  if (!(l > luminance_floor)) l = luminance_floor
 *     tl = tolerance * l;  want = (gain * v) / (tl * tl)
 *     !(v >= 0) (negative, NaN):          counts = max_samples        (unknown counts as noisy)
 *     !(want < (double)max_samples):      counts = max_samples        (+inf and NaN land here)
 *     else  t = (long long)want;  k = t + ((double)t < want ? 1 : 0)  (ceil by truncation; want >= 0 here)
 *           if (k < min_samples) k = min_samples;   counts = (int)k
 * The count is the variance over the squared relative tolerance, times `gain`, clamped: `gain` is the caller's handle on the
 * total.  Input: `variance` fp64 [m], `colour` planar fp64 [3, m], `shape` int32 [m].  Output: `counts` int32 [m].  One launch,
 * one pixel per lane.
 *
 * 2. OFFSETS.  offsets[0] = 0, offsets[i + 1] = offsets[i] + max(counts[i], 0), in int64: n + 1 values, offsets[n] is the total
 * -- what a caller reads back, once, if it wants to size the workspace exactly, and the ray budget of the frame.  Integer
 * arithmetic: the result does not depend on the launch.  Three launches on the caller's stream (reduce, then scan): the sums of
 * workgroups of 256 counts; the scan of those sums by one workgroup; the scan of every workgroup's counts on top of its sum's
 * prefix.  No workgroup waits for another within a launch.  Workspace: pt_rays_adaptive_offsets_workspace_bytes(n) = 8 bytes per
 * 256 counts (at least 8).  n = 0: PT_OK, nothing launched, nothing written.
 *
 * 3. GATHER.  n records (a world point p_i and a normal n_i, as in ptrace_gather.h), `counts` int32 [n], `offsets` int64 [n + 1]
 * of query 2, and `capacity`, the number of samples the workspace's sample planes hold:
 *     K_i    = min(max(counts[i], 0), max(capacity - offsets[i], 0))             SAMPLES TAKEN: a batch whose total exceeds
 *              `capacity` is truncated in record order -- a defined, pure function of the inputs, the caller's hard ray budget
 *     j      = offsets[i] + k, k < K_i                                           the sample's place in the sample planes
 *     seq_i  = seq[i], or with seq = NULL: init_seq + offsets[i]                 (disjoint streams; 64-bit wrap)
 *     g_ik   = PCG(init_state, seq_i + k)
 *     L_ik   = exactly what the gather query computes for record i and that generator (scatter_ray at (p_i, n_i), depth0, then
 *              PathTracer(world, background, g_ik, num_of_rays, max_depth, russian_roulette_limit))
 *     out_i  = (((0 + L_i0) + L_i1) + ... + L_i,K_i-1) * (1.0 / (double)K_i)     per channel, STRICTLY in k order
 *     count_i = sum over k < K_i of the rays handed to a world query, in the same order (uint64; it wraps)
 *     K_i = 0:  radiance (0, 0, 0), count 0.
 * THE CONTRACT: for every record, radiance and count are BIT FOR BIT what the gather query of ptrace_gather.h returns for that
 * record alone with samples = K_i and seq = seq_i.  No bit depends on the other records' counts, on n, on capacity beyond K_i or
 * on the launch's shape.
 *
 * Cases spelled out:
 *   - `active` (int32 per record, or NULL): a record with a NEGATIVE value is skipped -- radiance 0, count 0, taken 0 -- as in the
 *     gather.  Its samples keep their places: offsets come from counts alone.
 *   - every value in points and normals is legal, NaN and infinity included: the walk ends by integer counters alone.
 *   - depth0 > max_depth: every radiance is black and every count is 0; `taken` is still K_i.
 *   - a GARBAGE `offsets` plane (not the prefix sum of `counts`) is the caller's own doing: results are then undefined, but no
 *     store leaves the buffers.  The walk's and the expand launch's sample index j runs below min(offsets[n], capacity) and is
 *     never formed from an offset; a record found for j is clamped into [0, n); the mean reads addresses offsets[i] + k only where 0 <= offsets[i]
 *     and k < K_i <= capacity - offsets[i].  So every sample address lies in [0, capacity).
 *
 * WORK LAYOUT is the gather's: a wave takes the 64 consecutive samples [base, base + 64) and then the next 64 no other wave of
 * the launch takes; the node stacks are sized by the lanes a launch keeps resident (PTRACE_ADAPTIVE_LANES lowers that number,
 * as PTRACE_GATHER_LANES does for the gather; read at every call).  A lane finds (i, k) from j through an OWNER PLANE: a small
 * expand launch in front of the walk writes owner[j] (int32) into the workspace, by searching `offsets` for the upper bound (a
 * wave together for its first and last sample, then every lane in between).  PTRACE_ADAPTIVE_LOOKUP=search lets the walk do that
 * search itself, without the plane: the same bits, measured 1 % slower (profiles/adaptive_kernel.txt).  The mean is a launch
 * behind the walk, one record per lane, tiles staged through LDS; its trip count is the workgroup's largest K_i.
 *
 * Workspace: pt_rays_adaptive_workspace_bytes(device, n, capacity, num_of_rays, max_depth, depth0): the node stacks, planar
 * [level][field][lane], behind them the sample planes [4][capacity] of 8 bytes (L r, g, b and the sample's count), and behind
 * those the owner plane, up8(4 capacity) bytes (not with PTRACE_ADAPTIVE_LOOKUP=search).  Scratch.
 *
 * Output: one buffer of pt_rays_adaptive_bytes(n, channels) bytes, planar, every plane starting on 8 bytes, in this order:
 *     radiance            3 fp64 planes of n (r, g, b), always written          offset 8 n c
 *     PT_ADAPTIVE_COUNT   1 uint64 plane of n: count_i                          offset 24 n
 *     PT_ADAPTIVE_TAKEN   1 int32 plane of n: K_i, PADDED to up8(4 n) bytes     offset 24 n (+ 8 n with PT_ADAPTIVE_COUNT)
 * A plane that is not selected costs no stores and no bytes.  up8(x) = (x + 7) & ~7; the padding is not written.
 *
 * A THIRTEENTH shared object, for the reasons the twelve before it give.  It links to none of the others, loads nothing, and gets
 * the scene from its caller as the argument block of pt_scene_kernel_args (ptrace.h, ABI 1.7); a block of another size is refused.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never
 * throws, and checks every argument before its first HIP call.  The *_device forms are asynchronous on the caller's stream (a
 * hipStream_t; NULL: the default stream, and the call returns when the work is done), allocate nothing and make no host round
 * trip.  The forms without `_device` take host buffers, stage them through device memory they allocate and free (workspace
 * included) and are synchronous.  REFUSALS:
 *     counts: m < 0 or > 2^31 - 1; a NULL struct; min_samples < 0, max_samples < min_samples, max_samples > 2^20; a tolerance
 *     that is not > 0 (NaN included; +inf is legal); a luminance_floor or a gain that is not finite and > 0; NULL planes  PT_ERR_INVALID
 *     offsets: n < 0 or > 2^31 - 1; NULL planes or workspace                                                             PT_ERR_INVALID
 *     gather: as the gather query's (num_of_rays < 1, n < 0 or > 2^31 - 1, max_depth < 0, depth0 < 0, unknown channel bits, NULL
 *     planes), and capacity < 0 or > 2^31 - 1, NULL counts or offsets                                                    PT_ERR_INVALID
 *     max_depth - depth0 > 64                                                                                            PT_ERR_UNSUPPORTED
 *     an output or a workspace that is too small                                                                         PT_ERR_SIZE
 * m = 0 / n = 0 is PT_OK with nothing launched and nothing written (the struct is still checked).
 */
#ifndef PTRACE_ADAPTIVE_H
#define PTRACE_ADAPTIVE_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ADAPTIVE_COUNT 1 /* 1 plane: rays traced per record (uint64) */
#define PT_ADAPTIVE_TAKEN 2 /* 1 plane: samples taken per record, K_i (int32, padded to 8 bytes) */
#define PT_ADAPTIVE_ALL   3

#define PT_ADAPTIVE_MAX_LEVELS 64       /* max_depth - depth0 at most */
#define PT_ADAPTIVE_MAX_SAMPLES 1048576 /* 2^20: max_samples at most */

typedef struct pt_adaptive_count_params {
  int min_samples;        /* 0 <= min_samples <= max_samples                                   */
  int max_samples;        /* <= 2^20                                                           */
  double tolerance;       /* > 0 (or +inf): the relative standard error aimed at               */
  double luminance_floor; /* finite, > 0: the least luminance the tolerance is relative to     */
  double gain;            /* finite, > 0: scales every count; the caller's handle on the total */
} pt_adaptive_count_params;

/* pt_gather_params of ptrace_gather.h without `samples`, plus `capacity` */
typedef struct pt_adaptive_params {
  int num_of_rays;               /* >= 1                                                                     */
  int max_depth;                 /* >= 0                                                                     */
  int rr_limit;                  /* russian_roulette_limit: any value (<= depth0: the roulette at every hit) */
  int depth0;                    /* Ray.depth of the hemisphere's rays, one value for the batch, >= 0        */
  unsigned long long init_state; /* PCG(init_state, .)                                                       */
  unsigned long long init_seq;   /* with seq = NULL: record i's sample k draws from stream init_seq + offsets[i] + k */
  double background[3];          /* the renderer's background_color                                          */
  long long capacity;            /* 0 .. 2^31 - 1: samples the workspace's sample planes hold                */
} pt_adaptive_params;

/* (major << 16) | minor of the ray library's interface this library implements: 1.11. */
int pt_rays_adaptive_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_adaptive_args_bytes(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_adaptive_last_error(char *buf, size_t n);

/* Bytes of the gather's output: 24 n, + 8 n with PT_ADAPTIVE_COUNT, + up8(4 n) with PT_ADAPTIVE_TAKEN. */
size_t pt_rays_adaptive_bytes(long long n, int channels);
/* Byte offset of a plane in that buffer: `channel` 0 (radiance; component 0 .. 2), PT_ADAPTIVE_COUNT (0) or PT_ADAPTIVE_TAKEN
 * (0).  < 0: the channel is not selected (or no such channel / component / bad arguments). */
long long pt_rays_adaptive_plane_offset(long long n, int channels, int channel, int component);
/* Bytes of an offsets plane: 8 (n + 1) (0 on refusal). */
size_t pt_rays_adaptive_offsets_bytes(long long n);
/* Bytes of the workspace of pt_rays_adaptive_offsets_device: 8 per 256 counts, at least 8 (0 on refusal). */
size_t pt_rays_adaptive_offsets_workspace_bytes(long long n);
/* Bytes of the workspace of pt_rays_adaptive_gather_device on `device` (never 0 for arguments the library accepts; 0 on refusal,
 * with the reason in pt_rays_adaptive_last_error). */
size_t pt_rays_adaptive_workspace_bytes(int device, long long n, long long capacity, int num_of_rays, int max_depth, int depth0);

int pt_rays_adaptive_counts_device(int device, long long m, const pt_adaptive_count_params *params, const double *variance_dev,
                                   const double *colour_dev, const int *shape_dev, int *counts_dev, size_t counts_bytes, void *stream);
int pt_rays_adaptive_offsets_device(int device, long long n, const int *counts_dev, long long *offsets_dev, size_t offsets_bytes,
                                    void *workspace_dev, size_t workspace_bytes, void *stream);
int pt_rays_adaptive_gather_device(int device, const void *scene_args, size_t scene_args_bytes, const double *points_dev,
                                   const double *normals_dev, const int *active_dev, const unsigned long long *seq_dev, const int *counts_dev,
                                   const long long *offsets_dev, long long n, const pt_adaptive_params *params, int channels,
                                   void *workspace_dev, size_t workspace_bytes, void *out_dev, size_t out_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_adaptive_counts(int device, long long m, const pt_adaptive_count_params *params, const double *variance_host,
                            const double *colour_host, const int *shape_host, int *counts_host, size_t counts_bytes);
int pt_rays_adaptive_offsets(int device, long long n, const int *counts_host, long long *offsets_host, size_t offsets_bytes);
int pt_rays_adaptive_gather(int device, const void *scene_args, size_t scene_args_bytes, const double *points_host, const double *normals_host,
                            const int *active_host, const unsigned long long *seq_host, const int *counts_host, const long long *offsets_host,
                            long long n, const pt_adaptive_params *params, int channels, void *out_host, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_ADAPTIVE_H */
