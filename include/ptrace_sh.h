/* ptrace_sh.h — C-ABI of libptrace_sh.so: order-2 spherical-harmonic (SH) radiance probes at free points of the world.
 *
 * Interface 1.6 of the ray library, its eighth step: a PROBE QUERY.  The gather query (ptrace_gather.h) needs a normal and the
 * bake query (ptrace_bake.h) a shape with a (u, v) grid; a probe needs neither.  It is a world point x, and its answer is 27
 * numbers: the coefficients of the radiance arriving at x from every direction, in the nine real SH functions of bands 0 - 2,
 * per colour channel.  The cosine-weighted hemisphere mean for ANY normal follows from them without a new ray -- the quantity a
 * gather record or a light-map texel holds.
 *
 * DIRECTION  D(g) for a generator g, two draws -- uniform on the sphere, pdf 1 / (4 pi):
 *     u1 = g.random_float();  u2 = g.random_float()                                   (pcg.py:60-62)
 *     z  = 1.0 - 2.0 * u1;    r = sqrt(1.0 - z * z);   ph = (2.0 * pi) * u2           (|z| <= 1: the root's argument is >= 0)
 *     d  = (r * cos ph, r * sin ph, z)                 (one sincos, the function scatter_ray and the bake use)
 *
 * BASIS  the nine real SH functions of bands 0 - 2 as polynomials in a direction (x, y, z) that the library does NOT normalise.
 * Each constant is ONE fp64 literal, and the products are taken in this order:
 *     Y0 = 0.28209479177387814                                   sqrt(1 / 4 pi)
 *     Y1 = 0.4886025119029199 * y                                sqrt(3 / 4 pi)
 *     Y2 = 0.4886025119029199 * z
 *     Y3 = 0.4886025119029199 * x
 *     Y4 = 1.0925484305920792 * (x * y)                          sqrt(15 / 4 pi)
 *     Y5 = 1.0925484305920792 * (y * z)
 *     Y6 = 0.31539156525252005 * (3.0 * (z * z) - 1.0)           sqrt(5 / 16 pi)
 *     Y7 = 1.0925484305920792 * (x * z)
 *     Y8 = 0.5462742152960396 * (x * x - y * y)                  sqrt(15 / 16 pi)
 * The literals, not the expressions beside them, define the bits.
 *
 * PROJECTION of n probes at K samples.  Probe i is a world point x_i; sample k draws from stream seq_i + k:
 *     g      = PCG(init_state, seq_i + k)                                               (pcg.py:25-41; 64-bit wrap)
 *     d_ik   = D(g)
 *     ray    = Ray(origin = x_i, dir = d_ik, tmin = 1e-5, tmax = inf, depth = depth0)   (ray.py's defaults)
 *     L_ik   = PathTracer(world, background, g, num_of_rays, max_depth, rr_limit)(ray)  (render.py:99-139)
 *     c_i[j][ch] = ((((0 + Y_j(d_i0) * L_i0[ch]) + Y_j(d_i1) * L_i1[ch]) + ... ) * ((4.0 * pi) * (1.0 / K))
 *                  STRICTLY in k order, j = 0 .. 8, ch = r, g, b
 *     count_i    = sum over k of the rays handed to a world query                       (uint64; it wraps)
 * seq_i comes from the optional `seqs` plane (uint64[n]); NULL: seq_i = init_seq + i K, as in the gather.  The optional `active`
 * plane (int32[n], negative = skipped) gives coefficients 0 and count 0 for a skipped probe.  Every sample runs on a lane of its
 * own (j = i K + k) through the radiance query's walk; the projection is a second launch on the same stream, one lane per probe:
 * no atomics, nothing that depends on scheduling, on n, on K or on the launch's shape.
 *
 * EVALUATION of m records (probe index p_r, direction n_r) against a coefficient block [27][n]:
 *     out_r[ch] = (((0 + (A_0 * Y_0(n_r)) * c_p[0][ch]) + (A_1 * Y_1(n_r)) * c_p[1][ch]) + ... + (A_8 * Y_8(n_r)) * c_p[8][ch])
 *     PT_SH_RADIANCE:    A_j = 1.0                                     -> the band-limited L(n_r)
 *     PT_SH_HEMISPHERE:  A_0 = 1.0, A_1..3 = 2.0 / 3.0, A_4..8 = 0.25  -> (1 / pi) * integral of L cos over n_r's hemisphere
 * PT_SH_HEMISPHERE is the quantity a gather record or a light-map texel holds (render.py:128-139, materials.py:132-152).  The
 * index plane (int32[m]) may be NULL: record r then reads probe r, and m <= n is required.  An index outside [0, n) gives zeros.
 * There is no scene and no ray here; the coefficient block may be one the caller blended from several probes.
 *
 * DIRECTIONS as a query of its own: pt_rays_sh_directions returns d_ik for (init_state, seqs | init_seq, n, K), planar [3][n K],
 * sample j = i K + k, by the device function the projection's walk uses: the device's own bits, for a test or for a caller who
 * wants the samples.  Of `params` it reads samples, init_state and init_seq (and checks the rest).
 *
 * An EIGHTH shared object, for the reasons the sixth and the seventh give.  It links to none of the others, loads nothing, and
 * gets the scene as the argument block of pt_scene_kernel_args (ptrace.h, ABI 1.7); all eight must come from one build of the tree.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never
 * throws, and checks every argument before its first HIP call:
 *     n K > 2^31 - 1; K, num_of_rays < 1; max_depth < 0; depth0 < 0; unknown channel bits or an unknown kind; n or m < 0 or
 *     > 2^31 - 1; NULL where a buffer is needed; m > n with a NULL index                                 PT_ERR_INVALID
 *     max_depth - depth0 > 64                                                                            PT_ERR_UNSUPPORTED
 *     an output or a workspace that is too small                                                         PT_ERR_SIZE
 * n = 0 and m = 0 are PT_OK with nothing launched.  The *_device forms are asynchronous on the caller's stream (a hipStream_t;
 * NULL: the default stream, and the call returns when the work is done) and allocate nothing.
 *
 * Projection workspace: pt_rays_sh_workspace_bytes(device, n, params) bytes of device memory: the node stacks, planar
 * [level][field][lane], sized by the lanes one launch keeps resident (lowered to PTRACE_SH_LANES where that environment
 * variable names a smaller number; a multiple of 256, at least 256; read at every call), then the sample planes [7][n K] of 8
 * bytes: L r, g, b, the count, d x, y, z.  The contents are scratch; two calls that may overlap need a workspace each.
 *
 * Projection input: `points` planar [3, n] fp64.  Output: pt_rays_sh_bytes(n, channels) bytes, planar, 8-byte planes of n values:
 *     coefficients   27 fp64 planes, plane 3 j + ch, always written
 *     PT_SH_COUNT    1 uint64 plane: count_i
 * A plane that is not selected costs no stores.
 *
 * Evaluation input: `coeffs` [27][n] fp64 (the first 216 n bytes of a projection's output), `index` int32[m] or NULL, `dirs`
 * planar [3, m] fp64.  Output: planar [3, m] fp64, pt_rays_sh_eval_bytes(m) = 24 m bytes.
 */
#ifndef PTRACE_SH_H
#define PTRACE_SH_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_SH_COUNT 1 /* 1 plane: rays traced per probe (uint64) */
#define PT_SH_ALL   1

#define PT_SH_RADIANCE   0 /* evaluation kinds */
#define PT_SH_HEMISPHERE 1

#define PT_SH_COEFFS 27     /* planes of coefficients: 9 functions x 3 channels */
#define PT_SH_MAX_LEVELS 64 /* max_depth - depth0 at most */

typedef struct pt_sh_params {
  int samples;                   /* K >= 1: samples per probe                                 */
  int num_of_rays;               /* >= 1                                                      */
  int max_depth;                 /* >= 0                                                      */
  int rr_limit;                  /* russian_roulette_limit: any value                         */
  int depth0;                    /* Ray.depth of the probe's rays, >= 0                       */
  unsigned long long init_state; /* PCG(init_state, .)                                        */
  unsigned long long init_seq;   /* seqs == NULL: probe i's sample k draws from init_seq + i K + k */
  double background[3];          /* the renderer's background_color                           */
} pt_sh_params;

/* (major << 16) | minor of the ray library's interface this library implements: 1.6. */
int pt_rays_sh_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_sh_args_bytes(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_sh_last_error(char *buf, size_t n);

/* Bytes of the directions of n probes at `samples` samples: 24 n K (0 on refusal). */
size_t pt_rays_sh_dirs_bytes(long long n, int samples);
int pt_rays_sh_directions_device(int device, const unsigned long long *seqs_dev, long long n, const pt_sh_params *params, void *out_dev,
                                 size_t out_bytes, void *stream);
/* The same for host buffers: stages through device memory it allocates and frees.  Synchronous. */
int pt_rays_sh_directions(int device, const unsigned long long *seqs_host, long long n, const pt_sh_params *params, void *out_host,
                          size_t out_bytes);

/* Bytes of the coefficients of n probes: 216 n, + 8 n with PT_SH_COUNT. */
size_t pt_rays_sh_bytes(long long n, int channels);
/* Byte offset of a plane in that buffer: `channel` 0 (coefficients; component 3 j + ch, 0 .. 26) or PT_SH_COUNT (0).  < 0: not
 * selected. */
long long pt_rays_sh_plane_offset(long long n, int channels, int channel, int component);
/* Bytes of the workspace a projection of n probes with `params` needs on `device` (0 on refusal, the reason in
 * pt_rays_sh_last_error). */
size_t pt_rays_sh_workspace_bytes(int device, long long n, const pt_sh_params *params);

int pt_rays_sh_project_device(int device, const void *scene_args, size_t scene_args_bytes, const double *points_dev, const int *active_dev,
                              const unsigned long long *seqs_dev, long long n, const pt_sh_params *params, int channels, void *workspace_dev,
                              size_t workspace_bytes, void *out_dev, size_t out_bytes, void *stream);
/* The same for host buffers: inputs, workspace and output are staged in device memory it allocates and frees.  Synchronous. */
int pt_rays_sh_project(int device, const void *scene_args, size_t scene_args_bytes, const double *points_host, const int *active_host,
                       const unsigned long long *seqs_host, long long n, const pt_sh_params *params, int channels, void *out_host,
                       size_t out_bytes);

/* Bytes of m evaluated records: 24 m (0 on refusal). */
size_t pt_rays_sh_eval_bytes(long long m);
int pt_rays_sh_eval_device(int device, const double *coeffs_dev, long long n, const int *index_dev, const double *dirs_dev, long long m,
                           int kind, void *out_dev, size_t out_bytes, void *stream);
/* The same for host buffers.  Synchronous. */
int pt_rays_sh_eval(int device, const double *coeffs_host, long long n, const int *index_host, const double *dirs_host, long long m, int kind,
                    void *out_host, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_SH_H */
