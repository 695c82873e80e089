/* ptrace_bake.h — C-ABI of libptrace_bake.so: surface points from (shape, u, v), and light maps over a shape's (u, v) grid.
 *
 * Interface 1.5 of the ray library, its seventh step: a BAKE QUERY.  The gather query (ptrace_gather.h) takes a world point and
 * a normal per record; a light-map texel is neither -- it is an AREA of a shape's (u, v) square, and an antialiased map wants
 * every sample at a point of its own inside that area.  This library makes the points on the device, two ways.
 *
 * SURFACE POINT  S(shape s, u, v, side), side in {+1, -1} -- the inverse of the shapes' own (u, v) maps:
 *     Sphere:  th = v * pi,  ph = (2.0 * pi) * u,  p = (sin th * cos ph, sin th * sin ph, cos th)     (inverse of shapes.py:36-42;
 *              one sincos per angle, the function scatter_ray uses),  n_loc = side * p
 *     Plane:   p = (u, v, 0.0) for any real u, v (the reference's surface_point is its fractional part, shapes.py:183-185),
 *              n_loc = (0, 0, side)
 *     point  = T * Point(p)                          (transformations.py:58-96, the device's point transform)
 *     normal = (T * Normal(n_loc)).normalize()       (as World.ray_intersection leaves it, world.py:66-67)
 * Nothing else is checked: NaN or infinite u, v give NaN planes.  A record whose shape is not in [0, n_shapes) is skipped and
 * written as zeros.  A record's side: a negative value is -1, every other value +1 (NULL: +1 for all).
 *
 * BAKE of the rectangle [col0, col0 + w) x [row0, row0 + h) of a W x H map of shape s: with the GLOBAL texel
 * t = (row0 + r) * W + (col0 + c) and the samples k < K,
 *     g      = PCG(init_state, init_seq + t * K + k)                                  (pcg.py:25-41; 64-bit wrap)
 *     ju, jv = jitter ? (g.random_float(), g.random_float()) : (0.5, 0.5)             (no draw without jitter)
 *     u      = ((col0 + c) + ju) * (1.0 / W);   v = ((row0 + r) + jv) * (1.0 / H)     (cf. imagetracer.py:48-58)
 *     (p, n) = S(s, u, v, side)
 *     ray    = DiffuseBRDF.scatter_ray(g, ., p, n, depth0)                            (materials.py:132-152)
 *     L_tk   = PathTracer(world, background, g, num_of_rays, max_depth, rr_limit)(ray)   (render.py:99-139)
 *     out_t  = (((0 + L_t0) + L_t1) + ... + L_t,K-1) * (1.0 / K)                      per channel, STRICTLY in k order
 *     count_t = sum over k of the rays handed to a world query for sample k            (uint64; it wraps)
 * Because t is the global texel index, a map baked in tiles is bit for bit the map baked whole.  Every sample runs on a lane of
 * its own (j = t_local * K + k) through the gather's walk; the mean is a second launch on the same stream, one lane per texel:
 * no atomics, nothing that depends on scheduling or on the launch's shape.  Without jitter the result is what
 * pt_rays_surface_points at the texel centres followed by pt_rays_gather (seq_t = init_seq + t * K) returns, bit for bit.
 *
 * A SEVENTH shared object, for the reasons the sixth one gives.  It links to none of the others, loads nothing, and gets the
 * scene as the argument block of pt_scene_kernel_args (ptrace.h, ABI 1.7); all seven must come from one build of the tree.  It
 * finds a shape's record itself (the records' `index` field), so it takes no slot table.
 *
 * Every entry point is `extern "C"`, returns 0 or a negative PT_ERR_* of ptrace.h (the size queries: 0 on refusal), never
 * throws, and checks every argument before its first HIP call:
 *     w * h * K > 2^31 - 1; an unknown side; a rectangle outside the map (or w, h < 1); W, H, K, num_of_rays < 1; max_depth < 0;
 *     depth0 < 0; a shape outside [0, n_shapes); unknown channel bits; n < 0 or n > 2^31 - 1            PT_ERR_INVALID
 *     max_depth - depth0 > 64                                                                            PT_ERR_UNSUPPORTED
 *     an output or a workspace that is too small                                                         PT_ERR_SIZE
 * The *_device forms are asynchronous on the caller's stream (a hipStream_t; NULL: the default stream, and the call returns when
 * the work is done) and allocate nothing.
 *
 * Surface points.  In: `shape` int32[n], `uv` planar [2, n] fp64, `side` int32[n] or NULL.  Out: planar [6, n] fp64, point x, y,
 * z then normal x, y, z: pt_rays_points_bytes(n) = 48 n bytes -- its two halves are the `points` and `normals` of a gather.
 *
 * Bake workspace: pt_rays_bake_workspace_bytes(device, params) bytes of device memory: the node stacks, planar
 * [level][field][lane], sized by the lanes one launch keeps resident (lowered to PTRACE_BAKE_LANES where that environment
 * variable names a smaller number; a multiple of 256, at least 256; read at every call), then the sample planes [4][w h K] of 8
 * bytes.  The contents are scratch; two calls that may overlap need a workspace each.
 *
 * Bake output: pt_rays_bake_bytes(w * h, channels) bytes, planar, 8-byte planes of w * h values in row-major texel order:
 *     radiance       3 fp64 planes (r, g, b), always written
 *     PT_BAKE_COUNT  1 uint64 plane: count_t
 * A plane that is not selected costs no stores.
 */
#ifndef PTRACE_BAKE_H
#define PTRACE_BAKE_H

#include <stddef.h>

#include "ptrace.h" /* PT_OK, PT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define PT_BAKE_COUNT 1 /* 1 plane: rays traced per texel (uint64) */
#define PT_BAKE_ALL   1

#define PT_BAKE_MAX_LEVELS 64 /* max_depth - depth0 at most */

typedef struct pt_bake_params {
  int shape;                     /* World.shapes index of the shape whose map is baked                        */
  int side;                      /* +1: the side its local normal p (sphere) / +z (plane) points to; -1: the other */
  int W, H;                      /* the whole map, >= 1                                                       */
  int col0, row0, w, h;          /* the rectangle of it this call bakes                                       */
  int jitter;                    /* 0: every sample at the texel's centre, no draw; else two draws per sample */
  int samples;                   /* K >= 1: samples per texel                                                 */
  int num_of_rays;               /* >= 1                                                                      */
  int max_depth;                 /* >= 0                                                                      */
  int rr_limit;                  /* russian_roulette_limit: any value                                         */
  int depth0;                    /* Ray.depth of the hemisphere's rays, >= 0                                  */
  unsigned long long init_state; /* PCG(init_state, .)                                                        */
  unsigned long long init_seq;   /* texel t's sample k draws from stream init_seq + t K + k                   */
  double background[3];          /* the renderer's background_color                                           */
} pt_bake_params;

/* (major << 16) | minor of the ray library's interface this library implements: 1.5. */
int pt_rays_bake_version(void);
/* sizeof(PtKArgs) this library was built with: what pt_scene_kernel_args must be asked for. */
size_t pt_rays_bake_args_bytes(void);
/* Copy the last error message of the calling thread (NUL-terminated) into buf; returns its length. */
int pt_rays_bake_last_error(char *buf, size_t n);

/* Bytes of n surface points: 48 n (0 on refusal). */
size_t pt_rays_points_bytes(long long n);
int pt_rays_surface_points_device(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_dev, const double *uv_dev,
                                  const int *side_dev, long long n, void *out_dev, size_t out_bytes, void *stream);
/* The same for host buffers: stages through device memory it allocates and frees.  Synchronous. */
int pt_rays_surface_points(int device, const void *scene_args, size_t scene_args_bytes, const int *shape_host, const double *uv_host,
                           const int *side_host, long long n, void *out_host, size_t out_bytes);

/* Bytes of a baked rectangle of `texels` = w * h texels: 24 texels, + 8 texels with PT_BAKE_COUNT. */
size_t pt_rays_bake_bytes(long long texels, int channels);
/* Byte offset of a plane in that buffer: `channel` 0 (radiance; component 0 .. 2) or PT_BAKE_COUNT (0).  < 0: not selected. */
long long pt_rays_bake_plane_offset(long long texels, int channels, int channel, int component);
/* Bytes of the workspace the bake `params` describes needs on `device` (0 on refusal, the reason in pt_rays_bake_last_error;
 * the shape is not looked at: there is no scene here). */
size_t pt_rays_bake_workspace_bytes(int device, const pt_bake_params *params);

int pt_rays_bake_device(int device, const void *scene_args, size_t scene_args_bytes, const pt_bake_params *params, int channels,
                        void *workspace_dev, size_t workspace_bytes, void *out_dev, size_t out_bytes, void *stream);
/* The same into a host buffer: the workspace and the output are staged in device memory it allocates and frees.  Synchronous. */
int pt_rays_bake(int device, const void *scene_args, size_t scene_args_bytes, const pt_bake_params *params, int channels, void *out_host,
                 size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PTRACE_BAKE_H */
