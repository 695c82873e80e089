// ptrace_rays.hip — libptrace_rays.so: the C-ABI of include/ptrace_rays.h, ray batches through the path tracer's own query.
//
// What it restates: World.ray_intersection (world.py:51-69) and World.is_point_visible's inner loop (world.py:71-80) for
// rays the CALLER supplies.  The arithmetic is pt_query.h's world_query_lanes (every lane on its own candidate list) and
// pt_shade.h's hit_details, included here as they are: nothing of them is restated.
//
// Why a second translation unit and a second shared object: bench.py prices its roofline from profiles/pmc_*.json, each
// of which names the sha256 of libptrace.so's device code (build.code_hash); a kernel added to ptrace.hip would change
// that hash and unprice every profile.  So libptrace.so's device code stays what it was, and this library gets the scene
// from its caller as the argument block pt_scene_kernel_args (ptrace.h, ABI 1.7) hands out.  No link dependency between
// the two, nothing is loaded from here.
#include <hip/hip_runtime.h>

#include "../../include/ptrace_rays.h"
#define PT_QUERY_PARTS_ONLY
#include "pt_kernels.h"
#include "pt_host_common.h"

#define PT_RAYS_VERSION ((1 << 16) | 1)  // 1.1: the block also feeds the surface queries (include/ptrace_surface.h)
#define PT_RAYS_CHANNELS (PT_HIT_T | PT_HIT_POINT | PT_HIT_NORMAL | PT_HIT_UV)
#define PT_RAYS_MAX_N 2147483647LL  // the grid is n / 256 blocks in x

// One ray per lane.  Every lane of a wave enters the queries together (they ballot): the idle lanes of the batch's last wave
// stand on ray 0 with active = false, and nothing returns before the query.  `channels` is wave-uniform: a plane that is
// not selected costs neither its stores nor (UV, spheres) atan2 / acos.  A lane writes one value per plane, so a wave's
// stores are 512 consecutive bytes of a plane (256 of the int32 plane).
template <bool ANYHIT>
__global__ __launch_bounds__(PT_BLOCK) void pt_rays_kernel(const PtKArgs a, const double *__restrict__ rays, long long n, int channels,
                                                           void *__restrict__ out) {
  const long long i = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
  const bool active = i < n;
  const double *rp = rays + (active ? i : 0);
  Ray ray;
  ray.o = {rp[0], rp[n], rp[2 * n]};
  ray.d = {rp[3 * n], rp[4 * n], rp[5 * n]};
  ray.tmin = rp[6 * n];
  const double tmax = rp[7 * n];
  // The candidate filter knows that a scattered or shadow ray looks FORWARD: a ball behind the origin is dropped, and so is a
  // sphere the origin lies outside of and moves away from -- both roots are <= 0, hence below any tmin >= 0.  A caller's ray
  // may have tmin < 0 (an ordinary value here), and then those roots count.  Such lanes sit the filtered query out and go
  // through the exhaustive one (world_query: every shape, the reference's tests and nothing else), entered by the whole
  // wave only when some lane needs it.  (NaN tmin: no root is ever inside (tmin, tmax); it takes the same way.)
  const bool behind = active && !(ray.tmin >= 0.0);
  double t;
  int hit = world_query_lanes<ANYHIT>(a, ray, tmax, t, active && !behind, -1);
  if (__ballot(behind) != 0ULL) {
    double t_all;
    const int hit_all = world_query<ANYHIT, false>(a, ray, tmax, t_all, behind);
    if (behind) {
      hit = hit_all;
      t = t_all;
    }
  }
  int *const shape_out = (int *)out;
  if (ANYHIT) {
    if (active) shape_out[i] = hit >= 0 ? 1 : 0;
    return;
  }
  // world.py:51-69: None -> shape -1, t = +inf, zeros; else the winner's record, its normal normalised
  Hit h;
  h.wp = {0.0, 0.0, 0.0};
  h.n = {0.0, 0.0, 0.0};
  h.u = 0.0;
  h.v = 0.0;
  int index = -1;
  if (active && hit >= 0) {
    hit_details(a.recs + hit, a.aux + hit, ray, t, h, (channels & PT_HIT_UV) != 0);
    index = a.recs[hit].index;
  }
  if (!active) return;
  shape_out[i] = index;
  double *o = (double *)((char *)out + ((n * 4 + 7) & ~7LL)) + i;
  if (channels & PT_HIT_T) {
    o[0] = t;  // (the query leaves +inf where nothing was hit)
    o += n;
  }
  if (channels & PT_HIT_POINT) {
    o[0] = h.wp.x;
    o[n] = h.wp.y;
    o[2 * n] = h.wp.z;
    o += 3 * n;
  }
  if (channels & PT_HIT_NORMAL) {
    o[0] = h.n.x;
    o[n] = h.n.y;
    o[2 * n] = h.n.z;
    o += 3 * n;
  }
  if (channels & PT_HIT_UV) {
    o[0] = h.u;
    o[n] = h.v;
  }
}

extern "C" int pt_rays_version(void) { return PT_RAYS_VERSION; }

extern "C" size_t pt_rays_args_bytes(void) { return sizeof(PtKArgs); }

extern "C" int pt_rays_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

static int planes_of(int channel) {
  switch (channel) {
    case PT_HIT_T: return 1;
    case PT_HIT_POINT: return 3;
    case PT_HIT_NORMAL: return 3;
    case PT_HIT_UV: return 2;
    default: return 0;
  }
}

static bool shape_ok(long long n, int channels, int anyhit) {
  if (n < 0 || n > PT_RAYS_MAX_N) return false;
  if (anyhit != 0 && anyhit != 1) return false;
  if (channels < 0 || (channels & ~PT_RAYS_CHANNELS)) return false;
  return !(anyhit && channels != 0);
}

extern "C" size_t pt_rays_bytes(long long n, int channels, int anyhit) {
  if (!shape_ok(n, channels, anyhit)) return 0;
  int planes = 0;
  for (int bit = 1; bit <= PT_HIT_UV; bit <<= 1)
    if (channels & bit) planes += planes_of(bit);
  return (size_t)((n * 4 + 7) & ~7LL) + (size_t)n * 8 * (size_t)planes;
}

extern "C" long long pt_rays_plane_offset(long long n, int channels, int anyhit, int channel, int component) {
  if (!shape_ok(n, channels, anyhit)) return PT_ERR_INVALID;
  if (channel == 0) return component == 0 ? 0 : PT_ERR_INVALID;
  if (planes_of(channel) == 0 || !(channels & channel) || component < 0 || component >= planes_of(channel)) return PT_ERR_INVALID;
  long long planes = 0;
  for (int bit = 1; bit < channel; bit <<= 1)
    if (channels & bit) planes += planes_of(bit);
  return ((n * 4 + 7) & ~7LL) + n * 8 * (planes + component);
}

// every argument, before any HIP call; `need`: the bytes of the output
static int check_args(int device, const void *scene_args, size_t scene_args_bytes, const double *rays, long long n, int channels, int anyhit,
                      const void *out, size_t out_bytes, size_t &need) {
  need = 0;
  if (n < 0 || n > PT_RAYS_MAX_N) return fail(PT_ERR_INVALID, "ray count %lld outside [0, 2^31 - 1]", n);
  if (anyhit != 0 && anyhit != 1) return fail(PT_ERR_INVALID, "anyhit must be 0 or 1, not %d", anyhit);
  if (channels < 0 || (channels & ~PT_RAYS_CHANNELS))
    return fail(PT_ERR_INVALID, "channel bits %#x: a ray batch has PT_HIT_T | PT_HIT_POINT | PT_HIT_NORMAL | PT_HIT_UV", channels);
  if (anyhit && channels != 0) return fail(PT_ERR_INVALID, "any-hit writes the blocked / free plane only: channels must be 0, not %#x", channels);
  if (int rc = check_scene_block(device, scene_args, scene_args_bytes, 0)) return rc;
  need = pt_rays_bytes(n, channels, anyhit);
  if (n == 0) return PT_OK;
  if (!rays || !out) return fail(PT_ERR_INVALID, "null ray or output buffer");
  if (out_bytes < need) return fail(PT_ERR_SIZE, "ray-batch output too small: %zu < %zu bytes", out_bytes, need);
  return PT_OK;
}

static int enqueue(const void *scene_args, const double *rays_dev, long long n, int channels, int anyhit, void *out_dev, hipStream_t st) {
  const PtKArgs a = scene_block(scene_args);
  const dim3 grid = grid_of(n);
  if (anyhit)
    hipLaunchKernelGGL(pt_rays_kernel<true>, grid, dim3(PT_BLOCK), 0, st, a, rays_dev, n, channels, out_dev);
  else
    hipLaunchKernelGGL(pt_rays_kernel<false>, grid, dim3(PT_BLOCK), 0, st, a, rays_dev, n, channels, out_dev);
  HIP_TRY(hipGetLastError());
  return PT_OK;
}

extern "C" int pt_rays_trace_device(int device, const void *scene_args, size_t scene_args_bytes, const double *rays_dev, long long n,
                                    int channels, int anyhit, void *out_dev, size_t out_bytes, void *stream) {
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, rays_dev, n, channels, anyhit, out_dev, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  if ((rc = enqueue(scene_args, rays_dev, n, channels, anyhit, out_dev, (hipStream_t)stream))) return rc;
  if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
  return PT_OK;
}

extern "C" int pt_rays_trace(int device, const void *scene_args, size_t scene_args_bytes, const double *rays_host, long long n,
                             int channels, int anyhit, void *out_host, size_t out_bytes) {
  size_t need;
  int rc = check_args(device, scene_args, scene_args_bytes, rays_host, n, channels, anyhit, out_host, out_bytes, need);
  if (rc || n == 0) return rc;
  if ((rc = device_ok(device))) return rc;
  HIP_TRY(hipSetDevice(device));
  const size_t ray_bytes = (size_t)n * 8 * sizeof(double);
  Staged s;
  if ((rc = s.alloc(ray_bytes + need))) return rc;
  char *rays_d = s.dev, *out_d = rays_d + ray_bytes;
  hipError_t e = hipMemcpy(rays_d, rays_host, ray_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if ((rc = enqueue(scene_args, (const double *)rays_d, n, channels, anyhit, out_d, nullptr))) return rc;
    e = hipMemcpy(out_host, out_d, need, hipMemcpyDeviceToHost);  // (the null stream: behind the kernel)
  }
  if (e != hipSuccess) return fail(PT_ERR_HIP, "staging a ray batch failed: %s", hipGetErrorString(e));
  return PT_OK;
}
