// ptrace.hip — libptrace.so: the C-ABI of include/ptrace.h over the HIP kernels of pt_kernels.h.
//
// Boundary replaced: ImageTracer.fire_all_rays(renderer) — src/pytracer/imagetracer.py:60-110 with
// the solvers of src/pytracer/render.py:42-193.  No torch types, no exceptions across the ABI, every
// failure is a negative return code plus a thread-local message (pt_last_error).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ptrace.h"
#include "../../include/ptrace_debug.h"
#include "pt_kernels.h"
#include "pt_layout.h"
#include "pt_plan.h"
#include "pt_scene_build.h"
#include "pt_hits_plan.h"
#include "pt_frame_args.h"
#include "pt_post.h"
#include "pt_host_common.h"  // g_err, fail, HIP_TRY, copy_last_error, device_ok

// major << 16 | minor.  The minor grows whenever a struct of include/ptrace.h grows or an entry point is added (minor 2:
// pt_stats gained `kernel` + `_reserved`, pt_scene_clone / pt_image_sparse_* arrived; minor 3: PT_PCG_SEQ accepted for
// OnOff / Flat / PointLight at any samples_per_side; minor 4: pt_device_kernargs, and the library no longer sets
// HIP_FORCE_DEV_KERNARG when it is loaded; minor 5: pt_device_alloc / pt_device_free / pt_device_download / pt_stream_*;
// minor 6: hit-record frames -- pt_hits_bytes / pt_hits_plane_offset / pt_render_hits / pt_render_hits_device;
// minor 7: pt_scene_kernel_args, the scene's argument block for add-on libraries built from this tree -- libptrace_rays.so);
// a caller built against an older header checks pt_version() first.
#define PT_VERSION ((1 << 16) | 7)

// (Kernel arguments in device memory -- HIP_FORCE_DEV_KERNARG=1, ~1 us per launch, profiles/r04_dev_kernarg.txt -- are the
// CALLER's choice: the HIP runtime reads the variable when it initialises, and a library that edited the process environment
// at load time would change HIP for every other user of the runtime in the process.  pytracer_amd.prefer_device_kernargs(),
// the `render` command and bench.py set it before their first HIP call; pt_device_kernargs() reports what is in effect.)

// What pt_scene_upload makes of a scene and no launch changes: the tables in HBM and every scalar of the analysis.  One
// block per uploaded scene, shared by all its handles (pt_scene_clone); the last handle to be freed frees it.
struct PtSceneShared {
  PtShapeRec *recs = nullptr;
  PtShapeAux *aux = nullptr;
  PtDiagRec *diag = nullptr;
  float4 *bounds = nullptr;
  unsigned *grid_cells = nullptr, *grid_occ = nullptr;  // uniform grid for scattered / shadow rays (see PtKArgs)
  float4 *grid_balls = nullptr;
  unsigned short *grid_slots = nullptr;
  int *grid_always = nullptr;
  float *bsoa = nullptr;  // bounds as x[], y[], z[], r'[] (bs_stride floats each), then group and chunk balls
  PtLight *lights = nullptr;
  PtTex *tex = nullptr;
  double *tex_data = nullptr;
  PtSceneScalars sc;
  std::vector<PtDomeCand> dome_cands;
  int n_cu = 256;
  std::atomic<int> refs{1};
};

// the device's current copy of the cold half of an argument block (refresh_cold)
struct ColdArgs {
  PtKArgs *dev = nullptr;
  PtKArgs last;  // what `dev` holds
  bool valid = false;
  hipStream_t stream = nullptr;
};

// a handle: the scene it renders, and everything a launch writes
struct pt_scene {
  int device = 0;
  PtSceneShared *sh = nullptr;
  PtHoist *hoist = nullptr;
  PtHoistDiag *hoist_diag = nullptr;
  double *ws = nullptr;  // path-tracer frame stack, grown on demand
  size_t ws_bytes = 0;
  double *handover = nullptr;  // num_of_rays > 1: records of the pixels the one-queue kernel hands to the tree kernel
  size_t handover_doubles = 0;
  int4 *units_handed = nullptr;  // ... and their units
  size_t units_handed_n = 0;
  unsigned char *out_dev = nullptr;  // staging for pt_render (host output)
  size_t out_dev_bytes = 0;
  unsigned long long *ray_counter = nullptr;   // totals: all rays, rays resolved by the dome shortcut
  unsigned long long *ray_partials = nullptr;  // the same two per workgroup
  int ray_partials_n = 0;
  // path tracer: two queue blocks (pixel queue head / work units of the second pass, PT_QUEUE_WORDS each).  A frame
  // uses one and its last kernel zeroes the other for the next frame: no memset (and no launch gap after it) in front
  // of a frame.  queue_clean: the block the next frame will use is known to be zero.
  unsigned long long *queue = nullptr;
  unsigned long long *queue_last = nullptr;  // the block the most recent frame used (debug read-back)
  int queue_parity = 0;
  bool queue_clean = false;
  ColdArgs args;                        // the argument block (cold fields)
  ColdArgs args2;                       // ... pt_path_flagged_kernel's, when a frame enqueues both second-pass kernels (PT_Q_CHOICE)
  ColdArgs scene_args;                  // pt_scene_kernel_args: the scene-only block (no camera, no frame), made on first call
  int last_handover_cap = 0;            // records the last num_of_rays > 1 frame's hand-over table held (pt_debug_handed_over)
  bool choice_pending = false;          // ray_counter_host[2] will hold the frame's PT_Q_CHOICE word once ev_count has passed
  unsigned char *region_keys = nullptr;  // path tracer region ordering
  unsigned long long *region_mask = nullptr;
  int4 *units = nullptr;  // second pass: work units (pt_unit_scatter)
  size_t region_keys_cap = 0, region_mask_cap = 0, units_cap = 0;
  unsigned int *cell_list = nullptr;  // large scenes: per-cell survivor lists (pt_cell_kernel)
  int *cell_count = nullptr;
  size_t cell_list_cap = 0, cell_count_cap = 0;
  unsigned long long *ray_counter_host = nullptr;  // pinned
  hipStream_t stream = nullptr;
  hipStream_t last_stream = nullptr;  // stream of the most recent launch
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  hipEvent_t ev_count = nullptr;  // recorded behind the copy of the ray count into ray_counter_host
  bool count_pending = false;     // the last launch enqueued that copy: fold_stats waits for ev_count
  bool launched = false;          // last_stream names a stream this scene has work on
  std::vector<hipEvent_t> prof;  // 2 * capacity events while profiling
  int prof_used = 0;             // pairs recorded
  bool profiling = false;
  bool count_rays = true;
  bool dome_shortcut = true;  // pt_set_dome_shortcut
  bool timing = true;  // bracket render kernels with hipEvents
  bool pending = false;  // an async render whose stats are not folded yet
  bool pending_copy = false;
  bool stats_valid = true;  // ev0/ev1 bracket the last launch (false while the profiling ring is used)
  bool hoist_valid = false;  // s->hoist holds the constants of hoist_cam
  pt_camera hoist_cam = {};
  hipStream_t hoist_stream = nullptr;  // the stream the constants were produced on
  pt_stats stats = {};
};

extern "C" int pt_version(void) { return PT_VERSION; }

extern "C" int pt_device_kernargs(void) {
  const char *v = getenv("HIP_FORCE_DEV_KERNARG");
  return v && atoi(v) != 0 ? 1 : 0;
}

extern "C" int pt_last_error(char *buf, size_t n) { return copy_last_error(buf, n); }

extern "C" int pt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int pt_device_info(int device, int *compute_units, int *clock_khz) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(PT_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (clock_khz) *clock_khz = prop.clockRate;
  return PT_OK;
}

extern "C" int pt_rows_for_rank(const pt_params *p) { return pt_plan_rows(p); }

extern "C" size_t pt_output_bytes(const pt_params *p) {
  if (!p) return 0;
  return (size_t)pt_rows_for_rank(p) * (size_t)p->width * 3 * (p->out_format == PT_OUT_F32 ? 4 : 8);
}

static int check_desc(const pt_scene_desc *d) { return pt_check_desc(d, g_err, sizeof g_err); }

// drop a handle's reference on the scene's block; the last one frees the tables (the device is current)
static void shared_release(PtSceneShared *sh) {
  if (!sh || sh->refs.fetch_sub(1) != 1) return;
  for (void *p : {(void *)sh->recs, (void *)sh->aux, (void *)sh->diag, (void *)sh->bounds, (void *)sh->bsoa, (void *)sh->grid_cells,
                  (void *)sh->grid_occ, (void *)sh->grid_balls, (void *)sh->grid_slots, (void *)sh->grid_always, (void *)sh->lights,
                  (void *)sh->tex, (void *)sh->tex_data})
    (void)hipFree(p);
  delete sh;
}

extern "C" void pt_scene_free(pt_scene *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->launched && s->last_stream) (void)hipStreamSynchronize(s->last_stream);
  shared_release(s->sh);
  for (void *p : {(void *)s->hoist, (void *)s->hoist_diag, (void *)s->ws, (void *)s->handover, (void *)s->units_handed, (void *)s->out_dev,
                  (void *)s->ray_counter, (void *)s->ray_partials, (void *)s->queue, (void *)s->args.dev, (void *)s->args2.dev, (void *)s->scene_args.dev,
                  (void *)s->region_keys, (void *)s->units, (void *)s->region_mask, (void *)s->cell_list, (void *)s->cell_count})
    (void)hipFree(p);
  if (s->ray_counter_host) (void)hipHostFree(s->ray_counter_host);
  for (hipEvent_t e : {s->ev0, s->ev1, s->ev2, s->ev_count})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : s->prof) (void)hipEventDestroy(e);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

template <typename T>
static int upload(T **dst, const std::vector<T> &src) {
  const size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T);
  HIP_TRY(hipMalloc((void **)dst, bytes));
  if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return PT_OK;
}

// aux[] and, directly behind it in the same allocation, the Flat palette in whole zero-filled chunks (pt_layout.h: PtFlatPal):
// pt_tile4_kernel<FLAT, *> finds it as a.aux + a.n_shapes and may read every mapped chunk to its end
static int upload_aux_and_palette(PtShapeAux **dst, const PtSceneHost &h) {
  const std::vector<unsigned char> img = pt_aux_image(h);
  HIP_TRY(hipMalloc((void **)dst, std::max(img.size(), sizeof(PtShapeAux))));  // (an empty world: a pointer nobody reads through)
  if (!img.empty()) HIP_TRY(hipMemcpy(*dst, img.data(), img.size(), hipMemcpyHostToDevice));
  return PT_OK;
}

// what every handle has of its own besides the per-camera constants: counters, queue blocks, the argument block, a stream
// and events.  On failure the handle is freed.
static int handle_state(pt_scene *s) {
  auto hip_or_free = [&](hipError_t e, const char *what) -> int {
    if (e == hipSuccess) return PT_OK;
    int code = fail(PT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    pt_scene_free(s);
    return code;
  };
  int rc;
  if ((rc = hip_or_free(hipMalloc((void **)&s->ray_counter, 2 * sizeof(unsigned long long)), "hipMalloc(counter)"))) return rc;
  if ((rc = hip_or_free(hipMalloc((void **)&s->queue, 2 * PT_QUEUE_WORDS * sizeof(unsigned long long)), "hipMalloc(queue)"))) return rc;
  if ((rc = hip_or_free(hipMalloc((void **)&s->args.dev, sizeof(PtKArgs)), "hipMalloc(args)"))) return rc;
  if ((rc = hip_or_free(hipMalloc((void **)&s->args2.dev, sizeof(PtKArgs)), "hipMalloc(args)"))) return rc;
  if ((rc = hip_or_free(hipHostMalloc((void **)&s->ray_counter_host, 3 * sizeof(unsigned long long)), "hipHostMalloc"))) return rc;
  s->ray_counter_host[0] = s->ray_counter_host[1] = s->ray_counter_host[2] = 0;
  if ((rc = hip_or_free(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "hipStreamCreate"))) return rc;
  if ((rc = hip_or_free(hipEventCreate(&s->ev0), "hipEventCreate"))) return rc;
  if ((rc = hip_or_free(hipEventCreate(&s->ev1), "hipEventCreate"))) return rc;
  if ((rc = hip_or_free(hipEventCreate(&s->ev2), "hipEventCreate"))) return rc;
  if ((rc = hip_or_free(hipEventCreateWithFlags(&s->ev_count, hipEventDisableTiming), "hipEventCreate"))) return rc;
  return PT_OK;
}

static PtSceneFacts scene_facts(const pt_scene *s) { return pt_scene_facts(s->sh->sc, s->sh->n_cu, s->dome_shortcut); }

extern "C" int pt_scene_upload(const pt_scene_desc *d, int device, pt_scene **out) {
  if (!out) return fail(PT_ERR_INVALID, "null output handle");
  *out = nullptr;
  int rc = check_desc(d);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PT_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(PT_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
  HIP_TRY(hipSetDevice(device));

  pt_scene *s = new (std::nothrow) pt_scene();
  PtSceneShared *sh = s ? new (std::nothrow) PtSceneShared() : nullptr;
  if (!sh) {
    delete s;
    return fail(PT_ERR_NOMEM, "out of host memory");
  }
  s->device = device;
  s->sh = sh;
  PtSceneHost h;
  pt_build_scene(d, pt_tuning(), h);
  sh->sc = h.sc;
  sh->dome_cands = h.dome_cands;
#define UP(call)            \
  do {                      \
    rc = (call);            \
    if (rc) {               \
      pt_scene_free(s);     \
      return rc;            \
    }                       \
  } while (0)
  UP(upload(&sh->recs, h.recs));
  UP(upload(&sh->bounds, h.bounds));
  if (h.has_grid) {
    UP(upload(&sh->grid_cells, h.grid_cells));
    UP(upload(&sh->grid_occ, h.grid_occ));
    UP(upload(&sh->grid_slots, h.grid_slots));
    UP(upload(&sh->grid_balls, h.grid_balls));
    UP(upload(&sh->grid_always, h.grid_always));
  }
  UP(upload(&sh->bsoa, h.bsoa));
  UP(upload(&sh->diag, h.diag));
  {
    std::vector<PtHoistDiag> hd(std::max(sh->sc.n_diag, 1));
    UP(upload(&s->hoist_diag, hd));
  }
  UP(upload_aux_and_palette(&sh->aux, h));
  UP(upload(&sh->lights, h.lights));
  UP(upload(&sh->tex, h.tex));
  UP(upload(&sh->tex_data, h.tex_data));
  {
    std::vector<PtHoist> hh(std::max(sh->sc.n_shapes, 1));
    UP(upload(&s->hoist, hh));
  }
#undef UP
  if ((rc = handle_state(s))) return rc;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) sh->n_cu = prop.multiProcessorCount;
  *out = s;
  return PT_OK;
}

// A second handle on the same scene: it takes a reference on the block pt_scene_upload made (nothing a launch writes) and
// has its own per-camera constants, queues, counters, workspace, stream and events -- so frames rendered through different
// handles of a scene may be in flight at the same time, each on its own stream (include/ptrace.h).
extern "C" int pt_scene_clone(pt_scene *src, pt_scene **out) {
  if (!src || !out) return fail(PT_ERR_INVALID, "null argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(src->device));
  pt_scene *s = new pt_scene();
  s->device = src->device;
  s->sh = src->sh;
  s->sh->refs.fetch_add(1);
  s->count_rays = src->count_rays; s->dome_shortcut = src->dome_shortcut; s->timing = src->timing;
  int rc = PT_OK;
  const size_t nh = (size_t)std::max(s->sh->sc.n_shapes, 1), nd = (size_t)std::max(s->sh->sc.n_diag, 1);
  if (hipMalloc((void **)&s->hoist, nh * sizeof(PtHoist)) != hipSuccess || hipMalloc((void **)&s->hoist_diag, nd * sizeof(PtHoistDiag)) != hipSuccess) {
    pt_scene_free(s);  // (drops the reference: the tables stay with the handles that still use them)
    return fail(PT_ERR_NOMEM, "hipMalloc(per-camera constants) failed");
  }
  if ((rc = handle_state(s))) return rc;
  *out = s;
  return PT_OK;
}

extern "C" int pt_set_dome_shortcut(pt_scene *s, int enable) {
  if (!s) return fail(PT_ERR_INVALID, "null scene");
  s->dome_shortcut = enable != 0;
  return PT_OK;
}

extern "C" int pt_set_count_rays(pt_scene *s, int enable) {
  if (!s) return fail(PT_ERR_INVALID, "null scene");
  s->count_rays = enable != 0;
  return PT_OK;
}

static int check_params(const pt_camera *cam, const pt_params *p) {
  if (!cam || !p) return fail(PT_ERR_INVALID, "null argument");
  if (p->width <= 0 || p->height <= 0) return fail(PT_ERR_INVALID, "bad image size %dx%d", p->width, p->height);
  if (p->samples_per_side < 0 || p->samples_per_side > 1024)
    return fail(PT_ERR_INVALID, "bad samples_per_side %d", p->samples_per_side);
  if (p->renderer < PT_RENDERER_ONOFF || p->renderer > PT_RENDERER_POINTLIGHT)
    return fail(PT_ERR_INVALID, "unknown renderer %d", p->renderer);
  if (cam->kind != PT_CAMERA_ORTHOGONAL && cam->kind != PT_CAMERA_PERSPECTIVE)
    return fail(PT_ERR_INVALID, "unknown camera kind %d", cam->kind);
  if (p->out_format != PT_OUT_F64 && p->out_format != PT_OUT_F32)
    return fail(PT_ERR_INVALID, "unknown output format %d", p->out_format);
  const int nr = p->n_ranks > 0 ? p->n_ranks : 1;
  if (p->rank < 0 || p->rank >= nr) return fail(PT_ERR_INVALID, "rank %d outside [0,%d)", p->rank, nr);
  // PT_PCG_SEQ, the reference's own streams: the JITTER stream is one sequential generator from which every sample draws
  // exactly two numbers (imagetracer.py:84-101), so sample k of pixel i starts 2 (i S^2 + k) draws in -- parallel by
  // jump-ahead, and exact.  The path tracer's SCATTERING stream (render.py:118,128) is consumed in the order the paths of
  // ALL pixels end in, each taking a number of draws only known once it has been traced: serial by construction.
  if (p->pcg_mode == PT_PCG_SEQ && p->renderer == PT_RENDERER_PATHTRACER)
    return fail(PT_ERR_UNSUPPORTED,
                "PT_PCG_SEQ with the path tracer: its scattering stream is ONE generator consumed in the order the paths "
                "of all pixels end in (render.py:118,128), which only a serial program reproduces; the device path "
                "implements PT_PCG_PIXEL and PT_PCG_SAMPLE for it (PT_PCG_SEQ is exact for OnOff, Flat and PointLight)");
  if (p->pcg_mode == PT_PCG_SEQ && p->samples_per_side > 0 &&
      (unsigned long long)p->width * p->height > (~0ULL >> 2) / ((unsigned long long)p->samples_per_side * p->samples_per_side))
    return fail(PT_ERR_INVALID, "PT_PCG_SEQ: the frame draws more than 2^63 jitter numbers");
  if (p->pcg_mode < PT_PCG_SEQ || p->pcg_mode > PT_PCG_SAMPLE)
    return fail(PT_ERR_INVALID, "unknown pcg_mode %d", p->pcg_mode);
  if (p->renderer == PT_RENDERER_PATHTRACER) {
    if (p->num_of_rays < 1)
      return fail(PT_ERR_INVALID, "num_of_rays must be >= 1 (the reference divides by it, render.py:139)");
    if (p->max_depth > 4096) return fail(PT_ERR_INVALID, "max_depth %d too large", p->max_depth);
  }
  if ((long long)p->width * p->height > (1LL << 40)) return fail(PT_ERR_INVALID, "image too large");
  return PT_OK;
}

// dynamic LDS above the default 64 KiB has to be asked for, once per kernel
static hipError_t path_lds_limit(const void *kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PT_LDS_BUDGET);
}

#ifndef PT_WAVES_POINTLIGHT
#define PT_WAVES_POINTLIGHT 3  // waves per SIMD pt_tile_kernel<POINTLIGHT> is compiled for (register budget 512 / that)
#endif

// the shapes' tables alone: what a query of the whole world shape by shape reads (the probes of ptrace_debug.h)
static void fill_shape_tables(const pt_scene *s, PtKArgs &a) {
  const PtSceneShared &sh = *s->sh;
  a.recs = sh.recs;
  a.aux = sh.aux;
  a.diag = sh.diag;
  a.bounds = sh.bounds;
  pt_fill_shape_counts(a, sh.sc);
}

// the scene as the kernels see it (launch(), pt_scene_kernel_args, pt_debug_lanes_probe): the tables here, the scalars from
// pt_frame_args.h
static void fill_scene_args(const pt_scene *s, PtKArgs &a) {
  const PtSceneShared &sh = *s->sh;
  fill_shape_tables(s, a);
  a.hoist = s->hoist;
  a.hoist_diag = s->hoist_diag;
  a.queue = s->queue;
  a.bsoa = sh.bsoa;
  a.grid_cells = sh.grid_cells;
  a.grid_occ = sh.grid_occ;
  a.grid_balls = sh.grid_balls;
  a.grid_slots = sh.grid_slots;
  a.grid_always = sh.grid_always;
  a.lights = sh.lights;
  a.tex = sh.tex;
  a.tex_data = sh.tex_data;
  pt_fill_scene_scalars(a, sh.sc, pt_tuning());
}

// The scene's block for a library of kernels built from this tree but linked into another shared object (ptrace_rays.hip:
// ray batches): fill_scene_args with `cold` pointing to a device-resident copy of the same block, which this handle owns.
// Nothing a frame sets is in it (camera, output, workspace: zero), so it stays valid while frames run through the handle.
extern "C" int pt_scene_kernel_args(pt_scene *s, void *out, size_t out_bytes) {
  if (!s || !out) return fail(PT_ERR_INVALID, "null argument");
  if (out_bytes != sizeof(PtKArgs))
    return fail(PT_ERR_INVALID, "argument block of %zu bytes asked for, this library's has %zu: caller built from another tree?", out_bytes,
                sizeof(PtKArgs));
  HIP_TRY(hipSetDevice(s->device));
  PtKArgs a;
  memset(&a, 0, sizeof a);
  fill_scene_args(s, a);
  ColdArgs &c = s->scene_args;
  if (!c.dev) HIP_TRY(hipMalloc((void **)&c.dev, sizeof(PtKArgs)));
  a.cold = c.dev;
  if (!c.valid || memcmp(&c.last, &a, sizeof a) != 0) {  // (first call; or a tuning switch changed bs_levels in between)
    HIP_TRY(hipMemcpy(c.dev, &a, sizeof a, hipMemcpyHostToDevice));
    c.last = a;
    c.valid = true;
  }
  memcpy(out, &a, sizeof a);
  return PT_OK;
}

static_assert(PT_PLAN_BLOCK == PT_BLOCK && PT_PLAN_REGION == PT_REGION && PT_PLAN_CELL == PT_CELL && PT_PLAN_CELL_CHUNK == PT_CELL_CHUNK &&
                  PT_PLAN_TREE_FRAME == PT_TREE_FRAME && PT_PLAN_SCATTER_BLOCK == PT_SCATTER_BLOCK && PT_PLAN_DIAG_BYTES == sizeof(PtDiagRec) &&
                  PT_PLAN_REC_BYTES == sizeof(PtShapeRec) && PT_PLAN_AUX_BYTES == sizeof(PtShapeAux) && PT_PLAN_HANDOVER_HEADER == PT_HANDOVER_HEADER &&
                  PT_TREE_FRAME == 20,
              "pt_plan.h sizes the kernels' tiles and records by number: keep them equal to the kernels' own");

// grow-only device buffers of a handle: a launch that needs more lets the stream drain first
template <typename T>
static int ensure(T **ptr, size_t *have, size_t need, hipStream_t st) {
  if (need <= *have) return PT_OK;
  HIP_TRY(hipStreamSynchronize(st));
  if (*ptr) HIP_TRY(hipFree(*ptr));
  *ptr = nullptr;
  *have = 0;
  HIP_TRY(hipMalloc((void **)ptr, need * sizeof(T)));
  *have = need;
  return PT_OK;
}

// The cold half of the argument block is read from device memory: refresh the copy when it changed
// (the output pointer stays a by-value argument: double-buffered frames alternate it every launch).
static int refresh_cold(ColdArgs &c, const PtKArgs &a, hipStream_t st) {
  PtKArgs cold = a;
  cold.out = nullptr;
  cold.qpar = 0;
  if (c.valid && c.stream == st && memcmp(&c.last, &cold, sizeof cold) == 0) return PT_OK;
  // pageable source: the runtime stages the bytes before returning, so `cold` may go out of scope
  HIP_TRY(hipMemcpyAsync(c.dev, &cold, sizeof cold, hipMemcpyHostToDevice, st));
  c.last = cold;
  c.valid = true;
  c.stream = st;
  return PT_OK;
}

// ---- a frame's launches -------------------------------------------------------------------------------------------------------
// The kernels of one frame on its stream; the LAST one launched is the render kernel proper (pt_stats.vgprs).  Timing: the
// frame's first launch carries the start event and its last one the stop event IN the dispatch itself (hipExtLaunchKernel,
// the call hipExtLaunchKernelGGL makes: the events take the kernel's own begin / end timestamps), so a timed frame costs no
// barrier packet on the stream and the interval holds the frame's kernels, not the launch gaps around them.
struct FrameLaunches {
  hipStream_t st;
  hipEvent_t ev_a, ev_b;  // null: the frame is not timed
  bool started = false;
  const void *main_fn = nullptr;
  void operator()(const void *fn, dim3 grid, size_t lds, bool last, void **args) {
    main_fn = fn;
    (void)hipExtLaunchKernel(fn, grid, dim3(PT_BLOCK), args, lds, st, started ? nullptr : ev_a, last ? ev_b : nullptr, 0);
    started = true;
  }
};

// The variants of a kernel by what the plan names (one or two of its fields); the last row is the one for everything else.
// The tables stand where the frame launches from them, in the order the variants were always named in: the order in which
// this file first names its kernels is the order of the device code (build.code_hash).
struct KernelRow {
  int a, b;
  const void *fn;
  template <typename F>
  KernelRow(int a_, int b_, F *f) : a(a_), b(b_), fn((const void *)f) {}
};
template <size_t N>
static const void *pick(const KernelRow (&rows)[N], int a, int b = 0) {
  for (size_t i = 0; i + 1 < N; ++i)
    if (rows[i].a == a && rows[i].b == b) return rows[i].fn;
  return rows[N - 1].fn;
}

// the per-shape constants of a perspective camera's primary rays, unless the handle holds this camera's already
static void enqueue_hoist(pt_scene *s, const pt_camera *cam, const PtKArgs &a, hipStream_t st) {
  if (s->hoist_valid && s->hoist_stream == st && memcmp(&s->hoist_cam, cam, sizeof(pt_camera)) == 0) return;
  double o[3];
  pt_hoist_origin(cam, o);
  const V3 w = {o[0], o[1], o[2]};
  hipLaunchKernelGGL(pt_prep_hoist, dim3((a.n_shapes + 255) / 256), dim3(256), 0, st, a.recs, s->hoist, s->hoist_diag, a.n_shapes, a.n_diag, w);
  s->hoist_cam = *cam;
  s->hoist_valid = true;
  s->hoist_stream = st;
}

// render.py:100-101: every primary call returns Color(0, 0, 0) without a world query
static int enqueue_zero_frame(pt_scene *s, const pt_params *p, void *out_dev, hipStream_t st) {
  HIP_TRY(hipEventRecord(s->ev0, st));
  HIP_TRY(hipMemsetAsync(out_dev, 0, pt_output_bytes(p), st));
  HIP_TRY(hipEventRecord(s->ev1, st));
  if (s->count_rays) {
    HIP_TRY(hipMemsetAsync(s->ray_counter, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemcpyAsync(s->ray_counter_host, s->ray_counter, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s->ev_count, st));
    s->count_pending = true;
  }
  return PT_OK;
}

// The handle's buffers as this frame needs them (grow-only), and their pointers in the block.  The workspace (argument block
// copy, hoisted constants, region/cell tables, frame stack, ray partials) is shared by all launches of a handle.
static int frame_buffers(pt_scene *s, const pt_params *p, const PtPlan &pl, PtKArgs &a, hipStream_t st) {
  if (s->count_rays) {
    size_t have = (size_t)s->ray_partials_n * 2;
    int rc = ensure(&s->ray_partials, &have, (size_t)(pl.grid + pl.grid_first + pl.grid_q) * 2, st);
    s->ray_partials_n = (int)(have / 2);
    if (rc) return rc;
    a.ray_counter = s->ray_partials;
  }
  if (p->renderer == PT_RENDERER_PATHTRACER) {
    // the queue block (head, unit counts, F; pt_path.h: pt_unit_scatter) starts every frame zeroed: by the path
    // kernel of the frame before (it clears the OTHER block), by a memset after anything went wrong in between
    a.qpar = s->queue_parity;
    s->queue_last = s->queue + (size_t)a.qpar * PT_QUEUE_WORDS;
    if (!s->queue_clean) HIP_TRY(hipMemsetAsync(s->queue_last, 0, PT_QUEUE_WORDS * sizeof(unsigned long long), st));
    s->queue_clean = false;  // (true again once this frame's path kernel is enqueued)
    size_t have = s->ws_bytes / sizeof(double);
    int rc = ensure(&s->ws, &have, (pl.ws_bytes + sizeof(double) - 1) / sizeof(double), st);
    s->ws_bytes = have * sizeof(double);
    if (rc) return rc;
    a.ws = s->ws;
  }
  // path tracer: per-region masks/keys from the first pass, work units for the second from pt_unit_scatter
  if (pl.path_tiled) {
    int rc = ensure(&s->region_keys, &s->region_keys_cap, (size_t)pl.nregions, st);
    if (!rc) rc = ensure(&s->region_mask, &s->region_mask_cap, (size_t)pl.nregions, st);
    if (!rc) rc = ensure(&s->units, &s->units_cap, (size_t)pl.units_need, st);
    if (!rc && pl.q_alt) rc = ensure(&s->handover, &s->handover_doubles, pl.handover_doubles, st);
    if (!rc && pl.q_alt) rc = ensure(&s->units_handed, &s->units_handed_n, (size_t)pl.handover_cap, st);
    if (rc) return rc;
    a.units = s->units;
    a.region_keys = s->region_keys;
    a.region_mask = s->region_mask;
    a.handover = s->handover;
    a.units_handed = s->units_handed;
    s->last_handover_cap = a.handover_cap;
  }
  // large scenes: two-level culling (cells of PT_CELL x PT_CELL global pixels, then 8x8 tiles)
  if (pl.hier) {
    int rc = ensure(&s->cell_list, &s->cell_list_cap, (size_t)pl.ncells * pl.cell_stride, st);
    if (!rc) rc = ensure(&s->cell_count, &s->cell_count_cap, (size_t)pl.ncells, st);
    if (rc) return rc;
    a.cell_list = s->cell_list;
    a.cell_count = s->cell_count;
  }
  return PT_OK;
}

// large scenes: every cell's survivors, in front of the kernel whose tiles cull from them
static int enqueue_cells(pt_scene *s, const PtPlan &pl, PtKArgs &a, FrameLaunches &go) {
  if (pl.cell_chunk_len > PT_CELL_CHUNK) return fail(PT_ERR_INVALID, "internal: cell chunk exceeds its LDS staging");
  HIP_TRY(hipMemsetAsync(s->cell_count, 0, (size_t)pl.ncells * sizeof(int), go.st));
  int chunks = pl.cell_chunks, chunk_len = pl.cell_chunk_len;
  void *args[] = {&a, &chunks, &chunk_len};
  go((const void *)pt_cell_kernel, dim3(pl.cell_groups * pl.cell_chunks), 0, false, args);
  return PT_OK;
}

// a hit-record frame: the tile kernel's culling modes, or every shape through world_query
static int enqueue_hits(pt_scene *s, const PtPlan &pl, bool cull, PtKArgs &a, int channels, FrameLaunches &go) {
  const size_t lds = cull ? pl.lds_tile : 0;
  s->stats.lds_bytes = (int)lds;
  if (cull && pl.hier)
    if (int rc = enqueue_cells(s, pl, a, go)) return rc;
  // pt_hits_kernel<HIER, ORTHO, CULL> (pt_hits.h) by (cull, then: pl.tile_mode with it, pl.ortho without)
  static const KernelRow hits[] = {
      {0, 1, pt_hits_kernel<false, true, false>}, {0, 0, pt_hits_kernel<false, false, false>},
      {1, PT_TILE_HIER, pt_hits_kernel<true, false, true>}, {1, PT_TILE_ORTHO, pt_hits_kernel<false, true, true>},
      {1, PT_TILE_PLAIN, pt_hits_kernel<false, false, true>}};
  void *args[] = {&a, &channels};
  go(pick(hits, cull, cull ? pl.tile_mode : (int)pl.ortho), dim3(pl.grid), lds, true, args);
  return PT_OK;
}

// small worlds, 16x16 tiles: the shapes' Flat colours ride in LDS for shading (Flat; OnOff reads none of them)
static int enqueue_tile4(pt_scene *s, const PtPlan &pl, int R, PtKArgs &a, FrameLaunches &go) {
  s->stats.lds_bytes = (int)pl.lds_main;
  // pt_tile4_kernel<renderer, LDS> by (renderer, pl.t4lds)
  static const KernelRow tile4[] = {{PT_RENDERER_ONOFF, 0, pt_tile4_kernel<PT_RENDERER_ONOFF, false>},
                                    {PT_RENDERER_FLAT, 1, pt_tile4_kernel<PT_RENDERER_FLAT, true>},
                                    {PT_RENDERER_FLAT, 0, pt_tile4_kernel<PT_RENDERER_FLAT, false>}};
  const bool staged = R != PT_RENDERER_ONOFF && pl.t4lds;
  if (staged) {
    // the staged variant: every wave copies the Flat palette behind aux[] into a slice of its own with 16-byte global -> LDS
    // loads.  The tables and the dynamic LDS block (it follows the kernel's static LDS) must be 16-byte aligned, and the four
    // slices must lie inside the block, which the plan still sizes for the whole scene image
    static int static_lds = -1;  // (a property of the code: looked up once)
    if (static_lds < 0) {
      hipFuncAttributes fa;
      HIP_TRY(hipFuncGetAttributes(&fa, tile4[1].fn));
      static_lds = (int)fa.sharedSizeBytes;
    }
    if ((((uintptr_t)a.recs | (uintptr_t)a.aux) & 15) != 0 || (static_lds & 15) != 0)
      return fail(PT_ERR_INVALID, "internal: pt_tile4_kernel<FLAT, LDS> needs 16-byte aligned shape tables and LDS");
    const size_t pal_bytes = (size_t)pt_flat_pal_chunks(a.n_shapes) * PT_FLAT_PAL_CHUNK;
    if (pt_flat_pal_chunks(a.n_shapes) > PT_TILE4_PAL_CHUNKS ||
        (size_t)(PT_BLOCK / 64 - 1) * pt_flat_pal_slice(a.n_shapes) + pal_bytes > pl.lds_main)
      return fail(PT_ERR_INVALID, "internal: the four palette slices of pt_tile4_kernel<FLAT, LDS> do not fit its LDS block");
  }
  void *args[] = {&a};
  go(pick(tile4, R, staged), dim3(pl.grid4_x, pl.grid4_y, 1), pl.lds_main, true, args);
  return PT_OK;
}

// 8x8 tiles: the frame of OnOff / Flat / PointLight, the path tracer's first pass
static int enqueue_tiles(pt_scene *s, const PtPlan &pl, int R, PtKArgs &a, FrameLaunches &go) {
  s->stats.lds_bytes = (int)pl.lds_tile;
  if (pl.hier)
    if (int rc = enqueue_cells(s, pl, a, go)) return rc;
  // pt_tile_kernel<renderer, waves, HIER, ORTHO, BLOCKS> by (renderer, pl.tile_mode)
  static const KernelRow tiles[] = {
      {PT_RENDERER_ONOFF, PT_TILE_HIER, pt_tile_kernel<PT_RENDERER_ONOFF, 4, true>},
      {PT_RENDERER_ONOFF, PT_TILE_ORTHO, pt_tile_kernel<PT_RENDERER_ONOFF, 4, false, true>},
      {PT_RENDERER_ONOFF, PT_TILE_PLAIN, pt_tile_kernel<PT_RENDERER_ONOFF, 4, false>},
      {PT_RENDERER_FLAT, PT_TILE_HIER, pt_tile_kernel<PT_RENDERER_FLAT, 4, true>},
      {PT_RENDERER_FLAT, PT_TILE_ORTHO, pt_tile_kernel<PT_RENDERER_FLAT, 4, false, true>},
      {PT_RENDERER_FLAT, PT_TILE_PLAIN, pt_tile_kernel<PT_RENDERER_FLAT, 4, false>},
      {PT_RENDERER_POINTLIGHT, PT_TILE_HIER, pt_tile_kernel<PT_RENDERER_POINTLIGHT, PT_WAVES_POINTLIGHT, true>},
      {PT_RENDERER_POINTLIGHT, PT_TILE_ORTHO, pt_tile_kernel<PT_RENDERER_POINTLIGHT, PT_WAVES_POINTLIGHT, false, true>},
      {PT_RENDERER_POINTLIGHT, PT_TILE_PLAIN, pt_tile_kernel<PT_RENDERER_POINTLIGHT, PT_WAVES_POINTLIGHT, false>},
      {PT_RENDERER_PATHTRACER, PT_TILE_BLOCKS, pt_tile_kernel<PT_RENDERER_PATHTRACER, 4, false, false, true>},
      {PT_RENDERER_PATHTRACER, PT_TILE_HIER, pt_tile_kernel<PT_RENDERER_PATHTRACER, 4, true>},
      {PT_RENDERER_PATHTRACER, PT_TILE_ORTHO, pt_tile_kernel<PT_RENDERER_PATHTRACER, 4, false, true>},
      {PT_RENDERER_PATHTRACER, PT_TILE_PLAIN, pt_tile_kernel<PT_RENDERER_PATHTRACER, 4, false>}};
  int pgrid = pl.path_tiled ? pl.grid : 0;  // (the first pass is told the second pass's grid)
  void *args[] = {&a, &pgrid};
  go(pick(tiles, R, pl.tile_mode), dim3(pl.path_tiled ? pl.grid_first : pl.grid), pl.lds_tile, !pl.path_tiled, args);
  return PT_OK;
}

// the path tracer's second pass: the pixels the first one flagged, fullest regions first
static int enqueue_second_pass(pt_scene *s, const PtPlan &pl, PtKArgs &a, bool measured, FrameLaunches &go) {
  const hipStream_t st = go.st;
  if (pl.tree)  // one pixel per unit: "64 lanes per pixel, whatever the number of flagged pixels"
    hipLaunchKernelGGL(pt_unit_scatter, dim3(pl.grid_scatter), dim3(PT_SCATTER_BLOCK), 0, st, s->region_keys, s->region_mask, pl.nregions,
                       s->units, (int)s->units_cap, s->queue_last, (long long)1 << 60, 64, 1, pl.q_min, pl.q_budget_per_flagged, pl.q_budget_min);
  else
    hipLaunchKernelGGL(pt_unit_scatter, dim3(pl.grid_scatter), dim3(PT_SCATTER_BLOCK), 0, st, s->region_keys, s->region_mask, pl.nregions,
                       s->units, (int)s->units_cap, s->queue_last, pl.lanes_cap, pl.nsamp, (long long)pl.min_rounds);
  if (pl.q_alt) {
    // num_of_rays > 1: the one-queue kernel IN FRONT of the tree kernel, with an argument block of its own; it returns at once
    // unless PT_Q_CHOICE says 1, and then leaves the pixels over its budget to the tree kernel behind it (PT_Q_HEAVY)
    PtKArgs aq = pt_one_queue_args(a, pl);
    aq.cold = s->args2.dev;
    if (int rc = refresh_cold(s->args2, aq, st)) return rc;
    static const KernelRow alts[] = {
        {PT_ALT_FLAGGED_LEAN_LDS, 0, pt_path_flagged_kernel<1, 1>}, {PT_ALT_FLAGGED_LEAN_SPLIT, 0, pt_path_flagged_kernel<1, 2>},
        {PT_ALT_FLAGGED_SPLIT, 0, pt_path_flagged_kernel<0, 2>}, {PT_ALT_FLAGGED_LDS, 0, pt_path_flagged_kernel<0, 1>}};
    const void *alt = pick(alts, pl.alt);
    HIP_TRY(path_lds_limit(alt, pl.lds_q));
    void *args[] = {&aq};
    go(alt, dim3(pl.grid_q), pl.lds_q, false, args);
  }
  static const KernelRow seconds[] = {
      {PT_SECOND_TREE_LEAN, 0, pt_path_tree_kernel<true>}, {PT_SECOND_TREE_LEAN_SCENE, 0, pt_path_tree_kernel<true, true>},
      {PT_SECOND_TREE, 0, pt_path_tree_kernel<false>}, {PT_SECOND_REGIONS_LDS_SCENE_LEAN, 0, pt_path_regions_kernel<true, true, 1>},
      {PT_SECOND_REGIONS_LDS_SCENE, 0, pt_path_regions_kernel<true, true>}, {PT_SECOND_REGIONS_LDS_NOGRID, 0, pt_path_regions_kernel<true, false, 2>},
      {PT_SECOND_REGIONS_LDS, 0, pt_path_regions_kernel<true>}, {PT_SECOND_REGIONS_HBM, 0, pt_path_regions_kernel<false>}};
  const void *second = pick(seconds, pl.second);
  HIP_TRY(path_lds_limit(second, pl.lds_main));
  void *args[] = {&a};
  go(second, dim3(pl.grid), pl.lds_main, true, args);
  // (pt_stats.vgprs: the tree kernel's; pt_stats.kernel follows the device's choice, see fold_stats -- only when the frame
  // is measured at all: a frame loop with timing and counting off enqueues neither the copy nor its event)
  if (pl.q_alt && measured) {
    HIP_TRY(hipMemcpyAsync(s->ray_counter_host + 2, s->queue_last + PT_Q_CHOICE, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    s->choice_pending = true;
  }
  return PT_OK;
}

// no tile culling at all (worlds of fewer than four shapes, PTRACE_CULL=0): a lane per pixel
static void enqueue_untiled(const PtPlan &pl, int R, PtKArgs &a, FrameLaunches &go) {
  void *args[] = {&a};
  if (R == PT_RENDERER_PATHTRACER) {
    go((const void *)pt_path_kernel, dim3(pl.grid), 0, true, args);
    return;
  }
  // pt_simple_kernel<renderer, HOIST> by (renderer, pl.simple_hoist)
  static const KernelRow simple[] = {
      {PT_RENDERER_ONOFF, 1, pt_simple_kernel<PT_RENDERER_ONOFF, true>}, {PT_RENDERER_ONOFF, 0, pt_simple_kernel<PT_RENDERER_ONOFF, false>},
      {PT_RENDERER_FLAT, 1, pt_simple_kernel<PT_RENDERER_FLAT, true>}, {PT_RENDERER_FLAT, 0, pt_simple_kernel<PT_RENDERER_FLAT, false>},
      {PT_RENDERER_POINTLIGHT, 1, pt_simple_kernel<PT_RENDERER_POINTLIGHT, true>}, {PT_RENDERER_POINTLIGHT, 0, pt_simple_kernel<PT_RENDERER_POINTLIGHT, false>}};
  go(pick(simple, R, pl.simple_hoist), dim3(pl.grid), 0, true, args);
}

// registers per lane of a kernel (hipFuncGetAttributes; looked up once per kernel)
static int kernel_vgprs(const void *fn) {
  static std::vector<std::pair<const void *, int>> known;
  for (const auto &kv : known)
    if (kv.first == fn) return kv.second;
  hipFuncAttributes fa;
  const int regs = hipFuncGetAttributes(&fa, fn) == hipSuccess ? fa.numRegs : 0;
  (void)hipGetLastError();
  known.push_back({fn, regs});
  return regs;
}

// launch() = plan (pt_plan.h: a pure function of the scene's facts, the camera, the parameters and the tuning table) +
// argument block (pt_frame_args.h: a pure function of the same and the plan) + enqueue (here and in the helpers above: the
// handle's buffers, the launches the plan names, the bookkeeping of pt_stats -- no decision is taken here).
// hits_channels >= 0: a hit-record frame (pt_render_hits; pt_hits_plan.h) of those channels instead of the renderer's colours.
static int launch(pt_scene *s, const pt_camera *cam, const pt_params *p, void *out_dev, hipStream_t st, int hits_channels = -1) {
  const PtTuning &tn = pt_tuning();
  PtPlan pl;
  bool hits_cull = false;
  if (hits_channels >= 0)
    pt_make_hits_plan(scene_facts(s), cam, p, tn, pl, hits_cull);
  else
    pt_make_plan(scene_facts(s), cam, p, tn, pl);

  PtKArgs a;
  memset(&a, 0, sizeof a);
  fill_scene_args(s, a);
  pt_fill_frame_args(a, cam, p, pl, tn, s->dome_shortcut, s->sh->dome_cands);
  a.out = out_dev;

  // All launches of a handle are ordered by being on ONE stream.  A launch on another stream than the previous one first
  // lets that stream drain (host-side wait; a rare event).
  if (s->launched && s->last_stream != st) {
    if (hipStreamSynchronize(s->last_stream) != hipSuccess) (void)hipGetLastError();  // (a destroyed stream has nothing in flight)
  }
  s->last_stream = st;
  s->launched = true;
  s->count_pending = false;
  s->choice_pending = false;
  s->stats.n_pixels = (uint64_t)pl.npix;
  if (pl.npix == 0) return PT_OK;
  s->stats.grid = pl.grid;
  s->stats.block = PT_BLOCK;
  s->stats.lds_bytes = 0;
  s->stats.kernel = pl.kernel;

  if (pl.hoist) enqueue_hoist(s, cam, a, st);
  if (pl.zero_frame) return enqueue_zero_frame(s, p, out_dev, st);
  if (int rc = frame_buffers(s, p, pl, a, st)) return rc;
  a.cold = s->args.dev;
  if (int rc = refresh_cold(s->args, a, st)) return rc;

  const bool prof = s->timing && s->profiling && (size_t)(2 * s->prof_used + 1) < s->prof.size();
  FrameLaunches go{st, s->timing ? (prof ? s->prof[2 * s->prof_used] : s->ev0) : nullptr,
                   s->timing ? (prof ? s->prof[2 * s->prof_used + 1] : s->ev1) : nullptr};
  const int R = p->renderer;
#ifdef PT_DEBUG_TIME
  if (pl.tile4 || ((pl.tile || pl.path_tiled) && R != PT_RENDERER_PATHTRACER)) {
    s->queue_last = s->queue;  // (a.qpar = 0: the section sums land in block 0)
    HIP_TRY(hipMemsetAsync(s->queue, 0, 16 * sizeof(unsigned long long), st));
    if (s->queue_parity == 0) s->queue_clean = false;
  }
#endif
  int rc = PT_OK;
  if (hits_channels >= 0) {
    rc = enqueue_hits(s, pl, hits_cull, a, hits_channels, go);
  } else if (pl.tile4) {
    rc = enqueue_tile4(s, pl, R, a, go);
  } else if (pl.tile || pl.path_tiled) {
    rc = enqueue_tiles(s, pl, R, a, go);
    if (!rc && pl.path_tiled) rc = enqueue_second_pass(s, pl, a, s->timing || s->count_rays || prof, go);
  } else {
    enqueue_untiled(pl, R, a, go);
  }
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  if (R == PT_RENDERER_PATHTRACER) {  // its path kernel is enqueued: the other queue block will be zero
    s->queue_parity ^= 1;
    s->queue_clean = true;
  }
  if (go.main_fn) s->stats.vgprs = kernel_vgprs(go.main_fn);
  s->stats_valid = s->timing && !prof;
  if (prof) s->prof_used++;
  if (s->count_rays) {
    hipLaunchKernelGGL(pt_sum_counts, dim3(1), dim3(256), 0, st, s->ray_partials, pl.grid + pl.grid_first + pl.grid_q, s->ray_counter);
    HIP_TRY(hipMemcpyAsync(s->ray_counter_host, s->ray_counter, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    // ev1 was recorded BEFORE the count left the device: whoever reads ray_counter_host waits for this one
    HIP_TRY(hipEventRecord(s->ev_count, st));
    s->count_pending = true;
  } else if (s->choice_pending) {
    HIP_TRY(hipEventRecord(s->ev_count, st));
  }
  return PT_OK;
}

static int fold_stats(pt_scene *s) {
  if (!s->pending) return PT_OK;
  float ms = 0.f;
  if (s->stats_valid) HIP_TRY(hipEventSynchronize(s->pending_copy ? s->ev2 : s->ev1));
  if (!s->stats_valid) {
    HIP_TRY(hipStreamSynchronize(s->last_stream));
    s->stats.kernel_ms = s->stats.total_ms = 0.0;
  } else if (s->stats.n_pixels > 0) {
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->stats.kernel_ms = ms;
    if (s->pending_copy) {
      HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev2));
    }
    s->stats.total_ms = ms;
  } else {
    s->stats.kernel_ms = s->stats.total_ms = 0.0;
  }
  if (s->count_pending || s->choice_pending) HIP_TRY(hipEventSynchronize(s->ev_count));
  if (s->count_pending) {
    s->count_pending = false;
    s->stats.n_rays = s->ray_counter_host[0];
    s->stats.n_rays_resolved = s->ray_counter_host[1];
  } else {
    s->stats.n_rays = s->stats.n_rays_resolved = 0;  // (no pixels, or counting off)
  }
  if (s->choice_pending) {  // which of the two enqueued second-pass kernels the device let work (PT_Q_CHOICE)
    s->choice_pending = false;
    s->stats.kernel = s->ray_counter_host[2] ? PT_KERNEL_PATH : PT_KERNEL_PATH_TREE;
  }
  s->pending = false;
  s->pending_copy = false;
  return PT_OK;
}

// a frame (hits_channels >= 0: a hit-record frame) into a device buffer: asynchronous when the caller names a stream
static int render_to_device(pt_scene *s, const pt_camera *cam, const pt_params *p, void *out_dev, void *stream, int hits_channels = -1) {
  HIP_TRY(hipSetDevice(s->device));
  // an earlier asynchronous render that was never synchronised simply loses its statistics:
  // folding them here would block the host on the device every frame
  s->pending = false;
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  int rc = launch(s, cam, p, out_dev, st, hits_channels);
  if (rc) return rc;
  if (s->stats.n_pixels > 0) {
    s->pending = true;
    s->pending_copy = false;
  }
  if (!stream) return pt_sync(s);
  return PT_OK;
}

// ... and into a host buffer of `need` bytes, through the handle's staging buffer: kernel + copy, synchronised
static int render_to_host(pt_scene *s, const pt_camera *cam, const pt_params *p, void *out_host, size_t need, int hits_channels = -1) {
  HIP_TRY(hipSetDevice(s->device));
  int rc = s->pending ? fold_stats(s) : PT_OK;
  if (rc) return rc;
  if ((rc = ensure(&s->out_dev, &s->out_dev_bytes, need, s->stream))) return rc;
  rc = launch(s, cam, p, s->out_dev, s->stream, hits_channels);
  if (rc) return rc;
  if (need > 0) {
    // (a hit-record frame: the padding behind the shape plane is the only part no lane writes, the copy carries whatever the buffer held)
    HIP_TRY(hipMemcpyAsync(out_host, s->out_dev, need, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev2, s->stream));
    s->pending = true;
    s->pending_copy = true;
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return fold_stats(s);
}

extern "C" int pt_render_device(pt_scene *s, const pt_camera *cam, const pt_params *p, void *out_dev,
                                size_t out_bytes, void *stream) {
  if (!s) return fail(PT_ERR_INVALID, "null argument");
  int rc = check_params(cam, p);
  if (rc) return rc;
  const size_t need = pt_output_bytes(p);
  if (out_bytes < need) return fail(PT_ERR_SIZE, "output buffer too small: %zu < %zu bytes", out_bytes, need);
  if (need > 0 && !out_dev) return fail(PT_ERR_INVALID, "null output buffer");
  return render_to_device(s, cam, p, out_dev, stream);
}

extern "C" int pt_sync(pt_scene *s) {
  if (!s) return fail(PT_ERR_INVALID, "null scene");
  HIP_TRY(hipSetDevice(s->device));
  return fold_stats(s);
}

extern "C" int pt_render(pt_scene *s, const pt_camera *cam, const pt_params *p, void *out_host,
                         size_t out_bytes) {
  if (!s) return fail(PT_ERR_INVALID, "null argument");
  int rc = check_params(cam, p);
  if (rc) return rc;
  const size_t need = pt_output_bytes(p);
  if (out_bytes < need) return fail(PT_ERR_SIZE, "output buffer too small: %zu < %zu bytes", out_bytes, need);
  if (need > 0 && !out_host) return fail(PT_ERR_INVALID, "null output buffer");
  return render_to_host(s, cam, p, out_host, need);
}

// ---- hit-record frames (include/ptrace.h, ABI 1.6) -------------------------------------------------------------------
static int hits_planes_of(int channel) {
  switch (channel) {
    case PT_HIT_T: return 1;
    case PT_HIT_POINT: return 3;
    case PT_HIT_NORMAL: return 3;
    case PT_HIT_UV: return 2;
    case PT_HIT_RAY: return 6;
    default: return 0;
  }
}
static bool hits_channels_ok(int channels) { return channels >= 0 && (channels & ~PT_HIT_ALL) == 0; }
// values per plane: nsamp * rows_for_rank * W
static long long hits_plane_values(const pt_params *p) {
  if (!p || p->width <= 0 || p->samples_per_side < 0) return 0;
  const long long S = p->samples_per_side;
  return (S > 0 ? S * S : 1) * (long long)pt_rows_for_rank(p) * p->width;
}
// the fields a hit-record frame does not read, set to values every check accepts
static pt_params hits_params(const pt_params *p) {
  pt_params q = *p;
  q.renderer = PT_RENDERER_FLAT;
  q.out_format = PT_OUT_F64;
  q.num_of_rays = 1;
  q.max_depth = 0;
  return q;
}

extern "C" size_t pt_hits_bytes(const pt_params *p, int channels) {
  if (!p || !hits_channels_ok(channels)) return 0;
  const long long n = hits_plane_values(p);
  int planes = 0;
  for (int bit = 1; bit <= PT_HIT_RAY; bit <<= 1)
    if (channels & bit) planes += hits_planes_of(bit);
  return (size_t)((n * 4 + 7) & ~7LL) + (size_t)n * 8 * (size_t)planes;
}

extern "C" long long pt_hits_plane_offset(const pt_params *p, int channels, int channel, int component) {
  if (!p || !hits_channels_ok(channels)) return fail(PT_ERR_INVALID, "unknown hit channel bits %#x", channels);
  if (channel == 0) return component == 0 ? 0 : PT_ERR_INVALID;
  if (hits_planes_of(channel) == 0 || !(channels & channel) || component < 0 || component >= hits_planes_of(channel))
    return PT_ERR_INVALID;
  const long long n = hits_plane_values(p);
  long long planes = 0;
  for (int bit = 1; bit < channel; bit <<= 1)
    if (channels & bit) planes += hits_planes_of(bit);
  return ((n * 4 + 7) & ~7LL) + n * 8 * (planes + component);
}

static int hits_check(pt_scene *s, const pt_camera *cam, const pt_params *p, int channels, const void *out, size_t out_bytes,
                      pt_params &q) {
  if (!s || !cam || !p) return fail(PT_ERR_INVALID, "null argument");
  if (!hits_channels_ok(channels)) return fail(PT_ERR_INVALID, "unknown hit channel bits %#x", channels);
  q = hits_params(p);
  int rc = check_params(cam, &q);
  if (rc) return rc;
  const size_t need = pt_hits_bytes(&q, channels);
  if (out_bytes < need) return fail(PT_ERR_SIZE, "hit-record buffer too small: %zu < %zu bytes", out_bytes, need);
  if (need > 0 && !out) return fail(PT_ERR_INVALID, "null output buffer");
  return PT_OK;
}

extern "C" int pt_render_hits_device(pt_scene *s, const pt_camera *cam, const pt_params *p, int channels, void *out_dev,
                                     size_t out_bytes, void *stream) {
  pt_params q;
  int rc = hits_check(s, cam, p, channels, out_dev, out_bytes, q);
  if (rc) return rc;
  return render_to_device(s, cam, &q, out_dev, stream, channels);
}

extern "C" int pt_render_hits(pt_scene *s, const pt_camera *cam, const pt_params *p, int channels, void *out_host,
                              size_t out_bytes) {
  pt_params q;
  int rc = hits_check(s, cam, p, channels, out_host, out_bytes, q);
  if (rc) return rc;
  return render_to_host(s, cam, &q, out_host, pt_hits_bytes(&q, channels), channels);
}

// Page-locked host memory for pt_render's output: the D2H copy then is one DMA at link speed into the
// caller's buffer (a pageable destination goes through the runtime's staging path at roughly 2/3 of it).
extern "C" int pt_host_alloc(size_t bytes, void **out) {
  if (!out) return fail(PT_ERR_INVALID, "null output pointer");
  *out = nullptr;
  if (bytes == 0) return PT_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NODEVICE, "no HIP device visible");
  hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    *out = nullptr;
    return fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, "hipHostMalloc(%zu) failed: %s", bytes,
                hipGetErrorString(e));
  }
  return PT_OK;
}

extern "C" int pt_host_free(void *p) {
  if (!p) return PT_OK;
  HIP_TRY(hipHostFree(p));
  return PT_OK;
}

// ---- device memory and streams for callers WITHOUT a GPU framework of their own (ABI 1.5) ----
// The `render` command leaves its frame in HBM (pt_render_device) and post-processes it there (pt_image_*): with these it needs
// no torch for the buffer.  Thin and error-coded; a caller that owns device tensors keeps passing their pointers.
extern "C" int pt_device_alloc(int device, size_t bytes, void **out) {
  if (!out) return fail(PT_ERR_INVALID, "null output pointer");
  *out = nullptr;
  if (bytes == 0) return PT_OK;
  int rc = device_ok(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) {
    *out = nullptr;
    return fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  return PT_OK;
}

extern "C" int pt_device_free(int device, void *p) {
  if (!p) return PT_OK;
  int rc = device_ok(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipFree(p));  // (waits for the device's work on it)
  return PT_OK;
}

extern "C" int pt_device_download(int device, void *dst_host, const void *src_dev, size_t bytes, void *stream) {
  if (bytes == 0) return PT_OK;
  if (!dst_host || !src_dev) return fail(PT_ERR_INVALID, "null argument");
  int rc = device_ok(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return PT_OK;
}

extern "C" int pt_stream_create(int device, void **out) {
  if (!out) return fail(PT_ERR_INVALID, "null output pointer");
  *out = nullptr;
  int rc = device_ok(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));  // (the legacy default stream serialises the host with the device)
  *out = (void *)st;
  return PT_OK;
}

extern "C" int pt_stream_sync(int device, void *stream) {
  int rc = device_ok(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return PT_OK;
}

extern "C" int pt_stream_destroy(int device, void *stream) {
  if (!stream) return PT_OK;
  int rc = device_ok(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  return PT_OK;
}

extern "C" int pt_get_stats(pt_scene *s, pt_stats *out) {
  if (!s || !out) return fail(PT_ERR_INVALID, "null argument");
  if (s->pending) {
    int rc = pt_sync(s);
    if (rc) return rc;
  }
  *out = s->stats;
  return PT_OK;
}

extern "C" int pt_set_timing(pt_scene *s, int enable) {
  if (!s) return fail(PT_ERR_INVALID, "null scene");
  s->timing = enable != 0;
  return PT_OK;
}

extern "C" int pt_profile_begin(pt_scene *s, int capacity) {
  if (!s || capacity <= 0 || capacity > (1 << 20)) return fail(PT_ERR_INVALID, "bad profiling capacity");
  HIP_TRY(hipSetDevice(s->device));
  while ((int)s->prof.size() < 2 * capacity) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    s->prof.push_back(e);
  }
  s->prof_used = 0;
  s->profiling = true;
  return PT_OK;
}

extern "C" int pt_profile_end(pt_scene *s, double *total_kernel_ms, int *launches) {
  if (!s || !total_kernel_ms || !launches) return fail(PT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  double sum = 0.0;
  for (int k = 0; k < s->prof_used; ++k) {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(s->prof[2 * k + 1]));
    HIP_TRY(hipEventElapsedTime(&ms, s->prof[2 * k], s->prof[2 * k + 1]));
    sum += ms;
  }
  *total_kernel_ms = sum;
  *launches = s->prof_used;
  s->profiling = false;
  s->prof_used = 0;
  return PT_OK;
}

// ---- HdrImage post-processing (pt_post.h) -------------------------------------------------------------
static int post_check(int device, const void *img, int fmt, int w, int h) {
  if (!img) return fail(PT_ERR_INVALID, "null image");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad image size %dx%d", w, h);
  if (fmt != PT_OUT_F64 && fmt != PT_OUT_F32) return fail(PT_ERR_INVALID, "unknown pixel format %d", fmt);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(PT_ERR_INVALID, "device %d out of range", device);
  HIP_TRY(hipSetDevice(device));
  return PT_OK;
}

static int post_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 4096)); }

static bool is_device_ptr(const void *p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // plain host memory: not an error for us
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// Image and output buffers may be device memory (a frame left in HBM by pt_render_device) or plain host
// memory (an HdrImage's array); host buffers are staged through a temporary device copy.
struct StagedImage {
  void *dev = nullptr;
  void *host = nullptr;
  size_t bytes = 0;
  bool owned = false;
  ~StagedImage() {
    if (owned && dev) (void)hipFree(dev);
  }
  int in(const void *p, size_t n, bool copy_in, hipStream_t st) {
    bytes = n;
    if (is_device_ptr(p)) {
      dev = const_cast<void *>(p);
      return PT_OK;
    }
    host = const_cast<void *>(p);
    owned = true;
    HIP_TRY(hipMalloc(&dev, n));
    if (copy_in) HIP_TRY(hipMemcpyAsync(dev, p, n, hipMemcpyHostToDevice, st));
    return PT_OK;
  }
  int out(hipStream_t st) {
    if (owned) {
      HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    return PT_OK;
  }
};

extern "C" int pt_image_pack_pfm(int device, const void *img, int fmt, int width, int height, int big_endian,
                                 void *out, void *stream) {
  int rc = post_check(device, img, fmt, width, height);
  if (rc) return rc;
  if (!out) return fail(PT_ERR_INVALID, "null output");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)width * height * 3;
  StagedImage si, so;
  if ((rc = si.in(img, (size_t)n * (fmt == PT_OUT_F32 ? 4 : 8), true, st))) return rc;
  if ((rc = so.in(out, (size_t)n * 4, false, st))) return rc;
  hipLaunchKernelGGL(pt_post_pfm_kernel, dim3(post_grid(n)), dim3(256), 0, st, si.dev, fmt == PT_OUT_F32 ? 1 : 0,
                     width, height, big_endian ? 1 : 0, (uint32_t *)so.dev);
  HIP_TRY(hipGetLastError());
  if ((rc = so.out(st))) return rc;
  if (!stream || si.owned) HIP_TRY(hipStreamSynchronize(st));
  return PT_OK;
}

// ---- sparse shards for the multi-GPU gather (pt_post.h) ----
extern "C" long long pt_image_sparse_fixed_bytes(long long n_pixels, int fmt) {
  if (n_pixels <= 0 || (fmt != PT_OUT_F64 && fmt != PT_OUT_F32)) return -1;
  const long long nt = (n_pixels + PT_SPARSE_RUN - 1) / PT_SPARSE_RUN;
  return 8 + (nt + 1) / 2 * 8 + nt * 3 * (fmt == PT_OUT_F32 ? 4 : 8);
}

static int sparse_check(int device, const void *a, const void *b, long long n_pixels, int fmt) {
  if (!a || !b) return fail(PT_ERR_INVALID, "null buffer");
  if (n_pixels <= 0 || n_pixels > (1LL << 37)) return fail(PT_ERR_INVALID, "bad pixel count %lld", n_pixels);
  if (fmt != PT_OUT_F64 && fmt != PT_OUT_F32) return fail(PT_ERR_INVALID, "unknown pixel format %d", fmt);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(PT_ERR_INVALID, "device %d out of range", device);
  HIP_TRY(hipSetDevice(device));
  return PT_OK;
}

extern "C" int pt_image_sparse_encode(int device, const void *shard_dev, long long n_pixels, int fmt, void *fixed_dev,
                                      void *payload_dev, void *stream) {
  int rc = sparse_check(device, shard_dev, fixed_dev, n_pixels, fmt);
  if (rc) return rc;
  if (!payload_dev) return fail(PT_ERR_INVALID, "null buffer");
  hipStream_t st = (hipStream_t)stream;
  const long long nt = (n_pixels + PT_SPARSE_RUN - 1) / PT_SPARSE_RUN, ntp = (nt + 1) / 2 * 2;
  int *place = (int *)((unsigned char *)fixed_dev + 8);
  void *firsts = (unsigned char *)fixed_dev + 8 + ntp * 4;
  const unsigned grid = (unsigned)((nt + 3) / 4);
  if (fmt == PT_OUT_F32)
    hipLaunchKernelGGL(pt_sparse_classify_kernel<uint32_t>, dim3(grid), dim3(256), 0, st, (const uint32_t *)shard_dev, n_pixels, nt, place, (uint32_t *)firsts);
  else
    hipLaunchKernelGGL(pt_sparse_classify_kernel<uint64_t>, dim3(grid), dim3(256), 0, st, (const uint64_t *)shard_dev, n_pixels, nt, place, (uint64_t *)firsts);
  hipLaunchKernelGGL(pt_sparse_scan_kernel, dim3(1), dim3(1024), 0, st, place, nt, ntp, (long long *)fixed_dev);
  if (fmt == PT_OUT_F32)
    hipLaunchKernelGGL(pt_sparse_pack_kernel<uint32_t>, dim3(grid), dim3(256), 0, st, (const uint32_t *)shard_dev, n_pixels, nt, (const int *)place, (uint32_t *)payload_dev);
  else
    hipLaunchKernelGGL(pt_sparse_pack_kernel<uint64_t>, dim3(grid), dim3(256), 0, st, (const uint64_t *)shard_dev, n_pixels, nt, (const int *)place, (uint64_t *)payload_dev);
  HIP_TRY(hipGetLastError());
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return PT_OK;
}

extern "C" int pt_image_sparse_decode(int device, const void *fixed_dev, const void *payload_dev, long long n_pixels, int fmt,
                                      void *out_dev, int width, int row_block, int n_ranks, int rank, void *stream) {
  int rc = sparse_check(device, fixed_dev, out_dev, n_pixels, fmt);
  if (rc) return rc;
  if (n_ranks > 1 && (width <= 0 || row_block <= 0 || rank < 0 || rank >= n_ranks || n_pixels % width != 0 || n_pixels >= (1LL << 31)))
    return fail(PT_ERR_INVALID, "bad placement: width %d, row_block %d, rank %d of %d", width, row_block, rank, n_ranks);
  hipStream_t st = (hipStream_t)stream;
  const long long nt = (n_pixels + PT_SPARSE_RUN - 1) / PT_SPARSE_RUN, ntp = (nt + 1) / 2 * 2;
  const int *place = (const int *)((const unsigned char *)fixed_dev + 8);
  const void *firsts = (const unsigned char *)fixed_dev + 8 + ntp * 4;
  const unsigned grid = (unsigned)((nt + 3) / 4);
  // (payload_dev may be null when no run needs it: then no run reads it)
  if (fmt == PT_OUT_F32)
    hipLaunchKernelGGL(pt_sparse_unpack_kernel<uint32_t>, dim3(grid), dim3(256), 0, st, place, (const uint32_t *)firsts, (const uint32_t *)payload_dev,
                       n_pixels, nt, (uint32_t *)out_dev, width, row_block, n_ranks, rank);
  else
    hipLaunchKernelGGL(pt_sparse_unpack_kernel<uint64_t>, dim3(grid), dim3(256), 0, st, place, (const uint64_t *)firsts, (const uint64_t *)payload_dev,
                       n_pixels, nt, (uint64_t *)out_dev, width, row_block, n_ranks, rank);
  HIP_TRY(hipGetLastError());
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return PT_OK;
}

extern "C" int pt_image_sparse_decode_many(int device, int n_shards, const void *const *fixed_dev, const void *const *payload_dev,
                                           const long long *n_pixels, const int *ranks, int fmt, void *frame_dev, int width,
                                           int row_block, int n_ranks, void *stream) {
  if (n_shards <= 0 || n_shards > PT_SPARSE_MANY || !fixed_dev || !payload_dev || !n_pixels || !ranks)
    return fail(PT_ERR_INVALID, "bad shard list (%d shards, at most %d)", n_shards, PT_SPARSE_MANY);
  if (n_ranks <= 1 || width <= 0 || row_block <= 0) return fail(PT_ERR_INVALID, "bad placement: width %d, row_block %d, %d ranks", width, row_block, n_ranks);
  PtSparseMany m;
  memset(&m, 0, sizeof m);
  long long most = 0;
  for (int k = 0; k < n_shards; ++k) {
    int rc = sparse_check(device, fixed_dev[k], frame_dev, n_pixels[k], fmt);
    if (rc) return rc;
    if (ranks[k] < 0 || ranks[k] >= n_ranks || n_pixels[k] % width != 0 || n_pixels[k] >= (1LL << 31))
      return fail(PT_ERR_INVALID, "bad shard %d: rank %d of %d, %lld pixels", k, ranks[k], n_ranks, n_pixels[k]);
    m.fixed[k] = fixed_dev[k];
    m.payload[k] = payload_dev[k];
    m.npix[k] = n_pixels[k];
    m.rank[k] = ranks[k];
    most = std::max(most, n_pixels[k]);
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)(((most + PT_SPARSE_RUN - 1) / PT_SPARSE_RUN + 3) / 4);
  if (fmt == PT_OUT_F32)
    hipLaunchKernelGGL(pt_sparse_unpack_many_kernel<uint32_t>, dim3(gx, n_shards), dim3(256), 0, st, m, (uint32_t *)frame_dev, width, row_block, n_ranks);
  else
    hipLaunchKernelGGL(pt_sparse_unpack_many_kernel<uint64_t>, dim3(gx, n_shards), dim3(256), 0, st, m, (uint64_t *)frame_dev, width, row_block, n_ranks);
  HIP_TRY(hipGetLastError());
  if (!stream) HIP_TRY(hipStreamSynchronize(st));
  return PT_OK;
}

extern "C" int pt_image_average_luminosity(int device, const void *img, int fmt, int width, int height,
                                           double delta, double *out, void *stream) {
  int rc = post_check(device, img, fmt, width, height);
  if (rc) return rc;
  if (!out) return fail(PT_ERR_INVALID, "null output");
  hipStream_t st = (hipStream_t)stream;
  const long long npix = (long long)width * height;
  StagedImage si;
  if ((rc = si.in(img, (size_t)npix * 3 * (fmt == PT_OUT_F32 ? 4 : 8), true, st))) return rc;
  const int nblocks = (int)((npix + PT_POST_CHUNK - 1) / PT_POST_CHUNK);
  double *partials = nullptr;
  HIP_TRY(hipMalloc((void **)&partials, (size_t)(nblocks + 1) * sizeof(double)));
  hipLaunchKernelGGL(pt_post_loglum_kernel, dim3(nblocks), dim3(256), 0, st, si.dev, fmt == PT_OUT_F32 ? 1 : 0, npix,
                     delta, partials);
  hipLaunchKernelGGL(pt_post_sum_kernel, dim3(1), dim3(256), 0, st, partials, nblocks, partials + nblocks);
  double sum = 0.0;
  hipError_t e = hipMemcpyAsync(&sum, partials + nblocks, sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(partials);
  if (e != hipSuccess) return fail(PT_ERR_HIP, "average_luminosity failed: %s", hipGetErrorString(e));
  *out = std::pow(10.0, sum / (double)npix);  // hdrimages.py:128
  return PT_OK;
}

extern "C" int pt_image_tonemap(int device, void *img, int fmt, int width, int height, double scale, int clamp,
                                double gamma, unsigned char *rgb8, int write_back, void *stream) {
  int rc = post_check(device, img, fmt, width, height);
  if (rc) return rc;
  if (rgb8 && !(gamma > 0.0)) return fail(PT_ERR_INVALID, "gamma must be positive");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)width * height * 3;
  StagedImage si, so;
  if ((rc = si.in(img, (size_t)n * (fmt == PT_OUT_F32 ? 4 : 8), true, st))) return rc;
  if (rgb8 && (rc = so.in(rgb8, (size_t)n, false, st))) return rc;
  hipLaunchKernelGGL(pt_post_tonemap_kernel, dim3(post_grid(n)), dim3(256), 0, st, si.dev, fmt == PT_OUT_F32 ? 1 : 0, n,
                     scale, clamp ? 1 : 0, rgb8 ? 1.0 / gamma : 1.0, rgb8 ? (unsigned char *)so.dev : nullptr,
                     write_back ? 1 : 0);
  HIP_TRY(hipGetLastError());
  if (write_back && (rc = si.out(st))) return rc;
  if (rgb8 && (rc = so.out(st))) return rc;
  if (!stream || si.owned || so.owned) HIP_TRY(hipStreamSynchronize(st));
  return PT_OK;
}

static void plan_info(const PtPlan &pl, const PtSceneFacts &f, const pt_params *p, pt_plan_info *out) {
  memset(out, 0, sizeof *out);
  out->kernel = pl.kernel;
  out->rows = pl.rows;
  out->npix = pl.npix;
  pt_plan_kernel_name(pl, p->renderer, 0, out->pre_kernel, sizeof out->pre_kernel);
  pt_plan_kernel_name(pl, p->renderer, 1, out->first_kernel, sizeof out->first_kernel);
  pt_plan_kernel_name(pl, p->renderer, 2, out->main_kernel, sizeof out->main_kernel);
  pt_plan_kernel_name(pl, p->renderer, 3, out->alt_kernel, sizeof out->alt_kernel);
  out->grid = pl.grid;
  out->grid_first = pl.grid_first;
  out->grid_alt = pl.grid_q;
  out->grid4_x = (int)pl.grid4_x;
  out->grid4_y = (int)pl.grid4_y;
  out->npx = 4;  // (pt_tile4_kernel: four pixels per lane; the two-pixel variant is gone)
  out->lds_first = pl.path_tiled ? (long long)pl.lds_tile : 0;
  out->lds_main = (long long)pl.lds_main;
  out->lds_alt = (long long)pl.lds_q;
  const bool path = p->renderer == PT_RENDERER_PATHTRACER && !pl.zero_frame && pl.npix > 0;
  out->frame_stack_home = !path ? 0 : (pl.lds_frames ? 1 : 2);
  out->alt_frame_stack_home = !pl.q_alt ? 0 : (pl.q_home == 1 ? 1 : (pl.q_home == 2 ? 3 : 2));
  out->frame_doubles = path ? pl.frame_doubles : 0;
  out->workspace_bytes = (long long)pl.ws_bytes;
  out->q_min_flagged = pl.q_min;
  out->wg_per_cu = pl.wg_per_cu;
  out->block_h = pl.block_h;
  out->hier = pl.hier;
  out->ortho = pl.ortho;
  out->hoist = pl.hoist;
  out->tile4_lds = pl.t4lds;
  out->n_spheres = f.n_spheres;
  out->n_diag = f.n_diag;
  out->has_grid = f.has_grid;
  out->ball_levels = pl.bs_levels;
  out->units_need = pl.units_need;
  out->alt_budget = pl.q_alt ? pl.q_budget : 0;
  out->nregions = pl.nregions;
  out->min_rounds = pl.min_rounds;
  out->spec_draws = pl.spec_draws;
}

extern "C" int pt_debug_plan(const pt_scene_desc *desc, const pt_camera *cam, const pt_params *p, int n_cu, int dome_shortcut,
                             pt_plan_info *out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  int rc = check_desc(desc);
  if (rc) return rc;
  PtSceneHost h;
  pt_build_scene(desc, pt_tuning(), h);
  rc = check_params(cam, p);
  if (rc) return rc;
  const PtSceneFacts f = pt_scene_facts(h.sc, n_cu > 0 ? n_cu : 256, dome_shortcut != 0);
  PtPlan pl;
  pt_make_plan(f, cam, p, pt_tuning(), pl);
  plan_info(pl, f, p, out);
  return PT_OK;
}

extern "C" int pt_debug_plan_hits(const pt_scene_desc *desc, const pt_camera *cam, const pt_params *p, int channels, int n_cu,
                                  pt_plan_info *out) {
  if (!out || !p) return fail(PT_ERR_INVALID, "null argument");
  if (!hits_channels_ok(channels)) return fail(PT_ERR_INVALID, "unknown hit channel bits %#x", channels);
  int rc = check_desc(desc);
  if (rc) return rc;
  PtSceneHost h;
  pt_build_scene(desc, pt_tuning(), h);
  const pt_params q = hits_params(p);
  rc = check_params(cam, &q);
  if (rc) return rc;
  const PtSceneFacts f = pt_scene_facts(h.sc, n_cu > 0 ? n_cu : 256, true);
  PtPlan pl;
  bool cull = false;
  pt_make_hits_plan(f, cam, &q, pt_tuning(), pl, cull);
  plan_info(pl, f, &q, out);
  pt_hits_kernel_name(pl, cull, 0, out->pre_kernel, sizeof out->pre_kernel);
  out->first_kernel[0] = out->alt_kernel[0] = 0;
  pt_hits_kernel_name(pl, cull, 2, out->main_kernel, sizeof out->main_kernel);
  out->hier = cull && pl.hier;
  out->lds_main = cull ? (long long)pl.lds_tile : 0;
  return PT_OK;
}

extern "C" int pt_debug_plan_scene(pt_scene *s, const pt_camera *cam, const pt_params *p, pt_plan_info *out) {
  if (!out || !s) return fail(PT_ERR_INVALID, "null argument");
  int rc = check_params(cam, p);
  if (rc) return rc;
  const PtSceneFacts f = scene_facts(s);
  PtPlan pl;
  pt_make_plan(f, cam, p, pt_tuning(), pl);
  plan_info(pl, f, p, out);
  return PT_OK;
}

extern "C" int pt_debug_set_tuning(const char *name, long long value) {
  if (name && (strcmp(name, "grid_density") == 0 || strcmp(name, "PTRACE_GRID_DENSITY") == 0)) {  // (cells per sphere: whole numbers here)
    if (value <= 0) return fail(PT_ERR_INVALID, "grid_density must be positive");
    pt_tuning().grid_density = (double)value;
    return PT_OK;
  }
  if (!name || !pt_tuning_set(pt_tuning(), name, value)) return fail(PT_ERR_INVALID, "unknown tuning switch %s", name ? name : "(null)");
  return PT_OK;
}

extern "C" int pt_debug_get_tuning(const char *name, long long *value) {
  if (!name || !value) return fail(PT_ERR_INVALID, "null argument");
  PtTuning &t = pt_tuning();
#define X(field, env, dflt)                                    \
  if (strcmp(name, #field) == 0 || strcmp(name, env) == 0) {   \
    *value = t.field;                                          \
    return PT_OK;                                              \
  }
  PT_TUNING_TABLE(X)
#undef X
  if (strcmp(name, "grid_density") == 0 || strcmp(name, "PTRACE_GRID_DENSITY") == 0) {
    *value = (long long)t.grid_density;
    return PT_OK;
  }
  return fail(PT_ERR_INVALID, "unknown tuning switch %s", name);
}

// debug: the 16 words of the path-tracer queue block (word 0 = queue head, 1..8 = section cycle sums of
// a -DPT_DEBUG_TIME build)
extern "C" int pt_debug_read_queue(pt_scene *s, unsigned long long *out16) {
  if (!s || !out16) return fail(PT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out16, s->queue_last ? s->queue_last : s->queue, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return PT_OK;
}

extern "C" int pt_debug_handed_over(pt_scene *s, unsigned long long *pixels, unsigned long long *budget) {
  if (!s || !pixels || !budget) return fail(PT_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long w[3] = {0, 0, 0};  // PT_Q_CHOICE, PT_Q_HEAVY, PT_Q_BUDGET
  static_assert(PT_Q_HEAVY == PT_Q_CHOICE + 1 && PT_Q_BUDGET == PT_Q_CHOICE + 2, "read as one block");
  HIP_TRY(hipMemcpy(w, (s->queue_last ? s->queue_last : s->queue) + PT_Q_CHOICE, sizeof w, hipMemcpyDeviceToHost));
  // (PT_Q_HEAVY keeps counting the lanes that ASKED once the record table is full, pt_path.h: handed over are at most its capacity)
  *pixels = w[0] ? std::min<unsigned long long>(w[1], (unsigned long long)s->last_handover_cap) : 0ULL;
  *budget = w[2];
  return PT_OK;
}

#ifdef PT_DEBUG_TIME
extern "C" int pt_debug_read_dbg(unsigned long long *out8, int reset) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out8, HIP_SYMBOL(pt_dbg), 8 * sizeof(unsigned long long)));
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(pt_dbg), z, sizeof z));
  }
  return PT_OK;
}
extern "C" int pt_debug_read_lat_hist(unsigned long long *out160, int clear) {
#ifdef PT_DEBUG_TIME
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out160, HIP_SYMBOL(pt_lat_hist), 160 * sizeof(unsigned long long)));
  if (clear) {
    static const unsigned long long zeros[160] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(pt_lat_hist), zeros, sizeof(zeros)));
  }
  return PT_OK;
#else
  (void)out160;
  (void)clear;
  return PT_ERR_INVALID;
#endif
}
extern "C" int pt_debug_read_lat_events(unsigned long long *out, int clear) {  // out: PT_LAT_EVENTS * 3 + 1 words
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(pt_lat_events), (PT_LAT_EVENTS * 3 + 1) * sizeof(unsigned long long)));
  if (clear) {
    const unsigned long long zero = 0;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(pt_lat_events), &zero, sizeof(zero), (PT_LAT_EVENTS * 3) * sizeof(unsigned long long)));
  }
  return PT_OK;
}
extern "C" int pt_debug_read_unitlog(unsigned long long *out, int n_units) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(pt_unitlog), (size_t)std::min(n_units, PT_UNITLOG_LEN) * 8 * sizeof(unsigned long long)));
  return PT_OK;
}
extern "C" int pt_debug_read_trace(unsigned long long *out, int n) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(pt_trace), (size_t)std::min(n, PT_TRACE_LEN + 64 * 80) * sizeof(unsigned long long)));
  return PT_OK;
}
#endif

// ---- diagnostics (not part of the reference seam): probes of single device functions, used by the tests ------------------
// A probe's round trip through ONE device allocation, freed on every way out (Staged): [the block, where the kernel reads its
// cold half (`a` non-null: it gets `cold` and its device copy) | the input | the output].  launch(in_dev, out_dev) enqueues the
// kernel on the null stream; then out_bytes come back to `out` and the out2_bytes behind them to `out2`.
template <typename Launch>
static int run_probe(PtKArgs *a, const void *in, size_t in_bytes, void *out, size_t out_bytes, Launch launch, void *out2 = nullptr,
                     size_t out2_bytes = 0) {
  const size_t head = a ? sizeof(PtKArgs) : 0;
  Staged m;
  HIP_TRY(hipMalloc((void **)&m.dev, head + up8(in_bytes) + std::max<size_t>(out_bytes + out2_bytes, 8)));
  char *in_dev = m.dev + head, *out_dev = in_dev + up8(in_bytes);
  if (a) {
    a->cold = (const PtKArgs *)m.dev;
    HIP_TRY(hipMemcpy(m.dev, a, sizeof *a, hipMemcpyHostToDevice));
  }
  if (in_bytes) HIP_TRY(hipMemcpy(in_dev, in, in_bytes, hipMemcpyHostToDevice));
  launch(in_dev, out_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, out_dev, out_bytes, hipMemcpyDeviceToHost));
  if (out2_bytes) HIP_TRY(hipMemcpy(out2, out_dev + out_bytes, out2_bytes, hipMemcpyDeviceToHost));
  return PT_OK;
}

// The culling predicate on its own: keep[i] (by World.shapes index) = would the cull of the primary rays through the image
// rectangle [x0, x1] x [row0, row1 + 1] keep shape i?  pixel_x >= 0: the same for the cone of the single pixel
// (pixel_x, pixel_row) inside that tile (pixel_cone, perspective only).  Planes answer 1.
extern "C" int pt_debug_cull_probe(pt_scene *s, const pt_camera *cam, int width, int height, int x0, int x1, int row0,
                                   int row1, int pixel_x, int pixel_row, int *keep) {
  if (!s || !cam || !keep || width <= 0 || height <= 0) return fail(PT_ERR_INVALID, "bad probe arguments");
  HIP_TRY(hipSetDevice(s->device));
  PtKArgs a;
  memset(&a, 0, sizeof a);
  fill_cone_model(a, cam, width, height);
  fill_shape_tables(s, a);
  return run_probe(&a, nullptr, 0, keep, sizeof(int) * a.n_shapes, [&](char *, char *keep_dev) {
    hipLaunchKernelGGL(pt_cull_probe_kernel, dim3(1), dim3(64), 0, 0, a, x0, x1, row0, row1, pixel_x, pixel_row, (int *)keep_dev);
  });
}

// device primitives (sqrt, division, libm, the generator): out[i] = op(x[i], y[i])
extern "C" int pt_debug_probe(int op, const double *x, const double *y, double *out, int n) {
  if (n <= 0 || !x || !out) return fail(PT_ERR_INVALID, "bad probe arguments");
  const size_t bytes = (size_t)n * sizeof(double);
  Staged m;
  HIP_TRY(hipMalloc((void **)&m.dev, 3 * bytes));
  double *dx = (double *)m.dev, *dy = dx + n, *dout = dy + n;
  HIP_TRY(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dy, y ? y : x, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(pt_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, dx, dy, dout, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
  return PT_OK;
}

// the hit record, camera rays and BRDF scattering of the device path on their own
extern "C" int pt_debug_hit_probe(pt_scene *s, int shape_index, const double *rays, int n, double *out) {
  if (!s || !rays || !out || n <= 0 || shape_index >= s->sh->sc.n_shapes) return fail(PT_ERR_INVALID, "bad probe arguments");
  HIP_TRY(hipSetDevice(s->device));
  PtKArgs a;
  memset(&a, 0, sizeof a);
  fill_shape_tables(s, a);  // (and nothing else of the scene: one shape is queried as a one-record view of these)
  return run_probe(nullptr, rays, (size_t)n * 8 * sizeof(double), out, (size_t)n * 12 * sizeof(double), [&](char *rd, char *od) {
    hipLaunchKernelGGL(pt_hit_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, a, shape_index, (const double *)rd, n, (double *)od);
  });
}

extern "C" int pt_debug_lanes_probe(pt_scene *s, int anyhit, const double *rays, int n, double *out) {
  if (!s || !rays || !out || n <= 0) return fail(PT_ERR_INVALID, "bad probe arguments");
  HIP_TRY(hipSetDevice(s->device));
  PtKArgs a;
  memset(&a, 0, sizeof a);
  fill_scene_args(s, a);
  return run_probe(&a, rays, (size_t)n * 8 * sizeof(double), out, (size_t)n * 4 * sizeof(double), [&](char *rd, char *od) {
    if (anyhit)
      hipLaunchKernelGGL(pt_lanes_probe_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, 0, a, (const double *)rd, n, (double *)od);
    else
      hipLaunchKernelGGL(pt_lanes_probe_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, 0, a, (const double *)rd, n, (double *)od);
  });
}

extern "C" int pt_debug_camera_probe(const pt_camera *cam, int width, int height, const double *pix, int n, double *out) {
  if (!cam || !pix || !out || n <= 0 || width <= 0 || height <= 0) return fail(PT_ERR_INVALID, "bad probe arguments");
  PtKArgs a;
  memset(&a, 0, sizeof a);
  pt_fill_camera(a, cam, width, height);
  return run_probe(&a, pix, (size_t)n * 4 * sizeof(double), out, (size_t)n * 7 * sizeof(double), [&](char *pd, char *od) {
    hipLaunchKernelGGL(pt_camera_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, a, (const double *)pd, n, (double *)od);
  });
}

extern "C" int pt_debug_scatter_probe(const double *in, int n, double *out, unsigned long long *state_after) {
  if (!in || !out || !state_after || n <= 0) return fail(PT_ERR_INVALID, "bad probe arguments");
  const size_t out_bytes = (size_t)n * 7 * sizeof(double);
  return run_probe(
      nullptr, in, (size_t)n * 12 * sizeof(double), out, out_bytes,
      [&](char *id, char *od) {
        hipLaunchKernelGGL(pt_scatter_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, (const double *)id, n, (double *)od,
                           (unsigned long long *)(od + out_bytes));
      },
      state_after, (size_t)n * sizeof(unsigned long long));
}
