// pt_host_common.h — the host layer every library of this tree wraps around its kernels, written once: the thread-local error
// text, the device check, the scene-argument-block check of the add-on libraries, and the small helpers of their launches and
// host forms.  Host code only: nothing here is __global__ or __device__, so including it leaves a library's device code (and
// build.code_hash) what it was.  Every function is static: each shared object gets its own copy and its own g_err, there is
// still no link dependency between the libraries.  Include it behind pt_kernels.h (PT_BLOCK).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ptrace.h"
#include "pt_layout.h"

// ---- errors: a negative return code plus a thread-local message ----------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                                          \
  do {                                                                                                         \
    hipError_t _e = (expr);                                                                                    \
    if (_e != hipSuccess) return fail(PT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// the body of every *_last_error: the message, cut to the caller's buffer; returns its full length
static int copy_last_error(char *buf, size_t n) {
  const size_t len = strlen(g_err);
  if (buf && n) {
    const size_t c = std::min(len, n - 1);
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return (int)len;
}

static int device_ok(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(PT_ERR_INVALID, "device %d out of range (%d visible)", device, ndev);
  return PT_OK;
}

// ---- the scene argument block an add-on is handed (pt_scene_kernel_args of libptrace.so) ------------------------------------------
// Which negative counts a library refuses on top of the checks all of them make.  PT_BLOCK_LIGHTS is the surface library's: it
// reads the lights, and names both counts in its message.
enum { PT_BLOCK_SHAPES = 1, PT_BLOCK_LIGHTS = 2 };

static int check_scene_block(int device, const void *scene_args, size_t scene_args_bytes, int flags) {
  if (device < 0) return fail(PT_ERR_INVALID, "device %d", device);
  if (!scene_args) return fail(PT_ERR_INVALID, "null scene argument block");
  if (scene_args_bytes != sizeof(PtKArgs))
    return fail(PT_ERR_INVALID, "scene argument block of %zu bytes, this library's has %zu: all libraries must come from one build",
                scene_args_bytes, sizeof(PtKArgs));
  const PtKArgs *a = (const PtKArgs *)scene_args;
  if (!a->cold) return fail(PT_ERR_INVALID, "scene argument block without its device copy (not from pt_scene_kernel_args?)");
  if (flags & PT_BLOCK_LIGHTS) {
    if (a->n_shapes < 0 || a->n_lights < 0) return fail(PT_ERR_INVALID, "scene argument block with %d shapes and %d lights", a->n_shapes, a->n_lights);
  } else if ((flags & PT_BLOCK_SHAPES) && a->n_shapes < 0) {
    return fail(PT_ERR_INVALID, "scene argument block with %d shapes", a->n_shapes);
  }
  return PT_OK;
}

// the block as the kernels take it (the caller's bytes need not be aligned)
static PtKArgs scene_block(const void *scene_args) {
  PtKArgs a;
  memcpy(&a, scene_args, sizeof a);
  return a;
}

// ---- launches and host forms --------------------------------------------------------------------------------------------------
static size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }

static dim3 grid_of(long long n) { return dim3((unsigned)((n + PT_BLOCK - 1) / PT_BLOCK)); }

// the one device allocation of a host form: inputs, tables, workspace and output side by side; freed on every way out
struct Staged {
  char *dev = nullptr;
  ~Staged() { (void)hipFree(dev); }
  int alloc(size_t bytes) {
    const hipError_t e = hipMalloc((void **)&dev, bytes);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? PT_ERR_NOMEM : PT_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return PT_OK;
  }
};

// Lanes one launch of `kernel_fn` keeps resident on `device`: compute units x the workgroups of the kernel one of them holds x
// 256, no more than `total` needs, no more than the environment variable `env_name` allows.  Always a positive multiple of 256.
// (No wave ever waits for another: a grid that is not fully resident is merely dispatched in turns.)
static int resident_lanes(int device, long long total, const void *kernel_fn, const char *env_name, unsigned long long &lanes) {
  int cus = 0, per_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_fn, PT_BLOCK, 0));
  unsigned long long cap = (unsigned long long)std::max(cus, 1) * (unsigned long long)std::max(per_cu, 1) * PT_BLOCK;
  if (const char *e = getenv(env_name)) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end != e && *end == 0) cap = std::min(cap, std::max<unsigned long long>(v / PT_BLOCK, 1) * PT_BLOCK);
  }
  const unsigned long long want = ((unsigned long long)std::max<long long>(total, 1) + PT_BLOCK - 1) / PT_BLOCK * PT_BLOCK;
  lanes = std::min(cap, want);
  return PT_OK;
}
