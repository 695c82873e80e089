// pt_adaptive_host.h -- the host-side arithmetic of include/ptrace_adaptive.h: sizes, plane offsets and every check of a value
// (not of a device).  Host code only and no HIP call, so that a program with its own main can run it under the host sanitizers
// (tests/adaptive_checks/adaptive_checks.cpp).  Include it behind pt_host_common.h (fail, up8) and the interface's header.
#pragma once

#define PT_AD_MAX_N 2147483647LL
#define PT_AD_SCAN_BLOCK 256  // counts per workgroup of the scan (pt_adaptive.h: PT_AD_SCAN)
#define PT_AD_PLANES 4        // sample planes of the workspace (pt_adaptive.h: PT_AD_SAMPLE_PLANES)

static bool ad_shape_ok(long long n, int channels) { return n >= 0 && n <= PT_AD_MAX_N && channels >= 0 && !(channels & ~PT_ADAPTIVE_ALL); }

static size_t ad_bytes(long long n, int channels) {
  if (!ad_shape_ok(n, channels)) return 0;
  return (size_t)n * 24 + ((channels & PT_ADAPTIVE_COUNT) ? (size_t)n * 8 : 0) + ((channels & PT_ADAPTIVE_TAKEN) ? up8((size_t)n * 4) : 0);
}

static long long ad_plane_offset(long long n, int channels, int channel, int component) {
  if (!ad_shape_ok(n, channels) || component < 0) return PT_ERR_INVALID;
  if (channel == 0) return component < 3 ? n * 8 * component : PT_ERR_INVALID;
  if (component > 0) return PT_ERR_INVALID;
  if (channel == PT_ADAPTIVE_COUNT && (channels & PT_ADAPTIVE_COUNT)) return n * 24;
  if (channel == PT_ADAPTIVE_TAKEN && (channels & PT_ADAPTIVE_TAKEN)) return n * 24 + ((channels & PT_ADAPTIVE_COUNT) ? n * 8 : 0);
  return PT_ERR_INVALID;
}

static size_t ad_offsets_bytes(long long n) { return (n >= 0 && n <= PT_AD_MAX_N) ? ((size_t)n + 1) * 8 : 0; }

static long long ad_scan_blocks(long long n) { return (n + PT_AD_SCAN_BLOCK - 1) / PT_AD_SCAN_BLOCK; }

static size_t ad_offsets_workspace_bytes(long long n) {
  if (n < 0 || n > PT_AD_MAX_N) return 0;
  return (size_t)std::max<long long>(ad_scan_blocks(n), 1) * 8;
}

static int ad_check_counts(long long m, const pt_adaptive_count_params *p) {
  if (m < 0 || m > PT_AD_MAX_N) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", m);
  if (!p) return fail(PT_ERR_INVALID, "null pt_adaptive_count_params");
  if (p->min_samples < 0 || p->max_samples < p->min_samples || p->max_samples > PT_ADAPTIVE_MAX_SAMPLES)
    return fail(PT_ERR_INVALID, "min_samples = %d, max_samples = %d: 0 <= min <= max <= 2^20", p->min_samples, p->max_samples);
  if (!(p->tolerance > 0.0)) return fail(PT_ERR_INVALID, "tolerance = %g: positive (or +inf)", p->tolerance);
  if (!(p->luminance_floor > 0.0 && p->luminance_floor < __builtin_inf()))
    return fail(PT_ERR_INVALID, "luminance_floor = %g: positive and finite", p->luminance_floor);
  if (!(p->gain > 0.0 && p->gain < __builtin_inf())) return fail(PT_ERR_INVALID, "gain = %g: positive and finite", p->gain);
  return PT_OK;
}

static int ad_check_walk(long long n, long long capacity, int num_of_rays, int max_depth, int depth0) {
  if (n < 0 || n > PT_AD_MAX_N) return fail(PT_ERR_INVALID, "record count %lld outside [0, 2^31 - 1]", n);
  if (capacity < 0 || capacity > PT_AD_MAX_N) return fail(PT_ERR_INVALID, "capacity %lld outside [0, 2^31 - 1] samples", capacity);
  if (num_of_rays < 1) return fail(PT_ERR_INVALID, "num_of_rays must be at least 1, not %d", num_of_rays);
  if (max_depth < 0) return fail(PT_ERR_INVALID, "max_depth must not be negative, not %d", max_depth);
  if (depth0 < 0) return fail(PT_ERR_INVALID, "depth (the hemisphere rays' Ray.depth) must not be negative, not %d", depth0);
  if ((long long)max_depth - depth0 > PT_ADAPTIVE_MAX_LEVELS)
    return fail(PT_ERR_UNSUPPORTED, "max_depth - depth = %lld: an adaptive query walks at most %d levels below its hemisphere rays",
                (long long)max_depth - depth0, PT_ADAPTIVE_MAX_LEVELS);
  return PT_OK;
}

// the two parts of the gather's workspace: node stacks for `lanes` resident lanes, then [4][capacity] sample planes
static size_t ad_stacks_bytes(unsigned long long lanes, int num_of_rays, int max_depth, int depth0, int fields_one, int fields_many) {
  const long long levels = std::max<long long>((long long)max_depth - depth0, 1);
  return (size_t)lanes * (size_t)levels * (size_t)(num_of_rays > 1 ? fields_many : fields_one) * sizeof(double);
}

static size_t ad_planes_bytes(long long capacity) { return (size_t)capacity * PT_AD_PLANES * sizeof(double); }

// the owner plane of the expand variant: one int32 per sample, padded to 8 bytes
static size_t ad_owner_bytes(long long capacity) { return up8((size_t)capacity * 4); }
