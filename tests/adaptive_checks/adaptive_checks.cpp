// adaptive_checks.cpp -- csrc/pt_adaptive_host.h on its own, on the CPU: the sizes, the plane offsets and the checks of values of
// include/ptrace_adaptive.h, in a program with its own main that makes no HIP call.  tests/test_adaptive_host.py compiles it with
// the host AddressSanitizer and UndefinedBehaviorSanitizer and runs it; every expectation is written out from the header.
#include "../../include/ptrace_adaptive.h"
#define PT_QUERY_PARTS_ONLY
#include "../../pytracer_amd/csrc/pt_kernels.h"
#include "../../pytracer_amd/csrc/pt_host_common.h"
#include "../../pytracer_amd/csrc/pt_adaptive_host.h"

#include <cmath>
#include <cstdio>
#include <limits>

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      failures++;                                                 \
    }                                                             \
  } while (0)

int main() {
  const long long top = 2147483647LL;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // sizes: 24 n, + 8 n, + up8(4 n); the largest n does not overflow
  const long long sizes[] = {0, 1, 2, 3, 63, 130, 257, top};
  for (long long n : sizes) {
    for (int ch = 0; ch < 4; ch++) {
      const size_t want = (size_t)n * 24 + ((ch & 1) ? (size_t)n * 8 : 0) + ((ch & 2) ? (((size_t)n * 4 + 7) / 8) * 8 : 0);
      EXPECT(ad_bytes(n, ch) == want);
      EXPECT(ad_plane_offset(n, ch, 0, 0) == 0 && ad_plane_offset(n, ch, 0, 2) == n * 16 && ad_plane_offset(n, ch, 0, 3) == PT_ERR_INVALID);
      EXPECT(ad_plane_offset(n, ch, PT_ADAPTIVE_COUNT, 0) == ((ch & 1) ? n * 24 : PT_ERR_INVALID));
      EXPECT(ad_plane_offset(n, ch, PT_ADAPTIVE_TAKEN, 0) == ((ch & 2) ? n * 24 + ((ch & 1) ? n * 8 : 0) : PT_ERR_INVALID));
      EXPECT(ad_plane_offset(n, ch, PT_ADAPTIVE_TAKEN, 1) == PT_ERR_INVALID && ad_plane_offset(n, ch, 4, 0) == PT_ERR_INVALID);
      EXPECT(ad_plane_offset(n, ch, 0, -1) == PT_ERR_INVALID);
      if (ch & 2) EXPECT((size_t)ad_plane_offset(n, ch, PT_ADAPTIVE_TAKEN, 0) + (size_t)n * 4 <= ad_bytes(n, ch));  // the plane lies inside
    }
    EXPECT(ad_bytes(n, 4) == 0 && ad_bytes(n, -1) == 0);
    EXPECT(ad_offsets_bytes(n) == ((size_t)n + 1) * 8);
    EXPECT(ad_offsets_workspace_bytes(n) == (size_t)(n == 0 ? 1 : (n + 255) / 256) * 8);
    EXPECT(ad_planes_bytes(n) == (size_t)n * 32);
  }
  EXPECT(ad_bytes(-1, 0) == 0 && ad_bytes(top + 1, 0) == 0 && ad_offsets_bytes(-1) == 0 && ad_offsets_bytes(top + 1) == 0);
  EXPECT(ad_offsets_workspace_bytes(-1) == 0 && ad_offsets_workspace_bytes(top + 1) == 0);
  EXPECT(ad_scan_blocks(1) == 1 && ad_scan_blocks(256) == 1 && ad_scan_blocks(257) == 2 && ad_scan_blocks(top) == 8388608);
  // the node stacks: lanes x max(levels, 1) x fields x 8
  EXPECT(ad_stacks_bytes(256, 1, 3, 0, 6, 20) == 256u * 3 * 6 * 8 && ad_stacks_bytes(1024, 2, 2, 0, 6, 20) == 1024u * 2 * 20 * 8);
  EXPECT(ad_stacks_bytes(256, 1, 3, 7, 6, 20) == 256u * 1 * 6 * 8 && ad_stacks_bytes(256, 1, 2147483647, 2147483647 - 64, 6, 20) == 256u * 64 * 6 * 8);
  // the counts' struct
  pt_adaptive_count_params c = {1, 32, 0.05, 0.05, 1.0};
  EXPECT(ad_check_counts(0, &c) == PT_OK && ad_check_counts(top, &c) == PT_OK);
  EXPECT(ad_check_counts(-1, &c) == PT_ERR_INVALID && ad_check_counts(top + 1, &c) == PT_ERR_INVALID && ad_check_counts(5, nullptr) == PT_ERR_INVALID);
  const int bad_ints[][2] = {{-1, 4}, {5, 4}, {0, 1048577}, {2147483647, 2147483647}, {-2147483647 - 1, 0}};
  for (auto &b : bad_ints) {
    pt_adaptive_count_params x = c;
    x.min_samples = b[0], x.max_samples = b[1];
    EXPECT(ad_check_counts(5, &x) == PT_ERR_INVALID);
  }
  const int good_ints[][2] = {{0, 0}, {0, 1048576}, {1048576, 1048576}};
  for (auto &b : good_ints) {
    pt_adaptive_count_params x = c;
    x.min_samples = b[0], x.max_samples = b[1];
    EXPECT(ad_check_counts(5, &x) == PT_OK);
  }
  const double bad_doubles[] = {0.0, -0.0, -1.0, -inf, nan};
  for (double b : bad_doubles) {
    pt_adaptive_count_params x = c;
    x.tolerance = b;
    EXPECT(ad_check_counts(5, &x) == PT_ERR_INVALID);
    x = c, x.luminance_floor = b;
    EXPECT(ad_check_counts(5, &x) == PT_ERR_INVALID);
    x = c, x.gain = b;
    EXPECT(ad_check_counts(5, &x) == PT_ERR_INVALID);
  }
  {
    pt_adaptive_count_params x = c;
    x.tolerance = inf;
    EXPECT(ad_check_counts(5, &x) == PT_OK);
    x = c, x.luminance_floor = inf;
    EXPECT(ad_check_counts(5, &x) == PT_ERR_INVALID);
    x = c, x.gain = inf;
    EXPECT(ad_check_counts(5, &x) == PT_ERR_INVALID);
    x = c, x.tolerance = 5e-324, x.luminance_floor = 5e-324, x.gain = 1.7976931348623157e308;
    EXPECT(ad_check_counts(5, &x) == PT_OK);
  }
  // the walk's values
  EXPECT(ad_check_walk(5, 15, 1, 3, 0) == PT_OK && ad_check_walk(0, 0, 1, 0, 0) == PT_OK && ad_check_walk(top, top, 2147483647, 2147483647, 2147483647) == PT_OK);
  EXPECT(ad_check_walk(-1, 15, 1, 3, 0) == PT_ERR_INVALID && ad_check_walk(top + 1, 15, 1, 3, 0) == PT_ERR_INVALID);
  EXPECT(ad_check_walk(5, -1, 1, 3, 0) == PT_ERR_INVALID && ad_check_walk(5, top + 1, 1, 3, 0) == PT_ERR_INVALID);
  EXPECT(ad_check_walk(5, 15, 0, 3, 0) == PT_ERR_INVALID && ad_check_walk(5, 15, 1, -1, 0) == PT_ERR_INVALID && ad_check_walk(5, 15, 1, 3, -1) == PT_ERR_INVALID);
  EXPECT(ad_check_walk(5, 15, 1, 65, 0) == PT_ERR_UNSUPPORTED && ad_check_walk(5, 15, 1, 64, 0) == PT_OK);
  EXPECT(ad_check_walk(5, 15, 1, 2147483647, 2147483647 - 65) == PT_ERR_UNSUPPORTED && ad_check_walk(5, 15, 1, 3, 2147483647) == PT_OK);
  // the message of a refusal fits the buffer it is copied into, however small
  char small[8];
  EXPECT(ad_check_walk(5, 15, 1, 65, 0) == PT_ERR_UNSUPPORTED && copy_last_error(small, sizeof small) > 7 && small[7] == 0);
  printf("%s\n", failures ? "adaptive checks: FAILED" : "adaptive checks: ok");
  return failures ? 1 : 0;
}
