// The index rule of csrc/joint_psf_place.h on the host: the real header over the stand-in runtime of hip/hip_runtime.h
// (next to this file; the placement kernel itself is device code and is left out there).  For each (P, N): every grid
// pixel maps to a tap inside the stamp or to -1, no tap is used twice, the zero lag goes to the zero lag, and
// min(P, N)^2 taps are kept.  The stamps and grids are real arrays, filled through the rule, so an index out of range is
// the sanitizers' to report.  Built with -fsanitize=address,undefined by tests/test_joint_psf_size_cpu.py; exits 0 when
// every check holds.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "joint_psf_place.h"

using namespace lc;

static int failures = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::printf("FAILED line %d (P = %d, N = %d): %s\n", __LINE__, P, N, #cond);  \
      ++failures;                                                                   \
    }                                                                               \
  } while (0)

static void check_pair(int P, int N) {
  std::vector<float> stamp((size_t)P * P), grid((size_t)N * N, -1.f);
  for (size_t i = 0; i < stamp.size(); ++i) stamp[i] = (float)(i + 1);
  std::vector<int> used((size_t)P * P, 0);
  int kept = 0;
  bool in_range = true;
  for (int d = 0; d < N * N; ++d) {
    const int s = psf_place_source(P, N, d);
    if (s < -1 || s >= P * P) {
      in_range = false;
      continue;
    }
    grid[d] = s >= 0 ? stamp[s] : 0.f;  // what the kernel's thread d does
    if (s >= 0) {
      ++used[s];
      ++kept;
    }
  }
  CHECK(in_range);
  CHECK(*std::max_element(used.begin(), used.end()) <= 1);
  const int cP = (P - 1) / 2, cN = (N - 1) / 2;
  CHECK(psf_place_source(P, N, cN * N + cN) == cP * P + cP);
  CHECK(grid[(size_t)cN * N + cN] == stamp[(size_t)cP * P + cP]);
  const int m = std::min(P, N);
  CHECK(kept == m * m);
  // tap (a, b) lands on (a + cN - cP, b + cN - cP) or nowhere
  bool taps = true;
  for (int a = 0; a < P; ++a)
    for (int b = 0; b < P; ++b) {
      const int r = a + cN - cP, c = b + cN - cP;
      const bool inside = r >= 0 && r < N && c >= 0 && c < N;
      if (inside != (used[(size_t)a * P + b] == 1)) taps = false;
      if (inside && grid[(size_t)r * N + c] != stamp[(size_t)a * P + b]) taps = false;
    }
  CHECK(taps);
}

int main() {
  const int at32[] = {1, 8, 31, 32, 33, 48, 200}, at16[] = {9, 24};
  for (int P : at32) check_pair(P, 32);
  for (int P : at16) check_pair(P, 16);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
