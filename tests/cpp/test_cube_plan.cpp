// The host arithmetic of the cube front end (csrc/ws_cube_plan.hpp, plain C++): the extent and span of strided views against a
// walk over their elements, the refusals at the edge of size_t, the runs of the stacked minima, and the offsets summed across runs.
// No library, no GPU; the driver builds it with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <vector>

#include "../../rustronomy-watershed_amd/csrc/ws_cube_plan.hpp"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static int extents() {
  const size_t dims[] = {0, 1, 2, 5}, strides[] = {0, 1, 2, 7, 40};
  for (size_t n : dims) for (size_t h : dims) for (size_t w : dims)
    for (size_t ss : strides) for (size_t rs : strides) for (size_t cs : strides) {
      size_t total = 99, span = 99, far = 0;
      CHECK(wsplan::cube_extent(n, h, w, ss, rs, cs, &total, &span));
      CHECK(total == n * h * w);
      for (size_t k = 0; k < n; ++k) for (size_t r = 0; r < h; ++r) for (size_t c = 0; c < w; ++c) far = std::max(far, k * ss + r * rs + c * cs + 1);
      CHECK(span == (total ? far : 0));
      std::vector<unsigned char> store(span + 1, 0);      // every element of the view lies inside `span` elements: the sanitizer watches
      for (size_t k = 0; k < n; ++k) for (size_t r = 0; r < h; ++r) for (size_t c = 0; c < w; ++c) store[k * ss + r * rs + c * cs] = 1;
      CHECK(store[span] == 0 && (total == 0 || store[span - 1] == 1));
    }
  const size_t big = ~(size_t)0;
  size_t total = 0, span = 0;
  CHECK(!wsplan::cube_extent(big, 2, 1, 1, 1, 1, &total, &span));                    // n * h * w
  CHECK(!wsplan::cube_extent(big / 2 + 1, 1, 2, 1, 1, 1, &total, &span));
  CHECK(!wsplan::cube_extent(3, 3, 3, big / 2, 1, 1, &total, &span));                // (n - 1) * ss
  CHECK(!wsplan::cube_extent(3, 3, 3, 1, big / 2, 1, &total, &span));
  CHECK(!wsplan::cube_extent(3, 3, 3, 1, 1, big / 2, &total, &span));
  CHECK(!wsplan::cube_extent(2, 2, 2, big / 32, big / 32, 1, &total, &span));        // the sum passes size_t / 16
  CHECK(wsplan::cube_extent(2, 2, 2, big / 64, big / 64, 1, &total, &span) && span == 2 * (big / 64) + 2 && total == 8);
  CHECK(wsplan::cube_extent(0, big, big, big, big, big, &total, &span) == false);    // h * w overflows whatever the slice count
  CHECK(wsplan::cube_extent(0, 1 << 20, 1 << 20, big, big, big, &total, &span) && total == 0 && span == 0);      // empty: strides are not looked at
  return 0;
}

static int runs() {
  const size_t px = 0x7FFFFFFFull;
  CHECK(wsplan::minima_run_slices(5, 9, 33, 2 * 9 * 33 + 5, 256) == 2);              // the pixel limit: runs of 2, 2, 1
  CHECK(wsplan::minima_run_slices(5, 9, 33, 1, 256) == 1);                           // never fewer than one slice
  CHECK(wsplan::minima_run_slices(5, 9, 33, px, 256) == 5);                          // never more than there are
  CHECK(wsplan::minima_run_slices(70001, 8, 16, px, 256) == 70001);                  // 143 MB of nibbles: one run
  CHECK(wsplan::minima_run_slices((size_t)1 << 30, 3, 3, px, 256) == wsplan::MINIMA_RUN_NIBBLE_BYTES / (3 * 256));      // narrow slices: the scratch bound
  CHECK(wsplan::minima_run_slices(100, 0x7FFFFFF0ull, 3, ~(size_t)0, 256) == 1);
  for (size_t h : {3, 8, 13, 4096}) for (size_t w : {3, 16, 1028, 4096}) for (size_t lim : {(size_t)1, (size_t)100000, px}) {
    const size_t row = ((w + 1023) / 1024) * 256, n = 1000, per = wsplan::minima_run_slices(n, h, w, lim, row);
    CHECK(per >= 1 && per <= n);
    if (per > 1) CHECK(per * h * w <= lim && per * h <= wsplan::MINIMA_STACK_ROWS_MAX && per * h * row <= wsplan::MINIMA_RUN_NIBBLE_BYTES);
    if (per < n) CHECK((per + 1) * h * w > lim || (per + 1) * h * row > wsplan::MINIMA_RUN_NIBBLE_BYTES);
  }
  // offsets across runs: 7 slices in runs of 3, counts 0, 2, 5 | 0xFFFFFFF0, 1, 0 | 32 -- the total passes 32 bits
  const size_t n = 7, per = 3;
  const uint32_t counts[n] = {0, 2, 5, 0xFFFFFFF0u, 1, 0, 32};
  std::vector<size_t> offs(n + 1, 77);
  size_t total = 0;
  for (size_t k0 = 0; k0 < n; k0 += per) {
    const size_t g = std::min(per, n - k0);
    std::vector<uint32_t> run(g + 1, 0);      // exactly g + 1 words, as the driver reads back
    for (size_t i = 0; i < g; ++i) run[i + 1] = run[i] + counts[k0 + i];
    total = wsplan::minima_add_run(run.data(), g, k0, total, offs.data());
  }
  offs[n] = total;
  size_t want = 0;
  for (size_t k = 0; k < n; ++k) { CHECK(offs[k] == want); want += counts[k]; }
  CHECK(offs[n] == want && want > 0xFFFFFFFFull);
  return 0;
}

int main() {
  if (extents() || runs()) return 1;
  std::printf("cube plan ok\n");
  return 0;
}
