// The cube front end in the C++ mirror (include/ws_watershed.hpp: pre_processor_cube(_with_max), find_local_minima_cube) against
// the mirror's single calls on each slice made contiguous: pre_processor_with_max and find_local_minima.  Needs device 0.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../include/ws_watershed.hpp"
#include "../../oracle/ws_oracle.h"

namespace ws = rustronomy_watershed;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

// value of element (k, r, c): every slice its own range, a NaN and an exact zero in each
static double value(size_t k, size_t r, size_t c) {
  if (r == 1 && c == 2) return std::numeric_limits<double>::quiet_NaN();
  if (r == 0 && c == 1) return 0.0;
  return (double)((r * 31 + c * 17 + k * 5) % 23) * (double)(k + 1) - 3.0 * (double)(k + 1);
}

template <class E, class W>
static int check_pre_processor(const W &watershed, size_t S, size_t H, size_t Wd) {
  const size_t hw = H * Wd;
  // three layouts of the same cube: slice-major, channel-last, and every other element of a larger array
  std::vector<E> major(S * hw), last(S * hw), wide(2 * S * hw + 5, (E)20000);
  for (size_t k = 0; k < S; ++k)
    for (size_t r = 0; r < H; ++r)
      for (size_t c = 0; c < Wd; ++c) {
        double v = value(k, r, c);
        if (!std::numeric_limits<E>::has_quiet_NaN && std::isnan(v)) v = 1.0;
        const E e = (E)v;
        major[k * hw + r * Wd + c] = e;
        last[(r * Wd + c) * S + k] = e;
        wide[2 * (k * hw + r * Wd + c)] = e;
      }
  std::vector<std::pair<double, double>> mm;
  const auto a = watershed.template pre_processor_cube_with_max<127, E>(major.data(), S, H, Wd, hw, Wd, 1, &mm);
  const auto b = watershed.template pre_processor_cube_with_max<127, E>(last.data(), S, H, Wd, 1, Wd * S, S);
  const auto c = watershed.template pre_processor_cube_with_max<127, E>(wide.data(), S, H, Wd, 2 * hw, 2 * Wd, 2);
  const auto d = watershed.template pre_processor_cube<E>(last.data(), S, H, Wd, 1, Wd * S, S);
  CHECK(a.size() == S * hw && b == a && c == a && d.size() == a.size() && mm.size() == S);
  for (size_t k = 0; k < S; ++k) {
    const auto one = watershed.template pre_processor_with_max<127, E>(major.data() + k * hw, hw);
    const auto full = watershed.template pre_processor<E>(major.data() + k * hw, hw);
    double mn = 0.0, mx = 0.0;
    for (size_t p = 0; p < hw; ++p) {
      const double v = (double)major[k * hw + p];
      if (std::isfinite(v)) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
      CHECK(a[k * hw + p] == one[p] && d[k * hw + p] == full[p]);
    }
    CHECK(mm[k].first == mn && mm[k].second == mx);
  }
  return 0;
}

template <class W>
static int check_minima(const W &watershed, size_t S, size_t H, size_t Wd, unsigned seed) {
  const size_t hw = H * Wd, pitch = Wd + 3, plane = (H + 1) * pitch;
  std::vector<uint8_t> cube(S * hw), strided(S * plane + 1, 255);
  for (size_t s = 0; s < S; ++s) ws_or_random_field(cube.data() + s * hw, H, Wd, seed + 7 * (unsigned)s);
  if (S > 2) std::fill(cube.begin() + hw, cube.begin() + 2 * hw, (uint8_t)9);      // slice 1: no seed
  for (size_t s = 0; s < S; ++s)
    for (size_t r = 0; r < H; ++r)
      for (size_t c = 0; c < Wd; ++c) strided[1 + s * plane + r * pitch + c] = cube[s * hw + r * Wd + c];
  std::vector<size_t> offsets, offsets2;
  const auto all = watershed.find_local_minima_cube(cube.data(), S, H, Wd, Wd, hw, offsets);
  const auto all2 = watershed.find_local_minima_cube(strided.data() + 1, S, H, Wd, pitch, plane, offsets2);
  CHECK(offsets.size() == S + 1 && offsets[0] == 0 && offsets[S] == all.size() && offsets2 == offsets && all2 == all);
  for (size_t s = 0; s < S; ++s) {
    const auto one = watershed.find_local_minima(ws::ArrayView2<uint8_t>(cube.data() + s * hw, H, Wd, Wd));
    CHECK(offsets[s + 1] - offsets[s] == one.size());
    for (size_t i = 0; i < one.size(); ++i) CHECK(all[offsets[s] + i] == one[i]);
  }
  if (S > 2 && H >= 3 && Wd >= 3) CHECK(offsets[1] == offsets[2] && offsets[1] > 0);
  return 0;
}

// a WS_F64 range overflow names its slice, as the numpy and torch shims do
template <class W>
static int check_overflow(const W &watershed) {
  std::vector<double> cube(4 * 6, 1.0);
  cube[2 * 6 + 1] = -1e308;
  cube[2 * 6 + 4] = 1e308;
  bool named = false;
  try {
    watershed.template pre_processor_cube<double>(cube.data(), 4, 2, 3, 6, 3, 1);
  } catch (const ws::WatershedError &e) {
    named = e.status == WS_ERR_UNSUPPORTED && std::string(e.what()).find("slice 2") != std::string::npos;
  }
  CHECK(named);
  cube[2 * 6 + 1] = -8.9e307;
  cube[2 * 6 + 4] = 8.9e307;
  CHECK(watershed.template pre_processor_cube<double>(cube.data(), 4, 2, 3, 6, 3, 1).size() == 24);
  return 0;
}

int main() {
  auto seg = ws::TransformBuilder<>().build_segmenting();
  if (check_overflow(seg)) return 1;
  if (check_pre_processor<float>(seg, 5, 6, 67) || check_pre_processor<double>(seg, 65, 3, 43) || check_pre_processor<int16_t>(seg, 3, 1, 129) ||
      check_pre_processor<uint8_t>(seg, 2, 4, 64) ||
      check_pre_processor<float>(seg, 9, 3, 171) || check_pre_processor<int32_t>(seg, 17, 1, 257))
    return 1;
  if (check_minima(seg, 5, 9, 33, 1) || check_minima(seg, 4, 13, 1028, 2) || check_minima(seg, 3, 2, 9, 3) || check_minima(seg, 1, 8, 16, 4)) return 1;
  std::printf("cube input ok\n");
  return 0;
}
