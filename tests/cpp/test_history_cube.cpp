// transform_history_cube of the C++ mirror (include/ws_watershed.hpp, ws_transform_history_batch): every slice's planes equal
// transform_history_levels on that slice with its own minima -- both transforms, with and without edge correction, on a shape
// whose slices stack and on one whose slices do not.  Needs device 0.
#include <cstdio>
#include <vector>

#include "../../include/ws_watershed.hpp"
#include "../../oracle/ws_oracle.h"

namespace ws = rustronomy_watershed;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <class W>
static int check(const W &watershed, size_t S, size_t H, size_t Wd, unsigned seed) {
  std::vector<uint8_t> cube(S * H * Wd);
  for (size_t k = 0; k < S; ++k) ws_or_random_field(cube.data() + k * H * Wd, H, Wd, seed + (unsigned)k);
  const std::vector<uint8_t> levels = {watershed.max_water_level(), 0, 17, 17, 3};
  std::vector<size_t> n_seeds;
  const auto got = watershed.transform_history_cube(cube.data(), S, H, Wd, levels, &n_seeds);
  CHECK(got.size() == S && n_seeds.size() == S);
  for (size_t k = 0; k < S; ++k) {
    ws::ArrayView2<uint8_t> view(cube.data() + k * H * Wd, H, Wd, Wd);
    const auto mins = watershed.find_local_minima(view);
    CHECK(n_seeds[k] == mins.size());
    const auto want = watershed.transform_history_levels(view, mins, levels);
    CHECK(got[k].size() == want.size());
    for (size_t j = 0; j < want.size(); ++j) {
      CHECK(got[k][j].first == want[j].first);
      CHECK(got[k][j].second.rows == want[j].second.rows && got[k][j].second.cols == want[j].second.cols);
      CHECK(got[k][j].second.data == want[j].second.data);
    }
  }
  const auto none = watershed.transform_history_cube(cube.data(), S, H, Wd, {});
  CHECK(none.size() == S && none[0].empty());
  return 0;
}

int main() {
  auto seg = ws::TransformBuilder<>().set_max_water_lvl(120).build_segmenting();
  auto mer = ws::TransformBuilder<>().build_merging();
  auto seg_e = ws::TransformBuilder<>().enable_edge_correction().build_segmenting();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(60).enable_edge_correction().build_merging();
  // 128 x 96 planes stack (126 x 94 with edge correction pads to 128 x 96); 70 x 53 ones do not
  if (check(seg, 5, 128, 96, 3) || check(mer, 5, 128, 96, 40) || check(seg_e, 4, 126, 94, 50) || check(mer_e, 4, 126, 94, 60) ||
      check(mer, 3, 70, 53, 70) || check(seg_e, 3, 70, 53, 80))
    return 1;
  std::printf("history cube ok\n");
  return 0;
}
