// transform_history_levels of the C++ mirror (include/ws_watershed.hpp, ws_transform_history): with every level it equals the
// hook route's transform_history plane for plane, and a level list in any order with repeats picks the same planes -- both
// transforms, with and without edge correction.  Needs device 0.
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
static int check(const W &watershed, size_t H, size_t Wd, unsigned seed) {
  std::vector<uint8_t> img(H * Wd);
  ws_or_random_field(img.data(), H, Wd, seed);
  ws::ArrayView2<uint8_t> view(img.data(), H, Wd, Wd);
  const auto mins = watershed.find_local_minima(view);
  const auto hist = watershed.transform_history(view, mins);
  std::vector<uint8_t> all;
  for (unsigned l = 0; l <= watershed.max_water_level(); ++l) all.push_back((uint8_t)l);
  const auto got = watershed.transform_history_levels(view, mins, all);
  CHECK(got.size() == hist.size());
  for (size_t k = 0; k < got.size(); ++k) {
    CHECK(got[k].first == hist[k].first);
    CHECK(got[k].second.rows == hist[k].second.rows && got[k].second.cols == hist[k].second.cols);
    CHECK(got[k].second.data == hist[k].second.data);
  }
  const std::vector<uint8_t> some = {watershed.max_water_level(), 0, 17, 17, 3};
  const auto picked = watershed.transform_history_levels(view, mins, some);
  CHECK(picked.size() == some.size());
  for (size_t k = 0; k < some.size(); ++k) {
    CHECK(picked[k].first == some[k]);
    CHECK(picked[k].second.data == hist[some[k]].second.data);
  }
  CHECK(watershed.transform_history_levels(view, mins, {}).empty());
  return 0;
}

int main() {
  auto seg = ws::TransformBuilder<>().set_max_water_lvl(120).build_segmenting();
  auto mer = ws::TransformBuilder<>().build_merging();
  auto seg_e = ws::TransformBuilder<>().enable_edge_correction().build_segmenting();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(60).enable_edge_correction().build_merging();
  if (check(seg, 96, 80, 3) || check(mer, 96, 80, 4) || check(seg_e, 70, 53, 5) || check(mer_e, 70, 53, 6)) return 1;
  std::printf("history levels ok\n");
  return 0;
}
