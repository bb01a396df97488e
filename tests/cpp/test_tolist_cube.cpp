// transform_to_list_cube of the C++ mirror (include/ws_watershed.hpp, ws_transform_to_list_batch): every slice's lists, per
// level, are those of transform_to_list(slice, find_local_minima(slice)) -- records compared as sets -- for both transforms, on
// a cube that stacks (slices 128 x 96) and one that does not (130 x 98).  Needs device 0.
#include <algorithm>
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
static int check_cube(const W &watershed, size_t N, size_t H, size_t Wd, unsigned seed) {
  std::vector<uint8_t> cube(N * H * Wd);
  for (size_t k = 0; k < N; ++k) ws_or_random_field(cube.data() + k * H * Wd, H, Wd, seed + k);
  std::vector<size_t> n_seeds;
  auto lists = watershed.transform_to_list_cube(cube.data(), N, H, Wd, &n_seeds);
  CHECK(lists.size() == N && n_seeds.size() == N);
  for (size_t k = 0; k < N; ++k) {
    ws::ArrayView2<uint8_t> slice(cube.data() + k * H * Wd, H, Wd, Wd);
    auto mins = watershed.find_local_minima(slice);
    CHECK(mins.size() == n_seeds[k]);
    auto dense = watershed.transform_to_list(slice, mins);
    CHECK(lists[k].size() == dense.size());
    for (size_t l = 0; l < dense.size(); ++l) {
      const auto &got = lists[k][l];
      const auto &want = dense[l].second;
      CHECK(got.level == dense[l].first && got.uncoloured == want[0]);
      std::vector<ws::usize> hist(want.size(), 0);
      size_t nz = 0;
      for (const ws_lake &r : got.lakes) {
        CHECK(r.colour >= 1 && r.colour < hist.size() && hist[r.colour] == 0 && r.area > 0);
        hist[r.colour] = r.area;
      }
      for (size_t i = 1; i < want.size(); ++i) {
        CHECK(hist[i] == want[i]);
        nz += want[i] != 0;
      }
      CHECK(nz == got.lakes.size());
    }
  }
  return 0;
}

int main() {
  auto seg = ws::TransformBuilder<>().build_segmenting();
  auto mer = ws::TransformBuilder<>().set_max_water_lvl(90).build_merging();
  if (check_cube(seg, 6, 128, 96, 40) || check_cube(mer, 6, 128, 96, 50) || check_cube(seg, 5, 130, 98, 60) ||
      check_cube(mer, 5, 130, 98, 70))
    return 1;
  std::printf("cube lists ok\n");
  return 0;
}
