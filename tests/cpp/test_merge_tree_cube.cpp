// merge_tree_cube of the C++ mirror (include/ws_watershed.hpp, ws_merge_tree_batch) against the mirror's own merge_tree slice by
// slice: own minima and given seed lists, a cube whose slices stack and one whose slices do not, with and without edge correction
// and labels.  Needs device 0.
#include <cstdio>
#include <vector>

#include "../../include/ws_watershed.hpp"
#include "../../oracle/ws_oracle.h"

namespace ws = rustronomy_watershed;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <class T>
static int same(const T &a, const T &b) {
  CHECK(a.nodes.size() == b.nodes.size());
  for (size_t c = 0; c < a.nodes.size(); ++c)
    CHECK(a.nodes[c].parent == b.nodes[c].parent && a.nodes[c].death_level == b.nodes[c].death_level &&
          a.nodes[c].area == b.nodes[c].area && a.nodes[c].n_leaves == b.nodes[c].n_leaves);
  CHECK(a.labels.rows == b.labels.rows && a.labels.cols == b.labels.cols && a.labels.data == b.labels.data);
  return 0;
}

template <class W>
static int check(const W &watershed, size_t S, size_t H, size_t Wd, unsigned seed) {
  std::vector<uint8_t> cube(S * H * Wd);
  for (size_t k = 0; k < S; ++k) ws_or_random_field(cube.data() + k * H * Wd, H, Wd, seed + (unsigned)k);
  std::vector<std::vector<ws::Seed>> mins;
  for (size_t k = 0; k < S; ++k) mins.push_back(watershed.find_local_minima(ws::ArrayView2<uint8_t>(cube.data() + k * H * Wd, H, Wd, Wd)));
  std::vector<size_t> counts;
  const auto own = watershed.merge_tree_cube(cube.data(), S, H, Wd, nullptr, true, &counts);
  auto lists = mins;
  lists[1].clear();           // a slice without seeds owns its record 0 alone
  lists[2].resize(1);
  const auto given = watershed.merge_tree_cube(cube.data(), S, H, Wd, &lists);
  CHECK(own.size() == S && given.size() == S && counts.size() == S);
  for (size_t k = 0; k < S; ++k) {
    const ws::ArrayView2<uint8_t> view(cube.data() + k * H * Wd, H, Wd, Wd);
    CHECK(counts[k] == mins[k].size());
    if (same(own[k], watershed.merge_tree(view, mins[k], true))) return 1;
    if (same(given[k], watershed.merge_tree(view, lists[k]))) return 1;
  }
  CHECK(given[1].nodes.size() == 1 && given[1].nodes[0].death_level == W::MergeTree::ALIVE);
  return 0;
}

int main() {
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(200).enable_edge_correction().build_merging();
  // 128 x 96 planes stack (126 x 94 padded to them); 130 x 98 run as the loop
  if (check(mer, 5, 128, 96, 40) || check(mer_e, 4, 126, 94, 50) || check(mer, 4, 130, 98, 60) || check(mer_e, 3, 130, 98, 70)) return 1;
  std::printf("merge tree cube ok\n");
  return 0;
}
