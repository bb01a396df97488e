// merge_tree of the C++ mirror (include/ws_watershed.hpp, ws_merge_tree) against the mirror's own transform_history_levels planes,
// by the definition of the records: death level and parent from the colour's seed pixel, area and leaves from the plane before,
// and the parent walk of roots_at() against every plane -- with and without edge correction.  Needs device 0.
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
static int check(const W &watershed, size_t H, size_t Wd, unsigned seed, size_t shift = 0) {      // shift: seeds moved into the padded plane
  std::vector<uint8_t> img(H * Wd);
  ws_or_random_field(img.data(), H, Wd, seed);
  ws::ArrayView2<uint8_t> view(img.data(), H, Wd, Wd);
  const auto mins = watershed.find_local_minima(view);
  std::vector<uint8_t> all;
  for (unsigned l = 0; l <= watershed.max_water_level(); ++l) all.push_back((uint8_t)l);
  const auto planes = watershed.transform_history_levels(view, mins, all);
  const auto tree = watershed.merge_tree(view, mins, true);
  const size_t S = mins.size(), levels = all.size();
  CHECK(tree.nodes.size() == S + 1);
  CHECK(tree.labels.rows == planes[0].second.rows && tree.labels.cols == planes[0].second.cols);
  const size_t npx = tree.labels.rows * tree.labels.cols, cols = tree.labels.cols;
  // (find_local_minima gives distinct pixels: every colour exists)
  std::vector<size_t> px(S + 1, 0);
  for (size_t c = 1; c <= S; ++c) {
    px[c] = (mins[c - 1].first + shift) * cols + mins[c - 1].second + shift;
    CHECK(tree.labels.data[px[c]] == c);
  }
  const auto &last = planes[levels - 1].second.data;
  size_t uncoloured = 0;
  for (size_t p = 0; p < npx; ++p) uncoloured += last[p] == 0;
  CHECK(tree.nodes[0].parent == 0 && tree.nodes[0].death_level == W::MergeTree::ALIVE && tree.nodes[0].n_leaves == 0);
  CHECK(tree.nodes[0].area == uncoloured);
  for (size_t c = 1; c <= S; ++c) {
    const ws_tree_node &n = tree.nodes[c];
    size_t L = 0;
    while (L < levels && planes[L].second.data[px[c]] == c) ++L;
    if (L == levels) CHECK(n.death_level == W::MergeTree::ALIVE && n.parent == 0);
    else CHECK(n.death_level == L && n.parent == planes[L].second.data[px[c]] && n.parent > 0 && n.parent < c);
    if (L == 0) { CHECK(n.area == 1 && n.n_leaves == 1); continue; }
    const auto &before = planes[L - 1].second.data;
    size_t area = 0, leaves = 0;
    for (size_t p = 0; p < npx; ++p) area += before[p] == c;
    for (size_t x = 1; x <= S; ++x) leaves += before[px[x]] == c;
    CHECK(n.area == area && n.n_leaves == leaves);
  }
  for (size_t L = 0; L < levels; ++L) {
    const auto root = tree.roots_at((uint32_t)L);
    CHECK(root[0] == 0);
    for (size_t c = 1; c <= S; ++c) CHECK(root[c] == planes[L].second.data[px[c]]);
    // the label plane of the level is a table lookup
    for (size_t p = 0; p < npx; ++p)
      if (planes[L].second.data[p]) CHECK(root[tree.labels.data[p]] == planes[L].second.data[p]);
  }
  const auto bare = watershed.merge_tree(view, mins);
  CHECK(bare.labels.data.empty() && bare.nodes.size() == S + 1);
  for (size_t c = 0; c <= S; ++c)
    CHECK(bare.nodes[c].parent == tree.nodes[c].parent && bare.nodes[c].death_level == tree.nodes[c].death_level &&
          bare.nodes[c].area == tree.nodes[c].area && bare.nodes[c].n_leaves == tree.nodes[c].n_leaves);
  return 0;
}

int main() {
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_low = ws::TransformBuilder<>().set_max_water_lvl(60).build_merging();
  auto mer_e = ws::TransformBuilder<>().enable_edge_correction().shift_seeds_into_padded_plane().build_merging();
  auto mer_p = ws::TransformBuilder<>().set_max_water_lvl(200).enable_edge_correction().build_merging();
  if (check(mer, 96, 80, 4) || check(mer_low, 70, 53, 6) || check(mer_e, 64, 75, 7, 1) || check(mer_p, 40, 44, 8)) return 1;
  std::printf("merge tree ok\n");
  return 0;
}
